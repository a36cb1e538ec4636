#!/usr/bin/env python3
"""Lockstep work of the bsw_dp8 waves, from the CPU model's row trace (tools/gen/bsw_exit_model.c, gab_bsw_exit_trace) -- no GPU.

    python tools/profiling/bsw_wave_model.py [--pairs 500000] [--seed 2] [--mode 0] [--key KEY] [--rule default|capped|...]
                                             [--bound hop|ungapped]

Pairs are grouped as the kernels group them: by query-length class of 16 bases (one launch each at bench size), inside a class in
the order of the sort key bsw_key = (qlen, deficit of the seed's lower bound L), 64 consecutive pairs to a wave (the order inside
one key is atomic order on the GPU; here it is input order, so expect a per cent or two of difference).  A wave sweeps row r while
any lane has a row r (a restarted pair's second pass follows its first), and runs as many four-cell loop trips in it as its widest
lane.  Prints wave-rows, wave-trips, the share of lanes busy in each, and for every per-row path of the kernel the share of wave-rows
in which at least one lane takes it.  --key compares groupings: `current` is bsw_key as the kernels have it, `oracle` sorts by each
pair's true (rows, cells), `qlen_tmin_h0` by (qlen, min(tlen, qlen + 40) / 4, h0), `parent` by the key before the seeded prune
(qlen, min(tlen / 8, 63), min(h0 / 32, 3)).  The others are the candidates the seeded prune's key was picked from, all with qlen as
the major part and 256 values under it; deficit = qlen - (L - h0) for the seed's lower bound L (gabgen.bsw_hop_bound, what the
kernels make; --bound ungapped takes gabgen.bsw_seed_bound, the bound before the hops, which goes with --rule seed_no_hops):
`d8` (deficit), `d7_short` (deficit / 2, tlen < qlen), `d7_h1` (deficit / 2, h0 >= 64), `d6_t2` (deficit / 4, min(tlen / 32, 3)),
`d5_t3` (deficit / 8, min(tlen / 16, 7)); `q4_d2` is (qlen / 4, deficit / 2, tlen / 8, h0 / 32), which does not fit the 65 536 bins.
--rule picks the model's prune rule (gabgen.BSW_PRUNE_RULES)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tools import gabgen                      # noqa: E402
from tests.util import BSW_PARAM_SETS, bsw_oracle_params      # noqa: E402

PATHS = ["odd beg (head cell)", "remainder pair", "odd end (tail cell)", "lz == 4", "tz == 4", "left drop", "right drop", "bound pass",
         "no loop trip"]


SEED_KEYS = {
    "d8": lambda ql, tl, h0, d: (ql - 1) * 256 + d,
    "d7_short": lambda ql, tl, h0, d: (ql - 1) * 256 + (d >> 1) * 2 + (tl < ql),
    "d7_h1": lambda ql, tl, h0, d: (ql - 1) * 256 + (d >> 1) * 2 + (h0 >= 64),
    "d6_t2": lambda ql, tl, h0, d: (ql - 1) * 256 + (d >> 2) * 4 + np.minimum(tl >> 5, 3),
    "d5_t3": lambda ql, tl, h0, d: (ql - 1) * 256 + (d >> 3) * 8 + np.minimum(tl >> 4, 7),
    "q4_d2": lambda ql, tl, h0, d: ((((ql - 1) >> 2) * 128 + (d >> 1)) * 64 + np.minimum(tl >> 3, 63)) * 4 + np.minimum(h0 >> 5, 3),
}
CURRENT_KEY = "d8"                      # what bsw_key (genarchbench_amd/csrc/bsw.hip) computes


def lane_rows(beg, end, flags):
    """per traced row: loop trips and a bit per path of PATHS"""
    beg = beg.astype(np.int32); end = end.astype(np.int32)
    head = ((beg & 1) == 1) & (beg < end)
    j0 = beg + head
    inloop = j0 + 1 < end
    trips = np.where(inloop, np.maximum((end - 3 - j0 + 3) // 4, 0), 0)
    j1 = j0 + 4 * trips
    rem = inloop & (j1 + 1 < end)
    j2 = j1 + 2 * rem
    tail = j2 < end
    bits = (head * 1 | rem * 2 | tail * 4).astype(np.uint16)
    F = gabgen.BSW_TRACE_FLAGS
    for k, name in enumerate(("lz4", "tz4", "left_drop", "right_drop", "bound_pass")):
        bits |= (((flags & F[name]) != 0) * (8 << k)).astype(np.uint16)
    bits |= ((trips == 0) * 256).astype(np.uint16)
    return trips.astype(np.int16), bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=500000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--key", default="current", choices=["current", "oracle", "qlen_tmin_h0", "parent"] + list(SEED_KEYS))
    ap.add_argument("--rule", default="default", choices=list(gabgen.BSW_PRUNE_RULES))
    ap.add_argument("--bound", default="hop", choices=["hop", "ungapped"])
    a = ap.parse_args()
    b = gabgen.bsw(a.seed, a.pairs, a.mode)
    p = bsw_oracle_params(*BSW_PARAM_SETS[0])
    ql, tl, h0 = b.len2.astype(np.int64), b.len1.astype(np.int64), b.h0.astype(np.int64)
    cls = (ql - 1) // 16
    if a.key == "current":
        a.key = CURRENT_KEY
    if a.key == "parent":
        key = (ql - 1) * 256 + np.minimum(tl >> 3, 63) * 4 + np.minimum(h0 >> 5, 3)
    elif a.key in SEED_KEYS:
        bound = gabgen.bsw_hop_bound if a.bound == "hop" else gabgen.bsw_seed_bound
        deficit = np.clip(ql - (bound(b, p).astype(np.int64) - h0), 0, 255)
        key = SEED_KEYS[a.key](ql, tl, h0, deficit)
    elif a.key == "qlen_tmin_h0":
        key = ((ql - 1) * 128 + np.minimum(tl, ql + 40) // 4) * 1024 + np.minimum(h0, 1023)
    else:
        _, rows, cells, _ = gabgen.bsw_exit_model(b, p, rule=a.rule)
        key = rows.astype(np.int64) * (1 << 20) + cells
    order = np.lexsort((np.arange(b.n), key, cls))
    tot = dict(wave_rows=0, wave_trips=0, lane_rows=0, lane_trips=0, waves=0, cells=0)
    share = np.zeros(len(PATHS), np.int64)
    for c in np.unique(cls):
        idx = order[cls[order] == c]
        for lo in range(0, len(idx), 64 * 1024):
            sub = idx[lo:lo + 64 * 1024]
            batch = gabgen.BswBatch(b.ref, b.ref_off[sub].copy(), b.qry, b.qry_off[sub].copy(), b.len1[sub].copy(), b.len2[sub].copy(),
                                    b.h0[sub].copy())
            out = gabgen.bsw_exit_trace(batch, p, rule=a.rule)
            off, beg, end, flags = out[5], out[6], out[7], out[8]
            tot["cells"] += int(out[2].sum())
            nrows = np.diff(off)
            trips, bits = lane_rows(beg, end, flags)
            nw = (len(sub) + 63) // 64
            R = int(nrows.max())
            dt = np.zeros((nw * 64, R), np.int16); db = np.zeros((nw * 64, R), np.uint16); alive = np.zeros((nw * 64, R), bool)
            pair = np.repeat(np.arange(len(sub)), nrows)
            i = np.arange(off[-1]) - np.repeat(off[:-1], nrows)
            dt[pair, i] = trips; db[pair, i] = bits; alive[pair, i] = True
            dt = dt.reshape(nw, 64, R); db = db.reshape(nw, 64, R); alive = alive.reshape(nw, 64, R)
            wrow = alive.any(axis=1)
            tot["waves"] += nw
            tot["wave_rows"] += int(wrow.sum())
            tot["wave_trips"] += int(dt.max(axis=1).astype(np.int64).sum())
            tot["lane_rows"] += int(alive.sum())
            tot["lane_trips"] += int(dt.astype(np.int64).sum())
            anyb = np.bitwise_or.reduce(db, axis=1)
            for k in range(len(PATHS) - 1):
                share[k] += int(((anyb >> k) & 1).sum())
            share[-1] += int((wrow & (dt.max(axis=1) == 0)).sum())          # wave-rows in which NO lane runs a loop trip
    print(f"{a.pairs} pairs of seed {a.seed} mode {a.mode}, key {a.key}, rule {a.rule}: {tot['waves']} waves, cells {tot['cells']}")
    print(f"wave-rows  {tot['wave_rows']}   lanes busy {tot['lane_rows'] / (64 * tot['wave_rows']):.3f}")
    print(f"wave-trips {tot['wave_trips']}   lanes busy {tot['lane_trips'] / (64 * tot['wave_trips']):.3f}   "
          f"trips per wave-row {tot['wave_trips'] / tot['wave_rows']:.2f}")
    for name, s in zip(PATHS, share):
        print(f"  {name:22s} in {s / tot['wave_rows']:.4f} of the wave-rows")


if __name__ == "__main__":
    main()
