#!/usr/bin/env python3
"""abea throughput: a generated set of reads resident in HBM through gab_abea_align_device; median of warm repeats.

    python tools/abea_bench.py [--reads 4096] [--min-bases 5000] [--max-bases 15000] [--repeats 7] [--seed 1] [--json out.json]

Reports reads/s, band cells/s (cells filled, the reference's `fills`), ms per launch, and the DP kernel's share of the device time
against the rest (k-mer table and backtrack).  Wall time is taken around the call, which synchronises its stream before it returns."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def generate(rng, n_reads, lo, hi):
    """reads as tests/abea_model.py makes them (0 / 1 / 2 / 3..6 events per k-mer with probability 0.01 / 0.54 / 0.30 / 0.15, scalings
    by the method of moments), vectorised over the whole set"""
    from genarchbench_amd import abea
    mean = rng.uniform(60.0, 130.0, abea.NKMER).astype(np.float32); stdv = rng.uniform(1.0, 3.5, abea.NKMER).astype(np.float32)
    seq_len = rng.integers(lo, hi + 1, n_reads).astype(np.int32)
    seqs, evs, scale, shift = [], [], [], []
    for n in seq_len:
        codes = rng.integers(0, 4, int(n))
        nk = int(n) - abea.K + 1
        ranks = np.zeros(nk, np.int64)
        for t in range(abea.K):
            ranks = ranks * 4 + codes[t:t + nk]
        kind = rng.choice(4, nk, p=(0.01, 0.54, 0.30, 0.15))
        counts = np.where(kind == 3, rng.integers(3, 7, nk), kind)
        of = np.repeat(ranks, counts)
        sc, sh = 1.0 + 0.01 * rng.standard_normal(), 5.0 * rng.standard_normal()
        ev = (sc * mean[of].astype(np.float64) + sh + rng.standard_normal(of.size) * stdv[of]).astype(np.float32)
        levels = mean[ranks].astype(np.float64); e64 = ev.astype(np.float64)
        s = e64.mean() - levels.mean()
        scale.append(np.float32((((e64 - s) ** 2).mean()) / (levels * levels).mean())); shift.append(np.float32(s))
        seqs.append(np.frombuffer(b"ACGT", np.uint8)[codes]); evs.append(ev)
    n_events = np.array([e.size for e in evs], np.int32)
    off = lambda ln: np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.int64)]).astype(np.int64)
    room = abea.pair_room(seq_len, n_events)
    return (mean, stdv), (np.concatenate(seqs), off(seq_len), seq_len, np.concatenate(evs), off(n_events), n_events,
                          np.array(scale, np.float32), np.array(shift, np.float32), off(room)), int(room.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096); ap.add_argument("--min-bases", type=int, default=5000)
    ap.add_argument("--max-bases", type=int, default=15000); ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1); ap.add_argument("--json")
    a = ap.parse_args()
    import genarchbench_amd  # noqa: F401  (before torch: the runtime's default for pageable copies)
    import torch
    from genarchbench_amd import abea
    (mean, stdv), packed, room = generate(np.random.default_rng(a.seed), a.reads, a.min_bases, a.max_bases)
    h = abea.EventAligner(mean, stdv)
    dev = [torch.from_numpy(x).cuda() for x in packed]
    pairs = torch.empty((room, 2), dtype=torch.int32, device="cuda")
    res = torch.zeros(a.reads * abea.READ.itemsize, dtype=torch.uint8, device="cuda")
    walls, stats = [], []
    for it in range(a.repeats + 1):                                  # the first run allocates: not counted
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.align_device(*dev[:8], pairs, dev[8], res)
        walls.append(time.perf_counter() - t0); stats.append(h.last_stats())
    rec = res.cpu().numpy().view(abea.READ)
    order = np.argsort(walls[1:]); mid = 1 + int(order[len(order) // 2])
    st, wall = stats[mid], walls[mid]
    out = {"reads": a.reads, "bases": int(packed[2].sum()), "events": int(packed[5].sum()), "bands": st["bands"], "cells": st["cells"],
           "launches": st["launches"], "repeats": a.repeats, "wall_ms_median": round(wall * 1e3, 3),
           "wall_ms_all": [round(w * 1e3, 3) for w in walls[1:]], "reads_per_s": round(a.reads / wall, 1), "cells_per_s": round(st["cells"] / wall, 1),
           "ms_per_launch": round(wall * 1e3 / st["launches"], 3), "dp_kernel_ms": round(st["kernel_ms"], 3), "all_kernels_ms": round(st["total_ms"], 3),
           "dp_share": round(st["kernel_ms"] / st["total_ms"], 4), "reads_passing": int((rec["n_pairs"] > 0).sum()),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
