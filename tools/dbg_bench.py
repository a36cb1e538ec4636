#!/usr/bin/env python3
"""Throughput of the de Bruijn graph builder (gab_dbg_*) on a generated short-read set.  Standalone; needs a GPU.

    python tools/dbg_bench.py [--mbp 2] [--coverage 30] [--repeats 7] [--warmup 2] [--slice 512] [--check 3] [--out dbg_bench.json]

The set (seeded): a random contig of --mbp Mbp, reads of 151 bases at --coverage x, about 1 % substitutions, qualities mostly 30 .. 41
with 2 % of the bases at 2 .. 20 and one read in fifty bad throughout, one read in a hundred QC-fail, sorted by position, cut into
assembly regions by gab_dbg_plan_regions (the reference's own batch loop: a region every 750 bases, 3 000 .. 4 500 reference bases and
the reads of 1 500 bases each).  A call's scratch holds the tables of all its regions at once, so the regions go in slices of --slice.

It reports, warm, as the median of the repeats of the wall time over all slices:
    resident      inputs already on the GPU (gab_dbg_build_device), the records left there
    host          inputs in pageable host memory (gab_dbg_build), the records copied back
with regions/s and edge occurrences/s (offered, i.e. before the quality filter), and the device time of the three phases summed over
the slices.  --check N compares the first N regions with tests/dbg_model.py."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

READ_LEN = 151


def short_read_set(mbp, coverage, seed=20261021):
    """-> (contig uint8, seq uint8 (n, 151), qual uint8 (n, 151), flag int32, pos int32)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    n = int(mbp * 1e6)
    contig = acgt[rng.integers(0, 4, n)]
    n_reads = n * coverage // READ_LEN
    pos = np.sort(rng.integers(0, n - READ_LEN, n_reads)).astype(np.int32)
    seq = contig[pos[:, None].astype(np.int64) + np.arange(READ_LEN)]
    err = rng.random(seq.shape) < 0.01
    seq[err] = acgt[rng.integers(0, 4, int(err.sum()))]
    qual = rng.integers(30, 42, seq.shape).astype(np.uint8)
    low = rng.random(seq.shape) < 0.02
    qual[low] = rng.integers(2, 21, int(low.sum()))
    qual[rng.random(n_reads) < 0.02] = 12
    flag = np.where(rng.random(n_reads) < 0.01, 512, 0).astype(np.int32)
    return contig, seq, qual, flag, pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=2.0)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slice", type=int, default=512)
    ap.add_argument("--check", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import genarchbench_amd  # noqa: F401
    import torch
    from genarchbench_amd import dbg

    contig, seq, qual, flag, pos = short_read_set(a.mbp, a.coverage)
    n_reads = len(pos)
    plan = dbg.plan_regions(0, len(contig), pos, pos + READ_LEN, len(contig))
    n_regions = len(plan)
    read_off = np.arange(n_reads, dtype=np.int64) * READ_LEN
    read_len = np.full(n_reads, READ_LEN, np.int32)
    whole = dict(ref=contig, ref_off=plan["ref_start"].astype(np.int64), ref_len=plan["ref_len"].copy(), ref_start=plan["ref_start"].copy(), seq=seq.reshape(-1),
                 qual=qual.reshape(-1), read_off=read_off, read_len=read_len, read_flag=flag, read_begin=plan["read_begin"].copy(), read_end=plan["read_end"].copy())
    per_region = ("ref_off", "ref_len", "ref_start", "read_begin", "read_end")
    slices = [slice(s, min(s + a.slice, n_regions)) for s in range(0, n_regions, a.slice)]
    per_read = ("read_off", "read_len", "read_flag")
    packs = []
    for sl in slices:        # a slice sees its own window of the read arrays (src_read then counts from the window's first read)
        lo, hi = int(whole["read_begin"][sl].min()), int(whole["read_end"][sl].max())
        p = {f: (np.ascontiguousarray(v[sl]) if f in per_region else np.ascontiguousarray(v[lo:hi]) if f in per_read else v) for f, v in whole.items()}
        p["read_begin"] -= lo; p["read_end"] -= lo
        packs.append(p)
    rooms = [dbg.room(p) for p in packs]
    h = dbg.GraphBuilder(0)
    dev = torch.device("cuda:0")
    shared = {f: torch.from_numpy(np.ascontiguousarray(whole[f])).to(dev) for f in ("ref", "seq", "qual")}
    tens = [dict(shared, **{f: torch.from_numpy(p[f]).to(dev) for f in per_region + per_read}) for p in packs]
    nodes = torch.empty(max(rooms) * dbg.NODE.itemsize, dtype=torch.uint8, device=dev)
    node_off = torch.empty(a.slice + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def resident():
        tot = dict.fromkeys(("occurrences", "passed", "nodes", "edges", "probes", "insert_ms", "number_ms", "emit_ms", "kernel_ms"), 0)
        t0 = time.perf_counter()
        for t in tens:
            h.build_device(t, node_off, nodes, stream=0)
            s = h.last_stats()
            for f in tot:
                tot[f] += s[f]
        return (time.perf_counter() - t0) * 1e3, tot

    def host():
        t0 = time.perf_counter()
        for p, r in zip(packs, rooms):
            h.build(p, capacity=r)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        resident()
    runs = [resident() for _ in range(a.repeats)]
    wall = statistics.median(r[0] for r in runs)
    tot = runs[len(runs) // 2][1]
    phases = {f: round(statistics.median(r[1][f] for r in runs), 3) for f in ("insert_ms", "number_ms", "emit_ms", "kernel_ms")}
    for _ in range(a.warmup):
        host()
    host_wall = statistics.median(host() for _ in range(a.repeats))
    if a.check:
        from tests import dbg_model as M
        n = min(a.check, n_regions)
        reads = lambda b, e: [(seq[j].tobytes(), qual[j].tobytes(), int(flag[j])) for j in range(b, e)]
        sub = {f: (v[:n] if f in per_region else v) for f, v in whole.items()}
        off, recs = h.build(sub)
        for i in range(n):
            r = plan[i]
            want = M.build_region(contig[r["ref_start"]:r["ref_start"] + r["ref_len"]].tobytes(), int(r["ref_start"]), reads(int(r["read_begin"]), int(r["read_end"])), 15, 20, int(r["read_begin"]))
            assert recs[off[i]:off[i + 1]].tobytes() == want.tobytes(), f"region {i} differs from tests/dbg_model.py"
    occ = int(tot["occurrences"])
    out = dict(workload="dbg", mbp=a.mbp, coverage=a.coverage, reads=n_reads, regions=n_regions, slice=a.slice, occurrences=occ, passed=int(tot["passed"]), nodes=int(tot["nodes"]),
               edges=int(tot["edges"]), probes_per_node_lookup=round(tot["probes"] / max(1, 2 * tot["passed"]), 3), repeats=a.repeats,
               resident_wall_ms=round(wall, 3), resident_regions_per_s=round(n_regions / wall * 1e3, 1), resident_occurrences_per_s=round(occ / wall * 1e3, 1),
               host_wall_ms=round(host_wall, 3), host_regions_per_s=round(n_regions / host_wall * 1e3, 1), host_occurrences_per_s=round(occ / host_wall * 1e3, 1),
               checked_regions=a.check, **phases)
    h.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
