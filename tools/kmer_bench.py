#!/usr/bin/env python3
"""Throughput of the k-mer counter (gab_kmer_*) on a generated E. coli-like read set.  Standalone; needs a GPU.

    python tools/kmer_bench.py [--repeats 7] [--warmup 2] [--coverage 50] [--parts 1,2,4,8] [--minimizers W] [--solid] [--out kmer_bench.json]

The read set: a 4.6 Mbp random genome, reads of 5 .. 20 kb at 50x, both strands, 10 % errors (substitutions, seeded).
For k = 17 and 15 it reports, warm, as the median of the repeats:
    resident      reads already on the GPU (gab_kmer_count_device): k-mer positions per second over the call's device time
    host          reads in pageable host memory (gab_kmer_count): positions per second over the wall time of the call
and the device time of the stages -- 2-bit packing, table clear + extract-and-count (one kernel), reduction -- with the table
lines visited per insert.  The first call's result is compared with the numpy model of tests/kmer_model.py when --check is given
(minutes of CPU time at this size).

--parts N[,N...]: for every N, each of the N key-space partitions (gab_kmer_count_part) is run ON ITS OWN on the one GPU, resident,
the same warm-up and repeats: what one GPU of N would do, every GPU walking all reads and inserting its share of the k-mers.  Per
partition the stage times, and per N the slowest partition's call time with the positions per second it would give -- a ONE-GPU
FORECAST of an N-GPU run, not a measurement of one (no second card, no shared host link).  As N grows the count stage tends to
what extraction alone costs: the floor no number of GPUs gets under.

--minimizers W: INSTEAD of the count, the minimizer index (gab_kmer_index_minimizers_device, window W, repeat_kmer_rate --rate) on
the same reads, resident, for k = 17 and 15: the nine result fields, k-mer positions per second over the wall time of the call
(median of the warm repeats; the call synchronises twice, once for the filter's two integers) and the device time of its four
stages -- sketch, capacity count, fill, segmented sort.

--minimizers W --parts N[,N...]: for every N, the index in N key-space partitions (gab_kmer_index_part_begin_device /
gab_kmer_index_part_finish), every partition's two phases run in turn on the one GPU, each on a handle of its own: per partition the
wall time of its begin and of its finish (medians of the warm repeats) and the device time of its stages.  The two phases of N
GPUs are two rounds with the host's sum in between, so the ONE-GPU FORECAST of the N-GPU wall time is the slowest begin plus the
slowest finish -- not a measurement of one (no second card, no shared host link).  --check compares the merged dumps with the
unpartitioned index.

--solid: INSTEAD of the count, the solid k-mer index (gab_kmer_index_solid_device with --min-freq, --select-rate, --tandem and
--rate) on the same reads, resident, for k = 17 and 15: the thirteen result fields, k-mer positions per second over the wall time of
the call (median of the warm repeats; the call counts for itself and synchronises twice), the device time of its five stages --
count, frequency look-up + selection, capacity, fill, sort -- and the positions that took the tandem test with the reads that left
the on-chip table.  --check compares the fields with the numpy model of tests/solid_model.py (minutes of CPU time at this size).
"""
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

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def ecoli_like_reads(seed=4600000, genome_len=4_600_000, coverage=50, error=0.10):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, genome_len)]
    reads, total = [], 0
    while total < coverage * genome_len:
        ln = int(rng.integers(5001, 20001))
        at = int(rng.integers(0, genome_len - ln))
        a = genome[at:at + ln].copy()
        hit = np.flatnonzero(rng.random(ln) < error)
        a[hit] = acgt[rng.integers(0, 4, hit.size)]
        r = a.tobytes()
        if rng.integers(0, 2):
            r = r.translate(COMP)[::-1]
        reads.append(r)
        total += ln
    return reads


def write_fasta(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n%s\n" % (i, r))


def index_parts(a, reads, d_seq, d_off, d_len):
    """--minimizers W --parts ...: see the head of this file"""
    from genarchbench_amd.kmer import KmerCounter, KmerCounterSet
    out = {}
    whole = KmerCounter() if a.check else None
    for nparts in [int(x) for x in a.parts.split(",")]:
        ks = KmerCounterSet([0] * nparts)
        ks.reserve(len(reads), int(d_seq.numel()))
        per_k = {}
        for k in (17, 15):
            begin_s = [[] for _ in range(nparts)]; finish_s = [[] for _ in range(nparts)]; phases = [[] for _ in range(nparts)]
            for it in range(a.warmup + a.repeats):
                begun = []
                for p, kc in enumerate(ks.parts):
                    t0 = time.perf_counter()
                    begun.append(kc.index_part_begin_device(d_seq, d_off, d_len, k, a.minimizers, p, nparts))
                    if it >= a.warmup:
                        begin_s[p].append(time.perf_counter() - t0)
                m = sum(b["minimizers"] for b in begun); n = sum(b["distinct"] for b in begun)
                done = []
                for p, kc in enumerate(ks.parts):
                    t0 = time.perf_counter()
                    done.append(kc.index_part_finish(m, n, a.rate))
                    if it >= a.warmup:
                        finish_s[p].append(time.perf_counter() - t0)
                        phases[p].append(kc.index_last_phases())
            rows = []
            for p, kc in enumerate(ks.parts):
                row = {"part": p, "begin_seconds": statistics.median(begin_s[p]), "finish_seconds": statistics.median(finish_s[p]),
                       "minimizers": done[p]["minimizers"], "distinct": done[p]["distinct"], "index_entries": done[p]["index_entries"]}
                for f in ("sketch_ms", "count_ms", "fill_ms", "sort_ms"):
                    row[f] = statistics.median(s[f] for s in phases[p])
                row.update({f: v for f, v in kc.index_last_part().items() if f in ("table_slots", "retried")})
                rows.append(row)
            forecast = max(r["begin_seconds"] for r in rows) + max(r["finish_seconds"] for r in rows)
            sums = {f: sum(d[f] for d in done) for f in ("minimizers", "distinct", "filtered_kmers", "filtered_entries", "selected_kmers", "index_entries")}
            per_k[str(k)] = {"partitions": rows, "sums": dict(sums, repetitive_frequency=done[0]["repetitive_frequency"]),
                             "slowest_begin_seconds": max(r["begin_seconds"] for r in rows), "slowest_finish_seconds": max(r["finish_seconds"] for r in rows),
                             "forecast_seconds": forecast}
            if a.check:
                want = whole.index_minimizers_device(d_seq, d_off, d_len, k, a.minimizers, a.rate)
                got = dict(sums, reads_kept=done[0]["reads_kept"], total_len=done[0]["total_len"], repetitive_frequency=done[0]["repetitive_frequency"])
                per_k[str(k)]["matches_unpartitioned"] = bool(got == want and all(np.array_equal(x, y) for x, y in zip(ks.index_dump(), whole.index_dump())))
        ks.close()
        out[str(nparts)] = per_k
    if whole:
        whole.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--coverage", type=int, default=50)
    ap.add_argument("--parts", default="", help="comma-separated partition counts to forecast, e.g. 1,2,4,8")
    ap.add_argument("--minimizers", type=int, default=0, metavar="W", help="measure the minimizer index with window W instead of the count")
    ap.add_argument("--rate", type=float, default=100.0, help="repeat_kmer_rate of --minimizers and --solid")
    ap.add_argument("--solid", action="store_true", help="measure the solid k-mer index instead of the count")
    ap.add_argument("--min-freq", type=int, default=2)
    ap.add_argument("--select-rate", type=float, default=0.4)
    ap.add_argument("--tandem", type=int, default=100)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import genarchbench_amd  # noqa: F401  (before torch: it sets the runtime's default for pageable copies)
    import torch
    if not torch.cuda.is_available():
        sys.exit("kmer_bench.py needs a GPU: there is nothing to measure without one")
    from genarchbench_amd.kmer import KmerCounter, pack_reads

    reads = ecoli_like_reads(coverage=a.coverage)
    seq, off, ln = pack_reads(reads)
    d_seq, d_off, d_len = (torch.from_numpy(x).cuda() for x in (seq, off, ln))
    kc = KmerCounter()
    kc.reserve(len(reads), seq.size)
    out = {"reads": len(reads), "bases": int(seq.size), "repeats": a.repeats, "warmup": a.warmup, "k": {}}
    if a.solid:
        out["solid"] = {"min_freq": a.min_freq, "select_rate": a.select_rate, "tandem_freq": a.tandem, "rate": a.rate, "k": {}}
        for k in (17, 15):
            samples = []
            for it in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                res = kc.index_solid_device(d_seq, d_off, d_len, k, a.min_freq, a.select_rate, a.tandem, a.rate)
                wall = time.perf_counter() - t0
                if it >= a.warmup:
                    samples.append((wall, kc.solid_last_phases()))
            t = statistics.median(s[0] for s in samples)
            row = {"result": res, "positions_per_s": res["positions"] / t, "seconds_median": t, "seconds_min": min(s[0] for s in samples),
                   "seconds_max": max(s[0] for s in samples)}
            for f in ("count_ms", "select_ms", "capacity_ms", "fill_ms", "sort_ms"):
                row[f] = statistics.median(s[1][f] for s in samples)
            row.update(kc.solid_last_stats())
            if a.check:
                from tests import solid_model
                m = solid_model.build_index(reads, k, a.min_freq, a.select_rate, a.tandem, a.rate)
                row["matches_model"] = all(res[f] == m[f] for f in solid_model.FIELDS)
            out["solid"]["k"][str(k)] = row
    elif a.minimizers:
        out["minimizers"] = {"window": a.minimizers, "rate": a.rate, "k": {}}
        for k in (17, 15):
            samples = []
            for it in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                res = kc.index_minimizers_device(d_seq, d_off, d_len, k, a.minimizers, a.rate)
                wall = time.perf_counter() - t0
                if it >= a.warmup:
                    samples.append((wall, kc.index_last_phases()))
            positions = int(np.maximum(ln[ln > 5000].astype(np.int64) - k, 0).sum())
            t = statistics.median(s[0] for s in samples)
            row = {"result": res, "positions": positions, "positions_per_s": positions / t, "seconds_median": t,
                   "seconds_min": min(s[0] for s in samples), "seconds_max": max(s[0] for s in samples)}
            for f in ("sketch_ms", "count_ms", "fill_ms", "sort_ms"):
                row[f] = statistics.median(s[1][f] for s in samples)
            # the reference's own numbers for this very set, where they were recorded (tests/golden/make_minimizer_golden.py --time)
            rec_path = os.path.join(ROOT, "tests", "golden", "kmer_minimizer_expected.json")
            if os.path.exists(rec_path) and (a.coverage, a.minimizers, a.rate) == (50, 10, 100.0):
                rec = json.load(open(rec_path)).get("reference_cpu_time", {}).get("k", {}).get(str(k))
                if rec:
                    row["matches_reference_record"] = all(res[f] == rec[f] for f in ("repetitive_frequency", "filtered_entries", "selected_kmers",
                                                                                     "index_entries"))
            if a.check and not a.parts:      # (with --parts, --check compares the merged partitions with this build instead)
                from tests import minimizer_model
                m = minimizer_model.build_index(reads, k, a.minimizers, a.rate)
                row["matches_model"] = all(res[f] == m[f] for f in minimizer_model.FIELDS)
            out["minimizers"]["k"][str(k)] = row
    else:
        for k in (17, 15):
            row = {}
            res = None
            for mode in ("resident", "host"):
                samples = []
                for it in range(a.warmup + a.repeats):
                    t0 = time.perf_counter()
                    res = kc.count_device(d_seq, d_off, d_len, k) if mode == "resident" else kc.count((seq, off, ln), k)
                    wall = time.perf_counter() - t0
                    st = kc.last_stats()
                    if it >= a.warmup:
                        samples.append((st["total_ms"] * 1e-3 if mode == "resident" else wall, wall, st))
                pos = res["positions"]
                t = statistics.median(s[0] for s in samples)
                row[mode] = {"positions_per_s": pos / t, "seconds_median": t, "seconds_min": min(s[0] for s in samples), "seconds_max": max(s[0] for s in samples),
                             "wall_seconds_median": statistics.median(s[1] for s in samples),
                             "pack_ms": statistics.median(s[2]["pack_ms"] for s in samples),
                             "count_ms": statistics.median(s[2]["count_ms"] for s in samples),
                             "reduce_ms": statistics.median(s[2]["reduce_ms"] for s in samples)}
            st = kc.last_stats()
            inserts = res["positions"] - st["merged"]
            row["result"] = res
            row["inserts"] = inserts
            row["lines_per_insert"] = st["probes"] / max(inserts, 1)
            row["inserts_per_s_in_count_stage"] = inserts / (row["resident"]["count_ms"] * 1e-3)
            if a.check:
                from tests import kmer_model
                m = kmer_model.model(reads, k)
                row["matches_model"] = all(res[f] == m[f] for f in kmer_model.FIELDS)
            out["k"][str(k)] = row
    if a.solid:
        pass                                    # (key-space partitions of the solid index are not offered: the rank of a read needs every count)
    elif a.parts and a.minimizers:
        out["index_parts"] = index_parts(a, reads, d_seq, d_off, d_len)
    elif a.parts:
        out["parts"] = {}
        for nparts in [int(x) for x in a.parts.split(",")]:
            kc.reserve_part(len(reads), seq.size, nparts)
            per_k = {}
            for k in (17, 15):
                rows = []
                for part in range(nparts):
                    samples = []
                    for it in range(a.warmup + a.repeats):
                        res = kc.count_part_device(d_seq, d_off, d_len, k, part, nparts)
                        if it >= a.warmup:
                            samples.append(kc.last_stats())
                    st, lp = samples[-1], kc.last_part()
                    med = lambda f: statistics.median(s[f] for s in samples)
                    rows.append({"part": part, "pack_ms": med("pack_ms"), "count_ms": med("count_ms"), "reduce_ms": med("reduce_ms"),
                                 "total_ms": med("total_ms"), "total_ms_min": min(s["total_ms"] for s in samples),
                                 "total_ms_max": max(s["total_ms"] for s in samples), "distinct": res["distinct"],
                                 "probes": st["probes"], "merged": st["merged"], "table_slots": lp["table_slots"],
                                 "retried": lp["retried"]})
                slowest = max(r["total_ms"] for r in rows)
                per_k[str(k)] = {"partitions": rows, "positions": res["positions"], "distinct_sum": sum(r["distinct"] for r in rows),
                                 "merged_sum": sum(r["merged"] for r in rows), "probes_sum": sum(r["probes"] for r in rows),
                                 "slowest_total_ms": slowest, "slowest_count_ms": max(r["count_ms"] for r in rows),
                                 "forecast_positions_per_s": res["positions"] / (slowest * 1e-3)}
            out["parts"][str(nparts)] = per_k
    kc.close()
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
