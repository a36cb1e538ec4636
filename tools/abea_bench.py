#!/usr/bin/env python3
"""abea throughput: a generated set of reads resident in HBM through gab_abea_align_device; median of warm repeats.

    python tools/abea_bench.py [--reads 4096] [--min-bases 5000] [--max-bases 15000] [--repeats 7] [--seed 1] [--json out.json]
    python tools/abea_bench.py --signal --reads 1024      raw signal for the same kind of reads through gab_abea_events_device,
                                                          gab_abea_scalings_device and gab_abea_align_device: samples/s, events/s,
                                                          the stage times, chunks_redone and reads_serial_sums
    python tools/abea_bench.py [--signal] --calibrate     adds gab_abea_calibrate_device on the pairs of the alignment to either mode and
                                                          prints its time next to align's
    python tools/abea_bench.py [--signal] --calibrate --realign
                                                          adds gab_abea_realign_device behind that: a generated reference and CIGAR per read
                                                          (substitutions, insertions and deletions at 3 % each, half the reads reverse); wall
                                                          time, rows/s, cells/s, reads_requeued and the preparation / Viterbi / requeue split
    python tools/abea_bench.py [--signal] --calibrate --meth
                                                          adds gab_abea_meth_device on the same references and CIGARs (realign runs too, so that
                                                          align, realign and call-methylation are timed in one session) with a seeded CpG model:
                                                          wall time, sites/s, cells/s and the preparation / scoring split

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


RANGE, DIGITISATION = 1402.882, 8192.0      # pA over the ADC's span: a grid of about 0.17 pA


def generate_signal(rng, mean, seq, seq_off, seq_len):
    """raw samples for the same reads: the level of every k-mer held for 3 + geometric(1/6) samples (about 9), Gaussian noise of
    1.5 pA, quantised to ADC codes (kept as float, as the reference holds them); one offset per read"""
    from genarchbench_amd import abea
    code_of = np.zeros(256, np.int64); code_of[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)
    unit = RANGE / DIGITISATION
    raws, offsets = [], []
    for o, n in zip(seq_off, seq_len):
        codes = code_of[seq[o:o + n]]
        nk = int(n) - abea.K + 1
        ranks = np.zeros(nk, np.int64)
        for t in range(abea.K):
            ranks = ranks * 4 + codes[t:t + nk]
        dwell = 3 + rng.geometric(1 / 6.0, nk)
        pa = np.repeat(mean[ranks].astype(np.float64), dwell) + 1.5 * rng.standard_normal(int(dwell.sum()))
        offset = float(rng.integers(-20, 21))
        raws.append(np.clip(np.rint(pa / unit - offset), -32768, 32767).astype(np.float32)); offsets.append(offset)
    n_samples = np.array([r.size for r in raws], np.int32)
    raw_off = np.concatenate([[0], np.cumsum(n_samples[:-1], dtype=np.int64)]).astype(np.int64)
    n = len(raws)
    return (np.concatenate(raws), raw_off, n_samples, np.full(n, RANGE, np.float32), np.full(n, DIGITISATION, np.float32), np.array(offsets, np.float32))


def main_signal(a):
    """the chain on the resident set: events, scalings, align; per stage the median wall time of the warm repeats"""
    import genarchbench_amd  # noqa: F401
    import torch
    from genarchbench_amd import abea
    rng = np.random.default_rng(a.seed)
    (mean, stdv), packed, _ = generate(rng, a.reads, a.min_bases, a.max_bases)
    sig = generate_signal(rng, mean, packed[0], packed[1], packed[2])
    h = abea.EventAligner(mean, stdv)
    n = a.reads
    d_sig = [torch.from_numpy(x).cuda() for x in sig]
    d_seq, d_so, d_sl = (torch.from_numpy(x).cuda() for x in packed[:3])
    cap = int(sig[2].sum()) // 2 + n
    n_events = torch.zeros(n, dtype=torch.int32, device="cuda"); event_off = torch.zeros(n, dtype=torch.int64, device="cuda")
    ev_mean = torch.empty(cap, dtype=torch.float32, device="cuda"); ev_stdv = torch.empty_like(ev_mean); ev_len = torch.empty_like(ev_mean)
    ev_start = torch.empty(cap, dtype=torch.int32, device="cuda"); total = torch.zeros(1, dtype=torch.int64, device="cuda")
    scale = torch.zeros(n, dtype=torch.float32, device="cuda"); shift = torch.zeros_like(scale)
    res = torch.zeros(n * abea.READ.itemsize, dtype=torch.uint8, device="cuda")
    pairs = None
    n_kmers = packed[2].astype(np.int64) - abea.K + 1
    d_mo = torch.from_numpy(np.concatenate([[0], np.cumsum(n_kmers[:-1])]).astype(np.int64)).cuda()
    rmap = torch.empty((int(n_kmers.sum()), 2), dtype=torch.int32, device="cuda") if a.calibrate else None
    cal = torch.zeros(n * abea.CALIB.itemsize, dtype=torch.uint8, device="cuda")
    realign = Realign(torch, rng, packed) if a.realign else None
    meth = Meth(torch, rng, h, mean, stdv, realign.dev, realign.aln) if a.meth else None
    runs = []
    for it in range(a.repeats + 1):                                  # the first run allocates: not counted
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = h.detect_events_device(*d_sig, n_events, event_off, ev_mean, ev_stdv, ev_start, ev_len, total)
        t1 = time.perf_counter()
        if rc:
            raise SystemExit(f"{int(total.item())} events do not fit {cap}")
        est = h.events_last_stats()
        ne = n_events.cpu().numpy()
        room = abea.pair_room(packed[2], ne)
        pair_off = np.concatenate([[0], np.cumsum(room[:-1])]).astype(np.int64)
        d_po = torch.from_numpy(pair_off).cuda()
        if pairs is None:
            pairs = torch.empty((int(room.sum()), 2), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        h.estimate_scalings_device(d_seq, d_so, d_sl, ev_mean, event_off, n_events, scale, shift)
        t3 = time.perf_counter()
        h.align_device(d_seq, d_so, d_sl, ev_mean, event_off, n_events, scale, shift, pairs, d_po, res)
        t4 = time.perf_counter()
        runs.append({"events_ms": (t1 - t0) * 1e3, "scalings_ms": (t3 - t2) * 1e3, "align_ms": (t4 - t3) * 1e3, "ev": est, "sc": h.scalings_last_stats(), "al": h.last_stats()})
        if a.calibrate:
            runs[-1].update(timed_calibrate(h, torch, (d_seq, d_so, d_sl, ev_mean, event_off, n_events, scale, shift), pairs, d_po, res, rmap, d_mo, cal))
        if realign:
            runs[-1].update(realign.timed(h, d_sl, ev_mean, event_off, n_events, rmap, d_mo, cal))
        if meth:
            runs[-1].update(meth.timed(h, d_sl, ev_mean, event_off, n_events, rmap, d_mo, cal))
    warm = runs[1:]
    med = lambda f: float(np.median([f(r) for r in warm]))
    rec = res.cpu().numpy().view(abea.READ)
    est = warm[-1]["ev"]
    ev_ms = med(lambda r: r["events_ms"])
    out = {"mode": "signal", "reads": n, "bases": int(packed[2].sum()), "samples": est["samples"], "events": est["events"], "repeats": a.repeats,
           "events_wall_ms_median": round(ev_ms, 3), "events_wall_ms_all": [round(r["events_ms"], 3) for r in warm],
           "samples_per_s": round(est["samples"] / (ev_ms * 1e-3), 1), "events_per_s": round(est["events"] / (ev_ms * 1e-3), 1),
           "sums_tstat_kernels_ms": round(med(lambda r: r["ev"]["sums_ms"]), 3), "detector_kernels_ms": round(med(lambda r: r["ev"]["detect_ms"]), 3),
           "fill_kernels_ms": round(med(lambda r: r["ev"]["fill_ms"]), 3), "events_first_to_last_kernel_ms": round(med(lambda r: r["ev"]["total_ms"]), 3),
           "chunks": est["chunks"], "chunks_redone": est["chunks_redone"], "reads_serial_sums": est["reads_serial_sums"],
           "scalings_wall_ms_median": round(med(lambda r: r["scalings_ms"]), 3), "scalings_sums_in_order": warm[-1]["sc"], "align_wall_ms_median": round(med(lambda r: r["align_ms"]), 3),
           "align_all_kernels_ms": round(med(lambda r: r["al"]["total_ms"]), 3), "reads_passing": int((rec["n_pairs"] > 0).sum()),
           "device": torch.cuda.get_device_name(0)}
    if a.calibrate:
        out.update(calibrate_report(warm, cal.cpu().numpy().view(abea.CALIB)))
    if realign:
        out.update(realign.report(warm))
    if meth:
        out.update(meth.report(warm))
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1); f.write("\n")


def timed_calibrate(h, torch, inputs, pairs, d_po, res, rmap, d_mo, cal):
    """gab_abea_calibrate_device on the alignment's pairs and records, all resident; n_pairs is the first field of every record"""
    from genarchbench_amd import abea
    n = inputs[2].numel()
    n_pairs = res.view(torch.int32).view(n, abea.READ.itemsize // 4)[:, 0].contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h.calibrate_device(*inputs, pairs, d_po, n_pairs, rmap, d_mo, cal)
    return {"calibrate_ms": (time.perf_counter() - t0) * 1e3, "cal": h.calibrate_last_stats()}


def generate_alignments(rng, seq, seq_off, seq_len, rate=0.03):
    """per read a reference and a CIGAR, as a mapper would report them: every read base is an insertion, a substitution or a match,
    a deletion of one reference base goes before some; every other read maps to the reverse strand (its BAM record holds the reverse
    complement).  -> ref, ref_off, ref_len, ref_pos, is_rev, cigar (BAM encoding), cigar_off, n_cigar"""
    comp = np.zeros(256, np.uint8); comp[np.frombuffer(b"ACGT", np.uint8)] = np.frombuffer(b"TGCA", np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    refs, cigars = [], []
    for i, (o, n) in enumerate(zip(seq_off, seq_len)):
        bases = seq[o:o + n]
        if i % 2:
            bases = comp[bases[::-1]]
        u = rng.random(int(n))
        u[0] = u[-1] = 1.0                               # the CIGAR begins and ends with a match
        ins = u < rate; dele = (u >= rate) & (u < 2 * rate); sub = (u >= 2 * rate) & (u < 3 * rate)
        own = np.where(sub, acgt[(np.searchsorted(acgt, bases) + rng.integers(1, 4, int(n))) % 4], bases)
        two = np.stack([acgt[rng.integers(0, 4, int(n))], own], 1)      # (a deleted reference base, the base's own)
        keep = np.stack([dele, ~ins], 1)
        refs.append(two[keep])
        ops = np.stack([np.full(int(n), 2), np.where(ins, 1, 0)], 1)[np.stack([dele, np.ones(int(n), bool)], 1)]      # D before the base; I or M
        cut = np.flatnonzero(np.diff(ops)) + 1
        starts = np.concatenate([[0], cut]); lens = np.diff(np.concatenate([starts, [ops.size]]))
        cigars.append((lens.astype(np.uint32) << 4) | ops[starts].astype(np.uint32))
    ref_len = np.array([r.size for r in refs], np.int32); n_cigar = np.array([c.size for c in cigars], np.int32)
    off = lambda ln: np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.int64)]).astype(np.int64)
    return (np.concatenate(refs), off(ref_len), ref_len, rng.integers(0, 4_000_000, len(refs)).astype(np.int32), (np.arange(len(refs)) % 2).astype(np.uint8),
            np.concatenate(cigars), off(n_cigar), n_cigar)


class Realign:
    """gab_abea_realign_device behind calibrate, everything resident; the entries' room is one per event (no N operations)"""

    def __init__(self, torch, rng, packed):
        self.torch = torch
        aln = self.aln = generate_alignments(rng, packed[0], packed[1], packed[2])
        self.dev = [torch.from_numpy(np.ascontiguousarray(x if x.dtype != np.uint32 else x.view(np.int32))).cuda() for x in aln]
        self.out = None

    def timed(self, h, d_sl, ev_mean, event_off, n_events, rmap, d_mo, cal):
        from genarchbench_amd import abea
        torch = self.torch
        if self.out is None:
            self.out_off = event_off.clone()              # n_events entries of room per read, back to back as the events are
            self.out = torch.empty(int(n_events.sum().item()) * abea.EALN.itemsize, dtype=torch.uint8, device="cuda")
            self.res = torch.zeros(n_events.numel() * abea.REALIGN.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.realign_device(*self.dev, d_sl, ev_mean, event_off, n_events, rmap, d_mo, cal, self.out, self.out_off, self.res)
        return {"realign_ms": (time.perf_counter() - t0) * 1e3, "rl": h.realign_last_stats()}

    def report(self, warm):
        from genarchbench_amd import abea
        med = lambda f: float(np.median([f(r) for r in warm]))
        st = warm[-1]["rl"]
        ms = med(lambda r: r["realign_ms"])
        rec = self.res.cpu().numpy().view(abea.REALIGN)
        return {"realign_wall_ms_median": round(ms, 3), "realign_wall_ms_all": [round(r["realign_ms"], 3) for r in warm],
                "realign_rows_per_s": round(st["rows"] / (ms * 1e-3), 1), "realign_cells_per_s": round(st["cells"] / (ms * 1e-3), 1),
                "realign_hmm_segments": st["hmm_segments"], "realign_rows": st["rows"], "realign_cells": st["cells"], "reads_requeued": st["reads_requeued"],
                "realign_prep_ms": round(med(lambda r: r["rl"]["prep_ms"]), 3), "realign_viterbi_ms": round(med(lambda r: r["rl"]["viterbi_ms"]), 3),
                "realign_requeue_ms": round(med(lambda r: r["rl"]["requeue_ms"]), 3), "realign_first_to_last_kernel_ms": round(med(lambda r: r["rl"]["total_ms"]), 3),
                "realign_entries": int(rec["n_entries"].sum()), "realign_max_rows": int(rec["max_rows"].max()),
                "realign_flags": {str(k): int((rec["flags"] == k).sum()) for k in sorted(set(rec["flags"].tolist()))}}


def cpg_model(rng, mean, stdv):
    """15625 entries over A C G M T from the nucleotide model: a k-mer with M takes the values of the k-mer with C in its place, its
    mean shifted by -4 .. +4"""
    from genarchbench_amd import abea
    digits = np.stack([(np.arange(abea.NKMER_CPG) // 5 ** (abea.K - 1 - t)) % 5 for t in range(abea.K)], 1)
    r4 = (np.array([0, 1, 2, 1, 3])[digits] * 4 ** np.arange(abea.K - 1, -1, -1)).sum(1)
    has_m = (digits == 3).any(1)
    m = np.where(has_m, mean[r4] + rng.uniform(-4, 4, abea.NKMER_CPG), mean[r4]).astype(np.float32)
    sd = stdv[r4].astype(np.float32)
    return m, sd, np.log(sd.astype(np.float64)).astype(np.float32)


class Meth:
    """gab_abea_meth_device behind calibrate on Realign's references and CIGARs, everything resident; a site record of room per CpG group"""

    def __init__(self, torch, rng, h, mean, stdv, aln_dev, aln_host):
        from genarchbench_amd import abea
        self.torch, self.dev = torch, aln_dev
        h.set_cpg_model(*cpg_model(rng, mean, stdv))
        room = abea.meth_room(aln_host[0], aln_host[1], aln_host[2])
        self.out_off = torch.from_numpy(np.concatenate([[0], np.cumsum(room[:-1])]).astype(np.int64)).cuda()
        self.out = torch.empty(max(int(room.sum()), 1) * abea.SITE.itemsize, dtype=torch.uint8, device="cuda")
        self.res = torch.zeros(room.size * abea.METH.itemsize, dtype=torch.uint8, device="cuda")

    def timed(self, h, d_sl, ev_mean, event_off, n_events, rmap, d_mo, cal):
        torch = self.torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.call_methylation_device(*self.dev, d_sl, ev_mean, event_off, n_events, rmap, d_mo, cal, self.out, self.out_off, self.res)
        return {"meth_ms": (time.perf_counter() - t0) * 1e3, "mt": h.meth_last_stats()}

    def report(self, warm):
        from genarchbench_amd import abea
        med = lambda f: float(np.median([f(r) for r in warm]))
        st = warm[-1]["mt"]
        ms = med(lambda r: r["meth_ms"])
        rec = self.res.cpu().numpy().view(abea.METH)
        return {"meth_wall_ms_median": round(ms, 3), "meth_wall_ms_all": [round(r["meth_ms"], 3) for r in warm],
                "meth_sites_per_s": round(st["sites"] / (ms * 1e-3), 1), "meth_cells_per_s": round(st["cells"] / (ms * 1e-3), 1),
                "meth_groups": st["groups"], "meth_sites": st["sites"], "meth_rows": st["rows"], "meth_cells": st["cells"],
                "meth_prep_ms": round(med(lambda r: r["mt"]["prep_ms"]), 3), "meth_score_ms": round(med(lambda r: r["mt"]["score_ms"]), 3),
                "meth_first_to_last_kernel_ms": round(med(lambda r: r["mt"]["total_ms"]), 3),
                "meth_skipped": {k: int(rec[k].sum()) for k in ("skipped_start", "skipped_span", "skipped_unbounded", "skipped_short")},
                "meth_flags": {str(k): int((rec["flags"] == k).sum()) for k in sorted(set(rec["flags"].tolist()))}}


def calibrate_report(warm, rec):
    med = lambda f: float(np.median([f(r) for r in warm]))
    st = warm[-1]["cal"]
    return {"calibrate_wall_ms_median": round(med(lambda r: r["calibrate_ms"]), 3), "calibrate_wall_ms_all": [round(r["calibrate_ms"], 3) for r in warm],
            "calibrate_kernels_ms": round(med(lambda r: r["cal"]["kernel_ms"]), 3), "calibrate_first_to_last_kernel_ms": round(med(lambda r: r["cal"]["total_ms"]), 3),
            "reads_recalibrated": st["recalibrated"], "m_states": st["m_states"],
            "read_stat_flags": {str(k): int((rec["read_stat_flag"] == k).sum()) for k in (0, 1, 2, 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096); ap.add_argument("--min-bases", type=int, default=5000)
    ap.add_argument("--max-bases", type=int, default=15000); ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1); ap.add_argument("--json")
    ap.add_argument("--signal", action="store_true", help="raw signal in: event detection, scalings and align, timed per stage")
    ap.add_argument("--calibrate", action="store_true", help="add the base-to-event map, recalibration and read checks after align, timed")
    ap.add_argument("--realign", action="store_true", help="add realign_read after --calibrate, on a generated reference and CIGAR per read, timed")
    ap.add_argument("--meth", action="store_true", help="add call-methylation after --calibrate, on the references and CIGARs of --realign (which it implies), timed")
    a = ap.parse_args()
    a.realign = a.realign or a.meth
    if a.realign and not a.calibrate:
        ap.error("--realign and --meth run on what --calibrate leaves: give both")
    if a.signal:
        return main_signal(a)
    import genarchbench_amd  # noqa: F401  (before torch: the runtime's default for pageable copies)
    import torch
    from genarchbench_amd import abea
    rng = np.random.default_rng(a.seed)
    (mean, stdv), packed, room = generate(rng, a.reads, a.min_bases, a.max_bases)
    h = abea.EventAligner(mean, stdv)
    dev = [torch.from_numpy(x).cuda() for x in packed]
    pairs = torch.empty((room, 2), dtype=torch.int32, device="cuda")
    res = torch.zeros(a.reads * abea.READ.itemsize, dtype=torch.uint8, device="cuda")
    n_kmers = packed[2].astype(np.int64) - abea.K + 1
    d_mo = torch.from_numpy(np.concatenate([[0], np.cumsum(n_kmers[:-1])]).astype(np.int64)).cuda()
    rmap = torch.empty((int(n_kmers.sum()), 2), dtype=torch.int32, device="cuda") if a.calibrate else None
    cal = torch.zeros(a.reads * abea.CALIB.itemsize, dtype=torch.uint8, device="cuda")
    realign = Realign(torch, rng, packed) if a.realign else None
    meth = Meth(torch, rng, h, mean, stdv, realign.dev, realign.aln) if a.meth else None
    walls, stats, cals = [], [], []
    for it in range(a.repeats + 1):                                  # the first run allocates: not counted
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.align_device(*dev[:8], pairs, dev[8], res)
        walls.append(time.perf_counter() - t0); stats.append(h.last_stats())
        if a.calibrate:
            cals.append(timed_calibrate(h, torch, dev[:8], pairs, dev[8], res, rmap, d_mo, cal))
        if realign:
            cals[-1].update(realign.timed(h, dev[2], dev[3], dev[4], dev[5], rmap, d_mo, cal))
        if meth:
            cals[-1].update(meth.timed(h, dev[2], dev[3], dev[4], dev[5], rmap, d_mo, cal))
    rec = res.cpu().numpy().view(abea.READ)
    order = np.argsort(walls[1:]); mid = 1 + int(order[len(order) // 2])
    st, wall = stats[mid], walls[mid]
    out = {"reads": a.reads, "bases": int(packed[2].sum()), "events": int(packed[5].sum()), "bands": st["bands"], "cells": st["cells"],
           "launches": st["launches"], "repeats": a.repeats, "wall_ms_median": round(wall * 1e3, 3),
           "wall_ms_all": [round(w * 1e3, 3) for w in walls[1:]], "reads_per_s": round(a.reads / wall, 1), "cells_per_s": round(st["cells"] / wall, 1),
           "ms_per_launch": round(wall * 1e3 / st["launches"], 3), "dp_kernel_ms": round(st["kernel_ms"], 3), "all_kernels_ms": round(st["total_ms"], 3),
           "dp_share": round(st["kernel_ms"] / st["total_ms"], 4), "reads_passing": int((rec["n_pairs"] > 0).sum()),
           "device": torch.cuda.get_device_name(0)}
    if a.calibrate:
        out.update(calibrate_report(cals[1:], cal.cpu().numpy().view(abea.CALIB)))
    if realign:
        out.update(realign.report(cals[1:]))
    if meth:
        out.update(meth.report(cals[1:]))
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
