#!/usr/bin/env python3
"""Build machine only: writes tests/golden/abea_calib_small.npz (the reference's path for every read of abea_small.npz, one byte per
pair, and the constructed cases of tests/abea_calib_model.py's seeded generator: bases, event means, scalings and lattice paths) and
tests/golden/abea_calib_expected.json (what the reference's postalign, abea/src/align.c:550-650, and recalibrate_model,
align.c:655-762, return per read, and the flag that the checks of abea/src/f5c.c:1474-1501 set; under "long" the same for the
generator's reads of 16384 k-mers and more, whose inputs are not stored).

The reference's align.c is compiled on its own in a temporary directory outside the repository, with the stand-in headers of
make_abea_golden.py, -O2 -std=c++11 -ffp-contract=off, and a small harness of this script's own that declares the three prototypes,
runs align() on the fixture reads and hands the pairs (the fixture's own, or a constructed case's) to postalign and
recalibrate_model.  Nothing compiled and no reference text is kept.  The .npz is written with fixed time stamps, so that the script
reproduces the committed files byte for byte.

    python tests/golden/make_abea_calib_golden.py [/root/reference/benchmarks] [--keep-times]

--keep-times: the reference's measured seconds are taken from the committed .json instead of this run's (they are the only thing
that differs from one run to the next)."""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import abea_calib_model as M  # noqa: E402
import make_abea_events_golden as G1  # noqa: E402
import make_abea_golden as G0  # noqa: E402

# what the fixture held when it was made: the generator must not fall below it
AT_LEAST = {"align_returns_0": 13, "not_recalibrated": 69, "recalibrated": 123, "m_states_195_to_205": 7, "first_entry_E": 9,
            "kmer_without_event": 147}

HARNESS = r"""
#include "f5c.h"
#include <time.h>
int32_t align(AlignedPair* out_2, char* sequence, int32_t sequence_len, event_table events, model_t* models, scalings_t scaling, float sample_rate);
int32_t postalign(event_alignment_t* alignment, index_pair_t* base_to_event_map, double* events_per_base, char* sequence, int32_t n_kmers,
                  AlignedPair* event_alignment, int32_t n_events);
bool recalibrate_model(model_t* pore_model, event_table et, scalings_t* scallings, const event_alignment_t* alignment_output,
                       int32_t num_alignments, bool scale_var);
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
static double now() { struct timespec a; clock_gettime(CLOCK_MONOTONIC, &a); return a.tv_sec + 1e-9 * a.tv_nsec; }
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    static model_t model[4096];
    memset(model, 0, sizeof model);
    for (int i = 0; i < 4096; i++) { float v[3]; rd(v, sizeof v, in); model[i].level_mean = v[0]; model[i].level_stdv = v[1]; model[i].level_log_stdv = v[2]; }
    int32_t n_reads; rd(&n_reads, 4, in);
    double t_post = 0, t_recal = 0;
    for (int r = 0; r < n_reads; r++) {
        int32_t len, ne, given; float sc[2];            /* given: -1 = run align(), else that many pairs follow */
        rd(&len, 4, in); rd(&ne, 4, in); rd(&given, 4, in); rd(sc, 8, in);
        char *seq = (char *)malloc(len + 1); rd(seq, len, in); seq[len] = 0;
        float *ev = (float *)malloc(4 * (size_t)ne); rd(ev, 4 * (size_t)ne, in);
        event_table et; memset(&et, 0, sizeof et);
        et.n = ne; et.event = (event_t *)calloc(ne, sizeof(event_t));
        for (int i = 0; i < ne; i++) et.event[i].mean = ev[i];
        scalings_t s; memset(&s, 0, sizeof s); s.scale = sc[0]; s.shift = sc[1];
        const int32_t n_kmers = len - KMER_SIZE + 1;
        const size_t room = 2 * (size_t)ne + (size_t)n_kmers + 2;
        AlignedPair *pairs = (AlignedPair *)malloc(sizeof(AlignedPair) * room);
        memset(pairs, 0xff, sizeof(AlignedPair) * room);
        int32_t n_pairs, path_len = 0;
        if (given < 0) {
            n_pairs = align(pairs, seq, len, et, model, s, 4000.0f);
            while ((size_t)path_len < room && pairs[path_len].ref_pos != -1) path_len++;
        } else {
            for (int i = 0; i < given; i++) { int32_t v[2]; rd(v, 8, in); pairs[i].ref_pos = v[0]; pairs[i].read_pos = v[1]; }
            n_pairs = path_len = given;
        }
        /* what the reference leaves unset is set here to what the library defines */
        index_pair_t *map = (index_pair_t *)malloc(sizeof(index_pair_t) * n_kmers);
        for (int i = 0; i < n_kmers; i++) map[i].start = map[i].stop = -1;
        double events_per_base = 0;
        int32_t n_alignment = 0, n_m = 0, recalibrated = 0; uint32_t flag = 0;
        s.var = 1.0f; s.log_var = 0.0f;
        if (n_pairs > 0) {
            event_alignment_t *al = (event_alignment_t *)malloc(sizeof(event_alignment_t) * room);
            double t0 = now();
            n_alignment = postalign(al, map, &events_per_base, seq, n_kmers, pairs, n_pairs);
            double t1 = now();
            recalibrated = recalibrate_model(model, et, &s, al, n_alignment, 1) ? 1 : 0;
            double t2 = now();
            t_post += t1 - t0; t_recal += t2 - t1;
            for (int i = 0; i < n_alignment; i++) n_m += al[i].hmm_state == 'M';
            if (!recalibrated || s.var > 2.5) flag = FAILED_CALIBRATION;      /* MIN_CALIBRATION_VAR, f5cmisc.h:9 */
            else if (events_per_base > 5.0) flag = FAILED_QUALITY_CHK;
            free(al);
        } else flag = FAILED_ALIGNMENT;
        fwrite(&n_pairs, 4, 1, out); fwrite(&path_len, 4, 1, out);
        for (int i = 0; i < path_len; i++) { int32_t v[2] = {pairs[i].ref_pos, pairs[i].read_pos}; fwrite(v, 4, 2, out); }
        int32_t head[4] = {n_alignment, n_m, recalibrated, (int32_t)flag}; fwrite(head, 4, 4, out);
        float f4[4] = {s.scale, s.shift, s.var, s.log_var}; fwrite(f4, 4, 4, out);
        fwrite(&events_per_base, 8, 1, out);
        fwrite(map, sizeof(index_pair_t), n_kmers, out);
        free(seq); free(ev); free(et.event); free(pairs); free(map);
    }
    fwrite(&t_post, 8, 1, out); fwrite(&t_recal, 8, 1, out);
    fclose(out);
    return 0;
}
"""


def run_reference(ref, model, reads):
    """reads: (bases, events, scale, shift, path or None) -> per read (n_pairs, path, record, map), and the seconds of the two functions"""
    src = os.path.join(ref, "abea", "src")
    with tempfile.TemporaryDirectory(prefix="abea_calib_golden_") as tmp:
        os.makedirs(os.path.join(tmp, "stub", "htslib"))
        for name, text in (("htslib/sam.h", G0.STUB_SAM_H), ("htslib/faidx.h", ""), ("htslib/hts.h", ""), ("hdf5.h", "")):
            open(os.path.join(tmp, "stub", name), "w").write(text)
        open(os.path.join(tmp, "harness.cpp"), "w").write(HARNESS)
        flags = ["-O2", "-std=c++11", "-ffp-contract=off", "-DFAST5LITE_H", "-DNANOPOLISH_READ_DB_H", "-I" + os.path.join(tmp, "stub"), "-I" + src]
        exe = os.path.join(tmp, "harness")
        subprocess.check_call(["g++"] + flags + [os.path.join(tmp, "harness.cpp"), os.path.join(src, "align.c"), "-o", exe, "-lm"])
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.stack(model, 1).astype("<f4").tobytes())
            f.write(struct.pack("<i", len(reads)))
            for seq, ev, sc, sh, path in reads:
                f.write(struct.pack("<iiiff", len(seq), ev.size, -1 if path is None else len(path), float(sc), float(sh)) + seq + ev.astype("<f4").tobytes())
                if path is not None:
                    f.write(np.ascontiguousarray(path, "<i4").tobytes())
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], stderr=subprocess.DEVNULL)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    out, at = [], 0
    for seq, *_ in reads:
        n_kmers = len(seq) - M.K + 1
        n_pairs, path_len = struct.unpack_from("<ii", raw, at); at += 8
        path = np.frombuffer(raw, "<i4", 2 * path_len, at).reshape(-1, 2); at += 8 * path_len
        n_alignment, n_m, recal, flag = struct.unpack_from("<iiii", raw, at); at += 16
        scale, shift, var, log_var = np.frombuffer(raw, "<f4", 4, at); at += 16
        (epb,) = struct.unpack_from("<d", raw, at); at += 8
        m = np.frombuffer(raw, "<i4", 2 * n_kmers, at).reshape(-1, 2); at += 8 * n_kmers
        rec = dict(n_alignment=n_alignment, n_m_state=n_m, read_stat_flag=flag, recalibrated=recal, scale=scale, shift=shift, var=var,
                   log_var=log_var, events_per_base=epb)
        out.append((n_pairs, path, rec, m))
    t_post, t_recal = struct.unpack_from("<dd", raw, at)
    return out, t_post, t_recal


def first_entry_is_E(m, ranks):
    """does some k-mer's first entry come out 'E' (the previous k-mer that had events has the same rank)?"""
    prev = -1
    for k in range(len(m)):
        if m[k, 0] != -1:
            if ranks[k] == prev:
                return True
            prev = ranks[k]
    return False


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ref = args[0] if args else "/root/reference/benchmarks"
    z = np.load(os.path.join(HERE, "abea_small.npz"))
    model = (z["level_mean"], z["level_stdv"], z["level_log_stdv"])
    so = np.concatenate([[0], np.cumsum(z["seq_len"], dtype=np.int64)]); eo = np.concatenate([[0], np.cumsum(z["n_events"], dtype=np.int64)])
    fixture = [(z["seq"][so[i]:so[i + 1]].tobytes(), z["events"][eo[i]:eo[i + 1]], z["scale"][i], z["shift"][i], None) for i in range(z["seq_len"].size)]
    got, t_post, t_recal = run_reference(ref, model, fixture)

    # the constructed cases: the longest fixture read that aligned carries the re-noised events
    longest = max((i for i, g in enumerate(got) if g[0] > 0), key=lambda i: len(fixture[i][0]))
    cases = M.make_cases(model[0], model[1], fixture[longest][:4] + (got[longest][1][:got[longest][0]],))
    names = list(cases)
    got_c, t_post_c, t_recal_c = run_reference(ref, model, [cases[n] for n in names])
    # the reads longer than the map kernel's stride: regenerated by seed wherever they are used, only the reference's record (with the
    # digest of its map) is kept
    long_reads = M.long_reads(model[0], model[1])
    got_l, _, _ = run_reference(ref, model, list(long_reads.values()))
    for (n, r), g in zip(long_reads.items(), got_l):
        assert g[0] == len(r[4]) and len(g[3]) in M.LONG_KMERS and g[2]["recalibrated"] and (g[3][:, 0] == -1).sum() > len(g[3]) // 12, n

    # the conditions on the fixture
    recs = [g[2] for g in got]
    count = {"align_returns_0": sum(g[0] == 0 for g in got),
             "not_recalibrated": sum(g[0] > 0 and not r["recalibrated"] for g, r in zip(got, recs)),
             "recalibrated": sum(r["recalibrated"] for r in recs),
             "m_states_195_to_205": sum(g[0] > 0 and 195 <= r["n_m_state"] <= 205 for g, r in zip(got, recs)),
             "first_entry_E": sum(first_entry_is_E(g[3], M.A.kmer_ranks(f[0]).tolist()) for f, g in zip(fixture, got)),
             "kmer_without_event": sum(g[0] > 0 and bool((g[3][:, 0] == -1).any()) for g in got)}
    for k, v in AT_LEAST.items():
        assert count[k] >= v, f"{k}: {count[k]}, at least {v} needed"
    ms = sorted(r["n_m_state"] for g, r in zip(got, recs) if g[0] > 0)
    assert any(x < 200 for x in ms if x >= 195) and any(x >= 200 for x in ms if x <= 205), "both sides of the 200-state rule"
    assert all(r["read_stat_flag"] in (0, 1, 2) for r in recs)
    by = {n: g[2] for n, g in zip(names, got_c)}
    for f in M.VAR_FACTORS:
        r = by[f"var_{f}"]
        assert r["recalibrated"] and (float(r["var"]) > 2.5) == (f > 2.5) and r["read_stat_flag"] == (1 if f > 2.5 else 0), (f, r)
    assert float(by["epb_5"]["events_per_base"]) == 5.0 and by["epb_5"]["read_stat_flag"] == 0 and by["epb_5"]["recalibrated"]
    assert float(by["epb_6"]["events_per_base"]) == 6.0 and by["epb_6"]["read_stat_flag"] == 4 and by["epb_6"]["recalibrated"]
    for n in M.M_COUNTS:
        r = by[f"m_{n}"]
        assert r["n_m_state"] == n and r["recalibrated"] == (n >= 200) and r["read_stat_flag"] == (0 if n >= 200 else 1), (n, r)

    enc = [M.encode_path(g[1]) for g in got]
    enc_c = [M.encode_path(cases[n][4]) for n in names]
    npz = os.path.join(HERE, "abea_calib_small.npz")
    G1.save_npz(npz, [("n_pairs", np.array([g[0] for g in got], np.int32)), ("path_len", np.array([len(g[1]) for g in got], np.int32)),
                      ("first", np.stack([e[0] for e in enc])), ("steps", np.concatenate([e[1] for e in enc])),
                      ("c_name", np.array(names)), ("c_seq", np.frombuffer(b"".join(cases[n][0] for n in names), np.uint8)),
                      ("c_seq_len", np.array([len(cases[n][0]) for n in names], np.int32)),
                      ("c_events", np.concatenate([cases[n][1] for n in names])), ("c_n_events", np.array([cases[n][1].size for n in names], np.int32)),
                      ("c_scale", np.array([cases[n][2] for n in names], np.float32)), ("c_shift", np.array([cases[n][3] for n in names], np.float32)),
                      ("c_path_len", np.array([len(cases[n][4]) for n in names], np.int32)),
                      ("c_first", np.stack([e[0] for e in enc_c])), ("c_steps", np.concatenate([e[1] for e in enc_c]))])
    doc = {"fixture": "abea_calib_small.npz", "fixture_sha256": hashlib.sha256(open(npz, "rb").read()).hexdigest(), "reads_of": "abea_small.npz",
           "case_seed": M.CASE_SEED, "var_cases_from_read": int(longest),
           "reference_build": "g++ -O2 -std=c++11 -ffp-contract=off, align.c alone",
           "reference_postalign_seconds": round(t_post + t_post_c, 5), "reference_recalibrate_seconds": round(t_recal + t_recal_c, 5),
           "reference_host": "build host CPU, one thread", "counts": {k: int(v) for k, v in count.items()},
           "reads": [M.record_of(g[2], g[3]) for g in got], "cases": {n: M.record_of(g[2], g[3]) for n, g in zip(names, got_c)},
           "long": {n: M.record_of(g[2], g[3]) for n, g in zip(long_reads, got_l)}}
    old = os.path.join(HERE, "abea_calib_expected.json")
    if "--keep-times" in sys.argv and os.path.exists(old):      # reproduce the committed file: its times
        was = json.load(open(old))
        doc["reference_postalign_seconds"], doc["reference_recalibrate_seconds"] = was["reference_postalign_seconds"], was["reference_recalibrate_seconds"]
    with open(old, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(got)} reads + {len(names)} cases; {count}; postalign {t_post + t_post_c:.5f} s, recalibrate_model {t_recal + t_recal_c:.5f} s; {os.path.getsize(npz)} bytes")


if __name__ == "__main__":
    main()
