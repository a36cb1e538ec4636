#!/usr/bin/env python3
"""Build machine only: writes tests/golden/abea_realign_small.npz (per read of abea_small.npz a generated reference, position,
strand and CIGAR, from tests/abea_realign_model.py's seeded generator, and the full inputs of its constructed cases) and
tests/golden/abea_realign_expected.json (what the reference's realign_read, abea/src/eventalign.c:1942-2034, returns per read).

The reference's align.c and eventalign.c are compiled on their own in a temporary directory outside the repository, with
-O2 -std=c++11 -ffp-contract=off -DFAST5LITE_H -DNANOPOLISH_READ_DB_H, against the headers of the reference's own htslib archive
(unpacked there), a two-line stand-in for fast5_t / ReadDB and a small harness of this script's own.  The harness builds each
bam1_t itself (core.pos, core.flag, core.n_cigar, qname, CIGAR), stubs the seven htslib functions that eventalign.c's writers would
call, and runs align -> postalign -> recalibrate_model -> realign_read with summary_fp = NULL on the fixture reads, and
realign_read alone, on the map and scalings given, on the constructed cases.  It counts the calls of profile_hmm_align and their
rows through the one abs() of align_read_to_ref's loop (eventalign.c:1417), which a forced include turns into a counting function.
Nothing compiled and no reference text is kept.  The .npz is written with fixed time stamps, so that the script reproduces the
committed files byte for byte.

    python tests/golden/make_abea_realign_golden.py [/root/reference/benchmarks] [--keep-times]

--keep-times: the reference's measured seconds are taken from the committed .json instead of this run's."""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tarfile
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import abea_realign_model as M  # noqa: E402
import make_abea_events_golden as G1  # noqa: E402
from test_abea_calib_model import load_calib_fixture, model_of_fixture  # noqa: E402

# what the fixture held when it was made: the generator must not fall below it
AT_LEAST = {"realigned": 123, "skipped": 82, "reverse": 40, "with_I": 100, "with_D": 100, "with_S": 10, "with_EQ_X": 30, "with_N": 5,
            "break_short_ref": 1, "break_stop_event": 1, "from_same_m": 1, "from_prev_m": 1, "from_same_b": 1,
            "from_prev_b": 1, "from_prev_k": 1, "state_B": 1, "longest_k_run": 3}
# The third break of the loop, `num_output == 0` (eventalign.c:1530), no input can reach: the backtrack's first entry is (last row, last
# k-mer, MATCH) before any score is looked at, it is no K state, and its event is the stop event, at least 2 away from the start event
# (the break before it), so every call of profile_hmm_align is followed by at least one emitted entry.  The count is asserted to be 0.
FULL_READS = 3      # the shortest realigned reads, listed in full

PRE_H = r"""
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <cmath>
#include <cstdlib>
#include <string>
#include <map>
#include <vector>
#include <algorithm>
#include <fstream>
#include <iostream>
#include "error.h"
struct fast5_t; typedef struct fast5_t fast5_t;
class ReadDB;
extern long g_hmm_calls; extern int g_hmm_max_rows;
static inline int counted_abs(int x) { int a = x < 0 ? -x : x; if (a >= 2) { g_hmm_calls++; if (a + 1 > g_hmm_max_rows) g_hmm_max_rows = a + 1; } return a; }
#define abs(x) counted_abs(x)
"""

HARNESS = r"""
#include "f5c.h"
#include <time.h>
#undef abs
long g_hmm_calls = 0; int g_hmm_max_rows = 0;
int32_t align(AlignedPair* out_2, char* sequence, int32_t sequence_len, event_table events, model_t* models, scalings_t scaling, float sample_rate);
int32_t postalign(event_alignment_t* alignment, index_pair_t* base_to_event_map, double* events_per_base, char* sequence, int32_t n_kmers,
                  AlignedPair* event_alignment, int32_t n_events);
bool recalibrate_model(model_t* pore_model, event_table et, scalings_t* scallings, const event_alignment_t* alignment_output,
                       int32_t num_alignments, bool scale_var);
void realign_read(std::vector<event_alignment_t>* event_alignment_result, EventalignSummary *summary, FILE *summary_fp, char* ref,
                  const bam_hdr_t* hdr, const bam1_t* record, int32_t read_length, size_t read_idx, int region_start, int region_end,
                  event_table* events, model_t* model, index_pair_t* base_to_event_map, scalings_t scalings, double events_per_base, float sample_rate);
/* what eventalign.c's SAM writer and summary would call; never reached */
extern "C" {
uint8_t *bam_aux_get(const bam1_t *b, const char tag[2]) { abort(); }
int64_t bam_aux2i(const uint8_t *s) { abort(); }
int bam_aux_append(bam1_t *b, const char tag[2], char type, int len, const uint8_t *data) { abort(); }
bam1_t *bam_init1(void) { abort(); }
void bam_destroy1(bam1_t *b) { abort(); }
int sam_hdr_write(samFile *fp, const bam_hdr_t *h) { abort(); }
int sam_write1(samFile *fp, const bam_hdr_t *h, const bam1_t *b) { abort(); }
}
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
static double now() { struct timespec a; clock_gettime(CLOCK_MONOTONIC, &a); return a.tv_sec + 1e-9 * a.tv_nsec; }
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    static model_t model[4096];
    memset(model, 0, sizeof model);
    for (int i = 0; i < 4096; i++) { float v[3]; rd(v, sizeof v, in); model[i].level_mean = v[0]; model[i].level_stdv = v[1]; model[i].level_log_stdv = v[2]; }
    int32_t n_reads; rd(&n_reads, 4, in);
    double t_realign = 0;
    for (int r = 0; r < n_reads; r++) {
        int32_t len, ne, direct; float sc[4]; double epb;      /* direct: 0 = run the chain, 1 = map, var, log_var and events_per_base follow */
        rd(&len, 4, in); rd(&ne, 4, in); rd(&direct, 4, in); rd(sc, 16, in); rd(&epb, 8, in);
        char *seq = (char *)malloc(len + 1); rd(seq, len, in); seq[len] = 0;
        float *ev = (float *)malloc(4 * (size_t)ne); rd(ev, 4 * (size_t)ne, in);
        event_table et; memset(&et, 0, sizeof et);
        et.n = ne; et.event = (event_t *)calloc(ne, sizeof(event_t));
        for (int i = 0; i < ne; i++) et.event[i].mean = ev[i];
        scalings_t s; memset(&s, 0, sizeof s); s.scale = sc[0]; s.shift = sc[1]; s.var = 1.0f; s.log_var = 0.0f;
        const int32_t n_kmers = len - KMER_SIZE + 1;
        index_pair_t *map = (index_pair_t *)malloc(sizeof(index_pair_t) * n_kmers);
        for (int i = 0; i < n_kmers; i++) map[i].start = map[i].stop = -1;
        uint32_t flag = 0;
        if (direct) {
            s.var = sc[2]; s.log_var = sc[3];
            rd(map, sizeof(index_pair_t) * n_kmers, in);
        } else {
            const size_t room = 2 * (size_t)ne + (size_t)n_kmers + 2;
            AlignedPair *pairs = (AlignedPair *)malloc(sizeof(AlignedPair) * room);
            int32_t n_pairs = align(pairs, seq, len, et, model, s, 4000.0f);
            epb = 0;
            if (n_pairs > 0) {                           /* f5c.c:1438-1501 */
                event_alignment_t *al = (event_alignment_t *)malloc(sizeof(event_alignment_t) * room);
                int32_t n_alignment = postalign(al, map, &epb, seq, n_kmers, pairs, n_pairs);
                bool recalibrated = recalibrate_model(model, et, &s, al, n_alignment, 1);
                if (!recalibrated || s.var > 2.5) flag = FAILED_CALIBRATION;
                else if (epb > 5.0) flag = FAILED_QUALITY_CHK;
                free(al);
            } else flag = FAILED_ALIGNMENT;
            free(pairs);
        }
        int32_t ref_len, ref_pos, is_rev, n_cigar, region[2];
        rd(&ref_len, 4, in); rd(&ref_pos, 4, in); rd(&is_rev, 4, in); rd(&n_cigar, 4, in); rd(region, 8, in);
        char *ref = (char *)malloc(ref_len + 1); rd(ref, ref_len, in); ref[ref_len] = 0;
        bam1_t rec; memset(&rec, 0, sizeof rec);
        rec.core.pos = ref_pos; rec.core.flag = is_rev ? BAM_FREVERSE : 0; rec.core.n_cigar = n_cigar; rec.core.l_qname = 4;
        rec.l_data = rec.m_data = 4 + 4 * n_cigar;
        rec.data = (uint8_t *)calloc(rec.l_data + 4, 1);
        rec.data[0] = 'r';
        rd(rec.data + 4, 4 * (size_t)n_cigar, in);
        std::vector<event_alignment_t> result;
        g_hmm_calls = 0; g_hmm_max_rows = 0;
        if (flag == 0) {
            double t0 = now();
            realign_read(&result, NULL, NULL, ref, NULL, &rec, len, (size_t)r, region[0], region[1], &et, model, map, s, epb, 4000.0f);
            t_realign += now() - t0;
        }
        int32_t head[4] = {(int32_t)flag, (int32_t)result.size(), (int32_t)g_hmm_calls, g_hmm_max_rows};
        fwrite(head, 4, 4, out);
        for (size_t i = 0; i < result.size(); i++) {
            int32_t v[3] = {result[i].ref_position, result[i].event_idx, (int32_t)result[i].hmm_state};
            fwrite(v, 4, 3, out); fwrite(result[i].ref_kmer, 1, 6, out); fwrite(result[i].model_kmer, 1, 6, out);
        }
        free(seq); free(ev); free(et.event); free(map); free(ref); free(rec.data);
    }
    fwrite(&t_realign, 8, 1, out);
    fclose(out);
    return 0;
}
"""


def run_reference(ref_dir, model, reads):
    """reads: dicts with seq, events, scale, shift and either direct = (var, log_var, events_per_base, map) or None, and ref, ref_pos,
    is_rev, cigar, region -> per read (flag, entries (n, 3), ref k-mers, model k-mers, hmm calls, max rows), seconds of realign_read"""
    src = os.path.join(ref_dir, "abea", "src")
    with tempfile.TemporaryDirectory(prefix="abea_realign_golden_") as tmp:
        with tarfile.open(os.path.join(ref_dir, "abea", "htslib.tar.bz2")) as tf:
            tf.extractall(tmp, members=[m for m in tf.getmembers() if "/htslib/" in m.name and m.name.endswith(".h")])
        hts = [d for d in os.listdir(tmp) if d.startswith("htslib")][0]
        open(os.path.join(tmp, "pre.h"), "w").write(PRE_H)
        open(os.path.join(tmp, "harness.cpp"), "w").write(HARNESS)
        flags = ["-O2", "-std=c++11", "-ffp-contract=off", "-DFAST5LITE_H", "-DNANOPOLISH_READ_DB_H", "-include", os.path.join(tmp, "pre.h"),
                 "-I" + os.path.join(tmp, hts), "-I" + src, "-w"]
        exe = os.path.join(tmp, "harness")
        objs = []
        for name, path in (("harness", os.path.join(tmp, "harness.cpp")), ("align", os.path.join(src, "align.c")), ("eventalign", os.path.join(src, "eventalign.c"))):
            objs.append(os.path.join(tmp, name + ".o"))
            subprocess.check_call(["g++"] + flags + ["-x", "c++", "-c", path, "-o", objs[-1]])
        undefined = subprocess.run(["nm", "-u", objs[-1]], capture_output=True, text=True).stdout.split()
        assert "logf" in undefined and "log" not in undefined, "eventalign.c's run-time logarithms are logf's: the transitions that depend on events_per_base"
        subprocess.check_call(["g++"] + objs + ["-o", exe, "-lm"])
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.stack(model, 1).astype("<f4").tobytes())
            f.write(struct.pack("<i", len(reads)))
            for r in reads:
                d = r.get("direct")
                f.write(struct.pack("<iiiffffd", len(r["seq"]), r["events"].size, 1 if d else 0, float(r["scale"]), float(r["shift"]),
                                    float(d[0]) if d else 1.0, float(d[1]) if d else 0.0, float(d[2]) if d else 0.0))
                f.write(bytes(r["seq"]) + r["events"].astype("<f4").tobytes())
                if d:
                    f.write(np.ascontiguousarray(d[3], "<i4").tobytes())
                f.write(struct.pack("<iiiiii", len(r["ref"]), r["ref_pos"], r["is_rev"], len(r["cigar"]), *r["region"]))
                f.write(bytes(r["ref"]) + np.ascontiguousarray(r["cigar"], "<u4").tobytes())
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], stderr=subprocess.DEVNULL)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    out, at = [], 0
    rec_t = np.dtype([("v", "<i4", 3), ("ref_kmer", "S6"), ("model_kmer", "S6")])
    for _ in reads:
        flag, n, calls, max_rows = struct.unpack_from("<iiii", raw, at); at += 16
        e = np.frombuffer(raw, rec_t, n, at); at += rec_t.itemsize * n
        out.append((flag, e["v"].astype(np.int64), e["ref_kmer"].tolist(), e["model_kmer"].tolist(), calls, max_rows))
    (seconds,) = struct.unpack_from("<d", raw, at)
    return out, seconds


def ops_of(cigar):
    return {M.OPS[w & 15] for w in np.asarray(cigar).tolist()}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ref_dir = args[0] if args else "/root/reference/benchmarks"
    model, fixture, _, _ = load_calib_fixture()
    aln = M.fixture_alignments([r[0] for r in fixture])
    reads = [dict(seq=r[0], events=np.asarray(r[1], np.float32), scale=r[2], shift=r[3], ref=a[0], ref_pos=a[1], is_rev=a[2], cigar=a[3], region=(-1, -1))
             for r, a in zip(fixture, aln)]
    got, seconds = run_reference(ref_dir, model, reads)
    cases = M.make_cases(model)
    names = [n for n in cases if n not in M.DEVIATIONS]      # the reference cannot run the defined deviations: it indexes event -1 or asserts
    assert set(M.WINDOW_CASES) - set(M.WINDOW_NO_EVENT) <= set(names)      # ... but it runs every window case that finds an event
    flat = [n for n in names if n in M.FLAT_CASES]
    plain = [n for n in names if n not in M.FLAT_CASES]

    def as_read(c):
        cal = c["calib"]
        return dict(seq=b"A" * c["seq_len"], events=c["events"], scale=cal["scale"], shift=cal["shift"],
                    direct=(cal["var"], cal["log_var"], cal["events_per_base"], c["map"]), ref=c["ref"], ref_pos=c["ref_pos"], is_rev=c["is_rev"],
                    cigar=c["cigar"], region=c["region"])
    got_c, seconds_c = run_reference(ref_dir, model, [as_read(cases[n]) for n in plain])
    got_f, _ = run_reference(ref_dir, M.FLAT_MODEL, [as_read(cases[n]) for n in flat])
    by_case = dict(zip(plain + flat, got_c + got_f))

    # the model is the reference, entry for entry, on every read and case; what only a run from inside shows (breaks, movements, K
    # runs) is then counted on the model
    calib, _ = model_of_fixture()
    stats = M.new_stats()
    recs = []
    for i, (r, a, g) in enumerate(zip(fixture, aln, got)):
        rec, rmap = calib[i]
        assert int(rec["read_stat_flag"]) == g[0], f"read {i}: flag"
        e, mrec = M.realign(a[0], a[1], a[2], a[3], len(r[0]), r[1], rmap, rec, model, stats=stats)
        assert np.array_equal(e, g[1]), f"read {i}: the model's entries are not the reference's"
        assert (mrec["hmm_segments"], mrec["max_rows"]) == (g[4], g[5]), f"read {i}: {mrec} but the reference ran {g[4]} segments, {g[5]} rows at most"
        rows = M.eventalign_rows(a[0], a[1], a[2], e)
        assert [x[1].encode() for x in rows] == g[2] and [x[3].encode() for x in rows] == g[3], f"read {i}: k-mers"
        recs.append(M.record_of(e, mrec))
    case_recs = {}
    for n in names:
        c, g = cases[n], by_case[n]
        e, mrec = M.realign(c["ref"], c["ref_pos"], c["is_rev"], c["cigar"], c["seq_len"], c["events"], c["map"], c["calib"],
                            M.FLAT_MODEL if n in M.FLAT_CASES else model, c["region"])
        assert g[0] == 0 and np.array_equal(e, g[1]), f"{n}: the model's entries are not the reference's"
        assert (mrec["hmm_segments"], mrec["max_rows"]) == (g[4], g[5]), n
        case_recs[n] = dict(M.record_of(e, mrec), rows=[[int(v) for v in x] for x in e.tolist()] if len(e) <= 60 else None)

    run = [i for i, g in enumerate(got) if g[0] == 0]
    count = {"realigned": len(run), "skipped": len(got) - len(run), "reverse": sum(aln[i][2] for i in run),
             "with_I": sum("I" in ops_of(aln[i][3]) for i in run), "with_D": sum("D" in ops_of(aln[i][3]) for i in run),
             "with_S": sum("S" in ops_of(aln[i][3]) for i in run), "with_EQ_X": sum({"=", "X"} <= ops_of(aln[i][3]) for i in run),
             "with_N": sum("N" in ops_of(aln[i][3]) for i in run),
             "break_short_ref": stats["breaks"]["short_ref"], "break_stop_event": stats["breaks"]["stop_event"], "break_no_output": stats["breaks"]["no_output"],
             "from_same_m": stats["moves"][0], "from_prev_m": stats["moves"][1], "from_same_b": stats["moves"][2], "from_prev_b": stats["moves"][3],
             "from_prev_k": stats["moves"][4], "state_B": stats["b"], "longest_k_run": stats["k_run"]}
    print(count)
    for k, v in AT_LEAST.items():
        assert count[k] >= v, f"{k}: {count[k]}, at least {v} needed"
    assert count["break_no_output"] == 0
    assert count["realigned"] == 123 and count["skipped"] == 82 and count["reverse"] < count["realigned"]

    full = sorted(run, key=lambda i: len(got[i][1]) if len(got[i][1]) else 1 << 30)[:FULL_READS]
    npz = os.path.join(HERE, "abea_realign_small.npz")
    cn = list(cases)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs]) if xs else np.zeros(0, dt)
    G1.save_npz(npz, [("ref", cat([np.frombuffer(a[0], np.uint8) for a in aln], np.uint8)), ("ref_len", np.array([len(a[0]) for a in aln], np.int32)),
                      ("ref_pos", np.array([a[1] for a in aln], np.int32)), ("is_rev", np.array([a[2] for a in aln], np.uint8)),
                      ("cigar", cat([a[3] for a in aln], np.uint32)), ("n_cigar", np.array([len(a[3]) for a in aln], np.int32)),
                      ("c_name", np.array(cn)), ("c_ref", cat([np.frombuffer(cases[n]["ref"], np.uint8) for n in cn], np.uint8)),
                      ("c_ref_len", np.array([len(cases[n]["ref"]) for n in cn], np.int32)), ("c_ref_pos", np.array([cases[n]["ref_pos"] for n in cn], np.int32)),
                      ("c_is_rev", np.array([cases[n]["is_rev"] for n in cn], np.uint8)), ("c_cigar", cat([cases[n]["cigar"] for n in cn], np.uint32)),
                      ("c_n_cigar", np.array([len(cases[n]["cigar"]) for n in cn], np.int32)), ("c_seq_len", np.array([cases[n]["seq_len"] for n in cn], np.int32)),
                      ("c_events", cat([cases[n]["events"] for n in cn], np.float32)), ("c_n_events", np.array([cases[n]["events"].size for n in cn], np.int32)),
                      ("c_map", cat([cases[n]["map"] for n in cn], np.int32)), ("c_region", np.array([cases[n]["region"] for n in cn], np.int32)),
                      ("c_scalings", np.array([[cases[n]["calib"][k] for k in ("scale", "shift", "var", "log_var")] for n in cn], np.float32)),
                      ("c_epb", np.array([cases[n]["calib"]["events_per_base"] for n in cn], np.float64))])
    doc = {"fixture": "abea_realign_small.npz", "fixture_sha256": hashlib.sha256(open(npz, "rb").read()).hexdigest(), "reads_of": "abea_small.npz",
           "fixture_seed": M.FIXTURE_SEED, "case_seed": M.CASE_SEED,
           "reference_build": "g++ -O2 -std=c++11 -ffp-contract=off -DFAST5LITE_H -DNANOPOLISH_READ_DB_H, align.c and eventalign.c alone",
           "reference_realign_seconds": round(seconds, 5), "reference_host": "build host CPU, one thread",
           "counts": {k: int(v) for k, v in count.items()}, "reads": recs, "cases": case_recs,
           "full": {str(i): [[int(v[0]), rk.decode(), int(v[1]), mk.decode(), chr(int(v[2]))] for v, rk, mk in zip(got[i][1], got[i][2], got[i][3])] for i in full}}
    old = os.path.join(HERE, "abea_realign_expected.json")
    if "--keep-times" in sys.argv and os.path.exists(old):
        doc["reference_realign_seconds"] = json.load(open(old))["reference_realign_seconds"]
    with open(old, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(got)} reads + {len(names)} cases; realign_read {seconds:.5f} s (+ {seconds_c:.5f} s on the cases); {os.path.getsize(npz)} + {os.path.getsize(old)} bytes")


if __name__ == "__main__":
    main()
