#!/usr/bin/env python3
"""Build machine only: writes tests/golden/abea_meth_small.npz (the seeded CpG model, the logsum table as the reference's
p7_FLogsumInit fills it, and the full inputs of tests/abea_meth_model.py's constructed cases) and tests/golden/abea_meth_expected.json
(what the reference's calculate_methylation_for_read, abea/src/meth.c:501-658, returns per read).

The fixture is the reads of abea_small.npz with the alignments of abea_realign_small.npz, chained through the model's align ->
calibrate as the realign golden is (whose script asserts that the model's calibration is the reference's); reads whose CIGAR holds
an N operation are left out (the reference exits on them, meth.c:54-58).

The reference's meth.c and hmm.c are compiled on their own in a temporary directory outside the repository, with
-O2 -std=c++11 -ffp-contract=off -DFAST5LITE_H -DNANOPOLISH_READ_DB_H, against the headers of the reference's own htslib archive
(unpacked there), a two-line stand-in for fast5_t / ReadDB and a small harness of this script's own.  The harness builds each
bam1_t itself, defines flogsum_lookup and fills it by calling p7_FLogsumInit (abea/src/logsum.h:35-48), calls
calculate_methylation_for_read on the map and scalings given, and prints the sites of a read with one fprintf of its own in the
column order and precision of abea/src/f5c.c:1746-1753.  hmm.o's undefined symbols say which logarithms are left to run time (logf: the two transitions that depend
on events_per_base; everything else is folded by the compiler).  Nothing compiled and no reference text is kept.  The .npz is written
with fixed time stamps, so that the script reproduces the committed files byte for byte.

    python tests/golden/make_abea_meth_golden.py [/root/reference/benchmarks] [--keep-times]"""
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
import abea_meth_model as M  # noqa: E402
import make_abea_events_golden as G1  # noqa: E402
from test_abea_realign_model import load_realign_fixture  # noqa: E402

# what the fixture must hold, so that it cannot go hollow
AT_LEAST = {"scored_reads": 100, "sites": 1000, "reverse_reads_with_sites": 30, "skipped_start": 20, "skipped_unbounded": 20, "skipped_short": 20,
            "groups_of_3_or_more": 1, "dominated_folds_flat": 1}
FULL_READS = 3      # the scored reads with the fewest sites, their printed lines kept

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
"""

HARNESS = r"""
#include "f5c.h"
#include "f5cmisc.h"
#include "logsum.h"
#include <time.h>
float flogsum_lookup[p7_LOGSUM_TBL];
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
static double now() { struct timespec a; clock_gettime(CLOCK_MONOTONIC, &a); return a.tv_sec + 1e-9 * a.tv_nsec; }
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb"), *txt = fopen(argv[3], "w");
    p7_FLogsumInit();
    fwrite(flogsum_lookup, 4, p7_LOGSUM_TBL, out);
    static model_t model[15625];
    memset(model, 0, sizeof model);
    for (int i = 0; i < 15625; i++) { float v[3]; rd(v, sizeof v, in); model[i].level_mean = v[0]; model[i].level_stdv = v[1]; model[i].level_log_stdv = v[2]; }
    int32_t n_reads; rd(&n_reads, 4, in);
    double seconds = 0;
    for (int r = 0; r < n_reads; r++) {
        int32_t len, ne; float sc[4]; double epb;
        rd(&len, 4, in); rd(&ne, 4, in); rd(sc, 16, in); rd(&epb, 8, in);
        float *ev = (float *)malloc(4 * (size_t)ne); rd(ev, 4 * (size_t)ne, in);
        event_t *event = (event_t *)calloc(ne, sizeof(event_t));
        for (int i = 0; i < ne; i++) event[i].mean = ev[i];
        scalings_t s; memset(&s, 0, sizeof s); s.scale = sc[0]; s.shift = sc[1]; s.var = sc[2]; s.log_var = sc[3];
        const int32_t n_kmers = len - KMER_SIZE + 1;
        index_pair_t *map = (index_pair_t *)malloc(sizeof(index_pair_t) * n_kmers);
        rd(map, sizeof(index_pair_t) * n_kmers, in);
        int32_t ref_len, ref_pos, is_rev, n_cigar;
        rd(&ref_len, 4, in); rd(&ref_pos, 4, in); rd(&is_rev, 4, in); rd(&n_cigar, 4, in);
        char *ref = (char *)malloc(ref_len + 1); rd(ref, ref_len, in); ref[ref_len] = 0;
        bam1_t rec; memset(&rec, 0, sizeof rec);
        rec.core.pos = ref_pos; rec.core.flag = is_rev ? BAM_FREVERSE : 0; rec.core.n_cigar = n_cigar; rec.core.l_qname = 4;
        rec.l_data = rec.m_data = 4 + 4 * n_cigar;
        rec.data = (uint8_t *)calloc(rec.l_data + 4, 1);
        rec.data[0] = 'r';
        rd(rec.data + 4, 4 * (size_t)n_cigar, in);
        std::map<int, ScoredSite> sites;
        double t0 = now();
        calculate_methylation_for_read(&sites, ref, &rec, len, event, map, s, model, epb);
        seconds += now() - t0;
        int32_t n = (int32_t)sites.size();
        fwrite(&n, 4, 1, out);
        for (const auto &kv : sites) {                   /* the map's order: ascending start_position */
            const ScoredSite &site = kv.second;
            const int32_t v[4] = {site.start_position, site.end_position, site.n_cpg, site.strands_scored};
            const double u = site.ll_unmethylated[0], m = site.ll_methylated[0];
            const float f[2] = {(float)u, (float)m};
            if ((double)f[0] != u || (double)f[1] != m) { fprintf(stderr, "a score that is no float\n"); exit(3); }
            fwrite(v, 4, 4, out); fwrite(f, 4, 2, out);
            /* one line per site in the column order and precision of output version 1 (abea/src/f5c.c:1746-1753) */
            fprintf(txt, "contig\t%d\t%d\tread\t%.2lf\t%.2lf\t%.2lf\t%d\t%d\t%s\n", v[0], v[1], m - u, m, u, v[3], v[2], site.sequence.c_str());
        }
        fprintf(txt, "#\n");
        free(ev); free(event); free(map); free(ref); free(rec.data);
    }
    fwrite(&seconds, 8, 1, out);
    fclose(out); fclose(txt);
    return 0;
}
"""

BUILD = "g++ -O2 -std=c++11 -ffp-contract=off -DFAST5LITE_H -DNANOPOLISH_READ_DB_H, meth.c and hmm.c alone"


def run_reference(ref_dir, cpg, reads):
    """reads: the dicts of a constructed case -> (logsum table, per read (sites (n, 4) int, scores (n, 2) float32, printed lines), seconds)"""
    src = os.path.join(ref_dir, "abea", "src")
    with tempfile.TemporaryDirectory(prefix="abea_meth_golden_") as tmp:
        with tarfile.open(os.path.join(ref_dir, "abea", "htslib.tar.bz2")) as tf:
            tf.extractall(tmp, members=[m for m in tf.getmembers() if "/htslib/" in m.name and m.name.endswith(".h")])
        hts = [d for d in os.listdir(tmp) if d.startswith("htslib")][0]
        open(os.path.join(tmp, "pre.h"), "w").write(PRE_H)
        open(os.path.join(tmp, "harness.cpp"), "w").write(HARNESS)
        flags = ["-O2", "-std=c++11", "-ffp-contract=off", "-DFAST5LITE_H", "-DNANOPOLISH_READ_DB_H", "-include", os.path.join(tmp, "pre.h"),
                 "-I" + os.path.join(tmp, hts), "-I" + src, "-w"]
        exe = os.path.join(tmp, "harness")
        objs = []
        for name, path in (("harness", os.path.join(tmp, "harness.cpp")), ("meth", os.path.join(src, "meth.c")), ("hmm", os.path.join(src, "hmm.c"))):
            objs.append(os.path.join(tmp, name + ".o"))
            subprocess.check_call(["g++"] + flags + ["-x", "c++", "-c", path, "-o", objs[-1]])
        undefined = subprocess.run(["nm", "-u", objs[-1]], capture_output=True, text=True).stdout.split()
        assert "logf" in undefined and "log" not in undefined and "exp" not in undefined, \
            "hmm.c's run-time logarithms are logf's (the transitions that depend on events_per_base); the flanks' are folded"
        subprocess.check_call(["g++"] + objs + ["-o", exe, "-lm"])
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.stack(cpg, 1).astype("<f4").tobytes())
            f.write(struct.pack("<i", len(reads)))
            for r in reads:
                cal = r["calib"]
                f.write(struct.pack("<iiffffd", r["seq_len"], r["events"].size, float(cal["scale"]), float(cal["shift"]), float(cal["var"]), float(cal["log_var"]),
                                    float(cal["events_per_base"])))
                f.write(np.asarray(r["events"]).astype("<f4").tobytes())
                f.write(np.ascontiguousarray(np.asarray(r["map"]).view(np.int32).reshape(-1, 2), "<i4").tobytes())
                f.write(struct.pack("<iiii", len(r["ref"]), r["ref_pos"], r["is_rev"], len(r["cigar"])))
                f.write(bytes(r["ref"]) + np.ascontiguousarray(r["cigar"], "<u4").tobytes())
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), os.path.join(tmp, "out.txt")], stderr=subprocess.DEVNULL)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
        text = open(os.path.join(tmp, "out.txt")).read().split("#\n")
    table = np.frombuffer(raw, "<f4", M.LOGSUM_TBL, 0).copy()
    out, at = [], 4 * M.LOGSUM_TBL
    rec_t = np.dtype([("v", "<i4", 4), ("f", "<f4", 2)])
    for i, _ in enumerate(reads):
        (n,) = struct.unpack_from("<i", raw, at); at += 4
        e = np.frombuffer(raw, rec_t, n, at); at += rec_t.itemsize * n
        out.append((e["v"].astype(np.int64), e["f"].copy(), text[i].splitlines()))
    (seconds,) = struct.unpack_from("<d", raw, at)
    return table, out, seconds


def same_as_reference(name, c, sites, rec, got):
    v, f, lines = got
    assert len(sites) == len(v) == rec["n_sites"], f"{name}: {len(sites)} sites, the reference has {len(v)}"
    for s, gv, gf in zip(sites, v.tolist(), f):
        assert [s["start_position"], s["end_position"], s["n_cpg"], 1] == gv, f"{name}: {s} but the reference has {gv}"
        assert np.array([s["ll_unmethylated"], s["ll_methylated"]], np.float32).tobytes() == gf.tobytes(), f"{name}: {s} but the reference scores {gf}"
    assert M.methylation_rows("contig", "read", c["ref"], c["ref_pos"], sites) == lines, f"{name}: the printed lines"
    assert [s["start_position"] for s in sites] == sorted(s["start_position"] for s in sites)


def run_model(c, cpg):
    return M.call_methylation(c["ref"], c["ref_pos"], c["is_rev"], c["cigar"], c["seq_len"], c["events"], c["map"], c["calib"], cpg)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ref_dir = args[0] if args else "/root/reference/benchmarks"
    model, fixture, _, _ = load_realign_fixture()
    cpg = M.make_cpg_model(model)
    keep = [i for i, r in enumerate(fixture) if M.aligned_pairs(r["cigar"], r["ref_pos"]) is not None]
    run = [i for i in keep if int(fixture[i]["calib"]["read_stat_flag"]) == 0]
    table, got, seconds = run_reference(ref_dir, cpg, [fixture[i] for i in run])
    assert table.tobytes() == M.TABLE.tobytes(), "the logsum table"
    cases = M.make_cases(model)
    names = [n for n in cases if n not in M.DEVIATIONS and int(cases[n]["calib"]["read_stat_flag"]) == 0]
    assert (set(M.WINDOW_CASES) | set(M.STEP_CASES)) - set(M.WINDOW_NO_EVENT) <= set(names)      # the window cases that find an event, every step case
    plain = [n for n in names if n not in M.FLAT_CASES]; flat = [n for n in names if n in M.FLAT_CASES]
    _, got_c, _ = run_reference(ref_dir, cpg, [cases[n] for n in plain])
    _, got_f, _ = run_reference(ref_dir, M.FLAT_CPG, [cases[n] for n in flat])
    by_case = dict(zip(plain + flat, got_c + got_f))

    # the model is the reference, site for site and bit for bit, on every read and case
    recs, by_read = {}, dict(zip(run, got))
    count = dict.fromkeys(AT_LEAST, 0)
    for i in keep:
        sites, rec = run_model(fixture[i], cpg)
        if i in by_read:
            same_as_reference(f"read {i}", fixture[i], sites, rec, by_read[i])
            count["scored_reads"] += bool(sites); count["sites"] += len(sites)
            count["reverse_reads_with_sites"] += bool(sites) and fixture[i]["is_rev"]
            for k in ("skipped_start", "skipped_unbounded", "skipped_short"):
                count[k] += rec[k]
            count["groups_of_3_or_more"] += sum(s["n_cpg"] >= 3 for s in sites)
            assert rec["flags"] == 0, f"read {i}: the reference cannot have run this"
        else:
            assert rec["flags"] == M.SKIPPED and not sites
        recs[str(i)] = dict({k: int(rec[k]) for k in M.COUNTERS}, sites=M.site_bits(sites))
    case_recs = {}
    for n, c in cases.items():
        M.FOLDS["dominated"] = 0
        sites, rec = run_model(c, M.FLAT_CPG if n in M.FLAT_CASES else cpg)
        if n in by_case:
            same_as_reference(n, c, sites, rec, by_case[n])
        if n in M.FLAT_CASES:
            count["dominated_folds_flat"] += M.FOLDS["dominated"]
        case_recs[n] = dict({k: int(rec[k]) for k in M.COUNTERS}, sites=M.site_bits(sites), by_reference=n in by_case)
    print(count)
    for k, v in AT_LEAST.items():
        assert count[k] >= v, f"{k}: {count[k]}, at least {v} needed"

    full = sorted([i for i in run if len(by_read[i][0])], key=lambda i: len(by_read[i][0]))[:FULL_READS]
    npz = os.path.join(HERE, "abea_meth_small.npz")
    cn = list(cases)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs]) if xs else np.zeros(0, dt)
    G1.save_npz(npz, [("cpg_mean", cpg[0]), ("cpg_stdv", cpg[1]), ("cpg_log_stdv", cpg[2]), ("logsum", table),
                      ("c_name", np.array(cn)), ("c_ref", cat([np.frombuffer(cases[n]["ref"], np.uint8) for n in cn], np.uint8)),
                      ("c_ref_len", np.array([len(cases[n]["ref"]) for n in cn], np.int32)), ("c_ref_pos", np.array([cases[n]["ref_pos"] for n in cn], np.int32)),
                      ("c_is_rev", np.array([cases[n]["is_rev"] for n in cn], np.uint8)), ("c_cigar", cat([cases[n]["cigar"] for n in cn], np.uint32)),
                      ("c_n_cigar", np.array([len(cases[n]["cigar"]) for n in cn], np.int32)), ("c_seq_len", np.array([cases[n]["seq_len"] for n in cn], np.int32)),
                      ("c_events", cat([cases[n]["events"] for n in cn], np.float32)), ("c_n_events", np.array([cases[n]["events"].size for n in cn], np.int32)),
                      ("c_map", cat([cases[n]["map"] for n in cn], np.int32)),
                      ("c_scalings", np.array([[cases[n]["calib"][k] for k in ("scale", "shift", "var", "log_var")] for n in cn], np.float32)),
                      ("c_epb", np.array([cases[n]["calib"]["events_per_base"] for n in cn], np.float64)),
                      ("c_flag", np.array([cases[n]["calib"]["read_stat_flag"] for n in cn], np.uint32))])
    doc = {"fixture": "abea_meth_small.npz", "fixture_sha256": hashlib.sha256(open(npz, "rb").read()).hexdigest(), "reads_of": "abea_small.npz",
           "alignments_of": "abea_realign_small.npz", "cpg_seed": M.CPG_SEED, "case_seed": M.CASE_SEED, "blocks_per_lane": M.BLOCKS_PER_LANE, "one_block_kmers": M.ONE_BLOCK_KMERS,
           "reference_build": BUILD, "reference_meth_seconds": round(seconds, 5), "reference_host": "build host CPU, one thread",
           "counts": {k: int(v) for k, v in count.items()}, "reads": recs, "cases": case_recs,
           "lines": {str(i): by_read[i][2] for i in full}}
    old = os.path.join(HERE, "abea_meth_expected.json")
    if "--keep-times" in sys.argv and os.path.exists(old):
        doc["reference_meth_seconds"] = json.load(open(old))["reference_meth_seconds"]
    with open(old, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(run)} reads + {len(by_case)} cases by the reference; calculate_methylation_for_read {seconds:.5f} s; {os.path.getsize(npz)} + {os.path.getsize(old)} bytes")


if __name__ == "__main__":
    main()
