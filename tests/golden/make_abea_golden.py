#!/usr/bin/env python3
"""Build machine only: writes tests/golden/abea_small.npz (pore model, reads, events, scalings from tests/abea_model.py's seeded
generator) and tests/golden/abea_expected.json (what the reference's align(), abea/src/align.c:169-548, returns for every read).

The reference's align.c is compiled on its own, in a temporary directory outside the repository: empty stand-ins for the htslib /
HDF5 headers it never uses, -ffp-contract=off (the arithmetic this library is pinned to: the reference's -msse4.1 / -mavx2 builds
cannot fuse), and a small harness of this script's own that fills the pair buffer with -1 first, so that the path is recovered even
when align() returns 0 after a failed quality check.  Nothing compiled and no reference text is kept.

A second product, tests/golden/abea_cases.npz and tests/golden/abea_cases_expected.json: the constructed reads of tests/abea_cases.py
(the named edge cases, the reads its seeded searches find on the thresholds of the quality checks and of the kernel's 64-lane loops,
400 reads of its pool) over the pore model of abea_small.npz, and what the reference returns for each.  Here the pair buffer has
2 * n_events + seq_len + 64 entries, the record is made with -DNDEBUG, and every read also runs alone through a build with the
reference's assertions on: a read that trips the reference's assumption about its caller's buffer (outIndex < n_events * 2) is
marked "needs_room", a read that trips any other assertion is listed under "undefined_in_reference" and stays a model-only case,
and a read on which the two builds differ fails this script.  The fields that align() computes but does not return are computed
again from the reference's path (tests/abea_path_checks.py) and recorded beside it.

    python tests/golden/make_abea_golden.py [/root/reference/benchmarks] [--new-times]

--new-times: record this run's measured seconds; without it they are taken from the committed abea_expected.json, so that the script
reproduces the committed files byte for byte (the seconds are the only thing that differs from one run to the next).
"""
import collections
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import abea_cases as C  # noqa: E402
import abea_model as M  # noqa: E402
import abea_path_checks as P  # noqa: E402

SEED = 20250607
N_SMALL, N_LONG = 200, 3

STUB_SAM_H = """#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <string>
#include <map>
#include "error.h"
struct htsFile; struct bam_hdr_t; struct hts_idx_t; struct hts_itr_t; struct bam1_t; struct faidx_t; struct fast5_t; class ReadDB;
typedef struct htsFile htsFile; typedef struct bam_hdr_t bam_hdr_t; typedef struct hts_idx_t hts_idx_t; typedef struct hts_itr_t hts_itr_t;
typedef struct bam1_t bam1_t; typedef struct faidx_t faidx_t; typedef struct fast5_t fast5_t;
"""

HARNESS = r"""
#include "f5c.h"
#include <time.h>
#ifndef PAIR_ROOM
#define PAIR_ROOM(ne, len) (2 * (size_t)(ne))
#endif
int32_t align(AlignedPair* out_2, char* sequence, int32_t sequence_len, event_table events, model_t* models, scalings_t scaling, float sample_rate);
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    static model_t model[4096];
    memset(model, 0, sizeof model);
    for (int i = 0; i < 4096; i++) { float v[3]; rd(v, sizeof v, in); model[i].level_mean = v[0]; model[i].level_stdv = v[1]; model[i].level_log_stdv = v[2]; }
    int32_t n_reads; rd(&n_reads, 4, in);
    double seconds = 0;
    const int only = argc > 3 ? atoi(argv[3]) : -1;      // one read alone (an assertion ends the process)
    for (int r = 0; r < n_reads; r++) {
        int32_t len, ne; float sc[2];
        rd(&len, 4, in); rd(&ne, 4, in); rd(sc, 8, in);
        char *seq = (char *)malloc(len + 1); rd(seq, len, in); seq[len] = 0;
        float *ev = (float *)malloc(4 * (size_t)ne); rd(ev, 4 * (size_t)ne, in);
        event_table et; memset(&et, 0, sizeof et);
        et.n = ne; et.event = (event_t *)calloc(ne, sizeof(event_t));
        for (int i = 0; i < ne; i++) et.event[i].mean = ev[i];
        scalings_t s; memset(&s, 0, sizeof s); s.scale = sc[0]; s.shift = sc[1];
        if (only >= 0 && r != only) { free(seq); free(ev); continue; }
        const size_t room = PAIR_ROOM(ne, len);
        AlignedPair *pairs = (AlignedPair *)malloc(sizeof(AlignedPair) * room);
        memset(pairs, 0xff, sizeof(AlignedPair) * room);
        struct timespec a, b; clock_gettime(CLOCK_MONOTONIC, &a);
        int32_t n_pairs = align(pairs, seq, len, et, model, s, 4000.0f);
        clock_gettime(CLOCK_MONOTONIC, &b);
        seconds += (b.tv_sec - a.tv_sec) + 1e-9 * (b.tv_nsec - a.tv_nsec);
        int32_t path_len = 0;
        while ((size_t)path_len < room && pairs[path_len].ref_pos != -1) path_len++;
        fwrite(&n_pairs, 4, 1, out); fwrite(&path_len, 4, 1, out);
        for (int i = 0; i < path_len; i++) { int32_t v[2] = {pairs[i].ref_pos, pairs[i].read_pos}; fwrite(v, 4, 2, out); }
        free(seq); free(ev); free(et.event); free(pairs);
    }
    fwrite(&seconds, 8, 1, out);
    fclose(out);
    return 0;
}
"""


def make_fixture():
    rng = np.random.default_rng(SEED)
    mean, stdv, lstd = M.make_model(rng)
    reads = [M.make_read(rng, int(rng.integers(100, 401)), mean, stdv) for _ in range(N_SMALL)]
    reads += [M.make_read(rng, int(rng.integers(2900, 3101)), mean, stdv) for _ in range(N_LONG)]
    # two reads that fail a quality check: a run of 55 k-mers without events (the band loses the path: emission), a shift off by 12
    reads.append(M.make_gap_read(rng, mean, stdv))
    seq, ev, sc, sh = M.make_read(rng, 250, mean, stdv)
    reads.append((seq, ev, sc, M.F(sh + M.F(12.0))))
    order = rng.permutation(len(reads))
    return mean, stdv, lstd, [reads[i] for i in order]


def save_fixture(path, mean, stdv, lstd, reads):
    np.savez_compressed(path, level_mean=mean, level_stdv=stdv, level_log_stdv=lstd,
                        seq=np.frombuffer(b"".join(r[0] for r in reads), np.uint8), seq_len=np.array([len(r[0]) for r in reads], np.int32),
                        events=np.concatenate([r[1] for r in reads]), n_events=np.array([r[1].size for r in reads], np.int32),
                        scale=np.array([r[2] for r in reads], np.float32), shift=np.array([r[3] for r in reads], np.float32))


CASES_ROOM = "-DPAIR_ROOM(ne,len)=(2*(size_t)(ne)+(size_t)(len)+64)"
ROOM_ASSERTION = "outIndex < (int)(n_events * 2)"      # the reference's assumption about its caller's buffer


def build_harness(tmp, ref, name, extra=()):
    """compiles the reference's align.c and the harness into tmp/name; extra: more compiler flags"""
    src = os.path.join(ref, "abea", "src")
    if not os.path.exists(os.path.join(tmp, "stub")):
        os.makedirs(os.path.join(tmp, "stub", "htslib"))
        for header, text in (("htslib/sam.h", STUB_SAM_H), ("htslib/faidx.h", ""), ("htslib/hts.h", ""), ("hdf5.h", "")):
            open(os.path.join(tmp, "stub", header), "w").write(text)
        open(os.path.join(tmp, "harness.cpp"), "w").write(HARNESS)
    flags = ["-O2", "-std=c++11", "-ffp-contract=off", "-DFAST5LITE_H", "-DNANOPOLISH_READ_DB_H", "-I" + os.path.join(tmp, "stub"), "-I" + src]
    exe = os.path.join(tmp, name)
    subprocess.check_call(["g++"] + flags + list(extra) + [os.path.join(tmp, "harness.cpp"), os.path.join(src, "align.c"), "-o", exe, "-lm"])
    return exe


def write_input(path, mean, stdv, lstd, reads):
    with open(path, "wb") as f:
        f.write(np.stack([mean, stdv, lstd], 1).astype("<f4").tobytes())
        f.write(struct.pack("<i", len(reads)))
        for seq, ev, sc, sh in reads:
            f.write(struct.pack("<iiff", len(seq), ev.size, float(sc), float(sh)) + seq + ev.astype("<f4").tobytes())


def parse_output(raw, n):
    out, at = [], 0
    for _ in range(n):
        n_pairs, path_len = struct.unpack_from("<ii", raw, at); at += 8
        path = np.frombuffer(raw, "<i4", 2 * path_len, at).reshape(-1, 2); at += 8 * path_len
        out.append((n_pairs, path_len, path))
    (align_seconds,) = struct.unpack_from("<d", raw, at)
    return out, align_seconds


def run_reference(ref, mean, stdv, lstd, reads):
    with tempfile.TemporaryDirectory(prefix="abea_golden_") as tmp:
        exe = build_harness(tmp, ref, "harness")
        write_input(os.path.join(tmp, "in.bin"), mean, stdv, lstd, reads)
        t0 = time.time()
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], stderr=subprocess.DEVNULL)
        wall = time.time() - t0
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    out, align_seconds = parse_output(raw, len(reads))
    return out, align_seconds, wall


def run_reference_on_cases(ref, mean, stdv, lstd, reads):
    """-> (what the -DNDEBUG build returns per read, per read None or the text of the assertion that ends the build with assertions on).
    A read that passes the assertions must give the same record in both builds."""
    with tempfile.TemporaryDirectory(prefix="abea_golden_") as tmp:
        fast = build_harness(tmp, ref, "harness_ndebug", [CASES_ROOM, "-DNDEBUG"])
        checked = build_harness(tmp, ref, "harness_checked", [CASES_ROOM])
        inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        write_input(inp, mean, stdv, lstd, reads)
        subprocess.check_call([fast, inp, outp], stderr=subprocess.DEVNULL)
        got, _ = parse_output(open(outp, "rb").read(), len(reads))
        asserts = []
        for i in range(len(reads)):
            p = subprocess.run([checked, inp, outp, str(i)], stderr=subprocess.PIPE)
            if p.returncode == 0:
                (one,), _ = parse_output(open(outp, "rb").read(), 1)
                assert one[:2] == got[i][:2] and np.array_equal(one[2], got[i][2]), f"read {i}: the two builds of the reference differ"
                asserts.append(None)
            else:
                m = re.search(r"Assertion `(.*)' failed", p.stderr.decode(errors="replace"))
                assert m, f"read {i}: the reference ended with status {p.returncode} and no assertion: {p.stderr[-300:]!r}"
                asserts.append(m.group(1))
    return got, asserts


def kept_times():
    """the measured seconds of the committed abea_expected.json, or None"""
    path = os.path.join(HERE, "abea_expected.json")
    if "--new-times" in sys.argv or not os.path.exists(path):
        return None
    old = json.load(open(path))
    return old["reference_align_seconds"], old["reference_wall_seconds"]


def make_small(ref):
    mean, stdv, lstd, reads = make_fixture()
    got, align_seconds, wall = run_reference(ref, mean, stdv, lstd, reads)

    # the conditions on the fixture
    passed = sum(1 for n_pairs, _, _ in got if n_pairs > 0)
    assert passed >= 0.9 * len(reads), f"only {passed} of {len(reads)} reads pass the reference's checks"
    for (seq, ev, _, _), (n_pairs, path_len, path) in zip(reads, got):
        n_kmers = len(seq) - M.K + 1
        assert n_kmers + 8 <= ev.size, "a read with (nearly) more k-mers than events: the reference's pair buffer assert"
        assert path_len >= 1 and path[-1, 0] == n_kmers - 1 and path[0, 0] == 0, "a read whose end scan found nothing (or a path that is not spanned)"
        assert n_pairs in (0, path_len)
    failed = [i for i, g in enumerate(got) if g[0] == 0]
    assert len(failed) >= 2, "the two constructed failures must fail in the reference"

    npz = os.path.join(HERE, "abea_small.npz")
    save_fixture(npz, mean, stdv, lstd, reads)
    cells = sum((len(r[0]) - M.K + 1 + r[1].size) * M.BW for r in reads)
    times = kept_times() or (round(align_seconds, 4), round(wall, 4))
    doc = {"fixture": "abea_small.npz", "fixture_sha256": hashlib.sha256(open(npz, "rb").read()).hexdigest(), "seed": SEED,
           "reference_build": "g++ -O2 -std=c++11 -ffp-contract=off, align.c alone", "reference_align_seconds": times[0],
           "reference_wall_seconds": times[1], "reference_host": "build host CPU, one thread", "band_cells_upper_bound": int(cells),
           "reads_passing": passed,
           "reads": [{"n_pairs": int(n), "path_len": int(pl), "pairs": M.pairs_digest(p)} for n, pl, p in got]}
    with open(os.path.join(HERE, "abea_expected.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(reads)} reads, {passed} pass, {len(failed)} fail; reference align() {align_seconds:.3f} s; {os.path.getsize(npz)} bytes")
    return (mean, stdv, lstd), reads


def make_cases(ref, model, fixture):
    import make_abea_events_golden as G1      # (it imports this module: only here)
    _, names, reads = C.named_cases(model, fixture)
    keep = [i for i, n in enumerate(names) if not n.startswith("long_")]      # the long reads are in abea_small.npz and its record
    named = {names[i]: reads[i] for i in keep}
    named.update(C.extra_cases(model))
    named.update(C.search_max_gap(model))
    named.update(C.search_path_lengths(model))
    room, tightest = C.search_room(model)
    named.update(room)
    bracket, bracket_avg = C.search_emission_bracket(model)
    named.update(bracket)
    not_spanned = C.search_not_spanned(model)
    if not_spanned is not None:
        named["not_spanned"] = not_spanned
    modes, pool = C.pool_sample(model)
    named.update({f"pool_{i:03d}": r for i, r in enumerate(pool)})
    names, reads = list(named), [(bytes(r[0]), np.asarray(r[1], np.float32), np.float32(r[2]), np.float32(r[3])) for r in named.values()]

    got, asserts = run_reference_on_cases(ref, *model, reads)
    want = [C.model_of(model, r) for r in reads]
    recs, undefined, by = [], {}, {}
    for name, r, (n_pairs, path_len, path), a, (mrec, mpath) in zip(names, reads, got, asserts, want):
        if a is not None and a != ROOM_ASSERTION:
            undefined[name] = a
            recs.append({"name": name, "undefined_in_reference": True})
            continue
        assert path_len >= 1 and n_pairs in (0, path_len), name
        chk = P.recompute(r[0], r[1], *model, r[2], r[3], path)
        by[name] = (r, n_pairs, path_len, path, chk)
        rec = {"name": name, "n_pairs": int(n_pairs), "path_len": int(path_len), "pairs": M.pairs_digest(path), "end_event": chk["end_event"],
               "max_gap": chk["max_gap"], "flags": chk["flags"], "avg_log_emission": float(chk["avg_log_emission"]).hex()}
        if len(chk["admissible"]) > 1:
            rec["max_gap_and_flags_admissible"] = [list(x) for x in chk["admissible"]]
        if a == ROOM_ASSERTION:
            rec["needs_room"] = True
        recs.append(rec)
        if name == "no_end_nan_events":
            assert mrec["flags"] == M.NO_END
            continue
        # the one thing the reference shows of its checks: no pairs when one of them fails
        assert any((n_pairs == 0) == bool(f) for _, f in chk["admissible"]), f"{name}: the reference returns {n_pairs} pairs, the recomputed flags are {chk['flags']}"
        assert P.agrees(mrec, chk), f"{name}: the model's record {mrec} and the recomputation from the reference's path {chk} differ"

    # the conditions on the cases, on the reference's output where it shows them and on the recomputation from its path where not
    ref_of = lambda name: by[name][1:4]
    chk_of = lambda name: by[name][4]
    assert ref_of("max_gap_50")[0] == ref_of("max_gap_50")[1] > 0 and chk_of("max_gap_50")["admissible"] == [(50, 0)]
    assert ref_of("max_gap_51")[0] == 0 and chk_of("max_gap_51")["admissible"] == [(51, M.GAP)]
    for n in C.PATH_LENGTHS:
        assert ref_of(f"path_len_{n}")[:2] == (n, n), n
    slack = lambda name: len(by[name][0][0]) - M.K + 1 + by[name][0][1].size - by[name][2]
    assert slack("room_one_short") == 1 and slack("room_tightest") == tightest
    above, below = chk_of("emission_above"), chk_of("emission_below")
    assert ref_of("emission_above")[0] > 0 and ref_of("emission_below")[0] == 0
    assert (above["avg_log_emission"], below["avg_log_emission"]) == bracket_avg and above["avg_log_emission"] >= -5.0 > below["avg_log_emission"]
    assert above["flags"] == 0 and below["flags"] == M.LOW_EMISSION
    a, b = by["emission_above"][0], by["emission_below"][0]
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.nextafter(a[3], np.float32(np.inf)) == b[3]
    pool_names = [n for n in names if n.startswith("pool_")]
    assert len(pool_names) == C.POOL_READS and not any(n in undefined for n in pool_names)
    few_events = sum(1 for n in pool_names if by[n][0][1].size < len(by[n][0][0]) - M.K + 1)
    flags = collections.Counter(chk_of(n)["flags"] for n in pool_names)
    assert few_events >= 50 and sum(1 for n in pool_names if ref_of(n)[0] > 0) == flags[0] >= 10, (few_events, flags)
    assert flags[M.LOW_EMISSION] >= 10 and flags[M.LOW_EMISSION | M.GAP] >= 10, flags

    npz = os.path.join(HERE, "abea_cases.npz")
    G1.save_npz(npz, [("seq", np.frombuffer(b"".join(r[0] for r in reads), np.uint8)), ("seq_len", np.array([len(r[0]) for r in reads], np.int32)),
                      ("events", np.concatenate([r[1] for r in reads])), ("n_events", np.array([r[1].size for r in reads], np.int32)),
                      ("scale", np.array([r[2] for r in reads], np.float32)), ("shift", np.array([r[3] for r in reads], np.float32))])
    assert os.path.getsize(npz) < 400_000
    doc = {"fixture": "abea_cases.npz", "fixture_sha256": hashlib.sha256(open(npz, "rb").read()).hexdigest(), "model": "level_mean, level_stdv, level_log_stdv of abea_small.npz",
           "seeds": {"named": C.NAMED_SEED, "search": C.SEARCH_SEED, "pool": C.POOL_SEED},
           "reference_build": "g++ -O2 -std=c++11 -ffp-contract=off -DNDEBUG, align.c alone, a pair buffer of 2 * n_events + seq_len + 64; every read again alone without -DNDEBUG",
           "recomputed": "end_event, max_gap, flags, avg_log_emission: tests/abea_path_checks.py from the reference's path",
           "room_assertion": ROOM_ASSERTION, "undefined_in_reference": undefined,
           "deviation": {"name": "no_end_nan_events", "library": "flags NO_END, no pairs, every other field 0 but fills",
                         "reference": "backtracks from event 0 whatever its cell holds: the record below"},
           "not_spanned": "not_spanned" if not_spanned is not None else f"none in {C.NOT_SPANNED_CANDIDATES} candidates",
           "emission_bracket": {"above": float(bracket_avg[0]).hex(), "below": float(bracket_avg[1]).hex(),
                                "shift_above": float(a[3]).hex(), "shift_below": float(b[3]).hex()},
           "room_tightest": int(tightest),
           "pool": {"reads": len(pool_names), "modes": dict(collections.Counter(modes)), "fewer_events_than_kmers": few_events,
                    "flags": {str(k): v for k, v in sorted(flags.items())}},
           "reads": recs}
    with open(os.path.join(HERE, "abea_cases_expected.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(reads)} cases, {sum(1 for r in recs if r.get('needs_room'))} need room, {len(undefined)} undefined in the reference, "
          f"not_spanned: {doc['not_spanned']}; pool flags {dict(flags)}; {os.path.getsize(npz)} bytes")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ref = args[0] if args else "/root/reference/benchmarks"
    model, fixture = make_small(ref)
    make_cases(ref, model, fixture)


if __name__ == "__main__":
    main()


