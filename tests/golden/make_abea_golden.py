#!/usr/bin/env python3
"""Build machine only: writes tests/golden/abea_small.npz (pore model, reads, events, scalings from tests/abea_model.py's seeded
generator) and tests/golden/abea_expected.json (what the reference's align(), abea/src/align.c:169-548, returns for every read).

The reference's align.c is compiled on its own, in a temporary directory outside the repository: empty stand-ins for the htslib /
HDF5 headers it never uses, -ffp-contract=off (the arithmetic this library is pinned to: the reference's -msse4.1 / -mavx2 builds
cannot fuse), and a small harness of this script's own that fills the pair buffer with -1 first, so that the path is recovered even
when align() returns 0 after a failed quality check.  Nothing compiled and no reference text is kept.

    python tests/golden/make_abea_golden.py [/root/reference/benchmarks]
"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import abea_model as M  # noqa: E402

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
int32_t align(AlignedPair* out_2, char* sequence, int32_t sequence_len, event_table events, model_t* models, scalings_t scaling, float sample_rate);
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    static model_t model[4096];
    memset(model, 0, sizeof model);
    for (int i = 0; i < 4096; i++) { float v[3]; rd(v, sizeof v, in); model[i].level_mean = v[0]; model[i].level_stdv = v[1]; model[i].level_log_stdv = v[2]; }
    int32_t n_reads; rd(&n_reads, 4, in);
    double seconds = 0;
    for (int r = 0; r < n_reads; r++) {
        int32_t len, ne; float sc[2];
        rd(&len, 4, in); rd(&ne, 4, in); rd(sc, 8, in);
        char *seq = (char *)malloc(len + 1); rd(seq, len, in); seq[len] = 0;
        float *ev = (float *)malloc(4 * (size_t)ne); rd(ev, 4 * (size_t)ne, in);
        event_table et; memset(&et, 0, sizeof et);
        et.n = ne; et.event = (event_t *)calloc(ne, sizeof(event_t));
        for (int i = 0; i < ne; i++) et.event[i].mean = ev[i];
        scalings_t s; memset(&s, 0, sizeof s); s.scale = sc[0]; s.shift = sc[1];
        AlignedPair *pairs = (AlignedPair *)malloc(sizeof(AlignedPair) * 2 * (size_t)ne);
        memset(pairs, 0xff, sizeof(AlignedPair) * 2 * (size_t)ne);
        struct timespec a, b; clock_gettime(CLOCK_MONOTONIC, &a);
        int32_t n_pairs = align(pairs, seq, len, et, model, s, 4000.0f);
        clock_gettime(CLOCK_MONOTONIC, &b);
        seconds += (b.tv_sec - a.tv_sec) + 1e-9 * (b.tv_nsec - a.tv_nsec);
        int32_t path_len = 0;
        while (path_len < 2 * ne && pairs[path_len].ref_pos != -1) path_len++;
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


def run_reference(ref, mean, stdv, lstd, reads):
    src = os.path.join(ref, "abea", "src")
    with tempfile.TemporaryDirectory(prefix="abea_golden_") as tmp:
        os.makedirs(os.path.join(tmp, "stub", "htslib"))
        for name, text in (("htslib/sam.h", STUB_SAM_H), ("htslib/faidx.h", ""), ("htslib/hts.h", ""), ("hdf5.h", "")):
            open(os.path.join(tmp, "stub", name), "w").write(text)
        open(os.path.join(tmp, "harness.cpp"), "w").write(HARNESS)
        flags = ["-O2", "-std=c++11", "-ffp-contract=off", "-DFAST5LITE_H", "-DNANOPOLISH_READ_DB_H", "-I" + os.path.join(tmp, "stub"), "-I" + src]
        exe = os.path.join(tmp, "harness")
        subprocess.check_call(["g++"] + flags + [os.path.join(tmp, "harness.cpp"), os.path.join(src, "align.c"), "-o", exe, "-lm"])
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.stack([mean, stdv, lstd], 1).astype("<f4").tobytes())
            f.write(struct.pack("<i", len(reads)))
            for seq, ev, sc, sh in reads:
                f.write(struct.pack("<iiff", len(seq), ev.size, float(sc), float(sh)) + seq + ev.astype("<f4").tobytes())
        t0 = time.time()
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], stderr=subprocess.DEVNULL)
        wall = time.time() - t0
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    out, at = [], 0
    for _ in reads:
        n_pairs, path_len = struct.unpack_from("<ii", raw, at); at += 8
        path = np.frombuffer(raw, "<i4", 2 * path_len, at).reshape(-1, 2); at += 8 * path_len
        out.append((n_pairs, path_len, path))
    (align_seconds,) = struct.unpack_from("<d", raw, at)
    return out, align_seconds, wall


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/benchmarks"
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
    doc = {"fixture": "abea_small.npz", "fixture_sha256": hashlib.sha256(open(npz, "rb").read()).hexdigest(), "seed": SEED,
           "reference_build": "g++ -O2 -std=c++11 -ffp-contract=off, align.c alone", "reference_align_seconds": round(align_seconds, 4),
           "reference_wall_seconds": round(wall, 4), "reference_host": "build host CPU, one thread", "band_cells_upper_bound": int(cells),
           "reads_passing": passed,
           "reads": [{"n_pairs": int(n), "path_len": int(pl), "pairs": M.pairs_digest(p)} for n, pl, p in got]}
    with open(os.path.join(HERE, "abea_expected.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(reads)} reads, {passed} pass, {len(failed)} fail; reference align() {align_seconds:.3f} s; {os.path.getsize(npz)} bytes")


if __name__ == "__main__":
    main()
