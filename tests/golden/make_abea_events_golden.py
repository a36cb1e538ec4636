#!/usr/bin/env python3
"""Build machine only: writes tests/golden/abea_events_small.npz (ADC codes, range / digitisation / offset per read and the bases, from
tests/abea_events_model.py's seeded generator over the pore model of abea_small.npz) and tests/golden/abea_events_expected.json (what
the reference's getevents, abea/src/events.c:552-568, and estimate_scalings_using_mom, abea/src/align.c:49-97, return per read).

The reference's events.c and align.c are compiled on their own in a temporary directory outside the repository, with the stand-in
headers of make_abea_golden.py plus one typedef, -O2 -std=c++11 -ffp-contract=off, and a small harness of this script's own that
converts the codes to pA as f5c.c:1249-1253 does.  Nothing compiled and no reference text is kept.  The .npz is written with fixed
time stamps, so that the script reproduces the committed files byte for byte.

    python tests/golden/make_abea_events_golden.py [/root/reference/benchmarks] [--keep-times]

--keep-times: the reference's measured seconds are taken from the committed .json instead of this run's (they are the only thing
that differs from one run to the next)."""
import hashlib
import io
import json
import os
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import abea_events_model as M  # noqa: E402
import make_abea_golden as G0  # noqa: E402

SEED = 20250913
N_SMALL, N_LONG = 60, 2

HARNESS = r"""
#include "f5c.h"
#include <time.h>
event_table getevents(size_t nsample, float* rawptr);
scalings_t estimate_scalings_using_mom(char* sequence, int32_t sequence_len, model_t* pore_model, event_table et);
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
static double now() { struct timespec a; clock_gettime(CLOCK_MONOTONIC, &a); return a.tv_sec + 1e-9 * a.tv_nsec; }
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    static model_t model[4096];
    memset(model, 0, sizeof model);
    for (int i = 0; i < 4096; i++) { float v; rd(&v, 4, in); model[i].level_mean = v; }
    int32_t n_reads; rd(&n_reads, 4, in);
    double t_events = 0, t_scalings = 0;
    for (int r = 0; r < n_reads; r++) {
        int32_t n, len; float par[3];
        rd(&n, 4, in); rd(&len, 4, in); rd(par, 12, in);
        int16_t *codes = (int16_t *)malloc(2 * (size_t)n); rd(codes, 2 * (size_t)n, in);
        char *seq = (char *)malloc(len + 1); rd(seq, len, in); seq[len] = 0;
        float *raw = (float *)malloc(4 * (size_t)n);
        const float unit = par[0] / par[1];
        for (int i = 0; i < n; i++) raw[i] = ((float)codes[i] + par[2]) * unit;
        double t0 = now();
        event_table et = getevents((size_t)n, raw);
        double t1 = now();
        scalings_t sc = estimate_scalings_using_mom(seq, len, model, et);
        double t2 = now();
        t_events += t1 - t0; t_scalings += t2 - t1;
        int64_t ne = (int64_t)et.n;
        fwrite(&ne, 8, 1, out);
        for (int64_t i = 0; i < ne; i++) {
            int64_t st = (int64_t)et.event[i].start; float v[3] = {et.event[i].length, et.event[i].mean, et.event[i].stdv};
            fwrite(&st, 8, 1, out); fwrite(v, 4, 3, out);
        }
        float s2[2] = {sc.scale, sc.shift}; fwrite(s2, 4, 2, out);
        free(codes); free(seq); free(raw); free(et.event);
    }
    fwrite(&t_events, 8, 1, out); fwrite(&t_scalings, 8, 1, out);
    fclose(out);
    return 0;
}
"""


def make_fixture(level_mean):
    rng = np.random.default_rng(SEED)
    sizes = [int(rng.integers(1000, 4001)) for _ in range(N_SMALL)] + [30000] * N_LONG
    reads = [M.make_signal(rng, n, level_mean) for n in sizes]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def save_npz(path, arrays):
    """numpy's .npz layout (a zip of .npy members, deflated) with the time stamp of every member fixed"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def run_reference(ref, level_mean, reads):
    src = os.path.join(ref, "abea", "src")
    with tempfile.TemporaryDirectory(prefix="abea_events_golden_") as tmp:
        os.makedirs(os.path.join(tmp, "stub", "htslib"))
        sam_h = G0.STUB_SAM_H + "typedef struct htsFile samFile;\n"
        for name, text in (("htslib/sam.h", sam_h), ("htslib/faidx.h", ""), ("htslib/hts.h", ""), ("hdf5.h", "")):
            open(os.path.join(tmp, "stub", name), "w").write(text)
        open(os.path.join(tmp, "harness.cpp"), "w").write(HARNESS)
        flags = ["-O2", "-std=c++11", "-ffp-contract=off", "-DFAST5LITE_H", "-DNANOPOLISH_READ_DB_H", "-I" + os.path.join(tmp, "stub"), "-I" + src]
        exe = os.path.join(tmp, "harness")
        subprocess.check_call(["g++"] + flags + [os.path.join(tmp, "harness.cpp"), os.path.join(src, "events.c"), os.path.join(src, "align.c"), "-o", exe, "-lm"])
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.asarray(level_mean, "<f4").tobytes())
            f.write(struct.pack("<i", len(reads)))
            for codes, rg, dg, of, seq in reads:
                f.write(struct.pack("<iifff", codes.size, len(seq), float(rg), float(dg), float(of)) + codes.astype("<i2").tobytes() + seq)
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], stderr=subprocess.DEVNULL)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    out, at = [], 0
    rec = np.dtype([("start", "<i8"), ("length", "<f4"), ("mean", "<f4"), ("stdv", "<f4")])
    for _ in reads:
        (ne,) = struct.unpack_from("<q", raw, at); at += 8
        ev = np.frombuffer(raw, rec, ne, at); at += rec.itemsize * ne
        scale, shift = struct.unpack_from("<ff", raw, at); at += 8
        out.append((ev, scale, shift))
    t_events, t_scalings = struct.unpack_from("<dd", raw, at)
    return out, t_events, t_scalings


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ref = args[0] if args else "/root/reference/benchmarks"
    level_mean = np.load(os.path.join(HERE, "abea_small.npz"))["level_mean"]
    reads = make_fixture(level_mean)
    got, t_events, t_scalings = run_reference(ref, level_mean, reads)

    # the conditions on the fixture
    for (codes, _, _, _, seq), (ev, _, _) in zip(reads, got):
        assert codes.size >= 1000, "the reference's discarded trim step aborts or reads out of bounds on very short reads"
        assert ev.size >= 2, "a read without a peak: undefined in the reference"
        assert ev["start"][0] == 0 and np.all(np.diff(ev["start"]) > 0) and ev["start"][-1] < codes.size, "peaks must be strictly increasing"
        assert len(seq) >= M.K

    npz = os.path.join(HERE, "abea_events_small.npz")
    save_npz(npz, [("codes", np.concatenate([r[0] for r in reads])), ("n_samples", np.array([r[0].size for r in reads], np.int32)),
                   ("range", np.array([r[1] for r in reads], np.float32)), ("digitisation", np.array([r[2] for r in reads], np.float32)),
                   ("offset", np.array([r[3] for r in reads], np.float32)), ("seq", np.frombuffer(b"".join(r[4] for r in reads), np.uint8)),
                   ("seq_len", np.array([len(r[4]) for r in reads], np.int32))])
    doc = {"fixture": "abea_events_small.npz", "fixture_sha256": hashlib.sha256(open(npz, "rb").read()).hexdigest(), "seed": SEED,
           "model": "level_mean of abea_small.npz",
           "reference_build": "g++ -O2 -std=c++11 -ffp-contract=off, events.c and align.c alone",
           "reference_getevents_seconds": round(t_events, 4), "reference_scalings_seconds": round(t_scalings, 5),
           "reference_host": "build host CPU, one thread", "samples": int(sum(r[0].size for r in reads)), "events": int(sum(g[0].size for g in got)),
           "reads": [{"n_events": int(ev.size), "events": M.events_digest(ev), "scale": float(np.float32(sc)).hex(), "shift": float(np.float32(sh)).hex()}
                     for ev, sc, sh in got]}
    if "--keep-times" in sys.argv and os.path.exists(os.path.join(HERE, "abea_events_expected.json")):      # reproduce the committed file: its times
        old = json.load(open(os.path.join(HERE, "abea_events_expected.json")))
        doc["reference_getevents_seconds"], doc["reference_scalings_seconds"] = old["reference_getevents_seconds"], old["reference_scalings_seconds"]
    with open(os.path.join(HERE, "abea_events_expected.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(reads)} reads, {doc['samples']} samples, {doc['events']} events; getevents {t_events:.4f} s, scalings {t_scalings:.5f} s; {os.path.getsize(npz)} bytes")


if __name__ == "__main__":
    main()
