#!/usr/bin/env python3
"""Build machine only: writes tests/golden/abea_events_small.npz (ADC codes, range / digitisation / offset per read and the bases, from
tests/abea_events_model.py's seeded generator over the pore model of abea_small.npz) and tests/golden/abea_events_expected.json (what
the reference's getevents, abea/src/events.c:552-568, and estimate_scalings_using_mom, abea/src/align.c:49-97, return per read).

The reference's events.c and align.c are compiled on their own in a temporary directory outside the repository, with the stand-in
headers of make_abea_golden.py plus one typedef, -O2 -std=c++11 -ffp-contract=off, and a small harness of this script's own that
converts the codes to pA as f5c.c:1249-1253 does.  Nothing compiled and no reference text is kept.  The .npz is written with fixed
time stamps, so that the script reproduces the committed files byte for byte.

A second product, tests/golden/abea_events_cases.npz and tests/golden/abea_events_cases_expected.json: the constructed reads of
tests/abea_events_cases.py (float samples, as the library takes them, and the scaling edge cases under three pore models) and what
the reference returns for each.  A second harness takes float samples, or event means for a scalings-only read, and reads the pore
model per group of reads; every read runs alone through the build with assertions on, and a read the reference refuses is listed
under "undefined_in_reference" with the assertion's text and stays a model-only case.

    python tests/golden/make_abea_events_golden.py [/root/reference/benchmarks] [--keep-times]

--keep-times: the reference's measured seconds are taken from the committed .json instead of this run's (they are the only thing
that differs from one run to the next)."""
import hashlib
import io
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import abea_events_cases as C  # noqa: E402
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


HARNESS_CASES = r"""
#include "f5c.h"
event_table getevents(size_t nsample, float* rawptr);
scalings_t estimate_scalings_using_mom(char* sequence, int32_t sequence_len, model_t* pore_model, event_table et);
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
// groups of reads, each with its pore model; a read is float samples (kind 0: events, then scalings) or event means (kind 1: scalings);
// argv[3]: the one read to run (an assertion of the reference ends the process)
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    const int only = atoi(argv[3]);
    static model_t model[4096];
    int32_t n_groups; rd(&n_groups, 4, in);
    int at = 0;
    for (int g = 0; g < n_groups; g++) {
        memset(model, 0, sizeof model);
        for (int i = 0; i < 4096; i++) { float v; rd(&v, 4, in); model[i].level_mean = v; }
        int32_t n_reads; rd(&n_reads, 4, in);
        for (int r = 0; r < n_reads; r++, at++) {
            int32_t kind, n, len; float par[3];
            rd(&kind, 4, in); rd(&n, 4, in); rd(&len, 4, in); rd(par, 12, in);
            float *raw = (float *)malloc(4 * (size_t)n); rd(raw, 4 * (size_t)n, in);
            char *seq = (char *)malloc(len + 1); rd(seq, len, in); seq[len] = 0;
            if (at == only) {
                event_table et; memset(&et, 0, sizeof et);
                if (kind == 0) {
                    const float unit = par[0] / par[1];
                    for (int i = 0; i < n; i++) raw[i] = (raw[i] + par[2]) * unit;
                    et = getevents((size_t)n, raw);
                } else {
                    et.n = n; et.event = (event_t *)calloc(n, sizeof(event_t));
                    for (int i = 0; i < n; i++) et.event[i].mean = raw[i];
                }
                scalings_t sc = estimate_scalings_using_mom(seq, len, model, et);
                int64_t ne = (int64_t)et.n;
                fwrite(&ne, 8, 1, out);
                for (int64_t i = 0; i < ne; i++) {
                    int64_t st = (int64_t)et.event[i].start; float v[3] = {et.event[i].length, et.event[i].mean, et.event[i].stdv};
                    fwrite(&st, 8, 1, out); fwrite(v, 4, 3, out);
                }
                float s2[2] = {sc.scale, sc.shift}; fwrite(s2, 4, 2, out);
            }
            free(raw); free(seq);
        }
    }
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


def build_harness(tmp, ref, text):
    """compiles the reference's events.c and align.c and a harness into tmp/harness"""
    src = os.path.join(ref, "abea", "src")
    os.makedirs(os.path.join(tmp, "stub", "htslib"))
    sam_h = G0.STUB_SAM_H + "typedef struct htsFile samFile;\n"
    for name, header in (("htslib/sam.h", sam_h), ("htslib/faidx.h", ""), ("htslib/hts.h", ""), ("hdf5.h", "")):
        open(os.path.join(tmp, "stub", name), "w").write(header)
    open(os.path.join(tmp, "harness.cpp"), "w").write(text)
    flags = ["-O2", "-std=c++11", "-ffp-contract=off", "-DFAST5LITE_H", "-DNANOPOLISH_READ_DB_H", "-I" + os.path.join(tmp, "stub"), "-I" + src]
    exe = os.path.join(tmp, "harness")
    subprocess.check_call(["g++"] + flags + [os.path.join(tmp, "harness.cpp"), os.path.join(src, "events.c"), os.path.join(src, "align.c"), "-o", exe, "-lm"])
    return exe


def run_reference(ref, level_mean, reads):
    with tempfile.TemporaryDirectory(prefix="abea_events_golden_") as tmp:
        exe = build_harness(tmp, ref, HARNESS)
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
    make_cases(ref, level_mean, reads)


def run_reference_on_cases(ref, groups):
    """groups: list of (pore model level_mean, reads); a read is (kind, float data, range, digitisation, offset, bases), kind 0 for
    samples and 1 for event means.  Every read runs alone through the build with assertions on.
    -> per read (events or None, scale, shift), or the text of the assertion (or the signal) that ended the run"""
    rec = np.dtype([("start", "<i8"), ("length", "<f4"), ("mean", "<f4"), ("stdv", "<f4")])
    out = []
    with tempfile.TemporaryDirectory(prefix="abea_events_golden_") as tmp:
        exe = build_harness(tmp, ref, HARNESS_CASES)
        inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<i", len(groups)))
            for level_mean, reads in groups:
                f.write(np.asarray(level_mean, "<f4").tobytes() + struct.pack("<i", len(reads)))
                for kind, data, rg, dg, of, seq in reads:
                    f.write(struct.pack("<iiifff", kind, data.size, len(seq), float(rg), float(dg), float(of)) + np.asarray(data, "<f4").tobytes() + seq)
        kinds = [r[0] for _, reads in groups for r in reads]
        for i, kind in enumerate(kinds):
            p = subprocess.run([exe, inp, outp, str(i)], stderr=subprocess.PIPE)
            if p.returncode != 0:
                m = re.search(r"Assertion `(.*)' failed", p.stderr.decode(errors="replace"))
                out.append(m.group(1) if m else f"ended with status {p.returncode}")
                continue
            raw = open(outp, "rb").read()
            (ne,) = struct.unpack_from("<q", raw, 0)
            ev = np.frombuffer(raw, rec, ne, 8)
            scale, shift = struct.unpack_from("<ff", raw, 8 + rec.itemsize * ne)
            out.append((ev if kind == 0 else None, scale, shift))
    return out


def make_cases(ref, level_mean, fixture):
    """the second product: tests/golden/abea_events_cases.npz (the constructed signals of tests/abea_events_cases.py that have 1000 samples
    at least, as float samples, and its scalings reads) and tests/golden/abea_events_cases_expected.json (the reference's event table
    and scalings of each; a read it refuses under "undefined_in_reference" with the assertion's text)"""
    names, signals, seqs = C.reference_signals(level_mean, fixture=fixture)
    edge, _, _ = C.scalings_edge_cases()
    route, models = C.scalings_route_cases(), C.route_models(level_mean)
    one = np.float32(1)
    main_group = [(0, s[0], s[1], s[2], s[3], q) for s, q in zip(signals, seqs)] + [(1, e, one, one, 0 * one, q) for q, e in edge]
    groups = [(level_mean, main_group)] + [(models[m], [(1, e, one, one, 0 * one, q) for q, e in route]) for m in ("coarse", "tiny")]
    all_names = names + list(C.EDGE_NAMES) + [f"route_{m}_{i}" for m in ("coarse", "tiny") for i in range(len(route))]
    pore = ["level_mean"] * len(main_group) + [m for m in ("coarse", "tiny") for _ in route]
    got = run_reference_on_cases(ref, groups)
    assert len(got) == len(all_names) == len(set(all_names))

    undefined = {n: "fewer than 1000 samples: not run (the reference's discarded trim step aborts or reads out of bounds)"
                 for n in C.not_run_in_reference(level_mean, fixture=fixture)}
    recs = []
    for name, model, g in zip(all_names, pore, got):
        if isinstance(g, str):
            undefined[name] = g
            recs.append({"name": name, "pore_model": model, "undefined_in_reference": True})
            continue
        ev, sc, sh = g
        rec = {"name": name, "pore_model": model}
        if ev is not None:
            assert ev.size >= 2 and ev["start"][0] == 0 and np.all(np.diff(ev["start"]) > 0), name
            rec.update(n_events=int(ev.size), events=M.events_digest(ev))
        rec.update(scale=float(np.float32(sc)).hex(), shift=float(np.float32(sh)).hex())
        recs.append(rec)
    # the conditions on the cases: the reference runs everything but the flat read
    assert [n for n in all_names if n in undefined] == ["flat_1500"], undefined
    for n in [f"chunk_{k}" for k in (C.CHUNK - 1, C.CHUNK, C.CHUNK + 1, 2 * C.CHUNK + C.WARMUP)] + ["flat_run", "samples_1000", "samples_1001",
                                                                                                  "square_wave_14", "square_wave_6"]:
        assert n in names, n
    assert sum(n.startswith("planted_") for n in names) == 4

    n_sig = len(signals)
    given = [e for _, e in edge] + [e for _ in ("coarse", "tiny") for _, e in route]
    all_seqs = seqs + [q for q, _ in edge] + [q for _ in ("coarse", "tiny") for q, _ in route]
    npz = os.path.join(HERE, "abea_events_cases.npz")
    save_npz(npz, [("raw", np.concatenate([s[0] for s in signals]).astype(np.float32)), ("n_samples", np.array([s[0].size for s in signals], np.int32)),
                   ("range", np.array([s[1] for s in signals], np.float32)), ("digitisation", np.array([s[2] for s in signals], np.float32)),
                   ("offset", np.array([s[3] for s in signals], np.float32)), ("means", np.concatenate(given).astype(np.float32)),
                   ("n_means", np.array([e.size for e in given], np.int32)), ("seq", np.frombuffer(b"".join(all_seqs), np.uint8)),
                   ("seq_len", np.array([len(q) for q in all_seqs], np.int32))])
    assert os.path.getsize(npz) < 500_000
    doc = {"fixture": "abea_events_cases.npz", "fixture_sha256": hashlib.sha256(open(npz, "rb").read()).hexdigest(),
           "seeds": {"mixed": C.MIXED_SEED, "edge": C.EDGE_SEED, "route": C.ROUTE_SEED, "extra": C.EXTRA_SEED},
           "pore_models": {"level_mean": "level_mean of abea_small.npz", "coarse": "its levels rounded to 1/4 pA", "tiny": "its level of rank 0 set to 1e-30"},
           "reference_build": "g++ -O2 -std=c++11 -ffp-contract=off, events.c and align.c alone, assertions on, float samples, every read alone",
           "signals": n_sig, "undefined_in_reference": undefined, "reads": recs}
    with open(os.path.join(HERE, "abea_events_cases_expected.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{n_sig} signals and {len(given)} scalings reads; {len(undefined)} undefined in the reference; {os.path.getsize(npz)} bytes")


if __name__ == "__main__":
    main()
