#!/usr/bin/env python3
"""Writes the kmer-cnt fixtures and records what THE REFERENCE ITSELF prints for them.  Build machine only.

    python tests/golden/make_kmer_golden.py [--reference DIR] [--time]

Fixtures (seeded generator below, nothing of the reference's):
    kmer_small.fa        about 40 reads of 10 .. ~14 000 bases cut from a random genome with 5 % substitutions, both strands, some in
                         lower case, multi-line and single-line records; reads of exactly 5000 and 5001 bases (the two sides of the
                         length filter) and one shorter than k; a 300-base tandem repeat in every third read, poly-A tails (a key
                         with count >= 512) and one (AC)n stretch (keys with a count in 256 .. 511)
    kmer_small_n.fq.gz   a gzip FASTQ whose reads hold N and other bytes outside ACGTacgt (single ones, a run of 100, kept and
                         filtered reads): what the reference makes of them is in tests/kmer_model.py, unknown_to_t
The reference is compiled from DIR (default: the kmer-cnt directory of the reference tree) into a temporary directory outside the
repository with
    g++ -O3 -fopenmp -std=c++11 sequence_container.cpp sequence.cpp vertex_index.cpp kmer_cnt.cpp -Ilibcuckoo -lz -lm -ldl -o kmer-cnt
and run with its own config/asm_raw_reads.cfg at --kmer 11, 15, 16, 17 and --threads 1, 4; "Hash size" and "Total k-mers" of its --debug
output go into kmer_expected.json with the sha256 of the files; how the fixtures were made goes into KMER_MANIFEST.json.  Nothing compiled and no reference text is kept.
--time additionally generates the E. coli-like read set of tools/kmer_bench.py into the temporary directory, runs the reference
on it with --threads 16 at k = 17 and 15 and records its "Kernel time" -- the CPU of THIS build machine, for the README's caveat.
"""
import argparse
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import kmer_model  # noqa: E402

KS = (11, 15, 16, 17)
THREADS = (1, 4)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def _mutate(rng, s, rate):
    a = np.frombuffer(s, np.uint8).copy()
    hit = np.flatnonzero(rng.random(a.size) < rate)
    a[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, hit.size)]
    return a.tobytes()


def small_reads(seed=20261016):
    rng = np.random.default_rng(seed)
    genome = _bases(rng, 60000)
    unit = _bases(rng, 300)
    lengths = [int(x) for x in rng.integers(17, 14000, 38)]
    lengths[3], lengths[8], lengths[20] = 5000, 5001, 10
    reads = []
    for i, ln in enumerate(lengths):
        at = int(rng.integers(0, len(genome) - ln))
        body = _mutate(rng, genome[at:at + ln], 0.05)
        special = ln in (5000, 5001, 10)
        if not special and i % 3 == 0 and ln > 6000:
            cut = int(rng.integers(100, ln - 4500))
            rep = unit * int(rng.integers(2, 14))
            body = (body[:cut] + rep + body[cut:])[:ln]
        if not special and i % 4 == 0 and ln > 5300:
            body = body[:ln - 400] + b"A" * 400
        if i == 5:
            body = body[:1000] + b"AC" * 350 + body[1700:]
            body = body + _bases(rng, 5200)          # (kept whatever length the draw gave)
        if i % 2:
            body = body.translate(COMP)[::-1]
        if i % 5 == 2:
            body = body.lower()
        reads.append(body)
    return reads


def write_fasta(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">read_%d len=%d\n" % (i, len(r)))
            if i % 4 == 3:
                f.write(r + b"\n")
            else:
                for j in range(0, len(r), 80):
                    f.write(r[j:j + 80] + b"\n")


def n_reads(seed=20261017):
    rng = np.random.default_rng(seed)
    genome = _bases(rng, 30000)
    reads = []
    for i, ln in enumerate([300, 5600, 4999, 7000, 5001, 6100, 17, 5000, 8000, 5300]):
        at = int(rng.integers(0, len(genome) - ln))
        a = np.frombuffer(_mutate(rng, genome[at:at + ln], 0.03), np.uint8).copy()
        hit = np.flatnonzero(rng.random(ln) < 0.012)
        a[hit] = np.frombuffer(b"NNNNnRYK-", np.uint8)[rng.integers(0, 9, hit.size)]
        if i == 3:
            a[1000:1100] = ord("N")                 # a run of N
        reads.append(a.tobytes())
    return reads


def write_fastq_gz(path, reads):
    with open(path, "wb") as raw:
        with gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0, compresslevel=9) as f:
            for i, r in enumerate(reads):
                f.write(b"@nread_%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def build_reference(src, tmp):
    exe = os.path.join(tmp, "kmer-cnt")
    subprocess.check_call(["g++", "-O3", "-fopenmp", "-std=c++11", "sequence_container.cpp", "sequence.cpp", "vertex_index.cpp", "kmer_cnt.cpp",
                           "-Ilibcuckoo", "-lz", "-lm", "-ldl", "-o", exe], cwd=src)
    return exe


def run_reference(exe, src, reads, k, threads):
    r = subprocess.run([exe, "--reads", ",".join(reads), "--config", os.path.join(src, "config", "asm_raw_reads.cfg"), "--kmer", str(k),
                        "--threads", str(threads), "--debug"], capture_output=True, text=True, check=True)
    return {"hash_size": int(re.search(r"Hash size: (\d+)", r.stderr).group(1)),
            "total_kmers": int(re.search(r"Total k-mers (\d+)", r.stderr).group(1)),
            "kernel_time_s": float(re.search(r"Kernel time: ([0-9.]+) sec", r.stderr).group(1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference/benchmarks/kmer-cnt")
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    fa = os.path.join(HERE, "kmer_small.fa")
    fq = os.path.join(HERE, "kmer_small_n.fq.gz")
    write_fasta(fa, small_reads())
    write_fastq_gz(fq, n_reads())
    # the properties the tests rely on, checked with the model before the reference is asked
    reads = kmer_model.load_reads([fa])
    lens = [len(r) for r in reads]
    assert 5000 in lens and 5001 in lens and min(lens) < min(KS) and os.path.getsize(fa) < 400 * 1024
    assert any(r != r.upper() for r in reads)
    for k in KS:
        m = kmer_model.model(reads, k)
        assert m["max_count"] >= 512 and ((m["counts"] >= 256) & (m["counts"] < 512)).any() and m["total_kmers"] != m["distinct"], (k, m["max_count"])

    exp_path = os.path.join(HERE, "kmer_expected.json")
    exp = json.load(open(exp_path)) if os.path.exists(exp_path) else {}
    with tempfile.TemporaryDirectory(prefix="kmer_ref_") as tmp:
        exe = build_reference(a.reference, tmp)
        exp["command"] = ("kmer-cnt --reads <file> --config <reference>/kmer-cnt/config/asm_raw_reads.cfg --kmer K --threads T --debug; "
                          "built with g++ -O3 -fopenmp -std=c++11 sequence_container.cpp sequence.cpp vertex_index.cpp kmer_cnt.cpp "
                          "-Ilibcuckoo -lz -lm -ldl")
        exp["files"] = {}
        for path in (fa, fq):
            rows = {}
            for k in KS:
                got = [run_reference(exe, a.reference, [path], k, t) for t in THREADS]
                assert all((g["hash_size"], g["total_kmers"]) == (got[0]["hash_size"], got[0]["total_kmers"]) for g in got), "thread counts disagree"
                rows[str(k)] = {"hash_size": got[0]["hash_size"], "total_kmers": got[0]["total_kmers"]}
                print(os.path.basename(path), k, rows[str(k)], flush=True)
            exp["files"][os.path.basename(path)] = {"sha256": sha256(path), "threads": list(THREADS), "k": rows}
        # both files in one run
        both = run_reference(exe, a.reference, [fa, fq], 15, 1)
        exp["both_files_k15"] = {"order": [os.path.basename(fa), os.path.basename(fq)], "hash_size": both["hash_size"], "total_kmers": both["total_kmers"]}
        if a.time:
            from tools import kmer_bench
            big = os.path.join(tmp, "ecoli_like.fasta")
            kmer_bench.write_fasta(big, kmer_bench.ecoli_like_reads())
            rows = {}
            for k in (17, 15):
                g = run_reference(exe, a.reference, [big], k, 16)
                rows[str(k)] = g
                print("timed", k, g, flush=True)
            exp["reference_cpu_time"] = {"what": "the reference's own 'Kernel time' on tools/kmer_bench.py's E. coli-like set, --threads 16, on the build "
                                                 "machine's CPU (another machine than the GPU's; not a ratio)", "cpus_of_the_build_machine": os.cpu_count(),
                                         "k": rows}
    json.dump(exp, open(exp_path, "w"), indent=1, sort_keys=True)
    # (a manifest of its own: MANIFEST.json belongs to make_golden.py and stays as it is)
    man_path = os.path.join(HERE, "KMER_MANIFEST.json")
    man = {}
    man["kmer_small"] = {"generator": "tests/golden/make_kmer_golden.py small_reads()", "seed": 20261016, "files": ["kmer_small.fa"],
                         "expected": "kmer_expected.json", "reference": "kmer-cnt/kmer_cnt.cpp + vertex_index.cpp, built in a temporary directory",
                         "command": exp["command"]}
    man["kmer_small_n"] = {"generator": "tests/golden/make_kmer_golden.py n_reads()", "seed": 20261017, "files": ["kmer_small_n.fq.gz"],
                           "expected": "kmer_expected.json", "reference": "kmer-cnt/kmer_cnt.cpp + vertex_index.cpp, built in a temporary directory",
                           "command": exp["command"]}
    json.dump(man, open(man_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
