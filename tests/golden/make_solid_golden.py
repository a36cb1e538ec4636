#!/usr/bin/env python3
"""Records what THE REFERENCE ITSELF builds and prints in VertexIndex::buildIndexUnevenCoverage (kmer-cnt/vertex_index.cpp:30-130),
the solid k-mer index that its driver carries commented out (kmer-cnt/kmer_cnt.cpp:228-230, 290-292), for the two kmer-cnt fixtures.
Build machine only; the fixtures are those of make_kmer_golden.py and are not rewritten.

    python tests/golden/make_solid_golden.py [--reference DIR]

The reference's default build cannot run this path: with COUNT_VERSION 3 (kmer-cnt/vertex_index.h:23) getFreq throws
(kmer-cnt/vertex_index.cpp:863-890).  With COUNT_VERSION 0 getFreq is the exact count (kmer-cnt/vertex_index.cpp:517-617, 865-886).
So DIR is copied into a temporary directory outside the repository, that one define is flipped IN THE COPY, and SOLID_MAIN below --
a small program of our own that uses only the reference's public interface (countKmers, buildIndexUnevenCoverage, isRepetitive,
kmerFreq, iterKmerPos, globalPosition, Logger::get().setDebugging(true)) -- is compiled against the copy's three source files with
    g++ -O3 -fopenmp -std=c++11 sequence_container.cpp sequence.cpp vertex_index.cpp solid_dump.cpp -I. -Ilibcuckoo -lz -lm -ldl
It runs with 1 and 4 threads (which must agree: the lines and the index) for
    both fixtures x k in 11, 15, 17 x (min_freq, select_rate, tandem_freq, repeat_kmer_rate) in PARAMS.
Kept per case in kmer_solid_expected.json: the six debug lines as the reference wrote them ("Mean k-mer frequency", "Repetitive
k-mer frequency", "Filtered N repetitive k-mers (R)", "Selected k-mers", "Index size", "Mean k-mer index frequency"; integers as
integers, floats as the strings its ostream wrote), the sha256 of tests/minimizer_model.py's serialisation over the NON-EMPTY lists
(the reference's "Selected k-mers" counts keys whose list stayed empty too; through its public interface those read as absent), the
number of non-empty lists and of removed k-mers; and for one tiny case the arrays themselves in kmer_solid_tiny.npz.  Before
anything is recorded the harness must reproduce CHECK below.  Nothing compiled and no reference text is kept.
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import kmer_model, minimizer_model  # noqa: E402

KS = (11, 15, 17)
PARAMS = ((2, .40, 100, 100), (2, .40, 100, 1.5), (2, .40, 2, 1.5), (1, .05, 0, 1.5), (2, 0, 100, 1.5), (0, .9, 1, 1.5), (3, .40, 3, 1.5))
THREADS = (1, 4)
FILES = ("kmer_small.fa", "kmer_small_n.fq.gz")
TINY = {"file": "kmer_small.fa", "k": 11, "min_freq": 2, "select_rate": .40, "tandem_freq": 2, "rate": 1.5, "kept_reads": 6}
# kmer_small.fa, k = 15: (params) -> (thr, selected, non-empty, index size, filtered entries or None, removed keys or None)
CHECK = {(2, .40, 100, 100): (278, 25477, 25477, 66850, None, None), (2, .40, 2, 1.5): (3, 22210, 21910, 49383, 13607, 3267)}
SOURCES = ["sequence_container.cpp", "sequence.cpp", "vertex_index.cpp"]
FLAGS = ["-O3", "-fopenmp", "-std=c++11"]
LIBS = ["-I.", "-Ilibcuckoo", "-lz", "-lm", "-ldl"]

SOLID_MAIN = r"""
// solid_dump READS K MIN_FREQ SELECT_RATE TANDEM REPEAT_RATE THREADS OUT: counts, builds the solid index through the library's
// public interface and writes it out; the library's debug lines go to stderr
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#include <string>
#include <fstream>
#include "vertex_index.h"

int main(int argc, char **argv) {
    if (argc != 9) return 2;
    const std::string cfg = std::string(argv[8]) + ".cfg";
    { std::ofstream f(cfg); f << "repeat_kmer_rate = " << argv[6] << "\nassemble_kmer_sample = 1\n"; }
    Config::load(cfg);
    Logger::get().setDebugging(true);
    Parameters::get().numThreads = atoi(argv[7]);
    Parameters::get().kmerSize = atoi(argv[2]);
    Parameters::get().minimumOverlap = 1000;
    Parameters::get().unevenCoverage = true;
    SequenceContainer reads;
    reads.loadFromFile(argv[1], 5000);
    reads.buildPositionIndex();
    VertexIndex index(reads, (int)Config::get("assemble_kmer_sample"));
    index.outputProgress(false);
    index.countKmers();
    index.buildIndexUnevenCoverage(atoi(argv[3]), (float)atof(argv[4]), atoi(argv[5]));
    std::map<size_t, Kmer> seen;          // canonical k-mers of the forward strands
    for (const auto &rec : reads.iterSeqs()) {
        if (!rec.id.strand()) continue;
        for (auto kp : IterKmers(rec.sequence)) {
            Kmer km = kp.kmer;
            km.standardForm();
            seen.insert(std::make_pair(km.numRepr(), km));
        }
    }
    FILE *out = fopen(argv[8], "wb");
    if (!out) return 3;
    std::vector<long long> keys, sizes, positions, gone;
    for (const auto &it : seen) {
        if (index.isRepetitive(it.second)) { gone.push_back((long long)it.first); continue; }
        if (index.kmerFreq(it.second) == 0) continue;
        long long n = 0;
        for (auto pos : index.iterKmerPos(it.second)) { positions.push_back((long long)reads.globalPosition(pos.readId, pos.position)); n++; }
        keys.push_back((long long)it.first); sizes.push_back(n);
    }
    long long head[3] = {(long long)keys.size(), (long long)positions.size(), (long long)gone.size()};
    fwrite(head, 8, 3, out);
    fwrite(keys.data(), 8, keys.size(), out);
    fwrite(sizes.data(), 8, sizes.size(), out);
    fwrite(positions.data(), 8, positions.size(), out);
    fwrite(gone.data(), 8, gone.size(), out);
    fclose(out);
    return 0;
}
"""

LINES = (("mean_frequency", r"Mean k-mer frequency: (\S+)$"), ("repetitive_frequency", r"Repetitive k-mer frequency: (\d+)$"),
         ("filtered", r"Filtered (\d+) repetitive k-mers \((\S+)\)$"), ("selected_kmers", r"Selected k-mers: (\d+)$"),
         ("index_entries", r"Index size: (\d+)$"), ("mean_index_frequency", r"Mean k-mer index frequency: (\S+)$"))


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def parse_debug(stderr):
    """the six lines, in the reference's order"""
    text = [ln.split("DEBUG: ", 1)[1] for ln in stderr.splitlines() if "DEBUG: " in ln]
    row, at = {}, 0
    for name, pat in LINES:
        while at < len(text) and not re.match(pat, text[at]):
            at += 1
        assert at < len(text), (name, stderr[-600:])
        m = re.match(pat, text[at])
        at += 1
        if name == "filtered":
            row["filtered_entries"] = int(m.group(1)); row["filtered_rate"] = m.group(2)
        elif name in ("repetitive_frequency", "selected_kmers", "index_entries"):
            row[name] = int(m.group(1))
        else:
            row[name] = m.group(1)
    return row


def run_case(exe, reads, k, params, threads, out):
    """-> (the row, kmers, start, gpos, removed k-mers) of the reference's index"""
    mf, sr, tf, rr = params
    r = subprocess.run([exe, reads, str(k), str(mf), repr(float(sr)), str(tf), repr(float(rr)), str(threads), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    row = parse_debug(r.stderr)
    raw = np.fromfile(out, "<i8")
    nk, ne, gone = (int(x) for x in raw[:3])
    assert raw.size == 3 + 2 * nk + ne + gone
    kmers = raw[3:3 + nk].astype(np.uint64)
    sizes = raw[3 + nk:3 + 2 * nk]
    gpos = raw[3 + 2 * nk:3 + 2 * nk + ne]
    full = sizes > 0                        # (kmerFreq is the list's length, so an empty list never gets here; kept for the record)
    start = np.zeros(int(full.sum()) + 1, np.int64)
    start[1:] = np.cumsum(sizes[full])
    kmers = kmers[full]
    assert start[-1] == ne == row["index_entries"]
    inner = np.ones(ne, bool)
    inner[start[:-1][start[:-1] < ne]] = False
    assert (np.diff(gpos)[inner[1:]] > 0).all(), "a list of the reference's index is not ascending"
    row.update({"indexed_kmers": int(kmers.size), "filtered_kmers": gone, "index_sha256": minimizer_model.digest(kmers, start, gpos)})
    return row, kmers, start, gpos, raw[3 + 2 * nk + ne:].astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference/benchmarks/kmer-cnt")
    a = ap.parse_args()
    exp = {}
    with tempfile.TemporaryDirectory(prefix="kmer_solid_ref_") as tmp:
        src = os.path.join(tmp, "kmer-cnt")
        shutil.copytree(a.reference, src)
        hdr = os.path.join(src, "vertex_index.h")
        os.chmod(hdr, 0o644)
        text = open(hdr).read()
        assert text.count("#define COUNT_VERSION 3") == 1
        open(hdr, "w").write(text.replace("#define COUNT_VERSION 3", "#define COUNT_VERSION 0"))
        open(os.path.join(src, "solid_dump.cpp"), "w").write(SOLID_MAIN)
        exe = os.path.join(tmp, "solid_dump")
        subprocess.check_call(["g++", *FLAGS, "-w", *SOURCES, "solid_dump.cpp", *LIBS, "-o", exe], cwd=src)
        out = os.path.join(tmp, "index.bin")

        def both(path, k, params):
            got = [run_case(exe, path, k, params, t, out) for t in THREADS]
            assert got[0][0] == got[1][0], ("thread counts disagree", got[0][0], got[1][0])
            return got[0]

        for params, want in CHECK.items():
            row = both(os.path.join(HERE, "kmer_small.fa"), 15, params)[0]
            have = (row["repetitive_frequency"], row["selected_kmers"], row["indexed_kmers"], row["index_entries"], row["filtered_entries"],
                    row["filtered_kmers"])
            assert all(w is None or w == h for w, h in zip(want, have)), (params, want, have)
        exp["command"] = ("solid_dump (a main of our own over the reference's public interface: countKmers, buildIndexUnevenCoverage(min_freq, select_rate, "
                          "tandem_freq), repeat_kmer_rate from the config) on a copy of kmer-cnt/ with COUNT_VERSION 0; g++ -O3 -fopenmp -std=c++11")
        exp["serialisation"] = "little-endian int64: k-mers ascending, each followed by its ascending global positions; non-empty lists only"
        exp["min_len_exclusive"] = 5000
        exp["files"] = {}
        for name in FILES:
            path = os.path.join(HERE, name)
            rows = []
            for k in KS:
                for params in PARAMS:
                    row = {"k": k, "min_freq": params[0], "select_rate": params[1], "tandem_freq": params[2], "rate": params[3]}
                    row.update(both(path, k, params)[0])
                    rows.append(row)
                    print(name, row, flush=True)
            exp["files"][name] = {"sha256": sha256(path), "threads": list(THREADS), "rows": rows}
        reads = [r for r in kmer_model.load_reads([os.path.join(HERE, TINY["file"])]) if len(r) > 5000][:TINY["kept_reads"]]
        tiny_fa = os.path.join(tmp, "tiny.fasta")
        with open(tiny_fa, "wb") as f:
            for i, r in enumerate(reads):
                f.write(b">tiny_%d\n%s\n" % (i, r))
        row, kmers, start, gpos, gone = both(tiny_fa, TINY["k"], (TINY["min_freq"], TINY["select_rate"], TINY["tandem_freq"], TINY["rate"]))
        np.savez_compressed(os.path.join(HERE, "kmer_solid_tiny.npz"), kmers=kmers, start=start, gpos=gpos, repetitive=gone,
                            read_lengths=np.array([len(r) for r in reads], np.int64))
        exp["tiny"] = dict(TINY, **row)
        print("tiny", exp["tiny"], flush=True)
    json.dump(exp, open(os.path.join(HERE, "kmer_solid_expected.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
