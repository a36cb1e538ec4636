#!/usr/bin/env python3
"""Records what THE REFERENCE ITSELF prints and builds in its minimizer mode (use_minimizers = 1) for the two kmer-cnt fixtures.
Build machine only; the fixtures are those of make_kmer_golden.py and are not rewritten.

    python tests/golden/make_minimizer_golden.py [--reference DIR] [--time]

The reference is compiled from DIR into a temporary directory outside the repository with the command make_kmer_golden.py records,
    g++ -O3 -fopenmp -std=c++11 sequence_container.cpp sequence.cpp vertex_index.cpp kmer_cnt.cpp -Ilibcuckoo -lz -lm -ldl -o kmer-cnt
and run with --debug, --threads 1 and 4 (which must agree), on config files this script writes into the same temporary directory
(kmer_size, use_minimizers = 1, minimizer_window = W, repeat_kmer_rate = R, assemble_kmer_sample = 1), for
    k in 11, 15, 17    W in 1, 2, 5, 10, 19    R in 100, 3.
Its lines "Mean k-mer frequency", "Repetitive k-mer frequency", "Filtered N repetitive k-mers (R)", "Selected k-mers", "K-mer index
size", "Mean k-mer frequency", "Minimizer rate" go into kmer_minimizer_expected.json: the integers as integers, the floats as the
strings its ostream wrote.

The index itself: INDEX_MAIN below, a small program of our own that uses only the reference's public interface
(buildIndexMinimizers, kmerFreq, isRepetitive, iterKmerPos, globalPosition), is compiled against the same three source files in the
temporary directory.  It writes the index out; its digest is taken over little-endian int64 -- k-mers ascending, each followed by its ascending global
positions (the serialisation of tests/minimizer_model.py) -- and the removed (repetitive) k-mers; this script keeps the sha256 of the
serialisation per case, the number of emitted minimizers, of distinct and of removed k-mers, and for one tiny case (k = 11, W = 5, R = 3, the first 6 kept reads of
kmer_small.fa) the arrays themselves in kmer_minimizer_tiny.npz.  Nothing compiled and no reference text is kept.
--time additionally runs the reference on the E. coli-like read set of tools/kmer_bench.py (--threads 16, W = 10, R = 100, k = 17
and 15) and records its "Kernel time": the CPU of THIS build machine, for the README's caveat.
"""
import argparse
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
from tests import kmer_model, minimizer_model  # noqa: E402

KS = (11, 15, 17)
WINDOWS = (1, 2, 5, 10, 19)
RATES = (100, 3)
THREADS = (1, 4)
FILES = ("kmer_small.fa", "kmer_small_n.fq.gz")
TINY = {"file": "kmer_small.fa", "k": 11, "window": 5, "rate": 3, "kept_reads": 6}
SOURCES = ["sequence_container.cpp", "sequence.cpp", "vertex_index.cpp"]
FLAGS = ["-O3", "-fopenmp", "-std=c++11"]
LIBS = ["-Ilibcuckoo", "-lz", "-lm", "-ldl"]

INDEX_MAIN = r"""
// index_dump READS CONFIG K OUT: builds the minimizer index through the library's public interface and writes it out
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#include <algorithm>
#include <string>
#include "vertex_index.h"

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    Config::load(argv[2]);
    Parameters::get().numThreads = 1;
    Parameters::get().kmerSize = atoi(argv[3]);
    Parameters::get().minimumOverlap = 1000;
    Parameters::get().unevenCoverage = false;
    SequenceContainer reads;
    reads.loadFromFile(argv[1], 5000);
    reads.buildPositionIndex();
    VertexIndex index(reads, (int)Config::get("assemble_kmer_sample"));
    index.outputProgress(false);
    index.buildIndexMinimizers(1, (int)Config::get("minimizer_window"));
    std::map<size_t, Kmer> seen;          // canonical k-mers of the forward strands
    long long minimizers = 0;
    for (const auto &rec : reads.iterSeqs()) {
        if (!rec.id.strand()) continue;
        minimizers += (long long)yieldMinimizers(rec.sequence, (int)Config::get("minimizer_window")).size();
        for (auto kp : IterKmers(rec.sequence)) {
            Kmer km = kp.kmer;
            km.standardForm();
            seen.insert(std::make_pair(km.numRepr(), km));
        }
    }
    FILE *out = fopen(argv[4], "wb");
    if (!out) return 3;
    std::vector<long long> keys, sizes, positions, gone;
    for (const auto &it : seen) {
        if (index.isRepetitive(it.second)) { gone.push_back((long long)it.first); continue; }
        if (index.kmerFreq(it.second) == 0) continue;
        long long n = 0;
        for (auto pos : index.iterKmerPos(it.second)) { positions.push_back((long long)reads.globalPosition(pos.readId, pos.position)); n++; }
        keys.push_back((long long)it.first); sizes.push_back(n);
    }
    // four sections: the k-mers, the length of each list, the lists back to back, the removed k-mers
    long long head[4] = {(long long)keys.size(), (long long)positions.size(), (long long)gone.size(), minimizers};
    fwrite(head, 8, 4, out);
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
         ("index_entries", r"K-mer index size: (\d+)$"), ("mean_frequency_kept", r"Mean k-mer frequency: (\S+)$"),
         ("minimizer_rate", r"Minimizer rate: (\S+)$"))


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def write_cfg(tmp, k, w, rate):
    path = os.path.join(tmp, "mini_k%d_w%d_r%g.cfg" % (k, w, rate))
    with open(path, "w") as f:
        f.write("kmer_size = %d\nuse_minimizers = 1\nminimizer_window = %d\nrepeat_kmer_rate = %g\nassemble_kmer_sample = 1\n" % (k, w, rate))
    return path


def parse_debug(stderr):
    """the seven lines, in the reference's order (the label 'Mean k-mer frequency' comes twice)"""
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


def run_reference(exe, reads, cfg, threads):
    r = subprocess.run([exe, "--reads", reads, "--config", cfg, "--threads", str(threads), "--debug"], capture_output=True, text=True, check=True)
    row = parse_debug(r.stderr)
    return row, float(re.search(r"Kernel time: ([0-9.]+) sec", r.stderr).group(1))


def run_index(exe, reads, cfg, k, out):
    """-> (the row's fields, kmers, start, gpos, removed k-mers) of the reference's index"""
    subprocess.run([exe, reads, cfg, str(k), out], capture_output=True, text=True, check=True)
    raw = np.fromfile(out, "<i8")
    nk, ne, gone, minimizers = (int(x) for x in raw[:4])
    assert raw.size == 4 + 2 * nk + ne + gone
    kmers = raw[4:4 + nk].astype(np.uint64)
    start = np.zeros(nk + 1, np.int64)
    start[1:] = np.cumsum(raw[4 + nk:4 + 2 * nk])
    gpos = raw[4 + 2 * nk:4 + 2 * nk + ne]
    assert start[-1] == ne and (np.diff(kmers.astype(np.int64)) > 0).all()
    inner = np.ones(ne, bool)
    inner[start[:-1][start[:-1] < ne]] = False
    assert (np.diff(gpos)[inner[1:]] > 0).all(), "a list of the reference's index is not ascending"
    row = {"selected_kmers": nk, "index_entries": ne, "filtered_kmers": gone, "minimizers": minimizers,
           "distinct": nk + gone, "index_sha256": minimizer_model.digest(kmers, start, gpos)}
    return row, kmers, start, gpos, raw[4 + 2 * nk + ne:].astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference/benchmarks/kmer-cnt")
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    src = a.reference
    exp_path = os.path.join(HERE, "kmer_minimizer_expected.json")
    exp = json.load(open(exp_path)) if os.path.exists(exp_path) else {}
    with tempfile.TemporaryDirectory(prefix="kmer_mini_ref_") as tmp:
        exe = os.path.join(tmp, "kmer-cnt")
        subprocess.check_call(["g++", *FLAGS, *SOURCES, "kmer_cnt.cpp", *LIBS, "-o", exe], cwd=src)
        main_cpp = os.path.join(tmp, "index_dump.cpp")
        open(main_cpp, "w").write(INDEX_MAIN)
        idx = os.path.join(tmp, "index_dump")
        subprocess.check_call(["g++", *FLAGS, "-w", *SOURCES, main_cpp, "-I.", *LIBS, "-o", idx], cwd=src)
        exp["command"] = ("kmer-cnt --reads <file> --config <cfg> --threads T --debug, <cfg> = kmer_size = K, use_minimizers = 1, minimizer_window = W, "
                          "repeat_kmer_rate = R, assemble_kmer_sample = 1; built with g++ -O3 -fopenmp -std=c++11 sequence_container.cpp sequence.cpp "
                          "vertex_index.cpp kmer_cnt.cpp -Ilibcuckoo -lz -lm -ldl")
        exp["serialisation"] = "little-endian int64: k-mers ascending, each followed by its ascending global positions"
        exp["min_len_exclusive"] = 5000
        exp["files"] = {}
        for name in FILES:
            path = os.path.join(HERE, name)
            rows = []
            for k in KS:
                for w in WINDOWS:
                    for rate in RATES:
                        cfg = write_cfg(tmp, k, w, rate)
                        got = [run_reference(exe, path, cfg, t)[0] for t in THREADS]
                        assert all(g == got[0] for g in got), "thread counts disagree"
                        row = {"k": k, "window": w, "rate": rate}
                        row.update(got[0])
                        more = run_index(idx, path, cfg, k, os.path.join(tmp, "index.bin"))[0]
                        assert (more["selected_kmers"], more["index_entries"]) == (row["selected_kmers"], row["index_entries"])
                        row.update(more)
                        rows.append(row)
                        print(name, row, flush=True)
            exp["files"][name] = {"sha256": sha256(path), "threads": list(THREADS), "rows": rows}
        # the tiny case, arrays and all
        reads = [r for r in kmer_model.load_reads([os.path.join(HERE, TINY["file"])]) if len(r) > 5000][:TINY["kept_reads"]]
        tiny_fa = os.path.join(tmp, "tiny.fasta")
        with open(tiny_fa, "wb") as f:
            for i, r in enumerate(reads):
                f.write(b">tiny_%d\n%s\n" % (i, r))
        cfg = write_cfg(tmp, TINY["k"], TINY["window"], TINY["rate"])
        row, _ = run_reference(exe, tiny_fa, cfg, 1)
        more, kmers, start, gpos, gone = run_index(idx, tiny_fa, cfg, TINY["k"], os.path.join(tmp, "tiny.bin"))
        row.update(more)
        np.savez_compressed(os.path.join(HERE, "kmer_minimizer_tiny.npz"), kmers=kmers, start=start, gpos=gpos, repetitive=gone,
                            read_lengths=np.array([len(r) for r in reads], np.int64))
        exp["tiny"] = dict(TINY, **row)
        print("tiny", exp["tiny"], flush=True)
        if a.time:
            from tools import kmer_bench
            big = os.path.join(tmp, "ecoli_like.fasta")
            kmer_bench.write_fasta(big, kmer_bench.ecoli_like_reads())
            rows = {}
            for k in (17, 15):
                cfg = write_cfg(tmp, k, 10, 100)
                r = subprocess.run([exe, "--reads", big, "--config", cfg, "--threads", "16", "--debug"], capture_output=True, text=True, check=True)
                g = parse_debug(r.stderr)
                g["kernel_time_s"] = float(re.search(r"Kernel time: ([0-9.]+) sec", r.stderr).group(1))
                rows[str(k)] = g
                print("timed", k, g, flush=True)
            exp["reference_cpu_time"] = {"what": "the reference's own 'Kernel time' with use_minimizers = 1, minimizer_window = 10, repeat_kmer_rate = 100 on "
                                                 "tools/kmer_bench.py's E. coli-like set, --threads 16, on the build machine's CPU (another machine than the "
                                                 "GPU's; not a ratio)", "cpus_of_the_build_machine": os.cpu_count(), "k": rows}
    json.dump(exp, open(exp_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
