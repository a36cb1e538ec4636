#!/usr/bin/env python3
"""Build machine only: writes tests/golden/dbg_small.npz (a seeded contig, its reads and the assembly regions the planner cuts, plus
a few constructed regions) and tests/golden/dbg_expected.json (what the reference's createDeBruijnGraph, loadReferenceIntoGraph and
loadBAMDataIntoGraph, dbg/src/debruijn.cpp:846-861, 1291-1317, 1399-1414, leave in allNodes per region, and the read window
setWindowPointers, dbg/src/common.cpp:161-194, gives every planned region).

The reference's debruijn.cpp (its main renamed by a macro) and common.cpp are compiled in a temporary directory outside the
repository with -O2 -fopenmp, against the headers of the reference's own htslib archive (abea/htslib.tar.bz2, unpacked there).
The harness of this script fills the alignedRead array itself and calls only functions that need nothing of htslib at run time;
every function goes into a section of its own and the linker drops the unreferenced ones (main, getRead), so libhts.a is not
needed and is not built.  The harness walks allNodes and writes one record per node in the layout of gab_dbg_node; the verbose
line of a region is printed by the reference's own assembleReadsAndDetectVariants (:1418-1471).  Nothing compiled and no reference
text is kept.  The .npz is written with fixed time stamps, so that the script reproduces the committed files byte for byte.

    python tests/golden/make_dbg_golden.py [/root/reference/benchmarks] [--keep-times]"""
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
import dbg_model as M  # noqa: E402
import make_abea_events_golden as G1  # noqa: E402

SEED, CONTIG, K, MIN_QUAL = 20261021, 9000, 15, 20
# what the fixture must hold, so that it cannot go hollow
AT_LEAST = {"regions": 12, "empty_regions": 2, "qc_fail_reads": 5, "quality_drop_first": 20, "quality_drop_last": 20, "n_drop_first": 3, "n_drop_last": 3,
            "colour3_nodes": 5000, "nodes_first_in_read": 500, "self_loops": 2, "nodes_with_4_edges": 1, "dropped_fifth": 1, "shared_reads": 100,
            "iupac_reads": 5}
FULL_REGIONS = 3        # the non-empty regions with the fewest nodes, their records and printed lines kept

HARNESS = r"""
#define main reference_main
#include "debruijn.cpp"
#undef main
#include <map>
static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
static double now() { struct timespec a; clock_gettime(CLOCK_MONOTONIC, &a); return a.tv_sec + 1e-9 * a.tv_nsec; }
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    int32_t k, min_qual, n_reads, n_regions;
    rd(&k, 4, in); rd(&min_qual, 4, in); rd(&n_reads, 4, in);
    struct ReadArray ra; memset(&ra, 0, sizeof ra);
    ra.array = (struct alignedRead *)calloc(n_reads + 1, sizeof(struct alignedRead));
    ra.__size = n_reads; ra.__capacity = n_reads + 1; ra.__longestRead = 0;
    for (int r = 0; r < n_reads; r++) {
        int32_t v[4]; rd(v, 16, in);                     /* pos, end, rlen, flag */
        struct alignedRead *a = ra.array + r;
        if (v[2] + 1 > MAX_READ_LEN) { fprintf(stderr, "read too long\n"); exit(2); }
        a->pos = v[0]; a->end = v[1]; a->rlen = v[2]; a->flag = v[3];
        rd(a->seq, v[2], in); rd(a->qual, v[2], in);
        if ((int)(a->end - a->pos) > ra.__longestRead) ra.__longestRead = a->end - a->pos;       /* main, :1559-1562 */
    }
    rd(&n_regions, 4, in);
    double seconds = 0;
    for (int g = 0; g < n_regions; g++) {
        int32_t v[7]; rd(v, 28, in);                     /* planned, start, stop, ref_start, ref_len, read_begin, read_end */
        char *ref = (char *)malloc(v[4] + 1); rd(ref, v[4], in); ref[v[4]] = 0;
        struct alignedRead *ws = ra.array + v[5], *we = ra.array + v[6];
        if (v[0]) { setWindowPointers(&ra, v[1], v[2]); ws = ra.windowStart; we = ra.windowEnd; }
        const int32_t win[2] = {(int32_t)(ws - ra.array), (int32_t)(we - ra.array)};
        fwrite(win, 4, 2, out);
        double t0 = now();
        DeBruijnGraph *G = createDeBruijnGraph(k, 5000);
        loadReferenceIntoGraph(G, ref, v[3], k);
        loadBAMDataIntoGraph(G, ws, we, 1, 0, min_qual, k);
        seconds += now() - t0;
        const int32_t n = G->allNodes->top + 1;
        fwrite(&n, 4, 1, out);
        std::map<Node *, int> number;
        for (int i = 0; i < n; i++) number[G->allNodes->elements[i]] = i;
        for (int i = 0; i < n; i++) {
            Node *x = G->allNodes->elements[i];
            int32_t head[4], tail[6] = {x->nEdges, -1, -1, -1, -1, 0};
            int64_t w = (int64_t)x->weight, ew[4] = {0, 0, 0, 0};
            if ((double)w != x->weight) { fprintf(stderr, "a weight that is no integer\n"); exit(3); }
            if (x->sequence >= ref && x->sequence <= ref + v[4]) { head[0] = -1; head[1] = (int32_t)(x->sequence - ref); }
            else {
                const size_t r = (size_t)(x->sequence - (char *)ra.array) / sizeof(struct alignedRead);
                head[0] = (int32_t)r; head[1] = (int32_t)(x->sequence - ra.array[r].seq);
            }
            head[2] = x->colours; head[3] = x->position;
            for (int j = 0; j < 4; j++) if (x->edges[j]) {
                if (j >= x->nEdges || x->edges[j]->startNode != x) { fprintf(stderr, "edge slots\n"); exit(3); }
                tail[1 + j] = number.at(x->edges[j]->endNode);
                ew[j] = (int64_t)x->edges[j]->weight;
                if ((double)ew[j] != x->edges[j]->weight) { fprintf(stderr, "a weight that is no integer\n"); exit(3); }
            }
            fwrite(head, 4, 4, out); fwrite(&w, 8, 1, out); fwrite(tail, 4, 6, out); fwrite(ew, 8, 4, out);
        }
        destroyDeBruijnGraph(G);
        if (k == 15 && min_qual == 20) { fflush(stdout); assembleReadsAndDetectVariants(v[3], v[3] + v[4], ws, we, ref, true); fflush(stdout); }
        free(ref);
    }
    fwrite(&seconds, 8, 1, out);
    fclose(out);
    return 0;
}
"""

BUILD = "g++ -O2 -fopenmp, debruijn.cpp (main renamed) and common.cpp, htslib headers only, unreferenced functions dropped by the linker"


def run_reference(ref_dir, reads, meta, regions, k, min_qual):
    """reads: [(seq, qual, flag)], meta: [(pos, end)], regions: [(planned, start, stop, ref_start, ref bytes, read_begin, read_end)]
    -> (per region (window, records), the printed lines, seconds)"""
    src = os.path.join(ref_dir, "dbg", "src")
    with tempfile.TemporaryDirectory(prefix="dbg_golden_") as tmp:
        with tarfile.open(os.path.join(ref_dir, "abea", "htslib.tar.bz2")) as tf:
            tf.extractall(tmp, members=[m for m in tf.getmembers() if "/htslib/" in m.name and m.name.endswith(".h")])
        hts = [d for d in os.listdir(tmp) if d.startswith("htslib")][0]
        open(os.path.join(tmp, "harness.cpp"), "w").write(HARNESS)
        flags = ["-O2", "-fopenmp", "-w", "-ffunction-sections", "-fdata-sections", "-I" + os.path.join(tmp, hts), "-I" + src]
        exe = os.path.join(tmp, "harness")
        subprocess.check_call(["g++"] + flags + [os.path.join(tmp, "harness.cpp"), os.path.join(src, "common.cpp"), "-Wl,--gc-sections", "-o", exe, "-lm"])
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(struct.pack("<iii", k, min_qual, len(reads)))
            for (seq, qual, flag), (pos, end) in zip(reads, meta):
                f.write(struct.pack("<iiii", pos, end, len(seq), flag) + seq + bytes(qual))
            f.write(struct.pack("<i", len(regions)))
            for planned, start, stop, ref_start, ref, b, e in regions:
                f.write(struct.pack("<iiiiiii", planned, start, stop, ref_start, len(ref), b, e) + ref)
        with open(os.path.join(tmp, "out.txt"), "wb") as txt:
            subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], stdout=txt, stderr=subprocess.DEVNULL)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
        lines = open(os.path.join(tmp, "out.txt"), "rb").read().split(b"\n")[:-1]
    out, at = [], 0
    for _ in regions:
        b, e, n = struct.unpack_from("<iii", raw, at); at += 12
        out.append(((b, e), np.frombuffer(raw, M.NODE, n, at).copy())); at += M.NODE.itemsize * n
    (seconds,) = struct.unpack_from("<d", raw, at)
    return out, [ln + b"\n" for ln in lines], seconds


def make_fixture():
    """-> (contig bytes, reads [(seq, qual, flag)], meta [(pos, end)])"""
    rng = np.random.default_rng(SEED)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    contig = bytearray(acgt[rng.integers(0, 4, CONTIG)].tobytes())
    contig[1200:1240] = b"A" * 40                               # a homopolymer: one node, one edge to itself
    contig[2600:2660] = b"CAG" * 20                             # a tandem repeat of three bases
    contig[4100:4104] = b"NNNN"                                 # the reference's own N count as letters
    x = b"GATTACAGGCTTACC"                                      # a 15-mer with five next letters in the reference: the fifth is dropped
    for j, nxt in enumerate(b"ACGTN"):
        contig[5000 + 40 * j:5000 + 40 * j + 16] = x + bytes([nxt])
    contig = bytes(contig)
    n_reads = CONTIG * 8 // 120
    pos = np.sort(rng.integers(0, CONTIG - 40, n_reads))
    reads, meta = [], []
    for r, p in enumerate(pos.tolist()):
        n = int(rng.integers(60, 151)) if r % 23 else int(rng.choice([10, 15, 16, 17, 18]))
        n = min(n, CONTIG - p)
        seq = np.frombuffer(contig[p:p + n], np.uint8).copy()
        err = rng.random(n) < 0.01
        seq[err] = acgt[rng.integers(0, 4, int(err.sum()))]
        if r % 17 == 3:                                         # an N at a random place
            seq[int(rng.integers(0, n))] = ord("N")
        if r % 29 == 5:                                         # IUPAC letters are ordinary letters
            seq[int(rng.integers(0, n))] = M.LETTERS[int(rng.integers(0, 15))]
        qual = rng.integers(25, 42, n).astype(np.uint8)
        low = rng.random(n) < 0.02
        qual[low] = rng.integers(2, 21, int(low.sum()))         # (20 passes, 19 does not)
        if r % 31 == 7:
            qual[:] = 93
        flag = (M.QC_FAIL | 16) if r % 37 == 11 else int(rng.choice([0, 16, 99, 147, 1024]))
        reads.append((seq.tobytes(), qual.tobytes(), flag))
        meta.append((p, p + n))
    return contig, reads, meta


def all_regions(contig, reads, meta):
    """the planner's regions of the whole contig, then constructed ones: empty graphs, a window that is given and not planned"""
    plan = M.plan_regions(0, CONTIG, [m[0] for m in meta], [m[1] for m in meta], CONTIG)
    regions = [(1, int(s), min(int(s) + M.REGION_SIZE, CONTIG), int(rs), contig[int(rs):int(rs) + int(rl)], int(b), int(e)) for s, rs, rl, b, e in plan]
    regions += [(0, 0, 0, 0, b"", 0, 0), (0, 0, 0, 100, contig[100:100 + K + 1], 3, 3),        # empty graphs: no reference edge, no read
                (0, 0, 0, 7, contig[7:7 + K + 2], 0, 0),                                       # the first length with an edge
                (0, 0, 0, 1190, contig[1190:1260], 40, 43), (0, 0, 0, 0, b"", 100, 102)]         # given windows; reads only
    return plan, regions


def census(regions, reads, recs, k, min_qual):
    c = dict.fromkeys(AT_LEAST, 0)
    c["regions"] = len(regions)
    used = np.zeros(len(reads), np.int64)
    for (_, _, _, _, ref, b, e), r in zip(regions, recs):
        c["empty_regions"] += len(r) == 0
        used[b:e] += 1
        c["colour3_nodes"] += int((r["colours"] == 3).sum())
        c["nodes_first_in_read"] += int((r["src_read"] >= 0).sum())
        c["nodes_with_4_edges"] += int((r["n_edges"] == 4).sum())
        c["self_loops"] += int(sum((rec["edge_to"][:rec["n_edges"]] == i).any() for i, rec in enumerate(r)))
        st = {}
        M.build_region(ref, 0, reads[b:e], k, min_qual, b, st)
        c["dropped_fifth"] += st["dropped"]
        for seq, qual, flag in reads[b:e]:
            if flag & M.QC_FAIL:
                c["qc_fail_reads"] += 1
                continue
            c["iupac_reads"] += any(ch not in b"ACGTN" for ch in seq)
            q = np.frombuffer(qual, np.uint8) < min_qual
            isn = np.frombuffer(seq, np.uint8) == ord("N")
            for i in range(M.occurrences(len(seq), k)):
                for what, bad in (("quality", q), ("n", isn)):
                    w = bad[i:i + k + 1]
                    if w.sum() == 1:
                        c[what + "_drop_first"] += bool(w[0]); c[what + "_drop_last"] += bool(w[-1])
    c["shared_reads"] = int((used >= 2).sum())
    return {k_: int(v) for k_, v in c.items()}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ref_dir = args[0] if args else "/root/reference/benchmarks"
    contig, reads, meta = make_fixture()
    plan, regions = all_regions(contig, reads, meta)
    got, lines, seconds = run_reference(ref_dir, reads, meta, regions, K, MIN_QUAL)
    assert len(lines) == len(regions)

    # the model is the reference: the planner's windows, every record of every region, every printed line
    docs = []
    for i, (reg, ((b, e), recs)) in enumerate(zip(regions, got)):
        planned, start, stop, ref_start, ref, rb, re_ = reg
        assert (b, e) == (rb, re_), f"region {i}: the planner's window {(rb, re_)}, the reference's {(b, e)}"
        mine = M.build_region(ref, ref_start, reads[b:e], K, MIN_QUAL, b)
        assert mine.tobytes() == recs.tobytes(), f"region {i}: the model's records differ from the reference's"
        assert M.format_region(ref, ref_start, reads, recs) == lines[i], f"region {i}: the printed line"
        docs.append({"nodes": len(recs), "edges": int(recs["n_edges"].sum()), "weight": int(recs["weight"].sum()), "sha256": hashlib.sha256(recs.tobytes()).hexdigest()})
    # ... and under another k and quality bound (no printed line: assembleReadsAndDetectVariants has its own constants)
    other = {}
    for k, mq in ((1, 20), (16, 3), (7, 30)):
        got2, _, _ = run_reference(ref_dir, reads, meta, regions, k, mq)
        for i, (reg, ((b, e), recs)) in enumerate(zip(regions, got2)):
            assert M.build_region(reg[4], reg[3], reads[b:e], k, mq, b).tobytes() == recs.tobytes(), f"k {k} min_qual {mq} region {i}"
        other[f"{k},{mq}"] = [hashlib.sha256(r.tobytes()).hexdigest() for _, r in got2]
    count = census(regions, reads, [r for _, r in got], K, MIN_QUAL)
    print(count)
    for k_, v in AT_LEAST.items():
        assert count[k_] >= v, f"{k_}: {count[k_]}, at least {v} needed"

    full = sorted([i for i, (_, r) in enumerate(got) if len(r)], key=lambda i: len(got[i][1]))[:FULL_REGIONS]
    npz = os.path.join(HERE, "dbg_small.npz")
    cat = lambda xs: np.frombuffer(b"".join(xs), np.uint8)
    G1.save_npz(npz, [("contig", np.frombuffer(contig, np.uint8)), ("seq", cat([r[0] for r in reads])), ("qual", cat([r[1] for r in reads])),
                      ("read_len", np.array([len(r[0]) for r in reads], np.int32)), ("read_flag", np.array([r[2] for r in reads], np.int32)),
                      ("read_pos", np.array([m[0] for m in meta], np.int32)), ("read_end", np.array([m[1] for m in meta], np.int32)),
                      ("plan", plan),
                      ("region", np.array([[p, s, t, rs, len(ref), b, e] for p, s, t, rs, ref, b, e in regions], np.int32)),
                      ("region_ref", cat([r[4] for r in regions]))])
    doc = {"fixture": "dbg_small.npz", "fixture_sha256": hashlib.sha256(open(npz, "rb").read()).hexdigest(), "seed": SEED, "k": K, "min_qual": MIN_QUAL,
           "reference_build": BUILD, "reference_graph_seconds": round(seconds, 5), "reference_host": "build host CPU, one thread",
           "counts": count, "regions": docs, "other_parameters": other,
           "full": {str(i): {"records": got[i][1].tobytes().hex(), "line": lines[i].decode()} for i in full}}
    old = os.path.join(HERE, "dbg_expected.json")
    if "--keep-times" in sys.argv and os.path.exists(old):
        doc["reference_graph_seconds"] = json.load(open(old))["reference_graph_seconds"]
    with open(old, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(regions)} regions, {sum(d['nodes'] for d in docs)} nodes by the reference; the three graph calls {seconds:.5f} s; {os.path.getsize(npz)} + {os.path.getsize(old)} bytes")


if __name__ == "__main__":
    main()
