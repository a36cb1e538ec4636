"""The golden fixture of tests/golden/make_dbg_golden.py as the dbg tests use it, and the constructed regions of tests/test_dbg_gpu.py:
the smallest inputs at which each rule of include/gab.h's dbg section can break.  Expected records are tests/dbg_model.py's."""
import functools
import hashlib
import json
import os

import numpy as np

from tests import dbg_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK = 256                 # threads of a work-group of dbg.hip: the ref loop's sweep
GROUP = 64                  # threads that walk one read


@functools.lru_cache(maxsize=None)
def fixture():
    """-> (expected json, regions [(ref, ref_start, read_begin, read_end)], reads [(seq, qual, flag)], the npz)"""
    doc = json.load(open(os.path.join(GOLDEN, "dbg_expected.json")))
    z = np.load(os.path.join(GOLDEN, "dbg_small.npz"))
    ln = z["read_len"].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(ln)])
    seq, qual = z["seq"].tobytes(), z["qual"].tobytes()
    reads = [(seq[off[j]:off[j + 1]], qual[off[j]:off[j + 1]], int(z["read_flag"][j])) for j in range(len(ln))]
    rr, refs = z["region"], z["region_ref"].tobytes()
    roff = np.concatenate([[0], np.cumsum(rr[:, 4].astype(np.int64))])
    regions = [(refs[roff[i]:roff[i + 1]], int(rr[i, 3]), int(rr[i, 5]), int(rr[i, 6])) for i in range(len(rr))]
    return doc, regions, reads, z


@functools.lru_cache(maxsize=None)
def fixture_model():
    """the model's (node_off, records, stats) of the fixture, computed once and shared; callers do not write into it"""
    doc, regions, reads, _ = fixture()
    stats = {}
    off, recs = M.build(regions, reads, doc["k"], doc["min_qual"], stats)
    recs.setflags(write=False); off.setflags(write=False)
    return off, recs, stats


def sha(records):
    return hashlib.sha256(np.ascontiguousarray(records).tobytes()).hexdigest()


def _rand(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def distinct_kmers(n, k=15):
    """a sequence of n + k - 1 letters whose n k-mers are all different: the letters of a counter in base 16, then checked"""
    rng = np.random.default_rng(n)
    while True:
        s = np.frombuffer(M.LETTERS[:15], np.uint8)[rng.integers(0, 15, n + k - 1)].tobytes()      # (no N: reads may carry it too)
        if len({s[i:i + k] for i in range(n)}) == n:
            return s


def q(n, v=30):
    return bytes([v]) * n


def constructed():
    """{name: (k, min_qual, regions, reads)}"""
    rng = np.random.default_rng(4242)
    c = {}
    for k in (1, 15, 16):
        base = _rand(rng, 400)
        # reference and read lengths 0, k, k + 1, k + 2 (the first with an edge), k + 3; one region each, then all reads in one region
        lens = (0, k, k + 1, k + 2, k + 3)
        reads = [(base[50:50 + n], q(n), 0) for n in lens]
        regions = [(base[:n], 10 * i, 0, 0) for i, n in enumerate(lens)] + [(b"", 0, j, j + 1) for j in range(len(lens))] + [(base[:k + 2], 7, 0, len(lens))]
        c[f"lengths_k{k}"] = (k, 20, regions, reads)
        # qualities 19 and 20 at base i and at base i + k of the only edge; N at base i + k only, and at base i only
        s = base[100:100 + k + 2]
        rd = []
        for at in (0, k):
            for v in (19, 20):
                qq = bytearray(q(k + 2)); qq[at] = v
                rd.append((s, bytes(qq), 0))
            sn = bytearray(base[100:100 + k + 3]); sn[at] = ord("N")      # (k + 3 bases: two edges, the N in one of them or in both)
            rd.append((bytes(sn), q(k + 3), 0))
        c[f"quality_and_n_k{k}"] = (k, 20, [(b"", 0, 0, len(rd))] + [(b"", 0, j, j + 1) for j in range(len(rd))], rd)
    k = 15
    base = _rand(rng, 600)
    c["qc_fail_between"] = (k, 20, [(base[:60], 100, 0, 3)], [(base[5:55], q(50), 0), (base[200:260], q(60), 512 | 16), (base[10:70], q(60, 41), 1024)])
    c["homopolymer"] = (k, 20, [(b"A" * 40, 5, 0, 3), (b"A" * (k + 2), 0, 0, 0), (b"", 0, 1, 2)], [(b"A" * 30, q(30, 25), 0), (b"A" * (k + 2), q(k + 2, 93), 0), (b"C" * 20 + b"A" * 20, q(40), 0)])
    c["tandem_repeat"] = (k, 20, [(b"CAG" * 20, 0, 0, 2)], [(b"AGC" * 15, q(45), 0), (b"CAG" * 10 + b"T" + b"CAG" * 6, q(49, 22), 0)])
    x = _rand(rng, k)
    fill = [_rand(rng, 20) for _ in range(6)]
    five = lambda order: b"".join(x + bytes([ch]) + f for ch, f in zip(order, fill))
    c["five_successors"] = (k, 20, [(five(b"ACGTN"), 0, 0, 0), (five(b"NTGCA"), 0, 0, 0), (five(b"ACGTNA"), 0, 0, 1), (five(b"ACG"), 0, 0, 2)],
                            [(x + b"T" + fill[0], q(k + 21), 0), (x + b"R" + fill[1], q(k + 21), 0)])
    iu = bytes(M.LETTERS[:15]) * 3
    c["iupac_reads"] = (k, 20, [(base[:40], 0, 0, 2)], [(iu, q(len(iu)), 0), (base[:20] + b"RYK=" + base[24:40], q(40), 0)])
    # a k-mer first seen in read 2 of region 0, and again in the reference of the NEXT region only
    novel = _rand(rng, 40)
    c["read_then_next_reference"] = (k, 20, [(base[:80], 0, 0, 3), (base[40:80] + novel, 40, 2, 4)],
                                     [(base[:50], q(50), 0), (base[20:70], q(50), 0), (base[60:80] + novel[:30], q(50), 0), (novel, q(40), 0)])
    # weights beyond 2^24: 700 homopolymer reads of 151 bases at quality 93 on one node (2 x 135 x 93 each)
    c["weight_above_2_24"] = (k, 20, [(b"G" * 151, 0, 0, 700)], [(b"G" * 151, q(151, 93), 0)] * 700)
    # table pressure: every k-mer different (there is one table form, so two sizes around a sweep of the work-group, and a large one)
    for n in (BLOCK - 1, BLOCK + 1, 6000):
        s = distinct_kmers(n + 1)
        c[f"all_distinct_{n}"] = (k, 20, [(s[:len(s) // 2 + k], 0, 0, 1)], [(s, q(len(s)), 0)])
    # launch and lane edges: occurrence counts around 64 (a read's group), 256 (the work-group) and 512 (two sweeps); an empty region between two full ones
    long = _rand(rng, 700)
    edge_regions, edge_reads = [], []
    for n in (GROUP - 1, GROUP, GROUP + 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1):
        edge_reads.append((long[3:3 + n + k + 1], q(n + k + 1), 0))
        edge_regions += [(long[:n + k + 1], 0, 0, 0), (b"", 0, len(edge_reads) - 1, len(edge_reads))]
    edge_regions.insert(5, (b"", 9, 0, 0))
    c["lane_edges"] = (k, 20, edge_regions, edge_reads)
    c["one_region"] = (k, 20, [(long[:300], 1000, 0, 2)], [(long[10:160], q(150), 0), (long[100:250], q(150, 20), 0)])
    # the key that is all ones (sixteen N at k = 16) has a slot of its own; its neighbours do not
    c["all_ones_key"] = (16, 20, [(b"N" * 20 + b"B" * 20 + b"N" * 18, 0, 0, 1)], [(b"B" * 40, q(40), 0)])
    return c


def many_regions(n=70000):
    """more regions than a 16-bit grid dimension: tiny ones, three shapes in turn"""
    k = 15
    ref = b"ACGTTGCAAGCTTAGCATCAGT"
    reads = [(ref[2:], q(len(ref) - 2), 0), (b"ACGTNGCAAGCTTAGCATCAGT", q(22, 40), 0)]
    shapes = [(ref, 5, 0, 1), (b"", 0, 0, 2), (ref[:k + 2], 0, 1, 1)]
    return k, 20, [shapes[i % 3] for i in range(n)], reads
