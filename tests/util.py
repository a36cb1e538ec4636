"""helpers shared by the tests: golden-vector readers for the reference's text formats"""
import os
import re

import numpy as np

from tools import gabgen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def read_bsw_input(path):
    """reference bsw input format (bsw/src/main_banded.cpp:152-206): h0 / ref digits / query digits"""
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    n = len(lines) // 3
    refs, qrys, h0s = [], [], []
    for i in range(n):
        h0s.append(int(lines[3 * i]))
        refs.append(np.frombuffer(lines[3 * i + 1], np.uint8) - 48)
        qrys.append(np.frombuffer(lines[3 * i + 2], np.uint8) - 48)
    return gabgen.bsw_from_arrays(refs, qrys, h0s)


def read_scores(path):
    """'[i] score=s' lines -> int32 array indexed by i"""
    out = {}
    for line in open(path):
        m = re.match(r"\[(\d+)\] score=(-?\d+)", line)
        if m:
            out[int(m.group(1))] = int(m.group(2))
    return np.array([out[i] for i in range(len(out))], np.int32)


def live(name):
    """an array of tests/golden/live.npz: the reference's outputs for the inputs of the test_*_matches_live_reference tests
    (make_golden.py live)"""
    with np.load(os.path.join(GOLDEN, "live.npz")) as z:
        return z[name]


def read_bsw_full(path):
    """'[i] score qle tle gtle gscore max_off' lines (oracle/ref_harness/bsw_full_ref.cpp) -> int32 [n, 6]"""
    rows = [[int(v) for v in line.split()[1:]] for line in open(path) if line.startswith("[")]
    return np.array(rows, np.int32).reshape(-1, 6)


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def read_chain_output(path):
    """reference chain output (chain/src/host_data_io.cpp:53-60): n / score<TAB>parent x n / EOR"""
    sc, pa = [], []
    for line in open(path):
        f = line.split()
        if len(f) == 2:
            sc.append(int(f[0])); pa.append(int(f[1]))
    return np.array(sc, np.int32), np.array(pa, np.int32)


def read_cigars(path):
    """'id=N CIGAR' lines -> list indexed by id"""
    out = {}
    for line in open(path):
        m = re.match(r"id=(\d+) (\S*)", line)
        if m:
            out[int(m.group(1))] = m.group(2)
    return [out[i] for i in range(len(out))]


def read_fasta_codes(path):
    seq = b"".join(l.strip() for l in open(path, "rb") if not l.startswith(b">"))
    lut = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
    return lut[np.frombuffer(seq, np.uint8)]


def read_fastq_reads(path):
    """FASTQ -> ReadBatch the way fmi.cpp:121-151 encodes it (row stride = longest read, A C G T -> 0..3, else 4)"""
    lines = open(path, "rb").read().split(b"\n")
    seqs = [lines[i] for i in range(1, len(lines), 4) if i < len(lines) and lines[i - 1].startswith(b"@")]
    lut = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
    stride = max(len(s) for s in seqs)
    enc = np.full((len(seqs), stride), 4, np.uint8)
    for r, s in enumerate(seqs):
        enc[r, :len(s)] = lut[np.frombuffer(s, np.uint8)]
    return gabgen.ReadBatch(enc, np.array([len(s) for s in seqs], np.int32))


# ---------------------------------------------------------------- bsw off the driver's default parameters
# (a, b, ambig, o_del, e_del, o_ins, e_ins, zdrop, end_bonus, w): the score matrix is bwa_fill_scmat(a, b, ambig)
# (main_banded.cpp:94-102).  tests/golden/bsw_params.npz holds the reference's scalarBandedSWA result for each set, in this
# order (make_golden.py params).
BSW_PARAM_SETS = [
    (1, 4, -1, 6, 1, 6, 1, 100, 5, 100),          # the driver's defaults
    (2, 3, -2, 5, 2, 5, 2, 50, 30, 30),
    (1, 1, 0, 0, 1, 0, 1, 0, 5, 100),             # o = 0, zdrop = 0 (no z-drop exit)
    (3, 5, -1, 7, 3, 8, 3, 200, 5, 5),
    (1, 4, -1, 6, 1, 7, 1, 100, 5, 100),          # o_ins != o_del
    (4, 1, -1, 2, 1, 9, 2, 10, 0, 100),
    (1, 4, -1, 6, 1, 6, 1, 1, -5, 100),           # zdrop = 1, negative end_bonus
    (1, 4, -1, 6, 1, 6, 1, 100, 50, 0),           # w = 0
    (0, 4, -1, 6, 1, 6, 1, 100, 5, 100),          # no positive score (max_sc = 0)
    (5, 9, -3, 11, 2, 3, 4, 30, -20, 17),
    (1, 4, -1, 6, 1, 6, 1, 100, 5, 2000),         # w beyond every length
    (2, 4, 2, 6, 1, 6, 1, 100, 5, 100),           # N scores positive
    (-2, 3, -1, 6, 1, 6, 1, 100, 5, 100),         # every score negative
    (127, 4, -1, 6, 1, 6, 1, 100, 5, 100),        # the largest int8 match score
    (1, 128, -1, 6, 1, 6, 1, 100, 5, 100),        # mismatch score -128
    (127, 128, -128, 20, 3, 25, 2, 500, 10, 50),
    (1, 4, -1, 6, 1, 6, 1, 100, -1000, 100),      # end_bonus so negative that the band clamp leaves w = 1
    (1, 4, -1, 6, 1, 6, 1, 100, 5000, 100),       # large end_bonus
    (2, 3, -1, 1000, 200, 900, 300, 100, 5, 100),  # gaps far above any score
    (1, 4, -1, 0, 1, 0, 1, 1, 5, 0),              # o = 0, zdrop = 1, w = 0 together
]


def bsw_handmade_pairs():
    """hand-made pairs: N (code 4) in one or both sequences, perfect matches ending on the last row / column, a 1-base query
    against a 2047-base reference, a 1-base reference -> (refs, qrys, h0s)"""
    acgt = [k % 4 for k in range(0, 997, 7)]                           # 143 bases, no repeat of period < 4
    A = lambda x: np.array(x, np.uint8)
    refs, qrys, h0s = [], [], []

    def add(r, q, h):
        refs.append(A(r)); qrys.append(A(q)); h0s.append(h)

    add(acgt[:60], acgt[:60], 20)                                      # perfect match
    add(acgt[:60] + [4] * 5, acgt[:60], 20)                            # ... and an N tail on the reference
    add([4] * 40, [4] * 40, 30)                                        # N against N
    add(acgt[:50], [4 if k % 5 == 0 else c for k, c in enumerate(acgt[:50])], 15)        # N in the query
    add([4 if k % 7 == 3 else c for k, c in enumerate(acgt[:80])], acgt[:80], 15)       # N in the reference
    add([4 if k % 3 == 0 else c for k, c in enumerate(acgt[:90])],
        [4 if k % 4 == 1 else c for k, c in enumerate(acgt[:90])], 40)                   # N in both
    add(acgt[:30] + [4] * 10 + acgt[30:70], acgt[:30] + acgt[30:70], 25)                # N block = deletion
    add(acgt[:30] + acgt[30:70], acgt[:30] + [4] * 10 + acgt[30:70], 25)                # N block = insertion
    add([(k * 5) % 4 for k in range(2047)], [1], 3)                    # qlen 1, tlen at the harness's limit
    add([2], acgt[:100], 60)                                           # tlen 1
    add(acgt[:143], acgt[:143], 0)                                     # h0 = 0: never extends
    add(acgt[:143], acgt[:143], 1)
    add([3 - c for c in acgt[:120]], acgt[:120], 50)                   # no similarity
    add(acgt[:100] + [(k * 3) % 4 for k in range(400)], acgt[:100], 10)  # long tail behind the match
    return refs, qrys, h0s


def bsw_param_input():
    """the pairs tests/golden/bsw_params.npz is computed on: 1 024 adversarial generator pairs (mode 1, seed 995), 256 read-like
    ones (mode 0, seed 996) and the hand-made pairs, in this order"""
    refs, qrys, h0s = [], [], []
    for seed, n, mode in ((995, 1024, 1), (996, 256, 0)):
        b = gabgen.bsw(seed, n, mode)
        for i in range(b.n):
            r, q, h = b.pair(i)
            refs.append(r); qrys.append(q); h0s.append(h)
    hr, hq, hh = bsw_handmade_pairs()
    return gabgen.bsw_from_arrays(refs + hr, qrys + hq, h0s + hh)


def bsw_full_ref_params_line(a, b, ambig, o_del, e_del, o_ins, e_ins, zdrop, end_bonus, w):
    """the stderr line oracle/ref_harness/bsw_full_ref.cpp prints when it takes these parameters: a harness built before it took
    parameters prints nothing and computes the driver's defaults whatever it is given"""
    return (f"bsw_full_ref: a={a} b={b} ambig={ambig} o_del={o_del} e_del={e_del} o_ins={o_ins} e_ins={e_ins} zdrop={zdrop} "
            f"end_bonus={end_bonus} w={w}")


def bsw_oracle_params(a, b, ambig, o_del, e_del, o_ins, e_ins, zdrop, end_bonus, w):
    """pyoracle.BswParams of one BSW_PARAM_SETS entry"""
    from oracle import pyoracle
    p = pyoracle.bsw_params(a, b, o_del, e_del, ambig, zdrop, end_bonus, w)
    p.o_ins, p.e_ins = o_ins, e_ins
    return p
