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


# ---------------------------------------------------------------- bpm: a CPU model of the GPU cascade (genarchbench_amd/csrc/bpm.hip)
# A pair with W = ceil(plen / 64) <= 4 is scored by bpm_score32<D> (or bpm_score<W>), which finishes it when both strings are
# upper-case ACGT; the others go to bpm_band<D> (8 rows around the diagonal per column), from there to bpm_win<W> (64 rows) when the
# backtrace leaves the band, and to bpm_full<W> (complete columns) when it leaves the window.  W > 4: bpm_full<0> only.
BPM_STAGES = ("score", "band", "window", "full", "generic")
_BPM_CODE = {ord("A"): 0, ord("a"): 0, ord("C"): 1, ord("c"): 1, ord("G"): 2, ord("g"): 2, ord("T"): 3, ord("t"): 3}   # else 4


def bpm_band_start(col, cshift, W):
    """first of the 8 rows bpm_band keeps of column `col` (its start())"""
    return min(max(col + cshift - 4, 0), 64 * W - 8)


def bpm_win_start(col, cshift, W):
    """first of the 64 rows bpm_win keeps of column `col` (bpm_win_start<W>)"""
    return min(max(col + cshift - 32, 0), 64 * W - 64)


def bpm_model(p, t):
    """one pair (bytes, len(t) <= len(p), the driver's swap applied) -> (printed score, stage that finishes it, block steps).

    The columns are Myers' Pv / Mv as ONE Python integer each, advanced from the reference's 64-row match masks: one flat table of
    4 words per block plus one, where code 4 (not ACGT/acgt) of block b lands on code 0 of block b + 1 and that of the last block on
    the extra word (oracle/bpm.c).  The backtrace is the reference's (edit_bpm.c:289-313): Pv of column h + 1, then Mv of column h,
    else a diagonal step that counts when the raw bytes differ.  The stage is the first one whose rows hold every step of that walk
    (both columns of a step, the kernels' miss checks); the steps are tlen x W per stage passed (tlen x W once for W > 4)."""
    n, m = len(p), len(t)
    assert 1 <= n and 0 <= m <= n
    W = (n + 63) // 64
    flat = [0] * (4 * W + 1)
    for i, ch in enumerate(p):
        flat[(i >> 6) * 4 + _BPM_CODE.get(ch, 4)] |= 1 << (i & 63)
    if n & 63:                                        # rows n .. 64W - 1 match every code 0..3 (edit_bpm.c:106-113)
        pad = ((1 << 64) - 1) & ~((1 << (n & 63)) - 1)
        for c in range(4):
            flat[(W - 1) * 4 + c] |= pad
    eq = [sum(flat[b * 4 + c] << (64 * b) for b in range(W)) for c in range(5)]
    full = (1 << (64 * W)) - 1
    P, M = full, 0
    Pc, Mc = [P], [M]
    for ch in t:
        Eq = eq[_BPM_CODE.get(ch, 4)]
        Xv = Eq | M
        Xh = ((((Eq & P) + P) ^ P) | Eq) & full
        Ph = M | (~(Xh | P) & full)
        Mh = P & Xh
        Ph = ((Ph << 1) | 1) & full
        Mh = (Mh << 1) & full
        P = Mh | (~(Xv | Ph) & full)
        M = Ph & Xv
        Pc.append(P); Mc.append(M)
    cshift = (n - m) // 2
    in_band = in_win = True
    ops, v, h = 0, n - 1, m - 1
    while v >= 0 and h >= 0:
        if in_band:
            r1, rh = bpm_band_start(h + 1, cshift, W), bpm_band_start(h, cshift, W)
            in_band = r1 <= v < r1 + 8 and rh <= v < rh + 8
        if in_win:
            r1, rh = bpm_win_start(h + 1, cshift, W), bpm_win_start(h, cshift, W)
            in_win = r1 <= v < r1 + 64 and rh <= v < rh + 64
        if Pc[h + 1] >> v & 1:
            ops += 1; v -= 1
        elif Mc[h] >> v & 1:
            ops += 1; h -= 1
        else:
            ops += t[h] != p[v]; h -= 1; v -= 1
    score = -(ops + (h + 1) + (v + 1))
    if W > 4:
        return score, "generic", m * W
    if set(p) <= set(b"ACGT") and set(t) <= set(b"ACGT"):
        return score, "score", m * W
    stage = "band" if in_band else "window" if in_win else "full"
    return score, stage, m * W * (BPM_STAGES.index(stage) + 1)


def bpm_model_batch(batch):
    """bpm_model over a PairBatch (identical pairs computed once) -> (scores int32, stages list, block steps)"""
    memo = {}
    scores = np.empty(batch.n, np.int32)
    stages = []
    steps = 0
    for i in range(batch.n):
        pt = batch.pair(i)
        r = memo.get(pt)
        if r is None:
            r = memo[pt] = bpm_model(*pt)
        scores[i] = r[0]; stages.append(r[1]); steps += r[2]
    return scores, stages, steps


def bpm_census(batch, stages):
    """per W class (0 = W > 4), what GAB_BPM_TRACE reports: {cls: (pairs, queued by the score stage, band misses, window misses)}"""
    out = {}
    for n, st in zip(batch.pat_len.tolist(), stages):
        W = (n + 63) // 64
        c = W if W <= 4 else 0
        a = out.setdefault(c, [0, 0, 0, 0])
        a[0] += 1
        a[1] += st in ("band", "window", "full")
        a[2] += st in ("window", "full")
        a[3] += st == "full"
    return {c: tuple(a) for c, a in out.items()}


def parse_bpm_trace(text):
    """GAB_BPM_TRACE lines of ONE call -> (census {cls: (pairs, queued, band misses, window misses)}, [(stage, cls, slice or -1, kernel), ...] launched)"""
    census, launches = {}, []
    for line in text.splitlines():
        m = re.match(r"\[gab_bpm\] class (\d+) pairs (\d+) queued (\d+) band_miss (\d+) window_miss (\d+)", line)
        if m:
            census[int(m.group(1))] = tuple(int(x) for x in m.group(2, 3, 4, 5))
            continue
        m = re.match(r"\[gab_bpm\] (score|band|window|full) class (\d+) (?:slice (\d+) )?.*kernel (\S+)$", line)
        if m:
            launches.append((m.group(1), int(m.group(2)), int(m.group(3) or -1), m.group(4)))
    return census, launches


def _bpm_acgt(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def bpm_handmade_pairs():
    """pairs built to sit right at the cascade's miss checks -> [(pattern, text, stage it was built for)].

    Each is a random ACGT pattern with ONE unclean base (N, or a lower-case letter) and a text that is the pattern with a run of k
    bases deleted (the walk runs k rows above the diagonal; cshift = k / 2 centres the band: k <= 6 stays in the 8-row band, k <= 62
    in the 64-row window) or inserted (k rows below it, cshift = 0: k <= 3 band, k <= 31 window; a deletion of k at the far end
    keeps tlen = plen).  Class 1's window is all 64 rows: nothing of it reaches bpm_full<1>."""
    out = []

    def mark(p, at, ch=b"N"):
        return p[:at] + ch + p[at + 1:]

    def deletion(n, at, k, mk, ch=b"N", seed=0):
        p = mark(_bpm_acgt(n, seed), mk, ch)
        return p, p[:at] + p[at + k:]

    def insertion(n, at, k, mk, ch=b"N", seed=0, gap=None):
        # k bases inserted into the text at `at`, k deleted from it `gap` bases further on (default: at the far end)
        p = mark(_bpm_acgt(n, seed), mk, ch)
        b = n - k if gap is None else at + gap
        return p, p[:at] + _bpm_acgt(k, seed + 1) + p[at:b] + p[b + k:]

    for W in (1, 2, 3, 4):
        for n in sorted({64 * W, 64 * W - 5, 64 * W - 31, 64 * W - 32, 64 * (W - 1) + 1} - {0}):
            if n < 24:
                continue
            at = n // 2
            for k, st in ((6, "band"), (7, "window")):
                out.append((*deletion(n, at, k, n // 5, seed=n + k), st))
                out.append((*deletion(n, at, k, n - 1, b"g", seed=n + k + 100), st))
            for k, st in ((3, "band"), (4, "window")):
                out.append((*insertion(n, at, k, n // 5, seed=n + k + 200), st))
            if n >= 96:
                for k, st in ((62, "window"), (63, "full")):
                    out.append((*deletion(n, (n - k) // 2, k, 3, seed=n + k + 300), st))
            if n >= 160:            # (the first seed whose edit distance is the 2k indels, not fewer chance substitutions)
                for k, st in ((31, "window"), (32, "full")):
                    seed = n + k + 400
                    while -bpm_model(*insertion(n, 4, k, n - 3, b"C", seed=seed, gap=n - 2 * k - 8))[0] != 2 * k:
                        seed += 1
                    out.append((*insertion(n, 4, k, n - 3, b"c", seed=seed, gap=n - 2 * k - 8), st))
    # tlen 0 and 1, tlen << plen; the band clamp at row 0 holds the walk of (8, 1): its column 0 alone would start at row -1
    p = _bpm_acgt(256, 7)
    for n in (1, 8, 9, 64, 65, 200, 256):
        out.append((mark(p[:n], n // 2), b"", "band"))
    out.append((mark(p[:8], 2), p[7:8], "band"))
    out.append((mark(p[:9], 2), p[8:9], "window"))
    out.append((mark(p[:60], 2, b"a"), p[58:60], "window"))
    out.append((mark(p[:200], 2), p[190:200], "full"))
    out.append((mark(p[:256], 2), p[255:256], "full"))
    # N / lower-case on both sides of every 64-row block boundary and in the last block (code 4 of a block aliases onto the next
    # block's 'A' mask), two deleted bases: band
    for n in (256, 200):
        for mk in sorted({63, 64, 127, 128, 191, 192, n - 1, n - 2} & set(range(n))):
            for ch in (b"N", b"t"):
                q = mark(_bpm_acgt(n, 900 + mk), mk, ch)
                out.append((q, q[:n // 3] + q[n // 3 + 2:], "band"))
    return out


def bpm_model_steps(batch):
    """the block steps of bpm_model_batch(batch) alone: clean pairs of W <= 4 and pairs of W > 4 step tlen x W once and need no
    model run (cleanliness from the slabs with numpy), the others go through bpm_model"""
    def unclean(slab, off, ln):
        bad = np.ones(256, bool)
        bad[np.frombuffer(b"ACGT", np.uint8)] = False
        c = np.concatenate([[0], np.cumsum(bad[slab])])
        return (c[off + ln] - c[off]) > 0
    pl, tl = batch.pat_len.astype(np.int64), batch.txt_len.astype(np.int64)
    W = (pl + 63) // 64
    steps = int((tl * W).sum())
    memo = {}
    for i in np.flatnonzero((unclean(batch.pat, batch.pat_off, pl) | unclean(batch.txt, batch.txt_off, tl)) & (W <= 4)).tolist():
        pt = batch.pair(i)
        if pt not in memo:
            memo[pt] = bpm_model(*pt)[2]
        steps += memo[pt] - int(tl[i] * W[i])
    return steps
