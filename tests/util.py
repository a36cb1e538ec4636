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
    """first of the 8 rows bpm_band keeps of column `col` (bpm_rows_start<8, W>)"""
    return min(max(col + cshift - 4, 0), 64 * W - 8)


def bpm_win_start(col, cshift, W):
    """first of the 64 rows bpm_win keeps of column `col` (bpm_rows_start<64, W>)"""
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


BPM_TRIP_EDGE_TLEN = 70      # text lengths 0 .. 70: every boundary of the 32-, 16- and 4-base trips of the text walk up to 64 + 6


def bpm_trip_edge_pairs():
    """for every text length m in 0 .. BPM_TRIP_EDGE_TLEN one pair per stage -> [(pattern, text, stage built for, stage by bpm_model)].

    A random ACGT pattern of m + k bases and, as text, the pattern with k bases deleted at (n - k) // 2: k = 2 and clean for the score
    stage; with the last pattern base an N, k = 2 stays in the 8-row band, k = 20 leaves it for the window, k = 70 leaves the window
    too (classes 2 and 3).  For W > 4 a 260-base pattern with its m-base prefix as text.  At m = 0 the walk is empty, so the unclean
    pairs all end in the band: the last element is what the model says, not what the pair was built for."""
    out = []
    for m in range(BPM_TRIP_EDGE_TLEN + 1):
        for j, (k, unclean, built_for) in enumerate(((2, False, "score"), (2, True, "band"), (20, True, "window"), (70, True, "full"))):
            n = m + k
            p = _bpm_acgt(n, 7000 + 100 * j + m)
            if unclean:
                p = p[:-1] + b"N"
            at = (n - k) // 2
            t = p[:at] + p[at + k:]
            out.append((p, t, built_for, bpm_model(p, t)[1]))
        p = _bpm_acgt(260, 7400 + m)
        out.append((p, p[:m], "generic", bpm_model(p, p[:m])[1]))
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


# ---------------------------------------------------------------- wfa: a CPU model of the GPU cascade (genarchbench_amd/csrc/wfa.hip)
# A pair is finished by the first launch whose limits hold its wavefront history.  The model runs the forward recurrence of gap-affine
# WFA (no backtrace) on a whole batch at once -- one numpy array of diagonals per score, a row per pair -- and keeps, per pair, what the
# limits are about: the final score, the number of scores that have a wavefront, the offsets allocated up to the final score, the
# largest M offset and the work count (cells computed + bases matched).  Which launches a call makes and what each can hold is restated
# from the host code by wfa_plan; wfa_tier_of puts the two together.
WFA_NULL = -10
WFA_LDS_MAX_LEN = 2040                    # longer sequences go straight to wfa_global
WFA_OFFB_MAX, WFA_OFFB_SAFE = 245, 240    # one-byte offsets: the largest value, and the M offset above which a byte tier gives up


def wfa_rows(pen, max_rows=240, max_score=1024, table=True):
    """the row table of complete mode: [(score, lo, hi, has I / D, used_end)] per score that has a wavefront, from the penalties alone.
    lo / hi grow by one around the sources' range, M takes hi - lo + 1 offsets and I and D as many each when a gap source exists.
    table=True stops where gab_wfa_create's table does (240 rows, score 1 024, 60 000 offsets, 120 diagonals to either side);
    table=False goes on to max_score: the history every kernel allocates, whatever holds it."""
    x, o, e = pen
    oe = o + e
    ent = {0: (0, 0, False)}
    rows = [(0, 0, 0, False, 1)]
    used = 1
    for sc in range(1, max_score + 1):
        if table and len(rows) >= max_rows:
            break
        ms, mg, ie = ent.get(sc - x), ent.get(sc - oe), ent.get(sc - e)
        if ie is not None and not ie[2]:
            ie = None
        src = [s for s in (ms, mg, ie) if s is not None]
        if not src:
            continue
        lo, hi = min([s[0] for s in src] + [1] * (len(src) < 3)) - 1, max([s[1] for s in src] + [-1] * (len(src) < 3)) + 1
        gap = mg is not None or ie is not None
        used += (hi - lo + 1) * (3 if gap else 1)
        if table and (used > 60000 or lo < -120 or hi > 120):
            break
        ent[sc] = (lo, hi, gap)
        rows.append((sc, lo, hi, gap, used))
    return rows


def _wfa_pad(seqs, fill, left, right):
    """[n, left + longest + right] uint8: the sequences behind `left` bytes of `fill`, `fill` behind them"""
    out = np.full((len(seqs), left + max([len(s) for s in seqs] + [0]) + right), fill, np.uint8)
    for i, s in enumerate(seqs):
        out[i, left:left + len(s)] = np.frombuffer(s, np.uint8)
    return out


def wfa_model(pats, txts, pen, reduction=None):
    """lists of patterns and texts (bytes) -> dict of int64 arrays, one entry per pair:
      score  the final score
      rows   the scores up to it that have a wavefront (the final one's index in wfa_rows is rows - 1)
      used   the offsets allocated up to it: 1 for score 0, then width x (1 + has I + has D) per wavefront, the width from the
             (reduced) lo / hi of the sources
      max_m  the largest M offset after extension, over every diagonal computed
      work   sum of the widths computed + bases matched by the extensions
    A single pair may be given as two bytes objects.  The strings behave as if padded with 'X' (pattern) and 'Y' (text); a missing
    source reads as offset -10; reduction = (min_wavefront_length, max_distance_threshold) drops, after each extension, the outer
    diagonals whose distance to the end lags more than the threshold behind the best one (never diagonal tlen - plen's side)."""
    if isinstance(pats, (bytes, bytearray)):
        r = wfa_model([bytes(pats)], [bytes(txts)], pen, reduction)
        return {k: int(v[0]) for k, v in r.items()}
    x, o, e = pen
    oe = o + e
    n = len(pats)
    out = {k: np.zeros(n, np.int64) for k in ("score", "rows", "used", "max_m", "work")}
    if n == 0:
        return out
    longest = np.array([max(len(p), len(t)) for p, t in zip(pats, txts)])
    if longest.max() > 512 and longest.min() <= 512:        # a few long pairs among short ones: apart, or every row is padded to them
        for part in (np.flatnonzero(longest <= 512), np.flatnonzero(longest > 512)):
            r = wfa_model([pats[i] for i in part], [txts[i] for i in part], pen, reduction)
            for k in out:
                out[k][part] = r[k]
        return out
    PAD = 40
    P, T = _wfa_pad(pats, ord("X"), PAD, PAD), _wfa_pad(txts, ord("Y"), PAD, PAD)
    ids = np.arange(n)
    plen = np.array([len(p) for p in pats], np.int64); tlen = np.array([len(t) for t in txts], np.int64)
    ak = tlen - plen
    R = 8                                              # diagonals -R .. R are column k + R of the arrays
    NEG = np.iinfo(np.int64).min // 2
    used = np.ones(n, np.int64); nrows = np.ones(n, np.int64); work = np.zeros(n, np.int64); max_m = np.full(n, NEG, np.int64)

    def blank(m):
        return np.full((m, 2 * R + 1), WFA_NULL, np.int64)

    def extend(Mw, lo, hi):
        """extend every diagonal lo .. hi of Mw in place -> bases matched per pair"""
        kk = np.arange(-R, R + 1)
        rr, cc = np.nonzero((kk[None, :] >= lo[:, None]) & (kk[None, :] <= hi[:, None]))
        off = Mw[rr, cc]
        start = off.copy()
        live = np.arange(len(rr))
        L = 4
        while len(live):
            r_, o_ = rr[live], off[live]
            j = np.arange(L)
            v = np.clip(o_ - kk[cc[live]] + PAD, 0, P.shape[1] - 1)[:, None] + j
            h = np.clip(o_ + PAD, 0, T.shape[1] - 1)[:, None] + j
            eq = P[r_[:, None], np.minimum(v, P.shape[1] - 1)] == T[r_[:, None], np.minimum(h, T.shape[1] - 1)]
            run = np.where(eq.all(1), L, eq.argmin(1))
            off[live] += run
            live = live[run == L]
            L = 16
        Mw[rr, cc] = off
        return np.bincount(rr, off - start, len(Mw)).astype(np.int64)

    # per score that has a wavefront: [M, I, D, lo, hi, has gap], rows = the pairs still running
    M0 = blank(n); M0[:, R] = 0
    hist = {0: [M0, None, None, np.zeros(n, np.int64), np.zeros(n, np.int64), False]}
    score = 0
    while True:
        cur = hist.get(score)
        if cur is not None:
            Mw, _, _, lo, hi, _ = cur
            work += extend(Mw, lo, hi)
            m = len(Mw)
            kk = np.arange(-R, R + 1)[None, :]
            inr = (kk >= lo[:, None]) & (kk <= hi[:, None])
            max_m = np.maximum(max_m, np.where(inr, Mw, NEG).max(1))
            at_ak = np.where((lo <= ak) & (ak <= hi), Mw[np.arange(m), np.clip(ak + R, 0, 2 * R)], WFA_NULL)
            done = at_ak >= tlen
            if reduction is not None:
                min_len, max_dist = reduction
                dist = np.maximum(plen[:, None] - (Mw - kk), tlen[:, None] - Mw)
                min_d = np.minimum(np.where(inr, dist, np.iinfo(np.int64).max).min(1), np.maximum(plen, tlen))
                good = inr & (dist - min_d[:, None] <= max_dist)
                big = 4 * R
                top = np.minimum(ak - 1, hi)
                first = np.where(good & (kk < top[:, None]), kk, big).min(1)          # first good diagonal below top
                nlo = np.where(first < big, first, np.maximum(top, lo))
                bottom = np.maximum(ak + 1, nlo)
                last = np.where(good & (kk > bottom[:, None]), kk, -big).max(1)
                nhi = np.where(last > -big, last, np.minimum(bottom, hi))
                apply = (hi - lo + 1 >= min_len) & ~done
                nlo, nhi = np.where(apply, nlo, lo), np.where(apply, nhi, hi)
                drop = inr & ((kk < nlo[:, None]) | (kk > nhi[:, None]))
                for w in cur[:3]:
                    if w is not None:
                        w[drop] = WFA_NULL
                cur[3], cur[4] = lo, hi = nlo, nhi
            if done.any():
                fin = ids[done]
                out["score"][fin] = score; out["rows"][fin] = nrows[done]; out["used"][fin] = used[done]
                out["max_m"][fin] = max_m[done]; out["work"][fin] = work[done]
                keep = ~done
                ids, plen, tlen, ak = ids[keep], plen[keep], tlen[keep], ak[keep]
                used, nrows, work, max_m = used[keep], nrows[keep], work[keep], max_m[keep]
                P, T = P[keep], T[keep]
                for ent in hist.values():
                    for q in range(5):
                        if ent[q] is not None:
                            ent[q] = ent[q][keep]
                if len(ids) == 0:
                    return out
        score += 1
        for old in [s for s in hist if s < score - max(x, oe, e)]:
            del hist[old]
        ms, mg, ie = hist.get(score - x), hist.get(score - oe), hist.get(score - e)
        if ie is not None and not ie[5]:
            ie = None
        if ms is None and mg is None and ie is None:
            continue
        m = len(ids)
        # (a missing source counts as the empty range lo = 1, hi = -1: it matters once a reduction has pushed lo above 1)
        lo = np.minimum.reduce([s[3] if s is not None else np.ones(m, np.int64) for s in (ms, mg, ie)]) - 1
        hi = np.maximum.reduce([s[4] if s is not None else -np.ones(m, np.int64) for s in (ms, mg, ie)]) + 1
        if max(int(-lo.min()), int(hi.max())) + 1 > R:           # more diagonals: re-centre the history
            grow = R
            for ent in hist.values():
                for q in range(3):
                    if ent[q] is not None:
                        ent[q] = np.pad(ent[q], ((0, 0), (grow, grow)), constant_values=WFA_NULL)
            R += grow
            ms, mg, ie = hist.get(score - x), hist.get(score - oe), hist.get(score - e)
            if ie is not None and not ie[5]:
                ie = None
        kk = np.arange(-R, R + 1)[None, :]
        inr = (kk >= lo[:, None]) & (kk <= hi[:, None])
        gap = mg is not None or ie is not None
        # the sources hold -10 outside their (reduced) ranges, so a shifted read is the range-checked read
        best = np.full((m, 2 * R + 1), WFA_NULL, np.int64)
        if ms is not None:
            in_ms = (kk >= ms[3][:, None]) & (kk <= ms[4][:, None])
            best = np.where(in_ms, ms[0] + 1, WFA_NULL)
        Iw = Dw = None
        if gap:
            null = blank(m)
            mgm = mg[0] if mg is not None else null
            iei = ie[1] if ie is not None else null
            ied = ie[2] if ie is not None else null
            Iw = blank(m); Dw = blank(m)
            Iw[:, 1:] = np.maximum(mgm[:, :-1], iei[:, :-1]) + 1           # from diagonal k - 1
            Iw[:, 0] = WFA_NULL + 1
            Dw[:, :-1] = np.maximum(mgm[:, 1:], ied[:, 1:])                # from diagonal k + 1
            best = np.maximum(best, np.maximum(Iw, Dw))
            Iw[~inr] = WFA_NULL; Dw[~inr] = WFA_NULL
        best[~inr] = WFA_NULL
        width = hi - lo + 1
        used += width * (3 if gap else 1)
        work += width
        nrows += 1
        hist[score] = [best, Iw, Dw, lo, hi, gap]


def wfa_pad_bytes(batch):
    """bool per pair: the pattern holds the text's padding byte 'Y' or the text the pattern's 'X' (the static tiers pass such pairs on)"""
    def has(slab, off, ln, ch):
        c = np.concatenate([[0], np.cumsum(slab == ch)])
        return (c[off + ln] - c[off]) > 0
    return has(batch.pat, batch.pat_off, batch.pat_len.astype(np.int64), ord("Y")) | has(batch.txt, batch.txt_off, batch.txt_len.astype(np.int64), ord("X"))


def wfa_plan(batch, pen, adaptive=False, knobs=None):
    """the launches gab_wfa_run_device makes for the pairs with both strings <= 2040 bases, from the longest such pattern and text:
    -> dict with `launches` = [(kernel, pool in offsets, directory size or static_rows), ...] up to and including the first wfa_global
    launch, and the host's intermediate values (seqp, seqt, byte_ok, static_rows, static_pool, use_static, slots, n_lds, n_big).
    knobs = {"GAB_WFA_NO_STATIC": 1, "GAB_WFA_POOL2": offsets, "GAB_WFA_SLOTS": slots} as the environment would set them."""
    knobs = knobs or {}
    pl, tl = batch.pat_len.astype(np.int64), batch.txt_len.astype(np.int64)
    lds = (pl <= WFA_LDS_MAX_LEN) & (tl <= WFA_LDS_MAX_LEN)
    n_lds, n_big = int(lds.sum()), int((~lds).sum())
    max_plen, max_tlen = (int(pl[lds].max()), int(tl[lds].max())) if n_lds else (0, 0)
    seqp, seqt = (max_plen + 32 + 8 + 15) & ~15, (max_tlen + 32 + 8 + 15) & ~15
    A = "true" if adaptive else "false"
    dir0 = 48 if adaptive else 56
    room = 2496 - dir0 * (16 if adaptive else 4) - (seqp + seqt)       # LDS budget per pair of the byte tier
    byte_ok = room >= 1024
    byte_pool = min(room & ~15, 2032)
    if byte_ok and max_tlen + dir0 + 2 > WFA_OFFB_MAX:
        byte_ok = False
    if not byte_ok:
        dir0 = 48
    static_rows = min(len(wfa_rows(pen)), WFA_OFFB_MAX - 2 - max_tlen) if not adaptive else 0
    static_pool = min(1568 - (seqp + seqt), 4080) & ~15
    use_static = (not adaptive and byte_pool != 0 and not knobs.get("GAB_WFA_NO_STATIC") and static_rows >= 16 and static_pool >= 1024)
    launches, slots = [], 0
    if n_lds:
        if use_static:
            pool2 = int(knobs.get("GAB_WFA_POOL2", 2560))
            launches.append(("wfa_lds_static<16,false>", static_pool, static_rows))
            if pool2 > static_pool:
                launches.append(("wfa_lds_static<16,true>", pool2, static_rows))
                slots = min(n_lds, max(65536, n_lds // 8)) & ~7
                if "GAB_WFA_SLOTS" in knobs:
                    slots = min(n_lds, int(knobs["GAB_WFA_SLOTS"]))
        else:
            launches.append((f"wfa_lds<16,{A},OffB>", min(byte_pool, 2046), dir0) if byte_ok else (f"wfa_lds<16,{A},int16_t>", 1024, dir0))
        launches.append((f"wfa_lds<64,{A},int16_t>", 6144, 128))
        launches.append((f"wfa_lds<64,{A},int16_t>", 49152, 640))
        launches.append((f"wfa_global<{A}>", 1 << 20, 4096))
    return dict(launches=launches, seqp=seqp, seqt=seqt, byte_ok=byte_ok, static_rows=static_rows, static_pool=static_pool,
                use_static=use_static, slots=slots, n_lds=n_lds, n_big=n_big, adaptive=adaptive)


def wfa_launch_holds(launch, model, pad_byte, rows_table):
    """bool per pair: this launch (kernel, pool, directory / rows) finishes the pair.
    A static launch gives up on a padding byte, on an M offset > 240, when the table's used_end of the final row exceeds the pool and
    when that row is not below static_rows; wfa_lds / wfa_global when the final score is not below the directory size (the score
    steps visit every score that has a wavefront), when the offsets allocated exceed the pool, and -- one-byte offsets -- on an M
    offset > 240."""
    kernel, pool, dirsz = launch
    if kernel.startswith("wfa_lds_static"):
        row = model["rows"] - 1
        ok = ~pad_byte & (model["max_m"] <= WFA_OFFB_SAFE) & (row < dirsz)
        used_end = np.array([r[4] for r in rows_table], np.int64)[np.minimum(row, len(rows_table) - 1)]
        return ok & (used_end <= pool)
    ok = (model["score"] < dirsz) & (model["used"] <= pool)
    if kernel.endswith("OffB>"):
        ok &= model["max_m"] <= WFA_OFFB_SAFE
    return ok


def wfa_tier_of(batch, pen, model, plan):
    """-> (tier int array: index into `launches` of the launch that finishes each pair, launches = [(kernel, pool, directory, pairs in,
    pairs left), ...] in launch order).  The plan's launches come first; what the first wfa_global leaves gets rounds with 8 x the
    pool and 4 x the directory (at most 2^22 scores) until nothing is left, then the pairs too long for LDS get rounds of their own
    from 2^20 offsets / 4 096 scores."""
    pl, tl = batch.pat_len.astype(np.int64), batch.txt_len.astype(np.int64)
    lds = (pl <= WFA_LDS_MAX_LEN) & (tl <= WFA_LDS_MAX_LEN)
    pad = wfa_pad_bytes(batch)
    table = wfa_rows(pen)
    A = "true" if plan["adaptive"] else "false"
    tier = np.full(batch.n, -1, np.int64)
    out = []

    def run(launch, todo):
        ok = wfa_launch_holds(launch, model, pad, table) & todo
        tier[ok] = len(out)
        out.append(launch + (int(todo.sum()), int((todo & ~ok).sum())))
        return todo & ~ok

    todo = lds.copy()
    for launch in plan["launches"]:
        todo = run(launch, todo)
    for first, todo in ((not plan["launches"], todo), (True, ~lds)):
        pool, dirsz = (1 << 20, 4096) if first else (1 << 23, 4 * 4096)
        while todo.any():
            todo = run((f"wfa_global<{A}>", pool, dirsz), todo)
            pool, dirsz = pool * 8, min(dirsz * 4, 1 << 22)
    return tier, out


def parse_wfa_trace(text):
    """GAB_WFA_TRACE lines of ONE gab_wfa_run_device call -> ([(kernel, pool, directory, pairs in, pairs left, resumed or None), ...],
    {"n_lds", "n_big", "requeued"})"""
    launches, tail = [], None
    for line in text.splitlines():
        m = re.match(r"\[gab_wfa\] launch (\d+) kernel (\S+) pool (\d+) dir (\d+) in (\d+) left (\d+)(?: resumed (\d+))?$", line)
        if m:
            assert int(m.group(1)) == len(launches), line
            launches.append((m.group(2),) + tuple(int(v) for v in m.group(3, 4, 5, 6)) + (None if m.group(7) is None else int(m.group(7)),))
            continue
        m = re.match(r"\[gab_wfa\] n_lds (\d+) n_big (\d+) requeued (\d+)$", line)
        if m:
            tail = dict(zip(("n_lds", "n_big", "requeued"), (int(v) for v in m.groups())))
    return launches, tail


def wfa_fit(pen, pool, max_score=4096):
    """(the last score whose history fits `pool` offsets, the next score that has a wavefront) by the recurrence of wfa_rows"""
    rows = wfa_rows(pen, max_score=max_score, table=False)
    k = max(i for i, r in enumerate(rows) if r[4] <= pool)
    return rows[k][0], rows[k + 1][0]


_WFA_ACGT = np.frombuffer(b"ACGT", np.uint8)


def wfa_mutated(rng, n, err, cut=None):
    """a random n-base pattern and a text copied from it with `err` errors per base (a third each deletions, insertions and
    substitutions), the text cut to `cut` bases"""
    p = _WFA_ACGT[rng.integers(0, 4, n)].tobytes()
    t = bytearray()
    for c in p:
        r = rng.random()
        if r < err / 3:
            continue
        if r < 2 * err / 3:
            t.append(b"ACGT"[int(rng.integers(0, 4))])
        t.append(c if r > err else b"ACGT"[int(rng.integers(0, 4))])
    return p, bytes(t if cut is None else t[:cut])


WFA_CENSUS_RATES = (0.0, 0.02, 0.05, 0.08, 0.12, 0.2, 0.35, 0.6)


def wfa_census_pairs(n, seed, rates=WFA_CENSUS_RATES, long_pairs=0):
    """n pairs: patterns of 100 .. 151 bases, texts mutated copies cut to 180 bases, the error rates in turn; `long_pairs` pairs of
    more than 2 040 bases (1 % errors) spread among them -> (patterns, texts)"""
    rng = np.random.default_rng(seed)
    pats, txts = [], []
    for i in range(n):
        p, t = wfa_mutated(rng, int(rng.integers(100, 152)), rates[i % len(rates)], 180)
        pats.append(p); txts.append(t)
    for k in range(long_pairs):
        p, t = wfa_mutated(rng, 2041 + 150 * k + int(rng.integers(0, 100)), 0.01)
        at = (k + 1) * n // (long_pairs + 1)
        pats.insert(at, p); txts.insert(at, t)
    return pats, txts


def wfa_scored_pair(score, seed, n=150):
    """an n-base pair built for `score` under (4, 6, 2): score / 4 substitutions two bases apart, or -- score = 2 (mod 4) -- (score - 10)
    / 4 of them and one 2-base gap behind them.  (Whether a pair really scores that is for the oracle to say: tests/test_wfa_oracle.py
    asks it.)"""
    assert score % 2 == 0 and (score % 4 == 0 or score >= 10)
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 4, n)
    subs = score // 4 if score % 4 == 0 else (score - 10) // 4
    assert 3 + 2 * subs < n - 16
    t = p.copy()
    at = 3 + 2 * np.arange(subs)
    t[at] = (t[at] + 1 + rng.integers(0, 3, subs)) % 4
    if score % 4:
        t = np.delete(t, [n - 12, n - 11])
    return _WFA_ACGT[p].tobytes(), _WFA_ACGT[t].tobytes()


WFA_BIG_PENALTIES = ((50, 60, 20), (300, 400, 150), (1000, 1500, 500))       # the directory binds, not the pool
WFA_SMALL_PENALTIES = ((1, 1, 1), (2, 3, 1), (5, 8, 3), (3, 1, 4))
WFA_PENALTIES = ((4, 6, 2),) + WFA_SMALL_PENALTIES + WFA_BIG_PENALTIES
WFA_REDUCTIONS = ((10, 50), (5, 3), (1, 0))


def wfa_penalty_pairs(seed=31, n=150):
    """an identical pair, one / two / three substitutions, a 1-base gap, a 2-base gap, a 1-base insertion plus a 2-base deletion
    -> (patterns, texts, lambda pen: the scores they were built for)"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 4, n)

    def sub(t, at):
        t = t.copy(); t[at] = (t[at] + 1) % 4
        return t
    ins = np.insert(p, 40, (p[40] + 1) % 4)               # (a base that differs from its right neighbour's: the gap cannot slide into a match)
    txts = [p, sub(p, [30]), sub(p, [30, 70]), sub(p, [30, 70, 110]), np.delete(p, 60), np.delete(p, [60, 61]), np.delete(ins, [100, 101])]
    built = lambda pen: [0, pen[0], 2 * pen[0], 3 * pen[0], pen[1] + pen[2], pen[1] + 2 * pen[2], 2 * pen[1] + 3 * pen[2]]
    return [_WFA_ACGT[p].tobytes()] * len(txts), [_WFA_ACGT[t].tobytes() for t in txts], built


def wfa_limit_pairs(tmax, n=600):
    """n pairs whose longest text is exactly tmax: patterns of tmax - 25 .. tmax bases, mutated texts cut to tmax, then texts at the
    limit, pure insertions and pairs far beyond 16 score rows"""
    rng = np.random.default_rng(tmax)
    pats, txts = [], []
    while len(pats) < n - 5:
        p, t = wfa_mutated(rng, int(rng.integers(tmax - 25, tmax + 1)), float(rng.choice([0.0, 0.01, 0.03, 0.06, 0.12])), tmax)
        pats.append(p); txts.append(t)
    pats += [b"ACGT" * 50, b"A" * (tmax - 30), b"ACGTTGCA" * 25]
    txts += [(b"ACGT" * 60)[:tmax], b"A" * tmax, (b"ACGTTGCA" * 30)[:tmax]]
    for err in (0.3, 0.5):
        p, t = wfa_mutated(rng, tmax - 20, err, tmax)
        pats.append(p); txts.append(t)
    return pats, txts


def wfa_padding_tail_pairs(n=200):
    """n easy pairs and, among them, pairs whose pattern ends in the text's padding byte 'Y' (the extension runs on past the end of
    the text: M offsets of 236 .. 246, on both sides of the 240 a byte tier accepts) or whose text ends in the pattern's 'X'"""
    rng = np.random.default_rng(77)
    pats, txts = wfa_census_pairs(n, 78, rates=(0.0, 0.02, 0.05))
    for k, extra in enumerate((56, 59, 60, 61, 62, 66)):
        p, t = wfa_mutated(rng, 180, 0.0)
        at = (k + 1) * n // 8
        pats.insert(at, p + b"Y" * extra); txts.insert(at, t)
        p, t = wfa_mutated(rng, 150, 0.02, 170)
        pats.insert(at, p); txts.insert(at, t + b"X" * (extra - 50))
    return pats, txts


_wfa_cases = None


def wfa_tier_cases():
    """the batches of tests/test_wfa_tiers_gpu.py: name -> (patterns, texts, penalties, reduction or None, knobs).  Built once."""
    global _wfa_cases
    if _wfa_cases is not None:
        return _wfa_cases
    C = {}
    base_p, base_t = wfa_census_pairs(1500, 1)
    # a. the census: every kind of launch of the default plan, and three pairs too long for the LDS kernels
    cp, ct = list(base_p), list(base_t)
    rng = np.random.default_rng(5)
    for k in range(3):
        p, t = wfa_mutated(rng, 2041 + 200 * k + int(rng.integers(0, 100)), 0.01)
        cp.insert((k + 1) * 375, p); ct.insert((k + 1) * 375, t)
    C["census"] = (cp, ct, (4, 6, 2), None, {})
    k1_p, k1_t = base_p[:1000], base_t[:1000]
    # b. one pair on each side of every pool limit of the default plan, in random places among 200 easy pairs
    easy_p, easy_t = wfa_census_pairs(200, 3, rates=(0.0, 0.02, 0.05))
    plan = wfa_plan(gabgen.pairs_from_lists(easy_p, easy_t), (4, 6, 2))
    bound = []
    for _, pool, _ in plan["launches"][:-1]:
        bound += [wfa_scored_pair(s, 7000 + s) + (s,) for s in wfa_fit((4, 6, 2), pool)]
    bp, bt = list(easy_p), list(easy_t)
    for (p, t, _), at in zip(bound, np.random.default_rng(4).integers(0, 200, len(bound))):
        bp.insert(int(at), p); bt.insert(int(at), t)
    C["boundary"] = (bp, bt, (4, 6, 2), None, {})
    C["boundary_pairs"] = bound
    # c. penalties under which the directory sizes 56 / 128 / 640 / 4 096 bind; the small sets on the census recipe
    for pen in WFA_BIG_PENALTIES:
        pp, pt, _ = wfa_penalty_pairs()
        C["pen_%d_%d_%d" % pen] = (pp, pt, pen, None, {})
    C["pen_50_60_20_nostatic"] = (pp, pt, (50, 60, 20), None, {"GAB_WFA_NO_STATIC": 1})       # (its table has rows enough for the static tier)
    for pen in WFA_SMALL_PENALTIES:
        C["census1000_%d_%d_%d" % pen] = (k1_p, k1_t, pen, None, {})
    # d. the longest text on both sides of the switch that turns the static tier off; M offsets on both sides of 240 in a byte tier
    for tmax in (227, 228):
        C["tmax%d" % tmax] = wfa_limit_pairs(tmax) + ((4, 6, 2), None, {})
    C["tmax228_adaptive_10_50"] = C["tmax228"][:2] + ((4, 6, 2), (10, 50), {})                  # wfa_lds<16,true,int16_t>
    C["offb_exit"] = wfa_padding_tail_pairs() + ((4, 6, 2), None, {"GAB_WFA_NO_STATIC": 1})
    # e. adaptive mode: the pool need depends on the data
    for red in WFA_REDUCTIONS[:2]:
        C["adaptive_%d_%d" % red] = (k1_p + [b[0] for b in bound], k1_t + [b[1] for b in bound], (4, 6, 2), red, {})
    # g. more pairs than the grids of the chained launches (also f: more pairs leave the first launch than GAB_WFA_SLOTS = 1002)
    gp, gt = wfa_census_pairs(3000, 2, rates=(0.1, 0.1, 0.25, 0.1, 0.1, 0.25, 0.1, 0.1, 0.6, 0.25))
    C["grid"] = (gp, gt, (4, 6, 2), None, {})
    # f. resume and restart
    for slots in (0, 3, 1002):
        C["slots_%d" % slots] = (gp, gt, (4, 6, 2), None, {"GAB_WFA_SLOTS": slots})
    for pool2 in (1024, 4080):
        C["pool2_%d" % pool2] = (k1_p, k1_t, (4, 6, 2), None, {"GAB_WFA_POOL2": pool2})
    _wfa_cases = C
    return C


_wfa_models = {}


def wfa_case_model(name):
    """one case of wfa_tier_cases, run through the model once -> (PairBatch, penalties, reduction, knobs, model, plan, tier, launches)"""
    pats, txts, pen, red, knobs = wfa_tier_cases()[name]
    key = (id(pats), pen, red)
    if key not in _wfa_models:
        batch = gabgen.pairs_from_lists(pats, txts)
        _wfa_models[key] = (batch, wfa_model(pats, txts, pen, red))
    batch, model = _wfa_models[key]
    plan = wfa_plan(batch, pen, red is not None, knobs)
    tier, launches = wfa_tier_of(batch, pen, model, plan)
    return batch, pen, red, knobs, model, plan, tier, launches


WFA_CASE_NAMES = (["census", "boundary"] + ["pen_%d_%d_%d" % p for p in WFA_BIG_PENALTIES] + ["pen_50_60_20_nostatic"] + ["census1000_%d_%d_%d" % p for p in WFA_SMALL_PENALTIES] +
                  ["tmax227", "tmax228", "tmax228_adaptive_10_50", "offb_exit", "adaptive_10_50", "adaptive_5_3", "grid", "slots_0", "slots_3", "slots_1002", "pool2_1024", "pool2_4080"])


def wfa_expected_resumed(name):
    """(fewest, most) pairs the chained static launch of a case can resume, or None when its plan has no such launch.  A pair the
    first launch leaves is resumed when it stopped for want of pool room (not for a padding byte, a large offset or the end of the
    row table) and its place in the overflow list is below the slot count; the places are taken in arrival order, so the two
    numbers differ only when some pairs left cannot be resumed AND there are fewer slots than pairs left."""
    batch, pen, red, knobs, model, plan, tier, launches = wfa_case_model(name)
    if len(launches) < 2 or not launches[1][0].startswith("wfa_lds_static"):
        return None
    table = wfa_rows(pen)
    r_pool = min(i for i, r in enumerate(table) if r[4] > launches[0][1])
    lds = (batch.pat_len <= WFA_LDS_MAX_LEN) & (batch.txt_len <= WFA_LDS_MAX_LEN)
    left = lds & (tier != 0)
    sure = left & ~wfa_pad_bytes(batch) & (model["max_m"] <= WFA_OFFB_SAFE) & (r_pool < launches[0][2])
    maybe = left & ~wfa_pad_bytes(batch) & (model["max_m"] > WFA_OFFB_SAFE) & (r_pool < launches[0][2])
    n_left, n_sure, n_maybe, slots = int(left.sum()), int(sure.sum()), int(maybe.sum()), plan["slots"]
    return max(0, min(slots, n_left) - (n_left - n_sure)), min(slots, n_sure + n_maybe)


# ---- chain: which kernel form a call of a batch is sent to (genarchbench_amd/csrc/chain.hip, the batch-shape rule of gab_chain_run_device)
CHAIN_FORM_THROUGHPUT, CHAIN_FORM_LATENCY, CHAIN_FORM_TABLE, CHAIN_FORM_LEGACY = 1, 2, 3, 6
CHAIN_DISPATCH = {                      # the four settings tests/test_chain_gpu.py runs under
    "default-split": {},
    "latency-form-for-all": {"GAB_CHAIN_FAST_MIN": "1", "GAB_CHAIN_FAST_CALLS": "1000000000", "GAB_CHAIN_TAB": "0"},
    "throughput-form-for-all": {"GAB_CHAIN_FAST_CALLS": "0", "GAB_CHAIN_TAB": "0"},
    "table-form-for-all": {"GAB_CHAIN_TAB_MIN": "1"},
}
CHAIN_SPLIT_KNOBS = ("GAB_CHAIN_TAB", "GAB_CHAIN_TAB_MIN", "GAB_CHAIN_FAST_MIN", "GAB_CHAIN_FAST_CALLS", "GAB_CHAIN_KERNEL", "GAB_CHAIN_HELPERS")


def chain_split_model(n_per_call, mode, env=None, through=False, total=None):
    """the form gab_chain_run_device sends every call of a batch to, BEFORE the forms' own eligibility tests: 0 empty call,
    1 throughput form, 2 latency form, 3 table form, 6 the legacy-only launch -- per call, in the caller's order.  n_per_call: anchors of
    the calls (back to back: the batch's anchors are their sum); mode 0 chain, 1 fast-chain; env: the GAB_CHAIN_* pins that are set.

    The rule, as chain.hip words it.  The calls are sorted longest first (stable).  The throughput form takes ~0.30 us per anchor of a
    call and does ~2.85 G anchors/s over all calls; a batch whose longest call needs at least 0.75 of the batch's throughput time WAITS
    for it.  Such a batch hands to the table form every call that would take a quarter of that time, 2 048 anchors at least; whatever
    the batch, fast-chain sends calls of >= 4 096 anchors there and chain those of >= 8 192 -- except with through=True, a
    gab_chain_run_device_through call on page-locked host arrays (asked for AND page-locked: pageable arrays keep the floors), whose
    results would leave the table form in too short a burst for the bus.  total: the arrays' extent as chain.hip computes it, the
    largest call_off + n, where the calls do not lie back to back (gaps count as anchors of the batch).  GAB_CHAIN_TAB_MIN pins the table form's smallest call, GAB_CHAIN_TAB=0 turns the form off.  The same test on what is left
    (its anchors, its longest call) hands every remaining call of >= 512 anchors to the latency form; GAB_CHAIN_FAST_MIN pins that
    length and GAB_CHAIN_FAST_CALLS the number of calls (FAST_MIN alone: as many as there are).  The rest is the throughput form's.
    GAB_CHAIN_HELPERS, and GAB_CHAIN_KERNEL=walk for chain, send everything through one launch of the older kernels instead."""
    env = env or {}
    pin = lambda k: int(env[k]) if k in env else -1
    n = np.asarray(n_per_call, np.int64)
    form = np.zeros(len(n), np.uint8)
    order = [int(c) for c in np.argsort(-n, kind="stable") if n[c] > 0]
    if not order:
        return form
    if "GAB_CHAIN_HELPERS" in env or (mode == 0 and env.get("GAB_CHAIN_KERNEL") == "walk"):
        form[order] = CHAIN_FORM_LEGACY
        return form
    srt = [int(n[c]) for c in order]
    total, per_anchor, rate, wait = sum(srt) if total is None else int(total), 0.30e-6, 2.85e9, 0.75
    ntab = 0
    if pin("GAB_CHAIN_TAB") != 0:
        tp = total / rate
        least = max(2048, int(0.25 * tp / per_anchor)) if per_anchor * srt[0] >= wait * tp else None
        floor = float("inf") if through else 4096 if mode == 1 else 8192
        least = floor if least is None else min(least, floor)
        if pin("GAB_CHAIN_TAB_MIN") >= 0:
            least = pin("GAB_CHAIN_TAB_MIN")
        while ntab < len(srt) and srt[ntab] >= least:
            ntab += 1
    rest = srt[ntab:]
    nfast = 0
    if rest:
        tp = (total - sum(srt[:ntab])) / rate
        least, most = (512, len(rest)) if per_anchor * rest[0] >= wait * tp else (0, 0)
        if pin("GAB_CHAIN_FAST_MIN") >= 0:
            least = pin("GAB_CHAIN_FAST_MIN")
            most = len(rest)
        if pin("GAB_CHAIN_FAST_CALLS") >= 0:
            most = pin("GAB_CHAIN_FAST_CALLS")
        while nfast < min(len(rest), most) and rest[nfast] >= least:
            nfast += 1
    form[order[:ntab]] = CHAIN_FORM_TABLE
    form[order[ntab:ntab + nfast]] = CHAIN_FORM_LATENCY
    form[order[ntab + nfast:]] = CHAIN_FORM_THROUGHPUT
    return form


def chain_split_margins(n_per_call, mode, through=False, total=None):
    """how far the floating-point comparisons of the default rule are from flipping on this batch: the ratios (longest call's time) /
    (0.75 of the throughput time) of the two stages, for the table form and for what it leaves -- a test batch keeps both 10 %
    away from 1 (the lengths themselves are compared as integers).  through, total: as chain_split_model takes them"""
    n = sorted((int(v) for v in n_per_call if v > 0), reverse=True)
    total = sum(n) if total is None else int(total)
    ntab = int((chain_split_model(n, mode, through=through, total=total) == CHAIN_FORM_TABLE).sum())
    out = [0.30e-6 * n[0] / (0.75 * total / 2.85e9)]
    if n[ntab:]:
        out.append(0.30e-6 * n[ntab] / (0.75 * (total - sum(n[:ntab])) / 2.85e9))
    return out


CHAIN_THROUGH_NONE, CHAIN_THROUGH_WRITTEN, CHAIN_THROUGH_PAGEABLE, CHAIN_THROUGH_FORM, CHAIN_THROUGH_WRITTEN_COPIED = 0, 1, 2, 3, 4
CHAIN_SEVEN_HELPERS = 326              # chain_helpers_for: seven helper waves when the arrays' extent <= 326 x the longest call


def chain_extent(n_per_call, call_off=None):
    """`total` as chain_check_hdrs computes it: the largest call_off + n over ALL calls, empty ones included (0 without a call);
    call_off None: the calls lie back to back"""
    n = np.asarray(n_per_call, np.int64)
    if call_off is None:
        return int(n.sum())
    return int((np.asarray(call_off, np.int64) + n).max()) if len(n) else 0


def chain_through_route(n_per_call, call_off, mode, env, pinned, forms=None):
    """what gab_chain_last_through reports after a run of this batch (include/gab.h): 0 not asked for (pinned None: gab_chain_run_device),
    1 written through by the kernels, 2 copied because the host arrays are pageable, 3 copied because a launch that does not write
    through took part, 4 written through and copied after all.  pinned: the host arrays of gab_chain_run_device_through are
    page-locked; forms: what gab_chain_last_split reported, which alone tells 1 from 4 -- whether the table form handed a call back (4:
    not eligible, 5: no room or by the fold); without it, 1.

    The rules, as chain_run_device_impl words them.  A batch without an anchor launches and copies nothing: 1 (0 when not asked for).
    Pageable arrays: 2.  Otherwise the split decides (chain_split_model with through=True).  If the table or the latency form took a
    call: the latency form does not write through (3), the table form and the throughput launch beside it do (1 / 4).  If neither
    did, ONE launch runs everything and writes through only as the three-helper throughput kernel: GAB_CHAIN_HELPERS=3 does (as form
    6), 5 and 7 do not, the walk kernel (GAB_CHAIN_KERNEL=walk, chain) does not, and without a pin chain_helpers_for gives seven
    helpers to a batch whose extent -- gaps included -- is at most 326 times its longest call (3)."""
    env = env or {}
    n = np.asarray(n_per_call, np.int64)
    if pinned is None:
        return CHAIN_THROUGH_NONE
    if not (n > 0).any():
        return CHAIN_THROUGH_WRITTEN
    if not pinned:
        return CHAIN_THROUGH_PAGEABLE
    total = chain_extent(n, call_off)
    split = chain_split_model(n, mode, env, through=True, total=total)
    if (split == CHAIN_FORM_LATENCY).any():
        return CHAIN_THROUGH_FORM
    if (split == CHAIN_FORM_TABLE).any():
        back = forms is not None and bool(np.isin(np.asarray(forms), (4, 5)).any())
        return CHAIN_THROUGH_WRITTEN_COPIED if back else CHAIN_THROUGH_WRITTEN
    if mode == 0 and env.get("GAB_CHAIN_KERNEL") == "walk":
        return CHAIN_THROUGH_FORM
    helpers = int(env["GAB_CHAIN_HELPERS"]) if env.get("GAB_CHAIN_HELPERS") in ("3", "5", "7") else (7 if total <= CHAIN_SEVEN_HELPERS * int(n.max()) else 3)
    return CHAIN_THROUGH_WRITTEN if helpers == 3 else CHAIN_THROUGH_FORM
