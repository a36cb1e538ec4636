"""Constructed batches for genarchbench_amd/csrc/bitpal.hip and a restatement of its routing rule (no GPU, no library): which kernel
scores which pair -- the bit-vector kernel bitpal_edit_bv<D>, the integer DP with its boundary column in LDS (bitpal_dp<true, .>) or in
global scratch (bitpal_dp<false, .>) -- and what gab_bitpal_last_paths / gab_bitpal_last_stats must report for the batch.
tests/test_bitpal_cases.py holds the constants below against the sources and the batches against the edges they are named for;
tests/test_bitpal_paths_gpu.py runs them.  Pairs may share slab bytes (a PairBatch whose offsets repeat), so the slabs stay small."""
import functools
from dataclasses import dataclass

import numpy as np

from tools import gabgen

# ---- the constants of bitpal.hip / gab.h (test_bitpal_cases.py reads them back from the sources)
CHUNK = 32                  # kChunk: DP columns per register chunk
LDS_ROWS = 2048             # kLdsRows: longest row string on the LDS path
BIG_BLOCKS = 256            # kBigBlocks: workgroups of the global-scratch path, 64 pairs each per trip
BV_MAX_ROWS = 256           # kBvMaxRows
BV_BLOCK = 256              # kBvBlock
SLOT_LETTERS = b"ACGTN"     # bitpal_bv_slot: the bytes a row string may hold on the bit-vector path
GRID_CAP = 512              # workgroups of bitpal_classify / bitpal_scatter, 256 pairs each per trip
MAX_LEN = 16320             # GAB_BITPAL_MAX_LEN

EDIT, SCORED = 0, 1
SCORING = {EDIT: (0, -1, -1), SCORED: (1, -4, -2)}       # (match, mismatch, gap)
BV, LDS, GLOBAL = 0, 1, 2                               # the path of a pair
NO_REJECT, BY_ROWS, BY_BYTE = 0, 1, 2                   # why the bit-vector kernel hands a pair to the integer DP
PATH_KEYS = ("bv_words", "bv_pairs", "lds_pairs", "lds_rows", "global_pairs", "global_blocks", "global_rows", "id_lists")


# ------------------------------------------------------------------------------------------------ the routing rule
def bad_pairs(batch, pat_bytes=None, txt_bytes=None):
    """indices of the pairs bitpal_pair_ok refuses; pat_bytes / txt_bytes: the slab sizes handed to gab_bitpal_run_device (default:
    the whole arrays; gab_bitpal_run stages a window that always holds the rounded-up ends)"""
    pb = len(batch.pat) if pat_bytes is None else pat_bytes
    tb = len(batch.txt) if txt_bytes is None else txt_bytes
    pl, tl = batch.pat_len.astype(np.int64), batch.txt_len.astype(np.int64)
    po, to = batch.pat_off.astype(np.int64), batch.txt_off.astype(np.int64)
    ok = (pl >= 0) & (tl >= 0) & (pl <= MAX_LEN) & (tl <= MAX_LEN) & (po >= 0) & (to >= 0) & (((po + pl + 3) & ~3) <= pb) & (((to + tl + 3) & ~3) <= tb)
    return np.flatnonzero(~ok)


def _outside(slab):
    """prefix count of the bytes outside SLOT_LETTERS"""
    ok = np.zeros(256, bool)
    ok[list(SLOT_LETTERS)] = True
    return np.concatenate([[0], np.cumsum(~ok[slab])]).astype(np.int64)


@dataclass
class Route:
    path: np.ndarray         # BV / LDS / GLOBAL per pair
    reason: np.ndarray       # NO_REJECT / BY_ROWS / BY_BYTE per pair (bit-vector runs only)
    paths: dict              # gab_bitpal_last_paths
    cells: int               # gab_bitpal_last_stats
    long_pairs: int
    classify_trips: int      # trips of bitpal_classify's (and bitpal_scatter's) grid-stride loop
    global_trips: int        # trips of bitpal_dp<false, .>'s loop over groups of 64


def route(batch, alg, no_bv=False):
    """what a run of a batch without bad pairs does; alg: EDIT / SCORED, no_bv: GAB_BITPAL_NO_BV=1"""
    assert bad_pairs(batch).size == 0
    n = batch.n
    pl, tl = batch.pat_len.astype(np.int64), batch.txt_len.astype(np.int64)
    rows = np.minimum(pl, tl)
    to_lds = rows <= LDS_ROWS
    max_rows_lds = int(rows[to_lds].max()) if to_lds.any() else 0
    max_rows_big = int(rows[~to_lds].max()) if (~to_lds).any() else 0
    path = np.where(to_lds, LDS, GLOBAL).astype(np.int8)
    reason = np.zeros(n, np.int8)
    paths = dict.fromkeys(PATH_KEYS, 0)
    bitvec = alg == EDIT and not no_bv
    if bitvec:
        D = (min(max(max_rows_lds, 1), BV_MAX_ROWS) + 31) // 32
        po, to = batch.pat_off.astype(np.int64), batch.txt_off.astype(np.int64)
        cp, ct = _outside(batch.pat), _outside(batch.txt)
        pat_is_rows = pl <= tl                      # the kernel's tie rule: equal lengths, the pattern makes the rows
        outside = np.where(pat_is_rows, cp[po + pl] - cp[po], ct[to + tl] - ct[to])
        reason[outside > 0] = BY_BYTE
        reason[rows > min(32 * D, BV_MAX_ROWS)] = BY_ROWS       # (tested first: such a pair's bytes are never looked at)
        path[reason == NO_REJECT] = BV
        paths["bv_words"] = D
        paths["bv_pairs"] = int((path == BV).sum())
    n_lds, n_big = int((path == LDS).sum()), int((path == GLOBAL).sum())
    if n_lds:
        paths["lds_pairs"], paths["lds_rows"] = n_lds, max_rows_lds
    blocks = min(-(-n_big // 64), BIG_BLOCKS)
    if n_big:
        paths["global_pairs"], paths["global_blocks"], paths["global_rows"] = n_big, blocks, max_rows_big
    # the bit-vector kernel always lists its rejects; without it the lists exist only when a batch mixes the two DP paths
    paths["id_lists"] = int(bool(n_lds or n_big) and (bitvec or (~to_lds).any()))
    return Route(path, reason, paths, int((pl * tl).sum()), int((~to_lds).sum()), -(-n // (GRID_CAP * 256)),
                 -(-n_big // (64 * blocks)) if n_big else 0)


def plain_dp(p, t, alg):
    """Needleman-Wunsch score of two byte strings, linear gaps: three lines of DP"""
    ma, mi, g = SCORING[alg]
    prev = [j * g for j in range(len(t) + 1)]
    for i, a in enumerate(p, 1):
        cur = [i * g]
        for j, b in enumerate(t, 1):
            cur.append(max(prev[j - 1] + (ma if a == b else mi), prev[j] + g, cur[j - 1] + g))
        prev = cur
    return prev[-1]


_EXPECTED = {}


def expected(name, alg):
    """oracle scores of the batch BATCHES[name](), computed once and shared (read-only)"""
    if (name, alg) not in _EXPECTED:
        from oracle import pyoracle
        b = BATCHES[name]()
        if name == "global_second_trip":        # four distinct pairs, tiled
            want = pyoracle.bitpal(_second_trip_four(), alg)[second_trip_index()]
        else:
            want = pyoracle.bitpal(b, alg)
        want.setflags(write=False)
        _EXPECTED[(name, alg)] = want
    return _EXPECTED[(name, alg)]


# ------------------------------------------------------------------------------------------------ helpers
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_ACGTN = np.frombuffer(b"ACGTN", np.uint8)


def _rand(rng, n, alpha=_ACGT):
    return rng.choice(alpha, n).tobytes()


def _edited(rng, p, n, rate=0.1, alpha=_ACGT):
    """a string of n bytes: p with about `rate` substitutions, then bytes inserted or deleted at random places until n are left"""
    t = bytearray(p)
    for _ in range(int(len(t) * rate) + (1 if t else 0)):
        t[int(rng.integers(0, len(t)))] = int(rng.choice(alpha))
    while len(t) < n:
        t.insert(int(rng.integers(0, len(t) + 1)), int(rng.choice(alpha)))
    while len(t) > n:
        del t[int(rng.integers(0, len(t)))]
    return bytes(t)


def _frozen(b):
    for a in (b.pat, b.pat_off, b.pat_len, b.txt, b.txt_off, b.txt_len):
        a.setflags(write=False)
    return b


def aligned_batch(pats, txts, pat_align, txt_align):
    """pairs_from_lists with string i placed at a slab offset that is pat_align[i] resp. txt_align[i] modulo 4"""
    def slab(strings, align):
        off, cur = [], 0
        for s, a in zip(strings, align):
            cur = ((cur + 3) & ~3) + a
            off.append(cur); cur += len(s)
        buf = np.full(cur + 16, ord("#"), np.uint8)       # between the strings: a byte that equals none of theirs
        for s, o in zip(strings, off):
            buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
        return buf, np.array(off, np.int64), np.array([len(s) for s in strings], np.int32)
    p, po, pl = slab(pats, pat_align)
    t, to, tl = slab(txts, txt_align)
    return gabgen.PairBatch(p, po, pl, t, to, tl)


# ------------------------------------------------------------------------------------------------ width_D
COLUMN_EXTRA = (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 67)      # columns = rows + each: the 32-column, 16-column and 4-byte loops, their tails
CONTENTS = ("identical", "disjoint", "one_base", "edits", "longer_first", "across")


def across_words(rng, r, c):
    """rows whose two bases around every word boundary (rows 32 w - 1 and 32 w) the columns lack: the best alignment deletes them, a
    vertical run right after a match -- the cells the carry of the add from word w - 1 into word w exists for (myers_words below)"""
    rows = _rand(rng, r)
    cut = {x for w in range(32, r, 32) for x in (w - 1, w)}
    cols = bytes(ch for i, ch in enumerate(rows) if i not in cut)
    return rows, cols + _rand(rng, c - len(cols))


def myers_words(p, t, words, no_carry_into=None):
    """gab_myers_step32 / gab_myers_distance32 restated on one Python integer of 32 * words bits: the edit distance of p (rows, at most
    32 * words) and t.  no_carry_into = w: the add done as two adds, below and from bit 32 w, as if word w - 1 kept its carry"""
    full = (1 << 32 * words) - 1
    eq = {}
    for i, ch in enumerate(p):
        eq[ch] = eq.get(ch, 0) | 1 << i
    P, M = full, 0
    for ch in t:
        Eq = eq.get(ch, 0)
        Xv = Eq | M
        if no_carry_into is None:
            s = ((Eq & P) + P) & full
        else:
            k = 32 * no_carry_into
            lo = (1 << k) - 1
            s = (((Eq & P & lo) + (P & lo)) & lo) | (((((Eq & P) >> k) + (P >> k)) << k) & full)
        Xh = (s ^ P) | Eq
        Ph = M | (~(Xh | P) & full)
        Mh = P & Xh
        phs, mhs = ((Ph << 1) | 1) & full, (Mh << 1) & full
        P, M = mhs | (~(Xv | phs) & full), phs & Xv
    rows = (1 << len(p)) - 1
    return len(t) + bin(P & rows).count("1") - bin(M & rows).count("1")


def width_rows(D):
    """1, 31, 32, 33, every word boundary below D as 32 w - 1, 32 w, 32 w + 1, then 32 D - 1 and 32 D; nothing above 32 D"""
    r = {1, 31, 32, 33, 32 * D - 1, 32 * D}
    for w in range(1, D):
        r |= {32 * w - 1, 32 * w, 32 * w + 1}
    return sorted(x for x in r if 1 <= x <= 32 * D)


@functools.lru_cache(maxsize=None)
def width(D):
    rng = np.random.default_rng(100 + D)
    pats, txts = [], []
    for r in width_rows(D):
        for extra in COLUMN_EXTRA:
            c = r + extra
            for kind in CONTENTS:
                if kind == "identical":
                    p = _rand(rng, r, _ACGTN); t = (p * (c // r + 1))[:c]      # (the columns' surplus repeats the rows)
                elif kind == "disjoint":                       # distance = columns
                    p = _rand(rng, r, np.frombuffer(b"AC", np.uint8)); t = _rand(rng, c, np.frombuffer(b"GTN", np.uint8))
                elif kind == "one_base":                       # Eq all ones: the carry of the add runs through every word
                    p = b"G" * r; t = b"G" * c
                elif kind == "across":
                    p, t = across_words(rng, r, c)
                else:
                    p = _rand(rng, r, _ACGTN); t = _edited(rng, p, c, 0.1, _ACGTN)
                    if kind == "longer_first":
                        p, t = t, p
                pats.append(p); txts.append(t)
    return _frozen(gabgen.pairs_from_lists(pats, txts))


# ------------------------------------------------------------------------------------------------ bv_routes
@functools.lru_cache(maxsize=None)
def bv_routes():
    """-> (batch, the reject reason every pair must get)"""
    rng = np.random.default_rng(7)
    P = []                                                     # (pattern, text, reason)
    add = lambda p, t, why: P.append((p, t, why))
    s20, s30 = _rand(rng, 20, _ACGTN), _rand(rng, 30, _ACGTN)
    for bad in (b"x", b"a", b"t", b"n", b"\x00", b"\xff", b"@", b"O"):
        for pos in (0, 15, 16, 19):                         # in the 16-byte loop of the row masks and in its 4-byte tail
            rows_bad = s20[:pos] + bad + s20[pos + 1:]
            cols_bad = s30[:pos] + bad + s30[pos + 1:]
            add(rows_bad, s30, BY_BYTE); add(s30, rows_bad, BY_BYTE)          # in the row string only, given first or second
            add(s20, cols_bad, NO_REJECT); add(cols_bad, s20, NO_REJECT)      # in the column string only
            add(rows_bad, cols_bad, BY_BYTE)
    add(b"ACxT", b"ACGT", BY_BYTE); add(b"ACGT", b"ACxT", NO_REJECT)           # equal lengths: the pattern makes the rows
    add(b"acgt", b"ACGT", BY_BYTE); add(b"ACGT", b"acgt", NO_REJECT); add(b"acgtn", b"acgt", BY_BYTE)
    add(b"NNNN", b"NNNNNN", NO_REJECT); add(b"ANNA" * 9, b"NAAN" * 10, NO_REJECT); add(b"N", b"N", NO_REJECT)
    add(b"", b"ACGT", NO_REJECT); add(b"ACGTA", b"", NO_REJECT); add(b"", b"", NO_REJECT); add(b"", b"xyz", NO_REJECT)
    for r, why in ((255, NO_REJECT), (256, NO_REJECT), (257, BY_ROWS), (258, BY_ROWS)):
        p = _rand(rng, r, _ACGTN)
        for c in (r, r + 43):
            t = _edited(rng, p, c, 0.1, _ACGTN)
            add(p, t, why); add(t, p, why)
    p = _rand(rng, 257); add(p[:100] + b"x" + p[101:], p, BY_ROWS)             # too many rows and an outside byte: by rows
    # accepted and rejected pairs side by side in every wave; 333 pairs: neither whole waves nor whole workgroups
    k = 0
    while len(P) < 333:
        r = 1 + k % 37
        p = _rand(rng, r, _ACGTN); t = _edited(rng, p, r + k % 5, 0.2, _ACGTN)
        if k % 3 == 1:
            p = p[:r // 2] + b"y" + p[r // 2 + 1:]
        add(p, t, BY_BYTE if k % 3 == 1 else NO_REJECT)
        k += 1
    order = rng.permutation(len(P))
    P = [P[i] for i in order]
    why = np.array([w for _, _, w in P], np.int8)
    why.setflags(write=False)
    return _frozen(gabgen.pairs_from_lists([p for p, _, _ in P], [t for _, t, _ in P])), why


# ------------------------------------------------------------------------------------------------ all_reject, none_reject, all_long
@functools.lru_cache(maxsize=None)
def all_reject():
    rng = np.random.default_rng(8)
    pats = [_rand(rng, 1 + k % 50).lower() for k in range(70)]
    return _frozen(gabgen.pairs_from_lists(pats, [_edited(rng, p.upper(), len(p) + k % 7) for k, p in enumerate(pats)]))


@functools.lru_cache(maxsize=None)
def none_reject():
    rng = np.random.default_rng(9)
    pats = [_rand(rng, 1 + k % 50, _ACGTN) for k in range(70)]
    return _frozen(gabgen.pairs_from_lists(pats, [_edited(rng, p, len(p) + k % 7).lower() for k, p in enumerate(pats)]))


@functools.lru_cache(maxsize=None)
def all_long():
    rng = np.random.default_rng(10)
    a, b = _rand(rng, 2049), _rand(rng, 2100)
    return _frozen(gabgen.pairs_from_lists([a, _edited(rng, b, 2060)], [_edited(rng, a, 2049), b]))


# ------------------------------------------------------------------------------------------------ switch_2048
SWITCH_ROWS = (2047, 2048, 2049, 2050)


@functools.lru_cache(maxsize=None)
def switch_2048():
    """one wave: the eight long pairs among pairs of 1 and of 100 rows"""
    rng = np.random.default_rng(11)
    pats, txts = [], []
    for k, r in enumerate(SWITCH_ROWS):
        for c in (r, r + 40):
            p = _rand(rng, r); t = _edited(rng, p, c, 0.1)
            for small in (1, 100, 1):
                q = _rand(rng, small); pats.append(q); txts.append(_edited(rng, q, small + k, 0.1))
            if c != r and k % 2:
                p, t = t, p
            pats.append(p); txts.append(t)
    assert len(pats) <= 64
    return _frozen(gabgen.pairs_from_lists(pats, txts))


# ------------------------------------------------------------------------------------------------ bytes_256
def bytes_256_columns(v):
    """twelve columns = three dwords: each of the four byte positions meets v, v with bit 7 flipped and v with bit 0 flipped"""
    kinds = (v, v ^ 0x80, v ^ 0x01)
    return bytes(kinds[(b + s) % 3] for s in range(3) for b in range(4))


@functools.lru_cache(maxsize=None)
def bytes_256():
    """pair v: eight rows of the byte v against bytes_256_columns(v).  Every row holds the same byte, so a wrong answer of the compare
    in ANY column adds or takes one match and moves the score (by 1 for edit, by 5 for scored).  Odd v: the columns given first."""
    pats, txts = [], []
    for v in range(256):
        r, c = bytes([v]) * 8, bytes_256_columns(v)
        if v & 1:
            r, c = c, r
        pats.append(r); txts.append(c)
    return _frozen(gabgen.pairs_from_lists(pats, txts))


# ------------------------------------------------------------------------------------------------ chunk_edges
CHUNK_COLUMNS = (1, 31, 32, 33, 63, 64, 65, 96)
CHUNK_ROWS = (1, 2, 3, 4, 5, 15, 16, 17, 18)      # the two-rows-per-trip loop, its odd tail, the 16-byte reload of the row string


@functools.lru_cache(maxsize=None)
def chunk_edges():
    rng = np.random.default_rng(12)
    pats, txts, pa, ta = [], [], [], []
    for c in CHUNK_COLUMNS:
        for r in CHUNK_ROWS:
            if r > c:
                continue
            for a in range(4):                      # rows at alignment a, columns at (3 a + 1) % 4 = 1, 0, 3, 2
                cols = _rand(rng, c)
                rows = _edited(rng, cols[int(rng.integers(0, c - r + 1)):][:r], r, 0.15)
                if (r + a) % 2:
                    pats.append(rows); txts.append(cols); pa.append(a); ta.append((3 * a + 1) % 4)
                else:
                    pats.append(cols); txts.append(rows); pa.append((3 * a + 1) % 4); ta.append(a)
    return _frozen(aligned_batch(pats, txts, pa, ta))


# ------------------------------------------------------------------------------------------------ classify_stride
CLASSIFY_STRIDE_PAIRS = GRID_CAP * 256 + 256 + 3


@functools.lru_cache(maxsize=None)
def classify_stride(with_bad=False):
    """pairs of 1 .. 8 bases that share 4 KB slabs; the last pair is the only long one.  with_bad: one more pair behind it, of
    length -1 (for the refusal test alone; through gab_bitpal_run_device, the host entry point refuses it before the GPU sees it)"""
    rng = np.random.default_rng(13)
    n = CLASSIFY_STRIDE_PAIRS
    lp = _rand(rng, 2049); lt = _edited(rng, lp, 2070, 0.05)
    pat = np.concatenate([np.frombuffer(_rand(rng, 4096), np.uint8), np.frombuffer(lp, np.uint8), np.zeros(16, np.uint8)])
    txt = np.concatenate([np.frombuffer(_rand(rng, 4096), np.uint8), np.frombuffer(lt, np.uint8), np.zeros(16, np.uint8)])
    po = rng.integers(0, 4096 - 8, n).astype(np.int64); to = (po + rng.integers(-2, 3, n)).clip(0, 4096 - 8).astype(np.int64)
    pl = rng.integers(1, 9, n).astype(np.int32); tl = rng.integers(1, 9, n).astype(np.int32)
    po[-1], to[-1], pl[-1], tl[-1] = 4096, 4096, len(lp), len(lt)
    if with_bad:
        po, to = np.append(po, 0), np.append(to, 0)
        pl, tl = np.append(pl, np.int32(-1)), np.append(tl, np.int32(4))
    return _frozen(gabgen.PairBatch(pat, po, pl, txt, to, tl))


# ------------------------------------------------------------------------------------------------ global_second_trip
GLOBAL_SECOND_TRIP_PAIRS = BIG_BLOCKS * 64 + 70
SECOND_TRIP_ROWS = (2049, 2055, 2060, 2049)


def second_trip_index():
    """which of the four pair i is: i % 4, turned by one for the pairs behind the first trip (so also in list order = pair order)"""
    i = np.arange(GLOBAL_SECOND_TRIP_PAIRS)
    return (i + i // (BIG_BLOCKS * 64)) % 4


@functools.lru_cache(maxsize=None)
def _second_trip_four():
    rng = np.random.default_rng(14)
    pats, txts = [], []
    for k, r in enumerate(SECOND_TRIP_ROWS):
        p = _rand(rng, r); t = _edited(rng, p, r + (0, 33, 5, 64)[k], (0.02, 0.1, 0.3, 0.15)[k])
        if k == 2:
            p, t = t, p
        pats.append(p); txts.append(t)
    return _frozen(gabgen.pairs_from_lists(pats, txts))


@functools.lru_cache(maxsize=None)
def global_second_trip():
    """pair i is one of four distinct ones (shared offsets), mixed so that the lane of a second trip follows a different pair's boundary
    column, whatever order bitpal_scatter lists them in.  70 G cells: measured on an MI355X at 81 - 89 ms of device time per run
    (kernel_ms of gab_bitpal_last_stats; edit, edit without the bit-vector kernel and scored alike), 0.2 s per test with both entry points"""
    four = _second_trip_four()
    idx = second_trip_index()
    return _frozen(gabgen.PairBatch(four.pat, four.pat_off[idx], four.pat_len[idx], four.txt, four.txt_off[idx], four.txt_len[idx]))


# ------------------------------------------------------------------------------------------------ limits
@functools.lru_cache(maxsize=None)
def limits_accepted():
    rng = np.random.default_rng(15)
    a, b = _rand(rng, MAX_LEN), _rand(rng, MAX_LEN)
    return _frozen(gabgen.pairs_from_lists([a, b"G", b"ACGT"], [b"T", b, b"ACGA"]))


@dataclass
class Refusal:
    batch: object
    bad: tuple               # indices of the bad pairs, ascending
    pat_bytes: int           # the slab sizes for gab_bitpal_run_device
    txt_bytes: int
    host: str                # what gab_bitpal_run does with the batch: "scan" (refused on the host: negative offset / length),
                             # "classify" (refused by the GPU like gab_bitpal_run_device), None (accepted: its window holds every end)


def _good_strings(rng, k):
    pats = [_rand(rng, 5 + 3 * i) for i in range(k)]
    return pats, [_edited(rng, p, len(p) + i % 3, 0.2) for i, p in enumerate(pats)]


@functools.lru_cache(maxsize=None)
def limits_refused():
    """name -> Refusal: one batch per condition of bitpal_pair_ok, the bad pair at a known index among good ones; two bad pairs"""
    rng = np.random.default_rng(16)
    out = {}

    def tampered(name, field, index, value, host):
        pats, txts = _good_strings(rng, 7)
        b = gabgen.pairs_from_lists(pats, txts)
        getattr(b, field)[index] = value
        out[name] = Refusal(_frozen(b), (index,), len(b.pat), len(b.txt), host)

    for side in ("pat", "txt"):
        pats, txts = _good_strings(rng, 7)
        (pats if side == "pat" else txts)[3] = _rand(rng, MAX_LEN + 1)
        b = gabgen.pairs_from_lists(pats, txts)
        out[side + "_len_over"] = Refusal(_frozen(b), (3,), len(b.pat), len(b.txt), "classify")
        tampered(side + "_len_negative", side + "_len", 2 if side == "pat" else 5, -1, "scan")
        tampered(side + "_off_negative", side + "_off", 4 if side == "pat" else 1, -1, "scan")
        # the string that ends the slab belongs to pair 2; it ends one byte into a dword that the slab does not hold to its end
        pats, txts = _good_strings(rng, 7)
        strings = pats if side == "pat" else txts
        strings[6] += _rand(rng, (1 - sum(len(s) for s in strings)) % 4)
        b = gabgen.pairs_from_lists(pats, txts)
        end = {"pat": int(b.pat_off[6] + b.pat_len[6]), "txt": int(b.txt_off[6] + b.txt_len[6])}
        assert end[side] % 4 == 1
        order = np.array([0, 1, 6, 3, 4, 5, 2])
        b = gabgen.PairBatch(b.pat, b.pat_off[order], b.pat_len[order], b.txt, b.txt_off[order], b.txt_len[order])
        out[side + "_end_past_slab"] = Refusal(_frozen(b), (2,), end["pat"] if side == "pat" else len(b.pat),
                                               end["txt"] if side == "txt" else len(b.txt), None)
    pats, txts = _good_strings(rng, 9)
    pats[6] = _rand(rng, MAX_LEN + 1); txts[2] = _rand(rng, MAX_LEN + 1)
    b = gabgen.pairs_from_lists(pats, txts)
    out["two_bad"] = Refusal(_frozen(b), (2, 6), len(b.pat), len(b.txt), "classify")
    return out


@functools.lru_cache(maxsize=None)
def exact_slabs():
    """-> (batch, pat_bytes, txt_bytes): both slabs end with their last string's last byte, on a multiple of 4"""
    rng = np.random.default_rng(17)
    pats, txts = _good_strings(rng, 7)
    pats[-1] += _rand(rng, -sum(len(s) for s in pats) % 4)
    txts[-1] += _rand(rng, -sum(len(s) for s in txts) % 4)
    b = gabgen.pairs_from_lists(pats, txts)
    pe, te = int(b.pat_off[-1] + b.pat_len[-1]), int(b.txt_off[-1] + b.txt_len[-1])
    assert pe % 4 == 0 and te % 4 == 0
    return _frozen(b), pe, te


def refusal_message(r, host=False):
    """the part of the error text that names the count and the pair"""
    if host and r.host == "scan":
        return "negative offset/length at pair %d" % r.bad[0]
    return "%d pair(s) violate the limits (first: pair %d)" % (len(r.bad), r.bad[0])


BATCHES = {"bv_routes": lambda: bv_routes()[0], "all_reject": all_reject, "none_reject": none_reject, "all_long": all_long,
           "switch_2048": switch_2048, "bytes_256": bytes_256, "chunk_edges": chunk_edges, "classify_stride": classify_stride,
           "global_second_trip": global_second_trip, "limits_accepted": limits_accepted, "exact_slabs": lambda: exact_slabs()[0]}
BATCHES.update({"width_%d" % D: functools.partial(width, D) for D in range(1, 9)})
