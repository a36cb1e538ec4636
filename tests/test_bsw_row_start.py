"""CPU half of tests/test_bsw_row_start_gpu.py: the batches that test runs, and the proof that they hold the rows the 8-bit bsw
kernel's row tail can get wrong (bsw.hip, bsw_dp8; profiles/bsw_row_start.md).

The row tail moves both band edges from two four-cell windows, zeroes the cells the right prune drops, and hands the next row its
left edge; its flags, window moves and clamps are straight code.  What can go wrong is a matter of which rows a batch holds, and
the model's row trace (gabgen.bsw_exit_trace) says which: the right prune zeroing cells inside the words the next row starts with
(a right drop in a narrow band), every advance of the left edge at either parity, a zero trim past its window (lz4), a row that
starts at the band clamp i - w, and a pair that a guard sends through a second pass.  No case may pass without its rows."""
import numpy as np
import pytest

from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params

DEFAULTS = BSW_PARAM_SETS[0]
F = gabgen.BSW_TRACE_FLAGS
GUARDS = F["zdrop_guard"] | F["right_edge_guard"] | F["zero_row_guard"]
N_GEN = 4096
HAND_W = (0, 1, 2, 3, 100)


def max_sc(ps):
    """largest score of bwa_fill_scmat(a, b, ambig)"""
    a, b, amb = ps[:3]
    return max(a, -b, amb)


def byte_qmax(ps):
    """largest query-length class bound (a multiple of 16, at most 160) whose cells fit a byte with some h0 left; 0: none, the
    parameter set never runs the byte kernel"""
    m = max_sc(ps)
    if m < 0:
        return 0
    q = 160
    while q >= 16 and q * m > 255 - 15:
        q -= 16
    return max(q, 0)


BYTE_SETS = [k for k, ps in enumerate(BSW_PARAM_SETS) if byte_qmax(ps) >= 16]


def byte_batch(ps, seed, mode, n=N_GEN):
    """the first n generator pairs of the mode, queries cut to the longest class the byte kernel takes under ps and h0 folded
    into what that class leaves: max(h0) + qcap * max_sc <= 255"""
    b = gabgen.bsw(seed, n, mode)
    qmax = byte_qmax(ps)
    len2 = np.minimum(b.len2, qmax).astype(np.int32)
    h0 = (b.h0 % (255 - qmax * max_sc(ps) + 1)).astype(np.int32)
    return gabgen.BswBatch(b.ref, b.ref_off.copy(), b.qry, b.qry_off.copy(), b.len1.copy(), len2, h0)


def with_w(ps, w):
    return ps[:9] + (w,)


def handmade(seed=7, n=2048):
    """query length 4 .. 12, h0 1 .. 24: a reference that follows the query with a substitution, a deleted or an inserted base
    here and there, and a random tail of 0 .. 11 bases; every eighth pair has nothing in common with its query"""
    rng = np.random.default_rng(seed)
    refs, qrys, h0s = [], [], []
    for k in range(n):
        q = rng.integers(0, 4, 4 + k % 9).astype(np.uint8)
        r = []
        for c in q:
            u = rng.random()
            if u < 0.08:
                r.append((c + 1 + rng.integers(0, 3)) % 4)
            elif u < 0.13:
                continue
            elif u < 0.18:
                r += [c, rng.integers(0, 4)]
            else:
                r.append(c)
        if k % 8 == 7:
            r = list(3 - q)
        r = np.array(r + list(rng.integers(0, 4, rng.integers(0, 12))) or [0], np.uint8)
        refs.append(r); qrys.append(q); h0s.append(1 + (k * 5) % 24)
    return gabgen.bsw_from_arrays(refs, qrys, h0s)


def rows(batch, ps):
    """the model's row trace -> dict of per-row arrays: i (row index inside its pass), beg, end, flags, and nxt: the row is followed
    by another row of the same pass; restarted: per pair"""
    out = gabgen.bsw_exit_trace(batch, bsw_oracle_params(*ps))
    restarted, off, beg, end, flags, _ = out[4:]
    n = int(off[-1])
    first = np.zeros(n, bool)
    first[off[:-1][np.diff(off) > 0]] = True
    first[1:] |= (flags[:-1] & GUARDS) != 0               # the row behind an abandoned pass starts the second one
    start = np.maximum.accumulate(np.where(first, np.arange(n), 0))
    nxt = np.zeros(n, bool)
    nxt[:-1] = ~first[1:]
    return dict(i=np.arange(n) - start, beg=beg.astype(np.int64), end=end.astype(np.int64), flags=flags, nxt=nxt,
                restarted=restarted)


def advances(t):
    """{(advance of beg into the next row, parity of the old beg)} over the rows that have a next row"""
    at = np.flatnonzero(t["nxt"])
    return set(zip((t["beg"][at + 1] - t["beg"][at]).tolist(), (t["beg"][at] & 1).tolist()))


def narrow_right_drop(t):
    return ((t["flags"] & F["right_drop"]) != 0) & (t["end"] - t["beg"] <= 8)


def test_the_byte_sets():
    """the parameter sets the GPU half runs: those whose scores leave a byte kernel a class of at least 16 columns"""
    assert 0 in BYTE_SETS and len(BYTE_SETS) >= 10
    assert [max_sc(BSW_PARAM_SETS[k]) for k in BYTE_SETS if max_sc(BSW_PARAM_SETS[k]) > 15] == []
    for k in BYTE_SETS:
        ps = BSW_PARAM_SETS[k]
        b = byte_batch(ps, 5000 + k, 0, 256)
        assert int(b.h0.max()) + ((int(b.len2.max()) + 15) // 16 * 16) * max_sc(ps) <= 255


@pytest.mark.parametrize("mode", [0, 1])
def test_generator_batches_at_the_defaults_hold_the_rows(mode):
    t = rows(byte_batch(DEFAULTS, 5000, mode), DEFAULTS)
    adv = advances(t)
    print(f"mode {mode}: advances {sorted(adv)}, narrow right drops {narrow_right_drop(t).sum()}, lz4 {((t['flags'] & F['lz4']) != 0).sum()}, "
          f"restarted {int(t['restarted'].sum())}")
    assert {(a, p) for a in range(5) for p in (0, 1)} <= adv
    assert narrow_right_drop(t).any()
    # a narrow band that drops on the right and whose left edge moves in the same row, and one whose left edge stays: both windows
    # of the trimming then overlap, and the cells the right prune zeroes lie in the pair words the next row starts with
    at = np.flatnonzero(narrow_right_drop(t) & t["nxt"])
    assert (t["beg"][at + 1] > t["beg"][at]).any() and (t["beg"][at + 1] == t["beg"][at]).any()


def test_the_sets_together_hold_lz4_rows_clamped_rows_and_restarts():
    """... and WHICH (set, mode) batches carry each condition (printed): the defaults have lz4 rows in both modes and at least
    eight sets have some (a set whose prune is off, or whose band is a column or two wide, has none); the sets with a band of at
    most five columns have rows on the clamp in both modes (a wider band keeps the clamp left of the trimmed edge, so the count
    means nothing there); restarts come from the defaults' mode 1 batch and from at least two more"""
    lz4, clamp, restarts = {}, {}, {}
    for k in BYTE_SETS:
        ps = BSW_PARAM_SETS[k]
        for mode in (0, 1):
            t = rows(byte_batch(ps, 5000 + k, mode), ps)
            lz4[k, mode] = int(((t["flags"] & F["lz4"]) != 0).sum())
            restarts[k, mode] = int(t["restarted"].sum())
            if ps[9] <= 5:
                clamp[k, mode] = int(((t["beg"] > 0) & (t["beg"] == t["i"] - ps[9])).sum())
    print(f"lz4 rows {lz4}\nrows that start at the band clamp {clamp}\nrestarted pairs {restarts}")
    assert lz4[0, 0] > 0 and lz4[0, 1] > 0 and sum(lz4[k, 0] + lz4[k, 1] > 0 for k in BYTE_SETS) >= 8, lz4
    assert len(clamp) >= 6 and all(n > 0 for n in clamp.values()), clamp
    assert restarts[0, 1] > 0 and sum(n > 0 for n in restarts.values()) >= 3, restarts


@pytest.mark.parametrize("w", HAND_W)
def test_handmade_pairs_hold_the_rows(w):
    ps = with_w(DEFAULTS, w)
    b = handmade()
    assert sorted(set(b.len2)) == list(range(4, 13)) and b.h0.max() <= 24
    t = rows(b, ps)
    adv = advances(t)
    print(f"w {w}: advances {sorted(adv)}, narrow right drops {narrow_right_drop(t).sum()}")
    assert (t["end"] - t["beg"] <= 8).mean() > 0.5
    if w <= 3:                                              # the left edge IS the clamp: one column per row, from row w + 1 on
        assert ((t["beg"] > 0) & (t["beg"] == t["i"] - w)).any()
        assert {(1, 0), (1, 1)} <= adv
    else:                                                   # the zero trim and the left prune move it
        assert {(a, p) for a in (0, 1, 2) for p in (0, 1)} <= adv
        assert narrow_right_drop(t).any()
