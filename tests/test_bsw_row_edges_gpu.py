"""GPU: the row boundary of the 8-bit bsw kernel -- the head cell, the remainder pair and the tail cell of the column sweep at
every parity and width of the band, the per-row products (24-bit multiplies and a left-edge term carried from row to row) at the
bounds of their operands, and the slow paths of the trimming (zero trim past its window on either side, a band that ends left of
column 3, the exit's bound pass) when different lanes of one wave take different ones in the same row.

Every case goes through tests/test_bsw_early_exit_gpu.py's check(..., full=True): the score-only and the six-field call on one
handle, scores and fields equal to pyoracle.bsw with no tolerance, cells equal to the model's.  What a batch is meant to contain is
asserted on the CPU from the model's row trace (gabgen.bsw_exit_trace) first.  A batch of 64 pairs with one sort key (query
length, reference length / 8, h0 / 32) is exactly one wave, and its lanes sweep row i together."""
import numpy as np
import pytest

from tools import gabgen
from tests.util import bsw_oracle_params
from tests.test_bsw_early_exit_gpu import KERNEL_CASES, check
from tests.test_bsw_left_prune import handmade, scores_match, with_zdrop
from tests.test_bsw_right_prune import ZERO_ROWS
from tests.test_bsw_row_tail_gpu import DEFAULTS, F, cut, one_wave, trace

pytestmark = pytest.mark.gpu

GUARDS = F["zdrop_guard"] | F["right_edge_guard"] | F["zero_row_guard"]


def wave_rows(off):
    """-> (r, trace indices of the lanes still sweeping in the wave's row r)"""
    rows = np.diff(off)
    for r in range(int(rows.max())):
        yield r, off[:-1][rows > r] + r


def slow_paths(beg, end, flags, at):
    """the four slow paths of the trimming, one boolean per lane of `at`"""
    return [(flags[at] & F["lz4"]) != 0, (flags[at] & F["tz4"]) != 0,
            (end[at] <= 2) & ((flags[at] & F["right_drop"]) != 0), (flags[at] & F["bound_pass"]) != 0]


def test_mixed_slow_paths_in_one_wave_row(monkeypatch, capfd):
    """rows in which at least three of the four slow paths are taken, by lanes that differ in the paths they take; and rows in
    which exactly one lane takes exactly one"""
    batch = one_wave(25, 40, 48, np.arange(64) % 32)
    off, _, beg, end, flags, _ = trace(batch, ZERO_ROWS)
    mixed = single = 0
    for _, at in wave_rows(off):
        kinds = slow_paths(beg, end, flags, at)
        taken = np.array(kinds).T                           # lane x path
        lanes = taken.any(axis=1)
        mixed += sum(k.any() for k in kinds) >= 3 and len({tuple(t) for t in taken[lanes]}) >= 3
        single += lanes.sum() == 1 and taken.sum() == 1
    print(f"rows with three or more slow paths on different lanes: {mixed}; rows with one lane on one slow path: {single}")
    assert mixed >= 1 and single >= 1
    check(ZERO_ROWS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


@pytest.mark.parametrize("name,ps,seed", [("defaults", DEFAULTS, 29), ("zero_rows", ZERO_ROWS, 26)])
def test_every_parity_of_both_edges_at_band_widths_1_to_9(monkeypatch, capfd, name, ps, seed):
    """w = 4: no band is wider than 9 cells.  One wave holds every width 1 .. 9 with an even and with an odd `beg` (the parity of
    `end` follows), rows in which a lane without a loop trip sits beside one with two, a row with a band that is only a head cell
    beside one that is only a tail cell, and pairs whose band grows by two cells behind a row that ended on a lower half -- over
    the upper half that row left untouched."""
    ps = with_zdrop(ps, 100, 4)
    batch = one_wave(seed, 32, 40, np.arange(64) % 8)
    off, i, beg, end, _, _ = trace(batch, ps)
    width = end - beg
    assert width.max() <= 9
    assert {(w, p) for w in range(1, 10) for p in (0, 1)} <= {(int(w), int(p)) for w, p in zip(width, beg & 1)}
    first = beg + (beg & 1)                                 # the sweep's first even column
    trips = np.where(first + 1 < end, np.maximum(0, (end - first) // 4), 0)
    beside = head_tail = 0
    for _, at in wave_rows(off):
        beside += (trips[at] == 0).any() and (trips[at] >= 2).any()
        head_tail += ((width[at] == 1) & (beg[at] & 1 == 1)).any() and ((width[at] == 1) & (beg[at] & 1 == 0)).any()
    grown = (i[1:] == i[:-1] + 1) & (end[:-1] & 1 == 1) & (end[1:] == end[:-1] + 2)
    print(f"{name}: rows with no trip beside two: {beside}, only a head cell beside only a tail cell: {head_tail}, "
          f"bands grown over a stale upper half: {grown.sum()}")
    assert beside >= 1 and head_tail >= 1 and grown.any()
    check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def long_tail_pairs(qlen, h0, n=64, tlen=32767, seed=41):
    """hand-made: the reference starts with the query (with a mismatch every 16 bases in every other pair) and goes on with random
    bases up to GAB_BSW_MAX_TLEN: rows_left = tlen - 1 - i is as large as it gets, and behind the query's end the row maximum decays
    along the deletion path, so the reference row of the z-drop test runs far ahead of the best row's"""
    rng = np.random.default_rng(seed)
    refs, qrys = [], []
    for k in range(n):
        q = rng.integers(0, 4, qlen).astype(np.uint8)
        r = np.concatenate([q, rng.integers(0, 4, tlen - qlen).astype(np.uint8)])
        if k & 1:
            r[7:qlen:16] ^= 1
        if k % 8 == 7:
            r = np.delete(r, qlen // 2)[:tlen - 1]         # a deleted base, and a reference one row short of the limit
        refs.append(r); qrys.append(q)
    return gabgen.bsw_from_arrays(refs, qrys, [h0] * n)


@pytest.mark.parametrize("want_kernel,ps,qmax,h0_of", KERNEL_CASES[:4], ids=[k for k, *_ in KERNEL_CASES[:4]])
def test_products_at_their_bounds(monkeypatch, capfd, want_kernel, ps, qmax, h0_of):
    """tlen = GAB_BSW_MAX_TLEN under every <SYM, MS1>: the set's own gap penalties, e_del = e_ins = 1, a large e_del (the 8-bit
    kernel's condition limits the scores, not the penalties), and a z-drop that the long deletion tail behind the query's end does
    not outrun: the six-field sweep follows it, |di - dj| growing by one per row, until the band limit the gap penalties set,
    (qlen * max_sc + end_bonus - o_del) / e_del + 1 columns, or the set's own w cuts the query's last column off -- twenty-five
    rows or more behind the best one.  max_sc * qcap <= 255 bounds the score of the 8-bit kernel, so max_sc = 127 cannot reach it at any query length
    (qcap >= 16); that set runs whichever kernel the launch picks and is checked all the same, beside max_sc = 0 and the largest
    score the 8-bit kernel takes at qcap = 16."""
    a = ps[0]
    qlen = min(qmax, 48)
    h0 = max(0, min(255 - ((qlen + 15) // 16 * 16) * max(a, 1), 95))
    batch = long_tail_pairs(qlen, h0)
    sets = [(ps, want_kernel),
            (ps[:4] + (1,) + ps[5:6] + (1,) + ps[7:], None),                   # e_del = e_ins = 1
            (ps[:4] + (30000,) + ps[5:], None),                                # a large e_del
            (ps[:3] + (1, 1) + ps[5:7] + (2000,) + ps[8:], None)]              # o_del = e_del = 1 under a z-drop: a long tail
    for p, want in sets:
        scores_match(batch, p)
        check(p, batch, monkeypatch, capfd, want, full=True)
    rows = gabgen.bsw_exit_trace(batch, bsw_oracle_params(*sets[3][0]), early_exit=False, prune=False)[1]      # the six-field sweep
    print(f"rows of the full sweep under the z-drop set: up to {rows.max()} for a query of {qlen}")
    assert rows.max() >= qlen + 25
    short = long_tail_pairs(14, 8, tlen=4096, seed=42)
    for a_, want in ((0, None), (15, None), (127, None)):
        p = (a_,) + ps[1:]
        scores_match(short, p)
        check(p, short, monkeypatch, capfd, want, full=True)


@pytest.mark.parametrize("name,ps,pair", [("zero_rows", ZERO_ROWS, 605), ("zero_rows_long", ZERO_ROWS, 40), ("defaults", DEFAULTS, 810)])
def test_a_lane_restarts_in_a_row_where_another_takes_a_slow_path(monkeypatch, capfd, name, ps, pair):
    """a pair of handmade() that one of the guards sends back, with 63 more of them cut to its lengths: one key, one wave"""
    hb = handmade()
    b = cut(hb, np.arange(hb.n), h0=np.minimum(hb.h0, 31))
    q, t = int(b.len2[pair]), int(b.len1[pair])
    others = np.flatnonzero((b.len2 >= q) & (b.len1 >= t) & (np.arange(b.n) != pair))[:63]
    assert len(others) == 63
    batch = cut(b, np.concatenate([[pair], others]), qlen=q, tlen=t)
    assert len(set(batch.len2)) == 1 and len(set(batch.len1 >> 3)) == 1 and len(set(batch.h0 >> 5)) == 1
    off, _, beg, end, flags, _ = trace(batch, ps)
    fired = np.flatnonzero((flags[off[0]:off[1]] & GUARDS) != 0)
    assert len(fired) >= 1
    r = int(fired[0])
    rows = np.diff(off)
    at = off[1:-1][rows[1:] > r] + r
    slow = np.array(slow_paths(beg, end, flags, at)).any(axis=0)
    print(f"{name}: lane 0 abandons its pass in row {r}; {slow.sum()} other lanes take a slow path there")
    assert slow.any()
    scores_match(batch, ps)
    check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)
