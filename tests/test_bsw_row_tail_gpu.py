"""GPU: the per-row code of the 8-bit bsw kernel behind the column sweep -- score-only as a template argument, the one block that
trims and prunes both band edges, the zeroing of dropped cells, row -1 and the query nibbles of the per-pair set-up.

Every case goes through tests/test_bsw_early_exit_gpu.py's check(..., full=True): the score-only AND the six-field call on one
handle, scores and all six fields equal to pyoracle.bsw with no tolerance, last_stats()["cells"] of the score-only call equal to
the cell sum of tools/gen/bsw_exit_model.c (abandoned passes included), that of the six-field call equal to the full sweep's,
and the GAB_BSW_TRACE lines naming the dp8 instantiation that ran.  What a batch is meant to contain -- band parities, numbers of
dropped cells, zero trims past the window, guards that fire -- is asserted on the CPU from the model's row trace
(gabgen.bsw_exit_trace), so a case cannot silently stop exercising its path.  Lanes of a wave sweep row i together, and a batch
of 64 pairs with one sort key (query length, reference length / 8, h0 / 32) is exactly one wave."""
import numpy as np
import pytest

from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params
from tests.test_bsw_early_exit_gpu import KERNEL_CASES, check, generator_batch
from tests.test_bsw_left_prune import handmade, scores_match, with_zdrop
from tests.test_bsw_right_prune import ZERO_ROWS, handmade_right

pytestmark = pytest.mark.gpu

DEFAULTS = BSW_PARAM_SETS[0]
F = gabgen.BSW_TRACE_FLAGS


def trace(batch, ps):
    """-> (off, i, beg, end, flags, drops): the model's traced rows and the row index i of each inside its pass"""
    out = gabgen.bsw_exit_trace(batch, bsw_oracle_params(*ps))
    off, beg, end, flags, drops = out[5:]
    i = np.arange(off[-1]) - np.repeat(off[:-1], np.diff(off))
    return off, i, beg.astype(np.int64), end.astype(np.int64), flags, drops


def cut(b, idx, qlen=None, tlen=None, h0=None):
    """pairs idx of b, queries / references cut to qlen / tlen bases"""
    idx = np.asarray(idx)
    len2 = b.len2[idx].copy() if qlen is None else np.minimum(b.len2[idx], qlen).astype(np.int32)
    len1 = b.len1[idx].copy() if tlen is None else np.minimum(b.len1[idx], tlen).astype(np.int32)
    return gabgen.BswBatch(b.ref, b.ref_off[idx].copy(), b.qry, b.qry_off[idx].copy(), len1, len2,
                           b.h0[idx].copy() if h0 is None else np.asarray(h0, np.int32))


def one_wave(seed, qlen, tlen, h0):
    """64 read-like pairs with one sort key"""
    b = gabgen.bsw(seed, 4096, 0)
    idx = np.flatnonzero((b.len2 >= qlen) & (b.len1 >= tlen))[:64]
    assert len(idx) == 64
    h0 = np.array(np.broadcast_to(np.asarray(h0, np.int32), (64,)))
    assert len(set(h0 >> 5)) == 1
    return cut(b, idx, qlen, tlen, h0)


def test_query_lengths_1_to_9(monkeypatch, capfd):
    """end <= 9: the edge words of the trimming are clamped duplicates, the band is 1 .. 5 cells wide, no loop trip, and rows that are
    only a head cell, only a remainder pair, only a tail cell"""
    b = gabgen.bsw(21, 9 * 256, 0)
    rng = np.random.default_rng(21)
    batch = cut(b, np.arange(b.n), qlen=np.repeat(np.arange(1, 10), 256), h0=rng.integers(0, 31, b.n))
    batch.len1[:] = np.minimum(batch.len1, rng.integers(1, 24, b.n))
    assert sorted(set(batch.len2)) == list(range(1, 10))
    _, _, beg, end, _, _ = trace(batch, DEFAULTS)
    width = end - beg
    assert set(range(1, 6)) <= set(width)
    assert ((beg & 1) == 1)[width == 1].any() and ((beg & 1) == 0)[width == 1].any() and ((beg & 1) == 0)[width == 2].any()
    for ps in (DEFAULTS, ZERO_ROWS):
        check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_both_parities_of_both_edges_in_one_wave(monkeypatch, capfd):
    batch = one_wave(22, 60, 72, np.arange(64) % 32)
    off, i, beg, end, _, _ = trace(batch, DEFAULTS)
    rows = np.diff(off)
    mixed = []
    for r in range(int(rows.max())):
        at = off[:-1][rows > r] + r                      # the lanes still sweeping in the wave's row r
        if len(set(beg[at] & 1)) == 2 and len(set(end[at] & 1)) == 2:
            mixed.append(r)
    print(f"{len(mixed)} of {rows.max()} rows hold both parities of beg and of end among the wave's lanes")
    assert len(mixed) > 0
    check(DEFAULTS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_one_to_four_cells_dropped_on_either_side_and_on_both(monkeypatch, capfd):
    batch = generator_batch(23, 0, 151, None, n=8192)
    batch.h0[:] = np.minimum(batch.h0, 95)
    _, _, _, _, _, drops = trace(batch, DEFAULTS)
    left, right = drops & 15, drops >> 4
    assert {1, 2, 3, 4} <= set(left) and {1, 2, 3, 4} <= set(right) and left.max() <= 4 and right.max() <= 4
    both = set(zip(left[(left > 0) & (right > 0)], right[(left > 0) & (right > 0)]))
    print(f"rows that drop on both sides: {sorted(both)}")
    assert {l for l, _ in both} == {1, 2, 3, 4} and {r for _, r in both} == {1, 2, 3, 4}
    check(DEFAULTS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_zero_trim_past_the_window_and_all_three_guards(monkeypatch, capfd):
    """mismatch score -128: rows of zeros, so the zero trim runs past its four-cell window on the left, on the right and on both in
    one row; and on the read-like pairs each of the three guards sends a pair back"""
    b = gabgen.bsw(2, 50000, 0)
    batch = cut(b, np.arange(b.n), h0=np.minimum(b.h0, 95))
    _, _, _, _, flags, _ = trace(batch, ZERO_ROWS)
    lz4, tz4 = (flags & F["lz4"]) != 0, (flags & F["tz4"]) != 0
    print(f"rows: lz4 {lz4.sum()} tz4 {tz4.sum()} both {(lz4 & tz4).sum()}; guards: z-drop {((flags & F['zdrop_guard']) != 0).sum()} "
          f"right-edge {((flags & F['right_edge_guard']) != 0).sum()} zero-row {((flags & F['zero_row_guard']) != 0).sum()}")
    assert (lz4 & ~tz4).any() and (tz4 & ~lz4).any() and (lz4 & tz4).any()
    for g in ("zdrop_guard", "right_edge_guard", "zero_row_guard"):
        assert (flags & F[g]).any(), g
    check(ZERO_ROWS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_handmade_batches_with_zero_rows(monkeypatch, capfd):
    for b in (handmade(), handmade_right()):
        batch = cut(b, np.arange(b.n), h0=np.minimum(b.h0, 45))
        for ps in (DEFAULTS, ZERO_ROWS, with_zdrop(DEFAULTS, 10)):
            scores_match(batch, ps)
            check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_column_zero_with_a_live_and_with_a_dead_next_row_edge(monkeypatch, capfd):
    """beg == 0 rows whose next-row edge hb = h0 - o_del - e_del * (i + 2) is positive (h0 = 90: the left prune may not leave column
    0 while it can still reach best) and rows where it is not (h0 <= 7)"""
    b = handmade()
    keep = np.flatnonzero((b.len2 <= 120) & (b.len1 >= 2))[:1024]
    h0 = np.where(np.arange(len(keep)) % 2 == 0, 90, np.arange(len(keep)) % 8)
    batch = cut(b, keep, h0=h0)
    off, i, beg, end, _, _ = trace(batch, DEFAULTS)
    hb = np.repeat(batch.h0, np.diff(off)) - DEFAULTS[3] - DEFAULTS[4] * (i + 2)
    at0 = (beg == 0) & (i > 0)
    print(f"rows with beg == 0 behind row 0: {(at0 & (hb > 0)).sum()} with hb > 0, {(at0 & (hb <= 0)).sum()} with hb <= 0")
    assert (at0 & (hb > 0)).any() and (at0 & (hb <= 0)).any()
    check(DEFAULTS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_pruned_lanes_and_lanes_with_the_prune_off_in_one_wave(monkeypatch, capfd):
    """w = 40, qlen = 60 > w + 1: the prune is on only while h0 - oe_ins - (w + 1) * e_ins <= 0, that is h0 <= 48 -- half the lanes"""
    ps = with_zdrop(DEFAULTS, 100, 40)
    h0 = np.where(np.arange(64) % 2 == 0, 40, 60)
    batch = one_wave(24, 60, 72, h0)
    oe_ins, e_ins, w = ps[5] + ps[6], ps[6], ps[9]
    on = batch.h0 - oe_ins - (w + 1) * e_ins <= 0
    assert on.sum() == 32 and (batch.len2 > w + 1).all()
    off, _, _, _, flags, _ = trace(batch, ps)
    drop = np.add.reduceat((flags & (F["left_drop"] | F["right_drop"])) != 0, off[:-1]) > 0
    assert drop[on].all() and not drop[~on].any()
    check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_zdrop_guard_restarts(monkeypatch, capfd):
    ps = with_zdrop(DEFAULTS, 20, 100)
    batch = generator_batch(410, 1, 151, None, n=8192)
    batch.h0[:] = batch.h0 % 96
    _, _, _, _, flags, _ = trace(batch, ps)
    assert (flags & F["zdrop_guard"]).any()
    check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


@pytest.mark.parametrize("want_kernel,ps,qmax,h0_of", KERNEL_CASES[:4], ids=[k for k, *_ in KERNEL_CASES[:4]])
@pytest.mark.parametrize("mode", [0, 1])
def test_every_instantiation(monkeypatch, capfd, want_kernel, ps, qmax, h0_of, mode):
    batch = generator_batch(120 + mode, mode, qmax, h0_of, n=8192)
    check(ps, batch, monkeypatch, capfd, want_kernel, full=True)
