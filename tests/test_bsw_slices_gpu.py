"""GPU: a large bsw batch sorted in two slices, the second one's sort running beside the first one's DP (bsw.hip, bsw_run_device_impl).

A call of at least slice_min pairs cuts its pair range into slice 0 (the first slice0 pairs) and slice 1 (the rest); each slice has
its own histogram, class boundaries, statistics and class launches.  GAB_BSW_SLICE=slice0,slice_min (gab_internal.h: gab_tuning)
lowers both, so that every case here slices a few thousand generator pairs.  Unless a case says otherwise it checks: scores equal
to pyoracle.bsw with no tolerance; last_stats()["cells"] of the score-only call equal to tools/gen/bsw_exit_model.c (default rule)
and to the same batch run unsliced; all six result fields equal to the oracle's.  With GAB_BSW_TRACE every DP launch prints a line,
and a sliced call appends " slice K" to it.

The oracle and the model are computed once for one generator batch; the cases take subsets and permutations of its pairs (both
are per-pair functions), and only the case that changes h0 computes its own."""
import re

import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"\[gab_bsw_dp \S+\] class (\d+) qcap (\d+) pairs (\d+) bits (\d+) sym (\d) ms1 (\d)(?: slice (\d+))?")
DEFAULTS = BSW_PARAM_SETS[0]
N_BASE = 12000
SLICE0, SLICE_MIN = 5037, 8000      # the boundary is no multiple of 64 (a wave) nor of 256 (a sort workgroup)


def launches(err):
    """[(slice or None, class, pairs, bits)] of the DP launches the trace lines report"""
    return [(None if sl == "" else int(sl), int(c), int(n), int(bits)) for c, _, n, bits, _, _, sl in TRACE.findall(err)]


def subset(batch, idx, h0=None, len2=None):
    idx = np.asarray(idx)
    return gabgen.BswBatch(batch.ref, batch.ref_off[idx].copy(), batch.qry, batch.qry_off[idx].copy(), batch.len1[idx].copy(),
                           batch.len2[idx].copy() if len2 is None else np.asarray(len2, np.int32),
                           batch.h0[idx].copy() if h0 is None else np.asarray(h0, np.int32))


def reference(batch):
    """(six-field oracle result per pair, model's score-only cells per pair)"""
    p = bsw_oracle_params(*DEFAULTS)
    want = pyoracle.bsw(batch, p)
    mscore, _, mcells, _ = gabgen.bsw_exit_model(batch, p)
    np.testing.assert_array_equal(mscore, want[:, 0])
    return want, mcells


@pytest.fixture(scope="module")
def base():
    b = gabgen.bsw(4301, N_BASE, 1)
    want, mcells = reference(b)
    want.setflags(write=False); mcells.setflags(write=False)
    return b, want, mcells


@pytest.fixture()
def sw(monkeypatch):
    from genarchbench_amd.bsw import BandedPairWiseSW
    monkeypatch.setenv("GAB_BSW_TRACE", "1")
    h = BandedPairWiseSW()
    yield h
    h.close()


class Dev:
    """a batch's arrays on the GPU"""
    def __init__(self, batch):
        import torch
        self.n = batch.n
        dev = torch.device("cuda:0")
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        self.args = (t(batch.ref), t(batch.ref_off), t(batch.qry), t(batch.qry_off), t(batch.len1), t(batch.len2), t(batch.h0))
        torch.cuda.synchronize()      # (the calls may run on another stream than the one that copied)


def call(sw, d, slices, monkeypatch, capfd, full=False, stream=None):
    """one run_device call with GAB_BSW_SLICE = slices (None: unset) -> (scores or six fields, cells, launches)"""
    import torch
    if slices is None:
        monkeypatch.delenv("GAB_BSW_SLICE", raising=False)
    else:
        monkeypatch.setenv("GAB_BSW_SLICE", "%d,%d" % slices)
    dev = torch.device("cuda:0")
    stream = stream or torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        score = torch.full((d.n,), -7, dtype=torch.int32, device=dev)
        res = torch.full((d.n, 6), -7, dtype=torch.int32, device=dev) if full else None
        capfd.readouterr()
        sw.run_device(*d.args, score, res, stream=stream.cuda_stream)
        stream.synchronize()
    ran = launches(capfd.readouterr().err)
    got = score.cpu().numpy()
    if full:
        np.testing.assert_array_equal(res.cpu().numpy()[:, 0], got)
        got = res.cpu().numpy()
    return got, sw.last_stats()["cells"], ran


def check_sliced(sw, batch, want, mcells, monkeypatch, capfd, slices=(SLICE0, SLICE_MIN), stream=None):
    """the three checks of the module docstring on a call that must slice -> (launches of the score-only call, its cells)"""
    d = Dev(batch)
    got, cells, ran = call(sw, d, slices, monkeypatch, capfd, stream=stream)
    bad = np.flatnonzero(got != want[:, 0])
    assert len(bad) == 0, f"{len(bad)} of {batch.n} scores differ, first: pair {bad[0]} got {got[bad[0]]} want {want[bad[0], 0]}; {ran}"
    assert {sl for sl, *_ in ran} == {0, 1}, ran
    assert sum(n for sl, _, n, _ in ran if sl == 0) == slices[0] and sum(n for sl, _, n, _ in ran if sl == 1) == batch.n - slices[0], ran
    plain, plain_cells, plain_ran = call(sw, d, None, monkeypatch, capfd, stream=stream)
    assert {sl for sl, *_ in plain_ran} == {None}, plain_ran
    np.testing.assert_array_equal(plain, got)
    print(f"cells: model {int(mcells.sum())} sliced {cells} unsliced {plain_cells}")
    assert cells == int(mcells.sum()) and cells == plain_cells
    res, _, ran6 = call(sw, d, slices, monkeypatch, capfd, full=True, stream=stream)
    np.testing.assert_array_equal(res, want)
    assert [x[:3] for x in ran6] == [x[:3] for x in ran]
    return ran, cells


# ------------------------------------------------------------------------------------------------ the boundary
def test_odd_boundary(base, sw, monkeypatch, capfd):
    """neither the boundary nor slice 1 is a multiple of 64"""
    b, want, mcells = base
    n = 9001
    assert SLICE0 % 64 and (n - SLICE0) % 64
    check_sliced(sw, subset(b, np.arange(n)), want[:n], mcells[:n], monkeypatch, capfd)


def test_one_pair_slice(base, sw, monkeypatch, capfd):
    """n = boundary + 1: slice 1 is one pair, one launch of one wave"""
    b, want, mcells = base
    n = SLICE0 + 1
    ran, _ = check_sliced(sw, subset(b, np.arange(n)), want[:n], mcells[:n], monkeypatch, capfd, slices=(SLICE0, SLICE0 + 1))
    assert [(c, k) for sl, c, k, _ in ran if sl == 1] == [((int(b.len2[SLICE0]) - 1) // 16, 1)], ran


def test_below_slice_min_is_unsliced(base, sw, monkeypatch, capfd):
    """n = slice_min - 1: the call and its trace lines are those of a handle that knows no slices"""
    b, want, mcells = base
    n = SLICE_MIN - 1
    d = Dev(subset(b, np.arange(n)))
    got, cells, ran = call(sw, d, (SLICE0, SLICE_MIN), monkeypatch, capfd)
    plain, plain_cells, plain_ran = call(sw, d, None, monkeypatch, capfd)
    assert ran == plain_ran and len(ran) == 1 and ran[0][0] is None and ran[0][2] == n, (ran, plain_ran)
    np.testing.assert_array_equal(got, want[:n, 0])
    np.testing.assert_array_equal(plain, got)
    assert cells == plain_cells == int(mcells[:n].sum())
    res, _, _ = call(sw, d, (SLICE0, SLICE_MIN), monkeypatch, capfd, full=True)
    np.testing.assert_array_equal(res, want[:n])


# ------------------------------------------------------------------------------------------------ classes per slice
def test_class_in_one_slice_only(base, sw, monkeypatch, capfd):
    """class 3 occurs only in slice 1 and class 7 only in slice 0: the empty class launches nothing"""
    b, want, mcells = base
    cls = (b.len2 - 1) // 16
    first = np.flatnonzero(cls != 3)[:SLICE0]
    rest = np.setdiff1d(np.flatnonzero(cls != 7), first)[:4100]
    idx = np.concatenate([first, rest])
    assert len(first) == SLICE0 and (cls[first] == 7).any() and (cls[rest] == 3).any() and len(idx) >= SLICE_MIN
    ran, _ = check_sliced(sw, subset(b, idx), want[idx], mcells[idx], monkeypatch, capfd)
    for sl, part in ((0, first), (1, rest)):
        assert {c: k for s, c, k, _ in ran if s == sl} == {int(c): int(k) for c, k in zip(*np.unique(cls[part], return_counts=True))}, ran
    assert 3 not in {c for s, c, _, _ in ran if s == 0} and 7 not in {c for s, c, _, _ in ran if s == 1}


def test_cell_width_per_slice(sw, monkeypatch, capfd):
    """a class launch takes its cell width from its own slice's pairs: h0 above 255 - qcap * a occurs in class 2 (qcap 48) of
    slice 1 only, so that class runs the byte kernel in slice 0 and the 16-bit kernel in slice 1"""
    n = 9001
    b = gabgen.bsw(4302, n, 1)
    cls = (b.len2 - 1) // 16
    rng = np.random.default_rng(5)
    h0 = rng.integers(0, 100, n)
    big = np.flatnonzero((cls == 2) & (np.arange(n) >= SLICE0))[::3]
    h0[big] = rng.integers(255 - 48 + 1, 400, len(big))
    assert len(big) > 0 and (cls[:SLICE0] == 2).sum() > 64
    batch = subset(b, np.arange(n), h0=h0)
    want, mcells = reference(batch)
    ran, _ = check_sliced(sw, batch, want, mcells, monkeypatch, capfd)
    bits = {(sl, c): w for sl, c, _, w in ran}
    assert bits[(0, 2)] == 8 and bits[(1, 2)] == 16, ran
    assert bits[(0, 0)] == bits[(1, 0)] == 8 and bits[(0, 15)] == bits[(1, 15)] == 16, ran


# ------------------------------------------------------------------------------------------------ order, streams, repeats
def test_shuffled_batch_keeps_input_order(base, sw, monkeypatch, capfd):
    """rec.id is the pair's index in the whole batch, not in its slice"""
    b, want, mcells = base
    perm = np.random.default_rng(11).permutation(N_BASE)[:10003]
    check_sliced(sw, subset(b, perm), want[perm], mcells[perm], monkeypatch, capfd)


def test_other_stream_and_second_handle(base, sw, monkeypatch, capfd):
    """a call on a non-default torch stream, and a second handle used after the first"""
    import torch
    from genarchbench_amd.bsw import BandedPairWiseSW
    b, want, mcells = base
    n = 9001
    batch = subset(b, np.arange(n))
    ran, cells = check_sliced(sw, batch, want[:n], mcells[:n], monkeypatch, capfd, stream=torch.cuda.Stream())
    other = BandedPairWiseSW()
    try:
        ran2, cells2 = check_sliced(other, batch, want[:n], mcells[:n], monkeypatch, capfd)
        assert ran2 == ran and cells2 == cells
        got, cells3, _ = call(sw, Dev(batch), (SLICE0, SLICE_MIN), monkeypatch, capfd)      # ... and the first one again
        np.testing.assert_array_equal(got, want[:n, 0])
        assert cells3 == cells
    finally:
        other.close()


def test_two_sliced_calls_in_a_row(base, sw, monkeypatch, capfd):
    """nothing of a slice's state (counters, class boundaries, widths) survives into the next call"""
    b, want, mcells = base
    d1, d2 = Dev(subset(b, np.arange(9001))), Dev(subset(b, np.arange(1500, N_BASE)))
    out = [call(sw, d, (SLICE0, SLICE_MIN), monkeypatch, capfd) for d in (d1, d2, d1, d1)]
    np.testing.assert_array_equal(out[0][0], want[:9001, 0])
    np.testing.assert_array_equal(out[1][0], want[1500:, 0])
    assert out[0][1] == int(mcells[:9001].sum()) and out[1][1] == int(mcells[1500:].sum())
    for k in (2, 3):
        np.testing.assert_array_equal(out[k][0], out[0][0])
        assert out[k][1:] == out[0][1:]


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_pair_in_slice_0(base, sw, monkeypatch, capfd):
    """refused before any DP kernel runs, as an unsliced call is"""
    from genarchbench_amd._lib import GabError
    b, _, _ = base
    n, at = 9001, 4000
    len2 = b.len2[:n].copy(); len2[at] = 0; len2[SLICE0 + 50] = 0
    d = Dev(subset(b, np.arange(n), len2=len2))
    with pytest.raises(GabError, match=rf"first: pair {at}\)"):
        call(sw, d, (SLICE0, SLICE_MIN), monkeypatch, capfd)
    assert "[gab_bsw_dp" not in capfd.readouterr().err


def test_bad_pair_in_slice_1(base, sw, monkeypatch, capfd):
    """found while slice 0's DP runs: none of slice 1's DP is launched, the call returns with nothing in flight, and the handle
    is good for the next batch"""
    import torch
    from genarchbench_amd._lib import GabError
    b, want, mcells = base
    n, at = 9001, SLICE0 + 1234
    len2 = b.len2[:n].copy(); len2[at] = 0; len2[at + 700] = 0
    d = Dev(subset(b, np.arange(n), len2=len2))
    with pytest.raises(GabError, match=rf"first: pair {at}\)"):
        call(sw, d, (SLICE0, SLICE_MIN), monkeypatch, capfd)
    torch.cuda.synchronize()
    ran = launches(capfd.readouterr().err)
    assert ran and {sl for sl, *_ in ran} == {0} and sum(k for _, _, k, _ in ran) == SLICE0, ran
    check_sliced(sw, subset(b, np.arange(n)), want[:n], mcells[:n], monkeypatch, capfd)
