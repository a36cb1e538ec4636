"""CPU: the plan of the wfa cascade (genarchbench_amd/csrc/wfa_plan.h: wfa_table, wfa_plan) against the model of tests/util.py.

genarchbench_amd/wfa_plan_dump (built with the library; its source includes only wfa_plan.h) prints the score table of a penalty set
and, for a grid of longest pattern / text lengths, the launches up to the first wfa_global as `kernel pool dir` -- spelled as in the
GAB_WFA_TRACE lines -- and the host's intermediate values.  Everything is compared for equality with tests.util.wfa_rows and
tests.util.wfa_plan: both modes, every penalty set of WFA_PENALTIES, the knob values tests/test_wfa_tiers_gpu.py uses, and lengths on
both sides of every switch of the plan (187 | 188 the byte tier, 227 | 228 the static rows, 226 .. 229 the static pool)."""
import os
import subprocess
import types

import numpy as np
import pytest

import genarchbench_amd
from tests import util
from tests.util import WFA_PENALTIES

DUMP = os.path.join(os.path.dirname(os.path.abspath(genarchbench_amd.__file__)), "wfa_plan_dump")
LENGTHS = (0, 1, 150, 151, 180, 187, 188, 226, 227, 228, 229, 300, 600, 1000, 2039, 2040)
KNOBS = ({}, {"GAB_WFA_NO_STATIC": 1}, {"GAB_WFA_POOL2": 1024}, {"GAB_WFA_POOL2": 4080}, {"GAB_WFA_SLOTS": 0}, {"GAB_WFA_SLOTS": 3},
         {"GAB_WFA_SLOTS": 1002})
N_LDS = 1000                   # pairs per batch: GAB_WFA_SLOTS = 1002 is cut to it, 0 and 3 are not


def dump(adaptive, pen, n_lds, knobs, lengths=LENGTHS):
    """-> (rows as wfa_rows lists them, {(max_plen, max_tlen): (launches, values)}) as the program prints them"""
    assert os.path.exists(DUMP), f"{DUMP} is missing: build() makes it"
    args = [DUMP, str(int(adaptive))] + [str(v) for v in pen] + [str(n_lds), str(int(bool(knobs.get("GAB_WFA_NO_STATIC")))),
                                                                  str(knobs.get("GAB_WFA_POOL2", -1)), str(knobs.get("GAB_WFA_SLOTS", -1))]
    text = subprocess.run(args + [str(v) for v in lengths], check=True, capture_output=True, text=True).stdout
    rows, plans, cur = [], {}, None
    for line in text.splitlines():
        f = line.split()
        if f[0] == "row":
            sc, lo, hi, gap, used = (int(v) for v in f[1:])
            rows.append((sc, lo, hi, bool(gap), used))
        elif f[0] == "plan":
            cur = plans[int(f[1]), int(f[2])] = [[], None]
        elif f[0] == "vals":
            cur[1] = dict(zip(("seqp", "seqt", "static_rows", "static_pool", "use_static", "byte_ok", "slots"), (int(v) for v in f[1:])))
        else:
            cur[0].append((f[0], int(f[1]), int(f[2])))
    return rows, plans


def batch_of(max_plen, max_tlen, n):
    """what wfa_plan reads of a batch: n pairs, the longest pattern and the longest text in different pairs"""
    pl, tl = np.zeros(n, np.int32), np.zeros(n, np.int32)
    if n:
        pl[0] = max_plen; tl[-1] = max_tlen
    return types.SimpleNamespace(pat_len=pl, txt_len=tl, n=n)


@pytest.fixture(scope="module")
def cached_rows():
    """tests.util.wfa_plan asks wfa_rows for the same table at every grid point: keep each (the function is pure)"""
    mp = pytest.MonkeyPatch()
    real, memo = util.wfa_rows, {}

    def rows(pen, *a, **kw):
        key = (tuple(pen), a, tuple(sorted(kw.items())))
        if key not in memo:
            memo[key] = real(pen, *a, **kw)
        return memo[key]
    mp.setattr(util, "wfa_rows", rows)
    yield real
    mp.undo()


@pytest.mark.parametrize("pen", WFA_PENALTIES)
def test_rows(pen, cached_rows):
    """the row table (score, lo, hi, has I / D, used_end) of every penalty set"""
    rows, _ = dump(False, pen, N_LDS, {}, lengths=(151,))
    assert rows == cached_rows(pen)


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("pen", WFA_PENALTIES)
def test_plan(pen, adaptive, cached_rows):
    """launches and intermediate values on the whole grid of lengths, for every knob set"""
    for knobs in KNOBS:
        _, plans = dump(adaptive, pen, N_LDS, knobs)
        assert len(plans) == len(LENGTHS) ** 2
        for (mp, mt), (launches, vals) in plans.items():
            want = util.wfa_plan(batch_of(mp, mt, N_LDS), pen, adaptive, knobs)
            where = (pen, adaptive, knobs, mp, mt)
            assert launches == want["launches"], where
            assert vals == {k: int(want[k]) for k in vals}, where


@pytest.mark.parametrize("n_lds", [0, 1, 5, 70001, 600007])
def test_plan_batch_sizes(n_lds, cached_rows):
    """the resume slots by batch size (all pairs, 65 536, an eighth; a multiple of 8) and the empty batch's empty plan"""
    for adaptive in (False, True):
        _, plans = dump(adaptive, (4, 6, 2), n_lds, {}, lengths=(151, 228))
        for (mp, mt), (launches, vals) in plans.items():
            want = util.wfa_plan(batch_of(mp, mt, n_lds), (4, 6, 2), adaptive, {})
            if n_lds == 0:                  # (the model takes the lengths from the pairs: none)
                assert launches == want["launches"] == [] and vals["slots"] == 0
                continue
            assert launches == want["launches"], (adaptive, mp, mt)
            assert vals == {k: int(want[k]) for k in vals}, (adaptive, mp, mt)
