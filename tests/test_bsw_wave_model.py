"""CPU: the row trace of the bsw exit / prune model (tools/gen/bsw_exit_model.c, gab_bsw_exit_trace), which
tools/profiling/bsw_wave_model.py groups into waves.

The trace entry runs the same model_one as gab_bsw_exit_model: score, rows, cells, bound-pass cells and restarts must be equal pair by
pair, and the widths end - beg of a pair's traced rows -- an abandoned pass included -- must sum to its cell count exactly."""
import numpy as np
import pytest

from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params
from tests.test_bsw_left_prune import handmade, with_zdrop
from tests.test_bsw_right_prune import ZERO_ROWS, handmade_right

DEFAULTS = BSW_PARAM_SETS[0]
N = 20000


def batches():
    return {"read_like": gabgen.bsw(2, N, 0), "adversarial": gabgen.bsw(3, N, 1), "handmade": handmade(), "handmade_right": handmade_right()}


CASES = [(DEFAULTS, {}), (with_zdrop(DEFAULTS, 20), {}), (ZERO_ROWS, {}), (DEFAULTS, {"prune": False}), (DEFAULTS, {"early_exit": False}),
         (DEFAULTS, {"rule": "parent"})]


@pytest.fixture(scope="module")
def inputs():
    return batches()


@pytest.mark.parametrize("k", range(len(CASES)), ids=["defaults", "zdrop20", "zero_rows", "exit_only", "full_sweep", "parent_rule"])
def test_trace_equals_model_and_widths_sum_to_cells(inputs, k):
    ps, kw = CASES[k]
    p = bsw_oracle_params(*ps)
    restarts = 0
    for name, b in inputs.items():
        want = gabgen.bsw_exit_model(b, p, restarts=True, **kw)
        got = gabgen.bsw_exit_trace(b, p, **kw)
        for w, g, what in zip(want, got[:5], ("score", "rows", "cells", "pass_cells", "restarted")):
            np.testing.assert_array_equal(g, w, err_msg=f"{name}: {what}")
        off, beg, end, flags, drops = got[5:]
        assert len(beg) == len(end) == len(flags) == len(drops) == off[-1]
        F = gabgen.BSW_TRACE_FLAGS
        assert (((flags & F["left_drop"]) != 0) == ((drops & 15) != 0)).all() and (((flags & F["right_drop"]) != 0) == ((drops >> 4) != 0)).all()
        # a guard's bit closes an abandoned pass: as many as pairs that restarted
        assert ((flags & (F["zdrop_guard"] | F["right_edge_guard"] | F["zero_row_guard"])) != 0).sum() == want[4].sum()
        assert (beg >= 0).all() and (end <= np.repeat(b.len2, np.diff(off))).all()
        width = np.maximum(end.astype(np.int64) - beg, 0)
        per_pair = np.add.reduceat(np.append(width, 0), off[:-1]) * (np.diff(off) > 0)
        np.testing.assert_array_equal(per_pair, want[2], err_msg=f"{name}: traced widths against the cell count")
        # the final pass's rows close the trace; a restarted pair has an abandoned pass in front of them
        nrows = np.diff(off)
        assert (nrows >= want[1]).all() and ((nrows > want[1]) == (want[4] != 0)).all(), name
        restarts += int(want[4].sum())
        if not kw.get("early_exit", True) or not kw.get("prune", True):
            assert not (flags & (gabgen.BSW_TRACE_FLAGS["left_drop"] | gabgen.BSW_TRACE_FLAGS["right_drop"])).any()
    if k == 1:
        assert restarts > 0          # the two-pass trace is exercised


def test_the_flags_fire_on_read_like_input(inputs):
    """every per-row path the wave model prices occurs in the read-like batch at the defaults"""
    flags = gabgen.bsw_exit_trace(inputs["read_like"], bsw_oracle_params(*DEFAULTS))[8]
    for name, bit in gabgen.BSW_TRACE_FLAGS.items():
        if not name.endswith("guard"):
            assert (flags & bit).any(), name
