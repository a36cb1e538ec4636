"""CPU: the score-only early exit of the bsw DP kernels, as tools/gen/bsw_exit_model.c restates it, against the oracle.

The kernels stop a pair's row loop once no later row can raise its score (bsw.hip's header comment has the bound and its proof).
The model is the oracle's scalar DP with that rule; tests/test_bsw_early_exit_gpu.py pins the kernels' cell counter to the model's
count, and this file checks the rule itself: the scores it returns are the oracle's for every parameter set the suite knows, and
it really fires -- on the read-like input at the driver's defaults it must save at least a fifth of the DP cells (a rule that
never fires would pass every score check)."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_handmade_pairs, bsw_oracle_params

DEFAULTS = BSW_PARAM_SETS[0]
N = 200000


@pytest.fixture(scope="module")
def batches():
    """200 k read-like pairs (mode 0), 200 k adversarial ones (mode 1), and the hand-made pairs"""
    return {"bench": gabgen.bsw(2, N, 0), "adv": gabgen.bsw(3, N, 1), "handmade": gabgen.bsw_from_arrays(*bsw_handmade_pairs())}


def check(batch, ps):
    """scores of the model with the exit == the oracle's; returns (oracle cells, model cells, rows without / with the exit)"""
    p = bsw_oracle_params(*ps)
    want, cells = pyoracle.bsw(batch, p, want_cells=True)
    score, rows, mcells, _ = gabgen.bsw_exit_model(batch, p)
    bad = np.flatnonzero(score != want[:, 0])
    assert len(bad) == 0, (f"{len(bad)} of {batch.n} scores differ; first: pair {bad[0]} qlen {batch.len2[bad[0]]} tlen "
                           f"{batch.len1[bad[0]]} h0 {batch.h0[bad[0]]}: model {score[bad[0]]} oracle {want[bad[0], 0]}")
    assert (rows <= batch.len1).all() and (rows >= 1).all()
    return cells, int(mcells.sum()), rows


@pytest.mark.parametrize("ps", BSW_PARAM_SETS, ids=["_".join(map(str, p)) for p in BSW_PARAM_SETS])
def test_scores_at_every_parameter_set(batches, ps):
    for name, b in batches.items():
        cells, mcells, _ = check(b, ps)
        assert mcells <= cells, name


@pytest.mark.parametrize("w", [5, 20, 100])
def test_scores_at_narrow_bands(batches, w):
    """w = 5 and 20: the band clamp cuts live cells in most rows, so the stale-cell term of the bound carries the proof"""
    for name, b in batches.items():
        cells, mcells, _ = check(b, DEFAULTS[:9] + (w,))
        assert mcells <= cells, name


def test_without_the_exit_the_model_is_the_oracle(batches):
    for ps in (DEFAULTS, BSW_PARAM_SETS[9]):
        p = bsw_oracle_params(*ps)
        for b in batches.values():
            want, cells = pyoracle.bsw(b, p, want_cells=True)
            score, rows, mcells, pass_cells = gabgen.bsw_exit_model(b, p, early_exit=False)
            np.testing.assert_array_equal(score, want[:, 0])
            assert int(mcells.sum()) == cells and int(pass_cells.sum()) == 0


def test_the_exit_fires_on_read_like_input(batches):
    """necessary condition, not a measurement: at most 0.80 of the oracle's cells on the mode-0 input at the defaults (the model
    evaluates 0.768 of them and 0.639 of the rows; the bound passes read 0.009 of the cell count)"""
    b = batches["bench"]
    p = bsw_oracle_params(*DEFAULTS)
    _, cells = pyoracle.bsw(b, p, want_cells=True)
    _, rows, mcells, pass_cells = gabgen.bsw_exit_model(b, p)
    print(f"cells {mcells.sum() / cells:.4f} rows {rows.sum() / gabgen.bsw_exit_model(b, p, early_exit=False)[1].sum():.4f} "
          f"pass cells {pass_cells.sum() / cells:.4f}")
    assert mcells.sum() <= 0.80 * cells
    assert pass_cells.sum() <= 0.05 * cells          # the pass is rare: about one row per pair
