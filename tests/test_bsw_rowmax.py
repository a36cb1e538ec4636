"""CPU: the 8-bit bsw kernel's row maximum -- one key per group of four columns, the column resolved after the row -- as
tools/gen/bsw_rowmax_model.c restates it, against the oracle.

The kernel (bsw_dp8 in bsw.hip) no longer keeps a key per cell: a loop trip folds (largest H of its four columns << 16) | first
column into the row's running maximum, the cells outside the loop keep exact keys, and after the row the column is the last one of
[kj, min(kj + 3, end - 1)] that holds the maximum.  The model is the oracle's row loop with exactly that, so all six result fields
must equal the oracle's on every input; tests/test_bsw_rowmax_gpu.py runs the kernels on the tie-heavy batch used here.  The
negative control -- the same model without the resolve step -- must get a pair of that batch wrong at every parameter set the GPU
test uses: a batch on which it did not would not test the rule."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.bsw_rowmax_cases import GPU_PARAM_SETS, gpu_batch, tie_heavy_batch
from tests.util import BSW_PARAM_SETS, bsw_oracle_params

N = 200000


@pytest.fixture(scope="module")
def batches():
    """200 k read-like pairs (mode 0), 200 k adversarial ones (mode 1), and the tie-heavy batch"""
    return {"bench": gabgen.bsw(2, N, 0), "adv": gabgen.bsw(3, N, 1), "ties": tie_heavy_batch()}


def check(batch, ps, name):
    p = bsw_oracle_params(*ps)
    want = pyoracle.bsw(batch, p)
    got, _ = gabgen.bsw_rowmax_model(batch, p)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (f"{name}: {len(bad)} of {batch.n} pairs differ; first: pair {bad[0]} qlen {batch.len2[bad[0]]} tlen "
                           f"{batch.len1[bad[0]]} h0 {batch.h0[bad[0]]}: model {got[bad[0]].tolist()} oracle {want[bad[0]].tolist()}")


@pytest.mark.parametrize("ps", BSW_PARAM_SETS, ids=["_".join(map(str, p)) for p in BSW_PARAM_SETS])
def test_six_fields_at_every_parameter_set(batches, ps):
    for name, b in batches.items():
        check(b, ps, name)


@pytest.mark.parametrize("ps", [p for _, p in GPU_PARAM_SETS], ids=["_".join(map(str, p)) for _, p in GPU_PARAM_SETS])
def test_six_fields_at_the_gpu_parameter_sets(ps):
    check(tie_heavy_batch(), ps, "ties")


@pytest.mark.parametrize("ps", [p for _, p in GPU_PARAM_SETS], ids=["_".join(map(str, p)) for _, p in GPU_PARAM_SETS])
def test_the_batch_holds_every_kind_of_tie(ps):
    """a row maximum held by two columns of one group, by columns of neighbouring groups, by the head cell, by a column of the
    remainder pair and by the tail cell, each together with another column -- at every parameter set of the GPU test, on the
    pairs that set runs there"""
    b = gpu_batch(ps)
    assert b.n <= 4096
    _, ties = gabgen.bsw_rowmax_model(b, bsw_oracle_params(*ps))
    count = {bit: int(((ties & bit) != 0).sum()) for bit in (1, 2, 4, 8, 16)}
    print("pairs with a tied row maximum, by kind (1 group, 2 neighbouring groups, 4 head, 8 remainder pair, 16 tail):", count)
    assert all(count.values()), count


@pytest.mark.parametrize("ps", [p for _, p in GPU_PARAM_SETS], ids=["_".join(map(str, p)) for _, p in GPU_PARAM_SETS])
def test_without_the_resolve_step_the_batch_tells(ps):
    """negative control: column = the winning group's FIRST column must get at least one pair of the tie-heavy batch wrong"""
    b = gpu_batch(ps)
    p = bsw_oracle_params(*ps)
    want = pyoracle.bsw(b, p)
    got, _ = gabgen.bsw_rowmax_model(b, p, resolve=False)
    wrong = int((got != want).any(axis=1).sum())
    print(f"{wrong} of {b.n} pairs differ without the resolve step; fields that differ: {np.flatnonzero((got != want).any(axis=0)).tolist()}")
    assert wrong >= 1
