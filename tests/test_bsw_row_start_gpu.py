"""GPU: the row tail of the score-only 8-bit bsw kernel (bsw.hip, bsw_dp8<SYM, MS1, true>; profiles/bsw_row_start.md) -- flags
and small updates (best and its row and column, the z-drop test and its guard, the right-edge guard, the band clamp, the left-edge
potential, go / bestL) as selects, and the one-cell moves of the two four-cell windows as shift counts.  The cases put every
parity of both band edges, every advance of the left edge, narrow bands, clamped bands and restarted pairs through that code.

Every case: scores equal to pyoracle.bsw with no tolerance, last_stats()["cells"] of the score-only call equal to the cell sum of
tools/gen/bsw_exit_model.c (abandoned passes included), and every DP launch a dp8 instantiation.  The batches are those of
tests/test_bsw_row_start.py, which asserts on the CPU, from the model's row trace, that they hold the rows this code can get
wrong.  Both launch forms run: a small batch is one launch of its longest class; under GAB_BSW_SLICE it is two slices of
per-class launches."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params
from tests.test_bsw_early_exit_gpu import check, run
from tests.test_bsw_row_start import BYTE_SETS, DEFAULTS, HAND_W, N_GEN, byte_batch, handmade, with_w
from tests.test_bsw_slices_gpu import Dev, call

pytestmark = pytest.mark.gpu


def check_byte(ps, batch, monkeypatch, capfd):
    """scores == oracle, score-only cells == model, byte kernels only"""
    p = bsw_oracle_params(*ps)
    want = pyoracle.bsw(batch, p)
    mscore, _, mcells, _ = gabgen.bsw_exit_model(batch, p)
    np.testing.assert_array_equal(mscore, want[:, 0])
    got, cells, kernels = run(ps, batch, monkeypatch, capfd)
    bad = np.flatnonzero(got != want[:, 0])
    assert len(bad) == 0, (f"{len(bad)} of {batch.n} scores differ ({kernels}); first: pair {bad[0]} qlen {batch.len2[bad[0]]} tlen "
                           f"{batch.len1[bad[0]]} h0 {batch.h0[bad[0]]}: got {got[bad[0]]} want {want[bad[0], 0]}")
    print(f"{kernels} cells: model {int(mcells.sum())} gpu {cells}")
    assert cells == int(mcells.sum()), (cells, int(mcells.sum()), kernels)
    assert kernels and all(k.startswith("dp8<") for k in kernels), kernels


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", BYTE_SETS)
def test_generator_pairs_under_every_byte_parameter_set(monkeypatch, capfd, k, mode):
    ps = BSW_PARAM_SETS[k]
    check_byte(ps, byte_batch(ps, 5000 + k, mode), monkeypatch, capfd)


@pytest.mark.parametrize("w", HAND_W)
def test_handmade_pairs_of_query_length_4_to_12(monkeypatch, capfd, w):
    """bands of at most 12 cells: the right prune's zeroed cells lie inside the words the next row starts with; w <= 3 puts the
    left edge on the band clamp.  The six-field call runs on the same handle (check(..., full=True))."""
    check(with_w(DEFAULTS, w), handmade(), monkeypatch, capfd, "dp8<1,1>", full=True)


@pytest.mark.parametrize("mode", [0, 1])
def test_per_class_launches(monkeypatch, capfd, mode):
    """the defaults' batch again, sliced: every query-length class of either slice is a launch of its own"""
    from genarchbench_amd.bsw import BandedPairWiseSW
    batch = byte_batch(DEFAULTS, 5000, mode)
    p = bsw_oracle_params(*DEFAULTS)
    want = pyoracle.bsw(batch, p)[:, 0]
    mcells = int(gabgen.bsw_exit_model(batch, p)[2].sum())
    monkeypatch.setenv("GAB_BSW_TRACE", "1")
    sw = BandedPairWiseSW()
    try:
        d = Dev(batch)
        got, cells, ran = call(sw, d, (1501, 3000), monkeypatch, capfd)
        one, one_cells, one_ran = call(sw, d, None, monkeypatch, capfd)
    finally:
        sw.close()
    print(f"launches: sliced {ran}, unsliced {one_ran}")
    assert {sl for sl, *_ in ran} == {0, 1} and len(ran) > 4 and all(bits == 8 for *_, bits in ran), ran
    assert sum(n for _, _, n, _ in ran) == N_GEN and len(one_ran) == 1
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(one, want)
    assert cells == mcells and one_cells == mcells
