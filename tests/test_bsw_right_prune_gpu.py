"""GPU: the right-edge prune and the four-cell cap of the six bsw DP kernels against the oracle and the CPU model of the rule.

A score-only call zeroes the stored cells at the band's right edge that can no longer reach `best` and pulls `end` in behind
them; either edge moves over at most four cells per row (bsw.hip's header comment; tests/test_bsw_right_prune.py checks the rule
itself on the CPU).  Kernels are selected as in tests/test_bsw_left_prune_gpu.py -- GAB_BSW_TRACE, the h0 range and the
parameters -- and every case goes through the helpers of tests/test_bsw_early_exit_gpu.py: scores against the oracle with no
tolerance, the score-only cell counter equal to the sum of tools/gen/bsw_exit_model.c (abandoned passes included)."""
import numpy as np
import pytest

from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params
from tests.test_bsw_early_exit_gpu import byte_h0, check, generator_batch
from tests.test_bsw_left_prune_gpu import KERNEL_CASES, with_zdrop
from tests.test_bsw_left_prune import handmade
from tests.test_bsw_right_prune import ZERO_ROWS, handmade_right

pytestmark = pytest.mark.gpu

DEFAULTS = BSW_PARAM_SETS[0]
N = 8192


def short_query_batch(seed, qlo, qhi, h0_of):
    """N read-like pairs: the generator's reference windows and the first qlo .. qhi bases of its queries"""
    b = gabgen.bsw(seed, N, 0)
    rng = np.random.default_rng(seed)
    len2 = np.minimum(b.len2, rng.integers(qlo, qhi + 1, N)).astype(np.int32)
    len2[:2] = (qlo, qhi)
    assert len2.max() == qhi and b.len2[1] >= qhi
    return gabgen.BswBatch(b.ref, b.ref_off, b.qry, b.qry_off, b.len1, len2, np.asarray(h0_of(rng, N), np.int32))


# one batch inside the 16-column class, one across the classes' boundaries at 16, 32 (and 48) columns; at most 64 columns, and 48 for
# dp8<0,0>, whose max_sc = 4 leaves the byte kernel no more
@pytest.mark.parametrize("qlo,qhi", [(3, 16), (9, 64)], ids=["class16", "across"])
@pytest.mark.parametrize("want_kernel,ps,qmax,h0_of", KERNEL_CASES, ids=[k for k, *_ in KERNEL_CASES])
def test_every_kernel_on_short_read_like_pairs(monkeypatch, capfd, want_kernel, ps, qmax, h0_of, qlo, qhi):
    qhi = min(qhi, qmax, 64)
    batch = short_query_batch(500 + qhi, qlo, qhi, h0_of)
    _, _, cells = check(ps, batch, monkeypatch, capfd, want_kernel, full=(qhi > 16))
    parent = int(gabgen.bsw_exit_model(batch, bsw_oracle_params(*ps), rule="parent")[2].sum())
    print(f"{want_kernel} q {qlo}..{qhi}: {cells / parent:.4f} of the cells of the rule without the right prune")
    assert cells < parent


def test_handmade_right_edges(monkeypatch, capfd):
    """odd and even `end`, end == qlen, a band that shrinks to a cell or two and grows again over zeroed cells, a best path right of
    the diagonal: through bsw_dp8 and, with some h0 lifted, through bsw_dp<false>"""
    b = handmade_right()
    batch = gabgen.BswBatch(b.ref, b.ref_off, b.qry, b.qry_off, b.len1, b.len2, np.minimum(b.h0, 95).astype(np.int32))
    for ps in (DEFAULTS, with_zdrop(DEFAULTS, 10)):
        check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)
    batch.h0[::7] = 1000
    check(DEFAULTS, batch, monkeypatch, capfd, "dp16")


def test_pairs_that_restart(monkeypatch, capfd):
    """the adversarial pairs, z-drop and band of tests/test_bsw_left_prune_gpu.py's restart test: pairs abandon the pruned pass, and
    the counter holds both passes"""
    ps = with_zdrop(DEFAULTS, 20, 100)
    batch = generator_batch(410, 1, 151, byte_h0(255 - 160), n=16384)
    redo = gabgen.bsw_exit_model(batch, bsw_oracle_params(*ps), restarts=True)[4]
    print(f"{redo.sum()} of {batch.n} pairs restart")
    assert redo.sum() > 0
    check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_the_zero_row_guard(monkeypatch, capfd):
    """mismatch score -128 on the left-edge pairs of tests/test_bsw_left_prune.py: rows of zeros next to a live left edge, the
    third reason to abandon a pruned pass (tests/test_bsw_right_prune.py checks on the CPU that it fires here)"""
    b = handmade()
    batch = gabgen.BswBatch(b.ref, b.ref_off, b.qry, b.qry_off, b.len1, b.len2, np.minimum(b.h0, 45).astype(np.int32))
    redo = gabgen.bsw_exit_model(batch, bsw_oracle_params(*ZERO_ROWS), restarts=True)[4]
    assert redo.sum() > 0
    check(ZERO_ROWS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)
    batch.h0[::7] = 1000
    check(ZERO_ROWS, batch, monkeypatch, capfd, "dp16")
