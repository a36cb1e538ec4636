"""GPU: the seeded prune of the score-only bsw kernels -- the lower bound L that bsw_seed computes per pair, the threshold
max(best, L - 1) of both prunes and their guards, the prune of row -1 and the sort key made of the deficit (bsw.hip's header).

Every case goes through tests/test_bsw_early_exit_gpu.py's check(..., full=True): the score-only AND the six-field call on one
handle, scores and all six fields equal to pyoracle.bsw with no tolerance, last_stats()["cells"] of the score-only call equal to
the cell sum of tools/gen/bsw_exit_model.c (default rule, abandoned passes included) EXACTLY, that of the six-field call equal to
the full sweep's (the six-field form is untouched), and the GAB_BSW_TRACE lines naming the kernel that ran.  The hand-made pairs are
those of tests/test_bsw_seeded_prune.py; that a case really exercises the seed (fewer cells than the rule before it) is asserted on
the CPU from the model."""
import numpy as np
import pytest

from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params
from tests.test_bsw_early_exit_gpu import check, generator_batch, byte_h0, lifted_h0
from tests.test_bsw_seeded_prune import handmade
from tests.test_bsw_slices_gpu import check_sliced, reference, sw      # noqa: F401  (sw is a fixture)

pytestmark = pytest.mark.gpu

DEFAULTS = BSW_PARAM_SETS[0]
# (kernel, parameters, longest query, h0 of the generated pairs, h0 cap / lift of the hand-made pairs): every set has the prunes on
# (z-drop 0 or >= 8 * max_sc); the row -1 prune is on where max_sc <= e_ins -- off in the second dp8<0,0> case
CASES = [
    ("dp8<1,1>", DEFAULTS, 151, byte_h0(255 - 160), 130),
    ("dp8<1,0>", (2, 3, -2, 5, 2, 5, 2, 50, 30, 30), 112, byte_h0(255 - 224), 31),
    ("dp8<0,1>", (1, 4, -1, 6, 1, 7, 1, 100, 5, 100), 151, byte_h0(255 - 160), 130),
    ("dp8<0,0>", (2, 4, 2, 9, 1, 3, 2, 100, 5, 40), 48, byte_h0(255 - 96), 255 - 96),
    ("dp8<0,0>", (3, 5, -1, 7, 3, 4, 1, 200, 5, 100), 48, byte_h0(255 - 144), 255 - 144),
    ("dp16", DEFAULTS, 256, lifted_h0(100, 97, 1000), 1000),
    ("dp32", DEFAULTS, 256, lifted_h0(100, 5, 40000), 40000),
]
IDS = ["dp8_11", "dp8_10", "dp8_01", "dp8_00_row", "dp8_00_norow", "dp16", "dp32"]


def hand_batch(qmax, h0_arg, lifted):
    """the hand-made pairs, queries cut to qmax; h0 capped at h0_arg, or -- lifted -- every fifth pair's raised by it"""
    b, _ = handmade()
    h0 = b.h0.copy()
    if lifted:
        h0[::5] += h0_arg
    else:
        h0 = np.minimum(h0, h0_arg)
    return gabgen.BswBatch(b.ref, b.ref_off, b.qry, b.qry_off, b.len1, np.minimum(b.len2, qmax).astype(np.int32), h0.astype(np.int32))


def seed_share(batch, ps):
    p = bsw_oracle_params(*ps)
    return gabgen.bsw_exit_model(batch, p)[2].sum() / gabgen.bsw_exit_model(batch, p, rule="capped")[2].sum()


@pytest.mark.parametrize("want_kernel,ps,qmax,h0_of,h0_arg", CASES, ids=IDS)
def test_handmade_pairs_in_every_kernel(monkeypatch, capfd, want_kernel, ps, qmax, h0_of, h0_arg):
    batch = hand_batch(qmax, h0_arg, lifted=not want_kernel.startswith("dp8"))
    check(ps, batch, monkeypatch, capfd, want_kernel, full=True)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("want_kernel,ps,qmax,h0_of,h0_arg", CASES, ids=IDS)
def test_generated_pairs_in_every_kernel(monkeypatch, capfd, want_kernel, ps, qmax, h0_of, h0_arg, mode):
    batch = generator_batch(500 + mode, mode, qmax, h0_of, n=8192)
    share = seed_share(batch, ps)
    print(f"{want_kernel} mode {mode}: the model evaluates {share:.4f} of the cells of the rule before the seed")
    assert share <= 1.0
    if mode == 0:
        assert share < 0.99                     # the seed really fires in this kernel
    check(ps, batch, monkeypatch, capfd, want_kernel, full=True)


def test_pruned_lanes_and_unpruned_lanes_side_by_side(monkeypatch, capfd):
    """w = 40 and 60-base queries: restriction (a) holds for h0 <= 48 only, so neighbouring pairs differ in whether L is used"""
    ps = DEFAULTS[:9] + (40,)
    b = generator_batch(510, 0, 151, None, n=4096)
    batch = gabgen.BswBatch(b.ref, b.ref_off, b.qry, b.qry_off, b.len1, np.minimum(b.len2, 60).astype(np.int32),
                            np.where(np.arange(b.n) % 2 == 0, 40, 60).astype(np.int32))
    assert (batch.len2 > 41).sum() > 1000
    assert seed_share(batch, ps) < 0.99
    check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_guards_restart_pairs_under_the_seed(monkeypatch, capfd):
    """z-drop 20 on the adversarial input: pairs abandon their seeded pass for the z-drop guard and run again"""
    ps = DEFAULTS[:7] + (20,) + DEFAULTS[8:]
    batch = generator_batch(511, 1, 151, byte_h0(95), n=8192)
    redo = gabgen.bsw_exit_model(batch, bsw_oracle_params(*ps), restarts=True)[4]
    assert redo.sum() > 50
    check(ps, batch, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_sliced_call(sw, monkeypatch, capfd):      # noqa: F811
    """GAB_BSW_SLICE lowered: bsw_seed, the histogram and the scatter of slice 1 run beside slice 0's DP, each slice with its own L"""
    g = gabgen.bsw(512, 9001 - handmade()[0].n, 0)
    h = hand_batch(151, 95, lifted=False)
    refs = [h.pair(i)[0] for i in range(h.n)] + [g.pair(i)[0] for i in range(g.n)]
    qrys = [h.pair(i)[1] for i in range(h.n)] + [g.pair(i)[1] for i in range(g.n)]
    batch = gabgen.bsw_from_arrays(refs, qrys, list(h.h0) + list(g.h0))
    perm = np.random.default_rng(5).permutation(batch.n)          # hand-made pairs in both slices
    batch = gabgen.BswBatch(batch.ref, batch.ref_off[perm].copy(), batch.qry, batch.qry_off[perm].copy(), batch.len1[perm].copy(),
                            batch.len2[perm].copy(), batch.h0[perm].copy())
    want, mcells = reference(batch)
    check_sliced(sw, batch, want, mcells, monkeypatch, capfd)
