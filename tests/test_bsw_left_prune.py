"""CPU: the left-edge prune of the score-only bsw kernels, as tools/gen/bsw_exit_model.c restates it, against the oracle.

After a row, a score-only call moves the band's left edge over cells that can no longer reach `best` (bsw.hip's header comment has
the rule and its proof); a pair that has dropped a live cell and meets a row in which a z-drop could fire starts again without the
prune.  tests/test_bsw_early_exit.py already checks the model's scores (prune on, the default) against the oracle at every parameter
set; this file checks that the prune really fires, that the fallback really runs, that the score check has teeth (a wrong
potential changes scores), that the prune is tied to the exit, and hand-made pairs aimed at the boundary term, the z-drop
guard and the restriction to pairs whose row -1 leaves nothing live behind the band clamp."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params

DEFAULTS = BSW_PARAM_SETS[0]
N = 100000


@pytest.fixture(scope="module")
def bench():
    return gabgen.bsw(2, N, 0)


@pytest.fixture(scope="module")
def adv():
    return gabgen.bsw(3, N, 1)


def with_zdrop(ps, zdrop, w=None):
    return ps[:7] + (zdrop,) + ps[8:9] + (ps[9] if w is None else w,)


def scores_match(batch, ps, **kw):
    p = bsw_oracle_params(*ps)
    want = pyoracle.bsw(batch, p)[:, 0]
    out = gabgen.bsw_exit_model(batch, p, **kw)
    bad = np.flatnonzero(out[0] != want)
    assert len(bad) == 0, (f"{len(bad)} of {batch.n} scores differ at {ps}; first: pair {bad[0]} qlen {batch.len2[bad[0]]} tlen "
                           f"{batch.len1[bad[0]]} h0 {batch.h0[bad[0]]}: model {out[0][bad[0]]} oracle {want[bad[0]]}")
    return out


def test_the_prune_fires_on_read_like_input(bench):
    """necessary condition, not a measurement: at most 0.85 of the exit-only model's cells on the mode-0 input at the defaults
    (the model evaluates 0.788 of them), the same rows, the same scores, and no pair restarts"""
    p = bsw_oracle_params(*DEFAULTS)
    s0, r0, c0, _ = gabgen.bsw_exit_model(bench, p, prune=False)
    s1, r1, c1, _, redo = scores_match(bench, DEFAULTS, restarts=True)
    print(f"cells with the prune {c1.sum() / c0.sum():.4f} of the exit-only model's, rows {r1.sum() / r0.sum():.4f}, restarted {redo.sum()}")
    np.testing.assert_array_equal(s0, s1)
    assert c1.sum() <= 0.85 * c0.sum()
    assert (c1 <= c0).all() and redo.sum() == 0
    np.testing.assert_array_equal(r0, r1)


def test_the_prune_needs_the_exit(bench, adv):
    """without the exit the prune argument changes nothing: the full sweep stays the oracle's (tests/test_bsw_early_exit.py checks
    that sweep against the oracle)"""
    p = bsw_oracle_params(*DEFAULTS)
    for b in (bench, adv):
        a = gabgen.bsw_exit_model(b, p, early_exit=False, prune=True)
        c = gabgen.bsw_exit_model(b, p, early_exit=False, prune=False)
        for x, y in zip(a, c):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("zdrop,w", [(100, 100), (20, 100), (10, 30), (5, 100)])
def test_the_fallback_runs_on_adversarial_input(adv, zdrop, w):
    """mode 1: pairs restart for the z-drop guard (at z-drop 20 it must happen), scores stay the oracle's, and a restarted pair's
    count holds its abandoned pass: more cells than the exit-only model's"""
    ps = with_zdrop(DEFAULTS, zdrop, w)
    p = bsw_oracle_params(*ps)
    _, _, c1, _, redo = scores_match(adv, ps, restarts=True)
    _, _, c0, _ = gabgen.bsw_exit_model(adv, p, prune=False)
    print(f"z-drop {zdrop} w {w}: restarted {redo.sum()} of {adv.n}, cells {c1.sum() / c0.sum():.4f} of the exit-only model's")
    if zdrop == 20:
        assert redo.sum() > 0
    assert (c1[redo == 1] > c0[redo == 1]).all()
    assert (c1[redo == 0] <= c0[redo == 0]).all()


@pytest.mark.parametrize("ps", [with_zdrop(DEFAULTS, 30), with_zdrop(DEFAULTS, 100, 20), BSW_PARAM_SETS[1], BSW_PARAM_SETS[5],
                                (1, 1, -1, 1, 1, 1, 1, 100, 5, 100)], ids=["zdrop30", "w20", "2_3", "4_1", "all_ones"])
def test_scores_on_read_like_input_at_other_parameters(bench, ps):
    scores_match(bench, ps)


def test_a_wrong_potential_changes_scores(bench):
    """negative control: with the potential two columns short the prune drops cells that still reach `best`, and the score check
    that every other test relies on sees it"""
    p = bsw_oracle_params(*DEFAULTS)
    want = pyoracle.bsw(bench, p)[:, 0]
    score = gabgen.bsw_exit_model(bench, p, wrong_potential=True)[0]
    print(f"wrong potential: {(score != want).sum()} of {bench.n} scores differ")
    assert (score != want).sum() > bench.n // 10


# ------------------------------------------------------------------------------------------------ hand-made pairs
def rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def handmade():
    """pairs aimed at the rule's side conditions; each group also at small o_del / large h0 so that the left boundary stays live"""
    rng = np.random.default_rng(11)
    refs, qrys, h0s = [], [], []

    def add(r, q, h):
        refs.append(np.asarray(r, np.uint8)); qrys.append(np.asarray(q, np.uint8)); h0s.append(h)
    for k in range(400):
        L = int(rng.integers(8, 120))
        q = rnd(rng, L)
        # the query's start is missing from the reference's start and found after a deletion: only the left boundary (column 0,
        # rows 1..g) leads to the best score, so a prune that left column 0 too early would lose it
        g = int(rng.integers(1, 40))
        add(np.concatenate([rnd(rng, g), q, rnd(rng, int(rng.integers(0, 30)))]), q, int(rng.integers(20, 101)))
        # a good prefix, a long unrelated stretch, then a better second half: the score dips below best - zdrop for small zdrop
        a, b = rnd(rng, L), rnd(rng, L + 20)
        add(np.concatenate([a, rnd(rng, int(rng.integers(3, 25))), b]), np.concatenate([a, b])[:200], int(rng.integers(0, 60)))
        # reference shorter than the query (the rows left limit the potential) and tiny queries
        add(q[:max(1, L // 3)], q, int(rng.integers(0, 101)))
        add(rnd(rng, int(rng.integers(1, 30))), rnd(rng, int(rng.integers(1, 4))), int(rng.integers(0, 101)))
        # an insertion in the query right after the start: the best path runs left of the diagonal for a while
        add(np.concatenate([q[:5], q[5 + g % 7:], rnd(rng, 10)]), q, int(rng.integers(10, 101)))
    return gabgen.bsw_from_arrays(refs, qrys, h0s)


HAND_PARAMS = [DEFAULTS, with_zdrop(DEFAULTS, 10), with_zdrop(DEFAULTS, 8), with_zdrop(DEFAULTS, 100, 10),
               (1, 4, -1, 0, 1, 6, 1, 100, 5, 100),         # o_del = 0: the boundary decays by one per row
               (1, 4, -1, 0, 1, 0, 1, 9, 5, 100), (1, 4, -1, 1, 1, 6, 1, 100, 5, 8), (2, 3, -2, 1, 1, 5, 2, 16, 0, 100),
               with_zdrop(DEFAULTS, 7)]                     # under 8 x max_sc: the prune is off, the model is the exit alone


@pytest.mark.parametrize("ps", HAND_PARAMS, ids=["_".join(map(str, p)) for p in HAND_PARAMS])
def test_handmade_pairs(ps):
    b = handmade()
    out = scores_match(b, ps, restarts=True)
    p = bsw_oracle_params(*ps)
    c0 = gabgen.bsw_exit_model(b, p, prune=False)[2]
    print(f"{ps}: cells {out[2].sum() / c0.sum():.4f} of the exit-only model's, restarted {out[4].sum()} of {b.n}")
