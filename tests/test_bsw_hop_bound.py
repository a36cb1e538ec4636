"""CPU: the hop bound of the seeded prune -- the lower bound L of a pair's score that follows the alignment over at most three
one-gap hops behind the ungapped extension (tools/gen/bsw_exit_model.c, hop_bound; bsw.hip's header has the rule and the proof).

Against the oracle at every parameter set and both generator modes: h0 <= L_ungapped <= L_hop <= score, the model's scores, no
more cells than the rule before the seed.  The negative control (a hop from the h0 corner) is wrong where the rule is not.  Hand-made
pairs with L_hop written out (tests/bsw_hop_cases.py), and necessary conditions on the read-like input."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests import bsw_hop_cases as H
from tests.util import BSW_PARAM_SETS, bsw_oracle_params

DEFAULTS = BSW_PARAM_SETS[0]
N = 20000


@pytest.fixture(scope="module")
def batches():
    return {0: gabgen.bsw(2, N, 0), 1: gabgen.bsw(3, N, 1)}


@pytest.mark.parametrize("k", range(len(BSW_PARAM_SETS)), ids=["_".join(map(str, p)) for p in BSW_PARAM_SETS])
def test_bounds_scores_and_economy_at_every_parameter_set(batches, k):
    ps = BSW_PARAM_SETS[k]
    p = bsw_oracle_params(*ps)
    for mode, b in batches.items():
        want = pyoracle.bsw(b, p)[:, 0]
        L0, L = gabgen.bsw_seed_bound(b, p), gabgen.bsw_hop_bound(b, p)
        out = gabgen.bsw_exit_model(b, p, restarts=True)
        capped = gabgen.bsw_exit_model(b, p, rule="capped")
        print(f"set {k} mode {mode}: L_hop > L_ungapped in {(L > L0).sum()} pairs, L_hop == score in {(L == want).sum()}, cells "
              f"{out[2].sum() / capped[2].sum():.4f} of the rule's before the seed, restarted {out[4].sum()}")
        assert (b.h0 <= L0).all() and (L0 <= L).all()
        assert (L <= want).all(), (k, mode, int(np.flatnonzero(L > want)[0]))
        np.testing.assert_array_equal(out[0], want)
        assert out[2].sum() <= capped[2].sum(), (k, mode)


def test_ungated_hops_at_set_11():
    """match 2 > e_ins 1: the prune of row -1 is gated off; with the gates open the hop bound costs cells there as the ungapped did"""
    p = bsw_oracle_params(*BSW_PARAM_SETS[11])
    b = gabgen.bsw(2, N, 0)
    cells = {r: int(gabgen.bsw_exit_model(b, p, rule=r)[2].sum()) for r in ("default", "seed_ungated_hops", "seed_ungated", "seed_no_hops")}
    print(cells)
    assert cells["default"] <= cells["seed_ungated_hops"]
    assert cells["default"] <= cells["seed_no_hops"]


def corner_pair():
    """set 15 (match 127, mismatch and N -128, gaps 20 + 3 / 25 + 2): the first reference base is an N, row 0 is a row of zeros, the
    reference's row loop ends there and the score is h0 = 32 -- although one deleted reference base in front (32 - 23 = 9 > 0, the
    left edge is alive) would be followed by ten matches"""
    q = H.Q[:10]
    return gabgen.bsw_from_arrays([H.cat([4], q)], [q], [32])


def test_the_negative_control_hops_from_the_corner():
    p = bsw_oracle_params(*BSW_PARAM_SETS[15])
    b = corner_pair()
    want = pyoracle.bsw(b, p)[:, 0]
    assert want[0] == 32
    assert gabgen.bsw_seed_bound(b, p)[0] == 32 and gabgen.bsw_hop_bound(b, p)[0] == 32          # L == h0
    assert gabgen.bsw_hop_bound(b, p, wrong=True)[0] > 32                                        # the wrong rule: L > S
    np.testing.assert_array_equal(gabgen.bsw_exit_model(b, p)[0], want)
    # ... and on generated pairs at that set the control's L exceeds the score, the rule's never
    g = gabgen.bsw(2, N, 0)
    wg = pyoracle.bsw(g, p)[:, 0]
    over = (gabgen.bsw_hop_bound(g, p, wrong=True) > wg).sum()
    print(f"wrong_hop: L > score in {over} of {g.n} pairs")
    assert over > 0 and (gabgen.bsw_hop_bound(g, p) <= wg).all()
    assert (gabgen.bsw_exit_model(g, p, rule="wrong_hop")[0] != wg).sum() >= 0                   # (the model runs with it)


def oracle_scores(cs, p):
    """the oracle takes codes 0 .. 4 only: codes above count as N (4) in the kernels and the model"""
    b = gabgen.bsw_from_arrays([np.minimum(x[1], 4) for x in cs], [np.minimum(x[2], 4) for x in cs], [x[3] for x in cs])
    return pyoracle.bsw(b, p)[:, 0]


@pytest.mark.parametrize("cases,ps", [(H.cases, DEFAULTS), (H.zdrop_cases, DEFAULTS[:7] + (10,) + DEFAULTS[8:])], ids=["defaults", "zdrop10"])
def test_handmade_pairs_have_the_bound_written_out(cases, ps):
    cs = cases()
    b, p = H.batch(cs), bsw_oracle_params(*ps)
    L0, L, want = gabgen.bsw_seed_bound(b, p), gabgen.bsw_hop_bound(b, p), oracle_scores(cs, p)
    for i, (name, _, _, h0, e0, e1) in enumerate(cs):
        assert (L0[i], L[i]) == (e0, e1), (name, int(L0[i]), int(L[i]), e0, e1)
        assert h0 <= L0[i] <= L[i] <= want[i], (name, int(L[i]), int(want[i]))
    np.testing.assert_array_equal(gabgen.bsw_exit_model(b, p)[0], want)


def test_handmade_pairs_at_other_parameter_sets():
    """scores and L <= score wherever the pairs go; no hop outside the band: none at w = 0 (set 7), and with end_bonus = -1000
    (set 16: the clamp leaves w = 1) a single one-base hop only -- the two-base deletion and the second hop of 'two indels' stay out"""
    cs = H.cases()
    b = H.batch(cs)
    names = [x[0] for x in cs]
    for k in range(len(BSW_PARAM_SETS)):
        p = bsw_oracle_params(*BSW_PARAM_SETS[k])
        L0, L, want = gabgen.bsw_seed_bound(b, p), gabgen.bsw_hop_bound(b, p), oracle_scores(cs, p)
        assert (L0 <= L).all() and (L <= want).all(), (k, names[int(np.flatnonzero((L0 > L) | (L > want))[0])])
        np.testing.assert_array_equal(gabgen.bsw_exit_model(b, p)[0], want)
        if k == 7:
            np.testing.assert_array_equal(L, L0)
    p16, pd = bsw_oracle_params(*BSW_PARAM_SETS[16]), bsw_oracle_params(*DEFAULTS)
    L16, L0, Ld = gabgen.bsw_hop_bound(b, p16), gabgen.bsw_seed_bound(b, p16), gabgen.bsw_hop_bound(b, pd)
    at = names.index
    assert L16[at("indel after base 40")] == Ld[at("indel after base 40")] == 122            # |i - j| = 1
    assert L16[at("deletion of two after base 40")] == L0[at("deletion of two after base 40")] == 70      # |i - j| = 2
    assert L16[at("two indels")] == 60 - 7 + 29 + 3 * -4 < Ld[at("two indels")]                # one hop; its peak is the chunk end at step 32


def test_other_matrices_keep_the_ungapped_bound():
    """one mismatch score that differs from the others: not bwa_fill_scmat's form, no hops"""
    cs = H.cases()
    b, p = H.batch(cs), bsw_oracle_params(*DEFAULTS)
    assert (gabgen.bsw_hop_bound(b, p) > gabgen.bsw_seed_bound(b, p)).any()
    p.mat[1] = -3                     # A against C alone
    np.testing.assert_array_equal(gabgen.bsw_hop_bound(b, p), gabgen.bsw_seed_bound(b, p))
    g = gabgen.bsw(2, 2000, 0)
    np.testing.assert_array_equal(gabgen.bsw_hop_bound(g, p), gabgen.bsw_seed_bound(g, p))
    np.testing.assert_array_equal(gabgen.bsw_exit_model(g, p)[2], gabgen.bsw_exit_model(g, p, rule="seed_no_hops")[2])


def test_the_hops_fire_on_read_like_input():
    """necessary conditions, not measurements: on the first 50 000 mode-0 pairs at the defaults at most 0.70 of the cells of the same
    rule with the ungapped bound (the model gave 0.691 on 10 M pairs), the same rows per pair, no restart"""
    b = gabgen.bsw(2, 50000, 0)
    p = bsw_oracle_params(*DEFAULTS)
    new = gabgen.bsw_exit_model(b, p, restarts=True)
    old = gabgen.bsw_exit_model(b, p, restarts=True, rule="seed_no_hops")
    print(f"cells {new[2].sum()} of {old[2].sum()}: {new[2].sum() / old[2].sum():.4f}, restarted {new[4].sum()}")
    np.testing.assert_array_equal(new[0], old[0])
    assert new[2].sum() <= 0.70 * old[2].sum()
    np.testing.assert_array_equal(new[1], old[1])
    assert new[4].sum() == 0
