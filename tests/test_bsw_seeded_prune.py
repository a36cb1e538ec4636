"""CPU: the seeded prune of the score-only bsw kernels, as tools/gen/bsw_exit_model.c restates it, against the oracle.

Before row 0 the ungapped extension along the main diagonal gives a lower bound L of the pair's final score; the prunes and two
of their guards test against max(best, L - 1) instead of `best`, and the dead cells of row -1 are dropped before row 0 (bsw.hip's
header comment has the rule, its gates and the proof).  This file checks the model's scores and L against the oracle at every
parameter set and both generator modes, that the negative control (threshold L) really loses a score where the rule does not,
the economy conditions, and hand-made pairs aimed at the seed's edge cases."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params

DEFAULTS = BSW_PARAM_SETS[0]
N = 20000
ACGT = np.array([k % 4 for k in range(0, 997, 7)], np.uint8)           # 143 bases, no repeat of period < 4


@pytest.fixture(scope="module")
def batches():
    return {0: gabgen.bsw(2, N, 0), 1: gabgen.bsw(3, N, 1)}


def handmade():
    """-> (batch, names): one pair per named edge case of the seed, then each again with a few other h0"""
    refs, qrys, h0s, names = [], [], [], []

    def add(name, r, q, h):
        refs.append(np.asarray(r, np.uint8)); qrys.append(np.asarray(q, np.uint8)); h0s.append(int(h)); names.append(name)
    q = ACGT[:100]
    other = (q + 1) % 4
    for h in (30, 1, 95, 0):
        add("perfect match", q, q, h)
        add("perfect match, longer reference", np.concatenate([q, other[:40]]), q, h)
        add("one mismatch at the last base", np.concatenate([q[:-1], other[-1:]]), q, h)
        add("indel at base 1", np.concatenate([q[:1], q[2:], other[:20]]), q, h)           # the diagonal breaks at once: L = h0
        add("insertion at base 1", np.concatenate([q[:1], other[:1], q[1:], other[:20]]), q, h)
        add("qlen 1", q[:30], q[:1], h)
        add("tlen 1", q[:1], q[:30], h)
        add("qlen 1 tlen 1 mismatch", other[:1], q[:1], h)
        add("tlen < qlen", q[:60], q, h)
        add("N in both", np.where(np.arange(100) % 9 == 4, 4, q), np.where(np.arange(100) % 7 == 3, 4, q), h)
        add("match, break, match", np.concatenate([q[:40], other[40:48], q[48:]]), q, h)
        add("dip below the z-drop and back", np.concatenate([q[:10], other[10:40], q[40:]]), q[:100], h)
    # d reaching exactly 0: h0 = 4 * k mismatches' worth is used up by k mismatches at the start (mismatch -4 at the defaults)
    for k in (1, 2, 5):
        add("d reaches exactly 0", np.concatenate([other[:k], q[k:]]), q, 4 * k)
        add("d stays at 1", np.concatenate([other[:k], q[k:]]), q, 4 * k + 1)
    # h0 so large that row -1 is live behind the first band clamp: restriction (a) fails with a narrow band (w = 10 below)
    add("h0 fails restriction (a)", q, q, 120)
    add("h0 fails restriction (a), mismatches", np.concatenate([q[:50], other[50:53], q[53:]]), q, 120)
    return gabgen.bsw_from_arrays(refs, qrys, h0s), names


NARROW = DEFAULTS[:9] + (10,)                # w = 10: h0 = 120 leaves row -1 live behind the clamp of row 0 (120 - 7 - 11 > 0)
HAND_PARAMS = [DEFAULTS, NARROW, BSW_PARAM_SETS[1], BSW_PARAM_SETS[2], BSW_PARAM_SETS[11], BSW_PARAM_SETS[14],
               DEFAULTS[:7] + (20,) + DEFAULTS[8:], DEFAULTS[:7] + (8,) + DEFAULTS[8:]]


def model_vs_oracle(b, ps, rule="default"):
    p = bsw_oracle_params(*ps)
    want = pyoracle.bsw(b, p)[:, 0]
    out = gabgen.bsw_exit_model(b, p, restarts=True, rule=rule)
    return want, out, gabgen.bsw_seed_bound(b, p)


@pytest.mark.parametrize("k", range(len(BSW_PARAM_SETS)), ids=["_".join(map(str, p)) for p in BSW_PARAM_SETS])
def test_scores_bound_and_economy_at_every_parameter_set(batches, k):
    """scores == oracle, L <= the oracle's score for every pair, and no more cells than the rule before the seed"""
    ps = BSW_PARAM_SETS[k]
    for mode, b in batches.items():
        want, out, L = model_vs_oracle(b, ps)
        capped = gabgen.bsw_exit_model(b, bsw_oracle_params(*ps), rule="capped")
        print(f"set {k} mode {mode}: cells {out[2].sum()} of {capped[2].sum()} ({out[2].sum() / capped[2].sum():.4f}), restarted {out[4].sum()}, "
              f"L == score in {(L == want).sum()} pairs")
        np.testing.assert_array_equal(out[0], want)
        np.testing.assert_array_equal(capped[0], want)
        assert (L <= want).all(), (k, mode, int(np.flatnonzero(L > want)[0]))
        assert (L >= b.h0).all()
        assert out[2].sum() <= capped[2].sum(), (k, mode)


def test_the_seed_fires_on_read_like_input():
    """necessary condition, not a measurement: on the first 50 000 mode-0 pairs at the defaults at most 0.80 of the cells of the
    rule before the seed (the model gave 0.765 on 200 000), the same rows and no restart"""
    b = gabgen.bsw(2, 50000, 0)
    want, out, _ = model_vs_oracle(b, DEFAULTS)
    capped = gabgen.bsw_exit_model(b, bsw_oracle_params(*DEFAULTS), rule="capped")
    print(f"cells {out[2].sum() / capped[2].sum():.4f} of the rule's before the seed, restarted {out[4].sum()}")
    np.testing.assert_array_equal(out[0], want)
    assert out[2].sum() <= 0.80 * capped[2].sum()
    assert out[4].sum() == 0
    np.testing.assert_array_equal(out[1], capped[1])


def test_the_negative_control_loses_a_perfect_match():
    """threshold L instead of L - 1: every cell of a perfect ungapped match's diagonal has potential exactly L = h0 + qlen, so the
    wrong rule drops the path that reaches the score; the real rule does not"""
    b, names = handmade()
    i = names.index("perfect match")
    one = gabgen.bsw_from_arrays([b.pair(i)[0]], [b.pair(i)[1]], [b.pair(i)[2]])
    want, out, L = model_vs_oracle(one, DEFAULTS)
    wrong = gabgen.bsw_exit_model(one, bsw_oracle_params(*DEFAULTS), rule="wrong_seed")[0]
    assert want[0] == 130 and L[0] == 130 and out[0][0] == 130
    assert wrong[0] != want[0]
    # and on generated pairs the control is wrong often, the rule never
    g = gabgen.bsw(2, N, 0)
    want, out, _ = model_vs_oracle(g, DEFAULTS)
    wrong = gabgen.bsw_exit_model(g, bsw_oracle_params(*DEFAULTS), rule="wrong_seed")[0]
    print(f"wrong seed: {(wrong != want).sum()} of {g.n} scores differ")
    np.testing.assert_array_equal(out[0], want)
    assert (wrong != want).sum() > 0


@pytest.mark.parametrize("ps", HAND_PARAMS, ids=["_".join(map(str, p)) for p in HAND_PARAMS])
def test_handmade_pairs(ps):
    b, names = handmade()
    want, out, L = model_vs_oracle(b, ps)
    bad = np.flatnonzero(out[0] != want)
    assert len(bad) == 0, (names[bad[0]], int(b.h0[bad[0]]), int(out[0][bad[0]]), int(want[bad[0]]))
    over = np.flatnonzero(L > want)
    assert len(over) == 0, (names[over[0]], int(b.h0[over[0]]), int(L[over[0]]), int(want[over[0]]))


def test_the_handmade_pairs_hold_what_they_claim():
    b, names = handmade()
    p = bsw_oracle_params(*DEFAULTS)
    L = gabgen.bsw_seed_bound(b, p)
    want = pyoracle.bsw(b, p)[:, 0]
    at = lambda name, h: next(i for i in range(b.n) if names[i] == name and b.h0[i] == h)
    assert L[at("perfect match", 30)] == 130 == want[at("perfect match", 30)]
    assert L[at("one mismatch at the last base", 30)] == 129 == want[at("one mismatch at the last base", 30)]
    assert L[at("indel at base 1", 30)] == 31                      # one matching base, then the diagonal is lost
    assert want[at("indel at base 1", 30)] > 100                   # ... and the gapped path goes on
    assert L[at("perfect match", 0)] == 0                          # h0 = 0: d <= 0 before the first base
    assert L[at("qlen 1", 30)] == 31 and L[at("tlen 1", 30)] == 31 and L[at("qlen 1 tlen 1 mismatch", 30)] == 30
    assert L[at("tlen < qlen", 30)] == 90
    for k in (1, 2, 5):
        assert L[at("d reaches exactly 0", 4 * k)] == 4 * k          # the scan stops there, matches behind it do not count
        assert L[at("d stays at 1", 4 * k + 1)] > 4 * k + 1
    # codes above 4 count as N in the seed as in the kernels (the oracle is not asked: it takes codes 0 .. 4 only)
    q = ACGT[:100]
    r4, q4 = np.where(np.arange(100) % 11 == 5, 4, q), np.where(np.arange(100) % 13 == 6, 4, q)
    r9, q9 = np.where(r4 == 4, 9, r4), np.where(q4 == 4, 200, q4)
    two = gabgen.bsw_from_arrays([r4, r9], [q4, q9], [30, 30])
    L2 = gabgen.bsw_seed_bound(two, p)
    assert L2[0] == L2[1] and 30 < L2[0] < 130
    # restriction (a): with w = 10 the pair keeps the reference's cells, with the default band it is pruned
    i = at("h0 fails restriction (a)", 120)
    one = gabgen.bsw_from_arrays([b.pair(i)[0]], [b.pair(i)[1]], [120])
    narrow = [gabgen.bsw_exit_model(one, bsw_oracle_params(*NARROW), rule=r)[2][0] for r in ("default", "capped")]
    exit_only = gabgen.bsw_exit_model(one, bsw_oracle_params(*NARROW), prune=False)[2][0]
    wide = [gabgen.bsw_exit_model(one, p, rule=r)[2][0] for r in ("default", "capped")]
    assert narrow[0] == narrow[1] == exit_only and wide[0] < wide[1]


def test_the_row_minus_one_prune_is_gated():
    """max_sc > e_ins (set 11: match 2, e_ins 1): the prune of row -1 is off, the threshold is on; ungated, the right-edge guard
    restarts thousands of the read-like pairs and the cell count rises above the rule's before the seed"""
    ps = BSW_PARAM_SETS[11]
    assert ps[0] > ps[6]
    p = bsw_oracle_params(*ps)
    b = gabgen.bsw(2, N, 0)
    cells = {r: gabgen.bsw_exit_model(b, p, restarts=True, rule=r) for r in ("default", "seed_thr_only", "seed_ungated", "capped")}
    print({r: (int(o[2].sum()), int(o[4].sum())) for r, o in cells.items()})
    np.testing.assert_array_equal(cells["default"][2], cells["seed_thr_only"][2])
    assert cells["seed_ungated"][2].sum() > cells["capped"][2].sum() and cells["seed_ungated"][4].sum() > b.n // 10
    assert cells["default"][2].sum() < cells["capped"][2].sum()
