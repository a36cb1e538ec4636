"""CPU: the right-edge prune of the score-only bsw kernels and the four-cell cap of both prunes, as tools/gen/bsw_exit_model.c
restates them, against the oracle.

After a row, a score-only call zeroes the stored cells at the band's right edge that can no longer reach `best` and pulls `end` in
behind them; either edge moves over at most the four cells the zero trim has fetched (bsw.hip's header comment has the rule and
its proof).  This file checks the scores at every parameter set tests/test_bsw_left_prune.py uses, that the right prune really
fires, that the cap only ever keeps cells, and that the score check has teeth on the right side too."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params
from tests.test_bsw_left_prune import HAND_PARAMS, handmade, scores_match, with_zdrop

DEFAULTS = BSW_PARAM_SETS[0]
# every parameter set of tests/test_bsw_left_prune.py: its hand-made ones, its read-like ones and its adversarial z-drops
PARAMS = list(dict.fromkeys(HAND_PARAMS + [with_zdrop(DEFAULTS, 30), with_zdrop(DEFAULTS, 100, 20), BSW_PARAM_SETS[1], BSW_PARAM_SETS[5],
                                           (1, 1, -1, 1, 1, 1, 1, 100, 5, 100), with_zdrop(DEFAULTS, 20), with_zdrop(DEFAULTS, 10, 30),
                                           with_zdrop(DEFAULTS, 5)]))
assert len(PARAMS) >= 15
# a mismatch at -128 leaves rows of zeros next to a live left edge: what the zero-row guard is for
ZERO_ROWS = BSW_PARAM_SETS[14]
assert ZERO_ROWS[1] == 128 and ZERO_ROWS[7] == 100


def rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def right_edge_pairs(n=20000, seed=31):
    """long queries with a small h0 (the band starts narrow and grows to the right for many rows), a run of mismatches early on so
    that `best` stalls while the band still grows, and references one and two rows short of the query (the diagonal cannot reach
    the query's end), as long as it, and longer"""
    rng = np.random.default_rng(seed)
    refs, qrys, h0s = [], [], []
    for k in range(n):
        L = int(rng.integers(40, 250))
        q = rnd(rng, L)
        r = q.copy()
        at, run = int(rng.integers(2, 30)), int(rng.integers(1, 12))
        r[at:at + run] = (r[at:at + run] + 1 + rng.integers(0, 3, len(r[at:at + run]))) % 4
        tail = (-2, -1, 0, int(rng.integers(1, 40)))[k % 4]
        r = r[:L + tail] if tail < 0 else np.concatenate([r, rnd(rng, tail)])
        refs.append(r); qrys.append(q); h0s.append(int(rng.integers(0, 25)))
    return gabgen.bsw_from_arrays(refs, qrys, h0s)


def handmade_right():
    """2 000 pairs aimed at the right edge's bookkeeping: `end` on odd and on even columns (h0 sets where row -1 dies out),
    end == qlen (short queries under a large h0), a band that shrinks to one or two small cells and grows again over cells the
    prune has zeroed, a best path that runs RIGHT of the diagonal (bases missing from the reference), and references shorter than
    the query"""
    rng = np.random.default_rng(32)
    refs, qrys, h0s = [], [], []

    def add(r, q, h):
        refs.append(np.asarray(r, np.uint8)); qrys.append(np.asarray(q, np.uint8)); h0s.append(int(h))
    for k in range(400):
        L = int(rng.integers(30, 150))
        q = rnd(rng, L)
        add(np.concatenate([q, rnd(rng, k % 30)]), q, 7 + k % 60)                                   # end = h0 - 5 + 2: both parities
        add(np.concatenate([q[:5 + k % 25], rnd(rng, 20)]), q[:5 + k % 25], 60 + k % 41)             # row -1 live up to qlen: end == qlen
        h, a = 3 + k % 9, 2 + k % 5                                                                  # h + a matches, then mismatches down to 1..4
        m = max(1, (h + a - 1 - k % 2) // 4)
        r = q.copy(); r[a:a + m] = (r[a:a + m] + 1) % 4
        add(np.concatenate([r, rnd(rng, 10)]), q, h)
        g = 1 + k % 6                                                                                # g query bases missing from the reference
        cut = int(rng.integers(5, L - 10))
        add(np.concatenate([q[:cut], q[cut + g:], rnd(rng, 15)]), q, 10 + k % 80)
        add(q[:max(1, L - 1 - k % 40)], q, k % 101)                                                  # tlen < qlen
    return gabgen.bsw_from_arrays(refs, qrys, h0s)


@pytest.fixture(scope="module")
def bench():
    return gabgen.bsw(2, 50000, 0)


@pytest.fixture(scope="module")
def batches(bench):
    return {"read-like": bench, "adversarial": gabgen.bsw(3, 100000, 1), "right-edge": right_edge_pairs(), "hand-made": handmade_right()}


@pytest.mark.parametrize("ps", PARAMS, ids=["_".join(map(str, p)) for p in PARAMS])
def test_scores(batches, ps):
    for name, b in batches.items():
        out = scores_match(b, ps, restarts=True)
        p = bsw_oracle_params(*ps)
        c0 = gabgen.bsw_exit_model(b, p, rule="parent")[2]
        print(f"{name} {ps}: cells {out[2].sum() / c0.sum():.4f} of the rule's without the right prune and the cap, restarted {out[4].sum()} of {b.n}")


def test_the_zero_row_guard(batches):
    """pairs whose best path starts from the left edge after rows in which every band cell is zero (tests/test_bsw_left_prune.py's
    hand-made pairs, mismatch score -128): the right prune has dropped cells while column 0 is still held, the reference's row
    loop goes on over dead cells, and the pruned pass must be abandoned -- the rule without the right prune never restarts here
    (z-drop 100 is out of reach of these scores), the full rule does, and the scores are the oracle's on every batch"""
    b = handmade()
    p = bsw_oracle_params(*ZERO_ROWS)
    redo = scores_match(b, ZERO_ROWS, restarts=True)[4]
    redo_parent = gabgen.bsw_exit_model(b, p, restarts=True, rule="parent")[4]
    print(f"zero-row guard: {redo.sum()} of {b.n} pairs restart, {redo_parent.sum()} under the rule without the right prune")
    assert redo.sum() > 0 and redo_parent.sum() == 0
    for other in batches.values():
        scores_match(other, ZERO_ROWS)


def test_the_handmade_batch_holds_what_it_claims():
    b = handmade_right()
    assert b.n == 2000
    p = bsw_oracle_params(*DEFAULTS)
    on, off = gabgen.bsw_exit_model(b, p), gabgen.bsw_exit_model(b, p, rule="left_cap_only")
    for grp in range(5):                      # the right prune fires in every group
        sel = np.arange(b.n) % 5 == grp
        assert on[2][sel].sum() < off[2][sel].sum(), grp


def test_the_right_prune_fires_on_read_like_input(bench):
    """necessary condition, not a measurement: on the first 50 000 mode-0 pairs at the defaults the model evaluates 0.7250 of the
    cells of the rule without the right prune and the cap (profiles/bsw_right_prune.md); the threshold is that ratio plus two
    points.  Same rows as that rule and as the exit alone, same scores, no pair restarts"""
    p = bsw_oracle_params(*DEFAULTS)
    s0, r0, c0, _ = gabgen.bsw_exit_model(bench, p, prune=False)
    s3, r3, c3, _ = gabgen.bsw_exit_model(bench, p, rule="parent")
    s1, r1, c1, _, redo = scores_match(bench, DEFAULTS, restarts=True)
    print(f"cells {c1.sum() / c3.sum():.4f} of the rule's without the right prune, {c1.sum() / c0.sum():.4f} of the exit-only model's, restarted {redo.sum()}")
    np.testing.assert_array_equal(s0, s1)
    assert c1.sum() <= 0.7450 * c3.sum()
    assert redo.sum() == 0
    np.testing.assert_array_equal(r3, r1)
    np.testing.assert_array_equal(r0, r1)


def test_the_cap_only_keeps_cells(batches):
    """per pair, the capped left rule evaluates at least the cells of the uncapped one (it drops a subset of them per row), with
    the same scores"""
    p = bsw_oracle_params(*DEFAULTS)
    for name, b in batches.items():
        su, _, cu, _ = gabgen.bsw_exit_model(b, p, rule="parent")
        sc, _, cc, _ = gabgen.bsw_exit_model(b, p, rule="left_cap_only")
        print(f"{name}: capped / uncapped left prune {cc.sum() / cu.sum():.4f}")
        np.testing.assert_array_equal(su, sc)
        assert (cc >= cu).all(), name


def test_a_wrong_right_potential_changes_scores(bench):
    """negative control: with the right potential two columns short the prune zeroes cells that still reach `best`"""
    p = bsw_oracle_params(*DEFAULTS)
    want = pyoracle.bsw(bench, p)[:, 0]
    score = gabgen.bsw_exit_model(bench, p, rule="wrong_right")[0]
    print(f"wrong right potential: {(score != want).sum()} of {bench.n} scores differ")
    assert (score != want).sum() > bench.n // 10
