"""GPU: the left-edge prune of the six bsw DP kernels against the oracle and the CPU model of the rule.

A score-only call (result_out NULL) moves the band's left edge over cells that can no longer reach `best`, and sends a pair whose
pruned pass meets a possible z-drop through a second pass without the prune (bsw.hip's header comment; tests/test_bsw_left_prune.py
checks the rule itself on the CPU).  Every case goes through the three entry points -- run_device score-only, run_device with the
six-field result, and gab_bsw_run behind getScores16 -- with the helpers of tests/test_bsw_early_exit_gpu.py: scores against the
oracle with no tolerance, the score-only cell counter against tools/gen/bsw_exit_model.c (abandoned passes included), the
six-field call's counter against the oracle's, unchanged."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params
from tests.test_bsw_early_exit_gpu import byte_h0, check, generator_batch, lifted_h0

pytestmark = pytest.mark.gpu

DEFAULTS = BSW_PARAM_SETS[0]


def with_zdrop(ps, zdrop, w=None):
    return ps[:7] + (zdrop,) + ps[8:9] + (ps[9] if w is None else w,)


def model(batch, ps, **kw):
    return gabgen.bsw_exit_model(batch, bsw_oracle_params(*ps), **kw)


# (kernel, parameters, qmax, h0) as in tests/test_bsw_kernels_gpu.py: the byte kernels take h0 up to 255 - qcap * max_sc; every
# set has zdrop >= 8 * max_sc and w = 100, so the prune is on for every pair whose row -1 dies out inside the first row's band
KERNEL_CASES = [
    ("dp8<1,1>", DEFAULTS, 151, byte_h0(255 - 160)),
    ("dp8<1,0>", (2, 3, -2, 5, 2, 5, 2, 50, 30, 100), 112, byte_h0(255 - 224)),
    ("dp8<0,1>", (1, 4, -1, 6, 1, 7, 1, 100, 5, 100), 151, byte_h0(255 - 160)),
    ("dp8<0,0>", (4, 1, -1, 2, 1, 9, 2, 100, 0, 100), 48, byte_h0(255 - 192)),
    ("dp16", DEFAULTS, 256, lifted_h0(100, 97, 1000)),
    ("dp32", DEFAULTS, 256, lifted_h0(100, 5, 40000)),
]


@pytest.mark.parametrize("want_kernel,ps,qmax,h0_of", KERNEL_CASES, ids=[k for k, *_ in KERNEL_CASES])
def test_every_kernel_on_read_like_pairs(monkeypatch, capfd, want_kernel, ps, qmax, h0_of):
    batch = generator_batch(400, 0, qmax, h0_of)
    _, _, cells = check(ps, batch, monkeypatch, capfd, want_kernel, full=True)
    exit_only = int(model(batch, ps, prune=False)[2].sum())
    print(f"{want_kernel}: {cells / exit_only:.4f} of the exit-only model's cells")
    assert cells < 0.95 * exit_only          # the prune really fires in this kernel


@pytest.mark.parametrize("want_kernel,qmax,h0_of", [("dp8<1,1>", 151, byte_h0(255 - 160)), ("dp16", 256, lifted_h0(100, 97, 1000)),
                                                    ("dp32", 256, lifted_h0(100, 5, 40000))], ids=["dp8", "dp16", "dp32"])
@pytest.mark.parametrize("zdrop,w", [(10, 100), (20, 100), (10, 30)])
def test_pairs_that_restart(monkeypatch, capfd, want_kernel, qmax, h0_of, zdrop, w):
    """adversarial pairs at a small z-drop: the model shows pairs that abandon the pruned pass, and the counter holds both passes"""
    ps = with_zdrop(DEFAULTS, zdrop, w)
    batch = generator_batch(410, 1, qmax, h0_of, n=16384)
    redo = model(batch, ps, restarts=True)[4]
    print(f"{want_kernel} z-drop {zdrop} w {w}: {redo.sum()} of {batch.n} pairs restart")
    assert redo.sum() > 0
    check(ps, batch, monkeypatch, capfd, want_kernel, full=True)


def test_asymmetric_and_large_scores_with_restarts(monkeypatch, capfd):
    """the other byte instantiations on adversarial pairs, z-drop just above the 8 x max_sc gate"""
    for want_kernel, ps, qmax, hmax in (("dp8<1,0>", (2, 3, -2, 5, 2, 5, 2, 16, 30, 100), 112, 255 - 224),
                                        ("dp8<0,1>", (1, 4, -1, 6, 1, 7, 1, 8, 5, 100), 151, 255 - 160),
                                        ("dp8<0,0>", (4, 1, -1, 2, 1, 9, 2, 32, 0, 100), 48, 255 - 192)):
        batch = generator_batch(420, 1, qmax, byte_h0(hmax), n=8192)
        check(ps, batch, monkeypatch, capfd, want_kernel, full=True)


# ------------------------------------------------------------------------------------------------ hand-made edges
def rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def edges():
    rng = np.random.default_rng(21)
    refs, qrys, h0s = [], [], []

    def add(r, q, h):
        refs.append(np.asarray(r, np.uint8)); qrys.append(np.asarray(q, np.uint8)); h0s.append(int(h))
    for k in range(96):
        L = int(rng.integers(4, 150))
        q = rnd(rng, L)
        for ql in (1, 2, 3):                                                   # tiny queries, short and long references
            add(rnd(rng, int(rng.integers(1, 40))), q[:ql], rng.integers(0, 95))
        add(q[:max(1, L // 2 - k % 5)], q, rng.integers(0, 95))                # tlen < qlen: the rows left limit the potential
        add(np.concatenate([q, rnd(rng, k % 4)]), q, 95)                       # perfect match, a few rows more: the whole band goes in one row
        add(np.concatenate([q, rnd(rng, 40)]), q, k % 95)                      # ... and a long tail behind it
        add(np.concatenate([rnd(rng, 1 + k % 9), q, rnd(rng, 30)]), q, 95)     # diagonal shifted by 1..9 rows: the prune lands on either parity
        add(np.concatenate([q[:L // 2], q[L // 2 + 1 + k % 3:], rnd(rng, 25)]), q, 20 + k % 70)    # insertion: the path runs left of the diagonal
    return gabgen.bsw_from_arrays(refs, qrys, h0s)


EDGE_PARAMS = [DEFAULTS, with_zdrop(DEFAULTS, 10), (1, 4, -1, 0, 1, 6, 1, 100, 5, 100), (1, 4, -1, 1, 1, 1, 1, 0, 5, 100),
               with_zdrop(DEFAULTS, 100, 12)]


@pytest.mark.parametrize("ps", EDGE_PARAMS, ids=["_".join(map(str, p)) for p in EDGE_PARAMS])
def test_handmade_edges(monkeypatch, capfd, ps):
    """qlen 1..3, tlen < qlen, h0 at the byte kernel's limit with o_del 0 and 1 (the left boundary stays live for many rows), shifted
    diagonals (beg lands on odd and on even columns), perfect matches that end a few rows before the reference (the last rows
    prune the whole band)"""
    batch = edges()
    check(ps, batch, monkeypatch, capfd, f"dp8<{int(ps[3] + ps[4] == ps[5] + ps[6])},1>", full=True)
    big = gabgen.BswBatch(batch.ref, batch.ref_off, batch.qry, batch.qry_off, batch.len1, batch.len2, batch.h0.copy())
    big.h0[::7] = 1000
    check(ps, big, monkeypatch, capfd, "dp16")
    big.h0[::7] = 70000
    check(ps, big, monkeypatch, capfd, "dp32")


def test_the_prune_fires_in_the_edge_batch():
    """the model's part of the edge batch's claim: the prune fires in it without changing a score (a perfect match that ends k rows
    before its reference has every cell, the diagonal's included, at potential <= best after its last matching row: the band is
    empty in the next row, which the kernels must survive)"""
    batch = edges()
    on, off = model(batch, DEFAULTS), model(batch, DEFAULTS, prune=False)
    np.testing.assert_array_equal(on[0], pyoracle.bsw(batch, bsw_oracle_params(*DEFAULTS))[:, 0])
    assert on[2].sum() < 0.9 * off[2].sum()
    perfect = np.arange(batch.n) % 8 == 4                  # the fifth pair of every group of eight, k = 1..3 rows more
    more = perfect & (batch.len1 > batch.len2)
    assert more.any() and (on[2][more] < off[2][more]).all()
