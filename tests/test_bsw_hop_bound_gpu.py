"""GPU: the hop bound of the seeded prune, as bsw_hist<true> and bsw_seed compute it (bsw.hip's header: "L with hops").

Every case goes through tests/test_bsw_early_exit_gpu.py's check(..., full=True): scores and the six fields of a six-field call on
the same handle equal to pyoracle.bsw with no tolerance, and last_stats()["cells"] of the score-only call equal to the cell sum of
tools/gen/bsw_exit_model.c (default rule) EXACTLY.  The cell count depends on every pair's L, so this pins the kernels' scan --
sixteen bases per load, chunks by their counts -- to the model's base-by-base statement of the rule.  The six-field call's cells
are the full sweep's: that form is untouched.  The change adds no launch, so tests/stream_order_cases.py covers it as it stands."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests import bsw_hop_cases as H
from tests.util import BSW_PARAM_SETS, bsw_oracle_params
from tests.test_bsw_early_exit_gpu import KERNEL_CASES, check, generator_batch, run
from tests.test_bsw_slices_gpu import check_sliced, reference, sw      # noqa: F401  (sw is a fixture)

pytestmark = pytest.mark.gpu

DEFAULTS = BSW_PARAM_SETS[0]
IDS = [k for k, *_ in KERNEL_CASES]
Q, TAIL, cat = H.Q, H.TAIL, H.cat


def hand_batch(qmax, lift):
    """the hand-made pairs whose codes the oracle takes, queries cut to qmax; every fifth h0 raised by `lift`"""
    cs = [x for x in H.cases() + H.zdrop_cases() if x[0] != "codes above 4"]
    b = H.batch(cs)
    h0 = b.h0.copy()
    h0[::5] += lift
    return gabgen.BswBatch(b.ref, b.ref_off, b.qry, b.qry_off, b.len1, np.minimum(b.len2, qmax).astype(np.int32), h0.astype(np.int32))


def hops(batch, ps):
    p = bsw_oracle_params(*ps)
    return int((gabgen.bsw_hop_bound(batch, p) > gabgen.bsw_seed_bound(batch, p)).sum())


@pytest.mark.parametrize("want_kernel,ps,qmax,h0_of", KERNEL_CASES, ids=IDS)
def test_handmade_pairs_in_every_kernel(monkeypatch, capfd, want_kernel, ps, qmax, h0_of):
    batch = hand_batch(qmax, {"dp16": 1000, "dp32": 40000}.get(want_kernel, 0))
    if want_kernel != "dp8<0,0>":              # (z-drop 10 under a match score of 4: the prunes are off there, and L with them)
        assert hops(batch, ps) > 0
    check(ps, batch, monkeypatch, capfd, want_kernel, full=True)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("want_kernel,ps,qmax,h0_of", KERNEL_CASES, ids=IDS)
def test_generated_pairs_in_every_kernel(monkeypatch, capfd, want_kernel, ps, qmax, h0_of, mode):
    batch = generator_batch(700 + mode, mode, qmax, h0_of, n=4096)
    n = hops(batch, ps)
    print(f"{want_kernel} mode {mode}: L_hop > L_ungapped in {n} of {batch.n} pairs")
    assert n > 0
    check(ps, batch, monkeypatch, capfd, want_kernel, full=True)


def test_sliced_call(sw, monkeypatch, capfd):      # noqa: F811
    """GAB_BSW_SLICE lowered: slice 0's L is made inside bsw_hist<true>, slice 1's by bsw_seed beside slice 0's DP"""
    h = hand_batch(151, 0)
    g = gabgen.bsw(712, 9001 - h.n, 0)
    refs = [h.pair(i)[0] for i in range(h.n)] + [g.pair(i)[0] for i in range(g.n)]
    qrys = [h.pair(i)[1] for i in range(h.n)] + [g.pair(i)[1] for i in range(g.n)]
    batch = gabgen.bsw_from_arrays(refs, qrys, list(h.h0) + list(g.h0))
    perm = np.random.default_rng(6).permutation(batch.n)          # hand-made pairs in both slices
    batch = gabgen.BswBatch(batch.ref, batch.ref_off[perm].copy(), batch.qry, batch.qry_off[perm].copy(), batch.len1[perm].copy(),
                            batch.len2[perm].copy(), batch.h0[perm].copy())
    assert hops(batch, DEFAULTS) > 1000
    want, mcells = reference(batch)
    check_sliced(sw, batch, want, mcells, monkeypatch, capfd)


def edge_pairs():
    """the scan's edges: every (qlen, tlen) from 1 to 35 around an indel, peaks and hop starts on both sides of the chunk ends, a
    mismatch and an N in the last byte of a chunk and in the first of the next"""
    refs, qrys = [], []
    indel3 = cat(Q[:3], Q[4:], TAIL)
    for ql in range(1, 36):
        for tl in range(1, 36):
            refs.append(indel3[:tl]); qrys.append(Q[:ql])
    for s in (15, 16, 17, 31, 32):
        # main-diagonal peak, and with it the hop's start, at step s; the same with a deleted reference base
        refs.append(cat(Q[:s], Q[s + 1:], TAIL)); qrys.append(Q)
        refs.append(cat(Q[:s], [(Q[s] + 1) % 4], Q[s:], TAIL)); qrys.append(Q)
        # the segment behind a first hop (from base 6) peaks at its step s: a second indel there
        refs.append(cat(Q[:5], Q[6:6 + s], Q[7 + s:], TAIL)); qrys.append(Q)
        # a mismatch at the segment's byte s - 1 and an N at byte s, and the other way round (s = 16, 32: the last byte of a chunk
        # and the first of the next)
        for a, b in ((s - 1, s), (s, s - 1)):
            r = cat(Q[:5], Q[6:], TAIL)
            r[5 + a] = (r[5 + a] + 1) % 4; r[5 + b] = 4
            refs.append(r); qrys.append(Q)
            q = Q.copy(); q[6 + b] = 4
            refs.append(cat(Q[:5], Q[6:], TAIL)); qrys.append(q)
    return refs, qrys


def test_scan_edges(monkeypatch, capfd):
    refs, qrys = edge_pairs()
    b = gabgen.bsw_from_arrays(refs, qrys, [30 + (k % 3) for k in range(len(refs))])
    # sequences start at every alignment modulo 4, and the slabs end exactly three bytes behind the last reference and the last query
    assert {(int(r) % 4, int(q) % 4) for r, q in zip(b.ref_off, b.qry_off)} == {(r, q) for r in range(4) for q in range(4)}
    rt, qt = int(b.ref_off[-1] + b.len1[-1]), int(b.qry_off[-1] + b.len2[-1])
    b = gabgen.BswBatch(b.ref[:rt + 3].copy(), b.ref_off, b.qry[:qt + 3].copy(), b.qry_off, b.len1, b.len2, b.h0)
    assert hops(b, DEFAULTS) > 500
    check(DEFAULTS, b, monkeypatch, capfd, "dp8<1,1>", full=True)


def test_codes_above_4(monkeypatch, capfd):
    """codes above 4 count as N in the scan as in the DP: the same scores and cells as with 4 in their place (the oracle takes 0 .. 4)"""
    g = gabgen.bsw(713, 2048, 0)
    rng = np.random.default_rng(7)
    ref, qry = g.ref.copy(), g.qry.copy()
    ref[rng.random(len(ref)) < 0.01] = 4; qry[rng.random(len(qry)) < 0.01] = 4
    clean = gabgen.BswBatch(ref, g.ref_off, qry, g.qry_off, g.len1, g.len2, g.h0)
    hi_ref, hi_qry = np.where(ref == 4, 5 + np.arange(len(ref)) % 251, ref).astype(np.uint8), np.where(qry == 4, 255, qry).astype(np.uint8)
    high = gabgen.BswBatch(hi_ref, g.ref_off, hi_qry, g.qry_off, g.len1, g.len2, g.h0)
    cs = [x for x in H.cases() if x[0] == "codes above 4"]
    p = bsw_oracle_params(*DEFAULTS)
    mcells = gabgen.bsw_exit_model(high, p)[2]
    np.testing.assert_array_equal(mcells, gabgen.bsw_exit_model(clean, p)[2])
    np.testing.assert_array_equal(gabgen.bsw_hop_bound(H.batch(cs), p), [cs[0][5]])
    assert hops(high, DEFAULTS) > 100
    check(DEFAULTS, clean, monkeypatch, capfd, "dp8<1,1>", full=True)
    got = run(DEFAULTS, high, monkeypatch, capfd)
    np.testing.assert_array_equal(got[0], pyoracle.bsw(clean, p)[:, 0])
    assert got[1] == int(mcells.sum())


def test_a_matrix_of_another_form_keeps_the_ungapped_bound():
    """one mismatch score that differs from the others: the per-base scan and the ungapped L, as the model does"""
    from genarchbench_amd.bsw import BandedPairWiseSW, bwa_fill_scmat
    g = gabgen.bsw(714, 4096, 0)
    cs = [x for x in H.cases() if x[0] != "codes above 4"]
    h = H.batch(cs)
    batch = gabgen.bsw_from_arrays([h.pair(i)[0] for i in range(h.n)] + [g.pair(i)[0] for i in range(g.n)],
                                   [h.pair(i)[1] for i in range(h.n)] + [g.pair(i)[1] for i in range(g.n)], list(h.h0) + list(g.h0))
    p = bsw_oracle_params(*DEFAULTS)
    mat = bwa_fill_scmat(1, 4, -1)
    mat[1] = -3
    p.mat[1] = -3
    want = pyoracle.bsw(batch, p)[:, 0]
    mscore, _, mcells, _ = gabgen.bsw_exit_model(batch, p)
    np.testing.assert_array_equal(mscore, want)
    np.testing.assert_array_equal(mcells, gabgen.bsw_exit_model(batch, p, rule="seed_no_hops")[2])
    sw = BandedPairWiseSW(mat=mat)                                 # noqa: F811
    try:
        np.testing.assert_array_equal(sw.getScores16(batch), want)
        assert sw.last_stats()["cells"] == int(mcells.sum())
    finally:
        sw.close()
