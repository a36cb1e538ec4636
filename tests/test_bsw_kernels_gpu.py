"""GPU: every bsw DP kernel against the oracle, all six result fields, across scoring parameters and cell widths.

gab_bsw_run_device picks one of six DP kernels per launch (bsw.hip): bsw_dp8<SYM, MS1> (8-bit cells, four instantiations) when
max(h0) + qcap * max_sc <= 255, bsw_dp<false> (16-bit packed cells) up to 32767, bsw_dp<true> (32-bit cells) above.  SYM means
o_del + e_del == o_ins + e_ins, MS1 means max_sc <= 1.  With GAB_BSW_TRACE set, every DP launch prints the kernel it runs; each
test asserts from those lines that the kernel it targets really ran.  The oracle is pinned to the reference's scalarBandedSWA at
these parameters by tests/test_bsw_oracle.py, so it is the truth here: no tolerance, all six fields."""
import re

import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_handmade_pairs, bsw_oracle_params

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"\[gab_bsw_dp \S+\] class (\d+) qcap (\d+) pairs (\d+) bits (\d+) sym (\d) ms1 (\d)")
DEFAULTS = BSW_PARAM_SETS[0]


def kernel(bits, sym, ms1):
    return f"dp8<{int(sym)},{int(ms1)}>" if bits == 8 else f"dp{bits}"


def sym_ms1(ps):
    a, b, amb, od, ed, oi, ei = ps[:7]
    return od + ed == oi + ei, max(a, -b, amb, 0) <= 1


def launches(err):
    """the DP launches the trace lines on stderr report: [(class, qcap, pairs, kernel name)]"""
    return [(int(c), int(q), int(n), kernel(int(bits), int(s), int(m))) for c, q, n, bits, s, m in TRACE.findall(err)]


def run_both(ps, batch, monkeypatch, capfd, host=True):
    """batch through run_device (all six fields) and getScores16 (scores) on a fresh handle with parameters ps; both compared
    with the oracle.  Returns the launches the device call made."""
    import torch
    from genarchbench_amd.bsw import BandedPairWiseSW, bwa_fill_scmat
    a, b, amb, od, ed, oi, ei, zd, eb, w = ps
    want = pyoracle.bsw(batch, bsw_oracle_params(*ps))
    monkeypatch.setenv("GAB_BSW_TRACE", "1")
    sw = BandedPairWiseSW(od, ed, oi, ei, zd, eb, bwa_fill_scmat(a, b, amb), w)
    try:
        dev = torch.device("cuda:0")
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        score = torch.full((batch.n,), -7, dtype=torch.int32, device=dev)
        res = torch.full((batch.n, 6), -7, dtype=torch.int32, device=dev)
        capfd.readouterr()
        sw.run_device(t(batch.ref), t(batch.ref_off), t(batch.qry), t(batch.qry_off), t(batch.len1), t(batch.len2), t(batch.h0),
                      score, res, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dev_launches = launches(capfd.readouterr().err)
        assert sum(n for _, _, n, _ in dev_launches) == batch.n, dev_launches
        got = res.cpu().numpy()
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (f"{len(bad)} of {batch.n} pairs differ (kernels {sorted({k for *_, k in dev_launches})}); first: pair "
                               f"{bad[0]} qlen {batch.len2[bad[0]]} tlen {batch.len1[bad[0]]} h0 {batch.h0[bad[0]]}: "
                               f"got {got[bad[0]].tolist()} want {want[bad[0]].tolist()}")
        np.testing.assert_array_equal(score.cpu().numpy(), want[:, 0])
        if host:
            np.testing.assert_array_equal(sw.getScores16(batch), want[:, 0])
            assert [k for *_, k in launches(capfd.readouterr().err)] == [k for *_, k in dev_launches]
    finally:
        sw.close()
    return dev_launches, want


def subset(batch, idx, h0=None):
    """pairs idx of batch (same slabs), optionally with new h0 values"""
    idx = np.asarray(idx)
    return gabgen.BswBatch(batch.ref, batch.ref_off[idx].copy(), batch.qry, batch.qry_off[idx].copy(), batch.len1[idx].copy(),
                           batch.len2[idx].copy(), batch.h0[idx].copy() if h0 is None else np.asarray(h0, np.int32))


def bounded_batch(seed, qmax, hmax, n=4000):
    """generator pairs of both modes and the hand-made pairs with query length <= qmax, h0 drawn from [0, hmax] (one pair at
    hmax exactly): max(h0) + qcap * max_sc is then fixed by the caller's choice of qmax and hmax"""
    rng = np.random.default_rng(seed)
    refs, qrys = [], []
    for mode in (1, 0):
        b = gabgen.bsw(seed + mode, n, mode)
        for i in np.flatnonzero(b.len2 <= qmax):
            r, q, _ = b.pair(i)
            refs.append(r); qrys.append(q)
    hr, hq, _ = bsw_handmade_pairs()
    for r, q in zip(hr, hq):
        if len(q) <= qmax:
            refs.append(r); qrys.append(q)
    h0 = rng.integers(0, hmax + 1, len(refs))
    h0[len(h0) // 3] = hmax
    return gabgen.bsw_from_arrays(refs, qrys, [int(v) for v in h0])


def qcap_of(q):
    return (q + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ every kernel, >= 2 sets each
# byte kernels: (parameters, qmax); h0 then goes up to 255 - qcap * max_sc, the largest the byte kernel takes
BYTE_CASES = [
    ("dp8<1,1>", DEFAULTS, 151),
    ("dp8<1,1>", (1, 1, 0, 0, 1, 0, 1, 0, 5, 100), 100),
    ("dp8<1,1>", (0, 4, -1, 6, 1, 6, 1, 100, 5, 100), 250),
    ("dp8<1,1>", (-2, 3, -1, 6, 1, 6, 1, 100, 5, 100), 250),
    ("dp8<1,1>", (1, 128, -1, 6, 1, 6, 1, 100, 5, 100), 140),
    ("dp8<1,0>", (2, 3, -2, 5, 2, 5, 2, 50, 30, 30), 112),
    ("dp8<1,0>", (2, 4, 2, 6, 1, 6, 1, 100, 5, 100), 100),
    ("dp8<1,0>", (3, 5, -1, 7, 3, 8, 2, 200, 5, 5), 80),           # o_ins != o_del, o + e equal
    ("dp8<0,1>", (1, 4, -1, 6, 1, 7, 1, 100, 5, 100), 151),
    ("dp8<0,1>", (1, 1, 0, 0, 1, 3, 2, 0, 5, 100), 120),
    ("dp8<0,1>", (1, 4, -1, 6, 1, 6, 1, 100, 5, 100)[:5] + (2, 3, 1, -5, 7), 128),
    ("dp8<0,0>", (3, 5, -1, 7, 3, 8, 3, 200, 5, 5), 80),
    ("dp8<0,0>", (4, 1, -1, 2, 1, 9, 2, 10, 0, 100), 48),
    ("dp8<0,0>", (5, 9, -3, 11, 2, 3, 4, 30, -20, 17), 40),
    ("dp8<1,0>", (2, 3, -1, 1000, 200, 900, 300, 100, 5, 100), 100),    # gaps far above any score
]


@pytest.mark.parametrize("want_kernel,ps,qmax", BYTE_CASES, ids=[f"{k}-{'_'.join(map(str, p))}" for k, p, _ in BYTE_CASES])
def test_byte_kernels(monkeypatch, capfd, want_kernel, ps, qmax):
    max_sc = max(ps[0], -ps[1], ps[2], 0)
    hmax = 255 - qcap_of(qmax) * max_sc
    assert hmax >= 0
    batch = bounded_batch(1000 + qmax, qmax, hmax)
    ran, _ = run_both(ps, batch, monkeypatch, capfd)
    assert [k for *_, k in ran] == [want_kernel], ran
    assert kernel(8, *sym_ms1(ps)) == want_kernel


# 16-bit and 32-bit cells: (parameters, h0 scale); the generator's adversarial mode draws h0 up to 1000
WIDE_CASES = [
    ("dp16", DEFAULTS, None),
    ("dp16", (2, 3, -2, 5, 2, 5, 2, 50, 30, 30), None),
    ("dp16", (4, 1, -1, 2, 1, 9, 2, 10, 0, 100), None),
    ("dp16", (1, 4, -1, 6, 1, 7, 1, 100, 5, 100), None),
    ("dp16", (5, 9, -3, 11, 2, 3, 4, 30, -20, 17), None),
    ("dp16", (1, 4, -1, 6, 1, 6, 1, 1, -5, 100), None),
    ("dp32", (127, 4, -1, 6, 1, 6, 1, 100, 5, 100), None),
    ("dp32", (127, 128, -128, 20, 3, 25, 2, 500, 10, 50), None),
    ("dp32", DEFAULTS, 40000),
    ("dp32", (3, 5, -1, 7, 3, 8, 3, 200, 5, 5), 33000),
]


@pytest.mark.parametrize("k", range(len(WIDE_CASES)), ids=[f"{k}-{'_'.join(map(str, p))}-{h}" for k, p, h in WIDE_CASES])
def test_wide_kernels(monkeypatch, capfd, k):
    want_kernel, ps, big_h0 = WIDE_CASES[k]
    b = gabgen.bsw(2000 + k, 3000, 1)
    if big_h0:
        b.h0[::5] += big_h0
    ran, _ = run_both(ps, b, monkeypatch, capfd)
    assert [k for *_, k in ran] == [want_kernel], ran


# ------------------------------------------------------------------------------------------------ exact limits
def perfect_matches(qlen, h0, n=70, seed=5):
    """n pairs whose best score is h0 + qlen * a exactly: the query is the reference's prefix (some references have a random
    tail behind it, some an N tail)"""
    rng = np.random.default_rng(seed)
    refs, qrys = [], []
    for k in range(n):
        q = rng.integers(0, 4, qlen).astype(np.uint8)
        tail = [np.zeros(0, np.uint8), rng.integers(0, 4, int(rng.integers(1, 300))).astype(np.uint8), np.full(7, 4, np.uint8)][k % 3]
        refs.append(np.concatenate([q, tail])); qrys.append(q)
    return gabgen.bsw_from_arrays(refs, qrys, [h0] * n)


# (parameters, query length = qcap): the byte kernel's limit h0 + qcap * a = 255 and one past it
BYTE_LIMITS = [
    (DEFAULTS, 160),                                        # SYM, MS1
    ((1, 4, -1, 6, 1, 7, 1, 100, 5, 100), 160),             # MS1, not SYM
    ((2, 3, -2, 5, 2, 5, 2, 50, 30, 30), 112),              # SYM, not MS1
    ((4, 1, -1, 2, 1, 9, 2, 10, 0, 100), 48),               # neither
    ((1, 4, -1, 6, 1, 6, 1, 100, 5, 100), 16),              # the smallest class
]


@pytest.mark.parametrize("over", [0, 1], ids=["fits", "one_past"])
@pytest.mark.parametrize("ps,qlen", BYTE_LIMITS, ids=["_".join(map(str, p)) + f"-q{q}" for p, q in BYTE_LIMITS])
def test_byte_cell_limit(monkeypatch, capfd, ps, qlen, over):
    a = ps[0]
    batch = perfect_matches(qlen, 255 - qlen * a + over)
    ran, want = run_both(ps, batch, monkeypatch, capfd)
    assert want[:, 0].max() == 255 + over
    assert [k for *_, k in ran] == [kernel(8, *sym_ms1(ps)) if not over else "dp16"], ran


# the 16-bit kernel's limit h0 + 256 * a = 32767 and one past it (a = 1 and the largest int8 match score)
WORD_LIMITS = [(DEFAULTS, 32511), ((127, 4, -1, 6, 1, 6, 1, 100, 5, 100), 255), ((127, 128, -128, 20, 3, 25, 2, 500, 10, 50), 255)]


@pytest.mark.parametrize("over", [0, 1], ids=["fits", "one_past"])
@pytest.mark.parametrize("ps,h0", WORD_LIMITS, ids=["_".join(map(str, p)) for p, _ in WORD_LIMITS])
def test_word_cell_limit(monkeypatch, capfd, ps, h0, over):
    batch = perfect_matches(256, h0 + over, n=40)
    ran, want = run_both(ps, batch, monkeypatch, capfd)
    assert want[:, 0].max() == 32767 + over
    assert [k for *_, k in ran] == ["dp32" if over else "dp16"], ran


# ------------------------------------------------------------------------------------------------ band and z-drop edges
EDGE_SETS = [
    (1, 4, -1, 6, 1, 6, 1, 100, 5, 0),           # w = 0: one cell per row
    (1, 4, -1, 6, 1, 6, 1, 100, 5, 40000),       # w beyond every length
    (1, 4, -1, 6, 1, 6, 1, 0, 5, 100),           # zdrop = 0: no z-drop exit
    (1, 4, -1, 6, 1, 6, 1, 1, 5, 100),           # zdrop = 1
    (1, 4, -1, 6, 1, 9, 1, 1, 5, 3),             # o_ins != o_del with a narrow band and zdrop = 1
    (1, 4, -1, 6, 1, 6, 1, 100, -1000, 100),     # end_bonus so negative that the band clamp leaves w = 1
]


@pytest.mark.parametrize("cells", ["byte", "word"])
@pytest.mark.parametrize("ps", EDGE_SETS, ids=["_".join(map(str, p)) for p in EDGE_SETS])
def test_band_and_zdrop_edges(monkeypatch, capfd, ps, cells):
    if cells == "byte":
        batch = bounded_batch(77, 151, 255 - 160)
    else:
        batch = gabgen.bsw(78, 4000, 1)
    ran, _ = run_both(ps, batch, monkeypatch, capfd)
    assert [k for *_, k in ran] == (["dp8<1,1>"] if cells == "byte" and ps[5] + ps[6] == 7 else
                                    ["dp8<0,1>"] if cells == "byte" else ["dp16"]), ran


@pytest.mark.parametrize("ps", [DEFAULTS, (1, 4, -1, 6, 1, 6, 1, 0, 30000, 40000), (2, 3, -2, 5, 2, 7, 1, 0, 30000, 40000)],
                         ids=["defaults", "zdrop0_wide_band", "zdrop0_wide_band_asym"])
def test_longest_reference_one_base_query(monkeypatch, capfd, ps):
    """tlen up to GAB_BSW_MAX_TLEN with qlen = 1.  At the defaults the band clamp (bandedSWA.cpp:164-172) leaves w = 1 and every
    pair ends after two rows; with a large end_bonus and w the band keeps column 0 and the row loop runs until h0 has bled away
    along it -- a few hundred rows with a byte-sized h0, the whole reference with h0 near the 16-bit limit or above"""
    rng = np.random.default_rng(9)
    a = ps[0]
    for h0, want_kernel in ((255 - 16 * a, None), (32767 - 16 * a, "dp16"), (1 << 20, "dp32")):
        refs = [rng.integers(0, 5, 32767).astype(np.uint8) for _ in range(6)] + [rng.integers(0, 4, int(L)).astype(np.uint8)
                                                                                for L in (1, 2, 31, 32766)]
        qrys = [np.array([k % 5], np.uint8) for k in range(len(refs))]
        batch = gabgen.bsw_from_arrays(refs, qrys, [h0 - 7 * k for k in range(len(refs) - 1)] + [h0])
        ran, _ = run_both(ps, batch, monkeypatch, capfd)
        assert [k for *_, k in ran] == [want_kernel or kernel(8, *sym_ms1(ps))], ran
        if h0 > 255 and ps[8] > 1000:      # (the rows really ran that far down the references)
            assert pyoracle.bsw(batch, bsw_oracle_params(*ps), want_cells=True)[1] > 100000


# ------------------------------------------------------------------------------------------------ per-class launches
@pytest.mark.parametrize("n,ps", [(64 * 8192 + 1, DEFAULTS), (700000, (1, 4, -1, 6, 1, 7, 1, 100, 5, 100)),
                                  (600000, (2, 3, -2, 5, 2, 5, 2, 50, 30, 30))], ids=["524289-defaults", "700000-asym", "600000-a2"])
def test_per_class_launches_mix_kernels(monkeypatch, capfd, n, ps):
    """more than 64 * 8192 pairs go out as one launch per query-length class, each with the cell width its own pairs need: short
    queries with small h0 take the byte kernel, the middle classes the 16-bit one, the longest class (a few h0 beyond the 16-bit
    range) the 32-bit one -- three kernels in one call"""
    a = ps[0]
    b = gabgen.bsw(4242 + n % 1000, n, 1)
    cls = (b.len2 - 1) // 16
    rng = np.random.default_rng(n)
    h0 = b.h0.copy()
    short = cls == 0
    h0[short] = rng.integers(0, 255 - 16 * a + 1, int(short.sum()))              # byte cells for class 0
    top = np.flatnonzero(cls == 15)
    h0[top[::16]] = 40000                                                        # 32-bit cells for class 15
    b = subset(b, np.arange(n), h0)
    ran, _ = run_both(ps, b, monkeypatch, capfd)
    kinds = {k for *_, k in ran}
    assert len(ran) == 16 and len(kinds) >= 3, ran
    assert {c for c, _, _, k in ran if k.startswith("dp8")} == {0}
    assert {c for c, _, _, k in ran if k == "dp32"} == {15}
    assert kernel(8, *sym_ms1(ps)) in kinds and "dp16" in kinds
