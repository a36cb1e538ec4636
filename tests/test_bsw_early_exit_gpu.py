"""GPU: the score-only early exit of the six bsw DP kernels against the oracle and the CPU model of the rule.

A score-only call (result_out NULL: gab_bsw_run, getScores16, run_device(..., score, None)) stops a pair's row loop once no later
row can raise its score (bsw.hip's header comment).  Scores go against the oracle, no tolerance.  last_stats()["cells"] of a
score-only call must equal the pruned cell count of tools/gen/bsw_exit_model.c, which pins every kernel to the one specified
rule; with result_out given nothing changes and the counter is the oracle's.  The kernel each case targets is read off the
GAB_BSW_TRACE lines, as in tests/test_bsw_kernels_gpu.py."""
import re

import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_oracle_params

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"\[gab_bsw_dp \S+\] class (\d+) qcap (\d+) pairs (\d+) bits (\d+) sym (\d) ms1 (\d)")
DEFAULTS = BSW_PARAM_SETS[0]


def kernels_run(err):
    return [f"dp8<{s},{m}>" if bits == "8" else f"dp{bits}" for _, _, _, bits, s, m in TRACE.findall(err)]


def run(ps, batch, monkeypatch, capfd, full=False):
    """batch through run_device on a fresh handle: score-only, then (full) the six-field call on the SAME handle.
    -> (scores, cells, kernels) of the score-only call [, (result, cells) of the six-field call]"""
    import torch
    from genarchbench_amd.bsw import BandedPairWiseSW, bwa_fill_scmat
    a, b, amb, od, ed, oi, ei, zd, eb, w = ps
    monkeypatch.setenv("GAB_BSW_TRACE", "1")
    sw = BandedPairWiseSW(od, ed, oi, ei, zd, eb, bwa_fill_scmat(a, b, amb), w)
    try:
        dev = torch.device("cuda:0")
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        args = (t(batch.ref), t(batch.ref_off), t(batch.qry), t(batch.qry_off), t(batch.len1), t(batch.len2), t(batch.h0))
        stream = torch.cuda.current_stream().cuda_stream
        score = torch.full((batch.n,), -7, dtype=torch.int32, device=dev)
        capfd.readouterr()
        sw.run_device(*args, score, None, stream=stream)
        torch.cuda.synchronize()
        out = (score.cpu().numpy(), sw.last_stats()["cells"], kernels_run(capfd.readouterr().err))
        if full:
            score2 = torch.full((batch.n,), -7, dtype=torch.int32, device=dev)
            res = torch.full((batch.n, 6), -7, dtype=torch.int32, device=dev)
            sw.run_device(*args, score2, res, stream=stream)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(score2.cpu().numpy(), out[0])
            out += (res.cpu().numpy(), sw.last_stats()["cells"])
        # the host-pointer entry point is score-only too
        np.testing.assert_array_equal(sw.getScores16(batch), out[0])
        assert sw.last_stats()["cells"] == out[1]
    finally:
        sw.close()
    return out


def check(ps, batch, monkeypatch, capfd, want_kernel=None, full=False):
    """scores == oracle, score-only cells == model; -> (oracle cells, model's per-pair rows, score-only cells)"""
    p = bsw_oracle_params(*ps)
    want, ocells = pyoracle.bsw(batch, p, want_cells=True)
    mscore, mrows, mcells, _ = gabgen.bsw_exit_model(batch, p)
    np.testing.assert_array_equal(mscore, want[:, 0])
    got = run(ps, batch, monkeypatch, capfd, full)
    bad = np.flatnonzero(got[0] != want[:, 0])
    assert len(bad) == 0, (f"{len(bad)} of {batch.n} scores differ ({got[2]}); first: pair {bad[0]} qlen {batch.len2[bad[0]]} tlen "
                           f"{batch.len1[bad[0]]} h0 {batch.h0[bad[0]]}: got {got[0][bad[0]]} want {want[bad[0], 0]}")
    print(f"{got[2]} cells: oracle {ocells} model {int(mcells.sum())} gpu {got[1]}")
    assert got[1] == int(mcells.sum()), (got[1], int(mcells.sum()), ocells, got[2])
    if want_kernel:
        assert got[2] == [want_kernel], got[2]
    if full:
        np.testing.assert_array_equal(got[3], want)
        assert got[4] == ocells
    return ocells, mrows, got[1]


def generator_batch(seed, mode, qmax, h0_of, n=4096):
    """the first n pairs of generator mode `mode` with query length <= qmax, h0 replaced by h0_of(rng, n) when given"""
    b = gabgen.bsw(seed, 8 * n, mode)
    idx = np.flatnonzero(b.len2 <= qmax)[:n]
    assert len(idx) == n
    h0 = b.h0[idx].copy() if h0_of is None else np.asarray(h0_of(np.random.default_rng(seed), n), np.int32)
    return gabgen.BswBatch(b.ref, b.ref_off[idx].copy(), b.qry, b.qry_off[idx].copy(), b.len1[idx].copy(), b.len2[idx].copy(), h0)


def byte_h0(hmax):
    def f(rng, n):
        h = rng.integers(0, hmax + 1, n)
        h[n // 3] = hmax
        return h
    return f


def lifted_h0(base, every, add):
    """generator-like h0 with every `every`-th pair lifted by `add`: forces the 16-bit (add = 1000) or 32-bit (40000) kernel"""
    def f(rng, n):
        h = rng.integers(0, base + 1, n)
        h[::every] += add
        return h
    return f


# (kernel, parameters, qmax, h0): the byte kernels take h0 up to 255 - qcap * max_sc
KERNEL_CASES = [
    ("dp8<1,1>", DEFAULTS, 151, byte_h0(255 - 160)),
    ("dp8<1,0>", (2, 3, -2, 5, 2, 5, 2, 50, 30, 30), 112, byte_h0(255 - 224)),
    ("dp8<0,1>", (1, 4, -1, 6, 1, 7, 1, 100, 5, 100), 151, byte_h0(255 - 160)),
    ("dp8<0,0>", (4, 1, -1, 2, 1, 9, 2, 10, 0, 100), 48, byte_h0(255 - 192)),
    ("dp16", DEFAULTS, 256, lifted_h0(100, 97, 1000)),
    ("dp32", DEFAULTS, 256, lifted_h0(100, 5, 40000)),
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("want_kernel,ps,qmax,h0_of", KERNEL_CASES, ids=[k for k, *_ in KERNEL_CASES])
def test_every_kernel(monkeypatch, capfd, want_kernel, ps, qmax, h0_of, mode):
    batch = generator_batch(100 + mode, mode, qmax, h0_of)
    ocells, _, cells = check(ps, batch, monkeypatch, capfd, want_kernel, full=(mode == 1))
    if mode == 0 and ps[9] == 100:          # read-like pairs, wide band: the exit must really fire in this kernel
        assert cells < 0.9 * ocells


# ------------------------------------------------------------------------------------------------ hand-made batches
def rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def test_dip_then_new_best(monkeypatch, capfd):
    """query = A + B (50 + 50), reference = A + 10 unrelated bases + B: the score dips in the gap and B sets a new best, so the
    exit must not fire between the two"""
    rng = np.random.default_rng(1)
    refs, qrys = [], []
    for k in range(64):
        A, B = rnd(rng, 50), rnd(rng, 50)
        refs.append(np.concatenate([A, rnd(rng, 10), B, rnd(rng, 5 * (k % 8))])); qrys.append(np.concatenate([A, B]))
    batch = gabgen.bsw_from_arrays(refs, qrys, [30] * 64)
    _, mrows, _ = check(DEFAULTS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)
    want = pyoracle.bsw(batch)
    assert (want[:, 0] > 30 + 50).all() and (want[:, 2] > 60).all()          # B really extended the best (tle lies behind the gap)
    assert (mrows >= want[:, 2]).all()


def test_long_random_tail(monkeypatch, capfd):
    """reference ten times the query with a random tail: cells well under the full-result run's, same score"""
    rng = np.random.default_rng(2)
    qrys = [rnd(rng, 100) for _ in range(64)]
    refs = [np.concatenate([q, rnd(rng, 900)]) for q in qrys]
    batch = gabgen.bsw_from_arrays(refs, qrys, [40] * 64)
    ocells, _, cells = check(DEFAULTS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)
    assert cells < 0.75 * ocells


def test_band_clamp_cuts_live_row_minus_one_cells(monkeypatch, capfd):
    """w = 5 with h0 = 100: row -1 is non-zero far beyond the band, and the clamp cuts those live cells in every early row"""
    rng = np.random.default_rng(3)
    qrys = [rnd(rng, int(L)) for L in rng.integers(30, 140, 128)]
    refs = [np.concatenate([q[:len(q) // 2], rnd(rng, 3), q[len(q) // 2:], rnd(rng, 60)]) for q in qrys]
    batch = gabgen.bsw_from_arrays(refs, qrys, [100] * 128)
    check(DEFAULTS[:9] + (5,), batch, monkeypatch, capfd, "dp8<1,1>", full=True)
    batch.h0[::3] = 1000
    check(DEFAULTS[:9] + (5,), batch, monkeypatch, capfd, "dp16")


def test_smallest_pair(monkeypatch, capfd):
    """h0 = 0, qlen = 1, tlen = 1"""
    one = [np.array([2], np.uint8)]
    check(DEFAULTS, gabgen.bsw_from_arrays(one, one, [0]), monkeypatch, capfd, "dp8<1,1>", full=True)
    check(DEFAULTS, gabgen.bsw_from_arrays(one * 3, one * 3, [0, 1, 7]), monkeypatch, capfd, "dp8<1,1>", full=True)


@pytest.mark.parametrize("ps,want_kernel", [((3, 5, -1, 7, 3, 4, 1, 200, 5, 100), "dp8<0,0>"), ((2, 4, 2, 9, 1, 3, 2, 100, 5, 40), "dp8<0,0>"),
                                            ((5, 9, -3, 11, 2, 3, 4, 30, -20, 17), "dp16")], ids=["3_5", "2_4_n2", "5_9"])
def test_max_sc_above_one_with_asymmetric_gaps(monkeypatch, capfd, ps, want_kernel):
    qmax = 48 if want_kernel.startswith("dp8") else 256
    h0_of = byte_h0(255 - 48 * max(ps[0], ps[2])) if want_kernel.startswith("dp8") else None
    for mode in (0, 1):
        check(ps, generator_batch(200 + mode, mode, qmax, h0_of, n=2048), monkeypatch, capfd, want_kernel, full=(mode == 0))


def test_one_lane_runs_to_its_last_row(monkeypatch, capfd):
    """one wave (64 pairs are one workgroup): 63 lanes whose 40-base query is followed by 200 random reference bases -- they exit
    soon after the query ends -- and one lane whose 240-base query matches its reference to the last row, so every row raises its
    score and it cannot exit"""
    rng = np.random.default_rng(4)
    qrys = [rnd(rng, 40) for _ in range(64)]
    refs = [np.concatenate([q, rnd(rng, 200)]) for q in qrys]
    qrys[17] = rnd(rng, 240)
    refs[17] = qrys[17].copy()
    batch = gabgen.bsw_from_arrays(refs, qrys, [10] * 64)
    _, mrows, _ = check(DEFAULTS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)
    assert mrows[17] == 240 and (np.delete(mrows, 17) < 120).all()


def test_score_only_and_six_fields_on_one_handle(monkeypatch, capfd):
    """one batch through the score-only and the six-field call of the same handle: identical scores, the six-field counter is
    the oracle's (check(..., full=True) asserts both) and the score-only one is smaller"""
    batch = gabgen.bsw(300, 4096, 0)
    ocells, _, cells = check(DEFAULTS, batch, monkeypatch, capfd, "dp8<1,1>", full=True)
    assert cells < ocells
