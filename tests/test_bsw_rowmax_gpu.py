"""GPU: the row maximum of the 8-bit bsw kernel (one key per loop trip, the column resolved after the row) on a batch built to tie.

bsw_dp8 folds one key per four columns into the row's running maximum and reads the column back from the stored row afterwards
(bsw.hip; tools/gen/bsw_rowmax_model.c is the CPU model and tests/test_bsw_rowmax.py checks the rule and this batch on the CPU).  A
wrong column shows in qle, in max_off and -- through the z-drop test, which uses rowmax_j - best_j -- in every field, so the six-field
result, the score-only result and getScores16 all go against the oracle with no tolerance, at the defaults, at zdrop 5 and 10, with
asymmetric gaps (SYM false) and with a match score of 2 (MS1 false).  The score-only cell counter must be the early-exit model's, as
in tests/test_bsw_early_exit_gpu.py.  Which kernel ran is read off the GAB_BSW_TRACE lines.

A match score of 2 fits 8-bit cells only up to 127 query bases less h0 / 2, so those two sets run the pairs of the batch whose query
has at most 64 bases (every pair built to tie, the short queries and the hand-made pairs that fit)."""
import re

import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.bsw_rowmax_cases import GPU_PARAM_SETS, gpu_batch
from tests.util import bsw_oracle_params

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"\[gab_bsw_dp \S+\] class (\d+) qcap (\d+) pairs (\d+) bits (\d+) sym (\d) ms1 (\d)")


def kernels_run(err):
    return [f"dp8<{s},{m}>" if bits == "8" else f"dp{bits}" for _, _, _, bits, s, m in TRACE.findall(err)]


def run_all(ps, batch, monkeypatch, capfd):
    """-> (six-field result, its scores, kernels), (score-only scores, cells, kernels), (getScores16 scores, cells, kernels)"""
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
        res = torch.full((batch.n, 6), -7, dtype=torch.int32, device=dev)
        capfd.readouterr()
        sw.run_device(*args, score, res, stream=stream)
        torch.cuda.synchronize()
        full = (res.cpu().numpy(), score.cpu().numpy(), kernels_run(capfd.readouterr().err))
        score2 = torch.full((batch.n,), -7, dtype=torch.int32, device=dev)
        sw.run_device(*args, score2, None, stream=stream)
        torch.cuda.synchronize()
        only = (score2.cpu().numpy(), sw.last_stats()["cells"], kernels_run(capfd.readouterr().err))
        host = (sw.getScores16(batch), sw.last_stats()["cells"], kernels_run(capfd.readouterr().err))
    finally:
        sw.close()
    return full, only, host


def first_bad(batch, got, want):
    bad = np.flatnonzero((got != want).reshape(batch.n, -1).any(axis=1))
    if len(bad) == 0:
        return None
    k = bad[0]
    return (f"{len(bad)} of {batch.n} pairs differ; first: pair {k} qlen {batch.len2[k]} tlen {batch.len1[k]} h0 {batch.h0[k]}: "
            f"got {got[k].tolist()} want {want[k].tolist()}")


@pytest.mark.parametrize("want_kernel,ps", GPU_PARAM_SETS, ids=[f"{k}-{'_'.join(map(str, p))}" for k, p in GPU_PARAM_SETS])
def test_tie_heavy_batch(monkeypatch, capfd, want_kernel, ps):
    batch = gpu_batch(ps)
    p = bsw_oracle_params(*ps)
    want, ocells = pyoracle.bsw(batch, p, want_cells=True)
    mscore, _, mcells, _ = gabgen.bsw_exit_model(batch, p)
    np.testing.assert_array_equal(mscore, want[:, 0])
    full, only, host = run_all(ps, batch, monkeypatch, capfd)
    print(f"{batch.n} pairs, kernels {full[2]} {only[2]} {host[2]}; cells: oracle {ocells} model {int(mcells.sum())} score-only {only[1]} "
          f"getScores16 {host[1]}")
    assert full[2] == [want_kernel] and only[2] == [want_kernel] and host[2] == [want_kernel], (full[2], only[2], host[2])
    assert first_bad(batch, full[0], want) is None, first_bad(batch, full[0], want)
    np.testing.assert_array_equal(full[1], want[:, 0])
    assert first_bad(batch, only[0], want[:, 0]) is None, first_bad(batch, only[0], want[:, 0])
    assert first_bad(batch, host[0], want[:, 0]) is None, first_bad(batch, host[0], want[:, 0])
    assert only[1] == int(mcells.sum()), (only[1], int(mcells.sum()), ocells)
    assert host[1] == int(mcells.sum()), (host[1], int(mcells.sum()), ocells)


def test_all_four_instantiations_are_covered():
    """every case above asserts that its own kernel ran; together they are the four bsw_dp8<SYM, MS1>"""
    assert {k for k, _ in GPU_PARAM_SETS} == {"dp8<1,1>", "dp8<1,0>", "dp8<0,1>", "dp8<0,0>"}
