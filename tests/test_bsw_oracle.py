"""CPU: the bsw oracle (oracle/bsw.c) against the golden vectors produced by the compiled reference,
and against the compiled reference run live as well when oracle/_ref is present."""
import subprocess
import warnings

import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import (BSW_PARAM_SETS, GOLDEN, bsw_full_ref_params_line, bsw_oracle_params, bsw_param_input, live,
                        read_bsw_full, read_bsw_input, read_scores)


@pytest.mark.parametrize("name", ["bsw_bench", "bsw_adv"])
def test_oracle_matches_golden(name):
    batch = read_bsw_input(f"{GOLDEN}/{name}.in.txt")
    want = read_scores(f"{GOLDEN}/{name}.expected.txt")
    got = pyoracle.bsw(batch)[:, 0]
    assert batch.n == len(want)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", ["bsw_bench", "bsw_adv"])
def test_oracle_full_result_matches_golden(name):
    """all six fields (score, qle, tle, gtle, gscore, max_off) against the reference's scalarBandedSWAWrapper ==
    getScores16 output (bsw/src/bandedSWA.cpp:241-252,258-276)"""
    batch = read_bsw_input(f"{GOLDEN}/{name}.in.txt")
    want = read_bsw_full(f"{GOLDEN}/{name}.full.expected.txt")
    assert want.shape == (batch.n, 6)
    np.testing.assert_array_equal(pyoracle.bsw(batch), want)
    np.testing.assert_array_equal(want[:, 0], read_scores(f"{GOLDEN}/{name}.expected.txt"))


@pytest.mark.parametrize("how", ["scalar", "vector"])
def test_oracle_full_result_matches_live_reference(tmp_path, how):
    """fresh seed, adversarial mode: six fields against the reference's class -- its output as recorded in tests/golden
    (make_golden.py live: scalar and vector identical), and the class itself run live where oracle/_ref is built"""
    n, seed = 4096, 993
    want = live("bsw_full")
    if pyoracle.ref_path("bsw_full_ref_avx2"):
        p = str(tmp_path / "in.txt")
        gabgen.write_text("bsw", p, seed, n, 1)
        r = subprocess.run([pyoracle.ref_path("bsw_full_ref_avx2"), p, how], capture_output=True, text=True, check=True)
        np.testing.assert_array_equal(np.array([[int(v) for v in l.split()[1:]] for l in r.stdout.splitlines()], np.int32), want)
    assert want.shape == (n, 6)
    np.testing.assert_array_equal(pyoracle.bsw(gabgen.bsw(seed, n, 1)), want)


@pytest.mark.parametrize("name,seed,n,mode", [("bsw_bench", 101, 2048, 0), ("bsw_adv", 102, 1536, 1)])
def test_generator_reproduces_golden_input(name, seed, n, mode):
    """the in-memory generator and the committed text fixture are the same data"""
    a = read_bsw_input(f"{GOLDEN}/{name}.in.txt")
    b = gabgen.bsw(seed, n, mode)
    np.testing.assert_array_equal(a.len1, b.len1)
    np.testing.assert_array_equal(a.len2, b.len2)
    np.testing.assert_array_equal(a.h0, b.h0)
    np.testing.assert_array_equal(a.ref[:a.ref_off[-1] + a.len1[-1]], b.ref[:b.ref_off[-1] + b.len1[-1]])
    np.testing.assert_array_equal(a.qry[:a.qry_off[-1] + a.len2[-1]], b.qry[:b.qry_off[-1] + b.len2[-1]])


def test_oracle_thread_invariant():
    b = gabgen.bsw(5, 4000, 1)
    np.testing.assert_array_equal(pyoracle.bsw(b, threads=1), pyoracle.bsw(b, threads=3))


def test_oracle_edge_cases():
    """hand-made pairs: 1-base sequences, all-N, no similarity, h0=0 (row max 0 -> immediate exit)"""
    A = lambda *x: np.array(x, np.uint8)
    refs = [A(0), A(1), A(4, 4, 4, 4), A(0, 1, 2, 3) , A(0, 0, 0, 0, 0, 0, 0, 0), A(0, 1, 2, 3)]
    qrys = [A(0), A(0), A(4, 4, 4, 4), A(0, 1, 2, 3), A(3, 3, 3, 3), A(0, 1, 2, 3)]
    h0 = [10, 10, 50, 0, 3, 1]
    out = pyoracle.bsw(gabgen.bsw_from_arrays(refs, qrys, h0))
    # scores: match extends h0 by 1; mismatch leaves the seed score; h0=0 can never extend
    assert out[0, 0] == 11 and out[1, 0] == 10 and out[2, 0] == 50 and out[3, 0] == 0
    assert out[4, 0] == 3 and out[5, 0] == 5


def test_oracle_matches_live_reference(tmp_path):
    """fresh seed, adversarial mode, against the compiled reference: its output as recorded in tests/golden (make_golden.py
    live), and the reference itself run live where oracle/_ref is built"""
    n, seed = 4096, 991
    want = live("bsw_scores")
    if pyoracle.ref_path("bsw_ref_avx2"):
        p = str(tmp_path / "in.txt")
        gabgen.write_text("bsw", p, seed, n, 1)
        r = subprocess.run([pyoracle.ref_path("bsw_ref_avx2"), "-pairs", p, "-t", "2", "-b", "256"],
                           capture_output=True, text=True, check=True)
        np.testing.assert_array_equal(np.array([int(l.split("=")[1]) for l in r.stderr.splitlines() if "score=" in l][:n], np.int32), want)
    assert len(want) == n
    got = pyoracle.bsw(gabgen.bsw(seed, n, 1))[:, 0]
    np.testing.assert_array_equal(got, want)


@pytest.fixture(scope="module")
def param_golden():
    with np.load(f"{GOLDEN}/bsw_params.npz") as z:
        return z["sets"], z["full"]


@pytest.mark.parametrize("k", range(len(BSW_PARAM_SETS)), ids=["-".join(map(str, s)) for s in BSW_PARAM_SETS])
def test_oracle_full_result_matches_reference_at_other_parameters(tmp_path, param_golden, k):
    """off the driver's defaults (a b ambig o_del e_del o_ins e_ins zdrop end_bonus w): six fields against the reference's
    scalarBandedSWA -- its output as recorded in tests/golden (make_golden.py params), and the harness run live where oracle/_ref
    is built.  (The reference's vector getScores16 is not the truth here: it differs from its own scalar path at most of these
    sets, MANIFEST.json bsw_params.)"""
    sets, full = param_golden
    ps = BSW_PARAM_SETS[k]
    assert tuple(int(v) for v in sets[k]) == ps, "BSW_PARAM_SETS no longer matches bsw_params.npz"
    batch = bsw_param_input()
    want = full[k]
    assert want.shape == (batch.n, 6)
    np.testing.assert_array_equal(pyoracle.bsw(batch, bsw_oracle_params(*ps)), want)
    if pyoracle.ref_path("bsw_full_ref_avx2"):
        p = str(tmp_path / "in.txt")
        batch.write_text(p)
        r = subprocess.run([pyoracle.ref_path("bsw_full_ref_avx2"), p, "scalar"] + [str(v) for v in ps],
                           capture_output=True, text=True, check=True)
        if bsw_full_ref_params_line(*ps) not in r.stderr:
            # a binary of oracle/_ref built from the harness before it took parameters (the reference is needed to build it
            # again): it computes the driver's defaults whatever it is given, so it says nothing about this set
            warnings.warn("oracle/_ref/bsw_full_ref_avx2 predates the harness's parameters: live comparison not run "
                          "(make -C oracle ref where the reference is present)")
            return
        np.testing.assert_array_equal(np.array([[int(v) for v in l.split()[1:]] for l in r.stdout.splitlines()], np.int32), want)
        if k == 0:      # the driver's defaults: the same output as the harness without the ten numbers
            assert subprocess.run([pyoracle.ref_path("bsw_full_ref_avx2"), p, "scalar"], capture_output=True, text=True,
                                  check=True).stdout == r.stdout


def test_param_golden_covers_the_edges(param_golden):
    """the recorded sets reach the corners of the parameter space the kernels specialise on"""
    sets, _ = param_golden
    a, b, amb, od, ed, oi, ei, zd, eb, w = sets.T
    assert len(sets) == len(BSW_PARAM_SETS) >= 12
    assert (np.maximum(a, 0) == 0).any() and (a == 127).any() and (b == 128).any()
    assert (od == 0).any() and (zd == 0).any() and (zd == 1).any() and (w == 0).any() and (w >= 2000).any()
    assert (eb < 0).any() and (eb >= 1000).any() and (od + ed != oi + ei).any() and (od != oi).any()
    batch = bsw_param_input()
    hasn = lambda s, o, l: [(s[o[i]:o[i] + l[i]] == 4).any() for i in range(batch.n)]
    assert np.logical_and(hasn(batch.ref, batch.ref_off, batch.len1), hasn(batch.qry, batch.qry_off, batch.len2)).any()

