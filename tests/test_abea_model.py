"""abea without a GPU: the model (tests/abea_model.py) reproduces what the reference's align() returned for every read of the golden
fixture (tests/golden/make_abea_golden.py recorded it), the rule for a read whose end scan finds nothing, and the argument checks
of the mirror that run before a device is needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import abea_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    z = np.load(os.path.join(GOLDEN, "abea_small.npz"))
    exp = json.load(open(os.path.join(GOLDEN, "abea_expected.json")))
    so = np.concatenate([[0], np.cumsum(z["seq_len"], dtype=np.int64)]); eo = np.concatenate([[0], np.cumsum(z["n_events"], dtype=np.int64)])
    reads = [(z["seq"][so[i]:so[i + 1]].tobytes(), z["events"][eo[i]:eo[i + 1]], z["scale"][i], z["shift"][i]) for i in range(z["seq_len"].size)]
    return (z["level_mean"], z["level_stdv"], z["level_log_stdv"]), reads, exp


def test_the_fixture_is_the_one_the_reference_ran_on():
    import hashlib
    exp = json.load(open(os.path.join(GOLDEN, "abea_expected.json")))
    assert hashlib.sha256(open(os.path.join(GOLDEN, exp["fixture"]), "rb").read()).hexdigest() == exp["fixture_sha256"]
    assert exp["reads_passing"] >= 0.9 * len(exp["reads"]) and any(r["n_pairs"] == 0 for r in exp["reads"])


def test_model_reproduces_the_reference_on_every_read_of_the_fixture():
    model, reads, exp = load_fixture()
    assert len(reads) == len(exp["reads"])
    flags = set()
    for i, (r, want) in enumerate(zip(reads, exp["reads"])):
        rec, path = M.align(*r[:2], *model, *r[2:])
        assert (rec["n_pairs"], rec["path_len"], M.pairs_digest(path)) == (want["n_pairs"], want["path_len"], want["pairs"]), f"read {i}: {rec}"
        assert not rec["flags"] & M.NO_END and (rec["n_pairs"] == 0) == bool(rec["flags"])
        flags.add(rec["flags"])
    assert 0 in flags and M.LOW_EMISSION in flags


def test_a_read_whose_end_scan_finds_nothing_returns_no_pairs():
    """events that are not numbers: every filled cell is NaN, no end cell compares greater than -inf, so the end scan finds nothing;
    the reference would backtrack from event 0 whatever its cell holds, the library's rule is NO_END and an empty record"""
    rng = np.random.default_rng(3)
    mean, stdv, lstd = M.make_model(rng)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 80).tolist())
    rec, path = M.align(seq, np.full(120, np.nan, np.float32), mean, stdv, lstd, 1.0, 0.0)
    assert rec["flags"] == M.NO_END and rec["n_pairs"] == rec["path_len"] == rec["end_event"] == rec["max_gap"] == 0
    assert rec["avg_log_emission"] == 0.0 and rec["fills"] > 0 and path.shape == (0, 2)


def test_one_event_against_sixty_kmers_is_one_run_of_skips():
    """everything in band: the path is the only row, 59 skips and the diagonal step out of the start cell"""
    rng = np.random.default_rng(4)
    mean, stdv, lstd = M.make_model(rng)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 65).tolist())
    rec, path = M.align(seq, np.array([90.0], np.float32), mean, stdv, lstd, 1.0, 0.0)
    assert rec["path_len"] == 60 and rec["max_gap"] == 59 and rec["flags"] & M.GAP and rec["n_pairs"] == 0
    assert path[:, 0].tolist() == list(range(60)) and not path[:, 1].any()


def test_bytes_outside_ACGT_rank_as_A():
    assert M.kmer_ranks(b"ACGTNacgtXT").tolist() == M.kmer_ranks(b"ACGTAAAAAAT").tolist()


def test_the_mirror_checks_its_arguments_before_it_needs_a_device():
    import genarchbench_amd as g
    from genarchbench_amd import abea
    assert g.EventAligner is abea.EventAligner
    assert abea.READ.itemsize == 40 and abea.PAIR.itemsize == 8
    lib = g.lib()
    h = C.c_void_p()
    mean = np.full(abea.NKMER, 90.0, np.float32); stdv = np.full(abea.NKMER, 2.0, np.float32)
    assert lib.gab_abea_create(C.c_int(0), None, None, None, C.byref(h)) == -22
    bad = stdv.copy(); bad[17] = 0.0
    assert lib.gab_abea_create(C.c_int(0), mean.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p), None, C.byref(h)) == -22
    assert b"17" in lib.gab_last_error()
    assert lib.gab_abea_align(None, *([None] * 8), C.c_int64(1), None, None, None) == -22
    assert lib.gab_abea_last_stats(None, None, None, None, None, None) == -22
    with pytest.raises(ValueError):
        abea.EventAligner(mean[:10], stdv[:10])
    if lib.gab_device_count() <= 0:
        with pytest.raises(g.GabError) as e:
            abea.EventAligner(mean, stdv)
        assert e.value.code == -19      # GAB_ENODEV: no quiet fall-back
