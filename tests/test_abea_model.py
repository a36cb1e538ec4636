"""abea without a GPU: the model (tests/abea_model.py) reproduces what the reference's align() returned for every read of the golden
fixture and of the case fixture (tests/golden/make_abea_golden.py recorded both), the fields align() computes but does not return
computed again from the path (tests/abea_path_checks.py), the rule for a read whose end scan finds nothing, and the argument checks
of the mirror that run before a device is needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import abea_cases as CASES
import abea_model as M
import abea_path_checks as P
from abea_cases import load_fixture  # noqa: F401  (the other abea tests import it from here)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_the_fixture_is_the_one_the_reference_ran_on():
    import hashlib
    exp = json.load(open(os.path.join(GOLDEN, "abea_expected.json")))
    assert hashlib.sha256(open(os.path.join(GOLDEN, exp["fixture"]), "rb").read()).hexdigest() == exp["fixture_sha256"]
    assert exp["reads_passing"] >= 0.9 * len(exp["reads"]) and any(r["n_pairs"] == 0 for r in exp["reads"])


_MODEL = {}


def model_of_fixture():
    """the model's (record, path) of every read of abea_small.npz, computed once per process and left unchanged"""
    if "fixture" not in _MODEL:
        model, reads, _ = load_fixture()
        _MODEL["fixture"] = [M.align(*r[:2], *model, *r[2:]) for r in reads]
    return _MODEL["fixture"]


def model_of_cases():
    """the model's (record, path) of every read of abea_cases.npz, computed once per process and left unchanged"""
    if "cases" not in _MODEL:
        model, _, reads, _ = CASES.load_cases()
        _MODEL["cases"] = [M.align(*r[:2], *model, *r[2:]) for r in reads]
    return _MODEL["cases"]


def recorded(want):
    """a read's record in abea_cases_expected.json -> the four recomputed fields as (end_event, admissible (max_gap, flags), avg)"""
    adm = [tuple(x) for x in want.get("max_gap_and_flags_admissible", [[want["max_gap"], want["flags"]]])]
    return want["end_event"], adm, np.float64(float.fromhex(want["avg_log_emission"])).tobytes()


def test_model_reproduces_the_reference_on_every_read_of_the_fixture():
    model, reads, exp = load_fixture()
    assert len(reads) == len(exp["reads"])
    flags = set()
    for i, (r, want, (rec, path)) in enumerate(zip(reads, exp["reads"], model_of_fixture())):
        assert (rec["n_pairs"], rec["path_len"], M.pairs_digest(path)) == (want["n_pairs"], want["path_len"], want["pairs"]), f"read {i}: {rec}"
        assert not rec["flags"] & M.NO_END and (rec["n_pairs"] == 0) == bool(rec["flags"])
        flags.add(rec["flags"])
    assert 0 in flags and M.LOW_EMISSION in flags


def test_the_case_fixture_is_the_one_the_reference_ran_on():
    """abea_cases.npz by its hash, and its named cases byte for byte those of abea_cases.named_cases() that the GPU tests run"""
    import hashlib
    model, names, reads, exp = CASES.load_cases()
    path = os.path.join(GOLDEN, exp["fixture"])
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == exp["fixture_sha256"] and os.path.getsize(path) < 400_000
    by = dict(zip(names, reads))
    _, mod_names, mod_reads = CASES.named_cases()
    built = {n: r for n, r in zip(mod_names, mod_reads) if not n.startswith("long_")}
    built.update(CASES.extra_cases(model))
    assert len(built) == 17 + 4 and set(built) <= set(by)
    for n, r in built.items():
        g = by[n]
        assert g[0] == bytes(r[0]) and g[1].tobytes() == np.asarray(r[1], np.float32).tobytes(), n
        assert (g[2].tobytes(), g[3].tobytes()) == (np.float32(r[2]).tobytes(), np.float32(r[3]).tobytes()), n
    assert sum(n.startswith("pool_") for n in names) == exp["pool"]["reads"] == CASES.POOL_READS


def test_model_reproduces_the_reference_on_every_defined_case():
    """n_pairs, path_len and the path of every read of abea_cases.npz as the reference's -DNDEBUG build returned them with room for
    every path; the one documented deviation (no_end_nan_events: the reference backtracks from event 0 whatever its cell holds and
    returns one pair, the library's rule is NO_END) is checked for being exactly that"""
    model, names, reads, exp = CASES.load_cases()
    assert len(exp["reads"]) == len(reads) >= 420
    defined = 0
    for name, want, (rec, path) in zip(names, exp["reads"], model_of_cases()):
        if name in exp["undefined_in_reference"]:
            assert want.get("undefined_in_reference")
            continue
        if name == exp["deviation"]["name"]:
            assert rec["flags"] == M.NO_END and rec["path_len"] == 0 and (want["n_pairs"], want["path_len"]) == (0, 1)
            continue
        assert (rec["n_pairs"], rec["path_len"], M.pairs_digest(path)) == (want["n_pairs"], want["path_len"], want["pairs"]), f"{name}: {rec}"
        defined += 1
    assert defined >= len(reads) - 1 - len(exp["undefined_in_reference"]) and exp["deviation"]["name"] in names


def test_recomputation_from_the_path_equals_the_models_record():
    """end_event, max_gap, flags and avg_log_emission computed again from the path alone (tests/abea_path_checks.py) against the
    model's record, avg_log_emission as equal doubles: on every case (there also against what the golden script recorded from the
    reference's own path) and on all 205 reads of abea_small.npz.  fills depends on the band moves and stays model-only."""
    model, names, reads, exp = CASES.load_cases()
    for name, r, want, (rec, path) in zip(names, reads, exp["reads"], model_of_cases()):
        if name in exp["undefined_in_reference"] or name == exp["deviation"]["name"]:
            continue
        chk = P.recompute(r[0], r[1], *model, r[2], r[3], path)
        assert P.agrees(rec, chk), f"{name}: {rec} != {chk}"
        assert (chk["end_event"], chk["admissible"], np.float64(chk["avg_log_emission"]).tobytes()) == recorded(want), name
    model, reads, _ = load_fixture()
    for i, (r, (rec, path)) in enumerate(zip(reads, model_of_fixture())):
        chk = P.recompute(r[0], r[1], *model, r[2], r[3], path)
        assert P.agrees(rec, chk) and len(chk["admissible"]) == 1, f"read {i}: {rec} != {chk}"


def test_the_cases_are_on_the_thresholds_they_are_named_for():
    """the conditions under which the case fixture was made, on the reference's record and the recomputation recorded beside it"""
    model, names, reads, exp = CASES.load_cases()
    by = {w["name"]: (r, w) for r, w in zip(reads, exp["reads"])}
    gap50, gap51 = by["max_gap_50"][1], by["max_gap_51"][1]
    assert (gap50["max_gap"], gap50["flags"]) == (50, 0) and gap50["n_pairs"] == gap50["path_len"] > 0
    assert (gap51["max_gap"], gap51["flags"]) == (51, M.GAP) and gap51["n_pairs"] == 0
    assert not any("max_gap_and_flags_admissible" in w for w in (gap50, gap51))
    for n in CASES.PATH_LENGTHS:
        assert by[f"path_len_{n}"][1]["path_len"] == by[f"path_len_{n}"][1]["n_pairs"] == n
    slack = lambda n: len(by[n][0][0]) - M.K + 1 + by[n][0][1].size - by[n][1]["path_len"]
    assert slack("room_one_short") == 1 and slack("room_tightest") == exp["room_tightest"] >= 1
    (a, wa), (b, wb) = by["emission_above"], by["emission_below"]
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and np.nextafter(a[3], np.float32(np.inf)) == b[3]
    assert float.fromhex(wa["avg_log_emission"]) >= -5.0 > float.fromhex(wb["avg_log_emission"])
    assert (wa["avg_log_emission"], wb["avg_log_emission"]) == (exp["emission_bracket"]["above"], exp["emission_bracket"]["below"])
    assert (wa["flags"], wb["flags"]) == (0, M.LOW_EMISSION) and wa["n_pairs"] == wa["path_len"] and wb["n_pairs"] == 0
    assert by["two_kmers_one_event"][0][1].size == 1 and np.isinf(by["inf_event"][0][1]).sum() == 1 and by["scale_0"][0][2] == 0.0
    assert by["forty_events_per_kmer"][0][1].size == 280 and len(by["forty_events_per_kmer"][0][0]) == 12
    for n in ("half_an_event_per_kmer", "one_event_300_bases", "gap_one_event_60_kmers"):
        assert by[n][1]["needs_room"] and by[n][1]["path_len"] > 2 * by[n][0][1].size      # the reference's own caller could not hold this path
    pool = [(r, w) for n, (r, w) in by.items() if n.startswith("pool_")]
    assert sum(1 for r, _ in pool if r[1].size < len(r[0]) - M.K + 1) >= 50 and all(6 <= len(r[0]) <= 140 for r, _ in pool)
    for f in (0, M.LOW_EMISSION, M.LOW_EMISSION | M.GAP):
        assert sum(1 for _, w in pool if w["flags"] == f) >= 10, f
    assert sum(1 for _, w in pool if w["n_pairs"] > 0) == sum(1 for _, w in pool if w["flags"] == 0)
    # NOT_SPANNED: the seeded search found no read with it; only the reference's one-pair answer to the deviation read is not spanned
    assert exp["not_spanned"] == f"none in {CASES.NOT_SPANNED_CANDIDATES} candidates"
    assert [n for n, (_, w) in by.items() if w.get("flags", 0) & M.NOT_SPANNED] == [exp["deviation"]["name"]]


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
