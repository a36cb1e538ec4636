"""abea's event detection and scaling estimate without a GPU: the model (tests/abea_events_model.py) reproduces what the reference's
getevents and estimate_scalings_using_mom returned for every read of the golden fixture (tests/golden/make_abea_events_golden.py
recorded it); the proof that a read's sums are exact in any order; the rules for short reads and reads without a peak; the
argument checks of the library that run before a device is needed."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import abea_events_cases as CASES
import abea_events_model as M
from abea_events_cases import load_events_fixture  # noqa: F401  (the other abea tests import it from here)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32


_MODEL_EVENTS = {}


def model_events_of_fixture():
    """the model's event table of every fixture read, computed once per process"""
    if "ev" not in _MODEL_EVENTS:
        _, reads, _ = load_events_fixture()
        _MODEL_EVENTS["ev"] = [M.events_of(r[0].astype(F), r[1], r[2], r[3]) for r in reads]
    return _MODEL_EVENTS["ev"]


def model_events_of_case_fixture():
    """the model's event table of every signal of abea_events_cases.npz, computed once per process"""
    if "cases" not in _MODEL_EVENTS:
        _, signals, _, _ = CASES.load_cases()
        _MODEL_EVENTS["cases"] = [M.events_of(*s[:4]) for s in signals]
    return _MODEL_EVENTS["cases"]


def pore_models(level_mean):
    return {"level_mean": level_mean, **CASES.route_models(level_mean)}


def test_the_case_fixture_is_the_one_the_reference_ran_on():
    """abea_events_cases.npz by its hash, and its reads byte for byte those that abea_events_cases.py builds for the GPU tests"""
    level_mean, signals, given, exp = CASES.load_cases()
    path = os.path.join(GOLDEN, exp["fixture"])
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == exp["fixture_sha256"] and os.path.getsize(path) < 500_000
    names, built, seqs = CASES.reference_signals(level_mean)
    assert [r["name"] for r in exp["reads"]][:len(names)] == names and exp["signals"] == len(signals) == len(names)
    for n, s, q, g in zip(names, built, seqs, signals):
        assert g[0].tobytes() == np.asarray(s[0], F).tobytes() and g[4] == q, n
        assert [F(x).tobytes() for x in g[1:4]] == [F(x).tobytes() for x in s[1:4]], n
    edge, route = CASES.scalings_edge_cases()[0], CASES.scalings_route_cases()
    assert [r["name"] for r in exp["reads"]][len(names):len(names) + len(edge)] == list(CASES.EDGE_NAMES)
    for (q, e), g in zip(edge + route + route, given):
        assert g[0] == q and g[1].tobytes() == e.tobytes()
    # what the reference was not given (below 1000 samples) or refused (the flat read: its discarded trim step finds no start)
    assert set(CASES.not_run_in_reference(level_mean)) | {"flat_1500"} == set(exp["undefined_in_reference"])
    assert exp["undefined_in_reference"]["flat_1500"] == "rt.end > rt.start"
    for n in [f"chunk_{k}" for k in (1023, 1024, 1025, 2112)] + ["flat_run", "samples_1000", "samples_1001", "square_wave_14", "square_wave_6"] + \
            [f"planted_{v}" for v in (1e-30, 3e30, np.nan, np.inf)]:
        assert n in names and n not in exp["undefined_in_reference"], n


def test_model_reproduces_the_reference_on_every_defined_case():
    """the four event arrays and n_events of every signal the reference accepted, and scale / shift of every read under its pore model
    (the scaling edge cases and the two extra pore models included), bit for bit"""
    level_mean, signals, given, exp = CASES.load_cases()
    models = pore_models(level_mean)
    events = model_events_of_case_fixture()
    reads = [(s[4], ev["mean"]) for s, ev in zip(signals, events)] + given
    assert len(reads) == len(exp["reads"])
    defined = 0
    for i, ((seq, means), want) in enumerate(zip(reads, exp["reads"])):
        if want["name"] in exp["undefined_in_reference"]:
            assert want.get("undefined_in_reference")
            continue
        if i < len(signals):
            assert (events[i]["mean"].size, M.events_digest(events[i])) == (want["n_events"], want["events"]), want["name"]
        scale, shift = M.scalings(seq, means, models[want["pore_model"]])
        assert (float(scale).hex(), float(shift).hex()) == (want["scale"], want["shift"]), want["name"]
        defined += 1
    assert defined == len(reads) - 1


def test_the_fixture_is_the_one_the_reference_ran_on():
    exp = json.load(open(os.path.join(GOLDEN, "abea_events_expected.json")))
    assert hashlib.sha256(open(os.path.join(GOLDEN, exp["fixture"]), "rb").read()).hexdigest() == exp["fixture_sha256"]
    assert os.path.getsize(os.path.join(GOLDEN, exp["fixture"])) < 500_000 and len(exp["reads"]) >= 60


def test_model_reproduces_the_reference_on_every_read_of_the_fixture():
    level_mean, reads, exp = load_events_fixture()
    assert len(reads) == len(exp["reads"])
    for i, (r, ev, want) in enumerate(zip(reads, model_events_of_fixture(), exp["reads"])):
        assert ev["mean"].size == want["n_events"] and M.events_digest(ev) == want["events"], f"read {i}"
        scale, shift = M.scalings(r[4], ev["mean"], level_mean)
        assert (float(scale).hex(), float(shift).hex()) == (want["scale"], want["shift"]), f"read {i}"
    assert exp["events"] == sum(e["mean"].size for e in model_events_of_fixture())


def test_the_sums_of_every_fixture_read_are_exact_in_any_order():
    _, reads, _ = load_events_fixture()
    for r in reads:
        pa = M.to_pa(r[0].astype(F), r[1], r[2], r[3])
        assert M.sums_are_wide(pa)
        s, q = M.prefix_sums(pa)
        assert M.pairwise_sum(pa.astype(np.float64)) == s[-1] and M.pairwise_sum((pa * pa).astype(np.float64)) == q[-1]


@pytest.mark.parametrize("value", [1e-30, 3e30, np.nan, np.inf, 1e-41])
def test_the_proof_refuses_a_read_with_a_tiny_a_huge_or_no_number(value):
    """with one such sample the two orders may give different sums (printed), so the read must be added in the reference's order"""
    _, reads, _ = load_events_fixture()
    pa, *_ = M.with_planted(*reads[0][:4], 700, value)
    s, q = M.prefix_sums(pa)
    with np.errstate(all="ignore"):
        print(value, M.pairwise_sum(pa.astype(np.float64)) == s[-1], M.pairwise_sum((pa * pa).astype(np.float64)) == q[-1])
    assert not M.sums_are_wide(pa)
    assert M.sums_are_wide(np.delete(pa, 700))


def test_the_proof_is_tight_at_53_bits():
    """two addends (n < 2^2) on the grid 2^0: the bound on their sum, 2^(2 + emax + 1), may reach 2^53 and no more"""
    assert M.order_free(np.array([1.0, 2.0 ** 50], F))               # 2 + 50 + 1 <= 0 + 53
    assert not M.order_free(np.array([1.0, 2.0 ** 51], F))
    assert M.order_free(np.zeros(5, F)) and not M.order_free(np.array([0.0, np.inf], F))


def test_which_sums_of_the_scaling_estimate_are_order_free():
    """event means and levels of a few hundred arbitrary floats fit 53 bits with room to spare; the levels' squares, 48-bit numbers
    each, do not"""
    level_mean, reads, _ = load_events_fixture()
    for r, ev in zip(reads, model_events_of_fixture()):
        assert M.scalings_in_order(r[4], ev["mean"], level_mean) == (False, False, True)
    coarse = (np.round(level_mean * 4) / 4).astype(F)
    assert M.scalings_in_order(reads[0][4], model_events_of_fixture()[0]["mean"], coarse) == (False, False, False)
    lv = coarse[M.A.kmer_ranks(reads[0][4])].astype(np.float64)
    assert M.pairwise_sum(lv * lv) == np.add.accumulate(lv * lv)[-1]


def test_accumulate_adds_in_index_order():
    _, reads, _ = load_events_fixture()
    pa = M.to_pa(reads[1][0].astype(F), *reads[1][1:4])
    pa[10] = F(3e30); pa[500] = F(1e-30)                             # a read in which the order matters
    a, b = M.prefix_sums(pa), M.prefix_sums_by_loop(pa)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_short_reads_and_a_read_without_a_peak():
    level_mean, _, _ = load_events_fixture()
    rng = np.random.default_rng(5)
    for n in (1, 2, 5, 6, 11, 12, 13, 24):
        codes, rg, dg, of, _ = M.make_signal(rng, n, level_mean)
        ev = M.events_of(codes.astype(F), rg, dg, of)
        t1, t2 = ev["tstat"]
        if n < 6:
            assert not t1.any()
        if n < 12:
            assert not t2.any()
        assert not t1[:3].any() and not t1[n - 2:].any() and not t2[:6].any() and not t2[max(n - 5, 0):].any()
        if n >= 12:
            assert t1[3:n - 2].all() and t2[6:n - 5].all()          # noisy samples: every computed position is above zero
        assert ev["start"][0] == 0 and ev["start"].size == len(ev["peaks"]) + 1 and float(ev["length"].sum()) == n
    pa = np.full(40, 80.0, F)                                        # a flat read: no peak, one event over all of it
    ev = M.detect_events(pa)
    assert ev["peaks"] == [] and ev["start"].tolist() == [0] and ev["length"].tolist() == [40.0] and ev["mean"].tolist() == [80.0] and ev["stdv"].tolist() == [0.0]


def test_a_flat_run_across_a_chunk_boundary_can_leave_a_cold_start_in_another_state():
    level_mean, reads, _ = load_events_fixture()
    sig, _ = M.find_flat_run_read(level_mean, 1024, 64)
    t1, t2 = M.tstats_of(*sig[:4])
    assert M.chunks_to_redo(t1, t2, 1024, 64) >= 1
    long_read = max(reads, key=lambda r: r[0].size)
    assert M.chunks_to_redo(*M.tstats_of(*long_read[:4]), 1024, 64) == 0      # an ordinary read converges within the warm-up


def test_the_library_checks_its_arguments_before_it_needs_a_device():
    import genarchbench_amd as g
    from genarchbench_amd import abea
    lib = g.lib()
    assert abea.events_shape() == (1024, 64)
    assert lib.gab_abea_events(None, *([None] * 6), C.c_int64(1), *([None] * 6), C.c_int64(0), None) == -22
    assert lib.gab_abea_events_device(None, None, C.c_int64(0), *([None] * 5), C.c_int64(1), *([None] * 6), C.c_int64(0), None, None) == -22
    assert lib.gab_abea_scalings(None, *([None] * 6), C.c_int64(1), None, None) == -22
    assert lib.gab_abea_scalings_device(None, None, C.c_int64(0), None, None, None, C.c_int64(0), None, None, C.c_int64(1), None, None, None) == -22
    assert lib.gab_abea_events_last_stats(None, *([None] * 7)) == -22 and lib.gab_abea_events_stage_ms(None, None, None, None) == -22
    assert lib.gab_abea_scalings_last_stats(None, None, None, None, None) == -22
    raw, raw_off, n_samples, rg, dg, of = abea.pack_signals([(np.ones(7, F), 1.0, 1.0, 0.0), (np.ones(3, F), 2.0, 4.0, 1.0)])
    assert raw.size == 10 and raw_off.tolist() == [0, 7] and n_samples.tolist() == [7, 3] and dg.tolist() == [1.0, 4.0] and of.tolist() == [0.0, 1.0]
