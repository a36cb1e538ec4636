"""abea's base-to-event map, recalibration and read checks without a GPU: the model (tests/abea_calib_model.py) reproduces what the
reference's postalign and recalibrate_model returned, and the flag its checks set, for every read of the golden fixture and every
constructed case (tests/golden/make_abea_calib_golden.py recorded them); the two quirks of the event alignment; and the library's
new entry points and the mirror's new methods, with the argument checks that run before a device is needed."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import abea_calib_model as M
from test_abea_model import load_fixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
_CACHE = {}


def load_calib_fixture():
    """-> (pore model, fixture reads as (bases, events, scale, shift, n_pairs, path), cases name -> (bases, events, scale, shift,
    n_pairs, path), the recorded reference); n_pairs is what align() returned: 0 for a read that failed its checks"""
    if "fx" not in _CACHE:
        model, reads, _ = load_fixture()
        z = np.load(os.path.join(GOLDEN, "abea_calib_small.npz"))
        exp = json.load(open(os.path.join(GOLDEN, "abea_calib_expected.json")))
        at = np.concatenate([[0], np.cumsum(np.maximum(z["path_len"] - 1, 0), dtype=np.int64)])
        fixture = [(*r, int(z["n_pairs"][i]), M.decode_path(z["first"][i], z["steps"][at[i]:at[i + 1]])) for i, r in enumerate(reads)]
        so = np.concatenate([[0], np.cumsum(z["c_seq_len"], dtype=np.int64)]); eo = np.concatenate([[0], np.cumsum(z["c_n_events"], dtype=np.int64)])
        at = np.concatenate([[0], np.cumsum(np.maximum(z["c_path_len"] - 1, 0), dtype=np.int64)])
        cases = {}
        for i, name in enumerate(z["c_name"].tolist()):
            path = M.decode_path(z["c_first"][i], z["c_steps"][at[i]:at[i + 1]])
            cases[name] = (z["c_seq"][so[i]:so[i + 1]].tobytes(), z["c_events"][eo[i]:eo[i + 1]], z["c_scale"][i], z["c_shift"][i], len(path), path)
        _CACHE["fx"] = (model, fixture, cases, exp)
    return _CACHE["fx"]


def model_of(model, read):
    seq, events, scale, shift, n_pairs, path = read
    return M.calibrate(seq, events, model[0], model[1], scale, shift, path[:n_pairs])


def model_of_fixture():
    """the model's (record, map) of every fixture read and case, computed once per process"""
    if "model" not in _CACHE:
        model, fixture, cases, _ = load_calib_fixture()
        _CACHE["model"] = ([model_of(model, r) for r in fixture], {n: model_of(model, c) for n, c in cases.items()})
    return _CACHE["model"]


def test_the_fixture_is_the_one_the_reference_ran_on():
    exp = json.load(open(os.path.join(GOLDEN, "abea_calib_expected.json")))
    assert hashlib.sha256(open(os.path.join(GOLDEN, exp["fixture"]), "rb").read()).hexdigest() == exp["fixture_sha256"]
    assert os.path.getsize(os.path.join(GOLDEN, exp["fixture"])) < 500_000 and len(exp["reads"]) == 205 and len(exp["cases"]) == 9
    base = json.load(open(os.path.join(GOLDEN, "abea_expected.json")))
    _, fixture, _, _ = load_calib_fixture()
    for r, w in zip(fixture, base["reads"]):         # the stored paths are the ones align() was recorded with
        assert (r[4], len(r[5]), M.A.pairs_digest(r[5])) == (w["n_pairs"], w["path_len"], w["pairs"])


def test_model_reproduces_the_reference_on_every_read_of_the_fixture():
    _, fixture, _, exp = load_calib_fixture()
    got, _ = model_of_fixture()
    for i, ((rec, m), want) in enumerate(zip(got, exp["reads"])):
        assert M.record_of(rec, m) == want, f"read {i}"
    flags = [w["flag"] for w in exp["reads"]]
    assert flags.count(M.FAILED_ALIGNMENT) == 13 and flags.count(M.FAILED_CALIBRATION) == 69 and flags.count(0) == 123
    near = sorted(w["n_m_state"] for w in exp["reads"] if w["flag"] != M.FAILED_ALIGNMENT and 195 <= w["n_m_state"] <= 205)
    assert near[0] < 200 <= near[-1] and 200 in near                  # both sides of the 200-state rule, and the rule's own value


def test_model_reproduces_the_reference_on_every_constructed_case():
    _, _, cases, exp = load_calib_fixture()
    _, got = model_of_fixture()
    assert set(got) == set(exp["cases"])
    for name, (rec, m) in got.items():
        assert M.record_of(rec, m) == exp["cases"][name], name
    flag = {n: w["flag"] for n, w in exp["cases"].items()}
    var = {n: float.fromhex(w["var"]) for n, w in exp["cases"].items()}
    assert var["var_2.0"] < var["var_2.4"] <= 2.5 < var["var_2.6"] < var["var_3.0"]
    assert (flag["var_2.0"], flag["var_2.4"], flag["var_2.6"], flag["var_3.0"]) == (0, 0, 1, 1)
    assert float.fromhex(exp["cases"]["epb_5"]["events_per_base"]) == 5.0 and flag["epb_5"] == 0
    assert float.fromhex(exp["cases"]["epb_6"]["events_per_base"]) == 6.0 and flag["epb_6"] == M.FAILED_QUALITY_CHK
    assert [(exp["cases"][f"m_{n}"]["n_m_state"], exp["cases"][f"m_{n}"]["recalibrated"], flag[f"m_{n}"]) for n in (199, 200, 201)] == \
        [(199, 0, 1), (200, 1, 0), (201, 1, 0)]


def model_of_long_reads():
    """the generator's reads of 16384 k-mers and more, and the model's (record, map) of each, computed once per process"""
    if "long" not in _CACHE:
        model = load_calib_fixture()[0]
        reads = {n: (*r[:4], len(r[4]), r[4]) for n, r in M.long_reads(model[0], model[1]).items()}
        _CACHE["long"] = (reads, {n: model_of(model, r) for n, r in reads.items()})
    return _CACHE["long"]


def test_model_reproduces_the_reference_on_the_reads_longer_than_the_map_kernels_stride():
    exp = load_calib_fixture()[3]["long"]
    reads, got = model_of_long_reads()
    assert list(got) == list(exp) and sorted({len(r[0]) - M.K + 1 for r in reads.values()}) == list(M.LONG_KMERS)
    for name, (rec, m) in got.items():
        assert M.record_of(rec, m) == exp[name], name
        edges = [k for k in M.STRIDE_EDGES if k < len(m)]
        assert ((m[edges, 0] == -1) == ("none" in name)).all() and m[0, 0] == 0, name
        assert len(m) // 12 < (m[:, 0] == -1).sum() < len(m) // 8 and rec["recalibrated"] == 1 and rec["n_m_state"] > len(m) // 2, name


def test_the_first_entry_of_a_kmer_is_E_after_a_kmer_of_the_same_rank():
    """a homopolymer run, and a period-2 repeat whose middle k-mer got no event: in both the previous k-mer that had events has
    the same rank, so the k-mer's first entry is 'E' and is not counted; every later entry of a k-mer is 'E' anyway"""
    ranks = M.A.kmer_ranks(b"CAAAAAAAG").tolist()                     # k-mers 1 and 2 are AAAAAA
    m = M.path_of_counts([1, 1, 1, 1])
    bm, epb = M.base_to_event_map(m, 4)
    assert bm.tolist() == [[0, 0], [1, 1], [2, 2], [3, 3]] and epb == 0.75
    assert M.event_alignment(bm, ranks) == (4, [(0, 0), (1, 1), (3, 3)])
    ranks = M.A.kmer_ranks(b"ACACACAC").tolist()                      # ranks of k-mers 0 and 2 are equal
    bm, _ = M.base_to_event_map(M.path_of_counts([2, 0, 3]), 3)
    assert bm.tolist() == [[0, 1], [-1, -1], [2, 4]]                  # the skip's pair repeats event 1: not a new event for k-mer 1
    assert M.event_alignment(bm, ranks) == (5, [(0, 0)])
    bm, _ = M.base_to_event_map(M.path_of_counts([2, 1, 3]), 3)
    assert M.event_alignment(bm, ranks) == (6, [(0, 0), (1, 2), (2, 3)])


def test_a_pair_counts_only_when_its_event_differs_from_the_previous_pairs():
    """pairs (0, 4) (1, 4) (1, 5) (2, 5) (3, 5): k-mers 2 and 3 get no event, k-mer 1 only event 5; max - min over ALL pairs"""
    bm, epb = M.base_to_event_map([(0, 4), (1, 4), (1, 5), (2, 5), (3, 5)], 5)
    assert bm.tolist() == [[4, 4], [5, 5], [-1, -1], [-1, -1], [-1, -1]] and epb == 0.2
    assert M.decode_path(*M.encode_path([(0, 4), (1, 4), (1, 5), (2, 5), (3, 5)])).tolist() == [[0, 4], [1, 4], [1, 5], [2, 5], [3, 5]]


def test_a_flat_pore_model_has_singular_normal_equations():
    """constant level_mean: div = A00 * A11 - A01 * A01 = 0 up to rounding, so shift, scale and var are infinities or NaNs (or
    huge) as the arithmetic gives them; a NaN var fails neither comparison, so no calibration flag is set"""
    rng = np.random.default_rng(2)
    mean, stdv = np.full(M.A.NKMER, 90.0, F), np.full(M.A.NKMER, 2.0, F)
    seq, ev, sc, sh, path = M.read_of_counts(rng, M.changing_bases(rng, 220), np.ones(220, np.int64), mean, stdv)
    rec, _ = M.calibrate(seq, ev, mean, stdv, sc, sh, path)
    assert rec["recalibrated"] == 1 and rec["n_m_state"] == 220 and np.isnan(rec["var"]) and np.isnan(rec["log_var"]) and rec["read_stat_flag"] == 0


def test_no_pairs_is_a_failed_alignment():
    rec, m = M.calibrate(b"ACGTACG", np.ones(3, F), np.ones(M.A.NKMER, F), np.ones(M.A.NKMER, F), 1.25, -3.0, np.zeros((0, 2), np.int32))
    assert rec == dict(n_alignment=0, n_m_state=0, read_stat_flag=M.FAILED_ALIGNMENT, recalibrated=0, scale=F(1.25), shift=F(-3.0), var=F(1),
                       log_var=F(0), events_per_base=0.0) and m.tolist() == [[-1, -1], [-1, -1]]


def test_the_library_and_the_mirror_have_the_calibration():
    import genarchbench_amd as g
    from genarchbench_amd import abea
    lib = g.lib()
    for name in ("gab_abea_calibrate", "gab_abea_calibrate_device", "gab_abea_calibrate_last_stats"):
        assert hasattr(lib, name), f"libgab_hip.so does not export {name}"
    for name in ("calibrate", "calibrate_reads", "calibrate_device", "calibrate_last_stats", "signal_to_calibrated"):
        assert callable(getattr(abea.EventAligner, name, None)), f"EventAligner.{name}"
    assert (abea.FAILED_CALIBRATION, abea.FAILED_ALIGNMENT, abea.FAILED_QUALITY_CHK) == (1, 2, 4)
    assert abea.CALIB.itemsize == 40 and abea.CALIB.names[-1] == "events_per_base" and abea.CALIB.fields["events_per_base"][1] == 32
    assert abea.RANGE.itemsize == 8
    # the argument checks that run before a device is needed
    assert lib.gab_abea_calibrate(None, *([None] * 11), C.c_int64(1), None, None, None) == -22
    assert lib.gab_abea_calibrate_device(None, None, C.c_int64(0), None, None, None, C.c_int64(0), None, None, None, None, None, C.c_int64(0), None, None,
                                         C.c_int64(1), None, C.c_int64(0), None, None, None) == -22
    assert lib.gab_abea_calibrate_last_stats(None, None, None, None, None, None) == -22
