"""abea on the GPU: gab_abea_align / gab_abea_align_device against the model (tests/abea_model.py) on every field of gab_abea_read
and every pair of the path, bit for bit, and against the reference's recorded results on the golden fixture and on the case fixture
(tests/golden/abea_cases.npz: the constructed reads of tests/abea_cases.py), where the fields the reference computes but does not
return are also compared with their recomputation from the path (tests/abea_path_checks.py)."""
import numpy as np
import pytest

import abea_cases as CASES
import abea_model as M
import abea_path_checks as P
from test_abea_model import load_fixture, model_of_cases, recorded

pytestmark = pytest.mark.gpu
FIELDS = ("n_pairs", "path_len", "end_event", "max_gap", "flags", "avg_log_emission", "fills")


@pytest.fixture(scope="module")
def cases():
    """model, the named edge cases and the three long reads of the fixture (tests/abea_cases.py), in shuffled order, with the model's
    answer for each"""
    (mean, stdv, lstd), names, reads = CASES.named_cases()
    want = [M.align(r[0], r[1], mean, stdv, lstd, r[2], r[3]) for r in reads]
    return (mean, stdv, lstd), names, reads, want


@pytest.fixture(scope="module")
def case_fixture():
    """abea_cases.npz: names, reads, the reference's record and the model's answers"""
    model, names, reads, exp = CASES.load_cases()
    return model, names, reads, exp, model_of_cases()


@pytest.fixture(scope="module")
def aligner(cases):
    from genarchbench_amd.abea import EventAligner
    mean, stdv, lstd = cases[0]
    h = EventAligner(mean, stdv, lstd)
    yield h
    h.close()


def check(names, want, pairs, pair_off, res):
    for i, (name, (rec, path)) in enumerate(zip(names, want)):
        got = {f: res[i][f].item() for f in FIELDS}
        print(name, got)
        assert got == {f: rec[f] for f in FIELDS}, f"{name}: {got} != {rec}"      # avg_log_emission: equal doubles, bit for bit
        assert res[i]["pad"] == 0
        p = pairs[pair_off[i]:pair_off[i] + rec["path_len"]]
        assert np.array_equal(p["ref_pos"], path[:, 0]) and np.array_equal(p["read_pos"], path[:, 1]), name


def test_the_cases_cover_what_they_are_named_for(cases):
    _, names, reads, want = cases
    by = dict(zip(names, zip(reads, want)))
    bands = lambda n: len(by[n][0][0]) - M.K + 1 + len(by[n][0][1]) + 2
    assert [bands(n) for n in ("bands_99", "bands_100", "bands_101")] == [99, 100, 101] and bands("under_100_bands_a") < 100
    assert by["no_end_nan_events"][1][0]["flags"] == M.NO_END and by["one_event_300_bases"][1][0]["max_gap"] > 50
    assert by["gap_one_event_60_kmers"][1][0]["flags"] & M.GAP and by["wrong_shift"][1][0]["flags"] == M.LOW_EMISSION
    assert by["plain"][1][0]["flags"] == 0 and all(by[n][1][0]["flags"] == 0 for n in names if n.startswith("long_"))
    assert by["one_kmer_300_events"][1][0]["path_len"] >= 1


def test_host_call_equals_the_model_on_every_field_and_pair(cases, aligner):
    _, names, reads, want = cases
    pairs, pair_off, res = aligner.align_reads(reads)
    check(names, want, pairs, pair_off, res)
    st = aligner.last_stats()
    assert st["launches"] == 1 and st["cells"] == int(res["fills"].sum()) == sum(w[0]["fills"] for w in want)
    assert st["bands"] == sum(len(r[0]) - M.K + 1 + len(r[1]) + 2 for r in reads) and 0 < st["kernel_ms"] <= st["total_ms"]


def test_each_case_alone_equals_the_model(cases, aligner):
    _, names, reads, want = cases
    for name, r, w in zip(names, reads, want):
        if not name.startswith("long_"):
            pairs, pair_off, res = aligner.align_reads([r])
            check([name], [w], pairs, pair_off, res)


def test_a_small_trace_budget_cuts_the_call_into_launches_with_the_same_output(cases, aligner, monkeypatch):
    _, names, reads, want = cases
    first = aligner.align_reads(reads)
    monkeypatch.setenv("GAB_ABEA_TRACE_BYTES", str(32 * 9000))       # a long read (about 8400 bands) fills a launch
    pairs, pair_off, res = aligner.align_reads(reads)
    assert aligner.last_stats()["launches"] >= 3
    check(names, want, pairs, pair_off, res)
    assert res.tobytes() == first[2].tobytes()
    monkeypatch.delenv("GAB_ABEA_TRACE_BYTES")
    pairs, pair_off, res = aligner.align_reads(reads[:5])            # two calls on one handle are independent
    assert aligner.last_stats()["launches"] == 1
    check(names[:5], want[:5], pairs, pair_off, res)


def device_call(aligner, reads):
    """the host call and the device call on torch tensors -> (pair_off, host pairs, host records, device pairs, device records)"""
    import torch
    from genarchbench_amd import abea
    packed = abea.pack_reads(reads)
    host_pairs, pair_off, host_res = aligner.align(*packed)
    dev = [torch.from_numpy(a).cuda() for a in packed]
    room = int((pair_off + abea.pair_room(packed[2], packed[5])).max())
    pairs = torch.full((room, 2), -1, dtype=torch.int32, device="cuda")
    res = torch.zeros(len(reads) * abea.READ.itemsize, dtype=torch.uint8, device="cuda")
    aligner.align_device(*dev[:8], pairs, dev[8], res)
    return pair_off, host_pairs, host_res, pairs.cpu().numpy().reshape(-1).view(abea.PAIR), res.cpu().numpy().view(abea.READ)


def test_device_call_with_torch_tensors_equals_the_host_call(cases, aligner):
    _, names, reads, want = cases
    pair_off, _, host_res, got_pairs, got_res = device_call(aligner, reads)
    assert got_res.tobytes() == host_res.tobytes()
    check(names, want, got_pairs, pair_off, got_res)
    assert aligner.last_stats()["cells"] == int(got_res["fills"].sum())


# ---- the case fixture: the reference's record, the recomputation from the path, the model ------------------------------------------
def check_case_fixture(case_fixture, pairs, pair_off, res):
    """every read of abea_cases.npz: n_pairs, path_len and the path against the reference's record; end_event, max_gap, flags and
    avg_log_emission (an equal double) against the recomputation from the path (tests/abea_path_checks.py) and against what the
    golden script recorded of it from the reference's own path; every field and pair against the model.  fills depends on the band
    moves, which the reference does not show: it is compared with the model only."""
    model, names, reads, exp, want = case_fixture
    check(names, want, pairs, pair_off, res)
    for i, (name, r, w) in enumerate(zip(names, reads, exp["reads"])):
        if name in exp["undefined_in_reference"]:
            continue
        if name == exp["deviation"]["name"]:                          # the reference backtracks from event 0; the library's rule
            assert res[i]["flags"] == M.NO_END and res[i]["path_len"] == 0
            continue
        p = pairs[pair_off[i]:pair_off[i] + res[i]["path_len"]]
        path = np.stack([p["ref_pos"], p["read_pos"]], 1)
        assert (int(res[i]["n_pairs"]), int(res[i]["path_len"]), M.pairs_digest(path)) == (w["n_pairs"], w["path_len"], w["pairs"]), name
        chk = P.recompute(r[0], r[1], *model, r[2], r[3], path)
        assert P.agrees(res[i], chk), f"{name}: {res[i]} != {chk}"
        assert (chk["end_event"], chk["admissible"], np.float64(chk["avg_log_emission"]).tobytes()) == recorded(w), name


def test_the_case_fixture_in_one_host_call_and_in_the_device_call(case_fixture, aligner):
    reads = case_fixture[2]
    pair_off, host_pairs, host_res, dev_pairs, dev_res = device_call(aligner, reads)
    assert aligner.last_stats()["launches"] == 1
    check_case_fixture(case_fixture, host_pairs, pair_off, host_res)
    assert dev_res.tobytes() == host_res.tobytes()
    check_case_fixture(case_fixture, dev_pairs, pair_off, dev_res)


def test_the_case_fixture_cut_into_launches(case_fixture, aligner, monkeypatch):
    reads = case_fixture[2]
    bands = sum(len(r[0]) - M.K + 1 + len(r[1]) + 2 for r in reads)
    monkeypatch.setenv("GAB_ABEA_TRACE_BYTES", str(32 * (bands // 4)))      # 32 bytes of trace per band: four launches at least
    pairs, pair_off, res = aligner.align_reads(reads)
    st = aligner.last_stats()
    assert st["launches"] >= 3 and st["bands"] == bands
    check_case_fixture(case_fixture, pairs, pair_off, res)


def test_the_threshold_cases_by_name(case_fixture, aligner):
    """max_gap 50 passes and 51 sets GAP alone; the two reads whose shifts are neighbouring floats differ in LOW_EMISSION alone; the
    path lengths around the 64 lanes of the emission sum and of the move of the path; the paths that all but fill their room"""
    model, names, reads, exp, _ = case_fixture
    pick = ["max_gap_50", "max_gap_51", "emission_above", "emission_below", "room_one_short", "room_tightest"] + [f"path_len_{n}" for n in CASES.PATH_LENGTHS]
    pairs, pair_off, res = aligner.align_reads([reads[names.index(n)] for n in pick])
    got = dict(zip(pick, res))
    assert (got["max_gap_50"]["max_gap"], got["max_gap_50"]["flags"]) == (50, 0) and got["max_gap_50"]["n_pairs"] == got["max_gap_50"]["path_len"] > 0
    assert (got["max_gap_51"]["max_gap"], got["max_gap_51"]["flags"], got["max_gap_51"]["n_pairs"]) == (51, M.GAP, 0)
    above, below = got["emission_above"], got["emission_below"]
    assert (float(above["avg_log_emission"]).hex(), float(below["avg_log_emission"]).hex()) == (exp["emission_bracket"]["above"], exp["emission_bracket"]["below"])
    assert above["avg_log_emission"] >= -5.0 > below["avg_log_emission"]
    assert (above["flags"], below["flags"]) == (0, M.LOW_EMISSION) and above["n_pairs"] == above["path_len"] > 0 and below["n_pairs"] == 0
    for n in CASES.PATH_LENGTHS:
        assert got[f"path_len_{n}"]["path_len"] == got[f"path_len_{n}"]["n_pairs"] == n
    room = lambda n: len(reads[names.index(n)][0]) - M.K + 1 + len(reads[names.index(n)][1])
    assert room("room_one_short") - got["room_one_short"]["path_len"] == 1
    assert room("room_tightest") - got["room_tightest"]["path_len"] == exp["room_tightest"]


def test_the_golden_fixture_equals_the_reference(aligner):
    _, reads, exp = load_fixture()
    pairs, pair_off, res = aligner.align_reads(reads)
    for i, want in enumerate(exp["reads"]):
        p = pairs[pair_off[i]:pair_off[i] + res[i]["path_len"]]
        path = np.stack([p["ref_pos"], p["read_pos"]], 1)
        assert (int(res[i]["n_pairs"]), int(res[i]["path_len"]), M.pairs_digest(path)) == (want["n_pairs"], want["path_len"], want["pairs"]), i


def test_bad_reads_are_refused_by_name(cases, aligner):
    from genarchbench_amd import GabError
    _, names, reads, _ = cases
    for bad in ((b"ACGTA", np.ones(3, np.float32), 1.0, 0.0), (b"ACGTACGT", np.zeros(0, np.float32), 1.0, 0.0)):
        with pytest.raises(GabError) as e:
            aligner.align_reads([reads[0], bad])
        assert e.value.code == -22 and "read 1" in str(e.value)
