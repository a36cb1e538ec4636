"""The numpy model of realign_read (tests/abea_realign_model.py) against the reference's recorded results
(tests/golden/abea_realign_expected.json, made by tests/golden/make_abea_realign_golden.py): every constructed case, a fixed subset
of the fixture reads (all 123 take about a minute here), the defined deviations and the room bound by the model's own stated rules,
and the argument that lets the skip state of a row be computed in parallel."""
import hashlib
import json
import os

import numpy as np

import abea_realign_model as M
from test_abea_calib_model import load_calib_fixture, model_of_fixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
_CACHE = {}
# fixture reads the model is run on: one in six, the three listed in full, and reads that end through the first two breaks
SUBSET = sorted(set(range(0, 205, 6)) | {14, 16, 34, 86, 88, 97, 131})


def load_realign_fixture():
    """-> (pore model, fixture reads as dicts with the fields of a constructed case, cases name -> dict, the recorded reference)"""
    if "fx" not in _CACHE:
        model, fixture, _, _ = load_calib_fixture()
        calib, _ = model_of_fixture()
        z = np.load(os.path.join(GOLDEN, "abea_realign_small.npz"))
        exp = json.load(open(os.path.join(GOLDEN, "abea_realign_expected.json")))
        ro = np.concatenate([[0], np.cumsum(z["ref_len"], dtype=np.int64)]); co = np.concatenate([[0], np.cumsum(z["n_cigar"], dtype=np.int64)])
        reads = []
        for i, r in enumerate(fixture):
            rec, rmap = calib[i]
            reads.append(dict(ref=z["ref"][ro[i]:ro[i + 1]].tobytes(), ref_pos=int(z["ref_pos"][i]), is_rev=int(z["is_rev"][i]), cigar=z["cigar"][co[i]:co[i + 1]],
                              seq_len=len(r[0]), events=np.asarray(r[1], F), map=rmap, calib=rec, region=(-1, -1)))
        ro = np.concatenate([[0], np.cumsum(z["c_ref_len"], dtype=np.int64)]); co = np.concatenate([[0], np.cumsum(z["c_n_cigar"], dtype=np.int64)])
        eo = np.concatenate([[0], np.cumsum(z["c_n_events"], dtype=np.int64)]); mo = np.concatenate([[0], np.cumsum(z["c_seq_len"] - M.K + 1, dtype=np.int64)])
        cmap = z["c_map"].reshape(-1, 2)
        cases = {}
        for i, name in enumerate(z["c_name"].tolist()):
            s = z["c_scalings"][i]
            cases[name] = dict(ref=z["c_ref"][ro[i]:ro[i + 1]].tobytes(), ref_pos=int(z["c_ref_pos"][i]), is_rev=int(z["c_is_rev"][i]),
                               cigar=z["c_cigar"][co[i]:co[i + 1]], seq_len=int(z["c_seq_len"][i]), events=z["c_events"][eo[i]:eo[i + 1]],
                               map=cmap[mo[i]:mo[i + 1]].copy(), region=tuple(int(v) for v in z["c_region"][i]),
                               calib=dict(scale=s[0], shift=s[1], var=s[2], log_var=s[3], events_per_base=float(z["c_epb"][i]), read_stat_flag=0))
        _CACHE["fx"] = (model, reads, cases, exp)
    return _CACHE["fx"]


def level_of(model, name):
    return M.FLAT_MODEL if name in M.FLAT_CASES else model


def model_of(model, c, stats=None):
    return M.realign(c["ref"], c["ref_pos"], c["is_rev"], c["cigar"], c["seq_len"], c["events"], c["map"], c["calib"], model, c["region"], stats)


def model_of_cases():
    """the model's (entries, record) of every constructed case, computed once per process"""
    if "cases" not in _CACHE:
        model, _, cases, _ = load_realign_fixture()
        _CACHE["cases"] = {n: model_of(level_of(model, n), c) for n, c in cases.items()}
    return _CACHE["cases"]


def model_of_subset():
    if "subset" not in _CACHE:
        model, reads, _, _ = load_realign_fixture()
        _CACHE["subset"] = {i: model_of(model, reads[i]) for i in SUBSET}
    return _CACHE["subset"]


def test_the_fixture_is_the_one_the_reference_ran_on():
    exp = json.load(open(os.path.join(GOLDEN, "abea_realign_expected.json")))
    assert hashlib.sha256(open(os.path.join(GOLDEN, exp["fixture"]), "rb").read()).hexdigest() == exp["fixture_sha256"]
    assert os.path.getsize(os.path.join(GOLDEN, exp["fixture"])) < 500_000 and os.path.getsize(os.path.join(GOLDEN, "abea_realign_expected.json")) < 500_000
    assert len(exp["reads"]) == 205 and len(exp["full"]) == 3 and exp["reference_realign_seconds"] > 0
    c = exp["counts"]
    assert c["realigned"] == 123 and c["skipped"] == 82 and 0 < c["reverse"] < 123
    assert min(c[k] for k in ("with_I", "with_D", "with_S", "with_EQ_X", "with_N", "break_short_ref", "break_stop_event", "state_B")) >= 1
    assert min(c[k] for k in ("from_same_m", "from_prev_m", "from_same_b", "from_prev_b", "from_prev_k")) >= 1 and c["longest_k_run"] >= 3
    assert c["break_no_output"] == 0      # no input reaches it: tests/golden/make_abea_realign_golden.py says why
    # the generators are the ones the fixture was made with
    model, reads, cases, _ = load_realign_fixture()
    fixture = load_calib_fixture()[1]
    for r, a in zip(reads, M.fixture_alignments([f[0] for f in fixture])):
        assert (r["ref"], r["ref_pos"], r["is_rev"], r["cigar"].tolist()) == (a[0], a[1], a[2], a[3].tolist())
    made = M.make_cases(model)
    assert list(made) == list(cases)
    for n, c in made.items():
        for k in ("ref", "ref_pos", "is_rev", "seq_len", "region"):
            assert c[k] == cases[n][k], (n, k)
        assert c["cigar"].tolist() == cases[n]["cigar"].tolist() and c["events"].tobytes() == cases[n]["events"].tobytes() and np.array_equal(c["map"], cases[n]["map"]), n


def test_model_reproduces_the_reference_on_every_constructed_case():
    _, _, cases, exp = load_realign_fixture()
    got = model_of_cases()
    assert set(exp["cases"]) == set(cases) - set(M.DEVIATIONS)
    for n, want in exp["cases"].items():
        e, rec = got[n]
        assert M.record_of(e, rec) == {k: v for k, v in want.items() if k != "rows"}, n
        if want["rows"] is not None:
            assert e.tolist() == want["rows"], n
    # what each case is there for
    n_of = {n: got[n][1]["n_entries"] for n in got}
    assert n_of["ref_len_11"] == 0 and n_of["ref_len_12"] > 0 and n_of["stop_event_1"] == 0 and n_of["stop_event_2"] == 2
    assert [got[f"emittable_{n}"][0][:51, 1].tolist() == list(range(1, 52)) for n in (49, 50, 51)] == [True] * 3
    assert got["end_pair_100"][1]["hmm_segments"] == 1 and got["end_pair_101"][1]["hmm_segments"] == 2
    assert [got[f"rows_{n}"][1]["max_rows"] for n in (M.ROWS - 1, M.ROWS, M.ROWS + 1)] == [M.ROWS - 1, M.ROWS, M.ROWS + 1]
    assert got["second_segment_empty"][1]["flags"] == M.NO_PAIRS and n_of["second_segment_empty"] > 0
    assert (got["epb_0.8"][0][:, 2] == ord("M")).all() and (got["flat_model"][0][:, 2] == ord("B")).sum() > 100


def test_model_reproduces_the_reference_on_the_fixture_subset():
    _, reads, _, exp = load_realign_fixture()
    got = model_of_subset()
    run = 0
    for i, (e, rec) in got.items():
        assert M.record_of(e, rec) == exp["reads"][i], f"read {i}"
        run += rec["flags"] == 0
        if str(i) in exp["full"]:
            assert [list(r) for r in M.eventalign_rows(reads[i]["ref"], reads[i]["ref_pos"], reads[i]["is_rev"], e)] == exp["full"][str(i)], f"read {i}"
    assert run >= 15 and any(rec["flags"] == M.SKIPPED for _, rec in got.values())
    assert all((exp["reads"][i]["flags"] == M.SKIPPED) == (int(reads[i]["calib"]["read_stat_flag"]) != 0) for i in range(205))


def test_the_rows_listed_in_full_are_the_mirrors_rows():
    from genarchbench_amd import abea
    _, reads, _, exp = load_realign_fixture()
    assert len(exp["full"]) == 3
    for i, rows in exp["full"].items():
        r = reads[int(i)]
        entries = np.zeros(len(rows), abea.EALN)
        entries["ref_position"] = [x[0] for x in rows]; entries["event_idx"] = [x[2] for x in rows]; entries["hmm_state"] = [ord(x[4]) for x in rows]
        assert [list(x) for x in abea.eventalign_rows(r["ref"], r["ref_pos"], r["is_rev"], entries)] == rows
        assert any(x[4] == "B" and x[3] == "NNNNNN" for x in rows) or all(x[4] == "M" for x in rows)
        assert all((x[3] == x[1]) != bool(r["is_rev"]) or x[4] == "B" or x[1] == M.revcomp(x[1].encode()).decode() for x in rows)


def test_the_two_defined_deviations_end_the_read():
    _, _, cases, _ = load_realign_fixture()
    got = model_of_cases()
    e, rec = got["no_event"]
    assert (cases["no_event"]["map"] == -1).all() and rec["flags"] == M.NO_EVENT and len(e) == 0 and rec["hmm_segments"] == 0
    e, rec = got["strand"]
    c = cases["strand"]
    first, stop = M.closest_event(0, c["map"][:, 0], len(c["map"])), M.closest_event(100, c["map"][:, 0], len(c["map"]))
    assert not c["is_rev"] and stop < first - 1 and rec["flags"] == M.STRAND and len(e) == 0 and rec["hmm_segments"] == 0
    for n in M.WINDOW_NO_EVENT:
        e, rec = got[n]
        assert (cases[n]["map"] != -1).any() and rec["flags"] == M.NO_EVENT and len(e) == 0 and rec["hmm_segments"] == 0, n


def test_the_window_of_the_closest_event():
    """what each window case is there for, by the map it was made with and by the model's answer"""
    _, _, cases, exp = load_realign_fixture()
    got = model_of_cases()
    assert set(M.WINDOW_CASES) <= set(cases) and set(M.WINDOW_CASES) - set(M.WINDOW_NO_EVENT) <= set(exp["cases"])
    first_of = lambda n: M.closest_event(M.WINDOW_CASES[n][1], cases[n]["map"][:, 0], len(cases[n]["map"]))
    event_of = lambda n, k: int(cases[n]["map"][k, 0])
    for d in (63, 64, 65):                               # the k-mer d behind is the nearest with an event, and the read starts on its first event
        n = f"behind_{d}"
        assert (cases[n]["map"][70 - d + 1:71] == -1).all() and first_of(n) == event_of(n, 70 - d) >= 0 and got[n][0][0, 1] == first_of(n) + 1, n
    assert first_of("behind_999") == event_of("behind_999", 51) >= 0 and (cases["behind_999"]["map"][52:1051] == -1).all()
    assert event_of("behind_1000", 50) >= 0 and first_of("behind_1000") == event_of("behind_1000", 1051) == event_of("behind_1000", 50) + 2
    assert got["behind_999"][1]["n_entries"] > 100 and got["behind_1000"][1]["n_entries"] > 100
    assert got["behind_999"][0][:, 1].min() == first_of("behind_999") + 1 and got["behind_1000"][0][:, 1].min() == first_of("behind_1000") + 1
    c = cases["behind_1000_nothing_ahead"]
    assert c["map"][10, 0] >= 0 and c["map"][2010, 0] >= 0 and (c["map"][11:2010] == -1).all() and first_of("behind_1000_nothing_ahead") == -1
    assert first_of("ahead_999") == event_of("ahead_999", 1004) == 0 and (cases["ahead_999"]["map"][:1004] == -1).all() and got["ahead_999"][1]["flags"] == 0
    assert event_of("ahead_1000", 1005) == 0 and (cases["ahead_1000"]["map"][:1005] == -1).all() and first_of("ahead_1000") == -1
    assert event_of("entry_0_only", 0) == 0 and first_of("entry_0_only") == event_of("entry_0_only", 6) == 2 and got["entry_0_only"][0][0, 1] == 3
    c = cases["last_entry_only"]
    assert c["map"][-1, 0] == 0 and (c["map"][:-1] == -1).all() and first_of("last_entry_only") == -1


def test_an_event_is_emitted_once_per_bam_segment_at_most():
    _, reads, cases, _ = load_realign_fixture()
    every = [(f"case {n}", cases[n], e) for n, (e, _) in model_of_cases().items()] + [(f"read {i}", reads[i], e) for i, (e, _) in model_of_subset().items()]
    for name, c, e in every:
        room = M.room_of(c["events"].size, c["cigar"])
        assert len(e) <= room, name
        n_seg = room // c["events"].size
        if n_seg == 1:
            assert len(set(e[:, 1].tolist())) == len(e), name
        else:                                        # every segment's stretch of the entries has distinct events
            assert max(np.bincount(e[:, 1])) <= n_seg if len(e) else True, name


def test_the_skip_state_of_a_row_serial_doubling_and_fixed_point_agree():
    rng = np.random.default_rng(20251022)
    kk = M.transitions(2.0)["kk"]
    mk, bk = M.transitions(2.0)["mk"], M.transitions(2.0)["bk"]
    checked = 0
    for trial in range(300):
        n = int(rng.integers(1, 97))
        m = (rng.normal(-200, 60, n)).astype(F); b = (rng.normal(-210, 60, n)).astype(F)
        kind = trial % 6
        if kind == 1:
            m[rng.random(n) < 0.3] = -np.inf; b[rng.random(n) < 0.3] = -np.inf
        elif kind == 2:
            m[rng.random(n) < 0.2] = np.nan; b[rng.random(n) < 0.2] = np.nan      # a NaN candidate counts as absent
        elif kind == 3:
            m[:] = -np.inf; b[:] = -np.inf; m[int(rng.integers(n))] = F(-3.0)      # one finite source: a K run to the end of the row
        elif kind == 4:
            m = np.round(m).astype(F); b = (m + (mk - bk)).astype(F)               # ties between the M and the B candidate
        with np.errstate(all="ignore"):
            s1 = (mk + m).astype(F); s3 = (bk + b).astype(F)
            a = np.full(n, -np.inf, F)
            a = np.where(s1 > a, s1, a); a = np.where(s3 > a, s3, a)
            if kind == 5:                            # exact ties with the K chain: a[b] = fl(kk + a[b-1]), the candidates to match
                for i in range(1, n):
                    a[i] = F(kk + a[i - 1])
                s1 = a.copy(); s3 = np.full(n, -np.inf, F)
            want = M.skip_serial(a, kk)
            assert not np.isnan(want).any()
            assert M.skip_fixed_point(a, kk).tobytes() == want.tobytes(), (trial, "fixed point")
            assert M.skip_doubling(a, kk).tobytes() == want.tobytes(), (trial, "doubling")
            # and the serial loop is update_cell's: the K column of a row filled block by block
            prev = M.NI
            for i in range(n):
                mx, _ = M.update_cell(np.array([[-np.inf], [s1[i]], [-np.inf], [s3[i]], [F(kk + prev)], [-np.inf]], F))
                prev = F(mx[0] + F(0.0))
                assert prev.tobytes() == want[i].tobytes() or (prev == 0 and want[i] == 0), (trial, i)
        checked += 1
    assert checked == 300
    # one multiplication in place of repeated additions is NOT the same
    a = np.full(90, -np.inf, F); a[0] = F(-3.1)
    direct = (a[0] + (np.arange(90) * kk).astype(F)).astype(F)
    assert M.skip_serial(a, kk).tobytes() != direct.tobytes()


def test_update_cell_takes_the_largest_index_among_ties_and_keeps_a_leading_nan():
    inf = np.inf
    mx, frm = M.update_cell(np.array([[1, -inf, np.nan, 2, -inf], [1, -inf, 5, np.nan, 3], [0, -inf, 7, 2, np.nan], [1, -inf, 1, 1, 3], [0, -inf, 1, 2, 1], [-inf, -inf, 0, -inf, -inf]], F))
    assert frm.tolist() == [3, 5, 0, 4, 3] and np.isnan(mx[2]) and mx[[0, 1, 3, 4]].tolist() == [1, -inf, 2, 3]


def test_transitions_of_events_per_base_at_and_below_one():
    t = M.transitions(1.0)
    assert t["mm_self"] == -np.inf and np.isfinite(t["mm_next"])
    t = M.transitions(0.8)
    assert np.isnan(t["mm_self"]) and np.isfinite(t["mm_next"]) and t["soft"] == F(np.log(0.5))
    assert M.transitions(2.0)["kk"] == F(np.log(F(0.3)))
