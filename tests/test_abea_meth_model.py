"""The numpy model of calculate_methylation_for_read (tests/abea_meth_model.py) against the reference's recorded results
(tests/golden/abea_meth_expected.json, made by tests/golden/make_abea_meth_golden.py, which compares every read): every constructed
case, a fixed subset of the fixture reads (all of them take most of a minute here), the printed lines, the defined deviations by the
model's own stated rules, and the two string functions against their descriptions."""
import hashlib
import json
import os

import numpy as np

import abea_meth_model as M
import abea_realign_model as R
from test_abea_realign_model import load_realign_fixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
_CACHE = {}


def load_meth_fixture():
    """-> (pore model, CpG model, fixture reads by index (those without an N operation), cases name -> dict, the recorded reference)"""
    if "fx" not in _CACHE:
        model, reads, _, _ = load_realign_fixture()
        z = np.load(os.path.join(GOLDEN, "abea_meth_small.npz"))
        exp = json.load(open(os.path.join(GOLDEN, "abea_meth_expected.json")))
        cpg = (z["cpg_mean"], z["cpg_stdv"], z["cpg_log_stdv"])
        ro = np.concatenate([[0], np.cumsum(z["c_ref_len"], dtype=np.int64)]); co = np.concatenate([[0], np.cumsum(z["c_n_cigar"], dtype=np.int64)])
        eo = np.concatenate([[0], np.cumsum(z["c_n_events"], dtype=np.int64)]); mo = np.concatenate([[0], np.cumsum(z["c_seq_len"] - M.K + 1, dtype=np.int64)])
        cmap = z["c_map"].reshape(-1, 2)
        cases = {}
        for i, name in enumerate(z["c_name"].tolist()):
            s = z["c_scalings"][i]
            cases[name] = dict(ref=z["c_ref"][ro[i]:ro[i + 1]].tobytes(), ref_pos=int(z["c_ref_pos"][i]), is_rev=int(z["c_is_rev"][i]),
                               cigar=z["c_cigar"][co[i]:co[i + 1]], seq_len=int(z["c_seq_len"][i]), events=z["c_events"][eo[i]:eo[i + 1]],
                               map=cmap[mo[i]:mo[i + 1]].copy(),
                               calib=dict(scale=s[0], shift=s[1], var=s[2], log_var=s[3], events_per_base=float(z["c_epb"][i]), read_stat_flag=int(z["c_flag"][i])))
        _CACHE["fx"] = (model, cpg, {int(i): reads[int(i)] for i in exp["reads"]}, cases, exp)
    return _CACHE["fx"]


def cpg_of(cpg, name):
    return M.FLAT_CPG if name in M.FLAT_CASES else cpg


def model_of(cpg, c):
    return M.call_methylation(c["ref"], c["ref_pos"], c["is_rev"], c["cigar"], c["seq_len"], c["events"], c["map"], c["calib"], cpg)


def model_of_cases():
    """the model's (sites, record) of every constructed case, computed once per process"""
    if "cases" not in _CACHE:
        _, cpg, _, cases, _ = load_meth_fixture()
        _CACHE["cases"] = {n: model_of(cpg_of(cpg, n), c) for n, c in cases.items()}
    return _CACHE["cases"]


def subset():
    """fixture reads the model is run on: one in eight of those kept, and the three whose lines are recorded"""
    _, _, reads, _, exp = load_meth_fixture()
    return sorted(set(sorted(reads)[::8]) | {int(i) for i in exp["lines"]})


def same_as_recorded(sites, rec, want, name):
    assert {k: int(rec[k]) for k in M.COUNTERS} == {k: want[k] for k in M.COUNTERS}, name
    assert M.site_bits(sites) == want["sites"], name


def test_the_fixture_is_the_one_the_reference_ran_on():
    exp = json.load(open(os.path.join(GOLDEN, "abea_meth_expected.json")))
    assert hashlib.sha256(open(os.path.join(GOLDEN, exp["fixture"]), "rb").read()).hexdigest() == exp["fixture_sha256"]
    assert os.path.getsize(os.path.join(GOLDEN, exp["fixture"])) < 500_000 and os.path.getsize(os.path.join(GOLDEN, "abea_meth_expected.json")) < 500_000
    c = exp["counts"]
    assert c["scored_reads"] >= 100 and c["sites"] >= 1000 and c["reverse_reads_with_sites"] >= 30 and c["groups_of_3_or_more"] >= 1
    assert min(c["skipped_start"], c["skipped_unbounded"], c["skipped_short"]) >= 20 and c["dominated_folds_flat"] >= 1
    assert len(exp["lines"]) == 3 and exp["reference_meth_seconds"] > 0 and exp["blocks_per_lane"] == M.BLOCKS_PER_LANE and exp["one_block_kmers"] == M.ONE_BLOCK_KMERS
    assert sum(len(r["sites"]) for r in exp["reads"].values()) == c["sites"]
    _, _, reads, cases, _ = load_meth_fixture()
    assert all(M.aligned_pairs(r["cigar"], r["ref_pos"]) is not None for r in reads.values()) and len(reads) < 205
    assert set(cases) == set(exp["cases"]) and {n for n, w in exp["cases"].items() if not w["by_reference"]} == set(M.DEVIATIONS) | {"read_stat_flag"}


def test_the_generators_reproduce_the_fixture():
    model, cpg, _, cases, _ = load_meth_fixture()
    again = M.make_cpg_model(model)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, cpg))
    made = M.make_cases(model)
    assert list(made) == list(cases)
    for n, c in made.items():
        w = cases[n]
        assert c["ref"] == w["ref"] and c["events"].tobytes() == w["events"].tobytes() and np.array_equal(c["map"], w["map"]) and np.array_equal(c["cigar"], w["cigar"]), n


def test_the_logsum_table_is_the_references():
    z = np.load(os.path.join(GOLDEN, "abea_meth_small.npz"))
    assert M.TABLE.tobytes() == z["logsum"].tobytes() and M.TABLE.size == M.LOGSUM_TBL
    a = np.array([0.0, -np.inf, -3.0, -20.0, -15.7, -15.699], F); b = np.zeros(6, F)
    got = M.logsum(a, b)
    assert got[0] == F(F(0) + M.TABLE[0]) and got[1] == 0 and got[2] == F(F(0) + M.TABLE[3000]) and got[3] == 0 and got[4] == 0 and got[5] == F(F(0) + M.TABLE[15699])
    assert M.logsum(np.array([-np.inf], F), np.array([-np.inf], F))[0] == -np.inf


def test_methylate_and_its_reverse_complement():
    assert M.methylate(b"ACGCGTCCGG") == b"AMGMGTCMGG" and M.methylate(b"GACGC") == b"GAMGC" and M.methylate(b"TTC") == b"TTC"
    assert M.reverse_complement_meth(b"AMGT") == b"AMGT" and M.reverse_complement_meth(M.methylate(b"GACGCC")) == b"GGMGTC"
    for s in (b"GACGTACGCGAT", b"CGCGCG", b"TTTT"):
        assert M.reverse_complement_meth(M.methylate(s)) == M.methylate(R.revcomp(s))
    assert M.kmer_rank5(b"AAAAAA") == 0 and M.kmer_rank5(b"TTTTTT") == M.NKMER5 - 1 and M.kmer_rank5(b"AAAAMG") == 3 * 5 + 2
    assert M.cpg_groups(b"ACGTTTTTTTTCGTTTTTTTTTTTCG") == [(1, 11, 2), (24, 24, 1)]


def test_the_constructed_cases_equal_the_reference():
    _, _, _, cases, exp = load_meth_fixture()
    got = model_of_cases()
    for n in cases:
        same_as_recorded(*got[n], exp["cases"][n], n)
    bpl, one = M.BLOCKS_PER_LANE, M.ONE_BLOCK_KMERS
    assert {f"kmers_{n}" for n in M.kmer_count_cases(bpl, one)} <= set(cases) and {16, 216, one - 1, one, one + 1, 32 * bpl - 1, 32 * bpl + 1} <= set(M.kmer_count_cases(bpl, one))
    cells = lambda n: got[n][1]["cells"]
    assert cells("single_cpg") == 2 * 41 * 16 and cells("span_200") == 2 * 221 * 216 and cells("event_distance_11") == 2 * 12 * 16 and cells("rows_400") == 2 * 401 * 16
    assert got["separation_10"][1]["n_sites"] == 1 and got["separation_11"][1]["n_sites"] == 2 and got["span_202"][1]["skipped_span"] == 1
    assert got["sub_start_10"][1]["skipped_start"] == 1 and got["sub_start_11"][1]["n_sites"] == 1 and got["event_distance_10"][1]["skipped_short"] == 1
    assert got["past_the_last_pair"][1]["skipped_unbounded"] == 1 and got["degenerate_record"][1]["skipped_unbounded"] == 1 and got["no_cpg"][1]["groups"] == 0
    assert got["cgcg_run"][0][0]["n_cpg"] == 4 and [s["n_cpg"] for s in got["lower_case_and_iupac"][0]] == [1, 1, 1]
    assert [s["first_cpg"] for s in got["lower_case_and_iupac"][0]] == [40, 130, 160]
    for n in M.FLAT_CASES:                               # a flat model cannot tell the variants apart
        assert all(s["ll_unmethylated"] == s["ll_methylated"] for s in got[n][0]) and got[n][0]


def test_the_defined_deviations():
    got = model_of_cases()
    assert got["read_stat_flag"][1]["flags"] == M.SKIPPED and got["read_stat_flag"][1]["groups"] == 0 and not got["read_stat_flag"][0]
    assert got["no_event"][1]["flags"] == M.NO_EVENT and got["no_event"][1]["n_sites"] == 1 and got["no_event"][1]["groups"] == 2
    assert got["strand"][1]["flags"] == M.STRAND and not got["strand"][0]
    assert got["transitions"][1]["flags"] == M.TRANSITIONS and got["transitions"][1]["groups"] == 1 and not got["transitions"][0]
    for n in M.WINDOW_NO_EVENT:
        assert got[n][1]["flags"] == M.NO_EVENT and got[n][1]["groups"] == 1 and not got[n][0], n


def test_the_window_of_the_closest_event():
    """what each window case is there for, by the map it was made with and by the model's answer"""
    _, _, _, cases, exp = load_meth_fixture()
    got = model_of_cases()
    assert all(exp["cases"][n]["by_reference"] == (n not in M.WINDOW_NO_EVENT) for n in M.WINDOW_CASES)
    event_of = lambda n, k: int(cases[n]["map"][k, 0])
    e1_of = lambda n: M.closest_event(M.WINDOW_CASES[n][1] - M.MIN_SEPARATION, cases[n]["map"][:, 0], len(cases[n]["map"]))
    site = lambda n: (got[n][0][0]["event_start"], got[n][0][0]["event_stop"])
    for d in (63, 64, 65):
        n = f"behind_{d}"
        assert (cases[n]["map"][100 - d + 1:101] == -1).all() and site(n) == (event_of(n, 100 - d), event_of(n, 120)) and site(n)[0] == e1_of(n) >= 0, n
    assert site("behind_999") == (event_of("behind_999", 51), event_of("behind_999", 1070)) and (cases["behind_999"]["map"][52:1051] == -1).all()
    assert event_of("behind_1000", 50) == 50 and site("behind_1000") == (event_of("behind_1000", 1051), event_of("behind_1000", 1070)) == (51, 70)
    c = cases["behind_1000_nothing_ahead"]
    assert c["map"][10, 0] >= 0 and c["map"][2010, 0] >= 0 and (c["map"][11:2010] == -1).all() and e1_of("behind_1000_nothing_ahead") == -1
    assert e1_of("ahead_999") == event_of("ahead_999", 1010) == 0 and (cases["ahead_999"]["map"][:1010] == -1).all()
    assert got["ahead_999"][1]["skipped_short"] == 1 and got["ahead_999"][1]["flags"] == 0        # both ends of the group find entry 1010's event
    assert event_of("ahead_1000", 1011) == 0 and (cases["ahead_1000"]["map"][:1011] == -1).all() and e1_of("ahead_1000") == -1
    assert event_of("entry_0_only", 0) == 0 and site("entry_0_only") == (event_of("entry_0_only", 12), event_of("entry_0_only", 31)) == (1, 20)
    c = cases["last_entry_only"]                         # neither the first nor the last pair finds an event: the record is emptied (meth.c:169-178)
    assert c["map"][-1, 0] == 0 and (c["map"][:-1] == -1).all() and got["last_entry_only"][1]["skipped_unbounded"] == 1 and got["last_entry_only"][1]["flags"] == 0


def test_the_groups_on_the_edges_of_a_step_of_64_positions():
    _, _, _, cases, exp = load_meth_fixture()
    got = model_of_cases()
    assert all(exp["cases"][n]["by_reference"] for n in M.STEP_CASES)
    firsts = lambda n: [(s["first_cpg"], s["n_cpg"]) for s in got[n][0]]
    for p in (63, 64, 127, 128):
        assert firsts(f"start_{p}") == [(p, 1)] and cases[f"start_{p}"]["ref"][p:p + 2] == b"CG"
    for r in ("", "_reverse"):
        assert firsts("start_64" + r) == [(64, 1)] and firsts("sites_54_64" + r) == [(54, 2)] and firsts("sites_53_64" + r) == [(53, 1), (64, 1)]
        assert firsts("group_60_to_130" + r) == [(60, 8)] and got["group_60_to_130" + r][0][0]["end_position"] - got["group_60_to_130" + r][0][0]["start_position"] == 70
        assert bool(cases["start_64" + r]["is_rev"]) == bool(r)
    assert firsts("start_127_reverse") == [(127, 1)]
    c = cases["site_at_ref_len_minus_2"]
    assert c["ref"][-2:] == b"CG" and len(c["ref"]) == 120 and firsts("site_at_ref_len_minus_2") == [(60, 1)]
    assert got["site_at_ref_len_minus_2"][1]["groups"] == 2 and got["site_at_ref_len_minus_2"][1]["skipped_unbounded"] == 1


def test_a_subset_of_the_fixture_equals_the_reference():
    _, cpg, reads, _, exp = load_meth_fixture()
    for i in subset():
        sites, rec = model_of(cpg, reads[i])
        same_as_recorded(sites, rec, exp["reads"][str(i)], f"read {i}")
        if str(i) in exp["lines"]:
            assert M.methylation_rows("contig", "read", reads[i]["ref"], reads[i]["ref_pos"], sites) == exp["lines"][str(i)]
            assert [s["start_position"] for s in sites] == sorted(s["start_position"] for s in sites)
