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


def test_a_subset_of_the_fixture_equals_the_reference():
    _, cpg, reads, _, exp = load_meth_fixture()
    for i in subset():
        sites, rec = model_of(cpg, reads[i])
        same_as_recorded(sites, rec, exp["reads"][str(i)], f"read {i}")
        if str(i) in exp["lines"]:
            assert M.methylation_rows("contig", "read", reads[i]["ref"], reads[i]["ref_pos"], sites) == exp["lines"][str(i)]
            assert [s["start_position"] for s in sites] == sorted(s["start_position"] for s in sites)
