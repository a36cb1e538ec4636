"""CPU: tests/dbg_model.py against the golden fixture that tests/golden/make_dbg_golden.py took from the compiled reference
(dbg/src/debruijn.cpp, dbg/src/common.cpp), the fixture's own hashes and sizes, and format_region against the kept verbose lines."""
import hashlib
import os

import numpy as np

from tests import dbg_cases as dc
from tests import dbg_model as M


def test_fixture_hashes_and_sizes():
    doc, regions, reads, z = dc.fixture()
    npz = os.path.join(dc.GOLDEN, "dbg_small.npz")
    assert hashlib.sha256(open(npz, "rb").read()).hexdigest() == doc["fixture_sha256"]
    assert os.path.getsize(npz) < 500_000 and os.path.getsize(os.path.join(dc.GOLDEN, "dbg_expected.json")) < 500_000
    assert len(doc["regions"]) == len(regions) == len(z["region"]) and doc["k"] == 15 and doc["min_qual"] == 20
    assert doc["reference_graph_seconds"] > 0 and doc["reference_host"]
    for name in ("empty_regions", "qc_fail_reads", "quality_drop_first", "quality_drop_last", "n_drop_first", "n_drop_last", "colour3_nodes", "nodes_first_in_read",
                 "self_loops", "nodes_with_4_edges", "dropped_fifth", "shared_reads"):
        assert doc["counts"][name] >= 1, name
    assert len(doc["full"]) == 3


def test_model_is_the_reference_on_every_region():
    doc, regions, reads, _ = dc.fixture()
    off, recs, stats = dc.fixture_model()
    assert len(off) == len(regions) + 1
    for i, want in enumerate(doc["regions"]):
        mine = recs[off[i]:off[i + 1]]
        assert len(mine) == want["nodes"] and int(mine["n_edges"].sum()) == want["edges"] and int(mine["weight"].sum()) == want["weight"], i
        assert dc.sha(mine) == want["sha256"], f"region {i}"
    for i, full in doc["full"].items():
        i = int(i)
        assert recs[off[i]:off[i + 1]].tobytes().hex() == full["records"]
    assert stats["nodes"] == sum(r["nodes"] for r in doc["regions"]) and stats["dropped"] == doc["counts"]["dropped_fifth"]


def test_model_under_other_parameters():
    doc, regions, reads, _ = dc.fixture()
    for key, hashes in doc["other_parameters"].items():
        k, mq = (int(x) for x in key.split(","))
        for i, (ref, start, b, e) in enumerate(regions):
            assert dc.sha(M.build_region(ref, start, reads[b:e], k, mq, b)) == hashes[i], (key, i)


def test_planner_is_the_reference():
    """the fixture's planned regions carry the windows the compiled setWindowPointers returned (the golden script asserts it)"""
    _, regions, _, z = dc.fixture()
    plan = M.plan_regions(0, len(z["contig"]), z["read_pos"], z["read_end"], len(z["contig"]))
    assert np.array_equal(plan, z["plan"]) and len(plan) == int((z["region"][:, 0] == 1).sum()) == 12
    for row, reg in zip(plan, z["region"]):
        assert reg[1] == row[0] and reg[3] == row[1] and reg[4] == row[2] and reg[5] == row[3] and reg[6] == row[4]
    assert (plan[1:, 3] < plan[:-1, 4]).any(), "no read shared by two regions"


def test_format_region_gives_the_verbose_lines():
    from genarchbench_amd import dbg
    doc, regions, reads, _ = dc.fixture()
    for i, full in doc["full"].items():
        ref, start, b, e = regions[int(i)]
        recs = np.frombuffer(bytes.fromhex(full["records"]), M.NODE)
        assert M.format_region(ref, start, reads, recs).decode() == full["line"]
        assert dbg.format_region(ref, start, reads, recs).decode() == full["line"]
        assert dbg.format_region(ref, start, [r[0] for r in reads], recs).decode() == full["line"]
    assert dbg.NODE == M.NODE


def test_model_rules_by_hand():
    # k = 2: ref ACGT has one edge AC -> CG; a read ACGAT at qualities 30 .. 34 adds AC -> CG again and CG -> GA
    r = M.build_region(b"ACGT", 10, [(b"ACGAT", bytes([30, 31, 32, 33, 34]), 0)], k=2, min_qual=20)
    assert r["colours"].tolist() == [3, 3, 2] and r["position"].tolist() == [10, 11, -1] and r["weight"].tolist() == [31, 62, 31]
    assert r["src_read"].tolist() == [-1, -1, 0] and r["src_off"].tolist() == [0, 1, 2]
    assert r["n_edges"].tolist() == [1, 1, 0] and r["edge_to"][:2, 0].tolist() == [1, 2] and r["edge_weight"][:2, 0].tolist() == [31, 31]
    # a homopolymer: one node, its weight counted twice per occurrence, one edge to itself
    r = M.build_region(b"AAAAA", 0, [], k=2)
    assert len(r) == 1 and r["weight"][0] == 4 and r["n_edges"][0] == 1 and r["edge_to"][0, 0] == 0 and r["edge_weight"][0, 0] == 2
