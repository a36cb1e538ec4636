"""gab_dbg_build_device held to the stream contract of include/gab.h the way tests/test_stream_order_gpu.py holds the other `_device`
entry points: inputs that earlier work on the stream produces are read after it, and once the stream has run dry nothing of the call
reads an input or writes an output."""
import numpy as np
import pytest

from tests import dbg_cases as dc
from tests import stream_order_cases as soc
from tests.test_stream_order_gpu import delay, run_case  # noqa: F401  (delay is the module's fixture)

pytestmark = pytest.mark.gpu
ROOM = 4        # records of room behind the last node: they keep the sentinel


def dbg_case():
    """the golden fixture.  The decoy: the real offsets and read ranges, every length 0 (no region has a node), other letters, qualities
    and positions -- valid alone and in any mixture with the real arrays"""
    from genarchbench_amd import dbg
    doc, regions, reads, _ = dc.fixture()
    want_off, want, stats = dc.fixture_model()
    real = dbg.pack_regions(regions, reads)
    decoy = {k: v.copy() for k, v in real.items()}
    decoy.update(ref=soc.other_letters(real["ref"]), seq=soc.other_letters(real["seq"]), qual=np.full_like(real["qual"], 7), ref_len=np.zeros_like(real["ref_len"]),
                 read_len=np.zeros_like(real["read_len"]), ref_start=real["ref_start"] + 5, read_flag=real["read_flag"] ^ 512)
    for x in (real, decoy):
        soc.check_inside(x["ref_off"], x["ref_len"], len(real["ref"])); soc.check_inside(x["read_off"], x["read_len"], len(real["seq"]))
        assert (x["read_begin"] <= x["read_end"]).all() and x["read_end"].max() <= len(reads)
    nodes = np.full((len(want) + ROOM, dbg.NODE.itemsize), soc.SENTINEL8, np.uint8)
    nodes[:len(want)] = want.view(np.uint8).reshape(len(want), -1)
    valid = np.ones(len(nodes), bool)
    outs = dict(node_off=np.asarray(want_off).copy(), nodes=nodes)
    decoy_outs = dict(node_off=np.zeros_like(outs["node_off"]), nodes=np.full_like(nodes, soc.SENTINEL8))
    keys = ("regions", "occurrences", "passed", "nodes", "edges")
    case = soc.Case(real, decoy, outs, decoy_outs, valid={"nodes": valid}, stats={k: stats[k] for k in keys},
                    decoy_stats=dict(regions=len(regions), occurrences=0, passed=0, nodes=0, edges=0))
    for name in outs:
        assert soc.differing(case, name) >= soc.FLOOR, name
    return doc, case


def test_dbg_build_device(delay):  # noqa: F811
    """node_off and the records byte for byte, the room behind the last record untouched"""
    from genarchbench_amd.dbg import GraphBuilder
    doc, case = dbg_case()
    h = GraphBuilder(0)

    def call(inp, out, stream):
        h.build_device(inp, out["node_off"], out["nodes"], doc["k"], doc["min_qual"], stream=stream)
    try:
        run_case("dbg-build", case, call, delay, stats=h.last_stats)
    finally:
        h.close()
