"""gab_abea_meth_device held to the stream contract of include/gab.h the way tests/test_stream_order_gpu.py holds the other `_device`
entry points: inputs that earlier work on the stream produces are read after it, and once the stream has run dry nothing of the call
reads an input or writes an output."""
import numpy as np
import pytest

from tests import stream_order_cases as soc
from tests.test_stream_order_gpu import delay, run_case  # noqa: F401  (delay is the module's fixture)

pytestmark = pytest.mark.gpu


def meth_case():
    from genarchbench_amd import abea
    import abea_meth_model as M
    from test_abea_meth_model import load_meth_fixture, model_of_cases
    from test_abea_realign_gpu import read_of
    model, cpg, _, cases, _ = load_meth_fixture()
    names = ["kmers_64_reverse", "cigar_operations", "separation_11", "past_the_last_pair", "rows_400"]
    want = model_of_cases()
    p = abea.pack_aligned_reads([read_of(cases[n]) for n in names])
    room = abea.meth_room(p[0], p[1], p[2])
    out_off = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.int64)
    keys = ("ref", "ref_off", "ref_len", "ref_pos", "is_rev", "cigar", "cigar_off", "n_cigar", "seq_len", "events", "event_off", "n_events", "map", "map_off", "calib")
    real = dict(zip(keys, p))
    real.update(cigar=p[5].view(np.int32), map=p[12].view(np.int32).reshape(-1, 2), calib=p[14].view(np.uint8).reshape(len(names), -1), out_off=out_off)
    # the decoy: the same shapes, every read skipped by its calibration record, other events and another strand
    decoy = {k: v.copy() for k, v in real.items()}
    dc = p[14].copy(); dc["read_stat_flag"] = 1; dc["scale"] = 2.0
    decoy.update(calib=dc.view(np.uint8).reshape(len(names), -1), events=(real["events"] + np.float32(5)).astype(np.float32), is_rev=(1 - real["is_rev"]).astype(np.uint8))
    out = np.frombuffer(bytes([soc.SENTINEL8]) * 32 * int(room.sum() + 4), abea.SITE).copy()
    res = np.zeros(len(names), abea.METH)
    for i, n in enumerate(names):
        sites, rec = want[n]
        for j, s in enumerate(sites):
            for f in abea.SITE.names:
                out[int(out_off[i]) + j][f] = s[f]
        for f in M.COUNTERS:
            res[i][f] = rec[f]
    d_out = np.frombuffer(bytes([soc.SENTINEL8]) * out.nbytes, abea.SITE).copy()
    d_res = np.zeros(len(names), abea.METH); d_res["flags"] = M.SKIPPED
    as_rows = lambda a: a.view(np.uint8).reshape(len(a), -1)
    stats = dict(reads=len(names), groups=int(res["groups"].sum()), sites=int(res["n_sites"].sum()), cells=int(res["cells"].sum()))
    return model, cpg, soc.Case(real, decoy, dict(out=as_rows(out), res=as_rows(res)), dict(out=as_rows(d_out), res=as_rows(d_res)), stats=stats,
                                decoy_stats=dict(reads=len(names), groups=0, sites=0, cells=0))


def test_abea_meth_device(delay):  # noqa: F811
    """sites and records byte for byte, the room behind every read's sites untouched"""
    from genarchbench_amd.abea import EventAligner
    model, cpg, case = meth_case()
    h = EventAligner(*model)
    h.set_cpg_model(*cpg)
    names = ("ref", "ref_off", "ref_len", "ref_pos", "is_rev", "cigar", "cigar_off", "n_cigar", "seq_len", "events", "event_off", "n_events", "map", "map_off", "calib")

    def call(inp, out, stream):
        h.call_methylation_device(*(inp[k] for k in names), out["out"], inp["out_off"], out["res"], stream=stream)
    try:
        run_case("abea-meth", case, call, delay, stats=h.meth_last_stats)
    finally:
        h.close()
