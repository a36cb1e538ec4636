"""gab_abea_realign_device held to the stream contract of include/gab.h the way tests/test_stream_order_gpu.py holds the other
`_device` entry points: inputs that earlier work on the stream produces are read after it, and once the stream has run dry nothing
of the call reads an input or writes an output."""
import numpy as np
import pytest

from tests import stream_order_cases as soc
from tests.test_stream_order_gpu import delay, run_case  # noqa: F401  (delay is the module's fixture)

pytestmark = pytest.mark.gpu


def realign_case():
    from genarchbench_amd import abea
    import abea_realign_model as M
    from test_abea_realign_model import load_realign_fixture, model_of_cases
    model, _, cases, _ = load_realign_fixture()
    names = ["reverse", "leading_S", f"rows_{M.ROWS + 1}", "three_segments", "k_run_over_the_lane_wrap"]
    want = model_of_cases()
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs])
    cs = [cases[n] for n in names]
    ref_len = np.array([len(c["ref"]) for c in cs], np.int32); n_cigar = np.array([len(c["cigar"]) for c in cs], np.int32)
    n_events = np.array([c["events"].size for c in cs], np.int32); seq_len = np.array([c["seq_len"] for c in cs], np.int32)
    cigar = cat([c["cigar"] for c in cs], np.uint32)
    calib = np.zeros(len(cs), abea.CALIB)
    for i, c in enumerate(cs):
        for f in ("scale", "shift", "var", "log_var", "events_per_base", "read_stat_flag"):
            calib[i][f] = c["calib"][f]
    room = abea.realign_room(n_events, cigar, off(n_cigar), n_cigar)
    real = dict(ref=cat([np.frombuffer(c["ref"], np.uint8) for c in cs], np.uint8), ref_off=off(ref_len), ref_len=ref_len,
                ref_pos=np.array([c["ref_pos"] for c in cs], np.int32), is_rev=np.array([c["is_rev"] for c in cs], np.uint8), cigar=cigar.view(np.int32),
                cigar_off=off(n_cigar), n_cigar=n_cigar, seq_len=seq_len, events=cat([c["events"] for c in cs], np.float32), event_off=off(n_events),
                n_events=n_events, map=cat([c["map"] for c in cs], np.int32).reshape(-1, 2), map_off=off(seq_len.astype(np.int64) - M.K + 1),
                calib=calib.view(np.uint8).reshape(len(cs), -1), out_off=off(room))
    # the decoy: the same shapes, every read skipped by its calibration record, other events and another strand
    decoy = {k: v.copy() for k, v in real.items()}
    dc = calib.copy(); dc["read_stat_flag"] = 1; dc["scale"] = 2.0
    decoy.update(calib=dc.view(np.uint8).reshape(len(cs), -1), events=(real["events"] + np.float32(5)).astype(np.float32), is_rev=(1 - real["is_rev"]).astype(np.uint8))
    out = np.frombuffer(bytes([soc.SENTINEL8]) * 12 * int(room.sum() + 4), abea.EALN).copy()
    res = np.zeros(len(cs), abea.REALIGN)
    for i, n in enumerate(names):
        e, rec = want[n]
        o = int(real["out_off"][i])
        out["ref_position"][o:o + len(e)] = e[:, 0]; out["event_idx"][o:o + len(e)] = e[:, 1]; out["hmm_state"][o:o + len(e)] = e[:, 2]; out["pad"][o:o + len(e)] = 0
        for f in abea.REALIGN.names:
            res[i][f] = rec[f]
    d_out = np.frombuffer(bytes([soc.SENTINEL8]) * out.nbytes, abea.EALN).copy()
    d_res = np.zeros(len(cs), abea.REALIGN); d_res["flags"] = M.SKIPPED
    as_rows = lambda a: a.view(np.uint8).reshape(len(a), -1)
    stats = dict(reads=len(cs), hmm_segments=int(res["hmm_segments"].sum()), cells=int(res["cells"].sum()), reads_requeued=1)
    return model, soc.Case(real, decoy, dict(out=as_rows(out), res=as_rows(res)), dict(out=as_rows(d_out), res=as_rows(d_res)), stats=stats,
                           decoy_stats=dict(reads=len(cs), hmm_segments=0, cells=0, reads_requeued=0))


def test_abea_realign_device(delay):  # noqa: F811
    """entries and records byte for byte, the room behind every read's entries untouched; one read of the batch goes through the
    second launch, so the requeue decision's synchronisation is inside the call under test"""
    from genarchbench_amd.abea import EventAligner
    model, case = realign_case()
    h = EventAligner(*model)
    names = ("ref", "ref_off", "ref_len", "ref_pos", "is_rev", "cigar", "cigar_off", "n_cigar", "seq_len", "events", "event_off", "n_events", "map", "map_off", "calib")

    def call(inp, out, stream):
        h.realign_device(*(inp[k] for k in names), out["out"], inp["out_off"], out["res"], stream=stream)
    try:
        run_case("abea-realign", case, call, delay, stats=h.realign_last_stats)
    finally:
        h.close()
