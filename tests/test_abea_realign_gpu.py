"""abea's realign_read on the GPU: gab_abea_realign and its device form, bit for bit against the reference's recorded results
(tests/golden/abea_realign_expected.json) on the fixture reads and the constructed cases, against the model
(tests/abea_realign_model.py) where the reference cannot run, and the input rules."""
import numpy as np
import pytest

import abea_realign_model as M
from test_abea_calib_model import load_calib_fixture
from test_abea_realign_model import load_realign_fixture, model_of_cases

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def aligner():
    from genarchbench_amd.abea import EventAligner
    h = EventAligner(*load_realign_fixture()[0])
    yield h
    h.close()


@pytest.fixture(scope="module")
def flat_aligner():
    from genarchbench_amd.abea import EventAligner
    h = EventAligner(*M.FLAT_MODEL)
    yield h
    h.close()


def read_of(c, flag=None):
    """a case or fixture read as EventAligner.realign_reads takes it"""
    cal = dict(n_alignment=0, n_m_state=0, recalibrated=1, **{k: c["calib"][k] for k in ("scale", "shift", "var", "log_var", "events_per_base", "read_stat_flag")})
    if flag is not None:
        cal["read_stat_flag"] = flag
    return (c["ref"], c["ref_pos"], c["is_rev"], c["cigar"], c["seq_len"], c["events"], c["map"], cal)


def entries_of(got, i):
    e, off, res = got
    mine = e[off[i]:off[i] + res[i]["n_entries"]]
    assert (mine["pad"] == 0).all()
    return np.stack([mine["ref_position"], mine["event_idx"], mine["hmm_state"]], 1).astype(np.int64), res[i]


def check_model(got, i, want, name):
    e, rec = entries_of(got, i)
    we, wrec = want
    for f in ("n_entries", "hmm_segments", "max_rows", "flags", "cells"):
        assert int(rec[f]) == int(wrec[f]), f"{name}: {f} {rec[f]}, the model has {wrec[f]}"
    assert np.array_equal(e, we), f"{name}: entries"


def check_golden(got, i, want, name):
    e, rec = entries_of(got, i)
    assert M.record_of(e, rec) == {k: v for k, v in want.items() if k != "rows"}, name
    if want.get("rows") is not None:
        assert e.tolist() == want["rows"], name


def device_form(aligner, reads, region=(-1, -1), calib_from=None, canary=0x5a):
    """the same batch through gab_abea_realign_device -> (entries, out_off, records); calib_from: (rmap tensor, map_off tensor, calib
    tensor) of calibrate_device to take in place of the reads' own"""
    import torch
    from genarchbench_amd import abea
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs]) if xs else np.zeros(0, dt)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ref_len = np.array([len(r[0]) for r in reads], np.int32); n_cigar = np.array([len(r[3]) for r in reads], np.int32)
    n_events = np.array([len(r[5]) for r in reads], np.int32); n_map = np.array([len(r[6]) for r in reads], np.int64)
    cig = cat([r[3] for r in reads], np.uint32)
    room = abea.realign_room(n_events, cig, off(n_cigar), n_cigar)
    out_off = off(room)
    calib = np.zeros(len(reads), abea.CALIB)
    for i, r in enumerate(reads):
        for f in abea.CALIB.names:
            calib[i][f] = r[7][f]
    rmap, map_off, cal = calib_from or (up(cat([np.asarray(r[6], np.int32) for r in reads], np.int32).reshape(-1, 2)), up(off(n_map)), up(calib.view(np.uint8)))
    out = torch.full((int(room.sum()) * 12 + 24,), canary, dtype=torch.uint8, device="cuda")
    res = torch.full((len(reads) * 24,), canary, dtype=torch.uint8, device="cuda")
    try:
        aligner.realign_device(up(cat([np.frombuffer(bytes(r[0]), np.uint8) for r in reads], np.uint8)), up(off(ref_len)), up(ref_len), up(np.array([r[1] for r in reads], np.int32)),
                               up(np.array([r[2] for r in reads], np.uint8)), up(cig.view(np.int32)), up(off(n_cigar)), up(n_cigar), up(np.array([r[4] for r in reads], np.int32)),
                               up(cat([r[5] for r in reads], F)), up(off(n_events)), up(n_events), rmap, map_off, cal, out, up(out_off), res, region=region)
    finally:
        device_form.last = (out.cpu().numpy(), res.cpu().numpy())
    o = device_form.last[0]
    assert (o[int(room.sum()) * 12:] == canary).all()      # nothing behind the last read's room
    return o[:int(room.sum()) * 12].view(abea.EALN), out_off, device_form.last[1].view(abea.REALIGN)


def test_the_golden_fixture_equals_the_reference(aligner):
    """all 205 reads through the host entry and through the device entry, the latter chained from calibrate_device's own buffers"""
    import torch
    from genarchbench_amd import abea
    from test_abea_calib_gpu import flat_of
    _, reads, _, exp = load_realign_fixture()
    batch = [read_of(r) for r in reads]
    got = aligner.realign_reads(batch)
    st = aligner.realign_last_stats()
    for i, want in enumerate(exp["reads"]):
        check_golden(got, i, want, f"read {i}")
    assert (got[2]["flags"] == M.SKIPPED).sum() == 82 and (got[2]["flags"][got[2]["flags"] != M.SKIPPED] == 0).all()
    assert st["reads"] == 205 and st["hmm_segments"] == sum(w["hmm_segments"] for w in exp["reads"]) == int(got[2]["hmm_segments"].sum())
    assert st["cells"] == int(got[2]["cells"].sum()) and st["rows"] >= st["hmm_segments"] * 3 and st["reads_requeued"] == 0
    assert 0 < st["kernel_ms"] <= st["total_ms"] * 1.001 and abs(st["prep_ms"] + st["viterbi_ms"] + st["requeue_ms"] - st["kernel_ms"]) < 1e-3
    # calibrate_device's map and records, still on the device, go straight in
    flat = flat_of(load_calib_fixture()[1])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in flat]
    n_kmers = flat[2].astype(np.int64) - M.K + 1
    map_off = torch.from_numpy(np.concatenate([[0], np.cumsum(n_kmers)[:-1]]).astype(np.int64)).cuda()
    rmap = torch.full((int(n_kmers.sum()), 2), -7, dtype=torch.int32, device="cuda")
    cal = torch.zeros(len(reads) * abea.CALIB.itemsize, dtype=torch.uint8, device="cuda")
    aligner.calibrate_device(*dev, rmap, map_off, cal)
    got = device_form(aligner, batch, calib_from=(rmap, map_off, cal))
    for i, want in enumerate(exp["reads"]):
        check_golden(got, i, want, f"read {i}, device form")
    # the columns the suite's check reads, for the three reads listed in full
    for i, rows in exp["full"].items():
        r = reads[int(i)]
        e = got[0][got[1][int(i)]:got[1][int(i)] + got[2][int(i)]["n_entries"]]
        assert [list(x) for x in abea.eventalign_rows(r["ref"], r["ref_pos"], r["is_rev"], e)] == rows, f"read {i}"


def test_the_constructed_cases_equal_the_reference_and_the_model(aligner, flat_aligner):
    """reference length 11 / 12, stop event 1 / 2 away, 49 / 50 / 51 emittable entries, last pair at +100 / +101, deletions of 95 and 101,
    96 k-mers on 6 rows (a K run across every lane), events_per_base 1.0 / 0.8 / 5.0, a reverse read, lower case and IUPAC, leading S, H
    and I, an empty second segment, three segments, a region that cuts both ends, NO_EVENT and STRAND, and the nearest event 63, 64, 65,
    999 and 1000 entries behind the k-mer looked up, 999 and 1000 ahead of it, at entry 0 and at the last entry"""
    _, _, cases, exp = load_realign_fixture()
    want = model_of_cases()
    names = [n for n in cases if n not in M.FLAT_CASES and not n.startswith("rows_") and n != "region_cuts_both_ends"]
    batch = [read_of(cases[n]) for n in names]
    for got in (aligner.realign_reads(batch), device_form(aligner, batch)):
        for i, n in enumerate(names):
            check_model(got, i, want[n], n)
            if n not in M.DEVIATIONS:
                check_golden(got, i, exp["cases"][n], n)
    flags = {n: int(got[2][i]["flags"]) for i, n in enumerate(names)}
    assert flags["no_event"] == M.NO_EVENT and flags["strand"] == M.STRAND and flags["second_segment_empty"] == M.NO_PAIRS
    assert all(flags[n] == M.NO_EVENT for n in M.WINDOW_NO_EVENT)      # the event one entry outside the window of get_closest_event_to is not found
    assert sum(flags.values()) == M.NO_EVENT * (1 + len(M.WINDOW_NO_EVENT)) + M.STRAND + M.NO_PAIRS
    c = cases["region_cuts_both_ends"]
    for got in (aligner.realign_reads([read_of(c)], region=c["region"]), device_form(aligner, [read_of(c)], region=c["region"])):
        check_model(got, 0, want["region_cuts_both_ends"], "region"); check_golden(got, 0, exp["cases"]["region_cuts_both_ends"], "region")
        e, _ = entries_of(got, 0)
        assert e[:, 0].min() >= c["region"][0] and e[:, 0].max() <= c["region"][1] - 5
    for n in M.FLAT_CASES:                               # SAME / PREV ties fill the matrix: the largest index decides
        got = flat_aligner.realign_reads([read_of(cases[n])])
        check_model(got, 0, want[n], n); check_golden(got, 0, exp["cases"][n], n)


def test_the_trace_capacity_and_the_second_launch(aligner):
    """sections of ROWS - 1, ROWS and ROWS + 1 rows: reads_requeued 0, 0, 1; one batch mixes requeued and ordinary reads"""
    from genarchbench_amd import abea
    _, _, cases, exp = load_realign_fixture()
    want = model_of_cases()
    assert abea.realign_shape() == M.ROWS
    for n, requeued in ((M.ROWS - 1, 0), (M.ROWS, 0), (M.ROWS + 1, 1)):
        name = f"rows_{n}"
        got = aligner.realign_reads([read_of(cases[name])])
        check_model(got, 0, want[name], name); check_golden(got, 0, exp["cases"][name], name)
        st = aligner.realign_last_stats()
        assert st["reads_requeued"] == requeued and int(got[2][0]["max_rows"]) == n and st["rows"] == n, st
    names = ["reverse", f"rows_{M.ROWS + 1}", "three_segments", f"rows_{M.ROWS + 1}", f"rows_{M.ROWS}", "k_run_over_the_lane_wrap"]
    batch = [read_of(cases[n]) for n in names]
    for got in (aligner.realign_reads(batch), device_form(aligner, batch)):
        for i, n in enumerate(names):
            check_model(got, i, want[n], f"{n} in the mixed batch")
        assert aligner.realign_last_stats()["reads_requeued"] == 2


def test_a_read_with_flag_0_between_skipped_reads(aligner):
    _, _, cases, _ = load_realign_fixture()
    want = model_of_cases()
    a, b = cases["reverse"], cases["leading_S"]
    skipped = (np.zeros((0, 3), np.int64), dict(n_entries=0, hmm_segments=0, max_rows=0, flags=M.SKIPPED, cells=0))
    for order in ([(a, 1), (b, 0), (a, 4)], [(b, 0), (a, 2), (b, 0)], [(a, 2), (a, 1), (b, 0)], [(b, 0), (a, 4), (a, 2)]):
        batch = [read_of(c, flag) for c, flag in order]
        for got in (aligner.realign_reads(batch), device_form(aligner, batch)):
            for i, (c, flag) in enumerate(order):
                check_model(got, i, skipped if flag else want["reverse" if c is a else "leading_S"], f"{order}: read {i}")


def test_no_reads(aligner):
    e, off, res = aligner.realign_reads([])
    assert e.size == 0 and res.size == 0
    st = aligner.realign_last_stats()
    assert (st["reads"], st["hmm_segments"], st["rows"], st["cells"], st["reads_requeued"], st["kernel_ms"], st["total_ms"]) == (0, 0, 0, 0, 0, 0.0, 0.0)


def broken(cases, what):
    """three reads, an input rule broken in read 1"""
    reads = [list(read_of(cases[n])) for n in ("leading_S", "reverse", "deletion_95")]
    r = reads[1]
    r[3] = r[3].copy(); r[5] = r[5].copy(); r[6] = r[6].copy(); r[7] = dict(r[7])
    if what == "seq_len":
        r[4] = 5; r[6] = r[6][:0]; r[3] = M.encode_cigar([("M", 5)])
    elif what == "n_events":
        r[5] = r[5][:0]
    elif what == "reference_byte":
        r[0] = r[0][:30] + b"J" + r[0][31:]
    elif what == "cigar_operation_P":
        r[3][1] = (3 << 4) | 6
    elif what == "cigar_operation_9":
        r[3][1] = (3 << 4) | 9
    elif what == "reference_span":
        r[0] = r[0][:-1]
    elif what == "read_span":
        r[3] = np.concatenate([r[3], M.encode_cigar([("S", 1)])])
    elif what == "event_nan":
        r[5][7] = np.nan
    elif what == "event_inf":
        r[5][-1] = np.inf
    elif what == "scale_inf":
        r[7]["scale"] = F(np.inf)
    elif what == "shift_nan":
        r[7]["shift"] = F(np.nan)
    elif what == "var_zero":
        r[7]["var"] = F(0.0)
    elif what == "var_negative":
        r[7]["var"] = F(-1.0)
    elif what == "log_var_nan":
        r[7]["log_var"] = F(np.nan)
    elif what == "map_below":
        r[6][3, 0] = -2
    elif what == "map_above":
        r[6][-1, 0] = len(r[5])
    return [tuple(x) for x in reads]


RULES = ("seq_len", "n_events", "reference_byte", "cigar_operation_P", "cigar_operation_9", "reference_span", "read_span", "event_nan", "event_inf",
         "scale_inf", "shift_nan", "var_zero", "var_negative", "log_var_nan", "map_below", "map_above")


@pytest.mark.parametrize("what", RULES)
def test_a_broken_input_rule_is_refused_by_name_and_nothing_is_written(aligner, what):
    from genarchbench_amd import GabError, abea
    _, _, cases, _ = load_realign_fixture()
    batch = broken(cases, what)
    if what != "n_events":                               # (the mirror's own packing needs an event to size the room)
        with pytest.raises(GabError) as e:
            aligner.realign_reads(batch)
        assert e.value.code == -22 and "read 1" in str(e.value), str(e.value)
    with pytest.raises(GabError) as e:
        device_form(aligner, batch)
    assert e.value.code == -22 and "read 1" in str(e.value), str(e.value)
    out, res = device_form.last
    assert (out == 0x5a).all() and (res == 0x5a).all()


def test_the_host_entry_writes_nothing_when_it_refuses_and_checks_the_room(aligner):
    from genarchbench_amd import GabError, abea
    _, _, cases, _ = load_realign_fixture()
    good = [read_of(cases[n]) for n in ("leading_S", "three_segments", "deletion_95")]
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs])

    def args(reads):
        ref_len = np.array([len(r[0]) for r in reads], np.int32); n_cigar = np.array([len(r[3]) for r in reads], np.int32)
        n_events = np.array([len(r[5]) for r in reads], np.int32)
        calib = np.zeros(len(reads), abea.CALIB)
        for i, r in enumerate(reads):
            for f in abea.CALIB.names:
                calib[i][f] = r[7][f]
        return (cat([np.frombuffer(r[0], np.uint8) for r in reads], np.uint8), off(ref_len), ref_len, np.array([r[1] for r in reads], np.int32),
                np.array([r[2] for r in reads], np.uint8), cat([r[3] for r in reads], np.uint32), off(n_cigar), n_cigar, np.array([r[4] for r in reads], np.int32),
                cat([r[5] for r in reads], F), off(n_events), n_events, cat([r[6] for r in reads], np.int32).view(abea.RANGE),
                off(np.array([len(r[6]) for r in reads])), calib)
    a = args(good)
    room = abea.realign_room(a[11], a[5], a[6], a[7])
    assert room.tolist() == [len(good[0][5]), 3 * len(good[1][5]), len(good[2][5])]
    out = (np.frombuffer(bytes([0xa5]) * 12 * int(room.sum()), abea.EALN).copy(), np.frombuffer(bytes([0xa5]) * 72, abea.REALIGN).copy())
    tight = off(room)
    tight[2] -= 1                                        # read 1 is left one entry short of n_events * (1 + 2 N operations)
    with pytest.raises(GabError) as e:
        aligner.realign(*a, out_off=tight, out=out)
    assert e.value.code == -22 and "read 1" in str(e.value), str(e.value)
    bad = args(broken(cases, "reference_byte"))
    with pytest.raises(GabError) as e:
        aligner.realign(*bad, out=(out[0][:int(abea.realign_room(bad[11], bad[5], bad[6], bad[7]).sum())], out[1]))
    assert e.value.code == -22 and "read 1" in str(e.value)
    assert out[0].tobytes() == bytes([0xa5]) * out[0].nbytes and out[1].tobytes() == bytes([0xa5]) * 72
    got = aligner.realign(*a, out=out)                   # and the same buffers, whole, are filled
    want = model_of_cases()
    for i, n in enumerate(("leading_S", "three_segments", "deletion_95")):
        check_model(got, i, want[n], n)
