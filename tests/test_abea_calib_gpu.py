"""abea's base-to-event map, recalibration and read checks on the GPU: gab_abea_calibrate and its device form against the reference's
recorded results on the golden fixture and the constructed cases, and against the model (tests/abea_calib_model.py) on reads built
around the kernel's 64-lane chunks, bit for bit on every field and the whole map (a NaN only has to be a NaN)."""
import numpy as np
import pytest

import abea_calib_model as M
import abea_events_model as E
import abea_model as A
from test_abea_calib_model import load_calib_fixture, model_of, model_of_fixture
from test_abea_events_model import load_events_fixture, model_events_of_fixture

pytestmark = pytest.mark.gpu
F = np.float32
INTS = ("n_alignment", "n_m_state", "read_stat_flag", "recalibrated")
FLOATS = ("scale", "shift", "var", "log_var", "events_per_base")


@pytest.fixture(scope="module")
def aligner():
    from genarchbench_amd.abea import EventAligner
    mean, stdv, lstd = load_calib_fixture()[0]
    h = EventAligner(mean, stdv, lstd)
    yield h
    h.close()


def flat_of(reads):
    """reads as (bases, events, scale, shift, n_pairs, path) -> the arrays of EventAligner.calibrate: the whole path of every read
    sits in the pair buffer, as align() leaves it, n_pairs of it count"""
    from genarchbench_amd import abea
    packed = abea.pack_reads([r[:4] for r in reads])[:8]
    lens = np.array([len(r[5]) for r in reads], np.int64)
    pair_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(reads) else np.zeros(0, np.int64)
    pairs = np.concatenate([np.asarray(r[5], np.int32).reshape(-1, 2) for r in reads]) if len(reads) else np.zeros((0, 2), np.int32)
    return (*packed, pairs, pair_off, np.array([r[4] for r in reads], np.int32))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and ((np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes())


def check(got, want, names=None):
    """got: (map, map_off, records) of the library; want: per read the model's (record, map)"""
    rmap, map_off, res = got
    assert res.size == len(want)
    for i, (rec, m) in enumerate(want):
        name = names[i] if names else i
        for f in INTS:
            assert int(res[i][f]) == int(rec[f]), f"{name}: {f} {res[i][f]}, the model has {rec[f]}"
        for f in FLOATS:
            assert same(res[i][f], rec[f]), f"{name}: {f} {res[i][f]!r}, the model has {rec[f]!r}"
        mine = rmap[map_off[i]:map_off[i] + len(m)]
        assert np.array_equal(mine["start"], m[:, 0]) and np.array_equal(mine["stop"], m[:, 1]), f"{name}: map"


def device_form(aligner, flat, canary=None):
    """the same call through gab_abea_calibrate_device -> (map, map_off, records) as numpy arrays"""
    import torch
    from genarchbench_amd import abea
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in flat]
    n = flat[2].size
    n_kmers = np.maximum(flat[2].astype(np.int64) - A.K + 1, 0)
    map_off = np.concatenate([[0], np.cumsum(n_kmers)[:-1]]).astype(np.int64)
    rmap = torch.full((int(n_kmers.sum()) + 8, 2), -7 if canary is None else canary, dtype=torch.int32, device="cuda")
    res = torch.full((n * abea.CALIB.itemsize,), 0 if canary is None else canary & 0xff, dtype=torch.uint8, device="cuda")
    try:
        aligner.calibrate_device(*dev, rmap, torch.from_numpy(map_off).cuda(), res)
    finally:
        out = (rmap.cpu().numpy().reshape(-1).view(abea.RANGE), map_off, res.cpu().numpy().view(abea.CALIB))
        device_form.last = out
    return out


# ---- the reads built around the kernel's chunks of 64 k-mers ----------------------------------------------------------------------------
def counted(rng, model, counts, seq=None):
    seq, ev, sc, sh, path = M.read_of_counts(rng, M.changing_bases(rng, len(counts)) if seq is None else seq, counts, model[0], model[1])
    return (seq, ev, sc, sh, len(path), path)


@pytest.fixture(scope="module")
def boundary():
    """name -> read, and the model's answer for each"""
    model = load_calib_fixture()[0]
    rng = np.random.default_rng(61)
    named = {}
    for n in (63, 64, 65, 128, 129):
        named[f"kmers_{n}"] = counted(rng, model, rng.choice(4, n, p=(0.1, 0.5, 0.3, 0.1)) + (np.arange(n) == 1))
    seq = bytearray(M.changing_bases(rng, 300))
    seq[62:71] = b"CAAAAAAAC"                                         # k-mers 63 and 64 are AAAAAA: lane 63 and lane 0 of the next chunk
    named["homopolymer_63_64"] = counted(rng, model, np.ones(300, np.int64), bytes(seq))
    counts = np.ones(300, np.int64); counts[[0, 63, 64, 127]] = 0
    named["no_event_at_lane_0_and_63"] = counted(rng, model, counts)
    counts = np.ones(260, np.int64); counts[1:3] = 0
    named["first_pairs_share_an_event"] = counted(rng, model, counts)
    named["six_bases_one_pair"] = (b"GATTAC", np.array([88.5], F), F(1.0), F(0.0), 1, np.array([[0, 0]], np.int32))
    counts = np.zeros(320, np.int64)                                  # 'M' entries 1..64 in chunk 0, the 65th alone in chunk 1 at lane 63,
    counts[:64] = 1; counts[127] = 1; counts[128:256] = 1             # 66..193 in chunks 2 and 3, 194..199 and, at lane 63, the 200th in chunk 4
    counts[256:262] = 1; counts[319] = 1
    named["m_200_at_chunk_ends"] = counted(rng, model, counts)
    want = {n: model_of(model, r) for n, r in named.items()}
    assert [len(named[f"kmers_{n}"][0]) - 5 for n in (63, 64, 65, 128, 129)] == [63, 64, 65, 128, 129]
    assert want["homopolymer_63_64"][0]["n_m_state"] == 299 and want["homopolymer_63_64"][0]["n_alignment"] == 300
    w = want["no_event_at_lane_0_and_63"]
    assert w[1][[0, 63, 64, 127], 0].tolist() == [-1] * 4 and w[0]["n_m_state"] == 296 and named["no_event_at_lane_0_and_63"][5][0].tolist() == [1, 0]
    assert named["first_pairs_share_an_event"][5][:4].tolist() == [[0, 0], [1, 0], [2, 0], [3, 1]] and want["first_pairs_share_an_event"][1][:4].tolist() == [[0, 0], [-1, -1], [-1, -1], [1, 1]]
    assert want["six_bases_one_pair"][0]["n_alignment"] == 1 and want["six_bases_one_pair"][0]["read_stat_flag"] == M.FAILED_CALIBRATION
    w = want["m_200_at_chunk_ends"]
    assert w[0]["n_m_state"] == 200 and w[0]["recalibrated"] == 1 and (w[1][:, 0] != -1).sum() == 200
    return named, want


def run(aligner, reads, want, names=None):
    flat = flat_of(reads)
    got = aligner.calibrate(*flat)
    check(got, want, names)
    st = aligner.calibrate_last_stats()
    assert (st["reads"], st["recalibrated"], st["m_states"]) == (len(reads), sum(int(w[0]["recalibrated"]) for w in want), sum(int(w[0]["n_m_state"]) for w in want)), st
    return flat, got, st


def test_the_golden_fixture_equals_the_reference(aligner):
    _, fixture, _, exp = load_calib_fixture()
    want, _ = model_of_fixture()
    flat, (rmap, map_off, res), st = run(aligner, fixture, want)
    for form in ((rmap, map_off, res), device_form(aligner, flat)):
        rmap, map_off, res = form
        for i, w in enumerate(exp["reads"]):
            n_kmers = len(fixture[i][0]) - A.K + 1
            m = rmap[map_off[i]:map_off[i] + n_kmers]
            assert M.record_of(res[i], np.stack([m["start"], m["stop"]], 1)) == w, f"read {i}"
    check(form, want)
    assert (form[0][int(map_off[-1]) + len(fixture[-1][0]) - 5:].view(np.int32) == -7).all()      # nothing behind the last map
    assert st["recalibrated"] == 123 and 0 < st["kernel_ms"] <= st["total_ms"] * 1.001


def test_the_constructed_cases_equal_the_reference(aligner):
    _, _, cases, exp = load_calib_fixture()
    names = list(cases)
    _, want = model_of_fixture()
    flat, (rmap, map_off, res), _ = run(aligner, [cases[n] for n in names], [want[n] for n in names], names)
    for i, n in enumerate(names):
        m = rmap[map_off[i]:map_off[i] + len(cases[n][0]) - A.K + 1]
        assert M.record_of(res[i], np.stack([m["start"], m["stop"]], 1)) == exp["cases"][n], n
    flags = {n: int(res[i]["read_stat_flag"]) for i, n in enumerate(names)}
    assert flags == {"var_2.0": 0, "var_2.4": 0, "var_2.6": 1, "var_3.0": 1, "epb_5": 0, "epb_6": 4, "m_199": 1, "m_200": 0, "m_201": 0}
    check(device_form(aligner, flat), [want[n] for n in names], names)


def test_reads_around_the_chunks_of_64_kmers(aligner, boundary):
    named, want = boundary
    names = list(named)
    flat, _, _ = run(aligner, [named[n] for n in names], [want[n] for n in names], names)
    check(device_form(aligner, flat), [want[n] for n in names], names)


def test_reads_longer_than_the_map_kernels_stride(aligner):
    """cal_map runs at most 64 blocks of 256 threads a read and strides: a thread takes k-mers 16384 apart.  Reads of 16384 k-mers (one
    trip), 16385 (a second trip for one k-mer) and 32769 (a third), a tenth of their k-mers without an event, the k-mers on both sides
    of a stride (16383, 16384, 32768) among them in one variant and with an event in the other; a read of 102 bases in the same call, so
    that the blocks of a read are sized by another read.  The map entry for entry and the record against the model, and both against
    the reference's record of the same reads (regenerated by seed, tests/golden/abea_calib_expected.json holds no input of theirs)."""
    from test_abea_calib_model import model_of_long_reads
    model, _, _, exp = load_calib_fixture()
    reads, want_long = model_of_long_reads()
    short = counted(np.random.default_rng(71), model, np.ones(97, np.int64))
    names = ["bases_102"] + list(reads)
    want = [model_of(model, short)] + [want_long[n] for n in reads]
    assert len(short[0]) == 102 and [len(w[1]) for w in want[1:]] == [16384, 16384, 16385, 16385, 32769, 32769] and 64 * 256 == 16384
    flat, got, _ = run(aligner, [short] + list(reads.values()), want, names)
    for form in (got, device_form(aligner, flat)):
        check(form, want, names)
        rmap, map_off, res = form
        for i, n in enumerate(names[1:], 1):
            m = rmap[map_off[i]:map_off[i] + len(want[i][1])]
            assert M.record_of(res[i], np.stack([m["start"], m["stop"]], 1)) == exp["long"][n], n
    assert form[0].size == int(map_off[-1]) + 32769 + 8 and (form[0][int(map_off[-1]) + 32769:].view(np.int32) == -7).all()      # nothing behind the last map


def test_the_host_entry_with_slabs_that_do_not_start_at_0(aligner, boundary):
    """the three input slabs with a junk prefix of an odd length, the reads in reverse order with gaps, two reads on the same bases and
    events, the maps in reverse order with gaps behind a prefix: byte for byte the result of the same reads packed from 0, and not a byte
    of the map written outside a read's entries.  The junk is what the input rules refuse."""
    from genarchbench_amd import abea
    from test_abea_realign_launch_gpu import relay, scattered_room
    named, want = boundary
    names = ["kmers_65", "m_200_at_chunk_ends", "six_bases_one_pair", "homopolymer_63_64", "kmers_129", "no_event_at_lane_0_and_63", "kmers_65"]
    flat = flat_of([named[n] for n in names])
    plain = aligner.calibrate(*flat)
    check(plain, [want[n] for n in names], names)
    seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pairs, pair_off, n_pairs = flat
    rng = np.random.default_rng(73)
    path_len = np.array([len(named[n][5]) for n in names], np.int64)
    seq2, seq_off2 = relay(seq, seq_off, seq_len, ord("!"), 7, rng, (6, 0))
    events2, event_off2 = relay(events, event_off, n_events, np.nan, 5, rng, (6, 0))
    pairs2, pair_off2 = relay(np.ascontiguousarray(pairs, np.int32).view(np.int64).reshape(-1), pair_off, path_len, np.array([-1, -1], np.int32).view(np.int64)[0], 3, rng)
    assert seq_off2[6] == seq_off2[0] and event_off2[6] == event_off2[0] and seq_off2.min() == 7 and event_off2.min() == 5 and pair_off2.min() == 3
    n_kmers = seq_len.astype(np.int64) - A.K + 1
    map_off, total = scattered_room(n_kmers, 74)
    out = (np.full(total, -7, np.int32).repeat(2).view(abea.RANGE), np.frombuffer(bytes([0xa5]) * 40 * (len(names) + 1), abea.CALIB).copy())
    got = aligner.calibrate(seq2, seq_off2, seq_len, events2, event_off2, n_events, scale, shift, pairs2.view(np.int32).reshape(-1, 2), pair_off2, n_pairs, map_off=map_off, out=out)
    check((got[0], got[1], got[2][:len(names)]), [want[n] for n in names], names)
    assert out[1][:len(names)].tobytes() == plain[2].tobytes() and out[1][len(names):].tobytes() == bytes([0xa5]) * 40
    written = np.zeros(total, bool)
    for i, n in enumerate(names):
        assert out[0][map_off[i]:map_off[i] + n_kmers[i]].tobytes() == plain[0][plain[1][i]:plain[1][i] + n_kmers[i]].tobytes(), f"{n} (read {i})"
        written[map_off[i]:map_off[i] + n_kmers[i]] = True
    assert (out[0][~written].view(np.int32) == -7).all() and (~written).sum() >= 11 + len(names)


def test_a_flat_pore_model_sets_no_calibration_flag():
    from genarchbench_amd.abea import EventAligner
    rng = np.random.default_rng(2)
    mean, stdv = np.full(A.NKMER, 90.0, F), np.full(A.NKMER, 2.0, F)
    seq, ev, sc, sh, path = M.read_of_counts(rng, M.changing_bases(rng, 220), np.ones(220, np.int64), mean, stdv)
    want = M.calibrate(seq, ev, mean, stdv, sc, sh, path)
    assert np.isnan(want[0]["var"]) and want[0]["recalibrated"] == 1 and want[0]["read_stat_flag"] == 0
    h = EventAligner(mean, stdv)
    try:
        got = h.calibrate_reads([(seq, ev, sc, sh)], [path])
        check(got, [want])
        assert np.isnan(got[2][0]["var"]) and np.isnan(got[2][0]["log_var"]) and got[2][0]["read_stat_flag"] == 0
    finally:
        h.close()


def test_a_shuffled_mix_in_one_call_equals_each_read_alone(aligner, boundary):
    _, fixture, cases, _ = load_calib_fixture()
    named, want_b = boundary
    want_f, want_c = model_of_fixture()
    reads = list(fixture) + list(cases.values()) + list(named.values())
    want = list(want_f) + list(want_c.values()) + list(want_b.values())
    names = [f"fixture_{i}" for i in range(len(fixture))] + list(cases) + list(named)
    order = np.random.default_rng(67).permutation(len(reads))
    reads, want, names = [reads[i] for i in order], [want[i] for i in order], [names[i] for i in order]
    _, (rmap, map_off, res), _ = run(aligner, reads, want, names)
    for i, r in enumerate(reads):
        m1, _, r1 = aligner.calibrate(*flat_of([r]))
        assert r1[0].tobytes() == res[i].tobytes(), names[i]
        assert m1.tobytes() == rmap[map_off[i]:map_off[i] + m1.size].tobytes(), names[i]


def test_no_reads(aligner):
    rmap, map_off, res = aligner.calibrate(*flat_of([]))
    assert rmap.size == 0 and res.size == 0
    st = aligner.calibrate_last_stats()
    assert (st["reads"], st["recalibrated"], st["m_states"], st["kernel_ms"], st["total_ms"]) == (0, 0, 0, 0.0, 0.0)


def broken(flat, what):
    """the batch with one input rule broken in read 1"""
    seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pairs, pair_off, n_pairs = [np.array(a) for a in flat]
    o, n = int(pair_off[1]), int(n_pairs[1])
    n_kmers = int(seq_len[1]) - A.K + 1
    if what == "seq_len":
        seq_len[1] = 5
    elif what == "n_events":
        n_events[1] = 0
    elif what == "n_pairs_negative":
        n_pairs[1] = -1
    elif what == "n_pairs_large":
        n_pairs[1] = n_events[1] + n_kmers + 1
    elif what == "ref_pos_negative":
        pairs[o, 0] = -1
    elif what == "ref_pos_large":
        pairs[o + n - 1, 0] = n_kmers
    elif what == "read_pos_negative":
        pairs[o, 1] = -1
    elif what == "read_pos_large":
        pairs[o + n - 1, 1] = n_events[1]
    elif what == "ref_pos_decreasing":
        pairs[o + n // 2, 0] = pairs[o + n // 2 - 1, 0] - 1
    elif what == "read_pos_decreasing":
        pairs[o + n // 2, 1] = pairs[o + n // 2 - 1, 1] - 1
    return (seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pairs, pair_off, n_pairs)


RULES = ("seq_len", "n_events", "n_pairs_negative", "n_pairs_large", "ref_pos_negative", "ref_pos_large", "read_pos_negative", "read_pos_large",
         "ref_pos_decreasing", "read_pos_decreasing")


@pytest.mark.parametrize("what", RULES)
def test_a_broken_input_rule_is_refused_by_name_and_nothing_is_written(aligner, boundary, what):
    from genarchbench_amd import GabError, abea
    named, _ = boundary
    good = flat_of([named["kmers_65"], named["kmers_129"], named["kmers_64"]])
    assert good[10][1] > 8 and (np.diff(good[8][good[9][1]:good[9][1] + good[10][1]], axis=0) >= 0).all()
    flat = broken(good, what)
    out = (np.full(400, -7, np.int32).repeat(2).view(abea.RANGE), np.frombuffer(bytes([0xa5]) * 120, abea.CALIB).copy())
    with pytest.raises(GabError) as e:
        aligner.calibrate(*flat, out=out)
    assert e.value.code == -22 and "read 1" in str(e.value), str(e.value)
    assert (out[0].view(np.int32) == -7).all() and out[1].tobytes() == bytes([0xa5]) * 120
    with pytest.raises(GabError) as e:
        device_form(aligner, flat, canary=-7)
    assert e.value.code == -22 and "read 1" in str(e.value), str(e.value)
    rmap, _, res = device_form.last
    assert (rmap.view(np.int32) == -7).all() and res.tobytes() == bytes([0xf9]) * 120


def test_signal_to_calibrated_equals_the_chain_of_models(aligner):
    (mean, stdv, lstd), _, _, _ = load_calib_fixture()
    level_mean, reads, _ = load_events_fixture()
    four = sorted(range(len(reads)), key=lambda i: reads[i][0].size)[:4]
    ev = model_events_of_fixture()
    signals = [(reads[i][0].astype(F), reads[i][1], reads[i][2], reads[i][3]) for i in four]
    rmap, map_off, cal, pairs, pair_off, res, n_events = aligner.signal_to_calibrated(signals, [reads[i][4] for i in four])
    want = []
    for t, i in enumerate(four):
        sc, sh = E.scalings(reads[i][4], ev[i]["mean"], level_mean)
        rec, path = A.align(reads[i][4], ev[i]["mean"], mean, stdv, lstd, sc, sh)
        assert n_events[t] == ev[i]["mean"].size and {f: res[t][f].item() for f in rec} == rec, i
        want.append(M.calibrate(reads[i][4], ev[i]["mean"], mean, stdv, sc, sh, path[:rec["n_pairs"]]))
    check((rmap, map_off, cal), want)
    st = aligner.calibrate_last_stats()
    assert st["reads"] == 4 and st["m_states"] == sum(w[0]["n_m_state"] for w in want)
