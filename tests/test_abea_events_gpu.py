"""abea's event detection and scaling estimate on the GPU: gab_abea_events / gab_abea_scalings and their device forms against the
model (tests/abea_events_model.py) on every output array and count, bit for bit (NaNs by bit pattern), against the reference's
recorded results on the golden fixture and on the case fixture (tests/golden/abea_events_cases.npz), and the counters that show which route a read's sums and a chunk's detector took."""
import numpy as np
import pytest

import abea_events_cases as CASES
import abea_events_model as M
import abea_model as A
from abea_events_cases import signal
from test_abea_events_model import load_events_fixture, model_events_of_case_fixture, model_events_of_fixture
from test_abea_model import load_fixture

pytestmark = pytest.mark.gpu
F = np.float32
ARRAYS = ("mean", "stdv", "start", "length")


@pytest.fixture(scope="module")
def aligner():
    from genarchbench_amd.abea import EventAligner
    mean, stdv, lstd = load_fixture()[0]
    h = EventAligner(mean, stdv, lstd)
    yield h
    h.close()


@pytest.fixture(scope="module")
def level_mean():
    return load_fixture()[0][0]


def model_of(s):
    return M.events_of(*s)


def check_events(got, want, names=None):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        name = names[i] if names else i
        assert g["mean"].size == w["mean"].size, f"{name}: {g['mean'].size} events, the model has {w['mean'].size}"
        for a in ARRAYS:
            assert g[a].dtype == w[a].dtype and g[a].tobytes() == w[a].tobytes(), f"{name}: {a}"


def run(aligner, signals, want=None, names=None):
    got = aligner.detect_events(signals)
    check_events(got, [model_of(s) for s in signals] if want is None else want, names)
    st = aligner.events_last_stats()
    assert st["samples"] == sum(s[0].size for s in signals) and st["events"] == sum(g["mean"].size for g in got)
    return got, st


@pytest.fixture(scope="module")
def shape():
    from genarchbench_amd import abea
    return abea.events_shape()


@pytest.fixture(scope="module")
def mixed(level_mean, shape):
    """37 reads of every kind in shuffled order (tests/abea_events_cases.py), with the model's answer for each"""
    names, signals, _ = CASES.mixed_cases(level_mean, *shape)
    return names, signals, [model_of(s) for s in signals]


def test_tiny_reads_and_the_read_without_a_peak(aligner, mixed):
    names, signals, want = mixed
    tiny = [i for i, n in enumerate(names) if n.startswith("tiny_") or n == "flat_read"]
    assert len(tiny) == 9 and any(want[i]["peaks"] == [] for i in tiny) and want[names.index("tiny_1")]["length"].tolist() == [1.0]
    got, st = run(aligner, [signals[i] for i in tiny], [want[i] for i in tiny], [names[i] for i in tiny])
    assert st["reads_serial_sums"] == 0 and st["chunks"] == 9 and st["chunks_redone"] == 0
    for i in tiny:                                                    # and each alone
        run(aligner, [signals[i]], [want[i]], [names[i]])


def test_reads_around_the_chunk_size(aligner, mixed, shape):
    names, signals, want = mixed
    chunk, warmup = shape
    pick = [names.index(f"chunk_{n}") for n in (chunk - 1, chunk, chunk + 1, 2 * chunk + warmup)]
    _, st = run(aligner, [signals[i] for i in pick], [want[i] for i in pick], [names[i] for i in pick])
    assert st["chunks"] == 1 + 1 + 2 + 3 and st["reads_serial_sums"] == 0


def test_a_flat_run_across_a_boundary_is_redone_and_a_plain_read_is_not(aligner, mixed, shape, level_mean):
    names, signals, want = mixed
    chunk, warmup = shape
    i = names.index("flat_run")
    t1, t2 = want[i]["tstat"]
    redo = M.chunks_to_redo(t1, t2, chunk, warmup)
    assert redo >= 1
    _, st = run(aligner, [signals[i]], [want[i]], ["flat_run"])
    assert st["chunks_redone"] == redo > 0 and st["chunks"] == 3
    plain = signal(M.make_signal(np.random.default_rng(77), signals[i][0].size, level_mean))
    w = model_of(plain)
    assert M.chunks_to_redo(*w["tstat"], chunk, warmup) == 0
    _, st = run(aligner, [plain], [w], ["plain"])
    assert st["chunks_redone"] == 0 and st["chunks"] == 3


def test_reads_whose_sums_must_be_added_in_order(aligner, mixed):
    names, signals, want = mixed
    planted = [i for i, n in enumerate(names) if n.startswith("planted_")]
    assert len(planted) == 4 and not any(M.sums_are_wide(M.to_pa(*signals[i])) for i in planted)
    for i in planted:
        _, st = run(aligner, [signals[i]], [want[i]], [names[i]])
        assert st["reads_serial_sums"] == 1
    wide = names.index("chunk_1025") if "chunk_1025" in names else 0
    both = planted + [wide]
    _, st = run(aligner, [signals[i] for i in both], [want[i] for i in both], [names[i] for i in both])
    assert st["reads_serial_sums"] == 4


def test_a_peak_near_the_end_whose_event_is_the_last(aligner, level_mean):
    rng = np.random.default_rng(9)
    codes, rg, dg, of, _ = M.make_signal(rng, 700, level_mean)
    codes = codes.copy(); codes[-5:] += 300                           # a step five samples before the end
    s = (codes.astype(F), rg, dg, of)
    w = model_of(s)
    assert w["peaks"][-1] == 695 and w["start"][-1] == 695 and w["length"][-1] == 5.0
    run(aligner, [s], [w], ["step_at_the_end"])


def device_form(aligner, signals, want, names):
    """the device entry on torch tensors: counts, offsets, total, the four slabs against `want`, and nothing behind the events"""
    import torch
    from genarchbench_amd import abea
    packed = abea.pack_signals(signals)
    dev = [torch.from_numpy(a).cuda() for a in packed]
    n, total = len(signals), sum(w["mean"].size for w in want)
    n_events = torch.zeros(n, dtype=torch.int32, device="cuda"); event_off = torch.zeros(n, dtype=torch.int64, device="cuda")
    slabs = [torch.full((total + 16,), -7, dtype=dt, device="cuda") for dt in (torch.float32, torch.float32, torch.int32, torch.float32)]
    tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert aligner.detect_events_device(*dev, n_events, event_off, *slabs, tot, event_cap=total) == 0
    ne, eo = n_events.cpu().numpy(), event_off.cpu().numpy()
    assert int(tot.item()) == total and ne.tolist() == [w["mean"].size for w in want] and eo.tolist() == np.concatenate([[0], np.cumsum(ne)[:-1]]).tolist()
    host = [a.cpu().numpy() for a in slabs]
    got = [dict(zip(ARRAYS, (a[o:o + k] for a in host))) for o, k in zip(eo, ne)]
    check_events(got, want, names)
    assert all((a[total:] == -7).all() for a in host)                 # nothing behind the events
    return got


def test_the_mixed_batch_in_host_and_device_form(aligner, mixed, shape):
    names, signals, want = mixed
    _, st = run(aligner, signals, want, names)
    redo = sum(M.chunks_to_redo(*w["tstat"], *shape) for w in want)
    assert st["reads_serial_sums"] == 4 and st["chunks_redone"] == redo >= 1
    assert st["chunks"] == sum(-(-s[0].size // shape[0]) for s in signals)
    device_form(aligner, signals, want, names)
    st2 = aligner.events_last_stats()
    assert {k: st2[k] for k in ("samples", "events", "reads_serial_sums", "chunks", "chunks_redone")} == {k: st[k] for k in ("samples", "events", "reads_serial_sums", "chunks", "chunks_redone")}
    assert 0 < st2["sums_ms"] and 0 < st2["detect_ms"] and 0 < st2["fill_ms"] and st2["kernel_ms"] <= st2["total_ms"] * 1.001


def test_no_reads(aligner):
    from genarchbench_amd import abea
    rc, n_events, event_off, total, *_ = aligner.events(*abea.pack_signals([]))
    assert rc == 0 and total == 0 and n_events.size == 0
    assert aligner.events_last_stats()["samples"] == 0
    assert aligner.estimate_scalings([])[0].size == 0


def test_slabs_one_event_short(aligner, mixed):
    import torch
    from genarchbench_amd import abea
    names, signals, want = mixed
    signals, want = signals[:9], want[:9]
    total = sum(w["mean"].size for w in want)
    packed = abea.pack_signals(signals)
    slabs = (np.full(total + 8, -7, F), np.full(total + 8, -7, F), np.full(total + 8, -7, np.int32), np.full(total + 8, -7, F))
    rc, n_events, event_off, tot, *_ = aligner.events(*packed, event_cap=total - 1, slabs=slabs)
    assert rc == abea.ERANGE and tot == total and n_events.tolist() == [w["mean"].size for w in want]
    assert event_off.tolist() == np.concatenate([[0], np.cumsum(n_events)[:-1]]).tolist() and all((a == -7).all() for a in slabs)
    dev = [torch.from_numpy(a).cuda() for a in packed]
    d_ne = torch.zeros(9, dtype=torch.int32, device="cuda"); d_eo = torch.zeros(9, dtype=torch.int64, device="cuda"); d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_slabs = [torch.from_numpy(a).cuda() for a in slabs]
    assert aligner.detect_events_device(*dev, d_ne, d_eo, *d_slabs, d_tot, event_cap=total - 1) == abea.ERANGE
    assert int(d_tot.item()) == total and d_ne.cpu().numpy().tolist() == n_events.tolist() and d_eo.cpu().numpy().tolist() == event_off.tolist()
    assert all(bool((a == -7).all().item()) for a in d_slabs)         # the canaries, those behind event_cap included
    rc, *_ = aligner.events(*packed, event_cap=total, slabs=slabs)    # and with exactly enough room
    assert rc == 0 and all((a[total:] == -7).all() for a in slabs)
    check_events([dict(zip(ARRAYS, (a[o:o + k] for a in slabs))) for o, k in zip(event_off, n_events)], want)


def test_bad_reads_are_refused_by_name(aligner, mixed):
    from genarchbench_amd import GabError
    _, signals, _ = mixed
    for bad in ((np.zeros(0, F), 1.0, 1.0, 0.0), (np.ones(20, F), 1.0, 0.0, 0.0)):
        with pytest.raises(GabError) as e:
            aligner.detect_events([signals[0], bad])
        assert e.value.code == -22 and "read 1" in str(e.value)
    with pytest.raises(GabError) as e:
        aligner.estimate_scalings([(b"ACGTACGT", np.ones(4, F)), (b"ACGTA", np.ones(4, F))])
    assert e.value.code == -22 and "read 1" in str(e.value)


def test_the_golden_fixture_equals_the_reference(aligner, level_mean):
    _, reads, exp = load_events_fixture()
    got, st = run(aligner, [signal(r) for r in reads], model_events_of_fixture())
    assert st["reads_serial_sums"] == 0 and st["chunks_redone"] == 0 and st["events"] == exp["events"] and st["samples"] == exp["samples"]
    for i, (g, want) in enumerate(zip(got, exp["reads"])):
        assert (g["mean"].size, M.events_digest(g)) == (want["n_events"], want["events"]), i
    scale, shift = aligner.estimate_scalings([(r[4], g["mean"]) for r, g in zip(reads, got)])
    assert [float(x).hex() for x in scale] == [w["scale"] for w in exp["reads"]]
    assert [float(x).hex() for x in shift] == [w["shift"] for w in exp["reads"]]
    st = check_scalings(aligner, [(r[4], g["mean"]) for r, g in zip(reads, got)], level_mean)
    assert st["event_sums_in_order"] == 0 and st["kmer_sums_in_order"] == 0      # (the squares of arbitrary floats need more than 53 bits)


def test_scalings_edge_cases(aligner, level_mean):
    # 20 000 events: the order of addition shows in the sum of the squared double differences, and for events of every magnitude
    # in the plain sum too
    reads, many, wild = CASES.scalings_edge_cases()
    d = many.astype(np.float64) - 0.123456789
    assert M.pairwise_sum(d * d) != np.add.accumulate(d * d)[-1]
    assert M.pairwise_sum(wild.astype(np.float64)) != np.add.accumulate(wild.astype(np.float64))[-1]
    check_scalings(aligner, reads, level_mean)
    scale, _ = aligner.estimate_scalings(reads[:1])
    assert scale[0] == 1.0                                            # one event on one k-mer: the shift takes all of the difference
    routes = [M.scalings_in_order(s, e, level_mean) for s, e in reads]
    assert routes[2] == (False, False, True) and routes[3][0]         # the plain sum of 20 000 wild events must go in order, that of the tame ones not


def check_scalings(h, reads, level_mean):
    """results equal to the model bit for bit, and the counters of the sums added in order equal to the model's proof per read"""
    scale, shift = h.estimate_scalings(reads)
    for i, (s, e) in enumerate(reads):
        sc, sh = M.scalings(s, e, level_mean)
        assert (F(sc).tobytes(), F(sh).tobytes()) == (scale[i].tobytes(), shift[i].tobytes()), i
    routes = np.array([M.scalings_in_order(s, e, level_mean) for s, e in reads], np.int64).reshape(-1, 3)
    st = h.scalings_last_stats()
    assert (st["reads"], st["event_sums_in_order"], st["kmer_sums_in_order"], st["kmer_sq_sums_in_order"]) == (len(reads), *routes.sum(0).tolist()), st
    return st


def test_scalings_take_every_route(level_mean):
    """a pore model on a grid of 1/4 pA makes the sum of squared levels provable too; one with a level of 1e-30 forces the two
    k-mer sums of a read that has that k-mer into the reference's order"""
    from genarchbench_amd.abea import EventAligner
    stdv = np.full(A.NKMER, 2.0, F)
    reads = CASES.scalings_route_cases()
    coarse, tiny = (CASES.route_models(level_mean)[m] for m in ("coarse", "tiny"))
    h = EventAligner(coarse, stdv)
    st = check_scalings(h, reads, coarse)
    assert (st["event_sums_in_order"], st["kmer_sums_in_order"], st["kmer_sq_sums_in_order"]) == (0, 0, 0)
    h.close()
    h = EventAligner(tiny, stdv)
    st = check_scalings(h, reads, tiny)
    assert (st["event_sums_in_order"], st["kmer_sums_in_order"], st["kmer_sq_sums_in_order"]) == (0, 1, 2)
    h.close()


def test_signal_to_pairs_equals_the_model_aligned_on_the_references_events(aligner):
    (mean, stdv, lstd), _, _ = load_fixture()
    _, reads, exp = load_events_fixture()
    ten = sorted(range(len(reads)), key=lambda i: reads[i][0].size)[:10]
    ev = model_events_of_fixture()                                    # equal to the reference's by the recorded digests
    for i in ten:
        assert M.events_digest(ev[i]) == exp["reads"][i]["events"]
    pairs, pair_off, res, n_events, scale, shift = aligner.signal_to_pairs([signal(reads[i]) for i in ten], [reads[i][4] for i in ten])
    for t, i in enumerate(ten):
        w = exp["reads"][i]
        sc, sh = F(float.fromhex(w["scale"])), F(float.fromhex(w["shift"]))
        assert n_events[t] == w["n_events"] and (scale[t], shift[t]) == (sc, sh)
        rec, path = A.align(reads[i][4], ev[i]["mean"], mean, stdv, lstd, sc, sh)
        got = {f: res[t][f].item() for f in rec}
        assert got == rec, f"read {i}: {got} != {rec}"
        p = pairs[pair_off[t]:pair_off[t] + rec["path_len"]]
        assert np.array_equal(p["ref_pos"], path[:, 0]) and np.array_equal(p["read_pos"], path[:, 1]), i


# ---- the case fixture: the reference's record of the constructed reads --------------------------------------------------------------
@pytest.fixture(scope="module")
def case_fixture():
    """abea_events_cases.npz: level_mean, signals (with their bases), scalings reads, the reference's record, the model's event tables"""
    lm, signals, given, exp = CASES.load_cases()
    return lm, signals, given, exp, model_events_of_case_fixture()


def against_the_reference(got, exp):
    for g, want in zip(got, exp["reads"]):
        if want["name"] not in exp["undefined_in_reference"]:         # (the flat read, which the reference refuses: model only)
            assert (g["mean"].size, M.events_digest(g)) == (want["n_events"], want["events"]), want["name"]


def test_the_case_fixture_equals_the_reference_and_the_model_in_host_and_device_form(aligner, case_fixture, shape):
    """the reads around the chunk size, the flat run that makes a chunk run again, the four planted reads whose sums go in order, reads
    of 1000 and 1001 samples, two square waves: the four arrays and n_events of every read against the reference's digest and against
    the model, in one host call and in the device form, with the route counters"""
    _, signals, _, exp, want = case_fixture
    names = [r["name"] for r in exp["reads"]][:len(signals)]
    sigs = [s[:4] for s in signals]
    got, st = run(aligner, sigs, want, names)
    against_the_reference(got, exp)
    redo = sum(M.chunks_to_redo(*w["tstat"], *shape) for w in want)
    assert st["reads_serial_sums"] == sum(n.startswith("planted_") for n in names) == 4 and st["chunks_redone"] == redo >= 1
    assert st["chunks"] == sum(-(-s[0].size // shape[0]) for s in sigs)
    against_the_reference(device_form(aligner, sigs, want, names), exp)
    st2 = aligner.events_last_stats()
    assert all(st2[k] == st[k] for k in ("samples", "events", "reads_serial_sums", "chunks", "chunks_redone"))


def test_the_scalings_of_the_case_fixture_equal_the_reference(aligner, case_fixture, level_mean):
    """scale and shift of every read the reference accepted, on the events the library detects, and of the scaling edge cases; then the
    two reads of the extra pore models (levels on a grid of 1/4 pA; a level of 1e-30) on handles of their own"""
    from genarchbench_amd.abea import EventAligner
    lm, signals, given, exp, _ = case_fixture
    assert lm.tobytes() == level_mean.tobytes()
    got = aligner.detect_events([s[:4] for s in signals])
    reads = [(s[4], g["mean"]) for s, g in zip(signals, got)] + given
    records = exp["reads"]
    assert len(reads) == len(records)
    main = [i for i, w in enumerate(records) if w["pore_model"] == "level_mean" and w["name"] not in exp["undefined_in_reference"]]
    scale, shift = aligner.estimate_scalings([reads[i] for i in main])
    assert [float(x).hex() for x in scale] == [records[i]["scale"] for i in main]
    assert [float(x).hex() for x in shift] == [records[i]["shift"] for i in main]
    # ... and against the model bit for bit, with the counters of the sums added in order, where the result is a number (the reads with
    # a planted NaN or inf give a NaN, whose sign no rule fixes: the record above, "nan", is all the reference says of it)
    numbers = [i for i in main if "nan" not in (records[i]["scale"], records[i]["shift"])]
    assert len(numbers) == len(main) - 2
    check_scalings(aligner, [reads[i] for i in numbers], level_mean)
    for name, model in CASES.route_models(level_mean).items():
        pick = [i for i, w in enumerate(records) if w["pore_model"] == name]
        assert len(pick) == 2
        h = EventAligner(model, np.full(A.NKMER, 2.0, F))
        scale, shift = h.estimate_scalings([reads[i] for i in pick])
        h.close()
        assert [float(x).hex() for x in scale] == [records[i]["scale"] for i in pick]
        assert [float(x).hex() for x in shift] == [records[i]["shift"] for i in pick]
