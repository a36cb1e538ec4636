"""abea on the GPU: gab_abea_align / gab_abea_align_device against the model (tests/abea_model.py) on every field of gab_abea_read
and every pair of the path, bit for bit, and against the reference's recorded results on the golden fixture."""
import numpy as np
import pytest

import abea_model as M
from test_abea_model import load_fixture

pytestmark = pytest.mark.gpu
FIELDS = ("n_pairs", "path_len", "end_event", "max_gap", "flags", "avg_log_emission", "fills")


def _bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())


@pytest.fixture(scope="module")
def cases():
    """model, the named edge cases and the three long reads of the fixture, in shuffled order, with the model's answer for each"""
    rng = np.random.default_rng(11)
    (mean, stdv, lstd), fixture, _ = load_fixture()
    named = {}
    one = _bases(rng, 6)
    for n in (1, 2, 300):                                            # one k-mer
        named[f"one_kmer_{n}_events"] = (one, M.make_events(rng, one, mean, stdv, counts=[n]), 1.0, 0.0)
    named["under_100_bands_a"] = M.make_read(rng, 20, mean, stdv)    # clipped on all four sides
    named["under_100_bands_b"] = M.make_read(rng, 35, mean, stdv, counts=np.full(30, 1))
    s = _bases(rng, 45)
    named["bands_99"] = (s, M.make_events(rng, s, mean, stdv, counts=[2] * 17 + [1] * 23), 1.0, 0.0)      # 40 k-mers + 57 events + 2
    named["bands_100"] = (s, M.make_events(rng, s, mean, stdv, counts=[2] * 18 + [1] * 22), 1.0, 0.0)
    named["bands_101"] = (s, M.make_events(rng, s, mean, stdv, counts=[2] * 19 + [1] * 21), 1.0, 0.0)
    named["half_an_event_per_kmer"] = M.make_read(rng, 405, mean, stdv, counts=np.arange(400) % 2)
    named["five_events_per_kmer"] = M.make_read(rng, 150, mean, stdv, counts=np.full(145, 5))
    named["one_event_300_bases"] = (_bases(rng, 300), np.array([95.0], np.float32), 1.0, 0.0)
    named["no_end_nan_events"] = (_bases(rng, 80), np.full(120, np.nan, np.float32), 1.0, 0.0)
    named["gap_one_event_60_kmers"] = (_bases(rng, 65), np.array([95.0], np.float32), 1.0, 0.0)
    named["gap_run_of_55"] = M.make_gap_read(rng, mean, stdv)
    seq, ev, sc, sh = M.make_read(rng, 200, mean, stdv)
    named["wrong_shift"] = (seq, ev, sc, np.float32(sh + np.float32(15.0)))
    seq, ev, sc, sh = M.make_read(rng, 180, mean, stdv)
    named["non_acgt"] = (seq[:50] + b"N" + seq[51:90] + b"a" + seq[91:], ev, sc, sh)
    named["plain"] = M.make_read(rng, 260, mean, stdv)
    longs = sorted(range(len(fixture)), key=lambda i: -len(fixture[i][0]))[:3]
    for i in longs:
        named[f"long_{i}"] = fixture[i]
    names = list(named)
    names = [names[i] for i in rng.permutation(len(names))]
    reads = [named[n] for n in names]
    want = [M.align(r[0], r[1], mean, stdv, lstd, r[2], r[3]) for r in reads]
    return (mean, stdv, lstd), names, reads, want


@pytest.fixture(scope="module")
def aligner(cases):
    from genarchbench_amd.abea import EventAligner
    mean, stdv, lstd = cases[0]
    h = EventAligner(mean, stdv, lstd)
    yield h
    h.close()


def check(names, want, pairs, pair_off, res):
    for i, (name, (rec, path)) in enumerate(zip(names, want)):
        got = {f: res[i][f].item() for f in FIELDS}
        print(name, got)
        assert got == {f: rec[f] for f in FIELDS}, f"{name}: {got} != {rec}"      # avg_log_emission: equal doubles, bit for bit
        assert res[i]["pad"] == 0
        p = pairs[pair_off[i]:pair_off[i] + rec["path_len"]]
        assert np.array_equal(p["ref_pos"], path[:, 0]) and np.array_equal(p["read_pos"], path[:, 1]), name


def test_the_cases_cover_what_they_are_named_for(cases):
    _, names, reads, want = cases
    by = dict(zip(names, zip(reads, want)))
    bands = lambda n: len(by[n][0][0]) - M.K + 1 + len(by[n][0][1]) + 2
    assert [bands(n) for n in ("bands_99", "bands_100", "bands_101")] == [99, 100, 101] and bands("under_100_bands_a") < 100
    assert by["no_end_nan_events"][1][0]["flags"] == M.NO_END and by["one_event_300_bases"][1][0]["max_gap"] > 50
    assert by["gap_one_event_60_kmers"][1][0]["flags"] & M.GAP and by["wrong_shift"][1][0]["flags"] == M.LOW_EMISSION
    assert by["plain"][1][0]["flags"] == 0 and all(by[n][1][0]["flags"] == 0 for n in names if n.startswith("long_"))
    assert by["one_kmer_300_events"][1][0]["path_len"] >= 1


def test_host_call_equals_the_model_on_every_field_and_pair(cases, aligner):
    _, names, reads, want = cases
    pairs, pair_off, res = aligner.align_reads(reads)
    check(names, want, pairs, pair_off, res)
    st = aligner.last_stats()
    assert st["launches"] == 1 and st["cells"] == int(res["fills"].sum()) == sum(w[0]["fills"] for w in want)
    assert st["bands"] == sum(len(r[0]) - M.K + 1 + len(r[1]) + 2 for r in reads) and 0 < st["kernel_ms"] <= st["total_ms"]


def test_each_case_alone_equals_the_model(cases, aligner):
    _, names, reads, want = cases
    for name, r, w in zip(names, reads, want):
        if not name.startswith("long_"):
            pairs, pair_off, res = aligner.align_reads([r])
            check([name], [w], pairs, pair_off, res)


def test_a_small_trace_budget_cuts_the_call_into_launches_with_the_same_output(cases, aligner, monkeypatch):
    _, names, reads, want = cases
    first = aligner.align_reads(reads)
    monkeypatch.setenv("GAB_ABEA_TRACE_BYTES", str(32 * 9000))       # a long read (about 8400 bands) fills a launch
    pairs, pair_off, res = aligner.align_reads(reads)
    assert aligner.last_stats()["launches"] >= 3
    check(names, want, pairs, pair_off, res)
    assert res.tobytes() == first[2].tobytes()
    monkeypatch.delenv("GAB_ABEA_TRACE_BYTES")
    pairs, pair_off, res = aligner.align_reads(reads[:5])            # two calls on one handle are independent
    assert aligner.last_stats()["launches"] == 1
    check(names[:5], want[:5], pairs, pair_off, res)


def test_device_call_with_torch_tensors_equals_the_host_call(cases, aligner):
    import torch
    from genarchbench_amd import abea
    _, names, reads, want = cases
    packed = abea.pack_reads(reads)
    host_pairs, pair_off, host_res = aligner.align(*packed)
    dev = [torch.from_numpy(a).cuda() for a in packed]
    room = int((pair_off + abea.pair_room(packed[2], packed[5])).max())
    pairs = torch.full((room, 2), -1, dtype=torch.int32, device="cuda")
    res = torch.zeros(len(reads) * abea.READ.itemsize, dtype=torch.uint8, device="cuda")
    aligner.align_device(*dev[:8], pairs, dev[8], res)
    got_res = res.cpu().numpy().view(abea.READ)
    got_pairs = pairs.cpu().numpy().reshape(-1).view(abea.PAIR)
    assert got_res.tobytes() == host_res.tobytes()
    check(names, want, got_pairs, pair_off, got_res)
    assert aligner.last_stats()["cells"] == int(got_res["fills"].sum())


def test_the_golden_fixture_equals_the_reference(aligner):
    _, reads, exp = load_fixture()
    pairs, pair_off, res = aligner.align_reads(reads)
    for i, want in enumerate(exp["reads"]):
        p = pairs[pair_off[i]:pair_off[i] + res[i]["path_len"]]
        path = np.stack([p["ref_pos"], p["read_pos"]], 1)
        assert (int(res[i]["n_pairs"]), int(res[i]["path_len"]), M.pairs_digest(path)) == (want["n_pairs"], want["path_len"], want["pairs"]), i


def test_bad_reads_are_refused_by_name(cases, aligner):
    from genarchbench_amd import GabError
    _, names, reads, _ = cases
    for bad in ((b"ACGTA", np.ones(3, np.float32), 1.0, 0.0), (b"ACGTACGT", np.zeros(0, np.float32), 1.0, 0.0)):
        with pytest.raises(GabError) as e:
            aligner.align_reads([reads[0], bad])
        assert e.value.code == -22 and "read 1" in str(e.value)
