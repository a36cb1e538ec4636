"""GPU: the minimizer index in key-space partitions, built in two phases (gab_kmer_index_part_begin / _finish, through
genarchbench_amd.kmer), against the sequential model of tests/minimizer_model.py restricted to every partition
(tests/minimizer_parts_util.py) and, merged, against the reference's recorded index digests.  N handles on one device stand for N
GPUs.  Every comparison is equality; every output buffer is pre-filled with a sentinel by the Python mirror."""
import functools
import json

import numpy as np
import pytest

from tests import kmer_model, minimizer_model as mm, minimizer_parts_util as pu
from tests.kmer_parts_util import np_part_of
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

EXPECTED = json.load(open(f"{GOLDEN}/kmer_minimizer_expected.json"))
MIN_LEN = EXPECTED["min_len_exclusive"]
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
EINVAL = -22
RUN, TILE = 64, 4096        # GAB_KMER_RUN; a wave's tile of 64 runs
POINTS = [(15, 10), (11, 5), (17, 19)]
RATES = (100, 3)
NPARTS = (2, 3, 5)


def rand(seed, n):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


@functools.lru_cache(maxsize=None)
def reads_of(name):
    return kmer_model.load_reads([f"{GOLDEN}/{name}"])


@functools.lru_cache(maxsize=None)
def entries_of(name, k, window):
    return mm.entries(reads_of(name), k, window, MIN_LEN)      # (the reference: computed once, shared by the rates and the partition counts)


@pytest.fixture(scope="module")
def handles():
    """five handles on device 0: partitions 0 .. N - 1 of a build live side by side, as on N GPUs"""
    from genarchbench_amd.kmer import KmerCounter
    hs = [KmerCounter() for _ in range(5)]
    yield hs
    for h in hs:
        h.close()


@pytest.fixture(scope="module")
def kc(handles):
    return handles[0]


def check_dump_and_lookup(h, mp, others):
    """the handle's dump and look-ups == the model mp of its partition; others: k-mers that other partitions own"""
    kmers, start, gpos = h.index_dump()
    np.testing.assert_array_equal(kmers, mp["kmers"])
    np.testing.assert_array_equal(start, mp["start"])
    np.testing.assert_array_equal(gpos, mp["gpos"])
    if mp["kmers"].size:
        first, count, rep = h.index_lookup(mp["kmers"])
        np.testing.assert_array_equal(first, mp["start"][:-1])
        np.testing.assert_array_equal(count, np.diff(mp["start"]))
        assert not rep.any()
    if mp["repetitive"].size:
        first, count, rep = h.index_lookup(mp["repetitive"])
        assert (first == -1).all() and (count == 0).all() and (rep == 1).all()
    if others.size:
        first, count, rep = h.index_lookup(others)
        assert (first == -1).all() and (count == 0).all() and (rep == 0).all()
    return kmers, start, gpos


def build_parts(hs, reads, k, w, rate, nparts, min_len=0, found=None, retried=0):
    """both phases on handles hs[0 .. nparts): every reported field, dump and look-up against the restricted model -> (models, dumps)"""
    found = found if found is not None else mm.entries(reads, k, w, min_len)
    parts = pu.restrict(found, rate, nparts)
    begun = [hs[p].index_part_begin(reads, k, w, p, nparts, min_len) for p in range(nparts)]
    assert begun == [pu.begin_fields(mp) for mp in parts]
    M, U = sum(b["minimizers"] for b in begun), sum(b["distinct"] for b in begun)
    assert (M, U) == (int(found[0].size), int(np.unique(found[0]).size))
    done = [hs[p].index_part_finish(M, U, rate) for p in range(nparts)]
    assert done == [pu.fields(mp) for mp in parts]
    dumps = []
    for p in range(nparts):
        others = np.concatenate([np.concatenate([parts[q]["kmers"][:40], parts[q]["repetitive"][:40]]) for q in range(nparts) if q != p] + [np.zeros(0, np.uint64)])
        dumps.append(check_dump_and_lookup(hs[p], parts[p], others))
        lp = hs[p].index_last_part()
        assert (lp["part"], lp["nparts"], lp["retried"]) == (p, nparts, retried)
        ph = hs[p].index_last_phases()
        assert ph["sketch_ms"] > 0 and ph["count_ms"] > 0 and ph["fill_ms"] >= 0 and ph["sort_ms"] >= 0
    return parts, dumps


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nparts", NPARTS)
@pytest.mark.parametrize("k,window", POINTS)
@pytest.mark.parametrize("name", sorted(EXPECTED["files"]))
def test_golden_partitions(handles, name, k, window, nparts):
    reads = reads_of(name)
    slots = pu.first_table_slots(pu.positions_of(reads, k, MIN_LEN), k, nparts)
    for rate in RATES:
        row = next(r for r in EXPECTED["files"][name]["rows"] if (r["k"], r["window"], r["rate"]) == (k, window, rate))
        parts, dumps = build_parts(handles[:nparts], reads, k, window, rate, nparts, MIN_LEN, entries_of(name, k, window))
        assert mm.digest(*pu.merge(dumps)) == row["index_sha256"]
        assert {f: pu.sum_fields(parts)[f] for f in mm.FIELDS if f in row} == {f: row[f] for f in mm.FIELDS if f in row}
        assert [h.index_last_part()["table_slots"] for h in handles[:nparts]] == [slots] * nparts      # (the first table: no repeat)


# ---- 2. nparts = 1 --------------------------------------------------------------------------------------------------------------------
def test_one_partition_is_the_unpartitioned_build(handles):
    reads = [rand(80, 6000), b"C" * 300, rand(81, TILE + 70)]
    for k, w, rate in ((15, 5, 100), (11, 19, 3)):
        want = handles[1].index_minimizers(reads, k, w, rate, 0)
        want_dump = handles[1].index_dump()
        begun = handles[0].index_part_begin(reads, k, w, 0, 1, 0)
        assert begun == dict({f: 0 for f in mm.FIELDS}, **{f: want[f] for f in ("reads_kept", "total_len", "minimizers", "distinct")})
        assert handles[0].index_part_finish(begun["minimizers"], begun["distinct"], rate) == want
        for a, b in zip(handles[0].index_dump(), want_dump):
            np.testing.assert_array_equal(a, b)
        assert handles[0].index_last_part() == handles[1].index_last_part() and handles[0].index_last_part()["nparts"] == 1


# ---- 3. the threshold is the whole input's ---------------------------------------------------------------------------------------------
def _rate_for(total, unique, want):
    mean = np.float32(total) / np.float32(unique + 1)
    rate = float(np.float32((want + 0.5) / float(mean)))
    assert mm.repetitive_frequency(total, unique, rate) == want
    return rate


@pytest.mark.parametrize("nparts", NPARTS)
def test_global_threshold_on_the_poly_a_key(handles, nparts):
    """capacity 137 of the poly-A key: at a global threshold of 136 it goes, although the totals of the partition that owns it alone
    would give a threshold above 137 (tests/test_kmer_index_parts_model.py) -- a build that filters with local totals keeps it"""
    from genarchbench_amd.kmer import repetitive_frequency
    k, w = 15, 5
    reads = [rand(8, 900) + b"A" * 700 + rand(9, 800), rand(10, 1200)]
    found = mm.entries(reads, k, w, 0)
    M, U = int(found[0].size), int(np.unique(found[0]).size)
    cap = int(np.unique(found[0], return_counts=True)[1].max())
    owner = int(np_part_of(np.zeros(1, np.uint64), nparts)[0])
    for want, kept in ((cap, True), (cap - 1, False)):
        rate = _rate_for(M, U, want)
        assert repetitive_frequency(M, U, rate) == want
        parts, dumps = build_parts(handles[:nparts], reads, k, w, rate, nparts, 0, found)
        assert [mp["repetitive_frequency"] for mp in parts] == [want] * nparts
        assert (0 in parts[owner]["kmers"].tolist()) == kept and (0 in parts[owner]["repetitive"].tolist()) == (not kept)
        first, count, rep = handles[owner].index_lookup(np.array([0, (1 << 30) - 1], np.uint64))      # poly-A and poly-T
        assert rep.tolist() == [0 if kept else 1] * 2 and count.tolist() == [cap if kept else 0] * 2


# ---- 4. empty partitions, empty inputs ---------------------------------------------------------------------------------------------------
def test_64_partitions_of_one_short_read(kc):
    k, w, nparts = 15, 5, 64
    reads = [rand(5, 60)]
    found = mm.entries(reads, k, w, 0)
    parts = pu.restrict(found, 100, nparts)
    M, U = int(found[0].size), int(np.unique(found[0]).size)
    empty = [p for p in range(nparts) if parts[p]["distinct"] == 0]
    assert len(empty) >= 40 and len(empty) < nparts - 1
    dumps = []
    for p in range(nparts):          # one handle, partition after partition (finish needs only the two sums, known from the model)
        assert kc.index_part_begin(reads, k, w, p, nparts, 0) == pu.begin_fields(parts[p])
        assert kc.index_part_finish(M, U, 100) == pu.fields(parts[p])
        dumps.append(check_dump_and_lookup(kc, parts[p], found[0][np_part_of(found[0], nparts) != p]))
        if p in empty:
            assert dumps[-1][0].size == 0 and dumps[-1][1].tolist() == [0] and dumps[-1][2].size == 0
    whole = mm.index_of_entries(found, 100)
    for a, b in zip(pu.merge(dumps), (whole["kmers"], whole["start"], whole["gpos"])):
        np.testing.assert_array_equal(a, b)


def test_empty_inputs_and_rate_zero(handles):
    zeros = {f: 0 for f in mm.FIELDS}
    for reads, min_len, kept, total in (([], 0, 0, 0), ([rand(1, 100)], 5000, 0, 0), ([rand(1, 10), b""], 0, 1, 10)):
        for p in range(3):
            assert handles[p].index_part_begin(reads, 15, 5, p, 3, min_len) == dict(zeros, reads_kept=kept, total_len=total)
        for p in range(3):
            assert handles[p].index_part_finish(0, 0, 100) == dict(zeros, reads_kept=kept, total_len=total)
            kmers, start, gpos = handles[p].index_dump()
            assert kmers.size == 0 and start.tolist() == [0] and gpos.size == 0
            first, count, rep = handles[p].index_lookup(np.array([5], np.uint64))
            assert (first[0], count[0], rep[0]) == (-1, 0, 0)
    parts, dumps = build_parts(handles[:3], [rand(4, 2000)], 15, 5, 0.0, 3)
    assert all(mp["selected_kmers"] == 0 and mp["filtered_entries"] == mp["minimizers"] > 0 for mp in parts)
    assert all(d[0].size == 0 and d[1].tolist() == [0] and d[2].size == 0 for d in dumps)


# ---- 5. a long list inside a partition ---------------------------------------------------------------------------------------------------
def test_a_long_list_in_a_partition_comes_out_sorted(handles):
    k, w = 13, 4
    rng = np.random.default_rng(21)
    unit = rand(22, 40)
    reads = []
    for i in range(30):
        r = rand(100 + i, int(rng.integers(50, 400))) + unit * int(rng.integers(20, 90)) + rand(200 + i, 100)
        reads.append(r.translate(COMP)[::-1] if i % 2 else r)
    parts, dumps = build_parts(handles[:3], reads, k, w, 1e6, 3)
    assert max(int(np.diff(mp["start"]).max()) for mp in parts) > 500


# ---- 6. run and tile boundaries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 10])
def test_reads_that_end_on_run_and_tile_boundaries(handles, w):
    k = 15
    npos = [RUN - 1, RUN, RUN + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + RUN]
    reads = [rand(1000 + i, n + k) for i, n in enumerate(npos)]
    build_parts(handles[:2], reads, k, w, 100, 2)


# ---- 7. the repeat path ------------------------------------------------------------------------------------------------------------------
def test_a_full_first_table_repeats_the_capacity_pass(monkeypatch):
    """GAB_KMER_PART_FLOOR=1: the first table of a partition is the 16-line floor, 128 slots for hundreds of keys"""
    from genarchbench_amd.kmer import KmerCounter, table_slots
    k, w, nparts = 15, 5, 3
    reads = [rand(300, 6000)]
    found = mm.entries(reads, k, w, 0)
    assert min(mp["distinct"] for mp in pu.restrict(found, 100, nparts)) > 128
    for floor, retried in (("1", 1), (None, 0)):
        if floor:
            monkeypatch.setenv("GAB_KMER_PART_FLOOR", floor)
        else:
            monkeypatch.delenv("GAB_KMER_PART_FLOOR", raising=False)
        hs = [KmerCounter() for _ in range(nparts)]      # (fresh handles: the knob is read when a handle is made)
        try:
            build_parts(hs, reads, k, w, 100, nparts, 0, found, retried=retried)
            want_slots = table_slots(6000 - k, k, 1 if retried else nparts)
            assert [h.index_last_part()["table_slots"] for h in hs] == [want_slots] * nparts
        finally:
            for h in hs:
                h.close()


# ---- 8. state machine and arguments ------------------------------------------------------------------------------------------------------
def einval(call, word=None):
    from genarchbench_amd.kmer import GabError
    with pytest.raises(GabError) as e:
        call()
    assert e.value.code == EINVAL and (word is None or word in str(e.value)), str(e.value)


def test_handle_states():
    from genarchbench_amd.kmer import KmerCounter
    reads = [rand(40, 3000)]
    k, w = 15, 5
    m = mm.build_index(reads, k, w, 100, 0)
    M, U = m["minimizers"], m["distinct"]
    h = KmerCounter()
    try:
        accessors = (h.index_dump, lambda: h.index_lookup(np.zeros(1, np.uint64)), h.index_last_phases, h.index_last_part,
                     lambda: h.spectrum(8), lambda: h.query(np.zeros(1, np.uint64)), h.dump, h.last_stats, h.last_part)
        einval(lambda: h.index_part_finish(M, U, 100), "no pending")             # before any begin
        own = h.index_part_begin(reads, k, w, 1, 2, 0)
        for call in accessors:                                                      # pending: neither counted nor indexed
            einval(call)
        # refused arguments of finish leave the handle pending
        einval(lambda: h.index_part_finish(own["minimizers"] - 1, U, 100))
        einval(lambda: h.index_part_finish(M, own["distinct"] - 1, 100))
        einval(lambda: h.index_part_finish(U - 1, U, 100))                           # minimizers < distinct
        for rate in (-1.0, float("inf"), float("nan")):
            einval(lambda: h.index_part_finish(M, U, rate), "repeat_kmer_rate")
        assert h.index_part_finish(M, U, 100) == pu.fields(pu.restrict(mm.entries(reads, k, w, 0), 100, 2)[1])
        einval(lambda: h.index_part_finish(M, U, 100), "no pending")             # a second finish
        assert h.index_dump()[0].size > 0                                           # ... leaves the index alone
        # every other call drops a pending begin
        want = None
        for other in (lambda: h.count(reads, k, 0), lambda: h.count_part(reads, k, 0, 2, 0), lambda: h.sketch(reads, k, w, 0),
                      lambda: h.index_minimizers(reads, k, w, 100, 0)):
            h.index_part_begin(reads, k, w, 0, 2, 0)
            other()
            einval(lambda: h.index_part_finish(M, U, 100), "no pending")
        h.index_part_begin(reads, k, w, 0, 2, 0)
        h.index_part_begin(reads, k, w, 1, 2, 0)                                    # another begin replaces the first
        assert h.index_part_finish(M, U, 100)["minimizers"] == own["minimizers"]
        # a later count and a later unpartitioned index work on the same handle
        want = kmer_model.model(reads, k, 0)
        assert h.count(reads, k, 0) == {f: want[f] for f in kmer_model.FIELDS}
        assert h.index_minimizers(reads, k, w, 100, 0) == {f: m[f] for f in mm.FIELDS}
        np.testing.assert_array_equal(h.index_dump()[2], m["gpos"])
    finally:
        h.close()


def test_begin_arguments(kc):
    from genarchbench_amd.kmer import MAX_PARTS, MAX_WINDOW, repetitive_frequency
    reads = [rand(3, 600)]
    for part, nparts in ((-1, 2), (2, 2), (0, 0), (0, -1), (0, MAX_PARTS + 1)):
        einval(lambda: kc.index_part_begin(reads, 15, 5, part, nparts, 0), "nparts")
    for w in (0, -1, MAX_WINDOW + 1):
        einval(lambda: kc.index_part_begin(reads, 15, w, 0, 2, 0), "window")
    for k in (0, 18):
        einval(lambda: kc.index_part_begin(reads, k, 5, 0, 2, 0))
    einval(lambda: kc.index_part_begin([rand(50, 300), rand(51, 200) + b"N" + rand(52, 100)], 15, 5, 0, 2, 0), "read 1 ")
    einval(lambda: kc.index_part_finish(10, 5, 100), "no pending")                # none of the refused begins left anything pending
    for args in ((-1, 0, 100.0), (0, -1, 100.0), (5, 3, -1.0), (5, 3, float("nan"))):
        einval(lambda: repetitive_frequency(*args))
    for total, unique, rate in ((1093, 957, 100.0), (0, 0, 100.0), (163743, 104383, 3.0), (7, 2, 0.0), (10 ** 12, 3, 3.0e38)):
        want = min(mm.repetitive_frequency(total, unique, rate), 2 ** 63 - 1) if rate < 1e30 else 2 ** 63 - 1
        assert repetitive_frequency(total, unique, rate) == want


# ---- 9. device form ------------------------------------------------------------------------------------------------------------------------
def test_device_form_equals_the_host_form(handles):
    import torch
    from genarchbench_amd.kmer import pack_reads
    reads = [rand(70, 5000), rand(71, 30), b"A" * 900, rand(72, TILE + 500)]
    seq, off, ln = pack_reads(reads)
    dev = torch.device("cuda:0")
    t_seq, t_off, t_ln = (torch.from_numpy(a).to(dev) for a in (seq, off, ln))
    nparts = 3
    host_begun = [handles[p].index_part_begin(reads, 15, 10, p, nparts, 100) for p in range(nparts)]
    M, U = sum(b["minimizers"] for b in host_begun), sum(b["distinct"] for b in host_begun)
    host = [handles[p].index_part_finish(M, U, 3) for p in range(nparts)]
    host_dumps = [handles[p].index_dump() for p in range(nparts)]
    assert [handles[p].index_part_begin_device(t_seq, t_off, t_ln, 15, 10, p, nparts, 100) for p in range(nparts)] == host_begun
    assert [handles[p].index_part_finish(M, U, 3) for p in range(nparts)] == host
    for p in range(nparts):
        for a, b in zip(handles[p].index_dump(), host_dumps[p]):
            np.testing.assert_array_equal(a, b)
    whole = handles[3].index_minimizers(reads, 15, 10, 3, 100)
    assert pu.sum_fields(host) == whole
    for a, b in zip(pu.merge(host_dumps), handles[3].index_dump()):
        np.testing.assert_array_equal(a, b)


def test_every_operation_reads_one_input_the_same_way(handles):
    """count, sketch, index and the two-phase index take their reads through one descriptor, filled from host pointers or from
    device pointers: on one tiny input both forms of every operation give equal fields and equal dumps, and the three partitions
    add up to the unpartitioned call.  The reads: a second tile of a single position | min_len + 1 bases, kept | min_len bases,
    filtered | k bases, kept without a position"""
    import torch
    from genarchbench_amd.kmer import pack_reads
    k, w, min_len, nparts = 5, 4, 3, 3
    reads = [rand(80, TILE + 1 + k), rand(81, min_len + 1), rand(82, min_len), rand(83, k)]
    seq, off, ln = pack_reads(reads)
    t_seq, t_off, t_ln = (torch.from_numpy(a).to("cuda:0") for a in (seq, off, ln))
    hs, one = handles[:nparts], handles[3]

    def same(a, b):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)

    # count_part
    host = [hs[p].count_part(reads, k, p, nparts, min_len) for p in range(nparts)]
    host_dumps = [hs[p].dump() for p in range(nparts)]
    assert [hs[p].count_part_device(t_seq, t_off, t_ln, k, p, nparts, min_len) for p in range(nparts)] == host
    for p in range(nparts):
        same(hs[p].dump(), host_dumps[p])
    whole = one.count(reads, k, min_len)
    assert (whole["reads_kept"], whole["positions"]) == (3, TILE + 1)
    assert all((r["reads_kept"], r["positions"]) == (3, TILE + 1) for r in host)
    assert {f: sum(r[f] for r in host) for f in ("distinct", "total_kmers", "hash_size")} == {f: whole[f] for f in ("distinct", "total_kmers", "hash_size")}
    assert max(r["max_count"] for r in host) == whole["max_count"]
    kmers = np.concatenate([d[0] for d in host_dumps]); counts = np.concatenate([d[1] for d in host_dumps])
    order = np.argsort(kmers, kind="stable")
    same((kmers[order], counts[order]), one.dump())
    assert one.count_device(t_seq, t_off, t_ln, k, min_len) == whole
    same(one.dump(), (kmers[order], counts[order]))

    # sketch
    start, pos = one.sketch(reads, k, w, min_len)
    assert start[0] == 0 and (np.diff(start)[1:] == 0).all() and pos.size == start[-1] > 0
    t_start = torch.full((len(reads) + 1,), -12345, dtype=torch.int64, device="cuda:0")
    t_pos = torch.full((pos.size,), -12345, dtype=torch.int32, device="cuda:0")
    assert one.sketch_device(t_seq, t_off, t_ln, k, w, t_start, t_pos, min_len) == (0, pos.size)
    same((t_start.cpu().numpy(), t_pos.cpu().numpy()), (start, pos))

    # index_minimizers
    whole = one.index_minimizers(reads, k, w, 3, min_len)
    whole_dump = one.index_dump()
    assert (whole["reads_kept"], whole["total_len"], whole["minimizers"]) == (3, TILE + 1 + k + min_len + 1 + k, pos.size)
    assert one.index_minimizers_device(t_seq, t_off, t_ln, k, w, 3, min_len) == whole
    same(one.index_dump(), whole_dump)

    # index_part_begin -> index_part_finish
    begun = [hs[p].index_part_begin(reads, k, w, p, nparts, min_len) for p in range(nparts)]
    M, U = sum(b["minimizers"] for b in begun), sum(b["distinct"] for b in begun)
    assert (M, U) == (whole["minimizers"], whole["distinct"])
    done = [hs[p].index_part_finish(M, U, 3) for p in range(nparts)]
    dumps = [hs[p].index_dump() for p in range(nparts)]
    assert [hs[p].index_part_begin_device(t_seq, t_off, t_ln, k, w, p, nparts, min_len) for p in range(nparts)] == begun
    assert [hs[p].index_part_finish(M, U, 3) for p in range(nparts)] == done
    for p in range(nparts):
        same(hs[p].index_dump(), dumps[p])
    assert pu.sum_fields(done) == whole
    same(pu.merge(dumps), whole_dump)


# ---- 10. the set ---------------------------------------------------------------------------------------------------------------------------
def test_the_set_equals_one_counter(kc):
    from genarchbench_amd.kmer import KmerCounterSet
    reads = [rand(90, 5000), b"A" * 400 + rand(91, 700), rand(92, TILE + 33)]
    k, w = 15, 5
    ks = KmerCounterSet([0, 0, 0])
    try:
        for rate in (100.0, 0.5):
            want = kc.index_minimizers(reads, k, w, rate, 0)
            assert ks.index_minimizers(reads, k, w, rate, 0) == want
            want_dump = kc.index_dump()
            for a, b in zip(ks.index_dump(), want_dump):
                np.testing.assert_array_equal(a, b)
            m = mm.build_index(reads, k, w, rate, 0)
            assert m["repetitive"].size > 0 or rate == 100.0
            probe = np.concatenate([m["kmers"], m["repetitive"], np.array([(1 << 30) - 1, 12345], np.uint64)])
            for a, b in zip(ks.index_lookup(probe), kc.index_lookup(probe)):
                np.testing.assert_array_equal(a, b)
            rows = ks.index_last_phases()
            assert [(r["part"], r["nparts"]) for r in rows] == [(0, 3), (1, 3), (2, 3)] and all(r["sketch_ms"] > 0 for r in rows)
    finally:
        ks.close()
