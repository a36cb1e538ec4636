"""GPU: the probe walks of the k-mer table (kmer_insert, kmer_find, kmer_home in genarchbench_amd/csrc/kmer.hip) where lines fill,
spill, chain and wrap, on the tiny inputs of tests/kmer_table_cases.py -- a few hundred k-mers per test, every line's occupancy
chosen and asserted on the CPU when the case is built -- through the count, its partitions, the minimizer index, its partitions
and the solid index.  Every comparison is an equality against the numpy models (tests/kmer_model.py, tests/minimizer_model.py,
tests/solid_model.py, tests/kmer_parts_util.py); every output buffer is pre-filled with a sentinel by the Python mirror.

`probes` is asserted with == wherever every key of the input is inserted once (expected_probes; why: the head of
tests/kmer_table_cases.py), which is every case but `repeats`: there what holds is probes >= inserts."""
import numpy as np
import pytest

from tests import kmer_model, minimizer_model as mm, minimizer_parts_util as pu, solid_model as sm
from tests import kmer_table_cases as tc
from tests.kmer_parts_util import SLOTS, fields, merged_keys, np_part_of, restrict

pytestmark = pytest.mark.gpu

NBINS = 8
WINDOWS = (1, 10)


@pytest.fixture(scope="module")
def kc():
    from genarchbench_amd.kmer import KmerCounter
    e = KmerCounter()
    yield e
    e.close()


def both(keys, k):
    """every key as it is and as its reverse complement"""
    return np.concatenate([keys, tc.np_revcomp(keys, k)])


def check_table(kc, mp, k, absent):
    """what the handle holds after a count == the model mp of that table: spectrum, dump, a query of every key in both orientations,
    0 for every absent key in both orientations"""
    np.testing.assert_array_equal(kc.spectrum(NBINS), kmer_model.spectrum(mp["counts"], NBINS))
    kmers, counts = kc.dump()
    np.testing.assert_array_equal(kmers, mp["kmers"])
    np.testing.assert_array_equal(counts.astype(np.int64), mp["counts"])
    np.testing.assert_array_equal(kc.query(both(mp["kmers"], k)).astype(np.int64), np.concatenate([mp["counts"]] * 2))
    np.testing.assert_array_equal(kc.query(both(absent, k)), np.zeros(2 * absent.size, np.uint32))


def check_whole(kc, case, count):
    from genarchbench_amd.kmer import table_slots
    m, t = case.model, case.tables[0]
    assert count() == fields(m)
    assert table_slots(case.positions, case.k, 1) == t.nlines * SLOTS
    assert kc.last_part() == {"part": 0, "nparts": 1, "table_slots": t.nlines * SLOTS, "retried": 0}
    check_table(kc, m, case.k, case.absent_keys())
    st = kc.last_stats()
    assert st["merged"] == m["merged"] == 0
    print(f"{case.name}: probes {st['probes']}, expected {t.probes if case.once else '>= %d' % case.positions}")
    if case.once:
        assert st["probes"] == t.probes
    else:
        assert st["probes"] >= case.positions


# ---- the whole count --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.WHOLE_NAMES)
def test_count(kc, name):
    case = tc.whole_case(name)
    check_whole(kc, case, lambda: kc.count(case.reads, case.k, 0))
    if name == "repeats":
        assert sorted(np.unique(kc.dump()[1]).tolist()) == [1, 3, 5]


@pytest.mark.parametrize("name", ["wrap", "long_wrap"])
def test_count_device(kc, name):
    import torch
    from genarchbench_amd.kmer import pack_reads
    case = tc.whole_case(name)
    d = [torch.from_numpy(x).cuda() for x in pack_reads(case.reads)]
    check_whole(kc, case, lambda: kc.count_device(*d, case.k, 0))


# ---- partitions -------------------------------------------------------------------------------------------------------------------------
def check_parts(kc, case, tables, retried, slots):
    """count_part of every partition of `case` == the model restricted to it, in the tables `tables` -> the answers of every partition
    to a query of all keys"""
    m = case.model
    parts = restrict(m, merged_keys(case.reads, case.k, 0), case.nparts)
    answers = []
    for p, (mp, t) in enumerate(zip(parts, tables)):
        assert kc.count_part(case.reads, case.k, p, case.nparts, 0) == fields(mp)
        assert kc.last_part() == {"part": p, "nparts": case.nparts, "table_slots": slots[p], "retried": retried[p]}
        assert slots[p] == t.nlines * SLOTS and np.array_equal(t.keys, mp["kmers"])
        absent = np.concatenate([case.absent_keys(q) for q in range(case.nparts)])          # its own and the other partitions'
        check_table(kc, mp, case.k, absent)
        st = kc.last_stats()
        print(f"{case.name} part {p}: probes {st['probes']}, expected {t.probes}")
        assert st["merged"] == 0 and st["probes"] == t.probes
        answers.append(kc.query(both(m["kmers"], case.k)))
    answers = np.stack(answers).astype(np.int64)
    owner = np.concatenate([np_part_of(m["kmers"], case.nparts)] * 2)
    for p in range(case.nparts):
        np.testing.assert_array_equal(answers[p], np.where(owner == p, 1, 0))              # exactly one partition answers each key
    return answers


@pytest.mark.parametrize("name,nparts", tc.PART_NAMES)
def test_count_part(kc, name, nparts):
    from genarchbench_amd.kmer import table_slots
    case = tc.part_case(name, nparts)
    assert table_slots(case.positions, case.k, nparts) == tc.FLOOR_LINES * SLOTS
    check_parts(kc, case, case.tables, [0] * nparts, [tc.FLOOR_LINES * SLOTS] * nparts)


def test_count_part_floor_boundary(kc, monkeypatch):
    """GAB_KMER_PART_FLOOR=1, the 16-line first table: 128 keys fill every slot of it and the bounded insert must not give up; the
    129th key makes it give up, and the call runs again in the unpartitioned table size"""
    from genarchbench_amd.kmer import table_slots
    full, over = tc.floor_case("floor_full"), tc.floor_case("floor_over")
    floor = tc.FLOOR_LINES * SLOTS
    monkeypatch.setenv("GAB_KMER_PART_FLOOR", "1")
    check_parts(kc, full, full.floor, [0, 0], [floor, floor])
    # the table of partition 0 has no empty slot: a look-up of a key it does not hold ends after nlines lines
    assert kc.count_part(full.reads, full.k, 0, 2, 0) == fields(restrict(full.model, merged_keys(full.reads, full.k, 0), 2)[0])
    assert kc.last_part()["table_slots"] == floor and kc.last_stats()["probes"] == full.floor[0].probes
    absent = np.concatenate([full.floor_absent["full"][0], full.floor_absent["last"][0]])
    np.testing.assert_array_equal(kc.query(both(absent, full.k)), np.zeros(2 * absent.size, np.uint32))
    again = table_slots(over.positions, over.k, 1)
    assert again == over.again.nlines * SLOTS
    check_parts(kc, over, [over.again, over.floor[0]], [1, 0], [again, floor])
    monkeypatch.delenv("GAB_KMER_PART_FLOOR")
    for case in (full, over):
        first = table_slots(case.positions, case.k, 2)
        check_parts(kc, case, case.tables, [0, 0], [first, first])


# ---- the minimizer index: a read with one position has its minimizer there, for any window --------------------------------------------------
def check_index(h, mp, k, others):
    """dump and look-ups of the index in the handle == the model mp; others: keys it does not hold -> (-1, 0, 0)"""
    kmers, start, gpos = h.index_dump()
    np.testing.assert_array_equal(kmers, mp["kmers"])
    np.testing.assert_array_equal(start, mp["start"])
    np.testing.assert_array_equal(gpos, mp["gpos"])
    n = mp["kmers"].size
    first, count, rep = h.index_lookup(both(mp["kmers"], k))
    np.testing.assert_array_equal(first, np.concatenate([mp["start"][:-1]] * 2))
    np.testing.assert_array_equal(count, np.concatenate([np.diff(mp["start"])] * 2))
    assert not rep.any() and first.size == 2 * n
    for keys, flag in ((mp["repetitive"], 1), (others, 0)):
        if not keys.size:
            continue
        first, count, rep = h.index_lookup(both(keys, k))
        assert (first == -1).all() and (count == 0).all() and (rep == flag).all()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", ["wrap", "long_wrap", "repeats"])
def test_index_minimizers(kc, name, window):
    from genarchbench_amd.kmer import table_slots
    case = tc.whole_case(name)
    rate = 1.5 if name == "repeats" else 100.0
    m = mm.build_index(case.reads, case.k, window, rate, 0)
    assert m["minimizers"] == case.positions and m["distinct"] == case.keys.size          # one minimizer per read, at its one position
    if name == "repeats":      # the threshold falls between three and five copies: the five-fold keys go, two of them keys of the last line
        assert m["repetitive_frequency"] == 4 and np.array_equal(m["repetitive"], case.keys[case.counts == 5])
    else:
        assert m["repetitive"].size == 0
    assert kc.index_minimizers(case.reads, case.k, window, rate, 0) == {f: m[f] for f in mm.FIELDS}
    assert kc.index_last_part() == {"part": 0, "nparts": 1, "table_slots": table_slots(case.positions, case.k, 1), "retried": 0}
    check_index(kc, m, case.k, case.absent_keys())


def check_index_parts(kc, case, window, retried, slots):
    """index_part_begin / index_part_finish of every partition, one after the other on one handle (finish needs only the two sums,
    known from the model) == the model restricted to the partition"""
    found = mm.entries(case.reads, case.k, window, 0)
    assert np.array_equal(np.sort(found[0]), case.keys)
    parts = pu.restrict(found, 100.0, case.nparts)
    M, U = int(found[0].size), int(np.unique(found[0]).size)
    for p, mp in enumerate(parts):
        assert kc.index_part_begin(case.reads, case.k, window, p, case.nparts, 0) == pu.begin_fields(mp)
        assert kc.index_part_finish(M, U, 100.0) == pu.fields(mp)
        assert kc.index_last_part() == {"part": p, "nparts": case.nparts, "table_slots": slots[p], "retried": retried[p]}
        others = np.concatenate([case.absent_keys(q) for q in range(case.nparts)] + [parts[q]["kmers"] for q in range(case.nparts) if q != p])
        check_index(kc, mp, case.k, others)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name,nparts", tc.PART_NAMES)
def test_index_parts(kc, name, nparts, window):
    case = tc.part_case(name, nparts)
    check_index_parts(kc, case, window, [0] * nparts, [tc.FLOOR_LINES * SLOTS] * nparts)


def test_index_parts_floor_boundary(kc, monkeypatch):
    """the capacity pass of a partitioned index in the 16-line floor table: 128 keys fill it, the fill pass and the look-ups then
    walk a table with no empty slot; 129 keys repeat the capacity pass in the unpartitioned table size"""
    from genarchbench_amd.kmer import table_slots
    full, over = tc.floor_case("floor_full"), tc.floor_case("floor_over")
    floor = tc.FLOOR_LINES * SLOTS
    monkeypatch.setenv("GAB_KMER_PART_FLOOR", "1")
    check_index_parts(kc, full, 1, [0, 0], [floor, floor])
    found = mm.entries(full.reads, full.k, 10, 0)
    mp = pu.restrict(found, 100.0, 2)[0]
    assert kc.index_part_begin(full.reads, full.k, 10, 0, 2, 0) == pu.begin_fields(mp)
    assert kc.index_part_finish(int(found[0].size), int(np.unique(found[0]).size), 100.0) == pu.fields(mp)
    assert kc.index_last_part() == {"part": 0, "nparts": 2, "table_slots": floor, "retried": 0}
    check_index(kc, mp, full.k, np.concatenate([full.floor_absent["full"][0], full.floor_absent["last"][0]]))
    check_index_parts(kc, over, 1, [1, 0], [table_slots(over.positions, over.k, 1), floor])
    monkeypatch.delenv("GAB_KMER_PART_FLOOR")
    for case in (full, over):
        first = table_slots(case.positions, case.k, 2)
        check_index_parts(kc, case, 1, [0, 0], [first, first])


# ---- the solid index --------------------------------------------------------------------------------------------------------------------
def check_solid(kc, case, rate, tandem):
    rule = dict(tc.SOLID, tandem_freq=tandem)
    args = (case.k, rule["min_freq"], rule["select_rate"], rule["tandem_freq"])
    start, pos = kc.solid_positions(case.reads, *args, 0)
    want_start, want_pos = sm.positions(case.reads, *args, 0)             # (the counts come from kmer_find in the count table)
    np.testing.assert_array_equal(start, want_start)
    np.testing.assert_array_equal(pos, want_pos)
    m = sm.build_index(case.reads, *args, rate, 0)
    assert kc.index_solid(case.reads, *args, rate, 0) == {f: m[f] for f in sm.FIELDS}
    check_index(kc, m, case.k, np.concatenate([case.absent_keys(), m["empty"]]))          # an empty-list key reads as absent
    return m


@pytest.mark.parametrize("rate", [2, 3])
def test_solid_index_steps_over_a_retired_slot(kc, rate):
    """X has left the capacity table: its slot, in the walk of the twelve keys of the last line, holds a value no key equals; every
    one of them is still found behind it, X and the absent keys read as absent"""
    case = tc.retired_case()
    m = check_solid(kc, case, rate, 1)
    assert m["empty"].tolist() == [int(case.x)] and m["indexed_kmers"] == case.keys.size - 1 and m["selected_kmers"] == case.keys.size
    first, count, rep = kc.index_lookup(both(np.array([case.x], np.uint64), case.k))
    assert first.tolist() == [-1, -1] and count.tolist() == [0, 0] and rep.tolist() == [0, 0]


def test_solid_index_of_the_wrap_case(kc):
    case = tc.whole_case("wrap")
    m = check_solid(kc, case, 2, 0)
    assert m["indexed_kmers"] == m["index_entries"] == 64 and m["empty"].size == 0 and m["repetitive"].size == 0
