"""GPU: the k-mer counter in key-space partitions (gab_kmer_count_part, through genarchbench_amd.kmer) against the numpy model of
tests/kmer_model.py restricted to each partition by the numpy restatement of the hash in tests/kmer_parts_util.py.  Every comparison
is equality; every output buffer is pre-filled with a sentinel by the Python mirror.

`probes` (table lines visited).  An insert visits a second line only when its home line holds eight other keys, and which key of
an overfull line is the one pushed on depends on the order of the inserts.  The sum of the partitions' probes therefore equals the
unpartitioned call's exactly when no line of any of the tables is the home of more than eight keys -- no_line_overfull says so from
the model alone -- and every probes count then equals its inserts.  That holds for every k = 1 and k = 3 case here (asserted), and
the equalities are asserted wherever it holds.  Where lines are overfull but every key of the input occurs once, the walks are
still the same number in any order (tests/kmer_table_cases.py: expected_probes) and every probes count is asserted against it;
where keys repeat, what is asserted is what always holds: probes >= inserts per partition.  `merged` has no such condition and
adds up in every case."""
import json
import threading

import numpy as np
import pytest

from tests import kmer_model
from tests.kmer_parts_util import SLOTS, fields, merged_keys, no_line_overfull, np_line_of, np_part_of, restrict
from tests.kmer_table_cases import expected_probes
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

EXPECTED = json.load(open(f"{GOLDEN}/kmer_expected.json"))
ACGT = np.frombuffer(b"ACGT", np.uint8)
EINVAL = -22
INPUTS = sorted(EXPECTED["files"]) + ["random"]
KS = (1, 3, 16, 17)
NPARTS = (1, 2, 3, 8)
NBINS = 300


def rand_reads(seed, lengths):
    rng = np.random.default_rng(seed)
    return [ACGT[rng.integers(0, 4, n)].tobytes() for n in lengths]


_reads, _whole = {}, {}


def reads_of(name):
    if name not in _reads:
        _reads[name] = rand_reads(21, [14_000, 5001, 9000, 5000, 16, 0]) if name == "random" else kmer_model.load_reads([f"{GOLDEN}/{name}"])
    return _reads[name]


def whole_model(name, k):
    """(model of the whole input, keys of its merged positions), computed once per input and k"""
    if (name, k) not in _whole:
        _whole[(name, k)] = (kmer_model.model(reads_of(name), k), merged_keys(reads_of(name), k))
    return _whole[(name, k)]


@pytest.fixture(scope="module")
def kc():
    from genarchbench_amd.kmer import KmerCounter
    e = KmerCounter()
    yield e
    e.close()


def check_part(kc, reads, k, part, nparts, mp, count=None):
    """one partitioned count against its model mp: fields, spectrum, dump, merged, the table it ran in, and that it ran once"""
    from genarchbench_amd.kmer import table_slots
    got = (count or (lambda: kc.count_part(reads, k, part, nparts)))()
    assert got == fields(mp)
    np.testing.assert_array_equal(kc.spectrum(NBINS), kmer_model.spectrum(mp["counts"], NBINS))
    kmers, counts = kc.dump()
    np.testing.assert_array_equal(kmers, mp["kmers"])
    np.testing.assert_array_equal(counts.astype(np.int64), mp["counts"])
    st, lp = kc.last_stats(), kc.last_part()
    slots = table_slots(mp["positions"], k, nparts)
    assert 2 * mp["distinct"] <= slots            # (from the model: a table that is at most half full cannot fill up)
    assert lp == {"part": part, "nparts": nparts, "table_slots": slots, "retried": 0}
    assert st["merged"] == mp["merged"] and st["probes"] >= mp["inserts"]
    return got, st


@pytest.mark.parametrize("nparts", NPARTS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", INPUTS)
def test_every_partition_equals_the_model(kc, name, k, nparts):
    from genarchbench_amd.kmer import part_of, table_slots
    reads = reads_of(name)
    m, mk = whole_model(name, k)
    parts = restrict(m, mk, nparts)
    np.testing.assert_array_equal(part_of(m["kmers"], nparts), np_part_of(m["kmers"], nparts))
    whole = kc.count(reads, k)
    assert whole == fields(m)
    whole_st = kc.last_stats()
    got = [check_part(kc, reads, k, p, nparts, parts[p]) for p in range(nparts)]
    for f in ("reads_kept", "positions"):
        assert all(g[f] == whole[f] for g, _ in got)
    for f in ("distinct", "total_kmers", "hash_size"):
        assert sum(g[f] for g, _ in got) == whole[f]
    assert max(g["max_count"] for g, _ in got) == whole["max_count"]
    assert sum(st["merged"] for _, st in got) == whole_st["merged"] == m["merged"]
    # probes: see the head of this file
    exact = no_line_overfull(m["kmers"], 1, table_slots(m["positions"], k, 1) // SLOTS) and all(
        no_line_overfull(parts[p]["kmers"], nparts, table_slots(m["positions"], k, nparts) // SLOTS) for p in range(nparts))
    assert exact or k > 3
    if exact:
        assert [st["probes"] for _, st in got] == [parts[p]["inserts"] for p in range(nparts)]
        assert sum(st["probes"] for _, st in got) == whole_st["probes"] == m["positions"] - m["merged"]
    elif m["max_count"] == 1:                      # lines spill, but every key is inserted once: the walks add up to the same number in any order
        nl, nl1 = table_slots(m["positions"], k, nparts) // SLOTS, table_slots(m["positions"], k, 1) // SLOTS
        assert [st["probes"] for _, st in got] == [expected_probes(np_line_of(parts[p]["kmers"], nparts, nl), nl) for p in range(nparts)]
        assert whole_st["probes"] == expected_probes(np_line_of(m["kmers"], 1, nl1), nl1)
    if nparts == 1:                                # part 0 of 1 IS the unpartitioned count
        assert got[0][0] == whole
        assert got[0][1]["merged"] == whole_st["merged"] and (got[0][1]["probes"] == whole_st["probes"] or not exact)


def test_k1_over_8_partitions_leaves_most_of_them_empty(kc):
    """two canonical keys (A and C): at least six of the eight partitions own nothing"""
    reads = reads_of("random")
    m, mk = whole_model("random", 1)
    assert m["distinct"] == 2
    parts = restrict(m, mk, 8)
    empty = [p for p in range(8) if parts[p]["distinct"] == 0]
    assert len(empty) >= 6
    zeros = dict({f: 0 for f in kmer_model.FIELDS}, reads_kept=m["reads_kept"], positions=m["positions"])
    for p in empty:
        assert kc.count_part(reads, 1, p, 8) == zeros
        np.testing.assert_array_equal(kc.spectrum(NBINS), np.zeros(NBINS, np.int64))
        kmers, counts = kc.dump()
        assert kmers.size == 0 and counts.size == 0
        np.testing.assert_array_equal(kc.query(np.arange(4, dtype=np.uint64)), np.zeros(4, np.uint32))
        assert kc.last_stats()["probes"] == 0 and kc.last_part()["retried"] == 0


def test_no_state_leaks_between_whole_and_partitioned_counts(kc):
    name, k = "kmer_small.fa", 16
    reads, other = reads_of(name), reads_of("random")
    m, mk = whole_model(name, k)
    parts = restrict(m, mk, 3)
    mo, mko = whole_model("random", 17)
    for _ in range(2):
        assert kc.count(other, 17) == fields(mo)            # a whole count, then a part of another input and k
        check_part(kc, reads, k, 1, 3, parts[1])
        assert kc.count(reads, k) == fields(m)              # ... and the reverse
        kmers, counts = kc.dump()
        np.testing.assert_array_equal(kmers, m["kmers"])
        np.testing.assert_array_equal(counts.astype(np.int64), m["counts"])
        lp = kc.last_part()
        assert (lp["part"], lp["nparts"], lp["retried"]) == (0, 1, 0)
        check_part(kc, other, 17, 0, 2, restrict(mo, mko, 2)[0])
        check_part(kc, reads, k, 2, 3, parts[2])


def test_query_is_answered_by_exactly_one_partition(kc):
    name, k, nparts = "kmer_small.fa", 17, 3
    reads = reads_of(name)
    m, _ = whole_model(name, k)
    rng = np.random.default_rng(31)
    present = m["kmers"][rng.integers(0, m["kmers"].size, 3000)]
    rc = np.array([kmer_model.revcomp_value(int(x), k) for x in present[:500]], np.uint64)
    absent = rng.integers(0, 4 ** k, 3000).astype(np.uint64)
    q = np.concatenate([present, rc, absent])
    rc_all, x = np.zeros_like(q), q.copy()
    for _ in range(k):
        rc_all = (rc_all << np.uint64(2)) | (~x & np.uint64(3))
        x >>= np.uint64(2)
    canon = np.minimum(q, rc_all)
    at = np.searchsorted(m["kmers"], canon)
    at[at == m["kmers"].size] = 0
    want = np.where(m["kmers"][at] == canon, m["counts"][at], 0).astype(np.uint32)
    assert (want[:3500] > 0).all() and (want[3500:] == 0).any()
    owner = np_part_of(canon, nparts)
    answers = []
    for p in range(nparts):
        kc.count_part(reads, k, p, nparts)
        answers.append(kc.query(q))
    answers = np.stack(answers)
    for p in range(nparts):
        np.testing.assert_array_equal(answers[p], np.where(owner == p, want, 0))      # its own keys, 0 for every other key
    np.testing.assert_array_equal(answers.sum(0), want)
    assert ((answers > 0).sum(0) == (want > 0)).all()


def test_device_entry_point_on_a_side_stream(kc):
    import torch
    from genarchbench_amd.kmer import pack_reads
    name, k, nparts = "kmer_small_n.fq.gz", 17, 3
    reads = reads_of(name)
    m, mk = whole_model(name, k)
    parts = restrict(m, mk, nparts)
    seq, off, ln = pack_reads(reads)
    d = [torch.from_numpy(x).cuda() for x in (seq, off, ln)]
    side = torch.cuda.Stream()
    for p in range(nparts):
        host = kc.count_part((seq, off, ln), k, p, nparts)
        host_dump, host_st = kc.dump(), kc.last_stats()

        def on_side():
            with torch.cuda.stream(side):
                return kc.count_part_device(*d, k, p, nparts, stream=side.cuda_stream)
        got, st = check_part(kc, reads, k, p, nparts, parts[p], count=on_side)
        assert got == host and st["merged"] == host_st["merged"]
        dev_dump = kc.dump()
        np.testing.assert_array_equal(dev_dump[0], host_dump[0])
        np.testing.assert_array_equal(dev_dump[1], host_dump[1])


def test_a_full_first_table_repeats_the_call(kc, monkeypatch):
    """GAB_KMER_PART_FLOOR: the first table is the 16-line floor, 128 slots for some 60 000 keys.  The bounded inserts give up, the
    call runs once more in the unpartitioned table size and returns the same results."""
    from genarchbench_amd.kmer import table_slots
    name, k, nparts = "kmer_small.fa", 17, 2
    reads = reads_of(name)
    m, mk = whole_model(name, k)
    parts = restrict(m, mk, nparts)
    assert min(p["distinct"] for p in parts) > 16 * SLOTS
    for p in range(nparts):
        monkeypatch.delenv("GAB_KMER_PART_FLOOR", raising=False)
        plain, _ = check_part(kc, reads, k, p, nparts, parts[p])
        plain_spec, plain_dump = kc.spectrum(NBINS), kc.dump()
        monkeypatch.setenv("GAB_KMER_PART_FLOOR", "1")
        forced = kc.count_part(reads, k, p, nparts)
        assert kc.last_part() == {"part": p, "nparts": nparts, "table_slots": table_slots(m["positions"], k, 1), "retried": 1}
        assert forced == plain == fields(parts[p])
        np.testing.assert_array_equal(kc.spectrum(NBINS), plain_spec)
        dump = kc.dump()
        np.testing.assert_array_equal(dump[0], plain_dump[0])
        np.testing.assert_array_equal(dump[1], plain_dump[1])
        assert kc.last_stats()["merged"] == parts[p]["merged"]
    # the switch is for partitioned counts: a whole count has no forecast table and runs as ever
    assert kc.count(reads, k) == fields(m) and kc.last_part()["retried"] == 0


def test_two_handles_on_one_device_at_once():
    from genarchbench_amd.kmer import KmerCounter
    reads = reads_of("random")
    m, mk = whole_model("random", 17)
    parts = restrict(m, mk, 2)
    handles = [KmerCounter(0), KmerCounter(0)]
    results = [[], []]

    def run(p):
        for _ in range(3):
            got = handles[p].count_part(reads, 17, p, 2)
            results[p].append((got, handles[p].dump(), handles[p].last_part()["retried"]))
    threads = [threading.Thread(target=run, args=(p,)) for p in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for p in range(2):
        assert len(results[p]) == 3
        for got, (kmers, counts), retried in results[p]:
            assert got == fields(parts[p]) and retried == 0
            np.testing.assert_array_equal(kmers, parts[p]["kmers"])
            np.testing.assert_array_equal(counts.astype(np.int64), parts[p]["counts"])
        handles[p].close()


def test_counter_set_of_three_partitions_on_one_device():
    from genarchbench_amd.kmer import KmerCounterSet
    name, k = "kmer_small_n.fq.gz", 16
    reads = reads_of(name)
    m, mk = whole_model(name, k)
    parts = restrict(m, mk, 3)
    ks = KmerCounterSet([0, 0, 0])
    ks.reserve(len(reads), sum(len(r) for r in reads))
    assert ks.count(reads, k) == fields(m)
    np.testing.assert_array_equal(ks.spectrum(NBINS), kmer_model.spectrum(m["counts"], NBINS))
    kmers, counts = ks.dump()
    np.testing.assert_array_equal(kmers, m["kmers"])
    np.testing.assert_array_equal(counts.astype(np.int64), m["counts"])
    rng = np.random.default_rng(32)
    q = np.concatenate([m["kmers"][rng.integers(0, m["kmers"].size, 2000)], rng.integers(0, 4 ** k, 2000).astype(np.uint64)])
    rc_all, x = np.zeros_like(q), q.copy()
    for _ in range(k):
        rc_all = (rc_all << np.uint64(2)) | (~x & np.uint64(3))
        x >>= np.uint64(2)
    canon = np.minimum(q, rc_all)
    at = np.searchsorted(m["kmers"], canon)
    at[at == m["kmers"].size] = 0
    np.testing.assert_array_equal(ks.query(q), np.where(m["kmers"][at] == canon, m["counts"][at], 0).astype(np.uint32))
    rows = ks.last_stats()
    assert [(r["part"], r["nparts"], r["retried"]) for r in rows] == [(0, 3, 0), (1, 3, 0), (2, 3, 0)]
    assert [r["merged"] for r in rows] == [p["merged"] for p in parts]
    ks.close()


def test_errors():
    from genarchbench_amd import GabError
    from genarchbench_amd.kmer import KmerCounter, KmerCounterSet
    e = KmerCounter()
    with pytest.raises(GabError) as err:               # before any count, like last_stats
        e.last_part()
    assert err.value.code == EINVAL
    with pytest.raises(GabError) as err2:
        e.last_stats()
    assert err2.value.code == err.value.code
    reads = reads_of("random")
    for part, nparts in ((-1, 2), (2, 2), (0, 0), (0, 65)):
        with pytest.raises(GabError) as err:
            e.count_part(reads, 17, part, nparts)
        assert err.value.code == EINVAL and "part = %d" % part in str(err.value) and "nparts = %d" % nparts in str(err.value)
    with pytest.raises(GabError) as err:
        e.reserve_part(10, 1000, 65)
    assert err.value.code == EINVAL and "nparts = 65" in str(err.value)
    m, mk = whole_model("random", 17)
    assert e.count_part(reads, 17, 63, 64) == fields(restrict(m, mk, 64)[63])      # the largest split is fine
    e.close()
    with pytest.raises(ValueError):
        KmerCounterSet([])
