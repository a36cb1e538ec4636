"""GPU: the solid k-mer index (gab_kmer_index_solid, gab_kmer_solid_positions, through genarchbench_amd.kmer) against what the
reference recorded (tests/golden/kmer_solid_expected.json, kmer_solid_tiny.npz) and, array for array, against the numpy model of
tests/solid_model.py.  Every comparison is equality; every output buffer is pre-filled with a sentinel by the Python mirror."""
import functools
import json

import numpy as np
import pytest

from tests import kmer_model, minimizer_model as mm, solid_model as sm
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

EXPECTED = json.load(open(f"{GOLDEN}/kmer_solid_expected.json"))
MIN_LEN = EXPECTED["min_len_exclusive"]
ACGT = np.frombuffer(b"ACGT", np.uint8)
EINVAL, ERANGE = -22, -34
RUN, TILE = 64, 4096        # GAB_KMER_RUN; a wave's tile of 64 runs
LINES = ("mean_frequency", "repetitive_frequency", "filtered_entries", "filtered_rate", "selected_kmers", "index_entries", "mean_index_frequency")


@pytest.fixture(scope="module")
def kc():
    from genarchbench_amd.kmer import KmerCounter
    e = KmerCounter()
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def reads_of(name):
    return kmer_model.load_reads([f"{GOLDEN}/{name}"])


def rand(seed, n, letters=4):
    return ACGT[np.random.default_rng(seed).integers(0, letters, n)].tobytes()


def check_positions(kc, reads, k, min_freq, select_rate, tandem, min_len=0):
    start, pos = kc.solid_positions(reads, k, min_freq, select_rate, tandem, min_len)
    want_start, want_pos = sm.positions(reads, k, min_freq, select_rate, tandem, min_len)
    for r in range(len(reads)):            # read by read: a wrong rank or tie shows here first
        np.testing.assert_array_equal(pos[start[r]:start[r + 1]], want_pos[want_start[r]:want_start[r + 1]], err_msg=f"read {r} of length {len(reads[r])}")
    np.testing.assert_array_equal(start, want_start)
    return start, pos


def check_index(kc, reads, k, min_freq, select_rate, tandem, rate, min_len=0):
    """the thirteen fields, the dump and a look-up of every k-mer of the model == the model"""
    m = sm.build_index(reads, k, min_freq, select_rate, tandem, rate, min_len)
    got = kc.index_solid(reads, k, min_freq, select_rate, tandem, rate, min_len)
    assert got == {f: m[f] for f in sm.FIELDS}
    kmers, start, gpos = kc.index_dump()
    np.testing.assert_array_equal(kmers, m["kmers"])
    np.testing.assert_array_equal(start, m["start"])
    np.testing.assert_array_equal(gpos, m["gpos"])
    if m["kmers"].size:
        first, count, rep = kc.index_lookup(m["kmers"])
        np.testing.assert_array_equal(first, m["start"][:-1])
        np.testing.assert_array_equal(count, np.diff(m["start"]))
        assert not rep.any()
    if m["empty"].size:                     # an empty-list key reads as absent
        first, count, rep = kc.index_lookup(m["empty"])
        assert (first == -1).all() and (count == 0).all() and (rep == 0).all()
    if m["repetitive"].size:
        first, count, rep = kc.index_lookup(m["repetitive"])
        assert (first == -1).all() and (count == 0).all() and (rep == 1).all()
    return m


# ---- goldens --------------------------------------------------------------------------------------------------------------------------
GRID = [(name, i) for name in sorted(EXPECTED["files"]) for i in range(len(EXPECTED["files"][name]["rows"]))]


@pytest.mark.parametrize("name,i", GRID)
def test_golden_rows(kc, name, i):
    """the lines the reference printed, its index digest and its removed k-mers, from the library's own result"""
    row = EXPECTED["files"][name]["rows"][i]
    got = kc.index_solid(reads_of(name), row["k"], row["min_freq"], row["select_rate"], row["tandem_freq"], row["rate"], MIN_LEN)
    assert sm.printed(got) == {f: row[f] for f in LINES}
    assert (got["indexed_kmers"], got["filtered_kmers"]) == (row["indexed_kmers"], row["filtered_kmers"])
    kmers, start, gpos = kc.index_dump()
    assert kmers.size == got["indexed_kmers"] and gpos.size == got["index_entries"] and (np.diff(start) > 0).all()
    assert mm.digest(kmers, start, gpos) == row["index_sha256"]


def test_golden_tiny_element_for_element(kc):
    t = EXPECTED["tiny"]
    z = np.load(f"{GOLDEN}/kmer_solid_tiny.npz")
    reads = [r for r in reads_of(t["file"]) if len(r) > MIN_LEN][:t["kept_reads"]]
    got = kc.index_solid(reads, t["k"], t["min_freq"], t["select_rate"], t["tandem_freq"], t["rate"], MIN_LEN)
    assert sm.printed(got) == {f: t[f] for f in LINES}
    kmers, start, gpos = kc.index_dump()
    for name, a in (("kmers", kmers), ("start", start), ("gpos", gpos)):
        np.testing.assert_array_equal(a, z[name], err_msg=name)
    first, count, rep = kc.index_lookup(z["repetitive"])
    assert (rep == 1).all() and (count == 0).all() and (first == -1).all()
    first, count, rep = kc.index_lookup(z["kmers"])
    np.testing.assert_array_equal(first, z["start"][:-1])
    np.testing.assert_array_equal(count, np.diff(z["start"]))
    check_index(kc, reads, t["k"], t["min_freq"], t["select_rate"], t["tandem_freq"], t["rate"], MIN_LEN)      # (empty-list keys: the model names them)


# ---- random inputs against the model -----------------------------------------------------------------------------------------------------
NPOS = (1, RUN - 1, RUN, RUN + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


@pytest.mark.parametrize("letters", [2, 4])
@pytest.mark.parametrize("k", [1, 5, 11, 16, 17])
def test_random_positions_every_length_rate_and_tandem(kc, k, letters):
    """n = L - k at 1, one lane's run +- 1, one wave's tile +- 1 and two tiles + 1; 2 letters make ties at the rank and high counts
    the rule; every select_rate with every tandem_freq, min_freq walking along"""
    reads = [rand(100 * k + i, n + k, letters) for i, n in enumerate(NPOS)] + [rand(7, k, letters), b""]
    for i, rate in enumerate((0.0, 0.05, 0.4, 0.999)):
        for j, tandem in enumerate((0, 1, 2, 100)):
            check_positions(kc, reads, k, (0, 1, 2, 5)[(i + j) % 4], rate, tandem)


@pytest.mark.parametrize("letters", [2, 4])
@pytest.mark.parametrize("k,min_freq,select_rate,tandem,rate", [(1, 0, 0.05, 0, 100), (5, 1, 0.4, 1, 1.5), (11, 2, 0.999, 2, 1.5), (16, 5, 0.0, 100, 0),
                                                                (17, 0, 0.4, 2, 100), (11, 1, 0.0, 1, 0), (5, 2, 0.05, 100, 1.5), (17, 5, 0.999, 0, 1.5)])
def test_random_index(kc, k, min_freq, select_rate, tandem, rate, letters):
    reads = [rand(900 + 10 * k + i, n + k, letters) for i, n in enumerate(NPOS)] + [rand(901, 3000, letters)] * 2
    check_index(kc, reads, k, min_freq, select_rate, tandem, rate)


# ---- the digit boundaries of the select: its four passes take the bytes of a 32-bit count ---------------------------------------------------
def test_count_beyond_two_bytes(kc):
    """a homopolymer of 70 000 bases: its one k-mer has a count above 2^16 (third digit), the k-mers of the random reads counts
    below 2^8; in the read that holds both kinds the rank decides between digits"""
    k = 11
    mixed = b"A" * 600 + rand(3, 400) + b"A" * 300
    reads = [b"A" * 70000, rand(1, 5000), rand(2, 300), mixed]
    for rate in (0.0, 0.4, 0.7, 0.999):
        check_positions(kc, reads, k, 2, rate, 0)
    m = check_index(kc, reads, k, 2, 0.4, 0, 100.0)
    assert m["selected_positions"] > 1 << 16


def test_count_beyond_one_byte(kc):
    """counts on both sides of 2^8 in one read: a run of 300 T-mers among 2-letter sequence"""
    k = 5
    reads = [rand(11, 200, 2) + b"T" * 330 + rand(12, 200, 2), rand(13, 500, 2)]
    for rate in (0.0, 0.3, 0.6, 0.999):
        check_positions(kc, reads, k, 1, rate, 0)


def test_count_beyond_three_bytes(kc):
    """2^24 + 4 096 positions of one k-mer, in 17 homopolymer reads: the fourth digit.  No model run at this size: every position has
    the one count there is, so every rank selects everything, read by read"""
    k = 11
    n_each = ((1 << 24) + 4096) // 17 + 1
    reads = [b"C" * (n_each + k)] * 17 + [b"ACGTTGCAAGGTCA" * 3]
    start, pos = kc.solid_positions(reads, k, 2, 0.4, 0, 0, capacity=17 * n_each + 64)
    assert np.array_equal(np.diff(start)[:17], np.full(17, n_each))
    for r in (0, 16):
        assert np.array_equal(pos[start[r]:start[r + 1]], np.arange(n_each, dtype=np.int32))
    want = sm.positions(reads[17:], k, 2, 0.4, 0, 0)[1]                     # (the last read's k-mers are its own: counts of 1 to 3)
    assert want.size and np.array_equal(pos[start[17]:], want)


# ---- the tandem rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 7])
def test_tandem_boundary(kc, T):
    """one k-mer exactly T times in a read (kept), another T + 1 times (removed); both high enough in count to be selected"""
    k = 11
    a, b = rand(21, k), rand(22, k)
    sep = [rand(30 + i, 40) for i in range(2 * T + 3)]
    read = b"".join(s + a for s in sep[:T]) + b"".join(s + b for s in sep[T:2 * T + 1]) + sep[-1]
    other = rand(23, 50) + a + rand(24, 50) + b + rand(25, 50)               # (so that T = 1 still gives a a global count above T)
    reads = [read, other]
    start, pos = check_positions(kc, reads, k, 0, 0.999, T)              # (rank n - 1: every position is selected before the tandem rule)
    keys = kmer_model.canonical_kmers(read, k)
    ka, kb = kmer_model.canonical_kmers(a + b"A", k)[0], kmer_model.canonical_kmers(b + b"A", k)[0]
    mine = pos[start[0]:start[1]]
    assert (keys == ka).sum() == T and (keys == kb).sum() == T + 1
    assert np.isin(np.flatnonzero(keys == ka), mine).all() and not np.isin(np.flatnonzero(keys == kb), mine).any()
    check_index(kc, reads, k, 0, 0.999, T, 100.0)


def test_tandem_fallback(kc):
    """tandem_freq = 1 and a 20 000-base random read present twice: every position has a global count of 2 and needs the test, none is
    removed, and 20 000 distinct k-mers do not fit the on-chip table; plus a read with an internal duplication, whose copies go"""
    k = 15
    long = rand(41, 20000)
    unit = rand(42, 600)
    dup = rand(43, 900) + unit + rand(44, 700) + unit + rand(45, 300)
    reads = [long, dup, long, dup]
    start, pos = check_positions(kc, reads, k, 2, 0.999, 1)
    assert start[1] - start[0] == 20000 - k and start[2] - start[1] < len(dup) - k - 2 * (600 - k)
    m = check_index(kc, reads, k, 2, 0.999, 1, 100.0)
    stats = kc.solid_last_stats()
    assert stats["tested_positions"] == sum(len(r) - k for r in reads) and stats["fallback_reads"] >= 2
    check_index(kc, [dup, rand(46, 500)], k, 0, 0.5, 1, 100.0)               # (few tested keys: they fit)
    assert kc.solid_last_stats()["fallback_reads"] == 0 and m["index_entries"] > 0


# ---- degenerate and error cases -----------------------------------------------------------------------------------------------------------
ZERO = dict.fromkeys(sm.FIELDS, 0)


def empty_index(kc):
    kmers, start, gpos = kc.index_dump()
    return kmers.size == 0 and gpos.size == 0 and start.tolist() == [0]


def test_nothing_to_index(kc):
    assert kc.index_solid([], 15, 2, 0.4, 100, 1.5, 0) == ZERO and empty_index(kc)
    got = kc.index_solid([rand(1, 100), rand(2, 200)], 15, 2, 0.4, 100, 1.5, 5000)       # all reads filtered
    assert got == ZERO and empty_index(kc)
    got = kc.index_solid([rand(1, 15), rand(2, 7), b""], 15, 0, 0.4, 100, 1.5, 0)        # reads <= k
    assert got == dict(ZERO, reads_kept=2, total_len=22) and empty_index(kc)
    start, pos = kc.solid_positions([rand(1, 15), b""], 15, 0, 0.4, 100, 0)
    assert start.tolist() == [0, 0, 0] and pos.size == 0


def test_repeat_rate_zero_removes_everything(kc):
    reads = [rand(5, 3000, 2)]
    m = check_index(kc, reads, 11, 1, 0.4, 0, 0.0)
    assert m["repetitive_frequency"] == 0 and m["selected_kmers"] == 0 and m["filtered_kmers"] == m["candidates"] > 0 and empty_index(kc)


@pytest.mark.parametrize("kwargs,word", [(dict(rate=-1.0), "repeat_kmer_rate"), (dict(rate=float("nan")), "repeat_kmer_rate"), (dict(min_freq=-1), "min_freq"),
                                         (dict(select_rate=1.0), "select_rate"), (dict(select_rate=-0.1), "select_rate"),
                                         (dict(select_rate=float("nan")), "select_rate"), (dict(k=18), "k = 18"), (dict(k=0), "k = 0")])
def test_bad_arguments(kc, kwargs, word):
    from genarchbench_amd.kmer import GabError
    args = dict(k=15, min_freq=2, select_rate=0.4, tandem_freq=100, rate=1.5, min_len=0)
    args.update(kwargs)
    with pytest.raises(GabError) as e:
        kc.index_solid([rand(1, 500)], **args)
    assert e.value.code == EINVAL and word in str(e.value)
    if "rate" not in kwargs:
        args.pop("rate")
        with pytest.raises(GabError) as e:
            kc.solid_positions([rand(1, 500)], **args)
        assert e.value.code == EINVAL and word in str(e.value)


def test_bad_byte_names_the_read(kc):
    from genarchbench_amd.kmer import GabError
    reads = [rand(1, 500), rand(2, 300)[:100] + b"N" + rand(3, 199), rand(4, 100)]
    for call in (lambda: kc.index_solid(reads, 15, 2, 0.4, 100, 1.5, 0), lambda: kc.solid_positions(reads, 15, 2, 0.4, 100, 0)):
        with pytest.raises(GabError) as e:
            call()
        assert e.value.code == EINVAL and "read 1 " in str(e.value)


def test_positions_erange_then_retry(kc):
    reads = [rand(61, 5000, 2), rand(62, 77, 2)]
    want_start, want_pos = sm.positions(reads, 11, 1, 0.4, 2, 0)
    start = np.full(3, -12345, np.int64); pos = np.full(want_pos.size - 1, -12345, np.int32)
    rc, need = kc.solid_positions_into(reads, 11, start, pos, 1, 0.4, 2, 0)
    assert rc == ERANGE and need == want_pos.size and (start == -12345).all() and (pos == -12345).all()
    pos = np.full(need, -12345, np.int32)
    rc, need = kc.solid_positions_into(reads, 11, start, pos, 1, 0.4, 2, 0)
    assert rc == 0 and np.array_equal(start, want_start) and np.array_equal(pos, want_pos)


def test_device_form_equals_host_form(kc):
    import torch
    from genarchbench_amd.kmer import pack_reads
    reads = [rand(71, 9000, 2), rand(72, 5000), rand(73, 40), rand(71, 9000, 2)]
    args = (11, 2, 0.4, 2)
    seq, off, ln = (torch.from_numpy(a).cuda() for a in pack_reads(reads))
    host = kc.index_solid(reads, *args, 1.5, 0)
    host_dump = kc.index_dump()
    assert kc.index_solid_device(seq, off, ln, *args, 1.5, 0) == host
    for a, b in zip(kc.index_dump(), host_dump):
        np.testing.assert_array_equal(a, b)
    start, pos = kc.solid_positions(reads, *args, 0)
    d_start = torch.full((len(reads) + 1,), -12345, dtype=torch.int64, device="cuda"); d_pos = torch.full((pos.size,), -12345, dtype=torch.int32, device="cuda")
    rc, n = kc.solid_positions_device(seq, off, ln, 11, d_start, d_pos, 2, 0.4, 2, 0)
    assert rc == 0 and n == pos.size and np.array_equal(d_start.cpu().numpy(), start) and np.array_equal(d_pos.cpu().numpy(), pos)
    rc, n = kc.solid_positions_device(seq, off, ln, 11, d_start, d_pos[:-1], 2, 0.4, 2, 0)
    assert rc == ERANGE and n == pos.size


def test_two_calls_on_one_handle_are_independent(kc):
    a = [rand(81, 6000, 2), rand(82, 300)]
    b = [rand(83, 700)]
    check_index(kc, a, 11, 2, 0.4, 2, 1.5)
    check_index(kc, b, 17, 0, 0.05, 0, 100.0)
    check_index(kc, a, 11, 2, 0.4, 2, 1.5)


def test_handle_state_rules(kc):
    """after a solid build the handle holds an index and no count; solid_positions leaves a count and an index alone; a pending
    partitioned build is dropped"""
    from genarchbench_amd.kmer import GabError
    reads = [rand(91, 3000, 2), rand(92, 800)]
    m = check_index(kc, reads, 11, 1, 0.4, 2, 1.5)
    for call in (lambda: kc.dump(), lambda: kc.query(np.zeros(1, np.uint64)), lambda: kc.spectrum(4), lambda: kc.last_stats()):
        with pytest.raises(GabError) as e:
            call()
        assert e.value.code == EINVAL
    assert set(kc.solid_last_phases()) == {"count_ms", "select_ms", "capacity_ms", "fill_ms", "sort_ms"} and all(v >= 0 for v in kc.solid_last_phases().values())
    kc.solid_positions([rand(93, 900)], 15, 0, 0.4, 0, 0)                    # the index of `reads` stays
    for got, want in zip(kc.index_dump(), (m["kmers"], m["start"], m["gpos"])):
        np.testing.assert_array_equal(got, want)
    want = kmer_model.model(reads, 11, 0)
    assert kc.count(reads, 11, 0) == {f: want[f] for f in kmer_model.FIELDS}
    kc.solid_positions([rand(93, 900)], 15, 0, 0.4, 0, 0)                    # the count of `reads` stays
    kmers, counts = kc.dump()
    assert np.array_equal(kmers, want["kmers"]) and np.array_equal(counts, want["counts"])
    with pytest.raises(GabError):
        kc.solid_last_phases()                                              # (the index is gone with the count)
    kc.index_minimizers(reads, 11, 5, 100.0, 0)
    with pytest.raises(GabError):
        kc.solid_last_stats()                                               # (a minimizer index is not a solid one)
    kc.index_part_begin(reads, 11, 5, 0, 2, 0)
    kc.index_solid(reads, 11, 1, 0.4, 2, 1.5, 0)
    with pytest.raises(GabError) as e:
        kc.index_part_finish(10, 5, 100.0)
    assert "no pending" in str(e.value)
    kc.index_part_begin(reads, 11, 5, 0, 2, 0)
    kc.solid_positions(reads, 11, 1, 0.4, 2, 0)
    with pytest.raises(GabError) as e:
        kc.index_part_finish(10, 5, 100.0)
    assert "no pending" in str(e.value)
