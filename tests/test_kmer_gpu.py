"""GPU: the k-mer counter (gab_kmer_*, through genarchbench_amd.kmer) against the reference's recorded numbers and the numpy model of
tests/kmer_model.py.  Every comparison is equality; every output buffer is pre-filled with a sentinel by the Python mirror.
Most of this file's run time is the model on the CPU (np.unique over up to 250 M k-mers)."""
import json

import numpy as np
import pytest

from tests import kmer_model
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

EXPECTED = json.load(open(f"{GOLDEN}/kmer_expected.json"))
CASES = [(name, int(k)) for name, f in sorted(EXPECTED["files"].items()) for k in sorted(f["k"], key=int)]
ACGT = np.frombuffer(b"ACGT", np.uint8)
EINVAL, ERANGE = -22, -34


@pytest.fixture(scope="module")
def kc():
    from genarchbench_amd.kmer import KmerCounter
    e = KmerCounter()
    yield e
    e.close()


@pytest.fixture(scope="module")
def fixture_reads():
    return {name: kmer_model.load_reads([f"{GOLDEN}/{name}"]) for name in EXPECTED["files"]}


def rand_reads(seed, lengths):
    rng = np.random.default_rng(seed)
    return [ACGT[rng.integers(0, 4, n)].tobytes() for n in lengths]


def check_all(kc, reads, k, min_len, nbins=300, dump=True):
    """all six fields, spectrum(nbins), dump() and last_stats()['merged'] == the model"""
    m = kmer_model.model(reads, k, min_len)
    got = kc.count(reads, k, min_len)
    assert got == {f: m[f] for f in kmer_model.FIELDS}
    np.testing.assert_array_equal(kc.spectrum(nbins), kmer_model.spectrum(m["counts"], nbins))
    st = kc.last_stats()
    assert st["merged"] == m["merged"]
    assert st["probes"] >= m["positions"] - m["merged"]          # one table line per insert at least
    if dump:
        kmers, counts = kc.dump()
        np.testing.assert_array_equal(kmers, m["kmers"])
        np.testing.assert_array_equal(counts.astype(np.int64), m["counts"])
    return m


@pytest.mark.parametrize("name,k", CASES)
def test_golden(kc, fixture_reads, name, k):
    want = EXPECTED["files"][name]["k"][str(k)]
    got = kc.count(fixture_reads[name], k)
    assert (got["hash_size"], got["total_kmers"]) == (want["hash_size"], want["total_kmers"])


@pytest.mark.parametrize("name,k", CASES)
def test_fixtures_vs_model(kc, fixture_reads, name, k):
    check_all(kc, fixture_reads[name], k, 5000)


@pytest.mark.parametrize("k", [1, 2, 3, 16, 17])
def test_random_batch(kc, k):
    """k = 1, 2, 3: every count wraps many times and the table is nearly empty"""
    lengths = [int(x) for x in np.random.default_rng(k).integers(1, 9000, 300)] + [5000, 5001, k, k + 1, 0]
    m = check_all(kc, rand_reads(100 + k, lengths), k, 5000)
    if k <= 3:
        assert m["distinct"] <= 4 ** k and m["total_kmers"] > m["distinct"]


def test_min_len_zero_and_reads_not_longer_than_k(kc):
    reads = rand_reads(5, [0, 1, 16, 17, 18, 19, 64, 65, 4096 + 17, 4097 + 17, 81])
    m = check_all(kc, reads, 17, 0)
    assert m["reads_kept"] == 10 and m["positions"] == sum(max(len(r) - 17, 0) for r in reads)


def test_one_read_of_2m_bases(kc):
    check_all(kc, rand_reads(6, [2_000_000]), 17, 5000)


def test_50000_reads_of_5001_bases(kc):
    m = check_all(kc, rand_reads(7, [5001] * 50000), 16, 5000, dump=False)
    assert m["reads_kept"] == 50000


def test_one_base_repeated(kc):
    """one key, count = positions: the merge path, and 64 lanes per wave adding to one slot"""
    for base, n, k in ((b"A", 300_000, 17), (b"t", 70_001, 4), (b"G", 5001, 1)):
        m = check_all(kc, [base * n], k, 5000)
        assert (m["distinct"], m["max_count"]) == (1, n - k)
        assert m["total_kmers"] == (n - k + 255) // 256 and m["hash_size"] == 1


def test_short_period_repeats(kc):
    reads = [b"AC" * 4000, b"ACG" * 3000, b"acgt" * 2000, (b"A" * 100 + b"C" * 100) * 40]
    check_all(kc, reads, 15, 5000)
    check_all(kc, reads, 2, 5000)


def test_all_filtered_and_empty(kc):
    zeros = {f: 0 for f in kmer_model.FIELDS}
    got = kc.count(rand_reads(8, [5000, 4000, 17, 1]), 17)
    assert got == zeros
    np.testing.assert_array_equal(kc.spectrum(10), np.zeros(10, np.int64))
    kmers, counts = kc.dump()
    assert kmers.size == 0 and counts.size == 0
    np.testing.assert_array_equal(kc.query(np.arange(5, dtype=np.uint64)), np.zeros(5, np.uint32))
    assert kc.count([], 17) == zeros
    assert kc.count(rand_reads(9, [10, 12]), 17, 0) == dict(zeros, reads_kept=2)      # kept by the filter, not longer than k


def test_query(kc):
    from genarchbench_amd import GabError
    k = 17
    reads = rand_reads(10, [300_000, 6000, 200_000])
    m = check_all(kc, reads, k, 5000, dump=False)
    rng = np.random.default_rng(11)
    present = m["kmers"][rng.integers(0, m["kmers"].size, 400_000)]
    rc = np.array([kmer_model.revcomp_value(int(x), k) for x in present[:20_000]], np.uint64)
    absent = rng.integers(0, 4 ** k, 700_000).astype(np.uint64)
    q = np.concatenate([present, rc, absent])
    assert q.size >= 1_000_000
    # expected: a sorted look-up of the canonical form, computed here independently of the library
    rc_all = np.zeros_like(q)
    x = q.copy()
    for _ in range(k):
        rc_all = (rc_all << np.uint64(2)) | (~x & np.uint64(3))
        x >>= np.uint64(2)
    canon = np.minimum(q, rc_all)
    at = np.searchsorted(m["kmers"], canon)
    at[at == m["kmers"].size] = 0
    want = np.where(m["kmers"][at] == canon, m["counts"][at], 0).astype(np.uint32)
    got = kc.query(q)
    np.testing.assert_array_equal(got, want)
    assert (got[:present.size] > 0).all() and (got[present.size:present.size + rc.size] > 0).all() and (want[-absent.size:] == 0).any()
    with pytest.raises(GabError) as e:
        kc.query(np.array([1, 4 ** k], np.uint64))
    assert e.value.code == EINVAL


def test_device_entry_point_and_stream(kc, fixture_reads):
    import torch
    from genarchbench_amd.kmer import pack_reads
    reads = fixture_reads["kmer_small.fa"] + rand_reads(12, [70_000, 5001, 100])
    seq, off, ln = pack_reads(reads)
    host = kc.count((seq, off, ln), 17)
    host_dump = kc.dump()
    host_merged = kc.last_stats()["merged"]
    d = [torch.from_numpy(x).cuda() for x in (seq, off, ln)]
    assert kc.count_device(*d, 17) == host
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = kc.count_device(*d, 17, stream=side.cuda_stream)
    assert got == host and kc.last_stats()["merged"] == host_merged
    dev_dump = kc.dump()
    np.testing.assert_array_equal(dev_dump[0], host_dump[0])
    np.testing.assert_array_equal(dev_dump[1], host_dump[1])
    m = kmer_model.model(reads, 17)
    assert host == {f: m[f] for f in kmer_model.FIELDS}
    # reads anywhere in the slab, in any order, with unused (and invalid) bytes between them
    slab = np.full(seq.size + 1000, ord("N"), np.uint8)
    slab[500:500 + seq.size] = seq
    order = np.random.default_rng(13).permutation(len(reads))
    assert kc.count((slab, (off + 500)[order], ln[order]), 17) == host
    d2 = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (slab, (off + 500)[order], ln[order])]
    assert kc.count_device(*d2, 17) == host


def test_handle_is_reusable(kc, fixture_reads):
    """small after large, another k on the same handle, a second handle: the results are independent"""
    from genarchbench_amd.kmer import KmerCounter
    big = rand_reads(14, [1_500_000, 800_000])
    small = fixture_reads["kmer_small.fa"]
    ms = {k: kmer_model.model(small, k) for k in (17, 11)}
    mb = kmer_model.model(big, 17)
    for reads, k, m in ((big, 17, mb), (small, 17, ms[17]), (small, 11, ms[11]), (small, 17, ms[17]), (big, 17, mb)):
        assert kc.count(reads, k) == {f: m[f] for f in kmer_model.FIELDS}
    np.testing.assert_array_equal(kc.dump()[1].astype(np.int64), mb["counts"])
    other = KmerCounter()
    assert other.count(small, 11) == {f: ms[11][f] for f in kmer_model.FIELDS}
    np.testing.assert_array_equal(kc.dump()[0], mb["kmers"])      # the first handle still holds ITS last table
    other.close()


def test_errors(fixture_reads):
    from genarchbench_amd import GabError
    from genarchbench_amd.kmer import KmerCounter
    e = KmerCounter()
    for call in (lambda: e.spectrum(10), lambda: e.query(np.zeros(3, np.uint64)), lambda: e.dump(), lambda: e.last_stats()):
        with pytest.raises(GabError) as err:          # before any count
            call()
        assert err.value.code == EINVAL
    reads = fixture_reads["kmer_small.fa"]
    for k in (0, 18, -1):
        with pytest.raises(GabError) as err:
            e.count(reads, k)
        assert err.value.code == EINVAL and "k = %d" % k in str(err.value)
    bad = [reads[0], reads[1][:100] + b"N" + reads[1][101:], reads[2]]
    with pytest.raises(GabError) as err:
        e.count(bad, 17)
    assert err.value.code == EINVAL and "read 1 " in str(err.value)
    with pytest.raises(GabError) as err:              # a failed count leaves no table behind
        e.spectrum(10)
    assert err.value.code == EINVAL
    with pytest.raises(GabError) as err:              # a short read that the filter drops is validated too
        e.count([reads[0], b"ACGTXACGT"], 17)
    assert err.value.code == EINVAL and "read 1 " in str(err.value)
    m = kmer_model.model(reads, 17)
    assert e.count(reads, 17) == {f: m[f] for f in kmer_model.FIELDS}
    with pytest.raises(GabError) as err:
        e.spectrum(1)
    assert err.value.code == EINVAL
    # dump with a short buffer: GAB_ERANGE and the needed size, nothing written; then success
    kmers = np.full(m["distinct"] - 1, 0xDEADBEEFDEADBEEF, np.uint64); counts = np.full(m["distinct"] - 1, 0xDEADBEEF, np.uint32)
    rc, need = e.dump_into(kmers, counts)
    assert (rc, need) == (ERANGE, m["distinct"])
    assert (kmers == 0xDEADBEEFDEADBEEF).all() and (counts == 0xDEADBEEF).all()
    kmers = np.full(need, 0xDEADBEEFDEADBEEF, np.uint64); counts = np.full(need, 0xDEADBEEF, np.uint32)
    assert e.dump_into(kmers, counts) == (0, need)
    np.testing.assert_array_equal(kmers, m["kmers"])
    np.testing.assert_array_equal(counts.astype(np.int64), m["counts"])
    e.close()


def test_spectrum_bins(kc, fixture_reads):
    reads = fixture_reads["kmer_small.fa"]
    m = kmer_model.model(reads, 11)
    kc.count(reads, 11)
    for nbins in (2, 3, 257, 1024, 1025, 5000):        # around the kernel's LDS-resident bins, and past the largest count
        np.testing.assert_array_equal(kc.spectrum(nbins), kmer_model.spectrum(m["counts"], nbins))


def test_large_run_200_mbp(kc):
    """about 200 Mbp at k = 17: 20 000 reads of 10 kb, half of them copies (with 2 % substitutions) of the other half, so that
    counts above 1 are common"""
    rng = np.random.default_rng(15)
    base = ACGT[rng.integers(0, 4, (10_000, 10_000))]
    copy = base.copy()
    hit = rng.random(copy.shape) < 0.02
    copy[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    reads = [r.tobytes() for r in base] + [r.tobytes() for r in copy]
    del base, copy, hit
    m = kmer_model.model(reads, 17)
    assert m["positions"] == 20_000 * (10_000 - 17)
    got = kc.count(reads, 17)
    assert got == {f: m[f] for f in kmer_model.FIELDS}
    np.testing.assert_array_equal(kc.spectrum(300), kmer_model.spectrum(m["counts"], 300))
    assert kc.last_stats()["merged"] == m["merged"]
