"""CPU: the host side of the k-mer counter's key-space partitions.  gab_kmer_part_of against a numpy restatement of the hash, and
the table a partitioned call allocates first against the distinct keys tests/kmer_model.py gives every partition of the two fixtures:
at most half the slots, which is the condition under which tests/test_kmer_parts_gpu.py may assert that no call was repeated."""
import json

import numpy as np
import pytest

from tests import kmer_model
from tests.kmer_parts_util import SLOTS, np_part_of
from tests.util import GOLDEN

EXPECTED = json.load(open(f"{GOLDEN}/kmer_expected.json"))
EINVAL = -22


@pytest.fixture(scope="module")
def fixture_models():
    reads = {name: kmer_model.load_reads([f"{GOLDEN}/{name}"]) for name in EXPECTED["files"]}
    return {(name, k): kmer_model.model(r, k) for name, r in reads.items() for k in (15, 17)}


@pytest.mark.parametrize("nparts", [1, 2, 3, 7, 64])
def test_part_of_equals_the_numpy_hash(nparts):
    from genarchbench_amd.kmer import part_of
    rng = np.random.default_rng(nparts)
    keys = np.concatenate([rng.integers(0, 1 << 34, 200_000).astype(np.uint64), np.array([0, 1, 2, 3, (1 << 34) - 1], np.uint64)])
    got = part_of(keys, nparts)
    assert got.min() >= 0 and got.max() < nparts
    np.testing.assert_array_equal(got, np_part_of(keys, nparts))
    if nparts == 1:
        assert not got.any()
    else:                                          # every partition is used, none by much more than its share
        share = np.bincount(got, minlength=nparts) / keys.size
        assert share.min() > 0.9 / nparts and share.max() < 1.1 / nparts


def test_part_of_single_call_and_bad_nparts():
    import ctypes as C
    from genarchbench_amd import GabError
    from genarchbench_amd._lib import lib
    from genarchbench_amd.kmer import MAX_PARTS, part_of, table_slots
    assert MAX_PARTS == 64
    keys = np.arange(1000, dtype=np.uint64) * np.uint64(2654435761)
    one = [lib().gab_kmer_part_of(C.c_uint64(int(x)), C.c_int(7)) for x in keys[:50]]
    assert one == np_part_of(keys[:50], 7).tolist()
    for bad in (0, -1, 65):
        assert lib().gab_kmer_part_of(C.c_uint64(5), C.c_int(bad)) == EINVAL
        with pytest.raises(GabError) as e:
            part_of(keys, bad)
        assert e.value.code == EINVAL and "nparts = %d" % bad in str(e.value)
        with pytest.raises(GabError) as e:
            table_slots(1000, 17, bad)
        assert e.value.code == EINVAL and "nparts = %d" % bad in str(e.value)
    for k in (0, 18):
        with pytest.raises(GabError) as e:
            table_slots(1000, k, 2)
        assert e.value.code == EINVAL


def test_table_slots():
    from genarchbench_amd.kmer import table_slots
    for positions, k in ((0, 17), (1, 17), (63, 17), (64, 17), (65, 17), (1000, 3), (229_700_000, 17), (229_700_000, 12), (1 << 31, 17)):
        keys = min(max(positions, 1), 4 ** k)
        whole = max(16 * SLOTS, (2 * keys + SLOTS - 1) // SLOTS * SLOTS)      # today's table: twice the keys, whole lines, 16 lines at least
        assert table_slots(positions, k, 1) == whole
        last = whole
        for nparts in (2, 3, 8, 64):
            s = table_slots(positions, k, nparts)
            assert s % SLOTS == 0 and 16 * SLOTS <= s <= last      # never below the floor, never above a smaller split's
            last = s
            share = -(-keys // nparts)
            assert s >= min(whole, 2 * share)                      # room for an even share at half full
    assert table_slots(229_700_000, 17, 8) < table_slots(229_700_000, 17, 1) / 6      # the table of a partition shrinks to its share (x 1.25)


@pytest.mark.parametrize("nparts", [2, 3, 8])
@pytest.mark.parametrize("k", [15, 17])
@pytest.mark.parametrize("name", sorted(EXPECTED["files"]))
def test_fixture_partitions_fill_at_most_half_their_table(fixture_models, name, k, nparts):
    from genarchbench_amd.kmer import part_of, table_slots
    m = fixture_models[(name, k)]
    distinct = np.bincount(part_of(m["kmers"], nparts), minlength=nparts)
    assert distinct.sum() == m["distinct"]
    assert 2 * int(distinct.max()) <= table_slots(m["positions"], k, nparts), (distinct.tolist(), table_slots(m["positions"], k, nparts))
