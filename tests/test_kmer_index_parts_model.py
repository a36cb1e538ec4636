"""CPU: the model of the partitioned minimizer index (tests/minimizer_parts_util.py) against the unpartitioned model and the reference's
record, and the conditions -- worked out from the model alone -- that tests/test_kmer_index_parts_gpu.py relies on."""
import functools
import json

import numpy as np
import pytest

from tests import kmer_model, minimizer_model as mm, minimizer_parts_util as pu
from tests.kmer_parts_util import np_part_of
from tests.util import GOLDEN

EXPECTED = json.load(open(f"{GOLDEN}/kmer_minimizer_expected.json"))
MIN_LEN = EXPECTED["min_len_exclusive"]
ACGT = np.frombuffer(b"ACGT", np.uint8)
POINTS = [(15, 10), (11, 5), (17, 19)]
RATES = (100, 3)
NPARTS = (2, 3, 5)
RESULT_FIELDS = ("minimizers", "distinct", "repetitive_frequency", "filtered_kmers", "filtered_entries", "selected_kmers", "index_entries")


def rand(seed, n):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


@functools.lru_cache(maxsize=None)
def reads_of(name):
    return kmer_model.load_reads([f"{GOLDEN}/{name}"])


@functools.lru_cache(maxsize=None)
def entries_of(name, k, window):
    return mm.entries(reads_of(name), k, window, MIN_LEN)


def row_of(name, k, window, rate):
    return next(r for r in EXPECTED["files"][name]["rows"] if (r["k"], r["window"], r["rate"]) == (k, window, rate))


def poly_a_reads():
    return [rand(8, 900) + b"A" * 700 + rand(9, 800), rand(10, 1200)]


def rate_for(total, unique, want):
    """a float rate with repetitive_frequency(total, unique, rate) == want (checked with the model's own arithmetic)"""
    mean = np.float32(total) / np.float32(unique + 1)
    rate = float(np.float32((want + 0.5) / float(mean)))
    assert mm.repetitive_frequency(total, unique, rate) == want
    return rate


@pytest.mark.parametrize("nparts", NPARTS)
@pytest.mark.parametrize("k,window", POINTS)
@pytest.mark.parametrize("name", sorted(EXPECTED["files"]))
def test_restricted_models_merge_to_the_whole(name, k, window, nparts):
    found = entries_of(name, k, window)
    for rate in RATES:
        whole = mm.index_of_entries(found, rate)
        parts = pu.restrict(found, rate, nparts)
        row = row_of(name, k, window, rate)
        assert pu.sum_fields(parts) == {f: whole[f] for f in mm.FIELDS}
        assert {f: pu.sum_fields(parts)[f] for f in RESULT_FIELDS} == {f: row[f] for f in RESULT_FIELDS}
        kmers, start, gpos = pu.merge([(p["kmers"], p["start"], p["gpos"]) for p in parts])
        np.testing.assert_array_equal(kmers, whole["kmers"])
        np.testing.assert_array_equal(start, whole["start"])
        np.testing.assert_array_equal(gpos, whole["gpos"])
        assert mm.digest(kmers, start, gpos) == row["index_sha256"]
        np.testing.assert_array_equal(np.sort(np.concatenate([p["repetitive"] for p in parts])), whole["repetitive"])
        for i, p in enumerate(parts):
            assert (np_part_of(p["keys"], nparts) == i).all()


@pytest.mark.parametrize("nparts", NPARTS)
@pytest.mark.parametrize("k,window", POINTS)
@pytest.mark.parametrize("name", sorted(EXPECTED["files"]))
def test_no_partition_outgrows_its_first_table(name, k, window, nparts):
    """The first capacity table of a partition has room for share + share / 4 + 64 keys at half full, share = ceil(min(positions, 4^k)
    / nparts): a partition with no more keys than that cannot fill it, so the GPU test may assert retried == 0."""
    positions = pu.positions_of(reads_of(name), k, MIN_LEN)
    keys = min(positions, 4 ** k)
    share = (keys + nparts - 1) // nparts
    room = share + share // 4 + 64
    assert room == pu.first_table_room(positions, k, nparts)
    slots = pu.first_table_slots(positions, k, nparts)
    for p in pu.restrict(entries_of(name, k, window), 100, nparts):
        assert p["distinct"] <= room and 2 * p["distinct"] <= slots      # (at most half full)


def test_the_poly_a_key_separates_the_global_threshold_from_a_local_one():
    """reads with a poly-A stretch, k = 15, w = 5: the partition that owns key 0 would compute a HIGHER threshold from its own totals
    than the whole input gives, and the key's capacity lies between the two -- removed globally, kept by a build that filters with
    partition-local totals"""
    k, w = 15, 5
    found = mm.entries(poly_a_reads(), k, w, 0)
    base = mm.index_of_entries(found, 1e6)
    M, U = base["minimizers"], base["distinct"]
    caps = np.diff(base["start"])
    cap = int(caps.max())
    assert (M, U, cap, int(base["kmers"][caps.argmax()])) == (1093, 957, 137, 0)
    rate = rate_for(M, U, cap - 1)
    local = {}
    for nparts in NPARTS:
        parts = pu.restrict(found, rate, nparts)
        owner = int(np_part_of(np.zeros(1, np.uint64), nparts)[0])
        assert owner == 0
        own = parts[owner]
        assert own["repetitive_frequency"] == cap - 1 == 136 and 0 in own["repetitive"].tolist()
        local[nparts] = mm.repetitive_frequency(own["minimizers"], own["distinct"], rate)
        assert local[nparts] > cap - 1 and cap <= local[nparts]
    assert local == {2: 154, 3: 173, 5: 204}


def test_sixty_bases_over_64_partitions():
    found = mm.entries([rand(5, 60)], 15, 5, 0)
    parts = pu.restrict(found, 100, 64)
    assert int(np.unique(found[0]).size) == sum(p["distinct"] for p in parts)
    assert sum(p["distinct"] == 0 for p in parts) >= 40 and sum(p["distinct"] > 0 for p in parts) >= 2
