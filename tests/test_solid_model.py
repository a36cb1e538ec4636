"""tests/solid_model.py against what the reference itself built and printed (tests/golden/make_solid_golden.py): every row of
kmer_solid_expected.json and the arrays of kmer_solid_tiny.npz.  No GPU."""
import functools
import json
import os

import numpy as np
import pytest

from tests import kmer_model, minimizer_model, solid_model

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXP = json.load(open(os.path.join(GOLD, "kmer_solid_expected.json")))
ROWS = [(name, i) for name in sorted(EXP["files"]) for i in range(len(EXP["files"][name]["rows"]))]
LINES = ("mean_frequency", "repetitive_frequency", "filtered_entries", "filtered_rate", "selected_kmers", "index_entries", "mean_index_frequency")


@functools.lru_cache(maxsize=None)
def reads_of(name):
    return tuple(kmer_model.load_reads([os.path.join(GOLD, name)]))


def tiny_reads():
    t = EXP["tiny"]
    return [r for r in reads_of(t["file"]) if len(r) > 5000][:t["kept_reads"]]


def check_row(m, row):
    want = {f: row[f] for f in LINES}
    assert solid_model.printed(m) == want
    assert (m["indexed_kmers"], m["filtered_kmers"]) == (row["indexed_kmers"], row["filtered_kmers"])
    assert minimizer_model.digest(m["kmers"], m["start"], m["gpos"]) == row["index_sha256"]


@pytest.mark.parametrize("name,i", ROWS)
def test_model_matches_every_golden_row(name, i):
    row = EXP["files"][name]["rows"][i]
    m = solid_model.build_index(list(reads_of(name)), row["k"], row["min_freq"], row["select_rate"], row["tandem_freq"], row["rate"],
                                EXP["min_len_exclusive"])
    check_row(m, row)
    assert m["selected_kmers"] == m["indexed_kmers"] + m["empty"].size and m["candidates"] == m["selected_kmers"] + m["filtered_kmers"]


def test_model_matches_the_tiny_arrays():
    t = EXP["tiny"]
    z = np.load(os.path.join(GOLD, "kmer_solid_tiny.npz"))
    reads = tiny_reads()
    assert [len(r) for r in reads] == z["read_lengths"].tolist()
    m = solid_model.build_index(reads, t["k"], t["min_freq"], t["select_rate"], t["tandem_freq"], t["rate"])
    check_row(m, t)
    for f in ("kmers", "start", "gpos", "repetitive"):
        assert np.array_equal(m[f], z[f]), f


@pytest.mark.parametrize("name", sorted(EXP["files"]))
def test_goldens_hold_empty_lists_and_removed_keys(name):
    rows = EXP["files"][name]["rows"]
    assert any(r["selected_kmers"] > r["indexed_kmers"] for r in rows), "no golden row of this fixture has a key with an empty list"
    assert any(r["filtered_kmers"] > 0 for r in rows), "no golden row of this fixture has a removed key"


def test_positions_agree_with_the_index():
    """solid_positions is the selection the index is built from: as many positions as capacities"""
    t = EXP["tiny"]
    reads = tiny_reads()
    start, pos = solid_model.positions(reads, t["k"], t["min_freq"], t["select_rate"], t["tandem_freq"])
    m = solid_model.build_index(reads, t["k"], t["min_freq"], t["select_rate"], t["tandem_freq"], t["rate"])
    assert pos.size == m["selected_positions"] == start[-1] and all((np.diff(pos[a:b]) > 0).all() for a, b in zip(start[:-1], start[1:]))


def test_rank_is_a_float_product():
    assert solid_model.rank_of(0.4, 10) == 4 and solid_model.rank_of(0.0, 7) == 0 and solid_model.rank_of(0.999, 1) == 0
    top = float(np.nextafter(np.float32(1), np.float32(0)))                   # the largest select_rate there is: the rank stays inside the array
    assert solid_model.rank_of(top, 1 << 25) == (1 << 25) - 2 and all(solid_model.rank_of(top, n) == n - 1 for n in (1, 3, 4097, (1 << 24) - 1))
    assert solid_model.rank_of(0.05, 4097) == int(np.float32(0.05) * np.float32(4097))
