"""CPU: tests/minimizer_model.py against what the reference itself printed and built in its minimizer mode
(tests/golden/kmer_minimizer_expected.json, recorded by tests/golden/make_minimizer_golden.py): every row of the grid -- integers,
float strings, index digests -- and the tiny case array for array.  The model with the tie rule of yieldMinimizers switched off must
differ on at least one row, or the fixture could not tell the two readings apart."""
import functools
import json

import numpy as np
import pytest

from tests import kmer_model, minimizer_model as mm
from tests.util import GOLDEN

EXPECTED = json.load(open(f"{GOLDEN}/kmer_minimizer_expected.json"))
MIN_LEN = EXPECTED["min_len_exclusive"]
INTS = ("minimizers", "distinct", "repetitive_frequency", "filtered_kmers", "filtered_entries", "selected_kmers", "index_entries")
TEXTS = ("mean_frequency", "filtered_rate", "mean_frequency_kept", "minimizer_rate")


@functools.lru_cache(maxsize=None)
def reads_of(name):
    return kmer_model.load_reads([f"{GOLDEN}/{name}"])


@functools.lru_cache(maxsize=None)
def entries_of(name, k, window):
    return mm.entries(reads_of(name), k, window, MIN_LEN)      # (shared by the two rates of a grid point)


@pytest.mark.parametrize("name", sorted(EXPECTED["files"]))
def test_model_reproduces_the_reference_rows(name):
    for row in EXPECTED["files"][name]["rows"]:
        m = mm.index_of_entries(entries_of(name, row["k"], row["window"]), row["rate"])
        p = mm.printed(m)
        assert {f: m[f] for f in INTS} == {f: row[f] for f in INTS}, row
        assert {f: p[f] for f in TEXTS} == {f: row[f] for f in TEXTS}, row
        assert mm.digest(m["kmers"], m["start"], m["gpos"]) == row["index_sha256"], row


def test_model_equals_the_tiny_index_array_for_array():
    t = EXPECTED["tiny"]
    z = np.load(f"{GOLDEN}/kmer_minimizer_tiny.npz")
    reads = [r for r in reads_of(t["file"]) if len(r) > MIN_LEN][:t["kept_reads"]]
    assert [len(r) for r in reads] == z["read_lengths"].tolist()
    m = mm.build_index(reads, t["k"], t["window"], t["rate"], MIN_LEN)
    for f in ("kmers", "start", "gpos", "repetitive"):
        assert np.array_equal(m[f], z[f]), f
    assert {f: m[f] for f in INTS} == {f: t[f] for f in INTS}
    assert mm.digest(z["kmers"], z["start"], z["gpos"]) == t["index_sha256"]


def test_without_the_tie_rule_a_row_differs():
    name = "kmer_small.fa"
    rows = [r for r in EXPECTED["files"][name]["rows"] if r["k"] == 15 and r["rate"] == 100]
    differ = [r["window"] for r in rows if mm.build_index(reads_of(name), 15, r["window"], 100, MIN_LEN, tie_rule=False)["index_entries"] != r["index_entries"]]
    assert differ, "the fixture does not separate the tie rule from a plain sliding-window minimum"
    assert 1 not in differ      # window 1 has no queue at all


def test_sketch_small_cases_by_hand():
    # window 1: every position; a homopolymer: 0, w, 2w, ... from the start of the run
    assert mm.sketch(b"ACGTACGTAC", 3, 1).tolist() == list(range(7))
    assert mm.sketch(b"A" * 40, 5, 4).tolist() == list(range(0, 35, 4))
    assert mm.sketch(b"A" * 40, 5, 4, tie_rule=False).tolist() == list(range(32))      # the leftmost of the window's equals
    assert mm.sketch(b"ACGT", 4, 3).size == 0 and mm.sketch(b"ACGTA", 4, 3).tolist() == [0]
