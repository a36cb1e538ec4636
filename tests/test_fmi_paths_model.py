"""CPU: the route model of the fmi kernels (oracle_fmi_paths / oracle.pyoracle.fmi_paths) against the oracle itself, and every row of
tests/fmi_path_cases.py against what it is there to exercise.  tests/test_fmi_paths_gpu.py holds the library against this model."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from tests import fmi_path_cases as cases
from tests.util import GOLDEN, read_fasta_codes, read_fastq_reads
from tools import mkindex


def oracle_index(idx):
    oidx = pyoracle.FmIndex()
    cnt = (C.c_int64 * 5)(*[int(x) for x in idx.count])
    pyoracle.lib().oracle_fmi_from_arrays(C.byref(oidx), C.c_int64(idx.ref_seq_len), cnt, idx.cp_occ.ctypes.data_as(C.c_void_p),
                                          C.c_int64(idx.sentinel_index))
    return oidx


_memo = {}


def oracle_of(name, msl):
    """(smems, read_off, calls) of pyoracle.fmi for an input, computed once"""
    if (name, msl) not in _memo:
        idx, reads = cases.load(name)
        _memo[name, msl] = pyoracle.fmi(oracle_index(idx), reads, msl, want_calls=True)
    return _memo[name, msl]


def model_of(case, **over):
    key = (case.name, tuple(sorted(over.items())))
    if key not in _memo:
        idx, reads = cases.load(case.input)
        kw = dict(cases.model_args(case.env, reads.stride), **over)
        _memo[key] = pyoracle.fmi_paths(oracle_index(idx), reads, case.msl, slot_cap=cases.SLOT_CAP, detail=True, **kw)
    return _memo[key]


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_case_reaches_its_route_and_model_agrees_with_oracle(case):
    w, woff, calls = oracle_of(case.input, case.msl)
    p, x = model_of(case)
    print(case.name, p, {k: v for k, v in x.items() if k != "per_read"})
    assert tuple(p) == pyoracle.FMI_PATH_KEYS
    assert p["index_ext"] + p["table_ext"] == calls
    assert x["smems"] == len(w)
    np.testing.assert_array_equal(x["per_read"], np.diff(woff))
    assert p["overflow_reads"] == (np.diff(woff) > cases.SLOT_CAP).sum() and p["max_per_read"] == np.diff(woff).max()
    assert x["cp_occ_records"] >= p["index_ext"] and x["cp_occ_records"] <= 2 * p["index_ext"]
    assert p["spills"] <= p["positions"] and p["wide_entries"] >= 24 * p["wide_items"] * (p["wide_min"] == 24)
    if p["kmer_depth"] == 0:
        assert p["table_ext"] == 0
    assert case.want(p, x), "the case no longer reaches the route it is there for"


@pytest.mark.parametrize("name", ["handover_default", "p1_overflow_lds", "three_batches", "depth_9"])
def test_hand_over_moves_positions_but_not_work(name):
    """positions + wide_cands, the extensions and the SMEMs are the same whatever the threshold; without hand-over wide_* are 0"""
    case = next(c for c in cases.CASES if c.name == name)
    runs = [model_of(case, wide_min=m) for m in (0, 2, 4, 24)]
    p0 = runs[0][0]
    assert p0["wide_items"] == p0["wide_entries"] == p0["wide_cands"] == 0
    for p, x in runs:
        assert p["positions"] + p["wide_cands"] == p0["positions"]
        assert p["index_ext"] + p["table_ext"] == p0["index_ext"] + p0["table_ext"] and x["smems"] == runs[0][1]["smems"]
        assert p["table_ext"] <= p0["table_ext"] and (p["wide_min"] == 0 or p["wide_items"] >= runs[-1][0]["wide_items"])


def test_table_depths_differ():
    """table_ext grows with every depth of the table, index_ext shrinks by as much; 0 without a table and at depth 1, whose entries
    (single bases) no extension produces"""
    by = {d: model_of(next(c for c in cases.CASES if c.name == f"depth_{d}"))[0] for d in cases.NEIGHBOUR_DEPTHS}
    assert by[0]["table_ext"] == 0 and by[1]["table_ext"] == 0
    for a, b in zip(cases.NEIGHBOUR_DEPTHS, cases.NEIGHBOUR_DEPTHS[1:]):
        assert by[a]["table_ext"] < by[b]["table_ext"] or b == 1
        assert by[a]["table_ext"] + by[a]["index_ext"] == by[b]["table_ext"] + by[b]["index_ext"]


def test_global_form_has_no_ring_no_table_no_hand_over():
    case = next(c for c in cases.CASES if c.name == "stride_257")
    p, x = model_of(case)
    assert p["lds_entries"] == p["kmer_depth"] == p["wide_min"] == p["list_entry_bytes"] == p["table_ext"] == p["wide_items"] == 0
    assert 0 < p["spills"] <= p["positions"]                                  # every position with a list
    a, b = model_of(next(c for c in cases.CASES if c.name == "stride_255")), model_of(next(c for c in cases.CASES if c.name == "stride_256"))
    np.testing.assert_array_equal(a[1]["per_read"], x["per_read"]); np.testing.assert_array_equal(b[1]["per_read"], x["per_read"])
    assert a[0] == b[0]                                                       # the stride alone changes nothing inside a form
    for na in ("stride_255", "stride_256"):                                   # the same SMEMs in all three layouts
        for f in ("rid", "m", "n", "k", "l", "s"):
            np.testing.assert_array_equal(oracle_of("edge257", 19)[0][f], oracle_of("edge" + na[-3:], 19)[0][f])


def test_pass_one_overflow_is_put_off_whole():
    """a read whose pass-1 SMEMs of the seeding kernel exceed the slot runs its pass 2 in the second round: no candidates from it"""
    for name in ("p1_overflow_lds", "p1_overflow_global"):
        p, x = model_of(next(c for c in cases.CASES if c.name == name))
        assert 0 < x["deferred_reads"] <= x["p1_over_reads"] <= p["overflow_reads"]


def test_golden_smem_count():
    ref = read_fasta_codes(f"{GOLDEN}/fmi_small.ref.fa")
    reads = read_fastq_reads(f"{GOLDEN}/fmi_small.reads.fq")
    oidx = oracle_index(mkindex.FmIndex(ref))
    p, x = pyoracle.fmi_paths(oidx, reads, 19, 12, 8, 24, reads.stride <= 256, detail=True)
    want = sum(line.count("[") for line in open(f"{GOLDEN}/fmi_small.expected.txt"))
    w, woff, calls = pyoracle.fmi(oidx, reads, 19, want_calls=True)
    assert x["smems"] == want == len(w) and p["index_ext"] + p["table_ext"] == calls
