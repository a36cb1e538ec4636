"""CPU: the cases of tests/kmer_table_cases.py build with their preconditions, and expected_probes is what a plain sequential table
of 8-slot lines counts, whatever the order of the inserts -- the reason why tests/test_kmer_table_gpu.py may assert `probes` with ==
where lines spill."""
import numpy as np
import pytest

from tests import kmer_model
from tests import kmer_table_cases as tc
from tests.kmer_parts_util import SLOTS, np_line_of, np_part_of, restrict, merged_keys

ORDERS = 20


def simulate(home_lines, nlines, order):
    """a sequential open-addressing table: every key (distinct, given by its home line) goes into the first line from its home on,
    wrapping, that has a free slot -> (lines visited in all, slots taken per line)"""
    taken = [0] * nlines
    probes = 0
    for i in order:
        line = int(home_lines[i])
        for _ in range(nlines):
            probes += 1
            if taken[line] < SLOTS:
                taken[line] += 1
                break
            line = 0 if line + 1 == nlines else line + 1
        else:
            raise AssertionError("the table is full")
    return probes, taken


def tables_of(case):
    return list(case.tables) + list(getattr(case, "floor", [])) + ([case.again] if hasattr(case, "again") else [])


CASES = {c.name: c for c in tc.all_cases()}


def test_every_case_is_there():
    assert set(CASES) == {"exact8", "spill", "chain", "wrap", "long_wrap", "wrap_250", "wrap_k11", "repeats", "wrap/2", "wrap/3", "long_wrap/2",
                          "long_wrap/3", "floor_full", "floor_over", "retired"}
    for c in CASES.values():
        print(c.describe())


@pytest.mark.parametrize("name", sorted(CASES))
def test_expected_probes_is_what_a_sequential_table_counts_in_any_order(name):
    case = CASES[name]
    rng = np.random.default_rng(5)
    for t in tables_of(case):
        want = tc.expected_probes(t.lines, t.nlines)
        assert want == t.probes == t.keys.size + int(t.over.sum())
        seen = set()
        for _ in range(ORDERS):
            probes, taken = simulate(t.lines, t.nlines, rng.permutation(t.keys.size))
            seen.add(probes)
            assert taken == t.taken.tolist()
        print(f"{name} part {t.part}/{t.nparts} lines {t.nlines}: expected {want}, simulated {sorted(seen)}")
        assert seen == {want}


def test_the_numbers_the_shapes_promise():
    got = {n: CASES[n].tables[0].probes for n in tc.WHOLE}
    assert got == {"exact8": 64, "spill": 68, "chain": 72, "wrap": 72, "long_wrap": 96, "wrap_250": 1008, "wrap_k11": 72}
    assert [t.probes for t in CASES["wrap/2"].tables] == [40, 40] and [t.probes for t in CASES["long_wrap/3"].tables] == [12, 72, 12]
    full = CASES["floor_full"].floor[0]
    assert full.keys.size == 128 and full.nlines == 16 and full.probes == tc.expected_probes(full.lines, 16) > 128


def test_expected_probes_on_hand_made_tables():
    assert tc.expected_probes([], 16) == 0
    assert tc.expected_probes([3] * 8, 16) == 8                           # exactly full
    assert tc.expected_probes([3] * 9, 16) == 10                          # one leaver
    assert tc.expected_probes([15] * 9, 16) == 10                         # ... across the wrap
    assert tc.expected_probes([15] * 9 + [0] * 8, 16) == 17 + 2           # the leaver of line 15 pushes one out of line 0
    assert tc.expected_probes([0] * 24, 16) == 24 + 16 + 8                # 16 leave line 0, 8 of them leave line 1
    assert tc.expected_probes(list(range(16)) * 8, 16) == 128             # a full table in which nothing moves
    assert tc.expected_probes([5] * 128, 16) == 128 + sum(range(8, 128, 8))      # ... and one filled from a single line
    with pytest.raises(AssertionError):
        tc.expected_probes([0] * 129, 16)


def test_the_sizing_rule_restated():
    assert [tc.table_lines(n, 17) for n in (0, 1, 64, 65, 89, 168, 169, 192, 1000)] == [16, 16, 16, 17, 23, 42, 43, 48, 250]
    assert tc.table_lines(10 ** 6, 3) == 16 and tc.table_lines(10 ** 6, 5) == 256                 # 4^k keys at most
    assert [tc.part_table_lines(64, 17, n) for n in (1, 2, 3)] == [16, 16, 16]
    assert [tc.part_table_lines(168, 17, 2), tc.part_table_lines(169, 17, 2), tc.part_table_lines(100_000, 17, 2)] == [42, 43, 15641]
    for n in (1, 64, 1000, 12345):
        assert tc.part_table_lines(n, 17, 1) == tc.table_lines(n, 17)


@pytest.mark.parametrize("name,nparts", tc.PART_NAMES)
def test_partition_cases_against_the_partition_arithmetic(name, nparts):
    """every key sits in the partition and the line np_part_of / np_line_of give it, the partitions' models are the whole model
    restricted, and every read is one position of one partition"""
    case = tc.part_case(name, nparts)
    m = kmer_model.model(case.reads, case.k, 0)
    assert m["positions"] == 64 and m["distinct"] == 64 and m["merged"] == 0
    parts = restrict(m, merged_keys(case.reads, case.k, 0), nparts)
    owner = np_part_of(m["kmers"], nparts)
    assert sum(t.keys.size for t in case.tables) == 64
    for p, t in enumerate(case.tables):
        assert np.array_equal(t.keys, parts[p]["kmers"]) and np.array_equal(t.keys, m["kmers"][owner == p])
        assert parts[p]["inserts"] == t.keys.size and (parts[p]["counts"] == 1).all()
        assert np.array_equal(np.bincount(np_line_of(t.keys, nparts, 16), minlength=16), t.home)
        for keys, lines in case.absent[p].values():
            assert (np_part_of(keys, nparts) == p).all() and np.array_equal(np_line_of(keys, nparts, 16), lines)


@pytest.mark.parametrize("name", tc.FLOOR_NAMES)
def test_floor_cases(name):
    case = tc.floor_case(name)
    n0 = case.tables[0].keys.size
    assert (n0, case.tables[1].keys.size) == ({"floor_full": 128, "floor_over": 129}[name], 40)
    assert (np_part_of(case.tables[0].keys, 2) == 0).all() and (np_part_of(case.tables[1].keys, 2) == 1).all()
    if name == "floor_full":
        assert (case.floor[0].taken == SLOTS).all() and not (case.floor[1].taken == SLOTS).all()
    else:
        assert np.isin(tc.floor_case("floor_full").tables[0].keys, case.tables[0].keys).all()          # the same keys and one more
        assert np.array_equal(tc.floor_case("floor_full").tables[1].keys, case.tables[1].keys)
        assert case.again.nlines == tc.table_lines(169, 17) == 43 and case.again.keys.size == 129


def test_retired_case():
    case = tc.retired_case()
    line = np_line_of([case.x], 1, case.nlines)[0]
    assert line == case.nlines - 1 and case.tables[0].home[line] == 12 and case.counts[case.keys == case.x][0] == 4
