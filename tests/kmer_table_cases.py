"""helpers of the k-mer table tests (not a test): tiny inputs that put a chosen number of keys into chosen lines of the
open-addressing table of genarchbench_amd/csrc/kmer.hip, so that the probe walks of kmer_insert and kmer_find take the paths that big
random inputs reach only by chance: a line that is exactly full, a line that spills, a spill that chains, the wrap from the last line
to line 0, a table with no empty slot, a slot that kmer_solid_retire overwrote.

How.  A read of k + 1 bases kept with min_len = 0 has exactly one counted position (the last k-mer of a read is never visited), so
N such reads are N positions and the table has table_lines(N, k) lines of SLOTS slots.  The hash is restated in
tests/kmer_parts_util.py; random k-mers are drawn from a seeded pool and taken by their home line until every line has the number of
keys the case asks for.

`probes` (table lines visited by the inserts) for keys that are each inserted ONCE does not depend on the order of the inserts: a
line that receives a arrivals -- its own keys and the leavers of the line before it -- ends with min(a, SLOTS) slots taken and sends
exactly max(0, a - SLOTS) keys on, whichever they are.  With home[l] the keys whose home is line l and over[-1] the leavers of the
last line (the wrap),

    over[l] = max(0, home[l] + over[l - 1] - SLOTS)        (the least fixed point: iterate from 0)
    probes  = inserts + sum over[l]

(expected_probes; tests/test_kmer_table_cases.py checks it against a sequential table in random insert orders).  It holds for
concurrent inserts too, because a lane leaves a line only after it saw all SLOTS slots taken by other keys.

Every case asserts its own preconditions when it is built -- the home-line histogram, the leavers of every line, the line count, the
number of distinct keys and positions, "every key once" where probes is exact -- so a change of the hash, the slot count or the
sizing rule fails here, on the CPU, and not silently on the GPU.  `python -m tests.kmer_table_cases` prints every histogram."""
import functools
import zlib

import numpy as np

from tests import kmer_model, solid_model
from tests.kmer_parts_util import SLOTS, np_line_of, np_part_of

_U = np.uint64
FLOOR_LINES = 16        # the smallest table, and the first table of a partition under GAB_KMER_PART_FLOOR=1
POOL = 60_000           # random k-mers a case searches


# ---- the sizing rule of kmer.hip, restated (table_lines, part_table_lines) -----------------------------------------------------------
def table_lines(positions, k):
    keys = min(max(positions, 1), 4 ** k)
    return max(FLOOR_LINES, (2 * keys + SLOTS - 1) // SLOTS)


def part_table_lines(positions, k, nparts):
    keys = min(max(positions, 1), 4 ** k)
    share = (keys + nparts - 1) // nparts
    room = share + share // 4 + 64
    return min(table_lines(positions, k), max(FLOOR_LINES, (2 * room + SLOTS - 1) // SLOTS))


# ---- the walk arithmetic ----------------------------------------------------------------------------------------------------------------
def leavers(home_lines, nlines):
    """the home line of every key -> (home, over): keys per home line, and the keys every line sends on to the next"""
    home_lines = np.asarray(home_lines, np.int64)
    home = np.bincount(home_lines, minlength=nlines).astype(np.int64) if home_lines.size else np.zeros(nlines, np.int64)
    assert home.size == nlines and int(home.sum()) <= SLOTS * nlines, "more keys than slots"
    over = np.zeros(nlines, np.int64)
    carry, changed = 0, True
    while changed:              # monotone from 0; a sweep starts with the wrap of the sweep before it
        changed = False
        for line in range(nlines):
            carry = max(0, int(home[line]) + carry - SLOTS)
            if carry != over[line]:
                over[line], changed = carry, True
    return home, over


def expected_probes(home_lines, nlines):
    """table lines visited by the inserts of keys with these home lines, each inserted exactly once, in any order"""
    home, over = leavers(home_lines, nlines)
    return int(home.sum() + over.sum())


# ---- k-mers --------------------------------------------------------------------------------------------------------------------------
def np_revcomp(x, k):
    x = np.asarray(x, _U).copy()
    r = np.zeros_like(x)
    for _ in range(k):
        r = (r << _U(2)) | (~x & _U(3))
        x >>= _U(2)
    return r


def bases_of(value, k):
    return bytes(b"ACGT"[(int(value) >> (2 * (k - 1 - j))) & 3] for j in range(k))


@functools.lru_cache(maxsize=None)
def pool(k, seed):
    """POOL distinct canonical k-mers in random order"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4 ** k, POOL, dtype=np.uint64)
    canon = np.unique(np.minimum(x, np_revcomp(x, k)))
    return canon[rng.permutation(canon.size)]


def read_of(key, k, flip):
    """a read of k + 1 bases whose one counted position has the canonical k-mer `key`: the key itself or, flipped, its reverse
    complement (both strands reach the table), and one more base that no counted k-mer ends at"""
    return bases_of(int(np_revcomp([key], k)[0]) if flip else key, k) + b"A"


class Table:
    """what one table holds after the inserts of `keys` (canonical, distinct): the keys of `part` of `nparts` in `nlines` lines"""

    def __init__(self, keys, nlines, nparts=1, part=0):
        keys = np.asarray(keys, _U)
        self.nlines, self.nparts, self.part = nlines, nparts, part
        self.keys = np.sort(keys[np_part_of(keys, nparts) == part]) if keys.size else keys
        self.lines = np_line_of(self.keys, nparts, nlines) if self.keys.size else np.zeros(0, np.int64)
        self.home, self.over = leavers(self.lines, nlines)
        self.taken = np.minimum(SLOTS, self.home + np.roll(self.over, 1))          # slots taken per line, in any insert order
        assert int(self.taken.sum()) == self.keys.size
        self.probes = int(self.keys.size + self.over.sum())                         # for keys inserted once each

    def absent(self, candidates, each=2):
        """keys the table does not hold, of its own partition, by what a look-up of them has to do: {"full": home line full (walk
        on), "last": home is the last line, "empty": home line has no key at all (stop at once)} -> (keys, their home lines)"""
        c = np.asarray(candidates, _U)
        c = c[(np_part_of(c, self.nparts) == self.part) & ~np.isin(c, self.keys)]
        line = np_line_of(c, self.nparts, self.nlines)
        out = {"full": c[self.taken[line] == SLOTS][:each], "last": c[line == self.nlines - 1][:each], "empty": c[self.taken[line] == 0][:each]}
        return {w: (v, np_line_of(v, self.nparts, self.nlines)) for w, v in out.items()}


def _take(rng_keys, lines, nlines, total, fixed, caps, cap, pre=None):
    """indices into the pool: exactly fixed[line] keys of every fixed line, then pool order, no line above caps.get(line, cap); `pre`:
    keys per line that are in the table already and count towards both"""
    have = np.zeros(nlines, np.int64) if pre is None else np.asarray(pre, np.int64).copy()
    fixed = {line % nlines: n for line, n in fixed.items()}
    caps = {line % nlines: n for line, n in caps.items()}
    chosen = []
    for line, n in fixed.items():
        need = n - int(have[line])
        at = np.flatnonzero(lines == line)[:max(need, 0)]
        assert need >= 0 and at.size == need, f"line {line}: {need} keys wanted, the pool has {at.size}"
        chosen.extend(at.tolist())
        have[line] = n
    for i in range(rng_keys.size):
        if len(chosen) == total:
            break
        line = int(lines[i])
        if line in fixed or have[line] >= caps.get(line, cap):
            continue
        chosen.append(i)
        have[line] += 1
    assert len(chosen) == total, f"{len(chosen)} of {total} keys found"
    return np.array(chosen, np.int64)


# the shapes: exact home counts (negative lines count from the end), upper bounds, and the leavers they promise.  Every other line
# holds at most SLOTS - 1 keys and line nlines // 2 + 2 none, so nothing else spills and there is an empty line to stop at.
SHAPES = {
    "exact8": dict(fixed={-1: 8}, caps={}, over={}),                                         # full, and nothing leaves
    "spill": dict(fixed={6: 12}, caps={7: 4}, over={6: 4}),
    "chain": dict(fixed={6: 12, 7: 8}, caps={8: 4}, over={6: 4, 7: 4}),                      # four keys visit three lines
    "wrap": dict(fixed={-1: 12, 0: 8}, caps={1: 4}, over={-1: 4, 0: 4}),                     # ... the last line, line 0, line 1
    "long_wrap": dict(fixed={-3: 16, -2: 8, -1: 8, 0: 8, 1: 0}, caps={}, over={-3: 8, -2: 8, -1: 8, 0: 8}),      # eight keys visit five
}


def _shaped(keys, lines, nlines, total, shape, pre=None):
    s = SHAPES[shape]
    return _take(keys, lines, nlines, total, {**s["fixed"], nlines // 2 + 2: 0}, s["caps"], SLOTS - 1, pre)


def _check_shape(t, shape):
    s = SHAPES[shape]
    n = t.nlines
    for line, want in s["fixed"].items():
        assert t.home[line % n] == want, (shape, line, t.home.tolist())
    for line, most in s["caps"].items():
        assert t.home[line % n] <= most, (shape, line, t.home.tolist())
    want = np.zeros(n, np.int64)
    for line, v in s["over"].items():
        want[line % n] = v
    assert t.over.tolist() == want.tolist(), (shape, t.home.tolist(), t.over.tolist())
    assert t.taken[n // 2 + 2] == 0


class Case:
    """name, k, nparts, reads (min_len = 0), positions, keys (distinct canonical, ascending) and counts, once (every key at one
    position: probes is exact), tables (one per partition: the first table of a call over these reads), absent (per table: the
    dict of Table.absent)"""

    def __init__(self, name, k, keys, copies, seed, nparts=1, extra_reads=()):
        rng = np.random.default_rng(seed)
        self.name, self.k, self.nparts = name, k, nparts
        reads = [read_of(key, k, bool(rng.integers(0, 2))) for key, c in zip(keys, copies) for _ in range(int(c))]
        reads = [reads[i] for i in rng.permutation(len(reads))] + list(extra_reads)
        self.reads = reads
        m = kmer_model.model(reads, k, 0)
        self.model = m
        self.positions, self.keys, self.counts = m["positions"], m["kmers"], m["counts"]
        self.once = bool((m["counts"] == 1).all())
        self.nlines = part_table_lines(self.positions, k, nparts)
        self.tables = [Table(self.keys, self.nlines, nparts, p) for p in range(nparts)]
        if not extra_reads:            # single-position reads only: the keys come back as they went in, nothing merges
            assert self.positions == int(np.sum(copies)) == len(reads) and m["reads_kept"] == len(reads) and m["merged"] == 0
            assert np.array_equal(self.keys, np.sort(np.asarray(keys, _U))) and np.unique(keys).size == len(keys)
            assert np.array_equal(self.counts, np.asarray(copies, np.int64)[np.argsort(np.asarray(keys, _U))])
        self.absent = [t.absent(pool(k, seed)) for t in self.tables]

    def absent_keys(self, p=0):
        return np.concatenate([v[0] for v in self.absent[p].values()])

    def require_absent(self, p, kinds):
        for kind in kinds:
            keys, lines = self.absent[p][kind]
            t = self.tables[p]
            assert keys.size >= 1 and not np.isin(keys, self.keys).any(), (self.name, p, kind)
            assert {"full": (t.taken[lines] == SLOTS).all(), "last": (lines == t.nlines - 1).all(), "empty": (t.taken[lines] == 0).all()}[kind]

    def describe(self):
        return "\n".join(f"{self.name:<14} k={self.k} part {t.part}/{t.nparts} positions={self.positions} lines={t.nlines} keys={t.keys.size} "
                         f"probes={t.probes if self.once else '>=' + str(int(self.counts[np_part_of(self.keys, t.nparts) == t.part].sum()))} "
                         f"home={t.home.tolist() if t.nlines <= 64 else 'max %d, last %d, line 0 %d' % (t.home.max(), t.home[-1], t.home[0])}"
                         for t in self.tables)


def _seed(name):
    return zlib.crc32(name.encode())


# ---- the unpartitioned cases ------------------------------------------------------------------------------------------------------------
WHOLE = {"exact8": ("exact8", 17, 64, 64), "spill": ("spill", 17, 64, 68), "chain": ("chain", 17, 64, 72), "wrap": ("wrap", 17, 64, 72),
         "long_wrap": ("long_wrap", 17, 64, 96), "wrap_250": ("wrap", 17, 1000, 1008), "wrap_k11": ("wrap", 11, 64, 72)}      # shape, k, positions, probes


@functools.lru_cache(maxsize=None)
def whole_case(name):
    """one of WHOLE, or "repeats": the wrap shape with every key at three positions, some at one and some at five"""
    seed = _seed(name)
    if name == "repeats":
        return _repeats(seed)
    shape, k, n, probes = WHOLE[name]
    nlines = table_lines(n, k)
    keys = pool(k, seed)
    lines = np_line_of(keys, 1, nlines)
    at = _shaped(keys, lines, nlines, n, shape)
    c = Case(name, k, keys[at], np.ones(n, np.int64), seed)
    t = c.tables[0]
    assert c.once and c.nlines == nlines == {64: 16, 1000: 250}[n] and c.positions == n == c.keys.size
    _check_shape(t, shape)
    assert t.probes == probes == expected_probes(t.lines, nlines)
    c.require_absent(0, ("full", "last", "empty"))
    return c


def _repeats(seed):
    k, distinct = 17, 64
    copies = np.full(distinct, 3, np.int64)
    copies[[0, 1, 30, 31]] = 5          # (0 .. 11 are the keys of the last line, 12 .. 19 those of line 0: see _take)
    copies[[2, 3, 32, 33]] = 1
    nlines = table_lines(int(copies.sum()), k)
    keys = pool(k, seed)
    at = _shaped(keys, np_line_of(keys, 1, nlines), nlines, distinct, "wrap")
    c = Case("repeats", k, keys[at], copies, seed)
    assert not c.once and c.positions == 192 and c.nlines == nlines == 48 and c.keys.size == distinct
    assert sorted(np.unique(c.counts).tolist()) == [1, 3, 5] and (c.counts == 5).sum() == 4 and (c.counts == 1).sum() == 4
    _check_shape(c.tables[0], "wrap")
    five = c.keys[c.counts == 5]
    assert (np_line_of(five, 1, nlines) == nlines - 1).sum() == 2         # two of the five-fold keys live where the wrap starts
    c.require_absent(0, ("full", "last", "empty"))
    return c


# ---- partitions -----------------------------------------------------------------------------------------------------------------------
# name -> per nparts: (keys per partition, the partitions that get the shape); 64 positions in all, so every first table has 16 lines
PARTS = {"wrap": {2: ((32, 32), (0, 1)), 3: ((22, 21, 21), (0, 1, 2))},
         "long_wrap": {2: ((40, 24), (0,)), 3: ((12, 40, 12), (1,))}}


def _part_keys(k, seed, nparts, nlines, sizes, shapes):
    """sizes[p] pool keys of every partition p, in the shape shapes.get(p) (None: as they come, no line overfull, one line empty)"""
    keys = pool(k, seed)
    owner = np_part_of(keys, nparts)
    out = []
    for p in range(nparts):
        mine = keys[owner == p]
        lines = np_line_of(mine, nparts, nlines)
        if shapes.get(p) == "any":
            at = np.arange(sizes[p])
        elif shapes.get(p):
            at = _shaped(mine, lines, nlines, sizes[p], shapes[p])
        else:
            at = _take(mine, lines, nlines, sizes[p], {nlines // 2 + 2: 0}, {}, SLOTS - 1)
        out.append(mine[at])
    return out


@functools.lru_cache(maxsize=None)
def part_case(name, nparts):
    seed = _seed(f"{name}/{nparts}")
    sizes, shaped = PARTS[name][nparts]
    k = 17
    assert sum(sizes) == 64 and part_table_lines(64, k, nparts) == FLOOR_LINES
    per = _part_keys(k, seed, nparts, FLOOR_LINES, sizes, {p: name for p in shaped})
    c = Case(f"{name}/{nparts}", k, np.concatenate(per), np.ones(64, np.int64), seed, nparts)
    assert c.once and c.positions == 64 and c.nlines == FLOOR_LINES
    for p, t in enumerate(c.tables):
        assert np.array_equal(t.keys, np.sort(per[p])) and t.keys.size == sizes[p]
        assert np.array_equal(t.lines, np_line_of(t.keys, nparts, FLOOR_LINES)) and (np_part_of(t.keys, nparts) == p).all()
        if p in shaped:
            _check_shape(t, name)
            c.require_absent(p, ("full", "last", "empty"))
        else:
            assert t.over.sum() == 0 and t.probes == sizes[p]
            c.require_absent(p, ("last", "empty"))
    return c


class FloorCase(Case):
    """partition 0 of 2 fills the 16-line floor table exactly (floor_full: 128 keys) or by one key too many (floor_over: 129);
    partition 1 holds some 40 keys.  tables: the first table of a plain call; floor: the tables under GAB_KMER_PART_FLOOR=1;
    again: the table of the repeated call (table_lines of the whole input), for the partition that needs it"""


@functools.lru_cache(maxsize=None)
def floor_case(name):
    k, nparts = 17, 2
    n0 = {"floor_full": FLOOR_LINES * SLOTS, "floor_over": FLOOR_LINES * SLOTS + 1}[name]
    seed = _seed("floor")                       # one pool for both: floor_over is floor_full and one more key of partition 0
    per = _part_keys(k, seed, nparts, FLOOR_LINES, (n0, 40), {0: "any", 1: "any"})
    c = FloorCase(name, k, np.concatenate(per), np.ones(n0 + 40, np.int64), seed, nparts)
    assert c.once and c.positions == n0 + 40 and [t.keys.size for t in c.tables] == [n0, 40]
    assert c.nlines == part_table_lines(c.positions, k, nparts) == {128: 42, 129: 43}[n0]
    c.floor = [Table(c.keys, FLOOR_LINES, nparts, 1)]
    c.again = Table(c.keys, table_lines(c.positions, k), nparts, 0)
    assert c.again.nlines == {128: 42, 129: 43}[n0]
    if name == "floor_full":
        full = Table(c.keys, FLOOR_LINES, nparts, 0)
        c.floor.insert(0, full)
        assert (full.taken == SLOTS).all() and full.keys.size == FLOOR_LINES * SLOTS            # no empty slot at all
        assert full.probes > n0 and (full.over == 0).any()                                      # (the least fixed point: some line sends nothing on)
        c.floor_absent = full.absent(pool(k, seed), each=4)
        assert c.floor_absent["full"][0].size == 4 and c.floor_absent["last"][0].size == 4 and c.floor_absent["empty"][0].size == 0
    assert (c.floor[-1].taken < SLOTS).any()
    return c


# ---- the solid index: a key that leaves the capacity table ---------------------------------------------------------------------------
SOLID = dict(min_freq=1, select_rate=0.999, tandem_freq=1)      # rank n - 1 of every read here, as select_rate = 1 would give if the library took it


@functools.lru_cache(maxsize=None)
def retired_case():
    """the wrap shape in a table of 23 lines, and a key X with capacity 2 and count 4: twice in one longer read (both positions
    fall to the tandem rule) and once in each of two single-position reads.  At a threshold of 2 or 3 X stays (2 <= thr) with an
    empty list (4 > thr): kmer_solid_retire overwrites its slot, in or behind the last line, which is the home of twelve keys"""
    k, seed = 17, _seed("retired")
    positions = 64 + (k + 6) + 2
    nlines = table_lines(positions, k)
    keys = pool(k, seed)
    lines = np_line_of(keys, 1, nlines)
    rng = np.random.default_rng(seed)
    for x in keys[lines == nlines - 1]:
        long_read = bases_of(x, k) + bases_of(int(rng.integers(0, 4 ** 5)), 5) + bases_of(x, k) + b"A"
        inner = kmer_model.canonical_kmers(long_read, k)
        assert inner.size == k + 6 and inner[0] == inner[-1] == x
        junk = inner[1:-1]
        pre = np.bincount(np_line_of(np.concatenate([junk, [x]]), 1, nlines), minlength=nlines)
        if np.unique(inner).size == k + 5 and pre[-1] <= 12 and pre[0] <= 8 and pre[1] <= 4 and pre[nlines // 2 + 2] == 0 and pre.max() < SLOTS:
            break
    else:
        raise AssertionError("no X found")
    rest = keys[~np.isin(keys, inner)]
    at = _shaped(rest, np_line_of(rest, 1, nlines), nlines, 64, "wrap", pre)
    extra = [long_read, read_of(x, k, False), read_of(x, k, True)]
    c = Case("retired", k, rest[at], np.ones(64, np.int64), seed, extra_reads=extra)
    c.x = _U(x)
    assert c.positions == positions and c.nlines == nlines == 23 and c.keys.size == 64 + k + 5 and c.counts[c.keys == c.x] == [4]
    assert all(solid_model.rank_of(SOLID["select_rate"], len(r) - k) == len(r) - k - 1 == solid_model.rank_of(1.0, len(r) - k) for r in c.reads)
    _check_shape(c.tables[0], "wrap")           # the count table and the capacity table: every key of the input is selected
    c.require_absent(0, ("full", "last", "empty"))
    for rate in (2, 3):
        m = solid_model.build_index(c.reads, k, SOLID["min_freq"], SOLID["select_rate"], SOLID["tandem_freq"], rate, 0)
        assert m["candidates"] == c.keys.size and m["repetitive_frequency"] == rate and m["empty"].tolist() == [x] and m["repetitive"].size == 0
        selected = np.concatenate([m["kmers"], m["empty"]])
        assert np.array_equal(np.sort(selected), c.keys)
        assert np.bincount(np_line_of(selected, 1, nlines), minlength=nlines)[np_line_of([x], 1, nlines)[0]] >= 9
    return c


WHOLE_NAMES = tuple(WHOLE) + ("repeats",)
PART_NAMES = tuple((name, nparts) for name in PARTS for nparts in PARTS[name])
FLOOR_NAMES = ("floor_full", "floor_over")


def all_cases():
    return [whole_case(n) for n in WHOLE_NAMES] + [part_case(*n) for n in PART_NAMES] + [floor_case(n) for n in FLOOR_NAMES] + [retired_case()]


if __name__ == "__main__":
    for case in all_cases():
        print(case.describe())
        for t in getattr(case, "floor", []):
            print(f"{'  under the floor':<14} part {t.part}/{t.nparts} lines={t.nlines} keys={t.keys.size} probes={t.probes} home={t.home.tolist()}")
