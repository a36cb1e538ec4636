"""chain / fast-chain: the batches of tests/test_chain_through_gpu.py -- gab_chain_run_device_through (and gab_chain_run) on every
route the results take to the caller's host arrays, in every kernel form, at the edges the forms have, and in layouts other than
ascending and gapless.  Builders only; tests/test_chain_through_cases.py proves from tests.util's models and the oracle that each
case reaches the route and the forms it is named for.

A Case names its calls (a key of CALLS: built once, kept), the pins it runs under, whether the host arrays are page-locked (None: not
asked for, gab_chain_run_device), how the calls are laid out, and what to expect: `route` (gab_chain_last_through) and, where the
case is about them, the forms (gab_chain_last_split)."""
from dataclasses import dataclass, field

import numpy as np

from tools import gabgen
from tests import chain_form_cases as cases
from tests.util import CHAIN_DISPATCH, CHAIN_SEVEN_HELPERS, GOLDEN, chain_extent

TAB_ALL = CHAIN_DISPATCH["table-form-for-all"]
LAYOUTS = ("descending", "gaps", "empties", "off_line")
GAPS = (1, 15, 17)                    # elements between calls: calls start off the 16-element and the 64-element lines
NO_ROOM_MB = 2                        # GAB_CHAIN_TAB_MB of the no-room case: 2 048 groups of 16 rows
PATCHED = (31, 200, 0, 50, 20000, 3306, 1881, 49)     # gabgen.chain arguments; the call's length, the anchor, how far back its predecessor


def calls_of(batch):
    o, n = batch.call_off, batch.hdr["n"]
    return [(float(h["avg_qspan"]), int(h["max_dist_x"]), int(h["max_dist_y"]), int(h["bw"]), int(h["n_segs"]), batch.x[int(a):int(a) + int(k)], batch.y[int(a):int(a) + int(k)])
            for h, a, k in zip(batch.hdr, o, n)]


def fillers(rng, anchors, lo=150, hi=190):
    """plain calls of lo .. hi anchors, `anchors` anchors at least in all"""
    out, have = [], 0
    while have < anchors:
        n = int(rng.integers(lo, hi + 1))
        out.append(cases.call(*cases.diagonal(rng, n=n)))
        have += n
    return out


def edge_calls_throughput(anchors):
    """one call of each length of EDGE_LENGTHS up to 193 (windows reaching back across the 64-anchor blocks), spread among plain calls
    of 150 .. 190 anchors that bring the batch to `anchors` anchors: 193 is its longest call"""
    rng = np.random.default_rng(71)
    edge = [c for c in cases.block_edge_calls(16) if len(c[5]) <= 193]
    fill = fillers(rng, anchors - sum(len(c[5]) for c in edge))
    step = len(fill) // len(edge)
    out = []
    for k, c in enumerate(edge):
        out += fill[k * step:(k + 1) * step] + [c]
    return out + fill[len(edge) * step:]


def side_by_side_calls():
    """five 3 000-anchor calls among 400 of 100 .. 200: with GAB_CHAIN_TAB_MIN=2000 and GAB_CHAIN_FAST_CALLS=0 the long ones are the table
    form's and the rest the throughput form's, on two streams, both writing through"""
    rng = np.random.default_rng(72)
    short = [cases.call(*cases.diagonal(rng, n=int(rng.integers(100, 201)))) for _ in range(400)]
    out = []
    for k in range(5):
        out += short[80 * k:80 * k + 37] + [cases.call(*cases.diagonal(rng, n=3000))] + short[80 * k + 37:80 * (k + 1)]
    return out


def small_calls():
    """the 13-call batch of test_legacy_only_launch_and_the_record_itself: 12 calls of 100 .. 3 000 anchors and an empty one"""
    return calls_of(gabgen.chain(39, 12, 1, 100, 3000)) + [cases.call([], [], [])]


def one_long_calls():
    """one 1 500-anchor call among 30 of 100: the batch waits for it, no call reaches the table form's 2 048, the long one the latency form's 512"""
    rng = np.random.default_rng(73)
    short = [cases.call(*cases.diagonal(rng, n=100)) for _ in range(30)]
    return short[:11] + [cases.call(*cases.diagonal(rng, n=1500))] + short[11:]


def no_room_calls():
    """40 calls of 50 .. 2 000 anchors, the longest one last.  A block of the table form needs eight 16-row groups at least (four for a
    call's first block): these need more than the 2 048 groups of GAB_CHAIN_TAB_MB=2 whatever their windows, and the longest call --
    first in the sorted list -- fits whatever its windows (ctab_place)"""
    c = calls_of(gabgen.chain(35, 40, 0, 50, 2000))
    k = int(np.argmax([len(v[5]) for v in c]))
    return c[:k] + c[k + 1:] + [c[k]]


def least_groups(n_per_call):
    """16-row groups the table form needs for these calls at least: every 64-anchor block has the 128 near rows (a first block: 64)"""
    return sum(8 * ((int(n) + 63) // 64) - 4 for n in n_per_call if n > 0)


def most_groups(call):
    """... and at most: per block the rows from the window start of its first anchor (the first x within max_dist_x) to its last anchor,
    rounded up to groups, one more for a window that begins inside a group"""
    x, dist = call[5].astype(np.uint64), np.uint64(call[1])
    st = np.searchsorted(x, x[::64] - np.minimum(x[::64], dist), side="left")
    return int(sum((min(len(x), 64 * b + 64) - int(s) + 15) // 16 + 1 for b, s in enumerate(st)))


def patched_calls():
    """21 plain calls of 160 anchors, then the call of gabgen.chain(31, 200, 0, 50, 20000) in which max_skip changes a result: anchor 1 881
    of 3 306 takes a predecessor 49 back, which the table form's resolver finds by the reference's own scan, PATCHES, and restarts
    the fold from that block -- rewriting scores it has already stored and, two blocks behind, their parents"""
    seed, ncalls, gmode, nmin, nmax, length = PATCHED[:6]
    ids = np.nonzero(gabgen.chain_sizes(seed, ncalls, gmode, nmin, nmax) == length)[0]
    assert len(ids) == 1
    rng = np.random.default_rng(74)
    return [cases.call(*cases.diagonal(rng, n=160)) for _ in range(21)] + calls_of(gabgen.chain_ids(seed, ids, gmode, nmin, nmax))


def host_entry_calls():
    """gab_chain_run's copy-engine path (chain_run_overlapped) sends the longest calls ahead (group A: 64 calls at least, then until they
    hold a sixteenth of the anchors), splits the others by the middle of the arrays and copies the results back in two pieces, cut
    where the first second-half call begins.  70 calls of 300 .. 369 anchors (64 of them group A) and 60 of 90 .. 149 that are not"""
    rng = np.random.default_rng(75)
    long_ = [cases.call(*cases.diagonal(rng, n=300 + k)) for k in range(70)]
    short = [cases.call(*cases.diagonal(rng, n=90 + k)) for k in range(60)]
    out = []
    for k in range(10):
        out += long_[7 * k:7 * k + 7] + short[6 * k:6 * k + 6]
    return out


CALLS = {
    "edges_tp": lambda: edge_calls_throughput(int(1.15 * CHAIN_SEVEN_HELPERS * 193)),          # clear of the seven-helper rule
    "edges_tp_default": lambda: edge_calls_throughput(int(1.15 * 1140 * 193)),                 # ... and nobody waits for a 193-anchor call
    "edges_tab": lambda: cases.block_edge_calls(16),
    "side_by_side": side_by_side_calls,
    "small": small_calls,
    "three_500": lambda: [cases.call(*cases.diagonal(np.random.default_rng(76 + k), n=500)) for k in range(3)],
    "one_long": one_long_calls,
    "q_span_0_and_255": lambda: cases.limit_cases()["q_span_0_and_255"][0],
    "bw_neg1": lambda: cases.limit_cases()["bw_neg1"][0],
    "no_room": no_room_calls,
    "dense": lambda: calls_of(gabgen.read_chain_text(f"{GOLDEN}/chain_dense.in.txt")),
    "patched": patched_calls,
    "host_entry": host_entry_calls,
    "none": lambda: [],
    "only_empty": lambda: [cases.call([], [], [])] * 3,
}
_batches = {}


def batch_of(key):
    """the gapless batch of CALLS[key], built once"""
    if key not in _batches:
        _batches[key] = gabgen.chain_from_calls(CALLS[key]())
    return _batches[key]


@dataclass
class Case:
    name: str
    calls: str                          # key of CALLS
    env: dict
    pinned: object                      # True: page-locked host arrays, False: pageable, None: gab_chain_run_device
    route: int                          # what the case is named for: gab_chain_last_through
    modes: tuple = (0, 1)
    layout: str = None                  # None: back to back in the caller's order; else one of LAYOUTS / "host_entry" / "scattered_empty"
    forms: dict = None                  # mode -> gab_chain_last_split's forms, where the case names them
    all_form: int = None                # ... or the one form of every non-empty call
    has_form: tuple = ()                # ... or forms at least one call has
    default_rule: bool = False          # no pin decides the split: its comparisons are kept 10 % from flipping
    fresh: bool = False                 # GAB_CHAIN_TAB_MB: fixed at a handle's first table-form call
    extra: dict = field(default_factory=dict)


def _limit(name):
    want = cases.limit_cases()[name][1]
    return Case(f"handed_back_not_eligible_{name}", name, TAB_ALL, True, 4, forms=want)


def through_cases():
    tp = CHAIN_DISPATCH["throughput-form-for-all"]
    side = {"GAB_CHAIN_TAB_MIN": "2000", "GAB_CHAIN_FAST_CALLS": "0"}
    out = [
        # block edges in the throughput form, written
        Case("edges_throughput_pinned_rule", "edges_tp", tp, True, 1, all_form=1),
        Case("edges_throughput_default_rule", "edges_tp_default", {}, True, 1, all_form=1, default_rule=True),
        # block edges in the table form, written
        Case("edges_table", "edges_tab", TAB_ALL, True, 1, all_form=3),
        # table and throughput forms side by side, written
        Case("side_by_side", "side_by_side", side, True, 1, has_form=(1, 3)),
        # the legacy-only launch: three helpers write through, five do not, the walk kernel does not
        Case("legacy_3_helpers", "small", {"GAB_CHAIN_HELPERS": "3"}, True, 1, all_form=6),
        Case("legacy_5_helpers", "small", {"GAB_CHAIN_HELPERS": "5"}, True, 3, all_form=6),
        Case("legacy_walk", "small", {"GAB_CHAIN_KERNEL": "walk"}, True, 3, modes=(0,), all_form=6),
        # seven helpers: a few calls, nothing pinned
        Case("seven_helpers", "three_500", {}, True, 3, all_form=1, default_rule=True),
        # the latency form takes part
        Case("latency_for_all", "edges_tab", CHAIN_DISPATCH["latency-form-for-all"], True, 3, all_form=2),
        Case("latency_one_long_call", "one_long", {}, True, 3, has_form=(1, 2), default_rule=True),
        # pageable arrays
        Case("pageable_edges_throughput", "edges_tp", tp, False, 2, all_form=1),
        Case("pageable_side_by_side", "side_by_side", side, False, 2, has_form=(1, 3)),
        # handed back by the table form: not eligible (4), no room (5), by the fold (5)
        _limit("q_span_0_and_255"), _limit("bw_neg1"),
        Case("handed_back_no_room", "no_room", dict(TAB_ALL, GAB_CHAIN_TAB_MB=str(NO_ROOM_MB)), True, 4, has_form=(3, 5), fresh=True),
        Case("handed_back_by_the_fold", "dense", TAB_ALL, True, 4, modes=(0,), has_form=(5,)),
        # patched and restarted inside the table form
        Case("patched_in_the_table_form", "patched", TAB_ALL, True, 1, modes=(0,), all_form=3),
        # not asked for; nothing to do
        Case("not_asked_for", "small", {}, None, 0),
        Case("no_calls", "none", {}, True, 1), Case("no_calls_pageable", "none", {}, False, 1), Case("no_calls_not_asked_for", "none", {}, None, 0),
        Case("only_empty_calls", "only_empty", {}, True, 1, layout="scattered_empty"),
        Case("only_empty_calls_pageable", "only_empty", {}, False, 1, layout="scattered_empty"),
    ]
    for lay in LAYOUTS:
        out.append(Case(f"layout_{lay}_edges_throughput", "edges_tp", tp, True, 1, layout=lay, all_form=1))
        out.append(Case(f"layout_{lay}_side_by_side", "side_by_side", side, True, 1, layout=lay, has_form=(1, 3)))
    return out


@dataclass
class Placed:
    """a batch in a layout: `batch` (hdr, call_off, x, y over the arrays' extent), which elements belong to a call (`owned`, indices
    into the arrays) and where each comes from in the gapless batch (`src`), and the calls of the gapless batch in `batch`'s order
    (`call_src`, -1: an empty call the layout added)"""
    batch: object
    owned: np.ndarray
    src: np.ndarray
    call_src: np.ndarray
    off_line: bool = False

    @property
    def total(self):
        return self.batch.nanchors


def place(batch, layout):
    """the calls of a gapless batch laid out differently.  None: as they are.  descending: the first call last in the arrays.  gaps: 1,
    15, 17, 1, ... unowned elements before every call but the first.  empties: three empty calls added whose call_off points into
    the middle of another call, at the arrays' end and at 0.  off_line: as they are -- the HOST window starts one element past a
    64-byte line.  host_entry: descending in chunks of nine calls, with gaps.  scattered_empty: (only empty calls) call_off 0, 5, 3:
    the extent is 5 and holds no call"""
    n = batch.hdr["n"].astype(np.int64)
    nc = len(n)
    hdr = batch.hdr
    call_src = np.arange(nc)
    if layout in (None, "off_line", "empties"):
        off = batch.call_off.astype(np.int64).copy()
    elif layout == "scattered_empty":
        assert not n.any() and nc == 3
        off = np.array([0, 5, 3], np.int64)
    else:
        if layout == "descending":
            mem = list(range(nc))[::-1]
        elif layout == "gaps":
            mem = list(range(nc))
        else:
            assert layout == "host_entry"
            mem = [c for k in range((nc + 8) // 9 - 1, -1, -1) for c in range(9 * k, min(nc, 9 * k + 9))]
        gaps = GAPS if layout != "descending" else (0,)

        def lay(mem):
            off, at = np.zeros(nc, np.int64), 0
            for k, c in enumerate(mem):
                at += gaps[(k - 1) % len(gaps)] if k else 0
                off[c] = at
                at += int(n[c])
            return off
        off = lay(mem)
        if layout == "host_entry":
            # ... rotated until the call across the middle of the arrays is none of the 64 longest (group A of chain_run_overlapped)
            a = set(group_a(n, chain_extent(n, off)))
            for r in range(nc):
                off = lay(mem[r:] + mem[:r])
                mid = chain_extent(n, off) // 2
                if len(set(np.nonzero((off < mid) & (mid < off + n))[0].tolist()) - a) == 1:
                    break
    total = chain_extent(n, off)
    if layout == "empties":
        mid_call = int(np.argmax(n > 2))
        add = np.array([off[mid_call] + n[mid_call] // 2, total, 0], np.int64)
        at = [0, nc // 2, nc]                                        # first, in the middle and last in the call table
        empty = batch.hdr[:1].copy(); empty["n"] = 0
        hdr = np.insert(hdr, at, np.repeat(empty, 3))
        off = np.insert(off, at, add)
        call_src = np.insert(call_src, at, -1)
    x = np.full(total, 0xdeadbeefdeadbeef, np.uint64); y = np.full(total, 0xfeedfacefeedface, np.uint64)      # (the gaps: nobody's anchors)
    owned = np.concatenate([np.arange(o, o + k) for o, k in zip(off[call_src >= 0], n)] + [np.zeros(0, np.int64)]).astype(np.int64)
    src = np.concatenate([np.arange(o, o + k) for o, k in zip(batch.call_off, n)] + [np.zeros(0, np.int64)]).astype(np.int64)
    assert len(np.unique(owned)) == len(owned) == len(src) == batch.nanchors
    x[owned] = batch.x[src]; y[owned] = batch.y[src]
    return Placed(gabgen.ChainBatch(np.ascontiguousarray(hdr), np.ascontiguousarray(off), x, y), owned, src, call_src, layout == "off_line")


_placed = {}


def placed(calls, layout):
    """CALLS[calls] in `layout`, built once"""
    if (calls, layout) not in _placed:
        _placed[calls, layout] = place(batch_of(calls), layout)
    return _placed[calls, layout]


def placed_of(case):
    return placed(case.calls, case.layout)


def group_a(n_per_call, total):
    """the calls chain_run_overlapped sends ahead, given distinct lengths among the candidates: the 64 longest, then further ones while
    group A holds less than a sixteenth of the extent; at most 512"""
    n = np.asarray(n_per_call, np.int64)
    order = np.argsort(-n, kind="stable")[:512]
    a, acc = [], 0
    for k, c in enumerate(order):
        if n[c] == 0 or (k >= 64 and acc * 16 >= total):
            break
        a.append(int(c)); acc += int(n[c])
    return a


HOST_ENTRY_PATHS = {                  # gab_chain_run: (pins, page-locked)
    "small_batch": ({}, False),
    "fed": ({"GAB_CHAIN_FEED_MIN": "1000"}, True),
    "copy_engines": ({"GAB_CHAIN_FEED_MIN": "1000"}, False),
}
