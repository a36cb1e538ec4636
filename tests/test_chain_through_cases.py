"""CPU: every case of tests/chain_through_cases.py reaches the route (gab_chain_last_through) and the kernel forms it is named for -- by
tests.util's models of chain.hip's rules and by the oracle alone, so that no case of tests/test_chain_through_gpu.py can pass without
having run what it is about."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import chain_form_cases as form_cases
from tests import chain_through_cases as tc
from tests.util import (CHAIN_FORM_LATENCY, CHAIN_FORM_LEGACY, CHAIN_FORM_TABLE, CHAIN_FORM_THROUGHPUT, CHAIN_SEVEN_HELPERS, GOLDEN, chain_extent,
                        chain_split_margins, chain_split_model, chain_through_route, read_chain_output)

CASES = tc.through_cases()
fold = lambda f: 3 if f in (4, 5) else f


def split_of(case, mode):
    pl = tc.placed_of(case)
    return chain_split_model(pl.batch.hdr["n"], mode, case.env, through=bool(case.pinned), total=pl.total)


def test_case_names_are_unique_and_layouts_known():
    assert len({c.name for c in CASES}) == len(CASES)
    assert {c.layout for c in CASES} == set(tc.LAYOUTS) | {None, "scattered_empty"}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_reaches_its_route_and_forms(case):
    pl = tc.placed_of(case)
    n, off = pl.batch.hdr["n"], pl.batch.call_off
    assert pl.total == chain_extent(n, off) == len(pl.batch.x) and (len(pl.owned) == n.sum())
    for mode in case.modes:
        split = split_of(case, mode)
        assert ((split == 0) == (n == 0)).all()
        hint = None
        if case.forms:
            assert case.layout is None and [fold(f) for f in case.forms[mode]] == split.tolist()
            hint = case.forms[mode]
        if case.all_form is not None:
            assert (split[n > 0] == fold(case.all_form)).all() and (n > 0).any(), (case.name, mode, np.bincount(split).tolist())
        for f in case.has_form:
            assert fold(f) in split.tolist(), (case.name, mode, f)
        if {4, 5} & set(case.has_form):
            hint = [5]
        assert chain_through_route(n, off, mode, case.env, case.pinned, hint) == case.route, (case.name, mode)
        if case.route == 4:
            # ... and only the forms tell 4 from 1: the table form writes through, and takes part
            assert chain_through_route(n, off, mode, case.env, case.pinned) == 1 and CHAIN_FORM_TABLE in split.tolist()
        single = case.pinned and (n > 0).any() and not np.isin(split, (CHAIN_FORM_TABLE, CHAIN_FORM_LATENCY, CHAIN_FORM_LEGACY)).any()
        if single and case.route == 1:
            # one launch of the throughput form: written only with three helpers -- clear of the seven-helper rule by 10 %
            assert pl.total > 1.1 * CHAIN_SEVEN_HELPERS * int(n.max()), (case.name, pl.total, int(n.max()))
        if single and case.route == 3:
            assert pl.total <= CHAIN_SEVEN_HELPERS * int(n.max()) / 1.1
        if case.default_rule:
            assert not case.env
            assert all(abs(m - 1) > 0.1 for m in chain_split_margins(n, mode, through=bool(case.pinned), total=pl.total)), (case.name, mode)
        else:
            assert case.env or not (n > 0).any() or case.pinned is None


@pytest.mark.parametrize("mode", [0, 1])
def test_every_route_and_form_has_a_case(mode):
    mine = [c for c in CASES if mode in c.modes]
    assert {c.route for c in mine} == {0, 1, 2, 3, 4}
    # a route-1 case for each launch that writes through: the throughput form alone, the table form alone, both, the legacy launch with three helpers
    written = [set(split_of(c, mode).tolist()) - {0} for c in mine if c.route == 1 and c.pinned]
    for forms in ({CHAIN_FORM_THROUGHPUT}, {CHAIN_FORM_TABLE}, {CHAIN_FORM_THROUGHPUT, CHAIN_FORM_TABLE}, {CHAIN_FORM_LEGACY}):
        assert forms in written, forms
    # ... a route-3 case for each that does not: the latency form, five helpers, seven helpers by the rule, (chain) the walk kernel
    copied = [c for c in mine if c.route == 3]
    assert any(CHAIN_FORM_LATENCY in split_of(c, mode) for c in copied)
    assert any(c.env.get("GAB_CHAIN_HELPERS") == "5" for c in copied) and any(not c.env and c.all_form == 1 for c in copied)
    assert any(c.env.get("GAB_CHAIN_KERNEL") == "walk" for c in copied) == (mode == 0)
    seen = set()
    for c in mine:
        seen |= set(c.forms[mode] if c.forms else ()) | set(c.has_form) | ({c.all_form} if c.all_form is not None else set())
    assert seen >= {1, 2, 3, 4, 5, 6}
    # every layout, for a batch of one launch and for one of two
    for lay in tc.LAYOUTS:
        assert len([c for c in mine if c.layout == lay and c.route == 1]) == 2


def test_edge_lengths_are_all_there():
    for key in ("edges_tp", "edges_tp_default"):
        n = tc.batch_of(key).hdr["n"]
        assert n.max() == 193 and all((n == k).sum() >= 1 for k in form_cases.EDGE_LENGTHS if k <= 193)
        assert all((n == k).sum() == 1 for k in (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193))
    assert tuple(tc.batch_of("edges_tab").hdr["n"]) == form_cases.EDGE_LENGTHS
    # the smallest batches the rules allow: within 2 % of their thresholds' 115 %
    assert tc.batch_of("edges_tp").nanchors < 1.17 * CHAIN_SEVEN_HELPERS * 193 and tc.batch_of("edges_tp_default").nanchors < 1.17 * 1140 * 193


def test_layouts():
    b = tc.batch_of("side_by_side")
    n = b.hdr["n"].astype(np.int64)
    d = tc.place(b, "descending")
    assert (np.diff(d.batch.call_off) < 0).all() and d.total == b.nanchors
    g = tc.place(b, "gaps")
    gap = g.batch.call_off[1:] - (g.batch.call_off[:-1] + n[:-1])
    assert gap.tolist() == [tc.GAPS[k % 3] for k in range(len(n) - 1)] and g.total == b.nanchors + gap.sum()
    assert (g.batch.call_off % 16 != 0).sum() > len(n) // 2 and (g.batch.call_off % 64 != 0).sum() > len(n) // 2
    assert len(g.owned) == b.nanchors and g.total - len(np.unique(g.owned)) == gap.sum()
    e = tc.place(b, "empties")
    k = np.nonzero(e.call_src < 0)[0]
    assert k.tolist() == [0, len(n) // 2 + 1, len(n) + 2] and (e.batch.hdr["n"][k] == 0).all() and e.total == b.nanchors
    o = e.batch.call_off[k]
    inside = (e.batch.call_off < o[0]) & (o[0] < e.batch.call_off + e.batch.hdr["n"])
    assert inside.sum() == 1 and o[1] == e.total and o[2] == 0
    np.testing.assert_array_equal(e.batch.hdr["n"][e.call_src >= 0], n)
    for p in (d, g, e):
        np.testing.assert_array_equal(p.batch.x[p.owned], b.x[p.src]); np.testing.assert_array_equal(p.batch.y[p.owned], b.y[p.src])
        for c in np.nonzero(p.call_src >= 0)[0][::37]:          # a call's anchors are the call's, in order
            s, a, k = p.call_src[c], int(p.batch.call_off[c]), int(p.batch.hdr["n"][c])
            np.testing.assert_array_equal(p.batch.x[a:a + k], b.x[int(b.call_off[s]):int(b.call_off[s]) + k])
    s = tc.placed_of([c for c in CASES if c.layout == "scattered_empty"][0])
    assert s.total == 5 and len(s.owned) == 0 and not s.batch.hdr["n"].any()


def test_no_room_case_cannot_fit():
    n = tc.batch_of("no_room").hdr["n"]
    groups = tc.NO_ROOM_MB * 1024                          # 1 KB per group of 16 rows x 64 anchors
    assert tc.least_groups(n) > 1.1 * groups and n[-1] == n.max() and (n == n.max()).sum() == 1
    # the longest call, placed first, fits with room to spare
    assert tc.most_groups(tc.CALLS["no_room"]()[-1]) < 0.9 * groups


def test_patched_case_is_one_where_max_skip_decides():
    length, anchor, back = tc.PATCHED[5:]
    b = tc.batch_of("patched")
    assert b.hdr["n"].tolist() == [160] * 21 + [length] and b.call_off[-1] == 21 * 160
    (s0, p0), (s1, p1) = pyoracle.chain(b, 0), pyoracle.chain(b, 1)
    o = int(b.call_off[-1])
    assert ((s0[o:] != s1[o:]) | (p0[o:] != p1[o:])).sum() >= 1          # chain is not fast-chain here: max_skip cut a scan short
    assert p0[o + anchor] == anchor - back and p1[o + anchor] != p0[o + anchor]
    assert anchor // 64 + 2 < (length + 63) // 64                       # blocks behind the patched one have been folded and are folded again


def test_dense_case_is_the_golden_one():
    b = tc.batch_of("dense")
    ws, wp = read_chain_output(f"{GOLDEN}/chain_dense.chain.expected.txt")
    s, p = pyoracle.chain(b, 0)
    np.testing.assert_array_equal(s, ws); np.testing.assert_array_equal(p, wp)
    fs, fp = pyoracle.chain(b, 1)
    assert ((s != fs) | (p != fp)).sum() > 100          # hundreds of anchors where max_skip decides: more than eight patches in a call


def test_host_entry_layout():
    """the layout gab_chain_run is given on its three paths: out of order, with gaps, and -- for the copy-engine path -- calls beyond
    group A on both sides of the middle of the arrays, one of them ACROSS it, so that the first piece of results ends before the middle
    (`cut`).  (A call that lies wholly below the middle cannot begin behind a call that ends beyond it unless calls overlap, and
    overlapping calls have no defined result: the second piece of results never holds a whole first-half call of a valid batch.)"""
    pl = tc.place(tc.batch_of("host_entry"), "host_entry")
    n, off, total = pl.batch.hdr["n"].astype(np.int64), pl.batch.call_off, pl.total
    srt = np.sort(n)[::-1]
    assert len(n) > 64 and srt[63] > srt[64] and srt[:64].sum() * 16 >= total          # group A: exactly the 64 longest
    a = tc.group_a(n, total)
    assert len(a) == 64 and set(n[a].tolist()) == set(srt[:64].tolist())
    rest = np.setdiff1d(np.arange(len(n)), a)
    mid = total // 2
    first = rest[off[rest] + n[rest] <= mid]
    second = rest[off[rest] + n[rest] > mid]
    across = second[off[second] < mid]
    assert len(first) > 10 and len(second) > 10 and len(across) == 1
    cut = min(mid, int(off[second].min()))
    assert 0 < cut < mid and cut == off[across[0]]
    # out of order: first-half calls before AND behind second-half calls in the call table, and call_off does not ascend
    assert first.min() < second.max() and first.max() > second.min() and (np.diff(off) < 0).any()
    assert (off[1:] != off[:-1] + n[:-1]).sum() > len(n) // 2 and total > n.sum()      # gaps
    for pins, _ in tc.HOST_ENTRY_PATHS.values():
        assert total >= int(pins.get("GAB_CHAIN_FEED_MIN", total))
