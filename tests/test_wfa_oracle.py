"""CPU: the wfa oracle (oracle/wfa.c) against golden CIGARs from the compiled reference."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import GOLDEN, read_cigars


@pytest.mark.parametrize("name", ["wfa_bench", "wfa_adv"])
def test_oracle_matches_golden(name):
    batch = gabgen.read_pairs_text(f"{GOLDEN}/{name}.in.txt")
    want = read_cigars(f"{GOLDEN}/{name}.expected.txt")
    assert pyoracle.wfa_cigars(pyoracle.wfa(batch)) == want


@pytest.mark.parametrize("red", [(10, 10), (5, 3), (1, 0)])
def test_oracle_adaptive_matches_golden(red):
    """adaptive reduction (--minimum-wavefront-length / --maximum-difference-distance)"""
    batch = gabgen.read_pairs_text(f"{GOLDEN}/wfa_adv.in.txt")
    want = read_cigars(f"{GOLDEN}/wfa_adv.adaptive_{red[0]}_{red[1]}.expected.txt")
    got = pyoracle.wfa_cigars(pyoracle.wfa(batch, reduction=red))
    assert got == want
    assert got != read_cigars(f"{GOLDEN}/wfa_adv.expected.txt")       # the reduction really changes some alignments


def test_cigar_consistency():
    """size-independent property: the CIGAR consumes both strings and re-scores to the reported penalty"""
    b = gabgen.pairs(77, 3000, 1, 200)
    ops, off, ln, sc = pyoracle.wfa(b)
    for i in range(0, b.n, 7):
        o = bytes(ops[off[i]:off[i] + ln[i]])
        assert o.count(b"M") + o.count(b"X") + o.count(b"D") == b.pat_len[i]
        assert o.count(b"M") + o.count(b"X") + o.count(b"I") == b.txt_len[i]
        pen, prev = 0, b""
        for c in o:
            c = bytes([c])
            if c == b"X": pen += 4
            elif c in (b"I", b"D"): pen += 2 + (6 if c != prev else 0)
            prev = c
        assert pen == sc[i]


def test_edge_cases():
    b = gabgen.pairs_from_lists([b"A", b"ACGT", b"ACGT", b"AAAA", b"ACGTACGT", b"XXYY"], [b"A", b"ACGT", b"AGGT", b"AAAAAAAA", b"ACGT", b"YYXX"])
    got = pyoracle.wfa_cigars(pyoracle.wfa(b))
    assert got[0] == "1M" and got[1] == "4M" and got[2] == "1M1X2M"


# ---- the CPU model of the GPU cascade (tests/util.py) against the oracle: what tests/test_wfa_tiers_gpu.py relies on ---------------
from tests.util import (WFA_BIG_PENALTIES, WFA_CASE_NAMES, WFA_PENALTIES, WFA_REDUCTIONS, wfa_case_model, wfa_fit, wfa_model,
                        wfa_penalty_pairs, wfa_rows, wfa_tier_cases)


def _model_equals_oracle(pats, txts, pen, red):
    b = gabgen.pairs_from_lists(pats, txts)
    m = wfa_model(pats, txts, pen, red)
    _, _, _, score, cells = pyoracle.wfa(b, pen, want_cells=True, reduction=red)
    np.testing.assert_array_equal(m["score"], score)
    assert int(m["work"].sum()) == cells
    for i in range(0, b.n, max(1, b.n // 5)):                       # `work` pair by pair on a few of them, not only in total
        one = gabgen.pairs_from_lists(pats[i:i + 1], txts[i:i + 1])
        assert m["work"][i] == pyoracle.wfa(one, pen, want_cells=True, reduction=red)[4]


def _cross_inputs():
    """every input of the model tests, thinned to what a run under 8 penalty sets x 4 modes can afford: every 10th golden pair,
    150 generator pairs per mode, every 12th pair of each case of wfa_tier_cases -- and every hand-built pair of those cases whole"""
    pats, txts = [], []

    def add(p, t, step=1):
        pats.extend(p[::step]); txts.extend(t[::step])
    for name in ("wfa_bench", "wfa_adv"):
        b = gabgen.read_pairs_text(f"{GOLDEN}/{name}.in.txt")
        pt = [b.pair(i) for i in range(0, b.n, 10)]
        add([p for p, _ in pt], [t for _, t in pt])
    for seed, mode, plen in ((91, 0, 151), (92, 1, 200)):
        b = gabgen.pairs(seed, 150, mode, plen)
        pt = [b.pair(i) for i in range(b.n)]
        add([p for p, _ in pt], [t for _, t in pt])
    cases = wfa_tier_cases()
    seen = set()
    for name in WFA_CASE_NAMES:
        p, t = cases[name][:2]
        if id(p) not in seen:
            seen.add(id(p))
            add(p, t, 1 if len(p) < 20 else 12)
    add([b[0] for b in cases["boundary_pairs"]], [b[1] for b in cases["boundary_pairs"]])
    hp, ht = cases["offb_exit"][:2]
    tails = [i for i in range(len(hp)) if b"Y" in hp[i] or b"X" in ht[i]]
    add([hp[i] for i in tails], [ht[i] for i in tails])
    return pats, txts


_cross = []


@pytest.mark.parametrize("red", [None] + list(WFA_REDUCTIONS))
@pytest.mark.parametrize("pen", WFA_PENALTIES)
def test_model_matches_oracle_everywhere(pen, red):
    """score and work of the model equal the oracle's on the golden inputs, generator pairs of both modes and the batches of
    test_wfa_tiers_gpu.py (thinned, see _cross_inputs) under every penalty set of those tests, in complete mode and under three reductions"""
    if not _cross:
        _cross.append(_cross_inputs())
    _model_equals_oracle(*_cross[0], pen, red)


@pytest.mark.parametrize("name", ["wfa_bench", "wfa_adv"])
def test_model_matches_oracle_on_golden(name):
    b = gabgen.read_pairs_text(f"{GOLDEN}/{name}.in.txt")
    pt = [b.pair(i) for i in range(b.n)]
    for red in (None, (5, 3)):
        _model_equals_oracle([p for p, _ in pt], [t for _, t in pt], (4, 6, 2), red)


@pytest.mark.parametrize("name", WFA_CASE_NAMES)
def test_model_matches_oracle_on_tier_cases(name):
    """each batch of test_wfa_tiers_gpu.py whole, under its own penalties and reduction; every launch before the last hands pairs on
    or finishes some, and the launches account for every pair"""
    batch, pen, red, knobs, model, plan, tier, launches = wfa_case_model(name)
    _, _, _, score, cells = pyoracle.wfa(batch, pen, want_cells=True, reduction=red)
    np.testing.assert_array_equal(model["score"], score)
    assert int(model["work"].sum()) == cells
    assert (tier >= 0).all() and sum(l[3] - l[4] for l in launches) == batch.n
    for k, l in enumerate(launches):
        assert l[3] - l[4] == int((tier == k).sum())


def test_model_single_pair_form():
    r = wfa_model(b"ACGTACGTAC", b"ACGTTCGTAC", (4, 6, 2))
    assert r["score"] == 4 and r["rows"] == 2 and r["used"] == 1 + 3 and r["max_m"] == 10 and r["work"] == 3 + 9        # three cells of score 4; ACGT, then CGTAC behind the mismatch


def test_row_table_boundaries():
    """hand-derived for (4, 6, 2): the history first exceeds 1 152 .. 1 184 offsets at score 42, 2 560 at 62, 6 144 at 94 -- found by
    the recurrence; and the allocation the batch model reports per pair is the table's used_end of its final score"""
    rows = wfa_rows((4, 6, 2))
    assert [r[0] for r in rows[:6]] == [0, 4, 8, 10, 12, 14] and rows[1][1:] == (-1, 1, False, 4) and rows[2][1:] == (-2, 2, True, 19)
    first_over = lambda pool: next(r[0] for r in rows if r[4] > pool)
    assert [first_over(p) for p in (1152, 1168, 1184, 2560, 6144)] == [42, 42, 42, 62, 94]
    assert wfa_fit((4, 6, 2), 1152) == (40, 42) and wfa_fit((4, 6, 2), 2560) == (60, 62) and wfa_fit((4, 6, 2), 6144) == (92, 94)
    assert len(rows) == 121 and rows[-1][:3] == (244, -120, 120)          # the table ends where a diagonal would pass 120
    by_score = {r[0]: (k, r[4]) for k, r in enumerate(wfa_rows((4, 6, 2), table=False, max_score=400))}
    _, _, _, _, model, _, _, _ = wfa_case_model("census")
    short = model["score"] <= 400
    assert short.sum() >= 1500
    for s, nrow, used in zip(model["score"][short], model["rows"][short], model["used"][short]):
        assert by_score[int(s)] == (nrow - 1, used)


def test_census_gives_every_launch_pairs():
    """each census batch gives every launch of its plan at least 20 pairs, by the model alone"""
    for name, kinds in (("census", 5), ("adaptive_10_50", 4), ("grid", 5), ("census1000_2_3_1", 5), ("census1000_5_8_3", 5), ("census1000_3_1_4", 5)):
        launches = wfa_case_model(name)[7]
        assert len(launches) >= kinds and all(l[3] - l[4] >= 20 for l in launches[:kinds] if l[0] != "wfa_global<true>"), (name, launches)
    # (1, 1, 1): no census pair scores beyond what 49 152 offsets hold; (5, 3) cuts the history so far that none passes that tier
    assert wfa_case_model("census1000_1_1_1")[7][4][3] == 0 and wfa_case_model("adaptive_5_3")[7][3][3] == 0
    print("census:", [(l[0], l[1], l[3] - l[4]) for l in wfa_case_model("census")[7]])


def test_plan_switches():
    """the host's choices the GPU cases are built around, as the plan restates them"""
    plan = lambda name: wfa_case_model(name)[5]
    assert plan("census")["static_pool"] == 1168 and plan("census")["n_big"] == 3 and plan("census")["slots"] == 1496
    assert plan("tmax227")["static_rows"] == 16 and plan("tmax227")["use_static"] and not plan("tmax227")["byte_ok"]
    assert plan("tmax228")["static_rows"] == 15 and not plan("tmax228")["use_static"]
    assert plan("tmax228")["launches"][0] == ("wfa_lds<16,false,int16_t>", 1024, 48)
    assert len(wfa_rows((300, 400, 150))) < 16 and not plan("pen_300_400_150")["use_static"] and plan("pen_300_400_150")["byte_ok"]
    assert plan("pen_50_60_20")["use_static"] and not plan("pen_50_60_20_nostatic")["use_static"]
    assert [l[1] for l in plan("pool2_1024")["launches"]] == [1168, 6144, 49152, 1 << 20]
    assert plan("slots_3")["slots"] == 3 and plan("slots_1002")["slots"] == 1002 and plan("grid")["slots"] == 3000


def test_boundary_pairs_score_what_they_were_built_for():
    """each boundary pair gets from the oracle exactly the score it was built for, and the model puts the pair on the last score that
    fits into the launch with that pool and its neighbour into the next launch"""
    cases = wfa_tier_cases()
    bound = cases["boundary_pairs"]
    assert [b[2] for b in bound] == [40, 42, 60, 62, 92, 94, 258, 260]
    b = gabgen.pairs_from_lists([x[0] for x in bound], [x[1] for x in bound])
    assert pyoracle.wfa(b)[3].tolist() == [x[2] for x in bound]
    batch, pen, red, knobs, model, plan, tier, launches = wfa_case_model("boundary")
    where = {batch.pair(i): int(tier[i]) for i in range(batch.n)}
    assert [where[x[0], x[1]] for x in bound] == [0, 1, 1, 2, 2, 3, 3, 4]
    pp, pt, built = wfa_penalty_pairs()
    for p in WFA_BIG_PENALTIES:
        assert pyoracle.wfa(gabgen.pairs_from_lists(pp, pt), p)[3].tolist() == built(p)
    assert built((300, 400, 150)) == [0, 300, 600, 900, 550, 700, 1250] and max(built((1000, 1500, 500))) == 4500
