"""The constructed batches of tests/bitpal_cases.py reach the edges they are named for (no GPU): by the routing model there, whose
constants are read back from genarchbench_amd/csrc/bitpal.hip and include/gab.h here; and the oracle equals a plain DP on the small ones."""
import os
import re

import numpy as np
import pytest

from tests import bitpal_cases as bc

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(_ROOT, "genarchbench_amd", "csrc", "bitpal.hip")
MODES = [(bc.EDIT, False), (bc.EDIT, True), (bc.SCORED, False)]


def test_constants_are_the_ones_in_the_sources():
    src = open(_SRC).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert const("kChunk") == bc.CHUNK and const("kLdsRows") == bc.LDS_ROWS and const("kBigBlocks") == bc.BIG_BLOCKS
    assert const("kBvMaxRows") == bc.BV_MAX_ROWS and const("kBvBlock") == bc.BV_BLOCK and const("kBvSlots") == len(bc.SLOT_LETTERS) + 1
    slots = re.search(r"int bitpal_bv_slot\(uint32_t ch\) \{\s*return (.*?);\s*\}", src, re.S).group(1)
    assert re.findall(r"ch == '(.)' \? (\d)", slots) == [(chr(c), str(k)) for k, c in enumerate(bc.SLOT_LETTERS)] and slots.endswith(": 5")
    assert "std::min<int64_t>(gab_ceil_div(n, 256), %d)" % bc.GRID_CAP in src and src.count("__launch_bounds__(256) void bitpal_") == 2
    assert "std::min<int64_t>((n_big + 63) / 64, kBigBlocks)" in src and "std::min(std::max(h->h_ct->max_rows_lds, 1), kBvMaxRows)" in src
    assert "switch ((rows + 31) / 32)" in src and "if (pl <= tl) { nr = pl; rs = p;" in src
    assert src.count("<= kLdsRows") == 2 and "big = nr > kLdsRows" in src            # bitpal_classify, bitpal_scatter; bitpal_edit_bv
    hdr = open(os.path.join(_ROOT, "include", "gab.h")).read()
    assert int(re.search(r"#define GAB_BITPAL_MAX_LEN (\d+)", hdr).group(1)) == bc.MAX_LEN
    enum = re.search(r"enum \{([^}]*GAB_BITPAL_PATHS)\s*\};", hdr).group(1)
    names = re.findall(r"GAB_BITPAL_PATH_([A-Z_]+),", enum)
    assert tuple(n.lower() for n in names) == bc.PATH_KEYS
    from genarchbench_amd.bitpal import BitpalEngine
    assert BitpalEngine.PATH_KEYS == bc.PATH_KEYS


# ------------------------------------------------------------------------------------------------ width_D
@pytest.mark.parametrize("D", range(1, 9))
def test_width_batches_launch_their_width_and_nothing_else(D):
    b = bc.width(D)
    r = bc.route(b, bc.EDIT)
    assert r.paths == dict.fromkeys(bc.PATH_KEYS, 0) | {"bv_words": D, "bv_pairs": b.n} and (r.path == bc.BV).all()
    rows = np.minimum(b.pat_len, b.txt_len); cols = np.maximum(b.pat_len, b.txt_len)
    want = {1, 31, 32, 33, 32 * D - 1, 32 * D} | {32 * w + d for w in range(1, D) for d in (-1, 0, 1)}
    assert set(rows.tolist()) == {x for x in want if x <= 32 * D} and 32 * (D - 1) < rows.max() <= 32 * D
    for x in set(rows.tolist()):
        assert set((cols[rows == x] - x).tolist()) == set(bc.COLUMN_EXTRA)
    assert b.n == len(bc.width_rows(D)) * len(bc.COLUMN_EXTRA) * len(bc.CONTENTS) and (b.pat_len > b.txt_len).any()
    ed = bc.expected("width_%d" % D, bc.EDIT).reshape(-1, len(bc.CONTENTS))
    c2 = cols.reshape(-1, len(bc.CONTENTS)); r2 = rows.reshape(-1, len(bc.CONTENTS))
    k = bc.CONTENTS.index
    np.testing.assert_array_equal(ed[:, k("identical")], -(c2 - r2)[:, k("identical")])          # the rows are a prefix of the columns
    np.testing.assert_array_equal(ed[:, k("disjoint")], -c2[:, k("disjoint")])                    # distance = columns
    np.testing.assert_array_equal(ed[:, k("one_base")], -(c2 - r2)[:, k("one_base")])
    assert (ed[:, k("edits")] < -(c2 - r2)[:, k("edits")]).any()
    # every word boundary below D: some pair's distance needs the carry of the add across it (the rows of the "across" pairs)
    pairs = [b.pair(i) for i in range(k("across"), b.n, len(bc.CONTENTS))]
    dist = [bc.myers_words(p, t, D) for p, t in pairs]
    assert dist == (-ed[:, k("across")]).tolist()
    for w in range(1, D):
        assert any(bc.myers_words(p, t, D, no_carry_into=w) != d for (p, t), d in zip(pairs, dist)), w
    # the other modes take the same batch through the LDS column, slot = pair
    for alg, no_bv in MODES[1:]:
        assert bc.route(b, alg, no_bv).paths == dict.fromkeys(bc.PATH_KEYS, 0) | {"lds_pairs": b.n, "lds_rows": int(rows.max())}


# ------------------------------------------------------------------------------------------------ routes
def test_bv_routes_reasons_and_their_mix():
    b, why = bc.bv_routes()
    r = bc.route(b, bc.EDIT)
    np.testing.assert_array_equal(r.reason, why)
    assert r.paths == dict.fromkeys(bc.PATH_KEYS, 0) | {"bv_words": 8, "bv_pairs": int((why == 0).sum()), "lds_pairs": int((why != 0).sum()),
                                                        "lds_rows": 258, "id_lists": 1}
    assert b.n % 64 and b.n % 256 and b.n > 256
    for w0 in range(0, b.n, 64):                       # accepted and rejected pairs inside every wave
        assert {bc.NO_REJECT, bc.BY_BYTE} <= set(why[w0:w0 + 64].tolist())
    rows = np.minimum(b.pat_len, b.txt_len)
    assert set(rows[why == bc.BY_ROWS].tolist()) == {257, 258} and 256 in rows[why == bc.NO_REJECT] and 0 in rows[why == bc.NO_REJECT]
    assert ((b.pat_len == 0) & (b.txt_len == 0)).any()
    pairs = [b.pair(i) for i in range(b.n)]
    acgtn = set(bc.SLOT_LETTERS)
    # an outside byte in the column string alone stays; lower case on either side; N in both; the rule for equal lengths
    assert any(why[i] == 0 and set(p) - acgtn and len(p) > len(t) for i, (p, t) in enumerate(pairs))
    assert any(why[i] == 0 and set(t) - acgtn and len(t) > len(p) for i, (p, t) in enumerate(pairs))
    assert why[pairs.index((b"ACxT", b"ACGT"))] == bc.BY_BYTE and why[pairs.index((b"ACGT", b"ACxT"))] == bc.NO_REJECT
    assert why[pairs.index((b"acgt", b"ACGT"))] == bc.BY_BYTE and why[pairs.index((b"ACGT", b"acgt"))] == bc.NO_REJECT
    assert why[pairs.index((b"NNNN", b"NNNNNN"))] == bc.NO_REJECT
    outside = {c for i, (p, t) in enumerate(pairs) if why[i] == bc.BY_BYTE for c in set(p if len(p) <= len(t) else t) - acgtn}
    assert {0x00, 0xff, ord("a"), ord("n"), ord("x")} <= outside


def test_all_reject_none_reject_all_long():
    z = dict.fromkeys(bc.PATH_KEYS, 0)
    b = bc.all_reject(); r = bc.route(b, bc.EDIT)
    assert (r.reason == bc.BY_BYTE).all() and r.paths == z | {"bv_words": 2, "lds_pairs": b.n, "lds_rows": 50, "id_lists": 1}
    b = bc.none_reject(); r = bc.route(b, bc.EDIT)
    assert (r.path == bc.BV).all() and r.paths == z | {"bv_words": 2, "bv_pairs": b.n}       # no DP launch at all
    b = bc.all_long()
    assert b.n == 2 and bc.route(b, bc.EDIT).paths == z | {"bv_words": 1, "global_pairs": 2, "global_blocks": 1, "global_rows": 2060, "id_lists": 1}
    assert (bc.route(b, bc.EDIT).reason == bc.BY_ROWS).all() and bc.route(b, bc.SCORED).long_pairs == 2


def test_switch_2048_puts_two_row_counts_on_each_side():
    b = bc.switch_2048()
    rows = np.minimum(b.pat_len, b.txt_len); cols = np.maximum(b.pat_len, b.txt_len)
    assert b.n <= 64 and set(rows[rows > 100].tolist()) == set(bc.SWITCH_ROWS) and {1, 100} <= set(rows.tolist())
    assert set((cols - rows)[rows > 100].tolist()) == {0, 40} and (b.pat_len > b.txt_len).any()
    for alg, no_bv in MODES:
        r = bc.route(b, alg, no_bv)
        np.testing.assert_array_equal(np.flatnonzero(r.path == bc.GLOBAL), np.flatnonzero(rows >= 2049))
        np.testing.assert_array_equal(np.flatnonzero((r.path == bc.LDS) & (rows > 100)), np.flatnonzero((rows == 2047) | (rows == 2048)))
        assert r.paths["lds_rows"] == bc.LDS_ROWS == 2048 and r.paths["global_rows"] == 2050 and r.paths["global_pairs"] == 4 == r.long_pairs
        assert r.paths["id_lists"] == 1 and (r.paths["bv_words"], r.paths["bv_pairs"]) == ((8, b.n - 8) if (alg, no_bv) == MODES[0] else (0, 0))
    assert (bc.LDS_ROWS + 1) * 64 <= 160 * 1024          # the largest dynamic LDS request fits what gab_bitpal_create asks for


def test_bytes_256_meets_every_byte_at_every_place():
    b = bc.bytes_256()
    assert b.n == 256
    for v in range(256):
        p, t = b.pair(v)
        r, c = (t, p) if v & 1 else (p, t)
        assert r == bytes([v]) * 8 and len(c) == 12
        for place in range(4):
            assert {c[place], c[4 + place], c[8 + place]} == {v, v ^ 0x80, v ^ 0x01}
        assert bc.plain_dp(p, t, bc.EDIT) == -8 and bc.plain_dp(p, t, bc.SCORED) == 4 - 2 * 4 - 4 * 4       # four matches of twelve columns
    for alg, no_bv in MODES[1:]:
        assert bc.route(b, alg, no_bv).paths == dict.fromkeys(bc.PATH_KEYS, 0) | {"lds_pairs": 256, "lds_rows": 8}
    assert bc.route(b, bc.EDIT).paths["bv_pairs"] == len(bc.SLOT_LETTERS)


def test_chunk_edges_lengths_and_alignments():
    b = bc.chunk_edges()
    rows = np.minimum(b.pat_len, b.txt_len); cols = np.maximum(b.pat_len, b.txt_len)
    assert set(cols.tolist()) == set(bc.CHUNK_COLUMNS) and set(rows.tolist()) == set(bc.CHUNK_ROWS)
    pat_rows = b.pat_len < b.txt_len
    assert pat_rows.any() and (b.pat_len > b.txt_len).any()
    ro = np.where(b.pat_len <= b.txt_len, b.pat_off, b.txt_off) % 4; co = np.where(b.pat_len <= b.txt_len, b.txt_off, b.pat_off) % 4
    for c in bc.CHUNK_COLUMNS[1:]:
        for r in bc.CHUNK_ROWS:
            sel = (rows == r) & (cols == c)
            assert set(ro[sel].tolist()) == set(co[sel].tolist()) == {0, 1, 2, 3}, (r, c)
    for alg, no_bv in MODES[1:]:
        assert bc.route(b, alg, no_bv).paths == dict.fromkeys(bc.PATH_KEYS, 0) | {"lds_pairs": b.n, "lds_rows": 18}


def test_classify_stride_needs_a_second_trip():
    b = bc.classify_stride()
    assert b.n == 131072 + 256 + 3 == bc.CLASSIFY_STRIDE_PAIRS and bc.GRID_CAP * 256 == 131072
    rows = np.minimum(b.pat_len, b.txt_len)
    assert rows[:-1].min() == 1 and max(b.pat_len[:-1].max(), b.txt_len[:-1].max()) == 8 and rows[-1] == 2049
    for alg, no_bv in MODES:
        r = bc.route(b, alg, no_bv)
        assert r.classify_trips == 2 and r.long_pairs == 1 and r.paths["global_pairs"] == 1 and r.paths["id_lists"] == 1
        assert np.flatnonzero(r.path == bc.GLOBAL).tolist() == [b.n - 1] and b.n - 1 >= bc.GRID_CAP * 256      # bitpal_scatter strides to it
    assert bc.route(b, bc.EDIT).paths["bv_words"] == 1 and bc.route(b, bc.EDIT).paths["bv_pairs"] == b.n - 1
    bad = bc.classify_stride(True)
    assert bad.n == b.n + 1 and bc.bad_pairs(bad).tolist() == [b.n] and bad.pat_len[-1] == -1


def test_global_second_trip_needs_a_second_trip():
    b = bc.global_second_trip()
    assert b.n == 16384 + 70 == bc.GLOBAL_SECOND_TRIP_PAIRS
    four = [b.pair(i) for i in range(4)]
    assert tuple(min(len(p), len(t)) for p, t in four) == bc.SECOND_TRIP_ROWS == (2049, 2055, 2060, 2049) and len({p for p, _ in four}) == 4
    assert all(b.pair(i) == four[i % 4] for i in (4, 5, 6, 7, 16383)) and all(b.pair(i) == four[(i + 1) % 4] for i in (16384, 16385, b.n - 1))
    assert len(set(bc.expected("global_second_trip", bc.EDIT)[:4].tolist())) == 4 and len(b.pat) < 10000
    for alg, no_bv in MODES:
        r = bc.route(b, alg, no_bv)
        assert r.global_trips == 2 and r.paths["global_blocks"] == bc.BIG_BLOCKS and r.paths["global_pairs"] == b.n > 64 * r.paths["global_blocks"]
        assert r.paths["lds_pairs"] == 0 and r.paths["bv_pairs"] == 0 and r.paths["global_rows"] == 2060
    # in list order = pair order, the lane of slot 16384 + L ran slot L before: a different one of the four
    idx = bc.second_trip_index()
    assert (idx[16384:] != idx[:70]).all() and set(idx[16384:].tolist()) == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------ limits
def test_limits_one_batch_per_condition():
    acc = bc.limits_accepted()
    assert (acc.pat_len[0], acc.txt_len[0], acc.pat_len[1], acc.txt_len[1]) == (bc.MAX_LEN, 1, 1, bc.MAX_LEN) and bc.bad_pairs(acc).size == 0
    ref = bc.limits_refused()
    assert set(ref) == {s + k for s in ("pat", "txt") for k in ("_len_over", "_len_negative", "_off_negative", "_end_past_slab")} | {"two_bad"}
    for name, r in ref.items():
        assert bc.bad_pairs(r.batch, r.pat_bytes, r.txt_bytes).tolist() == list(r.bad), name
        assert 0 < r.bad[0] and r.bad[-1] < r.batch.n - 1, name                      # good pairs on both sides
        # exactly one condition fails per bad pair
        i = r.bad[0]; b = r.batch
        fails = [b.pat_len[i] < 0, b.txt_len[i] < 0, b.pat_len[i] > bc.MAX_LEN, b.txt_len[i] > bc.MAX_LEN, b.pat_off[i] < 0, b.txt_off[i] < 0,
                 ((b.pat_off[i] + b.pat_len[i] + 3) & ~3) > r.pat_bytes, ((b.txt_off[i] + b.txt_len[i] + 3) & ~3) > r.txt_bytes]
        assert sum(bool(f) for f in fails) == 1, name
    assert ref["pat_len_over"].batch.pat_len[3] == bc.MAX_LEN + 1 and ref["txt_len_over"].batch.txt_len[3] == bc.MAX_LEN + 1
    for side in ("pat", "txt"):
        r = ref[side + "_end_past_slab"]
        end = int(getattr(r.batch, side + "_off")[2] + getattr(r.batch, side + "_len")[2])
        assert end == getattr(r, side + "_bytes") and end % 4 == 1 and bc.bad_pairs(r.batch).size == 0      # every byte is there, the dword is not
    assert bc.refusal_message(ref["two_bad"]) == "2 pair(s) violate the limits (first: pair 2)"
    assert bc.refusal_message(ref["txt_len_negative"], host=True) == "negative offset/length at pair 5"
    b, pe, te = bc.exact_slabs()
    assert pe % 4 == 0 and te % 4 == 0 and pe == int((b.pat_off + b.pat_len).max()) and te == int((b.txt_off + b.txt_len).max())
    assert bc.bad_pairs(b, pe, te).size == 0 and bc.bad_pairs(b, pe - 1, te).tolist() == [b.n - 1] and bc.bad_pairs(b, pe, te - 1).tolist() == [b.n - 1]


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("alg", [bc.EDIT, bc.SCORED], ids=["edit", "scored"])
@pytest.mark.parametrize("name", ["bv_routes", "chunk_edges", "bytes_256"])
def test_oracle_equals_a_plain_dp(name, alg):
    b = bc.BATCHES[name]()
    want = bc.expected(name, alg)
    assert not want.flags.writeable
    np.testing.assert_array_equal(want, [bc.plain_dp(*b.pair(i), alg) for i in range(b.n)])
