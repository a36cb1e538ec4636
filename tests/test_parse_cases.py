"""The constructed parser inputs of tests/parse_cases.py reach the edges they are named for (no GPU): computed from the texts and the
constants of genarchbench_amd/csrc/parse.hip, which are read back from the source here."""
import os
import re

import numpy as np
import pytest

from tests import parse_cases as pc

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "genarchbench_amd", "csrc", "parse.hip")


def test_constants_are_the_ones_in_parse_hip():
    src = open(_SRC).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert const("kSubBytes") == pc.SUB_BYTES and const("kSubs") == pc.SUBS and const("kPer") == pc.SCAN_PER
    assert const("kCopyUnroll") == pc.COPY_UNROLL and const("kHdrSlot") == pc.HDR_SLOT
    assert "c0 += 1024 * kPer" in src and pc.SCAN_TRIP == 1024 * pc.SCAN_PER
    assert src.count("(int64_t)threadIdx.x * %d;" % pc.SPAN) == 2 and src.count("base + %d <= n" % pc.SPAN) == 2      # nl_count, nl_fill
    assert "for (int v = %d + lane; v < nT[u]; v += 64)" % pc.COPY_TRIP_DWORDS in src
    assert "b0 = wave * 64; b0 < npairs; b0 += nwaves * 64" in src and "blockIdx.x * 4 +" in src and pc.CODES_WG_PAIRS == 4 * 64
    assert "hl <= %d && l1 >= 1 && l1 <= %d && l2 >= 1 && l2 <= %d" % pc.BSW_MAX in src
    assert "len < kHdrSlot" in src


# ------------------------------------------------------------------------------------------------ nl_positions
LONG = ("end_on_span", "end_1_past", "end_63_past_even", "end_63_past_odd")


def test_nl_positions_cover_every_bit_of_both_paths():
    texts = pc.nl_positions()
    whole, last = set(), set()
    for t in texts.values():
        w, l = pc.nl_residues(t)
        whole |= w; last |= l
    assert whole == set(range(64))
    assert last == set(range(63))              # (a last span of 64 bytes is a whole one)
    for name in LONG:                          # each long text alone has every bit of the uint4 path, bit 0 and bit 63 included
        assert pc.nl_residues(texts[name])[0] == set(range(64)), name
    assert [len(texts[k]) % 64 for k in LONG] == [0, 1, 63, 63]
    assert pc.nl_residues(texts["end_on_span"])[1] == set() and pc.nl_residues(texts["end_1_past"])[1] == {0}
    assert pc.nl_residues(texts["end_63_past_even"])[1] == set(range(0, 63, 2)) and pc.nl_residues(texts["end_63_past_odd"])[1] == set(range(1, 63, 2))
    assert 0 < len(texts["under_64"]) < 64 and texts["under_64"].count(b"\n") == 6
    assert texts["no_newline"] and b"\n" not in texts["no_newline"] and texts["one_line"].count(b"\n") == 1 and texts["empty"] == b""


def test_nl_positions_sit_on_sweep_and_block_edges():
    texts = pc.nl_positions()
    on = lambda b: {k for k in LONG if texts[k][b:b + 1] == b"\n"}
    S, B = pc.SUB_BYTES, pc.BLOCK_BYTES
    assert (S, B) == (16384, 131072)
    for b in (S - 1, B - 1, 2 * B - 1):        # last byte of a sweep / a block
        assert on(b) == {"end_on_span", "end_63_past_even"}
    for b in (S, B, 2 * B):                    # first byte of the next
        assert on(b) == {"end_1_past", "end_63_past_odd"}
    for k in LONG:                             # about 300 KB: the carry crosses the eight sweeps of two whole blocks, the third is partial
        assert 2 * B + 2 * S < len(texts[k]) < 3 * B


def test_nl_masks_of_two_byte_lines():
    texts = pc.nl_positions()
    a, b = pc.span_masks(texts["two_byte_lines"]), pc.span_masks(texts["two_byte_lines_shifted"])
    assert len(a) == len(b) > 2 * pc.SUB_BYTES // pc.SPAN          # more than two sweeps
    assert set(a) == {0xAAAAAAAAAAAAAAAA}
    assert b[0] == 0x5555555555555554 and set(b[1:]) == {0x5555555555555555}
    assert len(texts["two_byte_lines"]) % 64 == 0 and len(texts["two_byte_lines_shifted"]) % 64 == 1


def _pairs_by_split(text, swap):
    """expect_pairs once more, with bytes.split and a loop"""
    lines = text.split(b"\n")[:-1]
    pos, out, cap = 0, [], 0
    starts = []
    for l in lines:
        starts.append(pos); pos += len(l) + 1
    for i in range(len(lines) // 2):
        a, b = (starts[2 * i] + 1, len(lines[2 * i]) - 1), (starts[2 * i + 1] + 1, len(lines[2 * i + 1]) - 1)
        if swap and b[1] > a[1]:
            a, b = b, a
        out.append((a[0], a[1], b[0], b[1], cap)); cap += (a[1] + b[1] + 3) & ~3
    return np.array(out, np.int64).reshape(-1, 5), cap


@pytest.mark.parametrize("name", ["under_64", "end_63_past_even", "two_byte_lines_shifted", "one_line", "empty"])
@pytest.mark.parametrize("swap", [False, True])
def test_expected_pairs_agree_with_a_plain_split(name, swap):
    text = pc.nl_positions()[name]
    want, cap = _pairs_by_split(text, swap)
    got = pc.expect_pairs(text, swap)
    assert got["n"] == len(want) and got["cap_bytes"] == cap and len(got["cap_off"]) == got["n"] + 1
    for k, f in enumerate(("pat_off", "pat_len", "txt_off", "txt_len")):
        np.testing.assert_array_equal(got[f], want[:, k], err_msg=f)
    np.testing.assert_array_equal(got["cap_off"][:-1], want[:, 4])


# ------------------------------------------------------------------------------------------------ scan_carry
def test_scan_carry_takes_three_trips():
    text = pc.scan_carry()
    want = pc.expect_pairs(text, True)
    assert want["n"] == pc.SCAN_CARRY_PAIRS
    values = -(-want["n"] // 256)                                  # block sums handed to scan_i64
    assert -(-values // pc.SCAN_TRIP) >= 3
    assert values % pc.SCAN_TRIP not in (0, pc.SCAN_TRIP - 1) and want["n"] % 256 == 1       # a partial last trip, a last block of one pair
    slots = np.diff(want["cap_off"])
    assert set(np.unique(slots).tolist()) == {0, 4, 8}
    plain = pc.expect_pairs(text, False)
    swapped = plain["pat_len"] < plain["txt_len"]
    assert swapped.any() and (plain["pat_len"] > plain["txt_len"]).any() and (plain["pat_len"] == plain["txt_len"]).any()
    np.testing.assert_array_equal(want["pat_off"][swapped], plain["txt_off"][swapped])
    # the carry is worth more than a trip's own sum can hide: the offsets of the third trip lie beyond everything before it
    assert want["cap_off"][2 * pc.SCAN_TRIP * 256] > 2 * 4 * pc.SCAN_TRIP * 256 // 2
    # the newline scan of this text stays inside one trip (one value per 128 KB; 8192 of them would be a gigabyte of text)
    assert -(-len(text) // pc.BLOCK_BYTES) < pc.SCAN_TRIP and 25e6 < len(text) < 35e6


# ------------------------------------------------------------------------------------------------ bsw
def test_bsw_copy_counts_and_lengths():
    assert pc.BSW_COPY_COUNTS == (1, 2, 3, 5, 63, 64, 65, 255, 256, 257)
    assert {c % pc.COPY_UNROLL for c in pc.BSW_COPY_COUNTS} == {0, 1, 2, 3}                  # the duplicated last pair: 1, 2, 3 of 4 missing
    assert {(c - 1) // 64 for c in pc.BSW_COPY_COUNTS} == {0, 1, 3, 4}                        # one wave's batch, two, a whole workgroup, a second one
    assert {c - pc.CODES_WG_PAIRS for c in pc.BSW_COPY_COUNTS} >= {-1, 0, 1} and {c - 64 for c in pc.BSW_COPY_COUNTS} >= {-1, 0, 1}
    tails = set()
    for c in pc.BSW_COPY_COUNTS:
        text = pc.bsw_copy(c)
        want = pc.expect_bsw(text)
        assert want["n"] == c and text.endswith(b"\n") and text.count(b"\n") == 3 * c
        r = int(want["len2"][-1]) % 4
        assert r in (1, 2, 3)
        tails.add(r)
        q_start = len(text) - 1 - int(want["len2"][-1])
        assert (q_start + 4 * ((int(want["len2"][-1]) + 3) // 4) > len(text)) == (r in (1, 2))      # the last dword load crosses the end
    assert tails == {1, 2, 3}
    for c in (63, 257):
        want = pc.expect_bsw(pc.bsw_copy(c))
        l1, l2 = want["len1"].astype(int), want["len2"].astype(int)
        total, nR = pc.pair_dwords(l1, l2), (l1 + 3) // 4
        assert {2, 63, 64, 65, 128, 129, 576} <= set(total.tolist())
        assert set(total.tolist()) & {pc.COPY_TRIP_DWORDS - 1, pc.COPY_TRIP_DWORDS, pc.COPY_TRIP_DWORDS + 1, 2 * pc.COPY_TRIP_DWORDS, 2 * pc.COPY_TRIP_DWORDS + 1}
        i = int(np.argmax(total))
        assert (l1[i], l2[i]) == pc.BSW_MAX[1:] and total[i] == 576
        assert set((l1 % 4).tolist()) == set((l2 % 4).tolist()) == {0, 1, 2, 3}
        # where the query's first dword falls: in the first trip with more to come, in the second, in a later one
        assert ((nR < 64) & (total > 64)).any() and ((nR > 64) & (nR < 128) & (total > nR)).any() and (nR > 128).any()
        assert len(set(want["h0"].tolist())) > 20 and (want["h0"] < 0).any()
        assert set(want["ref"].tolist()) == set(want["qry"].tolist()) == set(range(10))


def test_bsw_bytes_hold_every_value_and_every_borrow():
    text = pc.bsw_bytes()
    lines = text.split(b"\n")[:-1]
    every = set(range(1, 256)) - {10}
    ref, qry = lines[1::3], lines[2::3]
    assert set(lines[1]) == every and set(b"".join(qry[:2])) == every and max(len(q) for q in qry) == pc.BSW_MAX[2]
    want = pc.expect_bsw(text)
    assert want["n"] == 6 and set(want["ref"].tolist()) == set(want["qry"].tolist()) == {(b - 48) & 255 for b in every}
    # a subtraction of the whole dword would differ from the bytewise one in each of the three places a borrow can reach, on both lines
    for side in (ref, qry):
        hit = set()
        for l in side[2:]:
            assert len(l) % 4 == 0
            for k in range(0, len(l), 4):
                w = int.from_bytes(l[k:k + 4], "little")
                naive = (w - 0x30303030) & 0xffffffff
                bytewise = int.from_bytes(bytes((b - 48) & 255 for b in l[k:k + 4]), "little")
                hit |= {j for j in range(4) if (naive ^ bytewise) >> (8 * j) & 255}
        assert hit == {1, 2, 3}
        for j in range(4):         # a byte below '0' at place j among bytes >= 0x80, and a byte >= 0x80 among bytes below '0'
            dw = [l[k:k + 4] for l in side[2:] for k in range(0, len(l), 4)]
            assert any(d[j] < 48 and all(d[k] >= 0x80 for k in range(4) if k != j) for d in dw)
            assert any(d[j] >= 0x80 and all(d[k] < 48 for k in range(4) if k != j) for d in dw)


def test_bsw_h0_by_the_c_library():
    assert [pc.sscanf_h0(h) for h in pc.BSW_H0_HEADERS] == [0, 0, 19, 42, -7, 0, 0, 12, 0, 99999999, -9999999, 8]
    assert max(len(h) for h in pc.BSW_H0_HEADERS) == pc.BSW_MAX[0]
    np.testing.assert_array_equal(pc.expect_bsw(pc.bsw_h0())["h0"], [0, 0, 19, 42, -7, 0, 0, 12, 0, 99999999, -9999999, 8])
    text, pair = pc.bsw_refusals()["header_9"]
    assert len(text.split(b"\n")[3 * pair]) == pc.BSW_MAX[0] + 1
    lens = {k: [len(l) for l in t.split(b"\n")[3 * p:3 * p + 3]] for k, (t, p) in pc.bsw_refusals().items()}
    assert lens["ref_2046"][1] == pc.BSW_MAX[1] + 1 and lens["qry_254"][2] == pc.BSW_MAX[2] + 1
    assert lens["ref_empty"][1] == 0 and lens["qry_empty"][2] == 0 and lens["two_bad_past_256"][1] == 0


# ------------------------------------------------------------------------------------------------ pairs_swap
def test_pairs_swap_cases():
    t = pc.pairs_swap()
    e = lambda k, s: pc.expect_pairs(t[k], s)
    assert e("equal", True)["pat_off"][0] == 1 and e("first_longer", True)["pat_off"][0] == 1
    assert e("second_longer_by_1", True)["pat_off"][0] == 6 and e("second_longer_by_1", False)["pat_off"][0] == 1
    assert e("empty_sequences", True)["pat_len"].tolist() == [0, 1, 1] and e("empty_sequences", False)["pat_len"].tolist() == [0, 0, 1]
    assert e("empty_sequences", True)["cap_off"].tolist() == [0, 0, 4, 8] and e("incomplete_pair", True)["n"] == 1
    for text, pair in pc.pairs_refusals().values():
        lines = text.split(b"\n")[:-1]
        assert min(i for i, l in enumerate(lines) if not l) // 2 == pair


# ------------------------------------------------------------------------------------------------ chain_edges
def test_chain_accepted_texts_and_their_edges():
    texts = pc.chain_accepted()
    want = {k: pc.expect_chain(t) for k, t in texts.items()}
    many = texts["many_calls"].split(b"\n")
    n = want["many_calls"].hdr["n"]
    assert want["many_calls"].ncalls > 256 and many[255] == b"EOR" and many[256].count(b"\t") == 5
    assert n[0] == 0 and n[-1] == 0 and (n[100:-1] == 0).any() and ((n[:-1] == 0) & (n[1:] == 0)).any() and want["many_calls"].nanchors > 400
    assert want["separators"].ncalls == 3 and want["separators"].x.tolist() == [1, 3, 5, 7, 9] and want["separators"].hdr["max_dist_y"].tolist() == [5000, 4000, 5000]
    assert want["u64_max"].x.max() == want["u64_max"].y.max() == np.uint64(2**64 - 1)
    assert [len(l) for l in texts["header_127"].split(b"\n") if len(l) > 100] == [pc.HDR_SLOT - 1]
    assert want["header_127"].hdr["bw"].tolist() == [500] * 3 and want["header_127"].hdr["max_dist_y"][1] == 4000
    for k in ("blank_after_last_eor", "blank_tail_without_newline"):
        assert want[k].ncalls == 1 and not texts[k].endswith(b"EOR\n") and not texts[k][len(pc.CHAIN_OK):].strip()
    assert want["only_blanks"].ncalls == 0


def test_chain_refusals_and_the_call_they_name():
    bad = pc.chain_refusals()
    assert [len(l) for l in bad["header_128"][0].split(b"\n") if len(l) > 100] == [pc.HDR_SLOT]
    assert b"18446744073709551616" in bad["u64_overflow"][0] and 18446744073709551616 == 2**64
    for k in ("EORX", "EO", "blank_EOR"):
        assert bad[k][0].count(b"\nEOR\n") == 2 and bad[k][1] == 1
    for k in pc.CHAIN_CALL_AFTER_LAST_EOR + ("text_after_last_eor", "text_without_newline"):
        text, call = bad[k]
        eor_lines = [i for i, l in enumerate(text.split(b"\n")[:-1]) if l == b"EOR"]
        rest = b"\n".join(text.split(b"\n")[eor_lines[-1] + 1:])
        assert call == len(eor_lines) and rest.strip()            # ignoring `rest` gives GAB_OK with `call` calls
    # the token reader takes an "EOR" without its newline as the end of a third call; by lines there are two
    assert pc.expect_chain(bad["last_eor_without_newline"][0]).ncalls == 3 == bad["last_eor_without_newline"][1] + 1
