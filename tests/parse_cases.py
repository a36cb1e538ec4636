"""Input parsers: constructed texts for tests/test_parse_edges_gpu.py and the arrays a line-by-line reader gives for them.

Plain Python and numpy: no GPU, no library.  The expected values come from cutting the bytes at every newline and applying the reference
drivers' rules to each line (bsw: main_banded.cpp:164-206, bpm / wfa: align_benchmark.c's getline loops); chain texts that
are accepted go through tools.gabgen.read_chain_text, the token reader.  tests/test_parse_cases.py proves that every case
reaches the edge it is named for, from the text and the constants below alone.

The constants of genarchbench_amd/csrc/parse.hip the cases are built around (test_parse_cases.py reads the named ones back
from the source, so a retune breaks that test rather than hollowing out these cases):"""
import ctypes as C
import functools
import os
import tempfile

import numpy as np

SPAN = 64                  # text bytes per thread and sweep in nl_count / nl_fill (parse.hip:36, 88: threadIdx.x * 64)
SUB_BYTES = 16384          # kSubBytes, one sweep of a workgroup (parse.hip:19)
SUBS = 8                   # kSubs, sweeps per workgroup (parse.hip:20)
BLOCK_BYTES = SUB_BYTES * SUBS
SCAN_PER = 8               # kPer (parse.hip:60) ...
SCAN_TRIP = 1024 * SCAN_PER            # ... values per trip of scan_i64 (parse.hip:63)
COPY_TRIP_DWORDS = 64      # dwords of a pair the first copy trip of bsw_codes takes, one per lane (parse.hip:230-231)
COPY_UNROLL = 4            # kCopyUnroll, pairs in flight per wave (parse.hip:200)
CODES_WG_PAIRS = 256       # pairs per bsw_codes workgroup and trip: 4 waves x 64 lanes (parse.hip:206-207)
HDR_SLOT = 128             # kHdrSlot, bytes per chain header line handed to the host, the NUL included (parse.hip:270)
BSW_MAX = (8, 2045, 253)   # longest header / reference / query line bsw_meta accepts (parse.hip:135)
EINVAL = -22               # GAB_EINVAL (include/gab.h)

_ACGT = np.frombuffer(b"ACGT", np.uint8)


# ------------------------------------------------------------------------------------------------ expected arrays
def lines_of(text):
    """(start, length) of every line that ends in a newline, int64 each"""
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10).astype(np.int64)
    start = np.concatenate([[0], nl[:-1] + 1]).astype(np.int64) if len(nl) else np.zeros(0, np.int64)
    return start, nl - start


def _excl(v):
    return np.concatenate([[0], np.cumsum(v, dtype=np.int64)]).astype(np.int64)


def expect_pairs(text, swap):
    """bpm / wfa: the first character of a line and its newline go; with `swap` a strictly longer second line comes first"""
    start, length = lines_of(text)
    n = len(start) // 2
    ao, al, bo, bl = start[0:2 * n:2] + 1, length[0:2 * n:2] - 1, start[1:2 * n:2] + 1, length[1:2 * n:2] - 1
    assert (al >= 0).all() and (bl >= 0).all(), "not an accepted text"
    sw = (bl > al) if swap else np.zeros(n, bool)
    pat_len, txt_len = np.where(sw, bl, al), np.where(sw, al, bl)
    cap = _excl((pat_len + txt_len + 3) & ~3)
    return {"n": n, "pat_off": np.where(sw, bo, ao), "txt_off": np.where(sw, ao, bo), "pat_len": pat_len.astype(np.int32),
            "txt_len": txt_len.astype(np.int32), "cap_off": cap, "cap_bytes": int(cap[-1])}


_libc = C.CDLL(None)


def sscanf_h0(header):
    """what loadPairs' fgets(temp, 10) + sscanf(temp, "%d", &h0) leaves in h0 (main_banded.cpp:168-171), by the C library itself"""
    v = C.c_int(0)
    _libc.sscanf(C.c_char_p((header + b"\n")[:9]), C.c_char_p(b"%d"), C.byref(v))
    return v.value


def gather(slab, off, length):
    """the bytes slab[off[i] : off[i] + length[i]] of every i, back to back"""
    length = np.asarray(length, np.int64)
    return np.asarray(slab)[np.repeat(np.asarray(off, np.int64) - _excl(length)[:-1], length) + np.arange(int(length.sum()), dtype=np.int64)]


def expect_bsw(text):
    """bsw: header / reference / query lines; code = byte - 48 in uint8; every sequence starts on the next multiple of 4"""
    start, length = lines_of(text)
    n = len(start) // 3
    buf = np.frombuffer(text, np.uint8)
    len1, len2 = length[1:3 * n:3], length[2:3 * n:3]
    h0 = np.array([sscanf_h0(text[start[3 * i]:start[3 * i] + length[3 * i]]) for i in range(n)], np.int32)
    return {"n": n, "len1": len1.astype(np.int32), "len2": len2.astype(np.int32), "h0": h0,
            "ref_off": _excl((len1 + 3) & ~3)[:-1], "qry_off": _excl((len2 + 3) & ~3)[:-1],
            "ref": (gather(buf, start[1:3 * n:3], len1) - 48) & 255, "qry": (gather(buf, start[2:3 * n:3], len2) - 48) & 255}


def expect_chain(text):
    """the token reader's ChainBatch of an accepted chain text"""
    from tools import gabgen
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "in.txt")
        with open(path, "wb") as f:
            f.write(text)
        return gabgen.read_chain_text(path)


# ------------------------------------------------------------------------------------------------ nl_positions
def _pairs_body(seed, goals):
    """'>' / '<' lines of seeded length (sequences of 0 .. 119 characters) with a newline on every byte of `goals`, the last on
    the largest; a line is stretched or cut by at most a few bytes to end on a goal"""
    rng = np.random.default_rng(seed)
    goals = sorted(goals)
    assert all(b - a >= 2 for a, b in zip(goals, goals[1:])) and goals[0] >= 1      # (an empty line is not pairs format)
    nls, start, gi = [], 0, 0
    while gi < len(goals):
        nl = start + 1 + int(rng.integers(0, 120))
        if nl > goals[gi] - 2:                       # the line after this one could no longer end on the goal
            nl = goals[gi]; gi += 1
        nls.append(nl); start = nl + 1
    nls = np.array(nls, np.int64)
    buf = _ACGT[rng.integers(0, 4, int(nls[-1]) + 1)]
    starts = np.concatenate([[0], nls[:-1] + 1])
    buf[starts[0::2]] = ord(">"); buf[starts[1::2]] = ord("<"); buf[nls] = 10
    return buf.tobytes()


_NL_END = 4700 * SPAN              # ~300 KB: two whole 128 KB blocks and 38 KB (sweeps 0 .. 2) of a third
_NL_LAST = (SUB_BYTES - 1, BLOCK_BYTES - 1, 2 * BLOCK_BYTES - 1)       # last byte of a sweep, of a block, of the next block
_NL_FIRST = (SUB_BYTES, BLOCK_BYTES, 2 * BLOCK_BYTES)                  # first byte of the next sweep / block (two texts: byte b and b + 1
#                                                                        both '\n' would be an empty line)


@functools.lru_cache(maxsize=None)
def nl_positions():
    """name -> pairs-format text.  The four long texts differ in where they end relative to a 64-byte span: on it, 1 byte and
    63 bytes past it (twice: newlines on the even bytes of the last span, then on the odd ones)"""
    two = lambda k, first=0: b"".join(b"><"[(first + i) % 2:(first + i) % 2 + 1] + b"\n" for i in range(k))
    t = {}
    t["end_on_span"] = _pairs_body(101, _NL_LAST + (_NL_END - 1,))
    t["end_1_past"] = _pairs_body(102, _NL_FIRST + (_NL_END,))
    t["end_63_past_even"] = _pairs_body(103, _NL_LAST + (_NL_END - 2,)) + b">\n" + two(31, 1)
    t["end_63_past_odd"] = _pairs_body(104, _NL_FIRST + (_NL_END - 1,)) + two(31) + b">"
    t["under_64"] = b">ACGT\n<ACG\n>A\n<\n>\n<TTTTTTTT\n"
    t["two_byte_lines"] = two((2 * SUB_BYTES + 3 * SPAN) // 2)                      # newline masks 0xAAAA...
    t["two_byte_lines_shifted"] = b">A\n" + two((2 * SUB_BYTES + 3 * SPAN) // 2 - 1, 1)      # 0x5555... (byte 0 is no newline)
    t["no_newline"] = b">ACGTACGT"
    t["one_line"] = b">ACGTACGT\n"
    t["empty"] = b""
    return t


def nl_residues(text):
    """(residues mod 64 of the newlines in spans read as four uint4, residues of those in the last span, read byte by byte)"""
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    whole = nl // SPAN * SPAN + SPAN <= len(text)
    return set((nl[whole] % SPAN).tolist()), set((nl[~whole] % SPAN).tolist())


def span_masks(text):
    """the newlines of every whole 64-byte span as a 64-bit mask, bit b = byte b"""
    buf = np.frombuffer(text, np.uint8)[:len(text) // SPAN * SPAN].reshape(-1, SPAN)
    return [sum(1 << int(b) for b in np.flatnonzero(row == 10)) for row in buf]


# ------------------------------------------------------------------------------------------------ scan_carry
SCAN_CARRY_PAIRS = 2 * SCAN_TRIP * 256 + 257       # len_block_sums gives one value per 256 pairs: three trips of scan_i64


@functools.lru_cache(maxsize=None)
def scan_carry():
    """pairs-format text of SCAN_CARRY_PAIRS pairs, ~29 MB: sequence lengths i % 4 and i / 4 % 4, so a pair's output room is
    0, 4 or 8 bytes and both orders of "longer" occur"""
    i = np.arange(SCAN_CARRY_PAIRS, dtype=np.int64)
    seq = np.stack([i % 4, i // 4 % 4], 1).reshape(-1)             # per line
    nl = np.cumsum(seq + 2) - 1
    start = nl - seq - 1
    buf = np.repeat(_ACGT[np.arange(len(seq)) % 4], seq + 2)       # (every line one letter; the first and last byte are replaced)
    buf[start[0::2]] = ord(">"); buf[start[1::2]] = ord("<"); buf[nl] = 10
    return buf.tobytes()


# ------------------------------------------------------------------------------------------------ bsw
BSW_COPY_COUNTS = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257)
# (len1, len2) by the dwords of the pair, reference + query; both lines >= 1 character, so 2 is the least (a pair of ONE dword would
# have an empty line: refused, bsw_refusals).  Lengths 1, 2, 3 (and 0) mod 4 on both lines.
BSW_COPY_LENGTHS = {2: [(1, 1), (2, 2), (3, 3), (4, 4), (2, 1), (3, 2), (1, 3)],
                    63: [(125, 122), (126, 123), (127, 121), (128, 124)],
                    64: [(129, 123), (130, 121), (131, 122), (4, 249), (249, 4)],
                    65: [(157, 98), (158, 99), (159, 97), (1, 253), (253, 3)],
                    89: [(100, 253)],                           # the query starts in the first trip and ends in the second
                    128: [(397, 110), (398, 111), (399, 109), (258, 250)],
                    129: [(258, 253), (401, 111), (403, 109), (513, 2)],
                    576: [(2045, 253)]}


def pair_dwords(len1, len2):
    return (np.asarray(len1) + 3) // 4 + (np.asarray(len2) + 3) // 4


@functools.lru_cache(maxsize=None)
def _bsw_copy_lines():
    rng = np.random.default_rng(105)
    special = [p for v in BSW_COPY_LENGTHS.values() for p in v]      # pairs 0 .. 4 (the cuts at 1, 2, 3, 5): len2 = 1, 2, 3, 0, 1
    assert len(special) < 62
    lens = special[:5] + [(int(rng.integers(1, 300)), int(rng.integers(1, 254))) for _ in range(5, 257)]      # seeded lengths ...
    lens[5:len(special)] = special[5:]                                # ... behind the chosen ones
    for k, c in enumerate(BSW_COPY_COUNTS):            # the last pair of every later cut: len2 = 1, 2, 3 mod 4 in turn
        l1, l2 = lens[c - 1]
        if c > 5:
            lens[c - 1] = (l1, min(l2 - l2 % 4 + 1 + k % 3, 253))
    out = []
    for l1, l2 in lens:
        out += [b"%d" % rng.integers(-99, 100), (48 + rng.integers(0, 10, l1)).astype(np.uint8).tobytes(),
                (48 + rng.integers(0, 10, l2)).astype(np.uint8).tobytes()]
    return out


def bsw_copy(count):
    """the first `count` pairs of one 257-pair text; it ends at the newline of the last pair's query"""
    return b"".join(l + b"\n" for l in _bsw_copy_lines()[:3 * count])


def bsw_bytes():
    """every byte value but 0 and '\\n' on both lines (the query line holds 253 characters at most, so it takes two pairs), then
    a byte below '0' beside bytes of 0x80 and above, and the other way round, at each of the four places of a dword"""
    every = bytes(b for b in range(1, 256) if b != 10)
    lines = [b"1", every, every[::-1][:253], b"2", every[::-1], every[:253]]
    for j in range(4):
        at = lambda base, v: bytes(v if k == j else base for k in range(4))
        a, b, c = at(0xff, 0x2f), at(0x2f, 0x80), at(0x01, 0xb0)
        lines += [b"%d" % j, a + b + c, c + a + b]
    return b"".join(l + b"\n" for l in lines)


BSW_H0_HEADERS = (b"", b"0", b"19", b" +42", b"\t-7", b"-", b"+", b"12x", b"x12", b"99999999", b"-9999999", b"00000008")


def bsw_h0():
    return b"".join(h + b"\n0123\n012\n" for h in BSW_H0_HEADERS)


def bsw_refusals():
    """name -> (text, first refused pair)"""
    ok = b"19\n0123\n012\n"
    return {"header_9": (ok + b"123456789\n01\n01\n", 1),
            "ref_2046": (b"1\n" + b"0" * 2046 + b"\n01\n", 0),
            "qry_254": (ok * 2 + b"1\n01\n" + b"1" * 254 + b"\n", 2),
            "ref_empty": (ok + b"19\n\n012\n", 1),
            "qry_empty": (b"19\n0123\n\n" + ok, 0),
            "two_bad_past_256": (ok * 300 + b"19\n\n012\n" + ok * 400 + b"19\n0123\n\n", 300)}


# ------------------------------------------------------------------------------------------------ pairs_swap
def pairs_swap():
    """name -> accepted text: parsed with and without swap_longer_first"""
    return {"equal": b">ACGT\n<TTTT\n", "second_longer_by_1": b">ACG\n<TTTT\n", "first_longer": b">ACGTA\n<TTTT\n",
            "empty_sequences": b">\n<\n>\n<A\n>A\n<\n", "incomplete_pair": b">AC\n<ACG\n>A\n"}


def pairs_refusals():
    """name -> (text, first refused pair): a blank line has not even the prefix character"""
    ok = b">AC\n<ACG\n"
    return {"blank_first": (ok + b"\n<G\n" + ok, 1), "blank_second": (b">A\n\n" + ok, 0),
            "two_bad_past_256": (ok * 300 + b">A\n\n" + ok * 400 + b"\n<A\n", 300)}


# ------------------------------------------------------------------------------------------------ chain_edges
def _call(anchors, sep=b"\t", hdr=None):
    n = len(anchors)
    h = hdr if hdr is not None else b"%d\t15.000000\t5000\t5000\t500\t1" % n
    return b"".join([h + b"\n"] + [b"%d" % x + sep + b"%d" % y + b"\n" for x, y in anchors] + [b"EOR\n"])


def _many_calls():
    """more than 256 calls (two workgroups of chain_headers); line 255 is an "EOR" line and line 256 a header (two workgroups of
    the per-line kernels); calls of 0 anchors first, in the middle and last"""
    rng = np.random.default_rng(106)
    A = lambda n: [(int(a), int(b)) for a, b in rng.integers(0, 1 << 62, (n, 2))]
    calls = [_call([]), _call(A(252))]                       # lines 0-1, lines 2-255
    calls += [_call(A(int(n))) for n in rng.integers(0, 4, 150)] + [_call([]), _call([])] + [_call(A(int(n))) for n in rng.integers(1, 4, 150)] + [_call([])]
    return b"".join(calls)


_HDR127 = b"1" + b" " * (127 - len(b"1\t15.5\t5000\t4000\t500\t2")) + b"\t15.5\t5000\t4000\t500\t2"
CHAIN_OK = _call([(10, 20), (30, 40)])


def chain_accepted():
    """name -> text the parser takes; the token reader gives the expected arrays"""
    return {"many_calls": _many_calls(),
            "separators": _call([(1, 2), (3, 4)], b" \t ") + b"2  15.5 5000\t\t4000 500 2\r\n  5   6  \n7\t8\r\nEOR\n" + _call([(9, 10)], b"    "),
            "u64_max": _call([(18446744073709551615, 0), (0, 18446744073709551615), (18446744073709551610, 18446744073709551609)]),
            "header_127": CHAIN_OK + _call([(5, 6)], hdr=_HDR127) + CHAIN_OK,
            "blank_after_last_eor": CHAIN_OK + b"  \n\t\n \r\n\n",
            "blank_tail_without_newline": CHAIN_OK + b"\n \t ",
            "only_blanks": b" \t \r"}


def chain_refusals():
    """name -> (text, the call the message names)"""
    c3 = lambda mid: CHAIN_OK + mid + CHAIN_OK
    return {"u64_overflow": (c3(b"1\t15.0\t5000\t5000\t500\t1\n18446744073709551616\t20\nEOR\n"), 1),
            "header_128": (c3(_call([(5, 6)], hdr=b"1 " + _HDR127[1:])), 1),
            # ... as the last call, with more anchor lines than all other calls have anchors: a refused header counts no anchors
            "header_128_last": (CHAIN_OK + _call([(k, k) for k in range(6)], hdr=b"6 " + _HDR127[1:]), 1),
            "EORX": (c3(b"1\t15.0\t5000\t5000\t500\t1\n1\t2\nEORX\n"), 1),
            "EO": (c3(b"1\t15.0\t5000\t5000\t500\t1\n1\t2\nEO\n"), 1),
            "blank_EOR": (c3(b"1\t15.0\t5000\t5000\t500\t1\n1\t2\n EOR\n"), 1),
            "no_eor_at_all": (CHAIN_OK[:-4], 0),
            "no_newline_at_all": (b"EOR", 0),
            # after the last "EOR" line: each of these is GAB_OK with one call too few (or none) when the trailing lines are ignored
            "call_without_eor": (CHAIN_OK + CHAIN_OK[:-4], 1),
            "header_only": (CHAIN_OK * 2 + b"0\t15.0\t5000\t5000\t500\t1\n", 2),
            "text_after_last_eor": (CHAIN_OK + b"# end of file\n", 1),
            "text_without_newline": (CHAIN_OK + b"x", 1),
            "last_eor_without_newline": (CHAIN_OK * 2 + CHAIN_OK[:-1], 2),
            "blank_then_call_without_eor": (CHAIN_OK + b"\n\n" + CHAIN_OK[:-4], 1)}


# refusals whose text holds a further call after the last "EOR" LINE (read_call fills a call_t from each: it is token based)
CHAIN_CALL_AFTER_LAST_EOR = ("call_without_eor", "header_only", "last_eor_without_newline", "blank_then_call_without_eor")
