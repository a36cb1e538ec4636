"""GPU parity: the input parsers (genarchbench_amd/csrc/parse.hip) on the constructed texts of tests/parse_cases.py -- every block,
sweep, span and lane edge of the newline index, the carry of the single-workgroup scan, every trip and tail of the bsw copy,
the limits of each format from both sides -- against the arrays a line-by-line reader gives, element for element.
tests/test_parse_cases.py proves (without a GPU) that each text reaches the edge it is named for."""
import re
import time

import numpy as np
import pytest

from tests import parse_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ps():
    from genarchbench_amd.parse import InputParser
    p = InputParser()
    yield p
    p.close()


def _same_pairs(ps, pk, want):
    assert pk.n == want["n"] and pk.cap_bytes == want["cap_bytes"]
    if pk.n == 0:
        return None
    got = ps.pairs_to_host(pk)
    for f in ("pat_off", "txt_off", "pat_len", "txt_len", "cap_off"):
        assert got[f].dtype == want[f].dtype
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    assert got["cap_off"][-1] == pk.cap_bytes
    return got


def _same_bsw(ps, pk, want):
    assert pk.n == want["n"]
    got = ps.bsw_to_host(pk)
    for f in ("len1", "len2", "h0", "ref_off", "qry_off"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    assert pk.ref_bytes >= int(want["ref_off"][-1]) + ((int(want["len1"][-1]) + 3) & ~3) and pk.qry_bytes >= int(want["qry_off"][-1]) + ((int(want["len2"][-1]) + 3) & ~3)
    # EVERY pair's bytes
    np.testing.assert_array_equal(pc.gather(got["ref"], got["ref_off"], got["len1"]), want["ref"])
    np.testing.assert_array_equal(pc.gather(got["qry"], got["qry_off"], got["len2"]), want["qry"])
    return got


def _same_chain(ps, pk, want):
    assert pk.ncalls == want.ncalls and pk.total == want.nanchors
    if pk.ncalls == 0:
        return
    got = ps.chain_to_host(pk)
    np.testing.assert_array_equal(got["call_off"], np.concatenate([want.call_off, [want.nanchors]]))
    for f in ("n", "avg_qspan", "max_dist_x", "max_dist_y", "bw", "n_segs"):
        np.testing.assert_array_equal(got["hdr"][f], want.hdr[f], err_msg=f)
    np.testing.assert_array_equal(got["x"], want.x); np.testing.assert_array_equal(got["y"], want.y)


def _refused(call, word, index):
    """GAB_EINVAL, and the message names pair / call `index`"""
    from genarchbench_amd._lib import GabError
    with pytest.raises(GabError) as e:
        call()
    assert e.value.code == pc.EINVAL
    assert re.search(r"\b%s %d\b" % (word, index), str(e.value)), str(e.value)


def _on_device(text, shift=0):
    """(tensor that owns the bytes, device address of the text): 16-byte aligned, `shift` bytes past that when asked"""
    import torch
    t = torch.zeros(len(text) + 16, dtype=torch.uint8, device="cuda:0")
    if text:
        t[shift:shift + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift


# ------------------------------------------------------------------------------------------------ newline index
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("name", list(pc.nl_positions()))
def test_nl_positions(ps, name, swap):
    """newlines on every bit of a thread's 64-byte mask in both read paths, on the last byte of a sweep and of a block and on the
    first of the next, texts ending 0, 1 and 63 bytes past a span, shorter than a span, without a newline, empty"""
    text = pc.nl_positions()[name]
    _same_pairs(ps, ps.pairs(text, swap), pc.expect_pairs(text, swap))


@pytest.mark.parametrize("name", list(pc.nl_positions()))
def test_nl_positions_device_entry(ps, name):
    """gab_pairs_parse_device on a tensor gives what gab_pairs_parse gives on host bytes (the tensor ends with the text: the last
    span has nothing behind it)"""
    import torch
    from genarchbench_amd.parse import InputParser
    text = pc.nl_positions()[name]
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0") if text else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    pk = ps.pairs_device(t.data_ptr(), len(text), True)
    got = _same_pairs(ps, pk, pc.expect_pairs(text, True))
    if len(text):
        assert pk.d_text == t.data_ptr() and pk.text_bytes == len(text)
    other = InputParser()
    host = other.pairs(text, True)
    if got is not None:
        for f, v in other.pairs_to_host(host).items():
            np.testing.assert_array_equal(got[f], v, err_msg=f)
    assert (host.n, host.cap_bytes) == (pk.n, pk.cap_bytes)
    other.close()


def test_scan_carry(ps):
    """4 194 561 pairs: 16 386 block sums, three trips of scan_i64 with its running total carried from trip to trip -- every
    offset of the room per pair (d_cap_off, cap_bytes: what the wfa driver allocates from) and every sequence offset and length.
    The newline index uses the same kernel on one count per 128 KB of text: it would take a gigabyte of text to give THAT scan a
    second trip, so the carry is covered through this case alone."""
    text = pc.scan_carry()
    want = pc.expect_pairs(text, True)
    t0 = time.perf_counter()
    pk = ps.pairs(text, True)
    t1 = time.perf_counter()
    _same_pairs(ps, pk, want)
    print(f"scan_carry: {want['n']} pairs, {len(text)} bytes: parse {t1 - t0:.3f} s, parse + copy back + compare {time.perf_counter() - t0:.3f} s,"
          f" kernels {ps.last_stats()['kernel_ms']:.3f} ms")


# ------------------------------------------------------------------------------------------------ bsw
@pytest.mark.parametrize("count", pc.BSW_COPY_COUNTS)
def test_bsw_copy(ps, count):
    """pair counts around a wave's batch of 64, the 4 pairs in flight and a workgroup's 256; pairs of 2 .. 576 dwords (2045 + 253
    characters, the longest accepted) around the 64 dwords of the first copy trip; the last query ends the text"""
    text = pc.bsw_copy(count)
    _same_bsw(ps, ps.bsw_pairs(text), pc.expect_bsw(text))


@pytest.mark.parametrize("count", pc.BSW_COPY_COUNTS)
def test_bsw_copy_device_entry(ps, count):
    """gab_bsw_parse_pairs_device on a tensor that ends with the text: the last dword load has to stop at the text's end"""
    import torch
    from genarchbench_amd.parse import InputParser
    text = pc.bsw_copy(count)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    got = _same_bsw(ps, ps.bsw_pairs_device(t.data_ptr(), len(text)), pc.expect_bsw(text))
    other = InputParser()
    host = other.bsw_to_host(other.bsw_pairs(text))
    for f in ("len1", "len2", "h0", "ref_off", "qry_off"):
        np.testing.assert_array_equal(got[f], host[f], err_msg=f)
    for s, o, l in (("ref", "ref_off", "len1"), ("qry", "qry_off", "len2")):
        np.testing.assert_array_equal(pc.gather(got[s], got[o], got[l]), pc.gather(host[s], host[o], host[l]))
    other.close()


def test_bsw_bytes(ps):
    """every byte value a line can hold, and the borrow / high-bit cases of the four-bytes-at-once subtraction of '0'"""
    text = pc.bsw_bytes()
    _same_bsw(ps, ps.bsw_pairs(text), pc.expect_bsw(text))


def test_bsw_h0(ps):
    text = pc.bsw_h0()
    _same_bsw(ps, ps.bsw_pairs(text), pc.expect_bsw(text))


@pytest.mark.parametrize("name", list(pc.bsw_refusals()))
def test_bsw_refusals(ps, name):
    text, pair = pc.bsw_refusals()[name]
    _refused(lambda: ps.bsw_pairs(text), "pair", pair)


# ------------------------------------------------------------------------------------------------ pairs
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("name", list(pc.pairs_swap()))
def test_pairs_swap(ps, name, swap):
    text = pc.pairs_swap()[name]
    got = _same_pairs(ps, ps.pairs(text, swap), pc.expect_pairs(text, swap))
    if not swap:
        assert got["pat_off"][0] == 1                 # never swapped: the '>' line is the pattern


@pytest.mark.parametrize("name", list(pc.pairs_refusals()))
def test_pairs_refusals(ps, name):
    text, pair = pc.pairs_refusals()[name]
    for swap in (False, True):
        _refused(lambda: ps.pairs(text, swap), "pair", pair)


# ------------------------------------------------------------------------------------------------ chain
@pytest.mark.parametrize("name", list(pc.chain_accepted()))
def test_chain_edges(ps, name):
    text = pc.chain_accepted()[name]
    _same_chain(ps, ps.chain(text), pc.expect_chain(text))


@pytest.mark.parametrize("name", list(pc.chain_refusals()))
def test_chain_refusals(ps, name):
    """among them: content after the last "EOR" line (a further call without its "EOR" line, an "EOR" without its newline, any
    text), which used to be dropped with GAB_OK"""
    text, call = pc.chain_refusals()[name]
    _refused(lambda: ps.chain(text), "call", call)
    _same_chain(ps, ps.chain(pc.CHAIN_OK), pc.expect_chain(pc.CHAIN_OK))       # the handle is as good as before


def test_chain_device_entry(ps):
    text = pc.chain_accepted()["many_calls"]
    t, addr = _on_device(text)
    _same_chain(ps, ps.chain_device(addr, len(text)), pc.expect_chain(text))
    text, call = pc.chain_refusals()["last_eor_without_newline"]
    t, addr = _on_device(text)
    _refused(lambda: ps.chain_device(addr, len(text)), "call", call)


# ------------------------------------------------------------------------------------------------ device entry points, handle
def test_device_entries_refuse_a_text_that_is_not_16_byte_aligned(ps):
    from genarchbench_amd._lib import GabError
    texts = {"bsw": pc.bsw_copy(3), "pairs": pc.pairs_swap()["equal"], "chain": pc.CHAIN_OK}
    calls = {"bsw": lambda a, n: ps.bsw_pairs_device(a, n), "pairs": lambda a, n: ps.pairs_device(a, n, True), "chain": lambda a, n: ps.chain_device(a, n)}
    for k, text in texts.items():
        t, addr = _on_device(text, shift=1)
        assert addr % 16 == 1
        with pytest.raises(GabError) as e:
            calls[k](addr, len(text))
        assert e.value.code == pc.EINVAL and "16-byte aligned" in str(e.value)
        with pytest.raises(GabError):
            ps.last_stats()
        t, addr = _on_device(text)                    # the same bytes, aligned
        assert calls[k](addr, len(text)).__class__.__name__.endswith("Packed") and ps.last_stats()["kernel_ms"] > 0


def test_one_handle_large_small_refused_good(ps):
    """stale buffers, the reset of the refusal flags and of last_stats: a 29 MB text, a 3-line one, a refused one, then bsw_copy --
    which must come out as from a fresh handle"""
    from genarchbench_amd._lib import GabError
    from genarchbench_amd.parse import InputParser
    big = pc.scan_carry()
    _same_pairs(ps, ps.pairs(big, True), pc.expect_pairs(big, True))
    assert ps.last_stats()["kernel_ms"] > 0
    small = b"-5\n0123\n321\n"
    got = _same_bsw(ps, ps.bsw_pairs(small), pc.expect_bsw(small))
    assert got["h0"].tolist() == [-5] and got["ref"][:4].tolist() == [0, 1, 2, 3] and got["qry"][:3].tolist() == [3, 2, 1]
    assert ps.last_stats()["kernel_ms"] > 0
    text, pair = pc.bsw_refusals()["header_9"]
    _refused(lambda: ps.bsw_pairs(text), "pair", pair)
    with pytest.raises(GabError) as e:
        ps.last_stats()
    assert e.value.code == pc.EINVAL
    text = pc.bsw_copy(257)
    got = _same_bsw(ps, ps.bsw_pairs(text), pc.expect_bsw(text))
    assert ps.last_stats()["kernel_ms"] > 0
    fresh = InputParser()
    new = fresh.bsw_to_host(fresh.bsw_pairs(text))
    for f in ("len1", "len2", "h0", "ref_off", "qry_off"):
        np.testing.assert_array_equal(got[f], new[f], err_msg=f)
    for s, o, l in (("ref", "ref_off", "len1"), ("qry", "qry_off", "len2")):
        np.testing.assert_array_equal(pc.gather(got[s], got[o], got[l]), pc.gather(new[s], new[o], new[l]))
    fresh.close()
    # ... and the other two formats after it, a refusal between them
    text = pc.chain_accepted()["many_calls"]
    _same_chain(ps, ps.chain(text), pc.expect_chain(text))
    bad, pair = pc.pairs_refusals()["two_bad_past_256"]
    _refused(lambda: ps.pairs(bad, True), "pair", pair)
    text = pc.nl_positions()["end_63_past_odd"]
    _same_pairs(ps, ps.pairs(text, False), pc.expect_pairs(text, False))
