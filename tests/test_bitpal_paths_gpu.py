"""GPU: every kernel of genarchbench_amd/csrc/bitpal.hip on the batches of tests/bitpal_cases.py -- each width of bitpal_edit_bv<D> across
its own word boundaries, the bit-vector kernel's rejects, the LDS and the global boundary column at the 2048-row switch, the SWAR byte
compare on all 256 values, the chunk and row-loop edges, a second trip of every grid-stride loop, and each limit.  Scores against the
oracle element for element (canaries behind them), gab_bitpal_last_paths / gab_bitpal_last_stats against the routing model; through
gab_bitpal_run and gab_bitpal_run_device, for -a bitpal-edit, the same under GAB_BITPAL_NO_BV=1, and -a bitpal-scored.
tests/test_bitpal_cases.py asserts on the CPU that every batch reaches the edge it is named for."""
import numpy as np
import pytest

from tests import bitpal_cases as bc

pytestmark = pytest.mark.gpu

MODES = {"edit": (bc.EDIT, False), "edit_no_bv": (bc.EDIT, True), "scored": (bc.SCORED, False)}
CANARY = -7777777              # no score: |score| <= 4 * 2 * GAB_BITPAL_MAX_LEN
TAIL = 64                      # canary elements behind the last score
SIDE_STREAM = ("switch_2048",)  # the device run of these goes on a stream of its own
EINVAL = -22


def make_engine(mode, monkeypatch):
    from genarchbench_amd.bitpal import BitpalEngine
    alg, no_bv = MODES[mode]
    if no_bv:
        monkeypatch.setenv("GAB_BITPAL_NO_BV", "1")
    else:
        monkeypatch.delenv("GAB_BITPAL_NO_BV", raising=False)
    return BitpalEngine(alg)


def run_host(e, b):
    """gab_bitpal_run -> (scores, the canaries behind them); raises GabError with the buffer in .out"""
    from genarchbench_amd._lib import GabError
    out = np.full(b.n + TAIL, CANARY, np.int32)
    try:
        e.benchmark_bitpal(b, out=out)
    except GabError as err:
        err.out = out
        raise
    return out[:b.n], out[b.n:]


def run_device(e, b, pat_bytes=None, txt_bytes=None, side_stream=False):
    """gab_bitpal_run_device on slabs of exactly pat_bytes / txt_bytes (default: the whole arrays)"""
    import torch
    from genarchbench_amd._lib import GabError
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.ascontiguousarray(a)).to(dev)
    pat = t(b.pat if pat_bytes is None else b.pat[:pat_bytes]); txt = t(b.txt if txt_bytes is None else b.txt[:txt_bytes])
    args = (pat, t(b.pat_off), t(b.pat_len), txt, t(b.txt_off), t(b.txt_len))
    sc = torch.full((b.n + TAIL,), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    try:
        e.run_device(*args, sc, stream=stream.cuda_stream)
    except GabError as err:
        torch.cuda.synchronize()
        err.out = sc.cpu().numpy()
        raise
    torch.cuda.synchronize()
    out = sc.cpu().numpy()
    return out[:b.n], out[b.n:]


def check_good(e, name, mode, device):
    """one run of BATCHES[name]: scores, canaries, paths, stats"""
    alg, no_bv = MODES[mode]
    b = bc.BATCHES[name]()
    want, r = bc.expected(name, alg), bc.route(b, alg, no_bv)
    if device:
        slabs = bc.exact_slabs()[1:] if name == "exact_slabs" else (None, None)
        got, tail = run_device(e, b, *slabs, side_stream=name in SIDE_STREAM)
    else:
        got, tail = run_host(e, b)
    paths, st = e.last_paths(), e.last_stats()
    print(f"\n{name} {mode} {'device' if device else 'host'}: {paths} cells={st['cells']} long_pairs={st['long_pairs']} "
          f"kernel_ms={st['kernel_ms']:.3f} total_ms={st['total_ms']:.3f}")
    np.testing.assert_array_equal(got, want)
    assert (tail == CANARY).all()
    assert paths == r.paths
    assert st["cells"] == r.cells and st["long_pairs"] == r.long_pairs


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(bc.BATCHES))
def test_batch(name, mode, monkeypatch):
    e = make_engine(mode, monkeypatch)
    try:
        check_good(e, name, mode, device=False)
        check_good(e, name, mode, device=True)
    finally:
        e.close()


def test_every_width_is_launched_and_the_second_trips_happen(monkeypatch):
    """what the names promise, read from last_paths alone"""
    e = make_engine("edit", monkeypatch)
    try:
        for D in range(1, 9):
            run_host(e, bc.width(D))
            p = e.last_paths()
            assert p["bv_words"] == D and p["bv_pairs"] == bc.width(D).n and p["lds_pairs"] == p["global_pairs"] == 0
        run_host(e, bc.global_second_trip())
        p = e.last_paths()
        assert p["global_pairs"] > 64 * p["global_blocks"] > 0
    finally:
        e.close()


def check_refused(e, r, device, message):
    """the call is refused with GAB_EINVAL and the message; no score is written; last_stats / last_paths are refused afterwards"""
    from genarchbench_amd._lib import GabError
    with pytest.raises(GabError) as ei:
        run_device(e, r.batch, r.pat_bytes, r.txt_bytes) if device else run_host(e, r.batch)
    assert ei.value.code == EINVAL and message in str(ei.value), str(ei.value)
    assert (ei.value.out == CANARY).all()
    for call in (e.last_stats, e.last_paths):
        with pytest.raises(GabError) as ei:
            call()
        assert ei.value.code == EINVAL and "no completed run" in str(ei.value)


@pytest.mark.parametrize("mode", ["edit", "scored"])
@pytest.mark.parametrize("name", ["pat_len_over", "txt_len_over", "pat_len_negative", "txt_len_negative", "pat_off_negative", "txt_off_negative",
                                  "pat_end_past_slab", "txt_end_past_slab", "two_bad"])
def test_refusal(name, mode, monkeypatch):
    from oracle import pyoracle
    r = bc.limits_refused()[name]
    e = make_engine(mode, monkeypatch)
    try:
        check_good(e, "chunk_edges", mode, device=True)              # (so that there are stats to refuse afterwards)
        check_refused(e, r, True, bc.refusal_message(r))
        check_good(e, "chunk_edges", mode, device=True)              # the same handle still works
        if r.host is None:                                           # gab_bitpal_run stages a window that holds every end: accepted
            got, tail = run_host(e, r.batch)
            np.testing.assert_array_equal(got, pyoracle.bitpal(r.batch, MODES[mode][0]))
            assert (tail == CANARY).all()
        else:
            check_refused(e, r, False, bc.refusal_message(r, host=True))
        check_good(e, "chunk_edges", mode, device=False)
    finally:
        e.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_refusal_of_a_pair_only_the_second_trip_sees(mode, monkeypatch):
    b = bc.classify_stride(True)
    r = bc.Refusal(b, (b.n - 1,), len(b.pat), len(b.txt), "scan")
    e = make_engine(mode, monkeypatch)
    try:
        check_refused(e, r, True, "1 pair(s) violate the limits (first: pair %d)" % (bc.CLASSIFY_STRIDE_PAIRS))
        check_good(e, "bytes_256", mode, device=True)
    finally:
        e.close()


def test_last_paths_needs_a_completed_run(monkeypatch):
    from genarchbench_amd._lib import GabError
    e = make_engine("scored", monkeypatch)
    try:
        with pytest.raises(GabError) as ei:
            e.last_paths()
        assert ei.value.code == EINVAL and "no completed run" in str(ei.value)
        check_good(e, "bytes_256", "scored", device=False)
        empty = bc.gabgen.pairs_from_lists([], [])
        run_host(e, empty)                                           # an empty batch is no run
        with pytest.raises(GabError):
            e.last_paths()
    finally:
        e.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_one_handle_across_large_small_refused_and_good_batches(mode, monkeypatch):
    e = make_engine(mode, monkeypatch)
    try:
        check_good(e, "global_second_trip", mode, device=False)      # large: the scratch and the lists at their biggest
        check_good(e, "bytes_256", mode, device=True)                # small
        check_refused(e, bc.limits_refused()["two_bad"], True, "2 pair(s) violate the limits (first: pair 2)")
        check_good(e, "bv_routes", mode, device=False)               # edit: with rejects
        check_refused(e, bc.limits_refused()["pat_len_negative"], False, "negative offset/length at pair 2")
        check_good(e, "switch_2048", mode, device=True)
        check_good(e, "width_3", mode, device=False)
        check_good(e, "global_second_trip", mode, device=True)
    finally:
        e.close()
