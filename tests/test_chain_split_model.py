"""CPU: tests.util.chain_split_model -- the batch-shape rule of gab_chain_run_device as chain.hip's comments word it -- on batches
worked out by hand.  tests/test_chain_forms_gpu.py holds the library against this model (gab_chain_last_split)."""
import numpy as np
import pytest

from tests.util import CHAIN_DISPATCH, chain_split_margins, chain_split_model

T, L, P, G = 3, 2, 1, 6          # table, latency, throughput (P: the plain block kernels), legacy-only launch


def model(n, mode, **env):
    return chain_split_model(n, mode, {k: str(v) for k, v in env.items()}).tolist()


@pytest.mark.parametrize("mode", [0, 1])
def test_equal_short_calls_stay_in_the_throughput_form(mode):
    # 2 000 x 80 = 160 000 anchors > 1 140 x 80 (0.30 us x n >= 0.75 x total / 2.85e9  <=>  total <= 1 140 n): nobody is waited for
    assert model([80] * 2000, mode) == [P] * 2000
    # 100 x 300: the batch does wait for its longest call, but no call reaches 2 048 (table form) or 512 (latency form)
    assert model([300] * 100, mode) == [P] * 100
    # ... and empty calls are nobody's
    assert model([0, 80, 0], mode) == [0, P, 0]
    assert model([], mode) == [] and model([0, 0], mode) == [0, 0]


@pytest.mark.parametrize("mode", [0, 1])
def test_one_long_call_among_short_ones(mode):
    """42 918 anchors, longest 30 000: waited for.  A quarter of the throughput time is 12 anchors' worth, so the 2 048 minimum decides
    the table form; what it leaves (5 370 anchors, longest 2 047) waits again: latency form from 512"""
    n = [300, 2047, 400, 30000, 511, 3000, 512, 2048, 600, 2500, 1000]
    assert model(n, mode) == [P, L, P, T, P, T, L, T, L, T, L]


def test_the_quarter_of_the_throughput_time():
    """60 000 + 3 000 x 5 000 + 1 000 x 7 000 = 22 060 000 anchors <= 1 140 x 60 000: waited for; a quarter of 22.06 M / 2.85 G/s is
    1.935 ms = 6 450 anchors at 0.30 us.  chain: min(6 450, 8 192): the 7 000s go to the table, the 5 000s stay -- 15 M anchors left,
    longest 5 000 < 15 M / 1 140: throughput form.  fast-chain: min(6 450, 4 096): everything in the table form"""
    n = [5000] * 3000 + [60000] + [7000] * 1000
    assert model(n, 0) == [P] * 3000 + [T] + [T] * 1000
    assert model(n, 1) == [T] * 4001
    # the same batch without the 7 000s: 15.06 M, a quarter is 4 403 anchors: now chain sends the 5 000s too
    assert model([5000] * 3000 + [60000], 0) == [T] * 3001


def test_standing_floors():
    """16 382 500 anchors, longest 8 192 < total / 1 140 = 14 370: nobody is waited for, only the floors apply -- fast-chain 4 096,
    chain 8 192.  chain leaves 12 286 500 anchors, longest 8 191 < 10 777: throughput form.  fast-chain leaves 1 000 x 4 095 =
    4 095 000, longest 4 095 >= 3 592: those are waited for -- latency form"""
    n = [4095] * 1000 + [8192] * 500 + [4096] * 1000 + [8191] * 500
    assert model(n, 0) == [P] * 1000 + [T] * 500 + [P] * 1500
    assert model(n, 1) == [L] * 1000 + [T] * 2000
    assert all(m < 0.9 for m in chain_split_margins(n, 0))
    assert chain_split_margins(n, 1)[1] > 1.1


def test_written_through_has_no_standing_floors():
    """gab_chain_run_device_through on page-locked arrays (through=True): the same 16 382 500 anchors stay in the throughput form, all of
    them, in both modes -- nobody is waited for and the floors do not apply; pageable arrays (through=False) keep them"""
    n = [4095] * 1000 + [8192] * 500 + [4096] * 1000 + [8191] * 500
    for mode in (0, 1):
        assert chain_split_model(n, mode, through=True).tolist() == [P] * 3000
        assert chain_split_model(n, mode, through=False).tolist() == model(n, mode) != [P] * 3000
        assert all(m < 0.9 for m in chain_split_margins(n, mode, through=True))
    # a batch that waits keeps the rule itself: a quarter of the throughput time, 2 048 anchors at least (22.06 M anchors: 6 450)
    n = [5000] * 3000 + [60000] + [7000] * 1000
    for mode in (0, 1):
        assert chain_split_model(n, mode, through=True).tolist() == [P] * 3000 + [T] + [T] * 1000
    # ... and the pins: GAB_CHAIN_TAB_MIN decides with or without floors
    assert chain_split_model([5000, 300], 1, {"GAB_CHAIN_TAB_MIN": "301", "GAB_CHAIN_FAST_CALLS": "0"}, through=True).tolist() == [T, P]


def test_extent_with_gaps_counts_as_anchors():
    """total: the arrays' extent where the calls do not lie back to back.  100 x 300 back to back waits for its longest call (30 000
    <= 1 140 x 300) and [300] x 100 + [600] sends the 600 to the latency form; spread over 1 000 000 elements nobody waits"""
    n = [300] * 100 + [600]
    assert model(n, 0) == [P] * 100 + [L]
    assert chain_split_model(n, 0, total=1_000_000).tolist() == [P] * 101
    assert chain_split_margins(n, 0, total=1_000_000)[0] == pytest.approx(1140 * 600 / 1_000_000)


@pytest.mark.parametrize("mode", [0, 1])
def test_through_route(mode):
    from tests.util import chain_through_route as route
    n, off = [500, 500, 500], None
    assert route(n, off, mode, {}, None) == 0 and route([], off, mode, {}, None) == 0
    assert route([], off, mode, {}, True) == route([0, 0], off, mode, {}, False) == 1
    assert route(n, off, mode, {}, False) == 2
    assert route(n, off, mode, {}, True) == 3                                   # 1 500 <= 326 x 500: seven helpers
    assert route([500] * 326, off, mode, {}, True) == 3 and route([500] * 327, off, mode, {}, True) == 1
    assert route(n, [0, 1000, 326 * 500 - 499], mode, {}, True) == 1            # the extent counts, gaps included: 163 001 > 163 000
    assert route(n, [0, 1000, 326 * 500 - 500], mode, {}, True) == 3
    assert route(n, off, mode, {"GAB_CHAIN_HELPERS": "3"}, True) == 1 and route(n, off, mode, {"GAB_CHAIN_HELPERS": "5"}, True) == 3
    assert route([500] * 327, off, mode, {"GAB_CHAIN_HELPERS": "7"}, True) == 3
    assert route([500] * 327, off, mode, {"GAB_CHAIN_KERNEL": "walk"}, True) == (3 if mode == 0 else 1)
    assert route([500] * 30 + [1500], off, mode, {}, True) == 3                # the latency form takes the 1 500
    tab = {"GAB_CHAIN_TAB_MIN": "1"}
    assert route(n, off, mode, tab, True) == route(n, off, mode, tab, True, [3, 3, 3]) == 1
    assert route(n, off, mode, tab, True, [3, 4, 3]) == route(n, off, mode, tab, True, [5, 3, 3]) == 4
    assert route(n, off, mode, tab, False, [3, 4, 3]) == 2


@pytest.mark.parametrize("mode", [0, 1])
def test_env_pins(mode):
    n = [300, 2047, 400, 30000, 511, 3000, 512, 2048, 600, 2500, 1000, 0]
    assert model(n, mode, **CHAIN_DISPATCH["table-form-for-all"]) == [T] * 11 + [0]
    assert model(n, mode, **CHAIN_DISPATCH["latency-form-for-all"]) == [L] * 11 + [0]
    assert model(n, mode, **CHAIN_DISPATCH["throughput-form-for-all"]) == [P] * 11 + [0]
    assert model(n, mode, **CHAIN_DISPATCH["default-split"]) == [P, L, P, T, P, T, L, T, L, T, L, 0]
    # GAB_CHAIN_TAB_MIN: the table form's smallest call; the rest (9 918 anchors, longest 2 500) waits: latency form from 512
    assert model(n, mode, GAB_CHAIN_TAB_MIN=3000) == [P, L, P, T, P, T, L, L, L, L, L, 0]
    # GAB_CHAIN_TAB=0: no table form; the whole batch waits for the 30 000
    assert model(n, mode, GAB_CHAIN_TAB=0) == [P, L, P, L, P, L, L, L, L, L, L, 0]
    assert model(n, mode, GAB_CHAIN_TAB=1) == model(n, mode)
    # GAB_CHAIN_FAST_MIN alone: every remaining call of that length; with GAB_CHAIN_FAST_CALLS: that many at most
    assert model(n, mode, GAB_CHAIN_FAST_MIN=1000) == [P, L, P, T, P, T, P, T, P, T, L, 0]
    assert model(n, mode, GAB_CHAIN_FAST_MIN=1, GAB_CHAIN_FAST_CALLS=3) == [P, L, P, T, P, T, P, T, L, T, L, 0]
    # GAB_CHAIN_FAST_CALLS alone: the rule's length (512 here) and that many calls
    assert model(n, mode, GAB_CHAIN_FAST_CALLS=2) == [P, L, P, T, P, T, P, T, P, T, L, 0]
    # ... and on a batch nobody waits in, the rule's length is none at all: the longest calls, however short
    assert model([80] * 2000, mode, GAB_CHAIN_FAST_CALLS=2) == [L, L] + [P] * 1998
    assert model([80] * 2000, mode, GAB_CHAIN_FAST_MIN=81) == [P] * 2000
    # the legacy-only launch
    for h in (3, 5, 7, 0):
        assert model(n, mode, GAB_CHAIN_HELPERS=h) == [G] * 11 + [0]
    assert model(n, mode, GAB_CHAIN_KERNEL="walk") == ([G] * 11 + [0] if mode == 0 else model(n, mode))
    assert model(n, mode, GAB_CHAIN_KERNEL="block") == model(n, mode)


def test_sorted_order_is_stable():
    """equal lengths keep the caller's order in the sorted list: with room for two calls in the latency form, the first two"""
    assert model([700, 700, 700, 700], 0, GAB_CHAIN_FAST_MIN=1, GAB_CHAIN_FAST_CALLS=2) == [L, L, P, P]
    assert model([700, 900, 700, 900], 0, GAB_CHAIN_FAST_MIN=1, GAB_CHAIN_FAST_CALLS=3) == [L, L, P, L]


def test_margins():
    np.testing.assert_allclose(chain_split_margins([80] * 2000, 0), [1140 * 80 / 160000] * 2, rtol=1e-12)
    m = chain_split_margins([30000, 300, 400], 0)
    assert m[0] > 100 and len(m) == 2
