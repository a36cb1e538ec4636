"""CPU: the bpm oracle (oracle/bpm.c) against golden vectors from the compiled reference."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import BPM_STAGES, BPM_TRIP_EDGE_TLEN, GOLDEN, bpm_handmade_pairs, bpm_model, bpm_model_batch, bpm_trip_edge_pairs, read_scores


def lev(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


@pytest.mark.parametrize("name", ["bpm_bench", "bpm_adv"])
def test_oracle_matches_golden(name):
    batch = gabgen.read_pairs_text(f"{GOLDEN}/{name}.in.txt").swapped_longer_first()
    want = read_scores(f"{GOLDEN}/{name}.expected.txt")
    np.testing.assert_array_equal(pyoracle.bpm(batch), want)


def test_adv_fixture_contains_non_levenshtein_cases():
    """the N-aliasing / raw-compare quirks must be exercised: some printed scores differ from -Levenshtein"""
    batch = gabgen.read_pairs_text(f"{GOLDEN}/bpm_adv.in.txt").swapped_longer_first()
    want = read_scores(f"{GOLDEN}/bpm_adv.expected.txt")
    diff = clean_ok = 0
    for i in range(0, batch.n, 5):
        p, t = batch.pair(i)
        d = -lev(p, t)
        if set(p + t) <= set(b"ACGT"):
            assert want[i] == d          # clean pairs: exactly the edit distance
            clean_ok += 1
        elif want[i] != d:
            diff += 1
    assert diff > 5 and clean_ok > 5


def test_edge_cases():
    b = gabgen.pairs_from_lists([b"A", b"ACGT", b"NNNN", b"acgt", b"A" * 64, b"A" * 65, b"ACGTN" * 30],
                                [b"", b"ACGT", b"NNNN", b"ACGT", b"A" * 64, b"A" * 64, b"ACGTN" * 29])
    s = pyoracle.bpm(b)
    assert s[0] == -1 and s[1] == 0 and s[2] == 0 and s[3] == -4 and s[4] == 0 and s[5] == -1


# ---------------------------------------------------------------- the CPU model of the GPU cascade (tests/util.py: bpm_model)
@pytest.mark.parametrize("name", ["bpm_bench", "bpm_adv"])
def test_cascade_model_matches_golden(name):
    batch = gabgen.read_pairs_text(f"{GOLDEN}/{name}.in.txt").swapped_longer_first()
    np.testing.assert_array_equal(bpm_model_batch(batch)[0], read_scores(f"{GOLDEN}/{name}.expected.txt"))


@pytest.mark.parametrize("seed,n,mode,plen", [(71, 400, 0, 151), (72, 400, 1, 256), (73, 300, 1, 300), (74, 300, 0, 30),
                                              (75, 300, 1, 64), (76, 200, 0, 250)])
def test_cascade_model_matches_oracle(seed, n, mode, plen):
    batch = gabgen.pairs(seed, n, mode, plen).swapped_longer_first()
    want, steps = pyoracle.bpm(batch, want_steps=True)
    got, stages, model_steps = bpm_model_batch(batch)
    np.testing.assert_array_equal(got, want)
    # each stage a pair passes through steps it once more (tlen x W); the oracle steps every pair once
    assert model_steps >= steps and (model_steps == steps) == all(s in ("score", "generic") for s in stages)


def test_cascade_model_pattern_lengths_1_to_300():
    rng = np.random.default_rng(77)
    pats, txts = [], []
    for n in range(1, 301):
        p = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes())
        t = bytearray(p[: n - int(rng.integers(0, min(n, 12)))])
        for k in rng.integers(0, max(1, len(t)), len(t) // 20):
            t[k] = b"ACGTNa"[int(rng.integers(0, 6))]
        if n % 3 == 0:
            p[int(rng.integers(0, n))] = ord(b"N")
        pats.append(bytes(p)); txts.append(bytes(t))
    b = gabgen.pairs_from_lists(pats, txts)
    np.testing.assert_array_equal(bpm_model_batch(b)[0], pyoracle.bpm(b))


def test_cascade_model_clean_pairs_are_levenshtein():
    """what the score stage rests on: for upper-case ACGT pairs the printed score is -(edit distance)"""
    rng = np.random.default_rng(78)
    for _ in range(120):
        n = int(rng.integers(1, 200))
        p = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
        t = bytearray(p[: n - int(rng.integers(0, min(n, 20)))])
        for k in rng.integers(0, max(1, len(t)), len(t) // 8):
            t[k] = b"ACGT"[int(rng.integers(0, 4))]
        score, stage, _ = bpm_model(p, bytes(t))
        assert stage == "score" and score == -lev(p, bytes(t))


def test_cascade_model_handmade_pairs_land_where_built():
    pairs = bpm_handmade_pairs()
    b = gabgen.pairs_from_lists([p for p, _, _ in pairs], [t for _, t, _ in pairs])
    want = pyoracle.bpm(b)
    for i, (p, t, built_for) in enumerate(pairs):
        score, stage, _ = bpm_model(p, t)
        assert score == want[i]
        assert stage == built_for, (len(p), len(t), built_for, stage)
    got = {(min((len(p) + 63) // 64, 5), st) for p, _, st in pairs}
    # every band / window / full stage of every class that can reach it (class 1's window covers all of its 64 rows)
    assert got >= {(W, st) for W in (1, 2, 3, 4) for st in ("band", "window", "full") if (W, st) != (1, "full")}


def test_trip_edge_pairs_land_in_every_stage_at_every_text_length():
    """bpm_trip_edge_pairs(): each of score, band, window and full gets a pair of every text length 1 .. 70 (score and band of
    length 0 too: with an empty text there is no walk to leave the band), the pairs above 256 bases are class W = 5, and the
    model's scores are the oracle's"""
    pairs = bpm_trip_edge_pairs()
    lens = {st: set() for st in BPM_STAGES}
    for p, t, built_for, stage in pairs:
        lens[stage].add(len(t))
        assert stage == built_for or (len(t) == 0 and stage == "band"), (len(p), len(t), built_for, stage)
        if built_for == "generic":
            assert (len(p) + 63) // 64 == 5
    full = set(range(BPM_TRIP_EDGE_TLEN + 1))
    assert lens["score"] == full and lens["band"] == full and lens["generic"] == full
    assert lens["window"] == full - {0} and lens["full"] == full - {0}
    b = gabgen.pairs_from_lists([p for p, _, _, _ in pairs], [t for _, t, _, _ in pairs])
    np.testing.assert_array_equal(bpm_model_batch(b)[0], pyoracle.bpm(b))


def test_cascade_model_stage_rules():
    """the stage rules on hand-checkable pairs: generic above 256 bases, clean -> score, tlen 0 -> band"""
    assert bpm_model(b"ACGT" * 65, b"ACGT" * 60)[1:] == ("generic", 240 * 5)
    assert bpm_model(b"ACGT" * 10, b"ACGA" * 9)[1:] == ("score", 36)
    assert bpm_model(b"ACGN", b"") == (-4, "band", 0)
    assert bpm_model(b"acgt" * 20, b"ACGT" * 20) == (-80, "band", 2 * 80 * 2)
