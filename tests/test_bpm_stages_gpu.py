"""GPU: which stage of the bpm cascade finishes each pair (genarchbench_amd/csrc/bpm.hip), against the CPU model of tests/util.py.

Every call goes through run_device into an output filled with a sentinel and is checked three ways: the scores against the oracle,
the per-class stage counts GAB_BPM_TRACE prints against the model, and last_stats() against the model exactly."""
import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests.util import bpm_census, bpm_handmade_pairs, bpm_model_batch, bpm_trip_edge_pairs, parse_bpm_trace

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def eng():
    from genarchbench_amd.bpm import BpmEngine
    e = BpmEngine()
    yield e
    e.close()


@pytest.fixture
def traced(monkeypatch):
    monkeypatch.setenv("GAB_BPM_TRACE", "1")
    return monkeypatch


def run_checked(eng, batch, capfd):
    """one run_device call, checked against the oracle and the model -> (census, launches, {kernel: pairs it worked on})"""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)
    sc = torch.full((batch.n,), SENTINEL, dtype=torch.int32, device=dev)
    capfd.readouterr()
    eng.run_device(t(batch.pat), t(batch.pat_off), t(batch.pat_len), t(batch.txt), t(batch.txt_off), t(batch.txt_len),
                   sc, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    census, launches = parse_bpm_trace(capfd.readouterr().err)
    got = sc.cpu().numpy()
    np.testing.assert_array_equal(got, pyoracle.bpm(batch))
    scores, stages, steps = bpm_model_batch(batch)
    np.testing.assert_array_equal(scores, got)
    want = bpm_census(batch, stages)
    assert census == want, (census, want)
    st = eng.last_stats()
    assert st["block_steps"] == steps
    assert st["full_pairs"] == sum(c[1] for c in census.values()) + census.get(0, (0,))[0]
    # the template argument each score / band launch printed: D = 2W - 1 words exactly when the class's longest pattern fits them
    # (bpm_class_words, taken by the score and the band launch alike), W for the 64-row block form
    W_all = (batch.pat_len + 63) // 64
    for stage, cls, _, kernel in launches:
        if stage in ("score", "band"):
            arg = int(kernel[kernel.index("<") + 1:-1])
            odd = int(batch.pat_len[W_all == cls].max()) <= 32 * (2 * cls - 1)
            assert arg == (cls if kernel.startswith("bpm_score<") else 2 * cls - 1 if odd else 2 * cls), (kernel, cls)
    # a launch did work when its stage got pairs: score / band per slice, window = band misses, full = window misses
    worked = {}
    for stage, cls, _, kernel in launches:
        pairs, queued, band_miss, window_miss = census[cls]
        n = {"score": pairs, "band": queued, "window": band_miss, "full": window_miss if cls else pairs}[stage]
        if n:
            worked[kernel] = worked.get(kernel, 0) + n
    return census, launches, worked


def _random(seed, n, lo, hi, unclean=0.3):
    """n pairs with patterns of lo..hi bases, the text a mutated copy; a share of them with one N or lower-case base"""
    rng = np.random.default_rng(seed)
    pats, txts = [], []
    for _ in range(n):
        plen = int(rng.integers(lo, hi + 1))
        p = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, plen)].tobytes())
        t = bytearray(p[: plen - int(rng.integers(0, min(plen, 10)))])
        for k in rng.integers(0, max(1, len(t)), len(t) // 25):
            t[k] = b"ACGT"[int(rng.integers(0, 4))]
        if rng.random() < unclean:
            p[int(rng.integers(0, plen))] = ord(b"N" if rng.random() < 0.5 else b"a")
        pats.append(bytes(p)); txts.append(bytes(t))
    return pats, txts


def _census_batches():
    """three calls: every class's longest pattern fits 2W - 1 words (D odd), is one row longer, then fills 2W words; lengths on both
    sides of every 32-row boundary, unclean pairs in each class, the hand-made pairs of item 3 and pairs above 256 bases (bpm_full<0>)"""
    hand = bpm_handmade_pairs()
    out = []
    for extra in (0, 1, 32):
        pats, txts = [], []
        for W in (1, 2, 3, 4):
            top = 32 * (2 * W - 1) + extra
            lens = sorted(n for n in {64 * (W - 1) + 1, 64 * (W - 1) + 2, top - 33, top - 32, top - 31, top - 1, top} if 64 * (W - 1) < n <= top)
            for n in lens:
                p, t = _random(1000 * W + n, 12, n, n, unclean=0.5)
                pats += p; txts += t
            for p, t, _ in hand:
                if 64 * (W - 1) < len(p) <= top:
                    pats.append(p); txts.append(t)
        p, t = _random(99, 6, 257, 400)
        pats += p; txts += t
        out.append(gabgen.pairs_from_lists(pats, txts))
    return out


ALL_KERNELS = ({f"bpm_score32<{d}>" for d in range(1, 7)} | {"bpm_score32_wide<7>", "bpm_score32_wide<8>"} |
               {f"bpm_band<{d}>" for d in range(1, 9)} | {f"bpm_win<{w}>" for w in range(1, 5)} |
               {f"bpm_full<{w}>" for w in range(0, 5)})


@pytest.mark.parametrize("score64", [False, True])
def test_every_instantiation(eng, traced, capfd, score64):
    """score32 D = 1..8 (or, under GAB_BPM_SCORE64=1, bpm_score W = 1..4), band D = 1..8, win W = 1..4, full W = 2..4 and full<0>
    each finish pairs.  bpm_full<1> is launched but can get none: the window of class 1 holds all 64 of its rows."""
    if score64:
        traced.setenv("GAB_BPM_SCORE64", "1")
    worked, launched = {}, set()
    for batch in _census_batches():
        census, launches, w = run_checked(eng, batch, capfd)
        for k, v in w.items():
            worked[k] = worked.get(k, 0) + v
        launched |= {k for _, _, _, k in launches}
        assert census[1][3] == 0
    want = ALL_KERNELS - {"bpm_full<1>"}
    if score64:
        want = (want - {k for k in want if k.startswith("bpm_score32")}) | {f"bpm_score<{w}>" for w in range(1, 5)}
    assert "bpm_full<1>" in launched and "bpm_full<1>" not in worked
    assert set(worked) == want, sorted(set(worked) ^ want)
    print("pairs per kernel:", " ".join(f"{k}={worked[k]}" for k in sorted(worked)))


def test_handmade_pairs_at_the_miss_checks(eng, traced, capfd):
    """the pairs built one row inside and one row outside the 8-row band and the 64-row window, the clamps at row 0 and at the top
    of the class, tlen 0 / 1 / << plen, N and lower-case around every 64-row block boundary: each lands where the model says"""
    hand = bpm_handmade_pairs()
    batch = gabgen.pairs_from_lists([p for p, _, _ in hand], [t for _, t, _ in hand])
    census, _, _ = run_checked(eng, batch, capfd)
    assert census == bpm_census(batch, [st for _, _, st in hand])


@pytest.mark.parametrize("score64", [False, True])
def test_text_lengths_at_every_trip_edge(eng, traced, capfd, score64):
    """text lengths 0 .. 70 -- every boundary of the 32-, 16- and 4-base trips of the walks over the text -- in every stage:
    score (both forms), band, window, full (classes 2 and 3) and generic each get a pair of every length (bpm_trip_edge_pairs)"""
    if score64:
        traced.setenv("GAB_BPM_SCORE64", "1")
    pairs = bpm_trip_edge_pairs()
    batch = gabgen.pairs_from_lists([p for p, _, _, _ in pairs], [t for _, t, _, _ in pairs])
    census, _, worked = run_checked(eng, batch, capfd)
    assert census == bpm_census(batch, [st for _, _, _, st in pairs])
    assert any(k.startswith("bpm_score<" if score64 else "bpm_score32") for k in worked)
    assert {"bpm_full<2>", "bpm_full<3>", "bpm_full<0>"} <= set(worked)


def test_more_listed_pairs_than_history_slots(eng, traced, capfd):
    """> 65 536 pairs of class 1 reach bpm_win (its 65 536 history slots are reused) and > 16 384 pairs of class 2 reach
    bpm_full<2> (16 384 slots): the grid-stride loops.  Short texts (tlen << plen) keep it cheap."""
    rng = np.random.default_rng(5)
    lut = np.frombuffer(b"ACGT", np.uint8)
    pats, txts = [], []
    tmpl1 = []
    for _ in range(300):
        n = int(rng.integers(16, 65)); m = int(rng.integers(1, 5))
        p = bytearray(lut[rng.integers(0, 4, n)].tobytes()); p[int(rng.integers(0, n))] = ord("N")
        tmpl1.append((bytes(p), bytes(p[n - m:])))
    tmpl2 = []
    for _ in range(300):
        n = int(rng.integers(100, 129)); m = int(rng.integers(1, 9))
        p = bytearray(lut[rng.integers(0, 4, n)].tobytes()); p[int(rng.integers(0, n))] = ord("g")
        tmpl2.append((bytes(p), bytes(p[:m])))
    for k in rng.integers(0, 300, 70000):
        pats.append(tmpl1[k][0]); txts.append(tmpl1[k][1])
    for k in rng.integers(0, 300, 17500):
        pats.append(tmpl2[k][0]); txts.append(tmpl2[k][1])
    order = rng.permutation(len(pats))
    batch = gabgen.pairs_from_lists([pats[i] for i in order], [txts[i] for i in order])
    census, _, worked = run_checked(eng, batch, capfd)
    assert census[1][2] > 65536 and census[2][3] > 16384
    assert worked["bpm_win<1>"] > 65536 and worked["bpm_full<2>"] > 16384


@pytest.mark.parametrize("identity", [True, False])
def test_sixteen_slices(eng, traced, capfd, identity):
    """GAB_BPM_SLICES=16 on a few thousand pairs: some slices are empty, the band kernels of the others read their queue lengths
    on the device.  identity: one class (no scatter pass); else several classes in permuted order."""
    traced.setenv("GAB_BPM_SLICES", "16")
    batch = (gabgen.pairs(81, 3000, 0, 151) if identity else gabgen.pairs(82, 4000, 1, 256)).swapped_longer_first()
    census, launches, _ = run_checked(eng, batch, capfd)
    slices = {}
    for stage, cls, k, _ in launches:
        if stage == "score":
            slices.setdefault(cls, set()).add(k)
    if identity:
        assert list(census) == [3]
    else:
        assert len([c for c in census if c]) >= 3
    assert all(c[1] > 0 for k, c in census.items() if k)                       # unclean pairs in every class
    assert max(len(s) for s in slices.values()) > 1 and all(len(s) < 16 for s in slices.values())
