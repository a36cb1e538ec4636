"""GPU: which launch of the wfa cascade finishes each pair (genarchbench_amd/csrc/wfa.hip), against the CPU model of tests/util.py.

Every call goes through run_device into outputs filled with a sentinel and is checked three ways: operations, lengths and scores
against the oracle; last_stats()["work"] against the oracle's cell count; the launches GAB_WFA_TRACE prints against the plan (kernel
with its template arguments, pool, directory) and their pairs in / pairs left -- and `requeued`, their sum -- against the model.
The batches are the cases of tests.util.wfa_tier_cases; tests/test_wfa_oracle.py holds the model itself against the oracle."""
import numpy as np
import pytest

from oracle import pyoracle
from tests.util import WFA_BIG_PENALTIES, WFA_SMALL_PENALTIES, parse_wfa_trace, wfa_case_model, wfa_expected_resumed, wfa_fit

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def engines():
    from genarchbench_amd.wfa import AffineWavefronts
    made = {}

    def get(pen, red):
        if (pen, red) not in made:
            kw = {} if red is None else dict(min_wavefront_length=red[0], max_distance_threshold=red[1])
            made[pen, red] = AffineWavefronts(*pen, **kw)
        return made[pen, red]
    yield get
    for e in made.values():
        e.close()


_oracle = {}


def run_checked(engines, name, monkeypatch, capfd):
    """one run_device call of a case, checked against the oracle and the model -> (traced launches, model launches)"""
    import torch
    from genarchbench_amd.wfa import ops_layout
    batch, pen, red, knobs, model, plan, tier, launches = wfa_case_model(name)
    key = (id(batch), pen, red)
    if key not in _oracle:
        _oracle[key] = pyoracle.wfa(batch, pen, want_cells=True, reduction=red)
    w_ops, w_off, w_len, w_score, w_cells = _oracle[key]
    monkeypatch.setenv("GAB_WFA_TRACE", "1")
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    eng = engines(pen, red)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)
    off, total = ops_layout(batch)
    ops = torch.full((total + 16,), SENTINEL & 0xff, dtype=torch.uint8, device=dev)
    ln = torch.full((batch.n,), SENTINEL, dtype=torch.int32, device=dev); sc = torch.full_like(ln, SENTINEL)
    capfd.readouterr()
    eng.run_device(t(batch.pat), t(batch.pat_off), t(batch.pat_len), t(batch.txt), t(batch.txt_off), t(batch.txt_len),
                   ops, t(off), ln, sc, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    traced, tail = parse_wfa_trace(capfd.readouterr().err)
    stats = eng.last_stats()
    print(name, "traced:", traced, tail, "work", stats["work"])
    # 1. the results
    g_ops = ops.cpu().numpy()
    np.testing.assert_array_equal(sc.cpu().numpy(), w_score)
    np.testing.assert_array_equal(ln.cpu().numpy(), w_len)
    np.testing.assert_array_equal(off, w_off)
    mask = np.zeros(total, bool)
    for o, l in zip(w_off, w_len):
        mask[o:o + l] = True
    np.testing.assert_array_equal(g_ops[:total][mask], w_ops[:total][mask])
    assert (g_ops[total:] == SENTINEL & 0xff).all()                    # nothing written behind the last pair's room
    # 2. the work count
    assert stats["work"] == w_cells
    # 3. the launches and what each got and left
    assert [l[:3] for l in traced] == [l[:3] for l in launches]
    assert [l[3:5] for l in traced] == [l[3:5] for l in launches]
    requeued = sum(l[4] for l in launches)
    assert stats["requeued"] == requeued
    assert tail == {"n_lds": plan["n_lds"], "n_big": plan["n_big"], "requeued": requeued}
    want_resumed = wfa_expected_resumed(name)
    for k, l in enumerate(traced):
        if k == 1 and want_resumed is not None:
            assert want_resumed[0] <= l[5] <= want_resumed[1], (l, want_resumed)
        else:
            assert l[5] is None
    return traced, launches


def finished(launches):
    """{kernel + pool: pairs the launch finished}"""
    out = {}
    for l in launches:
        out[l[0], l[1]] = out.get((l[0], l[1]), 0) + l[3] - l[4]
    return out


def test_census(engines, monkeypatch, capfd):
    """a. complete mode, (4, 6, 2), 1 500 pairs at error rates 0 .. 0.6 and three pairs of more than 2 040 bases (so the LDS launches
    read the scattered list): both static launches, both wfa_lds<64> pools and wfa_global each finish at least 20 pairs"""
    traced, _ = run_checked(engines, "census", monkeypatch, capfd)
    assert [l[0] for l in traced] == ["wfa_lds_static<16,false>", "wfa_lds_static<16,true>", "wfa_lds<64,false,int16_t>",
                                      "wfa_lds<64,false,int16_t>", "wfa_global<false>", "wfa_global<false>"]
    assert all(l[3] - l[4] >= 20 for l in traced[:5])
    assert traced[5][3:5] == (3, 0)
    print("census, pairs per launch:", " ".join(f"{l[0]}/{l[1]}={l[3] - l[4]}" for l in traced))


def test_boundary_pairs(engines, monkeypatch, capfd):
    """b. for every pool of the default plan a pair on the last score that fits it and one on the next score that has a wavefront
    (40 | 42, 60 | 62, 92 | 94 and 258 | 260 as the recurrence places them), among 200 easy pairs"""
    traced, launches = run_checked(engines, "boundary", monkeypatch, capfd)
    assert [l[1] for l in traced] == [1184, 2560, 6144, 49152, 1 << 20]
    assert traced[4][3:5] == (1, 0)                     # the pair one score above the largest LDS pool, and nothing else


@pytest.mark.parametrize("name", ["pen_%d_%d_%d" % p for p in WFA_BIG_PENALTIES] + ["pen_50_60_20_nostatic"])
def test_directory_bound_penalties(engines, monkeypatch, capfd, name):
    """c. penalties so large that the directory sizes 56 / 128 / 640 / 4 096 end a tier, never the pool: seven pairs with scores on
    both sides of each.  (300, 400, 150) and (1000, 1500, 500) have fewer than 16 score rows below 1 024, so complete mode starts in
    wfa_lds<16,false,OffB>; under the latter the first stepped score is null (the step table's 255 cap) and a score of 4 500 takes
    the second round of wfa_global with four times the directory."""
    traced, _ = run_checked(engines, name, monkeypatch, capfd)
    kernels = [l[0] for l in traced]
    if name == "pen_50_60_20":
        assert kernels[0] == "wfa_lds_static<16,false>" and traced[0][3:5] == (7, 0)
    else:
        assert kernels[0] == "wfa_lds<16,false,OffB>" and traced[0][2] == 56 and traced[0][3] - traced[0][4] >= 1
    if name == "pen_50_60_20_nostatic":
        assert [l[3] - l[4] for l in traced] == [2, 3, 2, 0]               # scores 0 50 | 80 100 100 | 150 180
    if name == "pen_300_400_150":
        assert [l[3] - l[4] for l in traced] == [1, 0, 3, 3]               # 0 | | 300 550 600 | 700 900 1250
    if name == "pen_1000_1500_500":
        assert [l[3] - l[4] for l in traced] == [1, 0, 0, 5, 1] and traced[4][:3] == ("wfa_global<false>", 1 << 23, 16384)


@pytest.mark.parametrize("pen", WFA_SMALL_PENALTIES)
def test_small_penalties_on_the_census(engines, monkeypatch, capfd, pen):
    """c. the penalty sets of test_other_penalties on 1 000 pairs of the census recipe"""
    run_checked(engines, "census1000_%d_%d_%d" % pen, monkeypatch, capfd)


@pytest.mark.parametrize("tmax", [227, 228])
def test_static_tier_switch(engines, monkeypatch, capfd, tmax):
    """d. the longest text at 227 (static_rows = 16: the static tier is on, int16 pools behind it) and at 228 (off: the first tier
    is wfa_lds<16,false,int16_t> with 1 024 offsets), with texts at the limit, pure insertions and pairs past 16 score rows.

    The static tier's exit on an M offset > 240 cannot be taken by a pair without padding bytes: an offset passes the end of the
    text by at most one per score row, a static launch walks fewer than 243 - tlen rows, and with static_pool >= 1 024 the patterns
    are at most 232 bases, so an offset that reaches the end of a 227-base text by row 1 belongs to a pair that ends by score 20,
    and one that reaches it from row 2 on stays at or below 227 + 13.  test_byte_offset_exit covers the same exit of wfa_lds."""
    traced, _ = run_checked(engines, "tmax%d" % tmax, monkeypatch, capfd)
    if tmax == 227:
        assert traced[0][:3] == ("wfa_lds_static<16,false>", 1024, 16) and traced[1][:3] == ("wfa_lds_static<16,true>", 2560, 16)
        assert traced[1][3] == traced[1][4] and traced[1][5] == 0          # the row limit, not the pool, ended them: nothing to resume
        assert traced[2][0] == "wfa_lds<64,false,int16_t>"
    else:
        assert traced[0][:3] == ("wfa_lds<16,false,int16_t>", 1024, 48)
    assert traced[0][3] - traced[0][4] >= 20 and traced[0][4] >= 20


def test_adaptive_int16_first_tier(engines, monkeypatch, capfd):
    """d. the batch of the 228 case in adaptive mode: wfa_lds<16,true,int16_t>"""
    traced, _ = run_checked(engines, "tmax228_adaptive_10_50", monkeypatch, capfd)
    assert traced[0][:3] == ("wfa_lds<16,true,int16_t>", 1024, 48) and traced[0][3] - traced[0][4] >= 20


def test_byte_offset_exit(engines, monkeypatch, capfd):
    """d. GAB_WFA_NO_STATIC=1, patterns that end in 56 .. 66 'Y' behind a 180-base match: the extension of score 0 runs on into the
    text's padding to M offsets of 236 .. 246, on both sides of the 240 above which wfa_lds<16,false,OffB> passes a pair on (its
    first check).  No count can tell that exit from the directory's: a pair whose pattern reaches 54 bases past a text of at most
    187 needs a gap that long, i.e. a score beyond the tier's 56; what is checked is that such pairs leave the tier and end right."""
    traced, _ = run_checked(engines, "offb_exit", monkeypatch, capfd)
    assert traced[0][0] == "wfa_lds<16,false,OffB>" and traced[0][4] >= 12


@pytest.mark.parametrize("red", [(10, 50), (5, 3)])
def test_adaptive_census(engines, monkeypatch, capfd, red):
    """e. adaptive mode on 1 000 census pairs and the boundary pairs: the pool a pair needs now depends on its data -- the model's
    reduction decides which launch holds it"""
    traced, _ = run_checked(engines, "adaptive_%d_%d" % red, monkeypatch, capfd)
    assert traced[0][:3] == ("wfa_lds<16,true,OffB>", 1328, 48)
    assert all(l[0] == "wfa_lds<64,true,int16_t>" for l in traced[1:3]) and traced[3][0] == "wfa_global<true>"


def test_more_pairs_than_a_chained_grid(engines, monkeypatch, capfd):
    """g. 3 000 pairs most of which leave the static launches: more than 256 reach each wfa_lds<64> launch and more than 64 the
    first wfa_global, so their waves stride over the lists.  f, default slots: every pair the first launch leaves is resumed."""
    traced, _ = run_checked(engines, "grid", monkeypatch, capfd)
    assert traced[2][3] > 256 and traced[3][3] > 256 and traced[4][3] > 64
    assert traced[1][5] == traced[0][4]


@pytest.mark.parametrize("slots", [0, 3, 1002])
def test_resume_slots(engines, monkeypatch, capfd, slots):
    """f. GAB_WFA_SLOTS: the first `slots` pairs the first static launch leaves are resumed, the others start over -- with 3 and
    1 002 both kinds share a wave.  The batch has no 'X' / 'Y' and short texts, so every pair left stopped for want of room."""
    traced, _ = run_checked(engines, "slots_%d" % slots, monkeypatch, capfd)
    assert traced[0][4] > 1002 and traced[1][5] == slots


@pytest.mark.parametrize("pool2", [1024, 4080])
def test_second_static_pool(engines, monkeypatch, capfd, pool2):
    """f. GAB_WFA_POOL2 = 1 024 (not above the first pool: no second static launch) and 4 080 (its boundary moves to 74 | 76)"""
    traced, _ = run_checked(engines, "pool2_%d" % pool2, monkeypatch, capfd)
    statics = [l for l in traced if l[0].startswith("wfa_lds_static")]
    if pool2 == 1024:
        assert len(statics) == 1
    else:
        assert len(statics) == 2 and statics[1][1] == 4080 and wfa_fit((4, 6, 2), 4080) == (74, 76)
