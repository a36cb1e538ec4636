"""GPU: which kernel form of chain / fast-chain runs each call of a batch (genarchbench_amd/csrc/chain.hip, chain_tab.hip), and the
limits of each form.

Every run goes through gab_chain_run_device on device tensors filled with a sentinel and is checked twice: score and parent against
the oracle, and gab_chain_last_split -- the form that took each call -- against tests.util.chain_split_model (the batch-shape rule,
tests/test_chain_split_model.py) and, where a test sends every call to the table form, against that form's own conditions.
No GAB_CHAIN_TRACE here: the kernels that run are the ones a driver runs."""
import time

import numpy as np
import pytest

from oracle import pyoracle
from tools import gabgen
from tests import chain_form_cases as cases
from tests.util import CHAIN_DISPATCH, CHAIN_SPLIT_KNOBS, chain_split_margins, chain_split_model

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

PINNED = ("table-form-for-all", "latency-form-for-all", "throughput-form-for-all")
ONLY = {"latency-form-for-all": 2, "throughput-form-for-all": 1}
SENTINEL = -777


@pytest.fixture(scope="module")
def eng():
    from genarchbench_amd.chain import ChainEngine
    e = ChainEngine()
    yield e
    e.close()


_batches, _oracle, _device = {}, {}, {}


def batch_of(name, make):
    """the batch of a case, built once (and kept: the oracle's results and the device copies are filed under it)"""
    if name not in _batches:
        _batches[name] = make()
    return _batches[name]


def oracle(batch, mode):
    if (id(batch), mode) not in _oracle:
        _oracle[id(batch), mode] = pyoracle.chain(batch, mode)
    return _oracle[id(batch), mode]


def run(eng, monkeypatch, batch, mode, env, keep_device=True):
    """one gab_chain_run_device call under the pins `env`: results against the oracle, the split against the model -> (form, counters)"""
    import torch
    for k in CHAIN_SPLIT_KNOBS + ("GAB_CHAIN_TRACE", "GAB_CHAIN_TAB_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = torch.device("cuda:0")
    if id(batch) not in _device:
        xy = (torch.from_numpy(batch.x.view(np.int64)).to(dev), torch.from_numpy(batch.y.view(np.int64)).to(dev))
        if not keep_device:
            _device.clear()
        _device[id(batch)] = xy
    x, y = _device[id(batch)]
    sc = torch.full((batch.nanchors,), SENTINEL, dtype=torch.int32, device=dev); pa = torch.full_like(sc, SENTINEL)
    eng.run_device(mode, x, y, batch.call_off, batch.hdr, sc, pa, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    form, counters = eng.last_split(batch.ncalls)
    print("mode", mode, env, "forms", np.bincount(form, minlength=7).tolist(), form.tolist() if len(form) <= 32 else "", counters)
    ws, wp = oracle(batch, mode)
    np.testing.assert_array_equal(sc.cpu().numpy(), ws, err_msg=f"score, mode {mode}, {env}, forms {form.tolist()[:32]}")
    np.testing.assert_array_equal(pa.cpu().numpy(), wp, err_msg=f"parent, mode {mode}, {env}, forms {form.tolist()[:32]}")
    # the form before eligibility: 4 (not eligible) and 5 (handed back) are calls the rule sent to the table form
    np.testing.assert_array_equal(np.where((form == 4) | (form == 5), 3, form), chain_split_model(batch.hdr["n"], mode, env), err_msg=f"split, mode {mode}, {env}")
    assert counters["helpers"] == 0
    return form, counters


def per_call(batch, a):
    return [a[int(o):int(o) + int(n)] for o, n in zip(batch.call_off, batch.hdr["n"])]


def calls_of(batch):
    return [(float(h["avg_qspan"]), int(h["max_dist_x"]), int(h["max_dist_y"]), int(h["bw"]), int(h["n_segs"]), x, y)
            for h, x, y in zip(batch.hdr, per_call(batch, batch.x), per_call(batch, batch.y))]


# ---- C1: the pins are honoured ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dispatch", list(CHAIN_DISPATCH))
def test_dispatch_settings_are_honoured(eng, monkeypatch, dispatch, mode):
    """the four settings tests/test_chain_gpu.py runs under, on one mixed batch (200 calls of 50 .. 20 000 anchors): the forms are the
    model's, and a setting that names one form leaves no call to another"""
    batch = batch_of("mixed", lambda: gabgen.chain(31, 200, 0, 50, 20000))
    form, _ = run(eng, monkeypatch, batch, mode, CHAIN_DISPATCH[dispatch])
    if dispatch == "table-form-for-all":
        assert not np.isin(form, (1, 2)).any() and (form == 3).sum() > 150
    elif dispatch in ONLY:
        assert (form == ONLY[dispatch]).all()
    else:
        assert {1, 2} <= set(form.tolist()) and np.isin(form, (3, 5)).any()       # (a batch of 200 calls waits for its 20 000s)


@pytest.mark.parametrize("mode", [0, 1])
def test_legacy_only_launch_and_the_record_itself(eng, monkeypatch, mode):
    """GAB_CHAIN_HELPERS (both modes) and GAB_CHAIN_KERNEL=walk (chain) send everything through one launch of the older kernels: form
    6, and the helper count in the counters; gab_chain_last_split refuses another call count, and a handle that has not run"""
    from genarchbench_amd._lib import GabError
    from genarchbench_amd.chain import ChainEngine
    import torch
    batch = batch_of("small", lambda: gabgen.chain_from_calls(calls_of(gabgen.chain(39, 12, 1, 100, 3000)) + [cases.call([], [], [])]))
    assert batch.hdr["n"][-1] == 0
    run(eng, monkeypatch, batch, mode, {})
    x, y = _device[id(batch)]
    ws, wp = oracle(batch, mode)
    for env, want in (({"GAB_CHAIN_HELPERS": "5"}, 6), ({"GAB_CHAIN_KERNEL": "walk"}, 6 if mode == 0 else None)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sc = torch.full((batch.nanchors,), SENTINEL, dtype=torch.int32, device=x.device); pa = torch.full_like(sc, SENTINEL)
        eng.run_device(mode, x, y, batch.call_off, batch.hdr, sc, pa, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(sc.cpu().numpy(), ws)
        np.testing.assert_array_equal(pa.cpu().numpy(), wp)
        form, counters = eng.last_split(batch.ncalls)
        np.testing.assert_array_equal(form, chain_split_model(batch.hdr["n"], mode, env))
        if want:
            assert form.tolist() == [want] * 12 + [0]
        assert counters["helpers"] == 5 if "GAB_CHAIN_HELPERS" in env else (counters["helpers"] > 0) == (mode == 0)      # (walk: its own helper waves)
        for k in env:
            monkeypatch.delenv(k)
    with pytest.raises(GabError, match="calls"):
        eng.last_split(batch.ncalls + 1)
    fresh = ChainEngine()
    with pytest.raises(GabError, match="no completed"):
        fresh.last_split(batch.ncalls)
    fresh.close()


# ---- C2: the default rule, at shapes where it differs -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_default_rule_many_short_calls(eng, monkeypatch, mode):
    """2 000 calls of 60 .. 100 anchors: nobody waits for a 100-anchor call -- all in the throughput form"""
    batch = batch_of("short", lambda: gabgen.chain(54, 2000, 0, 60, 100))
    assert all(m < 0.9 for m in chain_split_margins(batch.hdr["n"], mode))
    form, _ = run(eng, monkeypatch, batch, mode, {})
    assert (form == 1).all()


def one_long_among_short():
    short = gabgen.chain(52, 80, 0, 300, 3000)
    keep = [c for c, k in zip(calls_of(short), short.hdr["n"]) if all(abs(int(k) - t) > 0.1 * t for t in (512, 2048))][:50]
    assert len(keep) == 50
    return gabgen.chain_from_calls(keep[:20] + calls_of(gabgen.chain(53, 1, 0, 30000, 30000)) + keep[20:])


@pytest.mark.parametrize("mode", [0, 1])
def test_default_rule_one_long_call_among_short_ones(eng, monkeypatch, mode):
    """one 30 000-anchor call among 50 of 300 .. 3 000: the batch waits for it.  A quarter of the batch's throughput time is a few
    dozen anchors' worth: the table form from 2 048 anchors, the latency form from 512, the rest in the throughput form"""
    batch = batch_of("one_long", one_long_among_short)
    n = batch.hdr["n"]
    assert n.max() >= 30000 and all(m > 1.1 for m in chain_split_margins(n, mode)) and n.sum() / 2.85e9 * 0.25 / 0.30e-6 < 0.9 * 2048
    form, _ = run(eng, monkeypatch, batch, mode, {})
    tab = np.isin(form, (3, 5))
    np.testing.assert_array_equal(tab, n >= 2048)
    np.testing.assert_array_equal(form == 2, (n >= 512) & (n < 2048))
    np.testing.assert_array_equal(form == 1, n < 512)
    assert tab.sum() > 5 and (form == 2).sum() > 5 and (form == 1).sum() > 1 and tab[np.argmax(n)]


@pytest.mark.parametrize("mode", [0, 1])
def test_default_rule_standing_floors(eng, monkeypatch, mode):
    """12.6 M anchors in 1 800 calls of 5 500 .. 8 500: nobody waits for the longest call, before or after the table form took its
    share (both comparisons 10 % away from flipping), so only the standing floors send calls to the table form: fast-chain those of
    >= 4 096 anchors -- all of them --, chain those of >= 8 192; the rest stays in the throughput form.  The split the full-size inputs run with."""
    t0 = time.time()
    batch = batch_of("floors", lambda: gabgen.chain(51, 1800, 0, 5500, 8500))
    n = batch.hdr["n"]
    assert batch.nanchors > 10_000_000 and (n >= 8192).sum() > 50 and (n < 8192).sum() > 50 and n.min() >= 4096
    assert all(m < 0.9 for m in chain_split_margins(n, mode))
    t1 = time.time()
    oracle(batch, mode)
    t2 = time.time()
    form, _ = run(eng, monkeypatch, batch, mode, {}, keep_device=False)
    print(f"standing floors, mode {mode}: {batch.nanchors} anchors, batch {t1 - t0:.1f} s, oracle {t2 - t1:.1f} s, GPU run and checks {time.time() - t2:.1f} s")
    tab = np.isin(form, (3, 5))
    np.testing.assert_array_equal(tab, n >= (8192 if mode == 0 else 4096))
    assert (form[~tab] == 1).all() and (form == 3).sum() >= 0.9 * tab.sum()
    if mode == 1:
        _device.clear(); _oracle.clear(); _batches.pop("floors")


# ---- C3: eligibility limits, one small call per side ------------------------------------------------------------------------------
LIMIT_CASES = ("q_span_0_and_255", "avg_qspan_4096", "max_dist_x_2p30", "max_dist_x_neg_and_0", "max_dist_y_0_and_neg", "min_max_dist_2p20", "bw_neg1",
               "x_span_2p31", "x_top_of_64_bits", "q_across_2p31", "n_segs_header_against_data")


def limit_case(name):
    if "limits" not in _batches:
        _batches["limits"] = {k: (gabgen.chain_from_calls(c), want, chains) for k, (c, want, chains) in cases.limit_cases().items()}
        assert set(_batches["limits"]) == set(LIMIT_CASES)
    return _batches["limits"][name]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", LIMIT_CASES)
def test_eligibility_limits(eng, monkeypatch, name, mode):
    """a call on each side of a limit (tests/chain_form_cases.py), sent to each form in turn: the oracle's result every time; in the
    table form the call is folded (3) on the eligible side and refused by ctab_prep (4) on the other"""
    batch, want, chains = limit_case(name)
    ws, wp = oracle(batch, mode)
    for wpc, ch in zip(per_call(batch, wp), chains):
        assert (wpc >= 0).sum() > 1900 if ch else (wpc == -1).all()
    if name == "q_across_2p31":
        # the reference's int32 q: differences wrap, so the call 2^30 lower on the query gives the same chains
        low = gabgen.chain_from_calls([c[:6] + ((c[6] & ~np.uint64(0xffffffff)) | ((c[6] - np.uint64(1 << 30)) & np.uint64(0xffffffff)),) for c in calls_of(batch)[:1]])
        ls, lp = pyoracle.chain(low, mode)
        np.testing.assert_array_equal(ls, per_call(batch, ws)[0]); np.testing.assert_array_equal(lp, per_call(batch, wp)[0])
    for dispatch in PINNED:
        form, _ = run(eng, monkeypatch, batch, mode, CHAIN_DISPATCH[dispatch])
        assert form.tolist() == (want[mode] if dispatch == "table-form-for-all" else [ONLY[dispatch]] * batch.ncalls), (dispatch, form.tolist())


@pytest.mark.parametrize("mode", [0, 1])
def test_byte_limit_of_the_table_form(eng, monkeypatch, mode):
    """the table form keeps a pair's overlap - gap cost + bias in a byte: calls whose largest q_span sweeps 166 .. 185 (and 250, 255)
    under bw = 500, avg_qspan = 15 are eligible up to some span and not from the next one on -- one change --, the call with spans of
    15 is; every one of them is the oracle's in every form"""
    batch = batch_of("sweep", lambda: gabgen.chain_from_calls(cases.byte_limit_sweep()))
    assert all((w >= 0).sum() > 1400 for w in per_call(batch, oracle(batch, mode)[1]))
    for dispatch in PINNED:
        form, _ = run(eng, monkeypatch, batch, mode, CHAIN_DISPATCH[dispatch])
        if dispatch != "table-form-for-all":
            assert (form == ONLY[dispatch]).all()
            continue
        assert form[0] == 3 and set(form.tolist()) == {3, 4}
        sweep = form[1:].tolist()
        k = sweep.index(4)
        assert 0 < k and sweep == [3] * k + [4] * (len(sweep) - k), sweep


# ---- C4: scores at the top of the 24 bits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_scores_at_the_top_of_the_key(eng, monkeypatch, mode):
    """the key forms keep a score in the 24 bits above a 7-bit code, up to 2^24 - 2^15 = 16 744 448.  Collinear calls (every anchor
    chains to the one before, the last score is n * span): 65 900 x 254 is 5 848 below the limit -- eligible for the table form, and
    beyond the latency form's 65 000 anchors --, 65 930 x 254 just above; 65 000 and 65 001 x 255 are the latency form's key path at
    its largest score and the first call beyond it (the table form refuses both: 255 + bias is no byte).  And a call of 65 900 anchors
    whose odd anchors lie beside the backbone: deeper windows, ties and filtered pairs next to scores of 2^23"""
    calls, want, last = cases.top_score_cases()
    batch = batch_of("top", lambda: gabgen.chain_from_calls(calls))
    ws, wp = oracle(batch, mode)
    assert [int(s[-1]) for s in per_call(batch, ws)[:4]] == last and all((p[1:] == np.arange(len(p) - 1)).all() for p in per_call(batch, wp)[:4])
    assert per_call(batch, ws)[4].max() == 65900 // 2 * 254
    for dispatch in PINNED:
        form, _ = run(eng, monkeypatch, batch, mode, CHAIN_DISPATCH[dispatch])
        if dispatch == "table-form-for-all":
            assert form[:4].tolist() == want[:4] and form[4] in (3, 5), form.tolist()
        else:
            assert (form == ONLY[dispatch]).all()


# ---- C5: lengths at block edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("step", [16, 3])
def test_lengths_at_block_edges(eng, monkeypatch, step, mode):
    """calls of 1, 2, 15 .. 17, 63 .. 65, 127 .. 129, 191 .. 193 and 4 095 .. 4 097 anchors -- the 64-anchor blocks of every form, the
    16-row groups and the special first block of the table form -- with windows that reach back across blocks: ~300 predecessors with
    anchors 16 apart, ~1 700 with anchors 3 apart.  The table form folds every one of them; the deep windows need three times the
    table a handle's first run allows for, so there a call may come back for want of room, and for nothing else"""
    batch = batch_of(f"edges{step}", lambda: gabgen.chain_from_calls(cases.block_edge_calls(step)))
    assert tuple(batch.hdr["n"]) == cases.EDGE_LENGTHS
    assert (oracle(batch, mode)[1] >= 0).sum() > 0.99 * (batch.nanchors - batch.ncalls)
    for dispatch in PINNED:
        form, counters = run(eng, monkeypatch, batch, mode, CHAIN_DISPATCH[dispatch])
        if dispatch != "table-form-for-all":
            assert (form == ONLY[dispatch]).all(), (dispatch, form.tolist())
        elif step == 16:
            assert (form == 3).all() and counters["no_room"] == 0, (form.tolist(), counters)
        else:
            assert np.isin(form, (3, 5)).all() and (form == 5).sum() == counters["no_room"] and form[-1] == 3, (form.tolist(), counters)
