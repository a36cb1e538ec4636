"""GPU: the results gab_chain_run_device_through (and gab_chain_run) leaves in the caller's HOST arrays -- on every route they take
there (written through by the DP kernels block by block, copied at the end, both), in every kernel form, at the forms' edges and in
layouts with gaps, calls out of order and empty calls (tests/chain_through_cases.py; tests/test_chain_through_cases.py shows on the
CPU that every case reaches what it is named for).

One helper does every run.  Device arrays pre-filled with one sentinel, host arrays with another, 64 canary elements on either side
of the window the library is given.  Then, in this order: the host window is the oracle's on every element of a call; so are the
device arrays; the canaries are untouched; an element of the window that belongs to no call holds the host sentinel or what the
device array holds there; gab_chain_last_split is tests.util.chain_split_model's split; gab_chain_last_through is
tests.util.chain_through_route's route.  Equalities throughout."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import chain_through_cases as tc
from tests.util import CHAIN_SPLIT_KNOBS, chain_split_model, chain_through_route

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

DEV_SENTINEL, HOST_SENTINEL, CANARY = -777, -555, 64
CASES = tc.through_cases()


@pytest.fixture(scope="module")
def eng():
    """one handle for the module, its table sized by a first table-form run of a thousand blocks (a handle's first run sizes the table for
    ~430 rows per block of THAT batch and later runs keep it: the cases that follow find room whatever their order)"""
    import os
    import torch
    from genarchbench_amd.chain import ChainEngine
    from tools import gabgen
    from tests import chain_form_cases as cases
    e = ChainEngine()
    warm = gabgen.chain_from_calls([cases.call(*cases.diagonal(np.random.default_rng(70), n=64000, step=100))])
    saved = {k: os.environ.pop(k, None) for k in CHAIN_SPLIT_KNOBS + ("GAB_CHAIN_TAB_MB",)}
    os.environ["GAB_CHAIN_TAB_MIN"] = "1"
    try:
        dev = torch.device("cuda:0")
        x, y = torch.from_numpy(warm.x.view(np.int64)).to(dev), torch.from_numpy(warm.y.view(np.int64)).to(dev)
        sc = torch.zeros(warm.nanchors, dtype=torch.int32, device=dev); pa = torch.zeros_like(sc)
        e.run_device(0, x, y, warm.call_off, warm.hdr, sc, pa, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert e.last_split(1)[0].tolist() == [3]
    finally:
        del os.environ["GAB_CHAIN_TAB_MIN"]
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    yield e
    e.close()


_oracle, _device = {}, {}


def oracle(key, mode):
    """the oracle's results for the gapless batch CALLS[key]: computed once, shared, never written to"""
    if (key, mode) not in _oracle:
        s, p = pyoracle.chain(tc.batch_of(key), mode)
        s.flags.writeable = p.flags.writeable = False
        _oracle[key, mode] = (s, p)
    return _oracle[key, mode]


def host_window(total, off_line=False):
    """-> (base, window): `total` elements that start on a 64-byte line (off_line: one element past it) inside an array of
    HOST_SENTINEL, CANARY elements at least on either side"""
    base = np.full(total + 2 * CANARY + 32, HOST_SENTINEL, np.int32)
    k = CANARY + (-(base.ctypes.data // 4 + CANARY)) % 16 + (1 if off_line else 0)
    w = base[k:k + total]
    assert k >= CANARY and len(base) - (k + total) >= CANARY
    assert total == 0 or (w.base is base and w.ctypes.data % 64 == (4 if off_line else 0))      # (an empty view has no address of its own)
    return base, w, k


def set_env(monkeypatch, env):
    for k in CHAIN_SPLIT_KNOBS + ("GAB_CHAIN_TRACE", "GAB_CHAIN_TAB_MB", "GAB_CHAIN_FEED_MIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_results(pl, key, mode, host, device, label, asked=True, gaps_untouched=False):
    """steps 1 to 4: host windows against the oracle, device arrays against the oracle, canaries, gaps.  host: (score, parent) as
    host_window made them; device: the (score, parent) device arrays as numpy, None where the library keeps them to itself
    (gab_chain_run); asked=False: the call was given no host arrays, nothing of them may be written"""
    want = oracle(key, mode)
    total = pl.total
    gap = np.ones(total, bool); gap[pl.owned] = False
    names = ("score", "parent")
    if asked:
        for (base, w, k), ww, what in zip(host, want, names):
            np.testing.assert_array_equal(w[pl.owned], ww[pl.src], err_msg=f"host {what}, {label}")
    if device is not None:
        for dev, ww, what in zip(device, want, names):
            np.testing.assert_array_equal(dev[pl.owned], ww[pl.src], err_msg=f"device {what}, {label}")
    for (base, w, k), what in zip(host, names):
        assert (base[:k] == HOST_SENTINEL).all() and (base[k + total:] == HOST_SENTINEL).all(), f"canaries of host {what}, {label}"
    for i, ((base, w, k), what) in enumerate(zip(host, names)):
        if not asked:
            assert (w == HOST_SENTINEL).all(), f"host {what} written to, {label}"
        elif device is not None:
            bad = np.nonzero(gap & (w != HOST_SENTINEL) & (w != device[i]))[0]
            assert len(bad) == 0, f"gaps of host {what} at {bad[:8].tolist()}, {label}"
        elif gaps_untouched:
            assert (w[gap] == HOST_SENTINEL).all(), f"gaps of host {what}, {label}"
    if device is not None:
        for dev, what in zip(device, names):                  # (the kernels store to the calls' own elements of the device arrays only)
            assert (dev[gap] == DEV_SENTINEL).all(), f"gaps of device {what}, {label}"


def run_case(eng, monkeypatch, case, mode):
    """one gab_chain_run_device_through call (gab_chain_run_device where the case does not ask for host arrays) -> (form, counters)"""
    import torch
    set_env(monkeypatch, case.env)
    pl = tc.placed_of(case)
    b, total = pl.batch, pl.total
    dev = torch.device("cuda:0")
    dkey = (case.calls, case.layout)
    if dkey not in _device:
        _device[dkey] = (torch.from_numpy(b.x.view(np.int64)).to(dev), torch.from_numpy(b.y.view(np.int64)).to(dev))
    x, y = _device[dkey]
    sc = torch.full((total,), DEV_SENTINEL, dtype=torch.int32, device=dev); pa = torch.full_like(sc, DEV_SENTINEL)
    hs, hp = host_window(total, pl.off_line), host_window(total, pl.off_line)
    stream = torch.cuda.current_stream().cuda_stream
    if case.pinned is None:
        eng.run_device(mode, x, y, b.call_off, b.hdr, sc, pa, stream=stream)
    else:
        rs, rp = eng.run_device_through(mode, x, y, b.call_off, b.hdr, sc, pa, pinned=case.pinned, stream=stream, host=(hs[1], hp[1]))
        assert rs is hs[1] and rp is hp[1]
    torch.cuda.synchronize()
    form, counters = eng.last_split(b.ncalls)
    route = eng.last_through()
    label = f"{case.name}, mode {mode}, {case.env}, route {route}, forms {np.bincount(form, minlength=7).tolist()}, {counters}"
    print(label)
    check_results(pl, case.calls, mode, (hs, hp), (sc.cpu().numpy(), pa.cpu().numpy()), label, asked=case.pinned is not None)
    n = b.hdr["n"]
    np.testing.assert_array_equal(np.where((form == 4) | (form == 5), 3, form), chain_split_model(n, mode, case.env, through=bool(case.pinned), total=total),
                                  err_msg=f"split, {label}")
    assert route == chain_through_route(n, b.call_off, mode, case.env, case.pinned, form), label
    # what the case is named for
    assert route == case.route, label
    if case.forms:
        assert form.tolist() == case.forms[mode], label
    if case.all_form is not None:
        assert (form[n > 0] == case.all_form).all() and (form[n == 0] == 0).all(), label
    for f in case.has_form:
        assert (form == f).any(), label
    return form, counters


RUNS = [pytest.param(c, m, id=f"{c.name}-{('chain', 'fastchain')[m]}") for c in CASES if not c.fresh for m in c.modes]


@pytest.mark.parametrize("case,mode", RUNS)
def test_written_through_results(eng, monkeypatch, case, mode):
    """every case of tests/chain_through_cases.py on the module's handle"""
    run_case(eng, monkeypatch, case, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_handed_back_for_want_of_room(monkeypatch, mode):
    """GAB_CHAIN_TAB_MB=2 on a fresh handle: the table holds 2 048 groups and the batch needs more whatever its windows -- calls come back
    (form 5) after the kernels wrote through for the others, the longest call (last in the batch, first in the sorted list) is folded"""
    from genarchbench_amd.chain import ChainEngine
    case = [c for c in CASES if c.fresh]
    assert len(case) == 1
    set_env(monkeypatch, case[0].env)                         # (the budget is fixed at the handle's first table-form call)
    e = ChainEngine()
    try:
        form, counters = run_case(e, monkeypatch, case[0], mode)
    finally:
        e.close()
    assert counters["no_room"] >= 1 and (form == 5).sum() >= counters["no_room"] and form[-1] == 3, (form.tolist(), counters)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path", list(tc.HOST_ENTRY_PATHS))
def test_host_entry_point_with_gaps_and_calls_out_of_order(eng, monkeypatch, path, mode):
    """gab_chain_run on its three paths -- the small-batch path (gab_chain_run_device between two copies of the whole extent), the fed
    path (page-locked: the DP kernel writes through at the caller's offsets from arrays it packs its own way) and the copy-engine
    path (results back in two pieces, cut where the first call of the second half begins) -- on a layout with gaps, out of order"""
    from genarchbench_amd._lib import GabError
    env, pinned = tc.HOST_ENTRY_PATHS[path]
    set_env(monkeypatch, env)
    pl = tc.placed("host_entry", "host_entry")
    hs, hp = host_window(pl.total), host_window(pl.total)
    rs, rp = eng.host_chain_kernel(pl.batch, mode, pinned=pinned, host=(hs[1], hp[1]))
    assert rs is hs[1] and rp is hp[1]
    # (fed: written through at the calls' own elements, nothing else of the window is touched; the other paths copy the whole extent
    # from arrays of the library's own: gaps unspecified)
    check_results(pl, "host_entry", mode, (hs, hp), None, f"gab_chain_run, {path}, mode {mode}", gaps_untouched=path == "fed")
    if path == "small_batch":
        form, _ = eng.last_split(pl.batch.ncalls)
        np.testing.assert_array_equal(form, chain_split_model(pl.batch.hdr["n"], mode, env, total=pl.total))
        assert eng.last_through() == 0
    else:
        with pytest.raises(GabError, match="no completed"):
            eng.last_through()
