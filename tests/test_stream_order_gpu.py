"""GPU: the stream contract of the `_device` entry points (include/gab.h, Conventions): they enqueue on `stream`, and whatever they
run on streams of their own is forked from and joined back into `stream` inside the call, so that a caller only orders against
`stream`.  Every other GPU test uploads its inputs, synchronises the device, calls, synchronises and reads: nothing is ever pending,
so an internal stream that does not wait for the caller's, a planning copy on the null stream or a missing join would still give
the right numbers.  Here the inputs are still being produced on the caller's stream when the entry point is called, and they are
destroyed on it right behind the call.

One call, ordered(): the input tensors hold a DECOY (tests/stream_order_cases.py: a valid input whose answer differs from the real
one in at least 90 % of every output), then, on a fresh side stream S:
    a delay; copy_ of every real input from resident staging tensors; a fill of every output with a sentinel; an event P;
    assert not P.query()  -- the producer is still pending (a failure says the delay is too short; it is no skip);
    the entry point with stream = S;
    directly behind it, no host synchronisation between: clone() of every output; the decoy over every input; an event, and the
    host waits for that event only.
Both the clones and -- after a device synchronisation -- the output tensors must be the real expected outputs bit for bit, and the
last_stats counters the model's.
    the pending copy_ catches early reads, the host's planning copies of lengths and offsets included;
    the sentinel fill behind the delay catches early writes of an internal stream (they are overwritten by the fill);
    the decoy behind the call catches an internal stream that is not joined into S before the call's work on S counts as done.
test_control_* run ordered() on stand-ins, plain torch ops over the same valid buffers, that break the contract in each of the
three ways: the harness reports the decoy's numbers, the sentinel, the decoy's numbers.  They touch no library code.

The delay is torch.cuda._sleep, calibrated once per module with torch events (a chain of large matrix products where _sleep does
not delay).  Before a delayed call the same call runs twice in the ordinary way, synchronised: once so that the handle's buffers
and lazily created streams exist, once timed (wall time).  Every test asserts delay >= 5 x its warm time and prints both, and the
module prints all of them at its end.

Measured on an MI355X, warm undelayed call, wall time with its synchronisation (ms):
    bsw      one launch 4.8 (score and result); multi class 23.0 / 25.2; sliced 35.0 / 33.5 (with GAB_BSW_TRACE printing)
    chain    default 0.8 .. 1.3; latency form 2.1 .. 2.6; throughput form 5.0 .. 6.1; table form 0.8 .. 1.2
    bpm 1.8; bitpal 0.6 / 0.5; wfa 3.6
    kmer     count 0.3, count_part 0.3, sketch 0.7, index_minimizers 1.1, index_part 0.9, index_solid 0.8, solid_positions 0.5
    abea     align 1.0, events 0.8, scalings 0.2, calibrate 0.3
    fmi      seed 1.7, sa_lookup 0.4;  parse  bsw 0.2, pairs 0.1, chain 0.2
The longest is 35 ms, five times that 175 ms.  DELAY_MS = 400 (the calibrated sleep measured 459 ms): eleven warm calls of the
slowest form, so that the host still finds the producer pending when a neighbour loads the GPU or the host."""
import time

import numpy as np
import pytest

from tests import stream_order_cases as soc
from tests.util import CHAIN_DISPATCH, CHAIN_SPLIT_KNOBS, chain_split_model

pytestmark = pytest.mark.gpu

DELAY_MS = 400.0
FILL_BEFORE, SENTINEL = 0xA5, soc.SENTINEL8
MEASURED = {}


class Delay:
    """enqueue(): DELAY_MS of work on the current stream that touches no buffer of the test"""

    def __init__(self):
        import torch
        self.torch = torch
        self.cycles, self.reps = 0, 0
        probe = 20_000_000
        torch.cuda._sleep(1000)
        ms = self._time(lambda: torch.cuda._sleep(probe))
        if ms > 1.0:
            self.cycles = int(probe * DELAY_MS * 1.15 / ms)
        else:        # _sleep does not delay on this device: large matrix products
            self.a = torch.ones((4096, 4096), device="cuda:0")
            one = self._time(lambda: [self.a @ self.a for _ in range(8)]) / 8
            self.reps = int(DELAY_MS * 1.15 / one) + 1
        self.ms = self._time(self.enqueue)
        print(f"\ndelay: probe {ms:.2f} ms, cycles {self.cycles} reps {self.reps}, measured {self.ms:.1f} ms (wanted {DELAY_MS})")

    def _time(self, fn):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def enqueue(self):
        if self.cycles:
            self.torch.cuda._sleep(self.cycles)
        else:
            for _ in range(self.reps):
                self.a @ self.a


@pytest.fixture(scope="module")
def delay():
    d = Delay()
    assert d.ms >= DELAY_MS, f"the calibrated delay came out at {d.ms:.1f} ms"
    yield d
    print("\nwarm call times (ms):", {k: round(v, 2) for k, v in MEASURED.items()}, "delay", round(d.ms, 1))


def _bytes(t):
    import torch
    return t.view(torch.uint8) if t.dtype != torch.uint8 else t


def ordered(name, real, decoy, outs, call, delay, grab=None):
    """real / decoy: {input name: numpy array}; outs: {output name: numpy array giving shape and dtype}; call(inp, out, stream) runs
    the entry point on {name: tensor} dicts and returns what it gives back on the host (or None).  grab(host, stream), for an entry
    point whose outputs lie in memory of the handle: -> {name: tensor} copied out of it on `stream`; they take the clones' place.
    -> (clones made on S behind the call, the output tensors after a device synchronisation, the host result), as numpy"""
    import torch
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    stage = {k: up(v) for k, v in real.items()}
    dec = {k: up(v) for k, v in decoy.items()}
    inp = {k: v.clone() for k, v in stage.items()}
    out = {k: torch.empty(v.shape, dtype=torch.from_numpy(np.empty(0, v.dtype)).dtype, device=dev) for k, v in outs.items()}
    for t in out.values():
        _bytes(t).fill_(FILL_BEFORE)
    torch.cuda.synchronize()
    # warm-up, the ordinary way: the handle's buffers and streams exist afterwards; the second run is timed
    call(inp, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(inp, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    warm_ms = (time.perf_counter() - t0) * 1e3
    MEASURED[name] = warm_ms
    for k in inp:
        inp[k].copy_(dec[k])
    for t in out.values():
        _bytes(t).fill_(FILL_BEFORE)
    torch.cuda.synchronize()
    print(f"\n{name}: warm call {warm_ms:.2f} ms, delay {delay.ms:.1f} ms")
    assert delay.ms >= 5 * warm_ms, f"the delay ({delay.ms:.1f} ms) is shorter than five warm calls ({warm_ms:.2f} ms each): raise DELAY_MS"

    S = torch.cuda.Stream()
    P, done = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(S):
        delay.enqueue()
        for k in inp:
            inp[k].copy_(stage[k], non_blocking=True)
        for t in out.values():
            _bytes(t).fill_(SENTINEL)
        P.record(S)
        pending = not P.query()
        print(f"{name}: not P.query() = {pending}")
        assert pending, "the producer had finished before the call: the delay is too short for this host (raise DELAY_MS)"
        host = call(inp, out, S.cuda_stream)
        clones = {k: t.clone() for k, t in out.items()}
        if grab is not None:
            clones.update(grab(host, S.cuda_stream))
        for k in inp:
            inp[k].copy_(dec[k], non_blocking=True)
        done.record(S)
    done.synchronize()
    first = {k: t.cpu().numpy() for k, t in clones.items()}
    torch.cuda.synchronize()
    final = {k: t.cpu().numpy() for k, t in out.items()}
    if grab is not None:
        final.update({k: t.cpu().numpy() for k, t in grab(host, 0).items()})
    return first, final, host


def assert_outputs(case, got, what, want=None):
    want = case.want if want is None else want
    for k, w in want.items():
        if isinstance(w, dict):
            continue
        g, v = got[k], case.valid.get(k)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: output {k}: {g.dtype}{g.shape}, the reference has {w.dtype}{w.shape}"
        if v is not None:
            g, w = g[v], w[v]
        bad = np.flatnonzero((soc.bits(g) != soc.bits(w)).reshape(len(g), -1).any(axis=1)) if g.size else []
        assert len(bad) == 0, f"{what}: output {k}: {len(bad)} of {len(g)} items differ from the reference, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"


def run_case(name, case, call, delay, stats=None, outs=None, grab=None):
    """ordered() on a case, both reads of the outputs against the reference, the counters against the model"""
    tensors = {k: v for k, v in case.want.items() if not isinstance(v, dict)}      # (a dict is a record the call returns on the host)
    first, final, host = ordered(name, case.inputs, case.decoy, tensors if outs is None else outs, call, delay, grab)
    assert_outputs(case, first, "clones made on the caller's stream behind the call")
    assert_outputs(case, final, "output tensors after a device synchronisation")
    if stats is not None:
        got = stats()
        assert {k: got[k] for k in case.stats} == case.stats, (got, case.stats, "the decoy's: %s" % case.decoy_stats)
    return host


# ------------------------------------------------------------------------------------------------------------ control
def _control_case():
    rng = np.random.default_rng(1)
    real = rng.integers(0, 1 << 20, 1 << 16).astype(np.int32)
    decoy = real + (1 << 24)
    return soc.Case(dict(a=real), dict(a=decoy), dict(r=real * 3 + 1), dict(r=decoy * 3 + 1))


def test_control_contract_kept(delay):
    """the stand-in on the caller's stream: the real numbers, both times"""
    case = _control_case()

    def call(inp, out, stream):
        import torch
        torch.add(inp["a"] * 3, 1, out=out["r"])          # (ordered() makes the caller's stream the current one)
    run_case("control-kept", case, call, delay)


def test_control_early_read_reports_the_decoy(delay):
    """the stand-in reads its input on a second stream that does not wait for the caller's (a planning copy on the wrong stream)
    and stores on the caller's: the harness sees the decoy's numbers"""
    import torch
    case = _control_case()
    side = torch.cuda.Stream()

    def call(inp, out, stream):
        s = torch.cuda.current_stream()                     # (ordered() makes the caller's stream the current one)
        with torch.cuda.stream(side):
            tmp = inp["a"] * 3 + 1
            ev = torch.cuda.Event(); ev.record(side)
        with torch.cuda.stream(s):
            s.wait_event(ev)
            out["r"].copy_(tmp)
            tmp.record_stream(s)
    first, final, _ = ordered("control-early-read", case.inputs, case.decoy, case.want, call, delay)
    np.testing.assert_array_equal(first["r"], case.decoy_want["r"])
    np.testing.assert_array_equal(final["r"], case.decoy_want["r"])
    with pytest.raises(AssertionError, match="differ from the reference"):
        assert_outputs(case, first, "control")


def test_control_early_write_reports_the_sentinel(delay):
    """the stand-in computes and stores on a second stream that does not wait for the caller's: the fill behind the delay wipes it"""
    import torch
    case = _control_case()
    side = torch.cuda.Stream()

    def call(inp, out, stream):
        s = torch.cuda.current_stream()                     # (ordered() makes the caller's stream the current one)
        with torch.cuda.stream(side):
            torch.add(inp["a"] * 3, 1, out=out["r"])
            ev = torch.cuda.Event(); ev.record(side)
        s.wait_event(ev)
    first, final, _ = ordered("control-early-write", case.inputs, case.decoy, case.want, call, delay)
    assert (first["r"] == 0x5A5A5A5A).all() and (final["r"] == 0x5A5A5A5A).all()


def test_control_missing_join_reports_the_decoy(delay):
    """the stand-in forks a second stream from the caller's and never joins it; the second stream is slow to start: it reads the
    decoy the harness wrote behind the call, and the clones made on the caller's stream hold the sentinel"""
    import torch
    case = _control_case()
    side = torch.cuda.Stream()
    warm = []

    def call(inp, out, stream):
        s = torch.cuda.current_stream()                     # (ordered() makes the caller's stream the current one)
        ev = torch.cuda.Event(); ev.record(s)
        with torch.cuda.stream(side):
            side.wait_event(ev)
            if len(warm) >= 2:                     # (the two warm-up calls are timed: no delay in them)
                delay.enqueue()
            torch.add(inp["a"] * 3, 1, out=out["r"])
        warm.append(1)
    first, final, _ = ordered("control-missing-join", case.inputs, case.decoy, case.want, call, delay)
    assert (first["r"] == 0x5A5A5A5A).all()
    np.testing.assert_array_equal(final["r"], case.decoy_want["r"])


# ------------------------------------------------------------------------------------------------------------ bsw
@pytest.fixture(scope="module")
def bsw():
    from genarchbench_amd.bsw import BandedPairWiseSW
    h = BandedPairWiseSW()
    yield h
    h.close()


@pytest.mark.parametrize("full", [False, True], ids=["score", "result"])
@pytest.mark.parametrize("form", ["one_launch", "multi_class", "sliced"])
def test_bsw_run_device(bsw, delay, monkeypatch, capfd, form, full):
    """the one-launch form, the class launches over the caller's and the aux stream, and a sliced call over all three streams; the
    GAB_BSW_TRACE lines say that the form is the one meant"""
    case = soc.bsw_case(form, full)
    monkeypatch.setenv("GAB_BSW_TRACE", "1")
    if case.host["slice"]:
        monkeypatch.setenv("GAB_BSW_SLICE", "%d,%d" % case.host["slice"])
    else:
        monkeypatch.delenv("GAB_BSW_SLICE", raising=False)
    names = ("ref", "ref_off", "qry", "qry_off", "len1", "len2", "h0")

    def call(inp, out, stream):
        bsw.run_device(*(inp[k] for k in names), out["score"], out.get("result"), stream=stream)
    capfd.readouterr()
    run_case(f"bsw-{form}-{'result' if full else 'score'}", case, call, delay, stats=bsw.last_stats)
    cap = capfd.readouterr()
    print(cap.out)
    lines = [l for l in cap.err.splitlines() if l.startswith("[gab_bsw_dp")]
    per_call = len(lines) // 3
    assert len(lines) == 3 * per_call and per_call >= 1
    sliced = [l for l in lines if " slice " in l]
    if form == "one_launch":
        assert per_call == 1 and not sliced, lines
    elif form == "multi_class":
        assert per_call > 2 and not sliced, lines
    else:
        assert len(sliced) == len(lines) and any(l.endswith("slice 1") for l in lines) and per_call > 4, lines


# ------------------------------------------------------------------------------------------------------------ chain
@pytest.fixture(scope="module")
def chain():
    from genarchbench_amd.chain import ChainEngine
    e = ChainEngine()
    yield e
    e.close()


@pytest.mark.parametrize("through", [False, True], ids=["run_device", "through"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dispatch", list(CHAIN_DISPATCH))
def test_chain_run_device(chain, delay, monkeypatch, dispatch, mode, through):
    """both entry points, both modes, under the default rule and each of the three pins, on the mixed batch of
    tests/test_chain_forms_gpu.py: the results (also those written through to the host), the split against the model, and for
    fast-chain the predecessor evaluations against the oracle's"""
    case = soc.chain_case(mode)
    env = CHAIN_DISPATCH[dispatch]
    for k in CHAIN_SPLIT_KNOBS + ("GAB_CHAIN_TRACE", "GAB_CHAIN_TAB_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    call_off, hdr = case.host["call_off"], case.host["hdr"]

    def call(inp, out, stream):
        if through:
            return chain.run_device_through(mode, inp["x"], inp["y"], call_off, hdr, out["score"], out["parent"], stream=stream)
        chain.run_device(mode, inp["x"], inp["y"], call_off, hdr, out["score"], out["parent"], stream=stream)
    host = run_case(f"chain-{'through' if through else 'device'}-mode{mode}-{dispatch}", case, call, delay)
    if through:
        np.testing.assert_array_equal(host[0], case.want["score"]); np.testing.assert_array_equal(host[1], case.want["parent"])
    if mode == 1:
        assert chain.last_stats()["evals"] == case.stats["evals"], (chain.last_stats(), case.stats, case.decoy_stats)
    form, _ = chain.last_split(len(hdr))
    if not through:      # (the written-through entry point has no standing floors: tests/util.py, chain_split_model)
        np.testing.assert_array_equal(np.where((form == 4) | (form == 5), 3, form), chain_split_model(hdr["n"], mode, env))


# ------------------------------------------------------------------------------------------------------------ bpm, bitpal, wfa
PAIR_NAMES = ("pat", "pat_off", "pat_len", "txt", "txt_off", "txt_len")


def test_bpm_run_device(delay):
    """every register class has unclean pairs, so every class's band kernel runs on the handle's second stream"""
    from genarchbench_amd.bpm import BpmEngine
    case = soc.bpm_case()
    eng = BpmEngine()
    try:
        run_case("bpm", case, lambda inp, out, stream: eng.run_device(*(inp[k] for k in PAIR_NAMES), out["score"], stream=stream), delay,
                 stats=eng.last_stats)
    finally:
        eng.close()


@pytest.mark.parametrize("algorithm", [0, 1], ids=["edit", "scored"])
def test_bitpal_run_device(delay, algorithm):
    from genarchbench_amd.bitpal import BitpalEngine
    case = soc.bitpal_case(algorithm)
    eng = BitpalEngine(algorithm)
    try:
        run_case(f"bitpal-{algorithm}", case, lambda inp, out, stream: eng.run_device(*(inp[k] for k in PAIR_NAMES), out["score"], stream=stream),
                 delay, stats=eng.last_stats)
    finally:
        eng.close()


def test_wfa_run_device(delay):
    """a batch whose pairs reach a second tier (the model says so, and `requeued` of the call)"""
    from genarchbench_amd.wfa import AffineWavefronts
    case = soc.wfa_case()
    eng = AffineWavefronts()

    def call(inp, out, stream):
        eng.run_device(*(inp[k] for k in PAIR_NAMES), out["ops"], inp["ops_off"], out["ops_len"], out["score"], stream=stream)
    try:
        run_case("wfa", case, call, delay, stats=eng.last_stats)
        assert eng.last_stats()["requeued"] >= 1
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ kmer
@pytest.fixture(scope="module")
def kmer():
    from genarchbench_amd.kmer import KmerCounter
    h = KmerCounter()
    yield h
    h.close()


@pytest.mark.parametrize("which", soc.KMER_ENTRIES)
def test_kmer_device(kmer, delay, which):
    """the seven device entry points; every one copies off / len to the host for its plan.  index_part: begin and finish are one
    call here -- the finish runs on the caller's stream and reads `len` again, so the decoy goes over the inputs behind the finish.
    Afterwards the handle's table or index is the model's."""
    case = soc.kmer_case(which)
    k, w, ml, s = soc.KMER_K, soc.KMER_WINDOW, soc.KMER_MIN_LEN, soc.KMER_SOLID

    def call(inp, out, stream):
        a = (inp["seq"], inp["off"], inp["len"])
        if which == "count":
            return dict(res=kmer.count_device(*a, k, ml, stream))
        if which == "count_part":
            return dict(res=kmer.count_part_device(*a, k, soc.KMER_PART, soc.KMER_NPARTS, ml, stream))
        if which == "index_minimizers":
            return dict(res=kmer.index_minimizers_device(*a, k, w, soc.KMER_RATE, ml, stream))
        if which == "index_part":
            begun = kmer.index_part_begin_device(*a, k, w, soc.KMER_PART, soc.KMER_NPARTS, ml, stream)
            return dict(res=begun, res2=kmer.index_part_finish(case.host["minimizers"], case.host["distinct"], soc.KMER_RATE))
        if which == "index_solid":
            return dict(res=kmer.index_solid_device(*a, k, s["min_freq"], s["select_rate"], s["tandem_freq"], s["rate"], ml, stream))
        if which == "sketch":
            rc, n = kmer.sketch_device(*a, k, w, out["read_start"], out["pos"], ml, stream)
        else:
            rc, n = kmer.solid_positions_device(*a, k, out["read_start"], out["pos"], s["min_freq"], s["select_rate"], s["tandem_freq"], ml, stream)
        assert rc == 0
        return dict(res=dict(nout=n))
    host = run_case(f"kmer-{which}", case, call, delay, stats=kmer.last_stats if case.stats else None)
    for key in ("res", "res2"):
        if key in case.want:
            assert host[key] == case.want[key], (key, host[key], case.want[key], "the decoy's: %s" % case.decoy_want[key])
    if "table" in case.want:
        dk, dc = kmer.dump()
        assert dk.tolist() == case.want["table"]["kmers"] and dc.tolist() == case.want["table"]["counts"]
    if "index" in case.want:
        got = dict(zip(("kmers", "start", "gpos"), (a.tolist() for a in kmer.index_dump())))
        assert got == case.want["index"]


# ------------------------------------------------------------------------------------------------------------ abea
@pytest.fixture(scope="module")
def aligner():
    from genarchbench_amd.abea import EventAligner
    h = EventAligner(*soc.abea_model_and_reads()[0])
    yield h
    h.close()


@pytest.mark.parametrize("which", soc.ABEA_ENTRIES)
def test_abea_device(aligner, delay, which):
    """align, events, scalings, calibrate: records and floats bit for bit (a NaN by its bit pattern), the room behind pairs, event
    slabs and map untouched"""
    case = soc.abea_case(which)
    reads = ("seq", "seq_off", "seq_len", "events", "event_off", "n_events")

    def call(inp, out, stream):
        if which == "align":
            aligner.align_device(*(inp[k] for k in reads), inp["scale"], inp["shift"], out["pairs"], inp["pair_off"], out["res"], stream=stream)
        elif which == "events":
            rc = aligner.detect_events_device(*(inp[k] for k in ("raw", "raw_off", "n_samples", "range", "digitisation", "offset")),
                                              *(out[k] for k in ("n_events", "event_off", "mean", "stdv", "start", "length", "total")), stream=stream)
            assert rc == 0
        elif which == "scalings":
            aligner.estimate_scalings_device(*(inp[k] for k in reads), out["scale"], out["shift"], stream=stream)
        else:
            aligner.calibrate_device(*(inp[k] for k in reads), inp["scale"], inp["shift"], inp["pairs"], inp["pair_off"], inp["n_pairs"],
                                     out["map"], inp["map_off"], out["res"], stream=stream)
    stats = {"align": aligner.last_stats, "events": aligner.events_last_stats, "scalings": aligner.scalings_last_stats,
             "calibrate": aligner.calibrate_last_stats}[which]
    run_case(f"abea-{which}", case, call, delay, stats=stats)


# ------------------------------------------------------------------------------------------------------------ outputs in the handle's memory
_hip = []


def from_handle(ptr, count, dtype, stream):
    """`count` items of numpy dtype `dtype` at device address `ptr` -> a new tensor, copied on `stream` (a raw hipStream_t value);
    how a caller reads an output that lies in memory of the handle without waiting for the device"""
    import ctypes as C
    import torch
    if not _hip:
        _hip.append(C.CDLL("libamdhip64.so"))
    nbytes = int(count) * np.dtype(dtype).itemsize
    t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda:0")
    if nbytes:
        assert ptr, "the entry point returned no address"
        assert _hip[0].hipMemcpyAsync(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), C.c_int(3), C.c_void_p(stream)) == 0
    t = t[:nbytes]
    return t if np.dtype(dtype).itemsize == 1 else t.view(torch.from_numpy(np.empty(0, dtype)).dtype)


# ------------------------------------------------------------------------------------------------------------ fmi
@pytest.fixture(scope="module")
def fmi():
    from genarchbench_amd.fmi import FMI_search
    idx = soc.fmi_index()[0]
    f = FMI_search(arrays=(idx.ref_seq_len, idx.count, idx.cp_occ, idx.sentinel_index))
    f.set_sa(idx.sa_ms_byte, idx.sa_ls_word)
    yield f
    f.close()


def test_fmi_seed_device(fmi, delay):
    """the records and read_off lie in the handle: they are copied out of it on the caller's stream right behind the call"""
    case = soc.fmi_case("seed")
    nreads = len(case.inputs["len"])

    def grab(host, stream):
        d_out, d_off, n = host
        smems = from_handle(d_out, n * 40, np.uint8, stream).reshape(n, 40)
        smems[:, 12:16] = 0          # (`pad` is not part of the result; on the current stream, which is the one the copy went to)
        return dict(smems=smems, read_off=from_handle(d_off, nreads + 1, np.int64, stream))
    host = run_case("fmi-seed", case, lambda inp, out, stream: fmi.seed_device(inp["enc"], inp["len"], soc.FMI_MIN_SEED_LEN, stream=stream), delay,
                    stats=fmi.last_stats, grab=grab)
    assert host[2] == case.want["res"]["nout"]


def test_fmi_sa_lookup_device(fmi, delay):
    case = soc.fmi_case("sa_lookup")
    n = len(case.inputs["smems"])

    def grab(host, stream):
        co, off, total = host
        return dict(coords=from_handle(co, total, np.int64, stream), coord_off=from_handle(off, n + 1, np.int64, stream))
    host = run_case("fmi-sa_lookup", case, lambda inp, out, stream: fmi.get_sa_entries_device(inp["smems"].data_ptr(), n, soc.FMI_MAX_OCC, stream=stream),
                    delay, stats=fmi.last_sa_stats, grab=grab)
    assert host[2] == case.want["res"]["total"]


# ------------------------------------------------------------------------------------------------------------ parse
@pytest.fixture(scope="module")
def parser():
    from genarchbench_amd.parse import InputParser
    p = InputParser()
    yield p
    p.close()


@pytest.mark.parametrize("which", soc.PARSERS)
def test_parse_device(parser, delay, which):
    """the three parsers on a text that is still being copied into place.  Their outputs lie in the parser's memory; the chain call
    table comes back on the host, complete when the call returns"""
    import ctypes as C
    from tests import parse_cases as pc
    from tools.gabgen import CHAIN_HDR
    case = soc.parse_case(which)
    nbytes, counts = case.host["nbytes"], case.host["counts"]

    def call(inp, out, stream):
        addr = inp["text"].data_ptr()
        if which == "bsw":
            pk = parser.bsw_pairs_device(addr, nbytes, stream)
            assert pk.n == counts["n"]
            return pk, None
        if which == "pairs":
            pk = parser.pairs_device(addr, nbytes, True, stream)
            assert (pk.n, pk.cap_bytes) == (counts["n"], counts["cap_bytes"]) and pk.d_text == addr and pk.text_bytes == nbytes
            return pk, None
        pk = parser.chain_device(addr, nbytes, stream)
        assert (pk.ncalls, pk.total) == (counts["ncalls"], counts["total"])
        table = dict(call_off=np.ctypeslib.as_array(pk.call_off, shape=(pk.ncalls + 1,)).tolist(),
                     hdr=np.ctypeslib.as_array(C.cast(pk.hdr, C.POINTER(C.c_uint8)), shape=(pk.ncalls * CHAIN_HDR.itemsize,)).copy().view(CHAIN_HDR).tolist())
        return pk, table

    def grab(host, stream):
        pk = host[0]
        if which == "bsw":
            n = counts["n"]
            got = {f: from_handle(getattr(pk, "d_" + f), n, dt, stream) for f, dt in (("len1", np.int32), ("len2", np.int32), ("h0", np.int32), ("ref_off", np.int64), ("qry_off", np.int64))}
            got["ref"] = from_handle(pk.d_ref, pk.ref_bytes, np.uint8, stream); got["qry"] = from_handle(pk.d_qry, pk.qry_bytes, np.uint8, stream)
            return got
        if which == "pairs":
            n = counts["n"]
            return {f: from_handle(getattr(pk, "d_" + f), n + (f == "cap_off"), dt, stream)
                    for f, dt in (("pat_off", np.int64), ("txt_off", np.int64), ("pat_len", np.int32), ("txt_len", np.int32), ("cap_off", np.int64))}
        return dict(x=from_handle(pk.d_x, counts["total"], np.int64, stream), y=from_handle(pk.d_y, counts["total"], np.int64, stream))
    first, final, host = ordered(f"parse-{which}", case.inputs, case.decoy, {}, call, delay, grab)
    if which == "chain":
        assert host[1] == case.want["res"], "the call table on the host"
    for what, got in (("copies made on the caller's stream behind the call", first), ("the parser's arrays after a device synchronisation", final)):
        if which == "bsw":          # the code slabs: every sequence where the reference puts it (between them the slab holds anything)
            for slab, off, ln in (("ref", "ref_off", "len1"), ("qry", "qry_off", "len2")):
                o, k = case.want[off], case.want[ln]
                assert len(got[slab]) >= int((o + k).max()), (slab, len(got[slab]))
                got[slab] = soc.words16(pc.gather(got[slab], o, k))
        assert_outputs(case, got, what)
