"""Model of abea's event detection and scaling estimate (include/gab.h: gab_abea_events, gab_abea_scalings) in numpy.float32 /
numpy.float64 arithmetic, written from the rules of the contract, and the seeded generator of its test signals.  No GPU, no library.

Arithmetic: an fp32 operation is one numpy.float32 operation and an fp64 operation one numpy.float64 operation, each rounded on
its own (no fused multiply-add).  The prefix sums are numpy.add.accumulate, which adds one element after the other in index order
(prefix_sums_by_loop is the same thing as a Python loop; the tests compare the two).  The t-statistic of one position does not
depend on that of another, so it is computed as arrays: element by element the operations of a scalar loop.  The peak detector
walks the samples one by one."""
import hashlib
import math

import numpy as np

import abea_model as A

F, D = np.float32, np.float64
K = A.K
FLT_MAX, FLT_MIN = np.finfo(F).max, np.finfo(F).tiny
PEAK_HEIGHT = F(0.2)
WINDOW = (3, 6)
THRESHOLD = (F(1.4), F(9.0))


def to_pa(raw, rng_, digitisation, offset):
    """(raw + offset) * (range / digitisation), all in float"""
    unit = F(rng_) / F(digitisation)
    return (np.asarray(raw, F) + F(offset)) * unit


# ---- sums ------------------------------------------------------------------------------------------------------------------------
def prefix_sums(x):
    """sum[i + 1] = sum[i] + x[i] and sumsq[i + 1] = sumsq[i] + (double)(x[i] * x[i]), the product in float; n + 1 entries each"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        s = np.concatenate([[D(0)], np.add.accumulate(x.astype(D))])
        q = np.concatenate([[D(0)], np.add.accumulate((x * x).astype(D))])
    return s, q


def prefix_sums_by_loop(x):
    x = np.asarray(x, F)
    s, q = np.zeros(x.size + 1, D), np.zeros(x.size + 1, D)
    with np.errstate(all="ignore"):
        for i in range(x.size):
            s[i + 1] = s[i] + D(x[i])
            q[i + 1] = q[i] + D(x[i] * x[i])
    return s, q


def grid_of(addends):
    """floats -> (emax, q): every one is a multiple of 2^q and smaller than 2^(emax + 1) in magnitude; None for a NaN, an infinity
    or a denormal; (None, None) when all are zero"""
    v = np.asarray(addends, F)
    bits = v.view(np.uint32).astype(np.int64)
    e, m = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    if np.any(e == 255) or np.any((e == 0) & (m != 0)):
        return None
    nz = e != 0
    if not nz.any():
        return None, None
    sig = m[nz] | 0x800000
    tz = np.array([(int(t) & -int(t)).bit_length() - 1 for t in sig])
    return int((e[nz] - 127).max()), int((e[nz] - 127 - 23 + tz).min())


def exact_in_any_order(n, grid, squared=False):
    """n addends on `grid` (or their squares taken in double, which are exact: grid 2^(2q), size below 2^(2 emax + 2)): is n * 2^(emax + 1),
    a bound on the sum of the magnitudes, at most 2^(q + 53)?  Zeros add nothing."""
    if grid is None:
        return False
    emax, q = grid
    if emax is None:
        return True
    if squared:
        emax, q = 2 * emax + 1, 2 * q
    return int(n).bit_length() + emax + 1 <= q + 53


def order_free(addends):
    """the proof that a double sum of these floats is exact in any order: every addend a multiple of 2^q, and the sum of the
    magnitudes below 2^(q + 53).  A NaN, an infinity or a denormal refuses."""
    return exact_in_any_order(np.size(addends), grid_of(addends))


def sums_are_wide(x):
    """what the library decides per read (reads_serial_sums counts the reads for which this is False)"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return order_free(x) and order_free(x * x)


def pairwise_sum(v):
    """a double sum in tree order, the opposite of the reference's"""
    v = np.asarray(v, D)
    with np.errstate(all="ignore"):
        while v.size > 1:
            if v.size % 2:
                v = np.concatenate([v, [D(0)]])
            v = v[0::2] + v[1::2]
    return v[0] if v.size else D(0)


# ---- t-statistic -------------------------------------------------------------------------------------------------------------------
def tstat(s, q, n, w):
    """compute_tstat: zeros for the first w positions, for those after n - w, and everywhere when n < 2 w"""
    t = np.zeros(n, F)
    if n < 2 * w:
        return t
    i = np.arange(w, n - w + 1)
    wf, wd = F(w), D(F(w))
    with np.errstate(all="ignore"):
        first = i > w
        sum1 = np.where(first, s[i] - s[np.maximum(i - w, 0)], s[i])
        sumsq1 = np.where(first, q[i] - q[np.maximum(i - w, 0)], q[i])
        sum2 = (s[i + w] - s[i]).astype(F)
        sumsq2 = (q[i + w] - q[i]).astype(F)
        mean1 = (sum1 / wd).astype(F)
        mean2 = sum2 / wf
        var = (((sumsq1 / wd - (mean1 * mean1).astype(D)) + (sumsq2 / wf).astype(D)) - (mean2 * mean2).astype(D)).astype(F)
        var = np.fmax(var, FLT_MIN)                                  # a NaN variance becomes FLT_MIN, as fmaxf gives it
        delta = mean2 - mean1
        out = np.abs(delta) / np.sqrt(var / wf)
    assert out.dtype == F and mean2.dtype == F and var.dtype == F
    t[w:n - w + 1] = out
    return t


# ---- detector ------------------------------------------------------------------------------------------------------------------
def cold_state():
    """[short, long]: masked_to, peak_pos, peak_value, valid_peak"""
    return [[0, -1, FLT_MAX, False], [0, -1, FLT_MAX, False]]


def detector_step(st, i, t1, t2, peaks):
    """one sample of the two detectors, short first; an emitted peak position is appended to `peaks`"""
    for k in (0, 1):
        d = st[k]
        if d[0] >= i:
            continue
        cur = t2 if k else t1
        if d[1] == -1:
            if cur < d[2]:
                d[2] = cur
            elif cur - d[2] > PEAK_HEIGHT:
                d[2] = cur; d[1] = i
        else:
            if cur > d[2]:
                d[2] = cur; d[1] = i
            if k == 0 and d[2] > THRESHOLD[0]:                       # the short detector knocks the long one out
                st[1][0] = d[1] + WINDOW[0]; st[1][1] = -1; st[1][2] = FLT_MAX; st[1][3] = False
            if d[2] - cur > PEAK_HEIGHT and d[2] > THRESHOLD[k]:
                d[3] = True
            if d[3] and i - d[1] > WINDOW[k] // 2:
                peaks.append(d[1])
                d[1] = -1; d[2] = cur; d[3] = False


def run_detector(t1, t2, lo=0, hi=None, state=None):
    """-> (peaks emitted at samples lo .. hi - 1 in emission order, the state after sample hi - 1)"""
    st = cold_state() if state is None else [list(state[0]), list(state[1])]
    peaks = []
    with np.errstate(all="ignore"):
        for i in range(lo, len(t1) if hi is None else hi):
            detector_step(st, i, t1[i], t2[i], peaks)
    return peaks, st


def same_state(a, b, nxt):
    """do two machines behave alike from sample `nxt` on?  masked_to counts only where it still masks a sample ahead"""
    for k in (0, 1):
        if a[k][1] != b[k][1] or F(a[k][2]).tobytes() != F(b[k][2]).tobytes() or a[k][3] != b[k][3]:
            return False
        if (a[k][0] >= nxt or b[k][0] >= nxt) and a[k][0] != b[k][0]:
            return False
    return True


def chunks_to_redo(t1, t2, chunk, warmup):
    """how many chunks a speculative run redoes: chunk c > 0 starts cold `warmup` samples before c * chunk, and stands only if its
    state at c * chunk is the true one"""
    n, redo = len(t1), 0
    _, true = run_detector(t1, t2, 0, min(chunk, n))
    for lo in range(chunk, n, chunk):
        _, cold = run_detector(t1, t2, lo - warmup, lo)
        redo += not same_state(true, cold, lo)
        _, true = run_detector(t1, t2, lo, min(lo + chunk, n), true)
    return redo


# ---- events ------------------------------------------------------------------------------------------------------------------
def create_event(start, end, s, q):
    with np.errstate(all="ignore"):
        length = F((end - start) % (1 << 64))                        # size_t arithmetic, as the reference has it
        mean = F(s[end] - s[start]) / length
        deltasqr = F(q[end] - q[start])
        var = deltasqr / length - mean * mean
        stdv = np.sqrt(np.fmax(var, F(0)))
    assert mean.dtype == F and stdv.dtype == F
    return start, length, mean, stdv


def detect_events(pa):
    """samples in pA -> dict(start int32, length, mean, stdv float32, peaks): getevents; with no peak one event over the read"""
    pa = np.asarray(pa, F)
    n = pa.size
    assert n >= 1
    s, q = prefix_sums(pa)
    t1, t2 = tstat(s, q, n, WINDOW[0]), tstat(s, q, n, WINDOW[1])
    peaks, _ = run_detector(t1, t2)
    assert all(0 < p < n for p in peaks)
    bounds = [0] + peaks + [n]
    ev = [create_event(bounds[i], bounds[i + 1], s, q) for i in range(len(bounds) - 1)]
    return dict(start=np.array([e[0] for e in ev], np.int32), length=np.array([e[1] for e in ev], F), mean=np.array([e[2] for e in ev], F),
                stdv=np.array([e[3] for e in ev], F), peaks=peaks, tstat=(t1, t2))


def events_of(raw, rng_, digitisation, offset):
    return detect_events(to_pa(raw, rng_, digitisation, offset))


def events_digest(ev):
    """sha256 over start (int32), length, mean, stdv (float32), little endian, first 16 hex digits"""
    h = hashlib.sha256()
    for name, dt in (("start", "<i4"), ("length", "<f4"), ("mean", "<f4"), ("stdv", "<f4")):
        h.update(np.ascontiguousarray(ev[name], dt).tobytes())
    return h.hexdigest()[:16]


# ---- scalings ------------------------------------------------------------------------------------------------------------------
def scalings(seq, event_mean, level_mean):
    """estimate_scalings_using_mom: four double sums in index order -> (scale, shift) as float"""
    ev = np.asarray(event_mean, F).astype(D)
    lv = np.asarray(level_mean, F)[A.kmer_ranks(seq)].astype(D)
    with np.errstate(all="ignore"):
        event_sum = np.add.accumulate(ev)[-1]
        kmer_sum = np.add.accumulate(lv)[-1]
        kmer_sq = np.add.accumulate(lv * lv)[-1]
        shift = event_sum / D(ev.size) - kmer_sum / D(lv.size)
        d = ev - shift
        event_sq = np.add.accumulate(d * d)[-1]
        scale = (event_sq / D(ev.size)) / (kmer_sq / D(lv.size))
    return F(scale), F(shift)


def scalings_in_order(seq, event_mean, level_mean):
    """which of the three sums the library must add in the reference's order for this read: (event means, k-mer levels, squared levels)"""
    lv = np.asarray(level_mean, F)[A.kmer_ranks(seq)]
    g = grid_of(lv)
    return (not order_free(event_mean), not exact_in_any_order(lv.size, g), not exact_in_any_order(lv.size, g, squared=True))


# ---- generator -------------------------------------------------------------------------------------------------------------------
RANGE, DIGITISATION = 1402.882, 8192.0               # pA over the ADC's span: a grid of about 0.17 pA


def make_signal(rng, n_samples, level_mean, noise=1.5, flat=None, plant=None, seq=None):
    """-> (ADC codes int16, range, digitisation, offset, bases).  Piecewise-constant levels of the pore model along random bases, a
    dwell of 3 + geometric samples per k-mer (about 9), Gaussian noise, quantised to the ADC grid.  flat = (first, length) writes
    a run of identical codes; plant = (index, value) is applied by with_planted on the float signal."""
    unit = RANGE / DIGITISATION
    offset = float(rng.integers(-20, 21))
    dwell = 3 + rng.geometric(1 / 6.0, n_samples // 3 + 2)
    dwell = dwell[:int(np.searchsorted(np.cumsum(dwell), n_samples)) + 1]
    bases = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), dwell.size + K - 1).tolist()) if seq is None else seq
    ranks = A.kmer_ranks(bases)[:dwell.size]
    level = np.repeat(np.asarray(level_mean, D)[ranks], dwell[:ranks.size])[:n_samples]
    if level.size < n_samples:
        level = np.concatenate([level, np.full(n_samples - level.size, level[-1])])
    pa = level + noise * rng.standard_normal(n_samples)
    codes = np.clip(np.rint(pa / unit - offset), -32768, 32767).astype(np.int16)
    if flat is not None:
        codes[flat[0]:flat[0] + flat[1]] = codes[flat[0]]
    return codes, F(RANGE), F(DIGITISATION), F(offset), bases


def tstats_of(codes, rng_, digitisation, offset):
    pa = to_pa(codes.astype(F), rng_, digitisation, offset)
    s, q = prefix_sums(pa)
    return tstat(s, q, pa.size, WINDOW[0]), tstat(s, q, pa.size, WINDOW[1])


def find_flat_run_read(level_mean, chunk, warmup, n_samples=None, seeds=range(200)):
    """-> (signal, seed): the first seed whose read, with a flat run of warmup + 236 samples that starts 200 samples before the
    boundary at `chunk`, leaves a cold start `warmup` samples before that boundary in another state than the true one there"""
    n = 2 * chunk + 100 if n_samples is None else n_samples
    for seed in seeds:
        sig = make_signal(np.random.default_rng(seed), n, level_mean, flat=(chunk - 200, warmup + 236))
        t1, t2 = tstats_of(*sig[:4])
        _, true = run_detector(t1, t2, 0, chunk)
        _, cold = run_detector(t1, t2, chunk - warmup, chunk)
        if not same_state(true, cold, chunk):
            return sig, seed
    raise AssertionError("no seed leaves a cold start in another state")


def with_planted(codes, rng_, digitisation, offset, index, value):
    """the read as float samples already in pA with one sample replaced: (raw, 1, 1, 0)"""
    pa = to_pa(codes.astype(F), rng_, digitisation, offset).copy()
    pa[index] = F(value)
    return pa, F(1), F(1), F(0)
