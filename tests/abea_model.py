"""Model of the adaptive banded event alignment (include/gab.h: gab_abea_align) in numpy.float32 / Python float arithmetic, written from
the rules of the kernel's contract, and the seeded generator of its test reads.  No GPU, no library.

Arithmetic: an fp32 operation is one numpy.float32 operation (rounded on its own, no fused multiply-add); a mixed expression widens
its fp32 operands to Python float (double), sums left to right and rounds to fp32 once.  The cells of one band do not depend on each
other, so a band is computed as arrays, element by element the same operations as a scalar loop."""
import math

import numpy as np

F = np.float32
K, BW, NKMER = 6, 100, 4096
FROM_D, FROM_U, FROM_L = 0, 1, 2
LOW_EMISSION, NOT_SPANNED, GAP, NO_END = 1, 2, 4, 8
NEG = F(-np.inf)
_RANK = np.zeros(256, np.int64)
for _i, _c in enumerate(b"ACGT"):
    _RANK[_c] = _i                       # every other byte, lower case included, ranks as 'A'


def kmer_ranks(seq):
    r = _RANK[np.frombuffer(bytes(seq), np.uint8)]
    n = r.size - K + 1
    out = np.zeros(n, np.int64)
    for t in range(K):
        out = out * 4 + r[t:t + n]
    return out


def log_stdv_of(stdv):
    """what a NULL level_log_stdv means: the double log of the float, rounded to float"""
    return np.array([math.log(float(s)) for s in np.asarray(stdv, F)], F)


def _emission(ev, gp_mean, stdv, log_stdv):
    a = (ev - gp_mean) / stdv
    return (F(-0.918938) - log_stdv) + ((F(-0.5) * a) * a)


def align(seq, events, mean, stdv, log_stdv, scale, shift):
    """-> (record dict with the fields of gab_abea_read, path as an (path_len, 2) int32 array of (ref_pos, read_pos) in read order)"""
    events = np.asarray(events, F)
    n_events, n_kmers = events.size, len(seq) - K + 1
    assert n_kmers >= 1 and n_events >= 1
    ranks = kmer_ranks(seq)
    gp_mean = F(scale) * np.asarray(mean, F)[ranks] + F(shift)
    k_stdv, k_lstd = np.asarray(stdv, F)[ranks], np.asarray(log_stdv, F)[ranks]
    assert gp_mean.dtype == F and k_stdv.dtype == F and k_lstd.dtype == F

    events_per_kmer = n_events / n_kmers
    p_stay = 1 - 1 / (events_per_kmer + 1)
    lp_skip = math.log(1e-10)
    lp_stay = math.log(p_stay)
    lp_step = math.log(1.0 - math.exp(lp_skip) - math.exp(lp_stay))
    lp_trim = math.log(0.01)

    n_bands = n_events + n_kmers + 2
    trace = np.zeros((n_bands, BW), np.uint8)
    ll_event = np.zeros(n_bands, np.int64); ll_kmer = np.zeros(n_bands, np.int64)      # lower-left corner of every band
    ll_event[0], ll_kmer[0] = BW // 2 - 1, -1 - BW // 2
    ll_event[1], ll_kmer[1] = ll_event[0] + 1, ll_kmer[0]
    # a band with one guard cell of -inf on either side: cell o at [o + 1]
    prev2 = np.full(BW + 2, NEG, F); prev2[1 + BW // 2] = F(0.0)           # band 0: the start cell
    prev = np.full(BW + 2, NEG, F); prev[1 + BW // 2] = F(lp_trim)         # band 1: the first event trimmed
    end_cells = {}                                                         # event -> score of (event, last k-mer) where in band
    fills = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(2, n_bands):
            ll, ur = prev[1], prev[BW]
            if ll == NEG and ur == NEG:
                right = b % 2 == 1
            else:
                right = bool(ll < ur)
            E, Kl = (ll_event[b - 1], ll_kmer[b - 1] + 1) if right else (ll_event[b - 1] + 1, ll_kmer[b - 1])
            ll_event[b], ll_kmer[b] = E, Kl
            cur = np.full(BW + 2, NEG, F)
            t = -1 - Kl                                                    # the trim column's cell
            if 0 <= t < BW and 0 <= E - t < n_events:
                cur[1 + t] = F(lp_trim * (E - t + 1)); trace[b, t] = FROM_U
            lo, hi = max(-Kl, E - (n_events - 1), 0), min(n_kmers - Kl, E + 1, BW)
            if lo < hi:
                o = np.arange(lo, hi)
                e, k = E - o, Kl + o
                if right:
                    up, left = prev[1 + o + 1], prev[1 + o]
                else:
                    up, left = prev[1 + o], prev[1 + o - 1]
                diag = prev2[1 + o + (Kl - ll_kmer[b - 2]) - 1]
                lp = _emission(events[e], gp_mean[k], k_stdv[k], k_lstd[k])
                assert lp.dtype == F
                s_d = ((diag.astype(np.float64) + lp_step) + lp.astype(np.float64)).astype(F)
                s_u = ((up.astype(np.float64) + lp_stay) + lp.astype(np.float64)).astype(F)
                s_l = (left.astype(np.float64) + lp_skip).astype(F)
                m = s_d; f = np.full(o.size, FROM_D, np.uint8)
                m = np.where(s_u > m, s_u, m); f = np.where(m == s_u, FROM_U, f)
                m = np.where(s_l > m, s_l, m); f = np.where(m == s_l, FROM_L, f)      # three -inf inputs: FROM_L
                cur[1 + lo:1 + hi] = m; trace[b, lo:hi] = f
                fills += hi - lo
            e_end = b - 1 - n_kmers
            o_end = n_kmers - 1 - Kl
            if e_end >= 0 and 0 <= o_end < BW:
                end_cells[e_end] = cur[1 + o_end]
            prev2, prev = prev, cur

    rec = dict(n_pairs=0, path_len=0, end_event=0, max_gap=0, flags=0, avg_log_emission=0.0, fills=int(fills))
    best, end_event = NEG, 0
    for e in range(n_events):                                              # strict >: the lowest event wins a tie
        if e in end_cells:
            s = F(float(end_cells[e]) + (n_events - e) * lp_trim)
            if s > best:
                best, end_event = s, e
    if best == NEG:                                                        # the defined deviation: nothing to start from
        rec["flags"] = NO_END
        return rec, np.zeros((0, 2), np.int32)

    path = []
    e, k = end_event, n_kmers - 1
    total, gap, max_gap = 0.0, 0, 0
    while k >= 0 and e >= 0:
        path.append((k, e))
        total += float(_emission(events[e], gp_mean[k], k_stdv[k], k_lstd[k]))
        b = e + k + 2
        o = int(ll_event[b] - e)
        assert o == k - ll_kmer[b] and 0 <= o < BW
        f = trace[b, o]
        if f == FROM_D:
            k -= 1; e -= 1; gap = 0
        elif f == FROM_U:
            e -= 1; gap = 0
        else:
            k -= 1; gap += 1; max_gap = max(max_gap, gap)
    path.reverse()
    avg = total / len(path)
    flags = 0
    if avg < -5.0:
        flags |= LOW_EMISSION
    if not (path[0][0] == 0 and path[-1][0] == n_kmers - 1):
        flags |= NOT_SPANNED
    if max_gap > 50:
        flags |= GAP
    rec.update(n_pairs=0 if flags else len(path), path_len=len(path), end_event=int(end_event), max_gap=int(max_gap), flags=flags,
               avg_log_emission=avg)
    return rec, np.array(path, np.int32).reshape(-1, 2)


# ---- generator ---------------------------------------------------------------------------------------------------------------------
def make_model(rng):
    """a random pore model: mean 60..130, stdv 1..3.5, log stdv as the library derives it"""
    mean = rng.uniform(60.0, 130.0, NKMER).astype(F)
    stdv = rng.uniform(1.0, 3.5, NKMER).astype(F)
    return mean, stdv, log_stdv_of(stdv)


def scalings_by_moments(seq, events, mean):
    """method of moments over the events and the levels of the read's k-mers, in double, rounded to float: (scale, shift)"""
    levels = np.asarray(mean, F)[kmer_ranks(seq)].astype(np.float64)
    ev = np.asarray(events, F).astype(np.float64)
    shift = ev.sum() / ev.size - levels.sum() / levels.size
    scale = (((ev - shift) ** 2).sum() / ev.size) / ((levels * levels).sum() / levels.size)
    return F(scale), F(shift)


EVENTS_PER_KMER = (0.01, 0.54, 0.30, 0.15)      # probability of 0, 1, 2, 3..6 events on a k-mer


def make_events(rng, seq, mean, stdv, probs=EVENTS_PER_KMER, counts=None):
    """events of a read: per k-mer a number of events (drawn by `probs`, or given in `counts`), each sc * mean + sh + N(0, 1) * stdv
    with one sc = 1 + 0.01 N and one sh = 5 N per read"""
    ranks = kmer_ranks(seq)
    if counts is None:
        kind = rng.choice(4, ranks.size, p=probs)
        counts = np.where(kind == 3, rng.integers(3, 7, ranks.size), kind)
    counts = np.asarray(counts, np.int64)
    if counts.sum() == 0:
        counts[0] = 1
    sc, sh = 1.0 + 0.01 * rng.standard_normal(), 5.0 * rng.standard_normal()
    of = np.repeat(ranks, counts)
    m, s = np.asarray(mean, F)[of].astype(np.float64), np.asarray(stdv, F)[of].astype(np.float64)
    return (sc * m + sh + rng.standard_normal(of.size) * s).astype(F)


def make_read(rng, n_bases, mean, stdv, probs=EVENTS_PER_KMER, counts=None):
    """-> (bases, events, scale, shift), the scalings by the method of moments"""
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n_bases).tolist())
    events = make_events(rng, seq, mean, stdv, probs, counts)
    scale, shift = scalings_by_moments(seq, events, mean)
    return seq, events, scale, shift


def make_gap_read(rng, mean, stdv, lead=60, flank=80, run=55):
    """a read that fails the gap check: `run` k-mers without events between two flanks of one event per k-mer, so that a path has no
    spare event to spend inside the run and crosses it in one run of skips; three events per k-mer on the far leads keep
    n_events above n_kmers"""
    n_kmers = 2 * lead + 2 * flank + run
    counts = np.full(n_kmers, 1); counts[:lead] = 3; counts[-lead:] = 3; counts[lead + flank:lead + flank + run] = 0
    return make_read(rng, n_kmers + K - 1, mean, stdv, counts=counts)


def pairs_digest(path):
    """hash of a path as the fixtures record it: sha256 of its little-endian int32 (ref_pos, read_pos) pairs, first 16 hex digits"""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(path, "<i4").tobytes()).hexdigest()[:16]
