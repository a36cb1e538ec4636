"""Model of abea's base-to-event map, recalibration and read checks (include/gab.h: gab_abea_calibrate) in numpy.float64 arithmetic,
written from the rules of the contract, and the seeded generator of its constructed test reads.  No GPU, no library.

Arithmetic: every double operation is one numpy.float64 operation (rounded on its own, no fused multiply-add; a division by zero
gives an infinity or a NaN as in C), sums are loops in the reference's order, log_var is libm's log of the double var."""
import hashlib
import math

import numpy as np

import abea_model as A

F, D = np.float32, np.float64
K = A.K
FAILED_CALIBRATION, FAILED_ALIGNMENT, FAILED_QUALITY_CHK = 1, 2, 4
MIN_M_STATES = 200


def base_to_event_map(pairs, n_kmers):
    """-> (map as an (n_kmers, 2) int32 array of (start, stop), -1 / -1 where a k-mer has no event; events_per_base): a pair counts
    only when its event differs from the previous pair's event"""
    m = np.full((n_kmers, 2), -1, np.int32)
    max_event, min_event, prev = 0, 2 ** 31 - 1, -1
    for k, e in np.asarray(pairs, np.int64).reshape(-1, 2).tolist():
        if e != prev:
            if m[k, 0] == -1:
                m[k, 0] = e
            m[k, 1] = e
        max_event, min_event, prev = max(max_event, e), min(min_event, e), e
    return m, D(max_event - min_event) / D(n_kmers)


def event_alignment(m, ranks):
    """-> (n_alignment, the 'M' entries in entry order as (k-mer, event)): k-mers in order, those without events skipped, one entry
    per event of start..stop; an entry is 'M' when its k-mer's rank differs from the rank of the previous entry"""
    n, prev, ms = 0, -1, []
    for k in range(len(m)):
        start, stop = int(m[k, 0]), int(m[k, 1])
        if start == -1:
            continue
        for e in range(start, stop + 1):
            if prev != ranks[k]:
                ms.append((k, e))
            n += 1
            prev = ranks[k]
    return n, ms


def libm_log(x):
    x = float(x)
    if x != x or x < 0:
        return float("nan")
    return -math.inf if x == 0 else math.log(x)


def recalibrate(ms, ranks, events, mean, stdv):
    """the weighted least-squares fit over the 'M' entries -> (shift, scale, var) as doubles"""
    A00 = A01 = A11 = b0 = b1 = D(0)
    with np.errstate(all="ignore"):
        for k, ei in ms:
            e, mu, sd = D(events[ei]), D(mean[ranks[k]]), D(stdv[ranks[k]])
            inv_var = D(1) / (sd * sd)
            A00 = A00 + inv_var
            A01 = A01 + mu * inv_var
            A11 = A11 + (mu * mu) * inv_var
            b0 = b0 + e * inv_var
            b1 = b1 + (mu * e) * inv_var
        A10 = A01
        div = A00 * A11 - A01 * A10
        x0 = -(A01 * b1 - A11 * b0) / div
        x1 = (A00 * b1 - A10 * b0) / div
        var = D(0)
        for k, ei in ms:
            e, mu, sd = D(events[ei]), D(mean[ranks[k]]), D(stdv[ranks[k]])
            yi = (e - x0) - x1 * mu
            var = var + (yi * yi) / (sd * sd)
        var = var / D(len(ms))
        var = np.sqrt(var)
    return x0, x1, var


def calibrate(seq, events, mean, stdv, scale, shift, pairs):
    """pairs: the first n_pairs pairs of the alignment as an (n, 2) array of (ref_pos, read_pos)
    -> (record dict with the fields of gab_abea_calib, the map)"""
    events, mean, stdv = np.asarray(events, F), np.asarray(mean, F), np.asarray(stdv, F)
    n_kmers = len(seq) - K + 1
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    assert n_kmers >= 1 and events.size >= 1 and len(pairs) <= events.size + n_kmers
    rec = dict(n_alignment=0, n_m_state=0, read_stat_flag=0, recalibrated=0, scale=F(scale), shift=F(shift), var=F(1), log_var=F(0),
               events_per_base=D(0))
    if len(pairs) == 0:
        rec["read_stat_flag"] = FAILED_ALIGNMENT
        return rec, np.full((n_kmers, 2), -1, np.int32)
    assert (pairs >= 0).all() and (pairs[:, 0] < n_kmers).all() and (pairs[:, 1] < events.size).all() and (np.diff(pairs, axis=0) >= 0).all()
    ranks = A.kmer_ranks(seq).tolist()
    m, rec["events_per_base"] = base_to_event_map(pairs, n_kmers)
    rec["n_alignment"], ms = event_alignment(m, ranks)
    rec["n_m_state"] = len(ms)
    if len(ms) >= MIN_M_STATES:
        x0, x1, var = recalibrate(ms, ranks, events, mean, stdv)
        with np.errstate(all="ignore"):
            rec.update(recalibrated=1, shift=F(x0), scale=F(x1), var=F(var), log_var=F(libm_log(var)))
    if not rec["recalibrated"] or D(rec["var"]) > 2.5:
        rec["read_stat_flag"] = FAILED_CALIBRATION
    elif rec["events_per_base"] > 5.0:
        rec["read_stat_flag"] = FAILED_QUALITY_CHK
    return rec, m


def map_digest(m):
    """hash of a map as the fixture records it: sha256 of its little-endian int32 (start, stop) entries, first 16 hex digits"""
    return hashlib.sha256(np.ascontiguousarray(m, "<i4").tobytes()).hexdigest()[:16]


def record_of(rec, m):
    """a record as tests/golden/abea_calib_expected.json holds it"""
    return {"n_alignment": int(rec["n_alignment"]), "n_m_state": int(rec["n_m_state"]), "map": map_digest(m),
            "events_per_base": float(rec["events_per_base"]).hex(), "shift": float(rec["shift"]).hex(), "scale": float(rec["scale"]).hex(),
            "var": float(rec["var"]).hex(), "log_var": float(rec["log_var"]).hex(), "recalibrated": int(rec["recalibrated"]),
            "flag": int(rec["read_stat_flag"])}


# ---- paths as the fixture stores them --------------------------------------------------------------------------------------------------
def encode_path(path):
    """-> (first pair, one byte per later pair: 2 * step in ref_pos + step in read_pos; lattice steps only, so 1, 2 or 3)"""
    path = np.asarray(path, np.int64).reshape(-1, 2)
    if len(path) == 0:
        return np.array([-1, -1], np.int32), np.zeros(0, np.uint8)
    d = np.diff(path, axis=0)
    assert ((d >= 0) & (d <= 1)).all() and d.any(axis=1).all(), "not a lattice path"
    return path[0].astype(np.int32), (2 * d[:, 0] + d[:, 1]).astype(np.uint8)


def decode_path(first, steps):
    if first[0] < 0:
        return np.zeros((0, 2), np.int32)
    s = np.asarray(steps, np.int64)
    d = np.stack([s >> 1, s & 1], 1)
    return (np.asarray(first, np.int64) + np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(d, axis=0)])).astype(np.int32)


# ---- generator -------------------------------------------------------------------------------------------------------------------------
def bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())


def path_of_counts(counts):
    """the lattice path that gives k-mer k its next counts[k] events; a k-mer with none shares the event of the k-mer before it
    (a skip), which is not a new event for it, and has no pair at all before the first event"""
    path, e = [], -1
    for k, c in enumerate(counts):
        if c == 0 and e >= 0:
            path.append((k, e))
        for _ in range(c):
            e += 1
            path.append((k, e))
    return np.array(path, np.int32)


def read_of_counts(rng, seq, counts, mean, stdv, noise=0.5):
    """-> (bases, events, scale, shift, path): counts[k] events on k-mer k, each its level + noise * stdv * N(0, 1), the scalings
    1 and 0"""
    counts = np.asarray(counts, np.int64)
    ranks = A.kmer_ranks(seq)
    of = np.repeat(ranks, counts)
    ev = (np.asarray(mean, F)[of].astype(D) + noise * rng.standard_normal(of.size) * np.asarray(stdv, F)[of].astype(D)).astype(F)
    return seq, ev, F(1.0), F(0.0), path_of_counts(counts)


def renoised(rng, seq, events, scale, shift, path, mean, stdv, factor):
    """the read with every event on its path redrawn: scale * level + shift + factor * stdv * N(0, 1) of the k-mer of the first pair
    that has the event (the k-mer whose map entry takes it)"""
    ranks = A.kmer_ranks(seq)
    ev = np.array(events, F)
    z = rng.standard_normal(len(path))
    prev = -1
    for (k, e), zi in zip(np.asarray(path).tolist(), z.tolist()):
        if e != prev:
            ev[e] = F(float(scale) * float(mean[ranks[k]]) + float(shift) + factor * float(stdv[ranks[k]]) * zi)
        prev = e
    return seq, ev, F(scale), F(shift), np.asarray(path, np.int32)


def changing_bases(rng, n_kmers):
    """bases whose consecutive k-mers all differ in rank (no run of K + 1 equal bases)"""
    while True:
        seq = bases(rng, n_kmers + K - 1)
        r = A.kmer_ranks(seq)
        if (np.diff(r) != 0).all():
            return seq


def changing_bases_repaired(rng, n_kmers):
    """the same property for a read so long that a draw without a run of K + 1 equal bases is rare: the last base of every such run
    is replaced until there is none"""
    seq = bytearray(bases(rng, n_kmers + K - 1))
    while True:
        same = np.flatnonzero(np.diff(A.kmer_ranks(bytes(seq))) == 0)
        if same.size == 0:
            return bytes(seq)
        for k in same.tolist():                       # k-mers k and k + 1 are equal: bases k .. k + K are one base
            seq[k + K] = int(rng.choice([b for b in b"ACGT" if b != seq[k]]))


LONG_SEED = 20251202
LONG_KMERS = (16384, 16385, 32769)                    # the map kernel's threads take k-mers 16384 apart: one trip, a second for one k-mer, a third
STRIDE_EDGES = (16383, 16384, 32768)


def long_reads(mean, stdv):
    """name -> (bases, events, scale, shift, path): reads of LONG_KMERS k-mers, generated where they are used and never stored.  A
    tenth of the k-mers have no event; in one variant the k-mers on both sides of the stride are among them, in the other they have one"""
    out = {}
    for n in LONG_KMERS:
        for with_events in (0, 1):
            rng = np.random.default_rng([LONG_SEED, n, with_events])
            counts = rng.choice(3, n, p=(0.1, 0.6, 0.3))
            counts[0] = 1
            counts[[k for k in STRIDE_EDGES if k < n]] = with_events
            out[f"kmers_{n}_{'events' if with_events else 'none'}_at_the_stride"] = read_of_counts(rng, changing_bases_repaired(rng, n), counts, mean, stdv)
    return out


VAR_FACTORS = (2.0, 2.4, 2.6, 3.0)
EPB_COUNTS = (5, 6)
M_COUNTS = (199, 200, 201)
CASE_SEED = 20251019


def make_cases(mean, stdv, long_read):
    """the constructed cases of the golden fixture, name -> (bases, events, scale, shift, path).  long_read: a fixture read of some
    3000 bases with the reference's path, (bases, events, scale, shift, path): enough 'M' entries for var to land within a few
    hundredths of the noise factor."""
    rng = np.random.default_rng(CASE_SEED)
    cases = {}
    for f in VAR_FACTORS:
        cases[f"var_{f}"] = renoised(rng, *long_read, mean, stdv, f)
    for c in EPB_COUNTS:                              # max_event - min_event = c * n_kmers exactly: one k-mer takes one event more
        n_kmers = 210
        counts = np.full(n_kmers, c); counts[n_kmers // 2] += 1
        cases[f"epb_{c}"] = read_of_counts(rng, changing_bases(rng, n_kmers), counts, mean, stdv)
    for n in M_COUNTS:                                # one event per k-mer, every rank differs from the one before: n 'M' entries
        cases[f"m_{n}"] = read_of_counts(rng, changing_bases(rng, n), np.ones(n, np.int64), mean, stdv)
    return cases
