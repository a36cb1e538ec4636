"""The constructed reads of abea's align stage, in one place: the named edge cases that the GPU tests run, the seeded searches that
find reads on the kernel's thresholds, and the pool of small random reads.  Seeded; no GPU, no pytest, no library.  The golden script
(tests/golden/make_abea_golden.py) runs the searches through the model once and keeps what they find in tests/golden/abea_cases.npz
with the reference's record of it; the tests load that fixture and never search.

A read is (bases, event means float32, scale, shift)."""
import json
import os

import numpy as np

import abea_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
NAMED_SEED, SEARCH_SEED, POOL_SEED = 11, 20251021, 7
POOL_READS, NOT_SPANNED_CANDIDATES = 400, 20000
MODES = ("plain", "sparse", "dense", "unrelated", "wild")
PATH_LENGTHS = (63, 64, 65, 127, 128, 129)


def load_fixture():
    """abea_small.npz and the reference's record of it -> ((level_mean, level_stdv, level_log_stdv), reads, record)"""
    return _load("abea_small.npz", "abea_expected.json")


def load_cases():
    """abea_cases.npz and the reference's record of it -> (model of abea_small.npz, names, reads, record)"""
    _, reads, exp = _load("abea_cases.npz", "abea_cases_expected.json")
    return load_fixture()[0], [r["name"] for r in exp["reads"]], reads, exp


def _load(npz, record):
    z = np.load(os.path.join(GOLDEN, npz))
    exp = json.load(open(os.path.join(GOLDEN, record)))
    so = np.concatenate([[0], np.cumsum(z["seq_len"], dtype=np.int64)]); eo = np.concatenate([[0], np.cumsum(z["n_events"], dtype=np.int64)])
    reads = [(z["seq"][so[i]:so[i + 1]].tobytes(), z["events"][eo[i]:eo[i + 1]], z["scale"][i], z["shift"][i]) for i in range(z["seq_len"].size)]
    model = (z["level_mean"], z["level_stdv"], z["level_log_stdv"]) if "level_mean" in z.files else None
    return model, reads, exp


def bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())


def named_cases(model=None, fixture=None):
    """-> (model, names, reads): the named edge cases and the three long reads of the fixture, in shuffled order"""
    if model is None:
        model, fixture, _ = load_fixture()
    mean, stdv, _ = model
    rng = np.random.default_rng(NAMED_SEED)
    named = {}
    one = bases(rng, 6)
    for n in (1, 2, 300):                                            # one k-mer
        named[f"one_kmer_{n}_events"] = (one, M.make_events(rng, one, mean, stdv, counts=[n]), 1.0, 0.0)
    named["under_100_bands_a"] = M.make_read(rng, 20, mean, stdv)    # clipped on all four sides
    named["under_100_bands_b"] = M.make_read(rng, 35, mean, stdv, counts=np.full(30, 1))
    s = bases(rng, 45)
    named["bands_99"] = (s, M.make_events(rng, s, mean, stdv, counts=[2] * 17 + [1] * 23), 1.0, 0.0)      # 40 k-mers + 57 events + 2
    named["bands_100"] = (s, M.make_events(rng, s, mean, stdv, counts=[2] * 18 + [1] * 22), 1.0, 0.0)
    named["bands_101"] = (s, M.make_events(rng, s, mean, stdv, counts=[2] * 19 + [1] * 21), 1.0, 0.0)
    named["half_an_event_per_kmer"] = M.make_read(rng, 405, mean, stdv, counts=np.arange(400) % 2)
    named["five_events_per_kmer"] = M.make_read(rng, 150, mean, stdv, counts=np.full(145, 5))
    named["one_event_300_bases"] = (bases(rng, 300), np.array([95.0], F), 1.0, 0.0)
    named["no_end_nan_events"] = (bases(rng, 80), np.full(120, np.nan, F), 1.0, 0.0)
    named["gap_one_event_60_kmers"] = (bases(rng, 65), np.array([95.0], F), 1.0, 0.0)
    named["gap_run_of_55"] = M.make_gap_read(rng, mean, stdv)
    seq, ev, sc, sh = M.make_read(rng, 200, mean, stdv)
    named["wrong_shift"] = (seq, ev, sc, F(sh + F(15.0)))
    seq, ev, sc, sh = M.make_read(rng, 180, mean, stdv)
    named["non_acgt"] = (seq[:50] + b"N" + seq[51:90] + b"a" + seq[91:], ev, sc, sh)
    named["plain"] = M.make_read(rng, 260, mean, stdv)
    longs = sorted(range(len(fixture)), key=lambda i: -len(fixture[i][0]))[:3]
    for i in longs:
        named[f"long_{i}"] = fixture[i]
    names = list(named)
    names = [names[i] for i in rng.permutation(len(names))]
    return model, names, [named[n] for n in names]


def extra_cases(model):
    """four more constructed reads, in this order: two k-mers with one event, an inf event, scale 0, 40 events per k-mer on 7 k-mers"""
    mean, stdv, _ = model
    rng = np.random.default_rng(SEARCH_SEED)
    out = {"two_kmers_one_event": (bases(rng, 7), np.array([95.0], F), 1.0, 0.0)}
    seq, ev, sc, sh = M.make_read(rng, 90, mean, stdv)
    ev = ev.copy(); ev[ev.size // 2] = F(np.inf)
    out["inf_event"] = (seq, ev, sc, sh)
    seq, ev, sc, sh = M.make_read(rng, 90, mean, stdv)
    out["scale_0"] = (seq, ev, F(0.0), F(float(ev.astype(np.float64).mean())))
    out["forty_events_per_kmer"] = M.make_read(rng, 12, mean, stdv, counts=np.full(7, 40))
    return out


# ---- the pool: small random reads in five input modes --------------------------------------------------------------------------------
def pool_read(rng, model, lo=6, hi=140):
    """-> (mode, read).  plain: the generator's events; sparse: events on a fraction of the k-mers only (fewer events than k-mers);
    dense: 2 to 8 events on every k-mer; unrelated: uniform events that know nothing of the bases, scale 1 and shift 0; wild: a plain
    read with up to three of: an event that is NaN, inf, -inf, 1e30 or 0, a byte outside ACGT, a shift moved by N(0, 8), a scale of
    0 or -1"""
    mean, stdv, _ = model
    mode = MODES[int(rng.integers(len(MODES)))]
    n = int(rng.integers(lo, hi + 1))
    nk = n - M.K + 1
    if mode == "plain":
        return mode, M.make_read(rng, n, mean, stdv)
    if mode == "sparse":
        return mode, M.make_read(rng, n, mean, stdv, counts=(rng.random(nk) < rng.uniform(0.0, 0.8) ** 2).astype(np.int64))
    if mode == "dense":
        return mode, M.make_read(rng, n, mean, stdv, counts=rng.integers(2, 9, nk))
    if mode == "unrelated":
        ne = max(1, int(nk * rng.uniform(0.0, 1.5) ** 2))
        return mode, (bases(rng, n), rng.uniform(60.0, 130.0, ne).astype(F), F(1.0), F(0.0))
    seq, ev, sc, sh = M.make_read(rng, n, mean, stdv)
    seq, ev = bytearray(seq), ev.copy()
    for _ in range(int(rng.integers(1, 4))):
        what = int(rng.integers(4))
        if what == 0:
            ev[int(rng.integers(ev.size))] = F((np.nan, np.inf, -np.inf, 1e30, 0.0)[int(rng.integers(5))])
        elif what == 1:
            seq[int(rng.integers(n))] = b"NacgtX-"[int(rng.integers(7))]
        elif what == 2:
            sh = F(sh + F(8.0 * rng.standard_normal()))
        else:
            sc = F((0.0, -1.0)[int(rng.integers(2))])
    return mode, (bytes(seq), ev, sc, sh)


def model_of(model, read):
    return M.align(read[0], read[1], *model, read[2], read[3])


def pool_sample(model, seed=POOL_SEED, n=POOL_READS):
    """-> (modes, reads): the first n pool reads of the seed whose end scan finds something in the model (the read whose end scan finds
    nothing is the documented deviation from the reference and has its one named case)"""
    rng = np.random.default_rng(seed)
    modes, reads = [], []
    while len(reads) < n:
        mode, r = pool_read(rng, model)
        if model_of(model, r)[0]["flags"] != M.NO_END:
            modes.append(mode); reads.append(r)
    return modes, reads


# ---- the seeded searches, through the model ------------------------------------------------------------------------------------------
def search_max_gap(model, limit=400):
    """-> {"max_gap_50": read, "max_gap_51": read}: reads whose longest run of skips is exactly 50 with no flag set, and exactly 51 with
    GAP as the only flag.  A skip costs log(1e-10), so a path skips only where it has no event to spend, and the pairs of a run of
    skips all carry one event: the emission check passes only when the k-mers of the run have that event's level.  The candidates
    are therefore runs of one base (every k-mer the same) of 50 to 56 k-mers with one to three events near that k-mer's level."""
    mean, stdv, _ = model
    rng = np.random.default_rng(SEARCH_SEED + 1)
    want = {"max_gap_50": (50, 0), "max_gap_51": (51, M.GAP)}
    out = {}
    for _ in range(limit):
        seq = bytes([b"ACGT"[int(rng.integers(4))]]) * int(rng.integers(55, 62))
        level = float(mean[M.kmer_ranks(seq)[0]])
        r = (seq, (level + 0.5 * rng.standard_normal(int(rng.integers(1, 4)))).astype(F), F(1.0), F(0.0))
        rec, _ = model_of(model, r)
        for name, (gap, flags) in want.items():
            if name not in out and (rec["max_gap"], rec["flags"]) == (gap, flags):
                out[name] = r
        if len(out) == len(want):
            return out
    raise AssertionError(f"search_max_gap: only {sorted(out)} in {limit} candidates")


def search_path_lengths(model, limit=4000):
    """-> {"path_len_N": read} for N in PATH_LENGTHS (multiples of the 64 lanes that sum the emissions and move the path, and their
    neighbours), each a read that passes every check"""
    rng = np.random.default_rng(SEARCH_SEED + 2)
    out = {}
    for _ in range(limit):
        target = PATH_LENGTHS[int(rng.integers(len(PATH_LENGTHS)))]
        if f"path_len_{target}" in out:
            continue
        r = M.make_read(rng, int(rng.integers(target // 2 + 5, target * 3 // 4 + 5)), model[0], model[1])
        rec, _ = model_of(model, r)
        name = f"path_len_{rec['path_len']}"
        if rec["path_len"] in PATH_LENGTHS and rec["flags"] == 0 and name not in out:
            out[name] = r
        if len(out) == len(PATH_LENGTHS):
            return {f"path_len_{n}": out[f"path_len_{n}"] for n in PATH_LENGTHS}
    raise AssertionError(f"search_path_lengths: only {sorted(out)} in {limit} candidates")


def search_room(model, limit=3000):
    """-> ({"room_one_short": read, "room_tightest": read}, the tightest cap - len).  cap = n_events + n_kmers pairs of room; a path has
    at most cap - 1 pairs.  room_one_short: the first pool read whose path is one pair short of its room: it
    starts at (0, 0), ends on the last event and has no diagonal move, which a read with two k-mers and two events at least never
    prefers (the detour costs a skip and one more emission), so it has one k-mer or one event; room_tightest: among pool reads with 20 k-mers and 20 events at least, the one with the
    smallest cap - len (the first of them)"""
    rng = np.random.default_rng(SEARCH_SEED + 3)
    short, tight, tightest = None, None, None
    for t in range(limit):
        _, r = pool_read(rng, model, *((7, 12) if t % 2 else (25, 60)))
        nk, ne = len(r[0]) - M.K + 1, r[1].size
        rec, _ = model_of(model, r)
        if rec["flags"] & M.NO_END:
            continue
        slack = nk + ne - rec["path_len"]
        assert slack >= 1
        if short is None and slack == 1:
            short = r
        if nk >= 20 and ne >= 20 and (tightest is None or slack < tightest):
            tight, tightest = r, slack
    assert short is not None and tight is not None, "search_room found nothing"
    return {"room_one_short": short, "room_tightest": tight}, tightest


def search_emission_bracket(model):
    """-> ({"emission_above": read, "emission_below": read}, (avg above, avg below)): one read with two shifts that are neighbouring
    floats, found by bisection between the read's own shift (average log emission above -5.0) and that shift plus 15 (below)"""
    rng = np.random.default_rng(SEARCH_SEED + 4)
    seq, ev, sc, sh = M.make_read(rng, 70, model[0], model[1])
    avg = lambda s: model_of(model, (seq, ev, sc, s))[0]["avg_log_emission"]
    lo, hi = F(sh), F(sh + F(15.0))
    assert avg(lo) >= -5.0 > avg(hi)
    while True:
        mid = F((float(lo) + float(hi)) / 2)
        if mid == lo or mid == hi:
            break
        if avg(mid) < -5.0:
            hi = mid
        else:
            lo = mid
    assert np.nextafter(lo, F(np.inf)) == hi and avg(lo) >= -5.0 > avg(hi)
    return {"emission_above": (seq, ev, sc, lo), "emission_below": (seq, ev, sc, hi)}, (avg(lo), avg(hi))


def search_not_spanned(model, n=NOT_SPANNED_CANDIDATES):
    """-> a pool read (6 to 40 bases) whose model record has NOT_SPANNED set, or None when none of n candidates has"""
    rng = np.random.default_rng(SEARCH_SEED + 5)
    for _ in range(n):
        _, r = pool_read(rng, model, 6, 40)
        if model_of(model, r)[0]["flags"] & M.NOT_SPANNED:
            return r
    return None
