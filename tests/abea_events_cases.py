"""The constructed reads of abea's event detection and scaling estimate, in one place: the mixed batch of every kind of signal, the
scaling edge cases, the two extra pore models, and the reads that go through the reference for tests/golden/abea_events_cases.npz
(tests/golden/make_abea_events_golden.py).  Seeded; no GPU, no pytest, no library.

A signal is (raw samples float32, range, digitisation, offset); a scalings read is (bases, event means float32)."""
import json
import os

import numpy as np

import abea_events_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
CHUNK, WARMUP = 1024, 64          # GAB_ABEA_EVENTS_CHUNK, GAB_ABEA_EVENTS_WARMUP (test_abea_events_model.py checks them against the library)
MIXED_SEED, EDGE_SEED, ROUTE_SEED, EXTRA_SEED = 23, 31, 41, 20251021
REFERENCE_MIN_SAMPLES = 1000      # below it the reference's discarded trim step aborts or reads out of bounds


def load_events_fixture():
    """-> (level_mean, reads as (codes int16, range, digitisation, offset, bases), the recorded reference)"""
    z = np.load(os.path.join(GOLDEN, "abea_events_small.npz"))
    exp = json.load(open(os.path.join(GOLDEN, "abea_events_expected.json")))
    so = np.concatenate([[0], np.cumsum(z["n_samples"], dtype=np.int64)]); qo = np.concatenate([[0], np.cumsum(z["seq_len"], dtype=np.int64)])
    reads = [(z["codes"][so[i]:so[i + 1]], z["range"][i], z["digitisation"][i], z["offset"][i], z["seq"][qo[i]:qo[i + 1]].tobytes())
             for i in range(z["n_samples"].size)]
    return np.load(os.path.join(GOLDEN, "abea_small.npz"))["level_mean"], reads, exp


def bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())


def signal(sig):
    """a generated read (codes, range, digitisation, offset, bases) as the library takes it: float samples"""
    return (sig[0].astype(F), sig[1], sig[2], sig[3])


def mixed_cases(level_mean, chunk=CHUNK, warmup=WARMUP, fixture=None):
    """-> (names, signals, bases or None per read): 37 reads of every kind in shuffled order"""
    if fixture is None:
        _, fixture, _ = load_events_fixture()
    rng = np.random.default_rng(MIXED_SEED)
    named, seqs = {}, {}

    def add(name, sig, keep=signal):
        named[name] = keep(sig); seqs[name] = sig[4] if len(sig) > 4 else None

    for n in (1, 2, 5, 6, 11, 12, 13, 24):
        add(f"tiny_{n}", M.make_signal(rng, n, level_mean))
    for n in (chunk - 1, chunk, chunk + 1, 2 * chunk + warmup):
        add(f"chunk_{n}", M.make_signal(rng, n, level_mean))
    add("flat_run", M.find_flat_run_read(level_mean, chunk, warmup)[0])
    add("flat_read", (np.full(300, 417.0, F), F(1402.882), F(8192.0), F(3.0)), keep=lambda s: s)
    for v in (1e-30, 3e30, np.nan, np.inf):
        sig = M.make_signal(rng, 1500, level_mean)
        named[f"planted_{v}"] = M.with_planted(*sig[:4], 1100, v); seqs[f"planted_{v}"] = sig[4]
    small = sorted(range(len(fixture)), key=lambda i: fixture[i][0].size)[:4]
    for i in small:
        add(f"fixture_{i}", fixture[i])
    for t in range(37 - len(named)):
        add(f"plain_{t}", M.make_signal(rng, int(rng.integers(50, 1800)), level_mean))
    names = list(named)
    names = [names[i] for i in rng.permutation(len(names))]
    assert len(names) == 37
    return names, [named[n] for n in names], [seqs[n] for n in names]


def scalings_edge_cases():
    """-> (reads, many, wild).  reads: one k-mer with one event; bytes outside ACGT; 20 000 tame events (`many`: the order of addition
    shows in the sum of the squared differences); 20 000 events of every magnitude (`wild`: it shows in the plain sum too); 64 events on
    65 k-mers and 65 on 64"""
    rng = np.random.default_rng(EDGE_SEED)
    seq = bases(rng, 120)
    many = (rng.uniform(60, 130, 20000) + rng.standard_normal(20000) * 0.37).astype(F)
    wild = (many * 10.0 ** rng.uniform(-8, 8, 20000)).astype(F)
    reads = [(bases(rng, 6), np.array([93.25], F)),                   # one k-mer, one event
             (seq[:40] + b"N" + seq[41:80] + b"a" + seq[81:], rng.uniform(60, 130, 200).astype(F)),
             (bases(rng, 3000), many), (bases(rng, 2500), wild),
             (bases(rng, 70), rng.uniform(60, 130, 64).astype(F)), (bases(rng, 69), rng.uniform(60, 130, 65).astype(F))]
    return reads, many, wild


EDGE_NAMES = ("one_kmer_one_event", "non_acgt", "many_20000", "wild_20000", "events_64_kmers_65", "events_65_kmers_64")


def route_models(level_mean):
    """the two extra pore models: levels on a grid of 1/4 pA (the sum of squared levels becomes provable too), and a level of 1e-30
    at rank 0, AAAAAA (forces the two k-mer sums of a read that has that k-mer into the reference's order)"""
    coarse = (np.round(level_mean * 4) / 4).astype(F)
    tiny = np.asarray(level_mean, F).copy(); tiny[0] = F(1e-30)
    return {"coarse": coarse, "tiny": tiny}


def scalings_route_cases():
    """two reads, the second with the k-mer AAAAAA"""
    rng = np.random.default_rng(ROUTE_SEED)
    return [(bases(rng, 400), rng.uniform(60, 130, 700).astype(F)), (bases(rng, 90) + b"AAAAAA" + bases(rng, 50), rng.uniform(60, 130, 300).astype(F))]


def square_wave(period, n=1500, low=80.0, high=100.0, offset=3.0):
    """ADC codes that alternate between two levels every period / 2 samples, without noise"""
    pa = np.where((np.arange(n) // (period // 2)) % 2 == 0, low, high)
    codes = np.rint(pa / (M.RANGE / M.DIGITISATION) - offset).astype(F)
    return codes, F(M.RANGE), F(M.DIGITISATION), F(offset)


def reference_signals(level_mean, chunk=CHUNK, warmup=WARMUP, fixture=None):
    """-> (names, signals, bases per read): the reads whose event table the reference records: every mixed case of 1000 samples at least
    (the reads around the chunk size, the flat run that makes a chunk run again, the four planted reads among them), reads of 1000 and
    1001 samples, two square waves (periods 14 and 6), and a flat read of 1500 samples, which the reference refuses"""
    names, signals, seqs = mixed_cases(level_mean, chunk, warmup, fixture)
    keep = [i for i, s in enumerate(signals) if s[0].size >= REFERENCE_MIN_SAMPLES]
    names, signals, seqs = [names[i] for i in keep], [signals[i] for i in keep], [seqs[i] for i in keep]
    rng = np.random.default_rng(EXTRA_SEED)
    for n in (1000, 1001):
        sig = M.make_signal(rng, n, level_mean)
        names.append(f"samples_{n}"); signals.append(signal(sig)); seqs.append(sig[4])
    for period in (14, 6):
        names.append(f"square_wave_{period}"); signals.append(square_wave(period)); seqs.append(bases(rng, 60))
    names.append("flat_1500"); signals.append((np.full(1500, 417.0, F), F(1402.882), F(8192.0), F(3.0))); seqs.append(bases(rng, 60))
    return names, signals, seqs


def not_run_in_reference(level_mean, chunk=CHUNK, warmup=WARMUP, fixture=None):
    """the mixed cases below 1000 samples: model-only"""
    names, signals, _ = mixed_cases(level_mean, chunk, warmup, fixture)
    return [n for n, s in zip(names, signals) if s[0].size < REFERENCE_MIN_SAMPLES]


def load_cases():
    """abea_events_cases.npz and the reference's record -> (level_mean, signals, scalings reads by pore model, record)"""
    z = np.load(os.path.join(GOLDEN, "abea_events_cases.npz"))
    exp = json.load(open(os.path.join(GOLDEN, "abea_events_cases_expected.json")))
    ro = np.concatenate([[0], np.cumsum(z["n_samples"], dtype=np.int64)]); so = np.concatenate([[0], np.cumsum(z["seq_len"], dtype=np.int64)])
    mo = np.concatenate([[0], np.cumsum(z["n_means"], dtype=np.int64)])
    n_sig = z["n_samples"].size
    seqs = [z["seq"][so[i]:so[i + 1]].tobytes() for i in range(z["seq_len"].size)]
    signals = [(z["raw"][ro[i]:ro[i + 1]], z["range"][i], z["digitisation"][i], z["offset"][i], seqs[i]) for i in range(n_sig)]
    given = [(seqs[n_sig + i], z["means"][mo[i]:mo[i + 1]]) for i in range(z["n_means"].size)]
    return np.load(os.path.join(GOLDEN, "abea_small.npz"))["level_mean"], signals, given, exp
