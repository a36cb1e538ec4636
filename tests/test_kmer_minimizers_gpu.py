"""GPU: the minimizer sketch and index (gab_kmer_sketch, gab_kmer_index_*, through genarchbench_amd.kmer) against what the reference
recorded (tests/golden/kmer_minimizer_expected.json, kmer_minimizer_tiny.npz) and, array for array, against the sequential model of
tests/minimizer_model.py.  Every comparison is equality; every output buffer is pre-filled with a sentinel by the Python mirror."""
import functools
import json

import numpy as np
import pytest

from tests import kmer_model, minimizer_model as mm
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

EXPECTED = json.load(open(f"{GOLDEN}/kmer_minimizer_expected.json"))
MIN_LEN = EXPECTED["min_len_exclusive"]
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
EINVAL, ERANGE = -22, -34
RUN, TILE = 64, 4096        # GAB_KMER_RUN; a wave's tile of 64 runs
RESULT_FIELDS = ("minimizers", "distinct", "repetitive_frequency", "filtered_kmers", "filtered_entries", "selected_kmers", "index_entries")


@pytest.fixture(scope="module")
def kc():
    from genarchbench_amd.kmer import KmerCounter
    e = KmerCounter()
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def reads_of(name):
    return kmer_model.load_reads([f"{GOLDEN}/{name}"])


@functools.lru_cache(maxsize=None)
def entries_of(name, k, window):
    return mm.entries(reads_of(name), k, window, MIN_LEN)      # (the reference: computed once, shared by the two rates)


def rand(seed, n):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def check_sketch(kc, reads, k, w, min_len=0):
    start, pos = kc.sketch(reads, k, w, min_len)
    want_start, want_pos = mm.sketch_reads(reads, k, w, min_len)
    np.testing.assert_array_equal(start, want_start)
    np.testing.assert_array_equal(pos, want_pos)
    return start, pos


def check_index(kc, reads, k, w, rate, min_len=0, m=None):
    """the nine fields, the dump and a look-up of every k-mer of the model == the model"""
    m = m or mm.build_index(reads, k, w, rate, min_len)
    got = kc.index_minimizers(reads, k, w, rate, min_len)
    assert got == {f: m[f] for f in mm.FIELDS}
    kmers, start, gpos = kc.index_dump()
    np.testing.assert_array_equal(kmers, m["kmers"])
    np.testing.assert_array_equal(start, m["start"])
    np.testing.assert_array_equal(gpos, m["gpos"])
    if m["kmers"].size:
        first, count, rep = kc.index_lookup(m["kmers"])
        np.testing.assert_array_equal(first, m["start"][:-1])
        np.testing.assert_array_equal(count, np.diff(m["start"]))
        assert not rep.any()
    if m["repetitive"].size:
        first, count, rep = kc.index_lookup(m["repetitive"])
        assert (first == -1).all() and (count == 0).all() and (rep == 1).all()
    return m


# ---- goldens --------------------------------------------------------------------------------------------------------------------------
GRID = [(name, r["k"], r["window"]) for name in sorted(EXPECTED["files"]) for r in EXPECTED["files"][name]["rows"] if r["rate"] == 100]


@pytest.mark.parametrize("name,k,window", GRID)
def test_golden_grid(kc, name, k, window):
    """both rates of a grid point: the fields the reference printed or built, its index digest, and the model array for array"""
    for row in (r for r in EXPECTED["files"][name]["rows"] if (r["k"], r["window"]) == (k, window)):
        m = mm.index_of_entries(entries_of(name, k, window), row["rate"])
        check_index(kc, reads_of(name), k, window, row["rate"], MIN_LEN, m)      # (the library == the model ...)
        assert {f: m[f] for f in RESULT_FIELDS} == {f: row[f] for f in RESULT_FIELDS}      # (... == the reference's record)
        assert mm.digest(*kc.index_dump()) == row["index_sha256"]


def test_golden_tiny_element_for_element(kc):
    t = EXPECTED["tiny"]
    z = np.load(f"{GOLDEN}/kmer_minimizer_tiny.npz")
    reads = [r for r in reads_of(t["file"]) if len(r) > MIN_LEN][:t["kept_reads"]]
    got = kc.index_minimizers(reads, t["k"], t["window"], t["rate"], MIN_LEN)
    assert {f: got[f] for f in RESULT_FIELDS} == {f: t[f] for f in RESULT_FIELDS}
    kmers, start, gpos = kc.index_dump()
    for name, a in (("kmers", kmers), ("start", start), ("gpos", gpos)):
        np.testing.assert_array_equal(a, z[name], err_msg=name)
    first, count, rep = kc.index_lookup(z["repetitive"])
    assert (rep == 1).all() and (count == 0).all()


def test_golden_sketch_of_the_fixture(kc):
    for name in sorted(EXPECTED["files"]):
        check_sketch(kc, reads_of(name), 15, 10, MIN_LEN)


# ---- sketch: edge shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 5, 255])
def test_sketch_edge_lengths(kc, w):
    """one call: L - k in -1, 0, 1, 2; around w; one lane's run (63, 64, 65) and one wave's tile (4095, 4096, 4097) +- 1; an empty read"""
    k = 15
    npos = [-1, 0, 1, 2, w - 1, w, w + 1, RUN - 1, RUN, RUN + 1, 2 * RUN, TILE - 1, TILE, TILE + 1, 2 * TILE + RUN, -k]
    reads = [rand(1000 + i, n + k) for i, n in enumerate(npos)]
    start, pos = check_sketch(kc, reads, k, w)
    assert start[1] == 0 and start[2] == 0 and start[3] - start[2] == 1      # L - k = -1, 0: nothing; 1: position 0


@pytest.mark.parametrize("k", [1, 2, 11, 16, 17])
def test_sketch_every_k(kc, k):
    check_sketch(kc, [rand(50 + k, n) for n in (3 * TILE + 77, 500, k, k + 1)], k, 7)


def test_window_and_k_bounds(kc):
    from genarchbench_amd.kmer import GabError, MAX_WINDOW
    assert MAX_WINDOW >= 255
    reads = [rand(3, 600)]
    check_sketch(kc, reads, 15, MAX_WINDOW)
    for w in (0, -1, MAX_WINDOW + 1):
        for call in (lambda: kc.sketch(reads, 15, w, 0), lambda: kc.index_minimizers(reads, 15, w, 100, 0)):
            with pytest.raises(GabError) as e:
                call()
            assert e.value.code == EINVAL and "window" in str(e.value)
    for k in (0, 18):
        with pytest.raises(GabError) as e:
            kc.index_minimizers(reads, k, 5, 100, 0)
        assert e.value.code == EINVAL
    for rate in (-1.0, float("inf"), float("nan")):
        with pytest.raises(GabError) as e:
            kc.index_minimizers(reads, 15, 5, rate, 0)
        assert e.value.code == EINVAL and "repeat_kmer_rate" in str(e.value)


def _with_minimizer_at(target, k, w, seed):
    """a random read one of whose minimizers lies exactly at position `target`: drawn until the model says so"""
    for s in range(seed, seed + 400):
        r = rand(s, target + 3 * w + k + 40)
        if target in mm.sketch(r, k, w).tolist():
            return r
    raise AssertionError("no such read in 400 draws")


@pytest.mark.parametrize("w", [3, 10, 100])
def test_minimizer_on_a_run_and_a_tile_boundary(kc, w):
    k = 13
    reads = [_with_minimizer_at(t, k, w, 7000 + 500 * i) for i, t in enumerate((RUN - 1, RUN, TILE - 1, TILE, 2 * TILE))]
    check_sketch(kc, reads, k, w)


# ---- ties -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 5, 64, 255])
def test_homopolymer_longer_than_two_tiles(kc, w):
    k = 15
    start, pos = check_sketch(kc, [b"A" * 9000], k, w)
    assert pos.tolist() == list(range(0, 9000 - k, w))      # from the start of the run, whatever lane or wave a position falls to


@pytest.mark.parametrize("w", [4, 19, 70])
def test_poly_a_inside_random_sequence(kc, w):
    k = 11
    reads = [rand(200 + o, o) + b"A" * n + rand(300 + o, 150) for o in (1, 63, 64, 65) for n in (40, 3 * RUN + 5, TILE + 200)]
    check_sketch(kc, reads, k, w)


@pytest.mark.parametrize("unit", [b"AC", b"ACGGTCA"])
def test_tandem_repeats_with_windows_around_the_period(kc, unit):
    k = 9
    p = len(unit)
    body = unit * (2 * TILE // p + 50)
    for w in sorted({max(p - 1, 2), p, p + 1, 2 * p, 3 * p + 1}):
        check_sketch(kc, [body, rand(9, 77) + body[:1500] + rand(10, 300)], k, w)


@pytest.mark.parametrize("w", [6, 33])
def test_the_same_kmer_w_and_w_plus_1_apart(kc, w):
    k = 12
    reads = []
    for gap in (w - 1, w, w + 1, 2 * w):
        for at in (5, RUN - 3, TILE - 2):
            r = bytearray(rand(4000 + gap + at, at + gap + k + 3 * w + 50))
            r[at + gap:at + gap + k] = r[at:at + k]
            reads.append(bytes(r))
    check_sketch(kc, reads, k, w)
    check_index(kc, reads, k, w, 100)


def test_low_complexity_two_letter_reads(kc):
    """reads over two letters at k = 3: eight k-mers, so nearly every window has tied minima and the walk back is the rule"""
    rng = np.random.default_rng(77)
    reads = [np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, n)].tobytes() for n in (TILE + 300, 700, 3 * RUN)]
    for w in (2, 3, 9, 40):
        check_sketch(kc, reads, 3, w)
    check_index(kc, reads, 3, 9, 100)


def test_palindromes_and_lower_case(kc):
    """k even: a k-mer equal to its reverse complement is entered on the forward strand; lower case reads as upper case"""
    k, w = 6, 4
    pal = b"ACGCGT"      # its own reverse complement
    assert pal.translate(COMP)[::-1] == pal
    reads = [rand(61, 300) + pal + rand(62, 200) + pal + rand(63, 100), (rand(64, 500) + pal * 3 + rand(65, 100)).lower(), pal * 40]
    check_sketch(kc, reads, k, w)
    check_index(kc, reads, k, w, 1000)
    m = check_index(kc, reads, k, 1, 1000)      # window 1: the palindrome is a minimizer wherever it stands
    key = int(kmer_model.canonical_kmers(pal + b"A", k)[0])
    assert key in m["kmers"].tolist()
    i = m["kmers"].tolist().index(key)
    lens = [len(r) for r in reads]
    for g in m["gpos"][m["start"][i]:m["start"][i + 1]]:          # every entry of the palindrome lies on a forward copy
        base = 0
        for n in lens:
            if base <= g < base + 2 * n:
                assert g < base + n
            base += 2 * n
    assert kc.index_minimizers([r.upper() for r in reads], k, w, 1000, 0) == kc.index_minimizers(reads, k, w, 1000, 0)


# ---- positions --------------------------------------------------------------------------------------------------------------------------
def test_a_read_and_its_reverse_complement(kc):
    k, w = 15, 1        # window 1: every k-mer of both reads is entered, so every list holds both strands
    r = rand(5, 700)
    reads = [r, r.translate(COMP)[::-1]]
    m = check_index(kc, reads, k, w, 1000)
    # k-mer i of the read is k-mer L - k - i of its reverse complement; both walks leave their last position out
    assert (np.diff(m["start"]) >= 2).sum() >= len(r) - k - 2
    first, count, rep = kc.index_lookup(kmer_model.canonical_kmers(r, k)[1:])
    assert (count >= 2).all()


def test_a_filtered_read_shifts_no_offsets(kc):
    k, w = 15, 5
    a, b, short = rand(1, 3000), rand(2, 2500), rand(3, 900)
    m2 = check_index(kc, [a, b], k, w, 100, 1000)
    m3 = check_index(kc, [a, short, b], k, w, 100, 1000)
    assert m3["reads_kept"] == 2
    for f in ("kmers", "start", "gpos"):
        np.testing.assert_array_equal(m2[f], m3[f])
    start, pos = check_sketch(kc, [a, short, b], k, w, 1000)
    assert start[1] == start[2]


# ---- filter -----------------------------------------------------------------------------------------------------------------------------
def _rate_for(total, unique, want):
    """a float rate with repetitive_frequency(total, unique, rate) == want (searched, then checked with the model's own arithmetic)"""
    mean = np.float32(total) / np.float32(unique + 1)
    rate = float(np.float32((want + 0.5) / float(mean)))
    assert mm.repetitive_frequency(total, unique, rate) == want
    return rate


def test_threshold_on_the_poly_a_key(kc):
    """capacity == repetitive_frequency stays, capacity == repetitive_frequency + 1 goes"""
    k, w = 15, 5
    reads = [rand(8, 900) + b"A" * 700 + rand(9, 800), rand(10, 1200)]
    base = mm.build_index(reads, k, w, 1e6, 0)
    cap = int(np.diff(base["start"]).max())
    poly = int(base["kmers"][np.diff(base["start"]).argmax()])
    assert poly == 0 and cap > 100
    for want, kept in ((cap, True), (cap - 1, False)):
        rate = _rate_for(base["minimizers"], base["distinct"], want)
        m = check_index(kc, reads, k, w, rate)
        assert m["repetitive_frequency"] == want and (0 in m["kmers"].tolist()) == kept
        first, count, rep = kc.index_lookup(np.array([0, (1 << 30) - 1], np.uint64))      # poly-A and its reverse complement, poly-T
        assert rep.tolist() == [0 if kept else 1] * 2 and count.tolist() == [cap if kept else 0] * 2
        if kept:
            got = kc.index_dump()[2][first[0]:first[0] + cap]
            assert (np.diff(got) > 0).all() and cap > 64      # a list longer than a wave, sorted


def test_rate_zero_gives_an_empty_index(kc):
    reads = [rand(4, 2000)]
    m = check_index(kc, reads, 15, 5, 0.0)
    assert m["selected_kmers"] == 0 and m["index_entries"] == 0 and m["filtered_entries"] == m["minimizers"] > 0
    kmers, start, gpos = kc.index_dump()
    assert kmers.size == 0 and start.tolist() == [0] and gpos.size == 0


def test_a_long_list_comes_out_sorted(kc):
    """one key with thousands of entries from both strands of many reads, between keys with one"""
    k, w = 13, 4
    rng = np.random.default_rng(21)
    unit = rand(22, 40)
    reads = []
    for i in range(30):
        r = rand(100 + i, int(rng.integers(50, 400))) + unit * int(rng.integers(20, 90)) + rand(200 + i, 100)
        reads.append(r.translate(COMP)[::-1] if i % 2 else r)
    m = check_index(kc, reads, k, w, 1e6)
    assert np.diff(m["start"]).max() > 500


# ---- ABI behaviour ------------------------------------------------------------------------------------------------------------------------
def test_erange_round_trips(kc):
    reads = [rand(30, 1500), rand(31, 40)]
    want_start, want_pos = mm.sketch_reads(reads, 15, 5, 0)
    start = np.full(3, -7, np.int64)
    small = np.full(want_pos.size - 1, -7, np.int32)
    rc, n = kc.sketch_into(reads, 15, 5, start, small, 0)
    assert rc == ERANGE and n == want_pos.size and (small == -7).all() and (start == -7).all()
    exact = np.full(n, -7, np.int32)
    rc, n = kc.sketch_into(reads, 15, 5, start, exact, 0)
    assert rc == 0 and np.array_equal(exact, want_pos) and np.array_equal(start, want_start)

    m = mm.build_index(reads, 15, 5, 100, 0)
    kc.index_minimizers(reads, 15, 5, 100, 0)
    nk, ne = m["selected_kmers"], m["index_entries"]
    for ck, ce in ((nk - 1, ne), (nk, ne - 1), (0, 0)):
        kmers = np.full(ck, 7, np.uint64); st = np.full(ck + 1, -7, np.int64); gpos = np.full(ce, -7, np.int64)
        rc, need_k, need_e = kc.index_dump_into(kmers, st, gpos)
        assert rc == ERANGE and (need_k, need_e) == (nk, ne) and (kmers == 7).all() and (st == -7).all() and (gpos == -7).all()
    kmers = np.full(nk, 7, np.uint64); st = np.full(nk + 1, -7, np.int64); gpos = np.full(ne, -7, np.int64)
    assert kc.index_dump_into(kmers, st, gpos) == (0, nk, ne)
    assert np.array_equal(kmers, m["kmers"]) and np.array_equal(st, m["start"]) and np.array_equal(gpos, m["gpos"])


def test_handle_state_between_count_and_index():
    from genarchbench_amd.kmer import GabError, KmerCounter
    reads = [rand(40, 3000)]
    h = KmerCounter()
    try:
        index_calls = (h.index_dump, lambda: h.index_lookup(np.zeros(1, np.uint64)), h.index_last_phases)
        count_calls = (lambda: h.spectrum(8), lambda: h.query(np.zeros(1, np.uint64)), h.dump)

        def all_einval(calls):
            for call in calls:
                with pytest.raises(GabError) as e:
                    call()
                assert e.value.code == EINVAL
        all_einval(index_calls)                     # before the first index call
        h.sketch(reads, 15, 5, 0)                   # a sketch alone builds no index
        all_einval(index_calls)
        want = h.count(reads, 15, 0)
        all_einval(index_calls)
        h.sketch(reads, 15, 5, 0)                   # ... and leaves a count alone
        assert h.dump()[0].size == want["distinct"]
        h.index_minimizers(reads, 15, 5, 100, 0)
        all_einval(count_calls)                     # the index took the table over
        assert h.index_dump()[0].size > 0 and h.index_last_phases()["sketch_ms"] > 0
        assert h.count(reads, 15, 0) == want
        all_einval(index_calls)                     # ... and a later count takes it back
        assert h.dump()[0].size == want["distinct"]
    finally:
        h.close()


def test_a_byte_outside_acgt_names_the_read(kc):
    from genarchbench_amd.kmer import GabError
    reads = [rand(50, 300), rand(51, 200) + b"N" + rand(52, 100), rand(53, 80)]
    for call in (lambda: kc.sketch(reads, 15, 5, 0), lambda: kc.index_minimizers(reads, 15, 5, 100, 0)):
        with pytest.raises(GabError) as e:
            call()
        assert e.value.code == EINVAL and "read 1 " in str(e.value)


def test_empty_inputs(kc):
    zeros = {f: 0 for f in mm.FIELDS}
    for reads, min_len, kept, total in (([], 0, 0, 0), ([rand(1, 100)], 5000, 0, 0), ([rand(1, 10), b""], 0, 1, 10)):
        got = kc.index_minimizers(reads, 15, 5, 100, min_len)
        assert got == dict(zeros, reads_kept=kept, total_len=total)
        kmers, start, gpos = kc.index_dump()
        assert kmers.size == 0 and start.tolist() == [0] and gpos.size == 0
        first, count, rep = kc.index_lookup(np.array([5], np.uint64))
        assert (first[0], count[0], rep[0]) == (-1, 0, 0)
        start, pos = kc.sketch(reads, 15, 5, min_len)
        assert start.tolist() == [0] * (len(reads) + 1) and pos.size == 0


def test_device_forms_equal_the_host_forms(kc):
    import torch
    from genarchbench_amd.kmer import pack_reads
    reads = [rand(70, 5000), rand(71, 30), b"A" * 900, rand(72, TILE + 500)]
    seq, off, ln = pack_reads(reads)
    dev = torch.device("cuda:0")
    t_seq, t_off, t_ln = (torch.from_numpy(a).to(dev) for a in (seq, off, ln))
    want_start, want_pos = kc.sketch(reads, 15, 10, 100)
    t_start = torch.full((len(reads) + 1,), -7, dtype=torch.int64, device=dev)
    t_small = torch.full((want_pos.size - 1,), -7, dtype=torch.int32, device=dev)
    assert kc.sketch_device(t_seq, t_off, t_ln, 15, 10, t_start, t_small, 100) == (ERANGE, want_pos.size)
    assert bool((t_small == -7).all())
    t_pos = torch.full((want_pos.size + 3,), -7, dtype=torch.int32, device=dev)
    assert kc.sketch_device(t_seq, t_off, t_ln, 15, 10, t_start, t_pos, 100) == (0, want_pos.size)
    np.testing.assert_array_equal(t_start.cpu().numpy(), want_start)
    np.testing.assert_array_equal(t_pos.cpu().numpy()[:want_pos.size], want_pos)
    assert t_pos.cpu().numpy()[want_pos.size:].tolist() == [-7] * 3
    host = kc.index_minimizers(reads, 15, 10, 3, 100)
    host_dump = kc.index_dump()
    assert kc.index_minimizers_device(t_seq, t_off, t_ln, 15, 10, 3, 100) == host
    for a, b in zip(kc.index_dump(), host_dump):
        np.testing.assert_array_equal(a, b)


def test_two_calls_on_one_handle_are_independent(kc):
    a, b = [rand(80, 6000), b"C" * 300], [rand(81, 700)]
    ma = check_index(kc, a, 15, 5, 100)
    check_index(kc, b, 11, 19, 3)
    check_sketch(kc, b, 11, 19)
    again = check_index(kc, a, 15, 5, 100)
    assert again["index_entries"] == ma["index_entries"]


def test_lookup_canonicalises_and_rejects_wide_values(kc):
    from genarchbench_amd.kmer import GabError
    k = 9
    reads = [rand(90, 2000)]
    m = check_index(kc, reads, k, 1, 1000)
    fw = np.array([kmer_model.revcomp_value(int(x), k) for x in m["kmers"][:50]], np.uint64)
    first, count, rep = kc.index_lookup(fw)
    np.testing.assert_array_equal(first, m["start"][:50])
    absent = np.setdiff1d(np.arange(4 ** k, dtype=np.uint64), np.concatenate([m["kmers"], m["repetitive"]]))[:20]
    absent = absent[[kmer_model.revcomp_value(int(x), k) not in set(m["kmers"].tolist()) for x in absent]]
    first, count, rep = kc.index_lookup(absent)
    assert (first == -1).all() and (count == 0).all() and (rep == 0).all()
    with pytest.raises(GabError) as e:
        kc.index_lookup(np.array([1, 4 ** k], np.uint64))
    assert e.value.code == EINVAL and "k-mer 1 " in str(e.value)
