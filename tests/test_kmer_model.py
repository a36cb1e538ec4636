"""CPU: the numpy model of kmer-cnt (tests/kmer_model.py) against what the reference printed (tests/golden/kmer_expected.json), against
the reference itself where its tree is present, and on handmade cases; the gab_kmer_* family in the header and the library."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import genarchbench_amd
from tests import kmer_model
from tests.util import GOLDEN, has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = json.load(open(f"{GOLDEN}/kmer_expected.json"))
CASES = [(name, int(k)) for name, f in sorted(EXPECTED["files"].items()) for k in sorted(f["k"], key=int)]
REF = os.environ.get("GAB_KMER_REFERENCE", "/root/reference/benchmarks/kmer-cnt")
FAMILY = ["gab_kmer_create", "gab_kmer_destroy", "gab_kmer_reserve", "gab_kmer_count", "gab_kmer_count_device", "gab_kmer_spectrum",
          "gab_kmer_query", "gab_kmer_dump", "gab_kmer_last_stats"]


def test_fixture_files_are_the_recorded_ones():
    for name, f in EXPECTED["files"].items():
        assert hashlib.sha256(open(f"{GOLDEN}/{name}", "rb").read()).hexdigest() == f["sha256"], name
    assert {k for _, k in CASES} == {11, 15, 16, 17} and len(EXPECTED["files"]) == 2


@pytest.mark.parametrize("name,k", CASES)
def test_model_equals_recorded_reference(name, k):
    want = EXPECTED["files"][name]["k"][str(k)]
    m = kmer_model.model_files([f"{GOLDEN}/{name}"], k)
    assert (m["hash_size"], m["total_kmers"]) == (want["hash_size"], want["total_kmers"])


def test_model_two_files_in_one_run():
    want = EXPECTED["both_files_k15"]
    m = kmer_model.model_files([f"{GOLDEN}/{n}" for n in want["order"]], 15)
    assert (m["hash_size"], m["total_kmers"]) == (want["hash_size"], want["total_kmers"])


def test_fixture_covers_what_it_is_for():
    reads = kmer_model.load_reads([f"{GOLDEN}/kmer_small.fa"])
    lens = [len(r) for r in reads]
    assert 5000 in lens and 5001 in lens and min(lens) < 11
    assert any(r != r.upper() for r in reads)
    for k in (11, 15, 16, 17):
        m = kmer_model.model(reads, k)
        assert m["max_count"] >= 512 and ((m["counts"] >= 256) & (m["counts"] < 512)).any()
        assert m["total_kmers"] != m["distinct"]          # the wrap shows in the printed number
    raw = kmer_model.read_records_raw(f"{GOLDEN}/kmer_small_n.fq.gz")
    assert any(b"N" in ln for rec in raw for ln in rec)
    assert any(len(rec[0]) <= 5000 and not kmer_model._valid(rec[0]).all() for rec in raw)


@pytest.fixture(scope="module")
def live_reference(tmp_path_factory):
    if not os.path.isdir(REF) or not shutil.which("g++"):
        pytest.skip("the reference tree is not on this machine")
    tmp = tmp_path_factory.mktemp("kmer_ref")
    exe = str(tmp / "kmer-cnt")
    subprocess.check_call(["g++", "-O3", "-fopenmp", "-std=c++11", "sequence_container.cpp", "sequence.cpp", "vertex_index.cpp", "kmer_cnt.cpp",
                           "-Ilibcuckoo", "-lz", "-lm", "-ldl", "-o", exe], cwd=REF)
    return exe


@pytest.mark.parametrize("name,k,threads", [("kmer_small.fa", 15, 4), ("kmer_small_n.fq.gz", 11, 1)])
def test_model_equals_live_reference(live_reference, name, k, threads):
    """(k = 15 and 11: the reference clears 4^k bytes per run, 16 GiB at k = 17)"""
    r = subprocess.run([live_reference, "--reads", f"{GOLDEN}/{name}", "--config", os.path.join(REF, "config", "asm_raw_reads.cfg"), "--kmer", str(k),
                        "--threads", str(threads), "--debug"], capture_output=True, text=True, check=True)
    got = (int(re.search(r"Hash size: (\d+)", r.stderr).group(1)), int(re.search(r"Total k-mers (\d+)", r.stderr).group(1)))
    m = kmer_model.model_files([f"{GOLDEN}/{name}"], k)
    assert got == (m["hash_size"], m["total_kmers"])
    want = EXPECTED["files"][name]["k"][str(k)]
    assert got == (want["hash_size"], want["total_kmers"])


# ---- handmade cases ---------------------------------------------------------------------------------------------------------------
def _rand_read(seed, n):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


@pytest.mark.parametrize("k", [1, 2, 11, 16, 17])
@pytest.mark.parametrize("length", [17, 18, 40, 300])
def test_a_read_of_length_l_gives_l_minus_k_kmers(k, length):
    m = kmer_model.model([_rand_read(k * 1000 + length, length)], k, min_len=0)
    assert m["positions"] == max(length - k, 0) == int(m["counts"].sum())


def test_length_filter_is_exclusive():
    a, b = _rand_read(1, 5000), _rand_read(2, 5001)
    m = kmer_model.model([a, b], 17)
    assert m["reads_kept"] == 1 and m["positions"] == 5001 - 17


def test_palindromic_kmers_at_even_k():
    # ACGT is its own reverse complement; in ACGTACGTA.. every 4-mer at a position = 0 mod 4 is ACGT
    read = b"ACGT" * 10 + b"A"
    km = kmer_model.canonical_kmers(read, 4)
    acgt = 0b00011011
    assert kmer_model.revcomp_value(acgt, 4) == acgt
    assert (km[0::4] == acgt).all()
    m = kmer_model.model([read], 4, min_len=0)
    assert m["counts"][list(m["kmers"]).index(acgt)] == 10
    # no k-mer of odd length is its own reverse complement (the middle base would have to be its own complement)
    assert all(kmer_model.revcomp_value(x, 3) != x for x in range(64))


def test_kmer_and_its_reverse_complement_count_as_one():
    fwd = _rand_read(7, 60)
    rev = fwd.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
    k = 17
    mf = kmer_model.model([fwd], k, min_len=0)
    both = kmer_model.model([fwd, rev + b"A"], k, min_len=0)      # (+ 1 base: the last k-mer of a read is not visited)
    assert both["distinct"] == mf["distinct"] + 1                 # the one k-mer of fwd that its last position hides
    shared = np.isin(both["kmers"], mf["kmers"])
    assert (both["counts"][shared] == 2 * mf["counts"]).all()
    x = int(mf["kmers"][0])
    assert min(x, kmer_model.revcomp_value(x, k)) == x


@pytest.mark.parametrize("c,total,hashed", [(1, 1, 0), (255, 1, 0), (256, 1, 1), (257, 2, 1), (512, 2, 1), (513, 3, 1), (7832, 31, 1)])
def test_counts_against_the_two_formulas(c, total, hashed):
    """a homopolymer of c + k bases holds one k-mer c times; an 8-bit counter that wraps sees 0 ceil(c / 256) times and
    is seen at 255 once c reaches 256"""
    k = 5
    m = kmer_model.model([b"A" * (c + k)], k, min_len=0)
    assert (m["distinct"], m["max_count"], m["total_kmers"], m["hash_size"]) == (1, c, total, hashed)
    # simulated literally
    byte, saw0, keys = 0, 0, set()
    for _ in range(c):
        if byte == 0:
            saw0 += 1
        elif byte == 255:
            keys.add(0)
        byte = (byte + 1) & 255
    assert (saw0, len(keys)) == (total, hashed)


def test_merges_are_counted_inside_runs_only():
    m = kmer_model.model([b"A" * (200 + 5)], 5, min_len=0)        # 200 equal keys: runs 0-63, 64-127, 128-191, 192-199
    assert m["merged"] == 200 - 4


def test_unknown_bytes_become_t_to_the_end_of_the_32_base_word():
    """the reference's behaviour on a 64-bit machine (kmer_model.unknown_to_t); the recorded numbers of kmer_small_n.fq.gz pin it"""
    read = b"ACGA" * 20
    assert kmer_model.unknown_to_t(read) == read
    assert kmer_model.unknown_to_t(read[:5] + b"N" + read[6:]) == read[:5] + b"T" * 27 + read[32:]
    assert kmer_model.unknown_to_t(read[:31] + b"n" + read[32:]) == read[:31] + b"T" + read[32:]
    assert kmer_model.unknown_to_t(read[:70] + b"-" + read[71:]) == read[:70] + b"T" * 10
    assert kmer_model.unknown_to_t(b"N" + read[1:40] + b"R" + read[41:]) == b"T" * 32 + read[32:40] + b"T" * 24 + read[64:]
    assert all(kmer_model._valid(r).all() for r in kmer_model.load_reads([f"{GOLDEN}/kmer_small_n.fq.gz"]))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_family():
    src = open(os.path.join(ROOT, "include", "gab.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for f in FAMILY:
        assert re.search(r"\b%s\s*\(" % f, src), f"include/gab.h does not declare {f}"
    assert re.search(r"typedef\s+struct\s*\{[^}]*reads_kept[^}]*positions[^}]*distinct[^}]*total_kmers[^}]*hash_size[^}]*max_count[^}]*\}\s*gab_kmer_result", src)


def test_library_exports_the_family():
    lib = genarchbench_amd.lib()
    for f in FAMILY:
        assert hasattr(lib, f), f"libgab_hip.so does not export {f}"


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_create_without_a_gpu_is_enodev():
    lib = genarchbench_amd.lib()
    h = C.c_void_p()
    assert lib.gab_kmer_create(C.c_int(0), C.byref(h)) == -19      # GAB_ENODEV
    assert not h.value
    from genarchbench_amd.kmer import KmerCounter
    with pytest.raises(genarchbench_amd.GabError) as e:
        KmerCounter()
    assert e.value.code == -19
