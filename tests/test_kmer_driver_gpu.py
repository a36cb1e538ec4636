"""GPU: the drop-in kmer-cnt driver (benchmarks/kmer-cnt/kmer-cnt) end to end: the reference's CLI and stderr lines on the two
fixtures against the reference's recorded numbers, the config parser, the error exits, several files, bytes outside ACGTacgt."""
import json
import os
import re
import subprocess

import pytest

from tests import kmer_model
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "benchmarks", "kmer-cnt", "kmer-cnt")
CFG = os.path.join(ROOT, "benchmarks", "kmer-cnt", "config", "raw_reads.cfg")
CFGS = os.path.join(GOLDEN, "kmer_cfg")
EXPECTED = json.load(open(f"{GOLDEN}/kmer_expected.json"))
CASES = [(name, int(k)) for name, f in sorted(EXPECTED["files"].items()) for k in sorted(f["k"], key=int)]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "benchmarks"), "-s", "kmer-cnt/kmer-cnt"])


def run(*args, debug=True):
    return subprocess.run([EXE, *args] + (["--debug"] if debug else []), capture_output=True, text=True, timeout=300)


def printed(r):
    assert r.returncode == 0, r.stderr[-800:]
    hs = re.findall(r"Hash size: (\d+)$", r.stderr, re.M)
    tk = re.findall(r"Total k-mers (\d+)$", r.stderr, re.M)
    assert len(hs) == 1 and len(tk) == 1, r.stderr[-800:]
    assert re.search(r"^Kernel time: \d+\.\d{3} sec$", r.stderr, re.M)
    return int(hs[0]), int(tk[0])


@pytest.mark.parametrize("name,k", CASES)
def test_fixtures_print_the_reference_numbers(name, k):
    """kmer_small_n.fq.gz: gzip FASTQ with N bytes in kept and in filtered reads.  The reference's source reads as
    if such bytes were replaced through rand(), in file order; on a 64-bit machine it never calls rand() (tests/kmer_model.py,
    unknown_to_t), and the numbers it printed -- which this test holds the driver to -- come from what its 2-bit packing makes of
    such bytes."""
    want = EXPECTED["files"][name]["k"][str(k)]
    assert printed(run("--reads", f"{GOLDEN}/{name}", "--config", CFG, "--kmer", str(k), "--threads", "4")) == (want["hash_size"], want["total_kmers"])


def test_config_gives_k_and_kmer_overrides_it():
    name = "kmer_small.fa"
    rows = EXPECTED["files"][name]["k"]
    assert printed(run("--reads", f"{GOLDEN}/{name}", "--config", CFG)) == (rows["17"]["hash_size"], rows["17"]["total_kmers"])      # kmer_size = 17
    assert printed(run("--reads", f"{GOLDEN}/{name}", "--config", CFG, "--kmer", "11")) == (rows["11"]["hash_size"], rows["11"]["total_kmers"])


def test_include_and_override_in_config():
    """include_outer.cfg includes sub/base.cfg (kmer_size = 11) relative to itself and then sets kmer_size = 15"""
    name = "kmer_small.fa"
    want = EXPECTED["files"][name]["k"]["15"]
    r = run("--reads", f"{GOLDEN}/{name}", "--config", os.path.join(CFGS, "include_outer.cfg"))
    assert printed(r) == (want["hash_size"], want["total_kmers"])
    assert "sub/base.cfg" in r.stderr and "Running with k-mer size: 15" in r.stderr
    # the same through a relative path from another directory
    r = subprocess.run([EXE, "--reads", f"{GOLDEN}/{name}", "--config", "kmer_cfg/include_outer.cfg", "--debug"], cwd=GOLDEN, capture_output=True, text=True)
    assert printed(r) == (want["hash_size"], want["total_kmers"])


def test_without_debug_only_the_kernel_time(tmp_path):
    log = tmp_path / "run.log"
    r = run("--reads", f"{GOLDEN}/kmer_small.fa", "--config", CFG, "--log", str(log), debug=False)
    assert r.returncode == 0 and "Total k-mers" not in r.stderr and re.search(r"^Kernel time: \d+\.\d{3} sec$", r.stderr, re.M)
    want = EXPECTED["files"]["kmer_small.fa"]["k"]["17"]
    assert "Total k-mers %d" % want["total_kmers"] in log.read_text()      # the log file gets the debug lines regardless


def test_error_exits():
    reads = f"{GOLDEN}/kmer_small.fa"
    r = run("--reads", reads, "--config", os.path.join(CFGS, "minimizers.cfg"))
    assert r.returncode != 0 and "use_minimizers" in r.stderr and "Kernel time" not in r.stderr
    for args in (("--config", os.path.join(CFGS, "k18.cfg")), ("--config", CFG, "--kmer", "18"), ("--config", CFG, "--kmer", "0")):
        r = run("--reads", reads, *args)
        assert r.returncode != 0 and "k-mer size" in r.stderr and "Kernel time" not in r.stderr
    r = run("--reads", reads)
    assert r.returncode == 1 and "Usage" in r.stderr
    r = run("--reads", reads, "--config", os.path.join(CFGS, "no_such.cfg"))
    assert r.returncode != 0 and "Can't open config file" in r.stderr
    r = run("--reads", reads + ".txt", "--config", CFG)
    assert r.returncode != 0 and "Can't identify input file type" in r.stderr


def test_two_files_equal_the_model_on_their_concatenation():
    """a comma-separated list of two files, in both orders; also the reference's recorded numbers for that run"""
    both = EXPECTED["both_files_k15"]
    paths = [f"{GOLDEN}/{n}" for n in both["order"]]
    got = printed(run("--reads", ",".join(paths), "--config", CFG, "--kmer", "15"))
    m = kmer_model.model_files(paths, 15)
    assert got == (m["hash_size"], m["total_kmers"]) == (both["hash_size"], both["total_kmers"])
    got = printed(run("--reads", ",".join(paths[::-1]), "--config", CFG, "--kmer", "15"))
    m = kmer_model.model_files(paths[::-1], 15)
    assert got == (m["hash_size"], m["total_kmers"])


def test_min_read_raises_the_length_filter():
    paths = [f"{GOLDEN}/kmer_small.fa"]
    for extra, min_len in ((("--min-read", "9000"), 9000), (("--min-read", "100"), 5000), (("--min-ovlp", "0", "--min-read", "100"), 100)):
        got = printed(run("--reads", paths[0], "--config", CFG, "--kmer", "15", *extra))
        m = kmer_model.model_files(paths, 15, min_len)
        assert got == (m["hash_size"], m["total_kmers"])
