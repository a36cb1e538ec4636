"""GPU: the kmer-cnt driver with --index-gpus N (use_minimizers = 1): the minimizer index in N key-space partitions, built in two
phases, prints the reference's debug lines, in its order, as the unpartitioned build does (tests/golden/kmer_minimizer_expected.json:
integers exact, float strings equal).  GAB_GPU_OVERSUBSCRIBE=1 puts the N logical GPUs on the cards there are."""
import json
import os
import re
import subprocess

import pytest

from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "benchmarks", "kmer-cnt", "kmer-cnt")
EXPECTED = json.load(open(f"{GOLDEN}/kmer_minimizer_expected.json"))
POINTS = [(15, 10, 100), (11, 5, 3), (17, 19, 3)]      # the three points of tests/test_kmer_driver_minimizers_gpu.py
LABELS = ("Mean k-mer frequency:", "Repetitive k-mer frequency:", "Filtered ", "Sorting k-mer index", "Selected k-mers:", "K-mer index size:",
          "Mean k-mer frequency:", "Minimizer rate:")
ENV = dict(os.environ, GAB_GPU_OVERSUBSCRIBE="1")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "benchmarks"), "-s", "kmer-cnt/kmer-cnt"])


def write_cfg(tmp_path, k, window, rate, use_minimizers=1):
    keys = {"kmer_size": k, "use_minimizers": use_minimizers, "minimizer_window": window, "repeat_kmer_rate": rate, "assemble_kmer_sample": 1}
    path = tmp_path / "mini.cfg"
    path.write_text("".join("%s = %g\n" % (key, v) for key, v in keys.items()))
    return str(path)


def run(*args):
    return subprocess.run([EXE, *args, "--debug"], capture_output=True, text=True, timeout=300, env=ENV)


def debug_text(r):
    return [ln.split("DEBUG: ", 1)[1] for ln in r.stderr.splitlines() if "DEBUG: " in ln]


def index_lines(r):
    """the reference's eight lines of the index build, in the order they were printed; exactly one Kernel time line"""
    assert r.returncode == 0, r.stderr[-800:]
    assert len(re.findall(r"^Kernel time: \d+\.\d{3} sec$", r.stderr, re.M)) == 1 and r.stderr.count("Kernel time") == 1
    got = [ln for ln in debug_text(r) if ln.startswith(LABELS)]
    assert [ln.startswith(lab) for ln, lab in zip(got, LABELS)] == [True] * len(LABELS) and len(got) == len(LABELS), got
    return got


def expected_lines(row):
    return ["Mean k-mer frequency: %s" % row["mean_frequency"], "Repetitive k-mer frequency: %d" % row["repetitive_frequency"],
            "Filtered %d repetitive k-mers (%s)" % (row["filtered_entries"], row["filtered_rate"]), "Sorting k-mer index",
            "Selected k-mers: %d" % row["selected_kmers"], "K-mer index size: %d" % row["index_entries"],
            "Mean k-mer frequency: %s" % row["mean_frequency_kept"], "Minimizer rate: %s" % row["minimizer_rate"]]


def row_of(name, k, window, rate):
    return next(r for r in EXPECTED["files"][name]["rows"] if (r["k"], r["window"], r["rate"]) == (k, window, rate))


@pytest.mark.parametrize("ngpus", [3, 1])
@pytest.mark.parametrize("name", sorted(EXPECTED["files"]))
@pytest.mark.parametrize("k,window,rate", POINTS)
def test_partitioned_index_prints_the_reference_lines(tmp_path, name, k, window, rate, ngpus):
    r = run("--reads", f"{GOLDEN}/{name}", "--config", write_cfg(tmp_path, k, window, rate), "--index-gpus", str(ngpus))
    assert index_lines(r) == expected_lines(row_of(name, k, window, rate))
    text = debug_text(r)
    assert "Building the minimizer index on %d GPU(s), one key-space partition each" % ngpus in text
    parts = [ln for ln in text if ln.startswith("Partition ")]
    assert [ln.split(":")[0] for ln in parts] == ["Partition %d of %d" % (g, ngpus) for g in range(ngpus)]
    row = row_of(name, k, window, rate)
    own = [[int(x) for x in re.match(r"Partition \d+ of \d+: (\d+) minimizers of (\d+) distinct k-mers, (\d+) removed", ln).groups()] for ln in parts]
    assert [sum(col) for col in zip(*own)] == [row["minimizers"], row["distinct"], row["filtered_kmers"]]
    assert "first of the" not in r.stderr and "Hash size" not in r.stderr and "filled" not in r.stderr


@pytest.mark.parametrize("value", ["0", "-2", "x", "65"])
def test_a_bad_value_gives_usage(tmp_path, value):
    r = run("--reads", f"{GOLDEN}/kmer_small.fa", "--config", write_cfg(tmp_path, 15, 10, 100), "--index-gpus", value)
    assert r.returncode == 1 and "Usage: kmer-cnt" in r.stderr and "--index-gpus" in r.stderr and "Kernel time" not in r.stderr


def test_counting_mode_ignores_the_flag(tmp_path):
    cfg = write_cfg(tmp_path, 15, 10, 100, use_minimizers=0)
    want = json.load(open(f"{GOLDEN}/kmer_expected.json"))["files"]["kmer_small.fa"]["k"]["15"]
    plain = run("--reads", f"{GOLDEN}/kmer_small.fa", "--config", cfg)
    flagged = run("--reads", f"{GOLDEN}/kmer_small.fa", "--config", cfg, "--index-gpus", "3")
    for r in (plain, flagged):
        assert r.returncode == 0 and "Hash size: %d" % want["hash_size"] in r.stderr and "Total k-mers %d" % want["total_kmers"] in r.stderr
        assert "Minimizer rate" not in r.stderr and "Counting on 1 GPU(s)" in r.stderr
    # the count's own lines are the same with and without the flag (device times aside); the flag adds one line that says it is ignored
    own = lambda r: [ln for ln in debug_text(r) if ln.startswith(("Hash size", "Total k-mers", "Counting on", "Reads:", "Running with"))]  # noqa: E731
    assert own(plain) == own(flagged)
    assert any("--index-gpus 3 is ignored" in ln for ln in debug_text(flagged)) and "--index-gpus" not in plain.stderr
