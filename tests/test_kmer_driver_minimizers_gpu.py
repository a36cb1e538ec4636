"""GPU: the kmer-cnt driver in minimizer mode (use_minimizers = 1): the reference's debug lines, in its order, on the two fixtures
against what the reference printed (tests/golden/kmer_minimizer_expected.json) -- integers exact, float strings equal."""
import json
import os
import re
import subprocess

import pytest

from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "benchmarks", "kmer-cnt", "kmer-cnt")
CFG_DIR = os.path.join(ROOT, "benchmarks", "kmer-cnt", "config")
EXPECTED = json.load(open(f"{GOLDEN}/kmer_minimizer_expected.json"))
POINTS = [(15, 10, 100), (11, 5, 3), (17, 19, 3)]      # three points of the grid: both rates, the smallest and the largest k and window
LABELS = ("Mean k-mer frequency:", "Repetitive k-mer frequency:", "Filtered ", "Sorting k-mer index", "Selected k-mers:", "K-mer index size:",
          "Mean k-mer frequency:", "Minimizer rate:")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "benchmarks"), "-s", "kmer-cnt/kmer-cnt"])


def write_cfg(tmp_path, k, window, rate, name="mini.cfg", leave_out=()):
    keys = {"kmer_size": k, "use_minimizers": 1, "minimizer_window": window, "repeat_kmer_rate": rate, "assemble_kmer_sample": 1}
    path = tmp_path / name
    path.write_text("".join("%s = %g\n" % (key, v) for key, v in keys.items() if key not in leave_out))
    return str(path)


def run(*args, debug=True, env=None):
    return subprocess.run([EXE, *args] + (["--debug"] if debug else []), capture_output=True, text=True, timeout=300, env=env)


def index_lines(r):
    """the reference's eight lines of the index build, in the order they were printed"""
    assert r.returncode == 0, r.stderr[-800:]
    assert re.search(r"^Kernel time: \d+\.\d{3} sec$", r.stderr, re.M)
    text = [ln.split("DEBUG: ", 1)[1] for ln in r.stderr.splitlines() if "DEBUG: " in ln]
    got = [ln for ln in text if ln.startswith(LABELS)]
    assert [ln.startswith(lab) for ln, lab in zip(got, LABELS)] == [True] * len(LABELS) and len(got) == len(LABELS), got
    return got


def expected_lines(row):
    return ["Mean k-mer frequency: %s" % row["mean_frequency"], "Repetitive k-mer frequency: %d" % row["repetitive_frequency"],
            "Filtered %d repetitive k-mers (%s)" % (row["filtered_entries"], row["filtered_rate"]), "Sorting k-mer index",
            "Selected k-mers: %d" % row["selected_kmers"], "K-mer index size: %d" % row["index_entries"],
            "Mean k-mer frequency: %s" % row["mean_frequency_kept"], "Minimizer rate: %s" % row["minimizer_rate"]]


def row_of(name, k, window, rate):
    return next(r for r in EXPECTED["files"][name]["rows"] if (r["k"], r["window"], r["rate"]) == (k, window, rate))


@pytest.mark.parametrize("name", sorted(EXPECTED["files"]))
@pytest.mark.parametrize("k,window,rate", POINTS)
def test_fixtures_print_the_reference_lines(tmp_path, name, k, window, rate):
    r = run("--reads", f"{GOLDEN}/{name}", "--config", write_cfg(tmp_path, k, window, rate), "--threads", "4")
    assert index_lines(r) == expected_lines(row_of(name, k, window, rate))
    assert "Hash size" not in r.stderr and "Total k-mers" not in r.stderr


def test_shipped_config_and_kmer_override():
    """config/minimizers.cfg includes raw_reads.cfg (k = 17, window 10, rate 100) and switches the mode on; --kmer overrides k"""
    cfg = os.path.join(CFG_DIR, "minimizers.cfg")
    name = "kmer_small.fa"
    assert index_lines(run("--reads", f"{GOLDEN}/{name}", "--config", cfg)) == expected_lines(row_of(name, 17, 10, 100))
    assert index_lines(run("--reads", f"{GOLDEN}/{name}", "--config", cfg, "--kmer", "15")) == expected_lines(row_of(name, 15, 10, 100))


def test_without_debug_only_the_kernel_time(tmp_path):
    log = tmp_path / "run.log"
    r = run("--reads", f"{GOLDEN}/kmer_small.fa", "--config", write_cfg(tmp_path, 15, 10, 100), "--log", str(log), debug=False)
    assert r.returncode == 0 and re.search(r"^Kernel time: \d+\.\d{3} sec$", r.stderr, re.M)
    assert "k-mer" not in r.stderr and "DEBUG" not in r.stderr and "Minimizer" not in r.stderr
    assert "K-mer index size: %d" % row_of("kmer_small.fa", 15, 10, 100)["index_entries"] in log.read_text()      # the log file gets the lines regardless


@pytest.mark.parametrize("missing", ["minimizer_window", "repeat_kmer_rate", "assemble_kmer_sample"])
def test_a_missing_key_exits_before_the_kernel(tmp_path, missing):
    r = run("--reads", f"{GOLDEN}/kmer_small.fa", "--config", write_cfg(tmp_path, 15, 10, 100, leave_out=(missing,)))
    assert r.returncode != 0 and "Kernel time" not in r.stderr
    assert "No such parameter: " + missing in r.stderr and "use_minimizers" in r.stderr


def test_window_out_of_range_exits(tmp_path):
    for w in (0, 256):
        r = run("--reads", f"{GOLDEN}/kmer_small.fa", "--config", write_cfg(tmp_path, 15, w, 100))
        assert r.returncode != 0 and "Kernel time" not in r.stderr and "minimizer" in r.stderr


def test_g2_prints_the_same_numbers(tmp_path):
    cfg = write_cfg(tmp_path, 15, 5, 3)
    # (GAB_GPU_OVERSUBSCRIBE=1 puts the two logical GPUs on the cards there are)
    r = run("--reads", f"{GOLDEN}/kmer_small.fa", "--config", cfg, "-g", "2", env=dict(os.environ, GAB_GPU_OVERSUBSCRIBE="1"))
    assert index_lines(r) == expected_lines(row_of("kmer_small.fa", 15, 5, 3))
    assert "first of the" in r.stderr


def test_counting_mode_still_ignores_the_new_keys(tmp_path):
    """use_minimizers = 0 beside the three keys: the count, as before"""
    cfg = tmp_path / "count.cfg"
    cfg.write_text("kmer_size = 15\nuse_minimizers = 0\nminimizer_window = 10\nrepeat_kmer_rate = 100\nassemble_kmer_sample = 1\n")
    want = json.load(open(f"{GOLDEN}/kmer_expected.json"))["files"]["kmer_small.fa"]["k"]["15"]
    r = run("--reads", f"{GOLDEN}/kmer_small.fa", "--config", str(cfg))
    assert r.returncode == 0 and "Hash size: %d" % want["hash_size"] in r.stderr and "Total k-mers %d" % want["total_kmers"] in r.stderr
    assert "Minimizer rate" not in r.stderr
