"""GPU: the kmer-cnt driver with --solid-index: after the count's two lines, the debug lines of the reference's
buildIndexUnevenCoverage, in its order, against what the reference printed (tests/golden/kmer_solid_expected.json) -- integers exact,
float strings equal; without the flag, the driver's lines are those of the count alone."""
import json
import os
import re
import subprocess

import pytest

from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "benchmarks", "kmer-cnt", "kmer-cnt")
EXPECTED = json.load(open(f"{GOLDEN}/kmer_solid_expected.json"))
COUNTS = json.load(open(f"{GOLDEN}/kmer_expected.json"))
LABELS = ("Hash size:", "Total k-mers", "Mean k-mer frequency:", "Repetitive k-mer frequency:", "Filtered ", "Sorting k-mer index", "Selected k-mers:",
          "Index size:", "Mean k-mer index frequency:")
# the golden rows with MIN_FREQ = 2, the driver's constant (kmer-cnt/kmer_cnt.cpp:228)
POINTS = [(15, .40, 100, 100), (15, .40, 2, 1.5), (11, 0, 100, 1.5), (17, .40, 100, 1.5)]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "benchmarks"), "-s", "kmer-cnt/kmer-cnt"])


def write_cfg(tmp_path, k, top, tandem, rate, leave_out=()):
    keys = {"kmer_size": k, "use_minimizers": 0, "repeat_kmer_rate": rate, "meta_read_top_kmer_rate": top, "meta_read_filter_kmer_freq": tandem}
    path = tmp_path / "solid.cfg"
    path.write_text("".join("%s = %g\n" % (key, v) for key, v in keys.items() if key not in leave_out))
    return str(path)


def run(*args):
    return subprocess.run([EXE, *args, "--debug"], capture_output=True, text=True, timeout=300)


def debug_lines(r):
    assert r.returncode == 0, r.stderr[-800:]
    assert re.search(r"^Kernel time: \d+\.\d{3} sec$", r.stderr, re.M)
    text = [ln.split("DEBUG: ", 1)[1] for ln in r.stderr.splitlines() if "DEBUG: " in ln]
    return [ln for ln in text if ln.startswith(LABELS)]


def row_of(name, k, top, tandem, rate):
    return next(r for r in EXPECTED["files"][name]["rows"]
                if (r["k"], r["min_freq"], r["select_rate"], r["tandem_freq"], r["rate"]) == (k, 2, top, tandem, rate))


def count_lines(name, k):
    want = COUNTS["files"][name]["k"][str(k)]
    return ["Hash size: %d" % want["hash_size"], "Total k-mers %d" % want["total_kmers"]]


@pytest.mark.parametrize("name", sorted(EXPECTED["files"]))
@pytest.mark.parametrize("k,top,tandem,rate", POINTS)
def test_solid_index_prints_the_reference_lines(tmp_path, name, k, top, tandem, rate):
    r = run("--reads", f"{GOLDEN}/{name}", "--config", write_cfg(tmp_path, k, top, tandem, rate), "--solid-index")
    row = row_of(name, k, top, tandem, rate)
    assert debug_lines(r) == count_lines(name, k) + [
        "Mean k-mer frequency: %s" % row["mean_frequency"], "Repetitive k-mer frequency: %d" % row["repetitive_frequency"],
        "Filtered %d repetitive k-mers (%s)" % (row["filtered_entries"], row["filtered_rate"]), "Sorting k-mer index",
        "Selected k-mers: %d" % row["selected_kmers"], "Index size: %d" % row["index_entries"],
        "Mean k-mer index frequency: %s" % row["mean_index_frequency"]]


def test_without_the_flag_the_count_alone(tmp_path):
    """the same config, keys of the solid index and all, without --solid-index: the count's two lines and nothing of the index"""
    name = "kmer_small.fa"
    r = run("--reads", f"{GOLDEN}/{name}", "--config", write_cfg(tmp_path, 15, .40, 100, 100))
    assert debug_lines(r) == count_lines(name, 15)
    assert "Solid index" not in r.stderr and "Sorting" not in r.stderr
    shipped = run("--reads", f"{GOLDEN}/{name}", "--config", os.path.join(ROOT, "benchmarks", "kmer-cnt", "config", "raw_reads.cfg"), "--kmer", "15")
    assert debug_lines(shipped) == count_lines(name, 15)


@pytest.mark.parametrize("missing", ["meta_read_top_kmer_rate", "meta_read_filter_kmer_freq", "repeat_kmer_rate"])
def test_a_missing_key_exits_before_the_kernel(tmp_path, missing):
    r = subprocess.run([EXE, "--reads", f"{GOLDEN}/kmer_small.fa", "--config", write_cfg(tmp_path, 15, .40, 100, 100, leave_out=(missing,)), "--solid-index"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "Kernel time" not in r.stderr and "No such parameter: " + missing in r.stderr
