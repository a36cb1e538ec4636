"""GPU: the kmer-cnt driver on several logical GPUs (-g N / $GAB_GPUS), each counting one partition of the key space: the printed
numbers are the reference's recorded ones whatever N is.  GAB_GPU_OVERSUBSCRIBE=1 puts the logical GPUs on the cards there are."""
import json
import os
import re
import subprocess

import pytest

from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "benchmarks", "kmer-cnt", "kmer-cnt")
CFG = os.path.join(ROOT, "benchmarks", "kmer-cnt", "config", "raw_reads.cfg")
EXPECTED = json.load(open(f"{GOLDEN}/kmer_expected.json"))
CASES = [(name, k) for name in sorted(EXPECTED["files"]) for k in (15, 17)]
# (extra arguments, extra environment, logical GPUs the run must report)
RUNS = {"g3": (["-g", "3"], {}, 3), "env2": ([], {"GAB_GPUS": "2"}, 2), "g1": (["-g", "1"], {"GAB_GPUS": "5"}, 1)}


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "benchmarks"), "-s", "kmer-cnt/kmer-cnt"])


def run(args, env):
    e = dict(os.environ, GAB_GPU_OVERSUBSCRIBE="1")
    e.pop("GAB_GPUS", None)
    e.update(env)
    return subprocess.run([EXE, *args, "--debug"], capture_output=True, text=True, timeout=300, env=e)


@pytest.mark.parametrize("how", sorted(RUNS))
@pytest.mark.parametrize("name,k", CASES)
def test_prints_the_reference_numbers_on_any_number_of_gpus(name, k, how):
    args, env, gpus = RUNS[how]
    want = EXPECTED["files"][name]["k"][str(k)]
    r = run(["--reads", f"{GOLDEN}/{name}", "--config", CFG, "--kmer", str(k), "--threads", "4", *args], env)
    assert r.returncode == 0, r.stderr[-800:]
    hs = re.findall(r"Hash size: (\d+)$", r.stderr, re.M)
    tk = re.findall(r"Total k-mers (\d+)$", r.stderr, re.M)
    assert (hs, tk) == ([str(want["hash_size"])], [str(want["total_kmers"])]), r.stderr[-800:]
    assert len(re.findall(r"^Kernel time: \d+\.\d{3} sec$", r.stderr, re.M)) == 1 and r.stderr.count("Kernel time") == 1
    assert "Counting on %d GPU(s)" % gpus in r.stderr
    assert "counted again" not in r.stderr          # no partition filled its first table (tests/test_kmer_parts_model.py)


def test_usage_names_the_flag_and_bad_values_are_refused():
    r = run(["-h"], {})
    assert r.returncode == 0 and "--gpus" in r.stderr and "one GPU" not in r.stderr
    r = run(["--reads", f"{GOLDEN}/kmer_small.fa", "--config", CFG, "--gpus", "2"], {"GAB_GPUS": "7"})      # the long form; the flag beats $GAB_GPUS
    assert r.returncode == 0 and "Counting on 2 GPU(s)" in r.stderr
    for bad in ("0", "-2", "x"):
        r = run(["--reads", f"{GOLDEN}/kmer_small.fa", "--config", CFG, "-g", bad], {})
        assert r.returncode == 1 and "Usage" in r.stderr and "Kernel time" not in r.stderr
