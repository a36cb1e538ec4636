#!/usr/bin/env python3
"""Regenerates the golden vectors under tests/golden/ from THE REFERENCE ITSELF.

Runs only in the build container: needs /root/reference (compiled in place into
oracle/_ref/ by `make -C oracle ref`).  Inputs come from the seeded generators in
tools/gen; expected outputs are what the reference binaries print.  Nothing from
the reference's sources is stored here -- only inputs and the outputs it produced.

    python tests/golden/make_golden.py [bsw|chain|bpm|wfa|fmi|live|params ...]
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import pyoracle  # noqa: E402
from tools import gabgen  # noqa: E402

MANIFEST = os.path.join(HERE, "MANIFEST.json")


def _manifest():
    if os.path.exists(MANIFEST):
        return json.load(open(MANIFEST))
    return {}


def _save(m):
    json.dump(m, open(MANIFEST, "w"), indent=1, sort_keys=True)


def make_bsw(m):
    # (name, seed, n, mode): n is a multiple of 32 so no padded pair is printed
    # (bsw/src/main_banded.cpp:254,407-409)
    for name, seed, n, mode in [("bsw_bench", 101, 2048, 0), ("bsw_adv", 102, 1536, 1)]:
        inp = os.path.join(HERE, name + ".in.txt")
        gabgen.write_text("bsw", inp, seed, n, mode)
        outs = {}
        for isa in ("avx512", "avx2", "sse41"):
            exe = pyoracle.ref_path("bsw_ref_" + isa)
            r = subprocess.run([exe, "-pairs", inp, "-t", "1", "-b", "512"], capture_output=True, text=True, check=True)
            outs[isa] = [l for l in r.stderr.splitlines() if "score=" in l][:n]
        assert outs["avx512"] == outs["avx2"] == outs["sse41"], "reference ISA variants disagree"
        with open(os.path.join(HERE, name + ".expected.txt"), "w") as f:
            f.write("\n".join(outs["avx2"]) + "\n")
        # all six fields of the extension result: the driver prints only the score, so the
        # reference's scalarBandedSWAWrapper AND its vector getScores16 are driven by oracle/ref_harness/bsw_full_ref.cpp
        full = {}
        for isa in ("avx512", "avx2"):
            for how in ("scalar", "vector"):
                r = subprocess.run([pyoracle.ref_path("bsw_full_ref_" + isa), inp, how], capture_output=True, text=True, check=True)
                full[isa, how] = r.stdout
        assert len(set(full.values())) == 1, "reference scalar / vector / ISA variants disagree on the full result"
        assert [l.split()[1] for l in full["avx2", "scalar"].splitlines()] == [l.split("=")[1] for l in outs["avx2"]]
        open(os.path.join(HERE, name + ".full.expected.txt"), "w").write(full["avx2", "scalar"])
        m[name] = {"generator": "tools/gen gabgen bsw", "seed": seed, "n": n, "mode": mode,
                   "full_command": "bsw_full_ref_<avx2|avx512> <in> scalar|vector (oracle/ref_harness/bsw_full_ref.cpp on the "
                                   "reference's scalarBandedSWAWrapper and getScores16: identical output) -> '[i] score qle tle gtle gscore max_off'",
                   "reference": "bsw/src/{main_banded,bandedSWA}.cpp built by oracle/Makefile "
                                "(-mavx512bw, -mavx2, -msse4.1: identical output)",
                   "command": "bsw_ref_<isa> -pairs <in> -t 1 -b 512 ; grep score= stderr"}


def make_chain(m):
    # one input serves both benchmarks (fast-chain reads chain's files: fast-chain/scripts/regression_small.sh:4)
    for name, seed, ncalls, mode, nmin, nmax in [("chain_bench", 201, 24, 0, 50, 2000),
                                                 ("chain_dense", 202, 5, 1, 1500, 6000)]:
        inp = os.path.join(HERE, name + ".in.txt")
        gabgen.write_text("chain", inp, seed, ncalls, mode, nmin, nmax)
        outs = {}
        for exe in ("chain_ref", "fastchain_ref_avx2", "fastchain_ref_avx512"):
            out = os.path.join(HERE, name + "." + exe + ".tmp")
            subprocess.run([pyoracle.ref_path(exe), "-i", inp, "-o", out, "-t", "1"], capture_output=True, check=True)
            outs[exe] = open(out).read()
            os.remove(out)
        assert outs["fastchain_ref_avx2"] == outs["fastchain_ref_avx512"], "fast-chain AVX2 != AVX-512"
        open(os.path.join(HERE, name + ".chain.expected.txt"), "w").write(outs["chain_ref"])
        open(os.path.join(HERE, name + ".fastchain.expected.txt"), "w").write(outs["fastchain_ref_avx2"])
        m[name] = {"generator": "tools/gen gabgen chain", "seed": seed, "ncalls": ncalls, "mode": mode,
                   "nmin": nmin, "nmax": nmax,
                   "reference": "chain/src/*.cpp and fast-chain/src/*.cpp built by oracle/Makefile "
                                "(fast-chain: -mavx2 and -mavx512bw builds, identical output)",
                   "command": "<exe> -i <in> -o <out> -t 1"}


def make_bpm(m):
    import re

    def run_ref(inp, alg):
        outs = []
        for t in ("1", "3"):
            out = inp + ".tmp"
            subprocess.run([pyoracle.ref_path("bpm_ref"), "-a", alg, "-i", inp, "-o", out, "-t", t], capture_output=True, check=True)
            lines = sorted(open(out).read().splitlines(), key=lambda l: int(re.match(r"\[(\d+)\]", l).group(1)))
            os.remove(out)
            outs.append(lines)
        assert outs[0] == outs[1], "bpm reference output depends on the thread count"
        return outs[0]

    for name, seed, n, mode, plen in [("bpm_bench", 301, 1500, 0, 151), ("bpm_adv", 302, 2500, 1, 220)]:
        inp = os.path.join(HERE, name + ".in.txt")
        gabgen.write_text("bpm", inp, seed, n, mode, plen)
        open(os.path.join(HERE, name + ".expected.txt"), "w").write("\n".join(run_ref(inp, "bpm-edit")) + "\n")
        # the driver's other two algorithms on the same inputs
        for alg in ("bitpal-edit", "bitpal-scored"):
            open(os.path.join(HERE, f"{name}.{alg.replace('-', '_')}.expected.txt"), "w").write("\n".join(run_ref(inp, alg)) + "\n")
        m[name] = {"generator": "tools/gen gabgen bpm", "seed": seed, "n": n, "mode": mode, "plen": plen,
                   "reference": "bpm/tools/align_benchmark.c + bpm/{benchmark,bitpal,edit,system,utils}/*.c built by oracle/Makefile",
                   "command": "bpm_ref -a bpm-edit|bitpal-edit|bitpal-scored -i <in> -o <out> -t 1|3 ; sort by id (as regression_small.sh:94 does)"}


# adaptive mode: the reduction parameters the adaptive fixtures are produced with
WFA_ADAPTIVE = [(10, 10), (5, 3), (1, 0)]


def make_wfa(m):
    import re

    def run_ref(inp, extra):
        outs = []
        for t in ("1", "3"):
            out = inp + ".tmp"
            subprocess.run([pyoracle.ref_path("wfa_ref"), "-i", inp, "-o", out, "-t", t] + extra, capture_output=True, check=True)
            lines = sorted(open(out).read().splitlines(), key=lambda l: int(re.match(r"id=(\d+)", l).group(1)))
            os.remove(out)
            outs.append(lines)
        assert outs[0] == outs[1], "wfa reference output depends on the thread count"
        return outs[0]

    for name, seed, n, mode, plen in [("wfa_bench", 401, 1500, 0, 151), ("wfa_adv", 402, 2000, 1, 240)]:
        inp = os.path.join(HERE, name + ".in.txt")
        gabgen.write_text("wfa", inp, seed, n, mode, plen)
        open(os.path.join(HERE, name + ".expected.txt"), "w").write("\n".join(run_ref(inp, [])) + "\n")
        m[name] = {"generator": "tools/gen gabgen wfa", "seed": seed, "n": n, "mode": mode, "plen": plen,
                   "reference": "wfa/tools/align_benchmark.c + wfa/{gap_affine,utils}/*.c built by oracle/Makefile",
                   "command": "wfa_ref -i <in> -o <out> -t 1|3 ; sort by id (as regression_small.sh:94 does)"}
    # the same adversarial input through the reference's adaptive reduction
    inp = os.path.join(HERE, "wfa_adv.in.txt")
    for mwl, mdd in WFA_ADAPTIVE:
        lines = run_ref(inp, ["--minimum-wavefront-length", str(mwl), "--maximum-difference-distance", str(mdd)])
        open(os.path.join(HERE, f"wfa_adv.adaptive_{mwl}_{mdd}.expected.txt"), "w").write("\n".join(lines) + "\n")
    m["wfa_adv"]["adaptive_command"] = ("wfa_ref -i <in> -o <out> -t 1|3 --minimum-wavefront-length L --maximum-difference-distance D "
                                        "for (L, D) in " + repr(WFA_ADAPTIVE))


def make_fmi(m):
    # 100 kb reference with planted repeats, 1200 reads of 60..151 bp (2 % substitutions, N's, both strands).
    # batch 64 keeps the reference clear of its realloc / dangling-pointer path.
    name, rseed, qseed, L, n = "fmi_small", 501, 502, 100000, 1200
    ref = gabgen.fmi_ref(rseed, L, 5)
    reads = gabgen.fmi_reads(qseed, ref, n, 60, 151)
    fa = os.path.join(HERE, name + ".ref.fa"); fq = os.path.join(HERE, name + ".reads.fq")
    gabgen.fmi_write_fasta(fa, ref); gabgen.fmi_write_fastq(fq, reads)
    subprocess.run([pyoracle.ref_path("bwa_mem2_index_ref"), "index", fa], capture_output=True, check=True)
    outs = []
    for batch, t in (("64", "1"), ("32", "2")):
        r = subprocess.run([pyoracle.ref_path("fmi_ref"), fa, fq, batch, "19", t], capture_output=True, text=True, check=True)
        lines = r.stdout.splitlines()
        assert not any("realloc" in l for l in lines[:8]), "reference hit its realloc path"
        outs.append("\n".join(lines[6:]) + "\n")          # the harness also drops the 6 header lines
    assert outs[0] == outs[1], "fmi reference output depends on batch size / threads"
    open(os.path.join(HERE, name + ".expected.txt"), "w").write(outs[0])
    # keep only the index header words as a fixture for the index builder (the full file is rebuilt in tests)
    import hashlib
    idx = open(fa + ".bwt.2bit.64", "rb").read()
    m[name] = {"generator": "tools/gen gab_gen_fmi_ref/_reads", "ref_seed": rseed, "read_seed": qseed, "ref_len": L, "n": n,
               "rl_min": 60, "rl_max": 151, "index_sha256": hashlib.sha256(idx).hexdigest(), "index_bytes": len(idx),
               "reference": "fmi/fmi.cpp + bwa-mem2 library, and bwa-mem2 index, built by oracle/Makefile (clang++)",
               "command": "bwa_mem2_index_ref index <fa>; fmi_ref <fa> <fq> 64 19 1 ; drop 6 header lines"}
    # suffix-array look-up: the driver never calls it, so the reference's own
    # FMI_search::get_sa_entries is driven by oracle/ref_harness/fmi_sa_ref.cpp on the SMEMs of this fixture
    import numpy as np
    oidx = pyoracle.fmi_load(fa)
    sm, off = pyoracle.fmi(oidx, reads, 19)
    assert pyoracle.fmi_text(sm, off) == outs[0], "oracle SMEMs differ from the reference's"
    smf = os.path.join(HERE, "_smems.bin"); cof = os.path.join(HERE, "_coords.bin")
    sm.tofile(smf)
    with open(os.path.join(HERE, name + ".sa_expected.txt"), "w") as f:
        for max_occ in (500, 2):
            subprocess.run([pyoracle.ref_path("fmi_sa_ref"), fa, smf, str(max_occ), cof], capture_output=True, check=True)
            co = np.fromfile(cof, np.int64)
            f.write(f"max_occ {max_occ} {len(co)}\n" + "\n".join(str(int(v)) for v in co) + "\n")
    os.remove(smf); os.remove(cof)
    m[name]["sa_command"] = "fmi_sa_ref <fa> <oracle SMEMs of the fixture, 40-byte records> <max_occ> <out> for max_occ 500 and 2"
    for ext in (".0123", ".amb", ".ann", ".pac", ".bwt.2bit.64"):
        os.remove(fa + ext)


def make_live(m):
    """the reference's outputs for the inputs the test_*_matches_live_reference tests generate (they compare the oracle with
    these, and with the reference itself where oracle/_ref is built), as arrays in one compressed live.npz; the inputs are not
    stored: the generators reproduce them"""
    import tempfile
    import numpy as np
    from tests.util import read_bsw_full, read_chain_output, read_scores
    out = {}
    with tempfile.TemporaryDirectory() as td:
        p, o = os.path.join(td, "in.txt"), os.path.join(td, "out.txt")
        gabgen.write_text("bsw", p, 993, 4096, 1)
        full = {how: subprocess.run([pyoracle.ref_path("bsw_full_ref_avx2"), p, how], capture_output=True, text=True, check=True).stdout
                for how in ("scalar", "vector")}
        assert full["scalar"] == full["vector"], "reference scalar / vector disagree on the full result"
        open(o, "w").write(full["scalar"])
        out["bsw_full"] = read_bsw_full(o)
        gabgen.write_text("bsw", p, 991, 4096, 1)
        r = subprocess.run([pyoracle.ref_path("bsw_ref_avx2"), "-pairs", p, "-t", "2", "-b", "256"], capture_output=True, text=True, check=True)
        open(o, "w").write("\n".join([l for l in r.stderr.splitlines() if "score=" in l][:4096]) + "\n")
        out["bsw_scores"] = read_scores(o)
        m["bsw_live"] = {"generator": "tools/gen gabgen bsw", "mode": 1, "n": 4096, "seed": {"full": 993, "scores": 991},
                         "command": "bsw_ref_avx2 -pairs <in> -t 2 -b 256 ; grep score= stderr -> live.npz bsw_scores",
                         "full_command": "bsw_full_ref_avx2 <in> scalar|vector (identical output) -> live.npz bsw_full [n, 6]"}
        gabgen.write_text("chain", p, 77, 12, 1, 800, 7000)
        for tag, exe in (("chain", "chain_ref"), ("fastchain", "fastchain_ref_avx2")):
            subprocess.run([pyoracle.ref_path(exe), "-i", p, "-o", o, "-t", "2"], capture_output=True, check=True)
            out[f"{tag}_score"], out[f"{tag}_parent"] = read_chain_output(o)
        m["chain_live"] = {"generator": "tools/gen gabgen chain", "seed": 77, "ncalls": 12, "mode": 1, "nmin": 800, "nmax": 7000,
                           "command": "chain_ref | fastchain_ref_avx2 -i <in> -o <out> -t 2 -> live.npz {chain,fastchain}_{score,parent}"}
        ref = gabgen.fmi_ref(71, 60000, 10)
        reads = gabgen.fmi_reads(72, ref, 800, 30, 200)
        fa, fq = os.path.join(td, "r.fa"), os.path.join(td, "q.fq")
        gabgen.fmi_write_fasta(fa, ref); gabgen.fmi_write_fastq(fq, reads)
        subprocess.run([pyoracle.ref_path("bwa_mem2_index_ref"), "index", fa], capture_output=True, check=True)
        r = subprocess.run([pyoracle.ref_path("fmi_ref"), fa, fq, "32", "19", "1"], capture_output=True, text=True, check=True)
        lines = r.stdout.splitlines()
        assert not any("realloc" in l for l in lines[:8])
        out["fmi_text"] = np.frombuffer(("\n".join(lines[6:]) + "\n").encode(), np.uint8)
        m["fmi_live"] = {"generator": "tools/gen gabgen fmi_ref(71, 60000, 10) + fmi_reads(72, ref, 800, 30, 200)",
                         "command": "bwa_mem2_index_ref index <fa> ; fmi_ref <fa> <fq> 32 19 1 ; stdout from line 7 on -> live.npz fmi_text (bytes)"}
    np.savez_compressed(os.path.join(HERE, "live.npz"), **out)


def make_params(m):
    """the reference's scalarBandedSWA (all six fields) at every parameter set of tests/util.py BSW_PARAM_SETS, on the pairs of
    tests/util.py bsw_param_input(), as one int32 array [set, pair, field] in bsw_params.npz (the inputs are not stored: the
    generators and the hand-made list reproduce them).  Off the driver's defaults the reference's vector getScores16 does not
    always agree with its own scalar path: the rows where it differs are counted per set in MANIFEST.json"""
    import tempfile
    import numpy as np
    from tests.util import BSW_PARAM_SETS, bsw_full_ref_params_line, bsw_param_input, read_bsw_full
    batch = bsw_param_input()
    scalar, vdiff, vdiff_score = [], [], []
    with tempfile.TemporaryDirectory() as td:
        p, o = os.path.join(td, "in.txt"), os.path.join(td, "out.txt")
        batch.write_text(p)
        for ps in BSW_PARAM_SETS:
            res = {}
            for isa in ("avx2", "avx512"):
                for how in ("scalar", "vector"):
                    r = subprocess.run([pyoracle.ref_path("bsw_full_ref_" + isa), p, how] + [str(v) for v in ps],
                                       capture_output=True, text=True, check=True)
                    assert bsw_full_ref_params_line(*ps) in r.stderr, "oracle/_ref predates the harness's parameters: rebuild it"
                    open(o, "w").write(r.stdout)
                    res[isa, how] = read_bsw_full(o)
            assert np.array_equal(res["avx2", "scalar"], res["avx512", "scalar"]), "reference scalar path depends on the ISA build"
            s, v = res["avx2", "scalar"], res["avx2", "vector"]
            assert s.shape == (batch.n, 6)
            scalar.append(s)
            vdiff.append(int((s != v).any(axis=1).sum()))
            vdiff_score.append(int((s[:, 0] != v[:, 0]).sum()))
    np.savez_compressed(os.path.join(HERE, "bsw_params.npz"), sets=np.array(BSW_PARAM_SETS, np.int32), full=np.stack(scalar))
    m["bsw_params"] = {"input": "tests/util.py bsw_param_input(): gabgen bsw (995, 1024, mode 1) + (996, 256, mode 0) + bsw_handmade_pairs()",
                       "n": int(batch.n), "sets": "tests/util.py BSW_PARAM_SETS (a b ambig o_del e_del o_ins e_ins zdrop end_bonus w)",
                       "command": "bsw_full_ref_<avx2|avx512> <in> scalar <set> (identical output) -> bsw_params.npz full [set, pair, 6]",
                       "vector_rows_differing": vdiff, "vector_scores_differing": vdiff_score,
                       "vector_command": "bsw_full_ref_avx2 <in> vector <set>: rows where getScores16 differs from scalarBandedSWA, per set"}


MAKERS = {"bsw": make_bsw, "chain": make_chain, "bpm": make_bpm, "wfa": make_wfa, "fmi": make_fmi, "live": make_live, "params": make_params}

if __name__ == "__main__":
    pyoracle.build(with_ref=True)
    which = sys.argv[1:] or list(MAKERS)
    m = _manifest()
    for w in which:
        MAKERS[w](m)
    _save(m)
    print("golden vectors written:", ", ".join(sorted(m)))
