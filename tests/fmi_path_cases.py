"""fmi: the inputs of tests/test_fmi_paths_gpu.py -- one row per route of genarchbench_amd/csrc/fmi.hip (LDS or global lists, ring
spill, list entry format, short-pattern table depth, hand-over of wide phases, queues full, pass 1 overflowing the slot, second
round in parts, several batches, output growth, stride edges).

A row is Case(name, input, msl, env, want, weak): `input` names a seeded (reference, reads) builder of INPUTS, `env` the GAB_FMI_*
knobs of the run, `want(paths, extra)` what the CPU model (oracle.pyoracle.fmi_paths) must show for the row to count as exercising its
route -- asserted in tests/test_fmi_paths_model.py, so a row that stops reaching its route fails there, without a GPU.  `weak`: the
hand-over queues run full, which phases get a place depends on timing, and only what always holds is asserted (1); 2: whichever
phase gets the place, its candidates outgrow their queue and the batch runs again without hand-over."""
import functools
from collections import namedtuple

import numpy as np

from tools import gabgen, mkindex

Case = namedtuple("Case", "name input msl env want weak", defaults=(0,))
SLOT_CAP = 48            # records of a first-round output slot
OUT_PER_READ = 16        # records per read the output array starts with


def _rand(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _revcomp(a):
    return (3 - a[::-1]).astype(np.uint8)


def _batch(reads, stride):
    enc = np.full((len(reads), stride), 4, np.uint8); ln = np.zeros(len(reads), np.int32)
    for i, r in enumerate(reads):
        enc[i, :len(r)] = r; ln[i] = len(r)
    return gabgen.ReadBatch(enc, ln)


def nested_ref(seed=701):
    """nested copies of one 200-base word S (copy i = S[100 - a_i : 100 + b_i], a_i = 40 + (7 i mod 23), b_i = 10 + 2 i), 50 random
    bases after each, then 5 000 random bases: a read from S keeps one list entry per distinct copy length -> (ref, S)"""
    rng = np.random.default_rng(seed)
    S = _rand(rng, 200)
    parts = []
    for i in range(40):
        parts += [S[100 - (40 + 7 * i % 23):100 + 10 + 2 * i], _rand(rng, 50)]
    return np.concatenate(parts + [_rand(rng, 5000)]), S


def nested_reads(S, seed, n, lo=100, hi=151):
    """substrings of S of lo..hi bases, up to two substitutions, a third of them reverse-complemented"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(lo, hi + 1)); st = int(rng.integers(0, len(S) - ln + 1))
        r = S[st:st + ln].copy()
        for p in rng.integers(0, ln, int(rng.integers(0, 3))):
            r[p] = (r[p] + 1 + rng.integers(0, 3)) & 3
        out.append(_revcomp(r) if i % 3 == 2 else r)
    return out


def pieces_reads(ref, seed, n, lo, hi, piece):
    """reads of lo..hi bases made of `piece`-base substrings of the reference separated by one N: every piece is an SMEM of pass 1"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        r = np.full(ln, 4, np.uint8)
        for p in range(0, ln - piece + 1, piece + 1):
            st = int(rng.integers(0, len(ref) - piece)); r[p:p + piece] = ref[st:st + piece]
        out.append(r)
    return out


def _nested():
    ref, S = nested_ref()
    return ref, _batch(nested_reads(S, 702, 200), 151)


def _plain():
    """300 reads of 151 bases on a 50 kbp reference; some with an N inside the first bases of a pass-3 start, some shorter than the
    table is deep"""
    ref = gabgen.fmi_ref(711, 50_000, 10)
    reads = gabgen.fmi_reads(712, ref, 300, 151, 151)
    for i, p in enumerate((0, 1, 3, 6, 7, 8, 9, 10, 11, 12)):
        reads.enc[10 + i, p] = 4; reads.enc[10 + i, 60 + p] = 4
    for i, ln in enumerate((0, 1, 2, 5, 7, 8, 9, 10, 11, 12)):
        reads.len[30 + i] = ln
    return ref, reads


def _p1_lds():
    ref = _rand(np.random.default_rng(721), 400)
    return ref, _batch(pieces_reads(ref, 722, 64, 240, 256, 4), 256)


def _p1_global(n=64):
    ref = _rand(np.random.default_rng(731), 3000)
    return ref, _batch(pieces_reads(ref, 732, n, 500, 700, 8), 700)


def _batches():
    """2 100 short reads, three batches of 700 at GAB_FMI_BATCH=1024: reads from the nested word (wide phases) and, in the second and
    third batch, reads of 4-base pieces (more SMEMs than a slot holds at minSeedLen 3)"""
    ref, S = nested_ref()
    reads = nested_reads(S, 741, 2100, 60, 151)
    for i, r in zip((5, 800, 1399, 1400, 2099), pieces_reads(ref, 742, 5, 140, 151, 4)):
        reads[i] = r
    return ref, _batch(reads, 151)


def _rerun():
    """64 reads of 100 bases, each with three partial copies in the reference: R[0:60], R[40:100] and R[20:90].  Pass 1 finds R[0:60]
    and goes on at base 60; there the list holds R[60:100] and R[60:90], both survive the first backward column (the read's first
    column with two survivors, and a pass-1 one), and further back each ends as an SMEM long and rare enough to be re-seeded: two
    candidates from the phase that takes the only place of a one-place queue, whichever read it belongs to"""
    rng = np.random.default_rng(761)
    reads, parts = [], []
    for _ in range(64):
        R = _rand(rng, 100)
        reads.append(R)
        parts += [R[0:60], _rand(rng, 30), R[40:100], _rand(rng, 30), R[20:90], _rand(rng, 30)]
    return np.concatenate(parts), _batch(reads, 100)


def _edge(stride):
    """the same 128 reads at three strides: lengths up to 255 (the odd stride: the last read fills the last row to the last byte of
    the buffer), lengths 0 and 1, an all-N read"""
    ref = gabgen.fmi_ref(751, 50_000, 10)
    a = gabgen.fmi_reads(752, ref, 127, 30, 255)
    last = gabgen.fmi_reads(753, ref, 1, 255, 255)
    reads = [a.enc[i, :a.len[i]].copy() for i in range(127)] + [last.enc[0, :255].copy()]
    reads[0] = reads[0][:0]; reads[1] = reads[1][:1]; reads[2] = np.full(200, 4, np.uint8); reads[3] = reads[3][:255]
    assert len(reads[127]) == 255 and max(len(r) for r in reads) == 255
    return ref, _batch(reads, stride)


INPUTS = {"nested": _nested, "plain": _plain, "p1_lds": _p1_lds, "p1_global": _p1_global, "p1_global_128": lambda: _p1_global(128),
          "batches": _batches, "rerun": _rerun, "edge255": lambda: _edge(255), "edge256": lambda: _edge(256), "edge257": lambda: _edge(257)}


@functools.lru_cache(maxsize=None)
def load(name):
    """-> (mkindex.FmIndex, ReadBatch); built once per process"""
    ref, reads = INPUTS[name]()
    return mkindex.FmIndex(ref), reads


def model_args(env, stride):
    """the knobs of a run as oracle.pyoracle.fmi_paths takes them (what gab_fmi_seed_device makes of the environment)"""
    wide = int(env.get("GAB_FMI_WIDE", 1))
    return dict(ring=int(env.get("GAB_FMI_LDS_ENTRIES", 12)), depth=min(11, int(env.get("GAB_FMI_KMER_DEPTH", 8))),
                wide_min=0 if wide == 0 else 24 if wide == 1 else wide, lds_form=stride <= 256,
                batch=int(env.get("GAB_FMI_BATCH", 1 << 24)), scratch_bytes=int(env["GAB_FMI_SCRATCH_MB"]) << 20 if "GAB_FMI_SCRATCH_MB" in env else 6 << 30,
                wide_lists=env.get("GAB_FMI_WIDE_LISTS", "0") != "0")


def _cases():
    c = []
    # hand-over of wide backward phases: at the shipping threshold, off, and with the threshold lowered
    c.append(Case("handover_default", "nested", 19, {}, lambda p, x: p["wide_min"] == 24 and p["wide_items"] >= 100 and p["wide_cands"] > 0))
    c.append(Case("handover_off", "nested", 19, {"GAB_FMI_WIDE": "0"}, lambda p, x: p["wide_items"] == 0 and x["widest_column"] >= 24))
    c.append(Case("handover_4", "nested", 19, {"GAB_FMI_WIDE": "4"}, lambda p, x: p["wide_items"] >= 100))
    c.append(Case("handover_2", "nested", 19, {"GAB_FMI_WIDE": "2"}, lambda p, x: p["wide_items"] >= 100))
    # the LDS ring and its spill, both list entry formats
    for wl in ({}, {"GAB_FMI_WIDE_LISTS": "1"}):
        tag = "_16B" if wl else "_13B"
        c.append(Case("ring_4" + tag, "nested", 19, dict(wl, GAB_FMI_LDS_ENTRIES="4"), lambda p, x: p["spills"] >= 100))
        c.append(Case("ring_12" + tag, "nested", 19, dict(wl, GAB_FMI_LDS_ENTRIES="12"), lambda p, x: p["spills"] > 0))
    # the short-pattern table: none, no jump, <= 8 and > 8 bases, and a jump switched off by minSeedLen + 1 <= depth.  (Depth 1 holds
    # the four single bases: those are the start intervals, never the result of an extension, so the table is built but not read.)
    for d in (0, 1, 2, 7, 8, 9, 11):
        c.append(Case(f"depth_{d}", "plain", 19, {"GAB_FMI_KMER_DEPTH": str(d)}, (lambda p, x, d=d: (p["table_ext"] == 0) == (d <= 1))))
    for d in (8, 11):
        c.append(Case(f"depth_{d}_msl5", "plain", 5, {"GAB_FMI_KMER_DEPTH": str(d)}, lambda p, x: p["table_ext"] > 0))
    # pass 1 alone overflows the 48-record slot; the output array grows
    c.append(Case("p1_overflow_lds", "p1_lds", 3, {}, lambda p, x: x["p1_over_reads"] >= 32 and p["out_growths"] >= 1 and p["form"] == 1))
    c.append(Case("p1_overflow_global", "p1_global", 5, {}, lambda p, x: x["p1_over_reads"] >= 32 and p["form"] == 0))
    c.append(Case("p1_overflow_global_1mb", "p1_global", 5, {"GAB_FMI_SCRATCH_MB": "1"}, lambda p, x: x["p1_over_reads"] >= 32 and p["second_round_parts"] >= 1))
    c.append(Case("second_round_in_parts", "p1_global_128", 5, {"GAB_FMI_SCRATCH_MB": "1"}, lambda p, x: p["second_round_parts"] >= 2))
    # several batches, an overflowing read in a later one, hand-over on
    c.append(Case("three_batches", "batches", 3, {"GAB_FMI_BATCH": "1024"},
                  lambda p, x: p["batches"] == 3 and p["wide_items"] > 0 and (x["per_read"][700:] > SLOT_CAP).any()))
    # stride edges: last LDS form, first global form, an odd stride whose last read ends at the last byte of the buffer
    c.append(Case("stride_255", "edge255", 19, {}, lambda p, x: p["form"] == 1))
    c.append(Case("stride_256", "edge256", 19, {}, lambda p, x: p["form"] == 1))
    c.append(Case("stride_257", "edge257", 19, {}, lambda p, x: p["form"] == 0))
    # queues full: the model is that of the run with room for everything -- it must want more places than the run has
    c.append(Case("queue_8_at_4", "nested", 19, {"GAB_FMI_WIDE": "4", "GAB_FMI_WIDE_CAP": "8"}, lambda p, x: p["wide_items"] > 8, 1))
    c.append(Case("queue_3_at_2", "nested", 19, {"GAB_FMI_WIDE": "2", "GAB_FMI_WIDE_CAP": "3"}, lambda p, x: p["wide_items"] > 3, 1))
    # ... and a re-run that is certain: every read that has a wide phase at all has a pass-1 one first, with two candidates
    c.append(Case("rerun_certain", "rerun", 19, {"GAB_FMI_WIDE": "2", "GAB_FMI_WIDE_CAP": "1"},
                  lambda p, x: x["rerun_sure_reads"] == x["item_reads"] >= 32, 2))
    return c


CASES = _cases()
NEIGHBOUR_DEPTHS = (0, 1, 2, 7, 8, 9, 11)     # table_ext must grow from neighbour to neighbour above depth 1 (tests/test_fmi_paths_model.py)
