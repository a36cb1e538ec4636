"""The batches of tests/test_stream_order_gpu.py: for every `_device` entry point a small real batch, a DECOY for every device input
array (same shape and dtype), and what the reference or model makes of each.  tests/test_stream_order_cases.py checks them on the CPU.

Why a decoy.  The GPU test leaves the decoy in the input tensors and has the real inputs arrive through copies that are still
pending on the caller's stream when the entry point is called.  A library that reads an input before the stream has produced it
sees the decoy, so the decoy has to be an input the entry point may safely be handed, alone or mixed with the real arrays:
  - offsets are the real ones, and every length is the smallest the entry point accepts, so every range of the decoy -- and of any
    mixture of decoy and real arrays -- lies inside the real slabs;
  - sequence content differs from the real content but is valid for the entry point;
  - what the decoy computes differs from the real answer in at least 90 % of the items of every output (FLOOR), so that a test
    which got the decoy's numbers, or a mixture, cannot pass.
Nothing here comes from the library: expected values are pyoracle's (the CPU oracle) or the models of tests/.

An "item" of the 90 % floor is one element of a one-dimensional output, one row of a two-dimensional one (the six result fields of
a bsw pair are one item, a record of 40 bytes, a word of 16 parsed bases), and the whole record where the output is one struct
on the host (a gab_kmer_result).  Where an entry point returns a count with an array (SMEMs, coordinates), an item the decoy's
shorter array does not have counts as differing.

Two kinds of entry point have no lengths to shrink.  chain takes its call table on the host, so the decoy is other anchors under
the real table.  The parsers take one text: their decoy is the real file's records in reverse order with the bases substituted --
the same bytes and newlines in all, so that every array the parser sizes from its counts has the same size whatever it read
(those counts are kept apart in host["counts"]: they are the same by construction and under no floor).

A case is a Case: `inputs` / `decoy` map the device input arrays by name, `want` / `decoy_want` the outputs.  An output of `want`
is the whole tensor as the test allocates it; `valid[name]`, where present, is a bool mask of the items the entry point defines
(the others are room: operation room of wfa, the slack of a positions array) and `want` holds SENTINEL there when the room has to
keep the test's fill.  `stats` are the last_stats counters the module's own tests compare with the model."""
from dataclasses import dataclass, field

import numpy as np

from oracle import pyoracle
from tools import gabgen
from tests import util

FLOOR = 0.9
SENTINEL8 = 0x5A                    # the GPU test fills every BYTE of an output tensor with this (an int32 reads 0x5A5A5A5A)


@dataclass
class Case:
    inputs: dict
    decoy: dict
    want: dict
    decoy_want: dict
    valid: dict = field(default_factory=dict)
    stats: dict = field(default_factory=dict)
    decoy_stats: dict = field(default_factory=dict)
    host: dict = field(default_factory=dict)          # arguments that stay on the host (call tables, scalars)


def differing(case, name):
    """share of the valid items of output `name` in which the decoy's answer differs from the real one"""
    a, b = case.want[name], case.decoy_want[name]
    if isinstance(a, dict):
        return float(a != b)
    assert a.shape == b.shape and a.dtype == b.dtype, name
    ne = bits(a) != bits(b)
    if ne.ndim > 1:
        ne = ne.reshape(len(ne), -1).any(axis=1)
    v = case.valid.get(name)
    if v is not None:
        ne = ne[v]
    return float(ne.mean()) if ne.size else 0.0


def bits(a):
    """floats as the unsigned integers of their bit patterns (a NaN equals itself, -0.0 differs from 0.0); other arrays as they are"""
    return a.view("u%d" % a.dtype.itemsize) if a.dtype.kind == "f" else a


def check_inside(off, ln, slab_len, slack=0):
    """every range [off, off + len + slack) lies inside its slab"""
    off = np.asarray(off, np.int64); ln = np.asarray(ln, np.int64)
    assert (off >= 0).all() and (ln >= 0).all() and (off + ln + slack <= slab_len).all()


_SUBST = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"CGTAcgta"):
    _SUBST[_a] = _b


def other_letters(slab):
    """the same bytes with A -> C -> G -> T -> A (either case); every other byte (N, a newline, slack) stays"""
    return _SUBST[slab]


# ---------------------------------------------------------------------------------------------------------------- bsw
BSW_SLICE = (5037, 8000)            # GAB_BSW_SLICE of tests/test_bsw_slices_gpu.py
BSW_SLICED_PAIRS = 9001
BSW_BASE_PAIRS = 4096
BSW_REPEATS = 129                   # 4 096 x 129 = 528 384 pairs: more than the 64 x 8 192 of the one-launch form, below a sliced call's
_bsw = {}


def _bsw_base(n):
    """n generator pairs, their decoy, and per pair: the oracle's six fields and the model's score-only cells, for both"""
    if n in _bsw:
        return _bsw[n]
    p = util.bsw_oracle_params(*util.BSW_PARAM_SETS[0])
    b = gabgen.bsw(4301, n, 1)
    one = np.ones(n, np.int32)
    d = gabgen.BswBatch((b.ref + 1) % 5, b.ref_off, (b.qry + 2) % 5, b.qry_off, one, one.copy(), (3000 + np.arange(n) % 97).astype(np.int32))
    out = []
    for x in (b, d):
        check_inside(x.ref_off, x.len1, len(x.ref), 3); check_inside(x.qry_off, x.len2, len(x.qry), 3)
        assert (x.len1 >= 1).all() and (x.len2 >= 1).all() and (x.h0 >= 0).all() and x.ref.max() <= 4 and x.qry.max() <= 4
        want, ocells = pyoracle.bsw(x, p, want_cells=True)
        mscore, _, mcells, _ = gabgen.bsw_exit_model(x, p)
        np.testing.assert_array_equal(mscore, want[:, 0])
        out.append((x, want, mcells, ocells))
    _bsw[n] = out
    return out


def bsw_case(form, full):
    """form: "one_launch" (4 096 pairs), "multi_class" (those, repeated to 528 384 pairs: class launches over the caller's and the aux
    stream), "sliced" (9 001 pairs under GAB_BSW_SLICE: all three streams); full: with result_out"""
    n_base = BSW_SLICED_PAIRS if form == "sliced" else BSW_BASE_PAIRS
    rep = BSW_REPEATS if form == "multi_class" else 1
    sides = []
    for x, want, mcells, ocells in _bsw_base(n_base):
        t = lambda a: np.tile(a, rep)
        arrays = dict(ref=x.ref, ref_off=t(x.ref_off), qry=x.qry, qry_off=t(x.qry_off), len1=t(x.len1), len2=t(x.len2), h0=t(x.h0))
        outs = dict(score=np.tile(want[:, 0], rep))
        if full:
            outs["result"] = np.tile(want, (rep, 1))
        sides.append((arrays, outs, {"cells": rep * (ocells if full else int(mcells.sum()))}))
    (ri, ro, rs), (di, do, ds) = sides
    return Case(ri, di, ro, do, stats=rs, decoy_stats=ds, host={"slice": BSW_SLICE if form == "sliced" else None})


# ---------------------------------------------------------------------------------------------------------------- chain
_chain = {}
CHAIN_DECOY_TRACKS = 7


def chain_batches():
    """the mixed batch of tests/test_chain_forms_gpu.py and its decoy.  The call table stays on the host, so it is the real one.
    A quarter of the real anchors have no predecessor (score = q_span, parent -1) and an eighth chain to the anchor before, so the
    decoy does neither: other q_spans, and in every call seven collinear tracks 2^20 query bases apart (further than any
    max_dist_y), anchor i on track i mod 7 -- its parent is anchor i - 7"""
    if "b" not in _chain:
        b = gabgen.chain(31, 200, 0, 50, 20000)
        U = np.uint64
        assert b.hdr["max_dist_y"].max() < 1 << 20 and b.hdr["n"].max() * 10 < 1 << 20
        idx = (np.arange(b.nanchors, dtype=np.int64) - np.repeat(b.call_off, b.hdr["n"])).astype(U)
        span = (b.y >> U(32)) & U(0xff)
        span = np.where(span >= U(200), span - U(7), span + U(7))
        y = (b.y & ~U(0xffffffffff)) | (span << U(32)) | (U(1000) + U(10) * idx + U(1 << 20) * (idx % U(CHAIN_DECOY_TRACKS)))
        x = (b.x & ~U(0xffffffff)) | (U(5000) + U(10) * idx)
        _chain["b"] = (b, gabgen.ChainBatch(b.hdr, b.call_off, x, y))
    return _chain["b"]


def chain_case(mode):
    if mode not in _chain:
        sides = []
        for x in chain_batches():
            s, p, ev = pyoracle.chain(x, mode, want_evals=True)
            sides.append((dict(x=x.x.view(np.int64), y=x.y.view(np.int64)), dict(score=s, parent=p), {"evals": ev}))
        (ri, ro, rs), (di, do, ds) = sides
        b = chain_batches()[0]
        _chain[mode] = Case(ri, di, ro, do, stats=rs, decoy_stats=ds, host={"call_off": b.call_off, "hdr": b.hdr, "batch": b})
    return _chain[mode]


# ---------------------------------------------------------------------------------------------------------------- bpm / bitpal / wfa
def _pair_sides(batch, min_plen, min_tlen):
    """(real arrays, decoy arrays, decoy batch) of a PairBatch: real offsets, the smallest lengths, the letters substituted"""
    n = batch.n
    d = gabgen.PairBatch(other_letters(batch.pat), batch.pat_off, np.full(n, min_plen, np.int32),
                         other_letters(batch.txt), batch.txt_off, np.full(n, min_tlen, np.int32))
    for x in (batch, d):
        check_inside(x.pat_off, x.pat_len, len(x.pat), 3); check_inside(x.txt_off, x.txt_len, len(x.txt), 3)
    arrays = lambda x: dict(pat=x.pat, pat_off=x.pat_off, pat_len=x.pat_len, txt=x.txt, txt_off=x.txt_off, txt_len=x.txt_len)
    return arrays(batch), arrays(d), d


_pairs = {}


def bpm_case():
    """the hand-made pairs of tests/test_bpm_stages_gpu.py (every register class with unclean pairs: each class's band kernel, on the
    second stream, has work) among 600 generator pairs.  Decoy: pattern_length 1, text_length 0, the smallest the entry accepts"""
    if "bpm" not in _pairs:
        g = gabgen.pairs(9, 600, 1, 200).swapped_longer_first()
        hand = util.bpm_handmade_pairs()
        pats = [g.pair(i)[0] for i in range(g.n)]; txts = [g.pair(i)[1] for i in range(g.n)]
        for k, (p, t, _) in enumerate(hand):
            at = (k * 7) % len(pats)
            pats.insert(at, p); txts.insert(at, t)
        b = gabgen.pairs_from_lists(pats, txts)
        ri, di, d = _pair_sides(b, 1, 0)
        sides = []
        for x in (b, d):
            assert (x.pat_len >= 1).all() and (x.txt_len <= x.pat_len).all()
            scores, stages, steps = util.bpm_model_batch(x)
            np.testing.assert_array_equal(scores, pyoracle.bpm(x))
            census = util.bpm_census(x, stages)
            sides.append((dict(score=scores), {"block_steps": steps, "full_pairs": sum(c[1] for c in census.values()) + census.get(0, (0,))[0]}, census))
        assert all(sides[0][2].get(c, (0, 0))[1] > 0 for c in (1, 2, 3, 4)), sides[0][2]
        _pairs["bpm"] = Case(ri, di, sides[0][0], sides[1][0], stats=sides[0][1], decoy_stats=sides[1][1])
    return _pairs["bpm"]


def bitpal_case(algorithm):
    """2 000 generator pairs.  Decoy: both lengths 0"""
    key = ("bitpal", algorithm)
    if key not in _pairs:
        b = gabgen.pairs(9, 2000, 1, 200)
        ri, di, d = _pair_sides(b, 0, 0)
        cells = lambda x: {"cells": int((x.pat_len.astype(np.int64) * x.txt_len).sum()), "long_pairs": int((np.minimum(x.pat_len, x.txt_len) > 2048).sum())}
        _pairs[key] = Case(ri, di, dict(score=pyoracle.bitpal(b, algorithm)), dict(score=pyoracle.bitpal(d, algorithm)), stats=cells(b), decoy_stats=cells(d))
    return _pairs[key]


WFA_RATES = (0.02, 0.05, 0.08, 0.12, 0.2, 0.35, 0.6)        # (no identical pairs: the decoy scores 0)


def wfa_case():
    """400 pairs of the census recipe of tests/util.py, whose high error rates leave the first tier (asserted through the model:
    pairs beyond the first launch of the plan).  The operation room is the real pairs'.  Decoy: both lengths 0 -- score 0, no operations"""
    if "wfa" not in _pairs:
        pats, txts = util.wfa_census_pairs(400, 21, rates=WFA_RATES)
        b = gabgen.pairs_from_lists(pats, txts)
        ri, di, d = _pair_sides(b, 0, 0)
        plan = util.wfa_plan(b, (4, 6, 2))
        tier, _ = util.wfa_tier_of(b, (4, 6, 2), util.wfa_model(pats, txts, (4, 6, 2)), plan)
        assert (tier > 0).sum() >= 10, "no pair reaches a second tier"
        sides = []
        for x in (b, d):
            ops, off, ln, sc, cells = pyoracle.wfa(x, want_cells=True)
            sides.append((off, ops, ln, sc, cells))
        off, total = sides[0][0], int((b.pat_len.astype(np.int64) + b.txt_len).sum())
        outs, valid = [], None
        for _, ops, ln, sc, cells in sides:
            room = np.full(total + 16, SENTINEL8, np.uint8)
            v = np.zeros(total + 16, bool)
            v[total:] = True                  # behind the last pair's room nothing is written (within a pair's room anything may be)
            for i in np.flatnonzero(ln):      # (the decoy's operations, had it any, would lie at ITS offsets: it has none)
                room[off[i]:off[i] + ln[i]] = ops[off[i]:off[i] + ln[i]]
                v[off[i]:off[i] + ln[i]] = True
            valid = v if valid is None else valid
            outs.append((dict(ops=room, ops_len=ln, score=sc), {"work": cells}))
        assert sides[1][2].max() == 0
        ri["ops_off"] = off; di["ops_off"] = off.copy()
        _pairs["wfa"] = Case(ri, di, outs[0][0], outs[1][0], valid={"ops": valid}, stats=outs[0][1], decoy_stats=outs[1][1])
    return _pairs["wfa"]


# ---------------------------------------------------------------------------------------------------------------- kmer
KMER_K, KMER_WINDOW, KMER_MIN_LEN, KMER_NPARTS, KMER_PART = 15, 10, 100, 3, 1
KMER_RATE = 3.0                                    # (removes the k-mers of the read that is there five times)
KMER_SOLID = dict(min_freq=2, select_rate=0.4, tandem_freq=2, rate=1.5)
KMER_ROOM = 64                                     # entries of room behind the positions a call returns
_kmer = {}


def kmer_reads():
    """36 reads of 60 .. 2 500 bases (three no longer than min_len: filtered), one of them there five times and a few twice, a
    tandem repeat and a homopolymer: every rule of the three index builds has work"""
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads = [acgt[rng.integers(0, 4, int(n))].tobytes() for n in rng.integers(300, 2500, 24)]
    reads = [reads[3]] * 4 + [reads[5], reads[7].lower(), reads[9][:700]] + reads     # (repeats first: the solid selection of read 0 is not empty)
    reads += [b"ACGGT" * 120, b"A" * 400, b"ACGT" * 15, b"C" * 100, b"G" * 99]
    return reads


def _kmer_inputs():
    if "in" not in _kmer:
        from genarchbench_amd.kmer import pack_reads
        reads = kmer_reads()
        seq, off, ln = pack_reads(reads)
        zero = np.zeros_like(ln)
        check_inside(off, ln, len(seq)); check_inside(off, zero, len(seq))
        _kmer["in"] = (reads, [b""] * len(reads), dict(seq=seq, off=off, len=ln), dict(seq=other_letters(seq), off=off.copy(), len=zero))
    return _kmer["in"]


def _positions_outputs(start, pos, cap):
    room = np.frombuffer(bytes([SENTINEL8]) * 4 * cap, np.int32).copy()
    room[:pos.size] = pos
    return dict(read_start=start, pos=room)


def kmer_case(which):
    """which: count, count_part, sketch, index_minimizers, index_part, index_solid, solid_positions.  The decoy has every length 0:
    no read is kept, every count is 0, every index empty.  The host records are one item each (`res`, and `res2` of the finish);
    `index` is the model's dump of the index the call leaves in the handle, `table` that of the counts"""
    if which in _kmer:
        return _kmer[which]
    from tests import kmer_model, minimizer_model, solid_model
    from tests import kmer_parts_util as kp, minimizer_parts_util as mp
    reads, none, real, decoy = _kmer_inputs()
    k, w, ml = KMER_K, KMER_WINDOW, KMER_MIN_LEN
    sides = []
    for rs in (reads, none):
        stats, valid, host = {}, {}, {}
        if which in ("count", "count_part"):
            m = kmer_model.model(rs, k, ml)
            if which == "count_part":
                m = kp.restrict(m, kp.merged_keys(rs, k, ml), KMER_NPARTS)[KMER_PART]
            want = dict(res=kp.fields(m), table=dict(kmers=m["kmers"], counts=m["counts"]))
            stats = {"merged": m["merged"]}
        elif which in ("sketch", "solid_positions"):
            if which == "sketch":
                start, pos = minimizer_model.sketch_reads(rs, k, w, ml)
            else:
                s = KMER_SOLID
                start, pos = solid_model.positions(rs, k, s["min_freq"], s["select_rate"], s["tandem_freq"], ml)
            cap = sides[0][3]["cap"] if sides else pos.size + KMER_ROOM
            want = _positions_outputs(start, pos, cap)
            want["res"] = dict(nout=int(pos.size))
            host = {"cap": cap}                       # (the room behind the positions keeps the sentinel: the whole array is compared)
        elif which == "index_minimizers":
            m = minimizer_model.build_index(rs, k, w, KMER_RATE, ml)
            want = dict(res=mp.fields(m), index={f: m[f] for f in ("kmers", "start", "gpos")})
        elif which == "index_part":
            found = minimizer_model.entries(rs, k, w, ml)
            parts = mp.restrict(found, KMER_RATE, KMER_NPARTS)
            m = parts[KMER_PART]
            host = {"minimizers": sum(p["minimizers"] for p in parts), "distinct": sum(p["distinct"] for p in parts)}
            want = dict(res=mp.begin_fields(m), res2=mp.fields(m), index={f: m[f] for f in ("kmers", "start", "gpos")})
        else:
            s = KMER_SOLID
            m = solid_model.build_index(rs, k, s["min_freq"], s["select_rate"], s["tandem_freq"], s["rate"], ml)
            want = dict(res={f: m[f] for f in solid_model.FIELDS}, index={f: m[f] for f in ("kmers", "start", "gpos")})
        sides.append((want, stats, valid, host))
    (rw, rs_, rv, rh), (dw, ds, _, _) = sides
    for name in ("index", "table"):                   # (dicts of arrays: compared as a whole)
        for wd in (rw, dw):
            if name in wd:
                wd[name] = {f: v.tolist() for f, v in wd[name].items()}
    if "index" in rw:
        assert len(rw["index"]["kmers"]) > 100 and rw.get("res2", rw["res"])["filtered_kmers"] > 0, rw["res"]
    _kmer[which] = Case(real, decoy, rw, dw, valid=rv, stats=rs_, decoy_stats=ds, host=rh)
    return _kmer[which]


KMER_ENTRIES = ("count", "count_part", "sketch", "index_minimizers", "index_part", "index_solid", "solid_positions")


# ---------------------------------------------------------------------------------------------------------------- abea
ABEA_SLACK = 16                    # entries behind the last read's room in pairs, the event slabs and the map: they keep the sentinel
ABEA_CHUNK, ABEA_WARMUP = 1024, 64      # GAB_ABEA_EVENTS_CHUNK, GAB_ABEA_EVENTS_WARMUP (include/gab.h)
_abea = {}


def _filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8).reshape(-1)[:] = SENTINEL8
    return a


def _records(recs, dtype):
    """dicts with the fields of a record -> the records as bytes, one row each (floats are compared by bit pattern this way)"""
    out = np.zeros(len(recs), dtype)
    for i, r in enumerate(recs):
        for f in dtype.names:
            if f != "pad":
                out[i][f] = r[f]
    return out.view(np.uint8).reshape(len(recs), dtype.itemsize)


def _offsets(lens):
    off = np.zeros(len(lens), np.int64)
    off[1:] = np.cumsum(np.asarray(lens, np.int64)[:-1])
    return off


def abea_model_and_reads():
    """a random pore model and 12 reads of 40 .. 330 bases with their events (tests/abea_model.py), scaled by the model of
    gab_abea_scalings and aligned by the model of gab_abea_align; three of them long enough to be recalibrated"""
    if "reads" not in _abea:
        from tests import abea_model as A, abea_events_model as E
        rng = np.random.default_rng(20260101)
        mean, stdv, lstd = A.make_model(rng)
        reads = []
        for n in (330, 40, 75, 300, 120, 6, 33, 64, 280, 100, 57, 150):
            seq, ev, _, _ = A.make_read(rng, n, mean, stdv)
            reads.append((seq, ev) + E.scalings(seq, ev, mean))
        _abea["reads"] = ((mean, stdv, lstd), reads, [A.align(s, e, mean, stdv, lstd, sc, sh) for s, e, sc, sh in reads])
    return _abea["reads"]


def _abea_sides():
    """the packed arrays of the twelve reads and of their decoy: the real offsets, seq_len 6 and n_events 1 (the smallest the entry
    points accept), the bases substituted, other finite events, scalings and pairs that are valid for any mixture (all zero)"""
    if "sides" not in _abea:
        from genarchbench_amd import abea
        (mean, stdv, lstd), reads, aligned = abea_model_and_reads()
        seq, seq_off, seq_len, ev, ev_off, n_ev, scale, shift, pair_off = abea.pack_reads(reads)
        n = len(reads)
        room = int(abea.pair_room(seq_len, n_ev).sum())
        pairs = np.zeros((room + ABEA_SLACK, 2), np.int32)
        n_pairs = np.array([rec["n_pairs"] for rec, _ in aligned], np.int32)
        for o, k, (_, path) in zip(pair_off, n_pairs, aligned):
            pairs[o:o + k] = path[:k]
        real = dict(seq=seq, seq_off=seq_off, seq_len=seq_len, events=ev, event_off=ev_off, n_events=n_ev, scale=scale, shift=shift,
                    pairs=pairs, pair_off=pair_off, n_pairs=n_pairs, map_off=_offsets(seq_len - 5))
        decoy = dict(seq=other_letters(seq), seq_off=seq_off.copy(), seq_len=np.full(n, 6, np.int32), events=(ev + np.float32(17.5)).astype(np.float32),
                     event_off=ev_off.copy(), n_events=np.ones(n, np.int32), scale=(scale * np.float32(1.25)).astype(np.float32),
                     shift=(shift + np.float32(3.0)).astype(np.float32), pairs=np.zeros_like(pairs), pair_off=pair_off.copy(),
                     n_pairs=np.zeros(n, np.int32), map_off=real["map_off"].copy())
        for x in (real, decoy):
            check_inside(x["seq_off"], x["seq_len"], len(seq)); check_inside(x["event_off"], x["n_events"], len(ev))
            assert (x["seq_len"] >= 6).all() and (x["n_events"] >= 1).all() and np.isfinite(x["events"]).all()
        _abea["sides"] = (real, decoy)
    return _abea["sides"]


def _abea_reads_of(x):
    return [(bytes(x["seq"][o:o + k]), x["events"][e:e + m], x["scale"][i], x["shift"][i])
            for i, (o, k, e, m) in enumerate(zip(x["seq_off"], x["seq_len"], x["event_off"], x["n_events"]))]


def abea_case(which):
    """which: align, scalings, calibrate, events"""
    if which in _abea:
        return _abea[which]
    from genarchbench_amd import abea
    from tests import abea_model as A, abea_events_model as E, abea_calib_model as Cm
    (mean, stdv, lstd), _, _ = abea_model_and_reads()
    if which == "events":
        rng = np.random.default_rng(5)
        signals = [E.make_signal(rng, int(n), mean)[:4] for n in rng.integers(1100, 2600, 16)]
        raw, raw_off, n_samples, rg, dig, offs = abea.pack_signals([(s[0].astype(np.float32),) + s[1:] for s in signals])
        real = dict(raw=raw, raw_off=raw_off, n_samples=n_samples, range=rg, digitisation=dig, offset=offs)
        decoy = dict(raw=(raw + np.float32(3)).astype(np.float32), raw_off=raw_off.copy(), n_samples=np.ones_like(n_samples),
                     range=(rg * np.float32(1.5)).astype(np.float32), digitisation=np.full_like(dig, 4096.0), offset=(offs + np.float32(2)).astype(np.float32))
        sides, cap = [], None
        for x in (real, decoy):
            check_inside(x["raw_off"], x["n_samples"], len(raw))
            assert (x["n_samples"] >= 1).all() and (x["digitisation"] != 0).all() and all(np.isfinite(x[f]).all() for f in ("raw", "range", "offset"))
            evs = [E.events_of(x["raw"][o:o + k], x["range"][i], x["digitisation"][i], x["offset"][i]) for i, (o, k) in enumerate(zip(x["raw_off"], x["n_samples"]))]
            n_ev = np.array([e["mean"].size for e in evs], np.int32)
            total = int(n_ev.sum())
            cap = total + ABEA_SLACK if cap is None else cap
            want = dict(n_events=n_ev, event_off=_offsets(n_ev), total=np.array([total], np.int64))
            for f, dt in (("mean", np.float32), ("stdv", np.float32), ("start", np.int32), ("length", np.float32)):
                want[f] = _filled(cap, dt)
                want[f][:total] = np.concatenate([e[f] for e in evs])
            pas = [E.to_pa(x["raw"][o:o + k], x["range"][i], x["digitisation"][i], x["offset"][i]) for i, (o, k) in enumerate(zip(x["raw_off"], x["n_samples"]))]
            stats = dict(samples=int(x["n_samples"].sum()), events=total, reads_serial_sums=sum(not E.sums_are_wide(p) for p in pas),
                         chunks=int(sum(-(-int(k) // ABEA_CHUNK) for k in x["n_samples"])),
                         chunks_redone=sum(E.chunks_to_redo(*e["tstat"], ABEA_CHUNK, ABEA_WARMUP) for e in evs))
            sides.append((want, stats))
        _abea[which] = Case(real, decoy, sides[0][0], sides[1][0], stats=sides[0][1], decoy_stats=sides[1][1])
        return _abea[which]
    real, decoy = _abea_sides()
    names = {"align": ("seq", "seq_off", "seq_len", "events", "event_off", "n_events", "scale", "shift", "pair_off"),
             "scalings": ("seq", "seq_off", "seq_len", "events", "event_off", "n_events"),
             "calibrate": ("seq", "seq_off", "seq_len", "events", "event_off", "n_events", "scale", "shift", "pairs", "pair_off", "n_pairs", "map_off")}[which]
    sides = []
    for x in (real, decoy):
        reads = _abea_reads_of(x)
        n = len(reads)
        if which == "align":
            got = [A.align(s, e, mean, stdv, lstd, sc, sh) for s, e, sc, sh in reads]
            pairs = _filled(real["pairs"].shape, np.int32)
            valid = np.zeros(len(pairs), bool)
            valid[len(pairs) - ABEA_SLACK:] = True
            for o, (rec, path) in zip(x["pair_off"], got):
                pairs[o:o + rec["path_len"]] = path
                valid[o:o + rec["path_len"]] = True
            want = dict(pairs=pairs, res=_records([dict(rec) for rec, _ in got], abea.READ))
            stats = dict(cells=sum(rec["fills"] for rec, _ in got), bands=sum(len(r[0]) - 5 + len(r[1]) + 2 for r in reads), launches=1)
            sides.append((want, stats, {"pairs": valid}))
        elif which == "scalings":
            got = [E.scalings(s, e, mean) for s, e, _, _ in reads]
            want = dict(scale=np.array([g[0] for g in got], np.float32), shift=np.array([g[1] for g in got], np.float32))
            routes = np.array([E.scalings_in_order(s, e, mean) for s, e, _, _ in reads], np.int64).reshape(-1, 3).sum(0).tolist()
            sides.append((want, dict(reads=n, event_sums_in_order=routes[0], kmer_sums_in_order=routes[1], kmer_sq_sums_in_order=routes[2]), {}))
        else:
            got = [Cm.calibrate(s, e, mean, stdv, sc, sh, x["pairs"][o:o + k]) for (s, e, sc, sh), o, k in zip(reads, x["pair_off"], x["n_pairs"])]
            rmap = _filled((int((real["seq_len"] - 5).sum()) + ABEA_SLACK, 2), np.int32)
            for o, (_, m) in zip(x["map_off"], got):
                rmap[o:o + len(m)] = m
            want = dict(map=rmap, res=_records([rec for rec, _ in got], abea.CALIB))
            stats = dict(reads=n, recalibrated=sum(int(rec["recalibrated"]) for rec, _ in got), m_states=sum(int(rec["n_m_state"]) for rec, _ in got))
            sides.append((want, stats, {}))
    if which == "calibrate":
        assert sides[0][1]["recalibrated"] >= 2, sides[0][1]
    _abea[which] = Case({k: real[k] for k in names}, {k: decoy[k] for k in names}, sides[0][0], sides[1][0], valid=sides[0][2],
                        stats=sides[0][1], decoy_stats=sides[1][1], host={"model": (mean, stdv, lstd)})
    return _abea[which]


ABEA_ENTRIES = ("align", "events", "scalings", "calibrate")


# ---------------------------------------------------------------------------------------------------------------- fmi
FMI_MIN_SEED_LEN, FMI_MAX_OCC = 19, 50
_fmi = {}


def _as_shape(a, like, fill):
    """`a` cut or padded with `fill` to the length of `like`: the decoy's output where an entry point returns a count with its
    array -- an item the decoy does not have differs from the real one"""
    out = np.full(like.shape, fill, like.dtype)
    k = min(len(a), len(like))
    out[:k] = a[:k]
    return out


def fmi_index():
    """(mkindex.FmIndex of a 60 000-base reference, the oracle's view of the same arrays, 400 reads of 80 .. 151 bases)"""
    if "ix" not in _fmi:
        import ctypes as C
        from tools import mkindex
        ref = gabgen.fmi_ref(11, 60000, 5)
        idx = mkindex.FmIndex(ref)
        oidx = pyoracle.FmIndex()
        cnt = (C.c_int64 * 5)(*[int(x) for x in idx.count])
        pyoracle.lib().oracle_fmi_from_arrays(C.byref(oidx), C.c_int64(idx.ref_seq_len), cnt, idx.cp_occ.ctypes.data_as(C.c_void_p), C.c_int64(idx.sentinel_index))
        pyoracle.lib().oracle_fmi_set_sa(C.byref(oidx), idx.sa_ms_byte.ctypes.data_as(C.c_void_p), idx.sa_ls_word.ctypes.data_as(C.c_void_p))
        _fmi["ix"] = (idx, oidx, gabgen.fmi_reads(12, ref, 400, 80, 151))
    return _fmi["ix"]


def fmi_case(which):
    """seed: the decoy has every length 0 (no SMEM) and other bases; sa_lookup: the oracle's SMEMs of the reads, the decoy k = 0,
    s = 1 for every one of them (one coordinate each, that of row 0)"""
    if which in _fmi:
        return _fmi[which]
    idx, oidx, reads = fmi_index()
    enc = np.ascontiguousarray(reads.enc)
    w, woff, calls = pyoracle.fmi(oidx, reads, FMI_MIN_SEED_LEN, want_calls=True)
    w["pad"] = 0                                      # (not part of the result: the test clears it in what the library returns too)
    rows = lambda sm: np.ascontiguousarray(sm).view(np.uint8).reshape(len(sm), 40)
    if which == "seed":
        d = gabgen.ReadBatch(np.ascontiguousarray((enc + 1) % 4), np.zeros_like(reads.len))
        assert enc.max() <= 4 and (reads.len <= enc.shape[1]).all()
        dw, dwoff, dcalls = pyoracle.fmi(oidx, d, FMI_MIN_SEED_LEN, want_calls=True)
        assert len(w) > 1000 and len(dw) == 0
        c = Case(dict(enc=enc, len=reads.len), dict(enc=d.enc, len=d.len), dict(smems=rows(w), read_off=woff, res=dict(nout=len(w))),
                 dict(smems=_as_shape(rows(dw), rows(w), 0xFF), read_off=dwoff, res=dict(nout=0)),
                 stats={"ext_calls": calls, "smems": len(w)}, decoy_stats={"ext_calls": dcalls, "smems": 0})
    else:
        w = np.roll(w, -int(np.flatnonzero(w["s"] > 1)[0]))      # (a repeat first: from there on the offsets are not the decoy's 0, 1, 2 ...)
        dsm = w.copy()
        dsm["k"] = 0; dsm["l"] = 0; dsm["s"] = 1
        sides = []
        for sm in (w, dsm):
            assert (sm["k"] >= 0).all() and (sm["s"] >= 1).all() and (sm["k"] + sm["s"] <= idx.ref_seq_len + 1).all()
            co, coff, steps = pyoracle.fmi_sa_lookup(oidx, sm, FMI_MAX_OCC)
            sides.append((co, coff, steps))
        (co, coff, steps), (dco, dcoff, dsteps) = sides
        c = Case(dict(smems=rows(w)), dict(smems=rows(dsm)), dict(coords=co, coord_off=coff, res=dict(total=len(co))),
                 dict(coords=_as_shape(dco, co, -1), coord_off=dcoff, res=dict(total=len(dco))), stats={"lf_steps": steps}, decoy_stats={"lf_steps": dsteps})
    c.host = {"index": idx}
    _fmi[which] = c
    return c


# ---------------------------------------------------------------------------------------------------------------- parse
PARSE_SLACK = 16
_parse = {}
_DIGITS = np.arange(256, dtype=np.uint8)
for _c in range(5):
    _DIGITS[48 + _c] = 48 + (_c + 1) % 5


def _text_bytes(batch):
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "in.txt")
        batch.write_text(path)
        with open(path, "rb") as f:
            return f.read()


def parse_texts(which):
    """(real text, decoy text) of parser `which` (bsw, pairs, chain).  The parsers' outputs are, but for the code bytes, a function
    of where the newlines are, so a decoy with the real lines would give the real lengths and offsets.  The decoy is the real
    file's RECORDS IN REVERSE ORDER with the bases substituted (and every digit of a bsw seed score one higher): as many bytes, as many newlines, every line well formed, and
    record i is another record's"""
    lines = lambda t: t.split(b"\n")[:-1]
    if which == "bsw":
        text = _text_bytes(gabgen.bsw(61, 700, 1))
        ls = lines(text)
        rec = [ls[i:i + 3] for i in range(0, len(ls), 3)][::-1]
        decoy = b"".join(bytes(48 + (c - 47) % 10 for c in h) + b"\n" + _DIGITS[np.frombuffer(r, np.uint8)].tobytes() + b"\n" + _DIGITS[np.frombuffer(q, np.uint8)].tobytes() + b"\n" for h, r, q in rec)
    elif which == "pairs":
        text = _text_bytes(gabgen.pairs(62, 600, 1, 180))
        ls = lines(text)
        rec = [ls[i:i + 2] for i in range(0, len(ls), 2)][::-1]
        decoy = b"".join(other_letters(np.frombuffer(p, np.uint8)).tobytes() + b"\n" + other_letters(np.frombuffer(t, np.uint8)).tobytes() + b"\n" for p, t in rec)
    else:
        text = _text_bytes(gabgen.chain(63, 24, 0, 20, 700))
        calls = [c + b"EOR\n" for c in text.split(b"EOR\n")[:-1]]
        decoy = b"".join(calls[::-1])
    assert len(decoy) == len(text) and decoy.count(b"\n") == text.count(b"\n") and decoy != text
    return text, decoy


def words16(codes):
    """the bases of all sequences back to back, in rows of 16 (the last one padded with 255).  Two random bases agree one time in
    four, so single bases cannot differ in 90 % of the places: the item of a code slab is a word of 16 bases"""
    codes = np.asarray(codes, np.uint8)
    out = np.full((len(codes) + 15) // 16 * 16, 255, np.uint8)
    out[:len(codes)] = codes
    return out.reshape(-1, 16)


def parse_case(which):
    """`text` is the file and PARSE_SLACK zero bytes; the expected arrays are those of tests/parse_cases.py"""
    if which in _parse:
        return _parse[which]
    from tests import parse_cases as pc
    sides = []
    for text in parse_texts(which):
        buf = np.zeros(len(text) + PARSE_SLACK, np.uint8)
        buf[:len(text)] = np.frombuffer(text, np.uint8)
        if which == "bsw":
            e = pc.expect_bsw(text)
            want = {f: np.ascontiguousarray(e[f]) for f in ("len1", "len2", "h0", "ref_off", "qry_off")}
            want["ref"] = words16(e["ref"]); want["qry"] = words16(e["qry"])
            counts = dict(n=int(e["n"]))
        elif which == "pairs":
            e = pc.expect_pairs(text, True)
            want = {f: np.ascontiguousarray(e[f]) for f in ("pat_off", "txt_off", "pat_len", "txt_len", "cap_off")}
            counts = dict(n=int(e["n"]), cap_bytes=int(e["cap_bytes"]))
        else:
            b = pc.expect_chain(text)
            want = dict(x=b.x.view(np.int64), y=b.y.view(np.int64), res=dict(call_off=b.call_off.tolist() + [b.nanchors], hdr=b.hdr.tolist()))
            counts = dict(ncalls=b.ncalls, total=b.nanchors)
        sides.append((dict(text=buf), want, counts))
    (ri, rw, counts), (di, dw, dcounts) = sides
    assert counts == dcounts        # (as many records in the decoy: the sizes of the parser's arrays are the same whatever it read)
    for k in rw:
        if not isinstance(rw[k], dict):
            assert rw[k].dtype == dw[k].dtype and len(rw[k]) == len(dw[k]), k
    _parse[which] = Case(ri, di, rw, dw, host={"nbytes": len(ri["text"]) - PARSE_SLACK, "counts": counts})
    return _parse[which]


PARSERS = ("bsw", "pairs", "chain")


# ---------------------------------------------------------------------------------------------------------------- the list
CASES = {}
for _form in ("one_launch", "multi_class", "sliced"):
    for _full in (False, True):
        CASES["bsw-%s-%s" % (_form, "result" if _full else "score")] = (lambda f=_form, r=_full: bsw_case(f, r))
for _mode in (0, 1):
    CASES["chain-mode%d" % _mode] = (lambda m=_mode: chain_case(m))
CASES["bpm"] = bpm_case
for _alg in (0, 1):
    CASES["bitpal-%d" % _alg] = (lambda a=_alg: bitpal_case(a))
CASES["wfa"] = wfa_case
for _which in KMER_ENTRIES:
    CASES["kmer-" + _which] = (lambda w=_which: kmer_case(w))
for _which in ABEA_ENTRIES:
    CASES["abea-" + _which] = (lambda w=_which: abea_case(w))
for _which in ("seed", "sa_lookup"):
    CASES["fmi-" + _which] = (lambda w=_which: fmi_case(w))
for _which in PARSERS:
    CASES["parse-" + _which] = (lambda w=_which: parse_case(w))


def case(name):
    return CASES[name]()
