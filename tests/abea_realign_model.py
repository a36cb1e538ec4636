"""A numpy restatement of realign_read (abea/src/eventalign.c:1942-2034): align_read_to_ref (eventalign.c:1263-1540) around
profile_hmm_align (eventalign.c:703-911) with hmm_flags = 0, in the arithmetic of the reference built without fused multiply-add:
float32 rounded after every operation, update_cell's comparisons as written (eventalign.c:621-633), logf from the C library (numpy's
float32 log is not glibc's).  It is the contract of gab_abea_realign (include/gab.h), the two defined deviations included, and it
holds the seeded generators of the fixture's references and CIGARs and of the constructed cases."""
import ctypes
import ctypes.util
import hashlib
import math

import numpy as np

import abea_model as A

K = A.K
F = np.float32
ROWS = 512            # GAB_ABEA_REALIGN_ROWS
SKIPPED, NO_PAIRS, NO_EVENT, STRAND = 1, 2, 4, 8      # gab_abea_realign_read.flags
ALIGN_STRIDE, OUTPUT_STRIDE = 100, 50                 # eventalign.c:1341-1342
OPS = "MIDNSHP=X"                                     # BAM operation codes
NI = F(-np.inf)
FROM_SAME_M, FROM_PREV_M, FROM_SAME_B, FROM_PREV_B, FROM_PREV_K, FROM_SOFT = range(6)
ST_K, ST_B, ST_M = 0, 1, 2

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x):
    return F(_libm.logf(float(x)))


def folded_log(p):
    """the logarithm of a compile-time constant, which the reference's compiler folds, correctly rounded"""
    return F(math.log(float(p)))


def transitions(events_per_base):
    """calculate_transitions (eventalign.c:171-240) -> dict of float32; `soft` is lp_sm + pre_flank[0] (eventalign.c:124, 523)"""
    with np.errstate(all="ignore"):
        p_stay = F(np.float64(1) - (np.float64(1) / np.float64(events_per_base)))
        p_skip, p_bad, p_skip_self = F(0.0025), F(0.001), F(0.3)
        p_mm_next = F(F(F(F(1.0) - p_stay) - p_skip) - p_bad)
        p_bk = F(F(F(1.0) - p_bad) / F(3))
        p_km = F(F(1.0) - p_skip_self)
        return dict(mm_self=logf(p_stay), mm_next=logf(p_mm_next), mb=folded_log(p_bad), mk=folded_log(p_skip),
                    bb=folded_log(p_bad), bk=folded_log(p_bk), bm_next=folded_log(p_bk), bm_self=folded_log(p_bk),
                    kk=folded_log(p_skip_self), km=folded_log(p_km), soft=F(F(0.0) + F(math.log(0.5))))


FIRST_SYMBOL = {**{c: "A" for c in "AMRWVHDN"}, **{c: "C" for c in "CSYB"}, **{c: "G" for c in "GK"}, "T": "T"}


def prepare_ref(ref):
    """upper case, every IUPAC code replaced by its first base (eventalign.c:1294-1300) -> bytes, or None if a byte is not valid"""
    try:
        return "".join(FIRST_SYMBOL[c] for c in bytes(ref).decode("latin-1").upper()).encode()
    except KeyError:
        return None


def revcomp(s):
    return bytes(s).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def encode_cigar(ops):
    """[(op character, length)] -> BAM encoding"""
    return np.array([(n << 4) | OPS.index(c) for c, n in ops], np.uint32)


def aligned_segments(cigar, ref_pos):
    """get_aligned_segments_two_params (eventalign.c:1112-1179), read stride 1 -> list of (n, 2) arrays of (ref_pos, read_pos)"""
    out, cur, ref_at, read_at = [], [], int(ref_pos), 0
    for w in np.asarray(cigar, np.uint32).tolist():
        n, op = w >> 4, OPS[w & 15]
        if op in "M=X":
            cur.append(np.stack([np.arange(ref_at, ref_at + n), np.arange(read_at, read_at + n)], 1))
            ref_at += n; read_at += n
        elif op == "D":
            ref_at += n
        elif op == "N":
            out.append(cur); cur = []
            ref_at += n
        elif op in "IS":
            read_at += n
        else:
            assert op == "H", op
    out.append(cur)
    return [np.concatenate(c).astype(np.int64) if c else np.zeros((0, 2), np.int64) for c in out]


def closest_event(k_idx, start_of, size):
    """get_closest_event_to (eventalign.c:962-987) over map[:, 0]"""
    def walk(start, stop, stride):
        while start != stop:
            if start_of[start] != -1:
                return int(start_of[start])
            start += stride
        return -1
    before = walk(k_idx, max(0, k_idx - 1000), -1)
    return before if before != -1 else walk(k_idx, min(k_idx + 1000, size - 1), 1)


def get_end_pair(ref_of, ref_max, pair_idx):
    while pair_idx < len(ref_of):
        if ref_of[pair_idx] > ref_max:
            return pair_idx - 1
        pair_idx += 1
    return len(ref_of) - 1


def update_cell(s):
    """update_cell (eventalign.c:621-633) on a (6, n) float32 array -> (max, from)"""
    mx = s[0].copy(); frm = np.zeros(s.shape[1], np.uint8)
    for i in range(1, 6):
        mx = np.where(s[i] > mx, s[i], mx)
        frm = np.where(mx == s[i], np.uint8(i), frm)
    return mx, frm


def skip_serial(a, kk):
    """K[b] = max(a[b], fl(kk + K[b-1])) as the reference's loop over the blocks computes it (max: replace on `>`, from -inf)"""
    out = np.empty_like(a); prev = NI
    for b in range(a.size):
        v = NI
        v = a[b] if a[b] > v else v
        c = F(kk + prev)
        v = c if c > v else v
        out[b] = prev = v
    return out


def skip_fixed_point(a, kk):
    """the same by iterating K <- max(K, fl(kk + shift(K))) from K = max(-inf, a) until nothing changes"""
    k = np.where(a > NI, a, NI).astype(F)
    while True:
        c = (kk + np.concatenate([[NI], k[:-1]])).astype(F)
        n = np.where(c > k, c, k)
        if n.tobytes() == k.tobytes():
            return k
        k = n


def skip_doubling(a, kk):
    """the same by a doubling scan: after the step at distance d, K[b] = max over j < 2d of a[b-j] with kk added j times, the
    addition applied d times, one rounding each, to the value that comes from distance d"""
    k = np.where(a > NI, a, NI).astype(F)
    d = 1
    while d < k.size:
        c = np.concatenate([np.full(d, NI, F), k[:-d]])
        for _ in range(d):
            c = (kk + c).astype(F)
        k = np.where(c > k, c, k)
        d *= 2
    return k


def hmm_align(kmer_ranks, events, e_start, e_stop, stride, level, scal, t, stats=None):
    """profile_hmm_align -> list of (event_idx, kmer_idx, state character) in order; level: (mean, stdv, log stdv); scal: (scale,
    shift, var, log_var)"""
    n_kmers = len(kmer_ranks)
    n_rows = abs(e_stop - e_start) + 1
    with np.errstate(all="ignore"):
        gp_mean = (F(scal[0]) * level[0][kmer_ranks] + F(scal[1])).astype(F)
        gp_stdv = (level[1][kmer_ranks] * F(scal[2])).astype(F)
        c = (F(-0.918938) - (level[2][kmer_ranks] + F(scal[3])).astype(F)).astype(F)
        M = np.full(n_kmers, NI, F); B = M.copy(); Kk = M.copy()
        ninf = np.full(n_kmers, NI, F)
        bt = np.zeros((n_rows + 1, 3, n_kmers), np.uint8)
        for row in range(1, n_rows + 1):
            x = F(events[e_start + (row - 1) * stride])
            pM = np.concatenate([[NI], M[:-1]]); pB = np.concatenate([[NI], B[:-1]]); pK = np.concatenate([[NI], Kk[:-1]])
            soft = ninf.copy()
            if row == 1:
                soft[0] = t["soft"]
            a = ((x - gp_mean) / gp_stdv).astype(F)
            em = (c + ((F(-0.5) * a).astype(F) * a).astype(F)).astype(F)
            mx, bt[row, ST_M] = update_cell(np.stack([t["mm_self"] + M, t["mm_next"] + pM, t["bm_self"] + B, t["bm_next"] + pB, t["km"] + pK, soft]).astype(F))
            nM = (mx + em).astype(F)
            mx, bt[row, ST_B] = update_cell(np.stack([t["mb"] + M, ninf, t["bb"] + B, ninf, ninf, ninf]).astype(F))
            nB = (mx + F(0.0)).astype(F)
            s1 = (t["mk"] + np.concatenate([[NI], nM[:-1]])).astype(F); s3 = (t["bk"] + np.concatenate([[NI], nB[:-1]])).astype(F)
            a01 = np.where(s3 > np.where(s1 > NI, s1, NI), s3, np.where(s1 > NI, s1, NI))
            nK = skip_fixed_point(a01, t["kk"])
            s4 = (t["kk"] + np.concatenate([[NI], nK[:-1]])).astype(F)
            mx, bt[row, ST_K] = update_cell(np.stack([ninf, s1, ninf, s3, s4, ninf]))
            nK = (mx + F(0.0)).astype(F)
            M, B, Kk = nM, nB, nK
    out = []
    row, kmer, st = n_rows, n_kmers - 1, ST_M
    while row > 0:
        out.append((e_start + (row - 1) * stride, kmer, "KBM"[st]))
        mv = int(bt[row, st, kmer])
        if stats is not None:
            stats["moves"][mv] += 1
        if mv == FROM_SOFT:
            break
        cur = st
        st = ST_K if mv == FROM_PREV_K else ST_B if mv in (FROM_SAME_B, FROM_PREV_B) else ST_M
        if mv in (FROM_PREV_M, FROM_PREV_B, FROM_PREV_K):
            kmer -= 1
        assert kmer >= 0
        if cur != ST_K:
            row -= 1
    out.reverse()
    if stats is not None:
        run = 0
        for e in out:
            run = run + 1 if e[2] == "K" else 0
            stats["k_run"] = max(stats["k_run"], run)
        stats["b"] += sum(e[2] == "B" for e in out)
    return out


def new_stats():
    return dict(moves=[0] * 6, k_run=0, b=0, breaks=dict(short_ref=0, stop_event=0, no_output=0))


def realign(ref, ref_pos, is_rev, cigar, seq_len, events, rmap, calib, level, region=(-1, -1), stats=None):
    """one read -> (entries as an (n, 3) int64 array of (ref_position, event_idx, state byte), record dict); calib: a dict or record
    with scale, shift, var, log_var, events_per_base, read_stat_flag; rmap: (n_kmers, 2)"""
    rec = dict(n_entries=0, hmm_segments=0, max_rows=0, flags=0, cells=0)
    out = []

    def done():
        rec["n_entries"] = len(out)
        return np.array(out, np.int64).reshape(-1, 3), rec
    if int(calib["read_stat_flag"]) != 0:
        rec["flags"] = SKIPPED
        return done()
    seq = prepare_ref(ref)
    assert seq is not None
    events = np.asarray(events, F)
    start_of = np.asarray(rmap)[:, 0]
    n_map = seq_len - K + 1
    assert len(start_of) == n_map
    fwd_ranks = A.kmer_ranks(seq) if len(seq) >= K else np.zeros(0, np.int64)
    rc_ranks = A.kmer_ranks(revcomp(seq))[::-1] if len(seq) >= K else fwd_ranks      # of the reverse complement of the 6-mer at each position
    t = transitions(calib["events_per_base"])
    scal = (calib["scale"], calib["shift"], calib["var"], calib["log_var"])
    for pairs in aligned_segments(cigar, ref_pos):
        if region[0] != -1 and region[1] != -1:
            pairs = pairs[(pairs[:, 0] >= region[0]) & (pairs[:, 0] <= region[1])]
        keep = len(pairs)
        while keep > 0 and pairs[keep - 1, 1] > seq_len - K:
            keep -= 1
        pairs = pairs[:keep]
        if len(pairs) == 0:
            rec["flags"] |= NO_PAIRS
            return done()
        flip = (lambda k: seq_len - k - K) if is_rev else (lambda k: k)
        first = closest_event(flip(int(pairs[0, 1])), start_of, n_map); last = closest_event(flip(int(pairs[-1, 1])), start_of, n_map)
        if first < 0 or last < 0:
            rec["flags"] |= NO_EVENT
            return done()
        forward = first < last
        cur_ev, cur_ref, cur_pair = first, int(pairs[0, 0]), 0
        ref_of = pairs[:, 0].tolist()
        while (forward and cur_ev < last) or (not forward and cur_ev > last):
            end_pair = get_end_pair(ref_of, cur_ref + ALIGN_STRIDE, cur_pair)
            end_ref, end_read = int(pairs[end_pair, 0]), flip(int(pairs[end_pair, 1]))
            s, ln = cur_ref - ref_pos, end_ref - cur_ref + 1
            if ln < 2 * K:
                if stats is not None:
                    stats["breaks"]["short_ref"] += 1
                break
            stop_ev = closest_event(end_read, start_of, n_map)
            if stop_ev < 0:
                rec["flags"] |= NO_EVENT
                return done()
            if abs(cur_ev - stop_ev) < 2:
                if stats is not None:
                    stats["breaks"]["stop_event"] += 1
                break
            stride = 1 if cur_ev < stop_ev else -1
            if bool(is_rev) != (stride == -1):
                rec["flags"] |= STRAND
                return done()
            n_kmers = ln - K + 1
            ranks = (rc_ranks if is_rev else fwd_ranks)[s:s + n_kmers]
            al = hmm_align(ranks, events, cur_ev, stop_ev, stride, level, scal, t, stats)
            n_rows = abs(stop_ev - cur_ev) + 1
            rec["hmm_segments"] += 1; rec["max_rows"] = max(rec["max_rows"], n_rows); rec["cells"] += n_rows * n_kmers
            last_section = end_pair == len(pairs) - 1
            num_output, last_ev_out, last_ref_out = 0, 0, 0
            for ev_idx, kmer, state in al:
                if not (num_output < OUTPUT_STRIDE or last_section):
                    break
                if state != "K" and ev_idx != cur_ev:
                    out.append((cur_ref + kmer, ev_idx, ord(state)))
                    last_ev_out, last_ref_out = ev_idx, cur_ref + kmer
                    num_output += 1
            cur_ev, cur_ref = last_ev_out, last_ref_out
            cur_pair = get_end_pair(ref_of, cur_ref, cur_pair)
            if num_output == 0:
                if stats is not None:
                    stats["breaks"]["no_output"] += 1
                break
    return done()


def eventalign_rows(ref, ref_pos, is_rev, entries):
    """the columns of events.tsv that the suite's check reads, per entry: (position, reference_kmer, event_index, model_kmer, state)"""
    seq = prepare_ref(ref)
    rows = []
    for pos, ev, st in np.asarray(entries).reshape(-1, 3).tolist():
        kmer = seq[pos - ref_pos:pos - ref_pos + K]
        rows.append((pos, kmer.decode(), ev, "N" * K if st == ord("B") else (revcomp(kmer) if is_rev else kmer).decode(), chr(st)))
    return rows


def entries_digest(entries):
    """hash of a read's entries as the fixture records it: sha256 of little-endian int32 (ref_position, event_idx, state), 16 hex digits"""
    return hashlib.sha256(np.ascontiguousarray(np.asarray(entries).reshape(-1, 3), "<i4").tobytes()).hexdigest()[:16]


def record_of(entries, rec):
    """a read as tests/golden/abea_realign_expected.json holds it"""
    return {"n_entries": int(rec["n_entries"]), "hmm_segments": int(rec["hmm_segments"]), "max_rows": int(rec["max_rows"]), "flags": int(rec["flags"]),
            "entries": entries_digest(entries)}


def room_of(n_events, cigar):
    """entries of room a read needs: n_events * (1 + its N operations)"""
    return int(n_events) * (1 + int(((np.asarray(cigar, np.uint32) & 15) == 3).sum()))


# ---- the generators ----------------------------------------------------------------------------------------------------------------------
FIXTURE_SEED = 20251020
CASE_SEED = 20251021


def mutate(rng, read, rate=0.03, n_skip=0, clip=None, eqx=False, big_del=0):
    """a reference and a CIGAR for `read` (the bases as the BAM record holds them): substitutions, insertions and deletions at
    `rate` each; n_skip N operations of 20-60 bases; clip: (operation, length) in front; big_del: one deletion of that many bases
    in the middle (more than a section spans: the read's realignment ends there) -> (reference bytes, [(op, n)])"""
    read = bytes(read)
    ref, ops, i = bytearray(), [], 0
    if clip:
        ops.append(clip)
        if clip[0] != "H":
            i = clip[1]
    skips = set(rng.choice(np.arange(len(read) // 4, 3 * len(read) // 4), n_skip, replace=False).tolist()) if n_skip else ()

    def push(op, n=1):
        if ops and ops[-1][0] == op:
            ops[-1] = (op, ops[-1][1] + n)
        else:
            ops.append((op, n))
    while i < len(read):
        u = rng.random()
        if big_del and i == len(read) // 2:
            ref += bytes(rng.choice(list(b"ACGT"), big_del).tolist()); push("D", big_del)
            big_del = 0
        if i in skips:
            n = int(rng.integers(20, 61))
            ref += bytes(rng.choice(list(b"ACGT"), n).tolist()); push("N", n)
            skips = skips - {i}
            continue
        if u < rate and ops and ops[-1][0] in "M=X":
            i += 1; push("I")
        elif u < 2 * rate and ops and ops[-1][0] in "M=X":
            ref.append(int(rng.choice(list(b"ACGT")))); push("D")
        elif u < 3 * rate:
            ref.append(int(rng.choice([b for b in b"ACGT" if b != read[i]]))); push("X" if eqx else "M"); i += 1
        else:
            ref.append(read[i]); push("=" if eqx else "M"); i += 1
    return bytes(ref), ops


def fixture_alignments(reads):
    """per fixture read (its bases): (reference, ref_pos, is_rev, cigar as uint32), from FIXTURE_SEED; every third read has its
    own flavour: = / X operations, a soft or hard clip, an N operation, a deletion longer than a section, lower case"""
    rng = np.random.default_rng(FIXTURE_SEED)
    out = []
    for i, seq in enumerate(reads):
        is_rev = int(i % 2)
        bam_seq = revcomp(seq) if is_rev else bytes(seq)
        clip = ("S", int(rng.integers(3, 30))) if i % 5 == 1 else ("H", 7) if i % 5 == 2 else None
        ref, ops = mutate(rng, bam_seq, n_skip=1 if i % 7 == 3 else 0, clip=clip, eqx=i % 3 == 0, big_del=150 if i % 9 == 5 else 94 if i % 9 == 7 else 0)
        if i % 11 == 4:
            ref = ref.lower()
        out.append((ref, int(rng.integers(0, 5_000_000)), is_rev, encode_cigar(ops)))
    return out


def level_of(model, seq):
    return model[0][A.kmer_ranks(seq)]


def synth_read(rng, model, read, counts, noise=0.3, epb=2.0, rev=False):
    """a read whose k-mer i has counts[i] events (in event order: descending k-mers for a reverse read, as the base-to-event map of
    such a read is looked up through flip_k_strand) -> (events, map, calib record)"""
    n_kmers = len(read) - K + 1
    counts = np.asarray(counts, np.int64)
    assert counts.size == n_kmers
    lv = level_of(model, read)
    rmap = np.full((n_kmers, 2), -1, np.int32)
    ev, at = [], 0
    for k in range(n_kmers):
        if counts[k]:
            rmap[k] = (at, at + counts[k] - 1)
            ev += [lv[k]] * int(counts[k]); at += int(counts[k])
    events = (np.array(ev, F) + rng.normal(0, noise, len(ev)).astype(F)).astype(F)
    calib = dict(scale=F(1.0), shift=F(0.0), var=F(1.0), log_var=F(0.0), events_per_base=float(epb), read_stat_flag=0)
    return events, rmap, calib


def case(rng, model, read, ops=None, counts=None, rev=False, epb=2.0, ref=None, region=(-1, -1), ref_pos=1000, calib=None, per=2):
    """one constructed case as a dict of everything gab_abea_realign takes for a read.  `read` is the original read; for a reverse
    case the BAM record (and so the CIGAR and the reference) holds its reverse complement."""
    read = bytes(read)
    n_kmers = len(read) - K + 1
    counts = np.full(n_kmers, per, np.int64) if counts is None else counts
    events, rmap, cal = synth_read(rng, model, read, counts, epb=epb, rev=rev)
    if calib:
        cal.update(calib)
    bam_seq = revcomp(read) if rev else read
    ops = [("M", len(read))] if ops is None else ops
    if ref is None:                                  # the reference the CIGAR implies, matching where it can
        ref, at = bytearray(), 0
        for op, n in ops:
            if op in "M=X":
                ref += bam_seq[at:at + n]; at += n
            elif op in "DN":
                ref += bytes(rng.choice(list(b"ACGT"), n).tolist())
            elif op in "IS":
                at += n
        ref = bytes(ref)
    return dict(ref=bytes(ref), ref_pos=ref_pos, is_rev=int(rev), cigar=encode_cigar(ops), seq_len=len(read), events=events, map=rmap, calib=cal,
                region=region)


def counts_with_rows(n_kmers, first_k, last_k, rows, per=1):
    """`per` event(s) per k-mer, but k-mers first_k .. last_k share exactly `rows` events between them"""
    c = np.full(n_kmers, per, np.int64)
    span = last_k - first_k + 1
    c[first_k:last_k + 1] = rows // span
    c[first_k:first_k + rows % span] += 1
    assert c[first_k:last_k + 1].sum() == rows
    return c


def make_cases(model):
    """name -> case; each the smallest shape at which its rule can go wrong (tests/test_abea_realign_gpu.py says which)"""
    rng = np.random.default_rng(CASE_SEED)
    B = lambda n: A_bases(rng, n)
    c = {}
    for n in (11, 12):                               # a reference of n bases: the 2 * k break
        c[f"ref_len_{n}"] = case(rng, model, B(24), ops=[("M", n), ("S", 24 - n)])
    for d in (1, 2):                                 # the stop event d events from the start event: k-mer 0 has events 0 .. d-1, k-mer 13 the next
        cnt = np.ones(19, np.int64); cnt[0] = d; cnt[1:13] = 0; cnt[13] = 2
        c[f"stop_event_{d}"] = case(rng, model, B(24), ops=[("M", 14), ("S", 10)], counts=cnt)
    for n in (49, 50, 51):                           # a first section of n + 1 rows, n of them emittable, and more sections behind it
        c[f"emittable_{n}"] = case(rng, model, B(260), counts=counts_with_rows(255, 0, 99, n))
    for n in (100, 101):                             # the last pair (read position seq_len - 6) exactly at curr_start_ref + n
        c[f"end_pair_{n}"] = case(rng, model, B(n + 6), per=1)
    for n in (95, 101):
        c[f"deletion_{n}"] = case(rng, model, B(60), ops=[("M", 30), ("D", n), ("M", 30)])
    cnt = np.zeros(35, np.int64); cnt[[0, 3, 7, 10, 14, 20, 24, 28, 31, 34]] = 1      # 96 k-mers on 6 rows: K runs across every lane
    c["k_run_over_the_lane_wrap"] = case(rng, model, B(40), ops=[("M", 20), ("D", 80), ("M", 20)], counts=cnt)
    for n in (ROWS - 1, ROWS, ROWS + 1):             # one section of n rows: k-mers 0 .. 123 share n - 1 events, an insertion among them
        c[f"rows_{n}"] = case(rng, model, B(130), ops=[("M", 40), ("I", 30), ("M", 60)], counts=counts_with_rows(125, 0, 123, n - 1), epb=4.0)
    for e in (1.0, 0.8, 5.0):
        c[f"epb_{e}"] = case(rng, model, B(150), epb=e)
    c["reverse"] = case(rng, model, B(180), rev=True, ops=[("M", 60), ("I", 3), ("M", 50), ("D", 4), ("M", 67)])
    read = B(120)
    ref = bytearray(read.lower()); ref[10:21] = b"MRWSYKVHDBN"; ref[40] = ord("n")
    c["lower_case_and_iupac"] = case(rng, model, read, ref=bytes(ref))
    c["leading_S"] = case(rng, model, B(100), ops=[("S", 9), ("M", 91)])
    c["leading_H"] = case(rng, model, B(100), ops=[("H", 9), ("M", 100)])
    c["leading_I"] = case(rng, model, B(100), ops=[("I", 9), ("M", 91)])
    c["second_segment_empty"] = case(rng, model, B(120), ops=[("M", 112), ("N", 30), ("S", 3), ("M", 5)])      # read positions 115 .. 119 > seq_len - 6
    c["three_segments"] = case(rng, model, B(200), ops=[("M", 70), ("N", 25), ("M", 60), ("N", 40), ("M", 70)])
    c["region_cuts_both_ends"] = case(rng, model, B(220), region=(1030, 1170))
    c["events_in_the_middle_only"] = case(rng, model, B(140))      # the first k-mers look forward for an event, the last ones back
    c["events_in_the_middle_only"]["map"][:20, :] = -1
    c["events_in_the_middle_only"]["map"][100:, :] = -1
    c["flat_model"] = case(rng, model, B(160))       # run on a handle whose pore model is flat
    # the two defined deviations: the reference cannot run these
    c["no_event"] = case(rng, model, B(140))
    c["no_event"]["map"][:, :] = -1
    c["strand"] = case(rng, model, B(140))           # a forward read whose first section stops at an event before its start event
    c["strand"]["map"][:, :] += 50
    c["strand"]["events"] = np.concatenate([np.full(50, 90.0, F), c["strand"]["events"]])
    c["strand"]["map"][100] = (10, 11)
    # the window of get_closest_event_to around the k-mer looked up first: read position k_idx, behind a soft clip of that length.
    # Back from k_idx to k_idx - 999, never entry k_idx - 1000 and never entry 0; then ahead from k_idx to k_idx + 999, never the last entry
    for name, (n, k_idx, empty) in WINDOW_CASES.items():
        cnt = np.full(n - K + 1, 2, np.int64)
        cnt[[e for e in empty if e < n - K + 1]] = 0
        c[name] = case(rng, model, B(n), ops=[("S", k_idx), ("M", n - k_idx)], counts=cnt)
        assert (c[name]["map"][:, 0] == -1).sum() == (cnt == 0).sum()
    return c


# name -> (bases, k_idx, the k-mers that have no event: their map entries are (-1, -1))
WINDOW_CASES = {
    **{f"behind_{d}": (200, 70, range(70 - d + 1, 71)) for d in (63, 64, 65)},      # the nearest event behind k_idx at distance d: a 64-entry chunk ends there
    "behind_999": (1200, 1050, range(52, 1051)),                     # found: the last entry the walk back reads
    "behind_1000": (1200, 1050, range(51, 1051)),                    # entry 50 is not read: the event is entry 1051's, from the walk ahead
    "behind_1000_nothing_ahead": (2100, 1010, range(11, 2010)),      # ... and entries 1010 .. 2009 have none: entry 2010 is not read, NO_EVENT
    "ahead_999": (1200, 5, range(0, 1004)),                          # nothing behind; entry 1004 is the last the walk ahead reads
    "ahead_1000": (1200, 5, range(0, 1005)),                         # entry 1005 is not read: NO_EVENT
    "entry_0_only": (200, 5, range(1, 6)),                           # entry 0 is not read going back from 5: the event is entry 6's
    "last_entry_only": (200, 5, range(0, 194)),                      # the last entry, 194, is not read going ahead: NO_EVENT
}
WINDOW_NO_EVENT = ("behind_1000_nothing_ahead", "ahead_1000", "last_entry_only")
DEVIATIONS = ("no_event", "strand") + WINDOW_NO_EVENT
FLAT_CASES = ("flat_model",)


def A_bases(rng, n):
    """n bases in which no two adjacent 6-mers are equal (no homopolymer runs of 6)"""
    while True:
        s = bytes(rng.choice(list(b"ACGT"), n).tolist())
        if all(s[i:i + K] != s[i + 1:i + 1 + K] for i in range(max(n - K, 0))):
            return s


FLAT_MODEL = (np.full(A.NKMER, 90.0, F), np.full(A.NKMER, 2.0, F), np.full(A.NKMER, math.log(2.0), F))
