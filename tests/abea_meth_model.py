"""A numpy restatement of calculate_methylation_for_read (abea/src/meth.c:501-658) around profile_hmm_score (abea/src/hmm.c:620-674:
the forward fill of hmm.c:305-524 with the output class of hmm.c:549-600), in the arithmetic of the reference built without fused
multiply-add and with ESL_LOG_SUM 1 (abea/src/f5c.h:70): float32 rounded after every operation, add_logs = the table-driven
p7_FLogsum (abea/src/logsum.h:61-71), the six scores of a state folded left to right in the order written.  It is the contract of
gab_abea_meth (include/gab.h), the defined deviations included, and it holds the seeded generators of the CpG model and of the
constructed cases.  The reference preparation, the CIGAR encoding, the transitions and the fixture's alignments are
abea_realign_model's.

The cells of one anti-diagonal (row + block constant) do not depend on each other, so the fill runs diagonal by diagonal as arrays,
element by element the same operations as the reference's loop; lp_end is folded afterwards over the rows of the last k-mer in row
order, M, B, K per row, which is the order in which the reference's loop meets them."""
import math

import numpy as np

import abea_model as A
import abea_realign_model as R

K = A.K
F = np.float32
NI = F(-np.inf)
NKMER5 = 15625                                        # 5 ** 6: the alphabet A C G M T (hmm.c:21-52)
LOGSUM_TBL = 16000                                    # logsum.h:18
MIN_SEPARATION, MAX_SPAN, MIN_EVENTS = 10, 200, 10    # meth.c:542, 571, 601
BLOCKS_PER_LANE = 4                                   # GAB_ABEA_METH_BLOCKS_PER_LANE: k-mer blocks a lane of the scoring kernel owns in a wide group
ONE_BLOCK_KMERS = 64                                  # GAB_ABEA_METH_ONE_BLOCK_KMERS: up to this many k-mers a lane owns one block
SKIPPED, NO_EVENT, STRAND, TRANSITIONS = 1, 2, 4, 8   # gab_abea_meth_read.flags
COUNTERS = ("n_sites", "groups", "skipped_start", "skipped_span", "skipped_unbounded", "skipped_short", "flags", "cells")
FOLDS = {"dominated": 0, "table": 0}                  # folds whose operands were 15.7 or more apart / that read the table


def logsum_table():
    """p7_FLogsumInit (logsum.h:35-48) with the C library's double exp and log"""
    return np.array([math.log(1.0 + math.exp(-i / 1000.0)) for i in range(LOGSUM_TBL)], F)


TABLE = logsum_table()


def logsum(a, b):
    """p7_FLogsum (logsum.h:61-71) on float32 arrays"""
    with np.errstate(all="ignore"):
        mx = np.where(a > b, a, b).astype(F); mn = np.where(a < b, a, b).astype(F)
        d = (mx - mn).astype(F)
        plain = (mn == NI) | (d >= F(15.7))
        idx = np.where(plain, F(0), (d * F(1000.0)).astype(F)).astype(np.int64)
        FOLDS["dominated"] += int(((mn != NI) & (d >= F(15.7))).sum()); FOLDS["table"] += int((~plain).sum())
        return np.where(plain, mx, (mx + TABLE[idx]).astype(F)).astype(F)


def fold(scores, emission):
    """update_cell of the forward output (hmm.c:558-566)"""
    s = scores[0]
    for x in scores[1:]:
        s = logsum(s, x)
    return (s + emission).astype(F)


def flank_table(n):
    """pre_flank[i] (hmm.c:172-205) for i < n.  post_flank (hmm.c:132-168) is the same numbers from the other end: post_flank[i] of a
    fill of num_events rows is this table at num_events - 1 - i, expression for expression.  The constants are doubles, every store
    rounds to float."""
    t = np.zeros(max(n, 2), F)
    t[0] = F(math.log(1 - 0.5))
    t[1] = F(math.log(0.5) + -3.0 + math.log(1 - 0.9))
    for i in range(2, n):
        t[i] = F(math.log(0.9) + -3.0 + float(t[i - 1]))
    return t


RANK5 = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("M"): 3, ord("T"): 4}


def kmer_rank5(s):
    r = 0
    for c in s:
        r = r * 5 + RANK5[c]
    return r


def methylate(s):
    """meth.c:359-382: every complete CG becomes MG, left to right, skipping past a match"""
    out, i = bytearray(s), 0
    while i < len(s):
        if s[i:i + 2] == b"CG":
            out[i] = ord("M"); i += 2
        else:
            i += 1
    return bytes(out)


def reverse_complement_meth(s):
    """meth.c:387-420: an MG of the input puts G at the output position of its M and M at the one of its G"""
    out, i, j = bytearray(len(s)), 0, len(s) - 1
    comp = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}
    while i < len(s):
        if s[i:i + 2] == b"MG":
            out[j] = ord("G"); out[j - 1] = ord("M"); j -= 2; i += 2
        else:
            assert s[i] != ord("M")
            out[j] = comp[s[i]]; j -= 1; i += 1
    return bytes(out)


def hmm_ranks(seq, rc_seq, rc):
    """hmm.c:376-393"""
    n = len(seq) - K + 1
    return np.array([kmer_rank5(rc_seq[len(seq) - ki - K:len(seq) - ki] if rc else seq[ki:ki + K]) for ki in range(n)], np.int64)


def hmm_score(ranks, events, e1, e2, stride, level, scal, t):
    """profile_hmm_score with HAF_ALLOW_PRE_CLIP | HAF_ALLOW_POST_CLIP for V variants of one sequence at once: ranks (V, n_kmers)
    -> V float32 scores"""
    ranks = np.atleast_2d(ranks)
    V, n_kmers = ranks.shape
    n_rows = abs(e2 - e1) + 1
    flank = flank_table(n_rows + 1)
    with np.errstate(all="ignore"):
        gp_mean = (F(scal[0]) * level[0][ranks] + F(scal[1])).astype(F)
        gp_stdv = (level[1][ranks] * F(scal[2])).astype(F)
        c = (F(-0.918938) - (level[2][ranks] + F(scal[3])).astype(F)).astype(F)
        x = np.asarray(events, F)[e1 + np.arange(n_rows) * stride]
        a = ((x[None, :, None] - gp_mean[:, None, :]) / gp_stdv[:, None, :]).astype(F)
        em = (c[:, None, :] + ((F(-0.5) * a).astype(F) * a).astype(F)).astype(F)       # (V, row - 1, k-mer)
        M = np.full((V, n_rows + 1, n_kmers + 1), NI, F); B = M.copy(); Kk = M.copy()  # block 0 is the start state, row 0 the initial row
        for d in range(2, n_rows + n_kmers + 1):
            r = np.arange(max(1, d - n_kmers), min(n_rows, d - 1) + 1); b = d - r
            ninf = np.full((V, r.size), NI, F)
            soft = np.where(b == 1, (F(0.0) + flank[r - 1]).astype(F), NI).astype(F)[None, :].repeat(V, 0)
            nM = fold([(t["mm_self"] + M[:, r - 1, b]).astype(F), (t["mm_next"] + M[:, r - 1, b - 1]).astype(F), (t["bm_self"] + B[:, r - 1, b]).astype(F),
                       (t["bm_next"] + B[:, r - 1, b - 1]).astype(F), (t["km"] + Kk[:, r - 1, b - 1]).astype(F), soft], em[:, r - 1, b - 1])
            nB = fold([(t["mb"] + M[:, r - 1, b]).astype(F), ninf, (t["bb"] + B[:, r - 1, b]).astype(F), ninf, ninf, ninf], F(0.0))
            nK = fold([ninf, (t["mk"] + M[:, r, b - 1]).astype(F), ninf, (t["bk"] + B[:, r, b - 1]).astype(F), (t["kk"] + Kk[:, r, b - 1]).astype(F), ninf], F(0.0))
            M[:, r, b] = nM; B[:, r, b] = nB; Kk[:, r, b] = nK
        end = np.full(V, NI, F)
        for row in range(1, n_rows + 1):                 # hmm.c:479-487
            post = flank[n_rows - row]
            for S in (M, B, Kk):
                end = logsum(end, ((F(0.0) + S[:, row, n_kmers]).astype(F) + post).astype(F))
    return end


def aligned_pairs(cigar, ref_pos):
    """get_aligned_segments (meth.c:15-87) with read_stride 1 -> (n, 2) (ref_pos, read_pos); None for an N operation (the reference exits)"""
    if any((int(w) & 15) == 3 for w in np.asarray(cigar, np.uint32).tolist()):
        return None
    return R.aligned_segments(cigar, ref_pos)[0]


def closest_event(k_idx, start_of, size):
    """get_closest_event_to (meth.c:92-117)"""
    def walk(start, stop, stride):
        while start != stop:
            if start_of[start] != -1:
                return int(start_of[start])
            start += stride
        return -1
    before = walk(k_idx, max(0, k_idx - 1000), -1)
    after = walk(k_idx, min(k_idx + 1000, size - 1), 1)
    return after if before == -1 else before


def event_alignment_record(cigar, ref_pos, is_rev, seq_len, start_of):
    """get_event_alignment_record (meth.c:124-185) -> (ref_pos array, event of pair i as a function)"""
    pairs = aligned_pairs(cigar, ref_pos)
    assert pairs is not None, "spliced alignment"
    pairs = pairs[(pairs[:, 1] >= K) & (pairs[:, 1] + K < seq_len)]
    n_map = seq_len - K + 1

    def event_of(i):
        k = int(pairs[i, 1])
        return closest_event(seq_len - k - K if is_rev else k, start_of, n_map)
    if len(pairs) and event_of(0) == event_of(len(pairs) - 1):
        pairs = pairs[:0]
    return pairs[:, 0], event_of


def find_by_ref_bounds(ref_of, event_of, ref_start, ref_stop):
    """meth.c:422-467 -> (e1, e2) or None"""
    n = len(ref_of)
    start = int(np.searchsorted(ref_of, ref_start, "left")); stop = int(np.searchsorted(ref_of, ref_stop, "left"))
    if start == n or stop == n:
        return None
    left = ref_of[start] <= ref_start or (start != 0 and ref_of[start - 1] <= ref_start)
    right = ref_of[stop] >= ref_stop or (stop != n and ref_of[stop + 1] >= ref_start)
    if not (left and right):
        return None
    return event_of(start), event_of(stop)


def cpg_groups(seq):
    """meth.c:532-558 on the prepared reference -> [(first, last, n_cpg)]"""
    sites = [i for i in range(len(seq) - 1) if seq[i:i + 2] == b"CG"]
    groups, i = [], 0
    while i < len(sites):
        j = i + 1
        while j < len(sites) and sites[j] - sites[j - 1] <= MIN_SEPARATION:
            j += 1
        groups.append((sites[i], sites[j - 1], j - i))
        i = j
    return groups


def call_methylation(ref, ref_pos, is_rev, cigar, seq_len, events, rmap, calib, cpg):
    """one read -> (sites: list of dicts with the fields of gab_abea_site, record dict with the fields of gab_abea_meth_read);
    cpg: (mean, stdv, log stdv) of 15625 entries"""
    rec = dict.fromkeys(COUNTERS, 0)
    sites = []
    if int(calib["read_stat_flag"]) != 0:
        rec["flags"] = SKIPPED
        return sites, rec
    seq = R.prepare_ref(ref)
    assert seq is not None
    groups = cpg_groups(seq)
    rec["groups"] = len(groups)
    if not float(calib["events_per_base"]) >= 1.0:
        rec["flags"] = TRANSITIONS
        return sites, rec
    t = R.transitions(calib["events_per_base"])
    scal = (calib["scale"], calib["shift"], calib["var"], calib["log_var"])
    ref_of, event_of = event_alignment_record(cigar, ref_pos, is_rev, seq_len, np.asarray(rmap).reshape(-1, 2)[:, 0])
    for first, last, n_cpg in groups:
        sub_start, sub_end = first - MIN_SEPARATION, last + MIN_SEPARATION
        if sub_start <= MIN_SEPARATION:
            rec["skipped_start"] += 1
            continue
        if last - first > MAX_SPAN:
            rec["skipped_span"] += 1
            continue
        sub = seq[sub_start:sub_end + 1]
        found = find_by_ref_bounds(ref_of, event_of, sub_start + ref_pos, sub_end + ref_pos)
        if found is None:
            rec["skipped_unbounded"] += 1
            continue
        e1, e2 = found
        if e1 < 0 or e2 < 0:                            # defined: the reference indexes event -1
            rec["flags"] |= NO_EVENT
            continue
        if abs(e2 - e1) <= MIN_EVENTS:                  # the ratio test of meth.c:597-601 divides by a negative span: it never fires
            rec["skipped_short"] += 1
            continue
        stride = 1 if e1 <= e2 else -1
        if bool(is_rev) != (stride == -1):              # defined: the assert of hmm.c:322
            rec["flags"] |= STRAND
            continue
        msub = methylate(sub)
        ranks = np.stack([hmm_ranks(sub, R.revcomp(sub), is_rev), hmm_ranks(msub, reverse_complement_meth(msub), is_rev)])
        ll = hmm_score(ranks, events, e1, e2, stride, cpg, scal, t)
        rec["cells"] += 2 * (abs(e2 - e1) + 1) * ranks.shape[1]
        sites.append(dict(start_position=first + ref_pos, end_position=last + ref_pos, n_cpg=n_cpg, first_cpg=first, event_start=e1, event_stop=e2,
                          ll_unmethylated=F(ll[0]), ll_methylated=F(ll[1])))
    rec["n_sites"] = len(sites)
    return sites, rec


def methylation_rows(contig, qname, ref, ref_pos, sites):
    """the lines of f5c.c:1746-1753, output version 1"""
    seq = R.prepare_ref(ref)
    rows = []
    for s in sites:
        u, m = float(F(s["ll_unmethylated"])), float(F(s["ll_methylated"]))
        a = int(s["first_cpg"]); b = a + int(s["end_position"]) - int(s["start_position"])
        rows.append("%s\t%d\t%d\t%s\t%.2f\t%.2f\t%.2f\t%d\t%d\t%s" % (contig, s["start_position"], s["end_position"], qname, m - u, m, u, 1, s["n_cpg"],
                                                                       seq[a - K + 1:b + K].decode()))
    return rows


def site_bits(sites):
    """a read's sites as the golden JSON holds them: [start, end, n_cpg, first_cpg, e1, e2, bits of ll_u, bits of ll_m]"""
    b = lambda v: int(np.array([v], F).view(np.uint32)[0])
    return [[int(s["start_position"]), int(s["end_position"]), int(s["n_cpg"]), int(s["first_cpg"]), int(s["event_start"]), int(s["event_stop"]),
             b(s["ll_unmethylated"]), b(s["ll_methylated"])] for s in sites]


# ---- the generators ----------------------------------------------------------------------------------------------------------------------
CPG_SEED = 20251101
CASE_SEED = 20251102


def make_cpg_model(model, seed=CPG_SEED):
    """15625 entries from the nucleotide model's 4096: a k-mer without M takes the values of the same bases, one with M those of the
    k-mer with C in its place, the mean shifted by a seeded -4 .. +4 and the spread widened a little -> (mean, stdv, log stdv)"""
    rng = np.random.default_rng(seed)
    digits = np.stack([(np.arange(NKMER5) // 5 ** (K - 1 - t)) % 5 for t in range(K)], 1)      # A C G M T
    as4 = np.array([0, 1, 2, 1, 3])[digits]
    r4 = (as4 * 4 ** np.arange(K - 1, -1, -1)).sum(1)
    has_m = (digits == 3).any(1)
    mean = model[0][r4].astype(F); stdv = model[1][r4].astype(F)
    mean = np.where(has_m, (mean + rng.uniform(-4, 4, NKMER5).astype(F)).astype(F), mean).astype(F)
    stdv = np.where(has_m, (stdv * F(1.125)).astype(F), stdv).astype(F)
    return mean, stdv, A.log_stdv_of(stdv)


FLAT_CPG = (np.full(NKMER5, 90.0, F), np.full(NKMER5, 2.0, F), np.full(NKMER5, math.log(2.0), F))


def bases_with_cpgs(rng, n, at):
    """n bases whose only CpGs start at the positions `at`"""
    s = bytearray(R.A_bases(rng, n))
    for i in range(1, n):
        if s[i - 1] == ord("C") and s[i] == ord("G"):
            s[i] = ord("A")
    for p in at:
        s[p] = ord("C"); s[p + 1] = ord("G")
    got = [i for i in range(n - 1) if s[i:i + 2] == b"CG"]
    assert got == sorted(set(at)), (got, at)
    return bytes(s)


def group_of(first, span):
    """CpG starts of one group from `first` to `first + span` (not 1: two CpGs cannot start on adjacent bases), ten apart where they can be"""
    assert span != 1
    at, last = [first], first + span
    while last - at[-1] > MIN_SEPARATION:
        at.append(at[-1] + (MIN_SEPARATION if last - at[-1] - MIN_SEPARATION != 1 else MIN_SEPARATION - 1))
    return sorted(set(at + [last]))


def kmer_count_cases(bpl=BLOCKS_PER_LANE, one=ONE_BLOCK_KMERS):
    """k-mers of a group = its span + 16, 16 .. 216: one below, at and one above the block counts at which the lanes in use change
    (every count up to `one`, where a lane owns one block and the kernel changes its path; multiples of the blocks a lane owns
    above it): at the low end, at the change of path, at half and at the whole of the widest group.  This is the sample that the
    reference itself ran (the golden files hold it); width_cases() below takes every count, against the model"""
    marks = sorted({bpl * 5, one, bpl * 32, (216 // bpl) * bpl})
    return sorted({n for m in marks for n in (m - 1, m, m + 1) if 16 <= n <= 216} | {16, 18, 215, 216})


WIDTH_SEED = 20251103


def width_cases(model, widths):
    """per k-mer count a case of one group that wide on 13 rows (the k-mers of the group share 12 events), every other one a reverse
    read: cheap enough to take EVERY count, so that each number of lanes in use and each position of the last k-mer in its lane's
    blocks is met, whatever the kernel's blocks a lane and change of path are"""
    rng = np.random.default_rng(WIDTH_SEED)
    out = {}
    for n in widths:
        ref = bases_with_cpgs(rng, n + 60, group_of(30, n - 16))
        rev = bool(n % 2)
        cnt = R.counts_with_rows(n + 55, 20, n + 23, 12)
        out[n] = R.case(rng, model, R.revcomp(ref) if rev else ref, rev=rev, counts=cnt[::-1].copy() if rev else cnt)
    return out


def all_widths(bpl=BLOCKS_PER_LANE, one=ONE_BLOCK_KMERS):
    """every k-mer count a group can have, 16 .. 216 without 17 (two CpGs cannot start on adjacent bases); `one` and the multiples of
    `bpl` above it are among them with both neighbours"""
    w = [n for n in range(16, 217) if n != 17]
    assert {one - 1, one, one + 1} <= set(w) and all({m - 1, m, m + 1} <= set(w) for m in range(one + bpl, 216, bpl))
    return w


def make_cases(model, bpl=BLOCKS_PER_LANE, one=ONE_BLOCK_KMERS):
    """name -> case (the dicts of abea_realign_model.case, without a region); each the smallest shape at which its rule can go wrong"""
    rng = np.random.default_rng(CASE_SEED)
    c = {}

    def simple(n, at, **kw):
        read = bases_with_cpgs(rng, n, at)
        kw.setdefault("per", 1)
        return R.case(rng, model, R.revcomp(read) if kw.get("rev") else read, **kw)
    c["single_cpg"] = simple(120, [60], per=2)
    c["separation_10"] = simple(140, [60, 70])
    c["separation_11"] = simple(140, [60, 71])
    c["span_200"] = simple(300, group_of(40, 200))
    c["span_202"] = simple(300, group_of(40, 200) + [242])
    c["sub_start_10"] = simple(100, [20])
    c["sub_start_11"] = simple(100, [21])
    for d in (10, 11):                                   # the events of sub_start and sub_end exactly d apart
        c[f"event_distance_{d}"] = simple(120, [60], counts=R.counts_with_rows(115, 50, 69, d))
    cnt = np.ones(115, np.int64); cnt[50:70] = 20
    c["rows_400"] = simple(120, [60], counts=cnt, epb=4.0)
    for n in kmer_count_cases(bpl, one):
        c[f"kmers_{n}"] = simple(n + 60, group_of(30, n - 16))
    c["kmers_64_reverse"] = simple(124, group_of(30, 48), rev=True)
    # a neighbouring group's CpG 11 before the first: its G is the first base of the sub-sequence and its C is outside, so it is
    # methylated in neither string; and 11 behind the last: its C is the base after the sub-sequence.  (An M at the very end of the
    # methylated reverse complement would need a CpG that starts at last + 9, which would belong to the group.)
    c["reverse_cpg_across_both_ends"] = simple(140, [49, 60, 71], rev=True)
    c["forward_cpg_across_both_ends"] = simple(140, [49, 60, 71])
    read = bytearray(bases_with_cpgs(rng, 130, [60])); read[60:68] = b"CGCGCGCG"
    c["cgcg_run"] = R.case(rng, model, bytes(read), per=1)
    c["cgcg_run_reverse"] = R.case(rng, model, R.revcomp(bytes(read)), per=1, rev=True)
    read = bases_with_cpgs(rng, 200, [40, 100, 160])
    ref = bytearray(read.lower()); ref[40] = ord("y"); ref[101] = ord("R"); ref[70:72] = b"NG"; ref[130:132] = b"sk"; ref[160:162] = b"Cg"
    c["lower_case_and_iupac"] = R.case(rng, model, read, ref=bytes(ref), per=1)      # yg makes a CpG, CR and NG none, sk one (S -> C, K -> G)
    read = bases_with_cpgs(rng, 260, [60, 130, 200])
    c["cigar_operations"] = R.case(rng, model, read, per=1, ops=[("S", 7), ("=", 38), ("X", 2), ("=", 8), ("I", 3), ("=", 10), ("D", 4), ("=", 50), ("X", 1), ("=", 60),
                                                                   ("D", 2), ("M", 30), ("I", 2), ("M", 49)])
    c["hard_clip"] = R.case(rng, model, bases_with_cpgs(rng, 120, [60]), per=1, ops=[("H", 9), ("M", 120)])
    c["past_the_last_pair"] = simple(120, [60, 108])     # sub_end = 118: its read position is beyond seq_len - 7
    read = bases_with_cpgs(rng, 120, [60])
    c["reference_longer_than_the_cigar"] = R.case(rng, model, read, per=1, ref=read + b"A" + bases_with_cpgs(rng, 40, [20]))
    c["no_cpg"] = simple(100, [])
    c["read_stat_flag"] = simple(120, [60], calib=dict(read_stat_flag=2))
    c["flat_model"] = simple(160, [50, 58, 110], per=2)  # run with FLAT_CPG: the operands of a fold differ by the transitions alone
    c["degenerate_record"] = simple(120, [60])           # the first and the last pair on one event: the record is emptied
    c["degenerate_record"]["map"][6:] = (5, 5)
    # the defined deviations: the reference cannot run these
    cnt = np.ones(2295, np.int64); cnt[100:2200] = 0
    c["no_event"] = simple(2300, [1150, 2250], counts=cnt)
    c["strand"] = simple(140, [60])                      # a forward read whose sub_end looks up an event far before sub_start's
    c["strand"]["map"][70] = (3, 3)
    c["transitions"] = simple(120, [60], epb=0.8)
    # the window of get_closest_event_to around the k-mer of sub_start (read position first CpG - 10 of a forward read): back from
    # k_idx to k_idx - 999, never entry k_idx - 1000 and never entry 0; then ahead from k_idx to k_idx + 999, never the last entry
    for name, (n, first, empty) in WINDOW_CASES.items():
        cnt = np.ones(n - K + 1, np.int64)
        cnt[list(empty)] = 0
        c[name] = simple(n, [first], counts=cnt)
        assert (c[name]["map"][:, 0] == -1).sum() == (cnt == 0).sum()
    # group starts on the edges of the 64 reference positions that the kernel looks at per step, and look-backs and groups across them
    for name, (n, at, rev) in STEP_CASES.items():
        c[name] = simple(n, at, rev=rev)
    return c


# name -> (bases, position of the one CpG, the k-mers that have no event: their map entries are (-1, -1)); k_idx = first - 10
WINDOW_CASES = {
    **{f"behind_{d}": (200, 110, range(100 - d + 1, 101)) for d in (63, 64, 65)},   # the nearest event behind k_idx at distance d
    "behind_999": (1200, 1060, range(52, 1051)),                     # found: the last entry the walk back reads
    "behind_1000": (1200, 1060, range(51, 1051)),                    # entry 50 is not read: the event is entry 1051's, from the walk ahead
    "behind_1000_nothing_ahead": (2100, 1020, range(11, 2010)),      # ... and entries 1010 .. 2009 have none: entry 2010 is not read, NO_EVENT
    "ahead_999": (1200, 21, range(0, 1010)),                         # nothing behind k_idx = 11; entry 1010 is the last the walk ahead reads
    "ahead_1000": (1200, 21, range(0, 1011)),                        # entry 1011 is not read: NO_EVENT
    "entry_0_only": (200, 21, range(1, 12)),                         # entry 0 is not read going back from 11, the lowest k_idx of a scored group
    "last_entry_only": (200, 100, range(0, 194)),                    # the last entry, 194, is not read: the first and the last pair find no
}                                                                    # event, the record is emptied and the group is unbounded
WINDOW_NO_EVENT = ("behind_1000_nothing_ahead", "ahead_1000")
# name -> (bases, CpG positions, reverse read)
STEP_CASES = {
    **{f"start_{p}": (200, [p], False) for p in (63, 64, 127, 128)},
    "start_64_reverse": (200, [64], True), "start_127_reverse": (200, [127], True),
    "sites_54_64": (200, [54, 64], False), "sites_54_64_reverse": (200, [54, 64], True),      # one group: the look-back from 64 crosses the step
    "sites_53_64": (200, [53, 64], False), "sites_53_64_reverse": (200, [53, 64], True),      # two groups
    "group_60_to_130": (220, group_of(60, 70), False), "group_60_to_130_reverse": (220, group_of(60, 70), True),
    "site_at_ref_len_minus_2": (120, [60, 118], False),              # the last position a site can have; its sub-sequence ends past the reference
}
DEVIATIONS = ("no_event", "strand", "transitions") + WINDOW_NO_EVENT
FLAT_CASES = ("flat_model",)
