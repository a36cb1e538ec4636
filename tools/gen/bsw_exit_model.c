/* CPU model of the score-only early exit and the left- and right-edge prune of the bsw DP kernels (genarchbench_amd/csrc/bsw.hip) -- TEST
 * INFRASTRUCTURE ONLY.  The prunes are described at model_one below.
 *
 * The scalar banded Smith-Waterman (BandedPairWiseSW::scalarBandedSWA of the reference), restated with the upper-bound exit
 * exactly as the kernels apply it, so
 * that a test can pin the kernels' cell counter to the rule.  After row i (band trimmed to the new [beg, end], R = tlen - 1 - i
 * rows left) a stored cell Hd[j] = H(i, j - 1) can still lead to at most
 *     pot(j) = Hd[j] + max_sc * min(R, qlen - j)        (0 when Hd[j] == 0: a zero diagonal yields M = 0)
 * in a later row.  The row loop ends when no source exceeds `best`:
 *     max( max_{beg <= j <= end} pot(j),
 *          hb + max_sc * min(R, qlen)   while beg == 0 and hb = h0 - o_del - e_del * (i + 2) > 0    (left boundary, next row),
 *          stale_pot )  <=  best
 * stale_pot is the running maximum of best + max_sc * (qlen - (i + w + 1)), folded in whenever the band clamp end > i + w + 1
 * fires (it cuts live cells, each at most `best`, which a later, wider row reads again).
 * The bound is evaluated only in rows that did not raise `best` and whose maximum cell alone passes it:
 *     rowmax + max_sc * min(R, qlen - 1 - rowmax_j) <= best.
 * With early_exit == 0 these are the score, rows and cells of the reference's full sweep (the prune needs the exit on). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {                      /* same layout as gab_bsw_params (include/gab.h) and the CPU checker's parameter struct */
    int32_t o_del, e_del, o_ins, e_ins, zdrop, end_bonus, w;
    int8_t mat[25];
} gab_bsw_model_params;

/* Left-edge prune (prune != 0, score-only rule like the exit): after row i and both zero trims, with m(j) = max(Hd[j], Ev[j]),
 * the band's left edge moves right over cell beg while beg < end and
 *     m(beg) == 0                                                      (the reference's own trim), or
 *     m(beg) + max_sc * min(R, qlen - beg) <= best, and -- while beg == 0 -- the next row's left boundary
 *     hb = h0 - o_del - e_del * (i + 2) is <= 0 or has hb + max_sc * min(R, qlen) <= best.
 * It applies only to pairs whose row -1 leaves no non-zero cell behind the first row's band clamp (qlen <= w + 1 or
 * h0 - oe_ins - (w + 1) * e_ins <= 0): then every cell right of `end` that a later row reads again is zero (bsw.hip's header has
 * the proof), and -- economy, not correctness -- only with zdrop == 0 or zdrop >= 8 * max_sc: under a z-drop worth fewer than eight
 * matches the guard below sends so many pairs back that the second passes cost more cells than the prune saves.
 * A pair that has dropped a live cell knows its row maxima only as lower bounds, so a row of it in which a z-drop could
 * fire (zdrop > 0, rowmax <= best, rowmax < best - zdrop) abandons the pass: the pair restarts from row -1 with the prune off and
 * the exit on, and the abandoned pass stays in the cell count.  So does a row of such a pair whose band ends inside the query and
 * short of the clamp (end < qlen, end != i + w + 1) on a cell hleft = H(i, end - 1) with hleft > e_ins and
 * hleft - e_ins + max_sc * min(R, qlen - end - 1) > best: the reference's band may be wider there and carry that F on.
 * Per row the left edge advances over at most the four cells beg0 .. beg0 + 3 next to the `beg` the row was swept with (the window
 * the kernels' zero trim has fetched anyway); a row whose zero trim has run past them prunes nothing on the left.
 *
 * Right-edge prune (same scope, same pairs): after the left prune, with jl the last live stored cell (where the reference's right
 * trim stopped; the next end is min(jl + 2, qlen)) and end0 the `end` the row was swept with, while jl >= beg, jl > end0 - 4 and
 *     m(jl) == 0  or  m(jl) + max_sc * min(R, qlen - jl) <= best
 * cell jl is SET TO ZERO (Hd = Ev = 0) and jl moves one cell left; end = min(jl + 2, qlen) afterwards.  The zeroing keeps every
 * cell right of `end` zero, which a later, wider row reads again.  A drop sets `dropped`: the two guards above cover these pairs
 * unchanged.  Again at most the four cells end0 - 3 .. end0 per row.
 * The right prune drops cells of pairs that still hold column 0, so a third guard joins the two: a row with rowmax == 0 of a pair
 * that has dropped a live cell, has beg == 0 and a left edge hb = h0 - o_del - e_del * (i + 1) > 0 (stored cell 0) with
 * hb + max_sc * min(R, qlen) > best abandons the pass too (the reference's row may hold dead cells that keep it going until that
 * edge raises the score).
 *
 *
 * Seeded prune (same scope, same pairs; bsw.hip's header has the proof).  The ungapped extension along the main diagonal is a path
 * of the DP, and so is its continuation over a gap onto a neighbouring diagonal, so a lower bound L of the pair's FINAL score is
 * known before row 0 (seed_bound and hop_bound below: the kernels use hop_bound's), and a cell whose potential is
 * below L cannot lead to the final score whatever `best` is at its row.  With thr = max(best, L - 1):
 *   thr replaces `best` in the left prune's cell test and its column-0 edge test, in the right prune's cell test, in the right-edge
 *   guard and in the zero-row guard; the z-drop guard, `best` itself and the exit's bound <= best are unchanged;
 *   before row 0 the cells of row -1 are dropped from the right under the right prune's test (R = tlen, best = h0, no cap: row -1
 *   and its potential both fall from left to right); an `end` below min(qlen, w + 1), what the reference sweeps row 0 with, counts
 *   as a drop, because row 0's F runs on right of the last live cell of row -1 and only the right-edge guard judges it.
 * Economy gates, on the parameters (seed_gates below) and per pair on the band (min(qlen, 2 w + 1) > 9, at model_one): thr == best
 * and row -1 stays whole where a gate is shut.
 *
 * `prune` selects the rule:  0 off;  7 what the kernels do (left prune capped, right prune, seeded);  1 the rule before the seed
 * (left prune capped, right prune);  3 the rule before the right prune (left prune uncapped, no right prune);  5 left prune capped,
 * no right prune;  6 left prune uncapped, right prune;  9 rule 7 without the prune of row -1;  10 rule 7 with thr == best (the prune
 * of row -1 alone);  11 rule 7 with its gates open at every parameter set AND the ungapped bound (what the gates were measured
 * against);  12 rule 11 with the hop bound;  14 rule 7 with the ungapped bound (what the hops are measured against).
 * TEST-ONLY wrong rules, the negative controls of tests/test_bsw_left_prune.py, tests/test_bsw_right_prune.py and
 * tests/test_bsw_seeded_prune.py: 2 is rule 1 with the left potential's columns short by two, 4 is rule 1 with the right potential's
 * columns short by two, 8 is rule 7 with thr = max(best, L): a cell of the diagonal path can have potential exactly L, 13 is rule 7
 * with the hop bound's gate (c) off (tests/test_bsw_hop_bound.py): a hop may then leave from the h0 corner. */
/* Row trace (gab_bsw_exit_trace below; NULL for the other entry points): per swept row of every pass, the abandoned one included,
 * the [beg, end) the row was swept with and which of the kernels' per-row paths the row takes. */
enum { TR_LZ4 = 1,        /* the left zero trim ran past its four-cell window */
       TR_TZ4 = 2,        /* the right one did */
       TR_LDROP = 4,      /* the left prune dropped a live cell */
       TR_RDROP = 8,      /* the right prune did */
       TR_BOUND = 16,     /* the exit's bound pass ran */
       TR_ZGUARD = 32,    /* the row abandoned the pass: z-drop guard */
       TR_RGUARD = 64,    /*                             right-edge guard */
       TR_ZROW = 128 };   /*                             zero-row guard */
typedef struct { int16_t *beg, *end; uint8_t *flags, *drops; int64_t cap, n; } row_trace;   /* drops: live and zero cells the left prune
                                                                                             * moved over beyond the zero trim | the right one's << 4 */

/* L: the ungapped extension from d = h0 along the main diagonal, k = 0 .. min(qlen, tlen) - 1, codes above 4 as N, stopped at the
 * first d <= 0.  While every d so far is positive, cell (k, k) holds at least d_{k+1} (M of a non-zero diagonal), lies inside the
 * reference's band (|i - j| = 0 <= w, and the zero trims pass only zero cells) and its row is not zero.  So the reference's score is
 * at least d_{k+1} if it sweeps row k, and if it z-drops in an earlier row i its score exceeds rowmax_i + zdrop >= d_{i+1} + zdrop. */
/* (kp: the first step, 1-based, that is worth L -- 0 while L == h0; mk: the minimum of d_0 .. d_kp.  Either may be NULL.) */
static int seed_scan(const gab_bsw_model_params *p, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int h0, int *kp, int *mk) {
    int d = h0, L = h0, mn = h0;
    const int n = qlen < tlen ? qlen : tlen;
    if (kp) *kp = 0;
    if (mk) *mk = h0;
    for (int k = 0; k < n && d > 0; k++) {
        d += p->mat[5 * (target[k] > 4 ? 4 : target[k]) + (query[k] > 4 ? 4 : query[k])];
        if (d <= 0) break;
        int v = d;
        if (p->zdrop > 0 && d - mn > p->zdrop) v = p->zdrop + 1 + mn;
        if (d < mn) mn = d;
        if (v > L) { L = v; if (kp) *kp = k + 1; if (mk) *mk = mn; }
    }
    return L;
}
static int seed_bound(const gab_bsw_model_params *p, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int h0) {
    return seed_scan(p, qlen, query, tlen, target, h0, NULL, NULL);
}

/* The three-value form of bwa_fill_scmat: one match score a > 0 on the diagonal of the four bases, one mismatch score off it, one
 * score wherever a code is 4 or above, neither above a.  The hop bound serves these matrices only; any other keeps the ungapped
 * bound. */
static int three_value(const gab_bsw_model_params *p, int *a, int *mm, int *nsc) {
    *a = p->mat[0]; *mm = p->mat[1]; *nsc = p->mat[4];
    for (int t = 0; t < 5; t++)
        for (int q = 0; q < 5; q++)
            if (p->mat[5 * t + q] != (t == 4 || q == 4 ? *nsc : t == q ? *a : *mm)) return 0;
    return *a > 0 && *mm <= *a && *nsc <= *a;
}

/* One chunk of a hop segment: the next cnt <= 16 bases from target[i], query[j] -> mismatches (both codes below 4 and different),
 * Ns (a code of 4 or above), and the matching bases in front of the first of either. */
static void hop_chunk(const uint8_t *target, const uint8_t *query, int i, int j, int cnt, int *nm, int *nn, int *lead) {
    *nm = *nn = 0; *lead = cnt;
    for (int b = cnt - 1; b >= 0; b--) {
        const int t = target[i + b], q = query[j + b];
        if (t >= 4 || q >= 4) { ++*nn; *lead = b; }
        else if (t != q) { ++*nm; *lead = b; }
    }
}

/* One diagonal segment behind a hop, from state (i, j, d, mn) -- the next step reads target[i] and query[j] -- in chunks of sixteen
 * bases counted from the segment's start (the last one shorter), by what a chunk's COUNTS say alone, so that the kernels need no
 * walk from base to base.  With nm mismatches and nn Ns among a chunk's cnt bases
 *     low   = d - nm * max(0, -mm) - nn * max(0, -nsc)        no prefix of the chunk is below it,
 *     d_end = d + cnt * a - nm * (a - mm) - nn * (a - nsc)    the exact value behind the chunk.
 * The scan stops in front of the first chunk with low <= 0 (it cannot vouch for a positive path there; stopping early only lowers L).
 * mn takes every low: it is at or below every path value so far, which only lowers the z-drop cap.  A chunk's end is worth
 * min(d_end, zdrop + 1 + mn); the largest worth is the peak.  Behind the peak's chunk the run of matching bases in front of the next
 * mismatch or N (of at most sixteen bases) is added: each of its steps is a step of the path, the last one worth the most.
 * Returns the peak's worth (0: none), its step (1-based), and d and mn there. */
typedef struct { int pk, kp, dk, mk; } hop_seg;
static hop_seg hop_scan(const gab_bsw_model_params *p, int a, int mm, int nsc, int qlen, const uint8_t *query, int tlen,
                        const uint8_t *target, int i, int j, int d, int mn) {
    hop_seg s = {0, 0, d, mn};
    const int n = tlen - i < qlen - j ? tlen - i : qlen - j, zd = p->zdrop;
    const int dm = mm < 0 ? -mm : 0, dn = nsc < 0 ? -nsc : 0;
    int nm, nn, lead;
    for (int k = 0; k < n; k += 16) {
        const int cnt = n - k < 16 ? n - k : 16;
        hop_chunk(target, query, i + k, j + k, cnt, &nm, &nn, &lead);
        const int low = d - nm * dm - nn * dn;
        if (low <= 0) break;
        d += cnt * a - nm * (a - mm) - nn * (a - nsc);
        if (low < mn) mn = low;
        int v = d;
        if (zd > 0 && d - mn > zd) v = zd + 1 + mn;
        if (v > s.pk) { s.pk = v; s.kp = k + cnt; s.dk = d; s.mk = mn; }
        if (zd > 0 && s.pk == zd + 1 + mn) break;           /* the cap is reached: no later step can be worth more */
    }
    /* behind the peak's chunk, the next (at most) sixteen bases once more in steps of four, by the same rule; then, of the four bases
     * behind the new peak and still among those sixteen, the run of matching bases in front of the first mismatch or N */
    const int base = s.kp, left = n - base < 16 ? n - base : 16;
    d = s.dk; mn = s.mk;
    for (int k = 0; k < left; k += 4) {
        const int cnt = left - k < 4 ? left - k : 4;
        hop_chunk(target, query, i + base + k, j + base + k, cnt, &nm, &nn, &lead);
        const int low = d - nm * dm - nn * dn;
        if (low <= 0) break;
        d += cnt * a - nm * (a - mm) - nn * (a - nsc);
        if (low < mn) mn = low;
        int v = d;
        if (zd > 0 && d - mn > zd) v = zd + 1 + mn;
        if (v > s.pk) { s.pk = v; s.kp = base + k + cnt; s.dk = d; s.mk = mn; }
    }
    const int o = s.kp - base;
    if (o < left) {
        hop_chunk(target, query, i + s.kp, j + s.kp, left - o < 4 ? left - o : 4, &nm, &nn, &lead);
        int d2 = s.dk + lead * a, v = d2;
        if (zd > 0 && d2 - s.mk > zd) v = zd + 1 + s.mk;
        if (lead > 0 && v > s.pk) { s.pk = v; s.kp += lead; s.dk = d2; }
    }
    return s;
}

/* L of the kernels: at most HOP_K one-gap hops on top of the ungapped extension (bsw.hip's header has the proof).  Segment 0 is
 * seed_bound's scan, base by base; the segments behind a hop are hop_scan's.  From a segment's peak step kp the candidates are its
 * cells at steps kp - {0, 4, 8}, each with three gaps: 1 or 2 reference bases deleted (o_del + g e_del), or 1 query base inserted
 * (o_ins + e_ins).  A candidate
 *   (c) starts at least one diagonal step into its segment (never from the h0 corner, the left edge or a gap cell),
 *   (a) lands on a positive value,  (b) lands inside the band |i - j| <= w of the pair's clamped w,
 *   and -- economy -- has at most HOP_EV mismatches or Ns among the first min(16, bases left) bases behind the gap, and a
 *   positive `low` there (hop_scan).
 * It carries mn = the minimum of the scan up to the peak and its own landing cell (at or below every value of its path: a smaller
 * cap).  ONE candidate is scanned: the one with the largest d behind its first chunk (first in the order back 0, 4, 8 x del 1,
 * del 2, ins 1 on a tie); it becomes the next segment if its peak exceeds L.  A segment whose peak is held down by the z-drop cap
 * starts no hop: no candidate's cap is higher.  no_gate_c is the negative control: a hop may leave from step 0 of segment 0. */
enum { HOP_K = 3, HOP_EV = 4 };
static int hop_bound(const gab_bsw_model_params *p, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int h0, int no_gate_c) {
    int a, mmis, nsc, kp, mk;
    int L = seed_scan(p, qlen, query, tlen, target, h0, &kp, &mk);
    if (!three_value(p, &a, &mmis, &nsc) || h0 <= 0) return L;
    int w = p->w;
    int lim = (int)((double)(qlen * a + p->end_bonus - p->o_ins) / p->e_ins + 1.);
    if (lim < 1) lim = 1;
    if (w > lim) w = lim;
    lim = (int)((double)(qlen * a + p->end_bonus - p->o_del) / p->e_del + 1.);
    if (lim < 1) lim = 1;
    if (w > lim) w = lim;
    const int dm = mmis < 0 ? -mmis : 0, dn = nsc < 0 ? -nsc : 0;
    int si = 0, sj = 0, dk = L;
    for (int hop = 0; hop < HOP_K; hop++) {
        if (p->zdrop > 0 && L - mk > p->zdrop) break;       /* (the peak is capped; dk = L holds otherwise) */
        int bestv = 0, bi = 0, bj = 0, bd = 0, dd = dk;
        for (int back = 0; back <= 8; back += 4) {
            const int c = kp - back;                             /* the start's step in its segment */
            if (c < (no_gate_c && hop == 0 ? 0 : 1)) break;
            if (back) for (int m = c + 4; m > c; m--) dd -= p->mat[5 * (target[si + m - 1] > 4 ? 4 : target[si + m - 1]) + (query[sj + m - 1] > 4 ? 4 : query[sj + m - 1])];
            const int ci = si + c, cj = sj + c;
            for (int g = 0; g < 3; g++) {
                const int ni = g < 2 ? ci + g + 1 : ci, nj = g < 2 ? cj : cj + 1;
                const int nd = g < 2 ? dd - p->o_del - (g + 1) * p->e_del : dd - p->o_ins - p->e_ins;
                int left = tlen - ni < qlen - nj ? tlen - ni : qlen - nj, nm, nn, lead;
                if (nd <= 0 || ni - nj > w || nj - ni > w || left < 1) continue;
                if (left > 16) left = 16;
                hop_chunk(target, query, ni, nj, left, &nm, &nn, &lead);
                if (nm + nn > HOP_EV || nd - nm * dm - nn * dn <= 0) continue;
                const int val = nd + left * a - nm * (a - mmis) - nn * (a - nsc);
                if (val > bestv) { bestv = val; bi = ni; bj = nj; bd = nd; }
            }
        }
        if (bestv == 0) break;
        const hop_seg s = hop_scan(p, a, mmis, nsc, qlen, query, tlen, target, bi, bj, bd, mk < bd ? mk : bd);
        if (s.pk <= L) break;
        L = s.pk; si = bi; sj = bj; kp = s.kp; dk = s.dk; mk = s.mk;
    }
    return L;
}

/* Economy gates of the seeded prune, on the parameters alone (bit 0: thr = max(best, L - 1); bit 1: the prune of row -1).  The
 * threshold is open wherever the prunes are: it measured no more cells than the rule before it at any parameter set.  The prune of
 * row -1 is open only with max_sc <= e_ins.  Where a match is worth more than an inserted base costs, the right-edge guard (the F
 * that leaves the narrowed band) sends 40 - 70 % of the read-like pairs through a second pass and the cell count rises by up to a
 * third; with max_sc <= e_ins that guard did not fire once for the row -1 prune (profiles/bsw_seeded_prune.md). */
static int seed_gates(const gab_bsw_model_params *p, int max_sc) {
    return 1 | (max_sc <= p->e_ins ? 2 : 0);
}

static void model_one(const gab_bsw_model_params *p, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int h0,
                      int early_exit, int prune, int32_t *Hd, int32_t *Ev, int32_t *score, int32_t *rows, int64_t *cells,
                      int64_t *pass_cells, int32_t *restarted, row_trace *tr) {
    const int oe_del = p->o_del + p->e_del, oe_ins = p->o_ins + p->e_ins;
    const int e_del = p->e_del, e_ins = p->e_ins;
    int64_t ncell = 0, npass = 0;

    int max_sc = 0;
    for (int k = 0; k < 25; k++) if (p->mat[k] > max_sc) max_sc = p->mat[k];
    int w = p->w;
    int lim = (int)((double)(qlen * max_sc + p->end_bonus - p->o_ins) / e_ins + 1.);
    if (lim < 1) lim = 1;
    if (w > lim) w = lim;
    lim = (int)((double)(qlen * max_sc + p->end_bonus - p->o_del) / e_del + 1.);
    if (lim < 1) lim = 1;
    if (w > lim) w = lim;
    const int prune_ok = early_exit && prune && (qlen <= w + 1 || h0 - oe_ins - (w + 1) * e_ins <= 0) &&
                         (p->zdrop == 0 || p->zdrop >= 8 * max_sc);
    const int short_by = prune == 2 ? 2 : 0, short_r = prune == 4 ? 2 : 0;
    const int left_cap = !(prune == 3 || prune == 6), right_prune = prune != 3 && prune != 5;
    const int seeded = prune >= 7 && prune <= 14;
    /* per pair: a band that can hold more than nine cells, min(qlen, 2 w + 1) > 9.  A narrower one is swept in at most two loop trips
     * of the kernels and the seed has next to nothing to remove there (with w <= 8 restriction (a) already fails for every h0 above
     * oe_ins + 9 e_ins); the narrow bands are also where the kernels' edge-cell paths live, whose tests read their cases off the
     * default rule's trace */
    const int seed_ok = seeded && (qlen < 2 * w + 1 ? qlen : 2 * w + 1) > 9;
    const int gates = !seed_ok ? 0 : prune == 11 || prune == 12 ? 3 : seed_gates(p, max_sc) & (prune == 9 ? 1 : prune == 10 ? 2 : 3);
    /* thr = max(best, Lm1): Lm1 = 0 leaves thr == best (best >= h0 >= 0) */
    const int Lm1 = !(prune_ok && (gates & 1)) ? 0
                    : prune == 11 || prune == 14 ? seed_bound(p, qlen, query, tlen, target, h0) - 1
                    : hop_bound(p, qlen, query, tlen, target, h0, prune == 13) - (prune == 8 ? 0 : 1);
    const int row_prune = prune_ok && (gates & 2);

    int best = h0, i = 0, redo = 0;
    for (int pass = 0; pass < 2; pass++) {
        const int do_prune = prune_ok && pass == 0;
        int abandon = 0, dropped = 0;
        memset(Hd, 0, sizeof(int32_t) * (size_t)(qlen + 1));
        memset(Ev, 0, sizeof(int32_t) * (size_t)(qlen + 1));
        Hd[0] = h0;
        if (qlen >= 1) Hd[1] = h0 > oe_ins ? h0 - oe_ins : 0;
        for (int j = 2; j <= qlen && Hd[j - 1] > e_ins; j++) Hd[j] = Hd[j - 1] - e_ins;

        int best_i = -1, best_j = -1, stale_pot = 0;
        int beg = 0, end = qlen;
        best = h0;
        if (do_prune && row_prune) {
            /* the prune of row -1: stored cell j is the diagonal of cell (0, j), tlen rows and qlen - j columns are left.  Cell 0
             * stays (its potential is that of the whole pair) */
            const int thr = best > Lm1 ? best : Lm1;
            int jl = qlen;
            for (; jl >= 1; jl--) {
                int cl = qlen - jl;
                if (Hd[jl] && Hd[jl] + max_sc * (tlen < cl ? tlen : cl) > thr) break;
                Hd[jl] = 0;
            }
            end = jl + 2 < qlen ? jl + 2 : qlen;
            if (end < (qlen < w + 1 ? qlen : w + 1)) dropped = 1;      /* the reference sweeps row 0 up to there */
        }
        for (i = 0; i < tlen; i++) {
            const int8_t *srow = p->mat + 5 * (target[i] > 4 ? 4 : target[i]);
            const int R = tlen - 1 - i;
            if (beg < i - w) beg = i - w;
            if (end > i + w + 1) {
                end = i + w + 1;
                int sp = best + max_sc * (qlen - end);
                if (sp > stale_pot) stale_pot = sp;
            }
            if (end > qlen) end = qlen;
            const int beg0 = beg, end0 = end;
            int hleft = 0;
            if (beg == 0) {
                hleft = h0 - (p->o_del + e_del * (i + 1));
                if (hleft < 0) hleft = 0;
            }
            int f = 0, rowmax = 0, rowmax_j = -1, j;
            for (j = beg; j < end; j++) {
                int diag = Hd[j], e = Ev[j];
                Hd[j] = hleft;
                int M = diag ? diag + srow[query[j] > 4 ? 4 : query[j]] : 0;
                int h = M > e ? M : e;
                if (f > h) h = f;
                hleft = h;
                if (!(rowmax > h)) rowmax_j = j;
                if (h > rowmax) rowmax = h;
                int t = M - oe_del; if (t < 0) t = 0;
                e -= e_del; if (t > e) e = t;
                Ev[j] = e;
                t = M - oe_ins; if (t < 0) t = 0;
                f -= e_ins; if (t > f) f = t;
            }
            ncell += (end > beg) ? end - beg : 0;
            Hd[end] = hleft; Ev[end] = 0;
            uint8_t *trf = NULL;
            if (tr) {
                if (tr->n < tr->cap) { tr->beg[tr->n] = (int16_t)beg; tr->end[tr->n] = (int16_t)end; tr->flags[tr->n] = 0; tr->drops[tr->n] = 0; trf = &tr->flags[tr->n]; }
                tr->n++;
            }
            if (rowmax == 0) {
                /* zero-row guard: a pair that has dropped a live cell cannot tell whether the reference's row is zero too; while it
                 * still holds column 0 and this row's left edge (stored cell 0, the diagonal of cell (i + 1, 0)) can reach `best`,
                 * the reference may go on from that edge */
                if (dropped && beg == 0) {
                    int hb = h0 - p->o_del - e_del * (i + 1);
                    if (hb > 0 && hb + max_sc * (R < qlen ? R : qlen) > (best > Lm1 ? best : Lm1)) abandon = 1;
                }
                if (trf && abandon) *trf |= TR_ZROW;
                i++; break;
            }
            int try_exit = 0;
            if (rowmax > best) {
                best = rowmax; best_i = i; best_j = rowmax_j;
            } else {
                if (p->zdrop > 0) {
                    if (dropped && rowmax < best - p->zdrop) { abandon = 1; if (trf) *trf |= TR_ZGUARD; i++; break; }
                    int di = i - best_i, dj = rowmax_j - best_j;
                    if (di > dj) {
                        if (best - rowmax - (di - dj) * e_del > p->zdrop) { i++; break; }
                    } else {
                        if (best - rowmax - (dj - di) * e_ins > p->zdrop) { i++; break; }
                    }
                }
                int cl = qlen - 1 - rowmax_j;
                try_exit = early_exit && rowmax + max_sc * (R < cl ? R : cl) <= best;
            }
            const int thr = best > Lm1 ? best : Lm1;      /* (best is this row's already) */
            /* right-edge guard: the F that leaves the band's last column is at most hleft - e_ins; the reference, whose band may
             * reach further right than a pruned pair's, carries it on */
            if (dropped && end < qlen && end != i + w + 1 && hleft > e_ins) {
                int cl = qlen - end - 1;
                if (hleft - e_ins + max_sc * (R < cl ? R : cl) > thr) { abandon = 1; if (trf) *trf |= TR_RGUARD; i++; break; }
            }
            for (j = beg; j < end && Hd[j] == 0 && Ev[j] == 0; j++) {}
            beg = j;
            for (j = end; j >= beg && Hd[j] == 0 && Ev[j] == 0; j--) {}
            int jl = j;
            end = j + 2 < qlen ? j + 2 : qlen;
            if (trf) *trf |= (beg - beg0 >= 4 ? TR_LZ4 : 0) | (end0 - jl >= 4 ? TR_TZ4 : 0);
            if (do_prune && beg < end) {
                int go = 1;
                if (beg == 0) {                    /* (cell 0 is live here: the zero trim stopped at it) */
                    int hb = h0 - p->o_del - e_del * (i + 2);
                    go = hb <= 0 || hb + max_sc * (R < qlen ? R : qlen) <= thr;
                }
                if (go) {
                    const int from = beg;
                    for (; beg < end && !(left_cap && beg >= beg0 + 4); beg++) {
                        int m = Hd[beg] > Ev[beg] ? Hd[beg] : Ev[beg];
                        int cl = qlen - beg - short_by;
                        if (m && m + max_sc * (R < cl ? R : cl) > thr) break;
                    }
                    if (beg > from) dropped = 1;   /* (cell `from` is live) */
                    if (trf && beg > from) { *trf |= TR_LDROP; tr->drops[tr->n - 1] |= (uint8_t)(beg - from > 15 ? 15 : beg - from); }
                }
            }
            if (do_prune && right_prune && jl >= beg && jl > end0 - 4) {     /* (cell jl is live: the zero trim stopped at it) */
                const int from = jl;
                for (; jl >= beg && jl > end0 - 4; jl--) {
                    int m = Hd[jl] > Ev[jl] ? Hd[jl] : Ev[jl];
                    int cl = qlen - jl - short_r;
                    if (m && m + max_sc * (R < cl ? R : cl) > thr) break;
                    Hd[jl] = 0; Ev[jl] = 0;
                }
                if (jl < from) { dropped = 1; end = jl + 2 < qlen ? jl + 2 : qlen; }
                if (trf && jl < from) { *trf |= TR_RDROP; tr->drops[tr->n - 1] |= (uint8_t)((from - jl) << 4); }
            }
            if (try_exit) {
                int bound = stale_pot;
                if (beg == 0) {
                    int hb = h0 - p->o_del - e_del * (i + 2);
                    if (hb > 0) { hb += max_sc * (R < qlen ? R : qlen); if (hb > bound) bound = hb; }
                }
                for (j = beg; j <= end; j++) {
                    int cl = qlen - j;
                    int pot = Hd[j] ? Hd[j] + max_sc * (R < cl ? R : cl) : 0;
                    if (pot > bound) bound = pot;
                }
                npass += end >= beg ? end - beg + 1 : 0;
                if (trf) *trf |= TR_BOUND;
                if (bound <= best) { i++; break; }
            }
        }
        if (!abandon) break;
        redo = 1;
    }
    *score = best; *rows = i; *cells = ncell; *pass_cells = npass;
    if (restarted) *restarted = redo;
}

/* per pair: score, rows swept (of the pass that finished), DP cells evaluated (an abandoned pass included), cells read by the bound
 * passes, and -- restarted may be NULL -- whether the pair abandoned its pruned pass */
void gab_bsw_exit_model(const gab_bsw_model_params *p, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry,
                        const int64_t *qry_off, const int32_t *len1, const int32_t *len2, const int32_t *h0, int64_t n,
                        int early_exit, int prune, int32_t *score, int32_t *rows, int64_t *cells, int64_t *pass_cells,
                        int32_t *restarted) {
#pragma omp parallel
    {
        int cap = 512;
        int32_t *buf = (int32_t *)malloc(sizeof(int32_t) * 2 * (size_t)(cap + 1));
#pragma omp for schedule(dynamic, 256)
        for (int64_t k = 0; k < n; k++) {
            int ql = len2[k];
            if (ql > cap) {
                cap = ql;
                free(buf);
                buf = (int32_t *)malloc(sizeof(int32_t) * 2 * (size_t)(cap + 1));
            }
            model_one(p, ql, qry + qry_off[k], len1[k], ref + ref_off[k], h0[k], early_exit, prune, buf, buf + ql + 1, &score[k],
                      &rows[k], &cells[k], &pass_cells[k], restarted ? &restarted[k] : NULL, NULL);
        }
        free(buf);
    }
}

/* gab_bsw_exit_model plus the row trace: pair k's rows go to tr_beg / tr_end / tr_flags [trace_off[k], trace_off[k + 1]) in the order
 * they were swept (an abandoned pass first), trace_rows[k] says how many there were -- rows beyond the pair's room are counted but not
 * stored, so a caller that sees trace_rows[k] > trace_off[k + 1] - trace_off[k] calls again with more room (2 * len1[k] always holds).
 * tr_beg / tr_end are the band [beg, end) the row's cells were computed over; tr_flags the TR_* bits above; tr_drops the cells the
 * left prune moved the edge over (low nibble, at most 15 is recorded) and the cells the right prune zeroed (high nibble). */
void gab_bsw_exit_trace(const gab_bsw_model_params *p, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry,
                        const int64_t *qry_off, const int32_t *len1, const int32_t *len2, const int32_t *h0, int64_t n,
                        int early_exit, int prune, int32_t *score, int32_t *rows, int64_t *cells, int64_t *pass_cells,
                        int32_t *restarted, const int64_t *trace_off, int32_t *trace_rows, int16_t *tr_beg, int16_t *tr_end,
                        uint8_t *tr_flags, uint8_t *tr_drops) {
#pragma omp parallel
    {
        int cap = 512;
        int32_t *buf = (int32_t *)malloc(sizeof(int32_t) * 2 * (size_t)(cap + 1));
#pragma omp for schedule(dynamic, 256)
        for (int64_t k = 0; k < n; k++) {
            int ql = len2[k];
            if (ql > cap) {
                cap = ql;
                free(buf);
                buf = (int32_t *)malloc(sizeof(int32_t) * 2 * (size_t)(cap + 1));
            }
            row_trace tr = {tr_beg + trace_off[k], tr_end + trace_off[k], tr_flags + trace_off[k], tr_drops + trace_off[k], trace_off[k + 1] - trace_off[k], 0};
            model_one(p, ql, qry + qry_off[k], len1[k], ref + ref_off[k], h0[k], early_exit, prune, buf, buf + ql + 1, &score[k],
                      &rows[k], &cells[k], &pass_cells[k], restarted ? &restarted[k] : NULL, &tr);
            trace_rows[k] = (int32_t)tr.n;
        }
        free(buf);
    }
}

/* the seeded prune's lower bound L of every pair's score (seed_bound above), whatever the gates say */
void gab_bsw_seed_bound(const gab_bsw_model_params *p, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry,
                        const int64_t *qry_off, const int32_t *len1, const int32_t *len2, const int32_t *h0, int64_t n, int32_t *L) {
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < n; k++) L[k] = seed_bound(p, len2[k], qry + qry_off[k], len1[k], ref + ref_off[k], h0[k]);
}

/* the lower bound the kernels use: seed_bound plus the chain of one-gap hops (hop_bound above), whatever the gates say */
void gab_bsw_hop_bound(const gab_bsw_model_params *p, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry,
                       const int64_t *qry_off, const int32_t *len1, const int32_t *len2, const int32_t *h0, int64_t n, int wrong, int32_t *L) {
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < n; k++) L[k] = hop_bound(p, len2[k], qry + qry_off[k], len1[k], ref + ref_off[k], h0[k], wrong);
}
