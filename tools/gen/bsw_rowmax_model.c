/* CPU model of how the 8-bit bsw DP kernel (bsw_dp8, genarchbench_amd/csrc/bsw.hip) takes a row's maximum and its column -- TEST
 * INFRASTRUCTURE ONLY.
 *
 * The scalar banded Smith-Waterman (BandedPairWiseSW::scalarBandedSWA of the reference) with all six result fields, its row loop
 * unchanged except for the row maximum.  The reference keeps (rowmax, rowmax_j) cell by cell, ties to the later column.  The kernel
 * folds keys (H << 16) | column into one running maximum:
 *   - an exact key for the head cell (a band that starts on an odd column),
 *   - ONE key per group of four columns behind it, (largest H of the group << 16) | the group's first column,
 *   - exact keys for the remainder pair (two or three columns left) and for the tail cell (one column left),
 * and resolves the column after the row: with kj the winning key's column, rowmax_j is the LAST column c of
 * [kj, min(kj + 3, end - 1)] with H(i, c) == rowmax.  Groups cover disjoint, increasing ranges, so the winning key names the last
 * group that holds the maximum; an exact key's own column matches and no later column can (it would have made a larger key).
 * With resolve == 0 the column is the key's (a group's FIRST column): the negative control of tests/test_bsw_rowmax.py.
 *
 * `ties` reports, per pair, where a row's (positive) maximum was held by more than one column, so that a test can tell whether a
 * batch exercises the rule: bit 0 two columns of one group, bit 1 columns of two neighbouring groups, bit 2 the head cell and
 * another column, bit 3 a column of the remainder pair and another column, bit 4 the tail cell and another column. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {                      /* same layout as gab_bsw_params (include/gab.h) and the CPU checker's parameter struct */
    int32_t o_del, e_del, o_ins, e_ins, zdrop, end_bonus, w;
    int8_t mat[25];
} gab_bsw_rowmax_params;

static void rowmax_one(const gab_bsw_rowmax_params *p, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int h0,
                       int resolve, int32_t *Hd, int32_t *Ev, int32_t *Hrow, int32_t *out, int32_t *ties) {
    const int oe_del = p->o_del + p->e_del, oe_ins = p->o_ins + p->e_ins;
    const int e_del = p->e_del, e_ins = p->e_ins;

    memset(Hd, 0, sizeof(int32_t) * (size_t)(qlen + 1));
    memset(Ev, 0, sizeof(int32_t) * (size_t)(qlen + 1));
    Hd[0] = h0;
    if (qlen >= 1) Hd[1] = h0 > oe_ins ? h0 - oe_ins : 0;
    for (int j = 2; j <= qlen && Hd[j - 1] > e_ins; j++) Hd[j] = Hd[j - 1] - e_ins;

    int max_sc = 0;
    for (int k = 0; k < 25; k++) if (p->mat[k] > max_sc) max_sc = p->mat[k];
    int w = p->w;
    int lim = (int)((double)(qlen * max_sc + p->end_bonus - p->o_ins) / e_ins + 1.);
    if (lim < 1) lim = 1;
    if (w > lim) w = lim;
    lim = (int)((double)(qlen * max_sc + p->end_bonus - p->o_del) / e_del + 1.);
    if (lim < 1) lim = 1;
    if (w > lim) w = lim;

    int best = h0, best_i = -1, best_j = -1, g_i = -1, gscore = -1, max_off = 0;
    int beg = 0, end = qlen;
    for (int i = 0; i < tlen; i++) {
        const int8_t *srow = p->mat + 5 * (target[i] > 4 ? 4 : target[i]);
        if (beg < i - w) beg = i - w;
        if (end > i + w + 1) end = i + w + 1;
        if (end > qlen) end = qlen;
        int hleft = 0;
        if (beg == 0) {
            hleft = h0 - (p->o_del + e_del * (i + 1));
            if (hleft < 0) hleft = 0;
        }
        int f = 0, j;
        for (j = beg; j < end; j++) {                    /* the reference's cell, H(i, j) kept for the keys */
            int diag = Hd[j], e = Ev[j];
            Hd[j] = hleft;
            int M = diag ? diag + srow[query[j] > 4 ? 4 : query[j]] : 0;
            int h = M > e ? M : e;
            if (f > h) h = f;
            hleft = h;
            Hrow[j] = h;
            int t = M - oe_del; if (t < 0) t = 0;
            e -= e_del; if (t > e) e = t;
            Ev[j] = e;
            t = M - oe_ins; if (t < 0) t = 0;
            f -= e_ins; if (t > f) f = t;
        }
        Hd[end] = hleft; Ev[end] = 0;
        /* the keys, in the kernel's order; a key is (value, column), compared value first */
        int64_t rowpk = 0;
#define KEY(v, c) (((int64_t)(v) << 32) | (int64_t)(c))
#define FOLD(k) do { int64_t k_ = (k); if (k_ > rowpk) rowpk = k_; } while (0)
        j = beg;
        if ((j & 1) && j < end) { FOLD(KEY(Hrow[j], j)); j++; }
        for (; j + 3 < end; j += 4) {
            int m4 = Hrow[j];
            for (int c = j + 1; c < j + 4; c++) if (Hrow[c] > m4) m4 = Hrow[c];
            FOLD(KEY(m4, j));
        }
        if (j + 1 < end) { FOLD(KEY(Hrow[j], j)); FOLD(KEY(Hrow[j + 1], j + 1)); j += 2; }
        if (j < end) { FOLD(KEY(Hrow[j], j)); j++; }
#undef KEY
#undef FOLD
        const int rowmax = (int)(rowpk >> 32);
        int rowmax_j = (int)(rowpk & 0xffffffff);
        if (j == qlen) {
            if (!(gscore > hleft)) g_i = i;
            if (hleft > gscore) gscore = hleft;
        }
        if (rowmax == 0) break;
        {                                                /* the census of ties: which kinds of key the maximum's columns fall under */
            int nmax = 0, last_group = -2, bits = 0, g = 0;
            for (int c = beg; c < end; c++) nmax += Hrow[c] == rowmax;
            int c = beg;
            if ((c & 1) && c < end) { if (Hrow[c] == rowmax && nmax > 1) bits |= 4; c++; }
            for (; c + 3 < end; c += 4, g++) {
                int in = 0;
                for (int d = c; d < c + 4; d++) in += Hrow[d] == rowmax;
                if (in > 1) bits |= 1;
                if (in && last_group == g - 1) bits |= 2;
                if (in) last_group = g;
            }
            if (c + 1 < end) { if ((Hrow[c] == rowmax || Hrow[c + 1] == rowmax) && nmax > 1) bits |= 8; c += 2; }
            if (c < end && Hrow[c] == rowmax && nmax > 1) bits |= 16;
            *ties |= bits;
        }
        if (resolve) {
            const int kj = rowmax_j;
            for (int c = kj; c <= kj + 3 && c <= end - 1; c++) if (Hrow[c] == rowmax) rowmax_j = c;
        }
        if (rowmax > best) {
            best = rowmax; best_i = i; best_j = rowmax_j;
            int off = rowmax_j - i; if (off < 0) off = -off;
            if (off > max_off) max_off = off;
        } else if (p->zdrop > 0) {
            int di = i - best_i, dj = rowmax_j - best_j;
            if (di > dj) {
                if (best - rowmax - (di - dj) * e_del > p->zdrop) break;
            } else {
                if (best - rowmax - (dj - di) * e_ins > p->zdrop) break;
            }
        }
        for (j = beg; j < end && Hd[j] == 0 && Ev[j] == 0; j++) {}
        beg = j;
        for (j = end; j >= beg && Hd[j] == 0 && Ev[j] == 0; j--) {}
        end = j + 2 < qlen ? j + 2 : qlen;
    }
    out[0] = best; out[1] = best_j + 1; out[2] = best_i + 1; out[3] = g_i + 1; out[4] = gscore; out[5] = max_off;
}

/* per pair: score, qle, tle, gtle, gscore, max_off (int32 [n][6]) and the tie census bits */
void gab_bsw_rowmax_model(const gab_bsw_rowmax_params *p, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry,
                          const int64_t *qry_off, const int32_t *len1, const int32_t *len2, const int32_t *h0, int64_t n,
                          int resolve, int32_t *result, int32_t *ties) {
#pragma omp parallel
    {
        int cap = 512;
        int32_t *buf = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)(cap + 1));
#pragma omp for schedule(dynamic, 256)
        for (int64_t k = 0; k < n; k++) {
            int ql = len2[k];
            if (ql > cap) {
                cap = ql;
                free(buf);
                buf = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)(cap + 1));
            }
            ties[k] = 0;
            rowmax_one(p, ql, qry + qry_off[k], len1[k], ref + ref_off[k], h0[k], resolve, buf, buf + cap + 1, buf + 2 * (cap + 1),
                       result + 6 * k, &ties[k]);
        }
        free(buf);
    }
}
