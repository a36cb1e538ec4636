// abea: calculate_methylation_for_read (abea/src/meth.c:501-658) around profile_hmm_score (abea/src/hmm.c:620-674), behind
// gab_abea_meth* (include/gab.h, which holds the contract).  The handle is the one of abea.hip (abea_handle.h).
//
// Arithmetic: the reference's as built without fused multiply-add (the pragma below) and with ESL_LOG_SUM 1: every add_logs is
// p7_FLogsum (abea/src/logsum.h:61-71), a float subtraction, a float multiplication, a truncation and a table read.  No log or exp on
// the device: the transitions, the flanks and the table come from the host's libm.
//
// Shape (DESIGN.md, section "abea: call-methylation"):
//   (host)      lengths, offsets, calibration records and every CIGAR come to the host and are validated there.  The walk over a
//               CIGAR writes its run table: one entry per M / = / X operation, cut to the pairs that get_event_alignment_record keeps
//               (6 <= read_pos < seq_len - 6).  No pair is expanded: the lower bounds of find_by_ref_bounds are binary searches there.
//   mt_prep     one wavefront per read.  Checks what only the device holds (reference bytes, event means, map entries), stores the
//               reference as base codes, finds the CpG groups (a site starts a group when no site lies in the ten bases before it,
//               so the lanes find the starts independently, 64 positions a step, and each lane that found one walks its group), and
//               per group runs the skips, the bounds and get_closest_event_to.  Scored groups become work items; their slot among
//               the read's sites is a prefix count over the lanes, so the sites keep the order of their positions.  Everything
//               goes to scratch: nothing of the caller's is written before the verdict is known.
//   mt_score    persistent wavefronts take work items from a counter.  A wavefront scores both variants of its group: they share
//               every event and differ only in the ranks of the k-mers that hold an M.  The table logsum is not associative, so the
//               K chain along a row cannot be reassociated as realign's maximum is; the cells run in skewed order instead: a lane
//               owns one k-mer block (groups of up to 64 k-mers) or BPL consecutive ones, at step t lane l computes row t - l, and takes its left neighbour's last block
//               for the same row from the step before (one lane shift) and for the row above from the step before that (kept).
//               Only one row of state lives in registers.  lp_end is folded by the lane that owns the last k-mer as it produces
//               the rows, which is row order.  The first thing the kernel does is look at the verdict; then it copies the per-read
//               records out and writes the sites with ordinary vector stores.
//
// The logsum table (64000 bytes) is read through the caches: a copy in LDS per block of four wavefronts measured slower, for the
// occupancy it costs (profiles/abea_meth.md), and is not built.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "gab_internal.h"
#include "gab_pair_stage.h"
#include "abea_handle.h"

#pragma clang fp contract(off)

namespace {

constexpr int K = GAB_ABEA_K;
constexpr int BPL = GAB_ABEA_METH_BLOCKS_PER_LANE;
constexpr int NK5 = GAB_ABEA_METH_NKMER, TBL = GAB_ABEA_METH_LOGSUM;
constexpr int MIN_SEPARATION = 10, MAX_SPAN = 200, MIN_EVENTS = 10;      // meth.c:542, 571, 601
constexpr int MAX_KMERS = MAX_SPAN + 2 * MIN_SEPARATION + 1 - K + 1;      // 216
constexpr int ONE_BLOCK_KMERS = GAB_ABEA_METH_ONE_BLOCK_KMERS;
constexpr int SCORE_WAVES = 4;                                            // wavefronts of a scoring block
constexpr unsigned SCORE_BLOCKS = 2048;                                   // persistent blocks: more than are resident at once (three a CU at 130 VGPRs);
                                                                          // those that start late find the item counter run out and end
static_assert(sizeof(gab_abea_site) == 32 && sizeof(gab_abea_meth_read) == 40, "record layout");
static_assert(MAX_KMERS <= 64 * BPL && ONE_BLOCK_KMERS <= 64, "a group's k-mers fit one wavefront");

struct mt_run { int32_t ref, read, len, pair; };           // the kept pairs of an M / = / X operation: the first, how many, its index in the record
struct mt_job {                                            // one read, as the host planned it
    int64_t code_off, ev_off, map_off, out_off, run_off, room;
    int32_t ref_pos, ref_len, seq_len, n_events, n_runs, n_pairs, is_rev, state;      // state: 0 runs, else the flag that stops it
    float t[11];                                           // as gab_abea_transitions writes them
    float scale, shift, var, log_var, pad;
};
struct mt_item { int32_t read, first, last, n_cpg, e1, e2; int64_t out_idx; };      // one scored group
struct mt_head { int32_t bad_read, short_room_read; uint32_t n_items, next_item; unsigned long long rows; };
GAB_STATIC_ATOMIC64(mt_head, rows);
struct mt_reads {                                          // the call's per-read arrays (device pointers)
    const char *ref; const int64_t *ref_off;
    const float *event_mean; const gab_abea_range *map;
};

// ---- the event alignment record, by run ---------------------------------------------------------------------------------------------------
// aligned_pair_lower_bound (meth.c:422-431): the index of the first pair whose reference position is not below v
__device__ __forceinline__ int mt_lower_bound(const mt_run *ru, int n_runs, int n_pairs, int64_t v) {
    int lo = 0, hi = n_runs;                               // -> the first run whose last pair is not below v
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)ru[mid].ref + ru[mid].len - 1 < v) lo = mid + 1; else hi = mid;
    }
    if (lo == n_runs) return n_pairs;
    const int64_t d = v - ru[lo].ref;
    return ru[lo].pair + (d > 0 ? (int)d : 0);
}
__device__ __forceinline__ void mt_pair(const mt_run *ru, int n_runs, int i, int *ref, int *read) {
    int lo = 0, hi = n_runs;                               // -> the first run whose pairs start above i
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (ru[mid].pair <= i) lo = mid + 1; else hi = mid;
    }
    const mt_run q = ru[lo > 0 ? lo - 1 : 0];
    *ref = q.ref + (i - q.pair); *read = q.read + (i - q.pair);
}
// get_closest_event_to (meth.c:92-117); k_idx lies in [0, size)
__device__ __forceinline__ int mt_closest_event(const gab_abea_range *m, int k_idx, int size) {
    const int stop_before = max(0, k_idx - 1000), stop_after = min(k_idx + 1000, size - 1);
    for (int s = k_idx; s != stop_before; s--) { const int ei = m[s].start; if (ei != -1) return ei; }
    for (int s = k_idx; s != stop_after; s++) { const int ei = m[s].start; if (ei != -1) return ei; }
    return -1;
}
__device__ __forceinline__ int mt_event_of(const mt_job &J, const mt_run *ru, const gab_abea_range *m, int pair) {
    int ref, read;
    mt_pair(ru, J.n_runs, pair, &ref, &read);
    return mt_closest_event(m, J.is_rev ? J.seq_len - read - K : read, J.seq_len - K + 1);
}

__device__ __forceinline__ bool mt_site(const uint8_t *code, int i, int ref_len) { return i >= 0 && i + 1 < ref_len && code[i] == 1 && code[i + 1] == 2; }

enum { G_NONE = 0, G_SCORED, G_START, G_SPAN, G_UNBOUNDED, G_SHORT, G_NO_EVENT, G_STRAND, G_IDLE };

__global__ __launch_bounds__(64) void mt_prep(mt_reads R, const mt_job *jobs, const mt_run *runs, uint8_t *codes, mt_head *head, mt_item *items,
                                              gab_abea_meth_read *recs) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const mt_job J = jobs[r];
    const char *ref = R.ref + R.ref_off[r];
    uint8_t *code = codes + J.code_off;
    bool bad = false;
    for (int p = lane; p < J.ref_len; p += 64) {
        const int b = gab_abea_base_code(ref[p]);
        bad |= b < 0;
        code[p] = (uint8_t)(b & 3);
    }
    const float *ev = R.event_mean + J.ev_off;
    for (int i = lane; i < J.n_events; i += 64) bad |= !isfinite(ev[i]);
    const gab_abea_range *m = R.map + J.map_off;
    for (int i = lane; i < J.seq_len - K + 1; i += 64) {
        const gab_abea_range g = m[i];
        bad |= g.start < -1 || g.start >= J.n_events || g.stop < -1 || g.stop >= J.n_events;
    }
    if (bad) atomicMin(&head->bad_read, r);
    __syncthreads();                                       // the codes are read back by other lanes
    gab_abea_meth_read q;
    memset(&q, 0, sizeof q);
    if (J.state == GAB_ABEA_METH_SKIPPED) {
        q.flags = GAB_ABEA_METH_SKIPPED;
        if (lane == 0) recs[r] = q;
        return;
    }
    const mt_run *ru = runs + J.run_off;
    int n_pairs = J.n_pairs;                               // meth.c:169-178: a record whose first and last event are equal is emptied
    if (J.state == 0 && n_pairs > 0 && mt_event_of(J, ru, m, 0) == mt_event_of(J, ru, m, n_pairs - 1)) n_pairs = 0;
    long long cells = 0, rows = 0;
    for (int base = 0; base + 1 < J.ref_len; base += 64) {
        const int i = base + lane;
        bool start = mt_site(code, i, J.ref_len);
        for (int j = 1; j <= MIN_SEPARATION && start; j++) start = !mt_site(code, i - j, J.ref_len);
        int kind = G_NONE, last = i, n_cpg = 1, e1 = -1, e2 = -1;
        if (start) {
            for (;;) {                                     // the group's sites, until the next one is more than ten away or the span is too long anyway
                int next = -1;
                for (int j = 1; j <= MIN_SEPARATION && next < 0; j++) if (mt_site(code, last + j, J.ref_len)) next = last + j;
                if (next < 0 || last - i > MAX_SPAN) break;
                last = next; n_cpg++;
            }
            const int sub_start = i - MIN_SEPARATION, sub_end = last + MIN_SEPARATION;
            if (J.state != 0) kind = G_IDLE;
            else if (sub_start <= MIN_SEPARATION) kind = G_START;
            else if (last - i > MAX_SPAN) kind = G_SPAN;
            else {                                         // find_iter_by_ref_bounds (meth.c:433-453), as written
                const int64_t ref_start = (int64_t)sub_start + J.ref_pos, ref_stop = (int64_t)sub_end + J.ref_pos;
                const int a = mt_lower_bound(ru, J.n_runs, n_pairs, ref_start), b = mt_lower_bound(ru, J.n_runs, n_pairs, ref_stop);
                bool bounded = a < n_pairs && b < n_pairs;
                if (bounded) {
                    int ra, rb, rx, unused;
                    mt_pair(ru, J.n_runs, a, &ra, &unused); mt_pair(ru, J.n_runs, b, &rb, &unused);
                    bool left = ra <= ref_start;
                    if (!left && a != 0) { mt_pair(ru, J.n_runs, a - 1, &rx, &unused); left = rx <= ref_start; }
                    bool right = rb >= ref_stop;
                    if (!right && b + 1 < n_pairs) { mt_pair(ru, J.n_runs, b + 1, &rx, &unused); right = rx >= ref_start; }
                    bounded = left && right;
                }
                if (!bounded) kind = G_UNBOUNDED;
                else {
                    e1 = mt_event_of(J, ru, m, a); e2 = mt_event_of(J, ru, m, b);
                    const int dist = e1 > e2 ? e1 - e2 : e2 - e1;
                    if (e1 < 0 || e2 < 0) kind = G_NO_EVENT;
                    else if (dist <= MIN_EVENTS) kind = G_SHORT;
                    else if ((J.is_rev != 0) != (e1 > e2)) kind = G_STRAND;
                    else {
                        kind = G_SCORED;
                        const int len = min(sub_end, J.ref_len - 1) - sub_start + 1;
                        cells += 2ll * (dist + 1) * (len - K + 1); rows += dist + 1;
                    }
                }
            }
        }
        const unsigned long long scored = __ballot(kind == G_SCORED);
        const int slot = q.n_sites + __popcll(scored & ((1ull << lane) - 1ull));
        const bool keep = kind == G_SCORED && slot < J.room;      // (a read with less room than groups is refused below; its items are never looked at)
        const uint32_t at = gab_wave_slot(&head->n_items, keep);
        if (keep) items[at] = {r, i, last, n_cpg, e1, e2, J.out_off + slot};
        q.n_sites += __popcll(scored);
        q.groups += __popcll(__ballot(start));
        q.skipped_start += __popcll(__ballot(kind == G_START)); q.skipped_span += __popcll(__ballot(kind == G_SPAN));
        q.skipped_unbounded += __popcll(__ballot(kind == G_UNBOUNDED)); q.skipped_short += __popcll(__ballot(kind == G_SHORT));
        if (__ballot(kind == G_NO_EVENT)) q.flags |= GAB_ABEA_METH_NO_EVENT;
        if (__ballot(kind == G_STRAND)) q.flags |= GAB_ABEA_METH_STRAND;
    }
    for (int d = 32; d > 0; d >>= 1) { cells += __shfl_xor(cells, d); rows += __shfl_xor(rows, d); }
    if (lane == 0 && rows) atomicAdd(&head->rows, (unsigned long long)rows);
    q.cells = cells;
    if (J.state != 0) q.flags |= (uint32_t)J.state;
    if (q.groups > J.room) atomicMin(&head->short_room_read, r);
    if (lane == 0) recs[r] = q;
}

// ---- the scoring ---------------------------------------------------------------------------------------------------------------------------
// p7_FLogsum (logsum.h:61-71).  The index is clamped so that the read is always inside the table; where it was clamped the table is not used.
__device__ __forceinline__ float mt_logsum(float a, float b, const float *tab) {
    const float mx = a > b ? a : b, mn = a < b ? a : b;
    const float d = mx - mn;
    const float dc = d < 15.9f ? d : 15.9f;                // (a NaN, from -inf - -inf, goes to 15.9 too)
    int idx = (int)(dc * 1000.f);
    idx = idx < 0 ? 0 : idx > TBL - 1 ? TBL - 1 : idx;
    const float with = mx + tab[idx];
    return (mn == -INFINITY || d >= 15.7f) ? mx : with;
}
__device__ __forceinline__ float mt_up(float v, int lane) {      // the left neighbour lane's v; block 0 (left of lane 0) is -inf
    const float t = __shfl_up(v, 1);
    return lane == 0 ? -INFINITY : t;
}
// the base-5 digit (A C G M T, hmm.c:21-36) of base p of the sub-sequence [s0, s1] of the prepared reference: forward (the base itself,
// methylate(): a C whose G follows inside the sub-sequence is M) or of the reverse complement (the complement, reverse_complement_meth():
// the G of such a pair is M there)
__device__ __forceinline__ uint32_t mt_digit(const uint8_t *code, int p, int s0, int s1, bool rc, bool meth) {
    const int b = code[p];
    if (!rc) {
        if (meth && b == 1 && p + 1 <= s1 && code[p + 1] == 2) return 3u;
        return b == 3 ? 4u : (uint32_t)b;
    }
    if (meth && b == 2 && p - 1 >= s0 && code[p - 1] == 1) return 3u;
    const int c = 3 - b;
    return c == 3 ? 4u : (uint32_t)c;
}

// one work item by one wavefront, B k-mer blocks a lane
template <int B>
__device__ __forceinline__ void mt_score_item(const mt_item &I, const mt_job &J, const uint8_t *code, const float *ev, const float *cpg, const float *tab,
                                              const float *flank, gab_abea_site *out, int s0, int s1, int n_kmers, int lane) {
    const float NI = -INFINITY;
    const int n_lanes = (n_kmers + B - 1) / B;
    const int n_rows = (I.e1 > I.e2 ? I.e1 - I.e2 : I.e2 - I.e1) + 1, stride = I.e1 <= I.e2 ? 1 : -1;
    const bool rc = J.is_rev != 0;
    float mean[2][B], sd[2][B], c[2][B];
#pragma unroll
    for (int v = 0; v < 2; v++)
#pragma unroll
        for (int t = 0; t < B; t++) {
            const int k = B * lane + t;
            uint32_t rank = 0;
            if (k < n_kmers)
                for (int j = 0; j < K; j++) rank = rank * 5u + mt_digit(code, rc ? s0 + k + K - 1 - j : s0 + k + j, s0, s1, rc, v == 1);
            mean[v][t] = J.scale * cpg[rank] + J.shift;            // log_probability_match_r9, hmm.c:64-100
            sd[v][t] = cpg[NK5 + rank] * J.var;
            const float lsd = cpg[2 * NK5 + rank] + J.log_var;
            c[v][t] = -0.918938f - lsd;
        }
    const float mmS = J.t[0], mmN = J.t[1], bmS = J.t[2], bmN = J.t[3], km = J.t[4], mb = J.t[6], bb = J.t[7], mk = J.t[8], bk = J.t[9], kk = J.t[10];
    float M[2][B], Bd[2][B], Kk[2][B];                            // this lane's blocks, the row above the one it computes next
    float aM[2], aB[2], aK[2];                                    // the left neighbour's last block, the row above
    float end[2] = {NI, NI};
#pragma unroll
    for (int v = 0; v < 2; v++) {
        aM[v] = aB[v] = aK[v] = NI;
#pragma unroll
        for (int t = 0; t < B; t++) M[v][t] = Bd[v][t] = Kk[v][t] = NI;
    }
    const int last_lane = (n_kmers - 1) / B, last_t = (n_kmers - 1) % B;
    const int steps = n_rows + n_lanes - 1;
    for (int step = 0; step < steps; step++) {
        const int row = step - lane + 1;                          // 1 .. n_rows where this lane has work
        float lM[2], lB[2], lK[2];                                // the left neighbour's last block, this row: what it computed a step ago
#pragma unroll
        for (int v = 0; v < 2; v++) { lM[v] = mt_up(M[v][B - 1], lane); lB[v] = mt_up(Bd[v][B - 1], lane); lK[v] = mt_up(Kk[v][B - 1], lane); }
        if (row >= 1 && row <= n_rows && lane < n_lanes) {
            const float x = ev[I.e1 + (row - 1) * stride];
            const float soft = lane == 0 ? 0.0f + flank[row - 1] : NI;          // lp_sm + pre_flank[row - 1]: k-mer 0, PRE_CLIP (hmm.c:452-454)
            const float post = flank[n_rows - row];                              // post_flank[row - 1]
#pragma unroll
            for (int v = 0; v < 2; v++) {
                float pM = aM[v], pB = aB[v], pK = aK[v];         // block b - 1, the row above
                float cM = lM[v], cB = lB[v], cK = lK[v];         // block b - 1, this row
#pragma unroll
                for (int t = 0; t < B; t++) {
                    const float oM = M[v][t], oB = Bd[v][t], oK = Kk[v][t];
                    const float a = (x - mean[v][t]) / sd[v][t];
                    const float em = c[v][t] + ((-0.5f * a) * a);                 // log_normal_pdf, hmm.c:55-62
                    // the six scores in the order written (hmm.c:441-474); a -inf operand leaves a fold as it is
                    float s = mt_logsum(mmS + oM, mmN + pM, tab);
                    s = mt_logsum(s, bmS + oB, tab);
                    s = mt_logsum(s, bmN + pB, tab);
                    s = mt_logsum(s, km + pK, tab);
                    if (t == 0) s = mt_logsum(s, soft, tab);
                    const float nM = s + em;
                    const float nB = mt_logsum(mb + oM, bb + oB, tab) + 0.0f;
                    const float nK = mt_logsum(mt_logsum(mk + cM, bk + cB, tab), kk + cK, tab) + 0.0f;
                    M[v][t] = nM; Bd[v][t] = nB; Kk[v][t] = nK;
                    pM = oM; pB = oB; pK = oK;
                    cM = nM; cB = nB; cK = nK;
                    if (lane == last_lane && t == last_t) {       // update_end, hmm.c:479-487
                        end[v] = mt_logsum(end[v], (0.0f + nM) + post, tab);
                        end[v] = mt_logsum(end[v], (0.0f + nB) + post, tab);
                        end[v] = mt_logsum(end[v], (0.0f + nK) + post, tab);
                    }
                }
                aM[v] = lM[v]; aB[v] = lB[v]; aK[v] = lK[v];
            }
        }
    }
    if (lane == last_lane) {
        gab_abea_site s;
        s.start_position = I.first + J.ref_pos; s.end_position = I.last + J.ref_pos; s.n_cpg = I.n_cpg; s.first_cpg = I.first;
        s.event_start = I.e1; s.event_stop = I.e2; s.ll_unmethylated = end[0]; s.ll_methylated = end[1];
        out[I.out_idx] = s;
    }
}

__global__ __launch_bounds__(64 * SCORE_WAVES) void mt_score(mt_reads R, const mt_job *jobs, const uint8_t *codes, mt_head *head, const mt_item *items,
                                             const gab_abea_meth_read *recs, int n_reads, const float *cpg, const float *tab,
                                             const float *flank, gab_abea_site *out, gab_abea_meth_read *res) {
    if (head->bad_read != INT32_MAX || head->short_room_read != INT32_MAX) return;      // an input rule is broken: the call writes nothing
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_reads; i += gridDim.x * blockDim.x) res[i] = recs[i];
    const int lane = threadIdx.x & 63;
    const uint32_t n_items = head->n_items;
    for (;;) {
        uint32_t it = 0;
        if (lane == 0) it = atomicAdd(&head->next_item, 1u);
        it = (uint32_t)__builtin_amdgcn_readfirstlane((int)it);
        if (it >= n_items) break;
        const mt_item I = items[it];
        const mt_job &J = jobs[I.read];
        const int s0 = I.first - MIN_SEPARATION, s1 = min(I.last + MIN_SEPARATION, J.ref_len - 1);
        const int n_kmers = min(s1 - s0 + 1 - K + 1, MAX_KMERS);
        // up to ONE_BLOCK_KMERS k-mers a lane owns one block (most groups hold one CpG: 16 k-mers); wider groups BPL blocks a lane
        if (n_kmers <= ONE_BLOCK_KMERS) mt_score_item<1>(I, J, codes + J.code_off, R.event_mean + J.ev_off, cpg, tab, flank, out, s0, s1, n_kmers, lane);
        else mt_score_item<BPL>(I, J, codes + J.code_off, R.event_mean + J.ev_off, cpg, tab, flank, out, s0, s1, n_kmers, lane);
    }
}

void mt_reset(gab_abea_meth_state &S) {
    S.reads = S.groups = S.sites = S.rows = S.cells = 0;
    S.prep_ms = S.score_ms = S.total_ms = 0.f;
}

// pre_flank[i] (hmm.c:172-205); post_flank[i] of num_events rows (hmm.c:132-168) is this at num_events - 1 - i, expression for expression.
// The reference's compiler folds the logarithms of these constants; doubles, every store rounds to float.
void mt_flank(std::vector<float> &t, size_t n) {
    t.assign(std::max<size_t>(n, 2), 0.0f);
    t[0] = log(1 - 0.5);
    t[1] = log(0.5) + -3.0f + log(1 - 0.9);
    for (size_t i = 2; i < n; i++) t[i] = log(0.9) + -3.0f + t[i - 1];
}

int mt_no_handle(const char *who) {
    if (gab_device_count() <= 0) { gab_set_error("%s: no usable gfx950 device", who); return GAB_ENODEV; }
    gab_set_error("%s: NULL handle", who);
    return GAB_EINVAL;
}

// the CpG groups of a reference (meth.c:532-558): a site starts one when no site lies in the ten bases before it
int32_t mt_groups(const char *ref, int32_t len) {
    int32_t n = 0, prev = -1 - MIN_SEPARATION;
    for (int32_t i = 0; i + 1 < len; i++)
        if (gab_abea_base_code(ref[i]) == 1 && gab_abea_base_code(ref[i + 1]) == 2) { n += i - prev > MIN_SEPARATION; prev = i; }
    return n;
}

}  // namespace

gab_abea_meth_state::~gab_abea_meth_state() {
    cpg.release(); table.release(); flank.release(); io.release(); scratch.release();
    for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v);
}

extern "C" int gab_abea_meth_shape(int32_t *blocks_per_lane, int32_t *one_block_kmers) {
    if (blocks_per_lane) *blocks_per_lane = BPL;
    if (one_block_kmers) *one_block_kmers = ONE_BLOCK_KMERS;
    return GAB_OK;
}

extern "C" int gab_abea_meth_logsum(float *table16000) {
    GAB_CHECK(table16000, "gab_abea_meth_logsum: NULL argument");
    for (int i = 0; i < TBL; i++) table16000[i] = log(1. + exp((double)-i / 1000.f));      // p7_FLogsumInit, logsum.h:44-46
    return GAB_OK;
}

extern "C" int gab_abea_meth_groups(const char *ref, const int64_t *ref_off, const int32_t *ref_len, int64_t n_reads, int32_t *groups) {
    GAB_CHECK(n_reads >= 0, "gab_abea_meth_groups: n_reads %lld out of range", (long long)n_reads);
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(ref_off && ref_len && groups, "gab_abea_meth_groups: NULL argument");
    for (int64_t i = 0; i < n_reads; i++) GAB_CHECK(ref_len[i] >= 0 && ref_off[i] >= 0 && (ref || ref_len[i] == 0), "gab_abea_meth_groups: read %lld: ref_off %lld, ref_len %d", (long long)i, (long long)ref_off[i], ref_len[i]);
    for (int64_t i = 0; i < n_reads; i++) groups[i] = mt_groups(ref + ref_off[i], ref_len[i]);
    return GAB_OK;
}

extern "C" int gab_abea_set_cpg_model(gab_abea *h, const float *level_mean, const float *level_stdv, const float *level_log_stdv) {
    if (!h) return mt_no_handle("gab_abea_set_cpg_model");
    GAB_CHECK(level_mean && level_stdv && level_log_stdv, "gab_abea_set_cpg_model: NULL argument");
    for (int i = 0; i < NK5; i++)
        GAB_CHECK(level_stdv[i] > 0.f && isfinite(level_stdv[i]) && isfinite(level_mean[i]) && isfinite(level_log_stdv[i]),
                  "gab_abea_set_cpg_model: model entry %d: stdv must be positive, mean and log stdv finite", i);
    gab_device_guard g(h->device);
    gab_abea_meth_state &S = h->meth;
    S.have_model = false;
    int rc;
    if (!S.table.p) {                                      // p7_FLogsumInit: once per handle
        std::vector<float> t(TBL);
        if ((rc = gab_abea_meth_logsum(t.data())) != GAB_OK || (rc = S.table.reserve(4 * (size_t)TBL)) != GAB_OK) return rc;
        GAB_HIP(hipMemcpy(S.table.p, t.data(), 4 * (size_t)TBL, hipMemcpyHostToDevice));
    }
    std::vector<float> m(3 * (size_t)NK5);
    memcpy(m.data(), level_mean, 4 * (size_t)NK5); memcpy(m.data() + NK5, level_stdv, 4 * (size_t)NK5); memcpy(m.data() + 2 * NK5, level_log_stdv, 4 * (size_t)NK5);
    if ((rc = S.cpg.reserve(4 * m.size())) != GAB_OK) return rc;
    GAB_HIP(hipMemcpy(S.cpg.p, m.data(), 4 * m.size(), hipMemcpyHostToDevice));
    S.have_model = true;
    return GAB_OK;
}

extern "C" int gab_abea_meth_device(gab_abea *h, const char *ref, int64_t ref_bytes, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_pos,
                                    const uint8_t *is_rev, const uint32_t *cigar, int64_t cigar_count, const int64_t *cigar_off, const int32_t *n_cigar,
                                    const int32_t *seq_len, const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events,
                                    const gab_abea_range *map, int64_t map_count, const int64_t *map_off, const gab_abea_calib *calib, int64_t n_reads,
                                    gab_abea_site *out, int64_t out_count, const int64_t *out_off, gab_abea_meth_read *res, void *stream) {
    if (!h) return mt_no_handle("gab_abea_meth_device");
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_meth_device: n_reads %lld out of range", (long long)n_reads);
    gab_abea_meth_state &S = h->meth;
    mt_reset(S);
    GAB_CHECK(S.have_model, "gab_abea_meth: no CpG model: call gab_abea_set_cpg_model first");
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK((ref || ref_bytes == 0) && ref_off && ref_len && ref_pos && is_rev && (cigar || cigar_count == 0) && cigar_off && n_cigar && seq_len && event_mean &&
              event_off && n_events && map && map_off && calib && (out || out_count == 0) && out_off && res, "gab_abea_meth_device: NULL argument");
    GAB_CHECK(ref_bytes >= 0 && cigar_count >= 0 && event_count >= 0 && map_count >= 0 && out_count >= 0 && out_count <= (int64_t)UINT32_MAX, "gab_abea_meth_device: slab size out of range");
    gab_device_guard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)n_reads;
    for (hipEvent_t &v : S.ev) if (!v) GAB_HIP(hipEventCreate(&v));

    // ---- the lengths, the offsets, the calibration records and every CIGAR come to the host
    std::vector<int64_t> ro(n), co(n), eo(n), mo(n), oo(n); std::vector<int32_t> rl(n), rp(n), nc(n), sl(n), ne(n); std::vector<uint8_t> rv(n);
    std::vector<gab_abea_calib> cal(n); std::vector<uint32_t> cg((size_t)cigar_count);
    GAB_HIP(hipMemcpyAsync(ro.data(), ref_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(co.data(), cigar_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(eo.data(), event_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(mo.data(), map_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(oo.data(), out_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(rl.data(), ref_len, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(rp.data(), ref_pos, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(nc.data(), n_cigar, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(sl.data(), seq_len, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(ne.data(), n_events, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(rv.data(), is_rev, n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(cal.data(), calib, sizeof(gab_abea_calib) * n, hipMemcpyDeviceToHost, s));
    if (cigar_count) GAB_HIP(hipMemcpyAsync(cg.data(), cigar, 4 * (size_t)cigar_count, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));

    // ---- validation, and the run table of every CIGAR (get_aligned_segments, meth.c:15-87, and the trim of meth.c:146-154, by run)
    std::vector<mt_job> jobs(n); std::vector<mt_run> runs;
    int64_t code_total = 0; int32_t max_events = 0;
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(sl[i] >= K && ne[i] >= 1, "gab_abea_meth: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, sl[i], K, ne[i]);
        GAB_CHECK(rl[i] >= 0 && nc[i] >= 0 && rp[i] >= 0, "gab_abea_meth: read %zu: ref_len %d, n_cigar %d, ref_pos %d: none may be negative", i, rl[i], nc[i], rp[i]);
        GAB_CHECK((int64_t)rp[i] + rl[i] + MIN_SEPARATION <= INT32_MAX, "gab_abea_meth: read %zu: ref_pos + ref_len beyond 2^31", i);
        GAB_CHECK(ro[i] >= 0 && ro[i] + rl[i] <= ref_bytes, "gab_abea_meth: read %zu: reference bases [%lld, +%d) outside the slab of %lld bytes", i, (long long)ro[i], rl[i], (long long)ref_bytes);
        GAB_CHECK(co[i] >= 0 && co[i] + nc[i] <= cigar_count, "gab_abea_meth: read %zu: CIGAR operations [%lld, +%d) outside the slab of %lld", i, (long long)co[i], nc[i], (long long)cigar_count);
        GAB_CHECK(eo[i] >= 0 && eo[i] + ne[i] <= event_count, "gab_abea_meth: read %zu: events [%lld, +%d) outside the slab of %lld", i, (long long)eo[i], ne[i], (long long)event_count);
        GAB_CHECK(mo[i] >= 0 && mo[i] + (sl[i] - K + 1) <= map_count, "gab_abea_meth: read %zu: map entries [%lld, +%d) outside the slab of %lld", i, (long long)mo[i], sl[i] - K + 1, (long long)map_count);
        GAB_CHECK(oo[i] >= 0 && oo[i] <= out_count, "gab_abea_meth: read %zu: out_off %lld outside the slab of %lld records", i, (long long)oo[i], (long long)out_count);
        const gab_abea_calib &c = cal[i];
        GAB_CHECK(isfinite(c.scale) && isfinite(c.shift) && isfinite(c.var) && isfinite(c.log_var) && c.var > 0.f,
                  "gab_abea_meth: read %zu: scale %g, shift %g, var %g, log_var %g: finite ones and var > 0 needed", i, c.scale, c.shift, c.var, c.log_var);
        mt_job &J = jobs[i];
        memset(&J, 0, sizeof J);
        J.code_off = code_total; J.ev_off = eo[i]; J.map_off = mo[i]; J.out_off = oo[i]; J.run_off = (int64_t)runs.size();
        J.ref_pos = rp[i]; J.ref_len = rl[i]; J.seq_len = sl[i]; J.n_events = ne[i]; J.is_rev = rv[i] != 0;
        J.state = c.read_stat_flag != 0 ? GAB_ABEA_METH_SKIPPED : !(c.events_per_base >= 1.0) ? GAB_ABEA_METH_TRANSITIONS : 0;
        J.scale = c.scale; J.shift = c.shift; J.var = c.var; J.log_var = c.log_var;
        if (J.state == 0) gab_abea_transitions(c.events_per_base, J.t);
        code_total += rl[i];
        max_events = std::max(max_events, ne[i]);
        int64_t ref_at = rp[i], read_at = 0, pair_at = 0;
        for (int32_t k = 0; k < nc[i]; k++) {
            const uint32_t w = cg[(size_t)co[i] + k], op = w & 15u;
            const int64_t len = w >> 4;
            GAB_CHECK(op <= 8u && op != 6u, "gab_abea_meth: read %zu: CIGAR operation %d has code %u: one of MIDSH=X needed", i, k, op);
            GAB_CHECK(op != 3u, "gab_abea_meth: read %zu: CIGAR operation %d is an N: spliced alignments are not called (meth.c:54-58)", i, k);
            if (op == 0 || op == 7 || op == 8) {           // M = X: the pairs with 6 <= read_pos and read_pos + 6 < seq_len
                const int64_t a = std::max<int64_t>(read_at, K), b = std::min<int64_t>(read_at + len, (int64_t)sl[i] - K);
                if (b > a) { runs.push_back({(int32_t)(ref_at + (a - read_at)), (int32_t)a, (int32_t)(b - a), (int32_t)pair_at}); pair_at += b - a; }
                ref_at += len; read_at += len;
            } else if (op == 2) ref_at += len;             // D
            else if (op == 1 || op == 4) read_at += len;   // I S (H: nothing)
            GAB_CHECK(ref_at - rp[i] <= rl[i], "gab_abea_meth: read %zu: the CIGAR spans more than the %d reference bases given", i, rl[i]);
            GAB_CHECK(read_at <= sl[i], "gab_abea_meth: read %zu: the CIGAR spans more than the read's %d bases", i, sl[i]);
        }
        J.n_runs = (int32_t)(runs.size() - (size_t)J.run_off); J.n_pairs = (int32_t)pair_at;
    }
    {   // a read's room: up to the next larger out_off, or the end of the slab
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return oo[x] < oo[y]; });
        for (size_t t = 0; t < n; t++) jobs[order[t]].room = (t + 1 < n ? oo[order[t + 1]] : out_count) - oo[order[t]];
    }
    GAB_CHECK(runs.size() <= (size_t)INT32_MAX, "gab_abea_meth: more than 2^31 CIGAR runs in one call");

    // ---- the flank table of the longest read, the scratch layout, the two launches
    int rc;
    if (S.flank_len < (int64_t)max_events + 2) {
        std::vector<float> f;
        mt_flank(f, (size_t)max_events + 2);
        GAB_HIP(hipStreamSynchronize(s));                  // (an earlier call on this stream may still read the shorter table)
        if ((rc = S.flank.reserve(4 * f.size())) != GAB_OK) return rc;
        GAB_HIP(hipMemcpy(S.flank.p, f.data(), 4 * f.size(), hipMemcpyHostToDevice));
        S.flank_len = (int64_t)f.size();
    }
    gab_stage_bump a;
    const size_t o_head = a.region(256), o_jobs = a.region(sizeof(mt_job) * n), o_recs = a.region(sizeof(gab_abea_meth_read) * n);
    const size_t o_runs = a.region(sizeof(mt_run) * std::max<size_t>(runs.size(), 1)), o_items = a.region(sizeof(mt_item) * std::max<size_t>((size_t)out_count, 1));
    const size_t o_codes = a.region((size_t)std::max<int64_t>(code_total, 1));
    if ((rc = S.scratch.reserve(a.o)) != GAB_OK) return rc;
    char *b = S.scratch.as<char>();
    mt_head *d_head = (mt_head *)(b + o_head), head = {INT32_MAX, INT32_MAX, 0u, 0u, 0ull};
    mt_job *d_jobs = (mt_job *)(b + o_jobs); gab_abea_meth_read *d_recs = (gab_abea_meth_read *)(b + o_recs);
    mt_run *d_runs = (mt_run *)(b + o_runs); mt_item *d_items = (mt_item *)(b + o_items); uint8_t *d_codes = (uint8_t *)(b + o_codes);
    GAB_HIP(hipMemcpyAsync(d_head, &head, sizeof head, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(mt_job) * n, hipMemcpyHostToDevice, s));
    if (!runs.empty()) GAB_HIP(hipMemcpyAsync(d_runs, runs.data(), sizeof(mt_run) * runs.size(), hipMemcpyHostToDevice, s));

    const mt_reads R = {ref, ref_off, event_mean, map};
    GAB_HIP(hipEventRecord(S.ev[0], s));
    hipLaunchKernelGGL(mt_prep, dim3((unsigned)n), dim3(64), 0, s, R, d_jobs, d_runs, d_codes, d_head, d_items, d_recs);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(S.ev[1], s));
    hipLaunchKernelGGL(mt_score, dim3(SCORE_BLOCKS), dim3(64 * SCORE_WAVES), 0, s, R, d_jobs, d_codes, d_head, d_items, d_recs, (int)n,
                       S.cpg.as<float>(), S.table.as<float>(), S.flank.as<float>(), out, res);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(S.ev[2], s));

    std::vector<gab_abea_meth_read> recs(n);
    GAB_HIP(hipMemcpyAsync(&head, d_head, sizeof head, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(recs.data(), d_recs, sizeof(gab_abea_meth_read) * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    GAB_CHECK(head.bad_read == INT32_MAX, "gab_abea_meth: read %d: a reference byte that is no IUPAC base, an event mean that is not finite, or a map entry outside -1 and [0, n_events)",
              head.bad_read);
    GAB_CHECK(head.short_room_read == INT32_MAX, "gab_abea_meth: read %d: out_off leaves %lld records of room, its %d CpG groups need one each (gab_abea_meth_groups)",
              head.short_room_read, (long long)jobs[(size_t)head.short_room_read].room, recs[(size_t)head.short_room_read].groups);
    GAB_HIP(hipEventElapsedTime(&S.prep_ms, S.ev[0], S.ev[1]));
    GAB_HIP(hipEventElapsedTime(&S.score_ms, S.ev[1], S.ev[2]));
    GAB_HIP(hipEventElapsedTime(&S.total_ms, S.ev[0], S.ev[2]));
    S.reads = n_reads;
    for (size_t i = 0; i < n; i++) { S.groups += recs[i].groups; S.sites += recs[i].n_sites; S.cells += recs[i].cells; }
    S.rows = (int64_t)head.rows;
    return GAB_OK;
}

extern "C" int gab_abea_meth(gab_abea *h, const char *ref, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_pos,
                             const uint8_t *is_rev, const uint32_t *cigar, const int64_t *cigar_off, const int32_t *n_cigar,
                             const int32_t *seq_len, const float *event_mean, const int64_t *event_off, const int32_t *n_events,
                             const gab_abea_range *map, const int64_t *map_off, const gab_abea_calib *calib, int64_t n_reads,
                             gab_abea_site *out, const int64_t *out_off, gab_abea_meth_read *res) {
    if (!h) return mt_no_handle("gab_abea_meth");
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_meth: n_reads %lld out of range", (long long)n_reads);
    mt_reset(h->meth);
    GAB_CHECK(h->meth.have_model, "gab_abea_meth: no CpG model: call gab_abea_set_cpg_model first");
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(ref_off && ref_len && ref_pos && is_rev && cigar_off && n_cigar && seq_len && event_mean && event_off && n_events && map && map_off && calib && out_off && res,
              "gab_abea_meth: NULL argument");
    const size_t n = (size_t)n_reads;
    // the windows of the five slabs that the reads refer to; the device call sees them re-based to the windows' starts
    int64_t ra = INT64_MAX, rb = 0, ca = INT64_MAX, cb = 0, ea = INT64_MAX, eb = 0, ma = INT64_MAX, mb = 0, oa = INT64_MAX, ob = 0;
    std::vector<int64_t> ro(n), co(n), eo(n), mo(n), oo(n); std::vector<int32_t> room(n);
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(seq_len[i] >= K && n_events[i] >= 1, "gab_abea_meth: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, seq_len[i], K, n_events[i]);
        GAB_CHECK(ref_len[i] >= 0 && n_cigar[i] >= 0 && ref_pos[i] >= 0, "gab_abea_meth: read %zu: ref_len %d, n_cigar %d, ref_pos %d: none may be negative", i, ref_len[i], n_cigar[i], ref_pos[i]);
        GAB_CHECK(ref_off[i] >= 0 && cigar_off[i] >= 0 && event_off[i] >= 0 && map_off[i] >= 0 && out_off[i] >= 0, "gab_abea_meth: read %zu: negative offset", i);
        GAB_CHECK((ref || ref_len[i] == 0) && (cigar || n_cigar[i] == 0), "gab_abea_meth: NULL argument");
        room[i] = mt_groups(ref + ref_off[i], ref_len[i]);
        GAB_CHECK(out || room[i] == 0, "gab_abea_meth: NULL argument");
        if (ref_len[i]) { ra = std::min(ra, ref_off[i]); rb = std::max(rb, ref_off[i] + ref_len[i]); }
        if (n_cigar[i]) { ca = std::min(ca, cigar_off[i]); cb = std::max(cb, cigar_off[i] + n_cigar[i]); }
        ea = std::min(ea, event_off[i]); eb = std::max(eb, event_off[i] + n_events[i]);
        ma = std::min(ma, map_off[i]); mb = std::max(mb, map_off[i] + seq_len[i] - K + 1);
        oa = std::min(oa, out_off[i]); ob = std::max(ob, out_off[i] + room[i]);
    }
    if (rb == 0) ra = 0;
    if (cb == 0) ca = 0;
    for (size_t i = 0; i < n; i++) {
        ro[i] = ref_len[i] ? ref_off[i] - ra : 0; co[i] = n_cigar[i] ? cigar_off[i] - ca : 0;
        eo[i] = event_off[i] - ea; mo[i] = map_off[i] - ma; oo[i] = out_off[i] - oa;
    }
    gab_device_guard g(h->device);
    hipStream_t s = nullptr;
    int rc = h->hs.get(&s);
    if (rc) return rc;
    gab_stage_bump a;
    const size_t o_ref = a.region(gab_pad256((size_t)(rb - ra))), o_cg = a.region(4 * (size_t)(cb - ca)), o_ev = a.region(4 * (size_t)(eb - ea));
    const size_t o_map = a.region(sizeof(gab_abea_range) * (size_t)(mb - ma)), o_cal = a.region(sizeof(gab_abea_calib) * n);
    const size_t o_out = a.region(sizeof(gab_abea_site) * (size_t)(ob - oa)), o_res = a.region(sizeof(gab_abea_meth_read) * n);
    const size_t o_ro = a.a8(n), o_co = a.a8(n), o_eo = a.a8(n), o_mo = a.a8(n), o_oo = a.a8(n);
    const size_t o_rl = a.a4(n), o_rp = a.a4(n), o_nc = a.a4(n), o_sl = a.a4(n), o_ne = a.a4(n), o_rv = a.a4((n + 3) / 4);
    if ((rc = h->meth.io.reserve(a.o)) != GAB_OK) return rc;
    char *b = h->meth.io.as<char>();
    {
        std::lock_guard<std::mutex> gate(gab_h2d_mutex(h->device));
        if (rb > ra) GAB_HIP(hipMemcpyAsync(b + o_ref, ref + ra, (size_t)(rb - ra), hipMemcpyHostToDevice, s));
        if (cb > ca) GAB_HIP(hipMemcpyAsync(b + o_cg, cigar + ca, 4 * (size_t)(cb - ca), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_ev, event_mean + ea, 4 * (size_t)(eb - ea), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_map, map + ma, sizeof(gab_abea_range) * (size_t)(mb - ma), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_cal, calib, sizeof(gab_abea_calib) * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_ro, ro.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_co, co.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_eo, eo.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_mo, mo.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_oo, oo.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_rl, ref_len, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_rp, ref_pos, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_nc, n_cigar, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_sl, seq_len, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_ne, n_events, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_rv, is_rev, n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    rc = gab_abea_meth_device(h, b + o_ref, rb - ra, (const int64_t *)(b + o_ro), (const int32_t *)(b + o_rl), (const int32_t *)(b + o_rp), (const uint8_t *)(b + o_rv),
                              (const uint32_t *)(b + o_cg), cb - ca, (const int64_t *)(b + o_co), (const int32_t *)(b + o_nc), (const int32_t *)(b + o_sl),
                              (const float *)(b + o_ev), eb - ea, (const int64_t *)(b + o_eo), (const int32_t *)(b + o_ne),
                              (const gab_abea_range *)(b + o_map), mb - ma, (const int64_t *)(b + o_mo), (const gab_abea_calib *)(b + o_cal), n_reads,
                              (gab_abea_site *)(b + o_out), ob - oa, (const int64_t *)(b + o_oo), (gab_abea_meth_read *)(b + o_res), s);
    if (rc) return rc;
    GAB_HIP(hipMemcpy(res, b + o_res, sizeof(gab_abea_meth_read) * n, hipMemcpyDeviceToHost));
    std::vector<gab_abea_site> all;
    try { all.resize((size_t)(ob - oa)); } catch (...) { gab_set_error("gab_abea_meth: out of host memory"); return GAB_ENOMEM; }
    if (!all.empty()) GAB_HIP(hipMemcpy(all.data(), b + o_out, sizeof(gab_abea_site) * all.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) if (res[i].n_sites > 0) memcpy(out + out_off[i], all.data() + oo[i], sizeof(gab_abea_site) * (size_t)res[i].n_sites);
    return GAB_OK;
}

extern "C" int gab_abea_meth_last_stats(gab_abea *h, int64_t *reads, int64_t *groups, int64_t *sites, int64_t *rows, int64_t *cells, float *kernel_ms, float *total_ms) {
    if (!h) return mt_no_handle("gab_abea_meth_last_stats");
    const gab_abea_meth_state &S = h->meth;
    if (reads) *reads = S.reads;
    if (groups) *groups = S.groups;
    if (sites) *sites = S.sites;
    if (rows) *rows = S.rows;
    if (cells) *cells = S.cells;
    if (kernel_ms) *kernel_ms = S.prep_ms + S.score_ms;
    if (total_ms) *total_ms = S.total_ms;
    return GAB_OK;
}

extern "C" int gab_abea_meth_stage_ms(gab_abea *h, float *prep_ms, float *score_ms) {
    if (!h) return mt_no_handle("gab_abea_meth_stage_ms");
    if (prep_ms) *prep_ms = h->meth.prep_ms;
    if (score_ms) *score_ms = h->meth.score_ms;
    return GAB_OK;
}
