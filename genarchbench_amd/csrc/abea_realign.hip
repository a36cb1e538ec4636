// abea: realign_read (abea/src/eventalign.c:1942-2034) = align_read_to_ref (eventalign.c:1263-1540) around profile_hmm_align
// (eventalign.c:703-911), behind gab_abea_realign* (include/gab.h).  The handle is the one of abea.hip (abea_handle.h).
//
// Arithmetic: the reference's as built without fused multiply-add (the pragma below); the division of the emission is the
// correctly rounded one.  The logarithms of the transitions are taken on the host (rl_transitions).
//
// Shape (DESIGN.md, section "abea: realign"):
//   (host)      lengths, offsets and every CIGAR come to the host and are validated there.  The same walk over a CIGAR that adds up
//               its spans writes its run-length table: one entry per M / = / X operation (reference start, read start, length, index
//               of its first pair) and the first run of every segment that an N operation opens.  No pair is ever expanded: get_end_pair,
//               the two trims and pair -> (reference, read) position are binary searches in that table (rl_first_gt, rl_pair).
//   rl_prep     one block per read.  Checks what only the device holds (reference bytes, event means, map entries) and writes
//               nothing but the lowest read that breaks a rule; upper-cases, disambiguates and ranks the reference: per reference
//               position the rank of its 6-mer and of that 6-mer's reverse complement, 16 bits each.
//   rl_viterbi  one wavefront per read, the reads of a launch dealt round-robin to the wavefronts.  A read is a serial chain of HMM
//               segments (each starts at the last entry the one before it emitted), so nothing of a read runs beside itself.  The
//               lanes own two k-mer blocks each (at most 96 k-mers: 48 lanes busy); the previous row's M, B and K of both blocks
//               stay in registers, the left neighbour's come by one lane shift.  Per row: two emissions, six update_cells, the
//               skip-state fixed point (below), one dword of backpointers per lane into the wave's trace (256 B a row, coalesced).
//               The backtrack reads the trace back eight rows at a time, all lanes loading, and walks it with lane reads, wave-
//               uniform; it leaves per row the k-mer and state of the row's entry, from which the lanes write the emitted entries
//               in parallel.  A segment with more rows than the trace holds stops the read there with its state saved.
//   (host)      the states come to the host: reads that stopped are launched once more, each with a trace of n_events rows (no
//               segment has more), in batches under a memory budget.
//
// The skip state is the only dependence inside a row: K[b] = max(mk + M[b-1], bk + B[b-1], fl(kk + K[b-1])), the maximum as
// update_cell takes it (start from -inf, replace on `>`: a NaN candidate never replaces anything, it counts as absent; the result
// is never a NaN).  Write a[b] for the maximum of the first two.  x -> fl(kk + x) is monotone and max is exact, so the serial loop
// computes the least K with K[b] = max(a[b], fl(kk + K[b-1])), and that system has one solution only (K[b] depends on K[b-1]
// alone, block 0 is -inf).  Here the lanes start from K = a, which lies below the solution, and apply K <- max(K, fl(kk + shift(K)))
// (in lane order for a lane's own two blocks) until a wave vote sees no change: every iterate stays below the solution by
// monotonicity, and an unchanged iterate satisfies the system, so it is the solution, bit for bit.  (b-1-j) * kk in one
// multiplication would not be: it rounds once where the loop rounds b-1-j times.  The `from` of a K cell is then taken from the
// final neighbour values by the literal rule.
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
constexpr int ROWS = GAB_ABEA_REALIGN_ROWS;
constexpr int ALIGN_STRIDE = 100, OUTPUT_STRIDE = 50;      // eventalign.c:1341-1342
constexpr int MAX_KMERS = ALIGN_STRIDE + 1 - K + 1;         // 96: a sub-sequence has at most 101 bases
constexpr int WAVES = 1024;                                 // wavefronts of the first launch: one per SIMD of 256 CUs
constexpr size_t REQUEUE_BYTES = (size_t)512 << 20;         // trace budget of one requeue launch
static_assert(sizeof(gab_abea_ealn) == 12 && sizeof(gab_abea_realign_read) == 24 && sizeof(gab_abea_calib) == 40, "record layout");
static_assert(MAX_KMERS <= 128, "two blocks per lane");

struct rl_run { int32_t ref, read, len, pair; };           // an M / = / X operation: its first pair, its length, that pair's index in the read
struct rl_job {                                            // one read, as the host planned it
    int64_t rk_off, ev_off, map_off, out_off, run_off, seg_off, room;
    int32_t ref_pos, ref_len, seq_len, n_events, n_seg, is_rev, skipped, pad;
    float t[11];                                           // mm_self mm_next bm_self bm_next km soft | mb bb | mk bk kk
    float scale, shift, var, log_var, pad2;
};
struct rl_state {                                          // where a read stands between two launches
    int32_t seg, mid, cur_ev, cur_ref, cur_pair, last_ev, forward, plo, phi, n_out, hmm_segments, max_rows;
    uint32_t flags; int32_t done, need_rows, pad;
    int64_t cells, rows;
};
struct rl_item { int32_t read, cap; int64_t trace_off; };  // one read of a launch: its trace (dwords from the launch's base) and rows
struct rl_verdict { int32_t bad_read, pad; };
struct rl_reads {                                          // the call's per-read arrays (device pointers)
    const char *ref; const int64_t *ref_off; const int32_t *ref_len;
    const float *event_mean; const int64_t *event_off; const int32_t *n_events;
    const gab_abea_range *map; const int64_t *map_off; const int32_t *seq_len;
};

__global__ __launch_bounds__(256) void rl_prep(rl_reads R, const rl_job *jobs, uint32_t *rk, rl_verdict *verdict) {
    const int r = blockIdx.x;
    const rl_job J = jobs[r];
    const char *ref = R.ref + R.ref_off[r];
    bool bad = false;
    for (int p = threadIdx.x; p < J.ref_len; p += 256) {
        uint32_t f = 0, c = 0;
        for (int t = 0; t < K; t++) {
            const int b = p + t < J.ref_len ? gab_abea_base_code(ref[p + t]) : 0;
            bad |= b < 0;
            f = (f << 2) | (uint32_t)(b & 3);
            c |= (uint32_t)(3 - (b & 3)) << (2 * t);       // the reverse complement's base K-1-t is the complement of base t
        }
        if (p + K <= J.ref_len) rk[J.rk_off + p] = f | (c << 16);
    }
    const float *ev = R.event_mean + J.ev_off;
    for (int i = threadIdx.x; i < J.n_events; i += 256) bad |= !isfinite(ev[i]);
    const gab_abea_range *m = R.map + J.map_off;
    for (int i = threadIdx.x; i < J.seq_len - K + 1; i += 256) {
        const gab_abea_range g = m[i];
        bad |= g.start < -1 || g.start >= J.n_events || g.stop < -1 || g.stop >= J.n_events;
    }
    if (bad) atomicMin(&verdict->bad_read, r);
}

// ---- the run-length table -------------------------------------------------------------------------------------------------------------
// the index of the first pair of the runs [r0, r1) (one segment, r0 < r1) whose reference (REF) or read position is above x
template <bool REF> __device__ __forceinline__ int rl_first_gt(const rl_run *ru, int r0, int r1, int64_t x) {
    int lo = r0, hi = r1;                                  // -> the first run that starts above x
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((REF ? ru[mid].ref : ru[mid].read) <= x) lo = mid + 1; else hi = mid;
    }
    if (lo == r0) return ru[r0].pair;
    const rl_run q = ru[lo - 1];
    const int64_t d = x - (REF ? q.ref : q.read) + 1;      // >= 1 pairs of q at or below x
    return q.pair + (d < q.len ? (int)d : q.len);
}
__device__ __forceinline__ void rl_pair(const rl_run *ru, int r0, int r1, int i, int *ref, int *read) {
    int lo = r0, hi = r1;                                  // -> the first run whose pairs start above i
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (ru[mid].pair <= i) lo = mid + 1; else hi = mid;
    }
    const rl_run q = ru[lo > r0 ? lo - 1 : r0];
    *ref = q.ref + (i - q.pair); *read = q.read + (i - q.pair);
}
// get_end_pair (eventalign.c:919-928) over the pairs [.., phi): the reference positions rise strictly, so the scan from pair_idx ends
// at the last pair at or below ref_max, or at pair_idx - 1 when pair_idx itself is above it
__device__ __forceinline__ int rl_end_pair(const rl_run *ru, int r0, int r1, int phi, int ref_max, int pair_idx) {
    int e = rl_first_gt<true>(ru, r0, r1, (int64_t)ref_max) - 1;
    e = e < phi - 1 ? e : phi - 1;
    return e > pair_idx - 1 ? e : pair_idx - 1;
}

// get_next_event (eventalign.c:962-972): start, start + stride, .. up to but without stop, 64 entries at a time
__device__ __forceinline__ int rl_next_event(const gab_abea_range *m, int start, int stop, int stride, int lane) {
    const int n = stop > start ? stop - start : start - stop;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const int ei = i < n ? m[start + i * stride].start : -1;
        const unsigned long long hit = __ballot(ei != -1);
        if (hit) return __builtin_amdgcn_readlane(ei, __builtin_ctzll(hit));
    }
    return -1;
}
__device__ __forceinline__ int rl_closest_event(const gab_abea_range *m, int k_idx, int size, int lane) {      // eventalign.c:975-987
    const int before = rl_next_event(m, k_idx, max(0, k_idx - 1000), -1, lane);
    if (before != -1) return before;
    return rl_next_event(m, k_idx, min(k_idx + 1000, size - 1), 1, lane);
}

// update_cell (eventalign.c:621-633), written as it stands
__device__ __forceinline__ float rl_cell(float s0, float s1, float s2, float s3, float s4, float s5, float emission, uint32_t *from) {
    float mx = s0; uint32_t f = 0;
    mx = s1 > mx ? s1 : mx; f = mx == s1 ? 1u : f;
    mx = s2 > mx ? s2 : mx; f = mx == s2 ? 2u : f;
    mx = s3 > mx ? s3 : mx; f = mx == s3 ? 3u : f;
    mx = s4 > mx ? s4 : mx; f = mx == s4 ? 4u : f;
    mx = s5 > mx ? s5 : mx; f = mx == s5 ? 5u : f;
    *from = f;
    return mx + emission;
}
__device__ __forceinline__ float rl_up(float v, int lane) {      // the left neighbour lane's v; block 0 (left of lane 0) is -inf
    const float t = __shfl_up(v, 1);
    return lane == 0 ? -INFINITY : t;
}
__device__ __forceinline__ float rl_emission(float x, float gp_mean, float gp_stdv, float c) {      // log_normal_pdf, eventalign.c:293-300
    const float a = (x - gp_mean) / gp_stdv;
    return c + ((-0.5f * a) * a);
}

// profile_hmm_fill_generic_r9 (eventalign.c:345-610) with hmm_flags = 0: rows 1 .. n_rows of the matrix, the backpointers of row r to
// trace[(r - 1) * 64 + lane]: block 2 * lane + 1 in the low half, 2 * lane + 2 in the high half, 3 bits a state at 3 * state (K, B, M)
__device__ __forceinline__ void rl_fill(const rl_job &J, const float *model, const uint32_t *rk, const float *ev, int e_start, int stride, int n_rows,
                                        int s, int n_kmers, uint32_t *trace, int lane) {
    const float NI = -INFINITY;
    float mean[2], sd[2], c[2];
    for (int t = 0; t < 2; t++) {
        const int k = 2 * lane + t;
        uint32_t rank = 0;
        if (k < n_kmers) { const uint32_t w = rk[s + k]; rank = J.is_rev ? w >> 16 : w & 0xffffu; }
        mean[t] = J.scale * model[rank] + J.shift;         // log_probability_match_r9, eventalign.c:320-330
        sd[t] = model[GAB_ABEA_NKMER + rank] * J.var;
        const float lsd = model[2 * GAB_ABEA_NKMER + rank] + J.log_var;
        c[t] = -0.918938f - lsd;
    }
    const float mmS = J.t[0], mmN = J.t[1], bmS = J.t[2], bmN = J.t[3], km = J.t[4], soft = J.t[5], mb = J.t[6], bb = J.t[7], mk = J.t[8], bk = J.t[9], kk = J.t[10];
    float M0 = NI, B0 = NI, K0 = NI, M1 = NI, B1 = NI;      // row 0 (the second block's K lives on as the right neighbour's pK)
    float pM = NI, pB = NI, pK = NI;                       // the left neighbour's second block, previous row
    for (int base = 0; base < n_rows; base += 64) {
        const int mine = base + lane;
        const float evv = mine < n_rows ? ev[e_start + mine * stride] : 0.f;
        const int top = min(64, n_rows - base);
        for (int j = 0; j < top; j++) {
            const int row = base + j + 1;
            const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(evv), j));
            uint32_t fm0, fb0, fk0, fm1, fb1, fk1;
            const float s5 = (lane == 0 && row == 1) ? soft : NI;      // event_idx == e_start on row 1 alone
            const float nM0 = rl_cell(mmS + M0, mmN + pM, bmS + B0, bmN + pB, km + pK, s5, rl_emission(x, mean[0], sd[0], c[0]), &fm0);
            const float nB0 = rl_cell(mb + M0, NI, bb + B0, NI, NI, NI, 0.0f, &fb0);
            const float nM1 = rl_cell(mmS + M1, mmN + M0, bmS + B1, bmN + B0, km + K0, NI, rl_emission(x, mean[1], sd[1], c[1]), &fm1);
            const float nB1 = rl_cell(mb + M1, NI, bb + B1, NI, NI, NI, 0.0f, &fb1);
            // the skip state of this row: see the head of the file
            pM = rl_up(nM1, lane); pB = rl_up(nB1, lane);
            const float a0m = mk + pM, a0b = bk + pB, a1m = mk + nM0, a1b = bk + nB0;
            float k0 = NI, k1 = NI;
            k0 = a0m > k0 ? a0m : k0; k0 = a0b > k0 ? a0b : k0;
            k1 = a1m > k1 ? a1m : k1; k1 = a1b > k1 ? a1b : k1;
            { const float t = kk + k0; k1 = t > k1 ? t : k1; }
            for (;;) {
                pK = rl_up(k1, lane);
                float t = kk + pK;
                const float n0 = t > k0 ? t : k0;
                t = kk + n0;
                const float n1 = t > k1 ? t : k1;
                const bool changed = n0 != k0 || n1 != k1;
                k0 = n0; k1 = n1;
                if (!__any(changed)) break;
            }
            const float nK0 = rl_cell(NI, a0m, NI, a0b, kk + pK, NI, 0.0f, &fk0);
            const float nK1 = rl_cell(NI, a1m, NI, a1b, kk + nK0, NI, 0.0f, &fk1);
            trace[(size_t)(row - 1) * 64 + lane] = (fk0 | fb0 << 3 | fm0 << 6) | (fk1 | fb1 << 3 | fm1 << 6) << 16;
            M0 = nM0; B0 = nB0; K0 = nK0; M1 = nM1; B1 = nB1;
            pK = rl_up(nK1, lane);
        }
    }
}

// The backtrack of profile_hmm_align (eventalign.c:809-886) from (last row, last k-mer, M).  Every row has at most one entry that is
// not a K: info[row] = its k-mer | 'B' << 8.  -> the lowest row that has one (the rows from there to n_rows all do), n_rows + 1 if none.
__device__ __forceinline__ int rl_backtrack(const uint32_t *trace, uint32_t *info, int n_rows, int n_kmers, int lane) {
    int kmer = n_kmers - 1, st = 2, low = n_rows + 1;
    bool stop = false;
    for (int base = n_rows; base > 0 && !stop; base -= 8) {
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = base - j >= 1 ? trace[(size_t)(base - j - 1) * 64 + lane] : 0u;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int row = base - j;
            if (row < 1 || stop) continue;
            for (;;) {                                     // the entries of this row: K states, then the one that consumes it
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)v[j], kmer >> 1);
                const uint32_t from = (w >> ((kmer & 1) * 16 + 3 * st)) & 7u;
                if (st != 0) { if (lane == 0) info[row] = (uint32_t)kmer | (st == 1 ? 256u : 0u); low = row; }
                if (from >= 5u) { stop = true; break; }    // HMT_FROM_SOFT
                const int cur = st;
                st = from == 4u ? 0 : from >= 2u ? 1 : 2;
                if (from & 1u || from == 4u) kmer -= 1;    // the three FROM_PREV movements
                if (kmer < 0 || (cur == 0 && from != 4u && !(from & 1u))) { stop = true; break; }      // block 0, a K cell that stays: no score leads there
                if (cur != 0) break;
            }
        }
    }
    return low;
}

__global__ __launch_bounds__(64) void rl_viterbi(rl_reads R, const rl_job *jobs, rl_state *states, const rl_item *items, int n_items, const rl_run *runs,
                                                 const int32_t *segs, const uint32_t *rk, const float *model, uint32_t *traces, const rl_verdict *verdict,
                                                 int32_t region_start, int32_t region_end, gab_abea_ealn *out, gab_abea_realign_read *res) {
    if (verdict->bad_read != INT32_MAX) return;            // an input rule is broken: the call writes nothing
    const int lane = threadIdx.x;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const rl_item I = items[it];
        const rl_job &J = jobs[I.read];
        rl_state S = states[I.read];
        uint32_t *trace = traces + I.trace_off, *info = trace + (size_t)I.cap * 64;      // info[1 .. cap]
        const rl_run *ru = runs + J.run_off;
        const int32_t *sg = segs + J.seg_off;
        const gab_abea_range *map = R.map + J.map_off;
        const float *ev = R.event_mean + J.ev_off;
        gab_abea_ealn *o = out + J.out_off;
        const int n_map = J.seq_len - K + 1;
        S.need_rows = 0;
        if (J.skipped) { S.flags = GAB_ABEA_REALIGN_SKIPPED; S.done = 1; }
        while (!S.done && S.seg < J.n_seg) {
            const int r0 = sg[S.seg], r1 = sg[S.seg + 1];
            if (!S.mid) {                                  // eventalign.c:1326-1361
                int plo = 0, phi = 0;
                if (r0 < r1) {
                    plo = ru[r0].pair; phi = ru[r1 - 1].pair + ru[r1 - 1].len;
                    if (region_start != -1 && region_end != -1) {
                        plo = max(plo, rl_first_gt<true>(ru, r0, r1, (int64_t)region_start - 1));
                        phi = min(phi, rl_first_gt<true>(ru, r0, r1, (int64_t)region_end));
                    }
                    phi = min(phi, rl_first_gt<false>(ru, r0, r1, (int64_t)J.seq_len - K));
                }
                if (phi <= plo) { S.flags |= GAB_ABEA_REALIGN_NO_PAIRS; S.done = 1; break; }
                int ref_a, read_a, ref_b, read_b;
                rl_pair(ru, r0, r1, plo, &ref_a, &read_a); rl_pair(ru, r0, r1, phi - 1, &ref_b, &read_b);
                if (J.is_rev) { read_a = J.seq_len - read_a - K; read_b = J.seq_len - read_b - K; }
                const int first = rl_closest_event(map, read_a, n_map, lane), last = rl_closest_event(map, read_b, n_map, lane);
                if (first < 0 || last < 0) { S.flags |= GAB_ABEA_REALIGN_NO_EVENT; S.done = 1; break; }
                S.forward = first < last; S.cur_ev = first; S.last_ev = last; S.cur_ref = ref_a; S.cur_pair = plo; S.plo = plo; S.phi = phi;
                S.mid = 1;
            }
            while (S.forward ? S.cur_ev < S.last_ev : S.cur_ev > S.last_ev) {      // eventalign.c:1373-1534
                const int end_pair = rl_end_pair(ru, r0, r1, S.phi, S.cur_ref + ALIGN_STRIDE, S.cur_pair);
                int end_ref, end_read;
                rl_pair(ru, r0, r1, end_pair, &end_ref, &end_read);
                if (J.is_rev) end_read = J.seq_len - end_read - K;
                const int s = S.cur_ref - J.ref_pos, l = end_ref - S.cur_ref + 1;
                if (l < 2 * K) break;
                if (l > ALIGN_STRIDE + 1 || s < 0 || s + l > J.ref_len || end_read < 0 || end_read >= n_map) { S.done = 1; break; }      // cannot happen; never index past a buffer
                const int stop_ev = rl_closest_event(map, end_read, n_map, lane);
                if (stop_ev < 0) { S.flags |= GAB_ABEA_REALIGN_NO_EVENT; S.done = 1; break; }
                const int span = S.cur_ev > stop_ev ? S.cur_ev - stop_ev : stop_ev - S.cur_ev;
                if (span < 2) break;
                const int stride = S.cur_ev < stop_ev ? 1 : -1;
                if ((J.is_rev != 0) != (stride == -1)) { S.flags |= GAB_ABEA_REALIGN_STRAND; S.done = 1; break; }
                const int n_rows = span + 1, n_kmers = l - K + 1;
                if (n_rows > I.cap) { S.need_rows = n_rows; break; }
                rl_fill(J, model, rk + J.rk_off, ev, S.cur_ev, stride, n_rows, s, n_kmers, trace, lane);
                __threadfence();
                const int low = rl_backtrack(trace, info, n_rows, n_kmers, lane);
                __threadfence();
                S.hmm_segments += 1; S.rows += n_rows; S.cells += (int64_t)n_rows * n_kmers; S.max_rows = max(S.max_rows, n_rows);
                // eventalign.c:1452-1517: the entries in order, K states and the start event's (row 1) left out; the first 50, or all of the last section
                const int first_row = max(low, 2), emittable = max(n_rows - first_row + 1, 0);
                const bool last_section = end_pair == S.phi - 1;
                const int n_emit = last_section ? emittable : min(emittable, OUTPUT_STRIDE);
                if (n_emit == 0 || S.n_out + (int64_t)n_emit > J.room) { if (n_emit) S.done = 1; break; }
                for (int t = lane; t < n_emit; t += 64) {
                    const int row = first_row + t;
                    const uint32_t w = info[row];
                    gab_abea_ealn e;
                    e.ref_position = S.cur_ref + (int)(w & 255u); e.event_idx = S.cur_ev + (row - 1) * stride; e.hmm_state = w & 256u ? 'B' : 'M';
                    e.pad[0] = e.pad[1] = e.pad[2] = 0;
                    o[S.n_out + t] = e;
                }
                const int last_row = first_row + n_emit - 1;
                S.n_out += n_emit;
                S.cur_ref += (int)(info[last_row] & 255u);
                S.cur_ev += (last_row - 1) * stride;
                S.cur_pair = rl_end_pair(ru, r0, r1, S.phi, S.cur_ref, S.cur_pair);
            }
            if (S.done || S.need_rows) break;
            S.seg += 1; S.mid = 0;
        }
        if (!S.need_rows) S.done = 1;
        if (lane == 0) {
            states[I.read] = S;
            gab_abea_realign_read q;
            q.n_entries = S.n_out; q.hmm_segments = S.hmm_segments; q.max_rows = S.max_rows; q.flags = S.flags; q.cells = S.cells;
            res[I.read] = q;
        }
    }
}

void rl_reset(gab_abea_realign_state &S) {
    S.reads = S.hmm_segments = S.rows = S.cells = S.reads_requeued = 0;
    S.prep_ms = S.viterbi_ms = S.requeue_ms = S.total_ms = 0.f;
}

}  // namespace

gab_abea_realign_state::~gab_abea_realign_state() {
    io.release(); scratch.release(); trace.release();
    for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v);
}

extern "C" int gab_abea_realign_shape(int32_t *rows_cap) {
    if (rows_cap) *rows_cap = ROWS;
    return GAB_OK;
}

static int rl_no_handle(const char *who) {
    if (gab_device_count() <= 0) { gab_set_error("%s: no usable gfx950 device", who); return GAB_ENODEV; }
    gab_set_error("%s: NULL handle", who);
    return GAB_EINVAL;
}

extern "C" int gab_abea_realign_device(gab_abea *h, const char *ref, int64_t ref_bytes, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_pos,
                                       const uint8_t *is_rev, const uint32_t *cigar, int64_t cigar_count, const int64_t *cigar_off, const int32_t *n_cigar,
                                       const int32_t *seq_len, const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events,
                                       const gab_abea_range *map, int64_t map_count, const int64_t *map_off, const gab_abea_calib *calib,
                                       int32_t region_start, int32_t region_end, int64_t n_reads,
                                       gab_abea_ealn *out, int64_t out_count, const int64_t *out_off, gab_abea_realign_read *res, void *stream) {
    if (!h) return rl_no_handle("gab_abea_realign_device");
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_realign_device: n_reads %lld out of range", (long long)n_reads);
    gab_abea_realign_state &S = h->realign;
    rl_reset(S);
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK((ref || ref_bytes == 0) && ref_off && ref_len && ref_pos && is_rev && (cigar || cigar_count == 0) && cigar_off && n_cigar && seq_len && event_mean &&
              event_off && n_events && map && map_off && calib && (out || out_count == 0) && out_off && res, "gab_abea_realign_device: NULL argument");
    GAB_CHECK(ref_bytes >= 0 && cigar_count >= 0 && event_count >= 0 && map_count >= 0 && out_count >= 0, "gab_abea_realign_device: negative slab size");
    GAB_CHECK((region_start == -1 && region_end == -1) || region_start <= region_end, "gab_abea_realign: region [%d, %d]: -1 / -1 or start <= end (eventalign.c:1275)", region_start, region_end);
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

    // ---- validation, and the run-length table of every CIGAR (get_aligned_segments_two_params, eventalign.c:1112-1179, by run)
    std::vector<rl_job> jobs(n); std::vector<rl_run> runs; std::vector<int32_t> segs;
    int64_t rk_total = 0;
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(sl[i] >= K && ne[i] >= 1, "gab_abea_realign: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, sl[i], K, ne[i]);
        GAB_CHECK(rl[i] >= 0 && nc[i] >= 0 && rp[i] >= 0, "gab_abea_realign: read %zu: ref_len %d, n_cigar %d, ref_pos %d: none may be negative", i, rl[i], nc[i], rp[i]);
        GAB_CHECK((int64_t)rp[i] + rl[i] + ALIGN_STRIDE <= INT32_MAX, "gab_abea_realign: read %zu: ref_pos + ref_len beyond 2^31", i);
        GAB_CHECK(ro[i] >= 0 && ro[i] + rl[i] <= ref_bytes, "gab_abea_realign: read %zu: reference bases [%lld, +%d) outside the slab of %lld bytes", i, (long long)ro[i], rl[i], (long long)ref_bytes);
        GAB_CHECK(co[i] >= 0 && co[i] + nc[i] <= cigar_count, "gab_abea_realign: read %zu: CIGAR operations [%lld, +%d) outside the slab of %lld", i, (long long)co[i], nc[i], (long long)cigar_count);
        GAB_CHECK(eo[i] >= 0 && eo[i] + ne[i] <= event_count, "gab_abea_realign: read %zu: events [%lld, +%d) outside the slab of %lld", i, (long long)eo[i], ne[i], (long long)event_count);
        GAB_CHECK(mo[i] >= 0 && mo[i] + (sl[i] - K + 1) <= map_count, "gab_abea_realign: read %zu: map entries [%lld, +%d) outside the slab of %lld", i, (long long)mo[i], sl[i] - K + 1, (long long)map_count);
        const gab_abea_calib &c = cal[i];
        GAB_CHECK(isfinite(c.scale) && isfinite(c.shift) && isfinite(c.var) && isfinite(c.log_var) && c.var > 0.f,
                  "gab_abea_realign: read %zu: scale %g, shift %g, var %g, log_var %g: finite ones and var > 0 needed", i, c.scale, c.shift, c.var, c.log_var);
        rl_job &J = jobs[i];
        memset(&J, 0, sizeof J);
        J.rk_off = rk_total; J.ev_off = eo[i]; J.map_off = mo[i]; J.out_off = oo[i]; J.run_off = (int64_t)runs.size(); J.seg_off = (int64_t)segs.size();
        J.ref_pos = rp[i]; J.ref_len = rl[i]; J.seq_len = sl[i]; J.n_events = ne[i]; J.is_rev = rv[i] != 0; J.skipped = c.read_stat_flag != 0;
        J.scale = c.scale; J.shift = c.shift; J.var = c.var; J.log_var = c.log_var;
        gab_abea_transitions(c.events_per_base, J.t);
        rk_total += std::max(rl[i] - K + 1, 0);
        int64_t ref_at = rp[i], read_at = 0, pair_at = 0, n_skip = 0;
        segs.push_back((int32_t)(runs.size() - (size_t)J.run_off));
        for (int32_t k = 0; k < nc[i]; k++) {
            const uint32_t w = cg[(size_t)co[i] + k], op = w & 15u;
            const int64_t len = w >> 4;
            GAB_CHECK(op <= 8u && op != 6u, "gab_abea_realign: read %zu: CIGAR operation %d has code %u: one of MIDNSH=X needed", i, k, op);
            if (op == 0 || op == 7 || op == 8) {           // M = X
                if (len) runs.push_back({(int32_t)ref_at, (int32_t)read_at, (int32_t)len, (int32_t)pair_at});
                ref_at += len; read_at += len; pair_at += len;
            } else if (op == 2) ref_at += len;             // D
            else if (op == 3) {                            // N: the segment ends, and the next one begins, before its reference bases
                segs.push_back((int32_t)(runs.size() - (size_t)J.run_off));
                ref_at += len; n_skip++;
            } else if (op == 1 || op == 4) read_at += len; // I S (H: nothing)
            GAB_CHECK(ref_at - rp[i] <= rl[i], "gab_abea_realign: read %zu: the CIGAR spans more than the %d reference bases given", i, rl[i]);
            GAB_CHECK(read_at <= sl[i], "gab_abea_realign: read %zu: the CIGAR spans more than the read's %d bases", i, sl[i]);
        }
        segs.push_back((int32_t)(runs.size() - (size_t)J.run_off));
        J.n_seg = (int32_t)n_skip + 1;
        J.room = (int64_t)ne[i] * (1 + n_skip);
        GAB_CHECK(oo[i] >= 0 && oo[i] + J.room <= out_count, "gab_abea_realign: read %zu: entries [%lld, +%lld = n_events * (1 + N operations)) outside the slab of %lld", i,
                  (long long)oo[i], (long long)J.room, (long long)out_count);
    }
    // the room of the entries: regions that overlap leave a read less than n_events * (1 + N operations) of its own
    {
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return oo[x] < oo[y]; });
        for (size_t t = 0; t + 1 < n; t++) {
            const size_t i = order[t], j = order[t + 1];
            GAB_CHECK(oo[i] + jobs[i].room <= oo[j], "gab_abea_realign: read %zu: out_off leaves %lld entries of room, n_events * (1 + N operations) = %lld needed", i,
                      (long long)(oo[j] - oo[i]), (long long)jobs[i].room);
        }
    }
    GAB_CHECK(runs.size() <= (size_t)INT32_MAX && segs.size() <= (size_t)INT32_MAX, "gab_abea_realign: more than 2^31 CIGAR runs in one call");

    // ---- the scratch layout and the first launch
    const int waves = (int)std::min<size_t>(n, WAVES);
    const size_t wave_dwords = (size_t)ROWS * 64 + ROWS + 1;
    gab_stage_bump a;
    const size_t o_verdict = a.region(256), o_jobs = a.region(sizeof(rl_job) * n), o_states = a.region(sizeof(rl_state) * n), o_items = a.region(sizeof(rl_item) * n);
    const size_t o_runs = a.region(sizeof(rl_run) * std::max<size_t>(runs.size(), 1)), o_segs = a.region(4 * segs.size()), o_rk = a.region(4 * (size_t)std::max<int64_t>(rk_total, 1));
    int rc = S.scratch.reserve(a.o);
    if (rc) return rc;
    if ((rc = S.trace.reserve(4 * wave_dwords * (size_t)waves)) != GAB_OK) return rc;
    char *b = S.scratch.as<char>();
    rl_verdict *d_verdict = (rl_verdict *)(b + o_verdict), verdict = {INT32_MAX, 0};
    rl_job *d_jobs = (rl_job *)(b + o_jobs); rl_state *d_states = (rl_state *)(b + o_states); rl_item *d_items = (rl_item *)(b + o_items);
    rl_run *d_runs = (rl_run *)(b + o_runs); int32_t *d_segs = (int32_t *)(b + o_segs); uint32_t *d_rk = (uint32_t *)(b + o_rk);
    std::vector<rl_item> items(n);
    for (size_t i = 0; i < n; i++) items[i] = {(int32_t)i, ROWS, (int64_t)(wave_dwords * (i % (size_t)waves))};
    GAB_HIP(hipMemcpyAsync(d_verdict, &verdict, sizeof verdict, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(rl_job) * n, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(rl_item) * n, hipMemcpyHostToDevice, s));
    if (!runs.empty()) GAB_HIP(hipMemcpyAsync(d_runs, runs.data(), sizeof(rl_run) * runs.size(), hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(d_segs, segs.data(), 4 * segs.size(), hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemsetAsync(d_states, 0, sizeof(rl_state) * n, s));

    const rl_reads R = {ref, ref_off, ref_len, event_mean, event_off, n_events, map, map_off, seq_len};
    const float *model = h->model.as<float>();
    GAB_HIP(hipEventRecord(S.ev[0], s));
    hipLaunchKernelGGL(rl_prep, dim3((unsigned)n), dim3(256), 0, s, R, d_jobs, d_rk, d_verdict);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(S.ev[1], s));
    hipLaunchKernelGGL(rl_viterbi, dim3((unsigned)waves), dim3(64), 0, s, R, d_jobs, d_states, d_items, (int)n, d_runs, d_segs, d_rk, model, S.trace.as<uint32_t>(), d_verdict,
                       region_start, region_end, out, res);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(S.ev[2], s));

    // ---- the requeue decision
    std::vector<rl_state> st(n);
    GAB_HIP(hipMemcpyAsync(&verdict, d_verdict, sizeof verdict, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(st.data(), d_states, sizeof(rl_state) * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    GAB_CHECK(verdict.bad_read == INT32_MAX, "gab_abea_realign: read %d: a reference byte that is no IUPAC base, an event mean that is not finite, or a map entry outside -1 and [0, n_events)",
              verdict.bad_read);
    std::vector<size_t> pending;
    for (size_t i = 0; i < n; i++) if (!st[i].done) pending.push_back(i);
    S.reads_requeued = (int64_t)pending.size();
    for (size_t at = 0; at < pending.size();) {            // a trace of n_events rows each: no segment of the read has more
        size_t dwords = 0, k = 0;
        while (at + k < pending.size()) {
            const size_t need = (size_t)ne[pending[at + k]] * 65 + 1;
            if (k && 4 * (dwords + need) > REQUEUE_BYTES) break;
            items[k] = {(int32_t)pending[at + k], ne[pending[at + k]], (int64_t)dwords};
            dwords += need; k++;
        }
        if ((rc = S.trace.reserve(4 * dwords)) != GAB_OK) return rc;      // (the stream is idle: the states have just come back)
        GAB_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(rl_item) * k, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(rl_viterbi, dim3((unsigned)k), dim3(64), 0, s, R, d_jobs, d_states, d_items, (int)k, d_runs, d_segs, d_rk, model, S.trace.as<uint32_t>(), d_verdict,
                           region_start, region_end, out, res);
        GAB_HIP(hipGetLastError());
        GAB_HIP(hipStreamSynchronize(s));                  // items and the trace are reused by the next batch
        at += k;
    }
    GAB_HIP(hipEventRecord(S.ev[3], s));
    GAB_HIP(hipMemcpyAsync(st.data(), d_states, sizeof(rl_state) * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    GAB_HIP(hipEventElapsedTime(&S.prep_ms, S.ev[0], S.ev[1]));
    GAB_HIP(hipEventElapsedTime(&S.viterbi_ms, S.ev[1], S.ev[2]));
    GAB_HIP(hipEventElapsedTime(&S.requeue_ms, S.ev[2], S.ev[3]));
    GAB_HIP(hipEventElapsedTime(&S.total_ms, S.ev[0], S.ev[3]));
    S.reads = n_reads;
    for (size_t i = 0; i < n; i++) { S.hmm_segments += st[i].hmm_segments; S.rows += st[i].rows; S.cells += st[i].cells; }
    return GAB_OK;
}

extern "C" int gab_abea_realign(gab_abea *h, const char *ref, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_pos,
                                const uint8_t *is_rev, const uint32_t *cigar, const int64_t *cigar_off, const int32_t *n_cigar,
                                const int32_t *seq_len, const float *event_mean, const int64_t *event_off, const int32_t *n_events,
                                const gab_abea_range *map, const int64_t *map_off, const gab_abea_calib *calib,
                                int32_t region_start, int32_t region_end, int64_t n_reads,
                                gab_abea_ealn *out, const int64_t *out_off, gab_abea_realign_read *res) {
    if (!h) return rl_no_handle("gab_abea_realign");
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_realign: n_reads %lld out of range", (long long)n_reads);
    rl_reset(h->realign);
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(ref_off && ref_len && ref_pos && is_rev && cigar_off && n_cigar && seq_len && event_mean && event_off && n_events && map && map_off && calib && out_off && res,
              "gab_abea_realign: NULL argument");
    const size_t n = (size_t)n_reads;
    // the windows of the five slabs that the reads refer to; the device call sees them re-based to the windows' starts
    int64_t ra = INT64_MAX, rb = 0, ca = INT64_MAX, cb = 0, ea = INT64_MAX, eb = 0, ma = INT64_MAX, mb = 0, oa = INT64_MAX, ob = 0;
    std::vector<int64_t> ro(n), co(n), eo(n), mo(n), oo(n), room(n);
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(seq_len[i] >= K && n_events[i] >= 1, "gab_abea_realign: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, seq_len[i], K, n_events[i]);
        GAB_CHECK(ref_len[i] >= 0 && n_cigar[i] >= 0 && ref_pos[i] >= 0, "gab_abea_realign: read %zu: ref_len %d, n_cigar %d, ref_pos %d: none may be negative", i, ref_len[i], n_cigar[i], ref_pos[i]);
        GAB_CHECK(ref_off[i] >= 0 && cigar_off[i] >= 0 && event_off[i] >= 0 && map_off[i] >= 0 && out_off[i] >= 0, "gab_abea_realign: read %zu: negative offset", i);
        GAB_CHECK((ref || ref_len[i] == 0) && (cigar || n_cigar[i] == 0), "gab_abea_realign: NULL argument");
        int64_t n_skip = 0;
        for (int32_t k = 0; k < n_cigar[i]; k++) n_skip += (cigar[cigar_off[i] + k] & 15u) == 3u;
        room[i] = (int64_t)n_events[i] * (1 + n_skip);
        GAB_CHECK(out, "gab_abea_realign: NULL argument");
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
    const size_t o_out = a.region(sizeof(gab_abea_ealn) * (size_t)(ob - oa)), o_res = a.region(sizeof(gab_abea_realign_read) * n);
    const size_t o_ro = a.a8(n), o_co = a.a8(n), o_eo = a.a8(n), o_mo = a.a8(n), o_oo = a.a8(n);
    const size_t o_rl = a.a4(n), o_rp = a.a4(n), o_nc = a.a4(n), o_sl = a.a4(n), o_ne = a.a4(n), o_rv = a.a4((n + 3) / 4);
    if ((rc = h->realign.io.reserve(a.o)) != GAB_OK) return rc;
    char *b = h->realign.io.as<char>();
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
    rc = gab_abea_realign_device(h, b + o_ref, rb - ra, (const int64_t *)(b + o_ro), (const int32_t *)(b + o_rl), (const int32_t *)(b + o_rp), (const uint8_t *)(b + o_rv),
                                 (const uint32_t *)(b + o_cg), cb - ca, (const int64_t *)(b + o_co), (const int32_t *)(b + o_nc), (const int32_t *)(b + o_sl),
                                 (const float *)(b + o_ev), eb - ea, (const int64_t *)(b + o_eo), (const int32_t *)(b + o_ne),
                                 (const gab_abea_range *)(b + o_map), mb - ma, (const int64_t *)(b + o_mo), (const gab_abea_calib *)(b + o_cal),
                                 region_start, region_end, n_reads, (gab_abea_ealn *)(b + o_out), ob - oa, (const int64_t *)(b + o_oo), (gab_abea_realign_read *)(b + o_res), s);
    if (rc) return rc;
    GAB_HIP(hipMemcpy(res, b + o_res, sizeof(gab_abea_realign_read) * n, hipMemcpyDeviceToHost));
    std::vector<gab_abea_ealn> all;
    try { all.resize((size_t)(ob - oa)); } catch (...) { gab_set_error("gab_abea_realign: out of host memory"); return GAB_ENOMEM; }
    if (!all.empty()) GAB_HIP(hipMemcpy(all.data(), b + o_out, sizeof(gab_abea_ealn) * all.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) if (res[i].n_entries > 0) memcpy(out + out_off[i], all.data() + oo[i], sizeof(gab_abea_ealn) * (size_t)res[i].n_entries);
    return GAB_OK;
}

extern "C" int gab_abea_realign_last_stats(gab_abea *h, int64_t *reads, int64_t *hmm_segments, int64_t *rows, int64_t *cells, int64_t *reads_requeued,
                                           float *kernel_ms, float *total_ms) {
    if (!h) return rl_no_handle("gab_abea_realign_last_stats");
    const gab_abea_realign_state &S = h->realign;
    if (reads) *reads = S.reads;
    if (hmm_segments) *hmm_segments = S.hmm_segments;
    if (rows) *rows = S.rows;
    if (cells) *cells = S.cells;
    if (reads_requeued) *reads_requeued = S.reads_requeued;
    if (kernel_ms) *kernel_ms = S.prep_ms + S.viterbi_ms + S.requeue_ms;
    if (total_ms) *total_ms = S.total_ms;
    return GAB_OK;
}

extern "C" int gab_abea_realign_stage_ms(gab_abea *h, float *prep_ms, float *viterbi_ms, float *requeue_ms) {
    if (!h) return rl_no_handle("gab_abea_realign_stage_ms");
    if (prep_ms) *prep_ms = h->realign.prep_ms;
    if (viterbi_ms) *viterbi_ms = h->realign.viterbi_ms;
    if (requeue_ms) *requeue_ms = h->realign.requeue_ms;
    return GAB_OK;
}
