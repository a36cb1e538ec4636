// abea: event detection (getevents, abea/src/events.c:552-568, after the pA conversion of f5c.c:1249-1253) and the scaling
// estimate by the method of moments (estimate_scalings_using_mom, abea/src/align.c:49-97), behind gab_abea_events* and
// gab_abea_scalings* (include/gab.h).  The handle is the one of abea.hip (abea_handle.h).
//
// Arithmetic: the reference's as built without fused multiply-add, every fp32 / fp64 operation rounded on its own (the pragma
// below; the divisions and sqrtf are the correctly rounded ones).
//
// Shape (DESIGN.md, section "abea: events"); a read is cut into chunks of CH samples:
//   ev_prove      one block per read: the largest exponent and the lowest set significand bit over the samples x and over the fp32
//                 products x * x.  If every addend is a multiple of 2^q and n * 2^(emax + 1) <= 2^(q + 53), every partial sum of
//                 any subset is an integer multiple of 2^q below 2^53 of them: exact in double, in whatever order.  Such a read is
//                 `wide`.  A NaN, an infinity, a denormal, a tiny or a huge sample fails the proof.
//   ev_totals     wide reads, one block per chunk: the chunk's two totals.
//   ev_offsets    one block per read.  Wide: the exclusive scan of its chunk totals.  Not wide: lane 0 adds the whole read in the
//                 reference's order and writes the prefix sums itself (counted in reads_serial_sums).
//   ev_scan       wide reads, one block per chunk: block scan of the chunk on top of its offset -> the prefix sums.
//   ev_tstat      one thread per sample: compute_tstat for w = 3 and w = 6.
//   ev_detect     one thread per chunk: short_long_peak_detector from a cold state, W samples before the chunk (sample 0 for
//                 chunk 0, where cold is the true state); the state at the boundary and at the chunk's end are kept, and the
//                 peaks emitted inside the chunk, in emission order.
//   ev_verify     one thread per read: a chunk stands if the state it assumed at its boundary equals the state the chunk before
//                 it ended in (masked_to only where it still masks a sample ahead); otherwise the chunk is run again from the
//                 true state (chunks_redone) and the comparison goes on with its new end state.  Then the peak counts are
//                 summed: n_events.
//   (host)        n_events come to the host: event_off, the total against event_cap.
//   ev_starts     the peaks of every chunk to their places in event_start.
//   ev_fill       create_event for every event.
//   abea_scalings one wavefront per read: the same proof per sum; a sum that passes is added by lanes and shuffles, one that fails,
//                 and always the sum of squared double differences, in the reference's order (64 addends fetched at a time,
//                 added one by one).
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
constexpr int CH = GAB_ABEA_EVENTS_CHUNK, W = GAB_ABEA_EVENTS_WARMUP;
constexpr int TPB = 256, PER = CH / TPB;             // threads of a chunk's block, samples per thread
static_assert(CH % TPB == 0 && W < CH, "chunk shape");
#define EV_FLT_MAX 3.402823466e+38f
#define EV_FLT_MIN 1.175494351e-38f

struct ev_job {                    // one read
    int64_t raw_off;
    int64_t sbase;                 // its first slot in the per-sample scratch (t-statistics; the peak lists are per chunk)
    int64_t pbase;                 // its first of n + 1 prefix sums
    int64_t cbase;                 // its first chunk
    int32_t n, n_chunks;
    float offset, unit;            // pA = (raw + offset) * unit, unit = range / digitisation (f5c.c:1250-1252)
};
struct ev_state {                  // the two Detectors of events.c:268-279, [0] short, [1] long: what changes while they run
    int64_t masked_to[2];
    int32_t peak_pos[2];
    float peak_value[2];
    int32_t valid[2];
};
struct ev_counters { unsigned long long serial_reads, redone; };
GAB_STATIC_ATOMIC64(ev_counters, serial_reads);
GAB_STATIC_ATOMIC64(ev_counters, redone);

struct ev_scratch {                // device pointers into the handle's scratch for one call
    double *sum, *sumsq;           // S + R each
    float2 *ts;                    // S
    double2 *tot, *coff;           // G each: chunk totals and their exclusive scan
    ev_state *entry, *exit;        // G each
    int32_t *peaks;                // G * CH: chunk g's peaks at g * CH
    int32_t *count, *poff;         // G each: peaks of the chunk, and peaks of the read before the chunk
    int32_t *wide;                 // R
    ev_counters *ctr;
};

__device__ __forceinline__ float ev_pa(const float *raw, const ev_job &j, int64_t i) { return (raw[j.raw_off + i] + j.offset) * j.unit; }

// the exponent and the lowest set bit of one addend; zero adds nothing
__device__ __forceinline__ void ev_bits(float v, int &emax, int &qmin, int &bad) {
    const unsigned b = __float_as_uint(v), e = (b >> 23) & 0xffu, m = b & 0x7fffffu;
    if (e == 255u || (e == 0u && m != 0u)) { bad = 1; return; }
    if (e == 0u) return;
    const int E = (int)e - 127;
    emax = E > emax ? E : emax;
    const int q = E - 23 + __builtin_ctz(m | 0x800000u);
    qmin = q < qmin ? q : qmin;
}
__device__ __forceinline__ bool ev_exact(int n, int emax, int qmin, int bad) {
    if (bad) return false;
    if (emax < qmin) return true;                    // every addend zero
    const int L = 32 - __clz(n);                     // n < 2^L
    return L + emax + 1 <= qmin + 53;
}

__global__ __launch_bounds__(TPB) void ev_prove(const ev_job *jobs, const float *raw, ev_scratch s) {
    __shared__ int sh[6];                            // emax, qmin, bad of x; of x * x
    const ev_job j = jobs[blockIdx.x];
    if (threadIdx.x < 6) sh[threadIdx.x] = (threadIdx.x % 3 == 0) ? -1000 : (threadIdx.x % 3 == 1) ? 1000 : 0;
    __syncthreads();
    int e1 = -1000, q1 = 1000, b1 = 0, e2 = -1000, q2 = 1000, b2 = 0;
    for (int i = threadIdx.x; i < j.n; i += TPB) {
        const float x = ev_pa(raw, j, i);
        ev_bits(x, e1, q1, b1);
        ev_bits(x * x, e2, q2, b2);
    }
    atomicMax(&sh[0], e1); atomicMin(&sh[1], q1); atomicOr(&sh[2], b1);
    atomicMax(&sh[3], e2); atomicMin(&sh[4], q2); atomicOr(&sh[5], b2);
    __syncthreads();
    if (threadIdx.x == 0) s.wide[blockIdx.x] = (ev_exact(j.n, sh[0], sh[1], sh[2]) && ev_exact(j.n, sh[3], sh[4], sh[5])) ? 1 : 0;
}

__global__ __launch_bounds__(TPB) void ev_totals(const ev_job *jobs, const int32_t *chunk_read, const float *raw, ev_scratch s) {
    __shared__ double a[TPB], b[TPB];
    const int64_t g = blockIdx.x;
    const int r = chunk_read[g];
    if (!s.wide[r]) return;                          // (uniform over the block)
    const ev_job j = jobs[r];
    const int64_t first = (g - j.cbase) * CH + (int64_t)threadIdx.x * PER;
    double x1 = 0.0, x2 = 0.0;
#pragma unroll
    for (int t = 0; t < PER; t++)
        if (first + t < j.n) { const float x = ev_pa(raw, j, first + t); x1 += (double)x; x2 += (double)(x * x); }
    a[threadIdx.x] = x1; b[threadIdx.x] = x2;
    __syncthreads();
    for (int w = TPB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { a[threadIdx.x] += a[threadIdx.x + w]; b[threadIdx.x] += b[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) s.tot[g] = make_double2(a[0], b[0]);
}

__global__ __launch_bounds__(64) void ev_offsets(const ev_job *jobs, const float *raw, ev_scratch s) {
    if (threadIdx.x != 0) return;
    const ev_job j = jobs[blockIdx.x];
    double x1 = 0.0, x2 = 0.0;
    if (s.wide[blockIdx.x]) {
        for (int c = 0; c < j.n_chunks; c++) {
            s.coff[j.cbase + c] = make_double2(x1, x2);
            const double2 t = s.tot[j.cbase + c];
            x1 += t.x; x2 += t.y;
        }
        return;
    }
    // compute_sum_sumsq, events.c:292-302, as written
    s.sum[j.pbase] = 0.0; s.sumsq[j.pbase] = 0.0;
    for (int64_t i = 0; i < j.n; i++) {
        const float x = ev_pa(raw, j, i);
        x1 = x1 + (double)x; x2 = x2 + (double)(x * x);
        s.sum[j.pbase + i + 1] = x1; s.sumsq[j.pbase + i + 1] = x2;
    }
    atomicAdd(&s.ctr->serial_reads, 1ull);
}

__global__ __launch_bounds__(TPB) void ev_scan(const ev_job *jobs, const int32_t *chunk_read, const float *raw, ev_scratch s) {
    __shared__ double a[2][TPB], b[2][TPB];
    const int64_t g = blockIdx.x;
    const int r = chunk_read[g];
    if (!s.wide[r]) return;
    const ev_job j = jobs[r];
    const int tid = threadIdx.x;
    const int64_t first = (g - j.cbase) * CH + (int64_t)tid * PER;
    double l1[PER], l2[PER];                         // inclusive within the thread
    double x1 = 0.0, x2 = 0.0;
#pragma unroll
    for (int t = 0; t < PER; t++) {
        if (first + t < j.n) { const float x = ev_pa(raw, j, first + t); x1 += (double)x; x2 += (double)(x * x); }
        l1[t] = x1; l2[t] = x2;
    }
    int cur = 0;
    a[0][tid] = x1; b[0][tid] = x2;
    __syncthreads();
    for (int d = 1; d < TPB; d <<= 1) {              // inclusive scan of the threads' totals
        double v1 = a[cur][tid], v2 = b[cur][tid];
        if (tid >= d) { v1 += a[cur][tid - d]; v2 += b[cur][tid - d]; }
        a[cur ^ 1][tid] = v1; b[cur ^ 1][tid] = v2;
        cur ^= 1;
        __syncthreads();
    }
    const double2 off = s.coff[g];
    const double o1 = off.x + (tid ? a[cur][tid - 1] : 0.0), o2 = off.y + (tid ? b[cur][tid - 1] : 0.0);
    if (first == 0) { s.sum[j.pbase] = 0.0; s.sumsq[j.pbase] = 0.0; }
#pragma unroll
    for (int t = 0; t < PER; t++)
        if (first + t < j.n) { s.sum[j.pbase + first + t + 1] = o1 + l1[t]; s.sumsq[j.pbase + first + t + 1] = o2 + l2[t]; }
}

// compute_tstat, events.c:314-363, at one position: the file is C++, so fabs and sqrt at line 359 are the float overloads
__device__ __forceinline__ float ev_tstat_at(const double *sum, const double *sumsq, int64_t n, int w, int64_t i) {
    if (n < 2 * w || i < w || i > n - w) return 0.0f;
    const float wf = (float)w;
    double sum1 = sum[i], sumsq1 = sumsq[i];
    if (i > w) { sum1 -= sum[i - w]; sumsq1 -= sumsq[i - w]; }
    const float sum2 = (float)(sum[i + w] - sum[i]);
    const float sumsq2 = (float)(sumsq[i + w] - sumsq[i]);
    const float mean1 = (float)(sum1 / (double)wf);
    const float mean2 = sum2 / wf;
    float combined_var = (float)(((sumsq1 / (double)wf - (double)(mean1 * mean1)) + (double)(sumsq2 / wf)) - (double)(mean2 * mean2));
    combined_var = fmaxf(combined_var, EV_FLT_MIN);
    const float delta_mean = mean2 - mean1;
    return fabsf(delta_mean) / sqrtf(combined_var / wf);
}

__global__ __launch_bounds__(TPB) void ev_tstat(const ev_job *jobs, const int32_t *chunk_read, ev_scratch s) {
    const int64_t g = blockIdx.x;
    const ev_job j = jobs[chunk_read[g]];
    const double *sum = s.sum + j.pbase, *sumsq = s.sumsq + j.pbase;
    const int64_t base = (g - j.cbase) * CH;
    for (int t = threadIdx.x; t < CH; t += TPB) {
        const int64_t i = base + t;
        if (i < j.n) s.ts[j.sbase + i] = make_float2(ev_tstat_at(sum, sumsq, j.n, 3, i), ev_tstat_at(sum, sumsq, j.n, 6, i));
    }
}

__device__ __forceinline__ ev_state ev_cold() {
    ev_state s;
    for (int k = 0; k < 2; k++) { s.masked_to[k] = 0; s.peak_pos[k] = -1; s.peak_value[k] = EV_FLT_MAX; s.valid[k] = 0; }
    return s;
}

// one sample of short_long_peak_detector, events.c:382-439; a peak that is emitted goes to out[*cnt] while *cnt < room
__device__ __forceinline__ void ev_step(ev_state &s, int64_t i, float2 t, int32_t *out, int *cnt, int room) {
    const float peak_height = 0.2f;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float threshold = k ? 9.0f : 1.4f;
        const int64_t window = k ? 6 : 3;
        if (s.masked_to[k] >= i) continue;
        const float current = k ? t.y : t.x;
        if (s.peak_pos[k] == -1) {
            if (current < s.peak_value[k]) {
                s.peak_value[k] = current;
            } else if (current - s.peak_value[k] > peak_height) {
                s.peak_value[k] = current; s.peak_pos[k] = (int32_t)i;
            }
        } else {
            if (current > s.peak_value[k]) { s.peak_value[k] = current; s.peak_pos[k] = (int32_t)i; }
            if (k == 0 && s.peak_value[0] > threshold) {
                s.masked_to[1] = (int64_t)s.peak_pos[0] + window;
                s.peak_pos[1] = -1; s.peak_value[1] = EV_FLT_MAX; s.valid[1] = 0;
            }
            if (s.peak_value[k] - current > peak_height && s.peak_value[k] > threshold) s.valid[k] = 1;
            if (s.valid[k] && (i - (int64_t)s.peak_pos[k]) > window / 2) {
                if (out && *cnt < room) out[*cnt] = s.peak_pos[k];
                if (out) (*cnt)++;
                s.peak_pos[k] = -1; s.peak_value[k] = current; s.valid[k] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(64) void ev_detect(const ev_job *jobs, const int32_t *chunk_read, int64_t n_chunks, ev_scratch s) {
    const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= n_chunks) return;
    const ev_job j = jobs[chunk_read[g]];
    const float2 *ts = s.ts + j.sbase;
    const int64_t lo = (g - j.cbase) * CH, hi = lo + CH < j.n ? lo + CH : j.n;
    ev_state st = ev_cold();
    for (int64_t i = lo ? lo - W : 0; i < lo; i++) ev_step(st, i, ts[i], nullptr, nullptr, 0);
    s.entry[g] = st;
    int cnt = 0;
    int32_t *out = s.peaks + g * CH;
    for (int64_t i = lo; i < hi; i++) ev_step(st, i, ts[i], out, &cnt, CH);
    s.exit[g] = st; s.count[g] = cnt;
}

// does a machine in state b behave, from sample `next` on, as one in state a?
__device__ __forceinline__ bool ev_same(const ev_state &a, const ev_state &b, int64_t next) {
    for (int k = 0; k < 2; k++) {
        if (a.peak_pos[k] != b.peak_pos[k] || __float_as_uint(a.peak_value[k]) != __float_as_uint(b.peak_value[k]) || a.valid[k] != b.valid[k]) return false;
        if ((a.masked_to[k] >= next || b.masked_to[k] >= next) && a.masked_to[k] != b.masked_to[k]) return false;
    }
    return true;
}

__global__ __launch_bounds__(64) void ev_verify(const ev_job *jobs, int64_t n_reads, ev_scratch s, int32_t *n_events) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= n_reads) return;
    const ev_job j = jobs[r];
    const float2 *ts = s.ts + j.sbase;
    unsigned long long redone = 0;
    int64_t peaks = 0;
    for (int c = 0; c < j.n_chunks; c++) {
        const int64_t g = j.cbase + c;
        if (c > 0) {
            const ev_state prev = s.exit[g - 1], mine = s.entry[g];
            const int64_t lo = (int64_t)c * CH, hi = lo + CH < j.n ? lo + CH : j.n;
            if (!ev_same(prev, mine, lo)) {
                ev_state st = prev;
                int cnt = 0;
                int32_t *out = s.peaks + g * CH;
                for (int64_t i = lo; i < hi; i++) ev_step(st, i, ts[i], out, &cnt, CH);
                s.exit[g] = st; s.count[g] = cnt;
                redone++;
            }
        }
        s.poff[g] = (int32_t)peaks;
        peaks += s.count[g];
    }
    n_events[r] = (int32_t)(peaks + 1);              // create_events counts from 1; with no peak: the one event of the whole read
    if (redone) atomicAdd(&s.ctr->redone, redone);
}

__global__ __launch_bounds__(64) void ev_starts(const ev_job *jobs, const int32_t *chunk_read, ev_scratch s, const int64_t *event_off, int32_t *event_start) {
    const int64_t g = blockIdx.x;
    const int r = chunk_read[g];
    const int64_t eo = event_off[r], cbase = jobs[r].cbase;
    const int cnt = s.count[g] < CH ? s.count[g] : CH;
    if (g == cbase && threadIdx.x == 0) event_start[eo] = 0;
    for (int t = threadIdx.x; t < cnt; t += 64) event_start[eo + 1 + s.poff[g] + t] = s.peaks[g * CH + t];
}

// create_event, events.c:456-472, for the events whose first sample this chunk's peaks give (and event 0 in the read's first chunk)
__global__ __launch_bounds__(64) void ev_fill(const ev_job *jobs, const int32_t *chunk_read, ev_scratch s, const int64_t *event_off, const int32_t *n_events,
                                              const int32_t *event_start, float *event_mean, float *event_stdv, float *event_length) {
    const int64_t g = blockIdx.x;
    const int r = chunk_read[g];
    const ev_job j = jobs[r];
    const int64_t eo = event_off[r];
    const int nev = n_events[r];
    const int cnt = s.count[g] < CH ? s.count[g] : CH;
    const double *sum = s.sum + j.pbase, *sumsq = s.sumsq + j.pbase;
    for (int t = (g == j.cbase ? -1 : 0) + (int)threadIdx.x; t < cnt; t += 64) {
        const int e = 1 + s.poff[g] + t;             // t = -1: event 0
        const uint64_t start = (uint64_t)event_start[eo + e];
        const uint64_t end = e + 1 < nev ? (uint64_t)event_start[eo + e + 1] : (uint64_t)j.n;
        const float length = (float)(end - start);
        const float mean = (float)(sum[end] - sum[start]) / length;
        const float deltasqr = (float)(sumsq[end] - sumsq[start]);
        const float var = deltasqr / length - mean * mean;
        event_length[eo + e] = length; event_mean[eo + e] = mean; event_stdv[eo + e] = sqrtf(fmaxf(var, 0.0f));
    }
}

__device__ __forceinline__ int sc_rank(char c) { return c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 0; }

struct sc_counters { unsigned long long event_sum, kmer_sum, kmer_sq_sum; };      // reads whose sum was added in order
GAB_STATIC_ATOMIC64(sc_counters, event_sum);

// a sum in the reference's order by one wavefront: 64 addends are fetched at a time and added one by one, in every lane alike
template <typename Addend> __device__ __forceinline__ double sc_in_order(int n, int lane, Addend addend) {
    double sum = 0.0;
    for (int base = 0; base < n; base += 64) {
        const double v = base + lane < n ? addend(base + lane) : 0.0;
        const int m = n - base < 64 ? n - base : 64;
        for (int t = 0; t < m; t++) sum += __shfl(v, t);
    }
    return sum;
}
// the lanes' partial sums of an order-free sum (every addition exact, so every lane ends with the same bits)
__device__ __forceinline__ double sc_wave_sum(double v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return __shfl(v, 0);
}
__device__ __forceinline__ void sc_wave_proof(int &emax, int &qmin, int &bad) {
    for (int d = 32; d > 0; d >>= 1) {
        const int e = __shfl_xor(emax, d), q = __shfl_xor(qmin, d), b = __shfl_xor(bad, d);
        emax = e > emax ? e : emax; qmin = q < qmin ? q : qmin; bad |= b;
    }
}

// estimate_scalings_using_mom, align.c:49-97, one wavefront per read.  Of its four double sums, those of the event means, of the
// k-mer levels and of the levels' squares (a float squared in double is exact: its grid is 2^(2q), its size below 2^(2 emax + 2))
// are added wide when ev_exact proves them order-free, and in the reference's order otherwise; the sum of the squared double
// differences is not exact in any order and is always added in order.
__global__ __launch_bounds__(64) void abea_scalings(const char *seq, const int64_t *seq_off, const int32_t *seq_len, const float *event_mean,
                                                    const int64_t *event_off, const int32_t *n_events, const float *level_mean, float *scale, float *shift,
                                                    sc_counters *ctr) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int n = n_events[r], n_kmers = seq_len[r] - K + 1;
    const float *ev = event_mean + event_off[r];
    const char *sq = seq + seq_off[r];
    auto level = [&](int i) {
        int rank = 0;
        for (int t = 0; t < K; t++) rank = (rank << 2) | sc_rank(sq[i + t]);
        return level_mean[rank];
    };

    int emax = -1000, qmin = 1000, bad = 0;
    double part = 0.0;
    for (int i = lane; i < n; i += 64) { const float v = ev[i]; ev_bits(v, emax, qmin, bad); part += (double)v; }
    sc_wave_proof(emax, qmin, bad);
    const bool wide_e = ev_exact(n, emax, qmin, bad);
    const double event_level_sum = wide_e ? sc_wave_sum(part) : sc_in_order(n, lane, [&](int i) { return (double)ev[i]; });

    emax = -1000; qmin = 1000; bad = 0;
    double part_k = 0.0, part_q = 0.0;
    for (int i = lane; i < n_kmers; i += 64) { const float l = level(i); ev_bits(l, emax, qmin, bad); part_k += (double)l; part_q += (double)l * (double)l; }
    sc_wave_proof(emax, qmin, bad);
    const bool wide_k = ev_exact(n_kmers, emax, qmin, bad), wide_q = ev_exact(n_kmers, 2 * emax + 1, 2 * qmin, bad);
    const double kmer_level_sum = wide_k ? sc_wave_sum(part_k) : sc_in_order(n_kmers, lane, [&](int i) { return (double)level(i); });
    const double kmer_level_sq_sum = wide_q ? sc_wave_sum(part_q) : sc_in_order(n_kmers, lane, [&](int i) { const double l = (double)level(i); return l * l; });

    const double sh = event_level_sum / (double)n - kmer_level_sum / (double)n_kmers;
    const double event_level_sq_sum = sc_in_order(n, lane, [&](int i) { const double v = (double)ev[i]; return (v - sh) * (v - sh); });
    const double sc = (event_level_sq_sum / (double)n) / (kmer_level_sq_sum / (double)n_kmers);
    if (lane == 0) {
        shift[r] = (float)sh; scale[r] = (float)sc;
        if (!wide_e) atomicAdd(&ctr->event_sum, 1ull);
        if (!wide_k) atomicAdd(&ctr->kmer_sum, 1ull);
        if (!wide_q) atomicAdd(&ctr->kmer_sq_sum, 1ull);
    }
}

void ev_reset(gab_abea_events_state &e) {
    e.samples = e.events = e.reads_serial_sums = e.chunks = e.chunks_redone = 0;
    e.sums_ms = e.detect_ms = e.fill_ms = e.total_ms = 0.f;
}

}  // namespace

gab_abea_events_state::~gab_abea_events_state() {
    io.release(); plan.release(); scratch.release(); sc_ctr.release();
    for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v);
}

extern "C" int gab_abea_events_device(gab_abea *h, const float *raw, int64_t raw_count, const int64_t *raw_off, const int32_t *n_samples,
                                      const float *range, const float *digitisation, const float *offset, int64_t n_reads,
                                      int32_t *n_events, int64_t *event_off, float *event_mean, float *event_stdv, int32_t *event_start,
                                      float *event_length, int64_t event_cap, int64_t *total_events, void *stream) {
    if (!h) { gab_set_error("gab_abea_events_device: NULL handle"); return GAB_EINVAL; }
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_events_device: n_reads %lld out of range", (long long)n_reads);
    gab_abea_events_state &E = h->events;
    ev_reset(E);
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(raw && raw_off && n_samples && range && digitisation && offset && n_events && event_off && total_events && event_cap >= 0 &&
              (event_cap == 0 || (event_mean && event_stdv && event_start && event_length)), "gab_abea_events_device: NULL argument");
    gab_device_guard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)n_reads;
    for (hipEvent_t &v : E.ev) if (!v) GAB_HIP(hipEventCreate(&v));

    std::vector<int64_t> ro(n); std::vector<int32_t> ns(n); std::vector<float> rg(n), dg(n), of(n);
    GAB_HIP(hipMemcpyAsync(ro.data(), raw_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(ns.data(), n_samples, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(rg.data(), range, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(dg.data(), digitisation, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(of.data(), offset, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));

    std::vector<ev_job> jobs(n);
    int64_t S = 0, G = 0;
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(ns[i] >= 1, "gab_abea_events: read %zu: n_samples %d (>= 1 needed)", i, ns[i]);
        GAB_CHECK(dg[i] != 0.0f, "gab_abea_events: read %zu: digitisation 0", i);
        GAB_CHECK(ro[i] >= 0 && ro[i] + ns[i] <= raw_count, "gab_abea_events: read %zu: samples [%lld, +%d) outside the slab of %lld", i, (long long)ro[i], ns[i], (long long)raw_count);
        ev_job &j = jobs[i];
        j.raw_off = ro[i]; j.sbase = S; j.pbase = S + (int64_t)i; j.cbase = G;
        j.n = ns[i]; j.n_chunks = (int32_t)gab_ceil_div(ns[i], CH);
        j.offset = of[i]; j.unit = rg[i] / dg[i];
        S += ns[i]; G += j.n_chunks;
    }
    GAB_CHECK(G <= INT32_MAX, "gab_abea_events: %lld chunks of %d samples in one call", (long long)G, CH);
    std::vector<int32_t> chunk_read((size_t)G);
    for (size_t i = 0; i < n; i++) std::fill(chunk_read.begin() + jobs[i].cbase, chunk_read.begin() + jobs[i].cbase + jobs[i].n_chunks, (int32_t)i);

    gab_stage_bump pl;
    const size_t p_jobs = pl.region(sizeof(ev_job) * n), p_cr = pl.region(4 * (size_t)G);
    int rc = E.plan.reserve(pl.o);
    if (rc) return rc;
    gab_stage_bump a;
    const size_t o_ctr = a.cursor();
    const size_t o_sum = a.region(8 * (size_t)(S + n_reads)), o_sumsq = a.region(8 * (size_t)(S + n_reads)), o_ts = a.region(8 * (size_t)S);
    const size_t o_tot = a.region(16 * (size_t)G), o_coff = a.region(16 * (size_t)G);
    const size_t o_entry = a.region(sizeof(ev_state) * (size_t)G), o_exit = a.region(sizeof(ev_state) * (size_t)G);
    const size_t o_peaks = a.region(4 * (size_t)G * CH), o_count = a.region(4 * (size_t)G), o_poff = a.region(4 * (size_t)G), o_wide = a.region(4 * n);
    GAB_CHECK_ATOMIC64(o_ctr);
    if ((rc = E.scratch.reserve(a.o)) != GAB_OK) return rc;
    char *b = E.scratch.as<char>();
    ev_scratch sc;
    sc.ctr = (ev_counters *)(b + o_ctr); sc.sum = (double *)(b + o_sum); sc.sumsq = (double *)(b + o_sumsq); sc.ts = (float2 *)(b + o_ts);
    sc.tot = (double2 *)(b + o_tot); sc.coff = (double2 *)(b + o_coff); sc.entry = (ev_state *)(b + o_entry); sc.exit = (ev_state *)(b + o_exit);
    sc.peaks = (int32_t *)(b + o_peaks); sc.count = (int32_t *)(b + o_count); sc.poff = (int32_t *)(b + o_poff); sc.wide = (int32_t *)(b + o_wide);
    const ev_job *dj = (const ev_job *)(E.plan.as<char>() + p_jobs);
    const int32_t *dcr = (const int32_t *)(E.plan.as<char>() + p_cr);
    GAB_HIP(hipMemcpyAsync((void *)dj, jobs.data(), sizeof(ev_job) * n, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync((void *)dcr, chunk_read.data(), 4 * (size_t)G, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemsetAsync(sc.ctr, 0, sizeof(ev_counters), s));

    const unsigned R = (unsigned)n, GC = (unsigned)G;
    GAB_HIP(hipEventRecord(E.ev[0], s));
    hipLaunchKernelGGL(ev_prove, dim3(R), dim3(TPB), 0, s, dj, raw, sc);
    hipLaunchKernelGGL(ev_totals, dim3(GC), dim3(TPB), 0, s, dj, dcr, raw, sc);
    hipLaunchKernelGGL(ev_offsets, dim3(R), dim3(64), 0, s, dj, raw, sc);
    hipLaunchKernelGGL(ev_scan, dim3(GC), dim3(TPB), 0, s, dj, dcr, raw, sc);
    hipLaunchKernelGGL(ev_tstat, dim3(GC), dim3(TPB), 0, s, dj, dcr, sc);
    GAB_HIP(hipEventRecord(E.ev[1], s));
    hipLaunchKernelGGL(ev_detect, dim3((unsigned)gab_ceil_div(G, 64)), dim3(64), 0, s, dj, dcr, G, sc);
    hipLaunchKernelGGL(ev_verify, dim3((unsigned)gab_ceil_div(n_reads, 64)), dim3(64), 0, s, dj, n_reads, sc, n_events);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(E.ev[2], s));

    // the counts come to the host: where every read's events start, and whether the slabs hold them
    std::vector<int32_t> ne(n); std::vector<int64_t> eo(n);
    ev_counters ctr;
    GAB_HIP(hipMemcpyAsync(ne.data(), n_events, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(&ctr, sc.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    int64_t total = 0;
    for (size_t i = 0; i < n; i++) { eo[i] = total; total += ne[i]; }
    GAB_HIP(hipMemcpyAsync(event_off, eo.data(), 8 * n, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(total_events, &total, 8, hipMemcpyHostToDevice, s));
    E.samples = S; E.events = total; E.chunks = G; E.reads_serial_sums = (int64_t)ctr.serial_reads; E.chunks_redone = (int64_t)ctr.redone;
    GAB_HIP(hipEventElapsedTime(&E.sums_ms, E.ev[0], E.ev[1]));
    GAB_HIP(hipEventElapsedTime(&E.detect_ms, E.ev[1], E.ev[2]));
    if (total > event_cap) {
        GAB_HIP(hipStreamSynchronize(s));
        E.total_ms = E.sums_ms + E.detect_ms;
        gab_set_error("gab_abea_events: %lld events, room for %lld", (long long)total, (long long)event_cap);
        return GAB_ERANGE;
    }
    GAB_HIP(hipEventRecord(E.ev[3], s));
    hipLaunchKernelGGL(ev_starts, dim3(GC), dim3(64), 0, s, dj, dcr, sc, event_off, event_start);
    hipLaunchKernelGGL(ev_fill, dim3(GC), dim3(64), 0, s, dj, dcr, sc, event_off, n_events, event_start, event_mean, event_stdv, event_length);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(E.ev[4], s));
    GAB_HIP(hipStreamSynchronize(s));
    GAB_HIP(hipEventElapsedTime(&E.fill_ms, E.ev[3], E.ev[4]));
    GAB_HIP(hipEventElapsedTime(&E.total_ms, E.ev[0], E.ev[4]));
    return GAB_OK;
}

extern "C" int gab_abea_events(gab_abea *h, const float *raw, const int64_t *raw_off, const int32_t *n_samples,
                               const float *range, const float *digitisation, const float *offset, int64_t n_reads,
                               int32_t *n_events, int64_t *event_off, float *event_mean, float *event_stdv, int32_t *event_start,
                               float *event_length, int64_t event_cap, int64_t *total_events) {
    if (!h) { gab_set_error("gab_abea_events: NULL handle"); return GAB_EINVAL; }
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_events: n_reads %lld out of range", (long long)n_reads);
    ev_reset(h->events);
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(raw && raw_off && n_samples && range && digitisation && offset && n_events && event_off && total_events && event_cap >= 0 &&
              (event_cap == 0 || (event_mean && event_stdv && event_start && event_length)), "gab_abea_events: NULL argument");
    const size_t n = (size_t)n_reads;
    int64_t ra = INT64_MAX, rb = 0, S = 0;
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(n_samples[i] >= 1, "gab_abea_events: read %zu: n_samples %d (>= 1 needed)", i, n_samples[i]);
        GAB_CHECK(digitisation[i] != 0.0f, "gab_abea_events: read %zu: digitisation 0", i);
        GAB_CHECK(raw_off[i] >= 0, "gab_abea_events: read %zu: negative offset", i);
        ra = std::min(ra, raw_off[i]); rb = std::max(rb, raw_off[i] + n_samples[i]); S += n_samples[i];
    }
    gab_device_guard g(h->device);
    hipStream_t s = nullptr;
    int rc = h->hs.get(&s);
    if (rc) return rc;
    const size_t cap = (size_t)std::min(event_cap, S);           // a read of n samples has at most n events
    gab_stage_bump a;
    const size_t o_raw = a.region(4 * (size_t)(rb - ra)), o_mean = a.region(4 * cap), o_stdv = a.region(4 * cap), o_start = a.region(4 * cap), o_len = a.region(4 * cap);
    const size_t o_ro = a.a8(n), o_eo = a.a8(n), o_tot = a.a8(1), o_ns = a.a4(n), o_rg = a.a4(n), o_dg = a.a4(n), o_of = a.a4(n), o_ne = a.a4(n);
    if ((rc = h->events.io.reserve(a.o)) != GAB_OK) return rc;
    char *b = h->events.io.as<char>();
    std::vector<int64_t> ro(n);
    for (size_t i = 0; i < n; i++) ro[i] = raw_off[i] - ra;
    {
        std::lock_guard<std::mutex> gate(gab_h2d_mutex(h->device));
        GAB_HIP(hipMemcpyAsync(b + o_raw, raw + ra, 4 * (size_t)(rb - ra), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_ro, ro.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_ns, n_samples, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_rg, range, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_dg, digitisation, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_of, offset, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    rc = gab_abea_events_device(h, (const float *)(b + o_raw), rb - ra, (const int64_t *)(b + o_ro), (const int32_t *)(b + o_ns), (const float *)(b + o_rg),
                                (const float *)(b + o_dg), (const float *)(b + o_of), n_reads, (int32_t *)(b + o_ne), (int64_t *)(b + o_eo),
                                (float *)(b + o_mean), (float *)(b + o_stdv), (int32_t *)(b + o_start), (float *)(b + o_len), (int64_t)cap, (int64_t *)(b + o_tot), s);
    if (rc != GAB_OK && rc != GAB_ERANGE) return rc;
    GAB_HIP(hipMemcpy(n_events, b + o_ne, 4 * n, hipMemcpyDeviceToHost));
    GAB_HIP(hipMemcpy(event_off, b + o_eo, 8 * n, hipMemcpyDeviceToHost));
    GAB_HIP(hipMemcpy(total_events, b + o_tot, 8, hipMemcpyDeviceToHost));
    if (rc == GAB_ERANGE) return rc;
    const size_t t = (size_t)*total_events;
    if (t) {
        GAB_HIP(hipMemcpy(event_mean, b + o_mean, 4 * t, hipMemcpyDeviceToHost));
        GAB_HIP(hipMemcpy(event_stdv, b + o_stdv, 4 * t, hipMemcpyDeviceToHost));
        GAB_HIP(hipMemcpy(event_start, b + o_start, 4 * t, hipMemcpyDeviceToHost));
        GAB_HIP(hipMemcpy(event_length, b + o_len, 4 * t, hipMemcpyDeviceToHost));
    }
    return GAB_OK;
}

extern "C" int gab_abea_scalings_device(gab_abea *h, const char *seq, int64_t seq_bytes, const int64_t *seq_off, const int32_t *seq_len,
                                        const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events, int64_t n_reads,
                                        float *scale, float *shift, void *stream) {
    if (!h) { gab_set_error("gab_abea_scalings_device: NULL handle"); return GAB_EINVAL; }
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_scalings_device: n_reads %lld out of range", (long long)n_reads);
    h->events.sc_reads = 0; h->events.sc_in_order[0] = h->events.sc_in_order[1] = h->events.sc_in_order[2] = 0;
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(seq && seq_off && seq_len && event_mean && event_off && n_events && scale && shift, "gab_abea_scalings_device: NULL argument");
    gab_device_guard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)n_reads;
    std::vector<int64_t> so(n), eo(n); std::vector<int32_t> sl(n), ne(n);
    GAB_HIP(hipMemcpyAsync(so.data(), seq_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(eo.data(), event_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(sl.data(), seq_len, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(ne.data(), n_events, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(sl[i] >= K && ne[i] >= 1, "gab_abea_scalings: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, sl[i], K, ne[i]);
        GAB_CHECK(so[i] >= 0 && so[i] + sl[i] <= seq_bytes, "gab_abea_scalings: read %zu: bases [%lld, +%d) outside the slab of %lld bytes", i, (long long)so[i], sl[i], (long long)seq_bytes);
        GAB_CHECK(eo[i] >= 0 && eo[i] + ne[i] <= event_count, "gab_abea_scalings: read %zu: events [%lld, +%d) outside the slab of %lld", i, (long long)eo[i], ne[i], (long long)event_count);
    }
    int rc = h->events.sc_ctr.reserve(sizeof(sc_counters));
    if (rc) return rc;
    sc_counters *dc = h->events.sc_ctr.as<sc_counters>(), ctr;
    GAB_HIP(hipMemsetAsync(dc, 0, sizeof(sc_counters), s));
    hipLaunchKernelGGL(abea_scalings, dim3((unsigned)n), dim3(64), 0, s, seq, seq_off, seq_len, event_mean, event_off, n_events, h->model.as<float>(), scale, shift, dc);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipMemcpyAsync(&ctr, dc, sizeof ctr, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    h->events.sc_reads = n_reads;
    h->events.sc_in_order[0] = (int64_t)ctr.event_sum; h->events.sc_in_order[1] = (int64_t)ctr.kmer_sum; h->events.sc_in_order[2] = (int64_t)ctr.kmer_sq_sum;
    return GAB_OK;
}

extern "C" int gab_abea_scalings(gab_abea *h, const char *seq, const int64_t *seq_off, const int32_t *seq_len,
                                 const float *event_mean, const int64_t *event_off, const int32_t *n_events, int64_t n_reads,
                                 float *scale, float *shift) {
    if (!h) { gab_set_error("gab_abea_scalings: NULL handle"); return GAB_EINVAL; }
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_scalings: n_reads %lld out of range", (long long)n_reads);
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(seq && seq_off && seq_len && event_mean && event_off && n_events && scale && shift, "gab_abea_scalings: NULL argument");
    const size_t n = (size_t)n_reads;
    int64_t sa = INT64_MAX, sb = 0, ea = INT64_MAX, eb = 0;
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(seq_len[i] >= K && n_events[i] >= 1, "gab_abea_scalings: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, seq_len[i], K, n_events[i]);
        GAB_CHECK(seq_off[i] >= 0 && event_off[i] >= 0, "gab_abea_scalings: read %zu: negative offset", i);
        sa = std::min(sa, seq_off[i]); sb = std::max(sb, seq_off[i] + seq_len[i]);
        ea = std::min(ea, event_off[i]); eb = std::max(eb, event_off[i] + n_events[i]);
    }
    gab_device_guard g(h->device);
    hipStream_t s = nullptr;
    int rc = h->hs.get(&s);
    if (rc) return rc;
    gab_stage_bump a;
    const size_t o_seq = a.region(gab_pad256((size_t)(sb - sa))), o_ev = a.region(4 * (size_t)(eb - ea));
    const size_t o_so = a.a8(n), o_eo = a.a8(n), o_sl = a.a4(n), o_ne = a.a4(n), o_sc = a.a4(n), o_sh = a.a4(n);
    if ((rc = h->events.io.reserve(a.o)) != GAB_OK) return rc;
    char *b = h->events.io.as<char>();
    std::vector<int64_t> so(n), eo(n);
    for (size_t i = 0; i < n; i++) { so[i] = seq_off[i] - sa; eo[i] = event_off[i] - ea; }
    {
        std::lock_guard<std::mutex> gate(gab_h2d_mutex(h->device));
        GAB_HIP(hipMemcpyAsync(b + o_seq, seq + sa, (size_t)(sb - sa), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_ev, event_mean + ea, 4 * (size_t)(eb - ea), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_so, so.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_eo, eo.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_sl, seq_len, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_ne, n_events, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    rc = gab_abea_scalings_device(h, b + o_seq, sb - sa, (const int64_t *)(b + o_so), (const int32_t *)(b + o_sl), (const float *)(b + o_ev), eb - ea,
                                  (const int64_t *)(b + o_eo), (const int32_t *)(b + o_ne), n_reads, (float *)(b + o_sc), (float *)(b + o_sh), s);
    if (rc) return rc;
    GAB_HIP(hipMemcpy(scale, b + o_sc, 4 * n, hipMemcpyDeviceToHost));
    GAB_HIP(hipMemcpy(shift, b + o_sh, 4 * n, hipMemcpyDeviceToHost));
    return GAB_OK;
}

extern "C" int gab_abea_events_last_stats(gab_abea *h, int64_t *samples, int64_t *events, int64_t *reads_serial_sums,
                                          int64_t *chunks, int64_t *chunks_redone, float *kernel_ms, float *total_ms) {
    if (!h) { gab_set_error("gab_abea_events_last_stats: NULL handle"); return GAB_EINVAL; }
    const gab_abea_events_state &E = h->events;
    if (samples) *samples = E.samples;
    if (events) *events = E.events;
    if (reads_serial_sums) *reads_serial_sums = E.reads_serial_sums;
    if (chunks) *chunks = E.chunks;
    if (chunks_redone) *chunks_redone = E.chunks_redone;
    if (kernel_ms) *kernel_ms = E.sums_ms + E.detect_ms + E.fill_ms;
    if (total_ms) *total_ms = E.total_ms;
    return GAB_OK;
}

extern "C" int gab_abea_scalings_last_stats(gab_abea *h, int64_t *reads, int64_t *event_sums_in_order, int64_t *kmer_sums_in_order, int64_t *kmer_sq_sums_in_order) {
    if (!h) { gab_set_error("gab_abea_scalings_last_stats: NULL handle"); return GAB_EINVAL; }
    if (reads) *reads = h->events.sc_reads;
    if (event_sums_in_order) *event_sums_in_order = h->events.sc_in_order[0];
    if (kmer_sums_in_order) *kmer_sums_in_order = h->events.sc_in_order[1];
    if (kmer_sq_sums_in_order) *kmer_sq_sums_in_order = h->events.sc_in_order[2];
    return GAB_OK;
}

extern "C" int gab_abea_events_stage_ms(gab_abea *h, float *sums_ms, float *detect_ms, float *fill_ms) {
    if (!h) { gab_set_error("gab_abea_events_stage_ms: NULL handle"); return GAB_EINVAL; }
    if (sums_ms) *sums_ms = h->events.sums_ms;
    if (detect_ms) *detect_ms = h->events.detect_ms;
    if (fill_ms) *fill_ms = h->events.fill_ms;
    return GAB_OK;
}

extern "C" int gab_abea_events_shape(int32_t *chunk, int32_t *warmup) {
    if (chunk) *chunk = CH;
    if (warmup) *warmup = W;
    return GAB_OK;
}
