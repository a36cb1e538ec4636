// abea: the block of process_single after align() (abea/src/f5c.c:1438-1501): postalign (abea/src/align.c:550-650),
// recalibrate_model (align.c:655-762) and the three checks that set read_stat_flag, behind gab_abea_calibrate* (include/gab.h).
// The handle is the one of abea.hip (abea_handle.h).
//
// Arithmetic: the reference's as built without fused multiply-add, every fp64 operation rounded on its own (the pragma below; the
// divisions and the sqrt are the correctly rounded ones).
//
// Shape (DESIGN.md, section "abea: calibrate"):
//   cal_check   one block per read: every pair inside the read's k-mers and events, both coordinates non-decreasing along the
//               list.  Writes nothing but the lowest read that breaks a rule; the host stops there.
//   cal_map     one thread per k-mer (up to 64 blocks of 256 a read, striding).  The lists are monotone, so a k-mer's pairs are one segment, found by binary search on
//               ref_pos; inside it the first pair whose event differs from the pair before it gives `start` (the segment's first
//               pair, or by one more search the first pair past that pair's event) and the segment's last pair gives `stop`.
//               One writer per entry, no atomics.
//   cal_fit     one wavefront per read.  The k-mers are walked 64 at a time: a ballot of "has events" and the rank of the nearest
//               earlier set lane (carried over from the 64 before) give every lane its 'M' bit; only a k-mer's first entry can be
//               'M', so the 'M' entries in entry order are the set bits of that ballot in lane order.  The lanes compute their
//               five addends at once; the set bits are walked in order and the addends fetched with lane reads, five independent
//               chains of double additions.  The sums are taken before it is known whether the read has 200 'M' entries (fewer:
//               they are dropped).  A second walk adds the residuals for var.
//   (host)      the double var of every read comes to the host: log_var = (float)log(var) with libm.
//   cal_logvar  one thread per read: stores log_var.
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
constexpr int MIN_M_STATES = 200;                    // minNumEventsToRescale, align.c:679
static_assert(sizeof(gab_abea_calib) == 40 && sizeof(gab_abea_range) == 8, "record layout");

struct cal_counters { unsigned long long recalibrated, m_states; int32_t bad_read, pad; };
GAB_STATIC_ATOMIC64(cal_counters, recalibrated);
GAB_STATIC_ATOMIC64(cal_counters, m_states);

struct cal_reads {                 // the call's per-read arrays (device pointers)
    const char *seq; const int64_t *seq_off; const int32_t *seq_len;
    const float *event_mean; const int64_t *event_off; const int32_t *n_events;
    const float *scale, *shift;
    const gab_abea_pair *pairs; const int64_t *pair_off; const int32_t *n_pairs;
    gab_abea_range *map; const int64_t *map_off;
};

__device__ __forceinline__ int cal_rank(char c) { return c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 0; }

__global__ __launch_bounds__(256) void cal_check(cal_reads R, cal_counters *ctr) {
    const int r = blockIdx.x;
    const int n = R.n_pairs[r], n_kmers = R.seq_len[r] - K + 1, n_events = R.n_events[r];
    const gab_abea_pair *p = R.pairs + R.pair_off[r];
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += 256) {
        const gab_abea_pair a = p[i];
        bad |= a.ref_pos < 0 || a.ref_pos >= n_kmers || a.read_pos < 0 || a.read_pos >= n_events;
        if (i > 0) { const gab_abea_pair b = p[i - 1]; bad |= a.ref_pos < b.ref_pos || a.read_pos < b.read_pos; }
    }
    if (bad) atomicMin(&ctr->bad_read, r);
}

// the first index in [lo, hi) at which key(i) >= v (keys non-decreasing)
template <typename Key> __device__ __forceinline__ int cal_lower_bound(int lo, int hi, int v, Key key) {
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (key(mid) < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the base-to-event map, align.c:561-585
__global__ __launch_bounds__(256) void cal_map(cal_reads R) {
    const int r = blockIdx.x;
    const int n = R.n_pairs[r], n_kmers = R.seq_len[r] - K + 1;
    const gab_abea_pair *p = R.pairs + R.pair_off[r];
    auto ref = [&](int i) { return p[i].ref_pos; };
    auto ev = [&](int i) { return p[i].read_pos; };
    for (int64_t k64 = (int64_t)blockIdx.y * 256 + threadIdx.x; k64 < n_kmers; k64 += 256ll * gridDim.y) {
        const int k = (int)k64;
        gab_abea_range out = {-1, -1};
        const int s = cal_lower_bound(0, n, k, ref), t = cal_lower_bound(s, n, k + 1, ref);      // the k-mer's pairs: [s, t)
        if (s < t) {
            // the first pair of the segment whose event is not the event of the pair before it (pair 0 always is one: prev_event_idx = -1)
            int f = s;
            if (s > 0 && ev(s) == ev(s - 1)) f = cal_lower_bound(s + 1, t, ev(s) + 1, ev);
            if (f < t) { out.start = ev(f); out.stop = ev(t - 1); }      // pairs after the last such pair repeat its event
        }
        R.map[R.map_off[r] + k] = out;
    }
}

__device__ __forceinline__ double cal_lane(double v, int t) {      // lane t's v, t wave-uniform
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), t), __builtin_amdgcn_readlane(__double2loint(v), t));
}

// The event alignment of align.c:595-646, 64 k-mers at a time: f(m_bits, is_m, start, rank) with m_bits the ballot of the lanes
// whose k-mer's first entry is 'M' (every later entry of a k-mer is 'E': prev_kmer_rank is its own rank by then), start the
// lane's first event.  -> entries in all (n_alignment) as a per-lane partial count.
template <typename F> __device__ __forceinline__ int cal_walk(const gab_abea_range *m, const char *sq, int n_kmers, int lane, F f) {
    int carry = -1, entries = 0;                     // prev_kmer_rank before the first entry
    for (int base = 0; base < n_kmers; base += 64) {
        const int k = base + lane;
        gab_abea_range rg = {-1, -1};
        int rank = 0;
        if (k < n_kmers) {
            rg = m[k];
            for (int t = 0; t < K; t++) rank = (rank << 2) | cal_rank(sq[k + t]);
        }
        const bool has = rg.start != -1;
        const unsigned long long hb = __ballot(has);
        const unsigned long long below = hb & ((1ull << lane) - 1ull);
        const int from = __shfl(rank, below ? 63 - __builtin_clzll(below) : lane);
        const int prev = below ? from : carry;       // the rank of the previous k-mer that had events
        const bool is_m = has && rank != prev;
        f(__ballot(is_m), is_m, rg.start, rank);
        if (has) entries += rg.stop - rg.start + 1;
        if (hb) carry = __shfl(rank, 63 - __builtin_clzll(hb));
    }
    return entries;
}

__global__ __launch_bounds__(64) void cal_fit(cal_reads R, const float *level_mean, const float *level_stdv, gab_abea_calib *res, double *dvar,
                                              cal_counters *ctr) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int n = R.n_pairs[r], n_kmers = R.seq_len[r] - K + 1;
    gab_abea_calib c;
    c.n_alignment = 0; c.n_m_state = 0; c.read_stat_flag = 0; c.recalibrated = 0;
    c.scale = R.scale[r]; c.shift = R.shift[r]; c.var = 1.0f; c.log_var = 0.0f; c.events_per_base = 0.0;
    double var = 1.0;
    if (n == 0) {                                    // f5c.c:1484-1490; cal_map has written -1 / -1 everywhere
        c.read_stat_flag = GAB_ABEA_FAILED_ALIGNMENT;
        if (lane == 0) { res[r] = c; dvar[r] = var; }
        return;
    }
    const gab_abea_pair *p = R.pairs + R.pair_off[r];
    const gab_abea_range *m = R.map + R.map_off[r];
    const float *ev = R.event_mean + R.event_off[r];
    const char *sq = R.seq + R.seq_off[r];
    // non-decreasing, non-negative events: the minimum is the first pair's, the maximum (which starts from 0) the last pair's
    c.events_per_base = (double)(p[n - 1].read_pos - p[0].read_pos) / n_kmers;

    double A00 = 0, A01 = 0, A11 = 0, b0 = 0, b1 = 0;
    int n_m = 0;
    int entries = cal_walk(m, sq, n_kmers, lane, [&](unsigned long long mb, bool is_m, int start, int rank) {
        double a0 = 0, a1 = 0, a2 = 0, y0 = 0, y1 = 0;
        if (is_m) {                                  // align.c:697-710
            const double e = (double)ev[start], mu = (double)level_mean[rank], sd = (double)level_stdv[rank];
            const double inv_var = 1. / (sd * sd);
            a0 = inv_var; a1 = mu * inv_var; a2 = (mu * mu) * inv_var;
            y0 = e * inv_var; y1 = (mu * e) * inv_var;
        }
        n_m += __popcll(mb);
        while (mb) {
            const int t = __builtin_ctzll(mb);
            mb &= mb - 1;
            A00 += cal_lane(a0, t); A01 += cal_lane(a1, t); A11 += cal_lane(a2, t);
            b0 += cal_lane(y0, t); b1 += cal_lane(y1, t);
        }
    });
    for (int d = 32; d > 0; d >>= 1) entries += __shfl_xor(entries, d);
    c.n_alignment = entries; c.n_m_state = n_m;

    if (n_m >= MIN_M_STATES) {
        const double A10 = A01;
        const double div = A00 * A11 - A01 * A10;
        const double x0 = -(A01 * b1 - A11 * b0) / div;
        const double x1 = (A00 * b1 - A10 * b0) / div;
        var = 0.;
        cal_walk(m, sq, n_kmers, lane, [&](unsigned long long mb, bool is_m, int start, int rank) {
            double a = 0;
            if (is_m) {                              // align.c:732-737
                const double e = (double)ev[start], mu = (double)level_mean[rank], sd = (double)level_stdv[rank];
                const double yi = (e - x0) - x1 * mu;
                a = (yi * yi) / (sd * sd);
            }
            while (mb) {
                const int t = __builtin_ctzll(mb);
                mb &= mb - 1;
                var += cal_lane(a, t);
            }
        });
        var /= (double)n_m;
        var = sqrt(var);
        c.shift = (float)x0; c.scale = (float)x1; c.var = (float)var;
        c.recalibrated = 1;
    }
    // f5c.c:1474-1501: the first check that fails ends the read (`>` is false for a NaN)
    if (!c.recalibrated || (double)c.var > 2.5) c.read_stat_flag = GAB_ABEA_FAILED_CALIBRATION;
    else if (c.events_per_base > 5.0) c.read_stat_flag = GAB_ABEA_FAILED_QUALITY_CHK;
    if (lane == 0) {
        res[r] = c; dvar[r] = var;
        if (c.recalibrated) atomicAdd(&ctr->recalibrated, 1ull);
        atomicAdd(&ctr->m_states, (unsigned long long)n_m);
    }
}

__global__ __launch_bounds__(64) void cal_logvar(const float *log_var, int64_t n_reads, gab_abea_calib *res) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r < n_reads) res[r].log_var = log_var[r];
}

void cal_reset(gab_abea_calib_state &S) { S.reads = S.recalibrated = S.m_states = 0; S.kernel_ms = S.total_ms = 0.f; }

}  // namespace

gab_abea_calib_state::~gab_abea_calib_state() {
    io.release(); scratch.release();
    for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v);
}

extern "C" int gab_abea_calibrate_device(gab_abea *h, const char *seq, int64_t seq_bytes, const int64_t *seq_off, const int32_t *seq_len,
                                         const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events,
                                         const float *scale, const float *shift,
                                         const gab_abea_pair *pairs, int64_t pair_count, const int64_t *pair_off, const int32_t *n_pairs, int64_t n_reads,
                                         gab_abea_range *map, int64_t map_count, const int64_t *map_off, gab_abea_calib *res, void *stream) {
    if (!h) { gab_set_error("gab_abea_calibrate_device: NULL handle"); return GAB_EINVAL; }
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_calibrate_device: n_reads %lld out of range", (long long)n_reads);
    gab_abea_calib_state &S = h->calib;
    cal_reset(S);
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(seq && seq_off && seq_len && event_mean && event_off && n_events && scale && shift && (pairs || pair_count == 0) && pair_off && n_pairs &&
              map && map_off && res, "gab_abea_calibrate_device: NULL argument");
    gab_device_guard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)n_reads;
    for (hipEvent_t &v : S.ev) if (!v) GAB_HIP(hipEventCreate(&v));

    std::vector<int64_t> so(n), eo(n), po(n), mo(n); std::vector<int32_t> sl(n), ne(n), np(n);
    GAB_HIP(hipMemcpyAsync(so.data(), seq_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(eo.data(), event_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(po.data(), pair_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(mo.data(), map_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(sl.data(), seq_len, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(ne.data(), n_events, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(np.data(), n_pairs, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    int32_t max_kmers = 1;
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(sl[i] >= K && ne[i] >= 1, "gab_abea_calibrate: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, sl[i], K, ne[i]);
        const int64_t n_kmers = (int64_t)sl[i] - K + 1;
        GAB_CHECK(np[i] >= 0 && np[i] <= ne[i] + n_kmers, "gab_abea_calibrate: read %zu: n_pairs %d outside [0, n_events + n_kmers = %lld]", i, np[i], (long long)(ne[i] + n_kmers));
        GAB_CHECK(so[i] >= 0 && so[i] + sl[i] <= seq_bytes, "gab_abea_calibrate: read %zu: bases [%lld, +%d) outside the slab of %lld bytes", i, (long long)so[i], sl[i], (long long)seq_bytes);
        GAB_CHECK(eo[i] >= 0 && eo[i] + ne[i] <= event_count, "gab_abea_calibrate: read %zu: events [%lld, +%d) outside the slab of %lld", i, (long long)eo[i], ne[i], (long long)event_count);
        GAB_CHECK(po[i] >= 0 && po[i] + np[i] <= pair_count, "gab_abea_calibrate: read %zu: pairs [%lld, +%d) outside the slab of %lld", i, (long long)po[i], np[i], (long long)pair_count);
        GAB_CHECK(mo[i] >= 0 && mo[i] + n_kmers <= map_count, "gab_abea_calibrate: read %zu: map entries [%lld, +%lld) outside the slab of %lld", i, (long long)mo[i], (long long)n_kmers, (long long)map_count);
        max_kmers = std::max(max_kmers, (int32_t)n_kmers);
    }

    gab_stage_bump a;
    const size_t o_ctr = a.cursor(), o_var = a.a8(n), o_lv = a.a4(n);
    GAB_CHECK_ATOMIC64(o_ctr);
    int rc = S.scratch.reserve(a.o);
    if (rc) return rc;
    char *b = S.scratch.as<char>();
    cal_counters *dc = (cal_counters *)(b + o_ctr), ctr;
    double *dvar = (double *)(b + o_var);
    float *dlv = (float *)(b + o_lv);
    memset(&ctr, 0, sizeof ctr);
    ctr.bad_read = INT32_MAX;
    GAB_HIP(hipMemcpyAsync(dc, &ctr, sizeof ctr, hipMemcpyHostToDevice, s));

    const cal_reads R = {seq, seq_off, seq_len, event_mean, event_off, n_events, scale, shift, pairs, pair_off, n_pairs, map, map_off};
    GAB_HIP(hipEventRecord(S.ev[0], s));
    hipLaunchKernelGGL(cal_check, dim3((unsigned)n), dim3(256), 0, s, R, dc);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(S.ev[1], s));
    GAB_HIP(hipMemcpyAsync(&ctr, dc, sizeof ctr, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    GAB_CHECK(ctr.bad_read == INT32_MAX, "gab_abea_calibrate: read %d: a pair outside the read's k-mers or events, or not in non-decreasing order", ctr.bad_read);

    GAB_HIP(hipEventRecord(S.ev[2], s));
    hipLaunchKernelGGL(cal_map, dim3((unsigned)n, (unsigned)std::min<int64_t>(gab_ceil_div(max_kmers, 256), 64)), dim3(256), 0, s, R);
    hipLaunchKernelGGL(cal_fit, dim3((unsigned)n), dim3(64), 0, s, R, h->model.as<float>(), h->model.as<float>() + GAB_ABEA_NKMER, res, dvar, dc);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(S.ev[3], s));

    // log_var: the double log of the double var, on the host as the per-read constants of align() are (1.0 where not recalibrated: 0)
    std::vector<double> var(n); std::vector<float> lv(n);
    GAB_HIP(hipMemcpyAsync(var.data(), dvar, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(&ctr, dc, sizeof ctr, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++) lv[i] = (float)log(var[i]);
    GAB_HIP(hipMemcpyAsync(dlv, lv.data(), 4 * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(cal_logvar, dim3((unsigned)gab_ceil_div(n_reads, 64)), dim3(64), 0, s, dlv, n_reads, res);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(S.ev[4], s));
    GAB_HIP(hipStreamSynchronize(s));
    float check_ms = 0.f, fit_ms = 0.f;
    GAB_HIP(hipEventElapsedTime(&check_ms, S.ev[0], S.ev[1]));
    GAB_HIP(hipEventElapsedTime(&fit_ms, S.ev[2], S.ev[3]));
    GAB_HIP(hipEventElapsedTime(&S.total_ms, S.ev[0], S.ev[4]));
    S.kernel_ms = check_ms + fit_ms;
    S.reads = n_reads; S.recalibrated = (int64_t)ctr.recalibrated; S.m_states = (int64_t)ctr.m_states;
    return GAB_OK;
}

extern "C" int gab_abea_calibrate(gab_abea *h, const char *seq, const int64_t *seq_off, const int32_t *seq_len,
                                  const float *event_mean, const int64_t *event_off, const int32_t *n_events,
                                  const float *scale, const float *shift,
                                  const gab_abea_pair *pairs, const int64_t *pair_off, const int32_t *n_pairs, int64_t n_reads,
                                  gab_abea_range *map, const int64_t *map_off, gab_abea_calib *res) {
    if (!h) { gab_set_error("gab_abea_calibrate: NULL handle"); return GAB_EINVAL; }
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_calibrate: n_reads %lld out of range", (long long)n_reads);
    cal_reset(h->calib);
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(seq && seq_off && seq_len && event_mean && event_off && n_events && scale && shift && pair_off && n_pairs && map && map_off && res,
              "gab_abea_calibrate: NULL argument");
    const size_t n = (size_t)n_reads;
    // the windows of the three slabs that the reads refer to; the device call sees them re-based to the windows' starts, and the
    // maps back to back
    int64_t sa = INT64_MAX, sb = 0, ea = INT64_MAX, eb = 0, pa = INT64_MAX, pb = 0, M = 0;
    std::vector<int64_t> so(n), eo(n), po(n), mo(n);
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(seq_len[i] >= K && n_events[i] >= 1, "gab_abea_calibrate: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, seq_len[i], K, n_events[i]);
        const int64_t n_kmers = (int64_t)seq_len[i] - K + 1;
        GAB_CHECK(n_pairs[i] >= 0 && n_pairs[i] <= n_events[i] + n_kmers, "gab_abea_calibrate: read %zu: n_pairs %d outside [0, n_events + n_kmers = %lld]", i, n_pairs[i], (long long)(n_events[i] + n_kmers));
        GAB_CHECK(seq_off[i] >= 0 && event_off[i] >= 0 && pair_off[i] >= 0 && map_off[i] >= 0, "gab_abea_calibrate: read %zu: negative offset", i);
        GAB_CHECK(pairs || n_pairs[i] == 0, "gab_abea_calibrate: NULL argument");
        sa = std::min(sa, seq_off[i]); sb = std::max(sb, seq_off[i] + seq_len[i]);
        ea = std::min(ea, event_off[i]); eb = std::max(eb, event_off[i] + n_events[i]);
        if (n_pairs[i]) { pa = std::min(pa, pair_off[i]); pb = std::max(pb, pair_off[i] + n_pairs[i]); }
        mo[i] = M; M += n_kmers;
    }
    if (pb == 0) pa = 0;                             // no read has a pair
    for (size_t i = 0; i < n; i++) { so[i] = seq_off[i] - sa; eo[i] = event_off[i] - ea; po[i] = n_pairs[i] ? pair_off[i] - pa : 0; }
    gab_device_guard g(h->device);
    hipStream_t s = nullptr;
    int rc = h->hs.get(&s);
    if (rc) return rc;
    gab_stage_bump a;
    const size_t o_seq = a.region(gab_pad256((size_t)(sb - sa))), o_ev = a.region(4 * (size_t)(eb - ea)), o_pairs = a.region(sizeof(gab_abea_pair) * (size_t)(pb - pa));
    const size_t o_map = a.region(sizeof(gab_abea_range) * (size_t)M), o_res = a.region(sizeof(gab_abea_calib) * n);
    const size_t o_so = a.a8(n), o_eo = a.a8(n), o_po = a.a8(n), o_mo = a.a8(n), o_sl = a.a4(n), o_ne = a.a4(n), o_np = a.a4(n), o_sc = a.a4(n), o_sh = a.a4(n);
    if ((rc = h->calib.io.reserve(a.o)) != GAB_OK) return rc;
    char *b = h->calib.io.as<char>();
    {
        std::lock_guard<std::mutex> gate(gab_h2d_mutex(h->device));
        GAB_HIP(hipMemcpyAsync(b + o_seq, seq + sa, (size_t)(sb - sa), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_ev, event_mean + ea, 4 * (size_t)(eb - ea), hipMemcpyHostToDevice, s));
        if (pb > pa) GAB_HIP(hipMemcpyAsync(b + o_pairs, pairs + pa, sizeof(gab_abea_pair) * (size_t)(pb - pa), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_so, so.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_eo, eo.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_po, po.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_mo, mo.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_sl, seq_len, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_ne, n_events, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_np, n_pairs, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_sc, scale, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_sh, shift, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    rc = gab_abea_calibrate_device(h, b + o_seq, sb - sa, (const int64_t *)(b + o_so), (const int32_t *)(b + o_sl), (const float *)(b + o_ev), eb - ea,
                                   (const int64_t *)(b + o_eo), (const int32_t *)(b + o_ne), (const float *)(b + o_sc), (const float *)(b + o_sh),
                                   (const gab_abea_pair *)(b + o_pairs), pb - pa, (const int64_t *)(b + o_po), (const int32_t *)(b + o_np), n_reads,
                                   (gab_abea_range *)(b + o_map), M, (const int64_t *)(b + o_mo), (gab_abea_calib *)(b + o_res), s);
    if (rc) return rc;
    GAB_HIP(hipMemcpy(res, b + o_res, sizeof(gab_abea_calib) * n, hipMemcpyDeviceToHost));
    std::vector<gab_abea_range> all;
    try { all.resize((size_t)M); } catch (...) { gab_set_error("gab_abea_calibrate: out of host memory"); return GAB_ENOMEM; }
    GAB_HIP(hipMemcpy(all.data(), b + o_map, sizeof(gab_abea_range) * all.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) memcpy(map + map_off[i], all.data() + mo[i], sizeof(gab_abea_range) * (size_t)(seq_len[i] - K + 1));
    return GAB_OK;
}

extern "C" int gab_abea_calibrate_last_stats(gab_abea *h, int64_t *reads, int64_t *recalibrated, int64_t *m_states, float *kernel_ms, float *total_ms) {
    if (!h) { gab_set_error("gab_abea_calibrate_last_stats: NULL handle"); return GAB_EINVAL; }
    if (reads) *reads = h->calib.reads;
    if (recalibrated) *recalibrated = h->calib.recalibrated;
    if (m_states) *m_states = h->calib.m_states;
    if (kernel_ms) *kernel_ms = h->calib.kernel_ms;
    if (total_ms) *total_ms = h->calib.total_ms;
    return GAB_OK;
}
