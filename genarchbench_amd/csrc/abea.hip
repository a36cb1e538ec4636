// abea: adaptive banded event alignment, align() of abea/src/align.c:169-548, behind gab_abea_* (include/gab.h).
//
// Arithmetic: the reference's as built without fused multiply-add.  hipcc contracts a * b + c by default; the pragma below
// stops that for this file (the Makefile's flags stay as they are), so every fp32 / fp64 operation rounds on its own.  The
// only FMAs left in the code object are those of the IEEE division sequence, which is correctly rounded.
//
// Shape (DESIGN.md, section "abea"):
//   abea_prep       one block per read: the scaled model entry of every k-mer of the read, {scale * mean + shift, stdv, log stdv}
//   abea_dp         one wavefront per read.  Lane l holds cells l and l + 64 of the 100-cell band; three rolling bands live in
//                   LDS behind -inf guard cells, so the up / left / diagonal reads need no bounds test.  The serial chain is
//                   one band decision per band (cells 0 and 99 of the previous band).  Per band 32 bytes go to global memory:
//                   the 2-bit `from` of the 100 cells as four 64-bit ballots, the move bit (right = 1) in bit 63 of the third.
//                   The end-cell scan of align.c:418-434 runs along with the sweep, in event order, so its tie rule holds.
//   abea_backtrack  one wavefront per read: 64 band records at a time into LDS, a uniform walk over them (the lower-left
//                   corner of a band is counted back down from the move bits), then the emission sum in double in backtrack
//                   order, the move of the path to the front of the read's room, the quality checks.
// The host side sorts the reads by band count (longest first, so that the tail of a launch is short reads) and cuts the call
// into launches whose traces fit GAB_ABEA_TRACE_BYTES.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>
#include "gab_internal.h"
#include "gab_pair_stage.h"
#include "abea_handle.h"

#pragma clang fp contract(off)

namespace {

constexpr int K = GAB_ABEA_K, BW = GAB_ABEA_BANDWIDTH;
constexpr int FROM_D = 0, FROM_U = 1, FROM_L = 2;
constexpr int REC_WORDS = 4;                                   // 64-bit words of a band's trace record
constexpr long long DEFAULT_TRACE_BYTES = 4ll << 30;
#define ABEA_NEG_INF (-__builtin_inff())

struct abea_job {                  // one read of a launch, in launch order
    int64_t seq_off, ev_off, pair_off;
    int64_t kp_off;                // into the launch's k-mer entries
    int64_t trace_off;             // into the launch's trace, in band records
    int32_t n_kmers, n_events, read, pad;
    float scale, shift;
    double lp_skip, lp_stay, lp_step, lp_trim;
};
struct abea_end {                  // what the sweep leaves for the backtrack
    float best; int32_t end_event, end_k, pad;      // end_k: k-mer index of the lower-left corner of the end cell's band
    int64_t fills;
};

__device__ __forceinline__ int abea_rank(char c) { return c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 0; }

// log_normal_pdf of align.c:99-106 on the scaled model entry: every operation rounds to fp32
__device__ __forceinline__ float abea_emission(float ev, float4 kp) {
    const float a = (ev - kp.x) / kp.y;
    return (-0.918938f - kp.z) + ((-0.5f * a) * a);
}

__global__ __launch_bounds__(256) void abea_prep(const abea_job *jobs, const char *seq, const float *mean, const float *stdv, const float *log_stdv,
                                                 float4 *kparam) {
    const abea_job j = jobs[blockIdx.x];
    const char *s = seq + j.seq_off;
    for (int i = threadIdx.x; i < j.n_kmers; i += blockDim.x) {
        int r = 0;
        for (int t = 0; t < K; t++) r = (r << 2) | abea_rank(s[i + t]);
        const float gp_mean = j.scale * mean[r] + j.shift;
        kparam[j.kp_off + i] = make_float4(gp_mean, stdv[r], log_stdv[r], 0.f);
    }
}

__global__ __launch_bounds__(64) void abea_dp(const abea_job *jobs, const float *events, const float4 *kparam, uint64_t *trace, abea_end *ends) {
    __shared__ float sb[3][BW + 4];                  // cell o of a band at [o + 1]; [0] and [BW + 1] stay -inf
    __shared__ unsigned long long s_fills;
    const abea_job j = jobs[blockIdx.x];
    const int lane = threadIdx.x;
    const int n_events = j.n_events, n_kmers = j.n_kmers;
    const float *ev = events + j.ev_off;
    const float4 *kp = kparam + j.kp_off;
    uint64_t *tr = trace + j.trace_off * REC_WORDS;

    for (int i = lane; i < 3 * (BW + 4); i += 64) (&sb[0][0])[i] = ABEA_NEG_INF;
    if (lane == 0) s_fills = 0;
    __syncthreads();
    if (lane == 0) {
        sb[0][1 + BW / 2] = 0.0f;                    // the start cell, event -1 x k-mer -1
        sb[1][1 + BW / 2] = (float)j.lp_trim;        // band 1: the first event trimmed
    }
    __syncthreads();

    int E = BW / 2, Kll = -1 - BW / 2;               // lower-left corner of band 1 (align.c:266-268)
    int rprev = 0;                                   // the move into the previous band
    unsigned fills = 0;
    float best = ABEA_NEG_INF; int best_e = 0, best_k = 0;
    const int n_bands = n_events + n_kmers + 2;
    int p = 1, pp = 0, c = 2;
    for (int b = 2; b < n_bands; b++) {
        // Suzuki's rule on the two end cells of the previous band (align.c:293-311)
        const float ll = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sb[p][1])));
        const float ur = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sb[p][BW])));
        const bool right = (ll == ABEA_NEG_INF && ur == ABEA_NEG_INF) ? (b & 1) : (ll < ur);
        if (right) Kll++; else E++;
        const int dup = right ? 1 : 0, dleft = right ? 0 : -1, ddiag = (right ? 1 : 0) + rprev - 1;
        float val[2]; int from[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int o = lane + 64 * h;
            float v = ABEA_NEG_INF; int f = 0;
            if (o < BW) {
                const int e = E - o, k = Kll + o;
                const bool e_in = e >= 0 && e < n_events;
                if (k == -1) {                       // the trim column
                    if (e_in) { v = (float)(j.lp_trim * (double)(e + 1)); f = FROM_U; }
                } else if (e_in && k >= 0 && k < n_kmers) {
                    const float up = sb[p][1 + o + dup], left = sb[p][1 + o + dleft], diag = sb[pp][1 + o + ddiag];
                    const float lp = abea_emission(ev[e], kp[k]);
                    const float sd = (float)(((double)diag + j.lp_step) + (double)lp);
                    const float su = (float)(((double)up + j.lp_stay) + (double)lp);
                    const float sl = (float)((double)left + j.lp_skip);
                    v = sd; f = FROM_D;              // the reference's own sequence (align.c:375-381): all -inf gives FROM_L
                    v = su > v ? su : v; f = (v == su) ? FROM_U : f;
                    v = sl > v ? sl : v; f = (v == sl) ? FROM_L : f;
                    fills++;
                }
            }
            val[h] = v; from[h] = f;
        }
        sb[c][1 + lane] = val[0];
        if (lane + 64 < BW) sb[c][1 + lane + 64] = val[1];
        const uint64_t w0 = __ballot(from[0] & 1), w1 = __ballot(from[0] & 2);
        const uint64_t w2 = __ballot(from[1] & 1) | ((uint64_t)(right ? 1 : 0) << 63), w3 = __ballot(from[1] & 2);
        if (lane < REC_WORDS) tr[(int64_t)b * REC_WORDS + lane] = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? w2 : w3;
        __syncthreads();
        // the end cell of this band's event, if the last k-mer is inside the band (align.c:418-434)
        const int e_end = b - 1 - n_kmers, o_end = n_kmers - 1 - Kll;
        if (e_end >= 0 && o_end >= 0 && o_end < BW) {
            const float cell = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sb[c][1 + o_end])));
            const float s = (float)((double)cell + (double)(n_events - e_end) * j.lp_trim);
            if (s > best) { best = s; best_e = e_end; best_k = Kll; }
        }
        rprev = right ? 1 : 0;
        const int t = pp; pp = p; p = c; c = t;
    }
    atomicAdd(&s_fills, (unsigned long long)fills);
    __syncthreads();
    if (lane == 0) {
        abea_end r; r.best = best; r.end_event = best_e; r.end_k = best_k; r.pad = 0; r.fills = (int64_t)s_fills;
        ends[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(64) void abea_backtrack(const abea_job *jobs, const float *events, const float4 *kparam, const uint64_t *trace,
                                                     const abea_end *ends, gab_abea_pair *pairs, gab_abea_read *res) {
    __shared__ uint64_t rec[64][REC_WORDS];
    const abea_job j = jobs[blockIdx.x];
    const abea_end end = ends[blockIdx.x];
    const int lane = threadIdx.x;
    gab_abea_read out; memset(&out, 0, sizeof out);
    out.fills = end.fills;
    if (end.best == ABEA_NEG_INF) {                  // no event has the last k-mer inside its band
        out.flags = GAB_ABEA_NO_END;
        if (lane == 0) res[j.read] = out;
        return;
    }
    const uint64_t *tr = trace + j.trace_off * REC_WORDS;
    const float *ev = events + j.ev_off;
    const float4 *kp = kparam + j.kp_off;
    gab_abea_pair *room = pairs + j.pair_off;
    const int cap = j.n_events + j.n_kmers;          // the path has at most cap - 1 pairs; it is written from the top of the room down

    int e = end.end_event, k = j.n_kmers - 1, b = e + k + 2, Kll = end.end_k;
    int lo = -(1 << 30);                            // the records in LDS are those of bands lo .. lo + 63
    int len = 0, gap = 0, max_gap = 0;
    while (k >= 0 && e >= 0) {
        if (b > lo + 63 || b < lo || (b == lo && b > 2)) {    // band b, and b - 1 for a diagonal step, must be in LDS
            __syncthreads();
            lo = b - 63 > 0 ? b - 63 : 0;
            const int mine = lo + lane;
#pragma unroll
            for (int w = 0; w < REC_WORDS; w++) rec[lane][w] = (mine >= 2 && mine <= b) ? tr[(int64_t)mine * REC_WORDS + w] : 0;
            __syncthreads();
        }
        if (lane == 0) { room[cap - 1 - len].ref_pos = k; room[cap - 1 - len].read_pos = e; }
        len++;
        const int o = k - Kll, h = (o >> 6) & 1, sh = o & 63;
        const int from = (int)((rec[b - lo][2 * h] >> sh) & 1) | ((int)((rec[b - lo][2 * h + 1] >> sh) & 1) << 1);
        const int right_b = (int)(rec[b - lo][2] >> 63);
        if (from == FROM_D) {
            const int right_b1 = b - 1 >= lo ? (int)(rec[b - 1 - lo][2] >> 63) : 0;
            k--; e--; Kll -= right_b + right_b1; b -= 2; gap = 0;
        } else if (from == FROM_U) {
            e--; Kll -= right_b; b -= 1; gap = 0;
        } else {
            k--; Kll -= right_b; b -= 1; gap++; max_gap = gap > max_gap ? gap : max_gap;
        }
    }
    __threadfence();
    __syncthreads();

    // sum of the path's emissions, in double, in backtrack order (align.c:462-465)
    double sum = 0.0;
    for (int base = 0; base < len; base += 64) {
        const int i = base + lane;
        float lp = 0.f;
        if (i < len) { const gab_abea_pair pr = room[cap - 1 - i]; lp = abea_emission(ev[pr.read_pos], kp[pr.ref_pos]); }
        const int n = len - base < 64 ? len - base : 64;
        for (int t = 0; t < n; t++) sum += (double)__shfl(lp, t);
    }
    const int first_ref = room[cap - len].ref_pos;
    // the path, now in read order at the top of the room, moves to its front: a chunk is loaded before it is stored, and a
    // later chunk reads above everything stored so far
    const int shift = cap - len;
    for (int base = 0; base < len; base += 64) {
        const int i = base + lane;
        gab_abea_pair pr = {0, 0};
        if (i < len) pr = room[shift + i];
        __syncthreads();
        if (i < len) room[i] = pr;
    }
    out.path_len = len; out.end_event = end.end_event; out.max_gap = max_gap;
    out.avg_log_emission = sum / (double)len;
    if (out.avg_log_emission < -5.0) out.flags |= GAB_ABEA_LOW_EMISSION;
    if (first_ref != 0) out.flags |= GAB_ABEA_NOT_SPANNED;      // (the last pair's k-mer is the last one by construction)
    if (max_gap > 50) out.flags |= GAB_ABEA_GAP;
    out.n_pairs = out.flags ? 0 : len;
    if (lane == 0) res[j.read] = out;
}

}  // namespace

// struct gab_abea: abea_handle.h (shared with abea_events.hip)

extern "C" int gab_abea_create(int device, const float *level_mean, const float *level_stdv, const float *level_log_stdv, gab_abea **out) {
    if (!out || !level_mean || !level_stdv) { gab_set_error("gab_abea_create: NULL argument"); return GAB_EINVAL; }
    *out = nullptr;
    for (int i = 0; i < GAB_ABEA_NKMER; i++)
        GAB_CHECK(level_stdv[i] > 0.f && level_stdv[i] == level_stdv[i] && level_mean[i] == level_mean[i], "gab_abea_create: model entry %d: stdv must be positive, mean a number", i);
    int rc = gab_check_device(device);
    if (rc) return rc;
    gab_device_guard g(device);
    gab_abea *h = new (std::nothrow) gab_abea();
    if (!h) { gab_set_error("out of host memory"); return GAB_ENOMEM; }
    h->device = device;
    std::vector<float> m(3 * GAB_ABEA_NKMER);
    for (int i = 0; i < GAB_ABEA_NKMER; i++) {
        m[i] = level_mean[i]; m[GAB_ABEA_NKMER + i] = level_stdv[i];
        m[2 * GAB_ABEA_NKMER + i] = level_log_stdv ? level_log_stdv[i] : (float)log(level_stdv[i]);      // model.c:53: double log of the float
    }
    rc = h->model.reserve(m.size() * sizeof(float));
    if (rc == GAB_OK) {
        hipError_t e = hipMemcpy(h->model.p, m.data(), m.size() * sizeof(float), hipMemcpyHostToDevice);
        for (hipEvent_t &v : h->ev) if (e == hipSuccess) e = hipEventCreate(&v);
        if (e != hipSuccess) { gab_set_error("gab_abea_create: %s", hipGetErrorString(e)); rc = GAB_EDEVICE; }
    }
    if (rc) { gab_abea_destroy(h); return rc; }
    *out = h;
    return GAB_OK;
}

extern "C" void gab_abea_destroy(gab_abea *h) {
    if (!h) return;
    gab_device_guard g(h->device);
    for (gab_devbuf *b : {&h->model, &h->io, &h->jobs, &h->ends, &h->kparam, &h->trace}) b->release();
    for (hipEvent_t v : h->ev) if (v) (void)hipEventDestroy(v);
    h->hs.release();
    delete h;
}

namespace {
struct abea_io_layout { size_t seq, ev, pairs, res, so, eo, po, sl, ne, sc, sh, bytes; };
abea_io_layout abea_layout(size_t seq_bytes, size_t n_ev, size_t n_pairs, size_t n) {
    gab_stage_bump a; abea_io_layout L;
    L.seq = a.region(gab_pad256(seq_bytes)); L.ev = a.region(4 * n_ev); L.pairs = a.region(sizeof(gab_abea_pair) * n_pairs);
    L.res = a.region(sizeof(gab_abea_read) * n);
    L.so = a.a8(n); L.eo = a.a8(n); L.po = a.a8(n); L.sl = a.a4(n); L.ne = a.a4(n); L.sc = a.a4(n); L.sh = a.a4(n);
    L.bytes = a.o;
    return L;
}
}  // namespace

extern "C" int gab_abea_reserve(gab_abea *h, int64_t max_reads, int64_t max_bases, int64_t max_events) {
    if (!h) { gab_set_error("gab_abea_reserve: NULL handle"); return GAB_EINVAL; }
    GAB_CHECK(max_reads >= 0 && max_bases >= 0 && max_events >= 0, "gab_abea_reserve: negative size");
    gab_device_guard g(h->device);
    int rc = h->io.reserve(abea_layout((size_t)max_bases + 256, (size_t)max_events, (size_t)(max_events + max_bases), (size_t)max_reads).bytes + 2048);
    if (rc == GAB_OK) rc = h->jobs.reserve(sizeof(abea_job) * (size_t)max_reads);
    if (rc == GAB_OK) rc = h->ends.reserve(sizeof(abea_end) * (size_t)max_reads);
    if (rc == GAB_OK) rc = h->kparam.reserve(sizeof(float4) * (size_t)max_bases);
    return rc;
}

extern "C" int gab_abea_align_device(gab_abea *h, const char *seq, int64_t seq_bytes, const int64_t *seq_off, const int32_t *seq_len,
                                     const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events,
                                     const float *scale, const float *shift, int64_t n_reads,
                                     gab_abea_pair *pairs, int64_t pair_count, const int64_t *pair_off, gab_abea_read *res, void *stream) {
    if (!h) { gab_set_error("gab_abea_align_device: NULL handle"); return GAB_EINVAL; }
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_align_device: n_reads %lld out of range", (long long)n_reads);
    h->cells = h->bands = h->launches = 0; h->kernel_ms = h->total_ms = 0.f;
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(seq && seq_off && seq_len && event_mean && event_off && n_events && scale && shift && pairs && pair_off && res,
              "gab_abea_align_device: NULL argument");
    gab_tuning_refresh(&h->tune);
    gab_device_guard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)n_reads;

    // the lengths, offsets and scalings come to the host: the launch plan and the per-read constants are made here
    std::vector<int64_t> so(n), eo(n), po(n); std::vector<int32_t> sl(n), ne(n); std::vector<float> sc(n), sh(n);
    GAB_HIP(hipMemcpyAsync(so.data(), seq_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(eo.data(), event_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(po.data(), pair_off, 8 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(sl.data(), seq_len, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(ne.data(), n_events, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(sc.data(), scale, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(sh.data(), shift, 4 * n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));

    std::vector<int32_t> order(n);
    int64_t bands = 0;
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(sl[i] >= K && ne[i] >= 1, "gab_abea_align: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, sl[i], K, ne[i]);
        const int64_t room = (int64_t)ne[i] + sl[i] - K + 1;
        GAB_CHECK(room + 2 <= INT32_MAX, "gab_abea_align: read %zu: %lld bands do not fit 32 bits", i, (long long)room + 2);
        GAB_CHECK(so[i] >= 0 && so[i] + sl[i] <= seq_bytes, "gab_abea_align: read %zu: bases [%lld, +%d) outside the slab of %lld bytes", i, (long long)so[i], sl[i], (long long)seq_bytes);
        GAB_CHECK(eo[i] >= 0 && eo[i] + ne[i] <= event_count, "gab_abea_align: read %zu: events [%lld, +%d) outside the slab of %lld", i, (long long)eo[i], ne[i], (long long)event_count);
        GAB_CHECK(po[i] >= 0 && po[i] + room <= pair_count, "gab_abea_align: read %zu: %lld pairs of room at %lld outside the slab of %lld", i, (long long)room, (long long)po[i], (long long)pair_count);
        order[i] = (int32_t)i; bands += room + 2;
    }
    auto n_bands = [&](int32_t i) { return (int64_t)ne[i] + sl[i] - K + 3; };
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return n_bands(a) > n_bands(b); });

    // the jobs of all launches, and where each launch starts: a launch takes reads while their traces fit the budget (one at least)
    const int64_t budget_recs = std::max<long long>(h->tune.abea_trace_bytes > 0 ? h->tune.abea_trace_bytes : DEFAULT_TRACE_BYTES, 1) / (8 * REC_WORDS);
    std::vector<abea_job> jobs(n); std::vector<size_t> cut{0};
    int64_t recs = 0, kps = 0, max_recs = 0, max_kps = 0;
    for (size_t q = 0; q < n; q++) {
        const int32_t i = order[q];
        if (q > cut.back() && recs + n_bands(i) > budget_recs) { cut.push_back(q); recs = kps = 0; }
        abea_job &j = jobs[q];
        j.seq_off = so[i]; j.ev_off = eo[i]; j.pair_off = po[i]; j.kp_off = kps; j.trace_off = recs;
        j.n_kmers = sl[i] - K + 1; j.n_events = ne[i]; j.read = i; j.pad = 0; j.scale = sc[i]; j.shift = sh[i];
        const double events_per_kmer = (double)j.n_events / j.n_kmers, p_stay = 1 - (1 / (events_per_kmer + 1));      // align.c:196-205
        j.lp_skip = log(1e-10); j.lp_stay = log(p_stay); j.lp_step = log(1.0 - exp(j.lp_skip) - exp(j.lp_stay)); j.lp_trim = log(0.01);
        recs += n_bands(i); kps += j.n_kmers;
        max_recs = std::max(max_recs, recs); max_kps = std::max(max_kps, kps);
    }
    cut.push_back(n);

    int rc = h->jobs.reserve(sizeof(abea_job) * n);
    if (rc == GAB_OK) rc = h->ends.reserve(sizeof(abea_end) * n);
    if (rc == GAB_OK) rc = h->kparam.reserve(sizeof(float4) * (size_t)max_kps);
    if (rc == GAB_OK) rc = h->trace.reserve(8 * REC_WORDS * (size_t)max_recs);
    if (rc) return rc;
    GAB_HIP(hipMemcpyAsync(h->jobs.p, jobs.data(), sizeof(abea_job) * n, hipMemcpyHostToDevice, s));
    const float *mean = h->model.as<float>(), *stdv = mean + GAB_ABEA_NKMER, *lstd = stdv + GAB_ABEA_NKMER;
    float dp_ms = 0.f, all_ms = 0.f;
    for (size_t c = 0; c + 1 < cut.size(); c++) {
        const abea_job *dj = h->jobs.as<abea_job>() + cut[c];
        abea_end *de = h->ends.as<abea_end>() + cut[c];
        const unsigned blocks = (unsigned)(cut[c + 1] - cut[c]);
        GAB_HIP(hipEventRecord(h->ev[0], s));
        hipLaunchKernelGGL(abea_prep, dim3(blocks), dim3(256), 0, s, dj, seq, mean, stdv, lstd, h->kparam.as<float4>());
        GAB_HIP(hipEventRecord(h->ev[1], s));
        hipLaunchKernelGGL(abea_dp, dim3(blocks), dim3(64), 0, s, dj, event_mean, h->kparam.as<float4>(), h->trace.as<uint64_t>(), de);
        GAB_HIP(hipEventRecord(h->ev[2], s));
        hipLaunchKernelGGL(abea_backtrack, dim3(blocks), dim3(64), 0, s, dj, event_mean, h->kparam.as<float4>(), h->trace.as<uint64_t>(), de, pairs, res);
        GAB_HIP(hipGetLastError());
        GAB_HIP(hipEventRecord(h->ev[3], s));
        // the four events are recorded again by the next launch: read them here (the stream's order already keeps that launch's
        // kernels behind this one's use of the trace and the k-mer entries)
        GAB_HIP(hipEventSynchronize(h->ev[3]));
        float a = 0.f, b2 = 0.f;
        GAB_HIP(hipEventElapsedTime(&a, h->ev[1], h->ev[2]));
        GAB_HIP(hipEventElapsedTime(&b2, h->ev[0], h->ev[3]));
        dp_ms += a; all_ms += b2;
    }
    GAB_HIP(hipStreamSynchronize(s));
    std::vector<abea_end> ends(n);
    GAB_HIP(hipMemcpy(ends.data(), h->ends.p, sizeof(abea_end) * n, hipMemcpyDeviceToHost));
    for (const abea_end &e : ends) h->cells += e.fills;
    h->bands = bands; h->launches = (int64_t)cut.size() - 1; h->kernel_ms = dp_ms; h->total_ms = all_ms;
    return GAB_OK;
}

extern "C" int gab_abea_align(gab_abea *h, const char *seq, const int64_t *seq_off, const int32_t *seq_len,
                              const float *event_mean, const int64_t *event_off, const int32_t *n_events,
                              const float *scale, const float *shift, int64_t n_reads,
                              gab_abea_pair *pairs, const int64_t *pair_off, gab_abea_read *res) {
    if (!h) { gab_set_error("gab_abea_align: NULL handle"); return GAB_EINVAL; }
    GAB_CHECK(n_reads >= 0 && n_reads <= INT32_MAX, "gab_abea_align: n_reads %lld out of range", (long long)n_reads);
    h->cells = h->bands = h->launches = 0; h->kernel_ms = h->total_ms = 0.f;
    if (n_reads == 0) return GAB_OK;
    GAB_CHECK(seq && seq_off && seq_len && event_mean && event_off && n_events && scale && shift && pairs && pair_off && res,
              "gab_abea_align: NULL argument");
    const size_t n = (size_t)n_reads;
    // the windows of the three slabs that the reads refer to; the device call sees them re-based to the windows' starts
    int64_t sa = INT64_MAX, sb = 0, ea = INT64_MAX, eb = 0, pa = INT64_MAX, pb = 0;
    for (size_t i = 0; i < n; i++) {
        GAB_CHECK(seq_len[i] >= K && n_events[i] >= 1, "gab_abea_align: read %zu: seq_len %d (>= %d) and n_events %d (>= 1) needed", i, seq_len[i], K, n_events[i]);
        GAB_CHECK(seq_off[i] >= 0 && event_off[i] >= 0 && pair_off[i] >= 0, "gab_abea_align: read %zu: negative offset", i);
        const int64_t room = (int64_t)n_events[i] + seq_len[i] - K + 1;
        sa = std::min(sa, seq_off[i]); sb = std::max(sb, seq_off[i] + seq_len[i]);
        ea = std::min(ea, event_off[i]); eb = std::max(eb, event_off[i] + n_events[i]);
        pa = std::min(pa, pair_off[i]); pb = std::max(pb, pair_off[i] + room);
    }
    gab_device_guard g(h->device);
    hipStream_t s = nullptr;
    int rc = h->hs.get(&s);
    if (rc) return rc;
    const abea_io_layout L = abea_layout((size_t)(sb - sa), (size_t)(eb - ea), (size_t)(pb - pa), n);
    if ((rc = h->io.reserve(L.bytes)) != GAB_OK) return rc;
    char *b = h->io.as<char>();
    std::vector<int64_t> so(n), eo(n), po(n);
    for (size_t i = 0; i < n; i++) { so[i] = seq_off[i] - sa; eo[i] = event_off[i] - ea; po[i] = pair_off[i] - pa; }
    {
        std::lock_guard<std::mutex> gate(gab_h2d_mutex(h->device));
        GAB_HIP(hipMemcpyAsync(b + L.seq, seq + sa, (size_t)(sb - sa), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.ev, event_mean + ea, 4 * (size_t)(eb - ea), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.so, so.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.eo, eo.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.po, po.data(), 8 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.sl, seq_len, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.ne, n_events, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.sc, scale, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.sh, shift, 4 * n, hipMemcpyHostToDevice, s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    rc = gab_abea_align_device(h, b + L.seq, sb - sa, (const int64_t *)(b + L.so), (const int32_t *)(b + L.sl), (const float *)(b + L.ev), eb - ea,
                               (const int64_t *)(b + L.eo), (const int32_t *)(b + L.ne), (const float *)(b + L.sc), (const float *)(b + L.sh), n_reads,
                               (gab_abea_pair *)(b + L.pairs), pb - pa, (const int64_t *)(b + L.po), (gab_abea_read *)(b + L.res), s);
    if (rc) return rc;
    // the records, then of the pairs' window only each read's own path: the caller's memory between the paths is not touched
    GAB_HIP(hipMemcpy(res, b + L.res, sizeof(gab_abea_read) * n, hipMemcpyDeviceToHost));
    std::vector<gab_abea_pair> win;
    try { win.resize((size_t)(pb - pa)); } catch (...) { gab_set_error("gab_abea_align: out of host memory"); return GAB_ENOMEM; }
    GAB_HIP(hipMemcpy(win.data(), b + L.pairs, sizeof(gab_abea_pair) * win.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) memcpy(pairs + pair_off[i], win.data() + po[i], sizeof(gab_abea_pair) * (size_t)res[i].path_len);
    return GAB_OK;
}

extern "C" int gab_abea_last_stats(gab_abea *h, int64_t *cells, int64_t *bands, int64_t *launches, float *kernel_ms, float *total_ms) {
    if (!h) { gab_set_error("gab_abea_last_stats: NULL handle"); return GAB_EINVAL; }
    if (cells) *cells = h->cells;
    if (bands) *bands = h->bands;
    if (launches) *launches = h->launches;
    if (kernel_ms) *kernel_ms = h->kernel_ms;
    if (total_ms) *total_ms = h->total_ms;
    return GAB_OK;
}
