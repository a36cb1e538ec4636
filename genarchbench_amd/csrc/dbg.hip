// dbg: Platypus' local-assembly de Bruijn graph, one work-group per assembly region (include/gab.h, dbg section).
//
// A region's graph is two open-addressing tables in global memory: nodes keyed by the k-mer (k <= 16 letters of 4 bits: one
// 64-bit word) and edges keyed by (node slot, next letter).  Every edge occurrence has its index t in the reference's own order
// (the reference's edges first, then the reads' by a prefix sum over the reads); its two node occurrences are 2t and 2t + 1.  A
// table entry keeps atomicMin of that index beside atomicAdd of the weight and atomicOr of the colour, so nothing depends on the
// order in which the atomics land.  Nodes are numbered by a prefix sum over "this occurrence is its node's first" (a bit map over
// the occurrence indices), a node's successors are ordered by their own first occurrence and the four earliest kept.
// Four launches, so that every phase reads what the one before wrote across a kernel boundary:
//   dg_insert   tables filled, bytes validated         dg_mark    first occurrences into the bit map
//   dg_scan     prefix popcounts, nodes per region      dg_emit    the records, into the caller's array
#include "gab_internal.h"
#include "gab_pair_stage.h"
#include <string.h>
#include <algorithm>
#include <vector>

namespace {

constexpr int DG_BLOCK = 256, DG_GROUP = 64;          // a read is walked by 64 consecutive threads (plain arithmetic, no wave intrinsics)
constexpr unsigned long long DG_EMPTY64 = ~0ull;      // the one k-mer with this value (sixteen N) lives in slot `cap`, outside the walk
constexpr uint32_t DG_NONE = ~0u;
constexpr uint32_t DG_QC_FAIL = 512;

struct dg_lut {
    uint8_t c[256];
    constexpr dg_lut() : c() {
        for (int i = 0; i < 256; i++) c[i] = 255;
        const char *letters = "=ACMGRSVTWYHKDBN";     // what getRead makes of a BAM record (dbg/src/common.cpp:14-17)
        for (int i = 0; i < 16; i++) c[(unsigned char)letters[i]] = (uint8_t)i;
    }
};
constexpr dg_lut DG_LUT = dg_lut();

struct dg_region {
    int64_t ref_off, rb, re;          // the reference slice, the reads [rb, re)
    int64_t tab, etab, bm;            // where the region's node table, edge table and bit map start in the scratch arrays
    int32_t ref_len, ref_start;
    uint32_t eref, occ;               // edge occurrences of the reference, of the whole region
    uint32_t cap, ecap, words, pad;   // node slots (+ 1 for the all-ones key), edge slots, bit-map words
};
struct dg_head { int32_t bad_region, pad; unsigned long long probes, passed, edges; };
GAB_STATIC_ATOMIC64(dg_head, probes);
GAB_STATIC_ATOMIC64(dg_head, passed);
GAB_STATIC_ATOMIC64(dg_head, edges);
struct dg_tables {
    unsigned long long *nkey; uint32_t *nfirst, *ncol; unsigned long long *nweight;
    uint32_t *ekey, *efirst; unsigned long long *eweight;
    uint32_t *bitmap, *wprefix, *count;
};
struct dg_input {
    const char *ref; const char *seq; const uint8_t *qual; const int64_t *read_off;
    const int64_t *occ_before;        // [n_reads + 1]: edge occurrences of the reads before read j (QC-fail reads have none)
};

__device__ __forceinline__ uint32_t dg_spread(unsigned long long key, uint32_t cap) {
    unsigned long long h = key;
    h ^= h >> 33; h *= 0xff51afd7ed558ccdULL; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ULL; h ^= h >> 33;
    return (uint32_t)(((h >> 32) * (unsigned long long)cap) >> 32);
}

// The slot of `key` among nkey[0 .. cap), claimed if absent and `insert`.  A key never changes once written, so a stale read of
// "empty" only sends the lane to the compare-and-swap, which tells the truth.
__device__ __forceinline__ uint32_t dg_node_slot(unsigned long long *nkey, uint32_t cap, unsigned long long key, bool insert, uint32_t &probes) {
    if (key == DG_EMPTY64) return cap;
    uint32_t s = dg_spread(key, cap);
    for (uint32_t n = 0; n < cap; n++) {
        probes++;
        unsigned long long cur = __hip_atomic_load(&nkey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == DG_EMPTY64 && insert) {
            cur = atomicCAS(&nkey[s], DG_EMPTY64, key);
            if (cur == DG_EMPTY64) return s;
        }
        if (cur == key) return s;
        if (cur == DG_EMPTY64) return DG_NONE;
        s = s + 1 == cap ? 0 : s + 1;
    }
    return DG_NONE;
}

__device__ __forceinline__ uint32_t dg_edge_slot(uint32_t *ekey, uint32_t ecap, uint32_t key, bool insert) {
    uint32_t s = dg_spread(key, ecap);
    for (uint32_t n = 0; n < ecap; n++) {
        uint32_t cur = __hip_atomic_load(&ekey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == DG_NONE && insert) {
            cur = atomicCAS(&ekey[s], DG_NONE, key);
            if (cur == DG_NONE) return s;
        }
        if (cur == key) return s;
        if (cur == DG_NONE) return DG_NONE;
        s = s + 1 == ecap ? 0 : s + 1;
    }
    return DG_NONE;
}

// DeBruijnGraph_AddEdge (dbg/src/debruijn.cpp:917-949) for edge occurrence t: both nodes found or inserted and updated, then the edge
__device__ __forceinline__ void dg_add_edge(const dg_region &R, const dg_tables &T, unsigned long long ks, uint32_t letter, unsigned long long kmask,
                                            uint32_t t, uint32_t w, uint32_t colour, uint32_t &probes) {
    const unsigned long long ke = ((ks << 4) | letter) & kmask;
    unsigned long long *nkey = T.nkey + R.tab;
    const uint32_t ss = dg_node_slot(nkey, R.cap, ks, true, probes), se = dg_node_slot(nkey, R.cap, ke, true, probes);
    if (ss == DG_NONE || se == DG_NONE) return;       // (cannot happen: the table has more slots than the region has k-mers)
    atomicMin(&T.nfirst[R.tab + ss], 2u * t);
    atomicAdd(&T.nweight[R.tab + ss], (unsigned long long)w);
    atomicOr(&T.ncol[R.tab + ss], colour | (1u << (16 + letter)));
    atomicMin(&T.nfirst[R.tab + se], 2u * t + 1u);
    atomicAdd(&T.nweight[R.tab + se], (unsigned long long)w);
    atomicOr(&T.ncol[R.tab + se], colour);
    const uint32_t es = dg_edge_slot(T.ekey + R.etab, R.ecap, ss * 16u + letter, true);
    if (es == DG_NONE) return;
    atomicMin(&T.efirst[R.etab + es], t);
    atomicAdd(&T.eweight[R.etab + es], (unsigned long long)w);
}

__global__ __launch_bounds__(DG_BLOCK) void dg_insert(const dg_region *regions, dg_tables T, dg_input in, const int32_t *read_len, dg_lut lut, int k, int min_qual, dg_head *head) {
    __shared__ uint8_t code[256];
    const int tid = (int)threadIdx.x;
    code[tid] = lut.c[tid];
    __syncthreads();
    const dg_region R = regions[blockIdx.x];
    const unsigned long long kmask = k == 16 ? ~0ull : (1ull << (4 * k)) - 1ull;
    uint32_t probes = 0, passed = 0;
    bool bad = false;
    // every byte of the reference slice and of the reads is one of the sixteen letters
    const uint8_t *ref = (const uint8_t *)in.ref + R.ref_off;
    for (int i = tid; i < R.ref_len; i += DG_BLOCK) bad |= code[ref[i]] == 255;
    for (int64_t j = R.rb + tid / DG_GROUP; j < R.re; j += DG_BLOCK / DG_GROUP) {
        const uint8_t *s = (const uint8_t *)in.seq + in.read_off[j];
        const int len = read_len[j];
        for (int i = tid % DG_GROUP; i < len; i += DG_GROUP) bad |= code[s[i]] == 255;
    }
    if (bad) atomicMin(&head->bad_region, (int32_t)blockIdx.x);
    if (R.occ == 0) return;
    // loadReferenceIntoGraph (dbg/src/debruijn.cpp:1291-1317): colour REF, weight 1, every byte counts
    for (uint32_t i = (uint32_t)tid; i < R.eref; i += DG_BLOCK) {
        unsigned long long ks = 0;
        for (int j = 0; j < k; j++) ks = (ks << 4) | (code[ref[i + j]] & 15u);
        dg_add_edge(R, T, ks, code[ref[i + k]] & 15u, kmask, i, 1u, 1u, probes);
        passed++;
    }
    // loadReadIntoGraph (:1351-1396): the k + 1 bases of an edge hold no N and no quality below min_qual; the weight is the lowest quality
    const int64_t before = in.occ_before[R.rb];
    for (int64_t j = R.rb + tid / DG_GROUP; j < R.re; j += DG_BLOCK / DG_GROUP) {
        const int64_t at = in.occ_before[j];
        const uint32_t e = (uint32_t)(in.occ_before[j + 1] - at);
        if (e == 0) continue;                          // too short, or QC fail
        const uint8_t *s = (const uint8_t *)in.seq + in.read_off[j], *q = in.qual + in.read_off[j];
        const uint32_t t0 = R.eref + (uint32_t)(at - before);
        for (uint32_t i = (uint32_t)(tid % DG_GROUP); i < e; i += DG_GROUP) {
            unsigned long long ks = 0;
            uint32_t lowest = 255u; bool has_n = false;
            for (int b = 0; b <= k; b++) {
                const uint32_t c = code[s[i + b]] & 15u;
                has_n |= c == 15u;
                lowest = min(lowest, (uint32_t)q[i + b]);
                if (b < k) ks = (ks << 4) | c;
            }
            if (has_n || (int)lowest < min_qual) continue;
            dg_add_edge(R, T, ks, code[s[i + k]] & 15u, kmask, t0 + i, lowest, 2u, probes);
            passed++;
        }
    }
    atomicAdd(&head->probes, (unsigned long long)probes);
    atomicAdd(&head->passed, (unsigned long long)passed);
}

__global__ __launch_bounds__(DG_BLOCK) void dg_mark(const dg_region *regions, dg_tables T) {
    const dg_region R = regions[blockIdx.x];
    if (R.occ == 0) return;
    for (uint32_t s = threadIdx.x; s <= R.cap; s += DG_BLOCK) {
        const uint32_t f = T.nfirst[R.tab + s];
        if (f != DG_NONE) atomicOr(&T.bitmap[R.bm + (f >> 5)], 1u << (f & 31u));
    }
}

// wprefix[w] = first occurrences in the words before w; count[region] = nodes
__global__ __launch_bounds__(DG_BLOCK) void dg_scan(const dg_region *regions, dg_tables T) {
    __shared__ uint32_t part[DG_BLOCK];
    __shared__ uint32_t carry;
    const dg_region R = regions[blockIdx.x];
    const int tid = (int)threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < R.words; base += DG_BLOCK) {
        const uint32_t w = base + (uint32_t)tid;
        const uint32_t mine = w < R.words ? (uint32_t)__popc(T.bitmap[R.bm + w]) : 0u;
        part[tid] = mine;
        __syncthreads();
        for (int off = 1; off < DG_BLOCK; off <<= 1) {
            const uint32_t add = tid >= off ? part[tid - off] : 0u;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const uint32_t c = carry;
        if (w < R.words) T.wprefix[R.bm + w] = c + part[tid] - mine;
        __syncthreads();
        if (tid == DG_BLOCK - 1) carry = c + part[tid];
        __syncthreads();
    }
    if (tid == 0) T.count[blockIdx.x] = carry;
}

__device__ __forceinline__ int32_t dg_number(const dg_region &R, const dg_tables &T, uint32_t f) {
    return (int32_t)(T.wprefix[R.bm + (f >> 5)] + (uint32_t)__popc(T.bitmap[R.bm + (f >> 5)] & ((1u << (f & 31u)) - 1u)));
}

__global__ __launch_bounds__(DG_BLOCK) void dg_emit(const dg_region *regions, dg_tables T, dg_input in, const int64_t *node_off, gab_dbg_node *nodes, int k, dg_head *head) {
    const dg_region R = regions[blockIdx.x];
    if (R.occ == 0) return;
    const unsigned long long kmask = k == 16 ? ~0ull : (1ull << (4 * k)) - 1ull;
    gab_dbg_node *out = nodes + node_off[blockIdx.x];
    uint32_t unused = 0, edges = 0;
    for (uint32_t s = threadIdx.x; s <= R.cap; s += DG_BLOCK) {
        const uint32_t f = T.nfirst[R.tab + s];
        if (f == DG_NONE) continue;
        const unsigned long long key = s == R.cap ? DG_EMPTY64 : T.nkey[R.tab + s];
        const uint32_t col = T.ncol[R.tab + s];
        gab_dbg_node rec;
        const uint32_t t = f >> 1, side = f & 1u;
        if (t < R.eref) {
            rec.src_read = -1; rec.src_off = (int32_t)(t + side); rec.position = R.ref_start + (int32_t)(t + side);
        } else {                                       // the read j with occ_before[j] <= u < occ_before[j + 1]
            const int64_t u = (int64_t)(t - R.eref) + in.occ_before[R.rb];
            int64_t lo = R.rb, hi = R.re;
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) / 2;
                if (in.occ_before[mid] <= u) lo = mid; else hi = mid;
            }
            rec.src_read = (int32_t)lo; rec.src_off = (int32_t)(u - in.occ_before[lo]) + (int32_t)side; rec.position = -1;
        }
        rec.colours = (int32_t)(col & 3u);
        rec.weight = (int64_t)T.nweight[R.tab + s];
        rec.pad = 0;
        // the successors by their own first occurrence, the four earliest kept (the slots of debruijn.cpp:928-941)
        uint32_t ef[4] = {DG_NONE, DG_NONE, DG_NONE, DG_NONE}, el[4] = {0, 0, 0, 0};
        unsigned long long ew[4] = {0, 0, 0, 0};
        int n = 0;
        for (uint32_t m = col >> 16; m; m &= m - 1u) {
            const uint32_t letter = (uint32_t)__ffs((int)m) - 1u;
            const uint32_t es = dg_edge_slot(T.ekey + R.etab, R.ecap, s * 16u + letter, false);
            if (es == DG_NONE) continue;
            uint32_t cf = T.efirst[R.etab + es], cl = letter;
            unsigned long long cw = T.eweight[R.etab + es];
            for (int j = 0; j < 4; j++) {              // insertion into the sorted four; what falls off the end is dropped
                if (cf < ef[j]) {
                    const uint32_t tf = ef[j], tl = el[j]; const unsigned long long tw = ew[j];
                    ef[j] = cf; el[j] = cl; ew[j] = cw; cf = tf; cl = tl; cw = tw;
                }
            }
            n = min(n + 1, 4);
        }
        rec.n_edges = n;
        for (int j = 0; j < 4; j++) {
            rec.edge_to[j] = -1; rec.edge_weight[j] = 0;
            if (j < n) {
                const unsigned long long ke = ((key << 4) | el[j]) & kmask;
                const uint32_t se = dg_node_slot(T.nkey + R.tab, R.cap, ke, false, unused);
                if (se != DG_NONE) rec.edge_to[j] = dg_number(R, T, T.nfirst[R.tab + se]);
                rec.edge_weight[j] = (int64_t)ew[j];
            }
        }
        edges += (uint32_t)n;
        out[dg_number(R, T, f)] = rec;
    }
    if (edges) atomicAdd(&head->edges, (unsigned long long)edges);
}

inline int64_t dg_occurrences(int64_t len, int k) { return std::max<int64_t>(0, len - k - 1); }
inline int64_t dg_kmers(int64_t len, int k) { const int64_t e = dg_occurrences(len, k); return e ? e + 1 : 0; }

}  // namespace

struct gab_dbg {
    int device = 0;
    gab_devbuf scratch, io;
    gab_host_stream hs;
    hipEvent_t ev[5] = {};
    bool have_events = false;
    gab_dbg_stats stats = {};
    float insert_ms = 0, number_ms = 0, emit_ms = 0;
};

static int dg_no_handle(const char *who) { gab_set_error("%s: NULL handle", who); return GAB_EINVAL; }

extern "C" int gab_dbg_create(int device, gab_dbg **out) {
    GAB_CHECK(out, "gab_dbg_create: NULL out");
    *out = nullptr;
    int rc = gab_check_device(device);
    if (rc) return rc;
    gab_dbg *h = new (std::nothrow) gab_dbg();
    if (!h) { gab_set_error("gab_dbg_create: out of host memory"); return GAB_ENOMEM; }
    h->device = device;
    gab_device_guard g(device);
    for (auto &e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) { gab_set_error("gab_dbg_create: hipEventCreate failed"); gab_dbg_destroy(h); return GAB_EDEVICE; }
    h->have_events = true;
    *out = h;
    return GAB_OK;
}

extern "C" void gab_dbg_destroy(gab_dbg *h) {
    if (!h) return;
    gab_device_guard g(h->device);
    for (auto &e : h->ev) if (e) (void)hipEventDestroy(e);
    h->scratch.release(); h->io.release(); h->hs.release();
    delete h;
}

// scratch bytes of a call: 24 per node slot, 16 per edge slot, 8 per bit-map word, the per-region and per-read arrays
static size_t dg_scratch_bytes(int64_t regions, int64_t reads, int64_t node_slots, int64_t edge_slots, int64_t words) {
    return (size_t)(24 * node_slots + 16 * edge_slots + 8 * words + (int64_t)(sizeof(dg_region) + 4 + 8) * (regions + 1) + 8 * (reads + 1)) + 16 * 256;
}

extern "C" int gab_dbg_reserve(gab_dbg *h, int64_t max_regions, int64_t max_reads, int64_t max_occurrences) {
    if (!h) return dg_no_handle("gab_dbg_reserve");
    GAB_CHECK(max_regions >= 0 && max_reads >= 0 && max_occurrences >= 0, "gab_dbg_reserve: negative size");
    gab_device_guard g(h->device);
    const int64_t slots = max_occurrences + max_occurrences / 2 + 10 * max_regions;
    return h->scratch.reserve(dg_scratch_bytes(max_regions, max_reads, slots + max_regions + max_occurrences / 2, slots, max_occurrences / 16 + max_regions));
}

extern "C" int64_t gab_dbg_room(const int32_t *ref_len, const int32_t *read_len, const int32_t *read_flag, const int64_t *read_begin, const int64_t *read_end,
                                int64_t n_reads, int64_t n_regions, int k, int64_t *per_region) {
    if (n_regions < 0 || n_reads < 0 || k < 1 || k > GAB_DBG_MAX_K || (n_regions && !(ref_len && read_begin && read_end)) || (n_reads && !(read_len && read_flag))) {
        gab_set_error("gab_dbg_room: NULL argument, a negative count or k %d outside 1 .. %d", k, GAB_DBG_MAX_K);
        return GAB_EINVAL;
    }
    std::vector<int64_t> before((size_t)n_reads + 1, 0);
    for (int64_t j = 0; j < n_reads; j++) before[(size_t)j + 1] = before[(size_t)j] + (((uint32_t)read_flag[j] & DG_QC_FAIL) ? 0 : dg_kmers(read_len[j], k));
    int64_t total = 0;
    for (int64_t r = 0; r < n_regions; r++) {
        if (read_begin[r] < 0 || read_end[r] < read_begin[r] || read_end[r] > n_reads) {
            gab_set_error("gab_dbg_room: region %lld: reads [%lld, %lld) outside the %lld given", (long long)r, (long long)read_begin[r], (long long)read_end[r], (long long)n_reads);
            return GAB_EINVAL;
        }
        const int64_t need = dg_kmers(ref_len[r], k) + before[(size_t)read_end[r]] - before[(size_t)read_begin[r]];
        if (per_region) per_region[r] = need;
        total += need;
    }
    return total;
}

extern "C" int gab_dbg_build_device(gab_dbg *h, const gab_dbg_params *params, const char *ref, int64_t ref_bytes, const int64_t *ref_off, const int32_t *ref_len,
                                    const int32_t *ref_start, const char *seq, const uint8_t *qual, int64_t seq_bytes, const int64_t *read_off, const int32_t *read_len,
                                    const int32_t *read_flag, int64_t n_reads, const int64_t *read_begin, const int64_t *read_end, int64_t n_regions,
                                    int64_t *node_off, gab_dbg_node *nodes, int64_t capacity, int64_t *nout, void *stream) {
    if (!h) return dg_no_handle("gab_dbg_build_device");
    GAB_CHECK(params && nout, "gab_dbg_build_device: NULL argument");
    const int k = params->k, min_qual = params->min_qual;
    GAB_CHECK(k >= 1 && k <= GAB_DBG_MAX_K, "gab_dbg_build_device: k %d outside 1 .. %d", k, GAB_DBG_MAX_K);
    GAB_CHECK(n_regions >= 0 && n_regions <= INT32_MAX && n_reads >= 0 && n_reads <= INT32_MAX, "gab_dbg_build_device: n_regions %lld or n_reads %lld out of range",
              (long long)n_regions, (long long)n_reads);
    GAB_CHECK(capacity >= 0 && ref_bytes >= 0 && seq_bytes >= 0, "gab_dbg_build_device: negative size");
    h->stats = {}; h->insert_ms = h->number_ms = h->emit_ms = 0;
    *nout = 0;
    GAB_CHECK(node_off, "gab_dbg_build_device: NULL argument");
    gab_device_guard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t nr = (size_t)n_regions, nd = (size_t)n_reads;
    if (nr == 0) { GAB_HIP(hipMemsetAsync(node_off, 0, 8, s)); GAB_HIP(hipStreamSynchronize(s)); return GAB_OK; }
    GAB_CHECK(ref_off && ref_len && ref_start && read_begin && read_end && (nd == 0 || (read_off && read_len && read_flag)), "gab_dbg_build_device: NULL argument");

    // ---- lengths, offsets and flags come to the host; everything the kernels index by is checked here
    std::vector<int64_t> ro(nr), rb(nr), re(nr), so(nd), before(nd + 1, 0), kmers_before(nd + 1, 0);
    std::vector<int32_t> rl(nr), rs(nr), sl(nd), sf(nd);
    GAB_HIP(hipMemcpyAsync(ro.data(), ref_off, 8 * nr, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(rl.data(), ref_len, 4 * nr, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(rs.data(), ref_start, 4 * nr, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(rb.data(), read_begin, 8 * nr, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(re.data(), read_end, 8 * nr, hipMemcpyDeviceToHost, s));
    if (nd) {
        GAB_HIP(hipMemcpyAsync(so.data(), read_off, 8 * nd, hipMemcpyDeviceToHost, s));
        GAB_HIP(hipMemcpyAsync(sl.data(), read_len, 4 * nd, hipMemcpyDeviceToHost, s));
        GAB_HIP(hipMemcpyAsync(sf.data(), read_flag, 4 * nd, hipMemcpyDeviceToHost, s));
    }
    GAB_HIP(hipStreamSynchronize(s));
    for (size_t j = 0; j < nd; j++) {
        GAB_CHECK(sl[j] >= 0 && so[j] >= 0 && so[j] + sl[j] <= seq_bytes, "gab_dbg_build: read %zu: bases [%lld, +%d) outside the slab of %lld bytes", j, (long long)so[j], sl[j],
                  (long long)seq_bytes);
        const bool fail = ((uint32_t)sf[j] & DG_QC_FAIL) != 0;
        before[j + 1] = before[j] + (fail ? 0 : dg_occurrences(sl[j], k));
        kmers_before[j + 1] = kmers_before[j] + (fail ? 0 : dg_kmers(sl[j], k));
    }
    GAB_CHECK(nd == 0 || (seq && qual), "gab_dbg_build_device: NULL argument");
    std::vector<dg_region> regions(nr);
    int64_t node_slots = 0, edge_slots = 0, words = 0, offered = 0;
    for (size_t r = 0; r < nr; r++) {
        GAB_CHECK(rl[r] >= 0 && ro[r] >= 0 && ro[r] + rl[r] <= ref_bytes, "gab_dbg_build: region %zu: reference bases [%lld, +%d) outside the slab of %lld bytes", r, (long long)ro[r],
                  rl[r], (long long)ref_bytes);
        GAB_CHECK(rl[r] == 0 || ref, "gab_dbg_build_device: NULL argument");
        GAB_CHECK(rs[r] >= 0 && (int64_t)rs[r] + rl[r] <= INT32_MAX, "gab_dbg_build: region %zu: ref_start %d + ref_len %d: positions are 0 .. 2^31 - 1", r, rs[r], rl[r]);
        GAB_CHECK(rb[r] >= 0 && rb[r] <= re[r] && re[r] <= n_reads, "gab_dbg_build: region %zu: reads [%lld, %lld) outside the %lld given", r, (long long)rb[r], (long long)re[r],
                  (long long)n_reads);
        const int64_t eref = dg_occurrences(rl[r], k), occ = eref + before[(size_t)re[r]] - before[(size_t)rb[r]];
        GAB_CHECK(occ <= GAB_DBG_MAX_OCCURRENCES, "gab_dbg_build: region %zu offers %lld edge occurrences, more than GAB_DBG_MAX_OCCURRENCES (%d)", r, (long long)occ, GAB_DBG_MAX_OCCURRENCES);
        const int64_t kmers = dg_kmers(rl[r], k) + kmers_before[(size_t)re[r]] - kmers_before[(size_t)rb[r]];
        dg_region &R = regions[r];
        memset(&R, 0, sizeof R);
        R.ref_off = ro[r]; R.rb = rb[r]; R.re = re[r]; R.ref_len = rl[r]; R.ref_start = rs[r]; R.eref = (uint32_t)eref; R.occ = (uint32_t)occ;
        if (occ) {
            R.cap = (uint32_t)(kmers + kmers / 2 + 8); R.ecap = (uint32_t)(occ + occ / 2 + 8); R.words = (uint32_t)((2 * occ + 31) / 32);
            R.tab = node_slots; R.etab = edge_slots; R.bm = words;
            node_slots += (int64_t)R.cap + 1; edge_slots += R.ecap; words += R.words;
        }
        offered += occ;
    }

    // ---- the scratch layout: what starts as all ones, then what starts as zero, then what is written before it is read
    int rc;
    gab_stage_bump a;
    const size_t o_head = a.region(256);
    const size_t o_nkey = a.region(8 * (size_t)node_slots), o_nfirst = a.region(4 * (size_t)node_slots), o_ekey = a.region(4 * (size_t)edge_slots), o_efirst = a.region(4 * (size_t)edge_slots);
    const size_t o_zero = a.region(0);
    const size_t o_nweight = a.region(8 * (size_t)node_slots), o_eweight = a.region(8 * (size_t)edge_slots), o_ncol = a.region(4 * (size_t)node_slots), o_bitmap = a.region(4 * (size_t)words);
    const size_t o_rest = a.region(0);
    const size_t o_wprefix = a.region(4 * (size_t)words), o_count = a.region(4 * nr), o_regions = a.region(sizeof(dg_region) * nr), o_before = a.region(8 * (nd + 1)), o_noff = a.region(8 * (nr + 1));
    GAB_CHECK_ATOMIC64(o_nkey); GAB_CHECK_ATOMIC64(o_nweight); GAB_CHECK_ATOMIC64(o_eweight); GAB_CHECK_ATOMIC64(o_head);
    if ((rc = h->scratch.reserve(a.o)) != GAB_OK) return rc;
    char *b = h->scratch.as<char>();
    dg_tables T = {(unsigned long long *)(b + o_nkey), (uint32_t *)(b + o_nfirst), (uint32_t *)(b + o_ncol), (unsigned long long *)(b + o_nweight),
                   (uint32_t *)(b + o_ekey), (uint32_t *)(b + o_efirst), (unsigned long long *)(b + o_eweight), (uint32_t *)(b + o_bitmap), (uint32_t *)(b + o_wprefix),
                   (uint32_t *)(b + o_count)};
    dg_head *d_head = (dg_head *)(b + o_head), head = {INT32_MAX, 0, 0ull, 0ull, 0ull};
    dg_region *d_regions = (dg_region *)(b + o_regions);
    int64_t *d_before = (int64_t *)(b + o_before), *d_noff = (int64_t *)(b + o_noff);
    const dg_input in = {ref, seq, qual, read_off, d_before};

    GAB_HIP(hipEventRecord(h->ev[0], s));
    GAB_HIP(hipMemcpyAsync(d_head, &head, sizeof head, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(d_regions, regions.data(), sizeof(dg_region) * nr, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(d_before, before.data(), 8 * (nd + 1), hipMemcpyHostToDevice, s));
    if (o_zero > o_nkey) GAB_HIP(hipMemsetAsync(b + o_nkey, 0xFF, o_zero - o_nkey, s));
    if (o_rest > o_zero) GAB_HIP(hipMemsetAsync(b + o_zero, 0, o_rest - o_zero, s));
    hipLaunchKernelGGL(dg_insert, dim3((unsigned)nr), dim3(DG_BLOCK), 0, s, d_regions, T, in, read_len, DG_LUT, k, min_qual, d_head);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(h->ev[1], s));
    hipLaunchKernelGGL(dg_mark, dim3((unsigned)nr), dim3(DG_BLOCK), 0, s, d_regions, T);
    GAB_HIP(hipGetLastError());
    hipLaunchKernelGGL(dg_scan, dim3((unsigned)nr), dim3(DG_BLOCK), 0, s, d_regions, T);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(h->ev[2], s));
    std::vector<uint32_t> count(nr);
    GAB_HIP(hipMemcpyAsync(count.data(), T.count, 4 * nr, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(&head, d_head, sizeof head, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    GAB_CHECK(head.bad_region == INT32_MAX, "gab_dbg_build: region %d: a byte of its reference or of one of its reads is none of the letters =ACMGRSVTWYHKDBN (lower case included)",
              head.bad_region);
    std::vector<int64_t> noff(nr + 1, 0);
    for (size_t r = 0; r < nr; r++) noff[r + 1] = noff[r] + count[r];
    *nout = noff[nr];
    if (noff[nr] > capacity) {
        gab_set_error("gab_dbg_build: %lld nodes, room for %lld", (long long)noff[nr], (long long)capacity);
        return GAB_ERANGE;
    }
    GAB_CHECK(nodes || noff[nr] == 0, "gab_dbg_build_device: NULL argument");

    // ---- the records
    GAB_HIP(hipMemcpyAsync(d_noff, noff.data(), 8 * (nr + 1), hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(node_off, d_noff, 8 * (nr + 1), hipMemcpyDeviceToDevice, s));
    GAB_HIP(hipEventRecord(h->ev[3], s));
    hipLaunchKernelGGL(dg_emit, dim3((unsigned)nr), dim3(DG_BLOCK), 0, s, d_regions, T, in, d_noff, nodes, k, d_head);
    GAB_HIP(hipGetLastError());
    GAB_HIP(hipEventRecord(h->ev[4], s));
    GAB_HIP(hipMemcpyAsync(&head, d_head, sizeof head, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    GAB_HIP(hipEventElapsedTime(&h->insert_ms, h->ev[0], h->ev[1]));
    GAB_HIP(hipEventElapsedTime(&h->number_ms, h->ev[1], h->ev[2]));
    GAB_HIP(hipEventElapsedTime(&h->emit_ms, h->ev[3], h->ev[4]));
    GAB_HIP(hipEventElapsedTime(&h->stats.total_ms, h->ev[0], h->ev[4]));
    h->stats.kernel_ms = h->insert_ms + h->number_ms + h->emit_ms;
    h->stats.regions = n_regions; h->stats.occurrences = offered; h->stats.passed = (int64_t)head.passed; h->stats.nodes = noff[nr];
    h->stats.edges = (int64_t)head.edges; h->stats.probes = (int64_t)head.probes;
    return GAB_OK;
}

extern "C" int gab_dbg_build(gab_dbg *h, const gab_dbg_params *params, const char *ref, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_start,
                             const char *seq, const uint8_t *qual, const int64_t *read_off, const int32_t *read_len, const int32_t *read_flag, int64_t n_reads,
                             const int64_t *read_begin, const int64_t *read_end, int64_t n_regions, int64_t *node_off, gab_dbg_node *nodes, int64_t capacity, int64_t *nout) {
    if (!h) return dg_no_handle("gab_dbg_build");
    GAB_CHECK(params && nout && node_off, "gab_dbg_build: NULL argument");
    GAB_CHECK(n_regions >= 0 && n_regions <= INT32_MAX && n_reads >= 0 && n_reads <= INT32_MAX && capacity >= 0, "gab_dbg_build: n_regions %lld, n_reads %lld or capacity %lld out of range",
              (long long)n_regions, (long long)n_reads, (long long)capacity);
    GAB_CHECK(params->k >= 1 && params->k <= GAB_DBG_MAX_K, "gab_dbg_build: k %d outside 1 .. %d", params->k, GAB_DBG_MAX_K);
    h->stats = {}; h->insert_ms = h->number_ms = h->emit_ms = 0;
    *nout = 0;
    const size_t nr = (size_t)n_regions, nd = (size_t)n_reads;
    if (nr == 0) { node_off[0] = 0; return GAB_OK; }
    GAB_CHECK(ref_off && ref_len && ref_start && read_begin && read_end && (nd == 0 || (read_off && read_len && read_flag && seq && qual)), "gab_dbg_build: NULL argument");
    // the windows of the two slabs that the call refers to; the device call sees them re-based to the windows' starts
    int64_t ra = INT64_MAX, rz = 0, sa = INT64_MAX, sz = 0;
    for (size_t r = 0; r < nr; r++) {
        GAB_CHECK(ref_len[r] >= 0 && ref_off[r] >= 0, "gab_dbg_build: region %zu: negative reference offset or length", r);
        GAB_CHECK(ref_len[r] == 0 || ref, "gab_dbg_build: NULL argument");
        if (ref_len[r]) { ra = std::min(ra, ref_off[r]); rz = std::max(rz, ref_off[r] + ref_len[r]); }
    }
    for (size_t j = 0; j < nd; j++) {
        GAB_CHECK(read_len[j] >= 0 && read_off[j] >= 0, "gab_dbg_build: read %zu: negative offset or length", j);
        if (read_len[j]) { sa = std::min(sa, read_off[j]); sz = std::max(sz, read_off[j] + read_len[j]); }
    }
    if (rz == 0) ra = 0;
    if (sz == 0) sa = 0;
    const int64_t room = gab_dbg_room(ref_len, read_len, read_flag, read_begin, read_end, n_reads, n_regions, params->k, nullptr);
    if (room < 0) return (int)room;
    const int64_t dev_cap = std::min(capacity, room);
    std::vector<int64_t> ro(nr), so(nd);
    for (size_t r = 0; r < nr; r++) ro[r] = ref_len[r] ? ref_off[r] - ra : 0;
    for (size_t j = 0; j < nd; j++) so[j] = read_len[j] ? read_off[j] - sa : 0;
    gab_device_guard g(h->device);
    hipStream_t s = nullptr;
    int rc = h->hs.get(&s);
    if (rc) return rc;
    gab_stage_bump a;
    const size_t o_ref = a.region(gab_pad256((size_t)(rz - ra))), o_seq = a.region(gab_pad256((size_t)(sz - sa))), o_qual = a.region(gab_pad256((size_t)(sz - sa)));
    const size_t o_out = a.region(sizeof(gab_dbg_node) * (size_t)dev_cap);
    const size_t o_ro = a.a8(nr), o_rb = a.a8(nr), o_re = a.a8(nr), o_so = a.a8(nd), o_noff = a.a8(nr + 1);
    const size_t o_rl = a.a4(nr), o_rs = a.a4(nr), o_sl = a.a4(nd), o_sf = a.a4(nd);
    if ((rc = h->io.reserve(a.o)) != GAB_OK) return rc;
    char *b = h->io.as<char>();
    {
        std::lock_guard<std::mutex> gate(gab_h2d_mutex(h->device));
        if (rz > ra) GAB_HIP(hipMemcpyAsync(b + o_ref, ref + ra, (size_t)(rz - ra), hipMemcpyHostToDevice, s));
        if (sz > sa) {
            GAB_HIP(hipMemcpyAsync(b + o_seq, seq + sa, (size_t)(sz - sa), hipMemcpyHostToDevice, s));
            GAB_HIP(hipMemcpyAsync(b + o_qual, qual + sa, (size_t)(sz - sa), hipMemcpyHostToDevice, s));
        }
        GAB_HIP(hipMemcpyAsync(b + o_ro, ro.data(), 8 * nr, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_rb, read_begin, 8 * nr, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_re, read_end, 8 * nr, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_rl, ref_len, 4 * nr, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_rs, ref_start, 4 * nr, hipMemcpyHostToDevice, s));
        if (nd) {
            GAB_HIP(hipMemcpyAsync(b + o_so, so.data(), 8 * nd, hipMemcpyHostToDevice, s));
            GAB_HIP(hipMemcpyAsync(b + o_sl, read_len, 4 * nd, hipMemcpyHostToDevice, s));
            GAB_HIP(hipMemcpyAsync(b + o_sf, read_flag, 4 * nd, hipMemcpyHostToDevice, s));
        }
        GAB_HIP(hipStreamSynchronize(s));
    }
    rc = gab_dbg_build_device(h, params, b + o_ref, rz - ra, (const int64_t *)(b + o_ro), (const int32_t *)(b + o_rl), (const int32_t *)(b + o_rs), b + o_seq,
                              (const uint8_t *)(b + o_qual), sz - sa, (const int64_t *)(b + o_so), (const int32_t *)(b + o_sl), (const int32_t *)(b + o_sf), n_reads,
                              (const int64_t *)(b + o_rb), (const int64_t *)(b + o_re), n_regions, (int64_t *)(b + o_noff), (gab_dbg_node *)(b + o_out), dev_cap, nout, s);
    if (rc) return rc;
    GAB_CHECK(nodes || *nout == 0, "gab_dbg_build: NULL argument");
    GAB_HIP(hipMemcpy(node_off, b + o_noff, 8 * (nr + 1), hipMemcpyDeviceToHost));
    if (*nout) GAB_HIP(hipMemcpy(nodes, b + o_out, sizeof(gab_dbg_node) * (size_t)*nout, hipMemcpyDeviceToHost));
    return GAB_OK;
}

extern "C" int gab_dbg_last_stats(gab_dbg *h, gab_dbg_stats *out) {
    if (!h) return dg_no_handle("gab_dbg_last_stats");
    GAB_CHECK(out, "gab_dbg_last_stats: NULL out");
    *out = h->stats;
    return GAB_OK;
}

extern "C" int gab_dbg_last_phases(gab_dbg *h, float *insert_ms, float *number_ms, float *emit_ms) {
    if (!h) return dg_no_handle("gab_dbg_last_phases");
    if (insert_ms) *insert_ms = h->insert_ms;
    if (number_ms) *number_ms = h->number_ms;
    if (emit_ms) *emit_ms = h->emit_ms;
    return GAB_OK;
}

// ---- the planner: the batch loop of main (dbg/src/debruijn.cpp:1576-1592) with setWindowPointers / bisectReadsLeft (dbg/src/common.cpp:161-227)
static int64_t dg_bisect_left(const int32_t *pos, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (pos[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

extern "C" int gab_dbg_plan_regions(int32_t beg, int32_t end, const int32_t *pos, const int32_t *read_end, int64_t n_reads, int32_t contig_len,
                                    gab_dbg_region *out, int64_t capacity, int64_t *nout) {
    GAB_CHECK(nout, "gab_dbg_plan_regions: NULL nout");
    GAB_CHECK(beg >= 0 && end >= beg && contig_len >= 0 && n_reads >= 0 && capacity >= 0 && (n_reads == 0 || (pos && read_end)), "gab_dbg_plan_regions: bad argument");
    GAB_CHECK((int64_t)end + 2 * GAB_DBG_REGION_SIZE <= INT32_MAX, "gab_dbg_plan_regions: end %d too close to 2^31", end);
    const int32_t size = GAB_DBG_REGION_SIZE, shift = std::max(100, std::min(1000, size / 2));
    const int64_t need = ((int64_t)end - beg + shift - 1) / shift;
    *nout = need;
    if (need > capacity) { gab_set_error("gab_dbg_plan_regions: %lld regions, room for %lld", (long long)need, (long long)capacity); return GAB_ERANGE; }
    GAB_CHECK(out || need == 0, "gab_dbg_plan_regions: NULL out");
    int64_t longest = 0;
    for (int64_t j = 0; j < n_reads; j++) {
        GAB_CHECK(read_end[j] >= pos[j] && (j == 0 || pos[j] >= pos[j - 1]), "gab_dbg_plan_regions: read %lld: pos[] must ascend and no read may end before it starts", (long long)j);
        longest = std::max<int64_t>(longest, (int64_t)read_end[j] - pos[j]);
    }
    int64_t at = 0;
    for (int64_t s = beg; s < end; s += shift, at++) {
        const int64_t stop = std::min<int64_t>(s + size, end), ref_start = std::max<int64_t>(0, s - size), ref_end = stop + size;
        gab_dbg_region &R = out[at];
        R.start = (int32_t)s; R.ref_start = (int32_t)ref_start; R.ref_len = (int32_t)std::max<int64_t>(0, std::min<int64_t>(ref_end, contig_len) - ref_start); R.pad = 0;
        int64_t first = 0, last = 0;
        if (n_reads) {
            first = dg_bisect_left(pos, n_reads, std::max<int64_t>(1, s - longest));
            last = dg_bisect_left(pos, n_reads, stop);
            while (first < n_reads && read_end[first] <= s) first++;
            last = std::min(last, n_reads);
            GAB_CHECK(first <= last, "gab_dbg_plan_regions: region at %lld: the window's first read %lld lies behind its last %lld (the reference exits here)", (long long)s,
                      (long long)first, (long long)last);
        }
        R.read_begin = first; R.read_end = last;
    }
    return GAB_OK;
}
