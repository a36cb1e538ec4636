// kmer.hip -- exact canonical k-mer counting (Flye's solid k-mer counter, kmer-cnt/vertex_index.cpp:787-860) on gfx950.
//
// The reference walks the forward strand of every kept read, canonicalises each k-mer (kmer-cnt/kmer.h:39-64) and bumps one wrapping
// 8-bit counter per possible k-mer (4^k bytes, 16 GiB at k = 17).  Here the counts are exact and live in an open-addressing table
// sized from the number of k-mer positions of the call; the reference's two printed numbers follow from the exact counts:
//     Total k-mers = sum over x of ceil(c(x) / 256)        (every increment that saw the byte at 0)
//     Hash size    = #{x : c(x) >= 256}                    (keys upserted when an increment saw 255)
//
// Stages of one call (all on the caller's stream, one synchronisation at the end):
//   kmer_pack     ASCII -> 2 bits per base, 16 bases per 32-bit word, every read on a word boundary; flags bytes outside ACGTacgt
//   kmer_count    one wave per tile of 64 x GAB_KMER_RUN positions of one read; a lane owns GAB_KMER_RUN consecutive positions, rolls the
//                 forward and the reverse-complement word (one shift-or each per base), takes the minimum and merges equal neighbouring
//                 keys of its run into one (key, n) before it touches memory: homopolymers and tandem repeats give one key thousands
//                 of hits in a row.  Extraction and counting are ONE kernel: a (key, n) list between them would cost 12 bytes of
//                 HBM traffic per position each way for nothing.
//   table         128-byte lines of 8 slots: 8 x 64-bit (key + 1) (0 = empty), 8 x 32-bit count, 32 bytes unused.  A lane reads the 64
//                 key bytes of its line, adds to the matching slot, or claims the first empty one with a compare-and-swap; a full line
//                 sends it to the next line.  Slots only ever go from empty to taken, so the taken slots of a line are a prefix and a
//                 look-up may stop at the first empty slot.
//   kmer_reduce   one pass over the table: distinct, sum ceil(c / 256), #(c >= 256), largest count; per-wave partial sums, one
//                 atomic per wave and value
// gab_kmer_spectrum / gab_kmer_query / gab_kmer_dump read the table of the last count; it stays in the handle until the next one.
//
// Several GPUs split the KEYS, not the reads (gab_kmer_count_part): every GPU walks all reads and inserts only the canonical k-mers
// whose hash falls into its partition, into a table sized for that share.  The partial results are disjoint, so nothing is merged
// and no GPU talks to another; what N GPUs add is atomic throughput, what each of them repeats is the extraction.
#include "gab_internal.h"
#include <string.h>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <new>
#include <vector>

namespace {

constexpr int kRun = GAB_KMER_RUN;         // positions per lane
constexpr int kTile = 64 * kRun;           // positions per wave
constexpr int kBlock = 256;
constexpr int kSlots = 8;                  // per 128-byte line
constexpr int kLdsBins = 1024;

struct KmerLine {
    unsigned long long key[kSlots];        // canonical k-mer + 1; 0 = empty
    uint32_t cnt[kSlots];
    uint32_t pad[kSlots];
};
static_assert(sizeof(KmerLine) == 128, "one table line is one 128-byte memory line");
typedef unsigned long long kmer_ull2 __attribute__((ext_vector_type(2)));

struct KmerCounters {
    unsigned long long bad_read;           // lowest index of a read with a byte outside ACGTacgt (~0 = none)
    unsigned long long probes, merged;     // table lines visited by the inserts; equal-neighbour merges inside the lanes' runs
    unsigned long long distinct, total_kmers, hash_size, max_count;
    unsigned long long bad_query;          // lowest index of a query >= 4^k (~0 = none)
    uint32_t dump_n;
    uint32_t overflow;                     // a bounded insert gave up: the partition's table is full (the host repeats the call)
};
GAB_STATIC_ATOMIC64(KmerCounters, bad_read);
GAB_STATIC_ATOMIC64(KmerCounters, bad_query);

struct KmerTile { int32_t read, start; };  // positions [start, start + kTile) of a kept read

__host__ __device__ __forceinline__ uint64_t kmer_hash(uint64_t key) {
    uint64_t h = key * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 32);
}
__host__ __device__ __forceinline__ uint64_t kmer_mulhi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// Key-space partitions: h * nparts is a 128-bit product whose high word is the partition, in [0, nparts), and whose low word -- the
// fraction of the way through that partition -- is as uniform as h itself, so it picks the line of the partition's own table.
// (Taking the line from h unchanged would put a partition's keys into 1 / nparts of its lines.)  nparts = 1: part 0, and the line
// of every key is the line it always had.
__host__ __device__ __forceinline__ uint32_t kmer_part_of_hash(uint64_t h, uint32_t nparts) { return (uint32_t)kmer_mulhi(h, nparts); }
__host__ __device__ __forceinline__ uint64_t kmer_line_of_hash(uint64_t h, uint32_t nparts, uint64_t nlines) { return kmer_mulhi(h * nparts, nlines); }
__device__ __forceinline__ uint64_t kmer_line_of(uint64_t key, uint64_t nlines) { return __umul64hi(kmer_hash(key), nlines); }

// ---- pack: thread = one output word of one read ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void kmer_pack(const char *__restrict__ seq, const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                    const int64_t *__restrict__ woff, int64_t n_reads, int64_t n_words,
                                                    uint32_t *__restrict__ packed, KmerCounters *ct) {
    const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (w >= n_words) return;
    int64_t lo = 0, hi = n_reads;          // the LAST read r with woff[r] <= w: woff is non-decreasing and woff[n_reads] = n_words > w,
    while (hi - lo > 1) {                  // so that read has at least one word and w is one of them
        const int64_t mid = (lo + hi) >> 1;
        if (woff[mid] <= w) lo = mid; else hi = mid;
    }
    const int64_t first = (w - woff[lo]) * 16;
    const int n = (int)min((int64_t)16, (int64_t)len[lo] - first);
    const char *p = seq + off[lo] + first;
    uint32_t word = 0;
    bool bad = false;
    for (int j = 0; j < n; j++) {
        const uint32_t c = (uint8_t)p[j];
        const uint32_t u = c & 0xDFu;
        bad |= !(u == 'A' || u == 'C' || u == 'G' || u == 'T');
        uint32_t x = (c >> 1) & 3u;        // A 0, C 1, T 2, G 3
        x ^= x >> 1;                       // A 0, C 1, G 2, T 3
        word |= x << (2 * j);
    }
    packed[w] = word;
    if (bad) atomicMin(&ct->bad_read, (unsigned long long)lo);
}

// ---- count -------------------------------------------------------------------------------------------------------------------------
// Why a key never lands in two slots: a lane tries the slots of a line in rising order, starting at the lowest slot it saw empty --
// a stale view can only show a taken slot as empty, never the reverse, so that start is at or below the line's true first empty slot --
// and it passes a slot only after the compare-and-swap (or a load) has shown it taken by ANOTHER key, which is final.  It leaves
// a line only after all eight slots were seen taken by other keys.
// kBounded (a partition's table, whose size is a forecast of the partition's share of the keys): the walk gives up once it has
// left `limit` lines, or as soon as it leaves a line after another lane gave up, and raises ct->overflow; the host then repeats the
// call with a table that cannot fill.  Slots never go back to empty, so `limit` = nlines full lines mean a full table.
template <bool kBounded>
__device__ __forceinline__ void kmer_insert(KmerLine *table, uint64_t nlines, uint64_t line, uint64_t key, uint32_t n, uint32_t &probes,
                                            uint64_t limit, KmerCounters *ct) {
    const unsigned long long stored = key + 1;
    uint64_t left = 0;
    for (;;) {
        probes++;
        KmerLine *L = table + line;
        const kmer_ull2 *src = reinterpret_cast<const kmer_ull2 *>(L->key);
        int match = -1, empty = -1;
#pragma unroll
        for (int j = kSlots / 2 - 1; j >= 0; j--) {
            const kmer_ull2 v = src[j];
            if (v.y == stored) match = 2 * j + 1;
            if (v.y == 0) empty = 2 * j + 1;
            if (v.x == stored) match = 2 * j;
            if (v.x == 0) empty = 2 * j;
        }
        if (match >= 0) { atomicAdd(&L->cnt[match], n); return; }
        if (empty >= 0)
            for (int s = empty; s < kSlots; s++) {
                const unsigned long long seen = atomicCAS(&L->key[s], 0ull, stored);
                if (seen == 0 || seen == stored) { atomicAdd(&L->cnt[s], n); return; }
            }
        if constexpr (kBounded) {
            if (++left >= limit || __hip_atomic_load(&ct->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { atomicOr(&ct->overflow, 1u); return; }
        }
        line = line + 1 == nlines ? 0 : line + 1;
    }
}

// kPart = false: the whole key space in one table (part, nparts and limit are not read).  kPart = true: the lane still merges equal
// neighbours first, then hashes the (key, n) run it flushes -- one hash per run, not per base -- and inserts it only when the key
// falls into `part`; `merged` and `probes` count the runs and inserts of that partition alone, so both add up over the partitions.
template <bool kPart>
__global__ __launch_bounds__(kBlock) void kmer_count(const uint32_t *__restrict__ packed, const int64_t *__restrict__ woff, const int32_t *__restrict__ len,
                                                     const KmerTile *__restrict__ tiles, int64_t n_tiles, int k, KmerLine *table, uint64_t nlines,
                                                     KmerCounters *ct, uint32_t part, uint32_t nparts, uint64_t limit) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    uint32_t probes = 0, merged = 0;
    if (t < n_tiles) {
        const KmerTile tile = tiles[t];
        const int32_t npos = len[tile.read] - k;                   // positions 0 .. L - k - 1 (the reference never visits the last k-mer)
        const int32_t p0 = tile.start + lane * kRun;
        const int32_t p1 = min(p0 + kRun, npos);
        if (p0 < p1) {
            const uint32_t *words = packed + woff[tile.read];
            const uint64_t mask = (1ull << (2 * k)) - 1ull;
            const int top = 2 * (k - 1);
            uint64_t fw = 0, rc = 0;
            int32_t b = p0;                                        // next base to take in
            uint32_t w = words[b >> 4] >> (2 * (b & 15));
            auto next_base = [&]() -> uint64_t {
                const uint64_t c = w & 3u;
                b++;
                w >>= 2;
                if ((b & 15) == 0) w = words[b >> 4];              // (the last base taken is p1 + k - 2 <= L - 2, so b <= L - 1: a word of the read)
                return c;
            };
            for (int j = 0; j < k - 1; j++) {
                const uint64_t c = next_base();
                fw = (fw << 2) | c;
                rc = (rc >> 2) | ((3ull - c) << top);
            }
            uint64_t cur = ~0ull;
            uint32_t n = 0;
            auto flush = [&]() {
                if constexpr (!kPart) kmer_insert<false>(table, nlines, kmer_line_of(cur, nlines), cur, n, probes, 0, ct);
                else {
                    const uint64_t h = kmer_hash(cur);
                    if (kmer_part_of_hash(h, nparts) == part) {
                        merged += n - 1;
                        kmer_insert<true>(table, nlines, kmer_line_of_hash(h, nparts, nlines), cur, n, probes, limit, ct);
                    }
                }
            };
            for (int32_t p = p0; p < p1; p++) {
                const uint64_t c = next_base();
                fw = ((fw << 2) | c) & mask;
                rc = (rc >> 2) | ((3ull - c) << top);
                const uint64_t key = fw < rc ? fw : rc;
                if (key == cur) { n++; if constexpr (!kPart) merged++; }
                else {
                    if (n) flush();
                    cur = key; n = 1;
                }
            }
            if (n) flush();
        }
    }
    // per-wave sums, one atomic per wave and value
    for (int d = 32; d; d >>= 1) { probes += __shfl_xor(probes, d); merged += __shfl_xor(merged, d); }
    if (lane == 0) {
        if (probes) atomicAdd(&ct->probes, (unsigned long long)probes);
        if (merged) atomicAdd(&ct->merged, (unsigned long long)merged);
    }
}

// ---- reduce ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void kmer_reduce(const KmerLine *__restrict__ table, uint64_t nslots, KmerCounters *ct) {
    unsigned long long distinct = 0, total = 0, hashed = 0, mx = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * kBlock) {
        const KmerLine *L = table + i / kSlots;
        const int s = (int)(i % kSlots);
        if (L->key[s]) {
            const unsigned long long c = L->cnt[s];
            distinct++;
            total += (c + 255) >> 8;
            hashed += c >= 256;
            mx = c > mx ? c : mx;
        }
    }
    for (int d = 32; d; d >>= 1) {
        distinct += __shfl_xor(distinct, d); total += __shfl_xor(total, d); hashed += __shfl_xor(hashed, d);
        const unsigned long long o = __shfl_xor(mx, d);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && distinct) {
        atomicAdd(&ct->distinct, distinct); atomicAdd(&ct->total_kmers, total);
        if (hashed) atomicAdd(&ct->hash_size, hashed);
        atomicMax(&ct->max_count, mx);
    }
}

// ---- spectrum: hist[min(c, nbins - 1)]++ over the taken slots; the low bins go through LDS -------------------------------------------
__global__ __launch_bounds__(kBlock) void kmer_spectrum(const KmerLine *__restrict__ table, uint64_t nslots, unsigned long long *hist, uint32_t nbins) {
    __shared__ uint32_t lds[kLdsBins];
    for (int j = threadIdx.x; j < kLdsBins; j += kBlock) lds[j] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t rounds = (nslots + stride - 1) / stride;        // (every lane takes every round: the ballot below wants whole waves)
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t i = r * stride + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
        uint32_t bin = 0;
        bool taken = false;
        if (i < nslots) {
            const KmerLine *L = table + i / kSlots;
            const int s = (int)(i % kSlots);
            taken = L->key[s] != 0;
            bin = min(L->cnt[s], nbins - 1);
        }
        // most k-mers of a read set are seen once: count bin 1 per wave, not per lane
        const unsigned long long ones = __ballot(taken && bin == 1);
        if (ones && (int)(threadIdx.x & 63) == __builtin_ctzll(ones)) atomicAdd(&lds[1], (uint32_t)__popcll(ones));
        if (taken && bin != 1) {
            if (bin < (uint32_t)kLdsBins) atomicAdd(&lds[bin], 1u);
            else atomicAdd(&hist[bin], 1ull);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < kLdsBins; j += kBlock)
        if (lds[j]) atomicAdd(&hist[j], (unsigned long long)lds[j]);      // (lds[j] != 0 only for j < nbins)
}

// ---- query -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t kmer_revcomp(uint64_t x, int k) {
    x = ~x;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = __builtin_bswap64(x);
    return x >> (64 - 2 * k);
}

__global__ __launch_bounds__(kBlock) void kmer_query(const KmerLine *__restrict__ table, uint64_t nlines, int k, const uint64_t *__restrict__ kmers,
                                                     int64_t n, uint32_t *__restrict__ counts, KmerCounters *ct, uint32_t part, uint32_t nparts) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t x = kmers[i];
    if (x >> (2 * k)) { counts[i] = 0; atomicMin(&ct->bad_query, (unsigned long long)i); return; }
    const uint64_t r = kmer_revcomp(x, k);
    const unsigned long long stored = (x < r ? x : r) + 1;
    const uint64_t h = kmer_hash(stored - 1);
    if (kmer_part_of_hash(h, nparts) != part) { counts[i] = 0; return; }       // another partition's key
    uint64_t line = kmer_line_of_hash(h, nparts, nlines);
    uint32_t c = 0;
    // (the walk ends at an empty slot; a partition's table may hold no empty slot near this line, or none at all: nlines lines at most)
    for (uint64_t visited = 0; visited < nlines; visited++) {
        const KmerLine *L = table + line;
        bool done = false;
#pragma unroll
        for (int s = 0; s < kSlots; s++) {
            const unsigned long long v = L->key[s];
            if (!done && v == stored) { c = L->cnt[s]; done = true; }
            if (v == 0) done = true;
        }
        if (done) break;
        line = line + 1 == nlines ? 0 : line + 1;
    }
    counts[i] = c;
}

// ---- dump: the taken slots, unordered; sorted afterwards ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void kmer_compact(const KmerLine *__restrict__ table, uint64_t nslots, uint64_t *__restrict__ keys,
                                                       uint32_t *__restrict__ counts, uint32_t capacity, KmerCounters *ct) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t rounds = (nslots + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t i = r * stride + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
        unsigned long long key = 0;
        uint32_t c = 0;
        if (i < nslots) {
            const KmerLine *L = table + i / kSlots;
            key = L->key[i % kSlots];
            c = L->cnt[i % kSlots];
        }
        const uint32_t slot = gab_wave_slot(&ct->dump_n, key != 0);
        if (key != 0 && slot < capacity) { keys[slot] = key - 1; counts[slot] = c; }
    }
}

}  // namespace

// =============================================================================== host side
struct gab_kmer {
    gab_host_stream hs;
    int device = 0;
    gab_devbuf io;          // staging of the host-pointer entry point: sequence window | off | len
    gab_devbuf packed;      // 2-bit reads
    gab_devbuf plan;        // woff | tiles
    gab_devbuf table;
    gab_devbuf ct;          // KmerCounters
    gab_devbuf aux;         // spectrum bins, query staging, dump keys / counts and the sort's scratch
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // start | packed | counted | reduced | end
    KmerCounters *h_ct = nullptr;      // pinned
    bool counted = false;              // the table of a finished count is in the handle
    int k = 0;
    uint64_t nlines = 0;
    gab_kmer_result last = {0, 0, 0, 0, 0, 0};
    int64_t probes = 0, merged = 0;
    float phase_ms[3] = {0, 0, 0}, total_ms = 0;
    int sweep_blocks = 2048;           // grid of the kernels that sweep the table
    int part = 0, nparts = 1;          // what the last count ran as (gab_kmer_last_part)
    bool retried = false;              // ... and whether its first table filled up and the call was repeated
    gab_tuning tun = gab_tuning_loaded();      // experiment knobs, read when the handle is made
};

static uint64_t table_lines(int64_t positions, int k) {
    // at most min(positions, 4^k) distinct keys; half full at worst, so every probe sequence ends at an empty slot
    const uint64_t keys = std::min<uint64_t>((uint64_t)positions, 1ull << (2 * k));
    return std::max<uint64_t>(16, (2 * keys + kSlots - 1) / kSlots);
}
// The first table of a partitioned call: room for the partition's even share of the keys plus a quarter (kPartSlack) plus 64 keys,
// at half full like the whole table.  The share of a partition is binomial around the even share; a quarter covers 6 standard
// deviations from 576 keys per partition on, the 64 keys cover them below that (6 sqrt(n) - n / 4 <= 36).  Keys that the hash
// spreads worse than that fill the table: the bounded insert says so and the call is repeated with table_lines, which cannot fill.
// Never more than table_lines; nparts = 1 gives table_lines itself.
static uint64_t part_table_lines(int64_t positions, int k, int nparts) {
    const uint64_t keys = std::min<uint64_t>((uint64_t)positions, 1ull << (2 * k));
    const uint64_t share = (keys + (uint64_t)nparts - 1) / (uint64_t)nparts;
    const uint64_t room = share + share / 4 + 64;
    return std::min<uint64_t>(table_lines(positions, k), std::max<uint64_t>(16, (2 * room + kSlots - 1) / kSlots));
}
constexpr uint64_t kProbeCap = 1024;   // lines a bounded insert walks in a first-attempt table before it calls the table full
static int kmer_check_parts(const char *fn, int nparts) {
    GAB_CHECK(nparts >= 1 && nparts <= GAB_KMER_MAX_PARTS, "%s: nparts = %d, supported 1..%d", fn, nparts, GAB_KMER_MAX_PARTS);
    return GAB_OK;
}
static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
static unsigned sweep_grid(const gab_kmer *h) {
    return (unsigned)std::min<uint64_t>((uint64_t)h->sweep_blocks, (h->nlines * kSlots + kBlock - 1) / kBlock);
}

extern "C" int gab_kmer_create(int device, gab_kmer **out) {
    if (!out) { gab_set_error("gab_kmer_create: NULL argument"); return GAB_EINVAL; }
    *out = nullptr;
    int rc = gab_check_device(device);
    if (rc) return rc;
    gab_device_guard g(device);
    gab_kmer *h = new (std::nothrow) gab_kmer();
    if (!h) { gab_set_error("out of host memory"); return GAB_ENOMEM; }
    h->device = device;
    for (int i = 0; i < 5; i++)
        if (hipEventCreate(&h->ev[i]) != hipSuccess) { gab_set_error("hipEventCreate failed"); gab_kmer_destroy(h); return GAB_EDEVICE; }
    if (hipHostMalloc((void **)&h->h_ct, sizeof(KmerCounters)) != hipSuccess) {
        h->h_ct = nullptr; gab_set_error("hipHostMalloc failed"); gab_kmer_destroy(h); return GAB_ENOMEM;
    }
    if ((rc = h->ct.reserve(sizeof(KmerCounters)))) { gab_kmer_destroy(h); return rc; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->sweep_blocks = prop.multiProcessorCount * 8;
    *out = h;
    return GAB_OK;
}

extern "C" void gab_kmer_destroy(gab_kmer *h) {
    if (!h) return;
    gab_device_guard g(h->device);
    h->io.release(); h->packed.release(); h->plan.release(); h->table.release(); h->ct.release(); h->aux.release(); h->hs.release();
    for (int i = 0; i < 5; i++) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    if (h->h_ct) (void)hipHostFree(h->h_ct);
    delete h;
}

extern "C" int gab_kmer_part_of(uint64_t canonical_kmer, int nparts) {
    int rc = kmer_check_parts("gab_kmer_part_of", nparts);
    if (rc) return rc;
    return (int)kmer_part_of_hash(kmer_hash(canonical_kmer), (uint32_t)nparts);
}

extern "C" int gab_kmer_parts_of(const uint64_t *canonical_kmers, int64_t n, int nparts, int32_t *parts) {
    int rc = kmer_check_parts("gab_kmer_parts_of", nparts);
    if (rc) return rc;
    GAB_CHECK(n >= 0 && (n == 0 || (canonical_kmers && parts)), "gab_kmer_parts_of: NULL or negative argument");
    for (int64_t i = 0; i < n; i++) parts[i] = (int32_t)kmer_part_of_hash(kmer_hash(canonical_kmers[i]), (uint32_t)nparts);
    return GAB_OK;
}

extern "C" int64_t gab_kmer_table_slots(int64_t positions, int k, int nparts) {
    int rc = kmer_check_parts("gab_kmer_table_slots", nparts);
    if (rc) return rc;
    GAB_CHECK(positions >= 0 && k >= 1 && k <= GAB_KMER_MAX_K, "gab_kmer_table_slots: positions = %lld, k = %d (k: 1..%d)", (long long)positions, k,
              GAB_KMER_MAX_K);
    return (int64_t)(part_table_lines(std::max<int64_t>(positions, 1), k, nparts) * kSlots);
}

extern "C" int gab_kmer_reserve(gab_kmer *h, int64_t max_reads, int64_t max_seq_bytes) { return gab_kmer_reserve_part(h, max_reads, max_seq_bytes, 1); }

extern "C" int gab_kmer_reserve_part(gab_kmer *h, int64_t max_reads, int64_t max_seq_bytes, int nparts) {
    if (!h || max_reads < 0 || max_seq_bytes < 0) { gab_set_error("gab_kmer_reserve: bad argument"); return GAB_EINVAL; }
    int rc = kmer_check_parts("gab_kmer_reserve_part", nparts);
    if (rc) return rc;
    gab_device_guard g(h->device);
    const size_t words = (size_t)max_seq_bytes / 16 + (size_t)max_reads + 1;
    const size_t tiles = (size_t)max_seq_bytes / kTile + (size_t)max_reads + 1;
    if ((rc = h->io.reserve(align256((size_t)max_seq_bytes + 64) + align256((size_t)max_reads * 8) + align256((size_t)max_reads * 4)))) return rc;
    if ((rc = h->packed.reserve(words * 4))) return rc;
    if ((rc = h->plan.reserve(align256(((size_t)max_reads + 1) * 8) + tiles * sizeof(KmerTile)))) return rc;
    if ((rc = h->table.reserve((size_t)part_table_lines(std::max<int64_t>(max_seq_bytes, 1), GAB_KMER_MAX_K, nparts) * sizeof(KmerLine)))) return rc;
    hipStream_t s;
    if ((rc = h->hs.get(&s))) return rc;
    return gab_warm_copy_engines(s, h->io.p, h->io.cap);
}

// d_*: device; off / len: the same two arrays on the host
// part / nparts: the partition of the key space this call counts (0 / 1: all of it, in the unpartitioned kernel)
static int kmer_count_impl(gab_kmer *h, const char *d_seq, int64_t seq_bytes, const int64_t *d_off, const int32_t *d_len, const int64_t *off,
                           const int32_t *len, int64_t n_reads, int k, int32_t min_len_exclusive, int part, int nparts, gab_kmer_result *res,
                           hipStream_t s) {
    h->counted = false;
    gab_tuning_refresh(&h->tun);
    // plan on the host: word offset of every read, tiles of the kept ones
    std::vector<int64_t> woff((size_t)n_reads + 1);
    std::vector<KmerTile> tiles;
    int64_t words = 0, positions = 0, kept = 0;
    GAB_CHECK(n_reads < (1ll << 31), "gab_kmer_count: %lld reads in one call (limit 2^31)", (long long)n_reads);
    for (int64_t r = 0; r < n_reads; r++) {
        GAB_CHECK(len[r] >= 0 && off[r] >= 0 && off[r] + len[r] <= seq_bytes,
                  "gab_kmer_count: read %lld (offset %lld, length %d) lies outside the %lld sequence bytes", (long long)r, (long long)off[r], (int)len[r],
                  (long long)seq_bytes);
        woff[(size_t)r] = words;
        words += ((int64_t)len[r] + 15) / 16;
        if (len[r] > min_len_exclusive) {
            kept++;
            const int32_t npos = len[r] - k;
            for (int32_t p = 0; p < npos; p += kTile) tiles.push_back(KmerTile{(int32_t)r, p});
            if (npos > 0) positions += npos;
        }
    }
    woff[(size_t)n_reads] = words;
    GAB_CHECK(positions < (1ll << 32), "gab_kmer_count: %lld k-mer positions in one call (limit 2^32: the counts are 32-bit)", (long long)positions);
    const int64_t n_tiles = (int64_t)tiles.size();
    // GAB_KMER_PART_FLOOR: the first table of a partitioned call is the 16-line floor (test hook of the repeat below)
    uint64_t nlines = nparts > 1 && h->tun.kmer_part_floor ? 16 : part_table_lines(std::max<int64_t>(positions, 1), k, nparts);
    int rc;
    const size_t tiles_at = align256(((size_t)n_reads + 1) * 8);
    if ((rc = h->packed.reserve((size_t)words * 4 + 4))) return rc;
    if ((rc = h->plan.reserve(tiles_at + (size_t)n_tiles * sizeof(KmerTile) + 8))) return rc;
    if ((rc = h->table.reserve((size_t)nlines * sizeof(KmerLine)))) return rc;
    int64_t *d_woff = h->plan.as<int64_t>();
    KmerTile *d_tiles = reinterpret_cast<KmerTile *>(h->plan.as<char>() + tiles_at);
    KmerCounters *d_ct = h->ct.as<KmerCounters>();
    uint32_t *packed = h->packed.as<uint32_t>();

    GAB_HIP(hipEventRecord(h->ev[0], s));
    KmerCounters zero = {};
    zero.bad_read = ~0ull; zero.bad_query = ~0ull;
    *h->h_ct = zero;
    GAB_HIP(hipMemcpyAsync(d_ct, h->h_ct, sizeof(KmerCounters), hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(d_woff, woff.data(), ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_tiles) GAB_HIP(hipMemcpyAsync(d_tiles, tiles.data(), (size_t)n_tiles * sizeof(KmerTile), hipMemcpyHostToDevice, s));
    if (words)
        hipLaunchKernelGGL(kmer_pack, dim3((unsigned)gab_ceil_div(words, kBlock)), dim3(kBlock), 0, s, d_seq, d_off, d_len, d_woff, n_reads, words, packed, d_ct);
    GAB_HIP(hipEventRecord(h->ev[1], s));
    // (a bad byte packs as some base: the count below runs on it harmlessly and the call fails after the one synchronisation)
    // A partition's first table is a forecast (part_table_lines) and its inserts are bounded: when one gave up, the host sees
    // ct->overflow after the call's one synchronisation and runs clear, count and reduce once more in a table of table_lines lines,
    // which is at most half full whatever the hash does.  (After such a repeat pack_ms includes the first attempt.)
    h->retried = false;
    for (int attempt = 0;; attempt++) {
        if (attempt && (rc = h->table.reserve((size_t)nlines * sizeof(KmerLine)))) return rc;
        KmerLine *table = h->table.as<KmerLine>();
        GAB_HIP(hipMemsetAsync(table, 0, (size_t)nlines * sizeof(KmerLine), s));
        if (n_tiles) {
            const dim3 grid((unsigned)gab_ceil_div(n_tiles, kBlock / 64));
            if (nparts == 1)
                hipLaunchKernelGGL(kmer_count<false>, grid, dim3(kBlock), 0, s, packed, d_woff, d_len, d_tiles, n_tiles, k, table, nlines, d_ct, 0u, 1u,
                                   (uint64_t)0);
            else
                hipLaunchKernelGGL(kmer_count<true>, grid, dim3(kBlock), 0, s, packed, d_woff, d_len, d_tiles, n_tiles, k, table, nlines, d_ct, (uint32_t)part,
                                   (uint32_t)nparts, attempt ? nlines : std::min<uint64_t>(nlines, kProbeCap));
        }
        GAB_HIP(hipEventRecord(h->ev[2], s));
        h->nlines = nlines;
        hipLaunchKernelGGL(kmer_reduce, dim3(sweep_grid(h)), dim3(kBlock), 0, s, table, nlines * kSlots, d_ct);
        GAB_HIP(hipEventRecord(h->ev[3], s));
        GAB_HIP(hipMemcpyAsync(h->h_ct, d_ct, sizeof(KmerCounters), hipMemcpyDeviceToHost, s));
        GAB_HIP(hipEventRecord(h->ev[4], s));
        GAB_HIP(hipStreamSynchronize(s));
        GAB_HIP(hipGetLastError());
        GAB_CHECK(h->h_ct->bad_read == ~0ull, "gab_kmer_count: read %lld holds a byte outside ACGTacgt (a driver replaces such bytes before the call)",
                  (long long)h->h_ct->bad_read);
        if (!h->h_ct->overflow) break;
        GAB_CHECK(attempt == 0, "gab_kmer_count: internal error: a table of %llu lines for %lld positions filled up", (unsigned long long)nlines,
                  (long long)positions);
        h->retried = true;
        nlines = table_lines(std::max<int64_t>(positions, 1), k);
        *h->h_ct = zero;
        GAB_HIP(hipMemcpyAsync(d_ct, h->h_ct, sizeof(KmerCounters), hipMemcpyHostToDevice, s));
        GAB_HIP(hipEventRecord(h->ev[1], s));
    }
    const KmerCounters &c = *h->h_ct;
    h->last = gab_kmer_result{kept, positions, (int64_t)c.distinct, (int64_t)c.total_kmers, (int64_t)c.hash_size, (int64_t)c.max_count};
    h->probes = (int64_t)c.probes; h->merged = (int64_t)c.merged;
    for (int i = 0; i < 3; i++) (void)hipEventElapsedTime(&h->phase_ms[i], h->ev[i], h->ev[i + 1]);
    (void)hipEventElapsedTime(&h->total_ms, h->ev[0], h->ev[4]);
    h->k = k; h->part = part; h->nparts = nparts; h->counted = true;
    if (res) *res = h->last;
    return GAB_OK;
}

static int kmer_check_args(gab_kmer *h, const void *off, const void *len, int64_t n_reads, int k, int part, int nparts) {
    GAB_CHECK(h && n_reads >= 0 && (n_reads == 0 || (off && len)), "gab_kmer_count: NULL or negative argument");
    GAB_CHECK(nparts >= 1 && nparts <= GAB_KMER_MAX_PARTS && part >= 0 && part < nparts,
              "gab_kmer_count_part: part = %d, nparts = %d (0 <= part < nparts, nparts: 1..%d)", part, nparts, GAB_KMER_MAX_PARTS);
    GAB_CHECK(k >= 1 && k <= GAB_KMER_MAX_K, "gab_kmer_count: k = %d, supported 1..%d (the reference's flat counter, kmer-cnt/vertex_index.cpp:793-796)", k,
              GAB_KMER_MAX_K);
    return GAB_OK;
}

extern "C" int gab_kmer_count_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads, int k,
                                     int32_t min_len_exclusive, gab_kmer_result *res, void *stream) {
    return gab_kmer_count_part_device(h, seq, seq_bytes, off, len, n_reads, k, min_len_exclusive, 0, 1, res, stream);
}

extern "C" int gab_kmer_count_part_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads,
                                          int k, int32_t min_len_exclusive, int part, int nparts, gab_kmer_result *res, void *stream) {
    int rc = kmer_check_args(h, off, len, n_reads, k, part, nparts);
    if (rc) return rc;
    GAB_CHECK(seq_bytes >= 0 && (seq || seq_bytes == 0), "gab_kmer_count_device: bad sequence slab");
    gab_device_guard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<int64_t> h_off((size_t)n_reads);
    std::vector<int32_t> h_len((size_t)n_reads);
    if (n_reads) {
        GAB_HIP(hipMemcpyAsync(h_off.data(), off, (size_t)n_reads * 8, hipMemcpyDeviceToHost, s));
        GAB_HIP(hipMemcpyAsync(h_len.data(), len, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    return kmer_count_impl(h, seq, seq_bytes, off, len, h_off.data(), h_len.data(), n_reads, k, min_len_exclusive, part, nparts, res, s);
}

extern "C" int gab_kmer_count(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int32_t min_len_exclusive,
                              gab_kmer_result *res) {
    return gab_kmer_count_part(h, seq, off, len, n_reads, k, min_len_exclusive, 0, 1, res);
}

extern "C" int gab_kmer_count_part(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int32_t min_len_exclusive,
                                   int part, int nparts, gab_kmer_result *res) {
    int rc = kmer_check_args(h, off, len, n_reads, k, part, nparts);
    if (rc) return rc;
    gab_device_guard g(h->device);
    hipStream_t s;
    if ((rc = h->hs.get(&s))) return rc;
    int64_t lo = INT64_MAX, hi = 0;                                // the window of the slab the reads span
    for (int64_t r = 0; r < n_reads; r++) {
        GAB_CHECK(len[r] >= 0 && off[r] >= 0, "gab_kmer_count: read %lld has a negative offset or length", (long long)r);
        if (len[r] == 0) continue;
        lo = std::min(lo, off[r]); hi = std::max(hi, off[r] + len[r]);
    }
    if (hi == 0) lo = 0;
    GAB_CHECK(seq || hi == 0, "gab_kmer_count: NULL sequence slab");
    const size_t span = (size_t)(hi - lo);
    const size_t off_at = align256(span + 64), len_at = off_at + align256((size_t)n_reads * 8);
    if ((rc = h->io.reserve(len_at + align256((size_t)n_reads * 4)))) return rc;
    char *d_seq = h->io.as<char>();
    int64_t *d_off = reinterpret_cast<int64_t *>(d_seq + off_at);
    int32_t *d_len = reinterpret_cast<int32_t *>(d_seq + len_at);
    std::vector<int64_t> rel((size_t)n_reads);
    for (int64_t r = 0; r < n_reads; r++) rel[(size_t)r] = len[r] ? off[r] - lo : 0;
    {
        std::lock_guard<std::mutex> lk(gab_h2d_mutex(h->device));
        if (span) GAB_HIP(hipMemcpyAsync(d_seq, seq + lo, span, hipMemcpyHostToDevice, s));
        if (n_reads) {
            GAB_HIP(hipMemcpyAsync(d_off, rel.data(), (size_t)n_reads * 8, hipMemcpyHostToDevice, s));
            GAB_HIP(hipMemcpyAsync(d_len, len, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
        }
        GAB_HIP(hipStreamSynchronize(s));
    }
    return kmer_count_impl(h, d_seq, (int64_t)span, d_off, d_len, rel.data(), len, n_reads, k, min_len_exclusive, part, nparts, res, s);
}

#define KMER_NEED_COUNT(fn) GAB_CHECK(h && h->counted, fn ": no finished gab_kmer_count on this handle")

extern "C" int gab_kmer_spectrum(gab_kmer *h, int64_t *hist, int32_t nbins) {
    KMER_NEED_COUNT("gab_kmer_spectrum");
    GAB_CHECK(hist && nbins >= 2, "gab_kmer_spectrum: NULL histogram or fewer than 2 bins");
    gab_device_guard g(h->device);
    hipStream_t s;
    int rc;
    if ((rc = h->hs.get(&s))) return rc;
    if ((rc = h->aux.reserve((size_t)nbins * 8))) return rc;
    unsigned long long *d_hist = h->aux.as<unsigned long long>();
    GAB_HIP(hipMemsetAsync(d_hist, 0, (size_t)nbins * 8, s));
    hipLaunchKernelGGL(kmer_spectrum, dim3(sweep_grid(h)), dim3(kBlock), 0, s, h->table.as<KmerLine>(), h->nlines * kSlots, d_hist, (uint32_t)nbins);
    GAB_HIP(hipMemcpyAsync(hist, d_hist, (size_t)nbins * 8, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    return GAB_OK;
}

extern "C" int gab_kmer_query(gab_kmer *h, const uint64_t *kmers, int64_t n, uint32_t *counts) {
    KMER_NEED_COUNT("gab_kmer_query");
    GAB_CHECK(n >= 0 && (n == 0 || (kmers && counts)), "gab_kmer_query: NULL or negative argument");
    if (n == 0) return GAB_OK;
    gab_device_guard g(h->device);
    hipStream_t s;
    int rc;
    if ((rc = h->hs.get(&s))) return rc;
    const size_t cnt_at = align256((size_t)n * 8);
    if ((rc = h->aux.reserve(cnt_at + (size_t)n * 4))) return rc;
    uint64_t *d_k = h->aux.as<uint64_t>();
    uint32_t *d_c = reinterpret_cast<uint32_t *>(h->aux.as<char>() + cnt_at);
    KmerCounters *d_ct = h->ct.as<KmerCounters>();
    h->h_ct->bad_query = ~0ull;
    GAB_HIP(hipMemcpyAsync(&d_ct->bad_query, &h->h_ct->bad_query, 8, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(d_k, kmers, (size_t)n * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(kmer_query, dim3((unsigned)gab_ceil_div(n, kBlock)), dim3(kBlock), 0, s, h->table.as<KmerLine>(), h->nlines, h->k, d_k, n, d_c, d_ct,
                       (uint32_t)h->part, (uint32_t)h->nparts);
    GAB_HIP(hipMemcpyAsync(&h->h_ct->bad_query, &d_ct->bad_query, 8, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(counts, d_c, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    GAB_CHECK(h->h_ct->bad_query == ~0ull, "gab_kmer_query: k-mer %lld has bits above 2k = %d", (long long)h->h_ct->bad_query, 2 * h->k);
    return GAB_OK;
}

extern "C" int gab_kmer_dump(gab_kmer *h, uint64_t *kmers, uint32_t *counts, int64_t capacity, int64_t *nout) {
    KMER_NEED_COUNT("gab_kmer_dump");
    GAB_CHECK(nout && capacity >= 0, "gab_kmer_dump: NULL or negative argument");
    const int64_t n = h->last.distinct;
    *nout = n;
    if (capacity < n) { gab_set_error("gab_kmer_dump: %lld k-mers, room for %lld", (long long)n, (long long)capacity); return GAB_ERANGE; }
    if (n == 0) return GAB_OK;
    GAB_CHECK(kmers && counts, "gab_kmer_dump: NULL output");
    gab_device_guard g(h->device);
    hipStream_t s;
    int rc;
    if ((rc = h->hs.get(&s))) return rc;
    size_t tmp_bytes = 0;
    GAB_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u,
                                      (unsigned)(2 * h->k), s));
    const size_t kb = align256((size_t)n * 8), cb = align256((size_t)n * 4);
    if ((rc = h->aux.reserve(2 * kb + 2 * cb + tmp_bytes + 256))) return rc;
    char *base = h->aux.as<char>();
    uint64_t *k_in = reinterpret_cast<uint64_t *>(base), *k_out = reinterpret_cast<uint64_t *>(base + kb);
    uint32_t *c_in = reinterpret_cast<uint32_t *>(base + 2 * kb), *c_out = reinterpret_cast<uint32_t *>(base + 2 * kb + cb);
    void *tmp = base + 2 * kb + 2 * cb;
    KmerCounters *d_ct = h->ct.as<KmerCounters>();
    GAB_HIP(hipMemsetAsync(&d_ct->dump_n, 0, 4, s));
    hipLaunchKernelGGL(kmer_compact, dim3(sweep_grid(h)), dim3(kBlock), 0, s, h->table.as<KmerLine>(), h->nlines * kSlots, k_in, c_in, (uint32_t)n, d_ct);
    GAB_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, k_in, k_out, c_in, c_out, (size_t)n, 0u, (unsigned)(2 * h->k), s));
    GAB_HIP(hipMemcpyAsync(kmers, k_out, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(counts, c_out, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    return GAB_OK;
}

extern "C" int gab_kmer_last_stats(gab_kmer *h, int64_t *probes, int64_t *merged, float *kernel_ms, float *total_ms) {
    KMER_NEED_COUNT("gab_kmer_last_stats");
    if (probes) *probes = h->probes;
    if (merged) *merged = h->merged;
    if (kernel_ms) *kernel_ms = h->phase_ms[1];
    if (total_ms) *total_ms = h->total_ms;
    return GAB_OK;
}

extern "C" int gab_kmer_last_phases(gab_kmer *h, float *pack_ms, float *count_ms, float *reduce_ms) {
    KMER_NEED_COUNT("gab_kmer_last_phases");
    if (pack_ms) *pack_ms = h->phase_ms[0];
    if (count_ms) *count_ms = h->phase_ms[1];
    if (reduce_ms) *reduce_ms = h->phase_ms[2];
    return GAB_OK;
}

extern "C" int gab_kmer_last_part(gab_kmer *h, int *part, int *nparts, int64_t *table_slots, int *retried) {
    KMER_NEED_COUNT("gab_kmer_last_part");
    if (part) *part = h->part;
    if (nparts) *nparts = h->nparts;
    if (table_slots) *table_slots = (int64_t)(h->nlines * kSlots);
    if (retried) *retried = h->retried ? 1 : 0;
    return GAB_OK;
}
