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
// The minimizer index splits the same way (gab_kmer_index_part_begin / _finish), but its filter needs two integers of the whole
// input, so its partitions meet once, on the host, in the middle of the build: see "minimizer index, host side" below.
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
    unsigned long long ix_kmers, ix_entries;       // minimizer index: kept k-mers and their entries
    unsigned long long ix_minimizers;      // ... and the emitted minimizers of the call (the low word is copied in from the scan)
    unsigned long long sx_total, sx_unique;        // solid index: capacities >= min_freq, their sum and their number (the filter's totals)
    unsigned long long sx_empty, sx_empty_cap;     // ... kept keys whose list stays empty (c(x) > thr), and the sum of their capacities
    unsigned long long sx_need, sx_fallback;       // ... positions that took the multiplicity test; reads that left the LDS table for the partitioned passes
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

// The one partition rule: does the table of `part` of `nparts` own the canonical k-mer `key`, and which of its nlines lines is the
// key's home?  One hash answers both.  kPart = false: the whole key space in one table; part and nparts are not read.
// (No early return for another partition's key: the compiler sinks the line's product below the caller's test either way, and in
// this shape the callers keep the registers they had.)
template <bool kPart>
__device__ __forceinline__ bool kmer_home(uint64_t key, uint32_t part, uint32_t nparts, uint64_t nlines, uint64_t *line) {
    if constexpr (!kPart) *line = kmer_line_of(key, nlines);
    else {
        const uint64_t h = kmer_hash(key);
        *line = kmer_line_of_hash(h, nparts, nlines);
        return kmer_part_of_hash(h, nparts) == part;
    }
    return true;
}

// ---- the rolling forward / reverse-complement words of a read (one shift-or each per base): seek(p), then every step() gives the
// k-mer at p, p + 1, ...
struct KmerRoller {
    const uint32_t *words;
    uint64_t mask, fw, rc;
    int top, k;
    int32_t b;                             // next base to take in
    uint32_t w;
    __device__ __forceinline__ KmerRoller(const uint32_t *words_, int k_)
        : words(words_), mask((1ull << (2 * k_)) - 1ull), fw(0), rc(0), top(2 * (k_ - 1)), k(k_), b(0), w(0) {}
    __device__ __forceinline__ uint64_t take() {
        const uint64_t c = w & 3u;
        b++;
        w >>= 2;
        if ((b & 15) == 0) w = words[b >> 4];      // (the last base taken belongs to position L - k - 1 and is base L - 2, so b <= L - 1: a word of the read)
        return c;
    }
    __device__ __forceinline__ void seek(int32_t p) {
        fw = 0; rc = 0; b = p;
        w = words[b >> 4] >> (2 * (b & 15));
        for (int j = 0; j < k - 1; j++) {
            const uint64_t c = take();
            fw = (fw << 2) | c;
            rc = (rc >> 2) | ((3ull - c) << top);
        }
    }
    __device__ __forceinline__ void step() {
        const uint64_t c = take();
        fw = ((fw << 2) | c) & mask;
        rc = (rc >> 2) | ((3ull - c) << top);
    }
    // from the k-mer at q + 1 to the k-mer at q (the cursor of take() stays where it is)
    __device__ __forceinline__ void back(int32_t q) {
        const uint64_t c = (words[q >> 4] >> (2 * (q & 15))) & 3u;
        fw = (fw >> 2) | (c << top);
        rc = ((rc << 2) | (3ull - c)) & mask;
    }
    __device__ __forceinline__ uint64_t canonical() const { return fw < rc ? fw : rc; }
    __device__ __forceinline__ bool forward() const { return fw <= rc; }      // palindromes are not flipped (kmer-cnt/kmer.h:54-63)
};

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
            KmerRoller R(packed + woff[tile.read], k);
            R.seek(p0);
            uint64_t cur = ~0ull;
            uint32_t n = 0;
            auto flush = [&]() {
                uint64_t line;
                if (!kmer_home<kPart>(cur, part, nparts, nlines, &line)) return;
                if constexpr (kPart) merged += n - 1;
                kmer_insert<kPart>(table, nlines, line, cur, n, probes, limit, ct);
            };
            for (int32_t p = p0; p < p1; p++) {
                R.step();
                const uint64_t key = R.canonical();
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
// kCaps (a partition of the minimizer index): total_kmers <- the sum of the counts themselves, the minimizers of the partition's keys
template <bool kCaps = false>
__global__ __launch_bounds__(kBlock) void kmer_reduce(const KmerLine *__restrict__ table, uint64_t nslots, KmerCounters *ct) {
    unsigned long long distinct = 0, total = 0, hashed = 0, mx = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * kBlock) {
        const KmerLine *L = table + i / kSlots;
        const int s = (int)(i % kSlots);
        if (L->key[s]) {
            const unsigned long long c = L->cnt[s];
            distinct++;
            total += kCaps ? c : (c + 255) >> 8;
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

// the slot of a key that is in the table, const or not (nullptr if it is not: the walk ends at an empty slot -- a line's taken slots
// are a prefix -- and the table is at most half full; a partition's table may hold no empty slot near this line, or none at all, so
// nlines lines at most).  line: the key's home line (kmer_home)
template <class Line>
__device__ __forceinline__ Line *kmer_find(Line *table, uint64_t nlines, uint64_t line, uint64_t key, int *slot) {
    const unsigned long long stored = key + 1;
    for (uint64_t visited = 0; visited < nlines; visited++) {
        Line *L = table + line;
        int match = -1;
        bool end = false;
#pragma unroll
        for (int s = kSlots - 1; s >= 0; s--) {
            const unsigned long long v = L->key[s];
            if (v == stored) match = s;
            if (v == 0) end = true;
        }
        if (match >= 0) { *slot = match; return L; }
        if (end) return nullptr;
        line = line + 1 == nlines ? 0 : line + 1;
    }
    return nullptr;
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
    const uint64_t key = x < r ? x : r;
    uint64_t line;
    int slot = 0;
    const KmerLine *L = nullptr;               // (another partition's key is answered without a probe)
    if (kmer_home<true>(key, part, nparts, nlines, &line)) L = kmer_find(table, nlines, line, key, &slot);
    counts[i] = L ? L->cnt[slot] : 0;
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

// ===================================================================================================================== minimizer index
// buildIndexMinimizers(1, w) (kmer-cnt/vertex_index.cpp:394-502) on the same packed reads, tiles and table.
//
// The sketch of a read (yieldMinimizers, kmer-cnt/kmer.h:206-262) keeps a monotone queue of (position, order key); the order key of a
// position is kmer_order_key of its canonical k-mer.  All that a step needs of that queue is its front f(p), and the front obeys
//     f(0) = 0
//     f(p) = p                                        if key[p] < key[f(p - 1)]            (everything before p is popped)
//          = the LAST position of (p - w, p] that
//            holds the minimum key of that window     else if f(p - 1) <= p - w            (expired; then the run of equals is skipped)
//          = f(p - 1)                                 otherwise,
// and position q is a minimizer iff f(p) = q for some p.  key[f(p)] is always the minimum of the window (p - w, p], so where that
// minimum is unique f(p) is its position whatever came before; where it is not, which of the equal positions is the front depends
// on the history (in a homopolymer the minimizers fall at 0, w, 2w, ... from the start of the run).  A lane that owns positions
// [p0, p1) therefore finds f(p0 - 1) like this: the window of p0 - 1 reaches the start of the read -> the first of its minima (no
// front has expired yet); its minimum m is unique -> that position; otherwise it walks back, one k-mer per step, to the first
// step s0 of the stretch of steps whose window minimum is m -- there the front is the last m of the window, because the step
// before either brought the first m in or saw a smaller key expire -- and plays the recurrence forward from s0.
// Nothing is kept per window position: when a front expires the lane re-rolls the w k-mers of the window from the packed words
// (about once per w steps in random sequence and in homopolymers alike; an adversarial read whose keys rise for a long stretch
// costs w k-mers per step).  Window state is a handful of scalars: no LDS, no private array.
// The walk back is serial and NOT bounded: inside a stretch of tied window minima -- a homopolymer, a tandem repeat of period <= w --
// every lane walks back to the stretch's start and replays forward to its p0, so a stretch of T positions costs its lanes
// T / 64 walks of up to T steps each: about T^2 / 64 k-mers in all, T of them on the slowest lane.  Measured
// (profiles/kmer_minimizers.md): about 0.65 us per position of the stretch -- a stretch of 1 kb holds one wave for 0.7 ms, which
// a call over many reads hides behind its other waves; a 16 kb read of one base takes 11 ms, one low-complexity stretch of 1 Mbp
// 0.68 s, random sequence of that length 0.5 ms.  Handing the front on from lane to lane through a wave scan would bound it and
// is not done here.
//
// A minimizer found at step p may lie up to w - 1 positions back, in another lane's run or another wave's tile, so the lanes mark
// minimizers in a bitmap (one 64-bit word per run of GAB_KMER_RUN positions, all tiles of a read back to back) with atomicOr.
__host__ __device__ __forceinline__ uint64_t kmer_order_key(uint64_t x) {      // kmer-cnt/kmer.h:91-98
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct KmerWindowMin { uint64_t m; int32_t first, last; };      // the minimum order key of a window, its first and last position
// re-rolls positions lo .. hi; fw_lo / rc_lo: the two words of the k-mer at lo
__device__ __forceinline__ KmerWindowMin kmer_window_min(KmerRoller &S, int32_t lo, int32_t hi, uint64_t *fw_lo = nullptr, uint64_t *rc_lo = nullptr) {
    KmerWindowMin x = {0, lo, lo};
    S.seek(lo);
    for (int32_t q = lo; q <= hi; q++) {
        S.step();
        const uint64_t h = kmer_order_key(S.canonical());
        if (q == lo) {
            x.m = h;
            if (fw_lo) { *fw_lo = S.fw; *rc_lo = S.rc; }
        } else if (h < x.m) { x.m = h; x.first = q; x.last = q; }
        else if (h == x.m) x.last = q;
    }
    return x;
}

// One wave per tile, one lane per run, as kmer_count.  masks: zeroed; word (first run of the read + q / 64), bit q % 64 <- position q
// of the read is a minimizer.
__global__ __launch_bounds__(kBlock) void kmer_sketch(const uint32_t *__restrict__ packed, const int64_t *__restrict__ woff, const int32_t *__restrict__ len,
                                                      const KmerTile *__restrict__ tiles, int64_t n_tiles, int k, int w, unsigned long long *masks) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (t >= n_tiles) return;
    const KmerTile tile = tiles[t];
    const int32_t npos = len[tile.read] - k;
    const int32_t p0 = tile.start + lane * kRun;
    const int32_t p1 = min(p0 + kRun, npos);
    if (p0 >= p1) return;
    unsigned long long *rmask = masks + (t - tile.start / kTile) * 64;      // the read's first run (its tiles are consecutive)
    if (w == 1) {                                                          // every position, no queue (kmer-cnt/kmer.h:222-229)
        rmask[p0 >> 6] = p1 - p0 == 64 ? ~0ull : (1ull << (p1 - p0)) - 1ull;
        return;
    }
    const uint32_t *words = packed + woff[tile.read];
    KmerRoller R(words, k), S(words, k);
    int32_t f = 0, last = -1;              // p0 = 0: step 0 makes position 0 the front (any key is <= ~0) and emits it
    uint64_t hf = ~0ull;
    auto advance = [&](int32_t p) {        // R.step() gives position p
        R.step();
        const uint64_t h = kmer_order_key(R.canonical());
        if (h < hf) { f = p; hf = h; }
        else if (f <= p - w) {
            const KmerWindowMin x = kmer_window_min(S, p - w + 1, p);
            f = x.last; hf = x.m;
        }
    };
    if (p0 > 0) {
        const int32_t s = p0 - 1, lo = max(0, s - w + 1);
        uint64_t fw_lo, rc_lo;
        const KmerWindowMin x = kmer_window_min(S, lo, s, &fw_lo, &rc_lo);
        hf = x.m;
        int32_t from = p0;                 // the recurrence is played forward from here
        if (lo == 0) f = x.first;
        else if (x.first == x.last) f = x.last;
        else {
            int32_t t2 = s, first = x.first;       // the window of step t2 is [t2 - w + 1, t2], its minimum x.m, the first of them at `first`
            bool at_start = false;
            S.fw = fw_lo; S.rc = rc_lo;
            for (;;) {
                const int32_t q = t2 - w;          // >= 0: the position the window of step t2 - 1 has and this one has not
                S.back(q);
                const uint64_t hq = kmer_order_key(S.canonical());
                if (hq < x.m) break;
                if (hq == x.m) first = q;
                else if (first == t2) break;       // (step t2 - 1 sees no m at all)
                t2--;
                if (t2 - w + 1 == 0) { at_start = true; break; }
            }
            f = at_start ? first : kmer_window_min(S, t2 - w + 1, t2).last;
            from = t2 + 1;
        }
        R.seek(from);
        for (int32_t p = from; p < p0; p++) advance(p);
        last = f;
    } else R.seek(0);
    unsigned long long own = 0;
    for (int32_t p = p0; p < p1; p++) {
        advance(p);
        if (f != last) {
            last = f;
            if (f >= p0) own |= 1ull << (f - p0);
            else atomicOr(&rmask[f >> 6], 1ull << (f & 63));
        }
    }
    if (own) atomicOr(&rmask[p0 >> 6], own);
}

struct KmerPopc {
    __host__ __device__ __forceinline__ uint32_t operator()(unsigned long long m) const {
#ifdef __HIP_DEVICE_COMPILE__
        return (uint32_t)__popcll(m);
#else
        return (uint32_t)__builtin_popcountll(m);
#endif
    }
};

// The second walk over the reads: a lane re-rolls its run from its first marked position to its last and does one of three things
// with every minimizer.  offs: exclusive scan of the popcounts of masks.
enum { kWalkSketch = 0, kWalkCount = 1, kWalkFill = 2 };
//   kWalkSketch  pos[offs + i] = position in the read
//   kWalkCount   canonical k-mer into the table (kmer_insert): cnt = capacity of the key
//   kWalkFill    keys with cnt <= thr: gpos[pad++] = global position (pad was set to the start of the key's list)
// kPart = false: the whole key space in one table (part, nparts and limit are not read).  kPart = true (kWalkCount, kWalkFill): the
// lane hashes the canonical k-mer of a minimizer once, skips it BEFORE it touches the table when the hash falls into another
// partition -- (nparts - 1) / nparts of them, each of which would otherwise pay a random 128-byte line that must miss -- and takes the
// home line from the same hash; the capacity inserts are bounded as those of kmer_count<true> (limit, ct->overflow).  Lanes that
// skip idle while their wave's owners probe.
template <int kMode, bool kPart = false>
__global__ __launch_bounds__(kBlock) void kmer_mini_walk(const uint32_t *__restrict__ packed, const int64_t *__restrict__ woff, const int32_t *__restrict__ len,
                                                         const KmerTile *__restrict__ tiles, int64_t n_tiles, int k,
                                                         const unsigned long long *__restrict__ masks, const uint32_t *__restrict__ offs,
                                                         int32_t *__restrict__ pos, KmerLine *table, uint64_t nlines, KmerCounters *ct,
                                                         const int64_t *__restrict__ rbase, uint32_t thr, int64_t *__restrict__ gpos,
                                                         uint32_t part, uint32_t nparts, uint64_t limit) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (t >= n_tiles) return;
    const KmerTile tile = tiles[t];
    const int32_t L = len[tile.read];
    const int32_t p0 = tile.start + lane * kRun;
    if (p0 >= L - k) return;
    const int64_t run = (t - tile.start / kTile) * 64 + (p0 >> 6);
    unsigned long long m = masks[run];
    if (!m) return;
    const int lead = __builtin_ctzll(m);
    m >>= lead;
    KmerRoller R(packed + woff[tile.read], k);
    R.seek(p0 + lead);
    uint32_t o = offs[run], probes = 0;
    const int64_t base = kMode == kWalkFill ? rbase[tile.read] : 0;
    for (int32_t p = p0 + lead; m; p++, m >>= 1) {
        R.step();
        if (!(m & 1)) continue;
        if constexpr (kMode == kWalkSketch) pos[o++] = p;
        else if constexpr (kMode == kWalkCount) {
            const uint64_t key = R.canonical();
            uint64_t home;
            if (kmer_home<kPart>(key, part, nparts, nlines, &home)) kmer_insert<kPart>(table, nlines, home, key, 1u, probes, limit, ct);
        } else {
            const uint64_t key = R.canonical();
            uint64_t home;
            int slot = 0;
            KmerLine *line = nullptr;
            if (kmer_home<kPart>(key, part, nparts, nlines, &home)) line = kmer_find(table, nlines, home, key, &slot);
            if (line && line->cnt[slot] <= thr) {
                const uint32_t at = atomicAdd(&line->pad[slot], 1u);
                gpos[at] = R.forward() ? base + p : base + L + (L - p - k);
            }
        }
    }
}

// read_start[r] = minimizers before read r (first_run[r] = the runs before it; first_run[n_reads] = all runs)
__global__ __launch_bounds__(kBlock) void kmer_read_starts(const uint32_t *__restrict__ offs, const int64_t *__restrict__ first_run, int64_t n,
                                                           int64_t *__restrict__ read_start) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) read_start[i] = (int64_t)offs[first_run[i]];
}

// every taken slot as (key, slot index), unordered.  A thread takes a whole line (its taken slots are a prefix), the block adds its
// lines up in LDS and draws ONE range from the counter per round: the table has two slots per k-mer POSITION of the call and few
// of them are taken, so a draw per wave would be millions of atomics on one address.
__global__ __launch_bounds__(kBlock) void kmer_index_compact(const KmerLine *__restrict__ table, uint64_t nlines, uint64_t *__restrict__ keys,
                                                             uint64_t *__restrict__ slots, uint32_t capacity, KmerCounters *ct) {
    __shared__ uint32_t wave_sum[kBlock / 64], wave_base[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t rounds = (nlines + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t i = r * stride + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
        unsigned long long key[kSlots] = {0, 0, 0, 0, 0, 0, 0, 0};      // (a thread past the last line takes part in the sums with nothing)
        uint32_t c = 0;
        if (i < nlines) {
            const kmer_ull2 *src = reinterpret_cast<const kmer_ull2 *>(table[i].key);
#pragma unroll
            for (int j = 0; j < kSlots / 2; j++) { const kmer_ull2 v = src[j]; key[2 * j] = v.x; key[2 * j + 1] = v.y; }
#pragma unroll
            for (int j = 0; j < kSlots; j++) c += key[j] != 0;
        }
        uint32_t incl = c;                         // inclusive sum over the lanes of the wave
        for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if (lane >= d) incl += t; }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0;
            for (int w = 0; w < kBlock / 64; w++) total += wave_sum[w];
            uint32_t at = total ? atomicAdd(&ct->dump_n, total) : 0;
            for (int w = 0; w < kBlock / 64; w++) { wave_base[w] = at; at += wave_sum[w]; }
        }
        __syncthreads();
        uint32_t at = wave_base[wave] + incl - c;
#pragma unroll
        for (int j = 0; j < kSlots; j++)
            if (key[j] != 0 && at < capacity) { keys[at] = key[j] - 1; slots[at] = i * kSlots + j; at++; }
        __syncthreads();                           // (the next round writes wave_sum again)
    }
}

// keys in ascending order: weight[i] = (1 << 32 | capacity) of a kept key, 0 of a removed one; weight[n] = 0 (the scan's total lands there)
__global__ __launch_bounds__(kBlock) void kmer_index_weigh(const KmerLine *__restrict__ table, const uint64_t *__restrict__ slots, int64_t n, uint32_t thr,
                                                           uint64_t *__restrict__ weight) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    uint64_t v = 0;
    if (i < n) {
        const uint32_t c = table[slots[i] / kSlots].cnt[slots[i] % kSlots];
        if (c <= thr) v = (1ull << 32) | c;
    }
    weight[i] = v;
}

// scan = exclusive scan of weight: high word = kept keys before i, low word = entries before i.  Writes the kept keys and the start
// of their lists in order, the start of every key's list (kept or not: a removed key's list is empty) for the segmented sort, and
// the start of the list into the key's own slot, where the fill pass counts it up.
__global__ __launch_bounds__(kBlock) void kmer_index_assign(KmerLine *table, const uint64_t *__restrict__ keys, const uint64_t *__restrict__ slots,
                                                            const uint64_t *__restrict__ weight, const uint64_t *__restrict__ scan, int64_t n,
                                                            uint64_t *__restrict__ kmers, int64_t *__restrict__ start, uint32_t *__restrict__ seg,
                                                            KmerCounters *ct) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    const uint64_t rank = scan[i] >> 32, off = scan[i] & 0xFFFFFFFFull;
    seg[i] = (uint32_t)off;
    if (i == n) { start[rank] = (int64_t)off; ct->ix_kmers = rank; ct->ix_entries = off; return; }
    if (weight[i]) {
        kmers[rank] = keys[i];
        start[rank] = (int64_t)off;
        table[slots[i] / kSlots].pad[slots[i] % kSlots] = (uint32_t)off;
    }
}

// first[i] = start of the list of the canonical form of kmers[i] in the dump's order, count[i] its length; an absent or removed
// k-mer: -1 and 0; repetitive[i] = 1 for a removed one.  After the fill pass pad = END of the key's list.
// kPart: the index of one partition; a key of another partition is absent, and is answered without a probe.
template <bool kPart>
__global__ __launch_bounds__(kBlock) void kmer_index_lookup(KmerLine *table, uint64_t nlines, int k, uint32_t thr, const uint64_t *__restrict__ kmers,
                                                            int64_t n, int64_t *__restrict__ first, int32_t *__restrict__ count,
                                                            uint8_t *__restrict__ repetitive, KmerCounters *ct, uint32_t part, uint32_t nparts) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t x = kmers[i];
    first[i] = -1; count[i] = 0; repetitive[i] = 0;
    if (x >> (2 * k)) { atomicMin(&ct->bad_query, (unsigned long long)i); return; }
    const uint64_t r = kmer_revcomp(x, k);
    int slot = 0;
    const uint64_t key = x < r ? x : r;
    uint64_t line;
    if (!kmer_home<kPart>(key, part, nparts, nlines, &line)) return;
    const KmerLine *L = kmer_find(table, nlines, line, key, &slot);
    if (!L) return;
    const uint32_t c = L->cnt[slot];
    if (c > thr) { repetitive[i] = 1; return; }
    first[i] = (int64_t)(L->pad[slot] - c);
    count[i] = (int32_t)c;
}

// =========================================================================================================================== solid index
// buildIndexUnevenCoverage(globalMinFreq, selectRate, tandemFreq) (kmer-cnt/vertex_index.cpp:30-130) with its selector
// yieldFrequentKmers (kmer-cnt/vertex_index.cpp:321-363), on the same packed reads, tiles, bitmap and table.  What is new is the
// producer of the bitmap: per read, the positions whose canonical k-mer has a global count of at least the read's cut -- the count
// of rank (size_t)(selectRate * n) among the read's n counts in descending order -- and of at least min_freq, minus the positions
// whose k-mer occurs more than tandem_freq times in the read itself.
//   kmer_solid_freq     one wave per tile, one lane per run, as kmer_count: freq[first position of the read + p] = c(k-mer at p); a
//                       lane probes the count table once per stretch of equal keys of its run
//   kmer_solid_select   one block per read.  The cut is an exact order statistic: four passes over the read's counts, most
//                       significant byte first, each a 256-bin histogram in LDS of the counts that share the bytes found so far,
//                       so the digit boundaries lie at 2^8, 2^16 and 2^24.  Then one ballot per run writes the bitmap word of the
//                       positions that pass on their count alone.  A position with c(x) <= tandem_freq cannot occur more often
//                       than that in its read, so only the others ("need") take the multiplicity test: their keys are counted in an LDS table of
//                       kSolidSlots entries and looked up again.  When the read has more such distinct keys than kSolidFill the
//                       block splits them by hash into P = 2, 4, ... classes and runs one count-and-mark pass per class, doubling P until
//                       every class fits: exact at any size, at P times the rolling (ct->sx_fallback counts those reads).
constexpr int kSolidSlots = 2048;
constexpr int kSolidFill = kSolidSlots * 3 / 4;        // claims allowed: kSolidFill + kBlock racing lanes still leave empty slots
constexpr uint32_t kSolidMaxClasses = 1u << 20;
struct KmerSolidRule { float select_rate; uint32_t min_freq, tandem; int32_t min_len; };      // tandem = 0: no multiplicity test

__global__ __launch_bounds__(kBlock) void kmer_solid_freq(const uint32_t *__restrict__ packed, const int64_t *__restrict__ woff, const int32_t *__restrict__ len,
                                                          const KmerTile *__restrict__ tiles, int64_t n_tiles, int k, const KmerLine *__restrict__ table,
                                                          uint64_t nlines, uint32_t *__restrict__ freq) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (t >= n_tiles) return;
    const KmerTile tile = tiles[t];
    const int32_t npos = len[tile.read] - k;
    const int32_t p0 = tile.start + lane * kRun;
    const int32_t p1 = min(p0 + kRun, npos);
    if (p0 >= p1) return;
    uint32_t *out = freq + (t - tile.start / kTile) * kTile;       // the read's first position (its tiles are consecutive)
    KmerRoller R(packed + woff[tile.read], k);
    R.seek(p0);
    uint64_t cur = ~0ull;
    uint32_t c = 0;
    for (int32_t p = p0; p < p1; p++) {
        R.step();
        const uint64_t key = R.canonical();
        if (key != cur) {
            cur = key;
            int slot = 0;
            const KmerLine *L = kmer_find(table, nlines, kmer_line_of(key, nlines), key, &slot);
            c = L ? L->cnt[slot] : 0;
        }
        out[p] = c;
    }
}

__global__ __launch_bounds__(kBlock) void kmer_solid_select(const uint32_t *__restrict__ packed, const int64_t *__restrict__ woff, const int32_t *__restrict__ len,
                                                            const int64_t *__restrict__ first_run, int k, KmerSolidRule rule, const uint32_t *__restrict__ freq,
                                                            unsigned long long *masks, KmerCounters *ct) {
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long tkey[kSolidSlots];
    __shared__ uint32_t tcnt[kSolidSlots];
    __shared__ uint32_t sh_prefix, sh_rank, sh_used, sh_over, sh_need;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const int32_t L = len[r], n = L - k;
    if (L <= rule.min_len || n <= 0) return;
    const uint32_t *f = freq + first_run[r] * kRun;
    unsigned long long *rmask = masks + first_run[r];
    if (tid == 0) sh_need = 0;

    // ---- the cut: rank maxKmers of the counts in descending order = rank n - 1 - maxKmers in ascending order
    uint32_t maxk = (uint32_t)__fmul_rn(rule.select_rate, (float)n);      // (size_t)(selectRate * topKmers.size()): one float product, truncated
    if (maxk >= (uint32_t)n) maxk = (uint32_t)n - 1;                      // (there the reference reads past its array)
    uint32_t prefix = 0, rank = (uint32_t)n - 1 - maxk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int j = tid; j < 256; j += kBlock) hist[j] = 0;
        __syncthreads();
        const uint32_t above = shift == 24 ? 0u : ~0u << (shift + 8);
        for (int32_t base = 0; base < n; base += kBlock) {                 // (whole waves take every round: ballots)
            const int32_t p = base + tid;
            const uint32_t v = p < n ? f[p] : 0u;
            const bool in = p < n && (v & above) == prefix;
            const uint32_t d = (v >> shift) & 255u;
            const unsigned long long act = __ballot(in);
            if (act) {                                                     // the lanes of a wave mostly share a digit: one add for them
                const int lead = __builtin_ctzll(act);
                const uint32_t d0 = __shfl(d, lead);
                const unsigned long long same = __ballot(in && d == d0);
                if (lane == lead) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
                if (in && d != d0) atomicAdd(&hist[d], 1u);
            }
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = 0;
            int b = 0;
            for (; b < 255 && cum + hist[b] <= rank; b++) cum += hist[b];
            sh_prefix = prefix | ((uint32_t)b << shift); sh_rank = rank - cum;
        }
        __syncthreads();
        prefix = sh_prefix; rank = sh_rank;
    }
    const uint32_t cut = max(prefix, rule.min_freq);

    // ---- the positions that pass on their count alone; the others of the read's top counts need the multiplicity test
    const int32_t nruns = (n + kRun - 1) / kRun;
    uint32_t need = 0;
    for (int32_t run = wave; run < nruns; run += kBlock / 64) {
        const int32_t p = run * kRun + lane;
        const uint32_t v = p < n ? f[p] : 0u;
        const bool top = p < n && v >= cut;
        const bool test = top && rule.tandem && v > rule.tandem;
        const unsigned long long m = __ballot(top && !test);
        need += (uint32_t)__popcll(__ballot(test));
        if (lane == 0) rmask[run] = m;
    }
    if (lane == 0 && need) atomicAdd(&sh_need, need);
    __syncthreads();
    if (!sh_need) return;
    if (tid == 0) atomicAdd(&ct->sx_need, (unsigned long long)sh_need);

    // ---- the multiplicity test.  Runs go to the waves in chunks of 64: one ballot per run, lane i keeps the word of the chunk's run i
    // and rolls that run.  Every occurrence of a key in the read has the key's global count, so either all of them are here or none.
    const int32_t nchunks = (nruns + 63) / 64;
    auto chunk_word = [&](int32_t chunk) {
        unsigned long long mine = 0;
        for (int i = 0; i < 64 && chunk * 64 + i < nruns; i++) {
            const int32_t p = (chunk * 64 + i) * kRun + lane;
            const uint32_t v = p < n ? f[p] : 0u;
            const unsigned long long b = __ballot(p < n && v >= cut && v > rule.tandem);
            if (lane == i) mine = b;
        }
        return mine;
    };
    const uint32_t *words = packed + woff[r];
    uint32_t classes = 1, cls = 0;
    while (cls < classes) {
        for (int j = tid; j < kSolidSlots; j += kBlock) { tkey[j] = 0; tcnt[j] = 0; }
        if (tid == 0) { sh_used = 0; sh_over = 0; }
        __syncthreads();
        for (int32_t chunk = wave; chunk < nchunks; chunk += kBlock / 64) {
            unsigned long long m = chunk_word(chunk);
            const int lead = m ? __builtin_ctzll(m) : 0;
            m >>= lead;
            KmerRoller R(words, k);
            if (m) R.seek((chunk * 64 + lane) * kRun + lead);
            for (; m; m >>= 1) {
                R.step();
                if (!(m & 1)) continue;
                const uint64_t key = R.canonical(), h = kmer_hash(key);
                if (((uint32_t)(h >> 40) & (classes - 1)) != cls) continue;
                if (*(volatile uint32_t *)&sh_over) break;
                const unsigned long long stored = key + 1;
                for (uint32_t s = (uint32_t)h & (kSolidSlots - 1);; s = (s + 1) & (kSolidSlots - 1)) {
                    const unsigned long long seen = atomicCAS(&tkey[s], 0ull, stored);
                    if (seen == 0 && atomicAdd(&sh_used, 1u) >= (uint32_t)kSolidFill) sh_over = 1;
                    if (seen == 0 || seen == stored) { atomicAdd(&tcnt[s], 1u); break; }
                }
            }
        }
        __syncthreads();
        if (sh_over) {                                 // more distinct keys than the table takes: twice the classes, from the first one
            __syncthreads();                           // (everyone has read sh_over before it is cleared)
            classes *= 2; cls = 0;
            if (classes > kSolidMaxClasses) { if (tid == 0) atomicOr(&ct->overflow, 1u); return; }
            continue;
        }
        for (int32_t chunk = wave; chunk < nchunks; chunk += kBlock / 64) {
            unsigned long long m = chunk_word(chunk), keep = 0;
            const int lead = m ? __builtin_ctzll(m) : 0;
            m >>= lead;
            KmerRoller R(words, k);
            if (m) R.seek((chunk * 64 + lane) * kRun + lead);
            for (int bit = lead; m; m >>= 1, bit++) {
                R.step();
                if (!(m & 1)) continue;
                const uint64_t key = R.canonical(), h = kmer_hash(key);
                if (((uint32_t)(h >> 40) & (classes - 1)) != cls) continue;
                uint32_t s = (uint32_t)h & (kSolidSlots - 1);
                while (tkey[s] != key + 1) s = (s + 1) & (kSolidSlots - 1);       // (the pass above put it there)
                if (tcnt[s] <= rule.tandem) keep |= 1ull << bit;
            }
            if (keep) rmask[chunk * 64 + lane] |= keep;          // (this lane owns the run's word in every pass)
        }
        __syncthreads();
        cls++;
    }
    if (tid == 0 && classes > 1) atomicAdd(&ct->sx_fallback, 1ull);
}

// the filter's totals over the capacity table (filterFrequentKmers, kmer-cnt/vertex_index.cpp:180-189): every key counts as a
// candidate, only capacities >= min_freq enter the mean
__global__ __launch_bounds__(kBlock) void kmer_solid_reduce(const KmerLine *__restrict__ table, uint64_t nslots, uint32_t min_freq, KmerCounters *ct) {
    unsigned long long distinct = 0, total = 0, unique = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * kBlock) {
        const KmerLine *L = table + i / kSlots;
        const int s = (int)(i % kSlots);
        if (L->key[s]) {
            const unsigned long long c = L->cnt[s];
            distinct++;
            if (c >= min_freq) { total += c; unique++; }
        }
    }
    for (int d = 32; d; d >>= 1) { distinct += __shfl_xor(distinct, d); total += __shfl_xor(total, d); unique += __shfl_xor(unique, d); }
    if ((threadIdx.x & 63) == 0 && distinct) {
        atomicAdd(&ct->distinct, distinct);
        if (unique) { atomicAdd(&ct->sx_total, total); atomicAdd(&ct->sx_unique, unique); }
    }
}

// kmer_index_weigh for the solid index: a key that stays (capacity <= thr) gets its capacity in slots only if its global count is
// <= thr too -- the second pass of the reference skips by global count (kmer-cnt/vertex_index.cpp:78-79) -- and an empty list
// otherwise.  counts: the table of the call's count, still alive.  n is rounded up to whole waves by the launch.
__global__ __launch_bounds__(kBlock) void kmer_solid_weigh(const KmerLine *__restrict__ table, const uint64_t *__restrict__ keys, const uint64_t *__restrict__ slots,
                                                           int64_t n, uint32_t thr, const KmerLine *__restrict__ counts, uint64_t count_lines,
                                                           uint64_t *__restrict__ weight, KmerCounters *ct) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint64_t v = 0;
    unsigned long long empty = 0, empty_cap = 0;
    if (i < n) {
        const uint32_t c = table[slots[i] / kSlots].cnt[slots[i] % kSlots];
        if (c <= thr) {
            int slot = 0;
            const KmerLine *L = kmer_find(counts, count_lines, kmer_line_of(keys[i], count_lines), keys[i], &slot);
            const bool full = L && L->cnt[slot] <= thr;
            v = full ? (1ull << 32) | c : 0;
            empty = full ? 0 : 1;
            empty_cap = full ? 0 : c;
        }
    }
    if (i <= n) weight[i] = v;
    for (int d = 32; d; d >>= 1) { empty += __shfl_xor(empty, d); empty_cap += __shfl_xor(empty_cap, d); }
    if ((threadIdx.x & 63) == 0 && empty) { atomicAdd(&ct->sx_empty, empty); atomicAdd(&ct->sx_empty_cap, empty_cap); }
}

// after kmer_index_assign: the keys with an empty list leave the table -- a look-up then reads them as absent and the fill pass
// passes them by.  Their slots stay taken (by a value no key + 1 equals), so the taken slots of a line are still a prefix.
__global__ __launch_bounds__(kBlock) void kmer_solid_retire(KmerLine *table, const uint64_t *__restrict__ slots, const uint64_t *__restrict__ weight, int64_t n,
                                                            uint32_t thr) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || weight[i]) return;
    KmerLine *L = table + slots[i] / kSlots;
    if (L->cnt[slots[i] % kSlots] <= thr) L->key[slots[i] % kSlots] = ~0ull;
}

struct KmerDev {           // where the stage put things (kmer_stage: the first line; kmer_mini_stage: all of it)
    int64_t *woff; KmerTile *tiles; uint32_t *packed; int64_t n_tiles, n_runs;
    unsigned long long *masks; uint32_t *offs; int64_t *rbase, *first_run;
};

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
    hipEvent_t ev[17] = {};            // count: start | packed | counted | reduced | end; then the six of the index (ev_ix) and of the solid front (ev_sx)
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
    // minimizer index (gab_kmer_index_minimizers): it takes the table over, so `counted` and `indexed` are never both set
    gab_devbuf mini;        // sketch: bitmap of the minimizers | its scan | per-read bases
    gab_devbuf idx;         // the index of the last build: k-mers | starts | global positions
    hipEvent_t *const ev_ix = ev + 5;  // start | sketched | counted | resumed | filled | sorted
    bool indexed = false;
    gab_kmer_index_result ix = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t ix_thr = 0;               // min(repetitive_frequency, 2^32 - 1): what the kernels compare the 32-bit capacities with
    float ix_ms[4] = {0, 0, 0, 0};     // sketch | count | fill | sort
    // solid index (gab_kmer_index_solid): the count table and the capacity table are alive together; the build ends with the capacity
    // table in `table` (it is the index's) and the counts dropped, so afterwards `indexed` is set as after a minimizer build
    gab_devbuf cap;         // the second table: the capacities during a solid build, the counts of gab_kmer_solid_positions
    gab_devbuf freq;        // c(x) of every position, read by read
    hipEvent_t *const ev_sx = ev + 11; // start | counted | selected | capacities (the later stages: ev_ix[3..5])
    bool solid = false;                // the index in the handle came from gab_kmer_index_solid
    gab_kmer_solid_result sx = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float sx_ms[3] = {0, 0, 0};        // count | look-up + selection | capacity
    int64_t sx_need = 0, sx_fallback = 0;
    // between gab_kmer_index_part_begin and _finish: packed, plan, mini and table (and io for the host form) hold what the stage and
    // the capacity walk left there, and these say where; neither `counted` nor `indexed` is set meanwhile
    struct Pending {
        bool on = false;
        KmerDev dev = {};
        const int32_t *d_len = nullptr;    // the handle's staging buffer (host form) or the caller's array (device form)
        hipStream_t stream = nullptr;
        int64_t kept = 0, total_len = 0, minimizers = 0, distinct = 0;     // the whole call's | the partition's own
    } pend;
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
    for (hipEvent_t &e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) { gab_set_error("hipEventCreate failed"); gab_kmer_destroy(h); return GAB_EDEVICE; }
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
    h->io.release(); h->packed.release(); h->plan.release(); h->table.release(); h->ct.release(); h->aux.release(); h->mini.release(); h->idx.release(); h->cap.release(); h->freq.release();
    h->hs.release();
    for (hipEvent_t e : h->ev) if (e) (void)hipEventDestroy(e);
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

// ---- the front half of every call: input, plan, stage, first table ---------------------------------------------------------------------
namespace {

// The reads of one call.  d_*: device; off / len: the same two arrays on the host.
struct KmerInput {
    const char *d_seq = nullptr; int64_t seq_bytes = 0;
    const int64_t *d_off = nullptr; const int32_t *d_len = nullptr;
    const int64_t *off = nullptr; const int32_t *len = nullptr;
    int64_t n_reads = 0;
    hipStream_t stream = nullptr;
    std::vector<int64_t> h_off;            // owner of `off` (host form: the offsets relative to the staged window) ...
    std::vector<int32_t> h_len;            // ... and, in the device form, of `len`
};

// The host-pointer entry points: on the handle's stream, the window of the slab that the reads span, their offsets relative to it
// and their lengths go into the handle's staging buffer.
int kmer_input_host(gab_kmer *h, const char *fn, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, KmerInput *in) {
    int rc;
    hipStream_t s;
    if ((rc = h->hs.get(&s))) return rc;
    h->pend.on = false;                                            // (a pending partitioned index build keeps its lengths in `io`)
    int64_t lo = INT64_MAX, hi = 0;                                // the window of the slab the reads span
    for (int64_t r = 0; r < n_reads; r++) {
        GAB_CHECK(len[r] >= 0 && off[r] >= 0, "%s: read %lld has a negative offset or length", fn, (long long)r);
        if (len[r] == 0) continue;
        lo = std::min(lo, off[r]); hi = std::max(hi, off[r] + len[r]);
    }
    if (hi == 0) lo = 0;
    GAB_CHECK(seq || hi == 0, "%s: NULL sequence slab", fn);
    const size_t span = (size_t)(hi - lo);
    const size_t off_at = align256(span + 64), len_at = off_at + align256((size_t)n_reads * 8);
    if ((rc = h->io.reserve(len_at + align256((size_t)n_reads * 4)))) return rc;
    char *d_seq = h->io.as<char>();
    int64_t *d_off = reinterpret_cast<int64_t *>(d_seq + off_at);
    int32_t *d_len = reinterpret_cast<int32_t *>(d_seq + len_at);
    std::vector<int64_t> &rel = in->h_off;
    rel.assign((size_t)n_reads, 0);
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
    in->d_seq = d_seq; in->seq_bytes = (int64_t)span; in->d_off = d_off; in->d_len = d_len;
    in->off = rel.data(); in->len = len; in->n_reads = n_reads; in->stream = s;
    return GAB_OK;
}

// The device-pointer entry points: everything stays where it is, on the caller's stream; the plan needs off and len on the host.
int kmer_input_device(const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads, void *stream, KmerInput *in) {
    hipStream_t s = (hipStream_t)stream;
    in->h_off.resize((size_t)n_reads); in->h_len.resize((size_t)n_reads);
    if (n_reads) {
        GAB_HIP(hipMemcpyAsync(in->h_off.data(), off, (size_t)n_reads * 8, hipMemcpyDeviceToHost, s));
        GAB_HIP(hipMemcpyAsync(in->h_len.data(), len, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    in->d_seq = seq; in->seq_bytes = seq_bytes; in->d_off = off; in->d_len = len;
    in->off = in->h_off.data(); in->len = in->h_len.data(); in->n_reads = n_reads; in->stream = s;
    return GAB_OK;
}

// The plan of a call, made on the host: the word offset of every read, the tiles of the kept ones, and what the minimizer paths
// need on top of that.
struct KmerPlan {
    std::vector<int64_t> woff, rbase, first_run;   // word offset | 2 S_i of a kept read | runs before the read (n_reads + 1)
    std::vector<KmerTile> tiles;
    int64_t words = 0, positions = 0, kept = 0, total_len = 0;
};

// global_positions (the sketch and the index): the kept reads must fit the 40 bits of a global position
int kmer_plan(const char *fn, const KmerInput &in, int k, int32_t min_len_exclusive, bool global_positions, KmerPlan *P) {
    const int64_t n_reads = in.n_reads;
    const int64_t *off = in.off;
    const int32_t *len = in.len;
    GAB_CHECK(n_reads < (1ll << 31), "%s: %lld reads in one call (limit 2^31)", fn, (long long)n_reads);
    P->woff.resize((size_t)n_reads + 1); P->rbase.assign((size_t)n_reads + 1, 0); P->first_run.resize((size_t)n_reads + 1);
    for (int64_t r = 0; r < n_reads; r++) {
        GAB_CHECK(len[r] >= 0 && off[r] >= 0 && off[r] + len[r] <= in.seq_bytes, "%s: read %lld (offset %lld, length %d) lies outside the %lld sequence bytes",
                  fn, (long long)r, (long long)off[r], (int)len[r], (long long)in.seq_bytes);
        P->woff[(size_t)r] = P->words;
        P->words += ((int64_t)len[r] + 15) / 16;
        P->first_run[(size_t)r] = (int64_t)P->tiles.size() * 64;
        if (len[r] > min_len_exclusive) {
            P->kept++;
            P->rbase[(size_t)r] = 2 * P->total_len;
            P->total_len += len[r];
            const int32_t npos = len[r] - k;
            for (int32_t p = 0; p < npos; p += kTile) P->tiles.push_back(KmerTile{(int32_t)r, p});
            if (npos > 0) P->positions += npos;
        }
    }
    P->woff[(size_t)n_reads] = P->words;
    P->first_run[(size_t)n_reads] = (int64_t)P->tiles.size() * 64;
    GAB_CHECK(P->positions < (1ll << 32), "%s: %lld k-mer positions in one call (limit 2^32%s)", fn, (long long)P->positions,
              global_positions ? "" : ": the counts are 32-bit");
    GAB_CHECK(!global_positions || 2 * P->total_len < (1ll << 40),
              "%s: %lld bases in the kept reads (global positions have 40 bits, kmer-cnt/sequence_container.h:266)", fn, (long long)P->total_len);
    return GAB_OK;
}

int kmer_zero_counters(gab_kmer *h, hipStream_t s) {
    KmerCounters zero = {};
    zero.bad_read = ~0ull; zero.bad_query = ~0ull;
    *h->h_ct = zero;
    GAB_HIP(hipMemcpyAsync(h->ct.as<KmerCounters>(), h->h_ct, sizeof(KmerCounters), hipMemcpyHostToDevice, s));
    return GAB_OK;
}

// plan to the device and pack; leaves the zeroed counters in h->ct
// (a bad byte packs as some base: what follows runs on it harmlessly and the call fails after its next synchronisation)
int kmer_stage(gab_kmer *h, const KmerInput &in, const KmerPlan &P, KmerDev *D) {
    int rc;
    const int64_t n_tiles = (int64_t)P.tiles.size();
    const size_t tiles_at = align256(((size_t)in.n_reads + 1) * 8);
    if ((rc = h->packed.reserve((size_t)P.words * 4 + 4))) return rc;
    if ((rc = h->plan.reserve(tiles_at + (size_t)n_tiles * sizeof(KmerTile) + 8))) return rc;
    D->woff = h->plan.as<int64_t>();
    D->tiles = reinterpret_cast<KmerTile *>(h->plan.as<char>() + tiles_at);
    D->packed = h->packed.as<uint32_t>();
    D->n_tiles = n_tiles; D->n_runs = n_tiles * 64;
    if ((rc = kmer_zero_counters(h, in.stream))) return rc;
    GAB_HIP(hipMemcpyAsync(D->woff, P.woff.data(), ((size_t)in.n_reads + 1) * 8, hipMemcpyHostToDevice, in.stream));
    if (n_tiles) GAB_HIP(hipMemcpyAsync(D->tiles, P.tiles.data(), (size_t)n_tiles * sizeof(KmerTile), hipMemcpyHostToDevice, in.stream));
    if (P.words)
        hipLaunchKernelGGL(kmer_pack, dim3((unsigned)gab_ceil_div(P.words, kBlock)), dim3(kBlock), 0, in.stream, in.d_seq, in.d_off, in.d_len, D->woff, in.n_reads,
                           P.words, D->packed, h->ct.as<KmerCounters>());
    return GAB_OK;
}

// The table of a call that may be partitioned.  A partition's first table is a forecast (part_table_lines; GAB_KMER_PART_FLOOR: the
// 16-line floor, test hook of the repeat) and its inserts are bounded: when one gave up, the host sees ct->overflow after the
// attempt's synchronisation and runs the attempt once more, with fresh counters, in a table of table_lines lines, which is at most
// half full whatever the hash does.  attempt(n, limit): clear, walk, reduce and fetch for the table h->table of h->nlines lines;
// n: 0, or 1 for the repeat; limit: the lines a bounded insert may leave.  It synchronises and leaves the counters in h->h_ct.
template <class Attempt>
int kmer_first_table(gab_kmer *h, const char *fn, int64_t positions, int k, int nparts, hipStream_t s, Attempt attempt) {
    int rc;
    gab_tuning_refresh(&h->tun);
    h->nlines = nparts > 1 && h->tun.kmer_part_floor ? 16 : part_table_lines(std::max<int64_t>(positions, 1), k, nparts);
    h->retried = false;
    for (int n = 0;; n++) {
        if ((rc = h->table.reserve((size_t)h->nlines * sizeof(KmerLine)))) return rc;
        if ((rc = attempt(n, n ? h->nlines : std::min<uint64_t>(h->nlines, kProbeCap)))) return rc;
        if (!h->h_ct->overflow) return GAB_OK;
        GAB_CHECK(n == 0, "%s: internal error: a table of %llu lines for %lld positions filled up", fn, (unsigned long long)h->nlines, (long long)positions);
        h->retried = true;
        h->nlines = table_lines(std::max<int64_t>(positions, 1), k);
        if ((rc = kmer_zero_counters(h, s))) return rc;
    }
}

}  // namespace

// part / nparts: the partition of the key space this call counts (0 / 1: all of it, in the unpartitioned kernel)
static int kmer_count_impl(gab_kmer *h, const KmerInput &in, int k, int32_t min_len_exclusive, int part, int nparts, gab_kmer_result *res) {
    h->counted = false; h->indexed = false; h->pend.on = false;
    hipStream_t s = in.stream;
    KmerPlan P;
    KmerDev D = {};
    int rc;
    if ((rc = kmer_plan("gab_kmer_count", in, k, min_len_exclusive, false, &P))) return rc;
    KmerCounters *d_ct = h->ct.as<KmerCounters>();
    GAB_HIP(hipEventRecord(h->ev[0], s));
    if ((rc = kmer_stage(h, in, P, &D))) return rc;
    GAB_HIP(hipEventRecord(h->ev[1], s));
    rc = kmer_first_table(h, "gab_kmer_count", P.positions, k, nparts, s, [&](int attempt, uint64_t limit) -> int {
        KmerLine *table = h->table.as<KmerLine>();
        if (attempt) GAB_HIP(hipEventRecord(h->ev[1], s));        // (after a repeat pack_ms includes the first attempt)
        GAB_HIP(hipMemsetAsync(table, 0, (size_t)h->nlines * sizeof(KmerLine), s));
        if (D.n_tiles) {
            const dim3 grid((unsigned)gab_ceil_div(D.n_tiles, kBlock / 64));
            if (nparts == 1)
                hipLaunchKernelGGL(kmer_count<false>, grid, dim3(kBlock), 0, s, D.packed, D.woff, in.d_len, D.tiles, D.n_tiles, k, table, h->nlines, d_ct, 0u, 1u,
                                   (uint64_t)0);
            else
                hipLaunchKernelGGL(kmer_count<true>, grid, dim3(kBlock), 0, s, D.packed, D.woff, in.d_len, D.tiles, D.n_tiles, k, table, h->nlines, d_ct,
                                   (uint32_t)part, (uint32_t)nparts, limit);
        }
        GAB_HIP(hipEventRecord(h->ev[2], s));
        hipLaunchKernelGGL(kmer_reduce<false>, dim3(sweep_grid(h)), dim3(kBlock), 0, s, table, h->nlines * kSlots, d_ct);
        GAB_HIP(hipEventRecord(h->ev[3], s));
        GAB_HIP(hipMemcpyAsync(h->h_ct, d_ct, sizeof(KmerCounters), hipMemcpyDeviceToHost, s));
        GAB_HIP(hipEventRecord(h->ev[4], s));
        GAB_HIP(hipStreamSynchronize(s));
        GAB_HIP(hipGetLastError());
        GAB_CHECK(h->h_ct->bad_read == ~0ull, "gab_kmer_count: read %lld holds a byte outside ACGTacgt (a driver replaces such bytes before the call)",
                  (long long)h->h_ct->bad_read);
        return GAB_OK;
    });
    if (rc) return rc;
    const KmerCounters &c = *h->h_ct;
    h->last = gab_kmer_result{P.kept, P.positions, (int64_t)c.distinct, (int64_t)c.total_kmers, (int64_t)c.hash_size, (int64_t)c.max_count};
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
    KmerInput in;
    if ((rc = kmer_input_device(seq, seq_bytes, off, len, n_reads, stream, &in))) return rc;
    return kmer_count_impl(h, in, k, min_len_exclusive, part, nparts, res);
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
    KmerInput in;
    if ((rc = kmer_input_host(h, "gab_kmer_count", seq, off, len, n_reads, &in))) return rc;
    return kmer_count_impl(h, in, k, min_len_exclusive, part, nparts, res);
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

static int kmer_last_part(gab_kmer *h, int *part, int *nparts, int64_t *table_slots, int *retried) {
    if (part) *part = h->part;
    if (nparts) *nparts = h->nparts;
    if (table_slots) *table_slots = (int64_t)(h->nlines * kSlots);
    if (retried) *retried = h->retried ? 1 : 0;
    return GAB_OK;
}

extern "C" int gab_kmer_last_part(gab_kmer *h, int *part, int *nparts, int64_t *table_slots, int *retried) {
    KMER_NEED_COUNT("gab_kmer_last_part");
    return kmer_last_part(h, part, nparts, table_slots, retried);
}

// =============================================================================== minimizer index, host side
// Stages of gab_kmer_index_minimizers (all on the caller's stream):
//   kmer_pack, kmer_sketch, a scan of the bitmap's popcounts                                              "sketch"
//   table clear, kmer_mini_walk<kWalkCount> (capacity of every key), kmer_reduce (distinct)               "count"
//   -- the one synchronisation in the middle: the host needs the two integers for repetitive_frequency --
//   every key with its slot, sorted by key; (kept, capacity) scanned in that order: the rank of a kept key and the start of its
//   list; both written out and the start put into the key's slot; kmer_mini_walk<kWalkFill> counts it up                  "fill"
//   one segmented sort over the lists (a removed key has an empty one)                                     "sort"
// and one synchronisation at the end for the two sizes.  The k-mers, the starts and the sorted lists stay in h->idx, the table
// with the END of every list in its slots stays for gab_kmer_index_lookup.
// In key-space partitions the build is cut at the synchronisation in the middle: gab_kmer_index_part_begin is everything before it,
// with the capacity walk and the table restricted to the keys of one partition (kmer_index_begin_impl), the caller adds up the two
// integers of all partitions, and gab_kmer_index_part_finish is everything after it (kmer_index_layout, shared with the
// unpartitioned build) over the partition's own keys and entries, with the threshold of the whole input.
namespace {

int kmer_mini_check(const char *fn, gab_kmer *h, const void *off, const void *len, int64_t n_reads, int k, int window) {
    GAB_CHECK(h && n_reads >= 0 && (n_reads == 0 || (off && len)), "%s: NULL or negative argument", fn);
    GAB_CHECK(k >= 1 && k <= GAB_KMER_MAX_K, "%s: k = %d, supported 1..%d", fn, k, GAB_KMER_MAX_K);
    GAB_CHECK(window >= 1 && window <= GAB_KMER_MAX_WINDOW, "%s: window = %d, supported 1..%d (yieldMinimizers takes any window >= 1, kmer-cnt/kmer.h:208)", fn,
              window, GAB_KMER_MAX_WINDOW);
    return GAB_OK;
}

// The bitmap of chosen positions of a call, one 64-bit word per run: kmer_stage plus the zeroed bitmap, the room of its scan and the
// per-read bases (rbase and first_run go up first: a copy behind the pack kernel would hold the marking kernel back) ...
struct KmerBitmapScan { void *tmp; size_t tmp_bytes; };
int kmer_bitmap_stage(gab_kmer *h, const KmerInput &in, const KmerPlan &P, KmerDev *D, KmerBitmapScan *B) {
    int rc;
    hipStream_t s = in.stream;
    const int64_t n_reads = in.n_reads, n_tiles = (int64_t)P.tiles.size(), n_runs = n_tiles * 64;
    size_t tmp_bytes = 0;
    GAB_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, rocprim::make_transform_iterator((const unsigned long long *)nullptr, KmerPopc()), (uint32_t *)nullptr, 0u,
                                    (size_t)n_runs + 1, rocprim::plus<uint32_t>(), s));
    const size_t offs_at = align256(((size_t)n_runs + 1) * 8), rbase_at = offs_at + align256(((size_t)n_runs + 1) * 4);
    const size_t first_at = rbase_at + align256(((size_t)n_reads + 1) * 8), tmp_at = first_at + align256(((size_t)n_reads + 1) * 8);
    if ((rc = h->mini.reserve(tmp_at + tmp_bytes + 256))) return rc;
    char *mb = h->mini.as<char>();
    D->masks = reinterpret_cast<unsigned long long *>(mb);
    D->offs = reinterpret_cast<uint32_t *>(mb + offs_at);
    D->rbase = reinterpret_cast<int64_t *>(mb + rbase_at);
    D->first_run = reinterpret_cast<int64_t *>(mb + first_at);
    GAB_HIP(hipMemcpyAsync(D->rbase, P.rbase.data(), ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(D->first_run, P.first_run.data(), ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = kmer_stage(h, in, P, D))) return rc;
    GAB_HIP(hipMemsetAsync(D->masks, 0, ((size_t)n_runs + 1) * 8, s));
    B->tmp = mb + tmp_at; B->tmp_bytes = tmp_bytes;
    return GAB_OK;
}
// ... and, once a kernel has marked the positions, offs = the exclusive scan of the words' popcounts
int kmer_bitmap_scan(const KmerDev &D, KmerBitmapScan B, hipStream_t s) {
    GAB_HIP(rocprim::exclusive_scan(B.tmp, B.tmp_bytes, rocprim::make_transform_iterator((const unsigned long long *)D.masks, KmerPopc()), D.offs, 0u,
                                    (size_t)D.n_runs + 1, rocprim::plus<uint32_t>(), s));
    return GAB_OK;
}

// kmer_bitmap_stage, sketch, scan
int kmer_mini_stage(gab_kmer *h, const KmerInput &in, const KmerPlan &P, int k, int window, KmerDev *D) {
    int rc;
    KmerBitmapScan B;
    if ((rc = kmer_bitmap_stage(h, in, P, D, &B))) return rc;
    if (D->n_tiles)
        hipLaunchKernelGGL(kmer_sketch, dim3((unsigned)gab_ceil_div(D->n_tiles, kBlock / 64)), dim3(kBlock), 0, in.stream, D->packed, D->woff, in.d_len, D->tiles,
                           D->n_tiles, k, window, D->masks);
    return kmer_bitmap_scan(*D, B, in.stream);
}

// the counters and the number of minimizers (the scan's last element) to the host; synchronises
int kmer_mini_fetch(gab_kmer *h, const char *fn, const KmerDev &D, hipStream_t s) {
    GAB_HIP(hipMemcpyAsync(h->h_ct, h->ct.as<KmerCounters>(), sizeof(KmerCounters), hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(&h->h_ct->ix_minimizers, D.offs + D.n_runs, 4, hipMemcpyDeviceToHost, s));     // (little-endian: the low word)
    GAB_HIP(hipStreamSynchronize(s));
    GAB_HIP(hipGetLastError());
    GAB_CHECK(h->h_ct->bad_read == ~0ull, "%s: read %lld holds a byte outside ACGTacgt (a driver replaces such bytes before the call)", fn,
              (long long)h->h_ct->bad_read);
    return GAB_OK;
}

// h->part of h->nparts (1: the unpartitioned kernel); limit: the lines a bounded capacity insert may leave
template <int kMode>
void kmer_mini_launch_walk(gab_kmer *h, const KmerDev &D, const int32_t *d_len, int k, int32_t *pos, uint32_t thr, int64_t *gpos, hipStream_t s,
                           uint64_t limit = 0) {
    if (!D.n_tiles) return;
    const dim3 grid((unsigned)gab_ceil_div(D.n_tiles, kBlock / 64));
    if (h->nparts == 1)
        hipLaunchKernelGGL((kmer_mini_walk<kMode, false>), grid, dim3(kBlock), 0, s, D.packed, D.woff, d_len, D.tiles, D.n_tiles, k, D.masks, D.offs, pos,
                           h->table.as<KmerLine>(), h->nlines, h->ct.as<KmerCounters>(), D.rbase, thr, gpos, 0u, 1u, (uint64_t)0);
    else
        hipLaunchKernelGGL((kmer_mini_walk<kMode, kMode != kWalkSketch>), grid, dim3(kBlock), 0, s, D.packed, D.woff, d_len, D.tiles, D.n_tiles, k, D.masks, D.offs,
                           pos, h->table.as<KmerLine>(), h->nlines, h->ct.as<KmerCounters>(), D.rbase, thr, gpos, (uint32_t)h->part, (uint32_t)h->nparts, limit);
}

// The marked positions of every read, out of the scanned bitmap: synchronises for their number, then writes read_start and pos
// (out_on_device: they are device pointers) or returns GAB_ERANGE with nothing written.
int kmer_bitmap_emit(gab_kmer *h, const char *fn, const KmerInput &in, const KmerDev &D, int k, int64_t *read_start, int32_t *pos, int64_t capacity,
                     int64_t *nout, bool out_on_device) {
    hipStream_t s = in.stream;
    const int64_t n_reads = in.n_reads;
    int rc;
    if ((rc = kmer_mini_fetch(h, fn, D, s))) return rc;
    const int64_t m = (int64_t)h->h_ct->ix_minimizers;
    *nout = m;
    if (capacity < m) { gab_set_error("%s: %lld positions, room for %lld", fn, (long long)m, (long long)capacity); return GAB_ERANGE; }
    GAB_CHECK(read_start && (pos || m == 0), "%s: NULL output", fn);
    int64_t *d_start = read_start;
    int32_t *d_pos = pos;
    const size_t pos_at = align256(((size_t)n_reads + 1) * 8);
    if (!out_on_device) {
        if ((rc = h->aux.reserve(pos_at + (size_t)m * 4 + 4))) return rc;
        d_start = h->aux.as<int64_t>();
        d_pos = reinterpret_cast<int32_t *>(h->aux.as<char>() + pos_at);
    }
    hipLaunchKernelGGL(kmer_read_starts, dim3((unsigned)gab_ceil_div(n_reads + 1, kBlock)), dim3(kBlock), 0, s, D.offs, D.first_run, n_reads + 1, d_start);
    kmer_mini_launch_walk<kWalkSketch>(h, D, in.d_len, k, d_pos, 0u, nullptr, s);
    if (!out_on_device) {
        GAB_HIP(hipMemcpyAsync(read_start, d_start, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
        if (m) GAB_HIP(hipMemcpyAsync(pos, d_pos, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    }
    GAB_HIP(hipStreamSynchronize(s));
    GAB_HIP(hipGetLastError());
    return GAB_OK;
}

// out_on_device: read_start / pos are device pointers
int kmer_sketch_impl(gab_kmer *h, const KmerInput &in, int k, int window, int32_t min_len_exclusive, int64_t *read_start, int32_t *pos, int64_t capacity,
                     int64_t *nout, bool out_on_device) {
    KmerPlan P;
    KmerDev D;
    int rc;
    h->pend.on = false;                    // (the stage below overwrites what a pending partitioned index build keeps)
    if ((rc = kmer_plan("gab_kmer_sketch", in, k, min_len_exclusive, true, &P))) return rc;
    if ((rc = kmer_mini_stage(h, in, P, k, window, &D))) return rc;
    return kmer_bitmap_emit(h, "gab_kmer_sketch", in, D, k, read_start, pos, capacity, nout, out_on_device);
}

// filterFrequentKmers (kmer-cnt/vertex_index.cpp:190-191) with its float operations: (size_t)(rate * mean), saturated where the float
// has no size_t
uint64_t kmer_repetitive(uint64_t total, uint64_t unique, float rate) {
    const float mean = (float)total / (float)(unique + 1);
    const float cut = rate * mean;
    return cut >= 18446744073709551615.0f ? ~0ull : (uint64_t)cut;
}

// The filter's threshold from the totals of the whole input: thr is min(repetitive_frequency, 2^32 - 1), what the kernels compare the
// 32-bit capacities with.  -> the result so far; minimizers and distinct are this table's own.
gab_kmer_index_result kmer_index_threshold(int64_t kept, int64_t total_len, int64_t minimizers, int64_t distinct, uint64_t total, uint64_t unique, float rate,
                                           uint32_t *thr) {
    const uint64_t rep = kmer_repetitive(total, unique, rate);
    *thr = (uint32_t)std::min<uint64_t>(rep, 0xFFFFFFFFull);
    return gab_kmer_index_result{kept, total_len, minimizers, distinct, (int64_t)std::min<uint64_t>(rep, (uint64_t)INT64_MAX), 0, 0, 0, 0};
}

// The second half of an index build, after the synchronisation that gave the host the filter's two integers: orders the n keys of
// the table, lays out their lists (m entries before the filter), fills and sorts them.  The table holds the keys of h->part of
// h->nparts, n = R.distinct and m = R.minimizers are that partition's own, thr comes from the totals of the whole input
// (kmer_index_threshold).  Fills the last four fields of R; the handle then holds the index.
// counts (the solid index): the count table of the call, count_lines lines.  A key that stays but whose global count is above thr
// keeps an empty list and leaves the table (kmer_solid_weigh, kmer_solid_retire); selected_kmers and index_entries are then those of
// the lists that are not empty, filtered_* include the empty ones, and the caller takes them apart again with ct->sx_empty*.
int kmer_index_layout(gab_kmer *h, const KmerDev &D, const int32_t *d_len, int k, gab_kmer_index_result R, uint32_t thr, gab_kmer_index_result *res,
                      hipStream_t s, const KmerLine *counts = nullptr, uint64_t count_lines = 0) {
    const int64_t n = R.distinct, m = R.minimizers;
    KmerLine *table = h->table.as<KmerLine>();
    KmerCounters *d_ct = h->ct.as<KmerCounters>();
    const uint64_t nlines = h->nlines;
    int rc;
    GAB_HIP(hipEventRecord(h->ev_ix[3], s));
    if (n) {
        size_t sort_bytes = 0, scan_bytes = 0, seg_bytes = 0;
        GAB_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, 0u,
                                          (unsigned)(2 * k), s));
        GAB_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s));
        GAB_HIP(rocprim::segmented_radix_sort_keys(nullptr, seg_bytes, (int64_t *)nullptr, (int64_t *)nullptr, (unsigned)m, (unsigned)n, (uint32_t *)nullptr,
                                                   (uint32_t *)nullptr, 0u, 40u, s));
        const size_t nb = align256(((size_t)n + 1) * 8), mb = align256((size_t)m * 8);
        const size_t tmp_bytes = std::max(sort_bytes, std::max(scan_bytes, seg_bytes));
        if ((rc = h->aux.reserve(6 * nb + align256(((size_t)n + 1) * 4) + mb + tmp_bytes + 256))) return rc;
        if ((rc = h->idx.reserve(2 * nb + mb + 256))) return rc;
        char *ab = h->aux.as<char>(), *ib = h->idx.as<char>();
        uint64_t *k_in = reinterpret_cast<uint64_t *>(ab), *k_out = reinterpret_cast<uint64_t *>(ab + nb);
        uint64_t *s_in = reinterpret_cast<uint64_t *>(ab + 2 * nb), *s_out = reinterpret_cast<uint64_t *>(ab + 3 * nb);
        uint64_t *weight = reinterpret_cast<uint64_t *>(ab + 4 * nb), *scan = reinterpret_cast<uint64_t *>(ab + 5 * nb);
        uint32_t *seg = reinterpret_cast<uint32_t *>(ab + 6 * nb);
        int64_t *g_in = reinterpret_cast<int64_t *>(ab + 6 * nb + align256(((size_t)n + 1) * 4));
        void *tmp = ab + 6 * nb + align256(((size_t)n + 1) * 4) + mb;
        uint64_t *kmers = reinterpret_cast<uint64_t *>(ib);
        int64_t *start = reinterpret_cast<int64_t *>(ib + nb), *g_out = reinterpret_cast<int64_t *>(ib + 2 * nb);
        const dim3 per_key((unsigned)gab_ceil_div(n + 1, kBlock));
        hipLaunchKernelGGL(kmer_index_compact, dim3(sweep_grid(h)), dim3(kBlock), 0, s, table, nlines, k_in, s_in, (uint32_t)n, d_ct);
        GAB_HIP(rocprim::radix_sort_pairs(tmp, sort_bytes, k_in, k_out, s_in, s_out, (size_t)n, 0u, (unsigned)(2 * k), s));
        if (counts) hipLaunchKernelGGL(kmer_solid_weigh, per_key, dim3(kBlock), 0, s, table, k_out, s_out, n, thr, counts, count_lines, weight, d_ct);
        else hipLaunchKernelGGL(kmer_index_weigh, per_key, dim3(kBlock), 0, s, table, s_out, n, thr, weight);
        GAB_HIP(rocprim::exclusive_scan(tmp, scan_bytes, weight, scan, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s));
        hipLaunchKernelGGL(kmer_index_assign, per_key, dim3(kBlock), 0, s, table, k_out, s_out, weight, scan, n, kmers, start, seg, d_ct);
        if (counts) hipLaunchKernelGGL(kmer_solid_retire, per_key, dim3(kBlock), 0, s, table, s_out, weight, n, thr);
        kmer_mini_launch_walk<kWalkFill>(h, D, d_len, k, nullptr, thr, g_in, s);
        GAB_HIP(hipEventRecord(h->ev_ix[4], s));
        GAB_HIP(rocprim::segmented_radix_sort_keys(tmp, seg_bytes, g_in, g_out, (unsigned)m, (unsigned)n, seg, seg + 1, 0u, 40u, s));
        GAB_HIP(hipEventRecord(h->ev_ix[5], s));
        GAB_HIP(hipMemcpyAsync(h->h_ct, d_ct, sizeof(KmerCounters), hipMemcpyDeviceToHost, s));
        GAB_HIP(hipStreamSynchronize(s));
        GAB_HIP(hipGetLastError());
        R.selected_kmers = (int64_t)h->h_ct->ix_kmers; R.index_entries = (int64_t)h->h_ct->ix_entries;
        R.filtered_kmers = n - R.selected_kmers; R.filtered_entries = m - R.index_entries;
    } else {
        GAB_HIP(hipEventRecord(h->ev_ix[4], s));
        GAB_HIP(hipEventRecord(h->ev_ix[5], s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    (void)hipEventElapsedTime(&h->ix_ms[2], h->ev_ix[3], h->ev_ix[4]);
    (void)hipEventElapsedTime(&h->ix_ms[3], h->ev_ix[4], h->ev_ix[5]);
    h->ix = R; h->ix_thr = thr; h->indexed = true; h->solid = counts != nullptr;
    if (res) *res = R;
    return GAB_OK;
}

int kmer_index_impl(gab_kmer *h, const KmerInput &in, int k, int window, int32_t min_len_exclusive, float rate, gab_kmer_index_result *res) {
    const char *fn = "gab_kmer_index_minimizers";
    h->counted = false; h->indexed = false; h->pend.on = false;
    hipStream_t s = in.stream;
    KmerPlan P;
    KmerDev D;
    int rc;
    if ((rc = kmer_plan(fn, in, k, min_len_exclusive, true, &P))) return rc;
    // a minimizer per position at most, so the table of a count over the same reads is never more than half full
    const uint64_t nlines = table_lines(std::max<int64_t>(P.positions, 1), k);
    if ((rc = h->table.reserve((size_t)nlines * sizeof(KmerLine)))) return rc;
    KmerLine *table = h->table.as<KmerLine>();
    h->nlines = nlines; h->k = k; h->part = 0; h->nparts = 1; h->retried = false;

    GAB_HIP(hipEventRecord(h->ev_ix[0], s));
    if ((rc = kmer_mini_stage(h, in, P, k, window, &D))) return rc;
    GAB_HIP(hipEventRecord(h->ev_ix[1], s));
    GAB_HIP(hipMemsetAsync(table, 0, (size_t)nlines * sizeof(KmerLine), s));
    kmer_mini_launch_walk<kWalkCount>(h, D, in.d_len, k, nullptr, 0u, nullptr, s);
    hipLaunchKernelGGL(kmer_reduce<false>, dim3(sweep_grid(h)), dim3(kBlock), 0, s, table, nlines * kSlots, h->ct.as<KmerCounters>());
    GAB_HIP(hipEventRecord(h->ev_ix[2], s));
    if ((rc = kmer_mini_fetch(h, fn, D, s))) return rc;
    (void)hipEventElapsedTime(&h->ix_ms[0], h->ev_ix[0], h->ev_ix[1]);
    (void)hipEventElapsedTime(&h->ix_ms[1], h->ev_ix[1], h->ev_ix[2]);

    const uint64_t total = h->h_ct->ix_minimizers, unique = h->h_ct->distinct;
    uint32_t thr;
    const gab_kmer_index_result R = kmer_index_threshold(P.kept, P.total_len, (int64_t)total, (int64_t)unique, total, unique, rate, &thr);
    return kmer_index_layout(h, D, in.d_len, k, R, thr, res, s);
}

// Phase 1 of a partitioned index build: stage and sketch as kmer_index_impl, then the capacities of the keys of `part` alone, in a
// table sized for that share (the first table and its repeat: kmer_first_table).  Ends with the synchronisation that every
// index build has in its middle; what it leaves in the handle is described at gab_kmer::pend.
int kmer_index_begin_impl(gab_kmer *h, const char *fn, const KmerInput &in, int k, int window, int32_t min_len_exclusive, int part, int nparts,
                          gab_kmer_index_result *res) {
    h->counted = false; h->indexed = false; h->pend.on = false;
    hipStream_t s = in.stream;
    KmerPlan P;
    KmerDev D;
    int rc;
    if ((rc = kmer_plan(fn, in, k, min_len_exclusive, true, &P))) return rc;
    h->k = k; h->part = part; h->nparts = nparts;

    GAB_HIP(hipEventRecord(h->ev_ix[0], s));
    if ((rc = kmer_mini_stage(h, in, P, k, window, &D))) return rc;
    GAB_HIP(hipEventRecord(h->ev_ix[1], s));
    rc = kmer_first_table(h, fn, P.positions, k, nparts, s, [&](int, uint64_t limit) -> int {
        KmerLine *table = h->table.as<KmerLine>();
        GAB_HIP(hipMemsetAsync(table, 0, (size_t)h->nlines * sizeof(KmerLine), s));
        kmer_mini_launch_walk<kWalkCount>(h, D, in.d_len, k, nullptr, 0u, nullptr, s, limit);
        hipLaunchKernelGGL(kmer_reduce<true>, dim3(sweep_grid(h)), dim3(kBlock), 0, s, table, h->nlines * kSlots, h->ct.as<KmerCounters>());
        GAB_HIP(hipEventRecord(h->ev_ix[2], s));
        return kmer_mini_fetch(h, fn, D, s);
    });
    if (rc) return rc;
    (void)hipEventElapsedTime(&h->ix_ms[0], h->ev_ix[0], h->ev_ix[1]);
    (void)hipEventElapsedTime(&h->ix_ms[1], h->ev_ix[1], h->ev_ix[2]);       // (after a repeat: both attempts)
    h->ix_ms[2] = 0; h->ix_ms[3] = 0;
    gab_kmer::Pending &Q = h->pend;
    Q.dev = D; Q.d_len = in.d_len; Q.stream = s;
    Q.kept = P.kept; Q.total_len = P.total_len;
    Q.minimizers = (int64_t)h->h_ct->total_kmers;                  // (kmer_reduce<true>: the sum of the capacities in this table)
    Q.distinct = (int64_t)h->h_ct->distinct;
    Q.on = true;
    if (res) *res = gab_kmer_index_result{Q.kept, Q.total_len, Q.minimizers, Q.distinct, 0, 0, 0, 0, 0};
    return GAB_OK;
}


// ---- solid index, host side ------------------------------------------------------------------------------------------------------------
// Stages of gab_kmer_index_solid (all on the caller's stream):
//   kmer_pack, table clear, kmer_count<false>                                                              "count"
//   kmer_solid_freq, kmer_solid_select, the scan of the bitmap                                             "select"
//   second table clear, kmer_mini_walk<kWalkCount> into it, kmer_solid_reduce                              "capacity"
//   -- the synchronisation in the middle, as in the minimizer build --
//   kmer_index_layout with the count table at hand                                                         "fill", "sort"
// The two tables trade places on the host before the capacity walk: `table` is whatever the index's kernels work on.
struct KmerSolidArgs { int k; int32_t min_len; int min_freq; float select_rate; int tandem; };

int kmer_solid_check(const char *fn, gab_kmer *h, const void *off, const void *len, int64_t n_reads, int k, int min_freq, float select_rate) {
    GAB_CHECK(h && n_reads >= 0 && (n_reads == 0 || (off && len)), "%s: NULL or negative argument", fn);
    GAB_CHECK(k >= 1 && k <= GAB_KMER_MAX_K, "%s: k = %d, supported 1..%d", fn, k, GAB_KMER_MAX_K);
    GAB_CHECK(min_freq >= 0, "%s: min_freq = %d (>= 0)", fn, min_freq);
    GAB_CHECK(select_rate >= 0.0f && select_rate < 1.0f, "%s: select_rate = %g (0 <= select_rate < 1: the rank select_rate * n must be a position of the read)", fn,
              (double)select_rate);
    return GAB_OK;
}

// stage, count into `counts` (count_lines lines, reserved by the caller), look-up, selection and scan: the bitmap then holds the
// selected positions.  ev: start | counted | selected
int kmer_solid_front(gab_kmer *h, const KmerInput &in, const KmerPlan &P, const KmerSolidArgs &a, KmerLine *counts, uint64_t count_lines, KmerDev *D,
                     hipEvent_t *ev) {
    int rc;
    hipStream_t s = in.stream;
    KmerBitmapScan B;
    KmerCounters *d_ct = h->ct.as<KmerCounters>();
    GAB_HIP(hipEventRecord(ev[0], s));
    if ((rc = kmer_bitmap_stage(h, in, P, D, &B))) return rc;
    if ((rc = h->freq.reserve((size_t)D->n_runs * kRun * 4 + 256))) return rc;
    GAB_HIP(hipMemsetAsync(counts, 0, (size_t)count_lines * sizeof(KmerLine), s));
    if (D->n_tiles) {
        const dim3 grid((unsigned)gab_ceil_div(D->n_tiles, kBlock / 64));
        hipLaunchKernelGGL(kmer_count<false>, grid, dim3(kBlock), 0, s, D->packed, D->woff, in.d_len, D->tiles, D->n_tiles, a.k, counts, count_lines, d_ct, 0u, 1u,
                           (uint64_t)0);
        GAB_HIP(hipEventRecord(ev[1], s));
        const KmerSolidRule rule = {a.select_rate, (uint32_t)a.min_freq, a.tandem > 0 ? (uint32_t)a.tandem : 0u, a.min_len};
        hipLaunchKernelGGL(kmer_solid_freq, grid, dim3(kBlock), 0, s, D->packed, D->woff, in.d_len, D->tiles, D->n_tiles, a.k, counts, count_lines,
                           h->freq.as<uint32_t>());
        hipLaunchKernelGGL(kmer_solid_select, dim3((unsigned)in.n_reads), dim3(kBlock), 0, s, D->packed, D->woff, in.d_len, D->first_run, a.k, rule,
                           h->freq.as<uint32_t>(), D->masks, d_ct);
    } else GAB_HIP(hipEventRecord(ev[1], s));
    if ((rc = kmer_bitmap_scan(*D, B, s))) return rc;
    GAB_HIP(hipEventRecord(ev[2], s));
    return GAB_OK;
}

int kmer_solid_fetch(gab_kmer *h, const char *fn, const KmerDev &D, hipStream_t s) {
    int rc;
    if ((rc = kmer_mini_fetch(h, fn, D, s))) return rc;
    GAB_CHECK(!h->h_ct->overflow, "%s: internal error: the multiplicity test of a read did not fit after %u classes", fn, kSolidMaxClasses);
    return GAB_OK;
}

int kmer_solid_impl(gab_kmer *h, const KmerInput &in, const KmerSolidArgs &a, float rate, gab_kmer_solid_result *res) {
    const char *fn = "gab_kmer_index_solid";
    h->counted = false; h->indexed = false; h->pend.on = false;
    hipStream_t s = in.stream;
    KmerPlan P;
    KmerDev D;
    int rc;
    if ((rc = kmer_plan(fn, in, a.k, a.min_len, true, &P))) return rc;
    // both tables: at most one key per position, so never more than half full
    const uint64_t nlines = table_lines(std::max<int64_t>(P.positions, 1), a.k);
    if ((rc = h->table.reserve((size_t)nlines * sizeof(KmerLine)))) return rc;
    if ((rc = h->cap.reserve((size_t)nlines * sizeof(KmerLine)))) return rc;
    h->nlines = nlines; h->k = a.k; h->part = 0; h->nparts = 1; h->retried = false;
    if ((rc = kmer_solid_front(h, in, P, a, h->table.as<KmerLine>(), nlines, &D, h->ev_sx))) return rc;
    std::swap(h->table, h->cap);           // from here on `table` is the capacity table and `cap` holds the counts
    KmerLine *table = h->table.as<KmerLine>();
    const KmerLine *counts = h->cap.as<KmerLine>();
    GAB_HIP(hipMemsetAsync(table, 0, (size_t)nlines * sizeof(KmerLine), s));
    kmer_mini_launch_walk<kWalkCount>(h, D, in.d_len, a.k, nullptr, 0u, nullptr, s);
    hipLaunchKernelGGL(kmer_solid_reduce, dim3(sweep_grid(h)), dim3(kBlock), 0, s, table, nlines * kSlots, (uint32_t)a.min_freq, h->ct.as<KmerCounters>());
    GAB_HIP(hipEventRecord(h->ev_sx[3], s));
    if ((rc = kmer_solid_fetch(h, fn, D, s))) return rc;
    for (int i = 0; i < 3; i++) (void)hipEventElapsedTime(&h->sx_ms[i], h->ev_sx[i], h->ev_sx[i + 1]);
    h->ix_ms[0] = h->sx_ms[0] + h->sx_ms[1]; h->ix_ms[1] = h->sx_ms[2];      // (gab_kmer_index_last_phases: everything before the capacities | the capacities)
    h->sx_need = (int64_t)h->h_ct->sx_need; h->sx_fallback = (int64_t)h->h_ct->sx_fallback;

    const uint64_t selected = h->h_ct->ix_minimizers, candidates = h->h_ct->distinct, total = h->h_ct->sx_total, unique = h->h_ct->sx_unique;
    uint32_t thr;
    gab_kmer_index_result R = kmer_index_threshold(P.kept, P.total_len, (int64_t)selected, (int64_t)candidates, total, unique, rate, &thr);
    if ((rc = kmer_index_layout(h, D, in.d_len, a.k, R, thr, &R, s, counts, nlines))) return rc;
    const int64_t empty = (int64_t)h->h_ct->sx_empty, empty_cap = (int64_t)h->h_ct->sx_empty_cap;
    h->sx = gab_kmer_solid_result{P.kept, P.total_len, P.positions, (int64_t)selected, (int64_t)candidates, (int64_t)total, (int64_t)unique,
                                  R.repetitive_frequency, R.filtered_kmers - empty, R.filtered_entries - empty_cap, R.selected_kmers + empty,
                                  R.selected_kmers, R.index_entries};
    if (res) *res = h->sx;
    return GAB_OK;
}

int kmer_solid_positions_impl(gab_kmer *h, const KmerInput &in, const KmerSolidArgs &a, int64_t *read_start, int32_t *pos, int64_t capacity, int64_t *nout,
                              bool out_on_device) {
    const char *fn = "gab_kmer_solid_positions";
    KmerPlan P;
    KmerDev D;
    int rc;
    h->pend.on = false;                    // (the stage below overwrites what a pending partitioned index build keeps)
    if ((rc = kmer_plan(fn, in, a.k, a.min_len, true, &P))) return rc;
    const uint64_t nlines = table_lines(std::max<int64_t>(P.positions, 1), a.k);
    if ((rc = h->cap.reserve((size_t)nlines * sizeof(KmerLine)))) return rc;      // (the counts go where a count or an index in the handle is not)
    if ((rc = kmer_solid_front(h, in, P, a, h->cap.as<KmerLine>(), nlines, &D, h->ev_sx))) return rc;
    if ((rc = kmer_bitmap_emit(h, fn, in, D, a.k, read_start, pos, capacity, nout, out_on_device))) return rc;
    GAB_CHECK(!h->h_ct->overflow, "%s: internal error: the multiplicity test of a read did not fit after %u classes", fn, kSolidMaxClasses);
    return GAB_OK;
}

}  // namespace

extern "C" int gab_kmer_sketch(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int window,
                               int32_t min_len_exclusive, int64_t *read_start, int32_t *pos, int64_t capacity, int64_t *nout) {
    int rc = kmer_mini_check("gab_kmer_sketch", h, off, len, n_reads, k, window);
    if (rc) return rc;
    GAB_CHECK(nout && capacity >= 0, "gab_kmer_sketch: NULL or negative argument");
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_host(h, "gab_kmer_sketch", seq, off, len, n_reads, &in))) return rc;
    return kmer_sketch_impl(h, in, k, window, min_len_exclusive, read_start, pos, capacity, nout, false);
}

extern "C" int gab_kmer_sketch_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int window,
                                      int32_t min_len_exclusive, int64_t *read_start, int32_t *pos, int64_t capacity, int64_t *nout, void *stream) {
    int rc = kmer_mini_check("gab_kmer_sketch_device", h, off, len, n_reads, k, window);
    if (rc) return rc;
    GAB_CHECK(nout && capacity >= 0 && seq_bytes >= 0 && (seq || seq_bytes == 0), "gab_kmer_sketch_device: bad argument");
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_device(seq, seq_bytes, off, len, n_reads, stream, &in))) return rc;
    return kmer_sketch_impl(h, in, k, window, min_len_exclusive, read_start, pos, capacity, nout, true);
}

static int kmer_check_rate(float rate) {
    GAB_CHECK(rate >= 0.0f && rate <= 3.0e38f, "gab_kmer_index_minimizers: repeat_kmer_rate = %g (a finite number >= 0)", (double)rate);
    return GAB_OK;
}

extern "C" int gab_kmer_index_minimizers(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int window,
                                         int32_t min_len_exclusive, float repeat_kmer_rate, gab_kmer_index_result *res) {
    int rc = kmer_mini_check("gab_kmer_index_minimizers", h, off, len, n_reads, k, window);
    if (rc || (rc = kmer_check_rate(repeat_kmer_rate))) return rc;
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_host(h, "gab_kmer_index_minimizers", seq, off, len, n_reads, &in))) return rc;
    return kmer_index_impl(h, in, k, window, min_len_exclusive, repeat_kmer_rate, res);
}

extern "C" int gab_kmer_index_minimizers_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads, int k,
                                                int window, int32_t min_len_exclusive, float repeat_kmer_rate, gab_kmer_index_result *res, void *stream) {
    int rc = kmer_mini_check("gab_kmer_index_minimizers_device", h, off, len, n_reads, k, window);
    if (rc || (rc = kmer_check_rate(repeat_kmer_rate))) return rc;
    GAB_CHECK(seq_bytes >= 0 && (seq || seq_bytes == 0), "gab_kmer_index_minimizers_device: bad sequence slab");
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_device(seq, seq_bytes, off, len, n_reads, stream, &in))) return rc;
    return kmer_index_impl(h, in, k, window, min_len_exclusive, repeat_kmer_rate, res);
}

extern "C" int64_t gab_kmer_repetitive_frequency(int64_t minimizers, int64_t distinct, float repeat_kmer_rate) {
    GAB_CHECK(minimizers >= 0 && distinct >= 0, "gab_kmer_repetitive_frequency: minimizers = %lld, distinct = %lld (both >= 0)", (long long)minimizers,
              (long long)distinct);
    int rc = kmer_check_rate(repeat_kmer_rate);
    if (rc) return rc;
    return (int64_t)std::min<uint64_t>(kmer_repetitive((uint64_t)minimizers, (uint64_t)distinct, repeat_kmer_rate), (uint64_t)INT64_MAX);
}

static int kmer_check_index_part(const char *fn, int part, int nparts) {
    int rc = kmer_check_parts(fn, nparts);
    if (rc) return rc;
    GAB_CHECK(part >= 0 && part < nparts, "%s: part = %d, nparts = %d (0 <= part < nparts)", fn, part, nparts);
    return GAB_OK;
}

extern "C" int gab_kmer_index_part_begin(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int window,
                                         int32_t min_len_exclusive, int part, int nparts, gab_kmer_index_result *res) {
    const char *fn = "gab_kmer_index_part_begin";
    int rc = kmer_mini_check(fn, h, off, len, n_reads, k, window);
    if (rc || (rc = kmer_check_index_part(fn, part, nparts))) return rc;
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_host(h, fn, seq, off, len, n_reads, &in))) return rc;
    return kmer_index_begin_impl(h, fn, in, k, window, min_len_exclusive, part, nparts, res);
}

extern "C" int gab_kmer_index_part_begin_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads, int k,
                                                int window, int32_t min_len_exclusive, int part, int nparts, gab_kmer_index_result *res, void *stream) {
    const char *fn = "gab_kmer_index_part_begin_device";
    int rc = kmer_mini_check(fn, h, off, len, n_reads, k, window);
    if (rc || (rc = kmer_check_index_part(fn, part, nparts))) return rc;
    GAB_CHECK(seq_bytes >= 0 && (seq || seq_bytes == 0), "%s: bad sequence slab", fn);
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_device(seq, seq_bytes, off, len, n_reads, stream, &in))) return rc;
    return kmer_index_begin_impl(h, fn, in, k, window, min_len_exclusive, part, nparts, res);
}

// (an argument that is refused leaves the pending state as it is: the caller may call again with the right totals)
extern "C" int gab_kmer_index_part_finish(gab_kmer *h, int64_t minimizers, int64_t distinct, float repeat_kmer_rate, gab_kmer_index_result *res) {
    GAB_CHECK(h, "gab_kmer_index_part_finish: NULL handle");
    GAB_CHECK(h->pend.on, "gab_kmer_index_part_finish: no pending gab_kmer_index_part_begin on this handle (each begin is finished once; any other "
                          "count, sketch or index call in between drops it)");
    int rc = kmer_check_rate(repeat_kmer_rate);
    if (rc) return rc;
    const gab_kmer::Pending &Q = h->pend;
    GAB_CHECK(minimizers >= Q.minimizers && distinct >= Q.distinct,
              "gab_kmer_index_part_finish: totals of %lld minimizers and %lld distinct k-mers, but this partition alone has %lld and %lld (pass the sums over ALL "
              "partitions)", (long long)minimizers, (long long)distinct, (long long)Q.minimizers, (long long)Q.distinct);
    GAB_CHECK(minimizers >= distinct, "gab_kmer_index_part_finish: %lld minimizers < %lld distinct k-mers", (long long)minimizers, (long long)distinct);
    gab_device_guard g(h->device);
    uint32_t thr;
    const gab_kmer_index_result R = kmer_index_threshold(Q.kept, Q.total_len, Q.minimizers, Q.distinct, (uint64_t)minimizers, (uint64_t)distinct, repeat_kmer_rate, &thr);
    h->pend.on = false;                    // (the fill consumes the list starts: there is no second finish, and none after a failure)
    return kmer_index_layout(h, Q.dev, Q.d_len, h->k, R, thr, res, Q.stream);
}

#define KMER_NEED_INDEX(fn) \
    GAB_CHECK(h && h->indexed, fn ": no finished gab_kmer_index_minimizers (or gab_kmer_index_part_finish, or gab_kmer_index_solid) on this handle")

extern "C" int gab_kmer_index_dump(gab_kmer *h, uint64_t *kmers, int64_t *start, int64_t *gpos, int64_t cap_kmers, int64_t cap_entries, int64_t *nk,
                                   int64_t *ne) {
    KMER_NEED_INDEX("gab_kmer_index_dump");
    GAB_CHECK(nk && ne && cap_kmers >= 0 && cap_entries >= 0, "gab_kmer_index_dump: NULL or negative argument");
    const int64_t n = h->ix.selected_kmers, m = h->ix.index_entries;
    *nk = n; *ne = m;
    if (cap_kmers < n || cap_entries < m) {
        gab_set_error("gab_kmer_index_dump: %lld k-mers and %lld entries, room for %lld and %lld", (long long)n, (long long)m, (long long)cap_kmers,
                      (long long)cap_entries);
        return GAB_ERANGE;
    }
    GAB_CHECK(start, "gab_kmer_index_dump: NULL output");
    if (n == 0) { start[0] = 0; return GAB_OK; }
    GAB_CHECK(kmers && gpos, "gab_kmer_index_dump: NULL output");
    gab_device_guard g(h->device);
    hipStream_t s;
    int rc;
    if ((rc = h->hs.get(&s))) return rc;
    const size_t nb = align256(((size_t)h->ix.distinct + 1) * 8);      // (the layout of the build)
    const char *ib = h->idx.as<char>();
    GAB_HIP(hipMemcpyAsync(kmers, ib, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(start, ib + nb, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(gpos, ib + 2 * nb, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    return GAB_OK;
}

extern "C" int gab_kmer_index_lookup(gab_kmer *h, const uint64_t *kmers, int64_t n, int64_t *first, int32_t *count, uint8_t *repetitive) {
    KMER_NEED_INDEX("gab_kmer_index_lookup");
    GAB_CHECK(n >= 0 && (n == 0 || (kmers && first && count && repetitive)), "gab_kmer_index_lookup: NULL or negative argument");
    if (n == 0) return GAB_OK;
    gab_device_guard g(h->device);
    hipStream_t s;
    int rc;
    if ((rc = h->hs.get(&s))) return rc;
    const size_t nb = align256((size_t)n * 8), cb = align256((size_t)n * 4);
    if ((rc = h->aux.reserve(2 * nb + cb + align256((size_t)n)))) return rc;
    char *ab = h->aux.as<char>();
    uint64_t *d_k = reinterpret_cast<uint64_t *>(ab);
    int64_t *d_first = reinterpret_cast<int64_t *>(ab + nb);
    int32_t *d_count = reinterpret_cast<int32_t *>(ab + 2 * nb);
    uint8_t *d_rep = reinterpret_cast<uint8_t *>(ab + 2 * nb + cb);
    KmerCounters *d_ct = h->ct.as<KmerCounters>();
    h->h_ct->bad_query = ~0ull;
    GAB_HIP(hipMemcpyAsync(&d_ct->bad_query, &h->h_ct->bad_query, 8, hipMemcpyHostToDevice, s));
    GAB_HIP(hipMemcpyAsync(d_k, kmers, (size_t)n * 8, hipMemcpyHostToDevice, s));
    if (h->nparts == 1)
        hipLaunchKernelGGL(kmer_index_lookup<false>, dim3((unsigned)gab_ceil_div(n, kBlock)), dim3(kBlock), 0, s, h->table.as<KmerLine>(), h->nlines, h->k, h->ix_thr,
                           d_k, n, d_first, d_count, d_rep, d_ct, 0u, 1u);
    else
        hipLaunchKernelGGL(kmer_index_lookup<true>, dim3((unsigned)gab_ceil_div(n, kBlock)), dim3(kBlock), 0, s, h->table.as<KmerLine>(), h->nlines, h->k, h->ix_thr,
                           d_k, n, d_first, d_count, d_rep, d_ct, (uint32_t)h->part, (uint32_t)h->nparts);
    GAB_HIP(hipMemcpyAsync(&h->h_ct->bad_query, &d_ct->bad_query, 8, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(first, d_first, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(count, d_count, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipMemcpyAsync(repetitive, d_rep, (size_t)n, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    GAB_CHECK(h->h_ct->bad_query == ~0ull, "gab_kmer_index_lookup: k-mer %lld has bits above 2k = %d", (long long)h->h_ct->bad_query, 2 * h->k);
    return GAB_OK;
}

extern "C" int gab_kmer_index_last_phases(gab_kmer *h, float *sketch_ms, float *count_ms, float *fill_ms, float *sort_ms) {
    KMER_NEED_INDEX("gab_kmer_index_last_phases");
    if (sketch_ms) *sketch_ms = h->ix_ms[0];
    if (count_ms) *count_ms = h->ix_ms[1];
    if (fill_ms) *fill_ms = h->ix_ms[2];
    if (sort_ms) *sort_ms = h->ix_ms[3];
    return GAB_OK;
}


extern "C" int gab_kmer_index_solid(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int32_t min_len_exclusive,
                                    int min_freq, float select_rate, int tandem_freq, float repeat_kmer_rate, gab_kmer_solid_result *res) {
    const char *fn = "gab_kmer_index_solid";
    int rc = kmer_solid_check(fn, h, off, len, n_reads, k, min_freq, select_rate);
    if (rc || (rc = kmer_check_rate(repeat_kmer_rate))) return rc;
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_host(h, fn, seq, off, len, n_reads, &in))) return rc;
    return kmer_solid_impl(h, in, KmerSolidArgs{k, min_len_exclusive, min_freq, select_rate, tandem_freq}, repeat_kmer_rate, res);
}

extern "C" int gab_kmer_index_solid_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads, int k,
                                           int32_t min_len_exclusive, int min_freq, float select_rate, int tandem_freq, float repeat_kmer_rate,
                                           gab_kmer_solid_result *res, void *stream) {
    const char *fn = "gab_kmer_index_solid_device";
    int rc = kmer_solid_check(fn, h, off, len, n_reads, k, min_freq, select_rate);
    if (rc || (rc = kmer_check_rate(repeat_kmer_rate))) return rc;
    GAB_CHECK(seq_bytes >= 0 && (seq || seq_bytes == 0), "%s: bad sequence slab", fn);
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_device(seq, seq_bytes, off, len, n_reads, stream, &in))) return rc;
    return kmer_solid_impl(h, in, KmerSolidArgs{k, min_len_exclusive, min_freq, select_rate, tandem_freq}, repeat_kmer_rate, res);
}

extern "C" int gab_kmer_solid_positions(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int32_t min_len_exclusive,
                                        int min_freq, float select_rate, int tandem_freq, int64_t *read_start, int32_t *pos, int64_t capacity, int64_t *nout) {
    const char *fn = "gab_kmer_solid_positions";
    int rc = kmer_solid_check(fn, h, off, len, n_reads, k, min_freq, select_rate);
    if (rc) return rc;
    GAB_CHECK(nout && capacity >= 0, "%s: NULL or negative argument", fn);
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_host(h, fn, seq, off, len, n_reads, &in))) return rc;
    return kmer_solid_positions_impl(h, in, KmerSolidArgs{k, min_len_exclusive, min_freq, select_rate, tandem_freq}, read_start, pos, capacity, nout, false);
}

extern "C" int gab_kmer_solid_positions_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads, int k,
                                               int32_t min_len_exclusive, int min_freq, float select_rate, int tandem_freq, int64_t *read_start, int32_t *pos,
                                               int64_t capacity, int64_t *nout, void *stream) {
    const char *fn = "gab_kmer_solid_positions_device";
    int rc = kmer_solid_check(fn, h, off, len, n_reads, k, min_freq, select_rate);
    if (rc) return rc;
    GAB_CHECK(nout && capacity >= 0 && seq_bytes >= 0 && (seq || seq_bytes == 0), "%s: bad argument", fn);
    gab_device_guard g(h->device);
    KmerInput in;
    if ((rc = kmer_input_device(seq, seq_bytes, off, len, n_reads, stream, &in))) return rc;
    return kmer_solid_positions_impl(h, in, KmerSolidArgs{k, min_len_exclusive, min_freq, select_rate, tandem_freq}, read_start, pos, capacity, nout, true);
}

#define KMER_NEED_SOLID(fn) GAB_CHECK(h && h->indexed && h->solid, fn ": no finished gab_kmer_index_solid on this handle")

extern "C" int gab_kmer_solid_last_phases(gab_kmer *h, float *count_ms, float *select_ms, float *capacity_ms, float *fill_ms, float *sort_ms) {
    KMER_NEED_SOLID("gab_kmer_solid_last_phases");
    if (count_ms) *count_ms = h->sx_ms[0];
    if (select_ms) *select_ms = h->sx_ms[1];
    if (capacity_ms) *capacity_ms = h->sx_ms[2];
    if (fill_ms) *fill_ms = h->ix_ms[2];
    if (sort_ms) *sort_ms = h->ix_ms[3];
    return GAB_OK;
}

extern "C" int gab_kmer_solid_last_stats(gab_kmer *h, int64_t *tested_positions, int64_t *fallback_reads) {
    KMER_NEED_SOLID("gab_kmer_solid_last_stats");
    if (tested_positions) *tested_positions = h->sx_need;
    if (fallback_reads) *fallback_reads = h->sx_fallback;
    return GAB_OK;
}

extern "C" int gab_kmer_index_last_part(gab_kmer *h, int *part, int *nparts, int64_t *table_slots, int *retried) {
    KMER_NEED_INDEX("gab_kmer_index_last_part");
    return kmer_last_part(h, part, nparts, table_slots, retried);
}
