// wfa_plan.h -- what the host decides about a wfa call, as data: the score table of a penalty set and the launches of the
// cascade.  Plain C++ with no HIP types: wfa.hip issues what this says, wfa_plan_dump.cc prints it, and tests/test_wfa_plan.py
// holds it against the model of tests/util.py (wfa_rows, wfa_plan) without a GPU.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

constexpr int kSeqPad = 32;                // physical 'X'/'Y' padding behind each LDS sequence (>= 16 + 3 for the 16-byte extension reads)
constexpr int kLdsMaxLen = 2040;           // longest sequence the LDS kernels accept
constexpr int kOffBMax = 245;              // one-byte offsets (OffB): the largest value
constexpr int kLdsLimit = 160 * 1024 - 512;   // dynamic LDS a launch may ask for
constexpr int kStaticPairBytes = 1568;     // LDS per pair of the first static launch: strings + pool (see wfa_plan)
constexpr size_t kResumeHdrBytes = 16;     // sizeof(WfResume)

// ---- the score table ---------------------------------------------------------------------------------------------------
// Complete mode, first tier: the directory as a table of the penalties.  Without the adaptive reduction nothing in a pair's
// directory depends on the data: whether M / I / D of a score exist, their [lo, hi] (min / max of the sources' -1 / +1) and
// where they land in the pool (allocation in score order) follow from the penalties alone.  One WfRow per score that has a
// wavefront, with the resolved facts of its three source scores; the kernel then needs no directory in LDS (the room goes to
// the offset pool), no look-ups and no decoding: all groups of a wave walk the rows in lockstep, so the row index is
// wave-uniform and the row arrives by scalar loads.  A missing source is an empty range (lo = 1, hi = -1): every read of it
// is out of range = null.
struct WfRow {
    int score, lo, hi, bM, bI, bD, used_end, has_gap;     // bI / bD valid iff has_gap (I and D exist at the same scores)
    int ms_m, ms_lo, ms_hi;                               // M[score - x]
    int mg_m, mg_lo, mg_hi;                               // M[score - o - e]
    int ie_i, ie_d, ie_lo, ie_hi;                         // I / D[score - e]
    int r_ms, r_mg, r_ie;                                 // rows of the three source scores (0 when there is none)
    int pad[3];
};
static_assert(sizeof(WfRow) == 96, "WfRow is read as dwords");

constexpr int kSteps = 1024;        // >= the largest LDS directory
// step: per score below kSteps the distance to the next score that has a wavefront (at most 255); rows: the scores that have
// one, in order, while the limits below hold
struct WfaTable { std::vector<uint8_t> step; std::vector<WfRow> rows; };
// One DP over the scores: M[s] exists iff M[s-x], M[s-o-e], I[s-e] or D[s-e] does; I[s] / D[s] iff M[s-o-e] or I[s-e] / D[s-e]
// does (affine_wavefront_align.c:283-321) -- no data involved.  The rows add ranges and pool positions: what wfa_pair would
// write into its directory, pair after pair (affine_wavefront_align.c:85-106 compute_limits, :56-84 allocate_wavefronts); they
// stop at 240 rows, 60 000 offsets or 120 diagonals to either side, the step table goes on to kSteps.
inline WfaTable wfa_table(int x, int o, int e) {
    constexpr int kMaxRows = 240;
    struct Ent { bool m = false, g = false; int lo = 1, hi = -1, bm = 0, bi = 0, bd = 0, row = 0; };
    const int oe = o + e;
    std::vector<Ent> ent(kSteps + 1);
    WfaTable t;
    ent[0].m = true; ent[0].lo = ent[0].hi = 0;
    WfRow r0; memset(&r0, 0, sizeof r0);
    r0.used_end = 1; r0.ms_lo = r0.mg_lo = r0.ie_lo = 1; r0.ms_hi = r0.mg_hi = r0.ie_hi = -1;
    t.rows.push_back(r0);
    int used = 1;
    bool open = true;               // rows are still being listed
    const Ent none;
    for (int sc = 1; sc <= kSteps; sc++) {
        // (a source that is missing -- for I / D[s-e]: an entry without I and D -- reads as `none`: the empty range, position and row 0)
        const Ent &ms = sc >= x ? ent[sc - x] : none, &mg = sc >= oe ? ent[sc - oe] : none, &ie = sc >= e && ent[sc - e].g ? ent[sc - e] : none;
        if (!ms.m && !mg.m && !ie.m) continue;
        Ent &c = ent[sc];
        c.m = true; c.g = mg.m || ie.m;
        if (!open || (int)t.rows.size() >= kMaxRows) { open = false; continue; }
        c.lo = std::min(std::min(ms.lo, mg.lo), ie.lo) - 1; c.hi = std::max(std::max(ms.hi, mg.hi), ie.hi) + 1;
        const int width = c.hi - c.lo + 1;
        c.bm = used; c.bi = used + width; c.bd = used + 2 * width;
        used += width * (c.g ? 3 : 1);
        if (used > 60000 || c.lo < -120 || c.hi > 120) { open = false; continue; }
        c.row = (int)t.rows.size();
        WfRow r; memset(&r, 0, sizeof r);
        r.score = sc; r.lo = c.lo; r.hi = c.hi; r.bM = c.bm; r.bI = c.bi; r.bD = c.bd; r.used_end = used; r.has_gap = c.g;
        r.ms_m = ms.bm; r.ms_lo = ms.lo; r.ms_hi = ms.hi; r.r_ms = ms.row; r.mg_m = mg.bm; r.mg_lo = mg.lo; r.mg_hi = mg.hi; r.r_mg = mg.row;
        r.ie_i = ie.bi; r.ie_d = ie.bd; r.ie_lo = ie.lo; r.ie_hi = ie.hi; r.r_ie = ie.row;
        t.rows.push_back(r);
    }
    t.step.assign(kSteps, 1);
    int next = kSteps + 255;
    for (int sc = kSteps - 1; sc >= 0; sc--) {
        if (ent[sc + 1].m) next = sc + 1;
        t.step[sc] = (uint8_t)std::min(next - sc, 255);
    }
    return t;
}
// ---- the launches ------------------------------------------------------------------------------------------------------
enum WfaKind { kWfaLdsStatic, kWfaLds, kWfaGlobal };
struct WfaLaunch {
    WfaKind kind;
    int G, off_bytes;       // lanes per pair (64 / G pairs per wave); 1 = OffB, 2 = int16_t, 4 = int32_t
    bool adaptive, chained; // chained = behind another tier: reads that tier's overflow count on the device
    long long pool, dir;    // in offsets; directory size in scores, or static_rows
    size_t group_bytes;     // LDS per group (wfa_global: none)
    // grid rule of a chained launch: waves for `share` of the batch, at least `floor_` of them (never more than for the
    // whole batch); one not chained gets a wave per 64 / G pairs
    double share; uint32_t floor_;
};
// as the kernel is spelled in the trace
inline void wfa_launch_name(const WfaLaunch &l, char *out, size_t n) {
    const char *a = l.adaptive ? "true" : "false";
    if (l.kind == kWfaLdsStatic) snprintf(out, n, "wfa_lds_static<%d,%s>", l.G, l.chained ? "true" : "false");
    else if (l.kind == kWfaLds) snprintf(out, n, "wfa_lds<%d,%s,%s>", l.G, a, l.off_bytes == 1 ? "OffB" : "int16_t");
    else snprintf(out, n, "wfa_global<%s>", a);
}
// dynamic LDS of a launch: the groups of a wave and, wfa_lds, the score-step table in front of them
constexpr size_t wfa_lds_bytes(WfaKind kind, int G, long long dir, size_t group_bytes) {
    return kind == kWfaGlobal ? 0 : group_bytes * (size_t)(64 / G) + (kind == kWfaLds ? ((size_t)dir + 15) & ~(size_t)15 : 0);
}
constexpr int wfa_seq_room(int max_len) { return ((max_len + kSeqPad + 8) + 15) & ~15; }
// wfa_lds: [dir: 4 bytes (OffB, complete: one dword), 12 (three) or 16 (adaptive: four) per score][P][T][pool]
constexpr size_t wfa_lds_group_bytes(bool adaptive, int off_bytes, long long dir, int seqs, long long pool) {
    return (((size_t)dir * (adaptive ? 16 : off_bytes == 1 ? 4 : 12) + (size_t)seqs + (size_t)(pool * off_bytes)) + 15) & ~(size_t)15;
}
// the largest launch there is -- the 96 KB pool behind two strings of kLdsMaxLen, adaptive -- fits: no launch is ever skipped
static_assert(wfa_lds_bytes(kWfaLds, 64, 640, wfa_lds_group_bytes(true, 2, 640, 2 * wfa_seq_room(kLdsMaxLen), 49152)) <= kLdsLimit,
              "the largest wfa_lds launch must fit the LDS");
inline uint32_t wfa_launch_grid(const WfaLaunch &l, uint32_t n_lds) {
    const uint32_t per_wave = 64 / l.G, all = (n_lds + per_wave - 1) / per_wave;
    if (!l.chained) return all;
    const uint32_t est = (uint32_t)((double)n_lds * l.share) / per_wave + 1;
    return std::max<uint32_t>(std::min<uint32_t>(est, all), std::min<uint32_t>(l.floor_, all));
}
// wfa_global, round r: 2^20 offsets and 4 096 scores per workgroup, then 8 x the pool and 4 x the directory (at most 2^22 scores)
inline WfaLaunch wfa_global_launch(bool adaptive, int round, bool chained) {
    WfaLaunch l = {kWfaGlobal, 64, 4, adaptive, chained, 1 << 20, 4096, 0, 0.0, 0};
    for (int r = 0; r < round; r++) { l.pool *= 8; l.dir = std::min<long long>(l.dir * 4, 1 << 22); }
    return l;
}
// int32 words of history per workgroup of a wfa_global round: the directory (five ints per score, seven if adaptive) + the pool
inline long long wfa_global_ints(const WfaLaunch &l) { return l.dir * (l.adaptive ? 7 : 5) + l.pool; }

// Resume slots of the two static launches (the pairs the first ran out of room for are continued by the second): a multiple of
// the pairs per wave, so that the boundary between resumed and restarted pairs falls between waves; the kernel copes with a
// mixed wave anyway.  In the scratch buffer: a header per pair of the batch, then a pool per slot.
inline uint32_t wfa_default_slots(uint64_t n_lds) { return (uint32_t)std::min<uint64_t>(n_lds, std::max<uint64_t>(65536, n_lds / 8)) & ~7u; }
inline size_t wfa_resume_hdr_bytes(size_t n_lds) { return (kResumeHdrBytes * n_lds + 255) & ~(size_t)255; }
inline size_t wfa_resume_bytes(size_t n_lds, size_t slots, size_t pool_bytes) { return wfa_resume_hdr_bytes(n_lds) + slots * pool_bytes; }
struct WfaKnobs { bool no_static = false; int pool2 = -1, slots = -1; };      // GAB_WFA_NO_STATIC / _POOL2 / _SLOTS; -1 = unset

struct WfaPlan {
    std::vector<WfaLaunch> launches;        // up to and including the first wfa_global; none when n_lds = 0
    int seqp, seqt, static_rows, static_pool;      // seqp / seqt: LDS room of the longest pattern / text
    bool use_static, byte_ok, resume;       // resume: two static launches, the first hands its unfinished pairs to the second
    uint32_t slots;
};

// The launches of a call for the n_lds pairs with both strings <= kLdsMaxLen, from the longest such pattern and text.
// nrows: rows of the penalties' table (complete mode).  LDS passes: (1) four pairs per wave with one-byte offsets -- complete
// mode: wfa_lds_static with the first pool (1 184 offsets behind two 151-bp strings) and then 2 560; adaptive mode:
// wfa_lds<16, OffB> with its directory in LDS; int16 offsets in a 2 KB pool when the strings are too long for bytes -- (2) one
// pair per wave with 12 KB of int16 offsets, (3) one pair per wave with 96 KB; whatever overflows goes to global memory.
inline WfaPlan wfa_plan(bool adaptive, int nrows, int max_plen, int max_tlen, uint32_t n_lds, const WfaKnobs &knobs) {
    WfaPlan p;
    const int seqs = (p.seqp = wfa_seq_room(max_plen)) + (p.seqt = wfa_seq_room(max_tlen));
    // First tier with one-byte offsets (OffB) when no offset can leave the byte's range: text length + one per score step.
    // Its LDS is budgeted per pair: 2496 B = 10 032 B per wave of four pairs = 16 waves per CU, the measured optimum (the
    // next allocation step down, 14 waves, costs 9 %; 18-20 waves with a smaller history re-queue too many pairs).  In
    // complete mode the history a pair needs is a function of its score alone (lo / hi do not depend on the data), so the
    // directory is sized to the scores the pool can hold: 56 scores, ~1.9 K offsets.
    int dir0 = adaptive ? 48 : 56;
    const int room = 2496 - dir0 * (adaptive ? 16 : 4) - seqs;
    bool byte_ok = room >= 1024;
    const int byte_pool = std::min(room & ~15, 2032);
    if (byte_ok && max_tlen + dir0 + 2 > kOffBMax) byte_ok = false;
    if (!byte_ok) dir0 = 48;
    // complete mode: the first tier takes its directory from the penalties' table (wfa_pair_static) -- no directory in LDS
    p.static_rows = adaptive ? 0 : std::min(nrows, kOffBMax - 2 - max_tlen);
    // LDS per pair of the first launch: 1568 B = 6272 B per wave of four = 24 waves per CU, six per SIMD (the kernel is
    // compiled for seven: 72 VGPRs and 12 bytes of scratch per lane; six would do), i.e. ~1.2 K offsets behind two 151-bp
    // strings = scores below 44 = 96 % of the pairs.  Measured: 1 520 offsets at 20 waves 382 M/s, 1 344 at 23 waves 391,
    // 1 088-1 184 at 24 waves 405; the history a pair needs steps with its score, so 1 216-1 312 offsets buy nothing over
    // 1 184 and cost a wave.
    p.static_pool = std::min(kStaticPairBytes - seqs, 4080) & ~15;
    p.use_static = !adaptive && byte_pool != 0 && !knobs.no_static && p.static_rows >= 16 && p.static_pool >= 1024;
    p.byte_ok = byte_ok; p.resume = false; p.slots = 0;
    if (!n_lds) return p;
    const double shares[4] = {1.0, 0.10, 0.02, 0.005};       // expected share of the batch that reaches tier k (151-bp reads at 2 %: 4 %, 0.07 %, ~0)
    auto add = [&](WfaKind kind, int G, int off_bytes, long long pool, long long dir, uint32_t floor_) {
        const size_t tier = p.launches.size();
        const size_t group_bytes = kind == kWfaLdsStatic ? (size_t)(seqs + pool) : wfa_lds_group_bytes(adaptive, off_bytes, dir, seqs, pool);
        p.launches.push_back({kind, G, off_bytes, adaptive, tier > 0, pool, dir, group_bytes, shares[std::min<size_t>(tier, 3)], floor_});
    };
    if (p.use_static) {
        // two launches: the small pool takes 96 % of the 151-bp pairs at 24 waves per CU, a 2.5 KB pool the scores up to ~64 of
        // the rest (measured: 2048-2560 B best, 4080 B 4 % slower).  The first leaves the wavefronts of the pairs it ran out of
        // room for in slots of the scratch buffer and the second continues them (the pool layout is the table's in both): it
        // does not repeat the ~40 score steps they had come
        const int pool2 = knobs.pool2 >= 0 ? knobs.pool2 : 2560;
        add(kWfaLdsStatic, 16, 1, p.static_pool, p.static_rows, 256);
        if (pool2 > p.static_pool) {
            add(kWfaLdsStatic, 16, 1, pool2, p.static_rows, 256);
            p.resume = true;
            p.slots = wfa_default_slots(n_lds);
            if (knobs.slots >= 0) p.slots = (uint32_t)std::min<uint64_t>(n_lds, (uint64_t)knobs.slots);      // tests force the boundary into a wave
        }
    } else if (byte_ok) add(kWfaLds, 16, 1, std::min(byte_pool, 2046), dir0, 256);
    else add(kWfaLds, 16, 2, 1024, dir0, 256);
    add(kWfaLds, 64, 2, 6144, 128, 256);
    add(kWfaLds, 64, 2, 49152, 640, 64);
    // what the last LDS tier leaves (almost never anything) goes to the global-history kernel WITHOUT asking the device how
    // many pairs that is: one launch of a few workgroups that reads the count itself
    p.launches.push_back(wfa_global_launch(adaptive, 0, true));
    return p;
}
