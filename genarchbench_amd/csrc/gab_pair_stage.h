// Staging of a batch of pattern / text pairs given by HOST pointers: what gab_bpm_run, gab_bitpal_run, gab_wfa_run and
// gab_wfa_run_packed do before they call their *_run_device entry point.
//   gab_pair_scan       validates the offsets and finds the window [min, max) of each slab that the pairs refer to
//   gab_pair_layout_of  places the windows and the per-pair arrays in the handle's staging buffer (*_reserve sizes it by the same)
//   gab_pair_upload     copies them up under the GPU's H2D gate and returns the arguments of *_run_device
// (gab_bsw_run keeps its own scan: it samples the window and retries, bsw.hip.)
#pragma once
#include <algorithm>
#include "gab_internal.h"

struct gab_host_pairs {      // the arguments of a host-pointer entry point
    const char *pat; const int64_t *pat_off; const int32_t *pat_len; const char *txt; const int64_t *txt_off; const int32_t *txt_len; int64_t n;
};

static inline size_t gab_pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// ---- scan --------------------------------------------------------------------------------------------------------------------
// Only [pa, pb) of `pat` and [ta, tb) of `txt` are staged, so a driver hands a chunk of a big input to each call without
// re-basing its offsets (`off + first_pair`).  pa / ta are rounded down to 256 to keep the device alignment of the slab origin;
// a window is padded by 3 bytes (the kernels read dwords) to a multiple of 256.
struct gab_pair_window {
    int64_t pa, pb, ta, tb;
    bool shared;                     // one slab for both and the windows overlap: [pa, pb) == [ta, tb), staged once
    size_t ppad, tpad;               // bytes of the staged windows (tpad = 0 when shared)
};

// per_pair(i) -> bool: the caller's own work on pair i in the same pass (false = reject the pair like a negative offset)
template <typename PerPair>
static inline int gab_pair_scan(const char *who, const gab_host_pairs &in, gab_pair_window *out, PerPair per_pair) {
    const int64_t *pat_off = in.pat_off, *txt_off = in.txt_off; const int32_t *pat_len = in.pat_len, *txt_len = in.txt_len;
    int64_t pb = 0, tb = 0, pa = INT64_MAX, ta = INT64_MAX;
    for (int64_t i = 0; i < in.n; i++) {
        GAB_CHECK(pat_off[i] >= 0 && txt_off[i] >= 0 && pat_len[i] >= 0 && txt_len[i] >= 0 && per_pair(i),
                  "%s: negative offset/length at pair %lld", who, (long long)i);
        pb = std::max(pb, pat_off[i] + pat_len[i]); tb = std::max(tb, txt_off[i] + txt_len[i]);
        pa = std::min(pa, pat_off[i]); ta = std::min(ta, txt_off[i]);
    }
    pa &= ~(int64_t)255; ta &= ~(int64_t)255;
    // one slab for both with overlapping windows (the drivers' pair files: '>' and '<' lines interleaved): staged once, not twice
    const bool shared = in.pat == in.txt && std::max(pb, tb) - std::min(pa, ta) <= (pb - pa) + (tb - ta);
    if (shared) { pa = ta = std::min(pa, ta); pb = tb = std::max(pb, tb); }
    *out = {pa, pb, ta, tb, shared, gab_pad256((size_t)(pb - pa) + 3), shared ? 0 : gab_pad256((size_t)(tb - ta) + 3)};
    return GAB_OK;
}
static inline int gab_pair_scan(const char *who, const gab_host_pairs &in, gab_pair_window *out) {
    return gab_pair_scan(who, in, out, [](int64_t) { return true; });
}

// ---- layout ------------------------------------------------------------------------------------------------------------------
// Bump allocator over a staging buffer (whose base is 256-byte aligned): regions first, then 8-byte arrays, then 4-byte arrays.
struct gab_stage_bump {
    size_t o = 0;
    size_t region(size_t bytes) { o = gab_pad256(o); const size_t at = o; o += bytes; return at; }
    size_t a8(size_t n) { o = (o + 7) & ~(size_t)7; const size_t at = o; o += 8 * n; return at; }
    size_t a4(size_t n) { o = (o + 3) & ~(size_t)3; const size_t at = o; o += 4 * n; return at; }
    size_t cursor() { return region(256); }      // a 64-bit device atomic: a 256-byte line of its own (an unaligned one faults, GAB_CHECK_ATOMIC64)
};

enum gab_pair_stage_kind {
    GAB_STAGE_SCORES,        // gab_bpm_run, gab_bitpal_run: the pairs in, a score per pair out
    GAB_STAGE_OPS,           // gab_wfa_run: + the operations' room, its offsets and lengths
    GAB_STAGE_TEXT           // gab_wfa_run_packed: + the printed text, its offsets and lengths, and wfa_rle_pack's cursor
};
struct gab_pair_layout {     // offsets into the staging buffer; the members a kind does not have stay 0
    size_t p, t, ops, text;              // regions: the two windows, the operations, the printed text
    size_t po, to, oo, co;               // int64 per pair: offsets of pattern, text, operations, printed text
    size_t pl, tl, ol, cl, sc;           // int32 per pair: lengths of the same, the score
    size_t cur;                          // the 64-bit cursor
    size_t bytes;                        // of the whole layout
};
static inline gab_pair_layout gab_pair_layout_of(gab_pair_stage_kind kind, size_t ppad, size_t tpad, size_t n, size_t opad = 0, size_t cpad = 0) {
    const bool ops = kind >= GAB_STAGE_OPS, text = kind == GAB_STAGE_TEXT;
    gab_stage_bump a; gab_pair_layout L = {};
    L.p = a.region(ppad); L.t = a.region(tpad); if (ops) L.ops = a.region(opad); if (text) L.text = a.region(cpad);
    L.po = a.a8(n); L.to = a.a8(n); if (ops) L.oo = a.a8(n); if (text) L.co = a.a8(n);
    L.pl = a.a4(n); L.tl = a.a4(n); if (ops) L.ol = a.a4(n); if (text) L.cl = a.a4(n); L.sc = a.a4(n);
    if (text) L.cur = a.cursor();
    L.bytes = a.o;
    return L;
}
// What *_reserve sizes the staging buffer by: the layout of a call of max_pairs pairs whose sequences span max_seq_bytes of each slab
// wherever the windows start (a start rounds down by up to 255, hence + 256), 2 KB of headroom, 4 MB at least.
static inline size_t gab_pair_reserve_bytes(gab_pair_stage_kind kind, int64_t max_pairs, int64_t max_seq_bytes, size_t opad = 0, size_t cpad = 0) {
    const size_t win = gab_pad256((size_t)max_seq_bytes + 3 + 256);
    return std::max<size_t>(gab_pair_layout_of(kind, win, win, (size_t)max_pairs, opad, cpad).bytes + 2048, (size_t)4 << 20);
}

// ---- upload ------------------------------------------------------------------------------------------------------------------
struct gab_staged_pairs {    // the staging buffer, the handle's stream and what gab_*_run_device takes for the staged pairs
    char *b; hipStream_t s;
    const char *pat; int64_t pat_bytes; const int64_t *pat_off; const int32_t *pat_len; const char *txt; int64_t txt_bytes; const int64_t *txt_off; const int32_t *txt_len;
};

// Reserves the layout in `io` and copies the windows, offsets and lengths up on the handle's stream: one batch of copies and one
// synchronisation inside the GPU's H2D gate (gab_core.hip: the workers of a GPU must not copy in lockstep).  `ops_off` (may be NULL)
// goes to L.oo in the same batch: with the other offsets (gab_wfa_run) or, `ops_off_last`, after the lengths (gab_wfa_run_packed).
// times (may be NULL): [0] = buffers and stream ready, [1] = gate obtained (gab_now_ms).  pat / txt of the result are VIRTUAL slab
// origins -- the device address byte 0 of the caller's slab would have, below the staging buffer by pa / ta and never dereferenced
// there -- so the pairs' own offsets apply to them unchanged.
static inline int gab_pair_upload(gab_devbuf &io, gab_host_stream &hs, int device, const gab_host_pairs &in, const gab_pair_window &w,
                                  const gab_pair_layout &L, gab_staged_pairs *out, const int64_t *ops_off = nullptr, bool ops_off_last = false,
                                  double *times = nullptr) {
    int rc = io.reserve(L.bytes);
    if (rc) return rc;
    char *b = io.as<char>();
    hipStream_t s = nullptr;
    if ((rc = hs.get(&s)) != GAB_OK) return rc;
    if (times) times[0] = gab_now_ms();
    const size_t nn = (size_t)in.n;
    {
        std::lock_guard<std::mutex> gate(gab_h2d_mutex(device));
        if (times) times[1] = gab_now_ms();
        GAB_HIP(hipMemcpyAsync(b + L.p, in.pat + w.pa, (size_t)(w.pb - w.pa), hipMemcpyHostToDevice, s));
        if (!w.shared) GAB_HIP(hipMemcpyAsync(b + L.t, in.txt + w.ta, (size_t)(w.tb - w.ta), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.po, in.pat_off, 8 * nn, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.to, in.txt_off, 8 * nn, hipMemcpyHostToDevice, s));
        if (ops_off && !ops_off_last) GAB_HIP(hipMemcpyAsync(b + L.oo, ops_off, 8 * nn, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.pl, in.pat_len, 4 * nn, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + L.tl, in.txt_len, 4 * nn, hipMemcpyHostToDevice, s));
        if (ops_off && ops_off_last) GAB_HIP(hipMemcpyAsync(b + L.oo, ops_off, 8 * nn, hipMemcpyHostToDevice, s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    const char *t = w.shared ? b + L.p : b + L.t;
    *out = {b, s, b + L.p - w.pa, w.pa + (int64_t)w.ppad, (const int64_t *)(b + L.po), (const int32_t *)(b + L.pl),
            t - w.ta, w.ta + (int64_t)(w.shared ? w.ppad : w.tpad), (const int64_t *)(b + L.to), (const int32_t *)(b + L.tl)};
    return GAB_OK;
}
