// The abea handle, shared by abea.hip (align), abea_events.hip (event detection, scaling estimate) and abea_calib.hip (base-to-event
// map, recalibration, read checks), abea_realign.hip (realign_read) and abea_meth.hip (calculate_methylation_for_read).
#pragma once
#include <math.h>
#include "gab_internal.h"

// What realign_read and calculate_methylation_for_read both do to a read before their HMM.
// toupper, isValid and getPossibleSymbols(c)[0] (eventalign.c:991-1109, meth.c:189-306) in one: the base's rank, or -1
__host__ __device__ __forceinline__ int gab_abea_base_code(char c) {
    if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    switch (c) {
        case 'A': case 'M': case 'R': case 'W': case 'V': case 'H': case 'D': case 'N': return 0;
        case 'C': case 'S': case 'Y': case 'B': return 1;
        case 'G': case 'K': return 2;
        case 'T': return 3;
        default: return -1;
    }
}
// calculate_transitions (eventalign.c:171-240, hmm.c:231-298) and pre_flank[0] (eventalign.c:124), once per read.  The reference's
// compiler folds the logarithms of the constants (correctly rounded); only the two that depend on events_per_base are calls of logf.
// t: mm_self mm_next bm_self bm_next km soft | mb bb | mk bk kk
inline void gab_abea_transitions(double events_per_base, float *t) {
    const float p_stay = 1 - (1 / events_per_base);
    const float p_skip = 0.0025, p_bad = 0.001, p_bad_self = p_bad, p_skip_self = 0.3;
    const float p_mk = p_skip, p_mb = p_bad, p_mm_self = p_stay, p_mm_next = 1.0f - p_mm_self - p_mk - p_mb;
    const float p_bb = p_bad_self, p_bk = (1.0f - p_bb) / 3, p_kk = p_skip_self, p_km = 1.0f - p_kk;
    auto folded = [](float p) { return (float)log((double)p); };
    t[0] = logf(p_mm_self); t[1] = logf(p_mm_next); t[2] = folded(p_bk); t[3] = folded(p_bk); t[4] = folded(p_km);
    t[5] = 0.0f + (float)log(0.5);
    t[6] = folded(p_mb); t[7] = folded(p_bb); t[8] = folded(p_mk); t[9] = folded(p_bk); t[10] = folded(p_kk);
}

// what abea_events.hip keeps on the handle; its destructor (abea_events.hip) frees it when the handle is deleted
struct gab_abea_events_state {
    gab_devbuf io;          // staging of the host-pointer entry points
    gab_devbuf plan;        // jobs | chunk -> read
    gab_devbuf scratch;     // prefix sums, t-statistics, per-chunk peaks and detector states
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // start, after sums + t-statistics, after the detector, before / after the fill
    int64_t samples = 0, events = 0, reads_serial_sums = 0, chunks = 0, chunks_redone = 0;
    float sums_ms = 0.f, detect_ms = 0.f, fill_ms = 0.f, total_ms = 0.f;
    gab_devbuf sc_ctr;      // the scaling estimate's counters
    int64_t sc_reads = 0, sc_in_order[3] = {0, 0, 0};      // last gab_abea_scalings*: reads, and those whose event / k-mer / k-mer square sum was added in order
    ~gab_abea_events_state();
};

// what abea_calib.hip keeps on the handle; its destructor (abea_calib.hip) frees it when the handle is deleted
struct gab_abea_calib_state {
    gab_devbuf io;          // staging of the host-pointer entry point
    gab_devbuf scratch;     // counters | the double var of every read | its log_var
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // before / after the check, before the map, after the fit, after log_var is stored
    int64_t reads = 0, recalibrated = 0, m_states = 0;
    float kernel_ms = 0.f, total_ms = 0.f;
    ~gab_abea_calib_state();
};

// what abea_realign.hip keeps on the handle; its destructor (abea_realign.hip) frees it when the handle is deleted
struct gab_abea_realign_state {
    gab_devbuf io;          // staging of the host-pointer entry point
    gab_devbuf scratch;     // verdict | jobs | states | launch items | CIGAR runs | segments | k-mer ranks of the references
    gab_devbuf trace;       // the wavefronts' backpointer traces
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // before / after the preparation, after the first launch, after the requeue
    int64_t reads = 0, hmm_segments = 0, rows = 0, cells = 0, reads_requeued = 0;
    float prep_ms = 0.f, viterbi_ms = 0.f, requeue_ms = 0.f, total_ms = 0.f;
    ~gab_abea_realign_state();
};

// what abea_meth.hip keeps on the handle; its destructor (abea_meth.hip) frees it when the handle is deleted
struct gab_abea_meth_state {
    gab_devbuf cpg;         // the CpG model: mean | stdv | log stdv, 15625 entries each
    gab_devbuf table;       // the logsum table (16000 floats), built with the first CpG model
    gab_devbuf flank;       // the flank table, flank_len floats: grown by a call whose longest read needs more
    gab_devbuf io;          // staging of the host-pointer entry point
    gab_devbuf scratch;     // verdict and counters | jobs | per-read records | CIGAR runs | work items | prepared reference codes
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};      // before / after the preparation, after the scoring
    bool have_model = false;
    int64_t flank_len = 0;
    int64_t reads = 0, groups = 0, sites = 0, rows = 0, cells = 0;
    float prep_ms = 0.f, score_ms = 0.f, total_ms = 0.f;
    ~gab_abea_meth_state();
};

struct gab_abea {
    gab_host_stream hs;
    int device = 0;
    gab_devbuf model;       // mean | stdv | log stdv
    gab_devbuf io;          // staging of the host-pointer entry point
    gab_devbuf jobs, ends, kparam, trace;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // before prep, before the sweep, after it, after the backtrack
    gab_tuning tune = gab_tuning_loaded();
    int64_t cells = 0, bands = 0, launches = 0;
    float kernel_ms = 0.f, total_ms = 0.f;
    gab_abea_events_state events;
    gab_abea_calib_state calib;
    gab_abea_realign_state realign;
    gab_abea_meth_state meth;
};
