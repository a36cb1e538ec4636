// The abea handle, shared by abea.hip (align), abea_events.hip (event detection, scaling estimate) and abea_calib.hip (base-to-event
// map, recalibration, read checks) and abea_realign.hip (realign_read).
#pragma once
#include "gab_internal.h"

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
};
