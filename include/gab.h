/* gab.h -- C ABI of libgab_hip.so: the MI355X (gfx950) engine for the GenArchBench
 * banded-DP / seed-chaining hot path.
 *
 * The reference has no plugin/FFI layer: each kernel library is linked straight into
 * its benchmark's main().  Every entry point below therefore replaces one *call site*
 * of a reference driver (cited per function, paths relative to
 * /root/reference/benchmarks/).  INTEGRATION.md shows the few lines a maintainer
 * changes in each driver to call this library instead.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a negative
 *     GAB_E* code and never calls exit(); gab_last_error() gives the message for the
 *     calling thread.
 *   - the caller owns every buffer.  "_run" variants take HOST pointers and do
 *     H2D + kernels + D2H synchronously (on a private non-blocking stream of the handle, so
 *     that calls on several handles of one GPU overlap); "_run_device" variants take DEVICE pointers
 *     (hipMalloc'ed or a torch tensor's data_ptr) and enqueue on `stream` (a hipStream_t passed
 *     as void*, NULL = the default stream); each entry says where it synchronises `stream`
 *     internally.  Three of them run part of their kernels on streams of the handle: bsw (an aux stream for every
 *     other class launch and, in a sliced call, a sort stream), bpm (an aux stream for the band kernels) and chain (one
 *     stream for the latency form and one for the table form, beside the throughput form on `stream`).  These are forked
 *     from and joined back into `stream` by events inside the call, so the caller only ever has to order against `stream`:
 *     inputs that earlier work on `stream` produces are read after it, the host's own planning copies (lengths, offsets,
 *     counters) go through `stream` too, and once the call's work on `stream` has completed nothing of the call reads an
 *     input or writes an output any more.  tests/test_stream_order_gpu.py holds every `_device` entry point to this.
 *   - a handle's work buffers belong to one call at a time, and some entry points (bsw, bpm) return with kernels still
 *     queued.  The next call on the same handle may be issued on the SAME stream at once; on ANOTHER stream only after
 *     the previous call's work on its stream has completed (synchronise that stream first): nothing inside the library
 *     orders the streams of two calls against each other, and the second call would reuse the workspace under the first.
 *   - a handle is bound to one GPU; calls on distinct handles are thread-safe, so the
 *     multi-GPU drivers run one host thread (or one process) per GPU with no collective.
 */
#ifndef GAB_H
#define GAB_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAB_OK 0
#define GAB_EINVAL (-22)   /* bad argument / unsupported size  */
#define GAB_ENOMEM (-12)   /* host or device allocation failed */
#define GAB_EDEVICE (-5)   /* HIP runtime error                */
#define GAB_ENODEV (-19)   /* no usable gfx950 device          */
#define GAB_ERANGE (-34)   /* result larger than the caller's buffer (the needed size is returned) */

/* ---- library ------------------------------------------------------------------- */
const char *gab_version(void);
const char *gab_last_error(void);
int gab_device_count(void);
/* PCI bus id ("0000:c1:00.0") of a device into buf (len >= 16): what the drivers need to find the NUMA node a card hangs
 * off (/sys/bus/pci/devices/<id>/numa_node) and place its worker threads there, as the reference places its threads with
 * OMP_PROC_BIND / OMP_PLACES (bsw/scripts/regression_small.sh:52) */
int gab_device_pci_bus_id(int device, char *buf, int len);
/* device memory for C callers that chain two *_device entry points (e.g. parser -> kernel) without a HIP toolchain */
int gab_device_alloc(int device, size_t bytes, void **out);
void gab_device_free(int device, void *p);
int gab_device_copy_to_host(int device, void *dst, const void *d_src, size_t bytes);
/* pinned (page-locked) host memory for the slabs handed to the host-pointer entry points gab_*_run: where the reference
 * drivers allocate theirs before the region of interest (_mm_malloc, bsw/src/main_banded.cpp:260-264; malloc / std::vector
 * elsewhere).  gab_*_run accepts any host memory; from pinned memory its chunked copies are direct DMA that overlaps the
 * kernels, from pageable memory the runtime stages them at a fraction of the link rate. */
int gab_host_alloc(size_t bytes, void **out);
void gab_host_free(void *p);
/* same, in place, for memory the caller already owns (malloc / realloc / std::vector storage): page-locks
 * [p, p + bytes) until gab_host_unregister(p); do it after the buffer has reached its final size, outside the ROI */
int gab_host_register(void *p, size_t bytes);
void gab_host_unregister(void *p);

/* ---- bsw: banded Smith-Waterman seed extension ------------------------------------
 * Replaces  bsw[tid]->getScores16(SeqPair*, ref, qer, nPairsBatch, 1, w)
 *           bsw/src/main_banded.cpp:338-350  (class: bsw/src/bandedSWA.h:240-245;
 *           semantics: scalarBandedSWA, bsw/src/bandedSWA.cpp:132-253).
 * Instead of T threads x batches of B pairs, the GPU driver makes ONE call over all
 * pairs inside the same region of interest.
 */
typedef struct gab_bsw gab_bsw;
typedef struct {
    int32_t o_del, e_del, o_ins, e_ins; /* BandedPairWiseSW ctor, bandedSWA.cpp:48-66    */
    int32_t zdrop, end_bonus;           /* main_banded.cpp:268                            */
    int32_t w;                          /* band width passed to getScores16 (100)         */
    int8_t mat[25];                     /* 5x5 scores, codes 0..3 = ACGT, 4 = N           */
} gab_bsw_params;

/* Limits (same as the reference driver's slabs, main_banded.cpp:76-79): query length
 * 1..256, reference length 1..32767, 0 <= h0, and h0 + qlen * max(mat) <= 2^30. */
#define GAB_BSW_MAX_QLEN 256
#define GAB_BSW_MAX_TLEN 32767

/* full extension result, as scalarBandedSWA returns it (bandedSWA.cpp:241-252) */
typedef struct {
    int32_t score, qle, tle, gtle, gscore, max_off;
} gab_bsw_result;

int gab_bsw_create(const gab_bsw_params *params, int device, gab_bsw **out);
void gab_bsw_destroy(gab_bsw *h);

/* optional: size the handle's device buffers now for calls of up to max_pairs pairs whose referenced windows of the two
 * slabs are at most max_ref_bytes / max_qry_bytes, so that the first gab_bsw_run of a timed region does not allocate
 * (the reference allocates its working buffers in the BandedPairWiseSW constructor, bsw/src/bandedSWA.cpp:80-96) */
int gab_bsw_reserve(gab_bsw *h, int64_t max_pairs, int64_t max_ref_bytes, int64_t max_qry_bytes);

/* Host buffers.  Pair i: reference (target) = ref[ref_off[i] .. +len1[i]), query =
 * qry[qry_off[i] .. +len2[i]), base codes 0..4 one byte each (what loadPairs produces,
 * main_banded.cpp:164-206), seed score h0[i].  score_out[i] = SeqPair.score. */
int gab_bsw_run(gab_bsw *h, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry,
                const int64_t *qry_off, const int32_t *len1, const int32_t *len2,
                const int32_t *h0, int64_t n, int32_t *score_out);

/* Device buffers.  Enqueues on `stream`, but synchronises it once mid-way (the launch geometry of the DP kernels needs
 * the sizes of the query-length classes on the host); the DP launches and the result stores that follow are asynchronous:
 * order later work against `stream` (or synchronise it) before reading score_out.  ref_bytes / qry_bytes = sizes of the two
 * sequence slabs, used for bounds validation: the kernels read a sequence four bytes at a time from its own (possibly
 * unaligned) start, so every sequence must be followed by at least 3 more bytes INSIDE its slab (off + len + 3 <= bytes;
 * their contents do not matter).  result_out may be NULL;
 * when given it receives all six result fields per pair.  On GAB_EINVAL the contents of score_out and result_out are
 * unspecified (nothing writes them any more once the call has returned). */
int gab_bsw_run_device(gab_bsw *h, const uint8_t *ref, int64_t ref_bytes, const int64_t *ref_off,
                       const uint8_t *qry, int64_t qry_bytes, const int64_t *qry_off,
                       const int32_t *len1, const int32_t *len2, const int32_t *h0, int64_t n,
                       int32_t *score_out, gab_bsw_result *result_out, void *stream);

/* Counters of the last run on this handle (for the roofline report): number of DP
 * cells evaluated (sum over rows of band width) and device time of the dominant kernel
 * as measured with HIP events on the run's stream (ms).
 * `cells` counts the cells the kernels evaluated.  With result_out given that is the
 * reference's own count.  A score-only call (gab_bsw_run, or gab_bsw_run_device with
 * result_out NULL) ends a pair's row loop once no later row can raise its score, so it
 * evaluates -- and counts -- fewer cells than the reference does for the same scores. */
int gab_bsw_last_stats(gab_bsw *h, int64_t *cells, float *kernel_ms, float *total_ms);

/* ---- chain / fast-chain: minimap2 seed chaining ------------------------------------
 * Replaces  host_chain_kernel(std::vector<call_t>&, std::vector<return_t>&, numThreads)
 *           chain/src/main.cpp:154 and fast-chain/src/main.cpp:154 (declared in each src/host_kernel.h:6;
 *           kernels chain/src/host_kernel.cpp:30-108, fast-chain/src/host_kernel.cpp:135-865).
 * The reference call is already a whole-input batch call; so is this one.
 * Anchors of all calls lie back to back: call c owns x/y/score/parent[call_off[c] ..
 * call_off[c] + hdr[c].n).  x, y are minimap2's mm128_t words (chain/src/host_data.h:18-21):
 * x = ref id/strand/pos (ascending), y = seg_id << 48 | q_span << 32 | query_pos.
 * Outputs are return_t.scores / return_t.parents (host_data.h:30-36).
 * call_off need not ascend and may leave gaps between calls; an empty call may point anywhere.  The arrays hold `total` elements,
 * total = the largest call_off[c] + hdr[c].n.  Every element of a call receives its result.  The elements of the HOST result
 * arrays (score_out / parent_out, host_score / host_parent) that lie below `total` but inside no call may be overwritten with
 * unspecified values -- they are wherever the arrays are filled by a copy of [0, total), and keep their contents where the
 * kernels write them through --, and x / y may be read there; the kernels store to the calls' own elements of d_score /
 * d_parent only.  Nothing at or beyond `total` is touched.
 */
#define GAB_CHAIN 0      /* chain:      max_skip / max_iter heuristics, 64-bit coordinates   */
#define GAB_FASTCHAIN 1  /* fast-chain: no max_skip, 32-bit coordinates, AVX2/AVX-512 rounding */
typedef struct gab_chain gab_chain;
typedef struct {           /* call_t header, chain/src/host_data.h:23-28 */
    int64_t n;
    float avg_qspan;
    int32_t max_dist_x, max_dist_y, bw, n_segs;
} gab_chain_hdr;

int gab_chain_create(int device, gab_chain **out);
void gab_chain_destroy(gab_chain *h);
/* optional: size the handle's device buffers now for calls of up to max_anchors anchors in max_calls calls (see gab_bsw_reserve) */
int gab_chain_reserve(gab_chain *h, int64_t max_anchors, int64_t max_calls);
/* gab_chain_reserve + what gab_chain_run_device[_through] of `mode` needs before a timed region: the first launches of its kernels
 * and, for GAB_FASTCHAIN (whose longer calls run in the table form, chain_tab.hip), the table for max_anchors anchors */
int gab_chain_reserve_mode(gab_chain *h, int mode, int64_t max_anchors, int64_t max_calls);
/* everything on the host */
int gab_chain_run(gab_chain *h, int mode, const uint64_t *x, const uint64_t *y, const int64_t *call_off,
                  const gab_chain_hdr *hdr, int64_t ncalls, int32_t *score_out, int32_t *parent_out);
/* anchors and results on the device; the small call table (call_off, hdr) stays on the host.
 * Returns after the kernel has completed on `stream`. */
int gab_chain_run_device(gab_chain *h, int mode, const uint64_t *d_x, const uint64_t *d_y,
                         const int64_t *call_off, const gab_chain_hdr *hdr, int64_t ncalls,
                         int32_t *d_score, int32_t *d_parent, void *stream);
/* The same, with the results in HOST memory as well when the call returns (a driver whose read phase parsed the file on the GPU,
 * gab_chain_parse): d_score / d_parent are filled as always, host_score / host_parent (page-locked for the fast way: the DP kernel
 * then writes every block of results through to them while it runs; pageable or small batches: copied at the end) receive them too. */
int gab_chain_run_device_through(gab_chain *h, int mode, const uint64_t *d_x, const uint64_t *d_y,
                                 const int64_t *call_off, const gab_chain_hdr *hdr, int64_t ncalls,
                                 int32_t *d_score, int32_t *d_parent, int32_t *host_score, int32_t *host_parent, void *stream);
/* predecessor evaluations performed (chain: the whole window of an anchor resolved by the plain-maximum path, plus the
 * reference's own visits for the anchors that needed its max_skip scan; fast-chain: the windows) and kernel time (HIP
 * events) of the last run */
int gab_chain_last_stats(gab_chain *h, int64_t *evals, float *kernel_ms);
/* which kernel form took each call of the last gab_chain_run_device / _through call on this handle (gab_chain_run too, where it
 * goes through gab_chain_run_device: batches below its big-batch paths).  ncalls must be that call's.  form[c], in the caller's call order:
 *   0 empty call
 *   1 throughput form
 *   2 latency form
 *   3 table form, folded there
 *   4 table form, not eligible
 *   5 table form, eligible but handed back (no room in the table, or by the fold)
 *   6 the legacy-only launch (GAB_CHAIN_KERNEL=walk for GAB_CHAIN, or GAB_CHAIN_HELPERS set)
 * (4 and 5: the call was then computed by the latency-form kernel behind the table form.)
 * counters: {calls that found no room in the table, exact re-scans that confirmed the fold's result, helper waves of the legacy-only
 * launch or 0, 16-row groups of table the eligible calls needed}.  form and counters may be NULL.
 * A run records nothing for this on the device and copies nothing: the call list of the table form is read here, from the
 * handle's buffers, where it stays until the handle's next run (or gab_chain_reserve_mode call, whose warm-up run uses them).
 * GAB_EINVAL: no such run since, or another ncalls. */
int gab_chain_last_split(gab_chain *h, int64_t ncalls, uint8_t *form, int64_t counters[4]);
/* how host_score / host_parent of the last gab_chain_run_device / _through call on this handle were filled.  Valid when
 * gab_chain_last_split is (GAB_EINVAL otherwise), and like it host state of that call: a run records nothing for it on the device
 * and copies nothing.
 * A batch without an anchor (ncalls == 0, or only empty calls) launches, writes and copies nothing: GAB_CHAIN_THROUGH_WRITTEN when
 * host arrays were passed, whether page-locked or not (no launch that does not write through took part, no copy was made), else
 * GAB_CHAIN_THROUGH_NONE. */
#define GAB_CHAIN_THROUGH_NONE 0             /* not asked for (gab_chain_run_device) */
#define GAB_CHAIN_THROUGH_WRITTEN 1          /* written through by the kernels while they ran, no copy */
#define GAB_CHAIN_THROUGH_COPIED_PAGEABLE 2  /* copied at the end: the host arrays are not page-locked */
#define GAB_CHAIN_THROUGH_COPIED_FORM 3      /* copied at the end: a launch that does not write through took part (the latency form; the
                                              * legacy-only launch with 5 or 7 helper waves or the walk kernel; a batch in the throughput
                                              * form alone that is given seven helper waves: last anchor's end <= 326 x its longest call) */
#define GAB_CHAIN_THROUGH_WRITTEN_COPIED 4   /* written through, then copied after all: the table form handed a call back */
int gab_chain_last_through(gab_chain *h, int *route);

/* ---- bpm: bit-parallel Myers edit distance (+ backtrace-derived score) -----------------
 * Replaces  it->score = benchmark_edit_bpm(&align_input)   bpm/tools/align_benchmark.c:243-257
 *           (bpm/benchmark/benchmark_edit.c:31-56; kernel bpm/edit/edit_bpm.c:70-331).
 * One call over all pairs instead of one call per pair.  The caller has already applied the
 * driver's swap (the longer line is the pattern, align_benchmark.c:177-181) and stripped the
 * leading '>' / '<' and the newline (:247-252): text_length <= pattern_length is required,
 * exactly the condition under which the reference never cuts a block off.
 * Sequences are raw ASCII bytes: pair i = pat[pat_off[i] .. +pat_len[i]), txt[...].
 * score_out[i] = the value the reference prints as "[i] score=%d" (<= 0).
 */
#define GAB_BPM_MAX_PLEN 16320 /* 255 x 64: top_level is a uint8_t, bpm/edit/edit_bpm.c:205-206 */
typedef struct gab_bpm gab_bpm;
int gab_bpm_create(int device, gab_bpm **out);
void gab_bpm_destroy(gab_bpm *h);
/* optional, outside the timed region: device buffers for calls of up to max_pairs pairs whose sequences span up to
 * max_seq_bytes of the slab(s), and warm copy queues (see gab_bsw_reserve).  pat and txt may be the same slab (the drivers'
 * pair files): its window is then staged once. */
int gab_bpm_reserve(gab_bpm *h, int64_t max_pairs, int64_t max_seq_bytes);
int gab_bpm_run(gab_bpm *h, const char *pat, const int64_t *pat_off, const int32_t *pat_len,
                const char *txt, const int64_t *txt_off, const int32_t *txt_len, int64_t n,
                int32_t *score_out);
/* device buffers; pat_bytes / txt_bytes = slab sizes: every sequence must be followed by at least 3 more bytes
 * inside its slab (off + len + 3 <= bytes; the kernels read four bytes at a time from the sequence's own start).
 * Synchronises `stream` once near the start (the sizes of the pattern-length classes come to the host for the launch
 * geometry) and, only when the batch holds patterns of more than 256 bases, again per batch of those pairs.  The score,
 * band, window and full-column launches of the other pairs are asynchronous, the band kernels on the handle's aux stream
 * joined back into `stream`: order later work against `stream` (or synchronise it) before reading score_out. */
int gab_bpm_run_device(gab_bpm *h, const char *pat, int64_t pat_bytes, const int64_t *pat_off,
                       const int32_t *pat_len, const char *txt, int64_t txt_bytes,
                       const int64_t *txt_off, const int32_t *txt_len, int64_t n,
                       int32_t *score_out, void *stream);
/* last run: 64-row block steps executed, pairs that needed the history + backtrace path,
 * device time of the score kernels together with the first backtrace stage that runs underneath them, and of the
 * whole call (HIP events, ms) */
int gab_bpm_last_stats(gab_bpm *h, int64_t *block_steps, int64_t *full_pairs,
                       float *score_kernel_ms, float *total_ms);

/* ---- bitpal: the bpm driver's BitPAl algorithms (global alignment score, no CIGAR) -----------
 * Replaces  it->score = benchmark_bitpal_m0_x1_g1(&align_input)   (-a bitpal-edit)
 *           it->score = benchmark_bitpal_m1_x4_g2(&align_input)   (-a bitpal-scored)
 *                                                    bpm/tools/align_benchmark.c:259-264, 330-338
 *           (bpm/benchmark/benchmark_bitpal.c:30-54; generated kernels bpm/bitpal/bitpal.m0.x1.g1.c,
 *            bpm/bitpal/bitpal.m1.x4.g2.c).
 * score_out[i] = the Needleman-Wunsch score of pair i: global, linear gaps, raw-byte comparison, with
 * (match, mismatch, gap) = (0, -1, -1) for GAB_BITPAL_EDIT and (+1, -4, -2) for GAB_BITPAL_SCORED --
 * the value the reference prints as "[i] score=%d".  Same buffers as gab_bpm_run; the score is
 * symmetric in the two strings, so the driver's swap is immaterial and not required.
 */
#define GAB_BITPAL_EDIT 0
#define GAB_BITPAL_SCORED 1
#define GAB_BITPAL_MAX_LEN 16320 /* kept equal to GAB_BPM_MAX_PLEN: the two algorithms share the driver and its inputs */
typedef struct gab_bitpal gab_bitpal;
int gab_bitpal_create(int algorithm, int device, gab_bitpal **out);
void gab_bitpal_destroy(gab_bitpal *h);
int gab_bitpal_reserve(gab_bitpal *h, int64_t max_pairs, int64_t max_seq_bytes);      /* see gab_bpm_reserve */
int gab_bitpal_run(gab_bitpal *h, const char *pat, const int64_t *pat_off, const int32_t *pat_len,
                   const char *txt, const int64_t *txt_off, const int32_t *txt_len, int64_t n,
                   int32_t *score_out);
/* device buffers; slabs readable to a multiple of 4 bytes past the last sequence; synchronises `stream` */
int gab_bitpal_run_device(gab_bitpal *h, const char *pat, int64_t pat_bytes, const int64_t *pat_off,
                          const int32_t *pat_len, const char *txt, int64_t txt_bytes,
                          const int64_t *txt_off, const int32_t *txt_len, int64_t n,
                          int32_t *score_out, void *stream);
/* last run: DP cells (pattern_length x text_length summed), pairs that took the global-scratch path,
 * device time of the DP kernels and of the whole call (HIP events, ms) */
int gab_bitpal_last_stats(gab_bitpal *h, int64_t *cells, int64_t *long_pairs, float *kernel_ms, float *total_ms);
/* last run: which kernel scored what.  Values the host side holds after the run anyway: the call launches, allocates and copies
 * nothing.  GAB_EINVAL without a completed run, like gab_bitpal_last_stats. */
enum {
    GAB_BITPAL_PATH_BV_WORDS,      /* D of the bitpal_edit_bv launch; 0: not launched */
    GAB_BITPAL_PATH_BV_PAIRS,      /* pairs the bit-vector kernel scored (n minus its rejects) */
    GAB_BITPAL_PATH_LDS_PAIRS,     /* pairs bitpal_dp<true, .> scored */
    GAB_BITPAL_PATH_LDS_ROWS,      /* rows its LDS column was sized for (0: not launched) */
    GAB_BITPAL_PATH_GLOBAL_PAIRS,  /* pairs bitpal_dp<false, .> scored */
    GAB_BITPAL_PATH_GLOBAL_BLOCKS, /* its workgroups (0: not launched) */
    GAB_BITPAL_PATH_GLOBAL_ROWS,   /* rows its scratch slices were sized for */
    GAB_BITPAL_PATH_ID_LISTS,      /* 1: the DP kernels read id lists, 0: slot = pair (or no DP kernel ran) */
    GAB_BITPAL_PATHS
};
int gab_bitpal_last_paths(gab_bitpal *h, int64_t paths[GAB_BITPAL_PATHS]);

/* ---- wfa: gap-affine wavefront alignment with CIGAR ---------------------------------------
 * Replaces  affine_wavefronts_clear(wf); affine_wavefronts_align(wf, pattern, plen, text, tlen);
 *           + the copy of wf->edit_cigar            wfa/tools/align_benchmark.c:415-437
 *           (kernel: wfa/gap_affine/affine_wavefront_align.c:325-361 and the files it calls).
 * One call over all pairs.  No swap: the '>' line is the pattern, the '<' line the text
 * (align_benchmark.c:152-160).  gab_wfa_create = complete mode (affine_wavefronts_new_complete, the
 * driver's default min_wavefront_length = -1, align_benchmark.c:91,359-363); gab_wfa_create_reduced =
 * the adaptive reduction (affine_wavefronts_new_reduced, wfa/gap_affine/affine_wavefront.c:162-181,
 * driver flags --minimum-wavefront-length / --maximum-difference-distance, align_benchmark.c:267-272,
 * 364-368; the heuristic of affine_wavefronts_reduce_wavefronts, affine_wavefront_extend.c:85-154).
 * min_wavefront_length < 0 selects the complete mode, as in the driver.
 * ops_out receives, for pair i, ops_len_out[i] operations 'M','X','I','D' starting at
 * ops_out[ops_off[i]]; the caller provides pattern_length + text_length bytes of room per pair
 * (edit_cigar_allocate, wfa/gap_affine/edit_cigar.c:38-47) and run-length encodes them when
 * printing (edit_cigar_print, :184-200).  score_out[i] = the alignment penalty.
 * Bytes equal to the reference's padding characters -- 'Y' in a pattern, 'X' in a text -- match the OTHER sequence's
 * padding as they do in the reference (wfa/utils/string_padded.c:88-117), so an alignment can run past the end of a
 * sequence.  Where that makes the CIGAR longer than pattern_length + text_length the reference overflows its buffer;
 * this library keeps the last pattern_length + text_length operations (never written outside the pair's room).
 */
#define GAB_WFA_MAX_LEN 100000 /* MAX_SEQUENCE_LENGTH, wfa/tools/align_benchmark.c:62 */
typedef struct gab_wfa gab_wfa;
typedef struct {
    int32_t mismatch, gap_opening, gap_extension; /* defaults 4, 6, 2 (align_benchmark.c:85-90); match = 0 */
} gab_wfa_penalties;
int gab_wfa_create(const gab_wfa_penalties *penalties, int device, gab_wfa **out);
int gab_wfa_create_reduced(const gab_wfa_penalties *penalties, int min_wavefront_length, int max_distance_threshold,
                           int device, gab_wfa **out);
void gab_wfa_destroy(gab_wfa *h);
/* see gab_bpm_reserve; max_ops_bytes = the room of the CIGAR operations of a call (pattern + text length per pair) */
int gab_wfa_reserve(gab_wfa *h, int64_t max_pairs, int64_t max_seq_bytes, int64_t max_ops_bytes);
int gab_wfa_run(gab_wfa *h, const char *pat, const int64_t *pat_off, const int32_t *pat_len,
                const char *txt, const int64_t *txt_off, const int32_t *txt_len, int64_t n,
                char *ops_out, const int64_t *ops_off, int32_t *ops_len_out, int32_t *score_out);
/* The same call for a driver that PRINTS the alignments (wfa/tools/align_benchmark.c:499-504): the result is the text
 * edit_cigar_print writes (wfa/gap_affine/edit_cigar.c:184-200) -- every run of equal operations as "%d%c", e.g. "70M1X80M" --
 * encoded on the device, so that ~20 bytes per 151-bp pair cross the bus instead of pattern_length + text_length bytes of
 * operation room.  Pair i's text is cigar_out[cigar_off_out[i] .. + cigar_len_out[i]) (no terminator; an empty CIGAR has
 * length 0; the texts are packed without gaps but NOT in pair order).  *cigar_bytes = bytes of text produced; when that exceeds
 * `capacity` no text is written and the call returns GAB_ERANGE (offsets, lengths and scores are valid): call again with
 * *cigar_bytes of room.  2 * (pattern_length + text_length) per pair always suffices; a quarter of the operation room is
 * ample for reads. */
int gab_wfa_run_packed(gab_wfa *h, const char *pat, const int64_t *pat_off, const int32_t *pat_len,
                       const char *txt, const int64_t *txt_off, const int32_t *txt_len, int64_t n,
                       char *cigar_out, int64_t capacity, int64_t *cigar_off_out, int32_t *cigar_len_out,
                       int32_t *score_out, int64_t *cigar_bytes);
/* The same for pairs that are already on the device (the read phase parsed the file there: gab_pairs_parse): DEVICE pointers in as
 * for gab_wfa_run_device -- `ops` / `ops_off` is operation room on the device, pattern_length + text_length bytes per pair, scratch
 * of the caller -- and the printed text, offsets, lengths and scores out to HOST memory as above (GAB_ERANGE likewise).
 * It takes no stream: it runs on the handle's private stream, which orders against no other, and returns when the results
 * are in host memory.  The device inputs must be complete before the call (gab_pairs_parse is, when it returns). */
int gab_wfa_run_packed_device(gab_wfa *h, const char *pat, int64_t pat_bytes, const int64_t *pat_off, const int32_t *pat_len,
                              const char *txt, int64_t txt_bytes, const int64_t *txt_off, const int32_t *txt_len, int64_t n,
                              char *ops, const int64_t *ops_off, char *cigar_out, int64_t capacity, int64_t *cigar_off_out,
                              int32_t *cigar_len_out, int32_t *score_out, int64_t *cigar_bytes);
/* device buffers (sequence slabs readable to a multiple of 4 bytes past the last base);
 * synchronises `stream` internally between its passes and behind the last one: the outputs are complete when it returns */
int gab_wfa_run_device(gab_wfa *h, const char *pat, int64_t pat_bytes, const int64_t *pat_off,
                       const int32_t *pat_len, const char *txt, int64_t txt_bytes,
                       const int64_t *txt_off, const int32_t *txt_len, int64_t n, char *ops_out,
                       const int64_t *ops_off, int32_t *ops_len_out, int32_t *score_out, void *stream);
/* last run: wavefront cells computed + bases extended, pairs re-run with a larger history,
 * device time of the first (LDS) pass and of the whole call (HIP events, ms) */
int gab_wfa_last_stats(gab_wfa *h, int64_t *work, int64_t *requeued, float *first_pass_ms, float *total_ms);

/* ---- fmi: FM-index SMEM seeding --------------------------------------------------------------
 * Replaces, per batch of reads, the sequence
 *     getSMEMsAllPosOneThread -> select -> getSMEMsOnePosOneThread -> bwtSeedStrategyAllPosOneThread
 *     -> rid += batch offset -> sortSMEMs                          fmi/fmi.cpp:288-348
 * on a shared read-only FMI_search (fmi/bwa-mem2/x86_64/src/FMI_search.h:101-...), and
 *     new FMI_search(prefix); load_index()                         fmi/fmi.cpp:102-103
 * by gab_fmi_load (outside the region of interest, as in the reference).  The index file is the
 * reference's own <prefix>.bwt.2bit.64 (FMI_search.cpp:144-304), read unchanged; only the count[],
 * CP_OCC[] and sentinel_index parts are used by seeding.
 * Reads are the driver's dense code matrix (fmi.cpp:121-151): read r = enc[r*stride .. +len[r]),
 * codes 0..3 = ACGT, anything above 3 = N.  Constants of the driver are fixed: re-seed width 10,
 * split factor 1.5, third-pass interval 20 (fmi.cpp:162-164).
 * Output: SMEM records (FMI_search.h:75-83) of ALL reads sorted by (rid, m ascending, n descending)
 * -- the order the driver prints -- as [m, n] inclusive query interval and the bi-interval k, l, s.
 */
#define GAB_FMI_MAX_READLEN 10000 /* assert(max_readlength < 10000), fmi/fmi.cpp:117 */
typedef struct gab_fmi gab_fmi;
typedef struct {
    uint32_t rid, m, n, pad;
    int64_t k, l, s;
} gab_smem; /* 40 bytes, layout of SMEM */
int gab_fmi_load(int device, const char *prefix, gab_fmi **out);
/* same, from memory: the three parts of the file as the reference writes them (count[] NOT yet +1) */
int gab_fmi_create(int device, int64_t reference_seq_len, const int64_t count[5], const void *cp_occ,
                   int64_t sentinel_index, gab_fmi **out);
/* a second handle on the same GPU that SHARES the read-only index of `src` (which must outlive it; attach the suffix
 * array to src first) and owns only its work buffers: the drivers run several host threads per GPU, each with its own
 * handle, the way the reference's threads share one FMI_search (fmi/fmi.cpp:102-103,250-263) */
int gab_fmi_clone(gab_fmi *src, gab_fmi **out);
void gab_fmi_destroy(gab_fmi *h);
/* host buffers; *out is malloc'ed by the library, release it with gab_fmi_free */
int gab_fmi_seed(gab_fmi *h, const uint8_t *enc, int32_t stride, const int32_t *len, int64_t nreads,
                 int32_t min_seed_len, gab_smem **out, int64_t *nout);
void gab_fmi_free(gab_smem *p);
/* same, into the CALLER's array of `capacity` records -- how the reference's threads collect their SMEMs: per-thread arrays
 * allocated before the region of interest and grown when a batch does not fit (fmi/fmi.cpp:242, 253-257, 277-286).  Page-lock
 * the array (gab_host_alloc / gab_host_register) and the result arrives as one DMA at the link rate instead of through
 * the runtime's staging of pageable memory.  *nout = SMEMs found; when that exceeds `capacity` nothing is written and the
 * call returns GAB_ERANGE: grow the array to *nout and call again. */
int gab_fmi_seed_into(gab_fmi *h, const uint8_t *enc, int32_t stride, const int32_t *len, int64_t nreads,
                      int32_t min_seed_len, gab_smem *out, int64_t capacity, int64_t *nout);
/* optional: size the handle's device buffers now for host-pointer calls of up to max_reads reads of `stride` bases and push
 * an empty batch of that size through the whole path (see gab_bsw_reserve): a driver that times ONE pass (fmi/fmi.cpp:236-362)
 * would otherwise allocate gigabytes of slots and output inside its region of interest */
int gab_fmi_reserve(gab_fmi *h, int64_t max_reads, int32_t stride);
/* device buffers; *d_out / *d_read_off (nreads + 1 offsets into d_out) point into memory owned by the
 * handle and stay valid until the next call on it.  Synchronises `stream` internally. */
int gab_fmi_seed_device(gab_fmi *h, const uint8_t *d_enc, int32_t stride, const int32_t *d_len,
                        int64_t nreads, int32_t min_seed_len, const gab_smem **d_out,
                        const int64_t **d_read_off, int64_t *nout, void *stream);
/* last run: backwardExt calls, SMEMs found, seeding-kernel ms */
int gab_fmi_last_stats(gab_fmi *h, int64_t *ext_calls, int64_t *nsmem, float *kernel_ms);
/* last run: 64-byte CP_OCC records the extensions fetched (GET_OCC, FMI_search.h:66-73: one when both interval
 * ends share a record, else two) -- the random index traffic of the run is 64 B x this number */
int gab_fmi_last_records(gab_fmi *h, int64_t *cp_occ_records);
/* last run: which route of the seeding path took what, summed over the batches of the call (of a batch that ran twice, the
 * round that was kept).  Read from the counters the kernels keep anyway; the call allocates and copies nothing on the device.
 * GAB_EINVAL without a completed run; gab_fmi_reserve leaves the answer as it was. */
enum {
    GAB_FMI_PATH_BATCHES,            /* launches of the seeding kernel over a slice of the reads */
    GAB_FMI_PATH_FORM,               /* 1: read and interval lists in LDS (stride <= 256), 0: lists in global scratch */
    GAB_FMI_PATH_LDS_ENTRIES,        /* entries of the LDS ring per lane (0 in the global form) */
    GAB_FMI_PATH_LIST_ENTRY_BYTES,   /* 13 or 16 (0 in the global form) */
    GAB_FMI_PATH_KMER_DEPTH,         /* depth of the short-pattern table the kernel used (0: none) */
    GAB_FMI_PATH_WIDE_MIN,           /* survivors that make a backward phase wide; 0 when phases are not handed over */
    GAB_FMI_PATH_POSITIONS,          /* seeding positions whose backward phase the seeding kernel started */
    GAB_FMI_PATH_LIST_SUM,           /* sum of their forward list lengths */
    GAB_FMI_PATH_SPILLS,             /* those whose list outgrew the ring */
    GAB_FMI_PATH_INDEX_EXT,          /* extensions answered by the index; + TABLE_EXT = ext_calls of gab_fmi_last_stats */
    GAB_FMI_PATH_TABLE_EXT,          /* extensions answered by the short-pattern table */
    GAB_FMI_PATH_WIDE_ITEMS,         /* wide backward phases handed to the wide kernel (those that got a place) */
    GAB_FMI_PATH_WIDE_ENTRIES,       /* list entries handed over with them */
    GAB_FMI_PATH_WIDE_CANDS,         /* re-seeding candidates the handed-over phases found */
    GAB_FMI_PATH_RERUNS,             /* batches run again without hand-over (candidates outgrew their queue) */
    GAB_FMI_PATH_OVERFLOW_READS,     /* reads whose SMEMs did not fit the first-round slot */
    GAB_FMI_PATH_SECOND_ROUND_PARTS, /* launches of the second round over them */
    GAB_FMI_PATH_MAX_PER_READ,       /* most SMEMs of one read */
    GAB_FMI_PATH_OUT_GROWTHS,        /* times the output array was re-allocated */
    GAB_FMI_PATHS
};
int gab_fmi_last_paths(gab_fmi *h, int64_t paths[GAB_FMI_PATHS]);

/* ---- fmi: suffix-array look-up -- the step BWA-MEM2 takes right after seeding:
 *     FMI_search::get_sa_entries(SMEM *smemArray, int64_t *coordArray, int32_t *coordCountArray, uint32_t count,
 *                                int32_t max_occ, int tid)          FMI_search.cpp:1177-1196
 *     -> get_sa_entry_compressed (SA_COMPX = 3)                     FMI_search.cpp:1103-1175
 * For SMEM i the BWT rows k, k+step, ... (< k+s, at most max_occ of them; step = s > max_occ ? s / max_occ : 1) are
 * resolved to reference coordinates: a row that is a multiple of 8 is stored, any other row walks the LF mapping (one
 * CP_OCC record per step) to a stored row or the sentinel.  Coordinates come back to back in SMEM order;
 * coord_off[n + 1] delimits them (the reference only returns the running total).
 * gab_fmi_load reads the sampled suffix array from <prefix>.bwt.2bit.64; a handle made by gab_fmi_create gets it
 * with gab_fmi_set_sa (arrays of (reference_seq_len >> 3) + 1 entries, FMI_search.cpp:439-447). */
int gab_fmi_set_sa(gab_fmi *h, const int8_t *sa_ms_byte, const uint32_t *sa_ls_word);
/* host buffers; *coords and *coord_off are malloc'ed by the library, release them with gab_fmi_free_coords */
int gab_fmi_sa_lookup(gab_fmi *h, const gab_smem *smems, int64_t n, int32_t max_occ, int64_t **coords,
                      int64_t **coord_off, int64_t *total);
void gab_fmi_free_coords(int64_t *p);
/* device buffers; the outputs point into memory owned by the handle, valid until the next call on it.  Synchronises `stream`
 * twice: after the counting pass (the total sizes the coordinate array) and at the end (lf_steps), so the coordinates are
 * complete when it returns */
int gab_fmi_sa_lookup_device(gab_fmi *h, const gab_smem *d_smems, int64_t n, int32_t max_occ,
                             const int64_t **d_coords, const int64_t **d_coord_off, int64_t *total, void *stream);
/* last look-up: LF-mapping steps taken (one random 64-byte CP_OCC record each) and kernel ms */
int gab_fmi_last_sa_stats(gab_fmi *h, int64_t *lf_steps, float *kernel_ms);

/* ---- kmer-cnt: exact canonical k-mer counting (Flye's solid k-mer counter) ----------------------------
 * Replaces  vertexIndex.countKmers()                                kmer-cnt/kmer_cnt.cpp:290
 *           -> KmerCounter::count(true), the COUNT_VERSION == 3 body kmer-cnt/vertex_index.cpp:787-860
 *           (k-mer arithmetic and standardForm: kmer-cnt/kmer.h:22-64; the iterator whose end is the last position, so that a
 *            read of length L yields L - k k-mers: kmer-cnt/kmer.h:177-198).
 * Reads are ASCII, read i = seq[off[i] .. +len[i]), bytes ACGTacgt only: what the reference makes of any other byte
 * (validateSequence, kmer-cnt/sequence_container.cpp:318-328, and the 2-bit packing, kmer-cnt/sequence.h:54-69: INTEGRATION.md)
 * is a property of its file reader and stays in the driver.
 * Only reads with len > min_len_exclusive are counted (loadFromFile, kmer-cnt/sequence_container.cpp:100-106), forward strand only
 * (kmer-cnt/vertex_index.cpp:812), every k-mer in its canonical form (the smaller of itself and its reverse complement, first base in
 * the most significant digit, A C G T = 0 1 2 3).
 * The reference keeps one WRAPPING 8-bit counter per possible k-mer; this library counts exactly, in a table sized from the
 * input, and derives the reference's two printed numbers from the exact count c(x) of every canonical k-mer x:
 *     total_kmers ("Total k-mers", increments that saw 0)   = sum over x of ceil(c(x) / 256)
 *     hash_size   ("Hash size", keys that saw 255)          = #{x : c(x) >= 256}
 * distinct, max_count, the spectrum, query and dump are what the reference's getFreq declines to give for this version
 * (kmer-cnt/vertex_index.cpp:863-891).  1 <= k <= 17 as in the reference (kmer-cnt/vertex_index.cpp:793-796); fewer than 2^32 k-mer
 * positions per call.  A call with no reads, with no read longer than k, or with every read filtered returns zeros.
 * Two calls on one handle are independent; the table of the last call stays in the handle for spectrum / query / dump, which
 * return GAB_EINVAL before the first successful count.
 */
#define GAB_KMER_MAX_K 17
#define GAB_KMER_RUN 64   /* consecutive positions of a read that one GPU lane walks and merges (see gab_kmer_last_stats) */
typedef struct gab_kmer gab_kmer;
typedef struct {
    int64_t reads_kept;    /* reads with len > min_len_exclusive */
    int64_t positions;     /* sum over the kept reads of max(len - k, 0) */
    int64_t distinct, total_kmers, hash_size, max_count;
} gab_kmer_result;
int gab_kmer_create(int device, gab_kmer **out);
void gab_kmer_destroy(gab_kmer *h);
/* optional, outside the timed region: device buffers for calls of up to max_reads reads in max_seq_bytes of sequence (see gab_bsw_reserve) */
int gab_kmer_reserve(gab_kmer *h, int64_t max_reads, int64_t max_seq_bytes);
/* host pointers; a byte outside ACGTacgt in any read (kept or not) -> GAB_EINVAL, the message names the first such read */
int gab_kmer_count(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k,
                   int32_t min_len_exclusive, gab_kmer_result *res);
/* device pointers; seq_bytes = size of the slab (bounds validation: off + len <= seq_bytes).  Copies off / len to the host
 * (the tiling of the reads is planned there) and synchronises `stream` before it returns; res is a HOST pointer. */
int gab_kmer_count_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len,
                          int64_t n_reads, int k, int32_t min_len_exclusive, gab_kmer_result *res, void *stream);
/* hist[c] = number of canonical k-mers seen exactly c times, c = 1 .. nbins - 2; hist[nbins - 1] = those seen >= nbins - 1 times;
 * hist[0] = 0 (k-mers that never occur are not enumerated).  nbins >= 2, host pointer. */
int gab_kmer_spectrum(gab_kmer *h, int64_t *hist, int32_t nbins);
/* counts[i] = c(canonical form of kmers[i]) under the k of the last count, 0 if absent; a value >= 4^k -> GAB_EINVAL.  Host pointers. */
int gab_kmer_query(gab_kmer *h, const uint64_t *kmers, int64_t n, uint32_t *counts);
/* every counted canonical k-mer with its count, ascending by k-mer; *nout = their number (= distinct); when that exceeds
 * `capacity` nothing is written and the call returns GAB_ERANGE: call again with *nout of room.  Host pointers. */
int gab_kmer_dump(gab_kmer *h, uint64_t *kmers, uint32_t *counts, int64_t capacity, int64_t *nout);
/* last count: 128-byte table lines the inserts visited (>= positions - merged; the excess is lines found full), positions
 * merged into their predecessor because it had the same canonical k-mer and lay in the same lane's run (runs start at the
 * multiples of GAB_KMER_RUN within a read), device time of the count stage (table clear + extract-and-count kernel) and of the
 * whole call from the first copy of the plan to the result (HIP events, ms) */
int gab_kmer_last_stats(gab_kmer *h, int64_t *probes, int64_t *merged, float *kernel_ms, float *total_ms);
/* last count, per stage (HIP events, ms): 2-bit packing, clear + extract-and-count, the reduction over the table */
int gab_kmer_last_phases(gab_kmer *h, float *pack_ms, float *count_ms, float *reduce_ms);

/* Key-space partitions: one count split over several GPUs (or several calls) without a merge.  A hash of the canonical k-mer puts
 * it into one of nparts partitions; a call with (part, nparts) walks ALL reads and counts only the k-mers of its partition, in a
 * table sized for that share.  The partitions are disjoint, so over part = 0 .. nparts - 1 distinct, total_kmers, hash_size and the
 * spectrum add, max_count is the largest, the sorted dumps interleave, and a query is answered by exactly one partition.  No call
 * needs anything from another.  nparts = 1, part = 0 is gab_kmer_count itself. */
#define GAB_KMER_MAX_PARTS 64
/* Plain host arithmetic, no GPU needed.  The partition of a canonical k-mer, 0 .. nparts - 1 (GAB_EINVAL for nparts outside
 * 1 .. GAB_KMER_MAX_PARTS); the same for n of them; the table slots the first attempt of a partitioned call over `positions`
 * k-mer positions allocates (16 bytes each): the even share of min(positions, 4^k) keys plus a quarter plus 64, at half full, never
 * more than the unpartitioned table and that table for nparts = 1. */
int gab_kmer_part_of(uint64_t canonical_kmer, int nparts);
int gab_kmer_parts_of(const uint64_t *canonical_kmers, int64_t n, int nparts, int32_t *parts);
int64_t gab_kmer_table_slots(int64_t positions, int k, int nparts);
/* gab_kmer_count / gab_kmer_count_device for partition `part` of `nparts`.  reads_kept and positions are those of the whole call,
 * the same on every partition; distinct, total_kmers, hash_size and max_count are the partition's.  Afterwards the handle holds
 * the partition: gab_kmer_spectrum and gab_kmer_dump return its bins and its sorted k-mers, gab_kmer_query its count for a k-mer it
 * owns and 0 for any other, gab_kmer_last_stats the table lines its own inserts visited and the merges of its own k-mers (both add
 * up over the partitions).  Nothing but the hash bounds a partition's share of the keys: should the table fill up, the call
 * notices after its one synchronisation and runs once more with the unpartitioned table size, which cannot (gab_kmer_last_part).
 * part < 0, part >= nparts, nparts < 1 or nparts > GAB_KMER_MAX_PARTS -> GAB_EINVAL. */
int gab_kmer_count_part(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k,
                        int32_t min_len_exclusive, int part, int nparts, gab_kmer_result *res);
int gab_kmer_count_part_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len,
                               int64_t n_reads, int k, int32_t min_len_exclusive, int part, int nparts, gab_kmer_result *res, void *stream);
/* gab_kmer_reserve with the table of one partition of nparts */
int gab_kmer_reserve_part(gab_kmer *h, int64_t max_reads, int64_t max_seq_bytes, int nparts);
/* what the last count ran as: its partition, the slots of the table it ended in, and whether it was repeated (0 / 1) */
int gab_kmer_last_part(gab_kmer *h, int *part, int *nparts, int64_t *table_slots, int *retried);

/* ---- kmer-cnt, minimizer mode: the sketch of every read and the k-mer -> positions index (use_minimizers = 1) -------------
 * Replaces  vertexIndex.buildIndexMinimizers(1, minimizer_window)   kmer-cnt/kmer_cnt.cpp:282-287
 *           -> VertexIndex::buildIndexMinimizers                    kmer-cnt/vertex_index.cpp:394-502
 *           (the sketch: yieldMinimizers, kmer-cnt/kmer.h:206-262; the filter: filterFrequentKmers, kmer-cnt/vertex_index.cpp:178-217).
 * Reads, the length filter, the strand and the k-mer positions 0 .. L - k - 1 are those of gab_kmer_count above.
 * Sketch of one read, window w: w = 1 -> every position.  Otherwise the order key of a position is the splitmix64 finaliser
 * (kmer-cnt/kmer.h:91-98) of its canonical k-mer, and a monotone queue is walked over the positions: entries with a strictly greater
 * key leave from the back (equal ones stay); when the front's position is <= p - w the expired fronts leave and, on such a step only,
 * the front moves on to the last of a leading run of equal keys; after every step the front is emitted unless it was the last
 * position emitted.  Position 0 is always emitted and emission starts before the first full window.  The tie rule is stateful: in a
 * homopolymer the minimizers fall at 0, w, 2w, ... from the start of the run.  The result equals that sequential definition on
 * every input.
 * Index: capacity(x) = emitted minimizers, over all kept reads, with canonical k-mer x; minimizers = their sum, distinct = their
 * number; repetitive_frequency = (size_t)(repeat_kmer_rate * ((float)minimizers / (distinct + 1))) in C float arithmetic; every x
 * with capacity(x) > repetitive_frequency is removed (filtered_kmers of them, filtered_entries minimizers); every other x keeps the
 * ascending list of the global positions of its minimizers (selected_kmers lists, index_entries positions).
 * Global positions (kmer-cnt/sequence_container.cpp:48-79, 359-370): kept read i of length L_i, S_i = the lengths of the kept reads
 * before it, owns [2 S_i, 2 S_i + L_i) forward and [2 S_i + L_i, 2 S_i + 2 L_i) reverse complement; a minimizer at forward position p
 * is entered at 2 S_i + p if its forward k-mer is the canonical one (palindromes are not flipped, kmer-cnt/kmer.h:54-63), at
 * 2 S_i + L_i + (L_i - p - k) otherwise.  2 * total_len < 2^40 as in the reference, fewer than 2^32 k-mer positions per call.
 * 1 <= k <= GAB_KMER_MAX_K, 1 <= window <= GAB_KMER_MAX_WINDOW, repeat_kmer_rate >= 0 and finite; anything else -> GAB_EINVAL.
 * An index call takes the handle's table over: afterwards gab_kmer_spectrum / query / dump (and last_stats / last_phases /
 * last_part) return GAB_EINVAL until the next count, and the gab_kmer_index_* accessors return GAB_EINVAL before the first index
 * call and after any later count.  gab_kmer_sketch touches neither.  Empty input, no kept read, no read longer than k, or a rate
 * that removes every k-mer give zeros and an empty index, not an error.  Two calls on one handle are independent.
 */
#define GAB_KMER_MAX_WINDOW 255
typedef struct {
    int64_t reads_kept;             /* reads with len > min_len_exclusive */
    int64_t total_len;              /* their bases (the reference's totalLen of the forward strands) */
    int64_t minimizers, distinct;   /* the reference's totalKmers and uniqueKmers of the filter */
    int64_t repetitive_frequency;
    int64_t filtered_kmers, filtered_entries;
    int64_t selected_kmers, index_entries;
} gab_kmer_index_result;
/* The minimizer positions of every read: pos[read_start[i] .. read_start[i + 1]) ascending, read_start has n_reads + 1 entries;
 * a filtered or too-short read has an empty range.  *nout = their number; when that exceeds `capacity` neither array is written
 * and the call returns GAB_ERANGE: call again with *nout of room.  Host pointers; a byte outside ACGTacgt -> GAB_EINVAL naming
 * the read. */
int gab_kmer_sketch(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int window,
                    int32_t min_len_exclusive, int64_t *read_start, int32_t *pos, int64_t capacity, int64_t *nout);
/* seq / off / len / read_start / pos: device pointers (see gab_kmer_count_device); nout: host pointer.  Synchronises `stream`. */
int gab_kmer_sketch_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads,
                           int k, int window, int32_t min_len_exclusive, int64_t *read_start, int32_t *pos, int64_t capacity,
                           int64_t *nout, void *stream);
/* Builds the index into the handle.  Host pointers / device pointers as gab_kmer_count / gab_kmer_count_device; res: host. */
int gab_kmer_index_minimizers(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int window,
                              int32_t min_len_exclusive, float repeat_kmer_rate, gab_kmer_index_result *res);
int gab_kmer_index_minimizers_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len,
                                     int64_t n_reads, int k, int window, int32_t min_len_exclusive, float repeat_kmer_rate,
                                     gab_kmer_index_result *res, void *stream);
/* The index of the last build: kmers[0 .. *nk) ascending, the list of kmers[i] is gpos[start[i] .. start[i + 1]) ascending
 * (start has *nk + 1 entries, so it needs cap_kmers + 1 of room).  *nk = selected_kmers, *ne = index_entries; when either exceeds
 * its capacity nothing is written and the call returns GAB_ERANGE with both needed sizes.  Host pointers. */
int gab_kmer_index_dump(gab_kmer *h, uint64_t *kmers, int64_t *start, int64_t *gpos, int64_t cap_kmers, int64_t cap_entries,
                        int64_t *nk, int64_t *ne);
/* kmers[i] is canonicalised as by gab_kmer_query (a value >= 4^k -> GAB_EINVAL).  count[i] = length of its list and first[i] = where
 * the list starts in gab_kmer_index_dump's gpos; an absent k-mer: count 0, first -1; a removed (repetitive) one: count 0, first -1,
 * repetitive[i] = 1 (0 for every other).  Host pointers. */
int gab_kmer_index_lookup(gab_kmer *h, const uint64_t *kmers, int64_t n, int64_t *first, int32_t *count, uint8_t *repetitive);
/* last index build, per stage (HIP events, ms): 2-bit packing + sketch + scan; table clear + capacity pass + reduction; ordering
 * the keys, list offsets and the fill pass; the segmented sort of the lists.  The host computes repetitive_frequency between
 * the second and the third: that wait is in none of them. */
int gab_kmer_index_last_phases(gab_kmer *h, float *sketch_ms, float *count_ms, float *fill_ms, float *sort_ms);

/* The minimizer index in key-space partitions, one per GPU (or per call), in two phases.  The filter's threshold needs the number of
 * minimizers and of distinct k-mers of the WHOLE input (filterFrequentKmers, kmer-cnt/vertex_index.cpp:178-217) before any list is
 * laid out, so the partitions meet in the middle of the build -- on the host, through two integers each:
 *   1. gab_kmer_index_part_begin on every partition: it sketches ALL reads (the sketch is replicated: a split by reads would need
 *      minimizers exchanged between GPUs, and this library has no collective) and counts the capacities of the k-mers it owns
 *      (ownership: gab_kmer_part_of, the same split as gab_kmer_count_part), in a table sized for that share;
 *   2. the caller adds up `minimizers` and `distinct` of all partitions;
 *   3. gab_kmer_index_part_finish on every partition with those sums: it filters with the GLOBAL threshold, then lays out, fills and
 *      sorts the lists of its own k-mers.
 * The partitions are disjoint: their dumps, merged by k-mer, are gab_kmer_index_minimizers' index of the same input bit for bit, and
 * minimizers, distinct, filtered_kmers, filtered_entries, selected_kmers and index_entries add up to its fields.  No call needs
 * anything from another but the two sums.  nparts = 1: begin(0 of 1) and finish with its own two numbers are
 * gab_kmer_index_minimizers. */
/* (size_t)(rate * ((float)minimizers / (distinct + 1))) in the reference's C float arithmetic (kmer-cnt/vertex_index.cpp:190-191),
 * saturated as gab_kmer_index_minimizers saturates it (at INT64_MAX): the ONE place the threshold is computed, for library, driver and
 * mirror.  Plain host arithmetic, no GPU needed.  A negative count or a rate that is negative or not finite -> GAB_EINVAL. */
int64_t gab_kmer_repetitive_frequency(int64_t minimizers, int64_t distinct, float repeat_kmer_rate);
/* Phase 1 of partition `part` of `nparts`.  Arguments as gab_kmer_index_minimizers / _device and gab_kmer_count_part; synchronises.
 * res: reads_kept and total_len of the whole call, the same on every partition; minimizers and distinct of the partition's OWN
 * k-mers (over the partitions minimizers adds up to what gab_kmer_sketch emits); the other five fields are 0.  The handle is then
 * PENDING: it keeps the packed reads, the sketch and the partition's capacity table for phase 2; it is neither counted nor
 * indexed, so every gab_kmer_* accessor of a count or an index returns GAB_EINVAL, and any gab_kmer_count*, gab_kmer_sketch*,
 * gab_kmer_index_minimizers* or another begin drops the pending state.  Device form: the caller's `len` array and `stream` must
 * stay valid and unchanged until gab_kmer_index_part_finish, which runs on that stream.  The first table is a forecast of the
 * partition's share, as for gab_kmer_count_part: should it fill up, the capacity pass runs once more in the unpartitioned table
 * size (gab_kmer_index_last_part). */
int gab_kmer_index_part_begin(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k, int window,
                              int32_t min_len_exclusive, int part, int nparts, gab_kmer_index_result *res);
int gab_kmer_index_part_begin_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads,
                                     int k, int window, int32_t min_len_exclusive, int part, int nparts, gab_kmer_index_result *res, void *stream);
/* Phase 2: minimizers / distinct = the sums of phase 1 over ALL partitions; the threshold is
 * gab_kmer_repetitive_frequency(minimizers, distinct, repeat_kmer_rate).  res: reads_kept and total_len of the whole call,
 * minimizers and distinct of the partition's own k-mers, repetitive_frequency the global value (the same on every partition),
 * filtered_kmers, filtered_entries, selected_kmers and index_entries of the partition's own k-mers.  Afterwards the handle holds the
 * partition's index: gab_kmer_index_dump returns its k-mers ascending with their ascending lists, gab_kmer_index_lookup answers for a
 * k-mer it owns and returns first -1, count 0, repetitive 0 for any k-mer of another partition, gab_kmer_index_last_phases returns
 * sketch | count of phase 1 and fill | sort of phase 2.  GAB_EINVAL: no pending begin on the handle (also a second finish: the fill
 * consumed the list starts), a bad rate, totals smaller than the partition's own numbers, minimizers < distinct; a refused argument
 * leaves the handle pending. */
int gab_kmer_index_part_finish(gab_kmer *h, int64_t minimizers, int64_t distinct, float repeat_kmer_rate, gab_kmer_index_result *res);
/* what the last index build ran as (cf. gab_kmer_last_part): its partition (0 of 1 after gab_kmer_index_minimizers), the slots of the
 * capacity table it ended in, and whether the capacity pass was repeated (0 / 1) */
int gab_kmer_index_last_part(gab_kmer *h, int *part, int *nparts, int64_t *table_slots, int *retried);

/* ---- kmer-cnt, solid k-mer index: per read, the k-mers of the highest global count (buildIndexUnevenCoverage) ---------------
 * Replaces  vertexIndex.buildIndexUnevenCoverage(MIN_FREQ, rate, tandem)   kmer-cnt/kmer_cnt.cpp:228-230, 290-292 (commented out there)
 *           -> VertexIndex::buildIndexUnevenCoverage                       kmer-cnt/vertex_index.cpp:30-130
 *           (the selector: yieldFrequentKmers, kmer-cnt/vertex_index.cpp:321-363; the filter: filterFrequentKmers,
 *            kmer-cnt/vertex_index.cpp:178-217; getFreq as the exact count, which is what COUNT_VERSION 0 makes of it).
 * Reads, the length filter, the strand, the positions 0 .. L - k - 1, the canonical form and the global positions are those of
 * gab_kmer_index_minimizers; c(x) is gab_kmer_count's exact count over the kept reads.  The call counts and builds in one go.
 * Selection, per kept read with n = L - k > 0 positions and f[p] = c(canonical k-mer at p):
 *   1. cut = the element of rank (size_t)(select_rate * (float)n) (a float product, truncated; 0-based) of f in descending order;
 *      where the product reaches n the reference reads past its array and this library takes rank n - 1;
 *   2. every position with f[p] >= cut stays (ties included, so these can be far more than the rank);
 *   3. tandem_freq > 0: positions whose canonical k-mer occurs more than tandem_freq times among ALL n positions of the read go;
 *   4. positions with f[p] < min_freq go.
 * Index: capacity(x) = selected positions with canonical k-mer x (`candidates` keys, `selected_positions` in all).  The filter's
 * mean runs over the keys with capacity >= min_freq (mean_total their sum, mean_unique their number): repetitive_frequency =
 * gab_kmer_repetitive_frequency(mean_total, mean_unique, repeat_kmer_rate).  Keys with capacity > repetitive_frequency are removed
 * (filtered_kmers, filtered_entries).  Every other key stays (selected_kmers, the reference's "Selected k-mers"), with the ascending
 * global positions of its selected positions if c(x) <= repetitive_frequency and with an EMPTY list otherwise (the reference's
 * second pass skips by global count, kmer-cnt/vertex_index.cpp:78-79); indexed_kmers lists are not empty, index_entries positions.
 * Afterwards the handle holds an index: gab_kmer_index_dump returns the indexed_kmers non-empty lists, gab_kmer_index_lookup reads a
 * key with an empty list as absent and a removed one as repetitive, the count accessors return GAB_EINVAL (the reference clears its
 * counter, kmer-cnt/vertex_index.cpp:111) and a pending gab_kmer_index_part_begin is dropped.
 * Limits: those of gab_kmer_index_minimizers, min_freq >= 0, 0 <= select_rate < 1 (NaN is refused); tandem_freq <= 0 switches rule 3 off.
 * Key-space partitions are not offered: the rank of a read needs every count. */
typedef struct {
    int64_t reads_kept, total_len, positions;      /* as gab_kmer_index_result / gab_kmer_result */
    int64_t selected_positions, candidates;        /* the sum of the capacities; the keys with capacity >= 1 */
    int64_t mean_total, mean_unique;               /* the filter's totals: over capacities >= min_freq */
    int64_t repetitive_frequency;
    int64_t filtered_kmers, filtered_entries;
    int64_t selected_kmers;                        /* kept keys, empty lists included (what the reference prints) */
    int64_t indexed_kmers, index_entries;          /* the non-empty lists and their positions */
} gab_kmer_solid_result;
int gab_kmer_index_solid(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k,
                         int32_t min_len_exclusive, int min_freq, float select_rate, int tandem_freq, float repeat_kmer_rate,
                         gab_kmer_solid_result *res);
/* device pointers as gab_kmer_count_device (off / len are copied to the host first); res: host.  Synchronises `stream` between
 * its stages (the host computes the threshold) and before it returns */
int gab_kmer_index_solid_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len, int64_t n_reads,
                                int k, int32_t min_len_exclusive, int min_freq, float select_rate, int tandem_freq,
                                float repeat_kmer_rate, gab_kmer_solid_result *res, void *stream);
/* The selection alone (rules 1-4), as gab_kmer_sketch returns the minimizers: pos[read_start[i] .. read_start[i + 1]) ascending;
 * GAB_ERANGE with *nout and nothing written when `capacity` is too small.  It counts into memory of its own: a count or an index
 * in the handle stays as it is (a pending gab_kmer_index_part_begin is dropped, as by gab_kmer_sketch). */
int gab_kmer_solid_positions(gab_kmer *h, const char *seq, const int64_t *off, const int32_t *len, int64_t n_reads, int k,
                             int32_t min_len_exclusive, int min_freq, float select_rate, int tandem_freq, int64_t *read_start,
                             int32_t *pos, int64_t capacity, int64_t *nout);
/* seq / off / len / read_start / pos: device pointers, nout: host, as gab_kmer_sketch_device.  Synchronises `stream`. */
int gab_kmer_solid_positions_device(gab_kmer *h, const char *seq, int64_t seq_bytes, const int64_t *off, const int32_t *len,
                                    int64_t n_reads, int k, int32_t min_len_exclusive, int min_freq, float select_rate, int tandem_freq,
                                    int64_t *read_start, int32_t *pos, int64_t capacity, int64_t *nout, void *stream);
/* last solid build, per stage (HIP events, ms): 2-bit packing + table clear + count; frequency look-up + selection + scan; second
 * table clear + capacity pass + reduction; ordering the keys, list offsets and the fill pass; the segmented sort. */
int gab_kmer_solid_last_phases(gab_kmer *h, float *count_ms, float *select_ms, float *capacity_ms, float *fill_ms, float *sort_ms);
/* last solid build: the positions that took the multiplicity test of rule 3 (those with c(x) > tandem_freq among a read's top
 * counts; a k-mer cannot occur more often in one read than in all), and the reads whose tested k-mers outgrew the on-chip table
 * of the test and were taken in several hash classes instead (exact either way). */
int gab_kmer_solid_last_stats(gab_kmer *h, int64_t *tested_positions, int64_t *fallback_reads);

/* ---- input parsers ---------------------------------------------------------
 * The reference drivers parse their text inputs on the host, line by line, outside the region of interest
 * (bsw: loadPairs, bsw/src/main_banded.cpp:164-206 -- fgets + sscanf per pair; bpm / wfa: getline per line,
 * bpm/tools/align_benchmark.c:150-200, wfa/tools/align_benchmark.c:110-194).  At 10 M items that is the bulk of the
 * end-to-end time.  These entry points take the WHOLE file as one buffer and build the packed, device-resident
 * inputs of gab_bsw_run_device / gab_bpm_run_device / gab_wfa_run_device on the GPU: a newline index (count, scan,
 * fill), then per pair the lengths, offsets, h0 and the code bytes.
 * They accept exactly the well-formed files the reference accepts without hitting one of its buffer limits
 * (every line ends with '\n'; bsw: h0 line of at most 8 characters, reference line < 2047, query line < 255
 * characters, both non-empty) and return GAB_EINVAL otherwise -- a caller then falls back to its line-by-line parser.
 * All outputs live in memory owned by the handle and stay valid until the next call on it. */
typedef struct gab_parser gab_parser;
typedef struct {
    int64_t n;                                   /* pairs = newline count / 3 (main_banded.cpp:237-253) */
    const uint8_t *d_ref; const int64_t *d_ref_off;      /* codes (character - '0'); byte offset of each pair's sequence, 4-byte aligned */
    const uint8_t *d_qry; const int64_t *d_qry_off;
    const int32_t *d_len1, *d_len2, *d_h0;
    int64_t ref_bytes, qry_bytes;
} gab_bsw_packed;
typedef struct {
    int64_t n;                                   /* pairs = newline count / 2 */
    const char *d_text;                          /* the file itself; sequences are used in place */
    int64_t text_bytes;                          /* readable bytes of d_text (>= nbytes; the staged copy has 64 bytes of slack) */
    const int64_t *d_pat_off, *d_txt_off;        /* first base of each sequence (the '>' / '<' prefix is skipped) */
    const int32_t *d_pat_len, *d_txt_len;
    const int64_t *d_cap_off;                    /* n + 1 offsets of per-pair output slots of pattern_length + text_length bytes */
    int64_t cap_bytes;                           /* (rounded up to 4): the ops_off / buffer size gab_wfa_run_device needs */
} gab_pairs_packed;
int gab_parser_create(int device, gab_parser **out);
void gab_parser_destroy(gab_parser *p);
/* text: host pointer (copied to the device) or, for the _device variants, device pointer (16-byte aligned).  Every parse call
 * enqueues on `stream` and synchronises it several times -- after the newline count, after the scans whose totals size the
 * outputs, for chain when the header lines have come to the host -- and at the end: the outputs are complete when it returns */
int gab_bsw_parse_pairs(gab_parser *p, const char *text, int64_t nbytes, gab_bsw_packed *out, void *stream);
int gab_bsw_parse_pairs_device(gab_parser *p, const char *d_text, int64_t nbytes, gab_bsw_packed *out, void *stream);
/* swap_longer_first != 0: the longer line becomes the pattern (bpm, align_benchmark.c:177-181); 0: '>' is the pattern (wfa) */
int gab_pairs_parse(gab_parser *p, const char *text, int64_t nbytes, int swap_longer_first, gab_pairs_packed *out, void *stream);
int gab_pairs_parse_device(gab_parser *p, const char *d_text, int64_t nbytes, int swap_longer_first, gab_pairs_packed *out,
                           void *stream);
/* chain / fast-chain (chain/src/host_data_io.cpp:13-51): files in the one-record-per-line layout -- a header line
 * "n avg_qspan max_dist_x max_dist_y bw n_segs", n lines "x y", one line "EOR" -- become the inputs of
 * gab_chain_run_device: anchors on the device, the call table (offsets and headers) on the host, as that entry point
 * takes it.  The header lines are converted on the host with the reference's own fscanf format.  After the last "EOR"
 * line only white space may follow: anything else (a further call without its "EOR" line, an "EOR" without its newline)
 * is GAB_EINVAL, and the message names the index that call would have had. */
typedef struct {
    int64_t ncalls, total;                       /* calls, anchors of all calls */
    const uint64_t *d_x, *d_y;                   /* device: anchors of all calls back to back */
    const int64_t *call_off;                     /* host: ncalls + 1 offsets into d_x / d_y */
    const gab_chain_hdr *hdr;                    /* host: ncalls headers */
} gab_chain_packed;
int gab_chain_parse(gab_parser *p, const char *text, int64_t nbytes, gab_chain_packed *out, void *stream);
int gab_chain_parse_device(gab_parser *p, const char *d_text, int64_t nbytes, gab_chain_packed *out, void *stream);
/* last parse: kernel milliseconds (HIP events on the launch stream, excluding the host-to-device copy of the text) */
int gab_parser_last_stats(gab_parser *p, float *kernel_ms);

/* ---- abea: adaptive banded event alignment (f5c / nanopolish) ------------------------------------------
 * Replaces  the loop of align_db over align_single -> align()      abea/src/f5c.c:1367-1394
 *           (where the reference's own, disabled, align_cuda hook sits; semantics: align(), abea/src/align.c:169-548).
 * One call aligns a batch of reads: the events of each read against the 6-mers of its base string, Suzuki-Kasahara adaptive
 * band of 100 cells, traceback, the reference's three quality checks.  The arithmetic is the reference's built WITHOUT fused
 * multiply-add (-msse4.1 / -mavx2, the first two choices of its Makefile): fp32 emission rounded after every operation, the
 * three transition sums in double rounded to float once, per-read constants in double with libm on the host.
 * One defined deviation: when no event has the last k-mer inside its band (the end scan of align.c:418-434 finds nothing
 * finite) the reference backtracks from a cell outside the band; this library returns 0 pairs, path_len 0, end_event 0,
 * max_gap 0, avg_log_emission 0 and the flag GAB_ABEA_NO_END alone.
 * Input rules: a byte outside "ACGT" ranks as 'A' (get_rank, align.c:10-23; lower case is not mapped); seq_len >= 6 and
 * n_events >= 1, anything else is GAB_EINVAL naming the read.  The two steps before align() in the reference's timed region,
 * event detection and the scaling estimate, are gab_abea_events and gab_abea_scalings below: their outputs are what this call
 * takes; the fixed block after it, postalign, recalibrate_model and the three read checks, is gab_abea_calibrate at the end
 * of this header, and realign_read, the step after that, is gab_abea_realign behind it; the other branch of that step, the methylation HMM of
 * call-methylation, is gab_abea_meth at the very end. */
#define GAB_ABEA_K 6
#define GAB_ABEA_BANDWIDTH 100
#define GAB_ABEA_NKMER 4096
typedef struct gab_abea gab_abea;
typedef struct { int32_t ref_pos, read_pos; } gab_abea_pair;        /* AlignedPair, f5c.h:163-166: k-mer index, event index */
enum { GAB_ABEA_LOW_EMISSION = 1, GAB_ABEA_NOT_SPANNED = 2, GAB_ABEA_GAP = 4, GAB_ABEA_NO_END = 8 };
typedef struct {
    int32_t n_pairs;      /* what align() returns: 0 when a quality check failed */
    int32_t path_len;     /* pairs on the path before the checks; pairs[] holds them (in read order, as the reference leaves them) even when n_pairs = 0 */
    int32_t end_event, max_gap;
    uint32_t flags; int32_t pad;
    double avg_log_emission;
    int64_t fills;        /* cells filled, the reference's `fills` */
} gab_abea_read;
/* the pore model: GAB_ABEA_NKMER entries indexed by k-mer rank; level_log_stdv NULL = (float)log(level_stdv), model.c:53 */
int gab_abea_create(int device, const float *level_mean, const float *level_stdv, const float *level_log_stdv, gab_abea **out);
void gab_abea_destroy(gab_abea *h);
/* optional: size the handle's buffers for host calls of up to max_reads reads, max_bases bases and max_events events in all */
int gab_abea_reserve(gab_abea *h, int64_t max_reads, int64_t max_bases, int64_t max_events);
/* Host buffers.  Read i: bases seq[seq_off[i] .. +seq_len[i]), events event_mean[event_off[i] .. +n_events[i]), scalings
 * scale[i], shift[i].  Its pairs go to pairs[pair_off[i] ..]: the caller gives n_events[i] + seq_len[i] - 5 pairs of room per
 * read (the reference gives 2 * n_events and asserts), regions disjoint; res[i] is the read's record. */
int gab_abea_align(gab_abea *h, const char *seq, const int64_t *seq_off, const int32_t *seq_len,
                   const float *event_mean, const int64_t *event_off, const int32_t *n_events,
                   const float *scale, const float *shift, int64_t n_reads,
                   gab_abea_pair *pairs, const int64_t *pair_off, gab_abea_read *res);
/* Device buffers.  seq_bytes / event_count / pair_count = sizes of the three slabs (bytes, floats, pairs), for bounds
 * validation.  Synchronises `stream` twice: once at the start (the launch plan needs the lengths on the host) and once at
 * the end (the stage times of gab_abea_last_stats), so pairs and res are complete when it returns. */
int gab_abea_align_device(gab_abea *h, const char *seq, int64_t seq_bytes, const int64_t *seq_off, const int32_t *seq_len,
                          const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events,
                          const float *scale, const float *shift, int64_t n_reads,
                          gab_abea_pair *pairs, int64_t pair_count, const int64_t *pair_off, gab_abea_read *res, void *stream);
/* last call: cells filled (the sum of `fills`), bands swept, launches the call was cut into (GAB_ABEA_TRACE_BYTES: the
 * trace budget of one launch), device time of the DP kernels and of all kernels (HIP events on the stream, ms).  Any may be NULL. */
int gab_abea_last_stats(gab_abea *h, int64_t *cells, int64_t *bands, int64_t *launches, float *kernel_ms, float *total_ms);

/* ---- abea: event detection and the scaling estimate ------------------------------------------------------
 * Replaces  event_single of event_db                                abea/src/f5c.c:1241-1264
 *           = the pA conversion (f5c.c:1249-1253), getevents (abea/src/events.c:552-568) and
 *             estimate_scalings_using_mom (abea/src/align.c:49-97), per read.
 * Raw samples go in; the event table (structure of arrays) and the scalings come out in the layout gab_abea_align_device
 * takes.  Bit for bit the reference built WITHOUT fused multiply-add: prefix sums in double (the square taken in float),
 * compute_tstat for windows 3 and 6 with its mixed float / double evaluation (compiled as C++: fabs and sqrt at events.c:359
 * are the float overloads), short_long_peak_detector as written (DNA parameters), create_event in float with correctly rounded
 * sqrtf and divisions, the four sums of the scaling estimate in double in the reference's order, rounded to float once.
 * NOT built: trim_and_segment_raw -- getevents discards what it returns (events.c:562), so it has no effect on the result.
 * One defined deviation: for a read in which no peak fires the reference indexes peaks[n - 2] with n = 1, which is undefined;
 * this library returns ONE event covering [0, n_samples), mean and stdv by create_event's formulas.
 * Input rules: n_samples >= 1 (an int32_t, so below 2^31) and digitisation != 0, anything else is GAB_EINVAL naming the read;
 * n_reads = 0 returns GAB_OK and writes nothing.  Signal already in pA: range = digitisation = 1, offset = 0 (the conversion
 * (raw + offset) * (range / digitisation) in float is then the identity).
 * How it runs: a read's sums are added wide when a per-read reduction proves them exact in any order (every addend a multiple
 * of 2^q, their magnitudes summing to less than 2^(q + 53)), in the reference's order otherwise (reads_serial_sums; a tiny or
 * huge sample, a NaN, an infinity or a denormal forces it).  The detector runs every chunk of GAB_ABEA_EVENTS_CHUNK samples at
 * once from a cold state GAB_ABEA_EVENTS_WARMUP samples before it; a chunk whose assumed state at its boundary is not the state
 * the chunk before it ended in is run again from the true state (chunks_redone). */
#define GAB_ABEA_EVENTS_CHUNK 1024
#define GAB_ABEA_EVENTS_WARMUP 64
/* Host buffers.  Read i: samples raw[raw_off[i] .. +n_samples[i]), range[i], digitisation[i], offset[i].  Written: n_events[i],
 * event_off[i] (the exclusive prefix sum of n_events: read i's events sit at event_off[i], back to back), *total_events, and
 * the four slabs event_mean / event_stdv / event_start (first sample) / event_length (samples, float as the reference holds
 * it), each with room for event_cap events.  More events than event_cap: GAB_ERANGE, the slabs are not touched, n_events,
 * event_off and *total_events are complete and valid -- size the slabs and call again. */
int gab_abea_events(gab_abea *h, const float *raw, const int64_t *raw_off, const int32_t *n_samples,
                    const float *range, const float *digitisation, const float *offset, int64_t n_reads,
                    int32_t *n_events, int64_t *event_off,
                    float *event_mean, float *event_stdv, int32_t *event_start, float *event_length,
                    int64_t event_cap, int64_t *total_events);
/* Device buffers (total_events too); raw_count = floats in the raw slab, for bounds validation.  Synchronises `stream` at the
 * start (the chunk plan needs the lengths on the host), once in the middle (n_events come to the host for event_off; nothing
 * else does) and at the end.  The call needs about 40 bytes of scratch per sample on the handle. */
int gab_abea_events_device(gab_abea *h, const float *raw, int64_t raw_count, const int64_t *raw_off, const int32_t *n_samples,
                           const float *range, const float *digitisation, const float *offset, int64_t n_reads,
                           int32_t *n_events, int64_t *event_off,
                           float *event_mean, float *event_stdv, int32_t *event_start, float *event_length,
                           int64_t event_cap, int64_t *total_events, void *stream);
/* scale[i], shift[i] of read i by the method of moments, against the handle's pore model.  The k-mer rank rule is that of
 * gab_abea_align (a byte outside "ACGT" ranks as 'A'); seq_len >= 6 and n_events >= 1, anything else is GAB_EINVAL naming the
 * read.  The sums of the event means, of the k-mer levels and of the levels' squares are each added wide when the proof above
 * shows them exact in any order, and in the reference's order otherwise; the sum of the squared double differences is not exact
 * in any order and is always added in order. */
int gab_abea_scalings(gab_abea *h, const char *seq, const int64_t *seq_off, const int32_t *seq_len,
                      const float *event_mean, const int64_t *event_off, const int32_t *n_events, int64_t n_reads,
                      float *scale, float *shift);
/* Device buffers; seq_bytes / event_count = sizes of the two slabs, for bounds validation.  Complete when it returns. */
int gab_abea_scalings_device(gab_abea *h, const char *seq, int64_t seq_bytes, const int64_t *seq_off, const int32_t *seq_len,
                             const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events, int64_t n_reads,
                             float *scale, float *shift, void *stream);
/* last gab_abea_events* call: samples read, events found, reads whose sums were added in order, chunks, chunks run again,
 * device time of the kernels and of the whole call from first to last kernel (HIP events on the stream, ms).  Any may be NULL. */
int gab_abea_events_last_stats(gab_abea *h, int64_t *samples, int64_t *events, int64_t *reads_serial_sums,
                               int64_t *chunks, int64_t *chunks_redone, float *kernel_ms, float *total_ms);
/* last gab_abea_scalings* call: reads, and how many of them had the sum of their event means, of their k-mer levels and of the
 * levels' squares added in the reference's order because it could not be proved order-free.  Any may be NULL. */
int gab_abea_scalings_last_stats(gab_abea *h, int64_t *reads, int64_t *event_sums_in_order, int64_t *kmer_sums_in_order,
                                 int64_t *kmer_sq_sums_in_order);
/* the last gab_abea_events* call's kernel time by stage: proof + sums + t-statistics | detector + verification | event starts + fill */
int gab_abea_events_stage_ms(gab_abea *h, float *sums_ms, float *detect_ms, float *fill_ms);
/* GAB_ABEA_EVENTS_CHUNK and GAB_ABEA_EVENTS_WARMUP as the library was built (no GPU needed) */
int gab_abea_events_shape(int32_t *chunk, int32_t *warmup);

/* ---- abea: base-to-event map, recalibration and read checks ----------------------------------------------
 * Replaces  the block of process_single after align_single          abea/src/f5c.c:1438-1501
 *           = postalign (abea/src/align.c:550-650), recalibrate_model (align.c:655-762) and the three checks that set
 *             read_stat_flag (f5c.c:1474-1501), per read.
 * The pairs of gab_abea_align go in; the base-to-event map, events_per_base, the recalibrated scalings and the read's flag
 * come out: everything the methylation HMM and realign_read (gab_abea_realign below) take from the alignment.  Bit for bit the
 * reference built WITHOUT fused multiply-add.
 * Map (align.c:561-585): a pair counts only when its event differs from the previous pair's event; `start` is the first such
 * event of the k-mer, `stop` the last.  events_per_base = (double)(max_event - min_event) / n_kmers over all pairs.
 * Event alignment (align.c:595-646): k-mers in order, those without events skipped, one entry per event of start..stop; an
 * entry is 'M' when its k-mer's rank differs from the rank of the previous ENTRY, 'E' otherwise -- so the first entry of a
 * k-mer is 'E' when the previous k-mer that had events has the same rank, and every later entry of a k-mer is 'E'.  The
 * entries are counted (n_alignment, n_m_state), not written: nothing downstream reads them.
 * recalibrate_model runs when n_m_state >= 200: five double sums over the 'M' entries in entry order (inv_var = 1. / (stdv *
 * stdv); mu * inv_var; (mu * mu) * inv_var; e * inv_var; (mu * e) * inv_var; e the float mean of the entry's event), the 2 x 2
 * solve, a second in-order sum of (yi * yi) / (stdv * stdv) with yi = e - x0 - x1 * mu on the double x0, x1, a division by
 * n_m_state and a correctly rounded sqrt; shift, scale and var rounded to float once, log_var = (float)log(var) of the double
 * var with libm on the host.
 * Defined where the reference leaves fields unset.  n_pairs = 0: flag GAB_ABEA_FAILED_ALIGNMENT, the map all -1 / -1,
 * events_per_base 0, n_alignment 0.  Not recalibrated (that case, or fewer than 200 'M' entries): scale and shift as given,
 * var 1, log_var 0 (what align()'s emission assumes, align.c:128,138).
 * Flags, at most one, in the reference's order: not recalibrated or (double)var > 2.5 (MIN_CALIBRATION_VAR, f5cmisc.h:9) ->
 * GAB_ABEA_FAILED_CALIBRATION; otherwise events_per_base > 5.0 -> GAB_ABEA_FAILED_QUALITY_CHK.  A NaN var (a pore model
 * whose normal equations are singular) fails neither comparison.
 * Input rules: seq_len >= 6 and n_events >= 1; 0 <= n_pairs[i] <= n_events[i] + seq_len[i] - 5; every pair has 0 <= ref_pos <
 * n_kmers and 0 <= read_pos < n_events, both non-decreasing along the list (what align() emits).  Anything else is GAB_EINVAL
 * naming the read, and nothing is written.  The k-mer rank rule is that of gab_abea_align.  n_reads = 0 returns GAB_OK and
 * writes nothing. */
enum { GAB_ABEA_FAILED_CALIBRATION = 1, GAB_ABEA_FAILED_ALIGNMENT = 2, GAB_ABEA_FAILED_QUALITY_CHK = 4 };      /* f5c.h:49-51 */
typedef struct { int32_t start, stop; } gab_abea_range;      /* index_pair_t, f5c.h:169-172: stop inclusive; -1 / -1 = no event */
typedef struct {
    int32_t n_alignment;      /* what postalign returns */
    int32_t n_m_state;        /* entries with hmm_state 'M' */
    uint32_t read_stat_flag;  /* at most one bit: the reference returns at the first failed check */
    int32_t recalibrated;     /* recalibrate_model's return */
    float scale, shift, var, log_var;
    double events_per_base;
} gab_abea_calib;
/* Host buffers.  seq*, event*, scale, shift, pairs and pair_off are the buffers of gab_abea_align; n_pairs[i] is res[i].n_pairs
 * of the alignment.  Read i's map, seq_len[i] - 5 entries, goes to map[map_off[i] ..]; res[i] is its record. */
int gab_abea_calibrate(gab_abea *h, const char *seq, const int64_t *seq_off, const int32_t *seq_len,
                       const float *event_mean, const int64_t *event_off, const int32_t *n_events,
                       const float *scale, const float *shift,
                       const gab_abea_pair *pairs, const int64_t *pair_off, const int32_t *n_pairs, int64_t n_reads,
                       gab_abea_range *map, const int64_t *map_off, gab_abea_calib *res);
/* Device buffers.  seq_bytes / event_count / pair_count / map_count = sizes of the four slabs (bytes, floats, pairs, map
 * entries), for bounds validation.  Three kernels, and a fourth that stores log_var.  Synchronises `stream` at the start (the
 * lengths are validated on the host), after the first kernel (it checks every pair and writes nothing but a verdict: a broken
 * rule returns GAB_EINVAL here) and at the end (the double var comes to the host for log_var). */
int gab_abea_calibrate_device(gab_abea *h, const char *seq, int64_t seq_bytes, const int64_t *seq_off, const int32_t *seq_len,
                              const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events,
                              const float *scale, const float *shift,
                              const gab_abea_pair *pairs, int64_t pair_count, const int64_t *pair_off, const int32_t *n_pairs, int64_t n_reads,
                              gab_abea_range *map, int64_t map_count, const int64_t *map_off, gab_abea_calib *res, void *stream);
/* last gab_abea_calibrate* call: reads, reads recalibrated, 'M' entries of all reads, device time of the check, map and fit
 * kernels and of the whole call from first to last kernel, the host's turns between them included (HIP events on the stream,
 * ms).  Any may be NULL. */
int gab_abea_calibrate_last_stats(gab_abea *h, int64_t *reads, int64_t *recalibrated, int64_t *m_states, float *kernel_ms, float *total_ms);

/* ---- abea: realign_read, the event alignment records of eventalign ------------------------------------------
 * Replaces  realign_read of process_single                          abea/src/f5c.c:1508-1515
 *           = align_read_to_ref (abea/src/eventalign.c:1263-1540) around profile_hmm_align (eventalign.c:703-911), per read.
 * The reference substring, position, strand and CIGAR of a read's BAM record and what gab_abea_calibrate wrote go in; the event
 * alignment records come out, the rows of events.tsv whose reference_kmer and model_kmer columns the suite's check compares
 * (abea/scripts/regression_small.sh:78-88).  Bit for bit the reference built WITHOUT fused multiply-add.
 * Which reads run: those with calib[i].read_stat_flag == 0 (f5c.c:1474-1501 return before realign_read otherwise); the others
 * get 0 entries and the flag GAB_ABEA_REALIGN_SKIPPED.
 * Reference string (eventalign.c:1294-1301): upper-cased, IUPAC codes replaced by their first base (disambiguate, :1091-1109),
 * and its reverse complement.  CIGAR (get_aligned_segments_two_params, :1112-1179): M = X emit pairs, D advances the reference,
 * I and S the read, H nothing, N closes a segment and opens the next.  Per segment the region trim (:932-943, when region_start
 * and region_end are not -1) and the trim to read positions <= seq_len - 6 (:947-957); an empty segment ends the read (:1335-1337,
 * GAB_ABEA_REALIGN_NO_PAIRS).  Then the loop of :1373-1534: get_end_pair 100 reference bases on, the three breaks (fewer than 12
 * bases, a stop event less than 2 from the start event, nothing emitted), the Viterbi fill of profile_hmm_fill_generic_r9
 * (:345-610, hmm_flags 0, CACHED_LOG emission, update_cell's comparisons as written, :621-633) and the backtrack from (last row,
 * last k-mer, MATCH); of its entries the first 50 that are not K states and not the start event's, or all of them in the last
 * section, are emitted, and the next section starts at the last one.  Not built: summarize_alignment (--summary only), the SAM
 * writer, the numeric columns of the TSV.
 * The transitions are per-read constants in float from calib[i].events_per_base (calculate_transitions, :171-240), their
 * logarithms taken on the host with libm, as log_var is.
 * Records: ref_kmer and model_kmer are not stored because they follow from a record.  ref_kmer is the six bases of the prepared
 * (upper-cased, disambiguated) reference at ref_position (:1474).  model_kmer (:1486-1503) is "NNNNNN" for a 'B'; otherwise, forward,
 * fwd_subseq.substr(kmer_idx, 6) = the same six bases, and, reverse, rc_subseq.substr(len - kmer_idx - 6, 6) with rc_subseq the
 * reverse complement of fwd_subseq, which is the reverse complement of those six bases.
 * Room: read i's entries go to out[out_off[i] ..], n_events[i] * (1 + its number of N operations) entries of room, regions
 * disjoint.  That is enough: a section never emits its start event (:1468) and its events lie strictly on one side of it, the
 * next section starts at the last event emitted, and the loop runs towards last_event only, so within one BAM segment every event
 * is emitted at most once; each N operation opens one more segment.  Less room is GAB_EINVAL.
 * Input rules: seq_len >= 6; n_events >= 1; every reference byte valid for isValid after toupper (ACGT and the IUPAC codes
 * MRWSYKVHDBN, either case); CIGAR operations in MIDNSH=X; the CIGAR's reference span <= ref_len and its read span <= seq_len;
 * event means, scale, shift, var and log_var finite, var > 0; map entries -1 or inside [0, n_events).  Anything else is
 * GAB_EINVAL naming the read, and nothing is written.  n_reads = 0 returns GAB_OK and writes nothing.
 * Defined where the reference has undefined behaviour or aborts: get_closest_event_to returns -1 for the first, last or stop
 * event (the reference indexes event[-1]) -> GAB_ABEA_REALIGN_NO_EVENT; the event stride disagrees with the strand (the assert of
 * :363) -> GAB_ABEA_REALIGN_STRAND.  The read ends there with the entries it has.  Everything else is the reference's, also
 * events_per_base <= 1, where p_stay <= 0 makes transitions -inf or NaN and update_cell's comparisons decide.
 * How it runs: one wavefront per read, two k-mer blocks per lane, the backpointers in a trace of GAB_ABEA_REALIGN_ROWS rows per
 * wavefront; a read that meets a section of more rows stops there and is finished by a second launch (reads_requeued). */
#define GAB_ABEA_REALIGN_ROWS 512
typedef struct { int32_t ref_position, event_idx; uint8_t hmm_state /* 'M' or 'B' */, pad[3]; } gab_abea_ealn;
enum { GAB_ABEA_REALIGN_SKIPPED = 1,   /* calib[i].read_stat_flag != 0: the reference never calls realign_read */
       GAB_ABEA_REALIGN_NO_PAIRS = 2,  /* a segment was empty after the trims: the reference returns what it has */
       GAB_ABEA_REALIGN_NO_EVENT = 4,  /* defined deviation, above */
       GAB_ABEA_REALIGN_STRAND = 8 };  /* defined deviation, above */
typedef struct {
    int32_t n_entries;     /* records written at out[out_off[i] ..] */
    int32_t hmm_segments;  /* calls of profile_hmm_align */
    int32_t max_rows;      /* events of the longest of them */
    uint32_t flags;
    int64_t cells;         /* events x k-mers over them */
} gab_abea_realign_read;
/* Host buffers.  Read i: the reference bases ref[ref_off[i] .. +ref_len[i]) of [ref_pos[i], ref_pos[i] + ref_len[i]) (what the
 * reference's fasta_cache holds), is_rev[i] (bam_is_rev), its CIGAR cigar[cigar_off[i] .. +n_cigar[i]) in BAM encoding (len << 4 |
 * op), seq_len[i] (read_length), its event means, its map at map[map_off[i] ..] and calib[i] exactly as gab_abea_calibrate wrote
 * them.  region_start = region_end = -1: no region (the driver's default). */
int gab_abea_realign(gab_abea *h, const char *ref, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_pos,
                     const uint8_t *is_rev, const uint32_t *cigar, const int64_t *cigar_off, const int32_t *n_cigar,
                     const int32_t *seq_len, const float *event_mean, const int64_t *event_off, const int32_t *n_events,
                     const gab_abea_range *map, const int64_t *map_off, const gab_abea_calib *calib,
                     int32_t region_start, int32_t region_end, int64_t n_reads,
                     gab_abea_ealn *out, const int64_t *out_off, gab_abea_realign_read *res);
/* Device buffers.  ref_bytes / cigar_count / event_count / map_count / out_count = sizes of the five slabs (bytes, operations,
 * floats, map entries, records), for bounds validation.  Synchronises `stream` at the start (lengths, offsets, calibration
 * records and CIGARs come to the host and are validated there; the CIGARs' run-length tables go back), after the first launch
 * (the requeue decision, and the verdict of the checks that ran on the device: a broken rule returns GAB_EINVAL here, and the
 * kernels have written nothing), once per requeue batch if there is one, and at the end, so out and res are complete when it
 * returns. */
int gab_abea_realign_device(gab_abea *h, const char *ref, int64_t ref_bytes, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_pos,
                            const uint8_t *is_rev, const uint32_t *cigar, int64_t cigar_count, const int64_t *cigar_off, const int32_t *n_cigar,
                            const int32_t *seq_len, const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events,
                            const gab_abea_range *map, int64_t map_count, const int64_t *map_off, const gab_abea_calib *calib,
                            int32_t region_start, int32_t region_end, int64_t n_reads,
                            gab_abea_ealn *out, int64_t out_count, const int64_t *out_off, gab_abea_realign_read *res, void *stream);
/* last gab_abea_realign* call: reads, calls of profile_hmm_align, their rows (events) and cells (events x k-mers), reads finished
 * by the second launch, device time of the kernels and of the whole call from first to last kernel, the host's turn between the
 * launches included (HIP events on the stream, ms).  Any may be NULL. */
int gab_abea_realign_last_stats(gab_abea *h, int64_t *reads, int64_t *hmm_segments, int64_t *rows, int64_t *cells,
                                int64_t *reads_requeued, float *kernel_ms, float *total_ms);
/* the last gab_abea_realign* call's time by stage: preparation | first launch | requeue */
int gab_abea_realign_stage_ms(gab_abea *h, float *prep_ms, float *viterbi_ms, float *requeue_ms);
/* GAB_ABEA_REALIGN_ROWS as the library was built (no GPU needed) */
int gab_abea_realign_shape(int32_t *rows_cap);

/* ---- abea: call-methylation, the log-likelihoods of every CpG group of a read --------------------------------
 * Replaces  calculate_methylation_for_read of meth_single             abea/src/f5c.c:1397-1411
 *           = abea/src/meth.c:501-658 around profile_hmm_score (abea/src/hmm.c:620-674), per read.
 * It takes what gab_abea_realign takes, without the region: the reference substring, position, strand and CIGAR of a read's BAM
 * record, its event means, and the map and calibration record that gab_abea_calibrate wrote.  Per scored CpG group one site
 * record comes out, with the two floats that the reference prints (f5c.c:1730-1754).  Bit for bit the reference built WITHOUT
 * fused multiply-add and with ESL_LOG_SUM 1 (abea/src/f5c.h:70): add_logs is the table-driven p7_FLogsum (abea/src/logsum.h:61-71).
 * Which reads run: those with calib[i].read_stat_flag == 0; the others get no sites and GAB_ABEA_METH_SKIPPED.
 * Reference string: upper-cased, IUPAC codes replaced by their first base (disambiguate, meth.c:288-306), as for realign.
 * Groups (meth.c:532-558): every i with ref[i] == 'C' and ref[i + 1] == 'G' is a site; consecutive sites at most 10 apart form a
 * group (first, last, n_cpg).  Per group (meth.c:560-603): sub_start = first - 10, sub_end = last + 10; skipped when
 * sub_start <= 10 (skipped_start) or last - first > 200 (skipped_span); the sub-sequence is ref[sub_start .. sub_end], cut at the
 * end of the string as substr cuts it.
 * Event alignment record (meth.c:124-185), one per read: the CIGAR walk of get_aligned_segments (meth.c:15-87; M = X emit pairs, D
 * advances the reference, I and S the read, H nothing), the pairs with read_pos < 6 or read_pos + 6 >= seq_len dropped, the k-mer
 * index flipped for a reverse read, the event of a pair by get_closest_event_to as written (meth.c:92-117: its loops leave their
 * stop index out); the record is emptied when its first and last event are equal.
 * Bounds (find_by_ref_bounds, meth.c:422-467): the two lower bounds of sub_start + ref_pos and sub_end + ref_pos among the pairs'
 * reference positions and the left / right tests as written; not bounded -> skipped_unbounded.  Then (meth.c:597-603) the group
 * is skipped when abs(e2 - e1) <= 10 (skipped_short).  The third test there, ratio > MAX_EVENT_TO_BP_RATIO, divides by
 * calling_start - calling_end, which is negative: the ratio is never positive and the test never fires; it is not built.
 * Scores: profile_hmm_score on the sub-sequence and its reverse complement, and on methylate() of it (meth.c:359-382: every
 * complete CG becomes MG) and reverse_complement_meth of that (meth.c:387-420), with hmm_flags = PRE_CLIP | POST_CLIP,
 * event_stride = e1 <= e2 ? 1 : -1 and rc = is_rev.  The fill is hmm.c:305-524 with the forward output of hmm.c:549-600:
 * |e2 - e1| + 1 rows, strlen - 5 k-mers ranked base 5 over A C G M T (hmm.c:21-52; of m_rc_seq + len - ki - 6 for rc, hmm.c:382-393),
 * the CACHED_LOG emission (hmm.c:55-100), the six scores of a state folded left to right by p7_FLogsum in the order written with
 * the emission added last (hmm.c:558-566), KMER_SKIP reading the same row of the previous block (hmm.c:468-474), and lp_end folding
 * M, B and K of the last k-mer of every row in row order (hmm.c:479-487).  HMM_REVERSE_FIX is not defined.
 * Host-side constants: the ten transition logarithms per read (hmm.c:231-298) as for realign; the flanks (hmm.c:132-205), one
 * table for both because post_flank read from its end is pre_flank expression for expression, doubles stored as floats; the
 * 16000-entry table of p7_FLogsumInit (logsum.h:35-48).  All with the host's libm.
 * Sites of a read are written in ascending start_position (the order in which the reference's std::map iterates), n_sites of
 * them at out[out_off[i] ..].  Room: gab_abea_meth_groups()[i] records (one per CpG group of the read, scored or not), regions
 * disjoint.  Less room is GAB_EINVAL.  A read that is not run (GAB_ABEA_METH_SKIPPED) needs no room: its groups are not counted
 * and its record says groups = 0.
 * Input rules: those of gab_abea_realign, and a CIGAR that holds an N operation is GAB_EINVAL naming the read (the reference
 * exits on spliced alignments, meth.c:54-58).  On GAB_EINVAL nothing is written.  n_reads = 0 returns GAB_OK.  Before
 * gab_abea_set_cpg_model the calls return GAB_EINVAL.
 * Defined where the reference has undefined behaviour or asserts; the group is not scored and the read is flagged:
 * e1 or e2 is -1 (the reference indexes event -1) -> GAB_ABEA_METH_NO_EVENT (checked after the bounds, before the short test);
 * the stride disagrees with the strand (the assert of hmm.c:322) -> GAB_ABEA_METH_STRAND; events_per_base < 1 (or no number),
 * where the transition logarithms are NaN and the table index undefined -> GAB_ABEA_METH_TRANSITIONS, no group of the read is
 * scored (groups is still counted).
 * How it runs: one wavefront per read prepares it (codes of the reference, groups, bounds, the work list); one wavefront per
 * group scores both variants, one k-mer block per lane for groups of up to GAB_ABEA_METH_ONE_BLOCK_KMERS k-mers and
 * GAB_ABEA_METH_BLOCKS_PER_LANE for wider ones, the lanes one row apart from each other so that every fold meets its operands in
 * the reference's order.  No trace, so no row cap. */
#define GAB_ABEA_METH_NKMER 15625
#define GAB_ABEA_METH_LOGSUM 16000
#define GAB_ABEA_METH_BLOCKS_PER_LANE 4
#define GAB_ABEA_METH_ONE_BLOCK_KMERS 64      /* groups of up to this many k-mers run with one block per lane */
typedef struct { int32_t start_position, end_position, n_cpg, first_cpg /* index into the read's reference substring */, event_start, event_stop;
                 float ll_unmethylated, ll_methylated; } gab_abea_site;
enum { GAB_ABEA_METH_SKIPPED = 1,       /* calib[i].read_stat_flag != 0: the reference never scores the read */
       GAB_ABEA_METH_NO_EVENT = 2,      /* defined deviation, above */
       GAB_ABEA_METH_STRAND = 4,        /* defined deviation, above */
       GAB_ABEA_METH_TRANSITIONS = 8 }; /* defined deviation, above */
typedef struct {
    int32_t n_sites;       /* records written at out[out_off[i] ..] */
    int32_t groups;        /* CpG groups of the prepared reference */
    int32_t skipped_start, skipped_span, skipped_unbounded, skipped_short;
    uint32_t flags;
    int32_t pad;
    int64_t cells;         /* rows x k-mers over the scored groups, both variants */
} gab_abea_meth_read;
/* the CpG model: 15625 entries each (k-mers over A C G M T, base 5), copied to the device.  The first call on a handle also builds its
 * logsum table (p7_FLogsumInit), once; a later call replaces the model only. */
int gab_abea_set_cpg_model(gab_abea *h, const float *level_mean, const float *level_stdv, const float *level_log_stdv);
/* No GPU needed.  groups[i] = CpG groups of read i's prepared reference: the room read i needs at out[out_off[i] ..]. */
int gab_abea_meth_groups(const char *ref, const int64_t *ref_off, const int32_t *ref_len, int64_t n_reads, int32_t *groups);
/* No GPU needed.  The 16000 floats of p7_FLogsumInit as the library builds them. */
int gab_abea_meth_logsum(float *table16000);
/* GAB_ABEA_METH_BLOCKS_PER_LANE and GAB_ABEA_METH_ONE_BLOCK_KMERS as the library was built (no GPU needed).  Either may be NULL. */
int gab_abea_meth_shape(int32_t *blocks_per_lane, int32_t *one_block_kmers);
/* Host buffers, as gab_abea_realign. */
int gab_abea_meth(gab_abea *h, const char *ref, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_pos,
                  const uint8_t *is_rev, const uint32_t *cigar, const int64_t *cigar_off, const int32_t *n_cigar,
                  const int32_t *seq_len, const float *event_mean, const int64_t *event_off, const int32_t *n_events,
                  const gab_abea_range *map, const int64_t *map_off, const gab_abea_calib *calib, int64_t n_reads,
                  gab_abea_site *out, const int64_t *out_off, gab_abea_meth_read *res);
/* Device buffers, with the sizes of the five slabs for bounds validation; a read's room is what lies between its out_off and the
 * next larger one (or out_count).  Synchronises `stream` at the start (lengths, offsets, calibration records and CIGARs come to
 * the host and are validated there; the CIGARs' run tables go back) and at the end (the verdict of the checks that ran on the
 * device, the reference bytes, event means, map entries and the room among them: a broken rule returns GAB_EINVAL here and the
 * kernels have written nothing; and the per-read records for the statistics), so out and res are complete when it returns.
 * A call whose longest read has more events than that of any call before it on the handle synchronises once more in between: the
 * flank table is made longer and uploaded then. */
int gab_abea_meth_device(gab_abea *h, const char *ref, int64_t ref_bytes, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_pos,
                         const uint8_t *is_rev, const uint32_t *cigar, int64_t cigar_count, const int64_t *cigar_off, const int32_t *n_cigar,
                         const int32_t *seq_len, const float *event_mean, int64_t event_count, const int64_t *event_off, const int32_t *n_events,
                         const gab_abea_range *map, int64_t map_count, const int64_t *map_off, const gab_abea_calib *calib, int64_t n_reads,
                         gab_abea_site *out, int64_t out_count, const int64_t *out_off, gab_abea_meth_read *res, void *stream);
/* last gab_abea_meth* call: reads, CpG groups, sites scored, their rows (events) and cells (rows x k-mers, both variants), device
 * time of the kernels and of the whole call from first to last kernel (HIP events on the stream, ms).  Any may be NULL. */
int gab_abea_meth_last_stats(gab_abea *h, int64_t *reads, int64_t *groups, int64_t *sites, int64_t *rows, int64_t *cells, float *kernel_ms, float *total_ms);
/* the last gab_abea_meth* call's time by stage: preparation | scoring */
int gab_abea_meth_stage_ms(gab_abea *h, float *prep_ms, float *score_ms);

/* ---- dbg: the de Bruijn graph of Platypus' local assembly, one graph per assembly region ------------------------------
 * Replaces  assembleReadsAndDetectVariants(...) once per region, the OpenMP loop of dbg/src/debruijn.cpp:1646-1661, which with the
 *           cycle search commented out (:1437-1457) is
 *           createDeBruijnGraph                                          dbg/src/debruijn.cpp:846-861
 *           loadReferenceIntoGraph                                       dbg/src/debruijn.cpp:1291-1317
 *           loadBAMDataIntoGraph -> loadReadIntoGraph                    dbg/src/debruijn.cpp:1399-1414, 1351-1396
 *           -> DeBruijnGraph_AddEdge -> NodeDict_FindOrInsert            dbg/src/debruijn.cpp:917-949, 759-843
 *           and what the verbose line prints of the graph (printDeBruijnGraph, dbg/src/debruijn.cpp:881-889, 1458-1465).
 * The BAM and FASTA reading (htslib) is outside the reference's timed region and stays with the caller: INTEGRATION.md.
 *
 * For one region, with k-mer size k (the reference's 15) and min_qual (its 20); everything is an integer:
 *   reference   for i in 0 .. ref_len - k - 2: an edge from the k-mer at i to the k-mer at i + 1, colour 1 (REF), positions ref_start + i
 *               and ref_start + i + 1, node weight 1 each, edge weight 1.  Every byte counts, N included.
 *   reads       read_begin .. read_end - 1 in order, without those whose flag has bit 512 (QC fail).  For i in 0 .. len - k - 2: q = the lowest
 *               quality of the k + 1 bases i .. i + k; if q >= min_qual and none of them is N, an edge from the k-mer at i to the one at i + 1,
 *               colour 2 (READ), position -1, node weight q on both, edge weight q.  Every other letter is an ordinary letter.
 *   an edge     finds or inserts its start node, then its end node (twice the same node for a homopolymer: its weight counts twice); a
 *               found node gets colours |=, weight +=, and keeps the position and source of its first occurrence.  Then the first of the start
 *               node's four slots that is empty or already leads to the end node takes the edge (weight +=); with four other successors
 *               present the edge is dropped, the nodes having been updated.
 * Nodes come out in the order of their first occurrence (the reference's allNodes), a node's edges in the order of theirs.  The reference's
 * hash function and buckets show nowhere.  Its weights are doubles that only ever hold sums of integers; here they are int64.
 *
 * Input, n_regions regions over one reference slab and one read slab: region r has the reference bytes ref[ref_off[r] .. + ref_len[r])
 * (slices may overlap, as neighbouring regions' do), ref_start[r], and the reads read_begin[r] .. read_end[r] - 1 (the reference's
 * windowStart / windowEnd: one read belongs to two or three regions); read j has seq and qual bytes at read_off[j] .. + read_len[j] of
 * their slabs and read_flag[j].  Qualities are any byte.
 * Output: node_off[n_regions + 1] and the records nodes[node_off[r] .. node_off[r + 1]) of region r.  src_read / src_off say where the
 * node's k-mer first stood (src_read -1: the region's reference; else the read's index in the call), which is the reference's `sequence`
 * pointer: its verbose line is "%d %d " of ref_start twice and, per node, the rest of that reference slice or read from src_off on.
 * edge_to is a node index within the region; unused slots hold -1 and weight 0.
 * Capacity as for gab_kmer_dump: when the graphs hold more than `capacity` nodes nothing is written, *nout gets the need and the call
 * returns GAB_ERANGE; gab_dbg_room gives an upper bound from lengths alone (a sequence with e > 0 edges has at most e + 1 k-mers).
 * Limits: 1 <= k <= GAB_DBG_MAX_K (sixteen letters of 4 bits: a k-mer is one 64-bit key; the one key that is all ones has a slot of its
 * own, so every value is a valid k-mer).  A byte that is none of =ACMGRSVTWYHKDBN in a region's reference slice or in one of its reads
 * (QC-fail ones included) is GAB_EINVAL naming the first such region, and nothing is written; lower case is such a byte: the reference
 * compares bytes, so a soft-masked reference never matches a read there, and upper-casing is the caller's decision.
 * A region may offer at most GAB_DBG_MAX_OCCURRENCES edge occurrences (reference and unfiltered reads together), else GAB_EINVAL: an
 * occurrence's two node indices 2t and 2t + 1 are kept in 32 bits, which alone would admit 2^31; the bound is 2^24 so that one region's
 * tables stay below 2 GiB.  Weights are summed in 64 bits: at most 2 x 255 x 2^24 per node.
 * How it runs: one work-group per region, the region's tables in global memory (DESIGN.md says why not LDS); every occurrence has its
 * index in the reference's order and a table entry keeps the lowest index it saw, so the result does not depend on the order in which
 * the atomics land.  Scratch is about 60 bytes per edge occurrence offered, all regions of a call at once: callers with more regions
 * than memory call in slices. */
#define GAB_DBG_MAX_K 16
#define GAB_DBG_MAX_OCCURRENCES (1 << 24)
#define GAB_DBG_REGION_SIZE 1500        /* assemblyRegionSize, dbg/src/debruijn.cpp:1576 */
typedef struct gab_dbg gab_dbg;
typedef struct { int32_t k, min_qual; } gab_dbg_params;
typedef struct {
    int32_t src_read, src_off;          /* first occurrence: -1 = the region's reference, else the read; the offset of the k-mer there */
    int32_t colours;                    /* 1 REF, 2 READ, 3 both */
    int32_t position;                   /* ref_start + src_off, or -1 for a node first seen in a read */
    int64_t weight;
    int32_t n_edges, edge_to[4], pad;
    int64_t edge_weight[4];
} gab_dbg_node;                          /* 80 bytes */
typedef struct { int64_t regions, occurrences /* offered */, passed /* the filter */, nodes, edges, probes /* node-table slots the inserts looked at */;
                 float kernel_ms, total_ms; } gab_dbg_stats;
typedef struct { int32_t start, ref_start, ref_len, pad; int64_t read_begin, read_end; } gab_dbg_region;
int gab_dbg_create(int device, gab_dbg **out);
void gab_dbg_destroy(gab_dbg *h);
/* optional: scratch for calls of up to this many regions, reads and edge occurrences offered, so that no call allocates */
int gab_dbg_reserve(gab_dbg *h, int64_t max_regions, int64_t max_reads, int64_t max_occurrences);
/* No GPU needed.  The nodes the regions can have at most (the sum; per_region, may be NULL, gets each region's), or a negative GAB_E* code. */
int64_t gab_dbg_room(const int32_t *ref_len, const int32_t *read_len, const int32_t *read_flag, const int64_t *read_begin, const int64_t *read_end,
                     int64_t n_reads, int64_t n_regions, int k, int64_t *per_region);
/* Host buffers. */
int gab_dbg_build(gab_dbg *h, const gab_dbg_params *params, const char *ref, const int64_t *ref_off, const int32_t *ref_len, const int32_t *ref_start,
                  const char *seq, const uint8_t *qual, const int64_t *read_off, const int32_t *read_len, const int32_t *read_flag, int64_t n_reads,
                  const int64_t *read_begin, const int64_t *read_end, int64_t n_regions, int64_t *node_off, gab_dbg_node *nodes, int64_t capacity, int64_t *nout);
/* Device buffers (params and nout on the host), with the sizes of the two slabs for bounds validation.  Synchronises `stream` three
 * times: at the start (offsets, lengths, flags and read ranges come to the host, are validated there and sized into the scratch
 * layout), after the graphs are built and counted (the verdict on the bytes, the node counts: GAB_EINVAL and GAB_ERANGE return here and
 * nothing of the caller's has been written) and at the end (the statistics), so node_off and nodes are complete when it returns. */
int gab_dbg_build_device(gab_dbg *h, const gab_dbg_params *params, const char *ref, int64_t ref_bytes, const int64_t *ref_off, const int32_t *ref_len,
                         const int32_t *ref_start, const char *seq, const uint8_t *qual, int64_t seq_bytes, const int64_t *read_off, const int32_t *read_len,
                         const int32_t *read_flag, int64_t n_reads, const int64_t *read_begin, const int64_t *read_end, int64_t n_regions,
                         int64_t *node_off, gab_dbg_node *nodes, int64_t capacity, int64_t *nout, void *stream);
/* last gab_dbg_build* call; the times are HIP events on the stream (ms): the kernels, and first to last kernel (the host's sizing of
 * the output in between included).  probes depends on which of two k-mers claimed a contested slot first: it is no part of the result. */
int gab_dbg_last_stats(gab_dbg *h, gab_dbg_stats *out);
/* the last call's kernel time by phase: tables cleared and filled | nodes numbered | records written.  Any may be NULL. */
int gab_dbg_last_phases(gab_dbg *h, float *insert_ms, float *number_ms, float *emit_ms);
/* No GPU needed.  The batch loop of the reference's main (dbg/src/debruijn.cpp:1576-1592) over [beg, end) of a contig of contig_len
 * bases: a region every max(100, min(1000, 1500 / 2)) bases, its reference span [max(0, start - 1500), min(start + 1500, end) + 1500)
 * cut at the contig's end as faidx_fetch_seq cuts it, and its reads by setWindowPointers / bisectReadsLeft (dbg/src/common.cpp:161-227)
 * from pos[] (ascending, soft clips subtracted as getRead does) and read_end[].  Capacity as above: *nout regions are needed. */
int gab_dbg_plan_regions(int32_t beg, int32_t end, const int32_t *pos, const int32_t *read_end, int64_t n_reads, int32_t contig_len,
                         gab_dbg_region *out, int64_t capacity, int64_t *nout);

#ifdef __cplusplus
}
#endif
#endif /* GAB_H */
