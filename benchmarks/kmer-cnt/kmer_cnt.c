/* kmer-cnt -- drop-in driver of the kmer-cnt benchmark (Flye's solid k-mer counter) on MI355X.
 *
 *     kmer-cnt --reads a.fasta[,b.fastq.gz,...] --config F [--kmer K] [--min-read N] [--min-ovlp N] [--threads T] [--log F] [--debug]
 *              [-g N | --gpus N] [--index-gpus N] [--solid-index]
 *
 * Options, the "Hash size: N" / "Total k-mers N" debug lines and the "Kernel time: %.3f sec" line on stderr are those of the
 * reference's driver (kmer-cnt/kmer_cnt.cpp:47-125, 155-337; the two counts: kmer-cnt/vertex_index.cpp:858-859).  --threads only
 * shaped the CPU scheduling and is accepted and ignored.  -g N / --gpus N (default $GAB_GPUS, else 1): N GPUs, each counting one
 * of N partitions of the KEY space (include/gab.h: gab_kmer_count_part) -- every GPU walks all reads and inserts only the k-mers
 * whose hash falls into its partition, so the partial results are disjoint: the two printed numbers add, and no GPU talks to
 * another.
 *
 * Outside the region of interest, as in the reference: the config file (key = value lines, '#' comments, "%include other.cfg"
 * relative to the including file, kmer-cnt/config.h:36-72; seven keys are read, see kc_key_names), then every reads file
 * in the order given, FASTA (multi-line) or FASTQ by its suffix, plain or gzip (kmer-cnt/sequence_container.cpp:22-46, 159-308).
 * A byte that is not one of ACGTacgt: the reference means to replace it by "ACGT"[rand() % 4] (validateSequence,
 * kmer-cnt/sequence_container.cpp:318-328), but its test compares a size_t table entry of -1 with -1U, which never holds where
 * size_t has 64 bits (and kmer-cnt/kmer.h:14 asserts that it has), so nothing is replaced and rand() is never called.  The 2-bit
 * packing then ORs that all-ones entry, shifted to the base's place, into the record's 32-base word
 * (kmer-cnt/sequence.h:54-69): the unknown base AND every base after it up to the end of that word read as T.  This driver does
 * the same to the record's text (positions counted from the start of the record, its lines joined), which is what makes its
 * numbers equal the reference's on reads with N.  Reads LONGER than max(--min-read, --min-ovlp) are kept
 * (kmer-cnt/kmer_cnt.cpp:205, kmer-cnt/sequence_container.cpp:100-106).
 * use_minimizers = 1 in the config file selects the minimizer index instead of the count (build_minimizer_index below); it also needs
 * minimizer_window, repeat_kmer_rate and assemble_kmer_sample there, and runs on the first GPU whatever -g says -- unless
 * --index-gpus N (1..GAB_KMER_MAX_PARTS) asks for the index in N key-space partitions, one per GPU, built in two phases
 * (build_minimizer_index_parts below; include/gab.h: gab_kmer_index_part_begin / _finish).  In counting mode --index-gpus is accepted
 * and ignored.
 * --solid-index (not an option of the reference; counting mode only): after the count, the solid k-mer index the reference's driver
 * carries commented out right behind countKmers() (kmer-cnt/kmer_cnt.cpp:228-230, 290-292), with its MIN_FREQ = 2 and
 * meta_read_top_kmer_rate, meta_read_filter_kmer_freq and repeat_kmer_rate from the config file (build_solid_index below).
 * Inside it: ONE gab_kmer_count_part per GPU over the kept reads, all at once (that GPU's copy of the reads included), where the
 * reference runs vertexIndex.countKmers() (kmer-cnt/kmer_cnt.cpp:282-294).  -g 1 is one gab_kmer_count_part(0 of 1) = gab_kmer_count.
 */
#define GAB_ENERGY_STREAM stderr      /* where the reference prints "Energy consumption:" in this driver */
#include "../common/gab_driver.h"
#include <getopt.h>
#include <time.h>
#include <zlib.h>

static int g_debug = 0;
static FILE *g_log = NULL;

/* Logger::debug (kmer-cnt/logger.h:82-96): "[YYYY-MM-DD HH:MM:SS] DEBUG: text" on stderr with --debug, always into the --log file */
static void log_debug(const char *fmt, ...) {
    char stamp[64], text[1024];
    time_t t = time(NULL);
    strftime(stamp, sizeof stamp, "[%Y-%m-%d %H:%M:%S]", localtime(&t));
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    if (g_debug) fprintf(stderr, "%s DEBUG: %s\n", stamp, text);
    if (g_log) fprintf(g_log, "%s DEBUG: %s\n", stamp, text);
}
static void die(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "ERROR: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(EXIT_FAILURE);
}

/* ---- config ---------------------------------------------------------------------------------------------------------------------- */
/* the keys this driver reads; values are floats, as the reference's Config keeps them (kmer-cnt/config.h:69, 100) */
enum { KC_KMER_SIZE, KC_USE_MINIMIZERS, KC_MINIMIZER_WINDOW, KC_REPEAT_KMER_RATE, KC_ASSEMBLE_KMER_SAMPLE, KC_META_TOP_KMER_RATE, KC_META_FILTER_KMER_FREQ,
       KC_NKEYS };
static const char *const kc_key_names[KC_NKEYS] = {"kmer_size", "use_minimizers", "minimizer_window", "repeat_kmer_rate", "assemble_kmer_sample",
                                                   "meta_read_top_kmer_rate", "meta_read_filter_kmer_freq"};
typedef struct { int have[KC_NKEYS]; float value[KC_NKEYS]; } kc_config;
static char *trim(char *s) {
    while (*s == ' ' || *s == '\t' || *s == '\r' || *s == '\n') s++;
    char *e = s + strlen(s);
    while (e > s && (e[-1] == ' ' || e[-1] == '\t' || e[-1] == '\r' || e[-1] == '\n')) *--e = 0;
    return s;
}
static void config_load(const char *path, kc_config *cfg, int depth) {
    if (depth > 16) die("config files include each other more than 16 deep: %s", path);
    FILE *f = fopen(path, "r");
    if (!f) die("Can't open config file: %s", path);
    log_debug("Loading %s", path);
    const char *slash = strrchr(path, '/');
    const size_t dirlen = slash ? (size_t)(slash - path) + 1 : 0;
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        char *s = line;
        s[strcspn(s, "\r\n")] = 0;
        if (!*s || *s == '#') continue;
        if (strncmp(s, "%include", 8) == 0) {
            char *name = trim(s + 8);
            if (!*name) die("Error parsing config file %s: %%include without a file name", path);
            char *sub = (char *)malloc(dirlen + strlen(name) + 1);
            memcpy(sub, path, dirlen);
            strcpy(sub + dirlen, name);
            config_load(sub, cfg, depth + 1);
            free(sub);
            continue;
        }
        char *eq = strchr(s, '=');
        if (!eq || strchr(eq + 1, '=')) die("Error parsing config file %s: '%s'", path, s);
        *eq = 0;
        const char *key = trim(s), *val = trim(eq + 1);
        log_debug("\t%s=%s", key, val);
        for (int i = 0; i < KC_NKEYS; i++)
            if (strcmp(key, kc_key_names[i]) == 0) { cfg->value[i] = (float)atof(val); cfg->have[i] = 1; }
    }
    fclose(f);
}

/* ---- reads ----------------------------------------------------------------------------------------------------------------------- */
typedef struct { char *seq; size_t bytes, cap; int64_t *off; int32_t *len; int64_t n, ncap, seen; } kc_reads;
typedef struct { char *p; size_t n, cap; } kc_buf;
static void buf_add(kc_buf *b, const char *s, size_t n) {
    if (b->n + n + 1 > b->cap) {
        b->cap = (b->n + n + 1) * 2 + 4096;
        b->p = (char *)realloc(b->p, b->cap);
        if (!b->p) die("out of memory");
    }
    memcpy(b->p + b->n, s, n);
    b->n += n;
    b->p[b->n] = 0;
}
static inline int is_base(unsigned char c) { c &= 0xDF; return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
/* what the reference's packing makes of a byte outside ACGTacgt (see the head of this file): T from there to the end of the
 * record's 32-base word */
static void unknown_to_t(char *s, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!is_base((unsigned char)s[i])) {
            size_t e = (i / 32 + 1) * 32;
            if (e > n) e = n;
            memset(s + i, 'T', e - i);
            i = e - 1;
        }
}
static void record_done(kc_reads *R, char *s, size_t n, int64_t min_len) {
    R->seen++;
    unknown_to_t(s, n);
    if ((int64_t)n <= min_len) return;
    if (n > (size_t)INT32_MAX) die("a read of %zu bases: longer than this driver takes", n);
    if (R->bytes + n > R->cap) {
        R->cap = (R->bytes + n) * 2 + (1 << 20);
        R->seq = (char *)realloc(R->seq, R->cap);
        if (!R->seq) die("out of memory");
    }
    if (R->n == R->ncap) {
        R->ncap = R->ncap * 2 + 1024;
        R->off = (int64_t *)realloc(R->off, (size_t)R->ncap * sizeof(int64_t));
        R->len = (int32_t *)realloc(R->len, (size_t)R->ncap * sizeof(int32_t));
        if (!R->off || !R->len) die("out of memory");
    }
    memcpy(R->seq + R->bytes, s, n);
    R->off[R->n] = (int64_t)R->bytes; R->len[R->n] = (int32_t)n;
    R->bytes += n; R->n++;
}
/* one line without its "\n" / "\r\n" into *line; returns 0 at the end of the file */
static int next_line(gzFile f, char *chunk, int chunk_bytes, kc_buf *line) {
    line->n = 0;
    if (line->p) line->p[0] = 0;
    int got = 0;
    while (gzgets(f, chunk, chunk_bytes)) {
        got = 1;
        const size_t n = strlen(chunk);
        buf_add(line, chunk, n);
        if (n && chunk[n - 1] == '\n') { line->p[--line->n] = 0; break; }
    }
    if (got && line->n && line->p[line->n - 1] == '\r') line->p[--line->n] = 0;
    return got;
}
static int is_fasta(const char *name) {
    char base[4096];
    snprintf(base, sizeof base, "%s", name);
    size_t n = strlen(base);
    if (n > 3 && strcmp(base + n - 3, ".gz") == 0) base[n - 3] = 0;
    const char *dot = strrchr(base, '.');
    if (dot && (strcmp(dot + 1, "fasta") == 0 || strcmp(dot + 1, "fa") == 0)) return 1;
    if (dot && (strcmp(dot + 1, "fastq") == 0 || strcmp(dot + 1, "fq") == 0)) return 0;
    die("Can't identify input file type: %s", name);
    return 0;
}
static void load_file(const char *name, kc_reads *R, int64_t min_len) {
    const int fasta = is_fasta(name);
    gzFile f = gzopen(name, "rb");
    if (!f) die("Can't open reads file %s", name);
    gzbuffer(f, 1 << 20);
    const int chunk_bytes = 1 << 20;
    char *chunk = (char *)malloc((size_t)chunk_bytes);
    kc_buf line = {0, 0, 0}, seq = {0, 0, 0};
    int have_header = 0, state = 0;
    long line_no = 1;
    while (next_line(f, chunk, chunk_bytes, &line)) {
        if (fasta) {
            if (line.n == 0) continue;
            if (line.p[0] == '>') {
                if (have_header) {
                    if (seq.n == 0) die("parse error in %s on line %ld: empty sequence", name, line_no);
                    record_done(R, seq.p, seq.n, min_len);
                    seq.n = 0;
                }
                if (line.n < 2 || line.p[1] == ' ' || line.p[1] == '\t') die("parse error in %s on line %ld: empty header", name, line_no);
                have_header = 1;
            } else {
                buf_add(&seq, line.p, line.n);
            }
        } else {
            if (line.n == 0) { state = (state + 1) % 4; continue; }      /* (the reference steps its state on an empty line too) */
            if (state == 0) {
                if (line.p[0] != '@') die("parse error in %s on line %ld: Fastq format error", name, line_no);
                if (line.n < 2 || line.p[1] == ' ' || line.p[1] == '\t') die("parse error in %s on line %ld: empty header", name, line_no);
            } else if (state == 1) {
                record_done(R, line.p, line.n, min_len);
            } else if (state == 2 && line.p[0] != '+') die("parse error in %s on line %ld: Fastq format error", name, line_no);
            state = (state + 1) % 4;
        }
        line_no++;
    }
    if (fasta) {
        if (seq.n == 0) die("parse error in %s on line %ld: empty sequence", name, line_no);
        if (!have_header) die("parse error in %s on line %ld: Fasta format error", name, line_no);
        record_done(R, seq.p, seq.n, min_len);
    }
    gzclose(f);
    free(chunk); free(line.p); free(seq.p);
}

static void usage(void) {
    fprintf(stderr, "Usage: kmer-cnt  --reads path --config path [--kmer size] [--min-read length] [--min-ovlp size]\n"
                    "\t\t[--threads num] [--log path] [--debug] [-g num | --gpus num] [--index-gpus num] [--solid-index] [-h]\n\n"
                    "Required arguments:\n"
                    "  --reads path\tcomma-separated list of read files (FASTA / FASTQ, plain or gzip)\n"
                    "  --config path\tpath to the config file\n\n"
                    "Optional arguments:\n"
                    "  --kmer size\tk-mer size, 1..%d [default = kmer_size of the config file]\n"
                    "  --min-ovlp size\tminimum overlap between reads [default = 5000]\n"
                    "  --min-read length\treads not longer than max(this, --min-ovlp) are dropped [default = 0]\n"
                    "  --debug \t\tenable debug output [default = false]\n"
                    "  --log log_file\toutput log to file [default = not set]\n"
                    "  --threads num_threads\taccepted and ignored (the count runs on the GPUs)\n"
                    "  -g, --gpus num\tGPUs to count on, each one partition of the k-mers [default = $GAB_GPUS, else 1]\n"
                    "  --index-gpus num\tuse_minimizers = 1: GPUs to build the index on, each one partition of the k-mers, 1..%d\n"
                    "\t\t\t[default = not set: the index is built on the first GPU, not partitioned]\n"
                    "  --solid-index\tafter the count, build the solid k-mer index (meta_read_top_kmer_rate,\n"
                    "\t\t\tmeta_read_filter_kmer_freq and repeat_kmer_rate of the config file) [default = false]\n", GAB_KMER_MAX_K, GAB_KMER_MAX_PARTS);
}

/* one partition per logical GPU, run by gab_run_parts */
typedef struct {
    gab_kmer **h; gab_kmer_result *res; int *rc; char (*err)[512];
    const kc_reads *R; int kmer, nparts; int32_t min_len;
} kc_parts;
static void count_part(int g, void *arg) {
    kc_parts *P = (kc_parts *)arg;
    P->rc[g] = gab_kmer_count_part(P->h[g], P->R->seq, P->R->off, P->R->len, P->R->n, P->kmer, P->min_len, g, P->nparts, &P->res[g]);
    if (P->rc[g]) snprintf(P->err[g], sizeof P->err[g], "%s", gab_last_error());      /* (the message is the calling thread's) */
}

/* use_minimizers = 1: ONE gab_kmer_index_minimizers over the kept reads where the reference runs
 * vertexIndex.buildIndexMinimizers(1, minimizer_window) (kmer-cnt/kmer_cnt.cpp:282-287), and its debug lines in its order
 * (kmer-cnt/vertex_index.cpp:190-216, 481, 494-500): the floats are computed with the reference's float expressions and written as
 * its ostream writes them (%g).  Without --index-gpus the index stays on the first GPU: its filter needs the number of minimizers
 * and of distinct k-mers of the WHOLE input before any list is laid out, so key-space partitions have to meet in the middle of the
 * build (build_minimizer_index_parts below does that). */
static int build_minimizer_index(const kc_reads *R, int kmer, int window, float rate, int32_t min_len, int ngpus) {
    if (ngpus > 1) log_debug("The minimizer index is built on the first of the %d GPUs (it is not partitioned)", ngpus);
    gab_kmer *h = NULL;
    GAB_DIE_IF(gab_kmer_create(gab_phys_gpu(0), &h), "gab_kmer_create");
    GAB_DIE_IF(gab_kmer_reserve(h, R->n, (int64_t)R->bytes), "gab_kmer_reserve");
    if (R->bytes) gab_pin(R->seq, R->bytes);
    gab_kmer_index_result x;
    memset(&x, 0, sizeof x);

    const double t0 = gab_now();
    gab_roi_begin_n(1);
    GAB_DIE_IF(gab_kmer_index_minimizers(h, R->seq, R->off, R->len, R->n, kmer, window, min_len, rate, &x), "gab_kmer_index_minimizers");
    const float mean = (float)(size_t)x.minimizers / ((size_t)x.distinct + 1);
    const float filtered_rate = (float)(size_t)x.filtered_entries / (size_t)x.minimizers;
    log_debug("Mean k-mer frequency: %g", (double)mean);
    log_debug("Repetitive k-mer frequency: %lld", (long long)x.repetitive_frequency);
    log_debug("Filtered %lld repetitive k-mers (%g)", (long long)x.filtered_entries, (double)filtered_rate);
    log_debug("Sorting k-mer index");
    log_debug("Selected k-mers: %lld", (long long)x.selected_kmers);
    log_debug("K-mer index size: %lld", (long long)x.index_entries);
    log_debug("Mean k-mer frequency: %g", (double)((float)(size_t)x.index_entries / (size_t)x.selected_kmers));
    log_debug("Minimizer rate: %g", (double)((float)(size_t)x.total_len / (size_t)x.index_entries));
    gab_roi_end();
    const double t1 = gab_now();

    float ms[4] = {0, 0, 0, 0};
    (void)gab_kmer_index_last_phases(h, &ms[0], &ms[1], &ms[2], &ms[3]);
    log_debug("Minimizers: %lld of %lld reads, %lld distinct k-mers, %lld removed; device: sketch %.3f ms, count %.3f ms, fill %.3f ms, sort %.3f ms",
              (long long)x.minimizers, (long long)x.reads_kept, (long long)x.distinct, (long long)x.filtered_kmers, ms[0], ms[1], ms[2], ms[3]);
    fprintf(stderr, "Kernel time: %.3f sec\n", t1 - t0);
    if (R->bytes) gab_unpin(R->seq);
    gab_kmer_destroy(h);
    return 0;
}

/* use_minimizers = 1 with --index-gpus N: the same index in N key-space partitions, one per logical GPU.  The filter's threshold
 * needs the minimizers and the distinct k-mers of the WHOLE input, so the partitions meet in the middle: one round of
 * gab_kmer_index_part_begin on every GPU (each sketches all reads and counts the capacities of its own k-mers), the two sums on the
 * host, one round of gab_kmer_index_part_finish with them.  Every count of the partitions adds up to the unpartitioned build's, so
 * the reference's lines are printed from the sums with the float expressions of build_minimizer_index above. */
typedef struct {
    gab_kmer **h; gab_kmer_index_result *res; int *rc; char (*err)[512];
    const kc_reads *R; int kmer, window, nparts; int32_t min_len;
    int64_t minimizers, distinct; float rate;        /* phase 2: the sums over all partitions */
} kc_index_parts;
static void index_part_begin(int g, void *arg) {
    kc_index_parts *P = (kc_index_parts *)arg;
    P->rc[g] = gab_kmer_index_part_begin(P->h[g], P->R->seq, P->R->off, P->R->len, P->R->n, P->kmer, P->window, P->min_len, g, P->nparts, &P->res[g]);
    if (P->rc[g]) snprintf(P->err[g], sizeof P->err[g], "%s", gab_last_error());      /* (the message is the calling thread's) */
}
static void index_part_finish(int g, void *arg) {
    kc_index_parts *P = (kc_index_parts *)arg;
    P->rc[g] = gab_kmer_index_part_finish(P->h[g], P->minimizers, P->distinct, P->rate, &P->res[g]);
    if (P->rc[g]) snprintf(P->err[g], sizeof P->err[g], "%s", gab_last_error());
}
static void index_parts_check(const kc_index_parts *P, const char *what) {
    for (int g = 0; g < P->nparts; g++)
        if (P->rc[g]) { fprintf(stderr, "ERROR: %s failed on partition %d (%d): %s\n", what, g, P->rc[g], P->err[g]); exit(EXIT_FAILURE); }
}
static int build_minimizer_index_parts(const kc_reads *R, int kmer, int window, float rate, int32_t min_len, int ngpus) {
    log_debug("Building the minimizer index on %d GPU(s), one key-space partition each", ngpus);
    gab_kmer **hs = (gab_kmer **)calloc((size_t)ngpus, sizeof *hs);
    gab_kmer_index_result *part_res = (gab_kmer_index_result *)calloc((size_t)ngpus, sizeof *part_res);
    int *part_rc = (int *)calloc((size_t)ngpus, sizeof *part_rc);
    char (*part_err)[512] = (char (*)[512])calloc((size_t)ngpus, 512);
    if (!hs || !part_res || !part_rc || !part_err) die("out of memory");
    for (int g = 0; g < ngpus; g++) {                                                  /* buffers before the region of interest */
        GAB_DIE_IF(gab_kmer_create(gab_phys_gpu(g), &hs[g]), "gab_kmer_create");
        GAB_DIE_IF(gab_kmer_reserve_part(hs[g], R->n, (int64_t)R->bytes, ngpus), "gab_kmer_reserve_part");
    }
    if (R->bytes) gab_pin(R->seq, R->bytes);
    kc_index_parts P = {hs, part_res, part_rc, part_err, R, kmer, window, ngpus, min_len, 0, 0, rate};
    gab_kmer_index_result x;
    memset(&x, 0, sizeof x);

    const double t0 = gab_now();
    gab_roi_begin_n(ngpus);
    if (ngpus == 1) index_part_begin(0, &P);
    else gab_run_parts(ngpus, index_part_begin, &P);
    index_parts_check(&P, "gab_kmer_index_part_begin");
    for (int g = 0; g < ngpus; g++) { P.minimizers += part_res[g].minimizers; P.distinct += part_res[g].distinct; }
    if (ngpus == 1) index_part_finish(0, &P);
    else gab_run_parts(ngpus, index_part_finish, &P);
    index_parts_check(&P, "gab_kmer_index_part_finish");
    x.reads_kept = part_res[0].reads_kept; x.total_len = part_res[0].total_len; x.repetitive_frequency = part_res[0].repetitive_frequency;
    for (int g = 0; g < ngpus; g++) {                                                  /* disjoint partitions of the keys: the counts add */
        x.minimizers += part_res[g].minimizers; x.distinct += part_res[g].distinct;
        x.filtered_kmers += part_res[g].filtered_kmers; x.filtered_entries += part_res[g].filtered_entries;
        x.selected_kmers += part_res[g].selected_kmers; x.index_entries += part_res[g].index_entries;
    }
    const float mean = (float)(size_t)x.minimizers / ((size_t)x.distinct + 1);
    const float filtered_rate = (float)(size_t)x.filtered_entries / (size_t)x.minimizers;
    log_debug("Mean k-mer frequency: %g", (double)mean);
    log_debug("Repetitive k-mer frequency: %lld", (long long)x.repetitive_frequency);
    log_debug("Filtered %lld repetitive k-mers (%g)", (long long)x.filtered_entries, (double)filtered_rate);
    log_debug("Sorting k-mer index");
    log_debug("Selected k-mers: %lld", (long long)x.selected_kmers);
    log_debug("K-mer index size: %lld", (long long)x.index_entries);
    log_debug("Mean k-mer frequency: %g", (double)((float)(size_t)x.index_entries / (size_t)x.selected_kmers));
    log_debug("Minimizer rate: %g", (double)((float)(size_t)x.total_len / (size_t)x.index_entries));
    gab_roi_end();
    const double t1 = gab_now();

    log_debug("Minimizers: %lld of %lld reads, %lld distinct k-mers, %lld removed", (long long)x.minimizers, (long long)x.reads_kept, (long long)x.distinct,
              (long long)x.filtered_kmers);
    for (int g = 0; g < ngpus; g++) {
        float ms[4] = {0, 0, 0, 0};
        int retried = 0;
        (void)gab_kmer_index_last_phases(hs[g], &ms[0], &ms[1], &ms[2], &ms[3]);
        (void)gab_kmer_index_last_part(hs[g], NULL, NULL, NULL, &retried);
        log_debug("Partition %d of %d: %lld minimizers of %lld distinct k-mers, %lld removed; device: sketch %.3f ms, count %.3f ms, fill %.3f ms, sort %.3f ms%s",
                  g, ngpus, (long long)part_res[g].minimizers, (long long)part_res[g].distinct, (long long)part_res[g].filtered_kmers, ms[0], ms[1], ms[2], ms[3],
                  retried ? "; its first table filled and the capacities were counted again in a larger one" : "");
    }
    fprintf(stderr, "Kernel time: %.3f sec\n", t1 - t0);
    if (R->bytes) gab_unpin(R->seq);
    for (int g = 0; g < ngpus; g++) gab_kmer_destroy(hs[g]);
    free(hs); free(part_res); free(part_rc); free(part_err);
    return 0;
}

/* --solid-index: ONE gab_kmer_index_solid over the kept reads, on a handle of its own on the first GPU, where the reference's driver
 * has vertexIndex.buildIndexUnevenCoverage(MIN_FREQ, SELECT_RATE, TANDEM_FREQ) commented out (kmer-cnt/kmer_cnt.cpp:290-292), and
 * that function's debug lines in its order (kmer-cnt/vertex_index.cpp:209-216, 113, 126-129), the floats with its float expressions.
 * The call counts for itself: the rank of a read needs every count, so it does not use the partitions of the count before it. */
static void build_solid_index(gab_kmer *h, const kc_reads *R, int kmer, int32_t min_len, float select_rate, int tandem_freq, float rate) {
    const int MIN_FREQ = 2;                                                              /* kmer-cnt/kmer_cnt.cpp:228 */
    gab_kmer_solid_result x;
    memset(&x, 0, sizeof x);
    GAB_DIE_IF(gab_kmer_index_solid(h, R->seq, R->off, R->len, R->n, kmer, min_len, MIN_FREQ, select_rate, tandem_freq, rate, &x), "gab_kmer_index_solid");
    log_debug("Mean k-mer frequency: %g", (double)((float)(size_t)x.mean_total / ((size_t)x.mean_unique + 1)));
    log_debug("Repetitive k-mer frequency: %lld", (long long)x.repetitive_frequency);
    log_debug("Filtered %lld repetitive k-mers (%g)", (long long)x.filtered_entries, (double)((float)(size_t)x.filtered_entries / (size_t)x.mean_total));
    log_debug("Sorting k-mer index");
    log_debug("Selected k-mers: %lld", (long long)x.selected_kmers);
    log_debug("Index size: %lld", (long long)x.index_entries);
    log_debug("Mean k-mer index frequency: %g", (double)((float)(size_t)x.index_entries / (size_t)x.selected_kmers));
    float ms[5] = {0, 0, 0, 0, 0};
    int64_t tested = 0, fallback = 0;
    (void)gab_kmer_solid_last_phases(h, &ms[0], &ms[1], &ms[2], &ms[3], &ms[4]);
    (void)gab_kmer_solid_last_stats(h, &tested, &fallback);
    log_debug("Solid index: %lld of %lld positions selected, %lld candidate k-mers, %lld removed, %lld lists not empty; %lld positions took the tandem test "
              "(%lld reads in hash classes); device: count %.3f ms, select %.3f ms, capacity %.3f ms, fill %.3f ms, sort %.3f ms",
              (long long)x.selected_positions, (long long)x.positions, (long long)x.candidates, (long long)x.filtered_kmers, (long long)x.indexed_kmers,
              (long long)tested, (long long)fallback, ms[0], ms[1], ms[2], ms[3], ms[4]);
}

int main(int argc, char **argv) {
    int kmer = -1, min_read = 0, min_ovlp = 5000, threads = 1, gpus_flag = 0, index_gpus = 0, solid_index = 0, c, idx = 0;
    const char *reads = NULL, *config = NULL, *logfile = NULL;
    static struct option lo[] = {{"reads", required_argument, 0, 0}, {"config", required_argument, 0, 0}, {"min-read", required_argument, 0, 0},
                                 {"log", required_argument, 0, 0}, {"threads", required_argument, 0, 0}, {"kmer", required_argument, 0, 0},
                                 {"min-ovlp", required_argument, 0, 0}, {"debug", no_argument, 0, 0}, {"gpus", required_argument, 0, 'g'},
                                 {"index-gpus", required_argument, 0, 0}, {"solid-index", no_argument, 0, 0}, {0, 0, 0, 0}};
    while ((c = getopt_long(argc, argv, "hg:", lo, &idx)) != -1) {
        if (c == 'h') { usage(); return 0; }
        if (c == 'g') { gpus_flag = atoi(optarg); if (gpus_flag < 1) { usage(); return 1; } continue; }
        if (c != 0) { usage(); return 1; }
        const char *name = lo[idx].name;
        if (!strcmp(name, "kmer")) kmer = atoi(optarg);
        else if (!strcmp(name, "min-read")) min_read = atoi(optarg);
        else if (!strcmp(name, "threads")) threads = atoi(optarg);
        else if (!strcmp(name, "min-ovlp")) min_ovlp = atoi(optarg);
        else if (!strcmp(name, "log")) logfile = optarg;
        else if (!strcmp(name, "debug")) g_debug = 1;
        else if (!strcmp(name, "reads")) reads = optarg;
        else if (!strcmp(name, "config")) config = optarg;
        else if (!strcmp(name, "solid-index")) solid_index = 1;
        else if (!strcmp(name, "index-gpus")) { index_gpus = atoi(optarg); if (index_gpus < 1 || index_gpus > GAB_KMER_MAX_PARTS) { usage(); return 1; } }
    }
    (void)threads;
    if (!reads || !*reads || !config || !*config) { usage(); return 1; }
    if (logfile && !(g_log = fopen(logfile, "a"))) die("Can't open log file %s", logfile);

    kc_config cfg;
    memset(&cfg, 0, sizeof cfg);
    config_load(config, &cfg, 0);
    if (kmer == -1) {
        if (!cfg.have[KC_KMER_SIZE]) die("No such parameter: kmer_size (give --kmer or set it in %s)", config);
        kmer = (int)cfg.value[KC_KMER_SIZE];
    }
    /* use_minimizers != 0: the minimizer index.  The reference then reads assemble_kmer_sample before the region of interest,
     * minimizer_window and repeat_kmer_rate inside it (kmer-cnt/kmer_cnt.cpp:216-217, 282-286, kmer-cnt/vertex_index.cpp:433) and
     * throws "No such parameter: KEY" for a missing one (kmer-cnt/config.h:74-82); here all three are asked for before any work. */
    const int use_minimizers = cfg.have[KC_USE_MINIMIZERS] && cfg.value[KC_USE_MINIMIZERS] != 0.0f;
    int window = 0;
    if (use_minimizers) {
        for (int i = KC_MINIMIZER_WINDOW; i <= KC_ASSEMBLE_KMER_SAMPLE; i++)
            if (!cfg.have[i]) die("No such parameter: %s (use_minimizers = 1 needs it; set it in %s)", kc_key_names[i], config);
        window = (int)cfg.value[KC_MINIMIZER_WINDOW];                                  /* const int minWnd = Config::get(...) */
        if (window < 1 || window > GAB_KMER_MAX_WINDOW) die("wrong minimizer length (minimizer_window = %d; supported 1..%d)", window, GAB_KMER_MAX_WINDOW);
    }
    if (solid_index && !use_minimizers) {                                              /* (the reference's Config::get throws for a missing key) */
        const int need[3] = {KC_META_TOP_KMER_RATE, KC_META_FILTER_KMER_FREQ, KC_REPEAT_KMER_RATE};
        for (int i = 0; i < 3; i++)
            if (!cfg.have[need[i]]) die("No such parameter: %s (--solid-index needs it; set it in %s)", kc_key_names[need[i]], config);
        const float top = cfg.value[KC_META_TOP_KMER_RATE];
        if (!(top >= 0.0f && top < 1.0f)) die("meta_read_top_kmer_rate = %g: --solid-index takes 0 <= rate < 1", (double)top);
    }
    if (kmer < 1 || kmer > GAB_KMER_MAX_K) die("Can't use flat counter for k-mer size > %d (k = %d; supported 1..%d)", GAB_KMER_MAX_K, kmer, GAB_KMER_MAX_K);
    log_debug("Running with k-mer size: %d", kmer);

    const int64_t min_len = min_read > min_ovlp ? min_read : min_ovlp;
    kc_reads R;
    memset(&R, 0, sizeof R);
    fprintf(stderr, "Reading sequences\n");
    char *list = strdup(reads);
    for (char *tok = list, *next; tok; tok = next) {       /* (the reference splits on ',' and keeps empty names: they fail to open) */
        next = strchr(tok, ',');
        if (next) *next++ = 0;
        load_file(tok, &R, min_len);
    }
    free(list);
    log_debug("Reads: %lld of %lld records kept, %zu bases", (long long)R.n, (long long)R.seen, R.bytes);

    int ngpus = gab_pick_gpus(gpus_flag);
    if (ngpus > GAB_KMER_MAX_PARTS) ngpus = GAB_KMER_MAX_PARTS;
    if (use_minimizers) {
        const int32_t min_len32 = (int32_t)(min_len > INT32_MAX ? INT32_MAX : min_len);
        int rc;
        if (index_gpus) {                                   /* (clamped to the cards there are, as -g is, unless GAB_GPU_OVERSUBSCRIBE) */
            int n = gab_pick_gpus(index_gpus);
            if (n > GAB_KMER_MAX_PARTS) n = GAB_KMER_MAX_PARTS;
            rc = build_minimizer_index_parts(&R, kmer, window, cfg.value[KC_REPEAT_KMER_RATE], min_len32, n);
        } else rc = build_minimizer_index(&R, kmer, window, cfg.value[KC_REPEAT_KMER_RATE], min_len32, ngpus);
        free(R.seq); free(R.off); free(R.len);
        if (solid_index) log_debug("--solid-index is ignored: use_minimizers is set, the index built is the minimizer index");
        if (g_log) fclose(g_log);
        return rc;
    }
    if (index_gpus) log_debug("--index-gpus %d is ignored: use_minimizers is not set, there is no index to build", index_gpus);
    log_debug("Counting on %d GPU(s), one key-space partition each", ngpus);
    gab_kmer **hs = (gab_kmer **)calloc((size_t)ngpus, sizeof *hs);
    gab_kmer_result *part_res = (gab_kmer_result *)calloc((size_t)ngpus, sizeof *part_res);
    int *part_rc = (int *)calloc((size_t)ngpus, sizeof *part_rc);
    char (*part_err)[512] = (char (*)[512])calloc((size_t)ngpus, 512);
    if (!hs || !part_res || !part_rc || !part_err) die("out of memory");
    for (int g = 0; g < ngpus; g++) {                                                  /* buffers before the region of interest */
        GAB_DIE_IF(gab_kmer_create(gab_phys_gpu(g), &hs[g]), "gab_kmer_create");
        GAB_DIE_IF(gab_kmer_reserve_part(hs[g], R.n, (int64_t)R.bytes, ngpus), "gab_kmer_reserve_part");
    }
    gab_kmer *solid = NULL;
    if (solid_index) GAB_DIE_IF(gab_kmer_create(gab_phys_gpu(0), &solid), "gab_kmer_create");
    if (R.bytes) gab_pin(R.seq, R.bytes);
    kc_parts P = {hs, part_res, part_rc, part_err, &R, kmer, ngpus, (int32_t)(min_len > INT32_MAX ? INT32_MAX : min_len)};
    gab_kmer_result res;
    memset(&res, 0, sizeof res);

    const double t0 = gab_now();
    gab_roi_begin_n(ngpus);
    if (ngpus == 1) count_part(0, &P);
    else gab_run_parts(ngpus, count_part, &P);
    for (int g = 0; g < ngpus; g++) {
        if (part_rc[g]) { fprintf(stderr, "ERROR: gab_kmer_count_part failed (%d): %s\n", part_rc[g], part_err[g]); exit(EXIT_FAILURE); }
        /* disjoint partitions of the keys: the counts add, the largest count is the largest of them */
        res.reads_kept = part_res[g].reads_kept; res.positions = part_res[g].positions;
        res.distinct += part_res[g].distinct; res.total_kmers += part_res[g].total_kmers; res.hash_size += part_res[g].hash_size;
        if (part_res[g].max_count > res.max_count) res.max_count = part_res[g].max_count;
    }
    log_debug("Hash size: %lld", (long long)res.hash_size);
    log_debug("Total k-mers %lld", (long long)res.total_kmers);
    if (solid)
        build_solid_index(solid, &R, kmer, P.min_len, cfg.value[KC_META_TOP_KMER_RATE], (int)cfg.value[KC_META_FILTER_KMER_FREQ], cfg.value[KC_REPEAT_KMER_RATE]);
    gab_roi_end();
    const double t1 = gab_now();

    float kernel_ms = 0, total_ms = 0;                                                  /* the slowest partition's */
    int retried = 0;
    for (int g = 0; g < ngpus; g++) {
        float km = 0, tm = 0;
        int rt = 0;
        if (gab_kmer_last_stats(hs[g], NULL, NULL, &km, &tm) == 0 && gab_kmer_last_part(hs[g], NULL, NULL, NULL, &rt) == 0) {
            if (km > kernel_ms) kernel_ms = km;
            if (tm > total_ms) total_ms = tm;
            retried += rt;
        }
    }
    log_debug("Distinct k-mers: %lld, positions: %lld, largest count: %lld; device: count stage %.3f ms, call %.3f ms", (long long)res.distinct,
              (long long)res.positions, (long long)res.max_count, kernel_ms, total_ms);
    if (retried) log_debug("%d partition(s) filled their first table and were counted again in a larger one", retried);
    fprintf(stderr, "Kernel time: %.3f sec\n", t1 - t0);
    if (R.bytes) gab_unpin(R.seq);
    for (int g = 0; g < ngpus; g++) gab_kmer_destroy(hs[g]);
    gab_kmer_destroy(solid);
    free(hs); free(part_res); free(part_rc); free(part_err);
    free(R.seq); free(R.off); free(R.len);
    if (g_log) fclose(g_log);
    return 0;
}
