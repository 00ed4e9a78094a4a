/* main.c -- slaMEM-compatible command line in front of the MI355X engine.
 *
 *   slaMEM-hip (<options>) <reference_file> <query_file(s)>
 *
 * Keeps the reference's options, stdout shape and *-mems.txt format (slamem.c:528-672, 37-218); the
 * index build and the MEM search run on the GPU through the C ABI of include/slamem_hip.h.
 * There is no CPU fallback: without a usable GPU the program prints the library's error and exits 255.
 *
 * Environment: SLAMEM_DEVICE (default 0) selects the GPU; SLAMEM_VERBOSE=1 prints one line per loaded
 * record and per strand for any number of records, as the reference does (default: first 100 only);
 * SLAMEM_BATCH_MB bounds the query characters sent to the GPU per batch (default 256); SLAMEM_OVERLAP_MB (default 256):
 * query files above this size in total are parsed in pieces of SLAMEM_PIECE_MB (128) beside the search, -1 = never;
 * SLAMEM_NO_BIND=1 leaves the host threads where the scheduler puts them (default: on the CPUs local to the GPU);
 * SLAMEM_FULL_TEARDOWN=1 frees every buffer and the index before returning (default: one process that ends with _exit
 * once the results are written -- the command returns when its GPU memory is back, so a job started right behind it
 * finds the device free, and schedulers see the job end when it ends).  SLAMEM_DETACH_TEARDOWN=1 (opt-in): the work runs
 * in a forked worker and the command returns as soon as the results are written, while the worker still gives back its
 * HBM and pinned memory behind the caller's back (0.3-0.4 s for the reference-sized run); never use it under a profiler
 * (the fork would follow the profiler's GPU initialisation).  SLAMEM_WAIT_HBM_S (default 30): how long start-up waits
 * for the HBM the index needs to become free (the tail of such a detached worker, or any other job) before it builds.
 * SLAMEM_READOUT_ROWS (a test knob; default 16 Mi, at least 64): the rows of the pileup that a read-out takes from the GPU at a
 * time, so that a test can make the records of a small reference cross the borders of these ranges.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <unistd.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <pthread.h>
#include <dlfcn.h>
#include <dirent.h>
#include <sched.h>
#include <ctype.h>
#include <errno.h>
#include <signal.h>
#include <sys/prctl.h>
#include <sys/wait.h>

#include "../../include/slamem_hip.h"
#include "../../include/slamem_rccl.h"
#include "slamem_host.h"

#define VERSION "0.8.2"
/* what the output lines call a match of each type: M%cM with the reference's "EAU" (slamem.c:35), SMEM for -smem,
 * "chained MEM" for the rows -chain keeps and "extended MEM" for the rows of -ext */
static const char *const MATCH_TYPE_NAME[9] = {"MEM", "MAM", "MUM", "SMEM", "chained MEM", "extended MEM", "alignment", "mapping", "pileup"};
#define MATCH_NAME(t) MATCH_TYPE_NAME[(t) >= 0 && (t) < 9 ? (t) : 0]

/* the device warm-up thread (see main) is joined before the process ends, whichever way it ends */
static pthread_t g_warm_tid;
static int g_warm_started = 0;
static void join_warmup(void) {
    if (g_warm_started) { g_warm_started = 0; pthread_join(g_warm_tid, NULL); }
}

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* Large query files are parsed in pieces by their own thread while the main thread already searches the first pieces
 * (slh_pieces_*): the FASTA parse (0.2 s for the reference-sized run) no longer stands in front of the search. */
typedef struct {
    char **argv;
    const int *file_args;
    int first_file, num_files, acgt_only, numbering;
    uint32_t min_len;
    long log_limit, piece_bytes;
    slh_seqset *sets;  /* room for every piece */
    uint64_t **masks;  /* -bq: per piece the low-quality mask over its letters (NULL: FASTA, or -bq 0), as many entries as sets */
    int min_bq;        /* -bq N: 0 = the qualities are not used */
    int keep_quals;    /* -sam: the quality bytes of every piece are kept for the QUAL column */
    char **quals;      /* ... per piece (NULL: FASTA), as many entries as sets */
    int fasta_seen;    /* a query file without qualities came in (said once when -bq asks for them) */
    int wq;            /* -wq: the quality bytes of every piece are kept for the pileup's quality sums, and -bq's mask is packed as well */
    int wq_fill;       /* -wq: the byte the letters of a FASTA piece get, 33 + -err's Q */
    int fasta_filled;  /* -wq: a query file without qualities came in and was filled (said once) */
    int invalid;       /* a query file is no valid FASTQ: the run ends */
    int cap;
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int ready, done, total_queries;
    int release_early; /* footprint before speed: see main */
    int failed;        /* more pieces than main made room for */
    double seconds;
} loader_t;

/* -bq N: the low-quality mask of a set's letters from its quality bytes, packed by the host threads; the
 * qualities go.  NULL when the qualities are not used or there are none. */
static uint64_t *mask_of_quals(loader_t *ld, const slh_seqset *s, char *quals) {
    uint64_t *mask = NULL;
    if (!quals) { if (ld->min_bq > 0) ld->fasta_seen = 1; return NULL; }
    if (ld->min_bq > 0) {
        mask = (uint64_t *)slh_big_malloc(((size_t)(s->total + 63) / 64 + 1) * sizeof(uint64_t));
        if (mask && slamem_pack_lowq(quals, s->total, (uint32_t)ld->min_bq, 33, mask, slh_thread_count()) != SLAMEM_OK) {
            free(mask);
            mask = NULL;
        }
        if (!mask) ld->invalid = 2; /* (out of memory: never count letters that were to be skipped) */
    }
    free(quals);
    return mask;
}

/* -wq: the set's quality bytes stay (a FASTA set gets wq_fill at every letter), and with -bq N the mask is packed from them as
 * well.  Returns the mask or NULL; *quals is the set's bytes afterwards (NULL: out of memory, ld->invalid says so). */
static uint64_t *wq_quals(loader_t *ld, const slh_seqset *s, char **quals) {
    uint64_t *mask = NULL;
    if (!*quals) {
        if (ld->min_bq > 0) ld->fasta_seen = 1;
        ld->fasta_filled = 1;
        *quals = (char *)slh_big_malloc((size_t)s->total + 16);
        if (!*quals) { ld->invalid = 2; return NULL; }
        memset(*quals, ld->wq_fill, (size_t)s->total + 16);
        return NULL;
    }
    if (ld->min_bq > 0) {
        mask = (uint64_t *)slh_big_malloc(((size_t)(s->total + 63) / 64 + 1) * sizeof(uint64_t));
        if (mask && slamem_pack_lowq(*quals, s->total, (uint32_t)ld->min_bq, 33, mask, slh_thread_count()) != SLAMEM_OK) {
            free(mask);
            mask = NULL;
        }
        if (!mask) ld->invalid = 2; /* (out of memory: never count letters that were to be skipped) */
    }
    return mask;
}

static void *loader_run(void *arg) {
    loader_t *ld = (loader_t *)arg;
    double t0 = now_s();
    int f;
    for (f = ld->first_file; f < ld->num_files; f++) {
        slh_pieces *p = slh_pieces_open(ld->argv[ld->file_args[f]], ld->acgt_only, ld->min_len, ld->numbering, ld->log_limit,
                                        ld->piece_bytes, stdout);
        if (!p) continue;
        slh_pieces_release_parsed(p, ld->release_early);
        for (;;) {
            slh_seqset s;
            char *quals = NULL;
            uint64_t *mask;
            int n = slh_pieces_next_q(p, &s, &quals);
            if (n < 0) ld->invalid = 1;
            if (n <= 0) break;
            mask = ld->wq ? wq_quals(ld, &s, &quals) : ld->keep_quals ? NULL : mask_of_quals(ld, &s, quals);
            pthread_mutex_lock(&ld->mu);
            if (ld->ready < ld->cap) {
                if (ld->keep_quals) { ld->quals[ld->ready] = quals; quals = NULL; }
                ld->masks[ld->ready] = mask;
                ld->sets[ld->ready++] = s;
                ld->total_queries += n;
                ld->numbering += n;
            } else { /* cannot happen (a piece is at least piece_bytes of its file): never drop reads silently */
                ld->failed = 1;
                free(mask);
                if (ld->keep_quals) free(quals);
                slh_free_seqset(&s);
            }
            pthread_cond_broadcast(&ld->cv);
            pthread_mutex_unlock(&ld->mu);
        }
        slh_pieces_close(p);
    }
    pthread_mutex_lock(&ld->mu);
    ld->done = 1;
    ld->seconds = now_s() - t0;
    pthread_cond_broadcast(&ld->cv);
    pthread_mutex_unlock(&ld->mu);
    return NULL;
}

/* While the loader thread still parses query files (and prints its "# NN [name]" lines), the main thread's lines are held
 * back in memory; release_stdout joins the loader, prints the reference's "successfully loaded" line and then the held
 * text, so that stdout reads as if everything had been loaded first (slamem.c:635-651 before :37-218).  Every exit path
 * calls it first. */
static loader_t g_ld;
static pthread_t g_ld_tid;
static int g_ld_started = 0;
static FILE *g_mo = NULL; /* the memory stream, NULL: print directly */
static char *g_mo_buf = NULL;
static size_t g_mo_len = 0;
static int g_num_refs = 0;
#define say(...) fprintf(g_mo ? g_mo : stdout, __VA_ARGS__)
static void release_stdout(void) {
    if (g_ld_started) {
        g_ld_started = 0;
        pthread_join(g_ld_tid, NULL);
        if (g_ld.ready > 0)
            printf("> %d reference%s and %d quer%s successfully loaded\n", g_num_refs, g_num_refs == 1 ? "" : "s", g_ld.total_queries,
                   g_ld.total_queries == 1 ? "y" : "ies");
    }
    if (g_mo) {
        FILE *m = g_mo;
        g_mo = NULL;
        fclose(m);
        if (g_mo_buf && g_mo_len) fwrite(g_mo_buf, 1, g_mo_len, stdout);
        free(g_mo_buf);
        g_mo_buf = NULL;
    }
}


static void exit_message(const char *msg) { /* tools.c:21-25 */
    release_stdout();
    printf("> ERROR: %s\n", msg);
    join_warmup();
    exit(-1);
}

static void gpu_fail(const char *what, int rc) {
    release_stdout();
    printf("\n> ERROR: %s failed: %s (%s)\n", what, slamem_strerror(rc), slamem_last_error_message());
    join_warmup();
    exit(-1);
}

static void gpu_fail_msg(const char *what, int rc, const char *detail) { /* the detail was captured on another thread */
    release_stdout();
    printf("\n> ERROR: %s failed: %s (%s)\n", what, slamem_strerror(rc), detail);
    join_warmup();
    exit(-1);
}

/* What a batch's search handed back, and whose reads they are: everything the formatters of a strand block read. */
typedef struct {
    const slh_seqset *q, *ref;
    const char *quals;       /* -sam: the quality bytes of the set, indexed as its letters (NULL: FASTA) */
    const slamem_mem *mems;
    const uint32_t *mism;    /* -ext: a fourth column, the mismatches of each row (NULL otherwise) */
    const slamem_aln *segs;  /* -aln: the segments in the place of the rows (NULL otherwise), their operations and offsets */
    const uint32_t *ops;
    const uint64_t *ooff;
    const slamem_map *reads; /* -paf: a record per read (NULL otherwise); the blocks are then the reads, strands = 1 */
    const uint32_t *md;      /* -sam: the MD entries of the batch's segments, their offsets per segment, the primary segment per read */
    const uint64_t *mdoff;   /*       (NULL otherwise) */
    const uint32_t *prim;
    const uint64_t *boff;
    uint64_t total;
    int first_rec, strands;
} batch_view;

/* formatting of a range of strand blocks of one batch, one range per thread */
typedef struct {
    const batch_view *v;
    uint64_t b0, b1; /* strand blocks [b0,b1) of the batch */
    slh_buffer buf;
    long long matches, sum;
    int failed;
    double t_start, t_end; /* (SLAMEM_TIMING) when the thread worked */
} fmt_job;

/* Text buffers go round: formatter -> writer -> pool -> formatter.  A fresh 20 MB buffer costs its page faults every
 * time (the output of the reference-sized run is 638 MB); a recycled one is already mapped. */
static pthread_mutex_t g_pool_mu = PTHREAD_MUTEX_INITIALIZER;
static slh_buffer g_pool[512];
static int g_pool_n = 0;
static long g_pool_hits = 0, g_pool_misses = 0; /* (SLAMEM_TIMING) */
static double g_fmt_busy = 0, g_fmt_longest = 0, g_fmt_latest_start = 0; /* (SLAMEM_TIMING) formatter threads: CPU time, per-batch maxima */
static void pool_put(slh_buffer *b) {
    pthread_mutex_lock(&g_pool_mu);
    if (b->data && g_pool_n < 512) { b->len = 0; g_pool[g_pool_n++] = *b; b->data = NULL; }
    pthread_mutex_unlock(&g_pool_mu);
    if (b->data) slh_buffer_free(b);
    b->data = NULL; b->len = b->cap = 0;
}
static void pool_get(slh_buffer *b, size_t need) {
    int i, best = -1;
    pthread_mutex_lock(&g_pool_mu);
    for (i = 0; i < g_pool_n; i++)
        if (g_pool[i].cap >= need && (best < 0 || g_pool[i].cap < g_pool[best].cap)) best = i;
    if (best >= 0) { *b = g_pool[best]; g_pool[best] = g_pool[--g_pool_n]; g_pool_hits++; }
    else g_pool_misses++;
    pthread_mutex_unlock(&g_pool_mu);
}

/* strand block b of a batch in the format of its mode: read b / strands of the batch is record i of its set */
static int format_block(const batch_view *v, uint64_t b, slh_buffer *buf, uint64_t *cnt, uint64_t *sum) {
    const int i = v->first_rec + (int)(b / (uint64_t)v->strands), s = (int)(b % (uint64_t)v->strands);
    const slh_seqset *q = v->q, *ref = v->ref;
    const uint64_t o = v->boff[b];
    *cnt = v->boff[b + 1] - o;
    *sum = 0;
    if (v->md)
        return slh_format_read_sam(buf, q->recs[i].name, q->chars + q->offsets[i], v->quals ? v->quals + q->offsets[i] : NULL,
                                   (uint32_t)(q->offsets[i + 1] - q->offsets[i]), v->reads[b].strand, v->reads[b].mapq, v->reads[b].s1,
                                   v->reads[b].s2, (const uint32_t *)(v->segs + o), v->ops, v->ooff + o, v->md, v->mdoff + o, v->prim[b],
                                   *cnt, ref->recs, ref->merged_start, ref->num, sum);
    if (v->reads)
        return slh_format_read_paf(buf, q->recs[i].name, q->recs[i].size, v->reads[b].strand, v->reads[b].mapq, v->reads[b].s1,
                                   v->reads[b].s2, (const uint32_t *)(v->segs + o), v->ops, v->ooff + o, *cnt, ref->recs,
                                   ref->merged_start, ref->num, sum);
    if (v->segs)
        return slh_format_block_aln(buf, q->recs[i].name, s, (const uint32_t *)(v->segs + o), v->ops, v->ooff + o, *cnt, ref->recs,
                                    ref->merged_start, ref->num, sum);
    return slh_format_block_ext(buf, q->recs[i].name, s, (const uint32_t *)(v->mems + o), v->mism ? v->mism + o : NULL, *cnt,
                                ref->recs, ref->merged_start, ref->num, sum);
}

static void *fmt_run(void *arg) {
    fmt_job *j = (fmt_job *)arg;
    const uint64_t *boff = j->v->boff;
    uint64_t b;
    j->t_start = now_s();
    /* about 36 characters per MEM line and a header per block: reserve once instead of doubling on the way */
    const size_t need = (size_t)(boff[j->b1] - boff[j->b0]) * (j->v->mism ? 44 : 36) + (size_t)(j->b1 - j->b0) * 48 + 4096;
    /* the buffer's head and the sums stay on this thread's stack while it works: the jobs lie side by side in one array, and
       a write per strand block into it would share cache lines with the threads that work on the neighbours */
    slh_buffer buf = {0, 0, 0};
    long long matches = 0, total = 0;
    pool_get(&buf, need);
    (void)slh_buffer_reserve(&buf, need);
    int failed = 0;
    for (b = j->b0; b < j->b1 && !failed; b++) {
        uint64_t cnt, sum;
        failed = format_block(j->v, b, &buf, &cnt, &sum) != 0;
        matches += (long long)cnt;
        total += (long long)sum;
    }
    j->failed = failed;
    j->buf = buf;
    j->matches = matches;
    j->sum = total;
    j->t_end = now_s();
    return NULL;
}


/* the formatter threads of a batch take its chunks (ranges of strand blocks) from a shared counter: equal shares per
 * thread left the batch waiting for its slowest thread (measured: twice the mean, on a box whose CPU share is smaller
 * than the number of threads) */
typedef struct {
    fmt_job *jobs;
    int njobs;
    int next; /* atomic */
} fmt_queue;

static void *fmt_worker(void *arg) {
    fmt_queue *q = (fmt_queue *)arg;
    for (;;) {
        int c = __atomic_fetch_add(&q->next, 1, __ATOMIC_RELAXED);
        if (c >= q->njobs) return NULL;
        fmt_run(&q->jobs[c]);
    }
}

/* The index is built on the GPU by its own host thread while the main thread parses the query files: the two do not
 * depend on each other (the reference does them one after the other, slamem.c:635-651 then :73-74). */
typedef struct {
    const char *text;
    uint32_t n;
    int device;
    slamem_index *idx;
    slamem_index_info info;
    slamem_timings tm;
    slamem_sslcp_stats st;
    int rc, rc_stats;
    double seconds;
    char err[512];
} build_job;

/* A job that starts right behind another one (a detached worker still giving back its arena, any other tenant of the
 * GPU) finds less HBM free than it will have a moment later: wait, with a bound, until the full layout's build peak
 * fits -- or the compact layout's when the device could never hold the full one -- instead of failing or silently
 * taking the slower layout.  The reference frees before it reports (slamem.c:208-216); this is the other half. */
static void wait_for_hbm(const build_job *b) {
    uint64_t arena = 0, peak_full = 0, peak_compact = 0, free_b = 0, total_b = 0, want;
    const char *env = getenv("SLAMEM_WAIT_HBM_S");
    double limit = env ? atof(env) : 30.0, t0 = now_s();
    int told = 0;
    if (limit <= 0) return;
    if (slamem_index_build_bytes(b->n, SLAMEM_LAYOUT_FULL, &arena, &peak_full) != SLAMEM_OK) return;
    if (slamem_index_build_bytes(b->n, SLAMEM_LAYOUT_COMPACT, &arena, &peak_compact) != SLAMEM_OK) return;
    for (;;) {
        if (slamem_device_mem_info(b->device, &free_b, &total_b) != SLAMEM_OK) return;
        want = (peak_full + (1ull << 30) <= total_b ? peak_full : peak_compact) + (256ull << 20);
        if (free_b >= want || want > total_b || now_s() - t0 > limit) break;
        if (!told) {
            fprintf(stderr, "> Waiting for HBM on GPU %d: %.1f GB free, %.1f GB needed to build the index (another job is still releasing its memory?)\n",
                    b->device, (double)free_b / 1e9, (double)want / 1e9);
            told = 1;
        }
        usleep(50000);
    }
    if (told) fprintf(stderr, "> Waited %.2f s for HBM (%.1f GB free now)\n", now_s() - t0, (double)free_b / 1e9);
}

static void *build_run(void *arg) {
    build_job *b = (build_job *)arg;
    double t0;
    wait_for_hbm(b);
    t0 = now_s();
    b->rc = slamem_index_build(b->text, b->n, b->device, &b->idx);
    if (b->rc == SLAMEM_OK) {
        slamem_index_get_info(b->idx, &b->info);
        slamem_get_timings(&b->tm); /* timings and error text are per thread: take them here */
        b->rc_stats = slamem_index_sampled_lcp_stats(b->idx, &b->st);
    }
    if (b->rc != SLAMEM_OK || b->rc_stats != SLAMEM_OK) snprintf(b->err, sizeof(b->err), "%s", slamem_last_error_message());
    b->seconds = now_s() - t0;
    return NULL;
}

/* The output file is written by its own thread: the main thread hands over formatted buffers in order and goes on
 * formatting the next ones (GPU(b+1), format(b) and write(b-1) overlap; the reference does everything in one loop,
 * slamem.c:90-207). */
typedef struct wnode {
    slh_buffer buf;
    struct wnode *next;
} wnode;
typedef struct {
    FILE *out;
    pthread_t tid;
    pthread_mutex_t mu;
    pthread_cond_t cv;
    wnode *head, *tail;
    size_t queued; /* bytes waiting */
    int done, failed, started;
    double seconds;
} writer_t;

static void *writer_run(void *arg) {
    writer_t *w = (writer_t *)arg;
    for (;;) {
        wnode *n;
        double t0;
        pthread_mutex_lock(&w->mu);
        while (!w->head && !w->done) pthread_cond_wait(&w->cv, &w->mu);
        n = w->head;
        if (n) { w->head = n->next; if (!w->head) w->tail = NULL; }
        pthread_mutex_unlock(&w->mu);
        if (!n) return NULL;
        t0 = now_s();
        if (n->buf.len && !w->failed && fwrite(n->buf.data, 1, n->buf.len, w->out) != n->buf.len) w->failed = 1;
        w->seconds += now_s() - t0;
        pthread_mutex_lock(&w->mu);
        w->queued -= n->buf.len;
        pthread_cond_broadcast(&w->cv);
        pthread_mutex_unlock(&w->mu);
        pool_put(&n->buf);
        free(n);
    }
}

/* takes ownership of *buf (and leaves it empty); waits while more than 1 GiB of text is queued */
static int writer_push(writer_t *w, slh_buffer *buf) {
    wnode *n;
    if (!buf->len) return 0;
    n = (wnode *)calloc(1, sizeof(wnode));
    if (!n) return -1;
    n->buf = *buf;
    buf->data = NULL; buf->len = buf->cap = 0;
    if (!w->started) { /* no thread: write here */
        int bad = fwrite(n->buf.data, 1, n->buf.len, w->out) != n->buf.len;
        if (bad) w->failed = 1;
        slh_buffer_free(&n->buf);
        free(n);
        return 0;
    }
    pthread_mutex_lock(&w->mu);
    while (w->queued > ((size_t)1 << 30)) pthread_cond_wait(&w->cv, &w->mu);
    if (w->tail) w->tail->next = n; else w->head = n;
    w->tail = n;
    w->queued += n->buf.len;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
    return 0;
}

static void writer_finish(writer_t *w) {
    if (!w->started) return;
    pthread_mutex_lock(&w->mu);
    w->done = 1;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
    pthread_join(w->tid, NULL);
    w->started = 0;
}

/* every exit after the search has started goes through here: batches in flight finish first (slamem_stream_destroy
 * waits for them), the writer drains -- never leave the process with kernels running or a thread writing */
static slamem_stream *g_streams[16];
static int g_nstreams = 0;
static writer_t g_writer;
static void shutdown_pipeline(void) {
    int g;
    for (g = 0; g < g_nstreams; g++) { slamem_stream_destroy(g_streams[g]); g_streams[g] = NULL; }
    g_nstreams = 0;
    writer_finish(&g_writer);
}
static void pipeline_fail(const char *msg) {
    shutdown_pipeline();
    exit_message(msg);
}

/* A piece of the query files whose batches are all formatted can be released by a thread of its own while the main thread
 * goes on.  Measured on the reference-sized run (1.5 GB of reads): it takes 0.10 s off the end of the process and adds
 * 0.10 s to the formatting beside it (the address-space work stalls the formatter threads), so it is only done when the
 * footprint matters: query files above SLAMEM_RELEASE_EARLY_GB (default 16) in total. */
static pthread_t *g_reap_tid = NULL;
static int g_reap_n = 0;
static void *reap_run(void *arg) {
    slh_free_seqset((slh_seqset *)arg);
    free(arg);
    return NULL;
}
static void reap_set(slh_seqset *s) {
    slh_seqset *copy = (slh_seqset *)malloc(sizeof(slh_seqset));
    if (!copy || !g_reap_tid) { free(copy); return; } /* stays allocated until the process ends */
    *copy = *s;
    if (pthread_create(&g_reap_tid[g_reap_n], NULL, reap_run, copy) != 0) { free(copy); return; }
    g_reap_n++;
    memset(s, 0, sizeof(*s));
}

/* The host threads (FASTA parsing, formatting, the copies behind uploads from ordinary memory) work on memory that the GPU's
 * NUMA node holds or receives: on a two-socket box they ran 1.5 times longer when the scheduler spread them over both
 * sockets (tools/cli_numa_probe.sh: 0.47-0.56 s -> 0.42 s for the reference-sized run).  Once the runtime is up, every thread
 * of the process is confined to the CPUs that are local to the GPU -- if the process may use CPUs of more than one node,
 * and unless SLAMEM_NO_BIND is set.  Threads created later inherit the mask. */
static void bind_to_gpu_node(int device) {
    char bdf[64], path[160], list[4096];
    cpu_set_t local, allowed, both;
    FILE *f;
    DIR *d;
    struct dirent *e;
    const char *p;
    size_t i;
    if (getenv("SLAMEM_NO_BIND") != NULL) return;
    if (slamem_device_pci_bus_id(device, bdf, (int)sizeof(bdf)) != SLAMEM_OK) return;
    for (i = 0; bdf[i]; i++) bdf[i] = (char)tolower((unsigned char)bdf[i]);
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", bdf);
    f = fopen(path, "r");
    if (!f) return;
    if (!fgets(list, (int)sizeof(list), f)) { fclose(f); return; }
    fclose(f);
    CPU_ZERO(&local);
    for (p = list; *p;) { /* "0-63,128-191" */
        char *end;
        long a, b;
        if (!isdigit((unsigned char)*p)) { p++; continue; }
        a = strtol(p, &end, 10);
        b = a;
        if (*end == '-') b = strtol(end + 1, &end, 10);
        for (; a <= b && a < CPU_SETSIZE; a++) CPU_SET((int)a, &local);
        p = end;
    }
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return;
    CPU_AND(&both, &local, &allowed);
    if (CPU_COUNT(&both) == 0 || CPU_COUNT(&both) == CPU_COUNT(&allowed)) return; /* nothing local allowed / already local */
    {   /* not onto a handful of CPUs: the loader and formatter threads need room (a cpuset that leaves one or two local
           CPUs would serialise them), and a mask the user narrowed on purpose is left alone */
        int want = slh_thread_count(), half = CPU_COUNT(&allowed) / 2;
        long online = sysconf(_SC_NPROCESSORS_ONLN);
        if (want > half) want = half;
        if (CPU_COUNT(&both) < want) return;
        if (online > 0 && CPU_COUNT(&allowed) < (int)online && getenv("SLAMEM_BIND") == NULL) return;
    }
    d = opendir("/proc/self/task");
    if (!d) { (void)sched_setaffinity(0, sizeof(both), &both); return; }
    while ((e = readdir(d)) != NULL)
        if (isdigit((unsigned char)e->d_name[0])) (void)sched_setaffinity((pid_t)atol(e->d_name), sizeof(both), &both);
    closedir(d);
}

static int g_warm_ok = 0;
static void *warmup_run(void *arg) { /* HIP runtime + context start-up, hidden behind the parsing of the reference file */
    g_warm_ok = slamem_device_warmup(*(int *)arg) == SLAMEM_OK;
    return NULL;
}

/* The command returns when its results are complete, not when the kernel has taken back the gigabytes behind them.
 * The work runs in a child process (forked before any thread or GPU call exists); the parent only waits for one byte
 * that the child sends once the output file and stdout are written, and leaves with status 0 then.  What follows in
 * the child -- the end of a process that holds the index in HBM, pinned buffers and the queries, 0.35 s for the
 * reference-sized run -- happens behind the caller's back.  A child that ends without that byte (any error exit, a
 * signal) is waited for and its status passed on.  SLAMEM_FOREGROUND=1: one process, as before. */
static int g_done_fd = -1;
static pid_t g_child = 0;
static void forward_signal(int sig) {
    if (g_child > 0) kill(g_child, sig);
}
/* has the process that forked us gone already?  (PR_SET_PDEATHSIG only covers a death AFTER the prctl call.)  Compared
 * with the pid the front had before the fork: getppid() == 1 says nothing when the front itself is pid 1 of a container,
 * and never happens under a subreaper. */
static int front_is_gone(pid_t front) { return getppid() != front; }
static void split_off_worker(void) {
    int pfd[2];
    pid_t pid, front = getpid();
    if (getenv("SLAMEM_DETACH_TEARDOWN") == NULL || getenv("SLAMEM_FOREGROUND") != NULL || pipe(pfd) != 0) return;
    fflush(stdout);
    fflush(stderr);
    pid = fork();
    if (pid < 0) { close(pfd[0]); close(pfd[1]); return; }
    if (pid == 0) { /* the worker */
        close(pfd[0]);
        g_done_fd = pfd[1];
        prctl(PR_SET_PDEATHSIG, SIGTERM); /* no worker without its front */
        if (front_is_gone(front)) _exit(255);
        return;
    }
    close(pfd[1]);
    g_child = pid;
    signal(SIGINT, forward_signal);
    signal(SIGTERM, forward_signal);
    signal(SIGHUP, forward_signal);
    for (;;) {
        char c;
        ssize_t n = read(pfd[0], &c, 1);
        int st;
        if (n == 1) _exit(0); /* everything is written */
        if (n < 0 && errno == EINTR) continue;
        while (waitpid(pid, &st, 0) < 0 && errno == EINTR) {}
        _exit(WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0));
    }
}
static void leave_now(void) { /* results complete: tell the front, then end without returning memory piece by piece */
    const char *linger = getenv("SLAMEM_TEST_LINGER_MS"); /* tests: hold the GPU memory this long after "done" */
    fflush(stdout);
    fflush(stderr);
    if (g_done_fd >= 0) {
        char c = 0;
        close(1);
        close(2);
        if (linger && atoi(linger) > 0) prctl(PR_SET_PDEATHSIG, 0); /* (the front's exit would end the worker at once) */
        if (write(g_done_fd, &c, 1) != 1) _exit(255);
        if (linger && atoi(linger) > 0) usleep((useconds_t)atoi(linger) * 1000u);
    }
    _exit(0);
}

/* "-v <mems_file>" (slamem.c:630-655): the sequences are loaded for their names and sizes only, then the picture is drawn */
static int image_tool(int argc, char **argv, slh_options *o, long log_limit) {
    slh_seqset ref, *sets;
    slh_record *seqs;
    int f, k, numbering = 1, loaded = 0, queries = 0, at = 0, status;
    (void)argc;
    memset(&ref, 0, sizeof(ref));
    sets = (slh_seqset *)calloc((size_t)o->num_files + 1, sizeof(slh_seqset));
    if (!sets) exit_message("Out of memory");
    for (f = 0; f < o->num_files; f++) {
        const char *path = argv[o->file_args[f]];
        int n = slh_load_file_q(path, loaded == 0, o->no_ns, (uint32_t)o->min_seq_len, loaded == 0 ? o->ref_name : NULL, numbering,
                                log_limit, loaded == 0 ? &ref : &sets[loaded], NULL, stdout);
        if (n < 0) { fflush(stdout); exit(-1); } /* (an invalid FASTQ file, or FASTQ as the reference: the loader said so) */
        if (n != 0) { loaded++; numbering += n; if (loaded > 1) queries += n; }
        if (loaded == 0) exit_message("No valid sequences found in reference file");
    }
    if (loaded == 1) exit_message("No query files provided");
    if (queries == 0) exit_message("No valid query sequences found");
    printf("> %d reference%s and %d quer%s successfully loaded\n", ref.num, ref.num == 1 ? "" : "s", queries, queries == 1 ? "y" : "ies");
    seqs = (slh_record *)calloc((size_t)queries + 1, sizeof(slh_record));
    if (!seqs) exit_message("Out of memory");
    seqs[at].name = ref.recs[0].name;
    seqs[at++].size = (uint32_t)ref.total; /* one record: its size; several: refused by the tool */
    for (f = 1; f < loaded; f++)
        for (k = 0; k < sets[f].num; k++) seqs[at++] = sets[f].recs[k];
    status = slh_mem_map_image(argv[o->image_arg], seqs, at, ref.num, stdout);
    fflush(stdout);
    free(seqs);
    for (f = 1; f < loaded; f++) slh_free_seqset(&sets[f]);
    free(sets);
    slh_free_seqset(&ref);
    slh_free_options(o);
    return status;
}

static void usage(const char *prog) { /* slamem.c:533-553 */
    printf("Usage:\n");
    printf("\t%s (<options>) <reference_file> <query_file(s)>\n", prog);
    printf("Options:\n");
    printf("\t-mem\tfind MEMs: any number of occurrences in both ref and query (default)\n");
    printf("\t-mam\tfind MAMs: unique in ref but any number in query\n");
    printf("\t-smem\tfind SMEMs: MEMs whose query interval no other MEM of the strand contains\n");
    printf("\t-occ\twith -smem: drop SMEMs found at more than this many places in ref (default: no limit)\n");
    printf("\t-chain\tkeep the MEMs of the best collinear chain of each strand\n");
    printf("\t-mgap\twith -chain: maximum gap between chained MEMs in ref and in query (default=5000)\n");
    printf("\t-ext\textend every MEM through mismatches (ungapped X-drop); writes a fourth column, the mismatches\n");
    printf("\t-pen\twith -ext: mismatch penalty, a match scores 1 (default=4)\n");
    printf("\t-xdrop\twith -ext: stop when the score falls this far below its best (default=20)\n");
    printf("\t-aln\tgapped alignment of the best chain of each strand; writes ref_pos query_pos ref_len query_len edits cigar\n");
    printf("\t-maxed\twith -aln: most edits in the gap between two chained MEMs, 0 to 127 (default=31); -mgap, -pen, -xdrop apply\n");
    printf("\t-affine\twith -aln and every mode that takes -maxed: X,O,E, gap-affine costs of the gap between two chained MEMs: X per mismatch (1 to 31), O per gap opened (0 to 63), E per gap letter (1 to 31); the gap closes when its cost is at most O + E * maxed (at most 512); without it: unit costs\n");
    printf("\t-gext\twith -affine: Z, a whole number from 1 to 31; each of an alignment's two outer ends may hold indels of at most Z letters of net diagonal drift (gapped X-drop extension); without it: ungapped ends\n");
    printf("\t-paf\tone mapping per read with a mapping quality, written as PAF with a cg:Z: CIGAR; -mgap, -pen, -xdrop, -maxed apply\n");
    printf("\t-sam\tthe mappings of -paf written as SAM: a line per segment with soft clips, NM:i:, MD:Z: (built on the GPU), s1:i:, s2:i: and SA:Z:; an unmapped read gets a line with flag 4; FASTQ queries keep their qualities; -mgap, -pen, -xdrop, -maxed apply\n");
    printf("\t-pile\tper-base pileup of the mappings of -paf: record, position, letter and the counts A C G T D I; -mgap, -pen, -xdrop, -maxed apply\n");
    printf("\t-minq\twith -pile: least mapping quality of a read that counts, 0 to 60 (default=0)\n");
    printf("\t-bq\twith -pile, -sites, -vcf, -cons, -depth: least base quality of a read letter that counts, 0 to 93 (default=0: all); needs FASTQ queries (a file that starts with '@')\n");
    printf("\t-sites\tvariant sites of the pileup: the rows of -pile where the reads differ from the reference, with a tenth column, the calls; -mgap, -pen, -xdrop, -maxed, -minq apply\n");
    printf("\t-mdep\twith -sites: least depth A+C+G+T+D of a site (default=4)\n");
    printf("\t-mpct\twith -sites: least share of the depth a call needs, in percent, 0 to 100 (default=20)\n");
    printf("\t-vcf\tthe calls of the pileup as VCF 4.2: the SNVs of -sites and the reads' insertions and deletions as left-normalised events; -mgap, -pen, -xdrop, -maxed, -minq, -mdep, -mpct apply\n");
    printf("\t-cons\tthe consensus sequence of the mapped reads as FASTA, a record per reference record: per position the plurality letter (lower case: the reference kept below the depth of -mdep), and the insertions and deletions that more than half of the reads show; -mgap, -pen, -xdrop, -maxed, -minq, -mdep, -evs apply\n");
    printf("\t-depth\tthe depth of coverage A+C+G+T+D of the mapped reads as a bedGraph: record, start, end (0-based, half-open) and the depth of each run of equal depth, the runs of depth 0 included; -mgap, -pen, -xdrop, -maxed, -minq apply; -mdep N: the depth from which a position counts as covered in the summary on stderr (default=1); -lev LIST: comma-separated ascending depths, the value of a run is the number of them it reaches; -win N: instead of the runs the mean depth of every N positions\n");
    printf("\t-dedup\twith -pile, -sites, -vcf, -cons, -depth: reads with the same strand and unclipped 5' position (PCR and optical copies) count once, the first in file order; found on the GPU; one GPU only\n");
    printf("\t-dslots\twith -dedup: slots of its table on the GPU, a power of two of at least 64 (default: at least 65536 and a quarter of the reference)\n");
    printf("\t-gt\twith -vcf: diploid genotypes called on the GPU from the counts at a constant error rate: one line per site with QUAL, and a sample column GT:DP:AD:GQ:PL; an indel event gets 0/1 or 1/1; -mdep applies, -mpct does not\n");
    printf("\t-ploidy\twith -gt: 1 or 2 (default=2)\n");
    printf("\t-err\twith -gt: the error rate of a read letter in Phred, 1 to 93 (default=20)\n");
    printf("\t-hetq\twith -gt: the prior cost of a non-reference allele in Phred, 0 to 999 (default=30)\n");
    printf("\t-qual\twith -gt: least QUAL of a call, 0 to 999 (default=20)\n");
    printf("\t-sb\twith -gt: strand counts in the pileup (a second accumulator on the GPU, fed by the forward-strand reads in the same pass); every line gets the strand table SB = reference forward, reference reverse, alternative forward, alternative reverse in the sample column and FS, the Phred-scaled Fisher exact test of it, in INFO\n");
    printf("\t-wq\twith -gt: every letter weighs with its own base quality in the likelihood of an SNV (a third accumulator on the GPU holds the sum of the qualities per row and letter); every SNV line gets ADQ, the quality sum per allele in AD's order; -err still scores the indel events and the letters of FASTA queries\n");
    printf("\t-fs\twith -sb: FILTER is sb for a line whose FS is above this whole number, 0 to 999, and PASS otherwise (default: FILTER stays .)\n");
    printf("\t-sv\twith -vcf: the long deletions and insertions that lie between two segments of one read (gaps that -maxed edits do not close), found on the GPU and written as <DEL> and <INS> lines with SVTYPE, END and SVLEN; not with -gt\n");
    printf("\t-svmin\twith -sv: least length of a junction that is written (default: maxed + 1)\n");
    printf("\t-svmis\twith -sv: mismatches the letters that both segments own may have in the best split between them, 0 to 64 (default=3)\n");
    printf("\t-svslots\twith -sv: slots of the junction table on the GPU, a power of two of at least 64 (default: at least 65536 and a 64th of the reference)\n");
    printf("\t-evs\twith -vcf: slots of the event table on the GPU, a power of two of at least 64 (default: at least 65536 and a sixteenth of the reference)\n");
    printf("\t-stats\tmap the reads as -paf does and write the mapping statistics, added up on the GPU: totals (reads, mapped, strands, mismatch and indel rates), MAPQ, read lengths, edits per read, per-cycle and per-base-quality error tables, the substitution spectrum and indel lengths; -minq sets the least mapping quality of the reads that count\n");
    printf("\t-l\tminimum match length (default=20)\n");
    printf("\t-o\toutput file name (default=\"*-mems.txt\")\n");
    printf("\t-b\tprocess both forward and reverse strands\n");
    printf("\t-n\tdiscard 'N' characters in the sequences\n");
    printf("\t-m\tminimum sequence size (e.g. to ignore small scaffolds)\n");
    printf("\t-r\tload only the reference(s) whose name(s) contain(s) this string\n");
    printf("Extra:\n");
    printf("\t-v\tgenerate MEMs map image from this MEMs file\n");
    printf("Example:\n");
    printf("\t%s -b -l 10 ./ref.fna ./query.fna\n", prog);
    printf("\t%s -v ./ref-mems.txt ./ref.fna ./query.fna\n", prog);
}

/* ------------------------------------------------------------------------------------------------ */
/* the run: one context, and main() as the list of its stages                                        */
/* ------------------------------------------------------------------------------------------------ */

typedef struct { int f, first, last; } batch_range; /* records [first,last) of query set f */
#define STREAM_SLOTS 6 /* upload, prepare, search and download of four batches beside the one being formatted */

typedef struct {
    int argc;
    char **argv;
    slh_run p;            /* what the command line says */
    slamem_gt_params gtp; /* -gt: the costs behind p.gt_* */
    int sb, fs;           /* -sb: strand counts; -fs N, or -1 */
    int wq;               /* -wq: per-letter base qualities in the SNV likelihood */
    slamem_gt_params gtp_wq; /* -wq: gtp with the costs 0, 3010, 4771 for the rows; the events keep gtp */
    int device, timing;
    long log_limit;
    uint64_t batch_bytes;  /* query characters per batch and GPU */
    long piece_bytes;      /* bytes of a query file per piece of the loader thread */
    uint64_t readout_rows; /* rows of the pileup per range of a read-out */
    slh_seqset ref, *qsets;
    loader_t *ld;
    int overlap; /* the loader thread parses beside the search */
    build_job bj;
    pthread_t build_tid;
    int build_async;
    char *out_name;
    FILE *out;
    slamem_index *gpus[16];
    int ngpu;
    slamem_pileup *piles[16];
    int sv, sv_min, sv_mis; /* -sv: junctions in the -vcf file; the least length written; mismatches of a split */
    uint64_t sv_slots, sv_skipped[4], sv_stored, sv_counts[2]; /* ... the table's slots; what GPUs 1.. did not store; keys; lines and first rows */
    int gext;              /* -gext Z: the band of the gapped outer ends; 0: the option is absent */
    int affine, costs[3];  /* -affine X,O,E: gap-affine costs of the gaps between chain anchors */
    int stats;             /* -stats: the mapping QC table; runs as -paf, nothing is formatted per read */
    int stats_fasta;       /* ... a batch without quality bytes was submitted (said once) */
    slamem_stats *tables[16]; /* ... one table per GPU */
    int strands; /* strand blocks per read */
    batch_range *ranges;
    size_t nranges, cap_ranges;
    uint64_t max_chars;
    uint32_t max_recs;
    int sets_seen, inflight[16];
    long printed; /* strand blocks that got their line on stdout */
    slh_buffer buf;
    slh_piece *pcs; /* the record pieces of a read-out's range (room for every record) */
    uint64_t skipped[3]; /* -vcf, -cons: indel observations that are in no event */
    int total_queries;
    long long total_matches, total_sum;
    double t_start, t_load, t_build, t_join, t_streams, t_gpu, t_format, t_wait_load;
} run_t;

static void pipeline_gpu_fail(const char *what, int rc) {
    shutdown_pipeline();
    gpu_fail(what, rc);
}

static void push_text(run_t *R) { /* what a stage has formatted goes to the writer */
    if (writer_push(&g_writer, &R->buf)) pipeline_fail("Out of memory");
    if (g_writer.failed) pipeline_fail("Cannot write output file");
}

/* Parse and refuse, before any GPU work.  Returns 1 when the command ends here with *status: the usage text and the tools
 * that need no GPU (-s, -c, -v). */
static int parse_and_refuse(run_t *R, int *status) {
    slh_options *o = &R->p.o;
    const char *refusal, *env;
    const int argc = R->argc, rc = slh_parse_run(R->argc, R->argv, &R->p, &refusal);
    char **argv = R->argv;
    if (o->usage) { usage(argv[0]); slh_free_options(o); *status = -1; return 1; }
    if (o->hidden_sort) { /* slamem.c:555-562 */
        slh_free_options(o);
        if (argc != 3) { printf("Usage: %s -s <mems_file>\n\n", argv[0]); *status = -1; return 1; }
        *status = slh_sort_mems_file(argv[2], stdout);
        return 1;
    }
    if (o->hidden_clean) { /* slamem.c:563-570 */
        slh_free_options(o);
        if (argc != 3) { printf("Usage: %s -c <fasta_file>\n\n", argv[0]); *status = -1; return 1; }
        *status = slh_clean_fasta(argv[2], stdout);
        return 1;
    }
    if (rc == -1) exit_message(refusal);
    R->sb = slh_parse_sb_params(argc, argv, &R->fs) & 1; /* (refused above when the value of -fs is not one) */
    R->affine = slh_parse_affine(argc, argv, &R->costs[0], &R->costs[1], &R->costs[2]) > 0; /* (the same) */
    if (slh_parse_gext(argc, argv, &R->gext) <= 0) R->gext = 0;
    R->sv = slh_parse_sv(argc, argv, &R->sv_min, &R->sv_mis, &R->sv_slots) & 1; /* (a bad value, -sv without -vcf or with -gt: refused above) */
    if (R->sv_min < 0) R->sv_min = (R->p.max_edits >= 0 ? R->p.max_edits : 31) + 1;
    memset(&R->gtp, 0, sizeof(R->gtp));
    if (R->p.gt) { /* host arithmetic: the three costs of a letter at the error rate of -err */
        uint32_t costs[3];
        if (slamem_gt_costs((uint32_t)R->p.gt_err, costs) != SLAMEM_OK) exit_message("Option -err needs a whole number from 1 to 93");
        R->gtp.ploidy = (uint32_t)R->p.gt_ploidy;
        R->gtp.match_cost = costs[0];
        R->gtp.het_cost = costs[1];
        R->gtp.err_cost = costs[2];
        R->gtp.het_prior = 1000u * (uint32_t)R->p.gt_hetq;
        R->gtp.min_depth = (uint32_t)R->p.min_depth;
        R->gtp.min_qual = (uint32_t)R->p.gt_qual;
    }
    R->wq = slh_parse_wq(argc, argv) && R->p.gt; /* (without -gt: refused above) */
    R->stats = slh_parse_stats(argc, argv);
    R->gtp_wq = R->gtp;
    R->gtp_wq.match_cost = 0; R->gtp_wq.het_cost = 3010; R->gtp_wq.err_cost = 4771; /* round(10000 log10 2), round(10000 log10 3) */
    /* one table per GPU would miss the duplicates whose copies went to different GPUs */
    if (R->p.dedup && (((env = getenv("SLAMEM_GPUS")) != NULL && atoi(env) != 1) || ((env = getenv("SLAMEM_LOGICAL_GPUS")) != NULL && atoi(env) > 1)))
        exit_message("Option -dedup runs on one GPU: every GPU would keep a table of its own and miss the duplicates whose copies went to different GPUs (leave SLAMEM_GPUS unset, or set it to 1)");
    if (rc != 0) exit_message(refusal);
    if ((env = getenv("SLAMEM_DEVICE")) != NULL) R->device = atoi(env);
    if ((env = getenv("SLAMEM_VERBOSE")) != NULL && atoi(env) != 0) R->log_limit = 0;
    if (o->image_arg != -1) { *status = image_tool(argc, argv, o, R->log_limit); return 1; } /* slamem.c:652-655; host only */
    if ((env = getenv("SLAMEM_BATCH_MB")) != NULL && atoll(env) > 0) R->batch_bytes = (uint64_t)atoll(env) << 20;
    if ((env = getenv("SLAMEM_READOUT_ROWS")) != NULL) R->readout_rows = atoll(env) < 64 ? 64 : (uint64_t)atoll(env);
    R->timing = getenv("SLAMEM_TIMING") != NULL;
    return 0;
}

/* Load everything (slamem.c:635-651); the index build starts on its own thread as soon as the reference is there.  Query files
 * above SLAMEM_OVERLAP_MB (default 256) in total are parsed in pieces by a loader thread while the search already runs; stdout
 * keeps the reference's order: what the main thread prints meanwhile is held back until the "successfully loaded" line can be
 * printed. */
static void load_inputs(run_t *R) {
    const slh_options *o = &R->p.o;
    loader_t *const ld = R->ld = &g_ld;
    uint64_t qbytes_total = 0, pieces_cap = 0;
    long thr_mb = 256;
    int f, ref_file = -1, numbering = 1;
    const char *env;
    char **argv = R->argv;
    if ((env = getenv("SLAMEM_OVERLAP_MB")) != NULL) thr_mb = atol(env);
    if ((env = getenv("SLAMEM_PIECE_MB")) != NULL && atol(env) > 0) R->piece_bytes = atol(env) << 20;
    for (f = 1; f < o->num_files; f++) {
        FILE *qf = fopen(argv[o->file_args[f]], "rb");
        if (qf) {
            long sz;
            fseek(qf, 0L, SEEK_END);
            sz = ftell(qf);
            fclose(qf);
            if (sz > 0) { qbytes_total += (uint64_t)sz; pieces_cap += (uint64_t)sz / (uint64_t)R->piece_bytes + 2; }
        }
    }
    R->overlap = thr_mb >= 0 && qbytes_total > ((uint64_t)thr_mb << 20);
    memset(ld, 0, sizeof(*ld));
    ld->release_early = qbytes_total > ((uint64_t)((env = getenv("SLAMEM_RELEASE_EARLY_GB")) != NULL ? atol(env) : 16) << 30);
    ld->cap = (int)(R->overlap ? pieces_cap + (uint64_t)o->num_files : (uint64_t)o->num_files);
    R->qsets = (slh_seqset *)calloc((size_t)ld->cap + 1, sizeof(slh_seqset));
    g_reap_tid = (pthread_t *)calloc((size_t)ld->cap + 1, sizeof(pthread_t));
    if (!R->qsets || !g_reap_tid) exit_message("Out of memory");
    ld->sets = R->qsets;
    ld->masks = (uint64_t **)calloc((size_t)ld->cap + 1, sizeof(uint64_t *));
    if (!ld->masks) exit_message("Out of memory");
    ld->min_bq = R->p.min_bq;
    ld->keep_quals = R->p.sam || R->wq || R->stats;
    ld->wq = R->wq;
    ld->wq_fill = 33 + R->p.gt_err;
    ld->quals = (char **)calloc((size_t)ld->cap + 1, sizeof(char *));
    if (!ld->quals) exit_message("Out of memory");
    pthread_mutex_init(&ld->mu, NULL);
    pthread_cond_init(&ld->cv, NULL);
    for (f = 0; f < o->num_files; f++) {
        const char *path = argv[o->file_args[f]];
        if (ref_file < 0) {
            int n = slh_load_file_q(path, 1, o->no_ns, (uint32_t)o->min_seq_len, o->ref_name, numbering, R->log_limit, &R->ref, NULL, stdout);
            if (n <= 0) exit_message("No valid sequences found in reference file");
            ref_file = f;
            numbering += n;
            g_num_refs = R->ref.num;
            o->file_args[0] = o->file_args[f]; /* remember which argument was the reference */
            R->bj.text = R->ref.chars;
            R->bj.n = (uint32_t)R->ref.total;
            R->bj.device = R->device;
            R->build_async = pthread_create(&R->build_tid, NULL, build_run, &R->bj) == 0;
            if (R->overlap) break;
        } else {
            char *quals = NULL;
            int n = slh_load_file_q(path, 0, o->no_ns, (uint32_t)o->min_seq_len, NULL, numbering, R->log_limit, &R->qsets[ld->ready], &quals, stdout);
            if (n < 0) { /* an invalid FASTQ file (the loader said so): before any search */
                if (R->build_async) pthread_join(R->build_tid, NULL);
                join_warmup();
                fflush(stdout);
                exit(-1);
            }
            if (n != 0) {
                if (ld->wq) { ld->masks[ld->ready] = wq_quals(ld, &R->qsets[ld->ready], &quals); ld->quals[ld->ready] = quals; }
                else if (ld->keep_quals) ld->quals[ld->ready] = quals;
                else ld->masks[ld->ready] = mask_of_quals(ld, &R->qsets[ld->ready], quals);
                if (ld->invalid) exit_message("Out of memory");
                numbering += n; ld->total_queries += n; ld->ready++;
            }
        }
    }
    if (R->overlap) {
        ld->argv = argv; ld->file_args = o->file_args; ld->first_file = ref_file + 1; ld->num_files = o->num_files;
        ld->acgt_only = o->no_ns; ld->min_len = (uint32_t)o->min_seq_len; ld->numbering = numbering; ld->log_limit = R->log_limit;
        ld->piece_bytes = R->piece_bytes;
        fflush(stdout);
        g_mo = open_memstream(&g_mo_buf, &g_mo_len);
        g_ld_started = g_mo != NULL && pthread_create(&g_ld_tid, NULL, loader_run, ld) == 0;
        if (!g_ld_started) { /* no thread: load here, as for small inputs */
            if (g_mo) release_stdout();
            R->overlap = 0;
            loader_run(ld);
        }
    } else {
        ld->done = 1;
    }
    R->t_load = now_s() - R->t_start;
}

/* the index is there (or failed) and the device is warm before anything else happens: never leave with a build in flight */
static void join_build(run_t *R) {
    const double t0 = now_s();
    if (R->build_async) pthread_join(R->build_tid, NULL);
    else build_run(&R->bj);
    join_warmup();
    if (g_warm_ok) bind_to_gpu_node(R->device); /* from the main thread, before the worker threads exist: they inherit the mask */
    R->t_join = now_s() - t0;
    if (!R->overlap) {
        if (R->ld->ready == 0) exit_message("No query files provided"); /* slamem.c:648 */
        printf("> %d reference%s and %d quer%s successfully loaded\n", R->ref.num, R->ref.num == 1 ? "" : "s", R->ld->total_queries,
               R->ld->total_queries == 1 ? "y" : "ies");
    }
    if (R->p.o.min_mem_len < 1) exit_message("Minimum match length must be at least 1");
}

/* the "Using options" line of GetMatches (slamem.c:37-218), and the output file */
static void open_output(run_t *R) {
    const slh_run *p = &R->p;
    const int t = p->o.match_type, gap = p->max_gap > 0 ? p->max_gap : 5000, pen = p->ext_pen > 0 ? p->ext_pen : 4;
    const int xdrop = p->ext_xdrop >= 0 ? p->ext_xdrop : 20;
    if (p->o.out_arg == -1) R->out_name = slh_append_to_basename(R->argv[p->o.file_args[0]], "-mems.txt");
    else R->out_name = R->argv[p->o.out_arg];
    say("> Using options: minimum %s length = %d ; strand = %s", MATCH_NAME(t), p->o.min_mem_len,
        p->o.both_strands == 0 ? "forward only" : "forward + reverse");
    if (p->max_occ > 0) say(" ; maximum occurrences = %d", p->max_occ);
    if (t == 4) say(" ; maximum gap = %d", gap);
    if (t == 5) say(" ; mismatch penalty = %d ; X-drop = %d", pen, xdrop);
    if (t == 6 || t == 7 || t == 8)
        say(" ; maximum gap = %d ; mismatch penalty = %d ; X-drop = %d ; maximum edits = %d", gap, pen, xdrop, p->max_edits >= 0 ? p->max_edits : 31);
    if (R->affine) say(" ; gap costs = %d,%d,%d", R->costs[0], R->costs[1], R->costs[2]);
    if (R->gext) say(" ; end band = %d", R->gext);
    if (t == 8 || R->stats) say(" ; minimum mapping quality = %d", p->min_mapq);
    if (p->bq_given == 1) say(" ; minimum base quality = %d", p->min_bq); /* (only when asked for: the line of a run without -bq stays) */
    if (p->gt) say(" ; minimum depth = %d ; ploidy = %d ; error rate = %d Phred ; prior = %d Phred ; minimum quality = %d", p->min_depth, p->gt_ploidy, p->gt_err, p->gt_hetq, p->gt_qual);
    else if (p->sites || p->vcf) say(" ; minimum depth = %d ; minimum share = %d %%", p->min_depth, p->min_pct);
    if (R->sb) say(" ; strand bias = on");
    if (R->sb && R->fs >= 0) say(" ; maximum FS = %d", R->fs);
    if (R->wq) say(" ; base qualities in the likelihood = on");
    if (p->cons) say(" ; minimum depth = %d", p->min_depth);
    if (p->depth) say(" ; covered from depth = %d", p->min_depth);
    if (R->sv) say(" ; sv min = %d", R->sv_min);
    say("\n");
    R->out = fopen(R->out_name, "w");
    if (!R->out) {
        release_stdout();
        printf("\n> ERROR: Cannot create output file <%s>\n", R->out_name);
        join_warmup();
        exit(-1);
    }
}

static void report_index(run_t *R) {
    const build_job *bj = &R->bj;
    const slamem_index_info *info = &bj->info;
    const slamem_timings *tm = &bj->tm;
    const slamem_sslcp_stats *st = &bj->st;
    const unsigned bwt_len = info->bwt_size;
    say("> Building index for reference sequence");
    if (R->ref.num == 1) say(" \"%s\"", R->ref.recs[0].name);
    else say("s");
    say(" (%u Mbp) ...\n", (unsigned)(R->ref.total / 1000000U));
    if (!g_mo) fflush(stdout);
    if (bj->rc != SLAMEM_OK) gpu_fail_msg("index construction on the GPU", bj->rc, bj->err);
    say("> Suffix sort + BWT + LCP + parent links on GPU %d ... OK (%.3f s, overlapped with the loading of the queries; device %.1f ms: sort %.1f, BWT %.1f, LCP %.1f, links %.1f; %u doubling rounds)\n",
        R->device, bj->seconds, tm->build_total_ms, tm->build_sort_ms, tm->build_bwt_ms, tm->build_lcp_ms, tm->build_links_ms, info->sort_rounds);
    say(":: Index size = %.1f MB in HBM (%s layout)\n", (double)info->arena_bytes / 1e6, info->layout == SLAMEM_LAYOUT_COMPACT ? "compact" : "full");
    /* the statistics lines of BuildSampledLCPArray (lcparray.c:709-711, 999-1000), from the per-row records */
    if (bj->rc_stats != SLAMEM_OK) gpu_fail_msg("LCP sampling statistics", bj->rc_stats, bj->err);
    say(":: %.2lf%% samples (%u of %u)\n", ((double)st->num_samples / (double)bwt_len) * 100.0, (unsigned)st->num_samples, bwt_len);
    say(":: %.2lf%% oversized samples (%d of %u)\n", ((double)st->num_oversized_lcp / (double)st->num_samples) * 100.0,
        (int)st->num_oversized_lcp, (unsigned)st->num_samples);
    say(":: Average LCP value = %d (max=%lld)\n", (int)(st->sum_lcp / (long long)bwt_len), (long long)st->max_lcp);
    say(":: %.2lf%% oversized values (%d of %u)\n", ((double)st->num_oversized_links / (double)st->num_samples) * 100.0,
        (int)st->num_oversized_links, (unsigned)st->num_samples);
    say(":: Average SV distance = %.2lf (max=%lld)\n", (double)st->sum_link_distance / (double)st->num_samples, (long long)st->max_link_distance);
}

/* SLAMEM_GPUS=N: replicate the index to N GPUs (device, device+1, ...) with one RCCL broadcast of its arena over xGMI; every
 * batch then goes to one of them (no data-path collective).  SLAMEM_LOGICAL_GPUS=N (self-test): N "GPUs" that are all this
 * device, each with its own copy of the index. */
static void replicate_index(run_t *R) {
    typedef int (*replicate_fn)(const slamem_index *, const int *, int, int, slamem_index **);
    const double t0 = now_s();
    const char *env;
    int logical = 0, devs[16], g, rc = SLAMEM_OK;
    R->gpus[0] = R->bj.idx;
    R->ngpu = 1;
    if ((env = getenv("SLAMEM_GPUS")) != NULL) {
        int avail = 0;
        slamem_device_count(&avail);
        R->ngpu = atoi(env) <= 0 ? avail - R->device : atoi(env);
        if (R->ngpu < 1) R->ngpu = 1;
        if (R->ngpu > 16) R->ngpu = 16;
        if (R->device + R->ngpu > avail) exit_message("SLAMEM_GPUS asks for more GPUs than are visible");
    } else if ((env = getenv("SLAMEM_LOGICAL_GPUS")) != NULL && atoi(env) > 1) {
        R->ngpu = atoi(env) > 16 ? 16 : atoi(env);
        logical = 1;
    }
    if (R->ngpu > 1 || getenv("SLAMEM_REPLICATE_SELFTEST") != NULL) {
        /* libslamem_rccl.so (and RCCL behind it, hundreds of MB of code) is loaded only when it is needed: a one-GPU run
           never pays for it at start-up */
        void *h = dlopen("libslamem_rccl.so", RTLD_NOW | RTLD_GLOBAL);
        replicate_fn fn = h ? (replicate_fn)dlsym(h, "slamem_index_replicate") : NULL;
        for (g = 0; g < R->ngpu; g++) devs[g] = logical ? R->device : R->device + g;
        if (!fn) {
            release_stdout();
            printf("\n> ERROR: cannot load libslamem_rccl.so (%s)\n", dlerror());
            join_warmup();
            exit(-1);
        }
        if (logical) /* one one-rank broadcast into a fresh arena per logical GPU: the scheduling of the batches is the real N-GPU one */
            for (g = 1; g < R->ngpu && rc == SLAMEM_OK; g++) rc = fn(R->gpus[0], devs, 1, 1, &R->gpus[g]);
        else rc = fn(R->gpus[0], devs, R->ngpu, R->ngpu == 1, R->gpus);
        if (rc != SLAMEM_OK) gpu_fail("index replication over RCCL", rc);
        if (R->ngpu == 1) slamem_index_free(R->bj.idx); /* self-test: search on the broadcast copy */
        say("> Index replicated to %d %sGPU%s by RCCL broadcast ... OK (%.3f s)\n", R->ngpu, logical ? "logical " : "",
            R->ngpu == 1 ? " (self-test copy)" : "s", now_s() - t0);
    }
    if (R->p.o.match_type != 8) { /* (-pile prints the reference letter of every row: it keeps the text) */
        free(R->ref.chars); /* the reference frees the text here too (slamem.c:75-77) */
        R->ref.chars = NULL;
    }
    say("> Matching query sequences against index ...\n");
    if (!g_mo) fflush(stdout);
}

/* the batches of the query sets that have come in since the last call: records [first,last) of one set each */
static void add_ranges_of_new_sets(run_t *R, int sets_ready) {
    for (; R->sets_seen < sets_ready; R->sets_seen++) {
        const slh_seqset *q = &R->qsets[R->sets_seen];
        int first = 0;
        while (first < q->num) {
            int last = first;
            const uint64_t base = q->offsets[first];
            /* the first batches are short, so that the search starts early */
            const uint64_t limit = R->nranges < (size_t)R->ngpu ? R->batch_bytes / 4 : R->nranges < 2 * (size_t)R->ngpu ? R->batch_bytes / 2 : R->batch_bytes;
            while (last < q->num && (last == first || q->offsets[last + 1] - base <= limit)) last++;
            if (R->nranges == R->cap_ranges) {
                R->cap_ranges = R->cap_ranges ? R->cap_ranges * 2 : 16;
                R->ranges = (batch_range *)realloc(R->ranges, R->cap_ranges * sizeof(batch_range));
                if (!R->ranges) pipeline_fail("Out of memory");
            }
            R->ranges[R->nranges].f = R->sets_seen; R->ranges[R->nranges].first = first; R->ranges[R->nranges].last = last;
            if (q->offsets[last] - base > R->max_chars) R->max_chars = q->offsets[last] - base;
            if ((uint32_t)(last - first) > R->max_recs) R->max_recs = (uint32_t)(last - first);
            R->nranges++;
            first = last;
        }
    }
}

/* The writer thread, and a search stream per GPU with the options of the mode: batch b is searched on GPU b mod ngpu.  A stream
 * counts for shutdown_pipeline from the moment it exists, so that a failure of its set-up tears it down too. */
static void open_streams(run_t *R) {
    const slh_run *p = &R->p;
    const int t = p->o.match_type;
    const uint32_t xdrop = p->ext_xdrop >= 0 ? (uint32_t)p->ext_xdrop : SLAMEM_EXT_XDROP_DEFAULT;
    const double t0 = now_s();
    int g;
    R->max_chars = R->max_recs = 1;
    add_ranges_of_new_sets(R, R->ld->ready); /* (!overlap: everything is there) */
    if (R->overlap) { /* the batches are not known yet: reserve for a piece's worth, the slots grow on demand */
        const uint64_t guess = R->batch_bytes < (uint64_t)R->piece_bytes ? R->batch_bytes : (uint64_t)R->piece_bytes;
        if (R->max_chars < guess) R->max_chars = guess;
        if (R->max_recs < R->max_chars / 64) R->max_recs = (uint32_t)(R->max_chars / 64);
    }
    memset(&g_writer, 0, sizeof(g_writer));
    g_writer.out = R->out;
    pthread_mutex_init(&g_writer.mu, NULL);
    pthread_cond_init(&g_writer.cv, NULL);
    if (p->sam) { /* the header, once, in front of the first batch's lines */
        slh_buffer hd = {0, 0, 0};
        if (slh_format_sam_header(&hd, R->ref.recs, R->ref.num)) pipeline_fail("Out of memory");
        if (fwrite(hd.data, 1, hd.len, R->out) != hd.len) pipeline_fail("Cannot write output file");
        slh_buffer_free(&hd);
    }
    g_writer.started = pthread_create(&g_writer.tid, NULL, writer_run, &g_writer) == 0;
    for (g = 0; g < R->ngpu && (R->nranges || R->overlap); g++) {
        slamem_stream *s;
        int rc = slamem_stream_create(R->gpus[g], STREAM_SLOTS, R->max_chars, R->max_recs, p->o.both_strands, t, &g_streams[g]);
        if (rc != SLAMEM_OK) pipeline_gpu_fail("setting up the search pipeline", rc);
        g_nstreams = g + 1;
        s = g_streams[g];
        if (p->max_occ > 0) rc = slamem_stream_set_max_occ(s, (uint32_t)p->max_occ);
        if (rc == SLAMEM_OK && t == 8) { /* one accumulator per GPU: the tables are added when the file is written */
            rc = slamem_pileup_create(R->gpus[g], &R->piles[g]);
            if (rc == SLAMEM_OK && R->sb) rc = slamem_pileup_enable_strands(R->piles[g]);
            if (rc == SLAMEM_OK && R->wq) rc = slamem_pileup_enable_quals(R->piles[g]);
            if (rc == SLAMEM_OK && (p->vcf || p->cons)) rc = slamem_pileup_enable_events(R->piles[g], p->ev_slots);
            if (rc == SLAMEM_OK && R->sv) rc = slamem_pileup_enable_junctions(R->piles[g], R->sv_slots, (uint32_t)R->sv_mis);
            if (rc == SLAMEM_OK && p->dedup) rc = slamem_pileup_enable_dedup(R->piles[g], p->dd_slots);
            if (rc == SLAMEM_OK) rc = slamem_stream_set_pileup(s, R->piles[g], (uint32_t)p->min_mapq);
            if (rc == SLAMEM_OK && p->dedup) rc = slamem_stream_set_dedup(s, 1);
            if (rc == SLAMEM_OK && R->wq) rc = slamem_stream_set_quals(s, 33);
        }
        if (rc == SLAMEM_OK && (t == 6 || t == 7 || t == 8 || (t == 4 && p->max_gap > 0))) rc = slamem_stream_set_max_gap(s, (uint32_t)p->max_gap);
        if (rc == SLAMEM_OK && (t == 5 || t == 6 || t == 7 || t == 8)) rc = slamem_stream_set_ext_params(s, (uint32_t)p->ext_pen, xdrop);
        if (rc == SLAMEM_OK && (t == 6 || t == 7 || t == 8))
            rc = slamem_stream_set_max_edits(s, slh_aln_word(p->max_edits, R->affine, R->costs[0], R->costs[1], R->costs[2]));
        if (rc == SLAMEM_OK && R->gext) rc = slamem_stream_set_end_band(s, (uint32_t)R->gext);
        if (rc == SLAMEM_OK && p->sam) rc = slamem_stream_set_md(s, 1); /* every batch also goes through the MD pass */
        if (rc == SLAMEM_OK && R->stats) { /* one table per GPU: they are added up before the report */
            rc = slamem_stats_create(R->gpus[g], &R->tables[g]);
            if (rc == SLAMEM_OK) rc = slamem_stream_set_stats(s, R->tables[g], (uint32_t)p->min_mapq, 1);
        }
        if (rc != SLAMEM_OK) pipeline_gpu_fail("setting up the search pipeline", rc);
        R->inflight[g] = 0;
    }
    R->t_streams = now_s() - t0;
}

/* keep every GPU's pipeline full: slots - 1 batches in flight beside the result being formatted */
static void submit_batches(run_t *R, size_t *submitted) {
    for (; *submitted < R->nranges && R->inflight[*submitted % (size_t)R->ngpu] < STREAM_SLOTS - 1; (*submitted)++) {
        const batch_range *br = &R->ranges[*submitted];
        const slh_seqset *qs = &R->qsets[br->f];
        const uint64_t *qmask = R->ld->masks[br->f];
        slamem_stream *s = g_streams[*submitted % (size_t)R->ngpu];
        const uint32_t nrec = (uint32_t)(br->last - br->first), min_len = (uint32_t)R->p.o.min_mem_len;
        /* -bq N on FASTQ reads: the set's mask is indexed as its letters, the stream takes the batch's words */
        /* -wq: the set's quality bytes beside its letters, indexed as they are */
        const char *sq = R->stats ? R->ld->quals[br->f] : NULL; /* -stats: a FASTQ set's bytes feed the quality sections */
        const int rc = sq ? slamem_stream_submit_quals(s, qs->chars, (const uint8_t *)sq, NULL, qs->offsets + br->first, nrec, min_len)
                     : R->wq ? slamem_stream_submit_quals(s, qs->chars, (const uint8_t *)R->ld->quals[br->f], qmask, qs->offsets + br->first, nrec, min_len)
                     : qmask ? slamem_stream_submit_masked(s, qs->chars, qmask, qs->offsets + br->first, nrec, min_len)
                             : slamem_stream_submit(s, qs->chars, qs->offsets + br->first, nrec, min_len);
        if (rc != SLAMEM_OK) pipeline_gpu_fail("MEM search on the GPU", rc);
        if (R->stats && !sq) R->stats_fasta = 1;
        R->inflight[*submitted % (size_t)R->ngpu]++;
    }
}

/* the next batch's results of stream s; 0: the batch is in its GPU's pileup and nothing came back to format */
static int fetch_batch(run_t *R, size_t bi, batch_view *v) {
    const int t = R->p.o.match_type, g = (int)(bi % (size_t)R->ngpu);
    slamem_stream *s = g_streams[g];
    const uint32_t *seg_eq = NULL;
    uint64_t nops = 0, nmd = 0;
    int rc = slamem_stream_next(s, &v->mems, &v->boff, &v->total, NULL, NULL);
    if (rc != SLAMEM_OK) {
        char detail[512];
        snprintf(detail, sizeof(detail), "%s", slamem_last_error_message());
        shutdown_pipeline();
        release_stdout();
        printf("\n> ERROR: MEM search on GPU %d failed: %s (%s)\n", R->device + g, slamem_strerror(rc), detail);
        join_warmup();
        exit(-1);
    }
    if (t == 8 || R->stats) return 0; /* (-stats: the batch is in its GPU's table) */
    if (t == 5 && (rc = slamem_stream_mismatches(s, &v->mism)) != SLAMEM_OK) /* the fourth column of this batch's rows */
        pipeline_gpu_fail("MEM extension on the GPU", rc);
    if ((t == 6 || t == 7) && (rc = slamem_stream_alns(s, &v->segs, &v->ops, &v->ooff, &nops)) != SLAMEM_OK) /* the segments stand in the place of the rows */
        pipeline_gpu_fail("alignment on the GPU", rc);
    if (t == 7 && (rc = slamem_stream_maps(s, &v->reads)) != SLAMEM_OK) /* ... and the offsets are per read */
        pipeline_gpu_fail("mapping on the GPU", rc);
    /* -sam: the MD entries and the primary segments came with them (seg_eq and nmd are what the interface hands out beside them:
       the writer needs neither, the primary segment is already chosen) */
    if (R->p.sam && (rc = slamem_stream_md(s, &v->md, &v->mdoff, &seg_eq, &v->prim, &nmd)) != SLAMEM_OK)
        pipeline_gpu_fail("the MD pass on the GPU", rc);
    return 1;
}

/* The first strand blocks get their ':: "name" ....' line (slamem.c:97,101,203) and are formatted here; the rest of the batch
 * is formatted by all host threads, in chunks taken from a shared counter, and handed to the writer in order. */
static void format_batch(run_t *R, const batch_view *v, uint64_t nblk) {
    const slh_seqset *q = v->q;
    uint64_t bseq = 0, b, per;
    int nthr = slh_thread_count(), njobs, t;
    fmt_job *jobs;
    pthread_t *tid;
    fmt_queue fq;
    double fmt_t0, fmt_longest = 0, fmt_latest_start = 0;
    if (R->log_limit == 0) bseq = nblk;
    else if (R->printed < R->log_limit) bseq = (uint64_t)(R->log_limit - R->printed) < nblk ? (uint64_t)(R->log_limit - R->printed) : nblk;
    for (b = 0; b < bseq; b++) {
        const int ri = v->first_rec + (int)(b / (uint64_t)v->strands), sidx = (int)(b % (uint64_t)v->strands);
        uint64_t cnt, sum;
        int d, dots;
        if (format_block(v, b, &R->buf, &cnt, &sum)) pipeline_fail("Out of memory");
        R->total_matches += (long long)cnt;
        R->total_sum += (long long)sum;
        dots = slh_progress_dots(q->recs[ri].size);
        say(":: \"%s%s\" ", q->recs[ri].name, sidx ? " Reverse" : "");
        for (d = 0; d < dots; d++) fputc('.', g_mo ? g_mo : stdout);
        say(" (%d %ss ; avg size = %d bp)\n", (int)cnt, MATCH_NAME(R->p.o.match_type), (int)(cnt ? sum / cnt : 0));
        R->printed++;
    }
    if (writer_push(&g_writer, &R->buf)) pipeline_fail("Out of memory");
    if (bseq == nblk) return;
    fmt_t0 = now_s();
    if ((nblk - bseq) < 4096 || nthr < 1) nthr = 1;
    njobs = (int)((nblk - bseq + 32767) / 32768); /* chunks of 32 k strand blocks, at least one per thread */
    if (njobs < nthr) njobs = nthr;
    jobs = (fmt_job *)calloc((size_t)njobs, sizeof(fmt_job));
    tid = (pthread_t *)calloc((size_t)nthr, sizeof(pthread_t));
    if (!jobs || !tid) pipeline_fail("Out of memory");
    per = (nblk - bseq + (uint64_t)njobs - 1) / (uint64_t)njobs;
    for (t = 0; t < njobs; t++) {
        jobs[t].v = v;
        jobs[t].b0 = bseq + per * (uint64_t)t < nblk ? bseq + per * (uint64_t)t : nblk;
        jobs[t].b1 = jobs[t].b0 + per < nblk ? jobs[t].b0 + per : nblk;
    }
    fq.jobs = jobs; fq.njobs = njobs; fq.next = 0;
    for (t = 0; t + 1 < nthr; t++)
        if (pthread_create(&tid[t], NULL, fmt_worker, &fq) != 0) tid[t] = 0;
    fmt_worker(&fq); /* the main thread takes chunks too */
    for (t = 0; t + 1 < nthr; t++)
        if (tid[t]) pthread_join(tid[t], NULL);
    for (t = 0; t < njobs; t++) {
        if (jobs[t].failed) pipeline_fail("Out of memory");
        g_fmt_busy += jobs[t].t_end - jobs[t].t_start;
        if (jobs[t].t_end - jobs[t].t_start > fmt_longest) fmt_longest = jobs[t].t_end - jobs[t].t_start;
        if (jobs[t].t_start - fmt_t0 > fmt_latest_start) fmt_latest_start = jobs[t].t_start - fmt_t0;
        R->total_matches += jobs[t].matches;
        R->total_sum += jobs[t].sum;
        if (writer_push(&g_writer, &jobs[t].buf)) pipeline_fail("Out of memory");
    }
    free(jobs);
    free(tid);
    g_fmt_longest += fmt_longest;
    g_fmt_latest_start += fmt_latest_start;
}

/* The pipeline over the list of batches: the GPUs search batches b+1.. (slamem_stream_*: upload, search and download of
 * neighbouring batches overlap), the main thread formats batch b with all host threads, the writer thread writes batch b-1. */
static void run_batches(run_t *R) {
    loader_t *ld = R->ld;
    size_t bi, submitted = 0;
    int sets_reaped = 0;
    for (bi = 0;; bi++) {
        batch_view v;
        const batch_range *br;
        double tg;
        if (R->overlap) { /* take in the pieces parsed meanwhile; wait for one only when there is nothing else to do */
            const double tw = now_s();
            int sets_ready, finished;
            pthread_mutex_lock(&ld->mu);
            while (bi >= R->nranges && R->sets_seen == ld->ready && !ld->done) pthread_cond_wait(&ld->cv, &ld->mu);
            sets_ready = ld->ready;
            pthread_mutex_unlock(&ld->mu);
            add_ranges_of_new_sets(R, sets_ready);
            R->t_wait_load += now_s() - tw;
            if (bi >= R->nranges) { /* nothing new: either the loader is done or a piece without batches came in */
                pthread_mutex_lock(&ld->mu);
                finished = ld->done && R->sets_seen == ld->ready;
                pthread_mutex_unlock(&ld->mu);
                if (finished) break;
                bi--;
                continue;
            }
        } else if (bi >= R->nranges) break;
        br = &R->ranges[bi];
        for (; ld->release_early && sets_reaped < br->f; sets_reaped++) /* every batch of the earlier sets is formatted */
            if (R->qsets[sets_reaped].chars) {
                reap_set(&R->qsets[sets_reaped]); free(ld->masks[sets_reaped]); ld->masks[sets_reaped] = NULL;
                free(ld->quals[sets_reaped]); ld->quals[sets_reaped] = NULL;
            }
        tg = now_s();
        submit_batches(R, &submitted);
        memset(&v, 0, sizeof(v));
        v.q = &R->qsets[br->f];
        v.ref = &R->ref;
        v.quals = ld->quals[br->f];
        v.first_rec = br->first;
        v.strands = R->strands;
        if (!fetch_batch(R, bi, &v)) R->total_matches += (long long)v.total; /* (the segments piled) */
        R->inflight[bi % (size_t)R->ngpu]--;
        R->t_gpu += now_s() - tg; /* time the main thread waited for the GPUs */
        if (R->p.o.match_type == 8 || R->stats) continue;
        tg = now_s();
        format_batch(R, &v, (uint64_t)(br->last - br->first) * (uint64_t)R->strands);
        if (g_writer.failed) pipeline_fail("Cannot write output file");
        R->t_format += now_s() - tg;
    }
    free(R->ranges);
    R->ranges = NULL;
}

/* the loader is done: the "successfully loaded" line, then what was held back, and what it found wrong with the query files */
static void check_loader(run_t *R) {
    loader_t *ld = R->ld;
    release_stdout();
    R->total_queries = ld->total_queries;
    if (ld->failed) pipeline_fail("Internal error: the query files came in more pieces than planned");
    if (ld->invalid || ld->ready == 0) {
        shutdown_pipeline();
        fclose(R->out);
        remove(R->out_name);
        /* the loader thread met a query file that is no valid FASTQ (it said so), or ran out of memory; or slamem.c:648 (an
           overlapped run only knows it now) */
        exit_message(ld->invalid == 1 ? "A query file is not valid FASTQ" : ld->invalid ? "Out of memory" : "No query files provided");
    }
    if (ld->fasta_filled) fprintf(stderr, "> NOTE: option -wq: FASTA queries carry no base qualities: their letters count with the quality of -err, %d\n", R->p.gt_err);
    if (R->stats_fasta) fprintf(stderr, "> NOTE: option -stats: FASTA queries carry no base qualities: the per-quality rows (BQ) count the FASTQ queries only\n");
    if (ld->fasta_seen) fprintf(stderr, "> WARNING: option -bq %d has no effect on FASTA queries: they carry no base qualities\n", R->p.min_bq);
}

/* ------------------------------------------------------------------------------------------------ */
/* the read-outs of the pileup: GPU 0's table, range after range of readout_rows rows                */
/* ------------------------------------------------------------------------------------------------ */

/* A read-out that has more to hand back than there is room for says SLAMEM_ERR_CAPACITY and how much: it is asked once more
 * with that room.  bufs: the arrays the call fills, *cap elements each; one that is NULL is allocated, and all are released
 * before they grow. */
typedef struct { void **p; size_t elem; int big; } grow_buf;
typedef int (*fetch_fn)(void *ctx, uint64_t cap, uint64_t *total);
static int fetch_growing(uint64_t *cap, const grow_buf *bufs, int nbufs, fetch_fn call, void *ctx, uint64_t *total) {
    for (;;) {
        int k, rc;
        for (k = 0; k < nbufs; k++)
            if (*cap && !*bufs[k].p) {
                const size_t bytes = (size_t)*cap * bufs[k].elem;
                if (!(*bufs[k].p = bufs[k].big ? slh_big_malloc(bytes) : malloc(bytes))) pipeline_fail("Out of memory");
            }
        rc = call(ctx, *cap, total);
        if (rc != SLAMEM_ERR_CAPACITY || *total <= *cap) return rc;
        for (k = 0; k < nbufs; k++) { free(*bufs[k].p); *bufs[k].p = NULL; }
        *cap = *total;
    }
}

/* the pieces of the records inside rows [x0, x0 + cnt), in R->pcs; *r goes on to the record the next range begins with */
static int pieces_of_range(run_t *R, int *r, uint64_t x0, uint64_t cnt) {
    uint64_t x = x0;
    int m = 0;
    while (slh_next_piece(R->ref.recs, R->ref.merged_start, R->ref.num, r, &x, x0 + cnt, &R->pcs[m])) m++;
    return m;
}

typedef struct { /* a range of a pileup and where its events go */
    slamem_pileup *pile;
    uint64_t x0, cnt, sk[3];
    slamem_event *evs;
} events_call;
static int fetch_events(void *ctx, uint64_t cap, uint64_t *total) {
    events_call *c = (events_call *)ctx;
    return slamem_pileup_events_host(c->pile, c->x0, c->cnt, 1, cap, c->evs, c->sk, total);
}

typedef struct { /* a range of a pileup and where its junctions go */
    slamem_pileup *pile;
    uint64_t x0, cnt, sk[4];
    uint32_t min_len;
    slamem_junction *jns;
} junctions_call;
static int fetch_junctions(void *ctx, uint64_t cap, uint64_t *total) {
    junctions_call *c = (junctions_call *)ctx;
    return slamem_pileup_junctions_host(c->pile, c->x0, c->cnt, 1, c->min_len, cap, c->jns, c->sk, total);
}

#define FOR_RANGES(x0, cnt) for (x0 = 0; x0 < n && (cnt = n - x0 < R->readout_rows ? n - x0 : R->readout_rows) > 0; x0 += R->readout_rows)

/* the tables of GPUs 1.. are added into GPU 0's, and their events, which arrive normalised and stay as they are */
static void merge_gpu_tables(run_t *R) {
    const uint64_t n = R->ref.total;
    const int with_events = R->p.vcf || R->p.cons;
    uint64_t x0, cnt, ecap = 1ull << 16, total;
    events_call ec;
    const grow_buf ebufs[1] = {{(void **)&ec.evs, sizeof(slamem_event), 0}};
    uint32_t *rows;
    int g, rc;
    if (g_nstreams < 2) return;
    memset(&ec, 0, sizeof(ec));
    rows = (uint32_t *)slh_big_malloc((size_t)(R->readout_rows < n ? R->readout_rows : n) * 24 + 24);
    if (!rows) pipeline_fail("Out of memory");
    for (g = 1; g < g_nstreams; g++)
        FOR_RANGES(x0, cnt) {
            rc = slamem_pileup_counts_host(R->piles[g], x0, cnt, rows);
            if (rc == SLAMEM_OK) rc = slamem_pileup_add_counts_host(R->piles[0], x0, cnt, rows);
            if (rc != SLAMEM_OK) pipeline_gpu_fail("adding up the pileups of the GPUs", rc);
        }
    for (g = 1; R->sb && g < g_nstreams; g++) { /* -sb: the forward accumulators, exactly as their owners */
        slamem_pileup *to = NULL, *from = NULL;
        rc = slamem_pileup_forward(R->piles[0], &to);
        if (rc == SLAMEM_OK) rc = slamem_pileup_forward(R->piles[g], &from);
        FOR_RANGES(x0, cnt) {
            if (rc == SLAMEM_OK) rc = slamem_pileup_counts_host(from, x0, cnt, rows);
            if (rc == SLAMEM_OK) rc = slamem_pileup_add_counts_host(to, x0, cnt, rows);
        }
        if (rc != SLAMEM_OK) pipeline_gpu_fail("adding up the forward-strand pileups of the GPUs", rc);
    }
    for (g = 1; R->wq && g < g_nstreams; g++) { /* -wq: the quality accumulators, the same way */
        slamem_pileup *to = NULL, *from = NULL;
        rc = slamem_pileup_quality(R->piles[0], &to);
        if (rc == SLAMEM_OK) rc = slamem_pileup_quality(R->piles[g], &from);
        FOR_RANGES(x0, cnt) {
            if (rc == SLAMEM_OK) rc = slamem_pileup_counts_host(from, x0, cnt, rows);
            if (rc == SLAMEM_OK) rc = slamem_pileup_add_counts_host(to, x0, cnt, rows);
        }
        if (rc != SLAMEM_OK) pipeline_gpu_fail("adding up the quality sums of the GPUs", rc);
    }
    free(rows);
    for (g = 1; with_events && g < g_nstreams; g++) {
        FOR_RANGES(x0, cnt) {
            ec.pile = R->piles[g]; ec.x0 = x0; ec.cnt = cnt;
            rc = fetch_growing(&ecap, ebufs, 1, fetch_events, &ec, &total);
            if (rc == SLAMEM_OK) rc = slamem_pileup_add_events_host(R->piles[0], ec.evs, total);
            if (rc != SLAMEM_OK) pipeline_gpu_fail("adding up the indel events of the GPUs", rc);
        }
        R->skipped[0] += ec.sk[0]; R->skipped[1] += ec.sk[1]; R->skipped[2] += ec.sk[2]; /* (what GPU g could not store) */
    }
    free(ec.evs);
    if (R->sv) { /* -sv: the junctions of GPUs 1.., whatever their length; they arrive normalised and stay as they are */
        uint64_t jcap = 1ull << 12;
        junctions_call jc;
        const grow_buf jbufs[1] = {{(void **)&jc.jns, sizeof(slamem_junction), 0}};
        int k;
        memset(&jc, 0, sizeof(jc));
        for (g = 1; g < g_nstreams; g++) {
            jc.pile = R->piles[g]; jc.x0 = 0; jc.cnt = n; jc.min_len = 0;
            rc = fetch_growing(&jcap, jbufs, 1, fetch_junctions, &jc, &total);
            if (rc == SLAMEM_OK) rc = slamem_pileup_add_junctions_host(R->piles[0], jc.jns, total);
            if (rc != SLAMEM_OK) pipeline_gpu_fail("adding up the junctions of the GPUs", rc);
            for (k = 0; k < 4; k++) R->sv_skipped[k] += jc.sk[k]; /* (what GPU g did not store) */
        }
        free(jc.jns);
    }
}

/* -sv: what became of the junctions, on stderr when there is anything to say */
static void report_junctions(run_t *R, const uint64_t sk[4]) {
    uint64_t s[4], total = 0;
    int k;
    if (slamem_pileup_junctions_host(R->piles[0], 0, R->ref.total, 1, 0, 0, NULL, s, &total) != SLAMEM_ERR_CAPACITY) total = 0;
    for (k = 0; k < 4; k++) s[k] = R->sv_skipped[k] + sk[k];
    if (total | R->sv_counts[0] | R->sv_counts[1] | s[0] | s[1] | s[2] | s[3])
        fprintf(stderr, "> Junctions: %llu stored, %llu lines written, %llu at a record's first row left out; not stored: %llu balanced, "
                        "%llu without room in the table%s, %llu with a letter that is none of A,C,G,T, %llu with more than 64 shared letters "
                        "or too many mismatches\n", (unsigned long long)total, (unsigned long long)R->sv_counts[0],
                (unsigned long long)R->sv_counts[1], (unsigned long long)s[0], (unsigned long long)s[1], s[1] ? " (a larger table: -svslots)" : "",
                (unsigned long long)s[2], (unsigned long long)s[3]);
}

/* -vcf, -cons: GPU 0's own counters (the merge included) come on top of the other GPUs' */
static void warn_skipped(run_t *R, const uint64_t sk[3]) {
    const uint64_t s0 = R->skipped[0] + sk[0], s1 = R->skipped[1] + sk[1], s2 = R->skipped[2] + sk[2];
    if (s0 | s1 | s2)
        fprintf(stderr, "> WARNING: indel observations that are in no event: %llu insertions of more than 31 letters, %llu without "
                        "room in the event table, %llu malformed%s\n", (unsigned long long)s0, (unsigned long long)s1,
                (unsigned long long)s2, s1 ? " (a larger table: -evs)" : "");
}

/* -pile: a line per row of a record that has a count; the GPUs' tables are added up here, range after range (24 bytes a row:
 * the table of a 100 Mbp text never sits in one buffer) */
static void write_pile(run_t *R) {
    const uint64_t n = R->ref.total;
    const size_t bytes = (size_t)(R->readout_rows < n ? R->readout_rows : n) * 24 + 24;
    uint32_t *rows = (uint32_t *)slh_big_malloc(bytes), *more = R->ngpu > 1 ? (uint32_t *)slh_big_malloc(bytes) : NULL;
    uint64_t x0, cnt, x, k;
    slh_piece pc;
    int r = 0, g, rc;
    if (!rows || (R->ngpu > 1 && !more)) pipeline_fail("Out of memory");
    FOR_RANGES(x0, cnt) {
        rc = slamem_pileup_counts_host(R->piles[0], x0, cnt, rows);
        for (g = 1; rc == SLAMEM_OK && g < g_nstreams; g++) {
            rc = slamem_pileup_counts_host(R->piles[g], x0, cnt, more);
            for (k = 0; rc == SLAMEM_OK && k < cnt * 6; k++) rows[k] += more[k];
        }
        if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the pileup from the GPU", rc);
        for (x = x0; slh_next_piece(R->ref.recs, R->ref.merged_start, R->ref.num, &r, &x, x0 + cnt, &pc);)
            if (slh_format_pile_rows(&R->buf, R->ref.recs[pc.rec].name, (uint32_t)(pc.a - pc.start) + 1u, R->ref.chars + pc.a,
                                     rows + (pc.a - x0) * 6, pc.b - pc.a))
                pipeline_fail("Out of memory");
        push_text(R);
    }
    free(rows);
    free(more);
}

typedef struct { /* -sites, -vcf: the selected rows of a range */
    run_t *R;
    uint64_t x0, cnt, *pos;
    uint32_t *rows;
    uint8_t *alleles;
    slamem_genotype *gts;
    uint32_t *qsums; /* -wq: four quality sums per selected row */
} sites_call;
static int fetch_sites(void *ctx, uint64_t cap, uint64_t *total) {
    sites_call *c = (sites_call *)ctx;
    const slh_run *p = &c->R->p;
    if (c->R->wq)
        return slamem_pileup_genotypes_weighted_host(c->R->piles[0], c->x0, c->cnt, &c->R->gtp_wq, cap, c->pos, c->rows, c->gts, c->qsums, total);
    return p->gt ? slamem_pileup_genotypes_host(c->R->piles[0], c->x0, c->cnt, &c->R->gtp, cap, c->pos, c->rows, c->gts, total)
                 : slamem_pileup_sites_host(c->R->piles[0], c->x0, c->cnt, SLAMEM_SITES_VARIANT, (uint32_t)p->min_depth,
                                            (uint32_t)p->min_pct, cap, c->pos, c->rows, c->alleles, total);
}

/* -sites, -vcf (with and without -gt): GPU 0 applies the rule to the summed table range after range and only the selected rows
 * come back, a line each; -vcf: with the events of the same range, the pileup rows of their anchors, and the lines of both
 * record by record */
static void write_sites_or_vcf(run_t *R) {
    const slh_run *p = &R->p;
    const slh_seqset *ref = &R->ref;
    const uint64_t n = ref->total;
    uint64_t x0, cnt, cap = 1ull << 20, ecap = 1ull << 16, jcap = 1ull << 12, total, etotal, jtotal, k, ek, e, ee, j, jk, je, *anchors = NULL;
    uint64_t *janchors = NULL; /* -sv: the junctions of the range, their anchor rows pos - 1 and the pileup rows there */
    uint32_t *jrows = NULL;
    junctions_call jc;
    uint32_t *arows = NULL, *frows = NULL, *afrows = NULL; /* -sb: the forward accumulator's rows at the sites and at the anchors */
    slamem_pileup *fwd = NULL;
    slamem_genotype *egts = NULL; /* -gt: the genotypes of the events, and which events are called */
    uint8_t *ecalled = NULL;
    sites_call sc;
    events_call ec;
    const grow_buf sbufs[6] = {{(void **)&sc.pos, 8, 0}, {(void **)&sc.rows, 24, 0}, {(void **)&sc.alleles, 1, 0}, {(void **)&sc.gts, sizeof(slamem_genotype), 0},
                               {(void **)&frows, 24, 0}, {(void **)&sc.qsums, 16, 0}};
    const grow_buf ebufs[6] = {{(void **)&ec.evs, sizeof(slamem_event), 0}, {(void **)&anchors, 8, 0}, {(void **)&arows, 24, 0},
                               {(void **)&egts, sizeof(slamem_genotype), 0}, {(void **)&ecalled, 1, 0}, {(void **)&afrows, 24, 0}};
    const grow_buf jbufs[3] = {{(void **)&jc.jns, sizeof(slamem_junction), 0}, {(void **)&janchors, 8, 0}, {(void **)&jrows, 24, 0}};
    int r = 0, m, pi, rc;
    memset(&sc, 0, sizeof(sc));
    memset(&ec, 0, sizeof(ec));
    memset(&jc, 0, sizeof(jc));
    sc.R = R;
    ec.pile = jc.pile = R->piles[0];
    jc.min_len = (uint32_t)R->sv_min;
    if (R->sb && (rc = slamem_pileup_forward(R->piles[0], &fwd)) != SLAMEM_OK) pipeline_gpu_fail("reading the forward-strand pileup from the GPU", rc);
    if (p->vcf && (R->wq ? slh_format_vcf_wq_header(&R->buf, ref->recs, ref->num, R->sb, R->fs)
                   : R->sb ? slh_format_vcf_sb_header(&R->buf, ref->recs, ref->num, R->fs)
                   : p->gt ? slh_format_vcf_gt_header(&R->buf, ref->recs, ref->num)
                   : R->sv ? slh_format_vcf_sv_header(&R->buf, ref->recs, ref->num) : slh_format_vcf_header(&R->buf, ref->recs, ref->num)))
        pipeline_fail("Out of memory");
    FOR_RANGES(x0, cnt) {
        sc.x0 = ec.x0 = x0;
        sc.cnt = ec.cnt = cnt;
        rc = fetch_growing(&cap, sbufs, R->wq ? 6 : R->sb ? 5 : p->gt ? 4 : 3, fetch_sites, &sc, &total);
        if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the variant sites from the GPU", rc);
        if (R->sb && (rc = slamem_pileup_rows_at_host(fwd, sc.pos, total, frows)) != SLAMEM_OK)
            pipeline_gpu_fail("reading the forward-strand rows of the variant sites from the GPU", rc);
        m = pieces_of_range(R, &r, x0, cnt);
        etotal = 0;
        if (p->vcf) {
            rc = fetch_growing(&ecap, ebufs, R->sb ? 6 : p->gt ? 5 : 3, fetch_events, &ec, &etotal);
            if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the indel events from the GPU", rc);
            for (j = 0, pi = 0; j < etotal; j++) { /* the anchor row: the letter in front, or the event's own row at a record's start */
                const uint64_t x = ec.evs[j].pos;
                while (pi + 1 < m && x >= R->pcs[pi + 1].start) pi++;
                anchors[j] = x > (m ? R->pcs[pi].start : 0) ? x - 1 : x;
            }
            rc = slamem_pileup_rows_at_host(R->piles[0], anchors, etotal, arows);
            if (rc == SLAMEM_OK && R->sb) rc = slamem_pileup_rows_at_host(fwd, anchors, etotal, afrows);
            if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the pileup rows of the indel events from the GPU", rc);
            if (p->gt) { /* every event on its own against everything else at its anchor, on the GPU */
                rc = slamem_pileup_genotype_events_host(R->piles[0], ec.evs, anchors, etotal, &R->gtp, egts, ecalled);
                if (rc != SLAMEM_OK) pipeline_gpu_fail("genotyping the indel events on the GPU", rc);
            }
        }
        jtotal = 0;
        if (R->sv) { /* the junctions of the range and the pileup rows of their anchors (a junction at row 0 has none: any row does) */
            jc.x0 = x0; jc.cnt = cnt;
            rc = fetch_growing(&jcap, jbufs, 3, fetch_junctions, &jc, &jtotal);
            if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the junctions from the GPU", rc);
            for (j = 0; j < jtotal; j++) janchors[j] = jc.jns[j].pos ? jc.jns[j].pos - 1 : 0;
            rc = slamem_pileup_rows_at_host(R->piles[0], janchors, jtotal, jrows);
            if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the pileup rows of the junctions from the GPU", rc);
        }
        for (pi = 0, k = ek = jk = 0; pi < m && (k < total || ek < etotal || jk < jtotal); pi++, k = e, ek = ee, jk = je) { /* the rows and events of one record after the other */
            const slh_piece *pc = &R->pcs[pi];
            const char *name = ref->recs[pc->rec].name;
            const uint32_t size = ref->recs[pc->rec].size;
            while (k < total && sc.pos[k] < pc->start) k++; /* (a separator: no record's row) */
            while (ek < etotal && ec.evs[ek].pos < pc->start) ek++;
            for (e = k; e < total && sc.pos[e] < pc->b; e++) {}
            for (ee = ek; ee < etotal && ec.evs[ee].pos < pc->start + size; ee++) {}
            while (jk < jtotal && jc.jns[jk].pos < pc->start) jk++;
            for (je = jk; je < jtotal && jc.jns[je].pos < pc->start + size; je++) {}
            if (e == k && ee == ek && je == jk) continue;
            if (!p->vcf ? slh_format_site_rows(&R->buf, name, pc->start, ref->chars, sc.pos + k, sc.rows + k * 6, sc.alleles + k, e - k)
                : R->wq ? slh_format_vcf_wq_rows(&R->buf, name, pc->start, size, ref->chars, sc.pos + k, sc.rows + k * 6, frows + k * 6,
                                                 sc.qsums + k * 4, (const slh_genotype *)(sc.gts + k), e - k, (const slh_event *)(ec.evs + ek),
                                                 arows + ek * 6, R->sb ? afrows + ek * 6 : NULL, (const slh_genotype *)(egts + ek), ecalled + ek, ee - ek, R->sb,
                                                 R->fs)
                : R->sb ? slh_format_vcf_sb_rows(&R->buf, name, pc->start, size, ref->chars, sc.pos + k, sc.rows + k * 6, frows + k * 6,
                                                 (const slh_genotype *)(sc.gts + k), e - k, (const slh_event *)(ec.evs + ek), arows + ek * 6,
                                                 afrows + ek * 6, (const slh_genotype *)(egts + ek), ecalled + ek, ee - ek, R->fs)
                : p->gt ? slh_format_vcf_gt_rows(&R->buf, name, pc->start, size, ref->chars, sc.pos + k, sc.rows + k * 6,
                                                 (const slh_genotype *)(sc.gts + k), e - k, (const slh_event *)(ec.evs + ek), arows + ek * 6,
                                                 (const slh_genotype *)(egts + ek), ecalled + ek, ee - ek)
                : R->sv ? slh_format_vcf_sv_rows(&R->buf, name, pc->start, size, ref->chars, sc.pos + k, sc.rows + k * 6, sc.alleles + k, e - k,
                                                 (const slh_event *)(ec.evs + ek), arows + ek * 6, ee - ek, (const slh_junction *)(jc.jns + jk),
                                                 jrows + jk * 6, je - jk, (uint32_t)p->min_depth, (uint32_t)p->min_pct, R->sv_counts)
                        : slh_format_vcf_rows(&R->buf, name, pc->start, size, ref->chars, sc.pos + k, sc.rows + k * 6, sc.alleles + k, e - k,
                                              (const slh_event *)(ec.evs + ek), arows + ek * 6, ee - ek, (uint32_t)p->min_depth,
                                              (uint32_t)p->min_pct))
                pipeline_fail("Out of memory");
        }
        push_text(R);
    }
    free(sc.pos); free(sc.rows); free(sc.alleles); free(sc.gts); free(sc.qsums);
    free(ec.evs); free(anchors); free(arows); free(egts); free(ecalled); free(frows); free(afrows);
    free(jc.jns); free(janchors); free(jrows);
    if (p->vcf) warn_skipped(R, ec.sk);
    if (R->sv) report_junctions(R, jc.sk);
}

typedef struct { /* -cons: the consensus of a range, cut at the bounds */
    run_t *R;
    uint64_t x0, cnt, *bnd, m, *offs, st[5];
    uint8_t *seq;
} cons_call;
static int fetch_consensus(void *ctx, uint64_t cap, uint64_t *total) {
    cons_call *c = (cons_call *)ctx;
    return slamem_pileup_consensus_host(c->R->piles[0], c->x0, c->cnt, (uint32_t)c->R->p.min_depth, cap, c->seq, c->bnd, c->m, c->offs,
                                        c->st, total);
}

/* -cons: GPU 0 builds the consensus of the summed table and events range after range; the bounds cut it at the records' first
 * rows and ends (a separator's row, and an insertion in front of it, is no record's), and a record is written when its last
 * piece is there */
static void write_cons(run_t *R) {
    const slh_seqset *ref = &R->ref;
    const uint64_t n = ref->total, most = R->readout_rows < n ? R->readout_rows : n;
    uint64_t x0, cnt, ccap = most + most / 64 + 64, rlen = 0, rcap = 0, stats[5] = {0, 0, 0, 0, 0}, total, none = 0, j;
    cons_call cc;
    events_call ec;
    const grow_buf bufs[1] = {{(void **)&cc.seq, 1, 1}};
    char *rec = NULL;
    int r = 0, m, pi, rc;
    memset(&cc, 0, sizeof(cc));
    memset(&ec, 0, sizeof(ec));
    cc.R = R;
    cc.bnd = (uint64_t *)malloc(((size_t)ref->num * 2 + 2) * 16);
    if (!cc.bnd) pipeline_fail("Out of memory");
    cc.offs = cc.bnd + (size_t)ref->num * 2 + 2;
    FOR_RANGES(x0, cnt) {
        m = pieces_of_range(R, &r, x0, cnt);
        for (pi = 0; pi < m; pi++) { cc.bnd[2 * pi] = R->pcs[pi].a; cc.bnd[2 * pi + 1] = R->pcs[pi].b; }
        cc.x0 = x0; cc.cnt = cnt; cc.m = 2 * (uint64_t)m;
        rc = fetch_growing(&ccap, bufs, 1, fetch_consensus, &cc, &total);
        if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the consensus from the GPU", rc);
        for (j = 0; j < 5; j++) stats[j] += cc.st[j];
        for (pi = 0; pi < m; pi++) {
            const uint64_t got = cc.offs[2 * pi + 1] - cc.offs[2 * pi];
            if (rlen + got > rcap) {
                char *more;
                rcap = (rlen + got) * 2 + 64;
                if (!(more = (char *)realloc(rec, (size_t)rcap))) pipeline_fail("Out of memory");
                rec = more;
            }
            if (got) memcpy(rec + rlen, cc.seq + cc.offs[2 * pi], (size_t)got);
            rlen += got;
            if (!R->pcs[pi].ends_record) break; /* (the record goes on in the next range) */
            if (slh_format_fasta_record(&R->buf, ref->recs[R->pcs[pi].rec].name, rec ? rec : "", rlen)) pipeline_fail("Out of memory");
            rlen = 0;
        }
        push_text(R);
    }
    free(cc.bnd); free(cc.seq); free(rec);
    fprintf(stderr, "> Consensus: %llu positions uncalled, %llu called unlike the reference, %llu deleted, %llu insertions of %llu letters\n",
            (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[2], (unsigned long long)stats[3],
            (unsigned long long)stats[4]);
    ec.pile = R->piles[0];
    rc = fetch_events(&ec, 0, &none); /* (no event: GPU 0's skipped counters) */
    if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the indel events from the GPU", rc);
    warn_skipped(R, ec.sk);
}

typedef struct { /* -depth: the runs of a range, and the sums at the bounds */
    run_t *R;
    uint64_t x0, cnt, *bnd, m, *cum;
    slamem_depth_run *runs;
} depth_call;
static int fetch_depth_runs(void *ctx, uint64_t cap, uint64_t *total) {
    depth_call *c = (depth_call *)ctx;
    const slh_run *p = &c->R->p;
    return slamem_pileup_depth_runs_host(c->R->piles[0], c->x0, c->cnt, p->levels, (uint32_t)p->num_levels, (uint32_t)p->min_depth, cap,
                                         c->runs, c->bnd, c->m, c->cum, total);
}

/* -win: the windows' borders of a record that lie inside its piece [a, b) */
static uint64_t borders_inside(const slh_piece *pc, uint64_t window) {
    return window ? (pc->b - pc->start - 1) / window - (pc->a - pc->start) / window : 0;
}

/* -depth: GPU 0 turns the summed table into runs of equal depth range after range; the bounds are the first rows and the ends of
 * the records' pieces inside the range (a separator's row is no record's) and with -win the windows' borders between them, and
 * cum at the bounds gives the windows' means and the records' summaries */
static void write_depth(run_t *R) {
    const slh_seqset *ref = &R->ref;
    const uint64_t n = ref->total, window = R->p.window;
    uint64_t x0, cnt, dcap = 1ull << 20, bcap = 0, total, j, ja, need;
    uint64_t rec_sum = 0, rec_cov = 0, wacc = 0; /* of the record so far; -win: of its window that is still open */
    depth_call dc;
    const grow_buf bufs[1] = {{(void **)&dc.runs, sizeof(slamem_depth_run), 1}};
    slh_depth_pending pend = {0, 0, 0, 0};
    slh_buffer sbuf = {0, 0, 0};
    int r = 0, m, pi, rc;
    memset(&dc, 0, sizeof(dc));
    dc.R = R;
    FOR_RANGES(x0, cnt) {
        m = pieces_of_range(R, &r, x0, cnt);
        for (pi = 0, need = 0; pi < m; pi++) need += borders_inside(&R->pcs[pi], window) + 2;
        if (need > bcap) {
            uint64_t *more;
            bcap = need * 2;
            if (!(more = (uint64_t *)realloc(dc.bnd, (size_t)bcap * 8))) pipeline_fail("Out of memory");
            dc.bnd = more;
        }
        for (pi = 0, dc.m = 0; pi < m; pi++) {
            const slh_piece *pc = &R->pcs[pi];
            const uint64_t inside = borders_inside(pc, window);
            dc.bnd[dc.m++] = pc->a;
            for (j = 1; j <= inside; j++) dc.bnd[dc.m++] = pc->start + ((pc->a - pc->start) / window + j) * window;
            dc.bnd[dc.m++] = pc->b;
        }
        free(dc.cum);
        if (!(dc.cum = (uint64_t *)malloc((size_t)(dc.m + 1) * 16))) pipeline_fail("Out of memory");
        dc.x0 = x0; dc.cnt = cnt;
        /* a range of more runs than there is room for says how many: once more with that room */
        rc = window ? fetch_depth_runs(&dc, 0, &total) : fetch_growing(&dcap, bufs, 1, fetch_depth_runs, &dc, &total);
        if (window && rc == SLAMEM_ERR_CAPACITY) rc = SLAMEM_OK; /* (the windows need the sums alone) */
        if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the depth runs from the GPU", rc);
        for (pi = 0, j = 0; pi < m; pi++, j++) {
            const slh_piece *pc = &R->pcs[pi];
            const char *name = ref->recs[pc->rec].name;
            const uint64_t size = ref->recs[pc->rec].size;
            ja = j;
            j += borders_inside(pc, window) + 1; /* (the piece's last bound: the record's end or the range's) */
            if (window) { /* the windows that end in the piece; what is behind the last of them waits for the next range */
                const uint64_t k = j - ja - (pc->ends_record || (pc->b - pc->start) % window == 0 ? 0 : 1);
                const uint64_t sum0 = dc.cum[2 * ja] - wacc;
                if (slh_format_depth_windows(&R->buf, name, size, window, (pc->a - pc->start) / window, sum0, dc.cum + 2 * (ja + 1), k))
                    pipeline_fail("Out of memory");
                wacc = dc.cum[2 * j] - (k ? dc.cum[2 * (ja + k)] : sum0);
            } else if (slh_format_depth_runs(&R->buf, name, pc->start, pc->a, pc->b, (const slh_depth_run *)dc.runs, total, &pend)) {
                pipeline_fail("Out of memory");
            }
            rec_sum += dc.cum[2 * j] - dc.cum[2 * ja];
            rec_cov += dc.cum[2 * j + 1] - dc.cum[2 * ja + 1];
            if (!pc->ends_record) break; /* (the record goes on in the next range) */
            if (slh_format_depth_flush(&R->buf, name, &pend) || slh_format_depth_summary(&sbuf, name, size, rec_cov, rec_sum))
                pipeline_fail("Out of memory");
            rec_sum = rec_cov = wacc = 0;
        }
        push_text(R);
    }
    if (sbuf.len) fwrite(sbuf.data, 1, sbuf.len, stderr);
    slh_buffer_free(&sbuf);
    free(dc.bnd); free(dc.cum); free(dc.runs);
}

/* the read-out of the mode, and the duplicate filter's counters */
static void write_pileup(run_t *R) {
    const slh_run *p = &R->p;
    const double t0 = now_s();
    int rc;
    if (g_nstreams == 0) return;
    if (!(R->pcs = (slh_piece *)malloc(((size_t)R->ref.num + 1) * sizeof(slh_piece)))) pipeline_fail("Out of memory");
    if (p->sites || p->vcf || p->cons || p->depth) merge_gpu_tables(R);
    if (p->cons) write_cons(R);
    else if (p->depth) write_depth(R);
    else if (p->sites || p->vcf) write_sites_or_vcf(R);
    else write_pile(R);
    free(R->pcs);
    R->t_format += now_s() - t0;
    if (p->dedup) { /* (one GPU: its counters are the run's) */
        uint64_t dd[4] = {0, 0, 0, 0};
        rc = slamem_pileup_dedup_stats(R->piles[0], dd);
        if (rc != SLAMEM_OK) pipeline_gpu_fail("reading the duplicate filter's counters from the GPU", rc);
        fprintf(stderr, "> Duplicates: %llu candidate reads, %llu duplicates (%.2f %%) not counted, %llu without room in the duplicate "
                        "table%s\n", (unsigned long long)dd[0], (unsigned long long)dd[1], dd[0] ? 100.0 * (double)dd[1] / (double)dd[0] : 0.0,
                (unsigned long long)dd[2], dd[2] ? " (a larger table: -dslots)" : "");
    }
}

/* -stats: the tables of GPUs 1.. are added into GPU 0's, and the report is written (nothing went through the writer thread) */
static void write_stats(run_t *R) {
    static uint64_t table[SLAMEM_STATS_WORDS];
    const double t0 = now_s();
    int g, rc = SLAMEM_OK;
    if (g_nstreams == 0) memset(table, 0, sizeof(table));
    for (g = 1; g < g_nstreams; g++) {
        rc = slamem_stats_table_host(R->tables[g], table);
        if (rc == SLAMEM_OK) rc = slamem_stats_add_table_host(R->tables[0], table);
        if (rc != SLAMEM_OK) pipeline_gpu_fail("adding up the mapping statistics of the GPUs", rc);
    }
    if (g_nstreams && (rc = slamem_stats_table_host(R->tables[0], table)) != SLAMEM_OK) pipeline_gpu_fail("reading the mapping statistics from the GPU", rc);
    if (slh_write_stats(table, R->out)) pipeline_fail("Cannot write output file");
    R->t_format += now_s() - t0;
}

/* the last lines of stdout, the timing lines, and the end of the process */
static int finish(run_t *R) {
    const slh_run *p = &R->p;
    const int t = p->o.match_type;
    double t_write, t_end0, t_end1;
    char overlap_note[96] = "";
    int i, f;
    writer_finish(&g_writer);
    t_write = g_writer.seconds;
    if (g_writer.failed) pipeline_fail("Cannot write output file");
    if (R->log_limit != 0 && t != 8 && (long)R->total_queries * R->strands > R->log_limit)
        say(":: ... (%ld more strand blocks matched; set SLAMEM_VERBOSE=1 for a line each)\n", (long)R->total_queries * R->strands - R->log_limit);
    t_end0 = now_s();
    if (R->total_queries != 1) /* slamem.c:210-212 (the reference divides by zero when nothing matched) */
        printf(":: Average %d %ss found per query sequence (total = %lld, avg size = %d bp)\n", (int)(R->total_matches / R->total_queries),
               MATCH_NAME(t), R->total_matches, (int)(R->total_matches ? R->total_sum / R->total_matches : 0));
    fflush(stdout);
    printf("> Saving %ss to <%s> ... ", R->stats ? "mapping statistic" : p->depth ? "depth run" : p->cons ? "consensus sequence" : p->vcf ? "variant call" : p->sites ? "variant site" : MATCH_NAME(t), R->out_name);
    if (fflush(R->out) != 0 || ferror(R->out)) exit_message("Cannot write output file");
    if (getenv("SLAMEM_FULL_TEARDOWN") != NULL && fclose(R->out) != 0) exit_message("Cannot write output file");
    t_end1 = now_s();
    printf("OK\n");
    printf("> Done!\n");
    if (g_ld.seconds > 0)
        snprintf(overlap_note, sizeof(overlap_note), " + queries parsed in pieces beside the search in %.3f s (%.3f s waited for)", g_ld.seconds, R->t_wait_load);
    if (R->timing)
        fprintf(stderr, "[timing] formatter threads: busy %.3f s in all; per batch the longest chunk %.3f s, the last chunk started %.3f s after the batch began (sums over the batches)\n",
                g_fmt_busy, g_fmt_longest, g_fmt_latest_start);
    if (R->timing)
        fprintf(stderr, "[timing] load %.3f s%s (index build of %.3f s overlapped; %.3f s more waiting for it), pipeline set-up %.3f s, "
                        "waiting for the GPU (upload + search + download, overlapped with formatting) %.3f s, format %.3f s "
                        "(writer thread busy %.3f s, overlapped; text buffers: %ld recycled, %ld fresh), close %.3f s, total %.3f s\n",
                R->t_load, overlap_note, R->t_build, R->t_join, R->t_streams, R->t_gpu, R->t_format, t_write, g_pool_hits, g_pool_misses,
                t_end1 - t_end0, now_s() - R->t_start);
    fflush(stdout);
    fflush(stderr);
    /* everything is written and nothing runs on the GPU any more: leave without returning gigabytes of buffers and HBM piece by
       piece (0.15-0.25 s of the reference-sized run); the kernel driver reclaims them with the process */
    if (getenv("SLAMEM_FULL_TEARDOWN") == NULL) leave_now();
    {
        double a = now_s(), b, c, d;
        shutdown_pipeline();
        for (i = 0; i < 16 && t == 8; i++) slamem_pileup_free(R->piles[i]);
        for (i = 0; i < 16; i++) slamem_stats_free(R->tables[i]);
        b = now_s();
        for (i = 0; i < R->ngpu; i++) slamem_index_free(R->gpus[i]);
        c = now_s();
        if (p->o.out_arg == -1) free(R->out_name);
        slh_buffer_free(&R->buf);
        slh_free_seqset(&R->ref);
        for (f = 0; f < g_reap_n; f++) pthread_join(g_reap_tid[f], NULL);
        free(g_reap_tid);
        for (f = 0; f < g_ld.ready; f++) { slh_free_seqset(&R->qsets[f]); free(g_ld.masks[f]); }
        free(g_ld.masks);
        free(R->qsets);
        pthread_mutex_lock(&g_pool_mu);
        while (g_pool_n > 0) slh_buffer_free(&g_pool[--g_pool_n]);
        pthread_mutex_unlock(&g_pool_mu);
        d = now_s();
        if (R->timing)
            fprintf(stderr, "[timing] teardown: search pipeline (pinned buffers, device work space) %.3f s, index %.3f s, host buffers %.3f s\n",
                    b - a, c - b, d - c);
    }
    slh_free_options(&R->p.o);
    return 0;
}

int main(int argc, char **argv) {
    static run_t run; /* (zeroed) */
    static int warm_device;
    run_t *R = &run;
    double t0;
    int status;
    R->argc = argc;
    R->argv = argv;
    R->log_limit = 100;
    R->batch_bytes = 256ull << 20;
    R->piece_bytes = 128L << 20;
    R->readout_rows = 16ull << 20;
    printf("[ slaMEM v%s ]\n\n", VERSION);
    if (parse_and_refuse(R, &status)) return status;
    if (getenv("SLAMEM_FULL_TEARDOWN") == NULL) split_off_worker();
    warm_device = R->device;
    g_warm_started = pthread_create(&g_warm_tid, NULL, warmup_run, &warm_device) == 0;
    R->t_start = now_s();
    load_inputs(R);
    join_build(R);
    open_output(R);
    t0 = now_s();
    report_index(R);
    replicate_index(R);
    R->t_build = R->bj.seconds + (now_s() - t0);
    /* (-paf, -pile: what is formatted and counted is a read, whichever strand its mapping lies on) */
    R->strands = (R->p.o.match_type == 7 || R->p.o.match_type == 8) ? 1 : R->p.o.both_strands ? 2 : 1;
    open_streams(R);
    run_batches(R);
    check_loader(R);
    if (R->p.o.match_type == 8) write_pileup(R);
    if (R->stats) write_stats(R);
    return finish(R);
}
