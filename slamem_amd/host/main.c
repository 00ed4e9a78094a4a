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
            mask = ld->keep_quals ? NULL : mask_of_quals(ld, &s, quals);
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

/* formatting of a range of strand blocks of one batch, one range per thread */
typedef struct {
    const slh_seqset *q;
    const slh_seqset *ref;
    const slamem_mem *mems;
    const uint32_t *mism; /* -ext: a fourth column, the mismatches of each row (NULL otherwise) */
    const slamem_aln *segs; /* -aln: the segments in the place of the rows (NULL otherwise), their operations and offsets */
    const uint32_t *ops;
    const uint64_t *ooff;
    const slamem_map *reads; /* -paf: a record per read (NULL otherwise); the blocks are then the reads, strands = 1 */
    const uint32_t *md;      /* -sam: the MD entries of the batch's segments, their offsets per segment, the primary segment per read */
    const uint64_t *mdoff;   /*       (NULL otherwise) */
    const uint32_t *prim;
    const char *quals;       /* -sam: the quality bytes of the set, indexed as its letters (NULL: FASTA) */
    const uint64_t *boff;
    int first_rec, strands;
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

/* a read of the -sam file: read b of the batch is record i of its set */
static int format_sam_read(slh_buffer *buf, const slh_seqset *q, const char *quals, int i, uint64_t b, const slamem_map *reads,
                           const slamem_aln *segs, const uint32_t *ops, const uint64_t *ooff, const uint64_t *boff, const uint32_t *md,
                           const uint64_t *mdoff, const uint32_t *prim, const slh_seqset *ref, uint64_t *sum) {
    return slh_format_read_sam(buf, q->recs[i].name, q->chars + q->offsets[i], quals ? quals + q->offsets[i] : NULL,
                               (uint32_t)(q->offsets[i + 1] - q->offsets[i]), reads[b].strand, reads[b].mapq, reads[b].s1, reads[b].s2,
                               (const uint32_t *)(segs + boff[b]), ops, ooff + boff[b], md, mdoff + boff[b], prim[b],
                               boff[b + 1] - boff[b], ref->recs, ref->merged_start, ref->num, sum);
}

static void *fmt_run(void *arg) {
    fmt_job *j = (fmt_job *)arg;
    uint64_t b;
    j->t_start = now_s();
    /* about 36 characters per MEM line and a header per block: reserve once instead of doubling on the way */
    const size_t need = (size_t)(j->boff[j->b1] - j->boff[j->b0]) * (j->mism ? 44 : 36) + (size_t)(j->b1 - j->b0) * 48 + 4096;
    pool_get(&j->buf, need);
    (void)slh_buffer_reserve(&j->buf, need);
    for (b = j->b0; b < j->b1; b++) {
        int i = j->first_rec + (int)(b / (uint64_t)j->strands), s = (int)(b % (uint64_t)j->strands);
        uint64_t cnt = j->boff[b + 1] - j->boff[b], sum = 0;
        if (j->md ? format_sam_read(&j->buf, j->q, j->quals, i, b, j->reads, j->segs, j->ops, j->ooff, j->boff, j->md, j->mdoff, j->prim,
                                    j->ref, &sum)
            : j->reads ? slh_format_read_paf(&j->buf, j->q->recs[i].name, j->q->recs[i].size, j->reads[b].strand, j->reads[b].mapq,
                                           j->reads[b].s1, j->reads[b].s2, (const uint32_t *)(j->segs + j->boff[b]), j->ops,
                                           j->ooff + j->boff[b], cnt, j->ref->recs, j->ref->merged_start, j->ref->num, &sum)
            : j->segs ? slh_format_block_aln(&j->buf, j->q->recs[i].name, s, (const uint32_t *)(j->segs + j->boff[b]), j->ops,
                                           j->ooff + j->boff[b], cnt, j->ref->recs, j->ref->merged_start, j->ref->num, &sum)
                    : slh_format_block_ext(&j->buf, j->q->recs[i].name, s, (const uint32_t *)(j->mems + j->boff[b]),
                                 j->mism ? j->mism + j->boff[b] : NULL, cnt, j->ref->recs, j->ref->merged_start, j->ref->num, &sum)) {
            j->failed = 1;
            return NULL;
        }
        j->matches += (long long)cnt;
        j->sum += (long long)sum;
    }
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
    printf("\t-evs\twith -vcf: slots of the event table on the GPU, a power of two of at least 64 (default: at least 65536 and a sixteenth of the reference)\n");
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

int main(int argc, char **argv) {
    slh_options o;
    slh_seqset ref, *qsets;
    int i, f, total_queries = 0, device = 0, numbering = 1;
    long log_limit = 100;
    uint64_t batch_bytes = 256ull << 20; /* query characters per batch and GPU */
    long piece_bytes = 128L << 20;       /* bytes of a query file per piece of the loader thread */
    const char *env;
    char *out_name;
    FILE *out;
    slamem_index *idx = NULL, *gpus[16];
    int rc, ngpu = 1, max_occ = 0, max_gap = 0, ext_pen = 0, ext_xdrop = -1, max_edits = -1, min_mapq = 0, min_bq = 0, bq_given = 0;
    int sites = 0, min_depth = 4, min_pct = 20; /* -sites: match type 8 with the sparse read-out */
    int vcf = 0;                                /* -vcf: match type 8 with the events enabled, written as VCF */
    int cons = 0;                               /* -cons: match type 8 with the events enabled, the consensus written as FASTA */
    int sam = 0;                                /* -sam: match type 7 with the MD pass, written as SAM */
    int depth = 0, num_levels = 0, sites_params; /* -depth: match type 8, the runs of the depth written as a bedGraph */
    uint32_t levels[16];
    uint64_t window = 0;
    uint64_t ev_slots = 0;
    int dedup = 0;                              /* -dedup: every batch is added through the duplicate filter */
    int gt = 0, gt_ploidy = 2, gt_err = 20, gt_hetq = 30, gt_qual = 20; /* -gt: -vcf with genotypes, called on the GPU */
    slamem_gt_params gtp;
    uint64_t dd_slots = 0;
    slamem_pileup *piles[16];
    double t0;
    long long total_matches = 0, total_sum = 0;
    slh_buffer buf = {0, 0, 0};
    build_job bj;
    pthread_t build_tid;
    int build_async = 0;

    printf("[ slaMEM v%s ]\n\n", VERSION);
    if (slh_parse_options(argc, argv, &o) != 0) exit_message("Out of memory");
    if (o.usage) { usage(argv[0]); slh_free_options(&o); return -1; }
    if (o.hidden_sort) { /* slamem.c:555-562 */
        slh_free_options(&o);
        if (argc != 3) { printf("Usage: %s -s <mems_file>\n\n", argv[0]); return -1; }
        return slh_sort_mems_file(argv[2], stdout);
    }
    if (o.hidden_clean) { /* slamem.c:563-570 */
        slh_free_options(&o);
        if (argc != 3) { printf("Usage: %s -c <fasta_file>\n\n", argv[0]); return -1; }
        return slh_clean_fasta(argv[2], stdout);
    }
    sites = slh_parse_argument(argc, argv, "SI", 0);
    vcf = slh_parse_argument(argc, argv, "VC", 0);
    cons = slh_parse_argument(argc, argv, "CO", 0);
    depth = slh_parse_depth(argc, argv);
    sam = slh_parse_argument(argc, argv, "SA", 0);
    if (o.match_type < 0) { /* before any GPU work */
        if (sam) exit_message("Option -sam excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites, -vcf, -cons and -depth");
        if (depth) exit_message("Option -depth excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites, -vcf and -cons");
        if (cons) exit_message("Option -cons excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites and -vcf");
        if (vcf) exit_message("Option -vcf excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile and -sites");
        if (sites) exit_message("Option -sites excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf and -pile");
        if (slh_parse_argument(argc, argv, "PI", 0)) exit_message("Option -pile excludes -mam, -mum, -smem, -chain, -ext, -aln and -paf");
        if (slh_parse_argument(argc, argv, "PA", 0)) exit_message("Option -paf excludes -mam, -mum, -smem, -chain, -ext and -aln");
        if (slh_parse_argument(argc, argv, "AL", 0)) exit_message("Option -aln excludes -mam, -mum, -smem, -chain and -ext");
        if (slh_parse_argument(argc, argv, "EX", 0)) exit_message("Option -ext excludes -mam, -mum, -smem and -chain");
        if (slh_parse_argument(argc, argv, "CH", 0)) exit_message("Option -chain excludes -mam, -mum and -smem");
        if (slh_parse_argument(argc, argv, "SM", 0)) exit_message("Option -smem excludes -mam and -mum");
        exit_message("Options -mam and -mum exclude each other");
    }
    switch (slh_parse_max_occ(argc, argv, &max_occ)) {
    case -1: exit_message("Option -occ needs a whole number of at least 1"); break;
    case 1: if (o.match_type != 3) exit_message("Option -occ needs -smem"); break;
    default: break;
    }
    switch (slh_parse_max_gap(argc, argv, &max_gap)) {
    case -1: exit_message("Option -mgap needs a whole number of at least 1"); break;
    case 1: if (o.match_type != 4 && o.match_type != 6 && o.match_type != 7 && o.match_type != 8) exit_message("Option -mgap needs -chain"); break;
    default: break;
    }
    switch (slh_parse_ext_params(argc, argv, &ext_pen, &ext_xdrop)) {
    case -1: exit_message("Option -pen needs a whole number of at least 1, option -xdrop one of at least 0"); break;
    case 1: if (o.match_type != 5 && o.match_type != 6 && o.match_type != 7 && o.match_type != 8) exit_message("Options -pen and -xdrop need -ext"); break;
    default: break;
    }
    switch (slh_parse_max_edits(argc, argv, &max_edits)) {
    case -1: exit_message("Option -maxed needs a whole number from 0 to 127"); break;
    case 1: if (o.match_type != 6 && o.match_type != 7 && o.match_type != 8) exit_message("Option -maxed needs -aln"); break;
    default: break;
    }
    switch (slh_parse_min_mapq(argc, argv, &min_mapq)) {
    case -1: exit_message("Option -minq needs a whole number from 0 to 60"); break;
    case 1: if (o.match_type != 8) exit_message("Option -minq needs -pile"); break;
    default: break;
    }
    switch ((bq_given = slh_parse_min_bq(argc, argv, &min_bq))) {
    case -1: exit_message("Option -bq needs a whole number from 0 to 93"); break;
    case 1: if (o.match_type != 8) exit_message("Option -bq needs -pile"); break;
    default: break;
    }
    switch ((sites_params = slh_parse_sites_params(argc, argv, &min_depth, &min_pct))) {
    case -1: exit_message("Option -mdep needs a whole number of at least 1"); break;
    case -2: exit_message("Option -mpct needs a whole number from 0 to 100"); break;
    case 1:
        if (cons && slh_parse_argument(argc, argv, "MP", 0)) exit_message("Option -mpct has no meaning with -cons: an allele is applied when more than half of the depth shows it");
        if (depth && slh_parse_argument(argc, argv, "MP", 0)) exit_message("Option -mpct has no meaning with -depth: the depth is written as it is");
        if (!sites && !vcf && !cons && !depth) exit_message("Options -mdep and -mpct need -sites");
        break;
    default: break;
    }
    if (depth && sites_params == 0) min_depth = 1; /* (-depth: a position is covered when one read shows it) */
    gt = slh_parse_argument(argc, argv, "GT", 0);
    switch (slh_parse_gt_params(argc, argv, &gt_ploidy, &gt_err, &gt_hetq, &gt_qual)) {
    case -1: exit_message("Option -ploidy needs 1 or 2"); break;
    case -2: exit_message("Option -err needs a whole number from 1 to 93"); break;
    case -3: exit_message("Option -hetq needs a whole number from 0 to 999"); break;
    case -4: exit_message("Option -qual needs a whole number from 0 to 999"); break;
    case 1:
        if (!gt && slh_parse_argument(argc, argv, "PL", 0)) exit_message("Option -ploidy needs -gt");
        if (!gt && slh_parse_argument(argc, argv, "ER", 0)) exit_message("Option -err needs -gt");
        if (!gt && slh_parse_argument(argc, argv, "HE", 0)) exit_message("Option -hetq needs -gt");
        if (!gt) exit_message("Option -qual needs -gt");
        break;
    default: break;
    }
    if (gt && !vcf) exit_message("Option -gt needs -vcf");
    if (gt && slh_parse_argument(argc, argv, "MP", 0)) exit_message("Option -mpct has no meaning with -gt: a call is made when its genotype's quality reaches -qual");
    memset(&gtp, 0, sizeof(gtp));
    if (gt) { /* host arithmetic: the three costs of a letter at the error rate of -err */
        uint32_t costs[3];
        if (slamem_gt_costs((uint32_t)gt_err, costs) != SLAMEM_OK) exit_message("Option -err needs a whole number from 1 to 93");
        gtp.ploidy = (uint32_t)gt_ploidy;
        gtp.match_cost = costs[0];
        gtp.het_cost = costs[1];
        gtp.err_cost = costs[2];
        gtp.het_prior = 1000u * (uint32_t)gt_hetq;
        gtp.min_depth = (uint32_t)min_depth;
        gtp.min_qual = (uint32_t)gt_qual;
    }
    switch (slh_parse_depth_params(argc, argv, levels, &num_levels, &window)) {
    case -1: exit_message("Option -lev needs 1 to 16 whole numbers of at least 1, ascending, separated by commas"); break;
    case -2: exit_message("Option -win needs a whole number of at least 1"); break;
    case 0: break;
    case 3:
        if (depth) exit_message("Options -lev and -win exclude each other");
        /* fall through */
    default: if (!depth) exit_message("Options -lev and -win need -depth"); break;
    }
    switch (slh_parse_event_slots(argc, argv, &ev_slots)) {
    case -1: exit_message("Option -evs needs a power of two of at least 64"); break;
    case 1: if (!vcf && !cons) exit_message("Option -evs needs -vcf"); break;
    default: break;
    }
    switch ((dedup = slh_parse_dedup(argc, argv, &dd_slots))) {
    case -1: exit_message("Option -dslots needs a power of two of at least 64"); break;
    case 2: exit_message("Option -dslots needs -dedup"); break;
    case 0: break;
    default:
        if (o.match_type != 8) exit_message("Option -dedup needs -pile, -sites, -vcf, -cons or -depth");
        /* one table per GPU would miss the duplicates whose copies went to different GPUs */
        if (((env = getenv("SLAMEM_GPUS")) != NULL && atoi(env) != 1) || ((env = getenv("SLAMEM_LOGICAL_GPUS")) != NULL && atoi(env) > 1))
            exit_message("Option -dedup runs on one GPU: every GPU would keep a table of its own and miss the duplicates whose copies went to different GPUs (leave SLAMEM_GPUS unset, or set it to 1)");
        dedup = 1;
        break;
    }
    if (o.num_files < 2) exit_message("Not enough input sequence files provided");
    if (o.ref_name_given && o.ref_name_empty) exit_message("No reference name string provided");
    if ((env = getenv("SLAMEM_DEVICE")) != NULL) device = atoi(env);
    if ((env = getenv("SLAMEM_VERBOSE")) != NULL && atoi(env) != 0) log_limit = 0;
    if (o.image_arg != -1) return image_tool(argc, argv, &o, log_limit); /* slamem.c:652-655; host only, before any GPU call */
    if ((env = getenv("SLAMEM_BATCH_MB")) != NULL && atoll(env) > 0) batch_bytes = (uint64_t)atoll(env) << 20;

    if (getenv("SLAMEM_FULL_TEARDOWN") == NULL) split_off_worker();
    {
        static int warm_device;
        warm_device = device;
        g_warm_started = pthread_create(&g_warm_tid, NULL, warmup_run, &warm_device) == 0;
    }
    double t_start = now_s(), t_load = 0, t_build = 0, t_gpu = 0, t_format = 0, t_write = 0, t_wait_load = 0;
    int timing = getenv("SLAMEM_TIMING") != NULL;
    /* load everything (slamem.c:635-651).  Query files above SLAMEM_OVERLAP_MB (default 256) in total are parsed in pieces by
       a loader thread while the search already runs; stdout keeps the reference's order: what the main thread prints meanwhile
       is held back until the "successfully loaded" line can be printed */
    memset(&ref, 0, sizeof(ref));
    memset(&bj, 0, sizeof(bj));
    loader_t *const ld = &g_ld;
    int overlap = 0, ref_file = -1;
    {
        uint64_t qbytes_total = 0, pieces_cap = 0;
        long thr_mb = 256;
        if ((env = getenv("SLAMEM_OVERLAP_MB")) != NULL) thr_mb = atol(env);
        if ((env = getenv("SLAMEM_PIECE_MB")) != NULL && atol(env) > 0) piece_bytes = atol(env) << 20;
        for (f = 1; f < o.num_files; f++) {
            FILE *qf = fopen(argv[o.file_args[f]], "rb");
            if (qf) {
                long sz;
                fseek(qf, 0L, SEEK_END);
                sz = ftell(qf);
                fclose(qf);
                if (sz > 0) { qbytes_total += (uint64_t)sz; pieces_cap += (uint64_t)sz / (uint64_t)piece_bytes + 2; }
            }
        }
        overlap = thr_mb >= 0 && qbytes_total > ((uint64_t)thr_mb << 20);
        memset(ld, 0, sizeof(*ld));
        ld->release_early = qbytes_total > ((uint64_t)((env = getenv("SLAMEM_RELEASE_EARLY_GB")) != NULL ? atol(env) : 16) << 30);
        ld->cap = (int)(overlap ? pieces_cap + (uint64_t)o.num_files : (uint64_t)o.num_files);
        qsets = (slh_seqset *)calloc((size_t)ld->cap + 1, sizeof(slh_seqset));
        g_reap_tid = (pthread_t *)calloc((size_t)ld->cap + 1, sizeof(pthread_t));
        if (!qsets || !g_reap_tid) exit_message("Out of memory");
        ld->sets = qsets;
        ld->masks = (uint64_t **)calloc((size_t)ld->cap + 1, sizeof(uint64_t *));
        if (!ld->masks) exit_message("Out of memory");
        ld->min_bq = min_bq;
        ld->keep_quals = sam;
        ld->quals = (char **)calloc((size_t)ld->cap + 1, sizeof(char *));
        if (!ld->quals) exit_message("Out of memory");
        pthread_mutex_init(&ld->mu, NULL);
        pthread_cond_init(&ld->cv, NULL);
    }
    for (f = 0; f < o.num_files; f++) {
        const char *path = argv[o.file_args[f]];
        if (ref_file < 0) {
            int n = slh_load_file_q(path, 1, o.no_ns, (uint32_t)o.min_seq_len, o.ref_name, numbering, log_limit, &ref, NULL, stdout);
            if (n <= 0) exit_message("No valid sequences found in reference file");
            ref_file = f;
            numbering += n;
            g_num_refs = ref.num;
            o.file_args[0] = o.file_args[f]; /* remember which argument was the reference */
            bj.text = ref.chars;
            bj.n = (uint32_t)ref.total;
            bj.device = device;
            build_async = pthread_create(&build_tid, NULL, build_run, &bj) == 0;
            if (overlap) break;
        } else {
            char *quals = NULL;
            int n = slh_load_file_q(path, 0, o.no_ns, (uint32_t)o.min_seq_len, NULL, numbering, log_limit, &qsets[ld->ready], &quals, stdout);
            if (n < 0) { /* an invalid FASTQ file (the loader said so): before any search */
                if (build_async) pthread_join(build_tid, NULL);
                join_warmup();
                fflush(stdout);
                exit(-1);
            }
            if (n != 0) {
                if (ld->keep_quals) ld->quals[ld->ready] = quals;
                else ld->masks[ld->ready] = mask_of_quals(ld, &qsets[ld->ready], quals);
                if (ld->invalid) exit_message("Out of memory");
                numbering += n; ld->total_queries += n; ld->ready++;
            }
        }
    }
    if (overlap) {
        ld->argv = argv; ld->file_args = o.file_args; ld->first_file = ref_file + 1; ld->num_files = o.num_files;
        ld->acgt_only = o.no_ns; ld->min_len = (uint32_t)o.min_seq_len; ld->numbering = numbering; ld->log_limit = log_limit;
        ld->piece_bytes = piece_bytes;
        fflush(stdout);
        g_mo = open_memstream(&g_mo_buf, &g_mo_len);
        g_ld_started = g_mo != NULL && pthread_create(&g_ld_tid, NULL, loader_run, ld) == 0;
        if (!g_ld_started) { /* no thread: load here, as for small inputs */
            if (g_mo) release_stdout();
            overlap = 0;
            loader_run(ld);
        }
    } else {
        ld->done = 1;
    }
    t_load = now_s() - t_start;
    double t_join0 = now_s();
    if (build_async) pthread_join(build_tid, NULL); /* before any exit: never leave the process with a build in flight */
    else build_run(&bj);
    join_warmup();
    if (g_warm_ok) bind_to_gpu_node(device); /* from the main thread, before the worker threads below exist: they inherit the mask */
    double t_join = now_s() - t_join0, t_streams = 0;
    if (!overlap) {
        if (ld->ready == 0) exit_message("No query files provided"); /* slamem.c:648 */
        printf("> %d reference%s and %d quer%s successfully loaded\n", ref.num, ref.num == 1 ? "" : "s", ld->total_queries,
               ld->total_queries == 1 ? "y" : "ies");
    }
    if (o.min_mem_len < 1) exit_message("Minimum match length must be at least 1");

    if (o.out_arg == -1) out_name = slh_append_to_basename(argv[o.file_args[0]], "-mems.txt");
    else out_name = argv[o.out_arg];

    /* GetMatches (slamem.c:37-218) */
    say("> Using options: minimum %s length = %d ; strand = %s", MATCH_NAME(o.match_type), o.min_mem_len,
           o.both_strands == 0 ? "forward only" : "forward + reverse");
    if (max_occ > 0) say(" ; maximum occurrences = %d", max_occ);
    if (o.match_type == 4) say(" ; maximum gap = %d", max_gap > 0 ? max_gap : 5000);
    if (o.match_type == 5) say(" ; mismatch penalty = %d ; X-drop = %d", ext_pen > 0 ? ext_pen : 4, ext_xdrop >= 0 ? ext_xdrop : 20);
    if (o.match_type == 6 || o.match_type == 7 || o.match_type == 8)
        say(" ; maximum gap = %d ; mismatch penalty = %d ; X-drop = %d ; maximum edits = %d", max_gap > 0 ? max_gap : 5000,
            ext_pen > 0 ? ext_pen : 4, ext_xdrop >= 0 ? ext_xdrop : 20, max_edits >= 0 ? max_edits : 31);
    if (o.match_type == 8) say(" ; minimum mapping quality = %d", min_mapq);
    if (bq_given == 1) say(" ; minimum base quality = %d", min_bq); /* (only when asked for: the line of a run without -bq stays) */
    if (gt) say(" ; minimum depth = %d ; ploidy = %d ; error rate = %d Phred ; prior = %d Phred ; minimum quality = %d", min_depth, gt_ploidy, gt_err, gt_hetq, gt_qual);
    else if (sites || vcf) say(" ; minimum depth = %d ; minimum share = %d %%", min_depth, min_pct);
    if (cons) say(" ; minimum depth = %d", min_depth);
    if (depth) say(" ; covered from depth = %d", min_depth);
    say("\n");
    out = fopen(out_name, "w");
    if (!out) {
        release_stdout();
        printf("\n> ERROR: Cannot create output file <%s>\n", out_name);
        join_warmup();
        exit(-1);
    }
    say("> Building index for reference sequence");
    if (ref.num == 1) say(" \"%s\"", ref.recs[0].name);
    else say("s");
    say(" (%u Mbp) ...\n", (unsigned)(ref.total / 1000000U));
    if (!g_mo) fflush(stdout);
    t0 = now_s();
    idx = bj.idx;
    if (bj.rc != SLAMEM_OK) gpu_fail_msg("index construction on the GPU", bj.rc, bj.err);
    {
        slamem_index_info info = bj.info;
        slamem_timings tm = bj.tm;
        say("> Suffix sort + BWT + LCP + parent links on GPU %d ... OK (%.3f s, overlapped with the loading of the queries; device %.1f ms: sort %.1f, BWT %.1f, LCP %.1f, links %.1f; %u doubling rounds)\n",
               device, bj.seconds, tm.build_total_ms, tm.build_sort_ms, tm.build_bwt_ms, tm.build_lcp_ms, tm.build_links_ms,
               info.sort_rounds);
        say(":: Index size = %.1f MB in HBM (%s layout)\n", (double)info.arena_bytes / 1e6,
            info.layout == SLAMEM_LAYOUT_COMPACT ? "compact" : "full");
        {   /* the statistics lines of BuildSampledLCPArray (lcparray.c:709-711, 999-1000), from the per-row records */
            slamem_sslcp_stats st = bj.st;
            unsigned bwt_len = info.bwt_size;
            if (bj.rc_stats != SLAMEM_OK) gpu_fail_msg("LCP sampling statistics", bj.rc_stats, bj.err);
            say(":: %.2lf%% samples (%u of %u)\n", ((double)st.num_samples / (double)bwt_len) * 100.0, (unsigned)st.num_samples, bwt_len);
            say(":: %.2lf%% oversized samples (%d of %u)\n", ((double)st.num_oversized_lcp / (double)st.num_samples) * 100.0,
                   (int)st.num_oversized_lcp, (unsigned)st.num_samples);
            say(":: Average LCP value = %d (max=%lld)\n", (int)(st.sum_lcp / (long long)bwt_len), (long long)st.max_lcp);
            say(":: %.2lf%% oversized values (%d of %u)\n", ((double)st.num_oversized_links / (double)st.num_samples) * 100.0,
                   (int)st.num_oversized_links, (unsigned)st.num_samples);
            say(":: Average SV distance = %.2lf (max=%lld)\n", (double)st.sum_link_distance / (double)st.num_samples,
                   (long long)st.max_link_distance);
        }
    }
    /* SLAMEM_GPUS=N: replicate the index to N GPUs (device, device+1, ...) with one RCCL broadcast of its arena over
       xGMI; every batch is then split by bases into N contiguous shares, one per GPU (no data-path collective). */
    gpus[0] = idx;
    int logical = 0; /* SLAMEM_LOGICAL_GPUS=N (self-test): N "GPUs" that are all this device, each with its own copy of the index */
    if ((env = getenv("SLAMEM_GPUS")) != NULL) {
        int avail = 0;
        slamem_device_count(&avail);
        ngpu = atoi(env) <= 0 ? avail - device : atoi(env);
        if (ngpu < 1) ngpu = 1;
        if (ngpu > 16) ngpu = 16;
        if (device + ngpu > avail) exit_message("SLAMEM_GPUS asks for more GPUs than are visible");
    } else if ((env = getenv("SLAMEM_LOGICAL_GPUS")) != NULL && atoi(env) > 1) {
        ngpu = atoi(env) > 16 ? 16 : atoi(env);
        logical = 1;
    }
    if (ngpu > 1 || getenv("SLAMEM_REPLICATE_SELFTEST") != NULL) {
        int devs[16], g;
        double tr = now_s();
        for (g = 0; g < ngpu; g++) devs[g] = logical ? device : device + g;
        {   /* libslamem_rccl.so (and RCCL behind it, hundreds of MB of code) is loaded only when it is needed: a
               one-GPU run never pays for it at start-up */
            typedef int (*replicate_fn)(const slamem_index *, const int *, int, int, slamem_index **);
            void *h = dlopen("libslamem_rccl.so", RTLD_NOW | RTLD_GLOBAL);
            replicate_fn fn = h ? (replicate_fn)dlsym(h, "slamem_index_replicate") : NULL;
            if (!fn) {
                release_stdout();
                printf("\n> ERROR: cannot load libslamem_rccl.so (%s)\n", dlerror());
                join_warmup();
                exit(-1);
            }
            if (logical) { /* one one-rank broadcast into a fresh arena per logical GPU: the scheduling below is the real N-GPU one */
                for (g = 1, rc = SLAMEM_OK; g < ngpu && rc == SLAMEM_OK; g++) rc = fn(idx, devs, 1, 1, &gpus[g]);
            } else {
                rc = fn(idx, devs, ngpu, ngpu == 1, gpus);
            }
        }
        if (rc != SLAMEM_OK) gpu_fail("index replication over RCCL", rc);
        if (ngpu == 1) { slamem_index_free(idx); idx = gpus[0]; } /* self-test: search on the broadcast copy */
        say("> Index replicated to %d %sGPU%s by RCCL broadcast ... OK (%.3f s)\n", ngpu, logical ? "logical " : "",
            ngpu == 1 ? " (self-test copy)" : "s", now_s() - tr);
    }
    t_build = bj.seconds + (now_s() - t0);
    if (o.match_type != 8) { /* (-pile prints the reference letter of every row: it keeps the text) */
        free(ref.chars); /* the reference frees the text here too (slamem.c:75-77) */
        ref.chars = NULL;
    }
    say("> Matching query sequences against index ...\n");
    if (!g_mo) fflush(stdout);

    {
        /* (-paf: what is formatted and counted is a read, whichever strand its mapping lies on) */
        int strands = (o.match_type == 7 || o.match_type == 8) ? 1 : o.both_strands ? 2 : 1;
        long printed = 0;
        /* the list of batches (records [first,last) of one query file each), then a pipeline over it: the GPUs search
           batches b+1.. (slamem_stream_*: upload, search and download of neighbouring batches overlap), the main thread
           formats batch b with all host threads, the writer thread writes batch b-1 */
        typedef struct { int f, first, last; } batch_range;
        batch_range *ranges = NULL;
        size_t nranges = 0, cap_ranges = 0, bi, submitted = 0;
        uint64_t max_chars = 1;
        uint32_t max_recs = 1;
        int inflight[16], g;
        const int slots = 6; /* upload, prepare, search and download of four batches beside the one being formatted */
        int sets_seen = 0, sets_reaped = 0, sets_ready = ld->ready; /* !overlap: everything is there */
#define ADD_RANGES_OF_NEW_SETS()                                                                                              \
        for (; sets_seen < sets_ready; sets_seen++) {                                                                          \
            slh_seqset *q = &qsets[sets_seen];                                                                                 \
            int first = 0;                                                                                                     \
            while (first < q->num) {                                                                                           \
                int last = first;                                                                                              \
                uint64_t base = q->offsets[first];                                                                             \
                /* the first batches are short, so that the search starts early */                                             \
                uint64_t limit = nranges < (size_t)ngpu ? batch_bytes / 4 : nranges < 2 * (size_t)ngpu ? batch_bytes / 2 : batch_bytes; \
                while (last < q->num && (last == first || q->offsets[last + 1] - base <= limit)) last++;                       \
                if (nranges == cap_ranges) {                                                                                   \
                    cap_ranges = cap_ranges ? cap_ranges * 2 : 16;                                                             \
                    ranges = (batch_range *)realloc(ranges, cap_ranges * sizeof(batch_range));                                 \
                    if (!ranges) pipeline_fail("Out of memory");                                                               \
                }                                                                                                              \
                ranges[nranges].f = sets_seen; ranges[nranges].first = first; ranges[nranges].last = last;                     \
                if (q->offsets[last] - base > max_chars) max_chars = q->offsets[last] - base;                                  \
                if ((uint32_t)(last - first) > max_recs) max_recs = (uint32_t)(last - first);                                  \
                nranges++;                                                                                                     \
                first = last;                                                                                                  \
            }                                                                                                                  \
        }
        ADD_RANGES_OF_NEW_SETS();
        if (overlap) { /* the batches are not known yet: reserve for a piece's worth, the slots grow on demand */
            uint64_t guess = batch_bytes < (uint64_t)piece_bytes ? batch_bytes : (uint64_t)piece_bytes;
            if (max_chars < guess) max_chars = guess;
            if (max_recs < max_chars / 64) max_recs = (uint32_t)(max_chars / 64);
        }
        memset(&g_writer, 0, sizeof(g_writer));
        g_writer.out = out;
        pthread_mutex_init(&g_writer.mu, NULL);
        pthread_cond_init(&g_writer.cv, NULL);
        if (sam) { /* the header, once, in front of the first batch's lines */
            slh_buffer hd = {0, 0, 0};
            if (slh_format_sam_header(&hd, ref.recs, ref.num)) pipeline_fail("Out of memory");
            if (fwrite(hd.data, 1, hd.len, out) != hd.len) pipeline_fail("Cannot write output file");
            slh_buffer_free(&hd);
        }
        g_writer.started = pthread_create(&g_writer.tid, NULL, writer_run, &g_writer) == 0;
        double ts0 = now_s();
        for (g = 0; g < 16; g++) piles[g] = NULL;
        for (g = 0; g < ngpu && (nranges || overlap); g++) { /* batch b is searched on GPU b mod ngpu: no data-path collective */
            rc = slamem_stream_create(gpus[g], slots, max_chars, max_recs, o.both_strands, o.match_type, &g_streams[g]);
            if (rc == SLAMEM_OK && max_occ > 0) {
                g_nstreams = g + 1; /* (so that a failure below tears this stream down too) */
                rc = slamem_stream_set_max_occ(g_streams[g], (uint32_t)max_occ);
            }
            if (rc == SLAMEM_OK && max_gap > 0) {
                g_nstreams = g + 1;
                rc = slamem_stream_set_max_gap(g_streams[g], (uint32_t)max_gap);
            }
            if (rc == SLAMEM_OK && o.match_type == 5) {
                g_nstreams = g + 1;
                rc = slamem_stream_set_ext_params(g_streams[g], (uint32_t)ext_pen,
                                                  ext_xdrop >= 0 ? (uint32_t)ext_xdrop : SLAMEM_EXT_XDROP_DEFAULT);
            }
            if (rc == SLAMEM_OK && o.match_type == 8) { /* one accumulator per GPU: the tables are added when the file is written */
                g_nstreams = g + 1;
                rc = slamem_pileup_create(gpus[g], &piles[g]);
                if (rc == SLAMEM_OK && (vcf || cons)) rc = slamem_pileup_enable_events(piles[g], ev_slots);
                if (rc == SLAMEM_OK && dedup) rc = slamem_pileup_enable_dedup(piles[g], dd_slots);
                if (rc == SLAMEM_OK) rc = slamem_stream_set_pileup(g_streams[g], piles[g], (uint32_t)min_mapq);
                if (rc == SLAMEM_OK && dedup) rc = slamem_stream_set_dedup(g_streams[g], 1);
            }
            if (rc == SLAMEM_OK && (o.match_type == 6 || o.match_type == 7 || o.match_type == 8)) {
                g_nstreams = g + 1;
                rc = slamem_stream_set_max_gap(g_streams[g], (uint32_t)max_gap);
                if (rc == SLAMEM_OK)
                    rc = slamem_stream_set_ext_params(g_streams[g], (uint32_t)ext_pen,
                                                      ext_xdrop >= 0 ? (uint32_t)ext_xdrop : SLAMEM_EXT_XDROP_DEFAULT);
                if (rc == SLAMEM_OK)
                    rc = slamem_stream_set_max_edits(g_streams[g], max_edits >= 0 ? (uint32_t)max_edits : SLAMEM_ALN_EDITS_DEFAULT);
            }
            if (rc == SLAMEM_OK && sam) { /* every batch also goes through the MD pass */
                g_nstreams = g + 1;
                rc = slamem_stream_set_md(g_streams[g], 1);
            }
            if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("setting up the search pipeline", rc); }
            g_nstreams = g + 1;
            inflight[g] = 0;
        }
        t_streams = now_s() - ts0;
        for (bi = 0;; bi++) {
            if (overlap) { /* take in the pieces parsed meanwhile; wait for one only when there is nothing else to do */
                double tw = now_s();
                pthread_mutex_lock(&ld->mu);
                while (bi >= nranges && sets_seen == ld->ready && !ld->done) pthread_cond_wait(&ld->cv, &ld->mu);
                sets_ready = ld->ready;
                pthread_mutex_unlock(&ld->mu);
                ADD_RANGES_OF_NEW_SETS();
                t_wait_load += now_s() - tw;
                if (bi >= nranges) { /* nothing new: either the loader is done or a piece without batches came in */
                    int finished;
                    pthread_mutex_lock(&ld->mu);
                    finished = ld->done && sets_seen == ld->ready;
                    pthread_mutex_unlock(&ld->mu);
                    if (finished) break;
                    bi--;
                    continue;
                }
            } else if (bi >= nranges) break;
            slh_seqset *q = &qsets[ranges[bi].f];
            const int first = ranges[bi].first, last = ranges[bi].last;
            for (; ld->release_early && sets_reaped < ranges[bi].f; sets_reaped++) /* every batch of the earlier sets is formatted */
                if (qsets[sets_reaped].chars) {
                    reap_set(&qsets[sets_reaped]); free(ld->masks[sets_reaped]); ld->masks[sets_reaped] = NULL;
                    free(ld->quals[sets_reaped]); ld->quals[sets_reaped] = NULL;
                }
            const slamem_mem *mems = NULL;
            const uint32_t *mism = NULL;
            const slamem_aln *segs = NULL;
            const uint32_t *ops = NULL;
            const uint64_t *ooff = NULL;
            uint64_t nops = 0;
            const slamem_map *reads = NULL;
            const uint32_t *md = NULL, *seg_eq = NULL, *prim = NULL;
            const uint64_t *mdoff = NULL;
            uint64_t nmd = 0;
            const uint64_t *boff = NULL;
            uint64_t total = 0;
            double tg = now_s();
            /* keep every GPU's pipeline full: slots - 1 batches in flight beside the result being formatted */
            while (submitted < nranges && inflight[submitted % (size_t)ngpu] < slots - 1) {
                slh_seqset *qs = &qsets[ranges[submitted].f];
                const uint64_t *qmask = ld->masks[ranges[submitted].f];
                if (qmask) /* -bq N on FASTQ reads: the set's mask is indexed as its letters, the stream takes the batch's words */
                    rc = slamem_stream_submit_masked(g_streams[submitted % (size_t)ngpu], qs->chars, qmask,
                                                     qs->offsets + ranges[submitted].first,
                                                     (uint32_t)(ranges[submitted].last - ranges[submitted].first), (uint32_t)o.min_mem_len);
                else
                rc = slamem_stream_submit(g_streams[submitted % (size_t)ngpu], qs->chars, qs->offsets + ranges[submitted].first,
                                          (uint32_t)(ranges[submitted].last - ranges[submitted].first), (uint32_t)o.min_mem_len);
                if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("MEM search on the GPU", rc); }
                inflight[submitted % (size_t)ngpu]++;
                submitted++;
            }
            rc = slamem_stream_next(g_streams[bi % (size_t)ngpu], &mems, &boff, &total, NULL, NULL);
            if (rc != SLAMEM_OK) {
                char detail[512];
                snprintf(detail, sizeof(detail), "%s", slamem_last_error_message());
                shutdown_pipeline();
                release_stdout();
                printf("\n> ERROR: MEM search on GPU %d failed: %s (%s)\n", device + (int)(bi % (size_t)ngpu), slamem_strerror(rc), detail);
                join_warmup();
                exit(-1);
            }
            if (o.match_type == 8) { /* the batch is in its GPU's table: nothing came back to format (total: the segments piled) */
                inflight[bi % (size_t)ngpu]--;
                total_matches += (long long)total;
                t_gpu += now_s() - tg;
                continue;
            }
            if (o.match_type == 5) { /* the fourth column of this batch's rows */
                rc = slamem_stream_mismatches(g_streams[bi % (size_t)ngpu], &mism);
                if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("MEM extension on the GPU", rc); }
            }
            if (o.match_type == 6 || o.match_type == 7) { /* the segments stand in the place of the rows */
                rc = slamem_stream_alns(g_streams[bi % (size_t)ngpu], &segs, &ops, &ooff, &nops);
                if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("alignment on the GPU", rc); }
            }
            if (o.match_type == 7) { /* ... and the offsets are per read */
                rc = slamem_stream_maps(g_streams[bi % (size_t)ngpu], &reads);
                if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("mapping on the GPU", rc); }
            }
            if (sam) { /* ... and the MD entries and the primary segments came with them (seg_eq and nmd are what the interface
                          hands out beside them: the writer needs neither, the primary segment is already chosen) */
                rc = slamem_stream_md(g_streams[bi % (size_t)ngpu], &md, &mdoff, &seg_eq, &prim, &nmd);
                if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("the MD pass on the GPU", rc); }
            }
            inflight[bi % (size_t)ngpu]--;
            t_gpu += now_s() - tg; /* time the main thread waited for the GPUs */
            tg = now_s();
            {
                /* the first strand blocks get their ':: "name" ....' line (slamem.c:97,101,203) and are formatted here;
                   the rest of the batch is formatted by all host threads and handed to the writer in order */
                uint64_t nblk = (uint64_t)(last - first) * strands, bseq = 0, b;
                int nthr = slh_thread_count(), t;
                if (log_limit == 0) bseq = nblk;
                else if (printed < log_limit) bseq = (uint64_t)(log_limit - printed) < nblk ? (uint64_t)(log_limit - printed) : nblk;
                for (b = 0; b < bseq; b++) {
                    int ri = first + (int)(b / strands), sidx = (int)(b % strands), d, dots;
                    uint64_t cnt = boff[b + 1] - boff[b], sum = 0;
                    if (md ? format_sam_read(&buf, q, ld->quals[ranges[bi].f], ri, b, reads, segs, ops, ooff, boff, md, mdoff, prim, &ref, &sum)
                        : reads ? slh_format_read_paf(&buf, q->recs[ri].name, q->recs[ri].size, reads[b].strand, reads[b].mapq, reads[b].s1,
                                                    reads[b].s2, (const uint32_t *)(segs + boff[b]), ops, ooff + boff[b], cnt, ref.recs,
                                                    ref.merged_start, ref.num, &sum)
                        : segs ? slh_format_block_aln(&buf, q->recs[ri].name, sidx, (const uint32_t *)(segs + boff[b]), ops, ooff + boff[b],
                                                    cnt, ref.recs, ref.merged_start, ref.num, &sum)
                             : slh_format_block_ext(&buf, q->recs[ri].name, sidx, (const uint32_t *)(mems + boff[b]),
                                             mism ? mism + boff[b] : NULL, cnt, ref.recs, ref.merged_start, ref.num, &sum))
                        pipeline_fail("Out of memory");
                    total_matches += (long long)cnt;
                    total_sum += (long long)sum;
                    dots = slh_progress_dots(q->recs[ri].size);
                    say(":: \"%s%s\" ", q->recs[ri].name, sidx ? " Reverse" : "");
                    for (d = 0; d < dots; d++) fputc('.', g_mo ? g_mo : stdout);
                    say(" (%d %ss ; avg size = %d bp)\n", (int)cnt, MATCH_NAME(o.match_type), (int)(cnt ? sum / cnt : 0));
                    printed++;
                }
                if (writer_push(&g_writer, &buf)) pipeline_fail("Out of memory");
                if (bseq < nblk) {
                    fmt_job *jobs;
                    pthread_t *tid;
                    fmt_queue fq;
                    uint64_t per;
                    int njobs;
                    double fmt_t0 = now_s(), fmt_longest = 0, fmt_latest_start = 0;
                    if ((nblk - bseq) < 4096 || nthr < 1) nthr = 1;
                    /* chunks of 32 k strand blocks, at least one per thread */
                    njobs = (int)((nblk - bseq + 32767) / 32768);
                    if (njobs < nthr) njobs = nthr;
                    jobs = (fmt_job *)calloc((size_t)njobs, sizeof(fmt_job));
                    tid = (pthread_t *)calloc((size_t)nthr, sizeof(pthread_t));
                    if (!jobs || !tid) pipeline_fail("Out of memory");
                    per = (nblk - bseq + (uint64_t)njobs - 1) / (uint64_t)njobs;
                    for (t = 0; t < njobs; t++) {
                        jobs[t].q = q; jobs[t].ref = &ref; jobs[t].mems = mems; jobs[t].mism = mism; jobs[t].boff = boff;
                        jobs[t].segs = segs; jobs[t].ops = ops; jobs[t].ooff = ooff; jobs[t].reads = reads;
                        jobs[t].md = md; jobs[t].mdoff = mdoff; jobs[t].prim = prim; jobs[t].quals = ld->quals[ranges[bi].f];
                        jobs[t].first_rec = first; jobs[t].strands = strands;
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
                        total_matches += jobs[t].matches;
                        total_sum += jobs[t].sum;
                        if (writer_push(&g_writer, &jobs[t].buf)) pipeline_fail("Out of memory");
                    }
                    free(jobs);
                    free(tid);
                    g_fmt_longest += fmt_longest;
                    g_fmt_latest_start += fmt_latest_start;
                }
                if (g_writer.failed) pipeline_fail("Cannot write output file");
            }
            t_format += now_s() - tg;
        }
#undef ADD_RANGES_OF_NEW_SETS
        free(ranges);
        release_stdout(); /* the loader is done: the "successfully loaded" line, then what was held back */
        total_queries = ld->total_queries;
        if (ld->failed) pipeline_fail("Internal error: the query files came in more pieces than planned");
        if (ld->invalid) { /* the loader thread met a query file that is no valid FASTQ (it said so), or ran out of memory */
            shutdown_pipeline();
            fclose(out);
            remove(out_name);
            exit_message(ld->invalid == 1 ? "A query file is not valid FASTQ" : "Out of memory");
        }
        if (ld->fasta_seen) fprintf(stderr, "> WARNING: option -bq %d has no effect on FASTA queries: they carry no base qualities\n", min_bq);
        if (ld->ready == 0) { /* slamem.c:648 (an overlapped run only knows it now) */
            shutdown_pipeline();
            fclose(out);
            remove(out_name);
            exit_message("No query files provided");
        }
        if (o.match_type == 8 && (sites || vcf || cons || depth)) {
            /* the tables of GPUs 1.. are added into GPU 0's, in chunks of 16 M rows; then GPU 0 applies the rule to the sum range
               after range and only the selected rows come back: a line each, the separators between records skipped */
            const uint64_t chunk = 16ull << 20, n = ref.total;
            uint64_t x0, cap = 1ull << 20, *pos = NULL;
            uint32_t *rows = NULL;
            uint8_t *alleles = NULL;
            uint64_t ecap = 1ull << 16, skipped[3] = {0, 0, 0}, sk[3] = {0, 0, 0};
            slamem_event *evs = NULL;
            uint64_t *anchors = NULL;
            uint32_t *arows = NULL;
            slamem_genotype *gts = NULL, *egts = NULL; /* -gt: the genotypes of the rows and of the events, and which events are called */
            uint8_t *ecalled = NULL;
            int r = 0;
            double tp = now_s();
            if (vcf && (gt ? slh_format_vcf_gt_header(&buf, ref.recs, ref.num) : slh_format_vcf_header(&buf, ref.recs, ref.num)))
                pipeline_fail("Out of memory");
            if (g_nstreams > 1) {
                rows = (uint32_t *)slh_big_malloc((size_t)(chunk < n ? chunk : n) * 24 + 24);
                if (!rows) pipeline_fail("Out of memory");
                for (g = 1; g < g_nstreams; g++)
                    for (x0 = 0; x0 < n; x0 += chunk) {
                        const uint64_t cnt = n - x0 < chunk ? n - x0 : chunk;
                        rc = slamem_pileup_counts_host(piles[g], x0, cnt, rows);
                        if (rc == SLAMEM_OK) rc = slamem_pileup_add_counts_host(piles[0], x0, cnt, rows);
                        if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("adding up the pileups of the GPUs", rc); }
                    }
                free(rows);
                rows = NULL;
            }
            for (g = 1; (vcf || cons) && g < g_nstreams; g++) { /* ... and their events, which arrive normalised and stay as they are */
                for (x0 = 0; x0 < n; x0 += chunk) {
                    const uint64_t cnt = n - x0 < chunk ? n - x0 : chunk;
                    uint64_t total = 0;
                    for (;;) {
                        if (!evs && !(evs = (slamem_event *)malloc((size_t)ecap * sizeof(slamem_event)))) pipeline_fail("Out of memory");
                        rc = slamem_pileup_events_host(piles[g], x0, cnt, 1, ecap, evs, sk, &total);
                        if (rc != SLAMEM_ERR_CAPACITY || total <= ecap) break;
                        free(evs);
                        evs = NULL;
                        ecap = total;
                    }
                    if (rc == SLAMEM_OK) rc = slamem_pileup_add_events_host(piles[0], evs, total);
                    if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("adding up the indel events of the GPUs", rc); }
                }
                skipped[0] += sk[0]; skipped[1] += sk[1]; skipped[2] += sk[2]; /* (what GPU g could not store) */
            }
            for (x0 = 0; !cons && !depth && g_nstreams > 0 && x0 < n; x0 += chunk) {
                const uint64_t cnt = n - x0 < chunk ? n - x0 : chunk;
                uint64_t total = 0, k = 0;
                for (;;) { /* a range that selects more rows than there is room for says how many: once more with that room */
                    if (!pos) {
                        pos = (uint64_t *)malloc((size_t)cap * 8);
                        rows = (uint32_t *)malloc((size_t)cap * 24);
                        alleles = (uint8_t *)malloc((size_t)cap);
                        if (gt) gts = (slamem_genotype *)malloc((size_t)cap * sizeof(slamem_genotype));
                        if (!pos || !rows || !alleles || (gt && !gts)) pipeline_fail("Out of memory");
                    }
                    rc = gt ? slamem_pileup_genotypes_host(piles[0], x0, cnt, &gtp, cap, pos, rows, gts, &total)
                            : slamem_pileup_sites_host(piles[0], x0, cnt, SLAMEM_SITES_VARIANT, (uint32_t)min_depth, (uint32_t)min_pct, cap, pos,
                                                       rows, alleles, &total);
                    if (rc != SLAMEM_ERR_CAPACITY || total <= cap) break;
                    free(pos); free(rows); free(alleles); free(gts);
                    gts = NULL;
                    pos = NULL;
                    cap = total;
                }
                if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("reading the variant sites from the GPU", rc); }
                if (vcf) { /* the events of the same range, the pileup rows of their anchors, and the lines of both record by record */
                    uint64_t etotal = 0, ek = 0, j;
                    int rr = r;
                    for (;;) {
                        if (!evs) {
                            evs = (slamem_event *)malloc((size_t)ecap * sizeof(slamem_event));
                            anchors = (uint64_t *)malloc((size_t)ecap * 8);
                            arows = (uint32_t *)malloc((size_t)ecap * 24);
                            if (!evs || !anchors || !arows) pipeline_fail("Out of memory");
                        } else if (!anchors) {
                            anchors = (uint64_t *)malloc((size_t)ecap * 8);
                            arows = (uint32_t *)malloc((size_t)ecap * 24);
                            if (!anchors || !arows) pipeline_fail("Out of memory");
                        }
                        if (gt && !egts) {
                            egts = (slamem_genotype *)malloc((size_t)ecap * sizeof(slamem_genotype));
                            ecalled = (uint8_t *)malloc((size_t)ecap);
                            if (!egts || !ecalled) pipeline_fail("Out of memory");
                        }
                        rc = slamem_pileup_events_host(piles[0], x0, cnt, 1, ecap, evs, sk, &etotal);
                        if (rc != SLAMEM_ERR_CAPACITY || etotal <= ecap) break;
                        free(evs); free(anchors); free(arows); free(egts); free(ecalled);
                        evs = NULL; anchors = NULL; arows = NULL; egts = NULL; ecalled = NULL;
                        ecap = etotal;
                    }
                    if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("reading the indel events from the GPU", rc); }
                    for (j = 0; j < etotal; j++) { /* the anchor row: the letter in front, or the event's own row at a record's start */
                        const uint64_t p = evs[j].pos;
                        while (rr + 1 < ref.num && p >= ref.merged_start[rr + 1]) rr++;
                        anchors[j] = p > (ref.num > 1 ? ref.merged_start[rr] : 0) ? p - 1 : p;
                    }
                    rc = slamem_pileup_rows_at_host(piles[0], anchors, etotal, arows);
                    if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("reading the pileup rows of the indel events from the GPU", rc); }
                    if (gt) { /* every event on its own against everything else at its anchor, on the GPU */
                        rc = slamem_pileup_genotype_events_host(piles[0], evs, anchors, etotal, &gtp, egts, ecalled);
                        if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("genotyping the indel events on the GPU", rc); }
                    }
                    while ((k < total || ek < etotal) && r < ref.num) {
                        const uint64_t start = ref.num > 1 ? ref.merged_start[r] : 0, end = start + ref.recs[r].size;
                        uint64_t e = k, ee;
                        while (k < total && pos[k] < start) k++; /* (a separator: no record's row) */
                        while (ek < etotal && evs[ek].pos < start) ek++;
                        for (e = k; e < total && pos[e] < end; e++) {}
                        for (ee = ek; ee < etotal && evs[ee].pos < end; ee++) {}
                        if (gt ? slh_format_vcf_gt_rows(&buf, ref.recs[r].name, start, ref.recs[r].size, ref.chars, pos + k, rows + k * 6,
                                                        (const slh_genotype *)(gts + k), e - k, (const slh_event *)(evs + ek), arows + ek * 6,
                                                        (const slh_genotype *)(egts + ek), ecalled + ek, ee - ek)
                               : slh_format_vcf_rows(&buf, ref.recs[r].name, start, ref.recs[r].size, ref.chars, pos + k, rows + k * 6, alleles + k,
                                                     e - k, (const slh_event *)(evs + ek), arows + ek * 6, ee - ek, (uint32_t)min_depth,
                                                     (uint32_t)min_pct))
                            pipeline_fail("Out of memory");
                        k = e;
                        ek = ee;
                        if (end > x0 + cnt) break; /* (the record goes on in the next range) */
                        r++;
                    }
                    k = total;
                }
                while (k < total && r < ref.num) { /* the rows of one record after the other */
                    const uint64_t start = ref.num > 1 ? ref.merged_start[r] : 0, end = start + ref.recs[r].size;
                    uint64_t e = k;
                    if (pos[k] >= end) { r++; continue; }
                    if (pos[k] < start) { k++; continue; } /* (a separator: no record's row) */
                    while (e < total && pos[e] < end) e++;
                    if (slh_format_site_rows(&buf, ref.recs[r].name, start, ref.chars, pos + k, rows + k * 6, alleles + k, e - k))
                        pipeline_fail("Out of memory");
                    k = e;
                }
                if (writer_push(&g_writer, &buf)) pipeline_fail("Out of memory");
                if (g_writer.failed) pipeline_fail("Cannot write output file");
            }
            if (cons && g_nstreams > 0) {
                /* -cons: GPU 0 builds the consensus of the summed table and events range after range; the bounds cut it at the
                   records' first rows and ends (a separator's row, and an insertion in front of it, is no record's), and a record
                   is written when its last piece is there */
                uint64_t ccap = (chunk < n ? chunk : n) + (chunk < n ? chunk : n) / 64 + 64, rlen = 0, rcap = 0, stats[5] = {0, 0, 0, 0, 0};
                uint64_t *bnd = (uint64_t *)malloc(((size_t)ref.num * 2 + 2) * 16), *offs, none = 0;
                uint8_t *seq = NULL;
                char *rec = NULL;
                if (!bnd) pipeline_fail("Out of memory");
                offs = bnd + (size_t)ref.num * 2 + 2;
                for (x0 = 0; x0 < n; x0 += chunk) {
                    const uint64_t cnt = n - x0 < chunk ? n - x0 : chunk;
                    uint64_t total = 0, st[5], m = 0, j;
                    int rr;
                    for (rr = r; rr < ref.num; rr++) { /* the pieces of the records inside the range */
                        const uint64_t start = ref.num > 1 ? ref.merged_start[rr] : 0, end = start + ref.recs[rr].size;
                        if (start >= x0 + cnt) break;
                        bnd[m++] = start > x0 ? start : x0;
                        bnd[m++] = end < x0 + cnt ? end : x0 + cnt;
                        if (end > x0 + cnt) break;
                    }
                    for (;;) {
                        if (!seq && !(seq = (uint8_t *)slh_big_malloc((size_t)ccap))) pipeline_fail("Out of memory");
                        rc = slamem_pileup_consensus_host(piles[0], x0, cnt, (uint32_t)min_depth, ccap, seq, bnd, m, offs, st, &total);
                        if (rc != SLAMEM_ERR_CAPACITY || total <= ccap) break;
                        free(seq);
                        seq = NULL;
                        ccap = total;
                    }
                    if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("reading the consensus from the GPU", rc); }
                    for (j = 0; j < 5; j++) stats[j] += st[j];
                    for (j = 0; j < m; j += 2) {
                        const uint64_t end = (ref.num > 1 ? ref.merged_start[r] : 0) + ref.recs[r].size, got = offs[j + 1] - offs[j];
                        if (rlen + got > rcap) {
                            char *more;
                            rcap = (rlen + got) * 2 + 64;
                            if (!(more = (char *)realloc(rec, (size_t)rcap))) pipeline_fail("Out of memory");
                            rec = more;
                        }
                        if (got) memcpy(rec + rlen, seq + offs[j], (size_t)got);
                        rlen += got;
                        if (bnd[j + 1] < end) break; /* (the record goes on in the next range) */
                        if (slh_format_fasta_record(&buf, ref.recs[r].name, rec ? rec : "", rlen)) pipeline_fail("Out of memory");
                        rlen = 0;
                        r++;
                    }
                    if (writer_push(&g_writer, &buf)) pipeline_fail("Out of memory");
                    if (g_writer.failed) pipeline_fail("Cannot write output file");
                }
                free(bnd); free(seq); free(rec);
                fprintf(stderr, "> Consensus: %llu positions uncalled, %llu called unlike the reference, %llu deleted, %llu insertions of %llu letters\n",
                        (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[2], (unsigned long long)stats[3],
                        (unsigned long long)stats[4]);
                rc = slamem_pileup_events_host(piles[0], 0, 0, 1, 0, NULL, sk, &none); /* (no event: GPU 0's skipped counters) */
                if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("reading the indel events from the GPU", rc); }
            }
            if (depth && g_nstreams > 0) {
                /* -depth: GPU 0 turns the summed table into runs of equal depth range after range; the bounds are the first rows
                   and the ends of the records' pieces inside the range (a separator's row is no record's) and with -win the
                   windows' borders between them, and cum at the bounds gives the windows' means and the records' summaries */
                uint64_t dcap = window ? 0 : 1ull << 20, bcap = 0, *bnd = NULL, *cum = NULL;
                uint64_t rec_sum = 0, rec_cov = 0, wacc = 0; /* of record r so far; -win: of its window that is still open */
                slamem_depth_run *runs = NULL;
                slh_depth_pending pend = {0, 0, 0, 0};
                slh_buffer sbuf = {0, 0, 0};
                for (x0 = 0; x0 < n; x0 += chunk) {
                    const uint64_t cnt = n - x0 < chunk ? n - x0 : chunk;
                    uint64_t total = 0, m = 0, j;
                    int rr;
                    for (rr = r; rr < ref.num; rr++) { /* the pieces of the records inside the range */
                        const uint64_t start = ref.num > 1 ? ref.merged_start[rr] : 0, end = start + ref.recs[rr].size;
                        const uint64_t a = start > x0 ? start : x0, b = end < x0 + cnt ? end : x0 + cnt;
                        const uint64_t inside = window && b > a ? (b - start - 1) / window - (a - start) / window : 0;
                        if (start >= x0 + cnt) break;
                        if (m + inside + 2 > bcap) {
                            uint64_t *more;
                            bcap = (m + inside + 2) * 2;
                            if (!(more = (uint64_t *)realloc(bnd, (size_t)bcap * 8))) pipeline_fail("Out of memory");
                            bnd = more;
                        }
                        bnd[m++] = a;
                        for (j = 1; j <= inside; j++) bnd[m++] = start + ((a - start) / window + j) * window;
                        bnd[m++] = b;
                        if (end > x0 + cnt) break;
                    }
                    free(cum);
                    if (!(cum = (uint64_t *)malloc((size_t)(m + 1) * 16))) pipeline_fail("Out of memory");
                    for (;;) { /* a range of more runs than there is room for says how many: once more with that room */
                        if (dcap && !runs && !(runs = (slamem_depth_run *)slh_big_malloc((size_t)dcap * sizeof(slamem_depth_run))))
                            pipeline_fail("Out of memory");
                        rc = slamem_pileup_depth_runs_host(piles[0], x0, cnt, levels, (uint32_t)num_levels, (uint32_t)min_depth, dcap, runs, bnd,
                                                           m, cum, &total);
                        if (window && rc == SLAMEM_ERR_CAPACITY) rc = SLAMEM_OK; /* (the windows need the sums alone) */
                        if (rc != SLAMEM_ERR_CAPACITY || total <= dcap) break;
                        free(runs);
                        runs = NULL;
                        dcap = total;
                    }
                    if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("reading the depth runs from the GPU", rc); }
                    for (j = 0; j < m;) {
                        const uint64_t start = ref.num > 1 ? ref.merged_start[r] : 0, size = ref.recs[r].size, end = start + size;
                        const uint64_t a = bnd[j], ja = j;
                        uint64_t b;
                        for (j++; bnd[j] < end && bnd[j] < x0 + cnt; j++) {} /* (the piece's last bound: the record's end or the range's) */
                        b = bnd[j];
                        if (window) { /* the windows that end in the piece; what is behind the last of them waits for the next range */
                            const uint64_t k = j - ja - (b == end || (b - start) % window == 0 ? 0 : 1);
                            const uint64_t sum0 = cum[2 * ja] - wacc;
                            if (slh_format_depth_windows(&buf, ref.recs[r].name, size, window, (a - start) / window, sum0, cum + 2 * (ja + 1), k))
                                pipeline_fail("Out of memory");
                            wacc = cum[2 * j] - (k ? cum[2 * (ja + k)] : sum0);
                        } else if (slh_format_depth_runs(&buf, ref.recs[r].name, start, a, b, (const slh_depth_run *)runs, total, &pend)) {
                            pipeline_fail("Out of memory");
                        }
                        rec_sum += cum[2 * j] - cum[2 * ja];
                        rec_cov += cum[2 * j + 1] - cum[2 * ja + 1];
                        j++;
                        if (b < end) break; /* (the record goes on in the next range) */
                        if (slh_format_depth_flush(&buf, ref.recs[r].name, &pend) ||
                            slh_format_depth_summary(&sbuf, ref.recs[r].name, size, rec_cov, rec_sum))
                            pipeline_fail("Out of memory");
                        rec_sum = rec_cov = wacc = 0;
                        r++;
                    }
                    if (writer_push(&g_writer, &buf)) pipeline_fail("Out of memory");
                    if (g_writer.failed) pipeline_fail("Cannot write output file");
                }
                if (sbuf.len) fwrite(sbuf.data, 1, sbuf.len, stderr);
                slh_buffer_free(&sbuf);
                free(bnd); free(cum); free(runs);
            }
            free(pos); free(rows); free(alleles);
            free(evs); free(anchors); free(arows);
            free(gts); free(egts); free(ecalled);
            if ((vcf || cons) && g_nstreams > 0) {
                skipped[0] += sk[0]; skipped[1] += sk[1]; skipped[2] += sk[2]; /* (GPU 0's, the merge included) */
                if (skipped[0] | skipped[1] | skipped[2])
                    fprintf(stderr, "> WARNING: indel observations that are in no event: %llu insertions of more than 31 letters, %llu without "
                                    "room in the event table, %llu malformed%s\n", (unsigned long long)skipped[0],
                            (unsigned long long)skipped[1], (unsigned long long)skipped[2],
                            skipped[1] ? " (a larger table: -evs)" : "");
            }
            t_format += now_s() - tp;
        } else if (o.match_type == 8) {
            /* the table, in chunks of at most 16 M rows (24 bytes a row: the table of a 100 Mbp text never sits in one buffer):
               the GPUs' tables added up, then a line per row of a record that has a count */
            const uint64_t chunk = 16ull << 20, n = ref.total;
            uint32_t *rows = NULL, *more = NULL;
            uint64_t x0;
            int r = 0;
            double tp = now_s();
            if (g_nstreams > 0) {
                rows = (uint32_t *)slh_big_malloc((size_t)(chunk < n ? chunk : n) * 24 + 24);
                if (ngpu > 1) more = (uint32_t *)slh_big_malloc((size_t)(chunk < n ? chunk : n) * 24 + 24);
                if (!rows || (ngpu > 1 && !more)) pipeline_fail("Out of memory");
            }
            for (x0 = 0; g_nstreams > 0 && x0 < n; x0 += chunk) {
                const uint64_t cnt = n - x0 < chunk ? n - x0 : chunk;
                uint64_t x = x0, k;
                rc = slamem_pileup_counts_host(piles[0], x0, cnt, rows);
                for (g = 1; rc == SLAMEM_OK && g < g_nstreams; g++) {
                    rc = slamem_pileup_counts_host(piles[g], x0, cnt, more);
                    for (k = 0; rc == SLAMEM_OK && k < cnt * 6; k++) rows[k] += more[k];
                }
                if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("reading the pileup from the GPU", rc); }
                while (x < x0 + cnt && r < ref.num) { /* the pieces of the records inside the chunk; the separators are skipped */
                    const uint64_t start = ref.num > 1 ? ref.merged_start[r] : 0, end = start + ref.recs[r].size;
                    uint64_t a, b;
                    if (end <= x) { r++; continue; }
                    a = start > x ? start : x;
                    b = end < x0 + cnt ? end : x0 + cnt;
                    if (a >= x0 + cnt) break;
                    if (slh_format_pile_rows(&buf, ref.recs[r].name, (uint32_t)(a - start) + 1u, ref.chars + a, rows + (a - x0) * 6, b - a))
                        pipeline_fail("Out of memory");
                    x = b;
                    if (b == end) r++;
                }
                if (writer_push(&g_writer, &buf)) pipeline_fail("Out of memory");
                if (g_writer.failed) pipeline_fail("Cannot write output file");
            }
            free(rows);
            free(more);
            t_format += now_s() - tp;
        }
        if (dedup && g_nstreams > 0) { /* (one GPU: its counters are the run's) */
            uint64_t dd[4] = {0, 0, 0, 0};
            rc = slamem_pileup_dedup_stats(piles[0], dd);
            if (rc != SLAMEM_OK) { shutdown_pipeline(); gpu_fail("reading the duplicate filter's counters from the GPU", rc); }
            fprintf(stderr, "> Duplicates: %llu candidate reads, %llu duplicates (%.2f %%) not counted, %llu without room in the duplicate "
                            "table%s\n", (unsigned long long)dd[0], (unsigned long long)dd[1], dd[0] ? 100.0 * (double)dd[1] / (double)dd[0] : 0.0,
                    (unsigned long long)dd[2], dd[2] ? " (a larger table: -dslots)" : "");
        }
        writer_finish(&g_writer);
        t_write = g_writer.seconds;
        if (g_writer.failed) pipeline_fail("Cannot write output file");
        if (log_limit != 0 && o.match_type != 8 && (long)total_queries * strands > log_limit)
            say(":: ... (%ld more strand blocks matched; set SLAMEM_VERBOSE=1 for a line each)\n",
                   (long)total_queries * strands - log_limit);
    }
    double t_end0 = now_s(), t_end1;
    if (total_queries != 1) /* slamem.c:210-212 (the reference divides by zero when nothing matched) */
        printf(":: Average %d %ss found per query sequence (total = %lld, avg size = %d bp)\n",
               (int)(total_matches / total_queries), MATCH_NAME(o.match_type), total_matches,
               (int)(total_matches ? total_sum / total_matches : 0));
    fflush(stdout);
    printf("> Saving %ss to <%s> ... ", depth ? "depth run" : cons ? "consensus sequence" : vcf ? "variant call" : sites ? "variant site" : MATCH_NAME(o.match_type), out_name);
    if (fflush(out) != 0 || ferror(out)) exit_message("Cannot write output file");
    if (getenv("SLAMEM_FULL_TEARDOWN") != NULL && fclose(out) != 0) exit_message("Cannot write output file");
    t_end1 = now_s();
    printf("OK\n");
    printf("> Done!\n");
    char overlap_note[96] = "";
    if (g_ld.seconds > 0)
        snprintf(overlap_note, sizeof(overlap_note), " + queries parsed in pieces beside the search in %.3f s (%.3f s waited for)", g_ld.seconds, t_wait_load);
    if (timing)
        fprintf(stderr, "[timing] formatter threads: busy %.3f s in all; per batch the longest chunk %.3f s, the last chunk started %.3f s after the batch began (sums over the batches)\n",
                g_fmt_busy, g_fmt_longest, g_fmt_latest_start);
    if (timing)
        fprintf(stderr, "[timing] load %.3f s%s (index build of %.3f s overlapped; %.3f s more waiting for it), pipeline set-up %.3f s, "
                        "waiting for the GPU (upload + search + download, overlapped with formatting) %.3f s, format %.3f s "
                        "(writer thread busy %.3f s, overlapped; text buffers: %ld recycled, %ld fresh), close %.3f s, total %.3f s\n",
                t_load, overlap_note, t_build, t_join, t_streams, t_gpu, t_format, t_write, g_pool_hits, g_pool_misses, t_end1 - t_end0,
                now_s() - t_start);
    fflush(stdout);
    fflush(stderr);
    if (getenv("SLAMEM_FULL_TEARDOWN") == NULL) {
        /* everything is written and nothing runs on the GPU any more: leave without returning gigabytes of buffers and
           HBM piece by piece (0.15-0.25 s of the reference-sized run); the kernel driver reclaims them with the process */
        leave_now();
    }
    {
        double a = now_s(), b, c, d;
        shutdown_pipeline();
        for (i = 0; i < 16 && o.match_type == 8; i++) slamem_pileup_free(piles[i]);
        b = now_s();
        for (i = 0; i < ngpu; i++) slamem_index_free(gpus[i]);
        c = now_s();
        if (o.out_arg == -1) free(out_name);
        slh_buffer_free(&buf);
        slh_free_seqset(&ref);
        for (f = 0; f < g_reap_n; f++) pthread_join(g_reap_tid[f], NULL);
        free(g_reap_tid);
        for (f = 0; f < g_ld.ready; f++) { slh_free_seqset(&qsets[f]); free(g_ld.masks[f]); }
        free(g_ld.masks);
        free(qsets);
        pthread_mutex_lock(&g_pool_mu);
        while (g_pool_n > 0) slh_buffer_free(&g_pool[--g_pool_n]);
        pthread_mutex_unlock(&g_pool_mu);
        d = now_s();
        if (timing)
            fprintf(stderr, "[timing] teardown: search pipeline (pinned buffers, device work space) %.3f s, index %.3f s, host buffers %.3f s\n",
                    b - a, c - b, d - c);
    }
    slh_free_options(&o);
    return 0;
}
