/* slamem_host.c -- FASTA loading, option parsing and MEM text formatting of the slaMEM-compatible
 * front end.  Plain C, no GPU code; see slamem_host.h for the reference lines each piece restates. */
#include "slamem_host.h"
#include "../../include/slamem_fisher.h"
#include "../../include/slamem_aln_word.h"

#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <errno.h>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif
#include <sys/mman.h>

/* ------------------------------------------------------------------------------------------------ */
/* FASTA                                                                                             */
/* ------------------------------------------------------------------------------------------------ */

/* InitCharsTable (sequence.c:61-81): A/C/G/T any case -> upper; other letters -> 'N' unless acgt_only;
 * '>' ends a record; everything else (digits, blanks, '*', '-') is dropped. */
static void init_table(char table[256], int allow_ns) {
    int i;
    memset(table, 0, 256);
    if (allow_ns)
        for (i = 'A'; i <= 'Z'; i++) { table[i] = 'N'; table[i + 32] = 'N'; }
    table['A'] = table['a'] = 'A';
    table['C'] = table['c'] = 'C';
    table['G'] = table['g'] = 'G';
    table['T'] = table['t'] = 'T';
}

typedef struct {
    const unsigned char *p, *end;
} reader;

/* record names are carved out of large chunks (10 M reads = 10 M names: one malloc each would dominate) */
typedef struct name_chunk {
    struct name_chunk *next;
    size_t used, cap;
    char data[1];
} name_chunk;

static char *name_alloc(void **arena, size_t len) {
    name_chunk *c = (name_chunk *)*arena;
    if (!c || c->used + len > c->cap) {
        size_t cap = len > (1u << 20) ? len : (1u << 20);
        name_chunk *n = (name_chunk *)malloc(sizeof(name_chunk) + cap);
        if (!n) return NULL;
        n->next = c;
        n->used = 0;
        n->cap = cap;
        *arena = n;
        c = n;
    }
    c->used += len;
    return c->data + c->used - len;
}

static int rd(reader *r) { return r->p < r->end ? (int)*r->p++ : EOF; }

/* Buffers of tens of MB and more (sequence characters, record tables): 2 MB aligned and marked for transparent huge
 * pages, which takes most of the page-fault and unmap time out of a 1.5 GB read set.  free() releases them. */
void *slh_big_malloc(size_t bytes) {
    void *p = NULL;
    if (bytes < ((size_t)32 << 20)) return malloc(bytes ? bytes : 1);
    bytes = (bytes + (((size_t)2 << 20) - 1)) & ~(((size_t)2 << 20) - 1);
    if (posix_memalign(&p, (size_t)2 << 20, bytes) != 0) return NULL;
#ifdef MADV_HUGEPAGE
    (void)madvise(p, bytes, MADV_HUGEPAGE);
#endif
    return p;
}

static int grow(char **buf, uint64_t *cap, uint64_t need) {
    if (need <= *cap) return 0;
    uint64_t nc = *cap ? *cap : (1u << 20);
    while (nc < need) nc += nc / 2 + (1u << 20);
    if (*buf == NULL) { /* the loaders size their character buffer once, from the file size */
        char *fb = (char *)slh_big_malloc(nc);
        if (!fb) return -1;
        *buf = fb;
        *cap = nc;
        return 0;
    }
    char *nb = (char *)realloc(*buf, nc);
    if (!nb) return -1;
    *buf = nb;
    *cap = nc;
    return 0;
}

void slh_free_seqset(slh_seqset *s) {
    int i;
    if (!s) return;
    (void)i;
    while (s->name_arena) {
        name_chunk *c = (name_chunk *)s->name_arena;
        s->name_arena = c->next;
        free(c);
    }
    free(s->recs);
    free(s->chars);
    free(s->offsets);
    free(s->merged_start);
    memset(s, 0, sizeof(*s));
}

/* A whole line at once (sequence.c:61-81 for a line that holds nothing but letters): the `len` bytes at p are written to dst as
 * the table would write them -- A,C,G,T of either case as upper case; every other letter as 'N' (allow_ns), or none may occur
 * (!allow_ns: such a line takes the byte loop, which drops them).  Returns 0 -- whatever it wrote so far is to be ignored -- when
 * the line holds a byte the rule does not cover (a digit, a blank, '>', '*', ...): the byte loop then does the line.  A
 * soft-masked assembly (half of it lower case) and IUPAC letters stay on this path; 16 bytes per step with SSE2. */
static int line_of_letters(unsigned char *dst, const unsigned char *p, size_t len, int allow_ns) {
    size_t i = 0;
    static int slow = -1; /* SLAMEM_LOADER_BYTEWISE=1: every line through the byte loop (what the tests compare this path with) */
    if (slow < 0) { const char *v = getenv("SLAMEM_LOADER_BYTEWISE"); slow = v && atoi(v) != 0; }
    if (slow) return 0;
#if defined(__SSE2__)
    const __m128i fold = _mm_set1_epi8((char)0xDF), a = _mm_set1_epi8('A'), c = _mm_set1_epi8('C'), g = _mm_set1_epi8('G'),
                  t = _mm_set1_epi8('T'), n = _mm_set1_epi8('N'), z = _mm_set1_epi8(25);
    for (; i + 16 <= len; i += 16) {
        const __m128i x = _mm_loadu_si128((const __m128i *)(p + i));
        const __m128i u = _mm_and_si128(x, fold);
        const __m128i ok = _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(u, a), _mm_cmpeq_epi8(u, c)),
                                        _mm_or_si128(_mm_cmpeq_epi8(u, g), _mm_cmpeq_epi8(u, t)));
        if (allow_ns) {
            const __m128i v = _mm_sub_epi8(u, a);                              /* 0..25 for a letter (as unsigned bytes) */
            if (_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_min_epu8(v, z), v)) != 0xFFFF) return 0;
            _mm_storeu_si128((__m128i *)(dst + i), _mm_or_si128(_mm_and_si128(ok, u), _mm_andnot_si128(ok, n)));
        } else {
            if (_mm_movemask_epi8(ok) != 0xFFFF) return 0;
            _mm_storeu_si128((__m128i *)(dst + i), u);
        }
    }
#endif
    for (; i < len; i++) {
        const unsigned char u = (unsigned char)(p[i] & 0xDF);
        const int ok = u == 'A' || u == 'C' || u == 'G' || u == 'T';
        if (!ok && !(allow_ns && u >= 'A' && u <= 'Z')) return 0;
        dst[i] = ok ? u : (unsigned char)'N';
    }
    return 1;
}

/* the records of one memory range that starts with '>' */
static int load_mem(const unsigned char *data, long fsize, int merge, int acgt_only, uint32_t min_len,
                    const char *name_filter, int first_number, long log_limit, slh_seqset *out, FILE *log) {
    char table[256];
    reader r;
    int c, k, numseqs = 0, reccap = 0, matchpos, desclen;
    uint64_t seqlen = 0, maxseqlen = 0, cap = 0, offcap = 0;
    uint32_t seqsize;
    long logged = 0;
    char *chars = NULL;

    memset(out, 0, sizeof(*out));
    out->file_bytes = fsize;
    r.p = data;
    r.end = data + fsize;
    c = rd(&r);
    if (c != '>') {
        if (log) fprintf(log, "> WARNING: Invalid FASTA file\n");
        return 0;
    }
    init_table(table, !acgt_only);
    table['>'] = (char)0xFF; /* record terminator for the fast path below */
    if (grow(&chars, &cap, (uint64_t)fsize + 16)) goto oom; /* characters (+ separators) never outnumber the file's bytes */
    for (;;) { /* all records of the file (sequence.c:128) */
        const unsigned char *name_start;
        int quiet;
        while (c != EOF && c != '>') c = rd(&r);
        if (c == EOF) break;
        quiet = !log || (log_limit > 0 && logged >= log_limit);
        if (!quiet) fprintf(log, "# %02d [", first_number + numseqs);
        name_start = r.p;
        matchpos = 0;
        desclen = 0;
        if (quiet && !name_filter) { /* nothing to print or to match: find the end of the line in one step */
            const unsigned char *nl = (const unsigned char *)memchr(r.p, '\n', (size_t)(r.end - r.p));
            const unsigned char *stop = nl ? nl : r.end;
            const unsigned char *cr = (const unsigned char *)memchr(r.p, '\r', (size_t)(stop - r.p));
            if (cr) stop = cr;
            desclen = (int)(stop - r.p);
            c = stop < r.end ? (int)*stop : EOF;
            r.p = stop < r.end ? stop + 1 : stop;
        } else
        while ((c = rd(&r)) != EOF && c != '\n' && c != '\r') {
            if (!quiet && desclen < 50) fputc(c, log);
            if (name_filter && name_filter[matchpos] != '\0') { /* sequence.c:137-140 */
                if (name_filter[matchpos] == (char)c) matchpos++;
                else matchpos = 0;
            }
            desclen++;
        }
        if (!quiet) {
            for (k = desclen; k < 50; k++) fputc(' ', log);
            fprintf(log, "] ");
        }
        if (name_filter && name_filter[matchpos] != '\0') {
            if (!quiet) { fprintf(log, "NAME DOES NOT MATCH\n"); logged++; }
            continue;
        }
        seqsize = 0;
        if (!merge) {
            maxseqlen = seqlen; /* every query record is its own sequence */
        } else if (numseqs == 0) {
            seqlen = 0; /* sequence.c:151-155 */
            maxseqlen = 0;
        }
        {
            uint64_t rec_start = seqlen;
            if (!merge) { /* query records: tight, branch-light copy loop (the 'N' separator logic is reference-only) */
                const unsigned char *p = r.p, *pe = r.end;
                unsigned char *dst = (unsigned char *)chars + seqlen;
                while (p < pe && *p != '>') { /* line by line; a '>' anywhere ends the record (sequence.c:157) */
                    const unsigned char *nl = (const unsigned char *)memchr(p, '\n', (size_t)(pe - p));
                    const unsigned char *end = nl ? nl : pe;
                    const unsigned char *le = (end > p && end[-1] == '\r') ? end - 1 : end; /* (a CR is skipped like the LF) */
                    if (line_of_letters(dst, p, (size_t)(le - p), !acgt_only)) {
                        dst += le - p;
                        p = end;
                    } else {
                        while (p < end) {
                            unsigned char t = (unsigned char)table[*p];
                            if (t == 0xFF) break;
                            p++;
                            *dst = t;
                            dst += (t != 0);
                        }
                        if (p < end) break; /* stopped at a '>' inside the line */
                    }
                    if (nl) p = nl + 1; /* (the table maps the newline to "skip") */
                }
                seqsize = (uint32_t)(dst - ((unsigned char *)chars + seqlen));
                seqlen += seqsize;
                c = p < pe ? '>' : EOF;
                r.p = p < pe ? p + 1 : p;
                maxseqlen = seqlen;
            } else
            while ((c = rd(&r)) != '>' && c != EOF) {
                char t = table[c];
                if (t && seqsize != 0 && seqlen + 1 < maxseqlen) {
                    /* inside a record (its first letter, with the separator 'N' of sequence.c:163-165, is behind us) and not at
                       one of the steps of maxseqlen: this letter, then whole lines while they hold nothing but letters */
                    const unsigned char *p = r.p, *pe = r.end;
                    chars[seqlen++] = t;
                    seqsize++;
                    for (;;) {
                        const unsigned char *nl, *end, *le;
                        if (p < pe && (*p == '\n' || *p == '\r')) { p++; continue; }
                        if (p >= pe || *p == '>') break;
                        nl = (const unsigned char *)memchr(p, '\n', (size_t)(pe - p));
                        end = nl ? nl : pe;
                        le = (end > p && end[-1] == '\r') ? end - 1 : end;
                        if ((uint64_t)(le - p) + seqlen + 1 >= maxseqlen || (uint64_t)(le - p) + seqlen >= 0xFFFFFFF0ull) break;
                        if (!line_of_letters((unsigned char *)chars + seqlen, p, (size_t)(le - p), !acgt_only)) break;
                        seqlen += (uint64_t)(le - p);
                        seqsize += (uint32_t)(le - p);
                        p = end;
                    }
                    r.p = p;
                    continue;
                }
                if (t) {
                    if (seqlen == maxseqlen) { /* sequence.c:160-166 */
                        maxseqlen += (1u << 20);
                        if (merge && numseqs != 0 && seqsize == 0) chars[seqlen++] = 'N';
                    }
                    chars[seqlen++] = t;
                    seqsize++;
                    if (seqlen >= 0xFFFFFFF0ull) {
                        if (log) fprintf(log, "\n> WARNING: Sequence lengths of more than %u bp are not supported\n", UINT_MAX);
                        goto fail;
                    }
                }
            }
            if (merge) {
                if (seqlen != 0) maxseqlen = seqlen; /* sequence.c:172-176 */
            }
            if (seqsize == 0) {
                if (!quiet) { fprintf(log, "EMPTY\n"); logged++; }
                continue;
            }
            if (min_len != 0 && seqsize < min_len) {
                if (!quiet) { fprintf(log, "(%u bp) TOO SHORT\n", seqsize); logged++; }
                if (merge) seqlen -= seqsize; /* sequence.c:200: the separator 'N' stays */
                else seqlen = rec_start;
                continue;
            }
            if (!quiet) fprintf(log, "(%u bp) ", seqsize);
            if (numseqs == reccap) {
                int nc = reccap ? reccap * 2 : 64;
                slh_record *nr = (slh_record *)realloc(out->recs, (size_t)nc * sizeof(slh_record));
                if (!nr) goto oom;
                out->recs = nr;
                reccap = nc;
            }
            out->recs[numseqs].name = name_alloc(&out->name_arena, (size_t)desclen + 1);
            if (!out->recs[numseqs].name) goto oom;
            memcpy(out->recs[numseqs].name, name_start, (size_t)desclen);
            out->recs[numseqs].name[desclen] = '\0';
            out->recs[numseqs].size = seqsize;
            if (!merge) {
                if ((uint64_t)numseqs + 2 > offcap) {
                    uint64_t nc = offcap ? offcap * 2 : 1024;
                    uint64_t *no = (uint64_t *)realloc(out->offsets, nc * sizeof(uint64_t));
                    if (!no) goto oom;
                    out->offsets = no;
                    offcap = nc;
                }
                out->offsets[numseqs] = rec_start;
                out->offsets[numseqs + 1] = seqlen;
            }
            numseqs++;
            out->num = numseqs;
            if (!quiet) { fprintf(log, "OK\n"); logged++; }
            else if (log && log_limit > 0 && logged == log_limit) {
                fprintf(log, "# ... (further records of this file are loaded without a line each)\n");
                logged++;
            }
        }
    }
    if (numseqs == 0) {
        free(chars);
        slh_free_seqset(out);
        return 0;
    }
    if (grow(&chars, &cap, seqlen + 16)) goto oom;
    memset(chars + seqlen, 0, 16);
    out->chars = chars;
    out->total = seqlen;
    if (merge) { /* sequence.c:258-265 */
        out->merged_start = (uint32_t *)malloc((size_t)numseqs * sizeof(uint32_t));
        if (!out->merged_start) { chars = NULL; goto oom; }
        out->merged_start[0] = 0;
        for (k = 1; k < numseqs; k++) out->merged_start[k] = out->merged_start[k - 1] + out->recs[k - 1].size + 1;
    } else if (!out->offsets) {
        goto oom;
    }
    return numseqs;
oom:
    if (log) fprintf(log, "\n> ERROR: Out of memory while loading sequences\n");
fail:
    if (chars != out->chars) free(chars);
    slh_free_seqset(out);
    return 0;
}


/* ---- FASTQ query files ---------------------------------------------------------------------------
 * A file whose first byte is '@'.  Its lines are what '\n' separates (a final '\n' ends the last line and starts none; a '\r' at
 * a line's end is dropped); they come in records of four: '@' and the name, the letters, a line that starts with '+', and as
 * many quality bytes as the second line has letter bytes.  Anything else -- another first byte, a third line without '+',
 * unequal lengths, a number of lines that is no multiple of four -- makes the file invalid.  The letters go through the table
 * of the FASTA loader (init_table), and a byte that the table drops takes its quality byte with it, so that quals stays
 * parallel to chars.  Records are numbered, logged, dropped when empty or shorter than min_len as FASTA records are. */
#define FASTQ_INVALID (-1)
#define FASTQ_NOMEM (-2)

static const unsigned char *fastq_line(const unsigned char *p, const unsigned char *end, const unsigned char **next) {
    const unsigned char *nl = (const unsigned char *)memchr(p, '\n', (size_t)(end - p));
    const unsigned char *le = nl ? nl : end;
    *next = nl ? nl + 1 : end;
    if (le > p && le[-1] == '\r') le--;
    return le;
}

/* the records of one memory range that starts at a record's '@': their number, FASTQ_INVALID or FASTQ_NOMEM (nothing is
 * printed for those two: the caller does, once) */
static int load_fastq_mem(const unsigned char *data, long fsize, int acgt_only, uint32_t min_len, int first_number, long log_limit,
                          slh_seqset *out, char **quals_out, FILE *log) {
    char table[256];
    const unsigned char *p = data, *end = data + fsize;
    int numseqs = 0, reccap = 0, k, rc = FASTQ_NOMEM;
    uint64_t seqlen = 0, cap = 0, qcap = 0, offcap = 0;
    long logged = 0;
    char *chars = NULL, *quals = NULL;

    memset(out, 0, sizeof(*out));
    *quals_out = NULL;
    out->file_bytes = fsize;
    init_table(table, !acgt_only);
    /* (two lines of a record's four hold as many bytes each as it has letters at most) */
    if (grow(&chars, &cap, (uint64_t)fsize / 2 + 16) || grow(&quals, &qcap, (uint64_t)fsize / 2 + 16)) goto fail;
    while (p < end) {
        const unsigned char *name, *name_end, *seq, *seq_end, *plus, *plus_end, *ql, *ql_end, *next;
        uint64_t rec_start = seqlen;
        uint32_t seqsize;
        int quiet, desclen;
        if (*p != '@') { rc = FASTQ_INVALID; goto fail; }
        name = p + 1;
        name_end = fastq_line(p, end, &next);
        if (name_end < name) name_end = name; /* (the line "@\r" cannot occur: the '@' is no '\r') */
        seq = next;
        if (seq >= end) { rc = FASTQ_INVALID; goto fail; } /* truncated: no second line */
        seq_end = fastq_line(seq, end, &next);
        plus = next;
        if (plus >= end || *plus != '+') { rc = FASTQ_INVALID; goto fail; }
        plus_end = fastq_line(plus, end, &next);
        (void)plus_end;
        ql = next;
        if (ql >= end) { rc = FASTQ_INVALID; goto fail; } /* truncated: no fourth line */
        ql_end = fastq_line(ql, end, &next);
        if (ql_end - ql != seq_end - seq) { rc = FASTQ_INVALID; goto fail; }
        p = next;
        desclen = (int)(name_end - name);
        quiet = !log || (log_limit > 0 && logged >= log_limit);
        if (!quiet) {
            fprintf(log, "# %02d [", first_number + numseqs);
            for (k = 0; k < desclen && k < 50; k++) fputc(name[k], log);
            for (k = desclen; k < 50; k++) fputc(' ', log);
            fprintf(log, "] ");
        }
        {
            unsigned char *dst = (unsigned char *)chars + seqlen, *qdst = (unsigned char *)quals + seqlen;
            const size_t len = (size_t)(seq_end - seq);
            size_t i;
            if (line_of_letters(dst, seq, len, !acgt_only)) { /* nothing is dropped: the qualities as they are */
                memcpy(qdst, ql, len);
                seqsize = (uint32_t)len;
            } else {
                size_t w = 0;
                for (i = 0; i < len; i++) {
                    const unsigned char t = (unsigned char)table[seq[i]];
                    if (!t) continue;
                    dst[w] = t;
                    qdst[w] = ql[i];
                    w++;
                }
                seqsize = (uint32_t)w;
            }
            seqlen += seqsize;
        }
        if (seqsize == 0) {
            if (!quiet) { fprintf(log, "EMPTY\n"); logged++; }
            continue;
        }
        if (min_len != 0 && seqsize < min_len) {
            if (!quiet) { fprintf(log, "(%u bp) TOO SHORT\n", seqsize); logged++; }
            seqlen = rec_start;
            continue;
        }
        if (!quiet) fprintf(log, "(%u bp) ", seqsize);
        if (numseqs == reccap) {
            int nc = reccap ? reccap * 2 : 64;
            slh_record *nr = (slh_record *)realloc(out->recs, (size_t)nc * sizeof(slh_record));
            if (!nr) goto fail;
            out->recs = nr;
            reccap = nc;
        }
        out->recs[numseqs].name = name_alloc(&out->name_arena, (size_t)desclen + 1);
        if (!out->recs[numseqs].name) goto fail;
        memcpy(out->recs[numseqs].name, name, (size_t)desclen);
        out->recs[numseqs].name[desclen] = '\0';
        out->recs[numseqs].size = seqsize;
        if ((uint64_t)numseqs + 2 > offcap) {
            uint64_t nc = offcap ? offcap * 2 : 1024;
            uint64_t *no = (uint64_t *)realloc(out->offsets, nc * sizeof(uint64_t));
            if (!no) goto fail;
            out->offsets = no;
            offcap = nc;
        }
        out->offsets[numseqs] = rec_start;
        out->offsets[numseqs + 1] = seqlen;
        numseqs++;
        out->num = numseqs;
        if (!quiet) { fprintf(log, "OK\n"); logged++; }
        else if (log && log_limit > 0 && logged == log_limit) {
            fprintf(log, "# ... (further records of this file are loaded without a line each)\n");
            logged++;
        }
    }
    if (numseqs == 0) {
        free(chars);
        free(quals);
        slh_free_seqset(out);
        out->file_bytes = fsize;
        return 0;
    }
    memset(chars + seqlen, 0, 16);
    memset(quals + seqlen, 0, 16);
    out->chars = chars;
    out->total = seqlen;
    *quals_out = quals;
    return numseqs;
fail:
    free(chars);
    free(quals);
    slh_free_seqset(out);
    return rc;
}

/* the first record start at or behind `target`, found by counting lines from the record start `from` (a '@' may begin a
 * quality line, so "newline + '@'" alone is no record start; four lines on from a record start is one) */
static long fastq_cut(const unsigned char *data, long from, long fsize, long target) {
    long p = from;
    while (p < fsize && p < target) {
        int k;
        for (k = 0; k < 4; k++) {
            const unsigned char *nl = (const unsigned char *)memchr(data + p, '\n', (size_t)(fsize - p));
            if (!nl) return fsize;
            p = (long)(nl - data) + 1;
        }
    }
    return p;
}

/* ---- parallel loading of large query files ------------------------------------------------------- */
#include <pthread.h>
#include <sys/mman.h>
#include <unistd.h>

typedef struct {
    const unsigned char *data;
    long size;
    int acgt_only;
    uint32_t min_len;
    int first_number;
    long log_limit;
    FILE *log;
    slh_seqset set;
    int n;
    slh_seqset *dst;   /* second phase: this piece is copied to characters dst_cpos.. / records dst_rpos.. of dst */
    uint64_t dst_cpos;
    int dst_rpos;
    int fastq;         /* the range holds FASTQ records: quals is parallel to set.chars, and goes to dst_quals as they go to dst */
    char *quals, *dst_quals;
} load_job;

static void *load_job_run(void *arg) {
    load_job *j = (load_job *)arg;
    if (j->size <= 0) j->n = 0;
    else if (j->fastq)
        j->n = load_fastq_mem(j->data, j->size, j->acgt_only, j->min_len, j->first_number, j->log_limit, &j->set, &j->quals, j->log);
    else j->n = load_mem(j->data, j->size, 0, j->acgt_only, j->min_len, NULL, j->first_number, j->log_limit, &j->set, j->log);
    return NULL;
}

void slh_free_seqset(slh_seqset *s);

static void *concat_job_run(void *arg) {
    load_job *j = (load_job *)arg;
    const slh_seqset *s = &j->set;
    int i;
    if (j->n <= 0) return NULL;
    memcpy(j->dst->chars + j->dst_cpos, s->chars, s->total);
    if (j->quals) {
        memcpy(j->dst_quals + j->dst_cpos, j->quals, s->total);
        free(j->quals);
        j->quals = NULL;
    }
    memcpy(j->dst->recs + j->dst_rpos, s->recs, (size_t)s->num * sizeof(slh_record));
    for (i = 0; i < s->num; i++) j->dst->offsets[j->dst_rpos + i] = s->offsets[i] + j->dst_cpos;
    slh_free_seqset(&j->set); /* its names were handed over before; unmapping 100 MB pieces is worth doing in parallel too */
    return NULL;
}

int slh_thread_count(void) {
    const char *e = getenv("SLAMEM_THREADS");
    long n = e ? atol(e) : sysconf(_SC_NPROCESSORS_ONLN);
    if (n < 1) n = 1;
    if (n > 32) n = 32;
    return (int)n;
}

/* Query files above 64 MB are cut at "newline + '>'" positions (always a true record start: header lines are single
 * lines, and in sequence context any '>' starts a record, sequence.c:157) and parsed by several threads; the
 * pieces are concatenated in order, so the result equals the sequential parse.  The per-record log lines come from
 * the first piece only (they are limited to the first log_limit records anyway). */
/* A FASTQ range (fastq; it starts at a record start) is cut by counting lines from its start (fastq_cut), since there a '@'
 * after a newline may begin a quality line: one pass of memchr over the range in front of the threads, and every piece is parsed
 * by one thread.  *quals_out gets the qualities, parallel to out->chars; a piece that is no valid FASTQ makes the whole range
 * FASTQ_INVALID.  Returns -1 when memory runs out (the caller parses in one piece then). */
static int load_parallel(const unsigned char *data, long fsize, int acgt_only, uint32_t min_len, int first_number,
                         long log_limit, slh_seqset *out, FILE *log, int threads, int fastq, char **quals_out) {
    load_job *jobs = (load_job *)calloc((size_t)threads, sizeof(load_job));
    pthread_t *tid = (pthread_t *)calloc((size_t)threads, sizeof(pthread_t));
    long *cut = (long *)calloc((size_t)threads + 1, sizeof(long));
    int t, total = 0, ok = 1, bad = 0;
    uint64_t chars_total = 0;
    if (!jobs || !tid || !cut) { free(jobs); free(tid); free(cut); return -1; }
    cut[0] = 0;
    cut[threads] = fsize;
    for (t = 1; t < threads; t++) {
        long p = fsize / threads * t;
        if (p < cut[t - 1]) p = cut[t - 1];
        if (fastq) p = fastq_cut(data, cut[t - 1], fsize, p);
        else
        while (p < fsize && !(data[p] == '>' && p > 0 && (data[p - 1] == '\n' || data[p - 1] == '\r'))) p++;
        cut[t] = p;
    }
    for (t = 0; t < threads; t++) {
        jobs[t].data = data + cut[t];
        jobs[t].size = cut[t + 1] - cut[t];
        jobs[t].acgt_only = acgt_only;
        jobs[t].min_len = min_len;
        jobs[t].first_number = first_number;
        jobs[t].log_limit = log_limit;
        jobs[t].log = t == 0 ? log : NULL;
        jobs[t].fastq = fastq;
        if (pthread_create(&tid[t], NULL, load_job_run, &jobs[t]) != 0) { load_job_run(&jobs[t]); tid[t] = 0; }
    }
    for (t = 0; t < threads; t++) if (tid[t]) pthread_join(tid[t], NULL);
    for (t = 0; t < threads; t++) {
        if (jobs[t].n < 0) { bad = jobs[t].n == FASTQ_INVALID ? FASTQ_INVALID : -1; jobs[t].n = 0; }
        total += jobs[t].n;
        chars_total += jobs[t].set.total;
    }
    memset(out, 0, sizeof(*out));
    out->file_bytes = fsize;
    if (quals_out) *quals_out = NULL;
    if (total > 0 && !bad) {
        char *quals = NULL;
        out->recs = (slh_record *)slh_big_malloc((size_t)total * sizeof(slh_record));
        out->offsets = (uint64_t *)slh_big_malloc(((size_t)total + 1) * sizeof(uint64_t));
        out->chars = (char *)slh_big_malloc(chars_total + 16);
        if (fastq) quals = (char *)slh_big_malloc(chars_total + 16);
        if (!out->recs || !out->offsets || !out->chars || (fastq && !quals)) { ok = 0; free(quals); }
        else {
            uint64_t cpos = 0;
            int rpos = 0;
            for (t = 0; t < threads; t++) { /* where every piece goes; then the pieces are copied by the threads again */
                slh_seqset *s = &jobs[t].set;
                jobs[t].dst = out;
                jobs[t].dst_cpos = cpos;
                jobs[t].dst_rpos = rpos;
                jobs[t].dst_quals = quals;
                if (jobs[t].n == 0) continue;
                cpos += s->total;
                rpos += s->num;
                if (s->name_arena) { /* the names stay where they are: chain the arenas */
                    name_chunk *last = (name_chunk *)s->name_arena;
                    while (last->next) last = last->next;
                    last->next = (name_chunk *)out->name_arena;
                    out->name_arena = s->name_arena;
                    s->name_arena = NULL;
                }
            }
            for (t = 0; t < threads; t++)
                if (pthread_create(&tid[t], NULL, concat_job_run, &jobs[t]) != 0) { concat_job_run(&jobs[t]); tid[t] = 0; }
            for (t = 0; t < threads; t++) if (tid[t]) pthread_join(tid[t], NULL);
            out->offsets[total] = cpos;
            memset(out->chars + cpos, 0, 16);
            if (quals) memset(quals + cpos, 0, 16);
            out->total = cpos;
            out->num = total;
            if (quals_out) *quals_out = quals;
            else free(quals);
        }
    }
    for (t = 0; t < threads; t++) { slh_free_seqset(&jobs[t].set); free(jobs[t].quals); }
    free(jobs); free(tid); free(cut);
    if (bad) { slh_free_seqset(out); return bad; }
    if (!ok) { slh_free_seqset(out); return -1; }
    return total;
}

/* fastq_ok: a file whose first byte is '@' is read as FASTQ (a query file) or refused by name (the reference file); without
 * it such a file is what it was before FASTQ was read: "not FASTA" */
static int load_file(const char *path, int merge, int acgt_only, uint32_t min_len, const char *name_filter, int first_number,
                     long log_limit, slh_seqset *out, char **quals_out, int fastq_ok, FILE *log) {
    FILE *f;
    unsigned char *data = NULL;
    long fsize;
    int n, threads, mapped = 0;
    memset(out, 0, sizeof(*out));
    if (quals_out) *quals_out = NULL;
    if (log) fprintf(log, "> Loading sequences from file <%s> ... ", path);
    f = fopen(path, "rb");
    if (!f) {
        if (log) fprintf(log, "\n> WARNING: Sequence file not found\n");
        return 0;
    }
    fseek(f, 0L, SEEK_END);
    fsize = ftell(f);
    rewind(f);
    if (log) fprintf(log, "(%ld bytes)\n", fsize);
    /* map the file instead of copying it: the parser threads fault its pages in parallel */
    if (fsize > 0) {
        void *m = mmap(NULL, (size_t)fsize, PROT_READ, MAP_PRIVATE, fileno(f), 0);
        if (m != MAP_FAILED) { data = (unsigned char *)m; mapped = 1; }
    }
    if (!mapped) {
        data = (unsigned char *)malloc(fsize > 0 ? (size_t)fsize : 1);
        if (!data || (fsize > 0 && fread(data, 1, (size_t)fsize, f) != (size_t)fsize)) {
            if (log) fprintf(log, "> WARNING: Cannot read file\n");
            free(data);
            fclose(f);
            return 0;
        }
    }
    fclose(f);
    threads = slh_thread_count();
    if (fastq_ok && fsize > 0 && data[0] == '@') {
        char *quals = NULL;
        if (merge) {
            if (log) fprintf(log, "> ERROR: The reference file is FASTQ: the reference must be FASTA\n");
            n = -1;
        } else {
            n = -1;
            if (threads > 1 && fsize > (64L << 20) && log_limit > 0)
                n = load_parallel(data, fsize, acgt_only, min_len, first_number, log_limit, out, log, threads, 1, &quals);
            if (n == -1) n = load_fastq_mem(data, fsize, acgt_only, min_len, first_number, log_limit, out, &quals, log);
            if (n == FASTQ_INVALID && log) fprintf(log, "> ERROR: Invalid FASTQ file\n");
            if (n == FASTQ_NOMEM && log) fprintf(log, "\n> ERROR: Out of memory while loading sequences\n");
            if (n < 0) n = -1;
            if (quals_out) *quals_out = quals;
            else free(quals);
        }
    } else
    if (!merge && threads > 1 && fsize > (64L << 20) && log_limit > 0 && data[0] == '>') {
        n = load_parallel(data, fsize, acgt_only, min_len, first_number, log_limit, out, log, threads, 0, NULL);
        if (n < 0) n = load_mem(data, fsize, merge, acgt_only, min_len, name_filter, first_number, log_limit, out, log);
    } else {
        n = load_mem(data, fsize, merge, acgt_only, min_len, name_filter, first_number, log_limit, out, log);
    }
    if (mapped) munmap(data, (size_t)fsize);
    else free(data);
    return n;
}

int slh_load_file(const char *path, int merge, int acgt_only, uint32_t min_len, const char *name_filter,
                  int first_number, long log_limit, slh_seqset *out, FILE *log) {
    return load_file(path, merge, acgt_only, min_len, name_filter, first_number, log_limit, out, NULL, 0, log);
}

int slh_load_file_q(const char *path, int merge, int acgt_only, uint32_t min_len, const char *name_filter,
                    int first_number, long log_limit, slh_seqset *out, char **quals_out, FILE *log) {
    return load_file(path, merge, acgt_only, min_len, name_filter, first_number, log_limit, out, quals_out, 1, log);
}

/* ---- a query file in pieces ----------------------------------------------------------------------------------
 * The same records as slh_load_file(path, 0, ...), handed out as consecutive sequence sets of about piece_bytes of the
 * file each (cut at "newline + '>'"), so that a front end can search the first reads while the rest is still parsed.
 * Every piece is parsed by all host threads (load_parallel).  The "> Loading ..." line and the per-record lines (first
 * piece only; they are limited to the first log_limit records anyway) go to `log` as with slh_load_file. */
struct slh_pieces {
    unsigned char *data;
    long fsize, pos, piece_bytes;
    int mapped, acgt_only, first_number, threads, first;
    uint32_t min_len;
    long log_limit;
    FILE *log;
    int release_parsed; /* drop the file pages of a piece once it is parsed (slh_pieces_release_parsed) */
    int fastq;          /* slh_pieces_next_q found a '@' at the file's start: its records are FASTQ */
};

slh_pieces *slh_pieces_open(const char *path, int acgt_only, uint32_t min_len, int first_number, long log_limit,
                            long piece_bytes, FILE *log) {
    slh_pieces *p = (slh_pieces *)calloc(1, sizeof(slh_pieces));
    FILE *f;
    if (!p) return NULL;
    if (log) fprintf(log, "> Loading sequences from file <%s> ... ", path);
    f = fopen(path, "rb");
    if (!f) {
        if (log) fprintf(log, "\n> WARNING: Sequence file not found\n");
        free(p);
        return NULL;
    }
    fseek(f, 0L, SEEK_END);
    p->fsize = ftell(f);
    rewind(f);
    if (log) fprintf(log, "(%ld bytes)\n", p->fsize);
    if (p->fsize > 0) {
        void *m = mmap(NULL, (size_t)p->fsize, PROT_READ, MAP_PRIVATE, fileno(f), 0);
        if (m != MAP_FAILED) { p->data = (unsigned char *)m; p->mapped = 1; }
    }
    if (!p->mapped) {
        p->data = (unsigned char *)malloc(p->fsize > 0 ? (size_t)p->fsize : 1);
        if (!p->data || (p->fsize > 0 && fread(p->data, 1, (size_t)p->fsize, f) != (size_t)p->fsize)) {
            if (log) fprintf(log, "> WARNING: Cannot read file\n");
            free(p->data);
            free(p);
            fclose(f);
            return NULL;
        }
    }
    fclose(f);
    p->piece_bytes = piece_bytes > (1L << 20) ? piece_bytes : (1L << 20);
    p->acgt_only = acgt_only;
    p->min_len = min_len;
    p->first_number = first_number;
    p->log_limit = log_limit;
    p->log = log;
    p->threads = slh_thread_count();
    p->first = 1;
    return p;
}

/* the next piece: number of records (> 0), 0 at the end of the file (or when the file holds no record at all).  fastq_ok (and
 * quals_out) as for load_file; -1: the file is no valid FASTQ, said on the log */
static int pieces_next(slh_pieces *p, slh_seqset *out, char **quals_out, int fastq_ok) {
    memset(out, 0, sizeof(*out));
    if (quals_out) *quals_out = NULL;
    if (p->first && fastq_ok && p->fsize > 0 && p->data[0] == '@') p->fastq = 1;
    while (p->pos < p->fsize) {
        long start = p->pos, end = start + p->piece_bytes;
        int n;
        if (end >= p->fsize) end = p->fsize;
        else if (p->fastq) end = fastq_cut(p->data, start, p->fsize, end); /* (start is a record start: lines are counted from it) */
        else {
            while (end < p->fsize && !(p->data[end] == '>' && (p->data[end - 1] == '\n' || p->data[end - 1] == '\r'))) end++;
        }
        p->pos = end;
        if (p->first && !p->fastq && p->data[start] != '>') {  /* as load_mem: a file that does not start with '>' is not FASTA */
            if (p->log) fprintf(p->log, "> WARNING: Invalid FASTA file\n");
            p->pos = p->fsize;
            return 0;
        }
        if (p->fastq) {
            char *quals = NULL;
            n = -1;
            if (p->threads > 1 && end - start > (16L << 20) && p->log_limit > 0)
                n = load_parallel(p->data + start, end - start, p->acgt_only, p->min_len, p->first_number, p->log_limit, out,
                                  p->first ? p->log : NULL, p->threads, 1, &quals);
            if (n == -1)
                n = load_fastq_mem(p->data + start, end - start, p->acgt_only, p->min_len, p->first_number, p->log_limit, out, &quals,
                                   p->first ? p->log : NULL);
            if (n < 0) {
                if (p->log) fprintf(p->log, n == FASTQ_INVALID ? "> ERROR: Invalid FASTQ file\n" : "\n> ERROR: Out of memory while loading sequences\n");
                p->pos = p->fsize;
                return -1;
            }
            if (quals_out) *quals_out = quals;
            else free(quals);
        } else {
        if (p->threads > 1 && end - start > (16L << 20) && p->log_limit > 0)
            n = load_parallel(p->data + start, end - start, p->acgt_only, p->min_len, p->first_number, p->log_limit, out,
                              p->first ? p->log : NULL, p->threads, 0, NULL);
        else n = -1;
        if (n < 0)
            n = load_mem(p->data + start, end - start, 0, p->acgt_only, p->min_len, NULL, p->first_number, p->log_limit, out,
                         p->first ? p->log : NULL);
        }
        p->first = 0;
        if (p->release_parsed && p->mapped && end - start > (1L << 20)) { /* the parsed part of the file is not read again */
            long a = (start + 4095) & ~4095L, b = end & ~4095L;
            if (b > a) (void)madvise(p->data + a, (size_t)(b - a), MADV_DONTNEED);
        }
        if (n > 0) { p->first_number += n; return n; }
        /* a piece without an accepted record (all too short / empty): go on */
    }
    return 0;
}

int slh_pieces_next(slh_pieces *p, slh_seqset *out) { return pieces_next(p, out, NULL, 0); }

int slh_pieces_next_q(slh_pieces *p, slh_seqset *out, char **quals_out) { return pieces_next(p, out, quals_out, 1); }

void slh_pieces_release_parsed(slh_pieces *p, int on) {
    if (p) p->release_parsed = on;
}

void slh_pieces_close(slh_pieces *p) {
    if (!p) return;
    if (p->mapped) munmap(p->data, (size_t)p->fsize);
    else free(p->data);
    free(p);
}

int slh_seq_id_from_merged_pos(const uint32_t *starts, int num, uint32_t *pos) {
    int lo = 0, hi = num - 1;
    while (lo != hi) { /* binary search for the last start <= pos */
        int mid = (lo + hi + 1) / 2;
        if (*pos >= starts[mid]) lo = mid;
        else hi = mid - 1;
    }
    *pos -= starts[lo];
    return lo;
}

int slh_next_piece(const slh_record *recs, const uint32_t *merged_start, int num, int *r, uint64_t *x, uint64_t range_end,
                   slh_piece *out) {
    while (*r < num) {
        const uint64_t start = num > 1 ? merged_start[*r] : 0, end = start + recs[*r].size;
        if (end <= *x) { (*r)++; continue; }
        if (start >= range_end || *x >= range_end) return 0;
        out->rec = *r;
        out->start = start;
        out->a = start > *x ? start : *x;
        out->b = end < range_end ? end : range_end;
        out->ends_record = out->b == end;
        *x = out->b;
        if (out->ends_record) (*r)++;
        return 1;
    }
    return 0;
}

/* ------------------------------------------------------------------------------------------------ */
/* options                                                                                           */
/* ------------------------------------------------------------------------------------------------ */

int slh_parse_argument(int argc, char **argv, const char *optionchars, int parse) {
    char uc[2] = {0, 0}, lc[2] = {0, 0};
    int i;
    for (i = 0; i < 2 && optionchars[i] != '\0'; i++) { /* only the first two characters of the option name count */
        char ch = optionchars[i];
        if (ch >= 'A' && ch <= 'Z') { uc[i] = ch; lc[i] = (char)(ch + 32); }
        else { uc[i] = (char)(ch - 32); lc[i] = ch; }
    }
    for (i = 1; i < argc; i++) {
        const char *a = argv[i];
        /* a one-letter option must be exactly two characters long: its third must equal the '\0' in uc[1] */
        if (a[0] == '-' && a[1] != '\0' && (a[1] == lc[0] || a[1] == uc[0]) && (a[2] == lc[1] || a[2] == uc[1])) {
            if (parse) {
                if (i == argc - 1) return -1; /* nothing in front of it */
                if (parse == 1) return atoi(argv[i + 1]);
                return i + 1;
            }
            return 1;
        }
    }
    return parse ? -1 : 0;
}

/* The options, one row each.  An argument is an option of a row when its first two letters are the row's (either case; a
 * one-letter row: when it is exactly two characters long) and the third-letter rule holds.  Everything that has to know an
 * option reads it here: which arguments are file names (slh_parse_options), the value and its range (option_value), the
 * refusal of a bad value and of a second mode (slh_parse_run). */
enum { V_NONE, V_INT, V_POW2, V_DIGITS, V_LEVELS, V_COSTS, V_ATOI, V_INDEX, V_STRING };
typedef struct {
    const char *name;   /* as usage() spells it; "l": a one-letter option */
    char third, unless; /* third == 1: the third letter is name[2] (-maxed, -dedup; -sv: the name ends there); third == 2: the whole name
                           counts (-svmin, -svmis, -svslots); unless: the third letter is not this one (-mam, -depth) */
    char kind;          /* V_NONE: no value.  V_INT: strtol's whole number in [lo, hi]; V_POW2: such a power of two; V_DIGITS: a number
                           that begins with a digit; V_LEVELS: 1 to 16 of those, ascending, with commas; V_COSTS: three of those with
                           commas, X in 1..31, O in 0..63, E in 1..31, handed out as X | O << 8 | E << 16; V_ATOI, V_INDEX, V_STRING:
                           the reference's -l and -m (atoi), -o and -v (where the value stands) and -r */
    char mode;          /* the match type the option selects (0: none) */
    uint64_t lo, hi;
    long long dflt;     /* what the entry points hand out when the option is absent */
    const char *refusal; /* of a bad value; a mode's: of another mode beside it */
} option_row;
enum { O_MEM, O_MAM, O_MUM, O_SMEM, O_OCC, O_CHAIN, O_MGAP, O_EXT, O_PEN, O_XDROP, O_ALN, O_MAXED, O_PAF, O_SAM, O_PILE, O_MINQ, O_BQ,
       O_SITES, O_MDEP, O_MPCT, O_VCF, O_CONS, O_DEPTH, O_LEV, O_WIN, O_DEDUP, O_DSLOTS, O_GT, O_PLOIDY, O_ERR, O_HETQ, O_QUAL, O_SB, O_FS, O_WQ, O_EVS, O_STATS, O_AFFINE, O_GEXT,
       O_SV, O_SVMIN, O_SVMIS, O_SVSLOTS,
       O_L, O_O, O_B, O_N, O_M, O_R, O_V, O_S, O_C, NUM_OPTIONS };
#define PEN_XDROP "Option -pen needs a whole number of at least 1, option -xdrop one of at least 0"
static const option_row OPTIONS[NUM_OPTIONS] = {
    [O_MEM] = {"mem", 0, 0, V_NONE, 0, 0, 0, 0, NULL},
    [O_MAM] = {"mam", 0, 'x', V_NONE, 1, 0, 0, 0, NULL},
    [O_MUM] = {"mum", 0, 0, V_NONE, 2, 0, 0, 0, NULL},
    [O_SMEM] = {"smem", 0, 0, V_NONE, 3, 0, 0, 0, "Option -smem excludes -mam and -mum"},
    [O_OCC] = {"occ", 0, 0, V_INT, 0, 1, 0x7FFFFFFF, 0, "Option -occ needs a whole number of at least 1"},
    [O_CHAIN] = {"chain", 0, 0, V_NONE, 4, 0, 0, 0, "Option -chain excludes -mam, -mum and -smem"},
    [O_MGAP] = {"mgap", 0, 0, V_INT, 0, 1, 0x7FFFFFFF, 0, "Option -mgap needs a whole number of at least 1"},
    [O_EXT] = {"ext", 0, 0, V_NONE, 5, 0, 0, 0, "Option -ext excludes -mam, -mum, -smem and -chain"},
    [O_PEN] = {"pen", 0, 0, V_INT, 0, 1, 0x7FFFFFFF, 0, PEN_XDROP},
    [O_XDROP] = {"xdrop", 0, 0, V_INT, 0, 0, 0x7FFFFFFF, -1, PEN_XDROP},
    [O_ALN] = {"aln", 0, 0, V_NONE, 6, 0, 0, 0, "Option -aln excludes -mam, -mum, -smem, -chain and -ext"},
    [O_MAXED] = {"maxed", 1, 0, V_INT, 0, 0, 127, -1, "Option -maxed needs a whole number from 0 to 127"},
    [O_PAF] = {"paf", 0, 0, V_NONE, 7, 0, 0, 0, "Option -paf excludes -mam, -mum, -smem, -chain, -ext and -aln"},
    [O_SAM] = {"sam", 0, 0, V_NONE, 7, 0, 0, 0, "Option -sam excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites, -vcf, -cons and -depth"},
    [O_PILE] = {"pile", 0, 0, V_NONE, 8, 0, 0, 0, "Option -pile excludes -mam, -mum, -smem, -chain, -ext, -aln and -paf"},
    [O_MINQ] = {"minq", 0, 0, V_INT, 0, 0, 60, 0, "Option -minq needs a whole number from 0 to 60"},
    [O_BQ] = {"bq", 0, 0, V_INT, 0, 0, 93, 0, "Option -bq needs a whole number from 0 to 93"},
    [O_SITES] = {"sites", 0, 0, V_NONE, 8, 0, 0, 0, "Option -sites excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf and -pile"},
    [O_MDEP] = {"mdep", 0, 0, V_INT, 0, 1, 0x7FFFFFFF, 4, "Option -mdep needs a whole number of at least 1"},
    [O_MPCT] = {"mpct", 0, 0, V_INT, 0, 0, 100, 20, "Option -mpct needs a whole number from 0 to 100"},
    [O_VCF] = {"vcf", 0, 0, V_NONE, 8, 0, 0, 0, "Option -vcf excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile and -sites"},
    [O_CONS] = {"cons", 0, 0, V_NONE, 8, 0, 0, 0, "Option -cons excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites and -vcf"},
    [O_DEPTH] = {"depth", 0, 'd', V_NONE, 8, 0, 0, 0, "Option -depth excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites, -vcf and -cons"},
    [O_LEV] = {"lev", 0, 0, V_LEVELS, 0, 1, 0xFFFFFFFFull, 0, "Option -lev needs 1 to 16 whole numbers of at least 1, ascending, separated by commas"},
    [O_WIN] = {"win", 0, 0, V_DIGITS, 0, 1, UINT64_MAX, 0, "Option -win needs a whole number of at least 1"},
    [O_DEDUP] = {"dedup", 1, 0, V_NONE, 0, 0, 0, 0, NULL},
    [O_DSLOTS] = {"dslots", 0, 0, V_POW2, 0, 64, 1ull << 32, 0, "Option -dslots needs a power of two of at least 64"},
    [O_GT] = {"gt", 0, 0, V_NONE, 0, 0, 0, 0, NULL},
    [O_PLOIDY] = {"ploidy", 0, 0, V_INT, 0, 1, 2, 2, "Option -ploidy needs 1 or 2"},
    [O_ERR] = {"err", 0, 0, V_INT, 0, 1, 93, 20, "Option -err needs a whole number from 1 to 93"},
    [O_HETQ] = {"hetq", 0, 0, V_INT, 0, 0, 999, 30, "Option -hetq needs a whole number from 0 to 999"},
    [O_QUAL] = {"qual", 0, 0, V_INT, 0, 0, 999, 20, "Option -qual needs a whole number from 0 to 999"},
    [O_SB] = {"sb", 0, 0, V_NONE, 0, 0, 0, 0, NULL},
    [O_FS] = {"fs", 0, 0, V_INT, 0, 0, 999, -1, "Option -fs needs a whole number from 0 to 999"},
    [O_WQ] = {"wq", 0, 0, V_NONE, 0, 0, 0, 0, NULL},
    [O_EVS] = {"evs", 0, 0, V_POW2, 0, 64, 1ull << 31, 0, "Option -evs needs a power of two of at least 64"},
    [O_STATS] = {"stats", 0, 0, V_NONE, 7, 0, 0, 0, "Option -stats excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -sam, -pile, -sites, -vcf, -cons and -depth"},
    [O_AFFINE] = {"affine", 0, 0, V_COSTS, 0, 0, 0, -1, "Option -affine needs three whole numbers X,O,E: X from 1 to 31, O from 0 to 63, E from 1 to 31, separated by commas"},
    [O_GEXT] = {"gext", 0, 0, V_INT, 0, 1, 31, 0, "Option -gext needs a whole number from 1 to 31"},
    [O_SV] = {"sv", 1, 0, V_NONE, 0, 0, 0, 0, NULL},
    [O_SVMIN] = {"svmin", 2, 0, V_INT, 0, 1, 0x7FFFFFFF, -1, "Option -svmin needs a whole number of at least 1"},
    [O_SVMIS] = {"svmis", 2, 0, V_INT, 0, 0, 64, 3, "Option -svmis needs a whole number from 0 to 64"},
    [O_SVSLOTS] = {"svslots", 2, 0, V_POW2, 0, 64, 1ull << 31, 0, "Option -svslots needs a power of two of at least 64"},
    [O_L] = {"l", 0, 0, V_ATOI, 0, 0, 0, 20, NULL},
    [O_O] = {"o", 0, 0, V_INDEX, 0, 0, 0, -1, NULL},
    [O_B] = {"b", 0, 0, V_NONE, 0, 0, 0, 0, NULL},
    [O_N] = {"n", 0, 0, V_NONE, 0, 0, 0, 0, NULL},
    [O_M] = {"m", 0, 0, V_ATOI, 0, 0, 0, 0, NULL},
    [O_R] = {"r", 0, 0, V_STRING, 0, 0, 0, 0, NULL},
    [O_V] = {"v", 0, 0, V_INDEX, 0, 0, 0, -1, NULL},
    [O_S] = {"s", 0, 0, V_NONE, 0, 0, 0, 0, NULL},
    [O_C] = {"c", 0, 0, V_NONE, 0, 0, 0, 0, NULL},
};
/* the modes that exclude each other, beside -mam and -mum; a refusal names the last of them that is given */
static const int MODES[] = {O_SMEM, O_CHAIN, O_EXT, O_ALN, O_PAF, O_PILE, O_SITES, O_VCF, O_CONS, O_DEPTH, O_SAM, O_STATS};
#define NUM_MODES ((int)(sizeof(MODES) / sizeof(MODES[0])))

static char lower(char c) { return c >= 'A' && c <= 'Z' ? (char)(c + 32) : c; }

static int is_option(const char *a, int id) {
    const option_row *r = &OPTIONS[id];
    if (a[0] != '-' || a[1] == '\0' || lower(a[1]) != r->name[0]) return 0;
    if (r->name[1] == '\0') return a[2] == '\0';
    if (lower(a[2]) != r->name[1]) return 0;
    if (r->third == 2) {
        size_t k;
        for (k = 2; r->name[k] != '\0' && lower(a[k + 1]) == r->name[k]; k++) {}
        return r->name[k] == '\0' && a[k + 1] == '\0';
    }
    if (r->third) return lower(a[3]) == r->name[2];
    return !r->unless || lower(a[3]) != r->unless;
}

/* the row of an argument, or -1 */
static int option_of(const char *a) {
    int id;
    for (id = 0; id < NUM_OPTIONS; id++)
        if (is_option(a, id)) return id;
    return -1;
}

static int has_option(int argc, char **argv, int id) {
    int i;
    for (i = 1; i < argc; i++)
        if (is_option(argv[i], id)) return 1;
    return 0;
}

int slh_option_info(int k, const char **name_out) {
    if (k < 0 || k >= NUM_OPTIONS) return -1;
    *name_out = OPTIONS[k].name;
    return OPTIONS[k].kind != V_NONE;
}

/* The value `a` of a row that takes a checked one: 0 and *out (V_LEVELS: the list in levels, its length in *out), or -1 and
 * *out as it was. */
static int option_value(const option_row *r, const char *a, uint64_t *out, uint32_t *levels) {
    const int digits = r->kind == V_DIGITS || r->kind == V_LEVELS;
    uint64_t v, k = 0;
    char *end;
    if (r->kind == V_COSTS) {
        static const uint64_t lo[3] = {1, 0, 1}, hi[3] = {31, 63, 31};
        uint64_t packed = 0;
        for (k = 0; k < 3; k++) {
            if (a[0] < '0' || a[0] > '9') return -1;
            errno = 0;
            v = strtoull(a, &end, 10);
            if (errno != 0 || v < lo[k] || v > hi[k] || *end != (k < 2 ? ',' : '\0')) return -1;
            packed |= v << (8 * k);
            a = end + 1;
        }
        *out = packed;
        return 0;
    }
    for (;;) {
        errno = 0;
        if (digits) {
            if (a[0] < '0' || a[0] > '9') return -1;
            v = strtoull(a, &end, 10);
        } else {
            const long long s = strtoll(a, &end, 10);
            if (s < 0) return -1;
            v = (uint64_t)s;
        }
        if (errno != 0 || end == a || v < r->lo || v > r->hi || (r->kind == V_POW2 && (v & (v - 1)) != 0)) return -1;
        if (r->kind != V_LEVELS) break;
        if (k == 16 || (k && (uint32_t)v <= levels[k - 1])) return -1;
        levels[k++] = (uint32_t)v;
        if (*end != ',') break; /* a number, then a comma and the next one, or the end */
        a = end + 1;
    }
    if (*end != '\0') return -1;
    *out = r->kind == V_LEVELS ? k : v;
    return 0;
}

/* Looks for the n rows ids[] among the arguments.  vals[k] starts as row k's default and takes its value, which is not looked
 * at as an option again; first_only: the first of the rows that is found ends the search.  Returns the rows seen as bits (bit k:
 * ids[k]), or -(k + 1) when the value of row k is missing or refused. */
static int scan_options(int argc, char **argv, const int *ids, int n, int first_only, uint64_t *vals, uint32_t *levels) {
    int i, k, seen = 0;
    for (k = 0; k < n; k++) vals[k] = (uint64_t)OPTIONS[ids[k]].dflt;
    for (i = 1; i < argc; i++) {
        for (k = 0; k < n && !is_option(argv[i], ids[k]); k++) {}
        if (k == n) continue;
        seen |= 1 << k;
        if (OPTIONS[ids[k]].kind == V_NONE) continue;
        if (i == argc - 1 || option_value(&OPTIONS[ids[k]], argv[i + 1], &vals[k], levels)) return -(k + 1);
        if (first_only) break;
        i++;
    }
    return seen;
}

/* the entry points with one whole number: 0 absent, 1 there, -1 refused */
static int scan_one(int argc, char **argv, int id, uint64_t *val) {
    return scan_options(argc, argv, &id, 1, 1, val, NULL);
}
static int scan_whole(int argc, char **argv, int id, int *out) {
    uint64_t v;
    const int rc = scan_one(argc, argv, id, &v);
    *out = (int)(long long)v;
    return rc;
}
int slh_parse_max_occ(int argc, char **argv, int *out) { return scan_whole(argc, argv, O_OCC, out); }
int slh_parse_max_gap(int argc, char **argv, int *out) { return scan_whole(argc, argv, O_MGAP, out); }
int slh_parse_max_edits(int argc, char **argv, int *out) { return scan_whole(argc, argv, O_MAXED, out); }
int slh_parse_min_mapq(int argc, char **argv, int *out) { return scan_whole(argc, argv, O_MINQ, out); }
int slh_parse_min_bq(int argc, char **argv, int *out) { return scan_whole(argc, argv, O_BQ, out); }
int slh_parse_event_slots(int argc, char **argv, uint64_t *out) { return scan_one(argc, argv, O_EVS, out); }
int slh_parse_depth(int argc, char **argv) { return has_option(argc, argv, O_DEPTH); }

/* ... and those with several options, each of which may stand more than once (the last one counts) */
static int scan_ints(int argc, char **argv, const int *ids, int n, int **outs) {
    uint64_t v[4];
    const int rc = scan_options(argc, argv, ids, n, 0, v, NULL);
    int k;
    for (k = 0; k < n; k++) *outs[k] = (int)(long long)v[k];
    return rc > 0 ? 1 : rc;
}
int slh_parse_ext_params(int argc, char **argv, int *penalty_out, int *xdrop_out) {
    static const int ids[2] = {O_PEN, O_XDROP};
    int *outs[2] = {penalty_out, xdrop_out};
    const int rc = scan_ints(argc, argv, ids, 2, outs);
    return rc < 0 ? -1 : rc;
}
int slh_parse_sites_params(int argc, char **argv, int *min_depth_out, int *min_pct_out) {
    static const int ids[2] = {O_MDEP, O_MPCT};
    int *outs[2] = {min_depth_out, min_pct_out};
    return scan_ints(argc, argv, ids, 2, outs);
}
int slh_parse_gt_params(int argc, char **argv, int *ploidy_out, int *err_out, int *hetq_out, int *qual_out) {
    static const int ids[4] = {O_PLOIDY, O_ERR, O_HETQ, O_QUAL};
    int *outs[4] = {ploidy_out, err_out, hetq_out, qual_out};
    return scan_ints(argc, argv, ids, 4, outs);
}
int slh_parse_sb_params(int argc, char **argv, int *fs_out) {
    static const int ids[2] = {O_SB, O_FS};
    uint64_t v[2];
    const int rc = scan_options(argc, argv, ids, 2, 0, v, NULL);
    *fs_out = (int)(long long)v[1];
    return rc < 0 ? -1 : rc;
}
int slh_parse_affine(int argc, char **argv, int *x_out, int *o_out, int *e_out) {
    uint64_t v;
    const int rc = scan_one(argc, argv, O_AFFINE, &v);
    *x_out = rc > 0 ? (int)(v & 0xFF) : 0;
    *o_out = rc > 0 ? (int)((v >> 8) & 0xFF) : 0;
    *e_out = rc > 0 ? (int)((v >> 16) & 0xFF) : 0;
    return rc;
}
int slh_parse_gext(int argc, char **argv, int *out) { return scan_whole(argc, argv, O_GEXT, out); }
/* -sv and its three values: bit 0 -sv, bit 1 -svmin, bit 2 -svmis, bit 3 -svslots; -(k + 1): the value of row k is refused.
 * *min_len_out is -1 when -svmin is absent (the caller's default is maxed + 1). */
int slh_parse_sv(int argc, char **argv, int *min_len_out, int *max_mis_out, uint64_t *slots_out) {
    static const int ids[4] = {O_SV, O_SVMIN, O_SVMIS, O_SVSLOTS};
    uint64_t v[4];
    const int rc = scan_options(argc, argv, ids, 4, 0, v, NULL);
    *min_len_out = (int)(long long)v[1];
    *max_mis_out = (int)(long long)v[2];
    *slots_out = v[3];
    return rc;
}
uint32_t slh_aln_word(int max_edits, int affine, int x, int o, int e) {
    if (!affine) return max_edits >= 0 ? (uint32_t)max_edits : SLAMEM_ALN_EDITS_DEFAULT;
    return SLAMEM_ALN_AFFINE(max_edits >= 0 ? max_edits : 31, x, o, e);
}
int slh_aln_word_decode(uint32_t word, uint32_t *fields_out, int *affine_out) {
    return slamem_decode_aln_word(word, &fields_out[0], &fields_out[1], &fields_out[2], &fields_out[3], affine_out);
}
int slh_parse_wq(int argc, char **argv) { return has_option(argc, argv, O_WQ); }
int slh_parse_stats(int argc, char **argv) { return has_option(argc, argv, O_STATS); }
int slh_parse_dedup(int argc, char **argv, uint64_t *slots_out) {
    static const int ids[2] = {O_DEDUP, O_DSLOTS};
    uint64_t v[2];
    const int rc = scan_options(argc, argv, ids, 2, 0, v, NULL);
    *slots_out = v[1];
    return rc < 0 ? -1 : rc;
}
int slh_parse_depth_params(int argc, char **argv, uint32_t *levels_out, int *num_levels_out, uint64_t *window_out) {
    static const int ids[2] = {O_LEV, O_WIN};
    uint64_t v[2];
    const int rc = scan_options(argc, argv, ids, 2, 0, v, levels_out);
    *num_levels_out = (int)v[0];
    *window_out = v[1];
    return rc;
}

/* the -r string (slamem.c:605-629): the argument at i, or when it opens with a quote the arguments up to the one that closes it,
 * joined by blanks; copied to out when out is not NULL.  Returns its length; *i: the last argument it took (argc: none closed it) */
static int ref_name_string(int argc, char **argv, int *i, char *out) {
    int j = 0, n = 0;
    char oc = argv[*i][0];
    if (oc == '\'' || oc == '\"') j = 1;
    else oc = '\0';
    while (argv[*i][j] != oc) {
        if (argv[*i][j] == '\0') {
            (*i)++;
            if (*i == argc) break;
            j = 0;
            if (out) out[n] = ' ';
        } else {
            if (out) out[n] = argv[*i][j];
            j++;
        }
        n++;
    }
    if (out) out[n] = '\0';
    return n;
}

int slh_parse_options(int argc, char **argv, slh_options *o) {
    int i, k, n = 0, ref_arg;
    memset(o, 0, sizeof(*o));
    o->image_arg = o->out_arg = -1;
    o->min_mem_len = 20;
    if (argc < 3) { o->usage = 1; return 0; }
    o->hidden_sort = has_option(argc, argv, O_S);
    o->hidden_clean = has_option(argc, argv, O_C);
    o->file_args = (int *)calloc((size_t)argc, sizeof(int));
    if (!o->file_args) return -1;
    for (i = 1; i < argc; i++) { /* which arguments are FASTA files (slamem.c:574-600) */
        int id;
        char oc;
        if (argv[i][0] != '-') { o->file_args[o->num_files++] = i; continue; }
        id = option_of(argv[i]);
        oc = lower(argv[i][1]);
        if (id == O_VCF) continue; /* (the one option that begins with l/o/m/v and takes no value) */
        /* the reference's rule: any option that begins with l/o/m/v takes the next argument, -mam and -mum included */
        if (oc == 'l' || oc == 'o' || oc == 'm' || oc == 'v' || (id >= 0 && id != O_R && OPTIONS[id].kind != V_NONE)) i++;
        else if (oc == 'r') { /* ... and any that begins with r a string */
            if (++i == argc) break;
            n = ref_name_string(argc, argv, &i, NULL);
        }
    }
    o->no_ns = has_option(argc, argv, O_N);
    o->min_seq_len = slh_parse_argument(argc, argv, "M", 1);
    if (o->min_seq_len == -1) o->min_seq_len = 0;
    ref_arg = slh_parse_argument(argc, argv, "R", 2);
    if (ref_arg != -1) { /* slamem.c:605-629 */
        o->ref_name_given = 1;
        if (n == 0) o->ref_name_empty = 1;
        else {
            o->ref_name = (char *)calloc((size_t)n + 1, 1);
            if (!o->ref_name) return -1;
            ref_name_string(argc, argv, &ref_arg, o->ref_name);
        }
    }
    o->image_arg = slh_parse_argument(argc, argv, "V", 2);
    o->match_type = has_option(argc, argv, O_MAM) ? 1 : 0;
    if (has_option(argc, argv, O_MUM)) o->match_type = o->match_type == 1 ? -1 : 2; /* the match type the reference reserves ("EAU", slamem.c:35) */
    for (k = 0; k < NUM_MODES; k++)
        if (has_option(argc, argv, MODES[k])) o->match_type = o->match_type != 0 ? -1 : OPTIONS[MODES[k]].mode;
    o->both_strands = has_option(argc, argv, O_B);
    o->min_mem_len = slh_parse_argument(argc, argv, "L", 1);
    if (o->min_mem_len == -1) o->min_mem_len = 20;
    o->out_arg = slh_parse_argument(argc, argv, "O", 2);
    return 0;
}

static int refuse(const char **refusal, const char *msg, int rc) {
    *refusal = msg;
    return rc;
}

int slh_parse_run(int argc, char **argv, slh_run *r, const char **refusal) {
    slh_options *o = &r->o;
    int t, k, occ, gap, ext, edits, mapq, sparams, gtp, dparams, evs, dd, mpct, sb, fs, aff, costs[3], gx, band, sv, svmin, svmis;
    uint64_t svslots;
    *refusal = NULL;
    memset(r, 0, sizeof(*r));
    if (slh_parse_options(argc, argv, o) != 0) return refuse(refusal, "Out of memory", -1);
    t = o->match_type;
    r->sites = has_option(argc, argv, O_SITES);
    r->vcf = has_option(argc, argv, O_VCF);
    r->cons = has_option(argc, argv, O_CONS);
    r->depth = has_option(argc, argv, O_DEPTH);
    r->sam = has_option(argc, argv, O_SAM);
    r->gt = has_option(argc, argv, O_GT);
    mpct = has_option(argc, argv, O_MPCT);
    occ = slh_parse_max_occ(argc, argv, &r->max_occ);
    gap = slh_parse_max_gap(argc, argv, &r->max_gap);
    ext = slh_parse_ext_params(argc, argv, &r->ext_pen, &r->ext_xdrop);
    edits = slh_parse_max_edits(argc, argv, &r->max_edits);
    mapq = slh_parse_min_mapq(argc, argv, &r->min_mapq);
    r->bq_given = slh_parse_min_bq(argc, argv, &r->min_bq);
    sparams = slh_parse_sites_params(argc, argv, &r->min_depth, &r->min_pct);
    if (r->depth && sparams == 0) r->min_depth = 1; /* (-depth: a position is covered when one read shows it) */
    gtp = slh_parse_gt_params(argc, argv, &r->gt_ploidy, &r->gt_err, &r->gt_hetq, &r->gt_qual);
    dparams = slh_parse_depth_params(argc, argv, r->levels, &r->num_levels, &r->window);
    evs = slh_parse_event_slots(argc, argv, &r->ev_slots);
    dd = slh_parse_dedup(argc, argv, &r->dd_slots);
    sb = slh_parse_sb_params(argc, argv, &fs); /* (the values are the caller's to ask for: slh_run keeps its layout) */
    aff = slh_parse_affine(argc, argv, &costs[0], &costs[1], &costs[2]); /* (the same) */
    gx = slh_parse_gext(argc, argv, &band); /* (the same) */
    sv = slh_parse_sv(argc, argv, &svmin, &svmis, &svslots); /* (the same) */
    r->dedup = dd > 0 && (dd & 1);
    if (o->usage || o->hidden_sort || o->hidden_clean) return 0; /* (the caller's business, before any refusal) */

    /* the refusals, the first that applies */
    if (t < 0) {
        for (k = NUM_MODES - 1; k >= 0; k--)
            if (has_option(argc, argv, MODES[k])) return refuse(refusal, OPTIONS[MODES[k]].refusal, -1);
        return refuse(refusal, "Options -mam and -mum exclude each other", -1);
    }
#define REFUSE_IF(cond, msg) do { if (cond) return refuse(refusal, msg, -1); } while (0)
    REFUSE_IF(occ < 0, OPTIONS[O_OCC].refusal);
    REFUSE_IF(occ && t != 3, "Option -occ needs -smem");
    REFUSE_IF(gap < 0, OPTIONS[O_MGAP].refusal);
    REFUSE_IF(gap && t != 4 && t != 6 && t != 7 && t != 8, "Option -mgap needs -chain");
    REFUSE_IF(ext < 0, PEN_XDROP);
    REFUSE_IF(ext && t != 5 && t != 6 && t != 7 && t != 8, "Options -pen and -xdrop need -ext");
    REFUSE_IF(edits < 0, OPTIONS[O_MAXED].refusal);
    REFUSE_IF(edits && t != 6 && t != 7 && t != 8, "Option -maxed needs -aln");
    REFUSE_IF(aff < 0, OPTIONS[O_AFFINE].refusal);
    REFUSE_IF(aff && t != 6 && t != 7 && t != 8, "Option -affine needs -aln");
    REFUSE_IF(aff && (uint32_t)(costs[1] + costs[2] * (r->max_edits >= 0 ? r->max_edits : 31)) > SLAMEM_ALN_COST_MAX,
              "Option -affine: a gap's cost is bounded by O + E * maxed, which may be at most 512");
    REFUSE_IF(gx < 0, OPTIONS[O_GEXT].refusal);
    REFUSE_IF(gx && t != 6 && t != 7 && t != 8, "Option -gext needs -aln");
    REFUSE_IF(gx && !aff, "Option -gext needs -affine");
    REFUSE_IF(mapq < 0, OPTIONS[O_MINQ].refusal);
    REFUSE_IF(mapq && t != 8 && !has_option(argc, argv, O_STATS), "Option -minq needs -pile");
    REFUSE_IF(r->bq_given < 0, OPTIONS[O_BQ].refusal);
    REFUSE_IF(r->bq_given && t != 8, "Option -bq needs -pile");
    REFUSE_IF(sparams < 0, OPTIONS[sparams == -1 ? O_MDEP : O_MPCT].refusal);
    if (sparams) {
        REFUSE_IF(r->cons && mpct, "Option -mpct has no meaning with -cons: an allele is applied when more than half of the depth shows it");
        REFUSE_IF(r->depth && mpct, "Option -mpct has no meaning with -depth: the depth is written as it is");
        REFUSE_IF(!r->sites && !r->vcf && !r->cons && !r->depth, "Options -mdep and -mpct need -sites");
    }
    REFUSE_IF(gtp < 0, OPTIONS[O_PLOIDY - 1 - gtp].refusal);
    if (gtp && !r->gt) {
        REFUSE_IF(has_option(argc, argv, O_PLOIDY), "Option -ploidy needs -gt");
        REFUSE_IF(has_option(argc, argv, O_ERR), "Option -err needs -gt");
        REFUSE_IF(has_option(argc, argv, O_HETQ), "Option -hetq needs -gt");
        REFUSE_IF(1, "Option -qual needs -gt");
    }
    REFUSE_IF(r->gt && !r->vcf, "Option -gt needs -vcf");
    REFUSE_IF(r->gt && mpct, "Option -mpct has no meaning with -gt: a call is made when its genotype's quality reaches -qual");
    REFUSE_IF(sb < 0, OPTIONS[O_FS].refusal);
    REFUSE_IF((sb & 1) && !r->gt, "Option -sb needs -gt");
    REFUSE_IF((sb & 2) && !(sb & 1), "Option -fs needs -sb");
    REFUSE_IF(has_option(argc, argv, O_WQ) && !r->gt, "Option -wq needs -gt");
    REFUSE_IF(dparams < 0, OPTIONS[dparams == -1 ? O_LEV : O_WIN].refusal);
    REFUSE_IF(dparams == 3 && r->depth, "Options -lev and -win exclude each other");
    REFUSE_IF(dparams && !r->depth, "Options -lev and -win need -depth");
    REFUSE_IF(evs < 0, OPTIONS[O_EVS].refusal);
    REFUSE_IF(evs && !r->vcf && !r->cons, "Option -evs needs -vcf");
    REFUSE_IF(dd < 0, OPTIONS[O_DSLOTS].refusal);
    REFUSE_IF(dd == 2, "Option -dslots needs -dedup");
    REFUSE_IF(dd && t != 8, "Option -dedup needs -pile, -sites, -vcf, -cons or -depth");
    REFUSE_IF(sv < 0, OPTIONS[O_SV - 1 - sv].refusal);
    REFUSE_IF((sv & 1) && !r->vcf, "Option -sv needs -vcf");
    REFUSE_IF((sv & 2) && !(sv & 1), "Option -svmin needs -sv");
    REFUSE_IF((sv & 4) && !(sv & 1), "Option -svmis needs -sv");
    REFUSE_IF((sv & 8) && !(sv & 1), "Option -svslots needs -sv");
    REFUSE_IF((sv & 1) && r->gt, "Option -sv excludes -gt");
#undef REFUSE_IF
    /* (here the caller refuses what depends on more than the arguments) */
    if (o->num_files < 2) return refuse(refusal, "Not enough input sequence files provided", -2);
    if (o->ref_name_given && o->ref_name_empty) return refuse(refusal, "No reference name string provided", -2);
    return 0;
}

char *slh_append_to_basename(const char *filename, const char *extra) {
    int n = (int)strlen(filename), i;
    char *res;
    for (i = n - 1; i > 0; i--)
        if (filename[i] == '.') break;
    if (i <= 0) i = n;
    res = (char *)calloc((size_t)i + strlen(extra) + 1, 1);
    if (!res) return NULL;
    memcpy(res, filename, (size_t)i);
    strcat(res, extra);
    return res;
}

void slh_free_options(slh_options *o) {
    free(o->ref_name);
    free(o->file_args);
    memset(o, 0, sizeof(*o));
}


/* ------------------------------------------------------------------------------------------------ */
/* output                                                                                            */
/* ------------------------------------------------------------------------------------------------ */

/* -stats: the report of the table */
int slh_write_stats(const uint64_t *t, FILE *f) {
    static const char *const names[16] = {"reads", "mapped", "forward", "reverse", "counted", "counted split", "segments", "letters",
                                          "counted letters", "matches", "mismatches", "insertions", "inserted letters", "deletions",
                                          "deleted letters", "segment letters"};
    /* histograms of one column: tag, first word, bins, whether the last bin folds */
    static const struct { const char *tag; int first, bins, folds; } one[] = {{"MQ", 24, 64, 0}, {"RL", 88, 512, 1}, {"NM", 600, 128, 1}};
    static const struct { const char *tag; int first; } lens[] = {{"IL", 2984}, {"DL", 3048}};
    const uint64_t aligned = t[9] + t[10];
    int k, i;
    for (k = 0; k < 16; k++) fprintf(f, "SN\t%s\t%llu\n", names[k], (unsigned long long)t[k]);
    fprintf(f, "SN\tclipped letters\t%llu\n", (unsigned long long)(t[8] > t[15] ? t[8] - t[15] : 0));
    fprintf(f, "SN\tmismatch rate\t%.6f\n", aligned ? (double)t[10] / (double)aligned : 0.0);
    fprintf(f, "SN\tindel rate\t%.6f\n", aligned ? (double)(t[11] + t[13]) / (double)aligned : 0.0);
    for (k = 0; k < 3; k++)
        for (i = 0; i < one[k].bins; i++)
            if (t[one[k].first + i]) fprintf(f, "%s\t%d%s\t%llu\n", one[k].tag, i, one[k].folds && i == one[k].bins - 1 ? "+" : "", (unsigned long long)t[one[k].first + i]);
    for (i = 0; i < 512; i++)
        if (t[728 + i] | t[1240 + i] | t[1752 + i] | t[2264 + i])
            fprintf(f, "CY\t%d%s\t%llu\t%llu\t%llu\t%llu\n", i, i == 511 ? "+" : "", (unsigned long long)t[728 + i], (unsigned long long)t[1240 + i],
                    (unsigned long long)t[1752 + i], (unsigned long long)t[2264 + i]);
    for (i = 0; i < 16; i++)
        if (t[2776 + i]) fprintf(f, "SU\t%c\t%c\t%llu\n", "ACGT"[i >> 2], "ACGT"[i & 3], (unsigned long long)t[2776 + i]);
    for (i = 0; i < 96; i++)
        if (t[2792 + i] | t[2888 + i])
            fprintf(f, "BQ\t%d\t%llu\t%llu\t%.2f\n", i, (unsigned long long)t[2792 + i], (unsigned long long)t[2888 + i],
                    -10.0 * log10(((double)t[2888 + i] + 1.0) / ((double)t[2792 + i] + 2.0)));
    for (k = 0; k < 2; k++)
        for (i = 0; i < 64; i++)
            if (t[lens[k].first + i]) fprintf(f, "%s\t%d%s\t%llu\n", lens[k].tag, i, i == 63 ? "+" : "", (unsigned long long)t[lens[k].first + i]);
    return ferror(f) ? -1 : 0;
}

void slh_buffer_free(slh_buffer *b) {
    free(b->data);
    b->data = NULL;
    b->len = b->cap = 0;
}

static int buf_reserve(slh_buffer *b, size_t extra) {
    if (b->len + extra <= b->cap) return 0;
    size_t nc = b->cap ? b->cap * 2 : (1u << 16);
    while (nc < b->len + extra) nc *= 2;
    if (b->data == NULL) { /* first reservation: callers that know their size ask for all of it (huge pages if large) */
        char *fd = (char *)slh_big_malloc(nc);
        if (!fd) return -1;
        b->data = fd;
        b->cap = nc;
        return 0;
    }
    char *nd = (char *)realloc(b->data, nc);
    if (!nd) return -1;
    b->data = nd;
    b->cap = nc;
    return 0;
}

int slh_buffer_reserve(slh_buffer *b, size_t bytes) { return buf_reserve(b, bytes); }

/* decimal digits, two at a time (24 M lines of three numbers each per 10 M reads: the formatter is the front end's
 * longest stage once the search is on the GPU) */
static const char DIGIT_PAIRS[201] =
    "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";

static inline char *put_u32(char *p, uint32_t v) {
    char tmp[10];
    int n = 10;
    while (v >= 100) {
        uint32_t q = v / 100, r = v - q * 100;
        n -= 2;
        memcpy(tmp + n, DIGIT_PAIRS + 2 * r, 2);
        v = q;
    }
    if (v >= 10) { n -= 2; memcpy(tmp + n, DIGIT_PAIRS + 2 * v, 2); }
    else tmp[--n] = (char)('0' + v);
    memcpy(p, tmp + n, (size_t)(10 - n));
    return p + (10 - n);
}

int slh_format_pile_rows(slh_buffer *buf, const char *record_name, uint32_t first_pos, const char *letters, const uint32_t *counts,
                         uint64_t rows) {
    size_t nl = 0;
    uint64_t i;
    int k;
    while (record_name[nl] != '\0' && record_name[nl] != ' ' && record_name[nl] != '\t') nl++;
    for (i = 0; i < rows; i++) {
        const uint32_t *c = counts + 6 * i;
        char *p, l = letters[i];
        if (!(c[0] | c[1] | c[2] | c[3] | c[4] | c[5])) continue;
        if (buf_reserve(buf, nl + 96)) return -1;
        p = buf->data + buf->len;
        memcpy(p, record_name, nl);
        p += nl;
        *p++ = '\t';
        p = put_u32(p, first_pos + (uint32_t)i);
        *p++ = '\t';
        *p++ = (l >= 'a' && l <= 'z') ? (char)(l - 32) : l;
        for (k = 0; k < 6; k++) { *p++ = '\t'; p = put_u32(p, c[k]); }
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
    }
    return 0;
}

int slh_format_site_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, const char *text, const uint64_t *pos,
                         const uint32_t *counts, const uint8_t *alleles, uint64_t rows) {
    size_t nl = 0;
    uint64_t i;
    int k;
    while (record_name[nl] != '\0' && record_name[nl] != ' ' && record_name[nl] != '\t') nl++;
    for (i = 0; i < rows; i++) {
        const uint32_t *c = counts + 6 * i;
        char *p, l = text[pos[i]];
        int some = 0;
        if (buf_reserve(buf, nl + 112)) return -1;
        p = buf->data + buf->len;
        memcpy(p, record_name, nl);
        p += nl;
        *p++ = '\t';
        p = put_u32(p, (uint32_t)(pos[i] - record_start) + 1u);
        *p++ = '\t';
        *p++ = (l >= 'a' && l <= 'z') ? (char)(l - 32) : l;
        for (k = 0; k < 6; k++) { *p++ = '\t'; p = put_u32(p, c[k]); }
        *p++ = '\t';
        for (k = 0; k < 6; k++)
            if ((alleles[i] >> k) & 1) {
                if (some) *p++ = ',';
                *p++ = "ACGTDI"[k];
                some = 1;
            }
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
    }
    return 0;
}

static size_t cut_name_len(const char *name) {
    size_t nl = 0;
    while (name[nl] != '\0' && name[nl] != ' ' && name[nl] != '\t') nl++;
    return nl;
}

static inline char upper_letter(char l) { return (l >= 'a' && l <= 'z') ? (char)(l - 32) : l; }

int slh_format_vcf_header(slh_buffer *buf, const slh_record *refs, int num_refs) {
    static const char *const INFO =
        "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth A+C+G+T+D at the row (SNV) or at the anchor row (indel)\">\n"
        "##INFO=<ID=AO,Number=1,Type=Integer,Description=\"Observations of the alternate allele\">\n"
        "##INFO=<ID=SF,Number=1,Type=Integer,Description=\"Observations of the alternate allele on forward-strand reads\">\n"
        "##INFO=<ID=SR,Number=1,Type=Integer,Description=\"Observations of the alternate allele on reverse-strand reads\">\n"
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    static const char *const FIRST = "##fileformat=VCFv4.2\n";
    int r;
    char *p;
    if (buf_reserve(buf, strlen(FIRST))) return -1;
    memcpy(buf->data + buf->len, FIRST, strlen(FIRST));
    buf->len += strlen(FIRST);
    for (r = 0; r < num_refs; r++) {
        size_t nl = cut_name_len(refs[r].name);
        if (buf_reserve(buf, nl + 48)) return -1;
        p = buf->data + buf->len;
        memcpy(p, "##contig=<ID=", 13);
        p += 13;
        memcpy(p, refs[r].name, nl);
        p += nl;
        memcpy(p, ",length=", 8);
        p += 8;
        p = put_u32(p, refs[r].size);
        *p++ = '>';
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
    }
    if (buf_reserve(buf, strlen(INFO))) return -1;
    memcpy(buf->data + buf->len, INFO, strlen(INFO));
    buf->len += strlen(INFO);
    return 0;
}

int slh_format_fasta_record(slh_buffer *buf, const char *record_name, const char *letters, uint64_t len) {
    const size_t nl = cut_name_len(record_name);
    uint64_t i;
    char *p;
    if (buf_reserve(buf, nl + 2 + (size_t)len + (size_t)(len / 60) + 2)) return -1;
    p = buf->data + buf->len;
    *p++ = '>';
    memcpy(p, record_name, nl);
    p += nl;
    *p++ = '\n';
    for (i = 0; i < len; i += 60) {
        const size_t k = (size_t)(len - i < 60 ? len - i : 60);
        memcpy(p, letters + i, k);
        p += k;
        *p++ = '\n';
    }
    buf->len = (size_t)(p - buf->data);
    return 0;
}

static inline char *put_u64(char *p, uint64_t v) {
    char tmp[20];
    int n = 20;
    do { tmp[--n] = (char)('0' + v % 10); v /= 10; } while (v);
    memcpy(p, tmp + n, (size_t)(20 - n));
    return p + (20 - n);
}

/* 100 * num // den (0 when den is 0; the product in 128 bits) as whole "." two digits */
static inline char *put_hundredths(char *p, uint64_t num, uint64_t den) {
    const uint64_t q = den ? (uint64_t)((unsigned __int128)100 * num / den) : 0;
    p = put_u64(p, q / 100);
    *p++ = '.';
    memcpy(p, DIGIT_PAIRS + 2 * (q % 100), 2);
    return p + 2;
}

/* name TAB start TAB end TAB */
static char *depth_line_head(char *p, const char *record_name, size_t nl, uint64_t start, uint64_t end) {
    memcpy(p, record_name, nl);
    p += nl;
    *p++ = '\t';
    p = put_u64(p, start);
    *p++ = '\t';
    p = put_u64(p, end);
    *p++ = '\t';
    return p;
}

int slh_format_depth_flush(slh_buffer *buf, const char *record_name, slh_depth_pending *pend) {
    const size_t nl = cut_name_len(record_name);
    char *p;
    if (!pend->open) return 0;
    if (buf_reserve(buf, nl + 72)) return -1;
    p = depth_line_head(buf->data + buf->len, record_name, nl, pend->start, pend->end);
    p = put_u64(p, pend->value);
    *p++ = '\n';
    buf->len = (size_t)(p - buf->data);
    pend->open = 0;
    return 0;
}

int slh_format_depth_runs(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t a, uint64_t b,
                          const slh_depth_run *runs, uint64_t num_runs, slh_depth_pending *pend) {
    uint64_t lo = 0, hi = num_runs, i;
    if (a >= b) return 0;
    while (hi - lo > 1) { /* the run that holds row a: the last one with pos <= a */
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (runs[mid].pos <= a) lo = mid; else hi = mid;
    }
    for (i = lo; i < num_runs && runs[i].pos < b; i++) {
        const uint64_t s = (runs[i].pos > a ? runs[i].pos : a) - record_start;
        const uint64_t e = (i + 1 < num_runs && runs[i + 1].pos < b ? runs[i + 1].pos : b) - record_start;
        if (pend->open && pend->value == runs[i].value && pend->end == s) { /* (the run went on over the border of two ranges) */
            pend->end = e;
            continue;
        }
        if (slh_format_depth_flush(buf, record_name, pend)) return -1;
        pend->start = s;
        pend->end = e;
        pend->value = runs[i].value;
        pend->open = 1;
    }
    return 0;
}

int slh_format_depth_windows(slh_buffer *buf, const char *record_name, uint64_t record_size, uint64_t window, uint64_t j0,
                             uint64_t sum_at_j0, const uint64_t *cum, uint64_t k) {
    const size_t nl = cut_name_len(record_name);
    uint64_t i, prev = sum_at_j0;
    for (i = 0; i < k; i++) {
        const uint64_t s = (j0 + i) * window, e = record_size - s < window ? record_size : s + window;
        char *p;
        if (buf_reserve(buf, nl + 96)) return -1;
        p = depth_line_head(buf->data + buf->len, record_name, nl, s, e);
        p = put_hundredths(p, cum[2 * i] - prev, e - s);
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
        prev = cum[2 * i];
    }
    return 0;
}

int slh_format_depth_summary(slh_buffer *buf, const char *record_name, uint64_t length, uint64_t covered, uint64_t sum) {
    static const char *const HEAD = "> Depth of ";
    const size_t nl = cut_name_len(record_name);
    char *p;
    if (buf_reserve(buf, nl + 160)) return -1;
    p = buf->data + buf->len;
    memcpy(p, HEAD, strlen(HEAD));
    p += strlen(HEAD);
    memcpy(p, record_name, nl);
    p += nl;
    p += sprintf(p, ": %llu positions, %llu covered (", (unsigned long long)length, (unsigned long long)covered);
    p = put_hundredths(p, 100 * covered, length);
    p += sprintf(p, " %%), mean depth ");
    p = put_hundredths(p, sum, length);
    *p++ = '\n';
    buf->len = (size_t)(p - buf->data);
    return 0;
}

/* "\t.\t" REF "\t" ALT "\t.\t.\tDP=" d ";AO=" ao behind name and POS */
static char *vcf_line_head(char *p, const char *record_name, size_t nl, uint32_t pos1) {
    memcpy(p, record_name, nl);
    p += nl;
    *p++ = '\t';
    p = put_u32(p, pos1);
    memcpy(p, "\t.\t", 3);
    return p + 3;
}

static char *vcf_put_u64(char *p, uint64_t v) {
    if (v <= 0xFFFFFFFFull) return put_u32(p, (uint32_t)v);
    p = put_u32(p, (uint32_t)(v / 1000000000ull));
    {
        uint32_t low = (uint32_t)(v % 1000000000ull), div = 100000000u;
        for (; div > 0; div /= 10) *p++ = (char)('0' + (low / div) % 10);
    }
    return p;
}

int slh_format_vcf_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                        const uint64_t *site_pos, const uint32_t *site_counts, const uint8_t *site_alleles, uint64_t sites,
                        const slh_event *events, const uint32_t *anchor_rows, uint64_t num_events, uint32_t min_depth,
                        uint32_t min_pct) {
    const size_t nl = cut_name_len(record_name);
    const uint64_t record_end = record_start + record_size;
    uint64_t i = 0, e = 0;
    while (i < sites || e < num_events) {
        uint64_t spos = i < sites ? site_pos[i] - record_start + 1 : ~0ull, epos = ~0ull;
        char *p;
        int k;
        if (e < num_events) epos = events[e].pos > record_start ? events[e].pos - record_start : 1;
        if (spos <= epos) { /* the SNVs of a row: a line per set bit of A C G T, the rows' own order */
            const uint32_t *c = site_counts + 6 * i;
            const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4];
            for (k = 0; k < 4; k++) {
                if (!((site_alleles[i] >> k) & 1)) continue;
                if (buf_reserve(buf, nl + 96)) return -1;
                p = vcf_line_head(buf->data + buf->len, record_name, nl, (uint32_t)spos);
                *p++ = upper_letter(text[site_pos[i]]);
                *p++ = '\t';
                *p++ = "ACGT"[k];
                memcpy(p, "\t.\t.\tDP=", 8);
                p = vcf_put_u64(p + 8, d);
                memcpy(p, ";AO=", 4);
                p = put_u32(p + 4, c[k]);
                *p++ = '\n';
                buf->len = (size_t)(p - buf->data);
            }
            i++;
        } else {
            const slh_event *ev = &events[e];
            const uint32_t *c = anchor_rows + 6 * e;
            const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4], ao = (uint64_t)ev->fwd + ev->rev;
            const uint64_t pos = ev->pos, len = ev->len;
            const int first = pos == record_start;
            uint64_t j;
            e++;
            if (d < min_depth || 100ull * ao < (uint64_t)min_pct * d) continue;
            if (ev->kind == 0 && first && pos + len >= record_end) continue; /* (the record ends with the deletion: no following base) */
            if (buf_reserve(buf, nl + 320)) return -1;
            p = vcf_line_head(buf->data + buf->len, record_name, nl, (uint32_t)epos);
            if (ev->kind == 0) { /* REF: the anchor and the deleted rows, ALT: the anchor (behind the rows at a record's start) */
                const uint64_t from = first ? pos : pos - 1;
                for (j = 0; j <= len; j++) *p++ = upper_letter(text[from + j]);
                *p++ = '\t';
                *p++ = upper_letter(text[first ? pos + len : pos - 1]);
            } else { /* REF: the anchor, ALT: the anchor and the inserted letters (in front of it at a record's start) */
                const char anchor = upper_letter(text[first ? pos : pos - 1]);
                *p++ = anchor;
                *p++ = '\t';
                if (!first) *p++ = anchor;
                for (j = 0; j < len; j++) *p++ = "ACGT"[(ev->letters >> (2 * (len - 1 - j))) & 3];
                if (first) *p++ = anchor;
            }
            memcpy(p, "\t.\t.\tDP=", 8);
            p = vcf_put_u64(p + 8, d);
            memcpy(p, ";AO=", 4);
            p = vcf_put_u64(p + 4, ao);
            memcpy(p, ";SF=", 4);
            p = put_u32(p + 4, ev->fwd);
            memcpy(p, ";SR=", 4);
            p = put_u32(p + 4, ev->rev);
            *p++ = '\n';
            buf->len = (size_t)(p - buf->data);
        }
    }
    return 0;
}

/* ---- -vcf -sv ---- */

int slh_format_vcf_sv_header(slh_buffer *buf, const slh_record *refs, int num_refs) {
    static const char *const COLUMNS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    static const char *const SV =
        "##ALT=<ID=DEL,Description=\"Deletion of the rows between two segments of a read\">\n"
        "##ALT=<ID=INS,Description=\"Insertion of the letters between two segments of a read\">\n"
        "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of the junction: DEL or INS\">\n"
        "##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last deleted position; POS for an insertion\">\n"
        "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"Inserted letters, or the deleted positions as a negative number\">\n";
    const size_t cl = strlen(COLUMNS), sl = strlen(SV);
    if (slh_format_vcf_header(buf, refs, num_refs)) return -1;
    if (buf_reserve(buf, sl)) return -1;
    memcpy(buf->data + buf->len - cl, SV, sl); /* (in front of the column line, which the header ends with) */
    memcpy(buf->data + buf->len - cl + sl, COLUMNS, cl);
    buf->len += sl;
    return 0;
}

/* slh_format_vcf_rows with the junctions of the record (ascending in pos, kind, len; jrows: the pileup rows of their anchors
 * pos - 1) behind the SNVs and the events of a POS.  counts_out[0] += the lines written, [1] += the junctions at the record's
 * first row, which have no anchor and give no line. */
int slh_format_vcf_sv_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                           const uint64_t *site_pos, const uint32_t *site_counts, const uint8_t *site_alleles, uint64_t sites,
                           const slh_event *events, const uint32_t *anchor_rows, uint64_t num_events, const slh_junction *junctions,
                           const uint32_t *jrows, uint64_t num_junctions, uint32_t min_depth, uint32_t min_pct, uint64_t *counts_out) {
    const size_t nl = cut_name_len(record_name);
    uint64_t i = 0, e = 0, j = 0;
    int rc = 0;
    while (!rc && (i < sites || e < num_events || j < num_junctions)) { /* the order of slh_format_vcf_rows, a line group at a time */
        uint64_t spos = i < sites ? site_pos[i] - record_start + 1 : ~0ull, epos = ~0ull, jpos = ~0ull;
        if (e < num_events) epos = events[e].pos > record_start ? events[e].pos - record_start : 1;
        if (j < num_junctions) {
            if (junctions[j].pos <= record_start) { counts_out[1]++; j++; continue; }
            jpos = junctions[j].pos - record_start;
        }
        if (spos <= epos && spos <= jpos) {
            rc = slh_format_vcf_rows(buf, record_name, record_start, record_size, text, site_pos + i, site_counts + 6 * i, site_alleles + i, 1,
                                     NULL, NULL, 0, min_depth, min_pct);
            i++;
        } else if (epos <= jpos) {
            rc = slh_format_vcf_rows(buf, record_name, record_start, record_size, text, NULL, NULL, NULL, 0, events + e, anchor_rows + 6 * e, 1,
                                     min_depth, min_pct);
            e++;
        } else {
            const slh_junction *jn = &junctions[j];
            const uint32_t *c = jrows + 6 * j;
            const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4], ao = (uint64_t)jn->fwd + jn->rev;
            char *p;
            j++;
            if (d < min_depth || 100ull * ao < (uint64_t)min_pct * d) continue;
            if (buf_reserve(buf, nl + 192)) return -1;
            p = vcf_line_head(buf->data + buf->len, record_name, nl, (uint32_t)jpos);
            *p++ = upper_letter(text[jn->pos - 1]);
#define PUT(str) do { memcpy(p, str, sizeof(str) - 1); p += sizeof(str) - 1; } while (0)
            if (jn->kind == 0) {
                PUT("\t<DEL>\t.\t.\tSVTYPE=DEL;END=");
                p = vcf_put_u64(p, jpos + jn->len);
                PUT(";SVLEN=-");
            } else {
                PUT("\t<INS>\t.\t.\tSVTYPE=INS;END=");
                p = vcf_put_u64(p, jpos);
                PUT(";SVLEN=");
            }
            p = put_u32(p, jn->len);
            PUT(";DP=");
            p = vcf_put_u64(p, d);
            PUT(";AO=");
            p = vcf_put_u64(p, ao);
            PUT(";SF=");
            p = put_u32(p, jn->fwd);
            PUT(";SR=");
            p = put_u32(p, jn->rev);
#undef PUT
            *p++ = '\n';
            buf->len = (size_t)(p - buf->data);
            counts_out[0]++;
        }
    }
    return rc;
}

/* ---- -vcf -gt ---- */

int slh_format_vcf_gt_header(slh_buffer *buf, const slh_record *refs, int num_refs) {
    static const char *const TAIL =
        "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth A+C+G+T+D at the row (SNV) or at the anchor row (indel)\">\n"
        "##INFO=<ID=AO,Number=A,Type=Integer,Description=\"Observations of each alternate allele\">\n"
        "##INFO=<ID=SF,Number=1,Type=Integer,Description=\"Observations of the alternate allele on forward-strand reads\">\n"
        "##INFO=<ID=SR,Number=1,Type=Integer,Description=\"Observations of the alternate allele on reverse-strand reads\">\n"
        "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
        "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Depth A+C+G+T+D at the row (SNV) or at the anchor row (indel)\">\n"
        "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Observations of the reference and of each alternate allele\">\n"
        "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: the Phred-scaled distance to the second-best genotype, at most 99\">\n"
        "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods, the smallest 0\">\n"
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n";
    static const char *const FIRST = "##fileformat=VCFv4.2\n";
    int r;
    char *p;
    if (buf_reserve(buf, strlen(FIRST))) return -1;
    memcpy(buf->data + buf->len, FIRST, strlen(FIRST));
    buf->len += strlen(FIRST);
    for (r = 0; r < num_refs; r++) {
        size_t nl = cut_name_len(refs[r].name);
        if (buf_reserve(buf, nl + 48)) return -1;
        p = buf->data + buf->len;
        memcpy(p, "##contig=<ID=", 13);
        p += 13;
        memcpy(p, refs[r].name, nl);
        p += nl;
        memcpy(p, ",length=", 8);
        p += 8;
        p = put_u32(p, refs[r].size);
        *p++ = '>';
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
    }
    if (buf_reserve(buf, strlen(TAIL))) return -1;
    memcpy(buf->data + buf->len, TAIL, strlen(TAIL));
    buf->len += strlen(TAIL);
    return 0;
}

/* "\tGT:DP:AD:GQ:PL\t" and the sample's values: alleles[0 .. na) are what a and b may be (REF first; na <= 3), ad their counts */
static char *vcf_gt_sample(char *p, const slh_genotype *g, const uint8_t *alleles, int na, uint64_t dp, const uint64_t *ad) {
    int ia = 0, ib = 0, j, k, nv = 0;
    uint32_t vals[6], low;
    uint64_t gq = ((uint64_t)g->gq + 500) / 1000;
    for (j = 0; j < na; j++) {
        if (alleles[j] == g->a) ia = j;
        if (alleles[j] == g->b) ib = j;
    }
    if (ia > ib) { j = ia; ia = ib; ib = j; }
    memcpy(p, "\tGT:DP:AD:GQ:PL\t", 16);
    p = put_u32(p + 16, (uint32_t)ia);
    if (g->ploidy == 2) {
        *p++ = '/';
        p = put_u32(p, (uint32_t)ib);
        for (k = 0; k < na; k++)
            for (j = 0; j <= k; j++) { /* VCF order over the allele numbers; the record's pl is indexed by the pair behind them */
                const uint32_t lo = alleles[j] < alleles[k] ? alleles[j] : alleles[k], hi = alleles[j] < alleles[k] ? alleles[k] : alleles[j];
                vals[nv++] = g->pl[hi * (hi + 1) / 2 + lo];
            }
    } else {
        for (j = 0; j < na; j++) vals[nv++] = g->pl[alleles[j]];
    }
    *p++ = ':';
    p = vcf_put_u64(p, dp);
    for (j = 0; j < na; j++) {
        *p++ = j ? ',' : ':';
        p = vcf_put_u64(p, ad[j]);
    }
    *p++ = ':';
    p = put_u32(p, gq > 99 ? 99u : (uint32_t)gq);
    low = vals[0];
    for (j = 1; j < nv; j++)
        if (vals[j] < low) low = vals[j];
    for (j = 0; j < nv; j++) {
        *p++ = j ? ',' : ':';
        p = put_u32(p, (uint32_t)(((uint64_t)(vals[j] - low) + 500) / 1000));
    }
    return p;
}

int slh_format_vcf_gt_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                           const uint64_t *site_pos, const uint32_t *site_counts, const slh_genotype *site_gts, uint64_t sites,
                           const slh_event *events, const uint32_t *anchor_rows, const slh_genotype *event_gts, const uint8_t *called,
                           uint64_t num_events) {
    const size_t nl = cut_name_len(record_name);
    const uint64_t record_end = record_start + record_size;
    uint64_t i = 0, e = 0;
    while (i < sites || e < num_events) {
        uint64_t spos = i < sites ? site_pos[i] - record_start + 1 : ~0ull, epos = ~0ull;
        char *p;
        int k;
        if (e < num_events) epos = events[e].pos > record_start ? events[e].pos - record_start : 1;
        if (spos <= epos) { /* the row's one line: REF, the best genotype's other letters, and the sample */
            const uint32_t *c = site_counts + 6 * i;
            const slh_genotype *g = &site_gts[i];
            const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4];
            uint8_t alleles[3];
            uint64_t ad[3];
            int na = 1;
            alleles[0] = (uint8_t)(g->ref & 3);
            if (g->a != alleles[0]) alleles[na++] = (uint8_t)(g->a & 3);
            if (g->b != alleles[0] && g->b != g->a) alleles[na++] = (uint8_t)(g->b & 3);
            for (k = 0; k < na; k++) ad[k] = c[alleles[k]];
            if (buf_reserve(buf, nl + 320)) return -1;
            p = vcf_line_head(buf->data + buf->len, record_name, nl, (uint32_t)spos);
            *p++ = upper_letter(text[site_pos[i]]);
            for (k = 1; k < na; k++) {
                *p++ = k == 1 ? '\t' : ',';
                *p++ = "ACGT"[alleles[k]];
            }
            if (na == 1) { *p++ = '\t'; *p++ = '.'; } /* (never from the engine: a selected row's best genotype is not rr) */
            *p++ = '\t';
            p = vcf_put_u64(p, ((uint64_t)g->qual + 500) / 1000);
            memcpy(p, "\t.\tDP=", 6);
            p = vcf_put_u64(p + 6, d);
            memcpy(p, ";AO=", 4);
            p += 4;
            for (k = 1; k < na; k++) {
                if (k > 1) *p++ = ',';
                p = vcf_put_u64(p, ad[k]);
            }
            p = vcf_gt_sample(p, g, alleles, na, d, ad);
            *p++ = '\n';
            buf->len = (size_t)(p - buf->data);
            i++;
        } else {
            static const uint8_t ZERO_ONE[2] = {0, 1};
            const slh_event *ev = &events[e];
            const slh_genotype *g = &event_gts[e];
            const uint32_t *c = anchor_rows + 6 * e;
            const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4], ao = (uint64_t)ev->fwd + ev->rev;
            const uint64_t pos = ev->pos, len = ev->len;
            const int first = pos == record_start, is_called = called[e] != 0;
            uint64_t j, ad[2];
            e++;
            if (!is_called) continue;
            if (ev->kind == 0 && first && pos + len >= record_end) continue; /* (the record ends with the deletion: no following base) */
            if (buf_reserve(buf, nl + 480)) return -1;
            p = vcf_line_head(buf->data + buf->len, record_name, nl, (uint32_t)epos);
            if (ev->kind == 0) { /* REF: the anchor and the deleted rows, ALT: the anchor (behind the rows at a record's start) */
                const uint64_t from = first ? pos : pos - 1;
                for (j = 0; j <= len; j++) *p++ = upper_letter(text[from + j]);
                *p++ = '\t';
                *p++ = upper_letter(text[first ? pos + len : pos - 1]);
            } else { /* REF: the anchor, ALT: the anchor and the inserted letters (in front of it at a record's start) */
                const char anchor = upper_letter(text[first ? pos : pos - 1]);
                *p++ = anchor;
                *p++ = '\t';
                if (!first) *p++ = anchor;
                for (j = 0; j < len; j++) *p++ = "ACGT"[(ev->letters >> (2 * (len - 1 - j))) & 3];
                if (first) *p++ = anchor;
            }
            *p++ = '\t';
            p = vcf_put_u64(p, ((uint64_t)g->qual + 500) / 1000);
            memcpy(p, "\t.\tDP=", 6);
            p = vcf_put_u64(p + 6, d);
            memcpy(p, ";AO=", 4);
            p = vcf_put_u64(p + 4, ao);
            memcpy(p, ";SF=", 4);
            p = put_u32(p + 4, ev->fwd);
            memcpy(p, ";SR=", 4);
            p = put_u32(p + 4, ev->rev);
            ad[0] = d > ao ? d - ao : 0;
            ad[1] = ao;
            p = vcf_gt_sample(p, g, ZERO_ONE, 2, d, ad);
            *p++ = '\n';
            buf->len = (size_t)(p - buf->data);
        }
    }
    return 0;
}

/* ---- -vcf -gt -sb ---- */

/* the lines of `from` that begin with `prefix`, or the others */
static int sb_copy_lines(slh_buffer *buf, const slh_buffer *from, const char *prefix, int matching) {
    const size_t pl = strlen(prefix);
    size_t i = 0;
    while (i < from->len) {
        size_t e = i;
        while (e < from->len && from->data[e] != '\n') e++;
        if (e < from->len) e++;
        if ((e - i >= pl && memcmp(from->data + i, prefix, pl) == 0) == (matching != 0)) {
            if (buf_reserve(buf, e - i)) return -1;
            memcpy(buf->data + buf->len, from->data + i, e - i);
            buf->len += e - i;
        }
        i = e;
    }
    return 0;
}

static int sb_put(slh_buffer *buf, const char *s) {
    const size_t n = strlen(s);
    if (buf_reserve(buf, n)) return -1;
    memcpy(buf->data + buf->len, s, n);
    buf->len += n;
    return 0;
}

int slh_format_vcf_sb_header(slh_buffer *buf, const slh_record *refs, int num_refs, int fs_filter) {
    slh_buffer gt = {0, 0, 0};
    char line[160];
    int rc = slh_format_vcf_gt_header(&gt, refs, num_refs);
    /* the head of -vcf -gt, with FILTER in front of the INFO lines, FS behind them and SB behind the FORMAT lines */
    if (!rc) rc = sb_copy_lines(buf, &gt, "##fileformat", 1);
    if (!rc) rc = sb_copy_lines(buf, &gt, "##contig", 1);
    if (!rc && fs_filter >= 0) {
        snprintf(line, sizeof(line), "##FILTER=<ID=sb,Description=\"Strand bias: FS above %d\">\n", fs_filter);
        rc = sb_put(buf, line);
    }
    if (!rc) rc = sb_copy_lines(buf, &gt, "##INFO", 1);
    if (!rc) rc = sb_put(buf, "##INFO=<ID=FS,Number=1,Type=Float,Description=\"Phred-scaled p-value of Fisher's exact test of the strand table SB\">\n");
    if (!rc) rc = sb_copy_lines(buf, &gt, "##FORMAT", 1);
    if (!rc) rc = sb_put(buf, "##FORMAT=<ID=SB,Number=4,Type=Integer,Description=\"Observations of the reference on forward and reverse reads, "
                              "then of the alternate alleles on forward and reverse reads\">\n");
    if (!rc) rc = sb_copy_lines(buf, &gt, "#CHROM", 1);
    slh_buffer_free(&gt);
    return rc;
}

static uint32_t sb_cell(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }
static uint64_t sb_minus(uint64_t a, uint64_t b) { return a > b ? a - b : 0; }

/* The line that slh_format_vcf_gt_rows has just written at buf->data + start, with FILTER, ;FS= behind INFO, :SB behind FORMAT
 * and the table behind the sample; tmp: scratch that is kept between lines. */
static int sb_decorate(slh_buffer *buf, size_t start, const uint32_t t[4], int fs_filter, slh_buffer *tmp) {
    const size_t n = buf->len - start;
    uint32_t norm[4];
    const double fs = slamem_fisher_strand_of(t, norm);
    const char *verdict = fs > (double)fs_filter ? "sb" : "PASS";
    const char *s;
    char *p;
    size_t i;
    int col = 0, k;
    tmp->len = 0;
    if (buf_reserve(tmp, n)) return -1;
    memcpy(tmp->data, buf->data + start, n);
    if (buf_reserve(buf, 128)) return -1;
    s = tmp->data;
    p = buf->data + start;
    for (i = 0; i < n; i++) {
        const char c = s[i];
        if (c == '\t' || c == '\n') { /* a column ends: what comes behind it */
            if (col == 7) p += snprintf(p, 32, ";FS=%.3f", fs);
            if (col == 8) { memcpy(p, ":SB", 3); p += 3; }
            for (k = 0; col == 9 && k < 4; k++) {
                *p++ = k ? ',' : ':';
                p = put_u32(p, t[k]);
            }
            col++;
        } else if (col == 6 && fs_filter >= 0) { /* (the "." of -gt) */
            memcpy(p, verdict, strlen(verdict));
            p += strlen(verdict);
            continue;
        }
        *p++ = c;
    }
    buf->len = (size_t)(p - buf->data);
    return 0;
}

int slh_format_vcf_sb_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                           const uint64_t *site_pos, const uint32_t *site_counts, const uint32_t *site_fwd, const slh_genotype *site_gts,
                           uint64_t sites, const slh_event *events, const uint32_t *anchor_rows, const uint32_t *anchor_fwd,
                           const slh_genotype *event_gts, const uint8_t *called, uint64_t num_events, int fs_filter) {
    slh_buffer tmp = {0, 0, 0};
    uint64_t i = 0, e = 0;
    int rc = 0;
    while (!rc && (i < sites || e < num_events)) { /* the order of slh_format_vcf_gt_rows, a line at a time */
        const uint64_t spos = i < sites ? site_pos[i] - record_start + 1 : ~0ull;
        uint64_t epos = ~0ull;
        const size_t start = buf->len;
        uint32_t t[4];
        int k;
        if (e < num_events) epos = events[e].pos > record_start ? events[e].pos - record_start : 1;
        if (spos <= epos) {
            const uint32_t *c = site_counts + 6 * i, *f = site_fwd + 6 * i;
            const slh_genotype *g = &site_gts[i];
            const int r = g->ref & 3;
            uint64_t af = 0, ar = 0;
            for (k = 0; k < 4; k++) /* the line's ALT letters: the best genotype's that are not the reference's */
                if (k != r && (k == (g->a & 3) || k == (g->b & 3))) { af += f[k]; ar += sb_minus(c[k], f[k]); }
            t[0] = f[r]; t[1] = sb_cell(sb_minus(c[r], f[r])); t[2] = sb_cell(af); t[3] = sb_cell(ar);
            rc = slh_format_vcf_gt_rows(buf, record_name, record_start, record_size, text, site_pos + i, c, g, 1, NULL, NULL, NULL, NULL, 0);
            i++;
        } else {
            const uint32_t *c = anchor_rows + 6 * e, *f = anchor_fwd + 6 * e;
            const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4], df = (uint64_t)f[0] + f[1] + f[2] + f[3] + f[4];
            const uint64_t af = events[e].fwd, ar = events[e].rev;
            t[0] = sb_cell(sb_minus(df, af)); t[1] = sb_cell(sb_minus(sb_minus(d, df), ar)); t[2] = (uint32_t)af; t[3] = (uint32_t)ar;
            rc = slh_format_vcf_gt_rows(buf, record_name, record_start, record_size, text, NULL, NULL, NULL, 0, events + e, c, event_gts + e,
                                        called + e, 1);
            e++;
        }
        if (!rc && buf->len > start) rc = sb_decorate(buf, start, t, fs_filter, &tmp);
    }
    slh_buffer_free(&tmp);
    return rc;
}

/* ---- -wq: the lines of -vcf -gt, with or without -sb, and the quality sums per allele behind them ---- */

int slh_format_vcf_wq_header(slh_buffer *buf, const slh_record *refs, int num_refs, int sb, int fs_filter) {
    slh_buffer base = {0, 0, 0};
    int rc = sb ? slh_format_vcf_sb_header(&base, refs, num_refs, fs_filter) : slh_format_vcf_gt_header(&base, refs, num_refs);
    /* the head of the file without -wq, with ADQ behind its FORMAT lines */
    if (!rc) rc = sb_copy_lines(buf, &base, "#CHROM", 0);
    if (!rc) rc = sb_put(buf, "##FORMAT=<ID=ADQ,Number=R,Type=Integer,Description=\"Sum of the base qualities of the observations of the reference "
                              "and of each alternate allele\">\n");
    if (!rc) rc = sb_copy_lines(buf, &base, "#CHROM", 1);
    slh_buffer_free(&base);
    return rc;
}

/* The line that has just been written at buf->data + start, with :ADQ behind FORMAT and the sums (na of them; 0: a dot) behind
 * the sample */
static int wq_decorate(slh_buffer *buf, size_t start, const uint32_t *adq, int na) {
    char *p, *tab;
    size_t tail;
    int k;
    if (buf_reserve(buf, 64)) return -1;
    p = buf->data + buf->len - 1; /* the line's '\n' */
    for (tab = p; tab > buf->data + start && *tab != '\t'; tab--) {} /* the tab in front of the sample */
    tail = (size_t)(buf->data + buf->len - tab);
    memmove(tab + 4, tab, tail);
    memcpy(tab, ":ADQ", 4);
    p += 4;
    if (na == 0) { *p++ = ':'; *p++ = '.'; }
    for (k = 0; k < na; k++) {
        *p++ = k ? ',' : ':';
        p = put_u32(p, adq[k]);
    }
    *p++ = '\n';
    buf->len = (size_t)(p - buf->data);
    return 0;
}

int slh_format_vcf_wq_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                           const uint64_t *site_pos, const uint32_t *site_counts, const uint32_t *site_fwd, const uint32_t *site_qsums,
                           const slh_genotype *site_gts, uint64_t sites, const slh_event *events, const uint32_t *anchor_rows,
                           const uint32_t *anchor_fwd, const slh_genotype *event_gts, const uint8_t *called, uint64_t num_events, int sb,
                           int fs_filter) {
    uint64_t i = 0, e = 0;
    int rc = 0;
    while (!rc && (i < sites || e < num_events)) { /* the order of slh_format_vcf_gt_rows, a line at a time */
        const uint64_t spos = i < sites ? site_pos[i] - record_start + 1 : ~0ull;
        uint64_t epos = ~0ull;
        const size_t start = buf->len;
        uint32_t adq[4];
        int na = 0, k;
        if (e < num_events) epos = events[e].pos > record_start ? events[e].pos - record_start : 1;
        if (spos <= epos) {
            const slh_genotype *g = &site_gts[i];
            const uint32_t *q = site_qsums + 4 * i;
            const int r = g->ref & 3;
            adq[na++] = q[r]; /* AD's order: the reference, then the line's ALT letters ascending */
            for (k = 0; k < 4; k++)
                if (k != r && (k == (g->a & 3) || k == (g->b & 3))) adq[na++] = q[k];
            rc = sb ? slh_format_vcf_sb_rows(buf, record_name, record_start, record_size, text, site_pos + i, site_counts + 6 * i, site_fwd + 6 * i,
                                             g, 1, NULL, NULL, NULL, NULL, NULL, 0, fs_filter)
                    : slh_format_vcf_gt_rows(buf, record_name, record_start, record_size, text, site_pos + i, site_counts + 6 * i, g, 1, NULL, NULL,
                                             NULL, NULL, 0);
            i++;
        } else {
            rc = sb ? slh_format_vcf_sb_rows(buf, record_name, record_start, record_size, text, NULL, NULL, NULL, NULL, 0, events + e,
                                             anchor_rows + 6 * e, anchor_fwd + 6 * e, event_gts + e, called + e, 1, fs_filter)
                    : slh_format_vcf_gt_rows(buf, record_name, record_start, record_size, text, NULL, NULL, NULL, 0, events + e, anchor_rows + 6 * e,
                                             event_gts + e, called + e, 1);
            e++;
        }
        if (!rc && buf->len > start) rc = wq_decorate(buf, start, adq, na);
    }
    return rc;
}

int slh_format_block_aln(slh_buffer *buf, const char *query_name, int reverse, const uint32_t *segs, const uint32_t *ops,
                         const uint64_t *op_off, uint64_t count, const slh_record *refs, const uint32_t *merged_start,
                         int num_refs, uint64_t *sum_len_out) {
    static const char OPC[16] = {'?', 'I', 'D', '?', '?', '?', '?', '=', 'X', '?', '?', '?', '?', '?', '?', '?'};
    size_t nl = strlen(query_name);
    uint64_t i, k, sum = 0;
    char *p;
    if (buf_reserve(buf, nl + 16)) return -1;
    p = buf->data + buf->len;
    *p++ = '>';
    memcpy(p, query_name, nl);
    p += nl;
    if (reverse) { memcpy(p, " Reverse", 8); p += 8; }
    *p++ = '\n';
    buf->len = (size_t)(p - buf->data);
    for (i = 0; i < count; i++) {
        uint32_t rp = segs[5 * i];
        const uint64_t nops = op_off[i + 1] - op_off[i];
        size_t namelen = 0;
        const char *rname = NULL;
        if (num_refs > 1) {
            rname = refs[slh_seq_id_from_merged_pos(merged_start, num_refs, &rp)].name;
            namelen = strlen(rname);
        }
        /* five numbers of at most ten digits with their tabs, and eleven characters an operation */
        if (buf_reserve(buf, namelen + 72 + (size_t)nops * 11)) return -1;
        p = buf->data + buf->len;
        if (rname) {
            *p++ = ' ';
            memcpy(p, rname, namelen);
            p += namelen;
            *p++ = '\t';
        }
        p = put_u32(p, rp + 1);
        *p++ = '\t';
        p = put_u32(p, segs[5 * i + 1] + 1);
        for (k = 2; k < 5; k++) { *p++ = '\t'; p = put_u32(p, segs[5 * i + k]); }
        *p++ = '\t';
        for (k = op_off[i]; k < op_off[i + 1]; k++) { p = put_u32(p, ops[k] >> 4); *p++ = OPC[ops[k] & 15u]; }
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
        sum += segs[5 * i + 3];
    }
    if (sum_len_out) *sum_len_out = sum;
    return 0;
}

int slh_format_read_paf(slh_buffer *buf, const char *query_name, uint32_t query_len, int strand, uint32_t mapq, uint32_t s1,
                        uint32_t s2, const uint32_t *segs, const uint32_t *ops, const uint64_t *op_off, uint64_t count,
                        const slh_record *refs, const uint32_t *merged_start, int num_refs, uint64_t *sum_len_out) {
    static const char OPC[16] = {'?', 'I', 'D', '?', '?', '?', '?', '=', 'X', '?', '?', '?', '?', '?', '?', '?'};
    size_t nl = strcspn(query_name, " \t");
    uint64_t i, k, sum = 0;
    char *p;
    if (sum_len_out) *sum_len_out = 0;
    if (strand != 1 && strand != 2) return 0;
    for (i = 0; i < count; i++) {
        uint32_t rp = segs[5 * i], qs = segs[5 * i + 1], eq = 0, all = 0;
        const uint32_t rlen = segs[5 * i + 2], qlen = segs[5 * i + 3];
        const uint64_t nops = op_off[i + 1] - op_off[i];
        const slh_record *rec = &refs[num_refs > 1 ? slh_seq_id_from_merged_pos(merged_start, num_refs, &rp) : 0];
        const size_t namelen = strcspn(rec->name, " \t");
        if (strand == 2) qs = query_len - qs - qlen;
        for (k = op_off[i]; k < op_off[i + 1]; k++) {
            all += ops[k] >> 4;
            if ((ops[k] & 15u) == 7u) eq += ops[k] >> 4;
        }
        /* thirteen numbers of at most ten digits, tabs and tags, and eleven characters an operation */
        if (buf_reserve(buf, nl + namelen + 192 + (size_t)nops * 11)) return -1;
        p = buf->data + buf->len;
        memcpy(p, query_name, nl);
        p += nl;
        *p++ = '\t'; p = put_u32(p, query_len);
        *p++ = '\t'; p = put_u32(p, qs);
        *p++ = '\t'; p = put_u32(p, qs + qlen);
        *p++ = '\t'; *p++ = strand == 2 ? '-' : '+';
        *p++ = '\t';
        memcpy(p, rec->name, namelen);
        p += namelen;
        *p++ = '\t'; p = put_u32(p, rec->size);
        *p++ = '\t'; p = put_u32(p, rp);
        *p++ = '\t'; p = put_u32(p, rp + rlen);
        *p++ = '\t'; p = put_u32(p, eq);
        *p++ = '\t'; p = put_u32(p, all);
        *p++ = '\t'; p = put_u32(p, mapq);
        memcpy(p, "\tNM:i:", 6); p += 6; p = put_u32(p, segs[5 * i + 4]);
        memcpy(p, "\ts1:i:", 6); p += 6; p = put_u32(p, s1);
        memcpy(p, "\ts2:i:", 6); p += 6; p = put_u32(p, s2);
        memcpy(p, "\tcg:Z:", 6); p += 6;
        for (k = op_off[i]; k < op_off[i + 1]; k++) { p = put_u32(p, ops[k] >> 4); *p++ = OPC[ops[k] & 15u]; }
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
        sum += qlen;
    }
    if (sum_len_out) *sum_len_out = sum;
    return 0;
}

/* ---- SAM ---- */

static const char SAM_OPC[16] = {'?', 'I', 'D', '?', '?', '?', '?', '=', 'X', '?', '?', '?', '?', '?', '?', '?'};

/* a line's CIGAR: soft clips around the segment's operations (at most 24 + 11 characters an operation) */
static char *sam_put_cigar(char *p, uint32_t n, const uint32_t *seg, const uint32_t *ops, uint64_t o0, uint64_t o1) {
    const uint32_t lead = seg[1], tail = n - seg[1] - seg[3];
    uint64_t k;
    if (lead) { p = put_u32(p, lead); *p++ = 'S'; }
    for (k = o0; k < o1; k++) { p = put_u32(p, ops[k] >> 4); *p++ = SAM_OPC[ops[k] & 15u]; }
    if (tail) { p = put_u32(p, tail); *p++ = 'S'; }
    return p;
}

/* the MD text of one segment's entries (at most 12 characters an entry) */
static char *sam_put_md(char *p, const uint32_t *md, uint64_t m0, uint64_t m1) {
    int prev_d = 0;
    uint64_t k;
    for (k = m0; k < m1; k++) {
        const uint32_t e = md[k], m = e >> 4;
        if (e & 8u) { p = put_u32(p, m); break; }
        if (e & 4u) {
            if (!(prev_d && m == 0)) { p = put_u32(p, m); *p++ = '^'; }
            prev_d = 1;
        } else {
            p = put_u32(p, m);
            prev_d = 0;
        }
        *p++ = "ACGT"[e & 3u];
    }
    return p;
}

/* the engine's complement rule: A<->T, C<->G in either case, anything else N */
static inline char sam_complement(char c) {
    switch (c & 0xDF) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    default: return 'N';
    }
}

int slh_format_sam_header(slh_buffer *buf, const slh_record *refs, int num_refs) {
    static const char HD[] = "@HD\tVN:1.6\tSO:unsorted\n", PG[] = "@PG\tID:slaMEM-hip\tPN:slaMEM-hip\n";
    int i;
    char *p;
    if (buf_reserve(buf, sizeof(HD))) return -1;
    memcpy(buf->data + buf->len, HD, sizeof(HD) - 1);
    buf->len += sizeof(HD) - 1;
    for (i = 0; i < num_refs; i++) {
        const size_t namelen = strcspn(refs[i].name, " \t");
        if (buf_reserve(buf, namelen + 32)) return -1;
        p = buf->data + buf->len;
        memcpy(p, "@SQ\tSN:", 7); p += 7;
        memcpy(p, refs[i].name, namelen); p += namelen;
        memcpy(p, "\tLN:", 4); p += 4;
        p = put_u32(p, refs[i].size);
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
    }
    if (buf_reserve(buf, sizeof(PG))) return -1;
    memcpy(buf->data + buf->len, PG, sizeof(PG) - 1);
    buf->len += sizeof(PG) - 1;
    return 0;
}

int slh_format_read_sam(slh_buffer *buf, const char *query_name, const char *letters, const char *quals, uint32_t n, int strand,
                        uint32_t mapq, uint32_t s1, uint32_t s2, const uint32_t *segs, const uint32_t *ops, const uint64_t *op_off,
                        const uint32_t *md, const uint64_t *md_off, uint32_t primary, uint64_t count, const slh_record *refs,
                        const uint32_t *merged_start, int num_refs, uint64_t *sum_len_out) {
    const size_t nl = strcspn(query_name, " \t");
    uint64_t i, j, sum = 0;
    size_t sa_room = 0;
    uint32_t x;
    char *p;
    if (sum_len_out) *sum_len_out = 0;
    if ((strand != 1 && strand != 2) || count == 0) {
        if (buf_reserve(buf, nl + 2 * (size_t)n + 32)) return -1;
        p = buf->data + buf->len;
        memcpy(p, query_name, nl); p += nl;
        memcpy(p, "\t4\t*\t0\t0\t*\t*\t0\t0\t", 17); p += 17;
        memcpy(p, letters, n); p += n;
        *p++ = '\t';
        if (quals) { memcpy(p, quals, n); p += n; } else *p++ = '*';
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
        return 0;
    }
    if (count > 1) /* what the other segments' SA entries take at most: name, position, strand, CIGAR, two numbers */
        for (i = 0; i < count; i++) {
            uint32_t rp = segs[5 * i];
            const slh_record *rec = &refs[num_refs > 1 ? slh_seq_id_from_merged_pos(merged_start, num_refs, &rp) : 0];
            sa_room += strcspn(rec->name, " \t") + 64 + (size_t)(op_off[i + 1] - op_off[i]) * 11;
        }
    for (i = 0; i < count; i++) {
        uint32_t rp = segs[5 * i];
        const slh_record *rec = &refs[num_refs > 1 ? slh_seq_id_from_merged_pos(merged_start, num_refs, &rp) : 0];
        const size_t namelen = strcspn(rec->name, " \t");
        const uint64_t nops = op_off[i + 1] - op_off[i], nmd = md_off[i + 1] - md_off[i];
        if (buf_reserve(buf, nl + namelen + 192 + (size_t)nops * 11 + 2 * (size_t)n + (size_t)nmd * 12 + sa_room)) return -1;
        p = buf->data + buf->len;
        memcpy(p, query_name, nl); p += nl;
        *p++ = '\t'; p = put_u32(p, (strand == 2 ? 16u : 0u) | (i == primary ? 0u : 2048u));
        *p++ = '\t'; memcpy(p, rec->name, namelen); p += namelen;
        *p++ = '\t'; p = put_u32(p, rp + 1);
        *p++ = '\t'; p = put_u32(p, mapq);
        *p++ = '\t'; p = sam_put_cigar(p, n, segs + 5 * i, ops, op_off[i], op_off[i + 1]);
        memcpy(p, "\t*\t0\t0\t", 7); p += 7;
        if (strand == 2) for (x = 0; x < n; x++) *p++ = sam_complement(letters[n - 1 - x]);
        else { memcpy(p, letters, n); p += n; }
        *p++ = '\t';
        if (!quals) *p++ = '*';
        else if (strand == 2) for (x = 0; x < n; x++) *p++ = quals[n - 1 - x];
        else { memcpy(p, quals, n); p += n; }
        memcpy(p, "\tNM:i:", 6); p += 6; p = put_u32(p, segs[5 * i + 4]);
        memcpy(p, "\tMD:Z:", 6); p += 6; p = sam_put_md(p, md, md_off[i], md_off[i + 1]);
        memcpy(p, "\ts1:i:", 6); p += 6; p = put_u32(p, s1);
        memcpy(p, "\ts2:i:", 6); p += 6; p = put_u32(p, s2);
        if (count > 1) {
            memcpy(p, "\tSA:Z:", 6); p += 6;
            for (j = 0; j < count; j++) {
                uint32_t op = segs[5 * j];
                const slh_record *orec;
                size_t on;
                if (j == i) continue;
                orec = &refs[num_refs > 1 ? slh_seq_id_from_merged_pos(merged_start, num_refs, &op) : 0];
                on = strcspn(orec->name, " \t");
                memcpy(p, orec->name, on); p += on;
                *p++ = ','; p = put_u32(p, op + 1);
                *p++ = ','; *p++ = strand == 2 ? '-' : '+';
                *p++ = ','; p = sam_put_cigar(p, n, segs + 5 * j, ops, op_off[j], op_off[j + 1]);
                *p++ = ','; p = put_u32(p, mapq);
                *p++ = ','; p = put_u32(p, segs[5 * j + 4]);
                *p++ = ';';
            }
        }
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
        sum += segs[5 * i + 3];
    }
    if (sum_len_out) *sum_len_out = sum;
    return 0;
}

int slh_format_block(slh_buffer *buf, const char *query_name, int reverse, const uint32_t *mems, uint64_t count,
                     const slh_record *refs, const uint32_t *merged_start, int num_refs, uint64_t *sum_len_out) {
    return slh_format_block_ext(buf, query_name, reverse, mems, NULL, count, refs, merged_start, num_refs, sum_len_out);
}

int slh_format_block_ext(slh_buffer *buf, const char *query_name, int reverse, const uint32_t *mems, const uint32_t *extra,
                         uint64_t count, const slh_record *refs, const uint32_t *merged_start, int num_refs,
                         uint64_t *sum_len_out) {
    size_t nl = strlen(query_name);
    uint64_t i, sum = 0;
    char *p;
    /* room for the whole block at once when its lines have a known bound (one reference record: three numbers of at
       most ten digits, two tabs, a newline) */
    if (buf_reserve(buf, nl + 16 + (num_refs == 1 ? (size_t)count * (extra ? 44 : 33) : 0))) return -1;
    p = buf->data + buf->len;
    *p++ = '>';
    memcpy(p, query_name, nl);
    p += nl;
    if (reverse) { memcpy(p, " Reverse", 8); p += 8; } /* slamem.c:102 */
    *p++ = '\n';
    if (num_refs == 1) { /* slamem.c:148 */
        for (i = 0; i < count; i++) {
            const uint32_t ln = mems[3 * i + 2];
            p = put_u32(p, mems[3 * i] + 1);
            *p++ = '\t';
            p = put_u32(p, mems[3 * i + 1] + 1);
            *p++ = '\t';
            p = put_u32(p, ln);
            if (extra) { *p++ = '\t'; p = put_u32(p, extra[i]); }
            *p++ = '\n';
            sum += ln;
        }
        buf->len = (size_t)(p - buf->data);
        if (sum_len_out) *sum_len_out = sum;
        return 0;
    }
    buf->len = (size_t)(p - buf->data);
    for (i = 0; i < count; i++) { /* slamem.c:144-148: several reference records, every line names its record */
        uint32_t rp = mems[3 * i], qp = mems[3 * i + 1], ln = mems[3 * i + 2];
        int id = slh_seq_id_from_merged_pos(merged_start, num_refs, &rp);
        const char *rname = refs[id].name;
        size_t namelen = strlen(rname);
        if (buf_reserve(buf, namelen + 60)) return -1;
        p = buf->data + buf->len;
        *p++ = ' ';
        memcpy(p, rname, namelen);
        p += namelen;
        *p++ = '\t';
        p = put_u32(p, rp + 1);
        *p++ = '\t';
        p = put_u32(p, qp + 1);
        *p++ = '\t';
        p = put_u32(p, ln);
        if (extra) { *p++ = '\t'; p = put_u32(p, extra[i]); }
        *p++ = '\n';
        buf->len = (size_t)(p - buf->data);
        sum += ln;
    }
    if (sum_len_out) *sum_len_out = sum;
    return 0;
}

int slh_progress_dots(uint32_t textsize) {
    uint32_t step = textsize / 10; /* slamem.c:94 */
    return (int)(textsize / (step + 1)); /* one dot each time the counter reaches the step (slamem.c:116-120) */
}

/* ------------------------------------------------------------------------------------------------
 * The two hidden utilities of the reference's command line (slamem.c:555-570).  Plain host text
 * processing; kept so that every invocation of the reference has a counterpart here.
 * ---------------------------------------------------------------------------------------------- */

typedef struct {
    char ref_name[65]; /* first word of the reference name, at most 64 characters (slamem.c:221,330) */
    int ref_pos, query_pos, size;
    size_t order;      /* input order: ties keep it (glibc's qsort is a merge sort) */
} sorted_mem;

static int sorted_mem_cmp(const void *pa, const void *pb) { /* MEMInfoSortFunction, slamem.c:227-239 */
    const sorted_mem *a = (const sorted_mem *)pa, *b = (const sorted_mem *)pb;
    const char *ca = a->ref_name, *cb = b->ref_name;
    int diff = 0;
    while ((diff = (int)(*ca) - (int)(*cb)) == 0 && *ca != '\0') { ca++; cb++; }
    if (diff == 0) {
        diff = a->ref_pos - b->ref_pos;
        if (diff == 0) diff = a->query_pos - b->query_pos;
    }
    if (diff == 0) diff = a->order < b->order ? -1 : (a->order > b->order ? 1 : 0);
    return diff;
}

/* a byte source with the reference's `char c = fgetc()` view: byte 0xFF reads as end of input */
typedef struct { const unsigned char *p, *end; } byte_src;
static int src_get(byte_src *s) {
    if (s->p >= s->end) return -1;
    if (*s->p == 0xFF) { s->p = s->end; return -1; }
    return *s->p++;
}
static int is_space_c(int c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }
static void skip_space(byte_src *s) { while (s->p < s->end && is_space_c(*s->p)) s->p++; }
/* scanf("%d"): optional sign, digits; returns 0 when no number starts here */
static int scan_int(byte_src *s, int *out) {
    const unsigned char *q;
    long long v = 0;
    int neg = 0, digits = 0;
    skip_space(s);
    q = s->p;
    if (q < s->end && (*q == '+' || *q == '-')) { neg = *q == '-'; q++; }
    while (q < s->end && *q >= '0' && *q <= '9') { if (v < (1LL << 40)) v = v * 10 + (*q - '0'); q++; digits++; }
    if (!digits) return 0;
    s->p = q;
    *out = (int)(neg ? -v : v);
    return 1;
}

static char *read_whole_file(const char *path, size_t *size_out) {
    FILE *f = fopen(path, "rb");
    char *buf;
    long sz;
    if (!f) return NULL;
    if (fseek(f, 0, SEEK_END) != 0 || (sz = ftell(f)) < 0) { fclose(f); return NULL; }
    rewind(f);
    buf = (char *)malloc((size_t)sz + 1);
    if (!buf) { fclose(f); return NULL; }
    if (sz && fread(buf, 1, (size_t)sz, f) != (size_t)sz) { free(buf); fclose(f); return NULL; }
    fclose(f);
    *size_out = (size_t)sz;
    return buf;
}

/* SortMEMsFile (slamem.c:244-352): every block of the MEMs file sorted by (reference name, reference position, query
 * position) and written in DESCENDING order (the reference walks its sorted array from the end, :310-317) to
 * <basename>-sorted.txt.  Returns the process status: 0, or 255 after an error message. */
int slh_sort_mems_file(const char *path, FILE *log) {
    size_t size = 0, cap = 0, num = 0, seqs = 0, k;
    char *data, *out_name, seqname[256];
    sorted_mem *arr = NULL;
    byte_src s;
    FILE *out;
    int c, fields = 0;
    fprintf(log, "> Sorting MEMs from <%s> ", path);
    fflush(log);
    data = read_whole_file(path, &size);
    if (!data) { fprintf(log, "\n> ERROR: Cannot read input file\n"); return 255; }
    s.p = (const unsigned char *)data;
    s.end = s.p + size;
    c = src_get(&s);
    if (c != '>') { fprintf(log, "\n> ERROR: Invalid MEMs file\n"); free(data); return 255; }
    while (c == '>') { /* :261-265: skip the header lines in front of the first MEM */
        c = src_get(&s);
        while (c != '\n' && c != -1) c = src_get(&s);
        c = src_get(&s);
    }
    if (c == -1) { fprintf(log, "\n> ERROR: No MEMs inside file\n"); free(data); return 255; }
    for (;;) { /* :271-278: number of fields of that line */
        while (c == ' ' || c == '\t') c = src_get(&s);
        if (c != '\n') {
            fields++;
            while (c != ' ' && c != '\t' && c != '\n' && c != -1) c = src_get(&s);
        }
        if (c == '\n' || c == -1) break;
    }
    if (fields != 3 && fields != 4) { fprintf(log, "\n> ERROR: Invalid MEMs file format\n"); free(data); return 255; }
    s.p = (const unsigned char *)data;
    s.end = s.p + size;
    if (fields == 4) fprintf(log, "(multiple references) ");
    fprintf(log, "...\n");
    out_name = slh_append_to_basename(path, "-sorted.txt");
    if (!out_name || (out = fopen(out_name, "w")) == NULL) {
        fprintf(log, "> ERROR: Cannot write output file\n");
        free(out_name); free(data);
        return 255;
    }
    seqname[0] = '\0';
    for (;;) {
        c = src_get(&s);
        if (c == '>' || c == -1) {
            if (seqs != 0) { /* :304-318 */
                fprintf(log, "(%d MEMs)\n", (int)num);
                fflush(log);
                if (num) qsort(arr, num, sizeof(sorted_mem), sorted_mem_cmp);
                fprintf(out, ">%s\n", seqname);
                for (k = num; k-- > 0;) {
                    if (fields == 4) fprintf(out, " %s\t", arr[k].ref_name);
                    fprintf(out, "%d\t%d\t%d\n", arr[k].ref_pos, arr[k].query_pos, arr[k].size);
                }
            }
            if (c == -1) break;
            num = 0;
            { /* fscanf(" %255[^\n]\n") :322 */
                size_t n = 0;
                skip_space(&s);
                while (s.p < s.end && *s.p != '\n' && n < 255) seqname[n++] = (char)*s.p++;
                seqname[n] = '\0';
                skip_space(&s);
            }
            fprintf(log, ":: '%s' ... ", seqname);
            fflush(log);
            seqs++;
            continue;
        }
        s.p--; /* ungetc */
        if (num == cap) {
            sorted_mem *na = (sorted_mem *)realloc(arr, (cap + 1024) * sizeof(sorted_mem));
            if (!na) { fprintf(log, "\n> ERROR: Not enough memory\n"); fclose(out); free(out_name); free(arr); free(data); return 255; }
            arr = na;
            cap += 1024;
        }
        if (fields == 4) { /* fscanf(" %64[^\t ]") :330 */
            size_t n = 0;
            skip_space(&s);
            while (s.p < s.end && *s.p != '\t' && *s.p != ' ' && n < 64) arr[num].ref_name[n++] = (char)*s.p++;
            arr[num].ref_name[n] = '\0';
        } else arr[num].ref_name[0] = '\0';
        if (!scan_int(&s, &arr[num].ref_pos) || !scan_int(&s, &arr[num].query_pos) || !scan_int(&s, &arr[num].size)) {
            fprintf(log, "\n> ERROR: Invalid format\n"); /* :333-337 (the reference also waits for a key here) */
            fclose(out); free(out_name); free(arr); free(data);
            return 255;
        }
        skip_space(&s);
        arr[num].order = num;
        num++;
    }
    fprintf(log, "> Saving sorted MEMs to <%s> ...\n", out_name);
    fflush(log);
    fclose(out);
    free(out_name);
    free(arr);
    free(data);
    fprintf(log, "> Done!\n");
    return 0;
}

/* CleanFasta (slamem.c:455-523): one record named after the file, holding the A/C/G/T letters (upper-cased) of all
 * records of the input, 100 per line, written to <basename>-clean.fasta. */
int slh_clean_fasta(const char *path, FILE *log) {
    size_t size = 0;
    char *data, *out_name;
    byte_src s;
    FILE *out;
    unsigned int chars = 0, invalid = 0, seqs = 0, line = 0;
    int c;
    fprintf(log, "> Opening FASTA file <%s> ... ", path);
    fflush(log);
    data = read_whole_file(path, &size);
    if (!data) { fprintf(log, "\n> ERROR: FASTA file not found\n"); return 255; }
    s.p = (const unsigned char *)data;
    s.end = s.p + size;
    c = src_get(&s);
    if (c != '>') { fprintf(log, "\n> ERROR: Invalid FASTA file\n"); free(data); return 255; }
    fprintf(log, "OK\n");
    out_name = slh_append_to_basename(path, "-clean.fasta");
    fprintf(log, "> Creating clean FASTA file <%s> ... ", out_name ? out_name : "");
    fflush(log);
    if (!out_name || (out = fopen(out_name, "w")) == NULL) {
        fprintf(log, "\n> ERROR: Can't write clean FASTA file\n");
        free(out_name); free(data);
        return 255;
    }
    fprintf(out, ">%s\n", path); /* the file name is the label (:479) */
    while (c != -1) {
        int up = (c == 'a' || c == 'c' || c == 'g' || c == 't') ? c - 32 : c;
        if (up == 'A' || up == 'C' || up == 'G' || up == 'T') {
            fputc(up, out);
            chars++;
            if (++line == 100) { fputc('\n', out); line = 0; }
        } else if (c == '>') {
            while (c != '\n' && c != -1) c = src_get(&s); /* skip the description */
            seqs++;
        } else if (c > 32 && c < 127) invalid++;
        c = src_get(&s);
    }
    if (line != 0) fputc('\n', out);
    fclose(out);
    free(out_name);
    free(data);
    fprintf(log, " OK\n");
    fprintf(log, ":: %u total chars", chars);
    if (invalid != 0) fprintf(log, " (%u non ACGT chars removed)", invalid);
    if (seqs > 1) fprintf(log, " ; %u sequences merged", seqs);
    fprintf(log, "\n");
    fprintf(log, "> Done!\n");
    return 0;
}
