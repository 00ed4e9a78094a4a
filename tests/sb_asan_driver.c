/* A stand-alone program for the sanitizer run of -sb (tests/test_sb_host.py builds it with slamem_host.c under
 * -fsanitize=address,undefined and runs it as a program):
 *   sb_asan_driver tables FILE   every line "rf rr af ar" of FILE goes through slamem_fisher_strand_table and slamem_fisher_strand;
 *                                prints the normalised table and FS with three decimals
 *   sb_asan_driver case FILE     FILE holds a reference and per record the arrays of slh_format_vcf_sb_rows, as the test packs them:
 *                                prints the file of slh_format_vcf_sb_header and slh_format_vcf_sb_rows
 * The sanitizers' reports, if any, go to stderr. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "slamem_hip.h"
#include "slamem_host.h"

static unsigned char *g_at, *g_end;

static void *take(size_t bytes) { /* the next `bytes` of the file, in a block of their own so that an overrun is seen */
    void *p = malloc(bytes ? bytes : 1);
    if (!p || (size_t)(g_end - g_at) < bytes) { fprintf(stderr, "short case file\n"); exit(2); }
    memcpy(p, g_at, bytes);
    g_at += bytes;
    return p;
}

static uint64_t take_u64(void) {
    uint64_t *p = (uint64_t *)take(8), v = *p;
    free(p);
    return v;
}

static int run_tables(const char *path) {
    FILE *f = fopen(path, "r");
    unsigned long long a, b, c, d;
    if (!f) return 2;
    while (fscanf(f, "%llu %llu %llu %llu", &a, &b, &c, &d) == 4) {
        const uint32_t t[4] = {(uint32_t)a, (uint32_t)b, (uint32_t)c, (uint32_t)d};
        uint32_t norm[4];
        slamem_fisher_strand_table(t, norm);
        printf("%u %u %u %u %.3f\n", norm[0], norm[1], norm[2], norm[3], slamem_fisher_strand(t));
    }
    fclose(f);
    return 0;
}

static int run_case(const char *path) {
    FILE *f = fopen(path, "rb");
    long size;
    unsigned char *data;
    slh_buffer buf = {0, 0, 0};
    slh_record *recs;
    char **names, *text;
    uint64_t num, r, n;
    int fs, rc;
    if (!f) return 2;
    fseek(f, 0L, SEEK_END);
    size = ftell(f);
    fseek(f, 0L, SEEK_SET);
    data = (unsigned char *)malloc((size_t)size + 1);
    if (!data || fread(data, 1, (size_t)size, f) != (size_t)size) return 2;
    fclose(f);
    g_at = data;
    g_end = data + size;
    fs = (int)(int64_t)take_u64();
    num = take_u64();
    recs = (slh_record *)calloc((size_t)num, sizeof(slh_record));
    names = (char **)calloc((size_t)num, sizeof(char *));
    if (!recs || !names) return 2;
    for (r = 0; r < num; r++) {
        const uint64_t nl = take_u64();
        char *raw = (char *)take((size_t)nl);
        names[r] = (char *)calloc((size_t)nl + 1, 1);
        if (!names[r]) return 2;
        memcpy(names[r], raw, (size_t)nl);
        free(raw);
        recs[r].name = names[r];
        recs[r].size = (uint32_t)take_u64();
    }
    n = take_u64();
    text = (char *)take((size_t)n);
    rc = slh_format_vcf_sb_header(&buf, recs, (int)num, fs);
    for (r = 0; r < num && rc == 0; r++) {
        const uint64_t start = take_u64(), rsize = take_u64(), m = take_u64();
        uint64_t *pos = (uint64_t *)take((size_t)m * 8);
        uint32_t *counts = (uint32_t *)take((size_t)m * 24), *fwd = (uint32_t *)take((size_t)m * 24);
        slh_genotype *gts = (slh_genotype *)take((size_t)m * sizeof(slh_genotype));
        const uint64_t ne = take_u64();
        slh_event *evs = (slh_event *)take((size_t)ne * sizeof(slh_event));
        uint32_t *rows = (uint32_t *)take((size_t)ne * 24), *frows = (uint32_t *)take((size_t)ne * 24);
        slh_genotype *eg = (slh_genotype *)take((size_t)ne * sizeof(slh_genotype));
        uint8_t *called = (uint8_t *)take((size_t)ne);
        rc = slh_format_vcf_sb_rows(&buf, names[r], start, rsize, text, pos, counts, fwd, gts, m, evs, rows, frows, eg, called, ne, fs);
        free(pos); free(counts); free(fwd); free(gts); free(evs); free(rows); free(frows); free(eg); free(called);
    }
    if (rc == 0 && buf.len) fwrite(buf.data, 1, buf.len, stdout);
    slh_buffer_free(&buf);
    for (r = 0; r < num; r++) free(names[r]);
    free(names); free(recs); free(text); free(data);
    return rc == 0 && g_at == g_end ? 0 : 3;
}

int main(int argc, char **argv) {
    if (argc == 3 && strcmp(argv[1], "tables") == 0) return run_tables(argv[2]);
    if (argc == 3 && strcmp(argv[1], "case") == 0) return run_case(argv[2]);
    fprintf(stderr, "usage: %s tables|case FILE\n", argv[0]);
    return 1;
}
