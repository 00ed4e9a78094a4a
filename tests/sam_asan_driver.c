/* A stand-alone program for the sanitizer run of the SAM writer (tests/test_sam_host.py builds it with slamem_host.c under
 * -fsanitize=address,undefined and runs it as a program): slh_format_sam_header and slh_format_read_sam on a reference of two
 * records -- a read of three segments with and without qualities, a read on the reverse strand with a deletion run followed by
 * a mismatch, an unmapped read, and a long read of many operations that makes the buffer grow.  The lines go to stdout (the test
 * compares them with tests/sam_spec.py); the sanitizers' reports, if any, go to stderr. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "slamem_host.h"

#define OP(k, c) (((uint32_t)(k) << 4) | (uint32_t)(c)) /* BAM's codes: = 7, X 8, I 1, D 2 */
#define MD(m, d, c) (((uint32_t)(m) << 4) | ((uint32_t)(d) << 2) | (uint32_t)(c))
#define MD_CLOSE(m) (((uint32_t)(m) << 4) | 8u)

int main(void) {
    slh_record recs[2] = {{(char *)"chrA first", 28}, {(char *)"chrB\tx", 14}};
    const uint32_t starts[2] = {0, 29};
    slh_buffer buf = {0, 0, 0};
    uint64_t sum = 0;
    int rc = 0, i;
    rc |= slh_format_sam_header(&buf, recs, 2);
    { /* three segments on the forward strand, the last one in the second record */
        const char *letters = "NATCCAATTNGCTTCCGANNACGTTGCANN";
        const char *quals = "()*+,-./0123456789:;<=>?@ABCDE";
        const uint32_t segs[15] = {0, 20, 8, 8, 0, 10, 10, 8, 8, 1, 31, 1, 8, 8, 0};
        const uint32_t ops[5] = {OP(8, 7), OP(4, 7), OP(1, 8), OP(3, 7), OP(8, 7)};
        const uint64_t ooff[4] = {0, 1, 4, 5};
        const uint32_t md[4] = {MD_CLOSE(8), MD(4, 0, 0), MD_CLOSE(3), MD_CLOSE(8)};
        const uint64_t moff[4] = {0, 1, 3, 4};
        rc |= slh_format_read_sam(&buf, "r1 a read", letters, quals, 30, 1, 37, 16, 6, segs, ops, ooff, md, moff, 0, 3, recs, starts, 2, &sum);
        rc |= slh_format_read_sam(&buf, "r1 a read", letters, NULL, 30, 1, 37, 16, 6, segs, ops, ooff, md, moff, 0, 3, recs, starts, 2, &sum);
    }
    { /* the reverse strand: 3= 1X 2= 2D 1X 2=, clipped on both sides */
        const char *letters = "acgtnACGTNACGT";
        const char *quals = "0123456789:;<=";
        const uint32_t segs[5] = {5, 2, 11, 9, 4};
        const uint32_t ops[6] = {OP(3, 7), OP(1, 8), OP(2, 7), OP(2, 2), OP(1, 8), OP(2, 7)};
        const uint64_t ooff[2] = {0, 6};
        const uint32_t md[5] = {MD(3, 0, 0), MD(2, 1, 1), MD(0, 1, 3), MD(0, 0, 3), MD_CLOSE(2)};
        const uint64_t moff[2] = {0, 5};
        rc |= slh_format_read_sam(&buf, "r2", letters, quals, 14, 2, 60, 9, 0, segs, ops, ooff, md, moff, 0, 1, recs, starts, 2, &sum);
    }
    /* unmapped, with and without qualities */
    rc |= slh_format_read_sam(&buf, "r3 x", "acgtn", NULL, 5, 0, 0, 0, 0, NULL, NULL, NULL, NULL, NULL, 0xFFFFFFFFu, 0, recs, starts, 2, &sum);
    rc |= slh_format_read_sam(&buf, "r3", "ACG", "!!#", 3, 0, 0, 0, 0, NULL, NULL, NULL, NULL, NULL, 0xFFFFFFFFu, 0, recs, starts, 2, &sum);
    { /* 40,000 letters in 20,000 operations 1= 1X ...: more than the buffer's first 64 KiB */
        const uint32_t n = 40000, nops = 20000;
        char *letters = (char *)malloc(n);
        uint32_t *ops = (uint32_t *)malloc(nops * sizeof(uint32_t)), *md = (uint32_t *)malloc((nops + 1) * sizeof(uint32_t));
        uint32_t segs[5] = {0, 0, 40000, 40000, 20000};
        uint64_t ooff[2] = {0, 20000}, moff[2] = {0, 20001};
        slh_record big = {(char *)"big", 40000};
        if (!letters || !ops || !md) return 2;
        memset(letters, 'A', n);
        for (i = 0; i < (int)nops; i++) ops[i] = OP(2, i % 2 ? 8 : 7);
        /* (an X of two letters is two entries: the second carries m = 0) */
        for (i = 0; i < (int)nops; i += 2) { md[i] = MD(2, 0, 1); md[i + 1] = MD(0, 0, 2); }
        md[nops] = MD_CLOSE(0);
        rc |= slh_format_read_sam(&buf, "r4", letters, NULL, n, 1, 60, 100, 0, segs, ops, ooff, md, moff, 0, 1, &big, NULL, 1, &sum);
        free(letters); free(ops); free(md);
    }
    if (rc) return 3;
    fwrite(buf.data, 1, buf.len, stdout);
    slh_buffer_free(&buf);
    return 0;
}
