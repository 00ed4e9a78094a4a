/* A stand-alone program for the sanitizer run of the FASTQ loader (tests/test_fastq_host.py builds it with slamem_host.c under
 * -fsanitize=address,undefined and runs it as a program): every file named on the command line goes through slh_load_file_q as a
 * query file and as a reference file and through slh_pieces_next_q, and the qualities it gives are packed into a low-quality
 * mask with slamem_pack_lowq.  It prints one line per step; the sanitizers' reports, if any, go to stderr. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "slamem_hip.h"
#include "slamem_host.h"

static uint64_t pack_and_count(const char *quals, uint64_t total) {
    const uint64_t words = (total + 63) / 64;
    uint64_t *mask = (uint64_t *)malloc((size_t)(words ? words : 1) * sizeof(uint64_t)), low = 0, w;
    if (!mask) return 0;
    if (slamem_pack_lowq(quals, total, 20, 33, mask, 2) != SLAMEM_OK) { free(mask); return (uint64_t)-1; }
    for (w = 0; w < words; w++) low += (uint64_t)__builtin_popcountll(mask[w]);
    free(mask);
    return low;
}

int main(int argc, char **argv) {
    int i;
    for (i = 1; i < argc; i++) {
        int acgt_only;
        for (acgt_only = 0; acgt_only < 2; acgt_only++) {
            slh_seqset s;
            char *quals = NULL;
            int n = slh_load_file_q(argv[i], 0, acgt_only, acgt_only ? 3 : 0, NULL, 1, 100, &s, &quals, NULL);
            printf("%s query n=%d acgt_only=%d", argv[i], n, acgt_only);
            if (n > 0) {
                printf(" letters=%llu quals=%d", (unsigned long long)s.total, quals != NULL);
                if (quals) printf(" low=%llu", (unsigned long long)pack_and_count(quals, s.total));
            }
            printf("\n");
            free(quals);
            slh_free_seqset(&s);
        }
        {
            slh_seqset s;
            char *quals = NULL;
            int n = slh_load_file_q(argv[i], 1, 0, 0, NULL, 1, 100, &s, &quals, NULL);
            printf("%s reference n=%d\n", argv[i], n);
            free(quals);
            slh_free_seqset(&s);
        }
        {
            slh_pieces *p = slh_pieces_open(argv[i], 0, 0, 1, 100, 1L << 20, NULL);
            int n = 0, pieces = 0;
            uint64_t low = 0;
            while (p) {
                slh_seqset s;
                char *quals = NULL;
                n = slh_pieces_next_q(p, &s, &quals);
                if (n <= 0) break;
                pieces++;
                if (quals) low += pack_and_count(quals, s.total);
                free(quals);
                slh_free_seqset(&s);
            }
            if (p) slh_pieces_close(p);
            printf("%s pieces=%d last=%d low=%llu\n", argv[i], pieces, n, (unsigned long long)low);
        }
    }
    return 0;
}
