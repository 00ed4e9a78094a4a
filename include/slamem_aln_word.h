/* slamem_aln_word.h -- the max_edits word of slamem_hip.h taken apart and checked (SLAMEM_ALN_AFFINE): the one
 * place that knows its fields and their ranges, for the library (decode_aln_word in filters.hip adds the messages) and for the
 * front end's host logic, which refuses a bad -affine before any GPU work. */
#ifndef SLAMEM_ALN_WORD_H
#define SLAMEM_ALN_WORD_H
#include "slamem_hip.h"

/* The word's fields, the default resolved (unit cost: x = 1, o = 0, e = 1, *affine_out = 0).  Returns 0, or the rule the
 * word breaks: 1 E above SLAMEM_ALN_EDITS_MAX, 2 x outside 1..31, 3 o above 63, 4 e outside 1..31, 5 o + e * E above
 * SLAMEM_ALN_COST_MAX. */
static inline int slamem_decode_aln_word(uint32_t word, uint32_t *E_out, uint32_t *x_out, uint32_t *o_out, uint32_t *e_out,
                                         int *affine_out) {
    const int affine = word != SLAMEM_ALN_EDITS_DEFAULT && (word >> 8) != 0u;
    const uint32_t E = word == SLAMEM_ALN_EDITS_DEFAULT ? 31u : affine ? (word & 0xFFu) : word;
    const uint32_t x = affine ? (word >> 8) & 0xFFu : 1u, o = affine ? (word >> 16) & 0xFFu : 0u, e = affine ? word >> 24 : 1u;
    *E_out = E; *x_out = x; *o_out = o; *e_out = e; *affine_out = affine;
    if (E > SLAMEM_ALN_EDITS_MAX) return 1;
    if (x < 1u || x > 31u) return 2;
    if (o > 63u) return 3;
    if (e < 1u || e > 31u) return 4;
    if (o + e * E > SLAMEM_ALN_COST_MAX) return 5;
    return 0;
}

#endif
