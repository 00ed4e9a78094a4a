// gt_shared.h -- the genotype likelihood of -gt as gt_filter.hip (the VCF read-out) and cons_filter.hip (the
// consensus of -cons -gt) share it: the rule's parameters, the call of a set of scores, the scores of a row's
// A C G T columns (with the row's quality sums when kWeighted) and of an indel event, and the check of a slamem_gt_params.
// Everything is an unsigned 64-bit integer in milli-Phred.  The ten (four, three) scores are formed with compile-time indices
// only -- every loop over genotypes is unrolled and a genotype's number is compared, never used as an index -- so they live in
// registers; a caller keeps it that way.
#pragma once

#include "common.h"

namespace slamem {

struct GtRule {
    uint32_t ploidy;     // 1 or 2
    uint32_t M, H, E;    // the cost of a letter under a genotype homozygous for it, heterozygous with it, without it
    uint32_t hp;         // the prior cost per non-reference allele
    uint32_t min_depth;  // A+C+G+T+D at least this
    uint32_t min_qual;   // in milli-Phred: qual at least this
};

struct GtCall {
    uint32_t qual, gq, a, b;
    uint32_t pl[10];
};

__device__ __forceinline__ uint32_t gt_sat(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// the call of `ng` genotypes (ng <= 10) with likelihoods L and scores S (entries from ng on are not looked at), rr the
// homozygous-reference one: the smallest S, on a tie rr, then the smallest g.  Returns the best genotype's number.
__device__ __forceinline__ uint32_t gt_call(const uint64_t (&L)[10], const uint64_t (&S)[10], uint32_t ng, uint32_t rr, GtCall& out,
                                            uint64_t& qual) {
    uint64_t sb = S[0], srr = S[0], ml = L[0];
    uint32_t best = 0;
#pragma unroll
    for (uint32_t g = 1; g < 10u; g++) {
        if (g < ng && S[g] < sb) { sb = S[g]; best = g; }
        if (g < ng && L[g] < ml) ml = L[g];
        if (g == rr) srr = S[g];
    }
    if (srr == sb) best = rr;
    uint64_t second = ~0ull;
#pragma unroll
    for (uint32_t g = 0; g < 10u; g++) {
        if (g < ng && g != best && S[g] - sb < second) second = S[g] - sb;
        out.pl[g] = g < ng ? gt_sat(L[g] - ml) : 0u;
    }
    qual = srr - sb;
    out.qual = gt_sat(qual);
    out.gq = gt_sat(second);
    return best;
}

// the genotype of a row with the columns c[0..3] under the text's letter r (0..3).  Returns whether the best genotype is another
// than the homozygous-reference one; qual in 64 bits.  kWeighted: qs[0..3] are the row's quality sums, and the
// letters i that a genotype does not hold cost c[i] * E + 1000 * qs[i]; without it qs is not looked at.
template <bool kWeighted>
__device__ __forceinline__ bool gt_snv(const uint32_t (&c)[4], const uint32_t (&qs)[4], uint32_t r, const GtRule& p, GtCall& out,
                                       uint64_t& qual) {
    uint64_t L[10], S[10];
    if (p.ploidy == 2u) {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
#pragma unroll
            for (uint32_t j = 0; j <= k; j++) {
                const uint32_t g = k * (k + 1u) / 2u + j;
                uint64_t l = 0;
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    l += (uint64_t)c[i] * (j == k ? (i == j ? p.M : p.E) : (i == j || i == k ? p.H : p.E));
                    if constexpr (kWeighted) {
                        if (i != j && i != k) l += 1000ull * qs[i];
                    }
                }
                L[g] = l;
                S[g] = l + (uint64_t)p.hp * ((j != r ? 1u : 0u) + (k != j && k != r ? 1u : 0u));
            }
        }
        const uint32_t best = gt_call(L, S, 10u, r * (r + 1u) / 2u + r, out, qual);
        out.a = out.b = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
#pragma unroll
            for (uint32_t j = 0; j <= k; j++)
                if (best == k * (k + 1u) / 2u + j) { out.a = j; out.b = k; }
        }
        return !(out.a == r && out.b == r);
    }
    const uint64_t all = (uint64_t)c[0] + c[1] + c[2] + c[3];
    uint64_t qall = 0;
    if constexpr (kWeighted) qall = (uint64_t)qs[0] + qs[1] + qs[2] + qs[3];
#pragma unroll
    for (uint32_t g = 0; g < 10u; g++) {
        if (g < 4u) {
            L[g] = (uint64_t)c[g] * p.M + (all - c[g]) * p.E;
            if constexpr (kWeighted) L[g] += 1000ull * (qall - qs[g]);
            S[g] = L[g] + (g != r ? p.hp : 0u);
        } else {
            L[g] = S[g] = 0;
        }
    }
    const uint32_t best = gt_call(L, S, 4u, r, out, qual);
    out.a = out.b = best;
    return best != r;
}

// the genotype of an event seen ao times at an anchor row of depth d: 00, 01, 11 (ploidy 1: 0, 1).  Returns whether the best
// genotype is another than 00.
__device__ __forceinline__ bool gt_event(uint64_t ao, uint64_t d, const GtRule& p, GtCall& out, uint64_t& qual) {
    const uint64_t ro = d > ao ? d - ao : 0ull;
    const uint64_t l00 = ro * p.M + ao * p.E, l01 = (ro + ao) * p.H, l11 = ao * p.M + ro * p.E;
    uint64_t L[10], S[10];
#pragma unroll
    for (uint32_t g = 0; g < 10u; g++) L[g] = S[g] = 0;
    L[0] = S[0] = l00;
    if (p.ploidy == 2u) {
        L[1] = l01; S[1] = l01 + p.hp;
        L[2] = l11; S[2] = l11 + p.hp;
        const uint32_t best = gt_call(L, S, 3u, 0u, out, qual);
        out.a = best == 2u ? 1u : 0u;
        out.b = best != 0u ? 1u : 0u;
        return best != 0u;
    }
    L[1] = l11; S[1] = l11 + p.hp;
    const uint32_t best = gt_call(L, S, 2u, 0u, out, qual);
    out.a = out.b = best;
    return best != 0u;
}

// gt_filter.hip: the parameters as every variant refuses them; `fn` names the caller in the message
int gt_check(const char* fn, const slamem_gt_params* p, GtRule& rule);

}  // namespace slamem
