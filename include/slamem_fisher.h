/* slamem_fisher.h -- FS of -sb: the Phred-scaled two-sided Fisher exact test of a strand table
 * t = (rf, rr, af, ar): reference forward, reference reverse, alternative forward, alternative reverse.
 *
 * One definition for libslamem_hip.so (slamem_fisher_strand) and the front end's formatter; engine.fisher_strand calls the
 * former and tests/sb_spec.py restates it with the same operations in the same order:
 *   1. s the sum of the cells; s > 400: every cell becomes cell * 200 / s in whole numbers (GATK's normalisation: it bounds the
 *      loop and keeps pow far from underflow)
 *   2. lf[0] = 0, lf[i] = lf[i - 1] + log10((double)i)
 *   3. r1 = rf + rr, r2 = af + ar, c1 = rf + af, N the sum;
 *      logp(x) = lf[r1] + lf[r2] + lf[c1] + lf[N - c1] - lf[N] - lf[x] - lf[r1 - x] - lf[c1 - x] - lf[r2 - c1 + x], left to right
 *   4. p = the sum of pow(10, logp(x)) over x ascending from max(0, c1 - r2) to min(r1, c1) with logp(x) <= logp(rf) + 1e-7
 *   5. FS = 0 when N == 0 or p >= 1, else -10 * log10(p)
 * Every intermediate is a volatile double: rounded on its own, never fused with the next operation, whatever compiles this. */
#ifndef SLAMEM_FISHER_H
#define SLAMEM_FISHER_H

#include <math.h>
#include <stdint.h>

static inline double slamem_fisher_logp(const double *lf, uint32_t r1, uint32_t r2, uint32_t c1, uint32_t N, uint32_t x) {
    volatile double v = lf[r1];
    v = v + lf[r2];
    v = v + lf[c1];
    v = v + lf[N - c1];
    v = v - lf[N];
    v = v - lf[x];
    v = v - lf[r1 - x];
    v = v - lf[c1 - x];
    v = v - lf[r2 - c1 + x];
    return v;
}

/* FS of t; norm: the table after step 1 */
static inline double slamem_fisher_strand_of(const uint32_t t[4], uint32_t norm[4]) {
    double lf[402];
    const uint64_t s = (uint64_t)t[0] + t[1] + t[2] + t[3];
    uint32_t r1, r2, c1, N, x, lo, hi, i;
    volatile double cut, p = 0.0, fs;
    for (i = 0; i < 4; i++) norm[i] = s > 400 ? (uint32_t)((uint64_t)t[i] * 200u / s) : t[i];
    r1 = norm[0] + norm[1];
    r2 = norm[2] + norm[3];
    c1 = norm[0] + norm[2];
    N = r1 + r2; /* <= 400 */
    if (N == 0) return 0.0;
    lf[0] = 0.0;
    for (i = 1; i <= N; i++) {
        volatile double l = log10((double)i);
        volatile double sum = lf[i - 1] + l;
        lf[i] = sum;
    }
    cut = slamem_fisher_logp(lf, r1, r2, c1, N, norm[0]);
    cut = cut + 1e-7;
    lo = c1 > r2 ? c1 - r2 : 0;
    hi = r1 < c1 ? r1 : c1;
    for (x = lo; x <= hi; x++) {
        volatile double l = slamem_fisher_logp(lf, r1, r2, c1, N, x);
        if (l <= cut) {
            volatile double term = pow(10.0, l);
            p = p + term;
        }
    }
    if (p >= 1.0) return 0.0;
    fs = log10(p);
    fs = -10.0 * fs;
    return fs;
}

#endif
