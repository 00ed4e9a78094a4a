// pile_filter.hip -- -pile (matchType 8): the per-base pileup of the read mappings, accumulated on the device.  DESIGN.md 4.16
// has the definition; in short, with n the merged text's length, the table has n rows of six counters A, C, G, T, D, I, and
// every segment of a read whose record has strand != 0 and mapq >= min_mapq is walked once, left to right:
//   = / X of k   the scanned strand's letter, if one of A,C,G,T, counts in its column at each of the k rows
//   D of k       column D of the k rows
//   I of k       column I of the row in front of which it stands, once (dropped at row n)
//
// The accumulator is a difference array and a table: int32 diff[n + 1], uint32 cnt[n][6].  An `=` run over [p, p + k) restates
// the text, so it costs two atomics (diff[p] += 1, diff[p + k] -= 1) whatever its length; X, D and I add to cnt directly.  A
// letter under `=` is the text's letter (that is what the operation says), so the rows of the run whose letter is none of
// A,C,G,T are the set bits of the text's letter mask over [p, p + k): the run is split there and those rows get nothing.
//   k_pile_lane    a lane per read: its segments of up to kPileLaneOps operations, one operation after the other
//   k_pile_wave    a wave per 64 reads finds the reads with a longer segment (ballot) and then takes those segments one by one:
//                  64 operations at a time, a wave scan of their lengths gives each lane the p and q of its operation
//   k_pile_tile_sums / k_pile_tile_scan / k_pile_counts
//                  the read-out of rows [first, first + count): the sums of diff per tile of kPileTile entries, their exclusive
//                  prefix sums (one workgroup), and per tile the running sum of diff = match[p], which goes to the column of the
//                  text's letter at p (none when it is not A,C,G,T) on top of cnt.  Nothing of the accumulator is written.
//   k_sites_count / k_sites_tile_scan / k_sites_emit
//                  the sparse read-out (-sites): per tile the number of rows of the range that the rule selects,
//                  the tiles' exclusive prefix sums, and the selected rows written in ascending p at base + rank in the tile
//                  (ballots and popcounts in a wave, the waves' totals through LDS; no atomics).  The rule is evaluated twice
//                  rather than kept as a bitmap: see 4.17.
//   k_pile_add_counts  a table added into cnt (atomicAdd, zeros skipped; diff is not touched)
//   k_pile_lane_masked / k_pile_wave_masked
//                  the two add kernels with a low-quality mask: a bit per letter of the batch's letter buffer,
//                  and a letter whose bit is set counts nowhere under = and X.  The same bodies (a template parameter); an `=`
//                  run ORs the mask's window over its letters into the text's exclusion bits, 64 rows at a time.
//   k_strand_lane / k_strand_wave / k_strand_lane_masked / k_strand_wave_masked
//                  the four add kernels of an accumulator with strand counts: the same bodies with a second
//                  template parameter.  A read of strand 1 issues each of its atomics on the forward accumulator as well; the
//                  operations, offsets and mask windows are loaded and formed once.
// Counters are 32 bits wide and every sum is taken modulo 2^32: a true depth of 2^31 or more at one row is outside the contract.
#include "buffers.h"
#include "pile_shared.h"

#include <new>

namespace slamem {

namespace {

struct PileAcc {
    const TextPlanes* tpl;
    int32_t* diff;   // n + 1
    uint32_t* cnt;   // n x 6
    uint32_t n;
};

// The writes of the walk.  kStrands: `f` is the forward accumulator (the same n, the same text) and `two` says that the read is of
// strand 1, whose every atomic goes to both; without kStrands neither is looked at.
template <bool kStrands>
__device__ __forceinline__ void pile_diff(const PileAcc& a, const PileAcc& f, bool two, uint64_t x, int32_t v) {
    atomicAdd(&a.diff[x], v);
    if constexpr (kStrands) {
        if (two) atomicAdd(&f.diff[x], v);
    }
}
template <bool kStrands>
__device__ __forceinline__ void pile_cnt(const PileAcc& a, const PileAcc& f, bool two, uint64_t at) {
    atomicAdd(&a.cnt[at], 1u);
    if constexpr (kStrands) {
        if (two) atomicAdd(&f.cnt[at], 1u);
    }
}

// an `=` run over rows [p, p + k): rows at and behind n are dropped, rows whose letter is none of A,C,G,T get nothing
template <bool kStrands>
__device__ __forceinline__ void pile_eq(const PileAcc& a, const PileAcc& f, bool two, uint64_t p, uint64_t k) {
    if (k == 0 || p >= a.n) return;
    if (p + k > a.n) k = a.n - p;
    const uint64_t e = p + k;  // <= n
    uint64_t any = 0;
    for (uint64_t u = p >> 6; u <= (e - 1) >> 6; u++) {
        uint64_t m = a.tpl[u].nm;
        if (u == p >> 6) m &= ~0ull << (p & 63u);
        if (u == (e - 1) >> 6 && (e & 63u)) m &= (1ull << (e & 63u)) - 1ull;
        any |= m;
    }
    if (!any) {
        pile_diff<kStrands>(a, f, two, p, 1);
        pile_diff<kStrands>(a, f, two, e, -1);
        return;
    }
    // (rare: only an anchor holds such a letter) row by row, a pair of atomics per stretch of A,C,G,T
    uint64_t start = ~0ull;
    for (uint64_t x = p; x < e; x++) {
        const bool bad = (a.tpl[x >> 6].nm >> (x & 63u)) & 1ull;
        if (!bad && start == ~0ull) start = x;
        if (bad && start != ~0ull) {
            pile_diff<kStrands>(a, f, two, start, 1);
            pile_diff<kStrands>(a, f, two, x, -1);
            start = ~0ull;
        }
    }
    if (start != ~0ull) {
        pile_diff<kStrands>(a, f, two, start, 1);
        pile_diff<kStrands>(a, f, two, e, -1);
    }
}

// an `=` run over rows [p, p + k) that shows letters [q, q + k) of the scanned strand: as pile_eq, with the letters' mask bits
// ORed into the text's, a text word (up to 64 rows) at a time.  A stretch between two excluded bits gets its pair of atomics;
// ctz finds the stretches' ends, and one that reaches the chunk's end stays open into the next chunk -- a run without an
// excluded bit costs its two atomics as before.
template <bool kStrands>
__device__ __forceinline__ void pile_eq_masked(const PileAcc& a, const PileAcc& f, bool two, const PileLow& m, uint64_t p, uint64_t k,
                                               uint64_t q) {
    if (k == 0 || p >= a.n) return;
    if (p + k > a.n) k = a.n - p;
    const uint64_t e = p + k;  // <= n
    uint64_t start = ~0ull;    // the first row of the open stretch
    for (uint64_t x0 = p; x0 < e;) {
        const uint32_t sh = (uint32_t)(x0 & 63u);
        const uint32_t c = e - x0 < 64u - sh ? (uint32_t)(e - x0) : 64u - sh;
        const uint64_t in = c < 64u ? (1ull << c) - 1ull : ~0ull;
        const uint64_t bad = ((a.tpl[x0 >> 6].nm >> sh) | lowq_letters(m, q + (x0 - p), c)) & in;  // bit i: row x0 + i
        uint32_t i = 0;
        while (i < c) {
            if (start == ~0ull) {
                const uint64_t good = ~bad & in & (~0ull << i);
                if (!good) break;
                i = (uint32_t)__builtin_ctzll(good);
                start = x0 + i;
            }
            const uint64_t stop = bad & (~0ull << i);
            if (!stop) break;
            i = (uint32_t)__builtin_ctzll(stop);
            pile_diff<kStrands>(a, f, two, start, 1);
            pile_diff<kStrands>(a, f, two, x0 + i, -1);
            start = ~0ull;
        }
        x0 += c;
    }
    if (start != ~0ull) {
        pile_diff<kStrands>(a, f, two, start, 1);
        pile_diff<kStrands>(a, f, two, e, -1);
    }
}

// one operation at (p, q): every write is checked against n.  kMasked: a letter whose mask bit is set counts nowhere under = and
// X; D and I are as without a mask.  kStrands: f and two as above.
template <bool kMasked, bool kStrands>
__device__ __forceinline__ void pile_op(const PileAcc& a, const PileAcc& f, bool two, const PileRead& r, const PileLow& m, uint32_t op,
                                        uint64_t p, uint64_t q) {
    const uint32_t code = op & 15u;
    const uint64_t k = op >> 4;
    if (code == kOpEq) {
        if constexpr (kMasked) pile_eq_masked<kStrands>(a, f, two, m, p, k, q);
        else pile_eq<kStrands>(a, f, two, p, k);
    } else if (code == kOpX) {
        for (uint64_t j = 0; j < k && p + j < a.n; j++) {
            const uint32_t c = pile_letter(r, q + j);
            if constexpr (kMasked) {
                if (c < 4u && !lowq_letters(m, q + j, 1u)) pile_cnt<kStrands>(a, f, two, (p + j) * 6u + c);
            } else {
                if (c < 4u) pile_cnt<kStrands>(a, f, two, (p + j) * 6u + c);
            }
        }
    } else if (code == kOpD) {
        for (uint64_t j = 0; j < k && p + j < a.n; j++) pile_cnt<kStrands>(a, f, two, (p + j) * 6u + 4u);
    } else if (code == kOpI) {
        if (k && p < a.n) pile_cnt<kStrands>(a, f, two, p * 6u + 5u);
    }
}

// a lane per read: its segments of up to kPileLaneOps operations
template <bool kMasked, bool kStrands>
__device__ __forceinline__ void pile_lane_body(const PileBatch& b, const PileAcc& a, const PileAcc& f, const uint64_t* lowq) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= b.nq) return;
    PileRead rd;
    if (!pile_contributes(b, r, rd)) return;
    const PileLow m = pile_low<kMasked>(b, rd, lowq);
    const uint64_t s1 = b.roff[r + 1];
    for (uint64_t s = b.roff[r]; s < s1; s++) {
        const uint64_t o0 = b.ooff[s], o1 = b.ooff[s + 1];
        if (o1 <= o0 || o1 - o0 > kPileLaneOps) continue;
        const slamem_aln sg = b.segs[s];
        uint64_t p = sg.ref_pos, q = sg.query_pos;
        for (uint64_t i = o0; i < o1; i++) {
            const uint32_t op = b.ops[i];
            pile_op<kMasked, kStrands>(a, f, !rd.rev, rd, m, op, p, q);
            p += pile_ref_step(op);
            q += pile_query_step(op);
        }
    }
}
__global__ void __launch_bounds__(256) k_pile_lane(PileBatch b, PileAcc a) { pile_lane_body<false, false>(b, a, a, nullptr); }
__global__ void __launch_bounds__(256) k_pile_lane_masked(PileBatch b, PileAcc a, const uint64_t* __restrict__ lowq) {
    pile_lane_body<true, false>(b, a, a, lowq);
}
__global__ void __launch_bounds__(256) k_strand_lane(PileBatch b, PileAcc a, PileAcc f) { pile_lane_body<false, true>(b, a, f, nullptr); }
__global__ void __launch_bounds__(256) k_strand_lane_masked(PileBatch b, PileAcc a, PileAcc f, const uint64_t* __restrict__ lowq) {
    pile_lane_body<true, true>(b, a, f, lowq);
}

// a wave per 64 reads: the reads that have a segment of more than kPileLaneOps operations, one after the other; of such a read
// those segments, 64 operations at a time
template <bool kMasked, bool kStrands>
__device__ __forceinline__ void pile_wave_body(const PileBatch& b, const PileAcc& a, const PileAcc& f, const uint64_t* lowq) {
    const uint32_t lane = threadIdx.x;
    const uint64_t chunks = (b.nq + 63u) >> 6;
    PileAcc g = f;
    if constexpr (kStrands) {
        // (the forward pointers live in vector registers: the body is at the limit of the scalar ones, and an atomic's address ends in
        // a vector register anyway)
        asm volatile("" : "+v"(g.diff), "+v"(g.cnt));
    }
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t r = c * 64u + lane;
        bool big = false;
        PileRead mine;
        if (r < b.nq && pile_contributes(b, r, mine)) {
            const uint64_t s1 = b.roff[r + 1];
            for (uint64_t s = b.roff[r]; s < s1 && !big; s++) big = b.ooff[s + 1] - b.ooff[s] > kPileLaneOps && b.ooff[s + 1] > b.ooff[s];
        }
        unsigned long long todo = __ballot(big);
        while (todo) {
            const uint32_t src = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint64_t rr = c * 64u + src;
            PileRead rd;
            (void)pile_contributes(b, rr, rd);  // (it does: its lane said so)
            const PileLow m = pile_low<kMasked>(b, rd, lowq);
            const uint64_t s1 = b.roff[rr + 1];
            for (uint64_t s = b.roff[rr]; s < s1; s++) {
                const uint64_t o0 = b.ooff[s], o1 = b.ooff[s + 1];
                if (o1 <= o0 || o1 - o0 <= kPileLaneOps) continue;
                const slamem_aln sg = b.segs[s];
                uint64_t p = sg.ref_pos, q = sg.query_pos;
                for (uint64_t base = o0; base < o1; base += 64u) {
                    const bool have = base + lane < o1;
                    const uint32_t op = have ? b.ops[base + lane] : 0u;
                    const uint64_t rs = pile_ref_step(op), qs = pile_query_step(op);
                    const uint64_t ri = wave_scan_inclusive(rs, lane), qi = wave_scan_inclusive(qs, lane);
                    if (have) pile_op<kMasked, kStrands>(a, g, !rd.rev, rd, m, op, p + ri - rs, q + qi - qs);
                    p += __shfl(ri, 63, 64);
                    q += __shfl(qi, 63, 64);
                }
            }
        }
    }
}
__global__ void __launch_bounds__(64) k_pile_wave(PileBatch b, PileAcc a) { pile_wave_body<false, false>(b, a, a, nullptr); }
__global__ void __launch_bounds__(64) k_pile_wave_masked(PileBatch b, PileAcc a, const uint64_t* __restrict__ lowq) {
    pile_wave_body<true, false>(b, a, a, lowq);
}
__global__ void __launch_bounds__(64) k_strand_wave(PileBatch b, PileAcc a, PileAcc f) { pile_wave_body<false, true>(b, a, f, nullptr); }
__global__ void __launch_bounds__(64) k_strand_wave_masked(PileBatch b, PileAcc a, PileAcc f, const uint64_t* __restrict__ lowq) {
    pile_wave_body<true, true>(b, a, f, lowq);
}

// ---- read-out --------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t* lds /* 4 words */) {
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t t = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return t;
}

// tile t: the sum of diff[t * kPileTile .. (t + 1) * kPileTile) below `entries`
__global__ void __launch_bounds__(256) k_pile_tile_sums(const int32_t* __restrict__ diff, uint64_t entries, uint32_t* __restrict__ tile) {
    __shared__ uint32_t lds[4];
    const uint64_t base = (uint64_t)blockIdx.x * kPileTile;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPileTile / 256u; j++) {
        const uint64_t x = base + j * 256u + threadIdx.x;
        if (x < entries) v += (uint32_t)diff[x];
    }
    v = block_sum_256(v, lds);
    if (threadIdx.x == 0) tile[blockIdx.x] = v;
}

// in place: tile[t] = the sum of the tiles in front of t (one workgroup of 1024 lanes, a stretch of tiles each)
__global__ void __launch_bounds__(1024) k_pile_tile_scan(uint32_t* __restrict__ tile, uint64_t tiles) {
    __shared__ uint32_t part[1024];
    const uint64_t per = (tiles + 1023u) / 1024u;
    const uint64_t s = (uint64_t)threadIdx.x * per, e = s + per < tiles ? s + per : tiles;
    uint32_t v = 0;
    for (uint64_t x = s; x < e; x++) v += tile[x];
    part[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < 1024u; k++) { const uint32_t t = part[k]; part[k] = run; run += t; }
    }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (uint64_t x = s; x < e; x++) { const uint32_t t = tile[x]; tile[x] = run; run += t; }
}

// tile t of a read-out that ends at `end` (<= n): match[p] = the sum of diff[0 .. p] and the column of the text's letter (4: none
// of A,C,G,T, or a row at or behind `end`) of its kPileTile rows, staged in LDS.  A lane takes kPileTile / 256 consecutive entries.
__device__ __forceinline__ void pile_tile_stage(const int32_t* __restrict__ diff, const uint32_t* __restrict__ tile,
                                                const TextPlanes* __restrict__ tpl, uint64_t t, uint64_t end, uint32_t* match,
                                                uint8_t* code, uint32_t* wsum) {
    const uint64_t base = t * kPileTile;
    constexpr uint32_t per = kPileTile / 256u;
    uint32_t v[per], run = 0;
    const uint64_t x0 = base + (uint64_t)threadIdx.x * per;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        run += x0 + j < end ? (uint32_t)diff[x0 + j] : 0u;
        v[j] = run;
    }
    // the lanes' totals: inside the wave, then across the four waves
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = run;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = tile[t] + inc - run;
    for (uint32_t w = 0; w < wave; w++) before += wsum[w];
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        const uint64_t x = x0 + j;
        const uint32_t at = threadIdx.x * per + j;
        match[at] = before + v[j];
        uint32_t c = 4u;
        if (x < end) {
            const TextPlanes u = tpl[x >> 6];
            const uint32_t bit = (uint32_t)(x & 63u);
            if (!((u.nm >> bit) & 1ull)) c = (uint32_t)((u.p0 >> bit) & 1ull) | ((uint32_t)((u.p1 >> bit) & 1ull) << 1);
        }
        code[at] = (uint8_t)c;
    }
    __syncthreads();
}

// a workgroup per tile of rows: match[p] = the sum of diff[0 .. p], then rows [first, first + count) of the table
__global__ void __launch_bounds__(256) k_pile_counts(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t tile0,
                                                     uint64_t first, uint64_t count, uint32_t* __restrict__ out) {
    __shared__ uint32_t match[kPileTile];
    __shared__ uint8_t code[kPileTile];
    __shared__ uint32_t wsum[4];
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile, end = first + count;  // (end <= n)
    pile_tile_stage(diff, tile, tpl, t, end, match, code, wsum);
    // the rows of the tile inside the range, counter by counter
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    if (hi <= lo) return;
    const uint64_t words = (hi - lo) * 6u;
    const uint32_t* src = cnt + lo * 6u;
    uint32_t* dst = out + (lo - first) * 6u;
    for (uint64_t w = threadIdx.x; w < words; w += 256u) {
        const uint32_t row = (uint32_t)(w / 6u), col = (uint32_t)(w - (uint64_t)row * 6u);
        const uint32_t at = (uint32_t)(lo - base) + row;
        dst[w] = src[w] + (code[at] == col ? match[at] : 0u);
    }
}


// ---- the sparse read-out (-sites) ------------------------------------------------------------------------------------------

struct SitesRule {
    uint32_t mode;       // 0: any counter non-zero; 1: what differs from the text's letter, with enough support
    uint32_t min_depth;  // mode 1: A+C+G+T+D at least this
    uint32_t min_pct;    // mode 1: 100 * counter >= min_pct * depth
};

// row x of the table as the read-out gives it: cnt[x], and match on top of the column of the text's letter
__device__ __forceinline__ void sites_row(const uint32_t* __restrict__ cnt, uint64_t x, uint32_t letter, uint32_t match, uint32_t c[6]) {
    const uint2* r = reinterpret_cast<const uint2*>(cnt + x * 6u);  // (24 bytes a row: 8-byte aligned)
    const uint2 a = r[0], b = r[1], d = r[2];
    c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y; c[4] = d.x; c[5] = d.y;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) c[k] += letter == k ? match : 0u;
}

// the allele mask of a row (bit k: column k of A C G T D I); 0: the row is not selected.  Sums and products in 64 bits.
__device__ __forceinline__ uint32_t sites_mask(const uint32_t c[6], uint32_t letter, const SitesRule& r) {
    uint32_t m = 0;
    if (r.mode == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) m |= (c[k] != 0u ? 1u : 0u) << k;
        return m;
    }
    if (letter >= 4u) return 0u;
    const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4];
    if (d < r.min_depth) return 0u;
    const uint64_t need = (uint64_t)r.min_pct * d;
#pragma unroll
    for (uint32_t k = 0; k < 6u; k++)
        if (k != letter && c[k] != 0u && 100ull * c[k] >= need) m |= 1u << k;
    return m;
}

// the mask of row `at` of the staged tile (0 outside [lo, hi)); rows are taken 256 apart, so a wave reads 64 neighbouring rows
__device__ __forceinline__ uint32_t sites_tile_mask(const uint32_t* __restrict__ cnt, uint64_t base, uint32_t at, uint64_t lo, uint64_t hi,
                                                    const uint32_t* match, const uint8_t* code, const SitesRule& r) {
    const uint64_t x = base + at;
    if (x < lo || x >= hi) return 0u;
    uint32_t c[6];
    sites_row(cnt, x, code[at], match[at], c);
    return sites_mask(c, code[at], r);
}

// a workgroup per tile of rows: sel[blockIdx.x] = how many rows of the tile inside [first, first + count) the rule selects
__global__ void __launch_bounds__(256) k_sites_count(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t tile0,
                                                     uint64_t first, uint64_t count, SitesRule rule, uint64_t* __restrict__ sel) {
    __shared__ uint32_t match[kPileTile];
    __shared__ uint8_t code[kPileTile];
    __shared__ uint32_t wsum[4];
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile, end = first + count;  // (end <= n)
    pile_tile_stage(diff, tile, tpl, t, end, match, code, wsum);
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPileTile / 256u; j++)
        mine += sites_tile_mask(cnt, base, j * 256u + threadIdx.x, lo, hi, match, code, rule) != 0u ? 1u : 0u;
    const uint32_t total = block_sum_256(mine, wsum);  // (pile_tile_stage ended with a barrier: wsum is free)
    if (threadIdx.x == 0) sel[blockIdx.x] = total;
}

// in place: sel[t] = the sum of the tiles in front of t, and sel[tiles] = the sum of all (one workgroup of 1024 lanes)
__global__ void __launch_bounds__(1024) k_sites_tile_scan(uint64_t* __restrict__ sel, uint64_t tiles) {
    __shared__ uint64_t part[1024];
    const uint64_t per = (tiles + 1023u) / 1024u;
    const uint64_t s = (uint64_t)threadIdx.x * per < tiles ? (uint64_t)threadIdx.x * per : tiles, e = s + per < tiles ? s + per : tiles;
    uint64_t v = 0;
    for (uint64_t x = s; x < e; x++) v += sel[x];
    part[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (uint32_t k = 0; k < 1024u; k++) { const uint64_t t = part[k]; part[k] = run; run += t; }
        sel[tiles] = run;
    }
    __syncthreads();
    uint64_t run = part[threadIdx.x];
    for (uint64_t x = s; x < e; x++) { const uint64_t t = sel[x]; sel[x] = run; run += t; }
}

// a workgroup per tile: its selected rows go to sel[blockIdx.x] + rank in the tile, rows behind `capacity` are dropped.  The order
// inside the tile is that of the rows: pass j takes rows j * 256 .. j * 256 + 255, wave w of it 64 neighbours, a lane's rank in
// its wave is the popcount of the ballot below it.
__global__ void __launch_bounds__(256) k_sites_emit(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                    const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t tile0,
                                                    uint64_t first, uint64_t count, SitesRule rule, const uint64_t* __restrict__ sel,
                                                    uint64_t capacity, uint64_t* __restrict__ pos, uint32_t* __restrict__ counts,
                                                    uint8_t* __restrict__ alleles) {
    __shared__ uint32_t match[kPileTile];
    __shared__ uint8_t code[kPileTile];
    __shared__ uint32_t wsum[4];
    constexpr uint32_t per = kPileTile / 256u;
    __shared__ uint32_t wcnt[per * 4u];
    const uint64_t out0 = sel[blockIdx.x];
    if (sel[blockIdx.x + 1] == out0 || out0 >= capacity) return;  // (the whole workgroup: nothing selected, or no room left)
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile, end = first + count;  // (end <= n)
    pile_tile_stage(diff, tile, tpl, t, end, match, code, wsum);
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t mask[per], below[per];
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        mask[j] = sites_tile_mask(cnt, base, j * 256u + threadIdx.x, lo, hi, match, code, rule);
        const unsigned long long b = __ballot(mask[j] != 0u);
        below[j] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0u) wcnt[j * 4u + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t run = 0;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            if (w == wave) mine = run;
            run += wcnt[j * 4u + w];
        }
        const uint64_t o = out0 + mine + below[j];
        if (mask[j] == 0u || o >= capacity) continue;
        const uint32_t at = j * 256u + threadIdx.x;
        uint32_t c[6];
        sites_row(cnt, base + at, code[at], match[at], c);
        pos[o] = base + at;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) counts[o * 6u + k] = c[k];
        alleles[o] = (uint8_t)mask[j];
    }
}

// cnt[first + i][k] += rows[i][k]: a lane per counter, zeros skipped, rows at or behind n dropped
__global__ void __launch_bounds__(256) k_pile_add_counts(uint32_t* __restrict__ cnt, uint64_t n, uint64_t first, uint64_t count,
                                                         const uint32_t* __restrict__ rows) {
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w >= count * 6u) return;
    const uint32_t v = rows[w];
    const uint64_t at = first * 6u + w;
    if (v != 0u && at < n * 6u) atomicAdd(&cnt[at], v);
}

}  // namespace

}  // namespace slamem

using namespace slamem;

namespace slamem {

int pileup_device(const slamem_pileup* p) { return p->device; }

int pileup_add(slamem_pileup* pile, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
               const slamem_aln* segs_dev, const uint64_t* read_offsets_dev, const uint32_t* ops_dev, const uint64_t* op_offsets_dev,
               const slamem_map* reads_dev, uint32_t min_mapq, hipStream_t stream) {
    return pileup_add_masked(pile, queries_dev, offsets_dev, num_queries, segs_dev, read_offsets_dev, ops_dev, op_offsets_dev, reads_dev,
                             min_mapq, nullptr, stream);
}

int pileup_add_masked(slamem_pileup* pile, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                      const slamem_aln* segs_dev, const uint64_t* read_offsets_dev, const uint32_t* ops_dev,
                      const uint64_t* op_offsets_dev, const slamem_map* reads_dev, uint32_t min_mapq, const uint64_t* lowq_dev,
                      hipStream_t stream) {
    if (num_queries == 0) return SLAMEM_OK;
    PileBatch b;
    b.queries = static_cast<const unsigned char*>(queries_dev);
    b.offsets = offsets_dev;
    b.segs = segs_dev;
    b.roff = read_offsets_dev;
    b.ops = ops_dev;
    b.ooff = op_offsets_dev;
    b.reads = reads_dev;
    b.nq = num_queries;
    b.min_mapq = min_mapq;
    PileAcc a;
    a.tpl = pile->idx->view.tpl;
    a.diff = pile->diff;
    a.cnt = pile->cnt;
    a.n = pile->n;
    const unsigned chunks = pile_grid(num_queries, 64);
    const dim3 lane_grid(pile_grid(num_queries, 256)), wave_grid(chunks < kPileWaveGrid ? chunks : kPileWaveGrid);
    pile->used.store(true, std::memory_order_relaxed);
    if (pile->fwd) {  // (one walk of the reads, the atomics of the strand-1 reads on both accumulators)
        PileAcc f = a;
        f.diff = pile->fwd->diff;
        f.cnt = pile->fwd->cnt;
        pile->fwd->used.store(true, std::memory_order_relaxed);
        if (lowq_dev) {
            hipLaunchKernelGGL(k_strand_lane_masked, lane_grid, dim3(256), 0, stream, b, a, f, lowq_dev);
            SLAMEM_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_strand_wave_masked, wave_grid, dim3(64), 0, stream, b, a, f, lowq_dev);
            SLAMEM_HIP(hipGetLastError());
        } else {
            hipLaunchKernelGGL(k_strand_lane, lane_grid, dim3(256), 0, stream, b, a, f);
            SLAMEM_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_strand_wave, wave_grid, dim3(64), 0, stream, b, a, f);
            SLAMEM_HIP(hipGetLastError());
        }
    } else if (lowq_dev) {  // (the same two kernels with the mask; without one, the instantiations that were there before)
        hipLaunchKernelGGL(k_pile_lane_masked, lane_grid, dim3(256), 0, stream, b, a, lowq_dev);
        SLAMEM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pile_wave_masked, wave_grid, dim3(64), 0, stream, b, a, lowq_dev);
        SLAMEM_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_pile_lane, lane_grid, dim3(256), 0, stream, b, a);
        SLAMEM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pile_wave, wave_grid, dim3(64), 0, stream, b, a);
        SLAMEM_HIP(hipGetLastError());
    }
    if (pile->ev) SLAMEM_TRY(events_add(pile, &b, stream));  // (the indel events of the same batch, behind the two kernels)
    if (pile->sv) SLAMEM_TRY(junctions_add(pile, &b, stream));  // (the breaks between the batch's segments)
    return SLAMEM_OK;
}

int pile_tile_prefix(slamem_pileup* pile, uint64_t end, hipStream_t stream) {
    const uint64_t tiles = (end + kPileTile - 1) / kPileTile;
    hipLaunchKernelGGL(k_pile_tile_sums, dim3((unsigned)tiles), dim3(256), 0, stream, (const int32_t*)pile->diff, end, pile->tile);
    SLAMEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pile_tile_scan, dim3(1), dim3(1024), 0, stream, pile->tile, tiles);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int pile_refuse_child(const slamem_pileup* pile, const char* fn) {
    if (!pile->child) return SLAMEM_OK;
    set_error("%s: this is the %s accumulator of another (%s): it is read, and counts may be added to it, but "
              "its owner adds the reads, enables and frees", fn, pile->child_qual ? "quality" : "forward",
              pile->child_qual ? "slamem_pileup_quality" : "slamem_pileup_forward");
    return SLAMEM_ERR_ARG;
}

int pile_refuse_quals(const slamem_pileup* pile, const char* fn) {
    if (!pile->qual) return SLAMEM_OK;
    set_error("%s: this accumulator keeps quality sums (slamem_pileup_enable_quals), which an add without quality bytes would leave "
              "behind its counts: add the reads with slamem_pileup_add_quals_device", fn);
    return SLAMEM_ERR_ARG;
}

int pile_scan_counts(uint64_t* sel, uint64_t tiles, hipStream_t stream) {
    hipLaunchKernelGGL(k_sites_tile_scan, dim3(1), dim3(1024), 0, stream, sel, tiles);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

}  // namespace slamem

extern "C" {

// the accumulator of slamem_pileup_create (role 0), the forward one of slamem_pileup_enable_strands (1) and the quality one of
// slamem_pileup_enable_quals (2); `fn` names the caller in messages
static int pile_new(const slamem_index* idx, const char* fn, int role, slamem_pileup** out) {
    const bool child = role != 0;
    SLAMEM_HIP(hipSetDevice(idx->device));
    const uint64_t n = idx->hdr.n;
    const uint64_t tiles = n / kPileTile + 2;
    const uint64_t need = (n + 1) * 4 + n * 24 + tiles * 12;
    size_t free_b = 0, total_b = 0;
    SLAMEM_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        set_error("%s: the %saccumulator of a text of %llu letters takes %llu bytes (28 per letter), %llu are free on "
                  "device %d", fn, role == 1 ? "forward " : role == 2 ? "quality " : "", (unsigned long long)n, (unsigned long long)need, (unsigned long long)free_b,
                  idx->device);
        return SLAMEM_ERR_NOMEM;
    }
    slamem_pileup* p = new (std::nothrow) slamem_pileup();
    if (!p) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    p->idx = idx; p->device = idx->device; p->n = (uint32_t)n;
    p->diff = nullptr; p->cnt = nullptr; p->tile = nullptr; p->sel = nullptr; p->ev = nullptr; p->sv = nullptr; p->cons = nullptr; p->depth = nullptr; p->dd = nullptr;
    p->fwd = nullptr; p->qual = nullptr; p->child = false; p->child_qual = false; p->used.store(false, std::memory_order_relaxed);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->diff), (n + 1) * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->cnt), n * 24 + 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->tile), tiles * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->sel), tiles * 8);
    if (e == hipSuccess) e = hipMemset(p->diff, 0, (n + 1) * 4);
    if (e == hipSuccess) e = hipMemset(p->cnt, 0, n * 24);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)slamem_pileup_free(p);
        return hip_fail(e, fn, __FILE__, __LINE__);
    }
    p->child = child;
    p->child_qual = role == 2;
    *out = p;
    return SLAMEM_OK;
}

int slamem_pileup_create(const slamem_index* idx, slamem_pileup** out) {
    if (!idx || !out) { set_error("slamem_pileup_create: null argument"); return SLAMEM_ERR_ARG; }
    *out = nullptr;
    if (idx->hdr.off_tpl == 0 || !idx->view.tpl) {
        set_error("slamem_pileup_create: -pile reads the text planes of the index, and this index has none (the compact layout, or "
                  "one built without the seed sections)");
        return SLAMEM_ERR_ARG;
    }
    return pile_new(idx, "slamem_pileup_create", 0, out);
}

int slamem_pileup_enable_strands(slamem_pileup* pile) {
    if (!pile) { set_error("slamem_pileup_enable_strands: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_enable_strands"));
    if (pile->fwd) return SLAMEM_OK;
    if (pile->used.load(std::memory_order_relaxed)) {
        set_error("slamem_pileup_enable_strands: something was added to this accumulator already; strand counts start on an empty one "
                  "(just created, or after slamem_pileup_reset)");
        return SLAMEM_ERR_ARG;
    }
    return pile_new(pile->idx, "slamem_pileup_enable_strands", 1, &pile->fwd);
}

int slamem_pileup_forward(slamem_pileup* pile, slamem_pileup** out) {
    if (!pile || !out) { set_error("slamem_pileup_forward: null argument"); return SLAMEM_ERR_ARG; }
    *out = pile->fwd;
    if (!pile->fwd) {
        set_error("slamem_pileup_forward: the strand counts of this accumulator are not enabled (slamem_pileup_enable_strands)");
        return SLAMEM_ERR_ARG;
    }
    return SLAMEM_OK;
}

int slamem_pileup_enable_quals(slamem_pileup* pile) {
    if (!pile) { set_error("slamem_pileup_enable_quals: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_enable_quals"));
    if (pile->qual) return SLAMEM_OK;
    if (pile->used.load(std::memory_order_relaxed)) {
        set_error("slamem_pileup_enable_quals: something was added to this accumulator already; quality sums start on an empty one "
                  "(just created, or after slamem_pileup_reset)");
        return SLAMEM_ERR_ARG;
    }
    return pile_new(pile->idx, "slamem_pileup_enable_quals", 2, &pile->qual);
}

int slamem_pileup_quality(slamem_pileup* pile, slamem_pileup** out) {
    if (!pile || !out) { set_error("slamem_pileup_quality: null argument"); return SLAMEM_ERR_ARG; }
    *out = pile->qual;
    if (!pile->qual) {
        set_error("slamem_pileup_quality: the quality sums of this accumulator are not enabled (slamem_pileup_enable_quals)");
        return SLAMEM_ERR_ARG;
    }
    return SLAMEM_OK;
}

static void pile_release(slamem_pileup* p) {
    (void)hipSetDevice(p->device);
    if (p->fwd) { pile_release(p->fwd); p->fwd = nullptr; }
    if (p->qual) { pile_release(p->qual); p->qual = nullptr; }
    if (p->diff) (void)hipFree(p->diff);
    if (p->cnt) (void)hipFree(p->cnt);
    if (p->tile) (void)hipFree(p->tile);
    if (p->sel) (void)hipFree(p->sel);
    events_free(p);
    junctions_free(p);
    cons_free(p);
    depth_free(p);
    dedup_free(p);
    delete p;
}

int slamem_pileup_free(slamem_pileup* p) {
    if (!p) return SLAMEM_OK;
    SLAMEM_TRY(pile_refuse_child(p, "slamem_pileup_free"));
    pile_release(p);
    return SLAMEM_OK;
}

int slamem_pileup_reset(slamem_pileup* p) {
    if (!p) { set_error("slamem_pileup_reset: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(p->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (adds of any stream that are still on their way belong to the table that goes)
    SLAMEM_HIP(hipMemset(p->diff, 0, ((uint64_t)p->n + 1) * 4));
    SLAMEM_HIP(hipMemset(p->cnt, 0, (uint64_t)p->n * 24));
    if (p->ev) { const int rc = events_reset(p); if (rc != SLAMEM_OK) return rc; }
    if (p->sv) { const int rc = junctions_reset(p); if (rc != SLAMEM_OK) return rc; }
    if (p->dd) { const int rc = dedup_reset(p); if (rc != SLAMEM_OK) return rc; }
    for (slamem_pileup* c : {p->fwd, p->qual}) {  // (a forward or a quality accumulator has neither events nor a filter)
        if (!c) continue;
        SLAMEM_HIP(hipMemset(c->diff, 0, ((uint64_t)p->n + 1) * 4));
        SLAMEM_HIP(hipMemset(c->cnt, 0, (uint64_t)p->n * 24));
    }
    SLAMEM_HIP(hipDeviceSynchronize());
    p->used.store(false, std::memory_order_relaxed);
    if (p->fwd) p->fwd->used.store(false, std::memory_order_relaxed);
    if (p->qual) p->qual->used.store(false, std::memory_order_relaxed);
    return SLAMEM_OK;
}

int slamem_pileup_add_device(slamem_pileup* pile, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                             const slamem_aln* segs_dev, const uint64_t* read_offsets_dev, const uint32_t* ops_dev,
                             const uint64_t* op_offsets_dev, const slamem_map* reads_dev, uint32_t min_mapq, void* stream) {
    if (!pile || !offsets_dev || !read_offsets_dev || !op_offsets_dev || !reads_dev || (num_queries && (!queries_dev || !segs_dev || !ops_dev))) {
        set_error("slamem_pileup_add_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_add_device"));
    SLAMEM_TRY(pile_refuse_quals(pile, "slamem_pileup_add_device"));
    if (min_mapq > 60u) { set_error("slamem_pileup_add_device: the minimum mapping quality is 0 to 60"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(pile->device));
    return pileup_add(pile, queries_dev, offsets_dev, num_queries, segs_dev, read_offsets_dev, ops_dev, op_offsets_dev, reads_dev,
                      min_mapq, static_cast<hipStream_t>(stream));
}

int slamem_pileup_add_masked_device(slamem_pileup* pile, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                                    const slamem_aln* segs_dev, const uint64_t* read_offsets_dev, const uint32_t* ops_dev,
                                    const uint64_t* op_offsets_dev, const slamem_map* reads_dev, uint32_t min_mapq,
                                    const uint64_t* lowq_dev, void* stream) {
    if (!pile || !offsets_dev || !read_offsets_dev || !op_offsets_dev || !reads_dev || (num_queries && (!queries_dev || !segs_dev || !ops_dev))) {
        set_error("slamem_pileup_add_masked_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_add_masked_device"));
    SLAMEM_TRY(pile_refuse_quals(pile, "slamem_pileup_add_masked_device"));
    if (min_mapq > 60u) { set_error("slamem_pileup_add_masked_device: the minimum mapping quality is 0 to 60"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(pile->device));
    return pileup_add_masked(pile, queries_dev, offsets_dev, num_queries, segs_dev, read_offsets_dev, ops_dev, op_offsets_dev,
                             reads_dev, min_mapq, lowq_dev, static_cast<hipStream_t>(stream));
}

int slamem_pileup_counts_device(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t* out_dev, void* stream) {
    if (!pile || (count && !out_dev)) { set_error("slamem_pileup_counts_device: null argument"); return SLAMEM_ERR_ARG; }
    if (first > pile->n || count > pile->n - first) {
        set_error("slamem_pileup_counts_device: rows %llu .. %llu + %llu lie outside the text's %u", (unsigned long long)first,
                  (unsigned long long)first, (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    if (count == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t end = first + count, tiles = (end + kPileTile - 1) / kPileTile, tile0 = first / kPileTile;
    hipLaunchKernelGGL(k_pile_tile_sums, dim3((unsigned)tiles), dim3(256), 0, st, (const int32_t*)pile->diff, end, pile->tile);
    SLAMEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pile_tile_scan, dim3(1), dim3(1024), 0, st, pile->tile, tiles);
    SLAMEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pile_counts, dim3((unsigned)(tiles - tile0)), dim3(256), 0, st, (const int32_t*)pile->diff,
                       (const uint32_t*)pile->cnt, (const uint32_t*)pile->tile, pile->idx->view.tpl, tile0, first, count, out_dev);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int slamem_pileup_counts_host(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t* out) {
    if (!pile || (count && !out)) { set_error("slamem_pileup_counts_host: null argument"); return SLAMEM_ERR_ARG; }
    if (first > pile->n || count > pile->n - first) {
        set_error("slamem_pileup_counts_host: rows %llu .. %llu + %llu lie outside the text's %u", (unsigned long long)first,
                  (unsigned long long)first, (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    if (count == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    DevBuf<uint32_t> d;
    SLAMEM_TRY(d.reserve(count * 6));
    SLAMEM_TRY(slamem_pileup_counts_device(pile, first, count, d.get(), nullptr));
    SLAMEM_HIP(hipMemcpy(out, d.get(), count * 24, hipMemcpyDeviceToHost));
    return SLAMEM_OK;
}

int slamem_pileup_sites_device(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t mode, uint32_t min_depth, uint32_t min_pct,
                               uint64_t capacity, uint64_t* pos_dev, uint32_t* counts_dev, uint8_t* alleles_dev, uint64_t* total_out,
                               void* stream) {
    if (!pile || !total_out || (capacity && (!pos_dev || !counts_dev || !alleles_dev))) {
        set_error("slamem_pileup_sites_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    if (first > pile->n || count > pile->n - first) {
        set_error("slamem_pileup_sites_device: rows %llu .. %llu + %llu lie outside the text's %u", (unsigned long long)first,
                  (unsigned long long)first, (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    if (mode > 1u) { set_error("slamem_pileup_sites_device: the mode is 0 (non-zero rows) or 1 (variant rows), not %u", mode); return SLAMEM_ERR_ARG; }
    if (min_pct > 100u) { set_error("slamem_pileup_sites_device: the least share is 0 to 100 percent, not %u", min_pct); return SLAMEM_ERR_ARG; }
    if (mode == 1u && (min_depth == 0u || min_depth >= 0x80000000u)) {
        set_error("slamem_pileup_sites_device: the least depth is 1 to 2^31 - 1, not %u", min_depth);
        return SLAMEM_ERR_ARG;
    }
    if (count == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t end = first + count, tiles = (end + kPileTile - 1) / kPileTile, tile0 = first / kPileTile, mine = tiles - tile0;
    const SitesRule rule{mode, min_depth, min_pct};
    hipLaunchKernelGGL(k_pile_tile_sums, dim3((unsigned)tiles), dim3(256), 0, st, (const int32_t*)pile->diff, end, pile->tile);
    SLAMEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pile_tile_scan, dim3(1), dim3(1024), 0, st, pile->tile, tiles);
    SLAMEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sites_count, dim3((unsigned)mine), dim3(256), 0, st, (const int32_t*)pile->diff, (const uint32_t*)pile->cnt,
                       (const uint32_t*)pile->tile, pile->idx->view.tpl, tile0, first, count, rule, pile->sel);
    SLAMEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sites_tile_scan, dim3(1), dim3(1024), 0, st, pile->sel, mine);  // (mine + 1 <= n / kPileTile + 2 words)
    SLAMEM_HIP(hipGetLastError());
    if (capacity) {  // rows behind `capacity` are dropped on the device, so the pass may run before the total is known
        hipLaunchKernelGGL(k_sites_emit, dim3((unsigned)mine), dim3(256), 0, st, (const int32_t*)pile->diff, (const uint32_t*)pile->cnt,
                           (const uint32_t*)pile->tile, pile->idx->view.tpl, tile0, first, count, rule, (const uint64_t*)pile->sel,
                           capacity, pos_dev, counts_dev, alleles_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    uint64_t total = 0;  // the call's one host round trip
    SLAMEM_HIP(hipMemcpyAsync(&total, pile->sel + mine, 8, hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipStreamSynchronize(st));
    *total_out = total;
    if (total > capacity) {
        set_error("slamem_pileup_sites_device: %llu rows are selected, the buffers hold %llu", (unsigned long long)total,
                  (unsigned long long)capacity);
        return SLAMEM_ERR_CAPACITY;
    }
    return SLAMEM_OK;
}

int slamem_pileup_sites_host(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t mode, uint32_t min_depth, uint32_t min_pct,
                             uint64_t capacity, uint64_t* pos, uint32_t* counts, uint8_t* alleles, uint64_t* total_out) {
    if (!pile || !total_out || (capacity && (!pos || !counts || !alleles))) {
        set_error("slamem_pileup_sites_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    const uint64_t room = capacity < count ? capacity : count;  // (a range selects at most its rows)
    DevBuf<char> d;
    if (room) SLAMEM_TRY(d.reserve(room * 33));
    char* b = d.get();
    uint64_t* pd = reinterpret_cast<uint64_t*>(b);
    uint32_t* cd = reinterpret_cast<uint32_t*>(b + room * 8);
    uint8_t* ad = reinterpret_cast<uint8_t*>(b + room * 32);
    const int rc = slamem_pileup_sites_device(pile, first, count, mode, min_depth, min_pct, room, pd, cd, ad, total_out, nullptr);
    if (rc != SLAMEM_OK && rc != SLAMEM_ERR_CAPACITY) return rc;
    // (the rows that fitted go back with SLAMEM_ERR_CAPACITY too; the call's code comes before a failed copy's)
    const uint64_t got = *total_out < room ? *total_out : room;
    hipError_t e = hipSuccess;
    if (got) e = hipMemcpy(pos, pd, got * 8, hipMemcpyDeviceToHost);
    if (got && e == hipSuccess) e = hipMemcpy(counts, cd, got * 24, hipMemcpyDeviceToHost);
    if (got && e == hipSuccess) e = hipMemcpy(alleles, ad, got, hipMemcpyDeviceToHost);
    if (rc == SLAMEM_OK && e != hipSuccess) return hip_fail(e, "hipMemcpy", __FILE__, __LINE__);
    return rc;
}

int slamem_pileup_add_counts_device(slamem_pileup* pile, uint64_t first, uint64_t count, const uint32_t* rows_dev, void* stream) {
    if (!pile || (count && !rows_dev)) { set_error("slamem_pileup_add_counts_device: null argument"); return SLAMEM_ERR_ARG; }
    if (first > pile->n || count > pile->n - first) {
        set_error("slamem_pileup_add_counts_device: rows %llu .. %llu + %llu lie outside the text's %u", (unsigned long long)first,
                  (unsigned long long)first, (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    if (count == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    pile->used.store(true, std::memory_order_relaxed);
    hipLaunchKernelGGL(k_pile_add_counts, dim3(pile_grid(count * 6u, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pile->cnt,
                       (uint64_t)pile->n, first, count, rows_dev);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int slamem_pileup_add_counts_host(slamem_pileup* pile, uint64_t first, uint64_t count, const uint32_t* rows) {
    if (!pile || (count && !rows)) { set_error("slamem_pileup_add_counts_host: null argument"); return SLAMEM_ERR_ARG; }
    if (first > pile->n || count > pile->n - first) {
        set_error("slamem_pileup_add_counts_host: rows %llu .. %llu + %llu lie outside the text's %u", (unsigned long long)first,
                  (unsigned long long)first, (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    if (count == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    DevBuf<uint32_t> d;
    SLAMEM_TRY(d.reserve(count * 6));
    SLAMEM_HIP(hipMemcpy(d.get(), rows, count * 24, hipMemcpyHostToDevice));
    SLAMEM_TRY(slamem_pileup_add_counts_device(pile, first, count, d.get(), nullptr));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the buffer goes when this returns)
    return SLAMEM_OK;
}

}  // extern "C"
