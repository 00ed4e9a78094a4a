// gt_filter.hip -- -gt: a genotype with QUAL, GQ and PL per row of the pileup and per indel event, from the six
// counters of the row and the strand counts of the event, under a constant per-letter error rate.  Everything is an unsigned
// 64-bit integer in milli-Phred; include/slamem_hip.h and DESIGN.md have the definition.
//   (pile_tile_prefix)   the sums of diff in front of every tile of kPileTile rows
//   k_gt_count           a workgroup per tile: the rows as k_pile_counts forms them from diff, tile, cnt and the text's letter, the
//                        rule on each, and the number of selected rows of the tile inside the range
//   (pile_scan_counts)   the tiles' exclusive prefix sums, with the total behind them
//   k_gt_emit            a workgroup per tile: the same again; the selected rows go to the tile's offset + their rank in the tile
//                        (ballots and popcounts in a wave, the waves' totals through LDS; no atomics), rows at or behind
//                        `capacity` are dropped: pos, the six counters and the slamem_genotype
//   k_gtw_count / k_gtw_emit
//                        the two passes of the weighted read-out (-wq): the tile of the quality accumulator is
//                        staged beside the counts', and a letter that a genotype does not hold costs E and 1000 times its quality
//   k_gt_events          a lane per given event: its genotype against everything else at its anchor row, and whether it is called
// The rule is evaluated in both passes rather than kept, as -sites does it (4.17).  The ten (four, three) scores of a row are
// formed with compile-time indices only -- every loop over genotypes is unrolled and a genotype's number is compared, never used
// as an index -- so they live in registers; the costs are kernel arguments.  Nothing of the accumulator is written.  The rule
// itself (GtRule, GtCall, gt_call, gt_snv, gt_event) is gt_shared.h's, which the consensus of -cons -gt reads as well.
#include "buffers.h"
#include "gt_shared.h"
#include "pile_shared.h"

namespace slamem {

namespace {

// the record as it is stored: 14 words, the padding 0 (a record is 4-byte aligned: 56 bytes behind one another)
__device__ __forceinline__ void gt_store(slamem_genotype* __restrict__ at, const GtCall& g, uint32_t ploidy, uint32_t ref) {
    uint32_t* w = reinterpret_cast<uint32_t*>(at);
    w[0] = g.qual;
    w[1] = g.gq;
    w[2] = g.a | (g.b << 8) | (ploidy << 16) | (ref << 24);
#pragma unroll
    for (uint32_t k = 0; k < 10u; k++) w[3u + k] = g.pl[k];
    w[13] = 0u;
}

struct GtTile {
    uint32_t match[kPileTile];  // the sum of diff[0 .. p]
    uint8_t code[kPileTile];    // the text's letter, 4: none of A,C,G,T, or a row at or behind the range's end
    uint32_t wsum[4];
};

// tile t of a read-out that ends at `end` (<= n), staged as pile_filter.hip stages it: a lane takes kPileTile / 256 consecutive
// entries of diff, a wave scan of the lanes' sums, the four waves through LDS.  Ends with a barrier.
__device__ __forceinline__ void gt_tile_stage(const int32_t* __restrict__ diff, const uint32_t* __restrict__ tile,
                                              const TextPlanes* __restrict__ tpl, uint64_t t, uint64_t end, GtTile& s) {
    const uint64_t base = t * kPileTile;
    constexpr uint32_t per = kPileTile / 256u;
    uint32_t v[per], run = 0;
    const uint64_t x0 = base + (uint64_t)threadIdx.x * per;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        run += x0 + j < end ? (uint32_t)diff[x0 + j] : 0u;
        v[j] = run;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = run;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63u) s.wsum[wave] = inc;
    __syncthreads();
    uint32_t before = tile[t] + inc - run;
    for (uint32_t w = 0; w < wave; w++) before += s.wsum[w];
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        const uint64_t x = x0 + j;
        const uint32_t at = threadIdx.x * per + j;
        s.match[at] = before + v[j];
        uint32_t c = 4u;
        if (x < end) {
            const TextPlanes u = tpl[x >> 6];
            const uint32_t bit = (uint32_t)(x & 63u);
            if (!((u.nm >> bit) & 1ull)) c = (uint32_t)((u.p0 >> bit) & 1ull) | ((uint32_t)((u.p1 >> bit) & 1ull) << 1);
        }
        s.code[at] = (uint8_t)c;
    }
    __syncthreads();
}

// row x of the table as the read-out gives it: cnt[x], and match on top of the column of the text's letter
__device__ __forceinline__ void gt_row(const uint32_t* __restrict__ cnt, uint64_t x, uint32_t letter, uint32_t match, uint32_t (&c)[6]) {
    const uint2* r = reinterpret_cast<const uint2*>(cnt + x * 6u);  // (24 bytes a row: 8-byte aligned)
    const uint2 a = r[0], b = r[1], d = r[2];
    c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y; c[4] = d.x; c[5] = d.y;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) c[k] += letter == k ? match : 0u;
}

// the rule on a row: its letter one of A,C,G,T, deep enough, the best genotype not the reference's, qual high enough
__device__ __forceinline__ bool gt_row_call(const uint32_t (&c)[6], uint32_t letter, const GtRule& p, GtCall& out) {
    if (letter >= 4u) return false;
    const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4];
    if (d < p.min_depth) return false;
    const uint32_t acgt[4] = {c[0], c[1], c[2], c[3]};
    uint64_t qual;
    const bool variant = gt_snv<false>(acgt, acgt, letter, p, out, qual);
    return variant && qual >= p.min_qual;
}

// the same rule with the row's quality sums qc (the row of the quality accumulator as the read-out gives it)
__device__ __forceinline__ bool gtw_row_call(const uint32_t (&c)[6], const uint32_t (&qc)[6], uint32_t letter, const GtRule& p, GtCall& out) {
    if (letter >= 4u) return false;
    const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4];
    if (d < p.min_depth) return false;
    const uint32_t acgt[4] = {c[0], c[1], c[2], c[3]}, qs[4] = {qc[0], qc[1], qc[2], qc[3]};
    uint64_t qual;
    const bool variant = gt_snv<true>(acgt, qs, letter, p, out, qual);
    return variant && qual >= p.min_qual;
}

// is row `at` of the staged tile (inside [lo, hi)) selected?  Rows are taken 256 apart, so a wave reads 64 neighbouring rows.
__device__ __forceinline__ bool gt_tile_selected(const uint32_t* __restrict__ cnt, uint64_t base, uint32_t at, uint64_t lo, uint64_t hi,
                                                 const GtTile& s, const GtRule& p) {
    const uint64_t x = base + at;
    if (x < lo || x >= hi) return false;
    uint32_t c[6];
    GtCall call;
    gt_row(cnt, x, s.code[at], s.match[at], c);
    return gt_row_call(c, s.code[at], p, call);
}

// a workgroup per tile of rows: sel[blockIdx.x] = how many rows of the tile inside [first, first + count) are selected
__global__ void __launch_bounds__(256) k_gt_count(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                  const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t tile0,
                                                  uint64_t first, uint64_t count, GtRule rule, uint64_t* __restrict__ sel) {
    __shared__ GtTile s;
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile, end = first + count;  // (end <= n)
    gt_tile_stage(diff, tile, tpl, t, end, s);
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    uint32_t mine = 0;
    for (uint32_t j = 0; j < kPileTile / 256u; j++) mine += gt_tile_selected(cnt, base, j * 256u + threadIdx.x, lo, hi, s, rule) ? 1u : 0u;
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63u) == 0u) s.wsum[threadIdx.x >> 6] = mine;  // (gt_tile_stage ended with a barrier: wsum is free)
    __syncthreads();
    if (threadIdx.x == 0) sel[blockIdx.x] = s.wsum[0] + s.wsum[1] + s.wsum[2] + s.wsum[3];
}

// a workgroup per tile: its selected rows go to sel[blockIdx.x] + rank in the tile, rows at or behind `capacity` are dropped.  The
// order inside the tile is that of the rows: pass j takes rows j * 256 .. j * 256 + 255, wave w of it 64 neighbours, a lane's rank
// in its wave is the popcount of the ballot below it.
__global__ void __launch_bounds__(256) k_gt_emit(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                 const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t tile0,
                                                 uint64_t first, uint64_t count, GtRule rule, const uint64_t* __restrict__ sel,
                                                 uint64_t capacity, uint64_t* __restrict__ pos, uint32_t* __restrict__ counts,
                                                 slamem_genotype* __restrict__ gts) {
    __shared__ GtTile s;
    constexpr uint32_t per = kPileTile / 256u;
    __shared__ uint32_t wcnt[per * 4u];
    const uint64_t out0 = sel[blockIdx.x];
    if (sel[blockIdx.x + 1] == out0 || out0 >= capacity) return;  // (the whole workgroup: nothing selected, or no room left)
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile, end = first + count;  // (end <= n)
    gt_tile_stage(diff, tile, tpl, t, end, s);
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t chosen = 0, below[per];
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        const bool on = gt_tile_selected(cnt, base, j * 256u + threadIdx.x, lo, hi, s, rule);
        chosen |= (on ? 1u : 0u) << j;
        const unsigned long long b = __ballot(on);
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
        if (!((chosen >> j) & 1u) || o >= capacity) continue;
        const uint32_t at = j * 256u + threadIdx.x;
        uint32_t c[6];
        GtCall call;
        gt_row(cnt, base + at, s.code[at], s.match[at], c);
        (void)gt_row_call(c, s.code[at], rule, call);  // (it is selected: the pass above said so)
        pos[o] = base + at;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) counts[o * 6u + k] = c[k];
        gt_store(gts + o, call, rule.ploidy, s.code[at]);
    }
}

// ---- the weighted read-out (-wq) ----------------------------------------------------------------------------------
// The two passes again with the quality accumulator beside the counts: its tile is staged the same way (its own diff and tile sums,
// the same text), so a row's quality sums are its cnt row with match on top of the column of the text's letter.

struct GtwAcc {
    const int32_t* diff;
    const uint32_t* cnt;
    const uint32_t* tile;
};

__device__ __forceinline__ bool gtw_tile_selected(const GtwAcc& a, const GtwAcc& q, uint64_t base, uint32_t at, uint64_t lo, uint64_t hi,
                                                  const GtTile& s, const GtTile& sq, const GtRule& p, uint32_t (&c)[6], uint32_t (&qc)[6],
                                                  GtCall& call) {
    const uint64_t x = base + at;
    if (x < lo || x >= hi) return false;
    gt_row(a.cnt, x, s.code[at], s.match[at], c);
    gt_row(q.cnt, x, s.code[at], sq.match[at], qc);
    return gtw_row_call(c, qc, s.code[at], p, call);
}

__global__ void __launch_bounds__(256) k_gtw_count(GtwAcc a, GtwAcc q, const TextPlanes* __restrict__ tpl, uint64_t tile0, uint64_t first,
                                                   uint64_t count, GtRule rule, uint64_t* __restrict__ sel) {
    __shared__ GtTile s, sq;
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile, end = first + count;  // (end <= n)
    gt_tile_stage(a.diff, a.tile, tpl, t, end, s);
    gt_tile_stage(q.diff, q.tile, tpl, t, end, sq);
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    uint32_t mine = 0;
    for (uint32_t j = 0; j < kPileTile / 256u; j++) {
        uint32_t c[6], qc[6];
        GtCall call;
        mine += gtw_tile_selected(a, q, base, j * 256u + threadIdx.x, lo, hi, s, sq, rule, c, qc, call) ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63u) == 0u) s.wsum[threadIdx.x >> 6] = mine;  // (gt_tile_stage ended with a barrier: wsum is free)
    __syncthreads();
    if (threadIdx.x == 0) sel[blockIdx.x] = s.wsum[0] + s.wsum[1] + s.wsum[2] + s.wsum[3];
}

// as k_gt_emit; a selected row also writes its four quality sums A C G T
__global__ void __launch_bounds__(256) k_gtw_emit(GtwAcc a, GtwAcc q, const TextPlanes* __restrict__ tpl, uint64_t tile0, uint64_t first,
                                                  uint64_t count, GtRule rule, const uint64_t* __restrict__ sel, uint64_t capacity,
                                                  uint64_t* __restrict__ pos, uint32_t* __restrict__ counts,
                                                  slamem_genotype* __restrict__ gts, uint32_t* __restrict__ qsums) {
    __shared__ GtTile s, sq;
    constexpr uint32_t per = kPileTile / 256u;
    __shared__ uint32_t wcnt[per * 4u];
    const uint64_t out0 = sel[blockIdx.x];
    if (sel[blockIdx.x + 1] == out0 || out0 >= capacity) return;  // (the whole workgroup: nothing selected, or no room left)
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile, end = first + count;  // (end <= n)
    gt_tile_stage(a.diff, a.tile, tpl, t, end, s);
    gt_tile_stage(q.diff, q.tile, tpl, t, end, sq);
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // (the output pointers live in vector registers: the kernel is at the limit of the scalar ones, and a store's address ends in a
    // vector register anyway)
    asm volatile("" : "+v"(qsums), "+v"(counts), "+v"(gts));
    uint32_t chosen = 0, below[per];
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        uint32_t c[6], qc[6];
        GtCall call;
        const bool on = gtw_tile_selected(a, q, base, j * 256u + threadIdx.x, lo, hi, s, sq, rule, c, qc, call);
        chosen |= (on ? 1u : 0u) << j;
        const unsigned long long b = __ballot(on);
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
        if (!((chosen >> j) & 1u) || o >= capacity) continue;
        const uint32_t at = j * 256u + threadIdx.x;
        uint32_t c[6], qc[6];
        GtCall call;
        (void)gtw_tile_selected(a, q, base, at, lo, hi, s, sq, rule, c, qc, call);  // (it is selected: the pass above said so)
        pos[o] = base + at;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) counts[o * 6u + k] = c[k];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) qsums[o * 4u + k] = qc[k];
        gt_store(gts + o, call, rule.ploidy, s.code[at]);
    }
}

// a lane per event: ao = fwd + rev against the depth of its anchor row
__global__ void __launch_bounds__(256) k_gt_events(const slamem_event* __restrict__ ev, const uint32_t* __restrict__ rows, uint64_t m,
                                                   GtRule rule, slamem_genotype* __restrict__ gts, uint8_t* __restrict__ called) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint32_t* c = rows + i * 6u;
    const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4], ao = (uint64_t)ev[i].fwd + ev[i].rev;
    GtCall call;
    uint64_t qual;
    const bool variant = gt_event(ao, d, rule, call, qual);
    gt_store(gts + i, call, rule.ploidy, 0u);
    called[i] = d >= rule.min_depth && variant && qual >= rule.min_qual ? 1u : 0u;
}

}  // namespace

// the parameters as every variant refuses them; `fn` names the caller in the message (gt_shared.h: cons_filter.hip checks with it too)
int gt_check(const char* fn, const slamem_gt_params* p, GtRule& rule) {
    constexpr uint32_t kMaxCost = 1u << 20;
    if (p->ploidy != 1u && p->ploidy != 2u) { set_error("%s: the ploidy is 1 or 2, not %u", fn, p->ploidy); return SLAMEM_ERR_ARG; }
    if (p->het_cost == 0u || p->err_cost == 0u || p->match_cost > kMaxCost || p->het_cost > kMaxCost || p->err_cost > kMaxCost) {
        set_error("%s: the costs of a letter are at most 2^20, and those under a heterozygous genotype and under one without the "
                  "letter at least 1; they are %u, %u, %u", fn, p->match_cost, p->het_cost, p->err_cost);
        return SLAMEM_ERR_ARG;
    }
    if (p->het_prior > kMaxCost) { set_error("%s: the prior cost per non-reference allele is at most 2^20, not %u", fn, p->het_prior); return SLAMEM_ERR_ARG; }
    if (p->min_depth == 0u || p->min_depth >= 0x80000000u) {
        set_error("%s: the least depth is 1 to 2^31 - 1, not %u", fn, p->min_depth);
        return SLAMEM_ERR_ARG;
    }
    if (p->min_qual > 999u) { set_error("%s: the least quality is 0 to 999 Phred, not %u", fn, p->min_qual); return SLAMEM_ERR_ARG; }
    rule = GtRule{p->ploidy, p->match_cost, p->het_cost, p->err_cost, p->het_prior, p->min_depth, p->min_qual * 1000u};
    return SLAMEM_OK;
}

namespace {

int gt_check_range(const char* fn, const slamem_pileup* pile, uint64_t first, uint64_t count) {
    if (first > pile->n || count > pile->n - first) {
        set_error("%s: rows %llu .. %llu + %llu lie outside the text's %u", fn, (unsigned long long)first, (unsigned long long)first,
                  (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    return SLAMEM_OK;
}

}  // namespace

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_pileup_genotypes_device(slamem_pileup* pile, uint64_t first, uint64_t count, const slamem_gt_params* params, uint64_t capacity,
                                   uint64_t* pos_dev, uint32_t* counts_dev, slamem_genotype* gts_dev, uint64_t* total_out, void* stream) {
    if (!pile || !params || !total_out || (capacity && (!pos_dev || !counts_dev || !gts_dev))) {
        set_error("slamem_pileup_genotypes_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    GtRule rule;
    SLAMEM_TRY(gt_check_range("slamem_pileup_genotypes_device", pile, first, count));
    SLAMEM_TRY(gt_check("slamem_pileup_genotypes_device", params, rule));
    if (count == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t end = first + count, tiles = (end + kPileTile - 1) / kPileTile, tile0 = first / kPileTile, mine = tiles - tile0;
    SLAMEM_TRY(pile_tile_prefix(pile, end, st));
    const TextPlanes* tpl = pile->idx->view.tpl;
    hipLaunchKernelGGL(k_gt_count, dim3((unsigned)mine), dim3(256), 0, st, (const int32_t*)pile->diff, (const uint32_t*)pile->cnt,
                       (const uint32_t*)pile->tile, tpl, tile0, first, count, rule, pile->sel);
    SLAMEM_HIP(hipGetLastError());
    SLAMEM_TRY(pile_scan_counts(pile->sel, mine, st));  // (mine + 1 <= n / kPileTile + 2 words)
    if (capacity) {  // rows behind `capacity` are dropped on the device, so the pass may run before the total is known
        hipLaunchKernelGGL(k_gt_emit, dim3((unsigned)mine), dim3(256), 0, st, (const int32_t*)pile->diff, (const uint32_t*)pile->cnt,
                           (const uint32_t*)pile->tile, tpl, tile0, first, count, rule, (const uint64_t*)pile->sel, capacity, pos_dev,
                           counts_dev, gts_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    uint64_t total = 0;  // the call's one host round trip
    SLAMEM_HIP(hipMemcpyAsync(&total, pile->sel + mine, 8, hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipStreamSynchronize(st));
    *total_out = total;
    if (total > capacity) {
        set_error("slamem_pileup_genotypes_device: %llu rows are selected, the buffers hold %llu", (unsigned long long)total,
                  (unsigned long long)capacity);
        return SLAMEM_ERR_CAPACITY;
    }
    return SLAMEM_OK;
}

int slamem_pileup_genotypes_host(slamem_pileup* pile, uint64_t first, uint64_t count, const slamem_gt_params* params, uint64_t capacity,
                                 uint64_t* pos, uint32_t* counts, slamem_genotype* gts, uint64_t* total_out) {
    if (!pile || !params || !total_out || (capacity && (!pos || !counts || !gts))) {
        set_error("slamem_pileup_genotypes_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    GtRule rule;
    SLAMEM_TRY(gt_check_range("slamem_pileup_genotypes_host", pile, first, count));
    SLAMEM_TRY(gt_check("slamem_pileup_genotypes_host", params, rule));
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    const uint64_t room = capacity < count ? capacity : count;  // (a range selects at most its rows)
    DevBuf<char> d;
    if (room) SLAMEM_TRY(d.reserve(room * (32 + sizeof(slamem_genotype))));
    char* b = d.get();
    uint64_t* pd = reinterpret_cast<uint64_t*>(b);
    uint32_t* cd = reinterpret_cast<uint32_t*>(b + room * 8);
    slamem_genotype* gd = reinterpret_cast<slamem_genotype*>(b + room * 32);
    const int rc = slamem_pileup_genotypes_device(pile, first, count, params, room, pd, cd, gd, total_out, nullptr);
    if (rc != SLAMEM_OK && rc != SLAMEM_ERR_CAPACITY) return rc;
    // (the rows that fitted go back with SLAMEM_ERR_CAPACITY too; the call's code comes before a failed copy's)
    const uint64_t got = *total_out < room ? *total_out : room;
    hipError_t e = hipSuccess;
    if (got) e = hipMemcpy(pos, pd, got * 8, hipMemcpyDeviceToHost);
    if (got && e == hipSuccess) e = hipMemcpy(counts, cd, got * 24, hipMemcpyDeviceToHost);
    if (got && e == hipSuccess) e = hipMemcpy(gts, gd, got * sizeof(slamem_genotype), hipMemcpyDeviceToHost);
    if (rc == SLAMEM_OK && e != hipSuccess) return hip_fail(e, "hipMemcpy", __FILE__, __LINE__);
    return rc;
}

int slamem_pileup_genotypes_weighted_device(slamem_pileup* pile, uint64_t first, uint64_t count, const slamem_gt_params* params,
                                            uint64_t capacity, uint64_t* pos_dev, uint32_t* counts_dev, slamem_genotype* gts_dev,
                                            uint32_t* qsums_dev, uint64_t* total_out, void* stream) {
    if (!pile || !params || !total_out || (capacity && (!pos_dev || !counts_dev || !gts_dev || !qsums_dev))) {
        set_error("slamem_pileup_genotypes_weighted_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    GtRule rule;
    SLAMEM_TRY(gt_check_range("slamem_pileup_genotypes_weighted_device", pile, first, count));
    SLAMEM_TRY(gt_check("slamem_pileup_genotypes_weighted_device", params, rule));
    if (!pile->qual) {
        set_error("slamem_pileup_genotypes_weighted_device: the quality sums of this accumulator are not enabled (slamem_pileup_enable_quals)");
        return SLAMEM_ERR_ARG;
    }
    if (count == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t end = first + count, tiles = (end + kPileTile - 1) / kPileTile, tile0 = first / kPileTile, mine = tiles - tile0;
    SLAMEM_TRY(pile_tile_prefix(pile, end, st));
    SLAMEM_TRY(pile_tile_prefix(pile->qual, end, st));
    const TextPlanes* tpl = pile->idx->view.tpl;
    const GtwAcc a{pile->diff, pile->cnt, pile->tile}, q{pile->qual->diff, pile->qual->cnt, pile->qual->tile};
    hipLaunchKernelGGL(k_gtw_count, dim3((unsigned)mine), dim3(256), 0, st, a, q, tpl, tile0, first, count, rule, pile->sel);
    SLAMEM_HIP(hipGetLastError());
    SLAMEM_TRY(pile_scan_counts(pile->sel, mine, st));  // (mine + 1 <= n / kPileTile + 2 words)
    if (capacity) {  // rows behind `capacity` are dropped on the device, so the pass may run before the total is known
        hipLaunchKernelGGL(k_gtw_emit, dim3((unsigned)mine), dim3(256), 0, st, a, q, tpl, tile0, first, count, rule,
                           (const uint64_t*)pile->sel, capacity, pos_dev, counts_dev, gts_dev, qsums_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    uint64_t total = 0;  // the call's one host round trip
    SLAMEM_HIP(hipMemcpyAsync(&total, pile->sel + mine, 8, hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipStreamSynchronize(st));
    *total_out = total;
    if (total > capacity) {
        set_error("slamem_pileup_genotypes_weighted_device: %llu rows are selected, the buffers hold %llu", (unsigned long long)total,
                  (unsigned long long)capacity);
        return SLAMEM_ERR_CAPACITY;
    }
    return SLAMEM_OK;
}

int slamem_pileup_genotypes_weighted_host(slamem_pileup* pile, uint64_t first, uint64_t count, const slamem_gt_params* params,
                                          uint64_t capacity, uint64_t* pos, uint32_t* counts, slamem_genotype* gts, uint32_t* qsums,
                                          uint64_t* total_out) {
    if (!pile || !params || !total_out || (capacity && (!pos || !counts || !gts || !qsums))) {
        set_error("slamem_pileup_genotypes_weighted_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    GtRule rule;
    SLAMEM_TRY(gt_check_range("slamem_pileup_genotypes_weighted_host", pile, first, count));
    SLAMEM_TRY(gt_check("slamem_pileup_genotypes_weighted_host", params, rule));
    if (!pile->qual) {
        set_error("slamem_pileup_genotypes_weighted_host: the quality sums of this accumulator are not enabled (slamem_pileup_enable_quals)");
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the tables that are read)
    const uint64_t room = capacity < count ? capacity : count;  // (a range selects at most its rows)
    // per row of room: the position (8 bytes), the counters (24), the quality sums (16), the genotype (56), in this order
    DevBuf<char> d;
    if (room) SLAMEM_TRY(d.reserve(room * (48 + sizeof(slamem_genotype))));
    char* b = d.get();
    uint64_t* pd = reinterpret_cast<uint64_t*>(b);
    uint32_t* cd = reinterpret_cast<uint32_t*>(b + room * 8);
    uint32_t* qd = reinterpret_cast<uint32_t*>(b + room * 32);
    slamem_genotype* gd = reinterpret_cast<slamem_genotype*>(b + room * 48);
    const int rc = slamem_pileup_genotypes_weighted_device(pile, first, count, params, room, pd, cd, gd, qd, total_out, nullptr);
    if (rc != SLAMEM_OK && rc != SLAMEM_ERR_CAPACITY) return rc;
    // (the rows that fitted go back with SLAMEM_ERR_CAPACITY too; the call's code comes before a failed copy's)
    const uint64_t got = *total_out < room ? *total_out : room;
    hipError_t e = hipSuccess;
    if (got) e = hipMemcpy(pos, pd, got * 8, hipMemcpyDeviceToHost);
    if (got && e == hipSuccess) e = hipMemcpy(counts, cd, got * 24, hipMemcpyDeviceToHost);
    if (got && e == hipSuccess) e = hipMemcpy(qsums, qd, got * 16, hipMemcpyDeviceToHost);
    if (got && e == hipSuccess) e = hipMemcpy(gts, gd, got * sizeof(slamem_genotype), hipMemcpyDeviceToHost);
    if (rc == SLAMEM_OK && e != hipSuccess) return hip_fail(e, "hipMemcpy", __FILE__, __LINE__);
    return rc;
}

int slamem_pileup_genotype_events_device(slamem_pileup* pile, const slamem_event* events_dev, const uint32_t* anchor_rows_dev, uint64_t m,
                                         const slamem_gt_params* params, slamem_genotype* gts_dev, uint8_t* called_dev, void* stream) {
    if (!pile || !params || (m && (!events_dev || !anchor_rows_dev || !gts_dev || !called_dev))) {
        set_error("slamem_pileup_genotype_events_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    GtRule rule;
    SLAMEM_TRY(gt_check("slamem_pileup_genotype_events_device", params, rule));
    if (m == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipLaunchKernelGGL(k_gt_events, dim3(pile_grid(m, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), events_dev, anchor_rows_dev, m,
                       rule, gts_dev, called_dev);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int slamem_pileup_genotype_events_host(slamem_pileup* pile, const slamem_event* events, const uint64_t* anchors, uint64_t m,
                                       const slamem_gt_params* params, slamem_genotype* gts, uint8_t* called) {
    if (!pile || !params || (m && (!events || !anchors || !gts || !called))) {
        set_error("slamem_pileup_genotype_events_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    GtRule rule;
    SLAMEM_TRY(gt_check("slamem_pileup_genotype_events_host", params, rule));
    for (uint64_t i = 0; i < m; i++)
        if (anchors[i] >= pile->n) {
            set_error("slamem_pileup_genotype_events_host: anchor %llu (entry %llu) lies outside the text's %u", (unsigned long long)anchors[i],
                      (unsigned long long)i, pile->n);
            return SLAMEM_ERR_ARG;
        }
    if (m == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    // the events (32 bytes each), their anchors (8), the anchors' rows (24), the genotypes (56) and the bytes, in this order
    DevBuf<char> d;
    SLAMEM_TRY(d.reserve(m * (sizeof(slamem_event) + 8 + 24 + sizeof(slamem_genotype) + 1)));
    char* b = d.get();
    slamem_event* ed = reinterpret_cast<slamem_event*>(b);
    uint64_t* ad = reinterpret_cast<uint64_t*>(b + m * 32);
    uint32_t* rd = reinterpret_cast<uint32_t*>(b + m * 40);
    slamem_genotype* gd = reinterpret_cast<slamem_genotype*>(b + m * 64);
    uint8_t* cd = reinterpret_cast<uint8_t*>(b + m * (64 + sizeof(slamem_genotype)));
    SLAMEM_HIP(hipMemcpy(ed, events, m * sizeof(slamem_event), hipMemcpyHostToDevice));
    SLAMEM_HIP(hipMemcpy(ad, anchors, m * 8, hipMemcpyHostToDevice));
    SLAMEM_TRY(slamem_pileup_rows_at_device(pile, ad, m, rd, nullptr));
    SLAMEM_TRY(slamem_pileup_genotype_events_device(pile, ed, rd, m, params, gd, cd, nullptr));
    SLAMEM_HIP(hipMemcpy(gts, gd, m * sizeof(slamem_genotype), hipMemcpyDeviceToHost));
    SLAMEM_HIP(hipMemcpy(called, cd, m, hipMemcpyDeviceToHost));
    return SLAMEM_OK;
}

}  // extern "C"
