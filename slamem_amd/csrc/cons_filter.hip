// cons_filter.hip -- -cons: the consensus sequence of the mapped reads, one byte per emitted letter, from what the
// accumulator holds after a batch: the six counters per row (4.16) and the left-normalised indel events (4.18).  Row p emits, in
// this order: the letters of the best applied insertion in front of it; nothing more if an applied deletion covers it; else N for a
// letter that is none of A,C,G,T, the text's letter in lower case for an uncalled row, the plurality letter in upper case.
//   (slamem_pileup_events_device)   E: the events of [first - 127, first + count), sorted on the device (the read-out of 4.18 as it is)
//   k_cons_applied   a wave per event: the depth of its anchor row as k_pile_rows_at forms it, and "applied" as a byte per event
//   k_cons_mark      a lane per event: an applied deletion sets bit 5 of the flag byte of its rows, the head of a (pos, kind 1) run
//                    picks the run's best applied insertion, marks it (2) and puts its length in bits 0..4 of the row's flag byte
//   k_cons_count     a workgroup per tile of kPileTile rows: the counters from diff, tile and cnt as the read-outs rebuild them, each
//                    row's emission, the tile's bytes to sel[], the five statistics
//   (pile_scan_counts)              the tiles' offsets and the total
//   k_cons_scatter   a workgroup per tile: the emissions again, a scan of their lengths in row order, the bytes below `capacity`,
//                    and offs[] of the bounds that lie in the tile
//   k_cons_bounds_edge  offs[] of a bound at first + count (the total) or outside the range (UINT64_MAX)
// A row finds its insertion's letters by a binary search for (p, kind 1) in E and a walk along the run to the marked event.
// Nothing of the accumulator or of the event table is written: the flag bytes, E and the marks are scratch of the read-out.
//
// -cons -gt: the same passes with every decision made by the likelihood of -gt (gt_shared.h).  k_cons_applied,
// cons_letter, cons_tile_rows, k_cons_count and k_cons_scatter are templates on the mode: kConsPlur is the code above,
// kConsGt calls a row by gt_snv -- lower case unless its GQ reaches the least one, the IUPAC code of a heterozygous genotype -- and
// applies an event whose gt_event genotype is homozygous for it with that GQ, kConsGtw does the same with the row's quality sums:
// the tile of the quality accumulator is staged beside the counts' (a second match[] in the tile), as k_gtw_count does it.  The
// genotype's scores stay in registers: compile-time indices only, as gt_shared.h asks.  Three more statistics: rows with an
// IUPAC code, rows uncalled for GQ alone, heterozygous events that were not applied.
#include "buffers.h"
#include "gt_shared.h"
#include "pile_shared.h"
#include "prims.h"

#include <new>
#include <type_traits>

namespace slamem {

struct ConsScratch {
    uint8_t* flag;              // a byte per row of the text (+ 8): bits 0..4 the inserted letters in front of it, bit 5 deleted
    unsigned long long* stats;  // 8 counters (the plurality read-out uses 5)
    slamem_event* ev;           // E, ev_cap records (events enabled)
    uint8_t* app;               // a byte per event: 0 not applied, 1 applied, 2 applied and its row's best insertion
    uint64_t ev_cap;
};

namespace {

constexpr uint32_t kConsDel = 32u, kConsLen = 31u;
constexpr uint64_t kConsReach = 127;  // a deletion covers rows up to this far behind its pos - 1 ... pos + 126
constexpr uint64_t kConsEvents0 = 4096;

// the mode of a read-out: plurality (4.19), the genotype of the counts, the genotype of the counts and the quality sums (4.32)
constexpr uint32_t kConsPlur = 0, kConsGt = 1, kConsGtw = 2;

// what decides a row, a kernel argument.  Plurality: the least depth.
struct ConsPlurRule {
    uint32_t min_depth;
};
// Genotype: the costs of the rows (rule.min_depth is the least depth, rule.min_qual is not looked at), the least GQ in
// milli-Phred, and (kConsGtw) the quality accumulator
struct ConsGtRule {
    GtRule rule;
    uint32_t min_gq;
    const int32_t* qdiff;
    const uint32_t* qcnt;
    const uint32_t* qtile;
};
template <uint32_t kMode>
using ConsRule = std::conditional_t<kMode == kConsPlur, ConsPlurRule, ConsGtRule>;
// what decides an event.  Genotype: the costs of the events, the least GQ, and the range whose heterozygous events are counted
struct ConsGtEvRule {
    GtRule rule;
    uint32_t min_gq;
    uint64_t first, end;
    unsigned long long* het;  // stats + 7
};
template <uint32_t kMode>
using ConsEvRule = std::conditional_t<kMode == kConsPlur, ConsPlurRule, ConsGtEvRule>;
// the statistics a tile's rows add to: 5, and with a genotype rows with an IUPAC code and rows uncalled for GQ alone
template <uint32_t kMode>
constexpr uint32_t kConsRowStats = kMode == kConsPlur ? 5u : 7u;

// the text's letter at x (x < n): A 0, C 1, G 2, T 3; anything else 4
__device__ __forceinline__ uint32_t cons_text(const TextPlanes* __restrict__ tpl, uint64_t x) {
    const TextPlanes* u = tpl + (x >> 6);
    const uint32_t bit = (uint32_t)(x & 63u);
    if ((u->nm >> bit) & 1ull) return 4u;
    return (uint32_t)((u->p0 >> bit) & 1ull) | ((uint32_t)((u->p1 >> bit) & 1ull) << 1);
}

// flag[x] |= v, the bytes of a word being set by several lanes: an atomic OR on the aligned word (little endian)
__device__ __forceinline__ void cons_flag_or(uint8_t* flag, uint64_t x, uint32_t v) {
    atomicOr(reinterpret_cast<unsigned int*>(flag) + (x >> 2), v << (8u * (uint32_t)(x & 3u)));
}

// a wave per event: app[i] = is the event applied?  The anchor row a is pos - 1 if that row holds one of A,C,G,T, else pos; its
// depth d is the sum of diff from its tile's first entry to a (32 entries a lane) on top of tile[] and cnt[a], as k_pile_rows_at.
// With a genotype lane 0 runs gt_event in the place of 2 * obs > d: applied iff the best genotype is homozygous for the event and
// its GQ reaches the least one; an event of [first, end) whose best genotype is heterozygous with that GQ is counted.
template <uint32_t kMode>
__global__ void __launch_bounds__(256) k_cons_applied(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                      const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t n,
                                                      const slamem_event* __restrict__ ev, uint64_t m, ConsEvRule<kMode> p,
                                                      uint8_t* __restrict__ app) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= m) return;  // (the whole wave)
    const uint64_t pos = ev[i].pos;
    if (pos >= n) {
        if (lane == 0u) app[i] = 0;
        return;
    }
    const uint64_t a = pos >= 1u && cons_text(tpl, pos - 1u) < 4u ? pos - 1u : pos;
    const uint32_t letter = cons_text(tpl, a);
    const uint64_t t = a / kPileTile, base = t * kPileTile;
    constexpr uint32_t per = kPileTile / 64u;
    uint32_t v = 0;
#pragma unroll 8
    for (uint32_t j = 0; j < per; j++) {
        const uint64_t x = base + (uint64_t)lane * per + j;
        if (x <= a) v += (uint32_t)diff[x];
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v += __shfl_xor(v, d, 64);
    if (lane != 0u) return;
    uint64_t d = 0;
    for (uint32_t k = 0; k < 5u; k++) d += (uint32_t)(cnt[a * 6u + k] + (k == letter ? tile[t] + v : 0u));
    const uint64_t obs = (uint64_t)ev[i].fwd + ev[i].rev;
    if constexpr (kMode == kConsPlur) {
        app[i] = letter < 4u && d >= p.min_depth && 2u * obs > d ? 1 : 0;
    } else {
        GtCall call;
        uint64_t qual;
        (void)gt_event(obs, d, p.rule, call, qual);
        const bool sure = call.gq >= p.min_gq;  // (gq saturates at 2^32 - 1, min_gq is below 10^6: the comparison of the 64-bit value)
        app[i] = letter < 4u && d >= p.rule.min_depth && sure && call.a == 1u && call.b == 1u ? 1 : 0;
        if (sure && call.a != call.b && pos >= p.first && pos < p.end) atomicAdd(p.het, 1ull);
    }
}

// a lane per event.  Rows outside [first, end) have no flag byte in this call.
__global__ void __launch_bounds__(256) k_cons_mark(const slamem_event* __restrict__ ev, uint64_t m, uint8_t* __restrict__ app,
                                                   uint8_t* __restrict__ flag, uint64_t first, uint64_t end) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint64_t pos = ev[i].pos;
    if (ev[i].kind == 0u) {
        if (!app[i]) return;
        const uint64_t lo = pos > first ? pos : first, stop = pos + ev[i].len < end ? pos + ev[i].len : end;
        for (uint64_t x = lo; x < stop; x++) cons_flag_or(flag, x, kConsDel);
        return;
    }
    if (i > 0u && ev[i - 1u].pos == pos && ev[i - 1u].kind == 1u) return;  // (not the head of its run)
    if (pos < first || pos >= end) return;
    uint64_t best = m, best_obs = 0;
    for (uint64_t j = i; j < m && ev[j].pos == pos && ev[j].kind == 1u; j++) {  // (the marks of this run are this lane's alone)
        const uint64_t obs = (uint64_t)ev[j].fwd + ev[j].rev;
        if (app[j] && obs > best_obs) { best = j; best_obs = obs; }
    }
    if (best == m) return;
    app[best] = 2;
    cons_flag_or(flag, pos, ev[best].len & kConsLen);
}

// the sums of k values over the workgroup's 256 lanes, in every lane; lds: 4 * K words
template <uint32_t K>
__device__ __forceinline__ void cons_block_sums(uint32_t (&v)[K], uint32_t* lds) {
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
#pragma unroll
        for (uint32_t d = 32; d >= 1u; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
        if ((threadIdx.x & 63u) == 0u) lds[k * 4u + (threadIdx.x >> 6)] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < K; k++) v[k] = lds[k * 4u] + lds[k * 4u + 1u] + lds[k * 4u + 2u] + lds[k * 4u + 3u];
    __syncthreads();
}

struct ConsNoQual {};
struct ConsQual {
    uint32_t qmatch[kPileTile];  // the sum of the quality accumulator's diff[0 .. p]
};
template <uint32_t kMode>
struct ConsTile : std::conditional_t<kMode == kConsGtw, ConsQual, ConsNoQual> {
    uint32_t match[kPileTile];  // the sum of diff[0 .. p]; the scatter pass keeps the rows' byte offsets here afterwards
    uint8_t code[kPileTile];    // the text's letter, 4: none of A,C,G,T or a row at or behind `end`
    uint8_t elen[kPileTile];    // bytes the row emits: 0 .. 32
    uint8_t elet[kPileTile];    // its own letter, 0: none (deleted, or outside the range)
    uint32_t wsum[4u * (kConsRowStats<kMode> + 1u)];
};

// tile t of a read-out that ends at `end` (<= n): match and code of its rows, as pile_filter.hip stages them for the other
// read-outs (a lane takes kPileTile / 256 consecutive entries of diff).  code == nullptr (the quality accumulator's tile, staged
// behind the counts'): the sums alone.  Ends with a barrier.
__device__ __forceinline__ void cons_tile_stage(const int32_t* __restrict__ diff, const uint32_t* __restrict__ tile,
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
        if (code) code[at] = (uint8_t)(x < end ? cons_text(tpl, x) : 4u);
    }
    __syncthreads();
}

// the byte of a genotype (a, b): the letter of a homozygous one, else the IUPAC code of the two -- AC M, AG R, AT W, CG S, CT Y,
// GT K -- found by the set of the two letters as four bits (a shift of a constant, no table in memory)
__device__ __forceinline__ uint32_t cons_iupac(uint32_t a, uint32_t b) {
    const uint32_t set = (1u << a) | (1u << b);
    // bytes, the lowest first:    . A C M G R S .                T W Y . K . . .
    const uint64_t low = 0x005352474D434100ull, high = 0x0000004B00595754ull;
    return (uint32_t)(((set < 8u ? low : high) >> (8u * (set & 7u))) & 0xFFull);
}

// the letter of a row that no deletion covers (rules 3 to 5); st[0] uncalled, st[1] called and not the text's letter.  With a
// genotype: st[5] an IUPAC code, st[6] uncalled although deep enough and with letters (its GQ is too low); qmatch (kConsGtw) is
// the row's entry of the quality tile.
template <uint32_t kMode>
__device__ __forceinline__ uint32_t cons_letter(const uint32_t* __restrict__ cnt, uint64_t x, uint32_t letter, uint32_t match,
                                                uint32_t qmatch, const ConsRule<kMode>& p, uint32_t* st) {
    if (letter >= 4u) return 'N';
    const uint2* r = reinterpret_cast<const uint2*>(cnt + x * 6u);  // (24 bytes a row: 8-byte aligned)
    const uint2 a = r[0], b = r[1];
    uint32_t c[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) c[k] += letter == k ? match : 0u;
    const uint64_t acgt = (uint64_t)c[0] + c[1] + c[2] + c[3], d = acgt + cnt[x * 6u + 4u];
    const uint32_t own = (0x54474341u >> (8u * letter)) & 0xFFu;
    if constexpr (kMode == kConsPlur) {
        if (d < p.min_depth || acgt == 0u) { st[0]++; return own | 0x20u; }
        uint32_t top = c[0], who = 0;
#pragma unroll
        for (uint32_t k = 1; k < 4u; k++)
            if (c[k] > top) { top = c[k]; who = k; }
        if (c[letter] == top) who = letter;
        if (who != letter) st[1]++;
        return (0x54474341u >> (8u * who)) & 0xFFu;
    } else {
        if (d < p.rule.min_depth || acgt == 0u) { st[0]++; return own | 0x20u; }
        GtCall call;
        uint64_t qual;
        if constexpr (kMode == kConsGtw) {
            const uint2* qr = reinterpret_cast<const uint2*>(p.qcnt + x * 6u);
            const uint2 qa = qr[0], qb = qr[1];
            uint32_t qs[4] = {qa.x, qa.y, qb.x, qb.y};
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) qs[k] += letter == k ? qmatch : 0u;
            (void)gt_snv<true>(c, qs, letter, p.rule, call, qual);
        } else {
            (void)gt_snv<false>(c, c, letter, p.rule, call, qual);
        }
        // (gq saturates at 2^32 - 1 and min_gq is below 10^6: the comparison of the 64-bit value)
        if (call.gq < p.min_gq) { st[0]++; st[6]++; return own | 0x20u; }
        const uint32_t byte = cons_iupac(call.a, call.b);
        if (call.a != call.b) st[5]++;
        if (byte != own) st[1]++;
        return byte;
    }
}

// the emissions of tile t's rows inside [lo, hi) into s.elen and s.elet; rows are taken 256 apart, so a wave reads 64 neighbouring
// rows.  st: this lane's share of the five (seven) statistics.  Ends with a barrier.
template <uint32_t kMode>
__device__ __forceinline__ void cons_tile_rows(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                               const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl,
                                               const uint8_t* __restrict__ flag, uint64_t t, uint64_t first, uint64_t end,
                                               const ConsRule<kMode>& p, ConsTile<kMode>& s, uint32_t* st) {
    cons_tile_stage(diff, tile, tpl, t, end, s.match, s.code, s.wsum);
    if constexpr (kMode == kConsGtw) cons_tile_stage(p.qdiff, p.qtile, tpl, t, end, s.qmatch, nullptr, s.wsum);
    const uint64_t base = t * kPileTile;
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
#pragma unroll
    for (uint32_t j = 0; j < kPileTile / 256u; j++) {
        const uint32_t at = j * 256u + threadIdx.x;
        const uint64_t x = base + at;
        uint32_t len = 0, let = 0;
        if (x >= lo && x < hi) {
            const uint32_t f = flag[x];
            len = f & kConsLen;
            if (len) { st[3]++; st[4] += len; }
            if (f & kConsDel) {
                st[2]++;
            } else {
                uint32_t qmatch = 0;
                if constexpr (kMode == kConsGtw) qmatch = s.qmatch[at];
                let = cons_letter<kMode>(cnt, x, s.code[at], s.match[at], qmatch, p, st);
                len++;
            }
        }
        s.elen[at] = (uint8_t)len;
        s.elet[at] = (uint8_t)let;
    }
    __syncthreads();
}

// a workgroup per tile of rows: sel[blockIdx.x] = the bytes its rows inside [first, end) emit; stats += its share
template <uint32_t kMode>
__global__ void __launch_bounds__(256) k_cons_count(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                    const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl,
                                                    const uint8_t* __restrict__ flag, uint64_t tile0, uint64_t first, uint64_t end,
                                                    ConsRule<kMode> p, uint64_t* __restrict__ sel, unsigned long long* __restrict__ stats) {
    __shared__ ConsTile<kMode> s;
    constexpr uint32_t K = kConsRowStats<kMode>;
    uint32_t v[K + 1u];
#pragma unroll
    for (uint32_t k = 0; k <= K; k++) v[k] = 0;
    cons_tile_rows<kMode>(diff, cnt, tile, tpl, flag, tile0 + blockIdx.x, first, end, p, s, v);
    for (uint32_t j = 0; j < kPileTile / 256u; j++) v[K] += s.elen[j * 256u + threadIdx.x];  // (the rows this lane wrote)
    cons_block_sums<K + 1u>(v, s.wsum);
    if (threadIdx.x == 0) sel[blockIdx.x] = v[K];
    // (lane k adds statistic k: v[] holds the same sums in every lane, and the choice by comparison keeps it in registers)
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) mine = threadIdx.x == k ? v[k] : mine;
    if (threadIdx.x < K && mine != 0u) atomicAdd(&stats[threadIdx.x], (unsigned long long)mine);
}

// a workgroup per tile: the bytes of its rows at sel[blockIdx.x] + the bytes of the tile's rows in front (a lane scans 8
// consecutive rows, the lanes' sums inside the wave, the waves' through LDS), bytes at or behind `capacity` dropped; and
// offs[j] of every bound inside the tile's part of [first, end)
template <uint32_t kMode>
__global__ void __launch_bounds__(256) k_cons_scatter(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                      const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl,
                                                      const uint8_t* __restrict__ flag, uint64_t tile0, uint64_t first, uint64_t end,
                                                      ConsRule<kMode> p, const uint64_t* __restrict__ sel,
                                                      const slamem_event* __restrict__ ev, uint64_t nev, const uint8_t* __restrict__ app,
                                                      uint64_t capacity, uint8_t* __restrict__ out, const uint64_t* __restrict__ bounds,
                                                      uint64_t m, uint64_t* __restrict__ offs) {
    __shared__ ConsTile<kMode> s;
    const uint64_t out0 = sel[blockIdx.x];
    if (m == 0u && (sel[blockIdx.x + 1] == out0 || out0 >= capacity)) return;  // (the whole workgroup: no bytes, or no room left)
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile;
    uint32_t st[kConsRowStats<kMode>] = {};
    cons_tile_rows<kMode>(diff, cnt, tile, tpl, flag, t, first, end, p, s, st);
    constexpr uint32_t per = kPileTile / 256u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, at0 = threadIdx.x * per;
    uint32_t run = 0;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) run += s.elen[at0 + j];
    uint32_t inc = run;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63u) s.wsum[wave] = inc;
    __syncthreads();  // (every lane has read its match in cons_tile_rows: the array is free)
    uint32_t before = inc - run;
    for (uint32_t w = 0; w < wave; w++) before += s.wsum[w];
    for (uint32_t j = 0; j < per; j++) {
        const uint32_t at = at0 + j, len = s.elen[at], let = s.elet[at];
        s.match[at] = before;
        uint64_t o = out0 + before;
        before += len;
        const uint32_t ins = len - (let ? 1u : 0u);
        if (ins && o < capacity) {
            // the run of (p, kind 1) in E, and in it the marked event
            const uint64_t p = base + at;
            uint64_t a = 0, b = nev;
            while (a < b) {
                const uint64_t mid = a + ((b - a) >> 1);
                if (ev[mid].pos < p || (ev[mid].pos == p && ev[mid].kind == 0u)) a = mid + 1u; else b = mid;
            }
            while (a < nev && ev[a].pos == p && app[a] != 2) a++;
            const uint64_t letters = a < nev && ev[a].pos == p ? ev[a].letters : 0ull;
            for (uint32_t k = 0; k < ins; k++)
                if (o + k < capacity) out[o + k] = (uint8_t)((0x54474341u >> (8u * (uint32_t)((letters >> (2u * (ins - 1u - k))) & 3ull))) & 0xFFu);
        }
        o += ins;
        if (let && o < capacity) out[o] = (uint8_t)let;
    }
    if (m == 0u) return;
    __syncthreads();
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    for (uint64_t j = threadIdx.x; j < m; j += 256u) {
        const uint64_t b = bounds[j];
        if (b >= lo && b < hi) offs[j] = out0 + s.match[b - base];
    }
}

// a lane per bound: one at `end` gets the total (0 without one), one outside [first, end] UINT64_MAX
__global__ void __launch_bounds__(256) k_cons_bounds_edge(const uint64_t* __restrict__ bounds, uint64_t m, uint64_t first, uint64_t end,
                                                          const uint64_t* __restrict__ total, uint64_t* __restrict__ offs) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= m) return;
    const uint64_t b = bounds[j];
    if (b < first || b > end) offs[j] = ~0ull;
    else if (b == end) offs[j] = total ? *total : 0ull;
}

int cons_scratch(slamem_pileup* pile) {
    if (pile->cons) return SLAMEM_OK;
    ConsScratch* c = new (std::nothrow) ConsScratch();
    if (!c) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    *c = ConsScratch{};
    pile->cons = c;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->flag), (uint64_t)pile->n + 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->stats), 8 * sizeof(unsigned long long));
    if (e != hipSuccess) {
        cons_free(pile);
        return hip_fail(e, "slamem_pileup_consensus_device", __FILE__, __LINE__);
    }
    return SLAMEM_OK;
}

// room for `cap` events and their marks (what is there goes: the device is idle when hipFree returns)
int cons_events_room(ConsScratch* c, uint64_t cap) {
    if (cap <= c->ev_cap) return SLAMEM_OK;
    if (c->ev) (void)hipFree(c->ev);
    if (c->app) (void)hipFree(c->app);
    c->ev = nullptr; c->app = nullptr; c->ev_cap = 0;
    SLAMEM_HIP(hipMalloc(reinterpret_cast<void**>(&c->ev), cap * sizeof(slamem_event)));
    SLAMEM_HIP(hipMalloc(reinterpret_cast<void**>(&c->app), cap));
    c->ev_cap = cap;
    return SLAMEM_OK;
}

// the read-out of rows [first, first + count) in one mode, its arguments checked: rowp decides the rows and evp the events
// (first, end and het of a genotype's are set here); stats_out has 5 entries (with a genotype 8), `fn` names the caller
template <uint32_t kMode>
int cons_readout(const char* fn, slamem_pileup* pile, uint64_t first, uint64_t count, const ConsRule<kMode>& rowp, ConsEvRule<kMode> evp,
                 uint64_t capacity, uint8_t* out_dev, const uint64_t* bounds_dev, uint64_t m, uint64_t* offs_dev, uint64_t* stats_out,
                 uint64_t* total_out, void* stream) {
    constexpr uint32_t K = kMode == kConsPlur ? 5u : 8u;
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t end = first + count;
    if (count == 0) {  // no row, no byte: every bound inside the range is `first`
        if (m) {
            hipLaunchKernelGGL(k_cons_bounds_edge, dim3(pile_grid(m, 256)), dim3(256), 0, st, bounds_dev, m, first, end,
                               (const uint64_t*)nullptr, offs_dev);
            SLAMEM_HIP(hipGetLastError());
        }
        return SLAMEM_OK;
    }
    int rc = cons_scratch(pile);
    if (rc != SLAMEM_OK) return rc;
    ConsScratch* c = pile->cons;
    // E: a deletion that covers a row of the range starts at most kConsReach - 1 rows in front of it
    uint64_t nev = 0;
    if (pile->ev) {
        const uint64_t elo = first > kConsReach ? first - kConsReach : 0;
        uint64_t skipped[3];
        rc = cons_events_room(c, kConsEvents0);
        if (rc != SLAMEM_OK) return rc;
        rc = slamem_pileup_events_device(pile, elo, end - elo, 1u, c->ev_cap, c->ev, skipped, &nev, stream);
        if (rc == SLAMEM_ERR_CAPACITY) {  // (more events than any call before this one met: once more with the need)
            rc = cons_events_room(c, nev);
            if (rc != SLAMEM_OK) return rc;
            rc = slamem_pileup_events_device(pile, elo, end - elo, 1u, c->ev_cap, c->ev, skipped, &nev, stream);
        }
        if (rc != SLAMEM_OK) return rc;
    }
    const uint64_t tiles = (end + kPileTile - 1) / kPileTile, tile0 = first / kPileTile, mine = tiles - tile0;
    rc = pile_tile_prefix(pile, end, st);
    if (rc != SLAMEM_OK) return rc;
    if constexpr (kMode == kConsGtw) {
        rc = pile_tile_prefix(pile->qual, end, st);
        if (rc != SLAMEM_OK) return rc;
    }
    const uint64_t w0 = first & ~3ull, w1 = (end + 3u) & ~3ull;  // (whole words: w1 <= n + 3)
    SLAMEM_HIP(hipMemsetAsync(c->flag + w0, 0, w1 - w0, st));
    SLAMEM_HIP(hipMemsetAsync(c->stats, 0, K * sizeof(unsigned long long), st));
    const TextPlanes* tpl = pile->idx->view.tpl;
    if (nev) {
        if constexpr (kMode != kConsPlur) { evp.first = first; evp.end = end; evp.het = c->stats + 7; }
        hipLaunchKernelGGL(k_cons_applied<kMode>, dim3(pile_grid(nev, 4)), dim3(256), 0, st, (const int32_t*)pile->diff,
                           (const uint32_t*)pile->cnt, (const uint32_t*)pile->tile, tpl, (uint64_t)pile->n, (const slamem_event*)c->ev, nev,
                           evp, c->app);
        SLAMEM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cons_mark, dim3(pile_grid(nev, 256)), dim3(256), 0, st, (const slamem_event*)c->ev, nev, c->app, c->flag, first,
                           end);
        SLAMEM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cons_count<kMode>, dim3((unsigned)mine), dim3(256), 0, st, (const int32_t*)pile->diff, (const uint32_t*)pile->cnt,
                       (const uint32_t*)pile->tile, tpl, (const uint8_t*)c->flag, tile0, first, end, rowp, pile->sel, c->stats);
    SLAMEM_HIP(hipGetLastError());
    rc = pile_scan_counts(pile->sel, mine, st);  // (mine + 1 <= n / kPileTile + 2 words)
    if (rc != SLAMEM_OK) return rc;
    if (capacity || m) {  // bytes behind `capacity` are dropped on the device, so the pass runs before the total is known
        hipLaunchKernelGGL(k_cons_scatter<kMode>, dim3((unsigned)mine), dim3(256), 0, st, (const int32_t*)pile->diff,
                           (const uint32_t*)pile->cnt, (const uint32_t*)pile->tile, tpl, (const uint8_t*)c->flag, tile0, first, end, rowp,
                           (const uint64_t*)pile->sel, (const slamem_event*)c->ev, nev, (const uint8_t*)c->app, capacity, out_dev,
                           bounds_dev, m, offs_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    if (m) {
        hipLaunchKernelGGL(k_cons_bounds_edge, dim3(pile_grid(m, 256)), dim3(256), 0, st, bounds_dev, m, first, end,
                           (const uint64_t*)(pile->sel + mine), offs_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    uint64_t total = 0;  // the round trip of the consensus itself (the events' read-out in front of it made its own)
    unsigned long long stats[K] = {};
    SLAMEM_HIP(hipMemcpyAsync(&total, pile->sel + mine, 8, hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipMemcpyAsync(stats, c->stats, sizeof(stats), hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipStreamSynchronize(st));
    *total_out = total;
    for (uint32_t k = 0; k < K; k++) stats_out[k] = stats[k];
    if (total > capacity) {
        set_error("%s: the consensus has %llu bytes, the buffer holds %llu", fn, (unsigned long long)total,
                  (unsigned long long)capacity);
        return SLAMEM_ERR_CAPACITY;
    }
    return SLAMEM_OK;
}

// the parameter block of the genotype consensus as both variants refuse it, and the rules of its kernels
int cons_gt_check(const char* fn, const slamem_pileup* pile, const slamem_cons_gt_params* p, ConsGtRule& rowp, ConsGtEvRule& evp) {
    slamem_gt_params row = p->row, ev = p->event;  // (their own min_depth and min_qual are not looked at)
    row.min_depth = ev.min_depth = p->min_depth;
    row.min_qual = ev.min_qual = 0;
    rowp = ConsGtRule{};
    evp = ConsGtEvRule{};
    SLAMEM_TRY(gt_check(fn, &row, rowp.rule));
    SLAMEM_TRY(gt_check(fn, &ev, evp.rule));
    if (p->min_gq > 999u) { set_error("%s: the least genotype quality is 0 to 999 Phred, not %u", fn, p->min_gq); return SLAMEM_ERR_ARG; }
    if (p->weighted > 1u) { set_error("%s: weighted is 0 or 1, not %u", fn, p->weighted); return SLAMEM_ERR_ARG; }
    if (p->weighted && !pile->qual) {
        set_error("%s: the quality sums of this accumulator are not enabled (slamem_pileup_enable_quals)", fn);
        return SLAMEM_ERR_ARG;
    }
    rowp.min_gq = evp.min_gq = p->min_gq * 1000u;
    if (p->weighted) { rowp.qdiff = pile->qual->diff; rowp.qcnt = pile->qual->cnt; rowp.qtile = pile->qual->tile; }
    return SLAMEM_OK;
}

int cons_check_range(const char* fn, const slamem_pileup* pile, uint64_t first, uint64_t count) {
    if (first > pile->n || count > pile->n - first) {
        set_error("%s: rows %llu .. %llu + %llu lie outside the text's %u", fn, (unsigned long long)first, (unsigned long long)first,
                  (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    return SLAMEM_OK;
}

// a device variant from and into host memory: `call` is the device variant with room for `room` bytes at the device's buffers
template <class Call>
int cons_host(const char* fn, slamem_pileup* pile, uint64_t first, uint64_t count, uint64_t capacity, uint8_t* out, const uint64_t* bounds,
              uint64_t m, uint64_t* offs, uint64_t* total_out, Call call) {
    if (first <= pile->n && count <= pile->n - first) {  // (a range outside the text: the device variant says so)
        for (uint64_t j = 0; j < m; j++) {
            if (bounds[j] < first || bounds[j] > first + count) {
                set_error("%s: bound %llu (entry %llu) lies outside rows %llu .. %llu", fn, (unsigned long long)bounds[j],
                          (unsigned long long)j, (unsigned long long)first, (unsigned long long)(first + count));
                return SLAMEM_ERR_ARG;
            }
        }
    }
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    const uint64_t most = count * 32u;  // (a row emits at most 31 inserted letters and its own)
    const uint64_t room = capacity < most ? capacity : most;
    DevBuf<uint8_t> d;
    DevBuf<uint64_t> bd;  // the m bounds, then their m offsets
    if (room) SLAMEM_TRY(d.reserve(room));
    if (m) SLAMEM_TRY(bd.reserve(m * 2));
    uint64_t* bdev = bd.get();
    if (m) SLAMEM_HIP(hipMemcpy(bdev, bounds, m * 8, hipMemcpyHostToDevice));
    const int rc = call(room, d.get(), bdev, m ? bdev + m : nullptr);
    if (rc != SLAMEM_OK && rc != SLAMEM_ERR_CAPACITY) return rc;
    // (what fitted goes back with SLAMEM_ERR_CAPACITY too; the call's code comes before a failed copy's)
    const uint64_t got = *total_out < room ? *total_out : room;
    hipError_t e = hipDeviceSynchronize();
    if (got && e == hipSuccess) e = hipMemcpy(out, d.get(), got, hipMemcpyDeviceToHost);
    if (m && e == hipSuccess) e = hipMemcpy(offs, bdev + m, m * 8, hipMemcpyDeviceToHost);
    if (rc == SLAMEM_OK && e != hipSuccess) return hip_fail(e, fn, __FILE__, __LINE__);
    return rc;
}

}  // namespace

void cons_free(slamem_pileup* pile) {
    ConsScratch* c = pile->cons;
    if (!c) return;
    if (c->flag) (void)hipFree(c->flag);
    if (c->stats) (void)hipFree(c->stats);
    if (c->ev) (void)hipFree(c->ev);
    if (c->app) (void)hipFree(c->app);
    delete c;
    pile->cons = nullptr;
}

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_pileup_consensus_device(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t min_depth, uint64_t capacity,
                                   uint8_t* out_dev, const uint64_t* bounds_dev, uint64_t m, uint64_t* offs_dev, uint64_t* stats_out,
                                   uint64_t* total_out, void* stream) {
    if (!pile || !total_out || !stats_out || (capacity && !out_dev) || (m && (!bounds_dev || !offs_dev))) {
        set_error("slamem_pileup_consensus_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    for (int k = 0; k < 5; k++) stats_out[k] = 0;
    SLAMEM_TRY(cons_check_range("slamem_pileup_consensus_device", pile, first, count));
    if (min_depth == 0u || min_depth >= 0x80000000u) {
        set_error("slamem_pileup_consensus_device: the least depth is 1 to 2^31 - 1, not %u", min_depth);
        return SLAMEM_ERR_ARG;
    }
    const ConsPlurRule p{min_depth};
    return cons_readout<kConsPlur>("slamem_pileup_consensus_device", pile, first, count, p, p, capacity, out_dev, bounds_dev, m, offs_dev,
                                   stats_out, total_out, stream);
}

int slamem_pileup_consensus_host(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t min_depth, uint64_t capacity, uint8_t* out,
                                 const uint64_t* bounds, uint64_t m, uint64_t* offs, uint64_t* stats_out, uint64_t* total_out) {
    if (!pile || !total_out || !stats_out || (capacity && !out) || (m && (!bounds || !offs))) {
        set_error("slamem_pileup_consensus_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    return cons_host("slamem_pileup_consensus_host", pile, first, count, capacity, out, bounds, m, offs, total_out,
                     [&](uint64_t room, uint8_t* out_dev, const uint64_t* bounds_dev, uint64_t* offs_dev) {
                         return slamem_pileup_consensus_device(pile, first, count, min_depth, room, out_dev, bounds_dev, m, offs_dev, stats_out,
                                                               total_out, nullptr);
                     });
}

int slamem_pileup_consensus_gt_device(slamem_pileup* pile, uint64_t first, uint64_t count, const slamem_cons_gt_params* params,
                                      uint64_t capacity, uint8_t* out_dev, const uint64_t* bounds_dev, uint64_t m, uint64_t* offs_dev,
                                      uint64_t* stats_out, uint64_t* total_out, void* stream) {
    const char* fn = "slamem_pileup_consensus_gt_device";
    if (!pile || !params || !total_out || !stats_out || (capacity && !out_dev) || (m && (!bounds_dev || !offs_dev))) {
        set_error("%s: null argument", fn);
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    for (int k = 0; k < 8; k++) stats_out[k] = 0;
    ConsGtRule rowp;
    ConsGtEvRule evp;
    SLAMEM_TRY(cons_check_range(fn, pile, first, count));
    SLAMEM_TRY(cons_gt_check(fn, pile, params, rowp, evp));
    if (params->weighted)
        return cons_readout<kConsGtw>(fn, pile, first, count, rowp, evp, capacity, out_dev, bounds_dev, m, offs_dev, stats_out, total_out, stream);
    return cons_readout<kConsGt>(fn, pile, first, count, rowp, evp, capacity, out_dev, bounds_dev, m, offs_dev, stats_out, total_out, stream);
}

int slamem_pileup_consensus_gt_host(slamem_pileup* pile, uint64_t first, uint64_t count, const slamem_cons_gt_params* params,
                                    uint64_t capacity, uint8_t* out, const uint64_t* bounds, uint64_t m, uint64_t* offs, uint64_t* stats_out,
                                    uint64_t* total_out) {
    if (!pile || !params || !total_out || !stats_out || (capacity && !out) || (m && (!bounds || !offs))) {
        set_error("slamem_pileup_consensus_gt_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    return cons_host("slamem_pileup_consensus_gt_host", pile, first, count, capacity, out, bounds, m, offs, total_out,
                     [&](uint64_t room, uint8_t* out_dev, const uint64_t* bounds_dev, uint64_t* offs_dev) {
                         return slamem_pileup_consensus_gt_device(pile, first, count, params, room, out_dev, bounds_dev, m, offs_dev, stats_out,
                                                                  total_out, nullptr);
                     });
}

}  // extern "C"
