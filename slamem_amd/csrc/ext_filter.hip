// ext_filter.hip -- -ext (matchType 5): every -mem row of a strand block is extended on its own diagonal, to the left and to
// the right, through mismatches, by an X-drop rule; rows that grow into the same segment are reported once.  DESIGN.md 4.13
// has the definition; in short, with the mismatch penalty P >= 1 and the drop X >= 0, one side of a row is
//   s = best = ext = 0;  for t = 0, 1, ...:  stop when a letter lies outside its sequence or is not one of A,C,G,T;
//   s += 1 on equal letters, s -= P otherwise;  s > best: best = s, ext = t + 1;  best - s > X: stop
// and the row (p, q, L) becomes (p - extL, q - extL, extL + L + extR) with the mismatches inside it.
//
// s only falls at a mismatch, so the rule is a walk over the set bits of the mismatch mask: per 64 letters the two planes of
// the strand and of the text are XORed, the results ORed, and per set bit (ctz) the run of matches in front of it is added, the
// maximum taken, P subtracted and the drop tested.  No loop here runs per letter.
//
// The filter runs on the -mem list K9 has placed in the workspace -- all on the stream, no host read-back:
//   k_ext_units / scan      64-letter units per record -> where each record's planes start
//   k_ext_pack / _long      the batch's letters -> planes {p0, p1, nm} per unit, ONCE per record (the forward strand; the
//                           reverse strand is its bit-reversed complement, taken per window): a lane per record of up to
//                           kExtPackLaneUnits units, a workgroup per longer one (device-side list)
//   k_ext_mark / _wave      a lane per strand block: the block of each of its rows, the emission order; blocks of more than
//                           kExtLaneMax rows go to a list and a wave writes theirs
//   k_ext_extend            a lane per -mem row: both sides, 64 letters a step
//   k_ext_dedup / _wave     a row is dropped when a row before it in the block extends to the same segment: those lie in the
//                           contiguous run of rows before it whose (seed) query start is inside the segment
//   scan                    kept rows per block -> new block offsets
//   k_filter_copy / k_ext_list_copy   the kept rows and their mismatches, in order
// Every row is checked against the one before it: a block out of the emission order fails the call -- never wrong rows.
#include "filter_shared.h"

namespace slamem {

namespace {

constexpr uint32_t kExtLaneMax = 32;        // rows of a block one lane de-duplicates
constexpr unsigned kExtWaveGrid = 2048;     // one-wave workgroups that share the list of larger blocks

struct ExtLayout : FilterPrefix {
    uint64_t off_owner, off_xrows, off_xmm, off_list, off_ucnt, off_uoff, off_uscan, uscan_bytes, off_long, off_units, bytes;
};

ExtLayout ext_layout(uint64_t num_queries, uint64_t num_blocks, uint64_t query_bytes, uint64_t capacity) {
    ExtLayout m;
    uint64_t off = m.begin(num_blocks, capacity);                                       // ctr: [0] listed blocks, [1] order violation, [2] listed records
    m.off_owner = off;  off = align_up(off + capacity * 4 + 16, 256);                   // the strand block of every -mem row
    m.off_xrows = off;  off = align_up(off + capacity * sizeof(slamem_mem) + 16, 256);  // the extended rows
    m.off_xmm = off;    off = align_up(off + capacity * 4 + 16, 256);                   // ... and their mismatches
    off = m.scan_at(off, num_blocks);
    m.off_list = off;   off = align_up(off + (capacity / (kExtLaneMax + 1) + 1) * 8, 256);  // listed strand blocks
    m.off_ucnt = off;   off = align_up(off + (num_queries + 1) * 4, 256);               // units per record
    m.off_uoff = off;   off = align_up(off + (num_queries + 1) * 8, 256);               // their exclusive sums
    size_t need = 0;
    (void)scan_sum_exclusive_u32_u64(nullptr, need, nullptr, nullptr, num_queries, 0);
    m.uscan_bytes = need;
    m.off_uscan = off;  off = align_up(off + need, 256);
    m.off_long = off;   off = align_up(off + (query_bytes / (64ull * kExtPackLaneUnits) + 1) * 8, 256);  // listed records
    m.off_units = off;  off = align_up(off + (query_bytes / 64 + num_queries + 1) * sizeof(QueryUnit), 256);  // the packed batch
    m.bytes = off;
    return m;
}

// ---- whose row is it, and is the block in order -----------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_ext_mark(const uint64_t* __restrict__ boff, uint64_t nb, const slamem_mem* __restrict__ rows,
                                                  uint64_t cap, uint32_t* __restrict__ owner, uint32_t* __restrict__ cnt,
                                                  uint64_t* __restrict__ list, unsigned long long* __restrict__ ctr) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b > nb) return;
    cnt[b] = 0u;  // (lane nb keeps the scan's last input at 0; the others are written again by the de-duplication)
    if (b == nb) return;
    uint64_t s, e;
    clamp_block(boff, b, cap, s, e);
    if (e - s > kExtLaneMax) { list[atomicAdd(&ctr[0], 1ull)] = b; return; }
    bool bad = false;
    for (uint64_t i = s; i < e; i++) {
        owner[i] = (uint32_t)b;
        if (i > s && out_of_order(rows[i - 1], rows[i])) bad = true;
    }
    if (bad) atomicMax(&ctr[1], (unsigned long long)b + 1ull);
}

__global__ void __launch_bounds__(64) k_ext_mark_wave(const uint64_t* __restrict__ list, const unsigned long long* __restrict__ ctr_in,
                                                      const uint64_t* __restrict__ boff, const slamem_mem* __restrict__ rows, uint64_t cap,
                                                      uint32_t* __restrict__ owner, unsigned long long* __restrict__ ctr) {
    const uint64_t nl = ctr_in[0];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t b = list[li];
        uint64_t s, e;
        clamp_block(boff, b, cap, s, e);
        bool bad = false;
        for (uint64_t i = s + threadIdx.x; i < e; i += 64u) {
            owner[i] = (uint32_t)b;
            if (i > s && out_of_order(rows[i - 1], rows[i])) bad = true;
        }
        if (bad) atomicMax(&ctr[1], (unsigned long long)b + 1ull);
    }
}

// ---- the extension -------------------------------------------------------------------------------------------------------

// one lane per -mem row
__global__ void __launch_bounds__(256) k_ext_extend(const uint64_t* __restrict__ boff, uint64_t nb, const slamem_mem* __restrict__ rows,
                                                    uint64_t cap, const uint32_t* __restrict__ owner, const uint64_t* __restrict__ offsets,
                                                    const uint64_t* __restrict__ uoff, const QueryUnit* __restrict__ units,
                                                    const TextPlanes* __restrict__ tpl, uint32_t n, uint32_t strands, uint32_t penalty,
                                                    uint32_t xdrop, slamem_mem* __restrict__ xrows, uint32_t* __restrict__ xmm) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint64_t total = boff[nb];
    if (total > cap) total = cap;
    if (i >= total) return;
    const slamem_mem r = rows[i];
    // (a batch that is refused -- its list did not fit, or it is searched again -- may leave rows that no block owns)
    const bool ok = owner[i] < nb;
    const uint32_t b = ok ? owner[i] : 0u;
    const uint64_t rec = b / strands;
    const bool rev = (b % strands) != 0u;
    const int64_t len = (int64_t)(offsets[rec + 1] - offsets[rec]);
    const int64_t qn = (len + 63) >> 6, tn = ((int64_t)n + 63) >> 6;
    const uint4* Q = reinterpret_cast<const uint4*>(units + uoff[rec]);
    const uint4* T = reinterpret_cast<const uint4*>(tpl);
    const int64_t p = r.ref_pos, q = r.query_pos, L = r.length;
    const int64_t P = penalty, X = xdrop;
    Side right = {0, 0, 0, 0, 0, 0}, left = {0, 0, 0, 0, 0, 0};
    // (a row outside its sequences is left as it is: nothing is read for it)
    if (ok && qn > 0 && q + L <= len && p + L <= (int64_t)n) {
        // the first 64 letters of both sides, of the strand and of the text, are requested before any is looked at
        Win qr = strand_window(Q, qn, len, rev, q + L), tr = window(T, tn, n, p + L);
        Win ql = mirrored(strand_window(Q, qn, len, rev, q - 64)), tl = mirrored(window(T, tn, n, p - 64));
        for (uint64_t t0 = 0; !walk(right, qr, tr, t0, P, X);) {
            t0 += 64u;
            qr = strand_window(Q, qn, len, rev, q + L + (int64_t)t0);
            tr = window(T, tn, n, p + L + (int64_t)t0);
        }
        for (uint64_t t0 = 0; !walk(left, ql, tl, t0, P, X);) {
            t0 += 64u;
            ql = mirrored(strand_window(Q, qn, len, rev, q - 64 - (int64_t)t0));
            tl = mirrored(window(T, tn, n, p - 64 - (int64_t)t0));
        }
    }
    slamem_mem x;
    x.ref_pos = (uint32_t)(p - (int64_t)left.ext);
    x.query_pos = (uint32_t)(q - (int64_t)left.ext);
    x.length = (uint32_t)((int64_t)left.ext + L + (int64_t)right.ext);
    xrows[i] = x;
    xmm[i] = left.mm_best + right.mm_best;
}

// ---- one row per segment ---------------------------------------------------------------------------------------------------

// Is there a row before row i of the block (rows R / extended X, both from the block's start) with the same segment?  Such a
// row's seed lies inside the segment, and q only falls along the block: the candidates are the run of rows right before i
// whose seed starts in front of the segment's end.
__device__ __forceinline__ bool has_earlier_twin(const slamem_mem* __restrict__ R, const slamem_mem* __restrict__ X, uint32_t i) {
    const slamem_mem x = X[i];
    const uint64_t end = (uint64_t)x.query_pos + x.length;
    for (uint32_t j = i; j-- > 0u;) {
        if ((uint64_t)R[j].query_pos >= end) break;
        const slamem_mem y = X[j];
        if (y.ref_pos == x.ref_pos && y.query_pos == x.query_pos && y.length == x.length) return true;
    }
    return false;
}

// one lane per strand block of up to kExtLaneMax rows
__global__ void __launch_bounds__(256) k_ext_dedup(const uint64_t* __restrict__ boff, uint64_t nb, const slamem_mem* __restrict__ rows,
                                                   uint64_t cap, const slamem_mem* __restrict__ xrows, uint8_t* __restrict__ keep,
                                                   uint32_t* __restrict__ cnt) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= nb) return;
    uint64_t s, e;
    clamp_block(boff, b, cap, s, e);
    const uint32_t n = (uint32_t)(e - s);
    if (n == 0u || n > kExtLaneMax) return;  // (empty: cnt is 0 already; larger: k_ext_dedup_wave)
    uint32_t kept = 1u;
    keep[s] = 1u;
    for (uint32_t i = 1u; i < n; i++) {
        const bool k = !has_earlier_twin(rows + s, xrows + s, i);
        keep[s + i] = k ? 1u : 0u;
        kept += k ? 1u : 0u;
    }
    cnt[b] = kept;
}

// a wave per listed block, a lane per row
__global__ void __launch_bounds__(64) k_ext_dedup_wave(const uint64_t* __restrict__ list, const unsigned long long* __restrict__ ctr,
                                                       const uint64_t* __restrict__ boff, const slamem_mem* __restrict__ rows, uint64_t cap,
                                                       const slamem_mem* __restrict__ xrows, uint8_t* __restrict__ keep,
                                                       uint32_t* __restrict__ cnt) {
    const uint32_t lane = threadIdx.x;
    const uint64_t nl = ctr[0];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t b = list[li];
        uint64_t s, e;
        clamp_block(boff, b, cap, s, e);
        const uint32_t n = (uint32_t)(e - s);
        uint32_t kept = 0;
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t i = base + lane;
            const bool k = i < n && !has_earlier_twin(rows + s, xrows + s, i);
            if (i < n) keep[s + i] = k ? 1u : 0u;
            kept += (uint32_t)__popcll(__ballot(k));
        }
        if (lane == 0u) cnt[b] = kept;
    }
}

// a listed block's kept rows, in order: a wave ranks 64 rows at a time
__global__ void __launch_bounds__(64) k_ext_list_copy(const uint64_t* __restrict__ list, const unsigned long long* __restrict__ ctr,
                                                      const uint64_t* __restrict__ boff, uint64_t cap, const slamem_mem* __restrict__ xrows,
                                                      const uint32_t* __restrict__ xmm, const uint8_t* __restrict__ keep,
                                                      const uint64_t* __restrict__ newoff, slamem_mem* __restrict__ out,
                                                      uint32_t* __restrict__ out_mm) {
    const uint32_t lane = threadIdx.x;
    const uint64_t nl = ctr[0];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t b = list[li];
        uint64_t s, e;
        clamp_block(boff, b, cap, s, e);
        const uint32_t n = (uint32_t)(e - s);
        uint64_t d = newoff[b];
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t i = base + lane;
            const bool k = i < n && keep[s + i];
            const unsigned long long m = __ballot(k);
            if (k) {
                const uint64_t at = d + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
                if (at < cap) {
                    out[at] = xrows[s + i];
                    if (out_mm) out_mm[at] = xmm[s + i];
                }
            }
            d += (uint64_t)__popcll(m);
        }
    }
}

}  // namespace

uint64_t ext_workspace_bytes(const FilterBatch& b, const FilterParams&) {
    return ext_layout(b.num_queries, b.num_blocks(), b.query_bytes, b.capacity).bytes;
}

#define XSTEP(call, what) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(e__, what, __FILE__, __LINE__); } while (0)

int ext_filter(void* ws, const FilterBatch& b, const FilterParams& prm, slamem_mem* out_mems, uint64_t* out_boff,
               unsigned long long* host_scalars, hipStream_t stream) {
    const uint64_t num_queries = b.num_queries, num_blocks = b.num_blocks(), capacity = b.capacity;
    const ExtLayout m = ext_layout(num_queries, num_blocks, b.query_bytes, capacity);
    const FilterBufs w = filter_bufs(ws, m);
    char* p = static_cast<char*>(ws);
    const slamem_mem* rows = w.rows;
    const uint64_t* boff = w.boff;
    uint32_t* owner = reinterpret_cast<uint32_t*>(p + m.off_owner);
    slamem_mem* xrows = reinterpret_cast<slamem_mem*>(p + m.off_xrows);
    uint32_t* xmm = reinterpret_cast<uint32_t*>(p + m.off_xmm);
    uint64_t* list = reinterpret_cast<uint64_t*>(p + m.off_list);
    uint32_t* ucnt = reinterpret_cast<uint32_t*>(p + m.off_ucnt);
    uint64_t* uoff = reinterpret_cast<uint64_t*>(p + m.off_uoff);
    uint64_t* longs = reinterpret_cast<uint64_t*>(p + m.off_long);
    QueryUnit* units = reinterpret_cast<QueryUnit*>(p + m.off_units);
    uint32_t* out_mm = prm.column_dev;
    XSTEP(hipMemsetAsync(w.ctr, 0, 24, stream), "memset");
    // the batch as planes
    XSTEP(pack_batch_planes(static_cast<const char*>(b.queries_dev), b.offsets_dev, num_queries, ucnt, uoff, p + m.off_uscan, m.uscan_bytes,
                            longs, units, w.ctr, stream),
          "pack_batch_planes");
    // the rows
    hipLaunchKernelGGL(k_ext_mark, dim3(grid_for(num_blocks + 1)), dim3(256), 0, stream, boff, num_blocks, rows, capacity, owner, w.cnt, list,
                       w.ctr);
    XSTEP(hipGetLastError(), "k_ext_mark");
    hipLaunchKernelGGL(k_ext_mark_wave, dim3(kExtWaveGrid), dim3(64), 0, stream, (const uint64_t*)list, (const unsigned long long*)w.ctr, boff,
                       rows, capacity, owner, w.ctr);
    XSTEP(hipGetLastError(), "k_ext_mark_wave");
    hipLaunchKernelGGL(k_ext_extend, dim3(grid_for(capacity)), dim3(256), 0, stream, boff, num_blocks, rows, capacity,
                       (const uint32_t*)owner, b.offsets_dev, (const uint64_t*)uoff, (const QueryUnit*)units, b.ix->tpl, b.ix->n, b.strands,
                       prm.penalty, prm.xdrop, xrows, xmm);
    XSTEP(hipGetLastError(), "k_ext_extend");
    hipLaunchKernelGGL(k_ext_dedup, dim3(grid_for(num_blocks)), dim3(256), 0, stream, boff, num_blocks, rows, capacity,
                       (const slamem_mem*)xrows, w.keep, w.cnt);
    XSTEP(hipGetLastError(), "k_ext_dedup");
    hipLaunchKernelGGL(k_ext_dedup_wave, dim3(kExtWaveGrid), dim3(64), 0, stream, (const uint64_t*)list, (const unsigned long long*)w.ctr,
                       boff, rows, capacity, (const slamem_mem*)xrows, w.keep, w.cnt);
    XSTEP(hipGetLastError(), "k_ext_dedup_wave");
    XSTEP((compact_kept<kExtLaneMax, true>(w, num_blocks, capacity, xrows, out_mems, out_boff, stream, xmm, out_mm)), "compact_kept");
    hipLaunchKernelGGL(k_ext_list_copy, dim3(kExtWaveGrid), dim3(64), 0, stream, (const uint64_t*)list, (const unsigned long long*)w.ctr,
                       boff, capacity, (const slamem_mem*)xrows, (const uint32_t*)xmm, (const uint8_t*)w.keep, (const uint64_t*)w.newoff,
                       out_mems, out_mm);
    XSTEP(hipGetLastError(), "k_ext_list_copy");
    XSTEP(kept_scalars(w, num_blocks, w.ctr + 1, host_scalars, stream), "memcpy");
    return SLAMEM_OK;
}
#undef XSTEP

}  // namespace slamem
