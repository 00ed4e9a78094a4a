// mum_filter.hip -- -mum (matchType 2, the mode the reference reserves in its "EAU" table, slamem.c:35, and never built):
// keep the MEMs of a strand block that no other MEM of the same block contains, in query OR in reference coordinates.
// Given the complete -mem list of the block, "contained in neither coordinate" is the same as "the match string occurs once
// in the merged reference and once in the scanned strand" (DESIGN.md 4.10 has the argument).  The filter runs on the -mem
// list K9 has placed in the workspace and writes the kept rows, in their order, to the caller's buffers:
//   k_mum_small   one lane per strand block: 0 or 1 MEM keep everything; 2 .. kMumPairMax MEMs: every pair is tested; more:
//                 the block goes to the list of large blocks (one 64-bit atomic gives it its ordinal and the place of its
//                 rows in the gathered arrays, in the same order)
//   scan          kept rows per block -> new block offsets
//   k_filter_copy one lane per block copies its kept rows; gated: skipped when the batch has a large block (its counts are
//                 not final yet: the host sees the flag with the batch's scalars and runs the large path, then this again)
// Large blocks (mum_filter_large): the rows are gathered and sorted per coordinate into (block ordinal, start, end
// descending) -- two stable radix sorts, the end first -- and one workgroup per large block walks its rows in that order:
// a row is contained when the largest end among the rows before it is >= its own end, or when the next row is the same
// interval (two equal intervals contain each other: both go).  O(n log n) per block.
#include "filter_blocks.h"

namespace slamem {

namespace {

constexpr uint64_t kMask40 = (1ull << 40) - 1ull;

// T: the most MEMs a block may have for its lane to test every pair.  At T = 256 one lane does 65 k pair tests on rows its
// L1 holds (3 KB), about what the large path's fixed cost is (four radix sorts of 8-bit digits, ~40 launches, and a host
// read-back); blocks of reads (-l 20: a handful of MEMs) are far below it and a 4.6 Mbp query against its genome far above.
constexpr uint32_t kMumPairMax = 256;

struct LargeBlk {
    uint64_t block;  // strand block
    uint32_t base;   // place of its first row in the gathered arrays
    uint32_t n;      // its rows
};

struct MumLayout : FilterPrefix {
    uint64_t off_large, off_grow, off_gord, off_keys_a, off_keys_b, off_vals_a, off_vals_b, off_cont, off_sort, sort_bytes, bytes;
};

MumLayout mum_layout(uint64_t num_blocks, uint64_t capacity) {
    MumLayout m;
    uint64_t off = m.begin(num_blocks, capacity);                                   // ctr: large blocks << 40 | their rows
    off = m.scan_at(off, num_blocks);
    // the large path: rows of all large blocks together are at most the capacity
    m.off_large = off;  off = align_up(off + (capacity / (kMumPairMax + 1) + 1) * sizeof(LargeBlk), 256);
    m.off_grow = off;   off = align_up(off + capacity * sizeof(slamem_mem) + 16, 256);
    m.off_gord = off;   off = align_up(off + capacity * 4 + 16, 256);
    m.off_keys_a = off; off = align_up(off + capacity * 8 + 16, 256);
    m.off_keys_b = off; off = align_up(off + capacity * 8 + 16, 256);
    m.off_vals_a = off; off = align_up(off + capacity * 4 + 16, 256);
    m.off_vals_b = off; off = align_up(off + capacity * 4 + 16, 256);
    m.off_cont = off;   off = align_up(off + capacity + 16, 256);
    size_t sneed = 0;
    (void)sort_pairs_u64_u32(nullptr, sneed, nullptr, nullptr, nullptr, nullptr, capacity, 0, 64, 0);
    m.sort_bytes = sneed;
    m.off_sort = off;   off = align_up(off + sneed, 256);
    m.bytes = off;
    return m;
}

// one lane per strand block (and lane num_blocks keeps the scan's last input at 0)
__global__ void __launch_bounds__(256) k_mum_small(const uint64_t* __restrict__ boff, uint64_t nb, const slamem_mem* __restrict__ rows,
                                                   uint64_t cap, uint32_t* __restrict__ cnt, uint8_t* __restrict__ keep,
                                                   LargeBlk* __restrict__ large, unsigned long long* __restrict__ large_ctr) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b > nb) return;
    if (b == nb) { cnt[nb] = 0u; return; }
    uint64_t s, e;
    clamp_block(boff, b, cap, s, e);
    const uint32_t n = (uint32_t)(e - s);
    if (n <= 1u) {
        cnt[b] = n;
        if (n) keep[s] = 1u;
        return;
    }
    if (n > kMumPairMax) {
        cnt[b] = 0u;
        const unsigned long long old = atomicAdd(large_ctr, (1ull << 40) | n);
        LargeBlk lb;
        lb.block = b;
        lb.base = (uint32_t)(old & kMask40);
        lb.n = n;
        large[old >> 40] = lb;
        return;
    }
    uint32_t kept = 0;
    for (uint32_t i = 0; i < n; i++) {
        const slamem_mem a = rows[s + i];
        const uint64_t aq = (uint64_t)a.query_pos + a.length, ap = (uint64_t)a.ref_pos + a.length;
        bool in = false;
        for (uint32_t j = 0; j < n && !in; j++) {
            if (j == i) continue;
            const slamem_mem c = rows[s + j];
            in = (c.query_pos <= a.query_pos && (uint64_t)c.query_pos + c.length >= aq) ||
                 (c.ref_pos <= a.ref_pos && (uint64_t)c.ref_pos + c.length >= ap);
        }
        keep[s + i] = in ? 0u : 1u;
        kept += in ? 0u : 1u;
    }
    cnt[b] = kept;
}

// ---- large blocks: one workgroup per block, grid = their number ----------------------------------------------------------
__global__ void __launch_bounds__(256) k_mum_gather(const LargeBlk* __restrict__ large, const uint64_t* __restrict__ boff, uint64_t cap,
                                                    const slamem_mem* __restrict__ rows, slamem_mem* __restrict__ grow,
                                                    uint32_t* __restrict__ gord) {
    const LargeBlk lb = large[blockIdx.x];
    uint64_t s, e;
    clamp_block(boff, lb.block, cap, s, e);
    for (uint32_t i = threadIdx.x; i < lb.n; i += 256u) {
        grow[lb.base + i] = rows[s + i];
        gord[lb.base + i] = blockIdx.x;
    }
}

__device__ __forceinline__ uint32_t row_start(const slamem_mem& r, int coord) { return coord ? r.ref_pos : r.query_pos; }

// first sort's keys: the end, descending (the radix sort is ascending); values: the gathered row
__global__ void __launch_bounds__(256) k_mum_keys_end(const slamem_mem* __restrict__ grow, uint32_t nrows, int coord,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= nrows) return;
    const slamem_mem r = grow[g];
    uint64_t end = (uint64_t)row_start(r, coord) + r.length;
    if (end > 0xFFFFFFFFull) end = 0xFFFFFFFFull;
    keys[g] = 0xFFFFFFFFull - end;
    vals[g] = g;
}

// second sort's keys, in the order the first sort left: (block ordinal, start)
__global__ void __launch_bounds__(256) k_mum_keys_start(const slamem_mem* __restrict__ grow, const uint32_t* __restrict__ gord,
                                                        const uint32_t* __restrict__ order, uint32_t nrows, int coord,
                                                        uint64_t* __restrict__ keys) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= nrows) return;
    const uint32_t v = order[k];
    keys[k] = ((uint64_t)gord[v] << 32) | row_start(grow[v], coord);
}

// rows of one large block in (start, end descending) order: contained when the largest end before it is >= its end, or
// when the next row is the same interval.  Tiles of 256 rows; the running maximum carries from tile to tile.
__global__ void __launch_bounds__(256) k_mum_contain(const LargeBlk* __restrict__ large, const slamem_mem* __restrict__ grow,
                                                     const uint32_t* __restrict__ order, int coord, uint8_t* __restrict__ cont) {
    __shared__ uint32_t wmax[4];
    const LargeBlk lb = large[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t carry = 0;  // (every end is >= 1: 0 contains nothing)
    for (uint32_t t0 = 0; t0 < lb.n; t0 += 256u) {
        const uint32_t i = t0 + threadIdx.x;
        uint32_t v = 0, start = 0, end = 0;
        bool same_next = false;
        if (i < lb.n) {
            v = order[lb.base + i];
            const slamem_mem r = grow[v];
            start = row_start(r, coord);
            end = start + r.length;
            if (i + 1u < lb.n) {
                const slamem_mem r2 = grow[order[lb.base + i + 1u]];
                const uint32_t s2 = row_start(r2, coord);
                same_next = s2 == start && s2 + r2.length == end;
            }
        }
        // inclusive max over the wave, then over the waves before this one
        uint32_t incl = end;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if ((int)lane >= d) incl = incl > o ? incl : o;
        }
        if (lane == 63u) wmax[w] = incl;
        __syncthreads();
        uint32_t before = carry;
        for (uint32_t q = 0; q < w; q++) before = before > wmax[q] ? before : wmax[q];
        const uint32_t prev = __shfl_up(incl, 1);
        if (lane) before = before > prev ? before : prev;
        if (i < lb.n && (before >= end || same_next)) cont[v] |= (uint8_t)(1u << coord);
        for (uint32_t q = 0; q < 4u; q++) carry = carry > wmax[q] ? carry : wmax[q];
        __syncthreads();
    }
}

// a large block's keep flags (by its rows' places in the -mem list) and its count of kept rows
__global__ void __launch_bounds__(256) k_mum_large_count(const LargeBlk* __restrict__ large, const uint64_t* __restrict__ boff, uint64_t cap,
                                                         const uint8_t* __restrict__ cont, uint8_t* __restrict__ keep,
                                                         uint32_t* __restrict__ cnt) {
    __shared__ uint32_t total;
    const LargeBlk lb = large[blockIdx.x];
    uint64_t s, e;
    clamp_block(boff, lb.block, cap, s, e);
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t i = threadIdx.x; i < lb.n; i += 256u) {
        const uint8_t k = cont[lb.base + i] ? 0u : 1u;
        keep[s + i] = k;
        mine += k;
    }
    atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) cnt[lb.block] = total;
}

// a large block's kept rows, in order: tiles of 256 rows ranked with wave ballots
__global__ void __launch_bounds__(256) k_mum_large_copy(const LargeBlk* __restrict__ large, const uint64_t* __restrict__ boff, uint64_t cap,
                                                        const slamem_mem* __restrict__ rows, const uint8_t* __restrict__ keep,
                                                        const uint64_t* __restrict__ newoff, slamem_mem* __restrict__ out) {
    __shared__ uint32_t wcnt[4];
    const LargeBlk lb = large[blockIdx.x];
    uint64_t s, e;
    clamp_block(boff, lb.block, cap, s, e);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t d0 = newoff[lb.block];
    for (uint32_t t0 = 0; t0 < lb.n; t0 += 256u) {
        const uint32_t i = t0 + threadIdx.x;
        const bool k = i < lb.n && keep[s + i];
        const unsigned long long m = __ballot(k);
        if (lane == 0u) wcnt[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t q = 0; q < 4u; q++) {
            if (q < w) before += wcnt[q];
            all += wcnt[q];
        }
        before += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (k && d0 + before < cap) out[d0 + before] = rows[s + i];
        d0 += all;
        __syncthreads();
    }
}

}  // namespace

uint64_t mum_workspace_bytes(const FilterBatch& b, const FilterParams&) { return mum_layout(b.num_blocks(), b.capacity).bytes; }

#define MSTEP(call, what) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(e__, what, __FILE__, __LINE__); } while (0)

int mum_filter_small(void* ws, const FilterBatch& b, const FilterParams&, slamem_mem* out_mems, uint64_t* out_boff,
                     unsigned long long* host_scalars, hipStream_t stream) {
    const uint64_t num_blocks = b.num_blocks(), capacity = b.capacity;
    const MumLayout m = mum_layout(num_blocks, capacity);
    const FilterBufs w = filter_bufs(ws, m);
    MSTEP(hipMemsetAsync(w.ctr, 0, 8, stream), "memset");
    hipLaunchKernelGGL(k_mum_small, dim3(grid_for(num_blocks + 1)), dim3(256), 0, stream, (const uint64_t*)w.boff, num_blocks,
                       (const slamem_mem*)w.rows, capacity, w.cnt, w.keep,
                       reinterpret_cast<LargeBlk*>(static_cast<char*>(ws) + m.off_large), w.ctr);
    MSTEP(hipGetLastError(), "k_mum_small");
    MSTEP((compact_kept<kMumPairMax, false, true>(w, num_blocks, capacity, w.rows, out_mems, out_boff, stream, nullptr, nullptr, w.ctr)),
          "compact_kept");
    // [0] rows kept (final when [1] is 0), [1] large blocks << 40 | their rows
    MSTEP(kept_scalars(w, num_blocks, w.ctr, host_scalars, stream), "memcpy");
    return SLAMEM_OK;
}

int mum_filter_large(void* ws, const FilterBatch& b, unsigned long long large_ctr, slamem_mem* out_mems, uint64_t* out_boff,
                     hipStream_t stream, uint64_t* total_out) {
    const uint64_t num_blocks = b.num_blocks(), capacity = b.capacity;
    const MumLayout m = mum_layout(num_blocks, capacity);
    const FilterBufs w = filter_bufs(ws, m);
    char* p = static_cast<char*>(ws);
    const slamem_mem* rows = w.rows;
    const uint64_t* boff = w.boff;
    const LargeBlk* large = reinterpret_cast<const LargeBlk*>(p + m.off_large);
    slamem_mem* grow = reinterpret_cast<slamem_mem*>(p + m.off_grow);
    uint32_t* gord = reinterpret_cast<uint32_t*>(p + m.off_gord);
    uint64_t* ka = reinterpret_cast<uint64_t*>(p + m.off_keys_a);
    uint64_t* kb = reinterpret_cast<uint64_t*>(p + m.off_keys_b);
    uint32_t* va = reinterpret_cast<uint32_t*>(p + m.off_vals_a);
    uint32_t* vb = reinterpret_cast<uint32_t*>(p + m.off_vals_b);
    uint8_t* cont = reinterpret_cast<uint8_t*>(p + m.off_cont);
    const uint64_t nl = large_ctr >> 40, nrows = large_ctr & kMask40;
    if (nl == 0 || nrows > capacity || nrows >= 0xFFFFFFFFull) {
        set_error("slamem_find_mums_device: inconsistent large-block count (%llu blocks, %llu rows)", (unsigned long long)nl,
                  (unsigned long long)nrows);
        return SLAMEM_ERR_ARG;
    }
    int obits = 1;
    while (obits < 32 && (1ull << obits) < nl) obits++;
    hipLaunchKernelGGL(k_mum_gather, dim3((unsigned)nl), dim3(256), 0, stream, large, boff, capacity, rows, grow, gord);
    MSTEP(hipGetLastError(), "k_mum_gather");
    MSTEP(hipMemsetAsync(cont, 0, nrows, stream), "memset");
    for (int coord = 0; coord < 2; coord++) {
        size_t need = m.sort_bytes;
        hipLaunchKernelGGL(k_mum_keys_end, dim3(grid_for(nrows)), dim3(256), 0, stream, (const slamem_mem*)grow, (uint32_t)nrows, coord, ka, va);
        MSTEP(hipGetLastError(), "k_mum_keys_end");
        MSTEP(sort_pairs_u64_u32(p + m.off_sort, need, ka, kb, va, vb, nrows, 0, 32, stream), "sort (end)");
        hipLaunchKernelGGL(k_mum_keys_start, dim3(grid_for(nrows)), dim3(256), 0, stream, (const slamem_mem*)grow, (const uint32_t*)gord,
                           (const uint32_t*)vb, (uint32_t)nrows, coord, ka);
        MSTEP(hipGetLastError(), "k_mum_keys_start");
        MSTEP(sort_pairs_u64_u32(p + m.off_sort, need, ka, kb, vb, va, nrows, 0, 32 + obits, stream), "sort (start)");
        hipLaunchKernelGGL(k_mum_contain, dim3((unsigned)nl), dim3(256), 0, stream, large, (const slamem_mem*)grow, (const uint32_t*)va,
                           coord, cont);
        MSTEP(hipGetLastError(), "k_mum_contain");
    }
    hipLaunchKernelGGL(k_mum_large_count, dim3((unsigned)nl), dim3(256), 0, stream, large, boff, capacity, (const uint8_t*)cont, w.keep, w.cnt);
    MSTEP(hipGetLastError(), "k_mum_large_count");
    MSTEP((compact_kept<kMumPairMax, false, true>(w, num_blocks, capacity, rows, out_mems, out_boff, stream)), "compact_kept");  // (no gate: final)
    hipLaunchKernelGGL(k_mum_large_copy, dim3((unsigned)nl), dim3(256), 0, stream, large, boff, capacity, rows, (const uint8_t*)w.keep,
                       (const uint64_t*)w.newoff, out_mems);
    MSTEP(hipGetLastError(), "k_mum_large_copy");
    unsigned long long kept = 0;
    MSTEP(hipMemcpyAsync(&kept, w.newoff + num_blocks, 8, hipMemcpyDeviceToHost, stream), "memcpy");
    MSTEP(hipStreamSynchronize(stream), "-mum large blocks (sync)");
    *total_out = kept;
    return SLAMEM_OK;
}
#undef MSTEP

}  // namespace slamem
