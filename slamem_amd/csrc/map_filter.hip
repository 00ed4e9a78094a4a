// map_filter.hip -- -paf (matchType 7): one mapping per read, with a mapping quality.  DESIGN.md 4.15 has the definition; in
// short, with c_b the score of strand block b's best chain (4.12) and c'_b the score of the best chain of b's rows WITHOUT that
// chain's rows:
//   primary block   the block of the read with the largest c_b, the forward one on a tie;  s1 = its score (0: unmapped)
//   s2              max(c'_primary, c_other)
//   mapq            60 * (s1 - s2) / s1 in whole numbers
//   segments        4.14's segments of the primary block; the other block gives none
//
// All on the stream behind K9, no host read-back:
//   chain_pass              keep flags, kept rows and score per block (chain_filter.hip, as it stands)
//   k_map_rest_count / scan / k_map_rest_copy / k_map_rest_list_copy
//                           the rows the chain left, compacted per block into a second -chain workspace: the copy kernels'
//                           shape with the flag inverted (a lane per block of up to lane_max rows, a wave per listed block)
//   chain_pass              over those rows: c'_b.  (A subsequence of an emission order is one; only the scores are used.)
//   k_map_pick              a lane per read: the primary block, s2, mapq, the read's record; clears the kept count of the other
//                           block, so that chain_compact leaves it empty
//   chain_compact           the primaries' chain rows, compacted per block
//   aln_after_chain         -aln's kernels (aln_filter.hip, unchanged) over them: an empty block costs them nothing
//   k_map_fold              block offsets -> read offsets
#include "filter_blocks.h"

namespace slamem {

namespace {

struct MapLayout {
    uint64_t aln_bytes, off_chain2, off_boff, bytes;
};

MapLayout map_layout(const FilterBatch& b, const FilterParams& p) {
    MapLayout m;
    m.aln_bytes = align_up(aln_workspace_bytes(b, p), 256);
    uint64_t off = m.aln_bytes;
    m.off_chain2 = off; off = align_up(off + chain_workspace_bytes(b, p), 256);          // the second chain pass
    m.off_boff = off;   off = align_up(off + (b.num_blocks() + 1) * 8, 256);             // the segments' block offsets
    m.bytes = off;
    return m;
}

// one lane per strand block: the rows its chain left (and lane num_blocks keeps the scan's last input at 0)
__global__ void __launch_bounds__(256) k_map_rest_count(const uint64_t* __restrict__ boff, uint64_t nb, uint64_t cap,
                                                        const uint32_t* __restrict__ cnt, uint32_t* __restrict__ rest) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b > nb) return;
    if (b == nb) { rest[nb] = 0u; return; }
    uint64_t s, e;
    clamp_block(boff, b, cap, s, e);
    const uint32_t n = (uint32_t)(e - s), k = cnt[b];
    rest[b] = k < n ? n - k : 0u;
}

// one lane per strand block of up to lane_max rows: its rows that are not kept, in order
__global__ void __launch_bounds__(256) k_map_rest_copy(const uint64_t* __restrict__ boff, uint64_t nb, const slamem_mem* __restrict__ rows,
                                                       uint64_t cap, const uint8_t* __restrict__ keep, uint32_t lane_max,
                                                       const uint64_t* __restrict__ roff, slamem_mem* __restrict__ out) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= nb) return;
    uint64_t s, e;
    clamp_block(boff, b, cap, s, e);
    if (e - s > lane_max) return;
    uint64_t d = roff[b];
    const uint64_t d_end = roff[b + 1];
    for (uint64_t i = s; i < e && d < d_end; i++) {
        if (keep[i]) continue;
        if (d < cap) out[d] = rows[i];
        d++;
    }
}

// a listed block's rows that are not kept, in order: a wave ranks 64 rows at a time
__global__ void __launch_bounds__(64) k_map_rest_list_copy(const uint64_t* __restrict__ list, const unsigned long long* __restrict__ ctr,
                                                           const uint64_t* __restrict__ boff, uint64_t cap,
                                                           const slamem_mem* __restrict__ rows, const uint8_t* __restrict__ keep,
                                                           const uint64_t* __restrict__ roff, slamem_mem* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const uint64_t nl = ctr[0];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t b = list[li];
        uint64_t s, e;
        clamp_block(boff, b, cap, s, e);
        const uint32_t n = (uint32_t)(e - s);
        uint64_t d = roff[b];
        const uint64_t d_end = roff[b + 1];
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t i = base + lane;
            const bool k = i < n && !keep[s + i];
            const unsigned long long m = __ballot(k);
            if (k) {
                const uint64_t at = d + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
                if (at < d_end && at < cap) out[at] = rows[s + i];
            }
            d += (uint64_t)__popcll(m);
        }
    }
}

// one lane per read: the primary block, the competitor, the quality
__global__ void __launch_bounds__(256) k_map_pick(uint64_t nq, uint32_t strands, const uint32_t* __restrict__ score,
                                                  const uint32_t* __restrict__ score2, uint32_t* __restrict__ cnt,
                                                  slamem_map* __restrict__ reads) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= nq) return;
    const uint64_t b0 = r * strands;
    const uint32_t c0 = score[b0], c1 = strands > 1u ? score[b0 + 1u] : 0u;
    const uint32_t prim = c1 > c0 ? 1u : 0u;  // (a tie: the forward block)
    const uint32_t s1 = prim ? c1 : c0, other = prim ? c0 : c1;
    const uint32_t rest = score2[b0 + prim];
    const uint32_t s2 = rest > other ? rest : other;
    slamem_map o;
    o.s1 = s1;
    o.s2 = s1 ? s2 : 0u;
    o.strand = s1 ? (uint8_t)(1u + prim) : (uint8_t)0u;
    // (s2 <= s1: a chain of the rows left is a chain of the block, and the other block's score is not larger)
    o.mapq = s1 ? (uint8_t)((60ull * (unsigned long long)(s1 - (s2 < s1 ? s2 : s1))) / (unsigned long long)s1) : (uint8_t)0u;
    o.reserved[0] = o.reserved[1] = 0u;
    reads[r] = o;
    if (strands > 1u) cnt[b0 + (1u - prim)] = 0u;  // the other block: no chain rows, hence no gap and no segment
}

__global__ void __launch_bounds__(256) k_map_fold(uint64_t nq, uint32_t strands, const uint64_t* __restrict__ boff,
                                                  uint64_t* __restrict__ roff) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r > nq) return;
    roff[r] = boff[r * strands];
}

}  // namespace

uint64_t map_workspace_bytes(const FilterBatch& b, const FilterParams& p) { return map_layout(b, p).bytes; }

#define MSTEP(call, what) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(e__, what, __FILE__, __LINE__); } while (0)

int map_filter(void* ws, const FilterBatch& bt, const FilterParams& args, slamem_mem*, uint64_t* out_roff, unsigned long long* host_scalars,
               hipStream_t stream) {
    const uint64_t num_queries = bt.num_queries, num_blocks = bt.num_blocks(), capacity = bt.capacity;
    const uint32_t strands = bt.strands;
    const MapLayout m = map_layout(bt, args);
    char* p = static_cast<char*>(ws);
    void* ws2 = p + m.off_chain2;
    uint64_t* seg_boff = reinterpret_cast<uint64_t*>(p + m.off_boff);
    const ChainBufs a = chain_buffers(ws, num_blocks, capacity), b = chain_buffers(ws2, num_blocks, capacity);
    slamem_mem* crows;
    uint64_t* coff;
    aln_chain_buffers(ws, bt, args, &crows, &coff);
    int rc = chain_pass(ws, num_blocks, capacity, args.max_gap, nullptr, stream);
    if (rc != SLAMEM_OK) return rc;
    // the rows the chains left, as a list of their own (b.cnt holds their counts until the second pass writes it)
    hipLaunchKernelGGL(k_map_rest_count, dim3(grid_for(num_blocks + 1)), dim3(256), 0, stream, (const uint64_t*)a.boff, num_blocks,
                       capacity, (const uint32_t*)a.cnt, b.cnt);
    MSTEP(hipGetLastError(), "k_map_rest_count");
    size_t need = b.scan_bytes;
    MSTEP(scan_sum_exclusive_u32_u64(b.scan, need, b.cnt, b.boff, num_blocks, stream), "scan");
    hipLaunchKernelGGL(k_map_rest_copy, dim3(grid_for(num_blocks)), dim3(256), 0, stream, (const uint64_t*)a.boff, num_blocks,
                       (const slamem_mem*)a.rows, capacity, (const uint8_t*)a.keep, a.lane_max, (const uint64_t*)b.boff, b.rows);
    MSTEP(hipGetLastError(), "k_map_rest_copy");
    hipLaunchKernelGGL(k_map_rest_list_copy, dim3(a.wave_grid), dim3(64), 0, stream, (const uint64_t*)a.list,
                       (const unsigned long long*)a.ctr, (const uint64_t*)a.boff, capacity, (const slamem_mem*)a.rows,
                       (const uint8_t*)a.keep, (const uint64_t*)b.boff, b.rows);
    MSTEP(hipGetLastError(), "k_map_rest_list_copy");
    rc = chain_pass(ws2, num_blocks, capacity, args.max_gap, nullptr, stream);
    if (rc != SLAMEM_OK) return rc;
    hipLaunchKernelGGL(k_map_pick, dim3(grid_for(num_queries)), dim3(256), 0, stream, num_queries, strands, (const uint32_t*)a.score,
                       (const uint32_t*)b.score, a.cnt, args.reads);
    MSTEP(hipGetLastError(), "k_map_pick");
    // [0] rows kept (replaced below), [1] the highest-numbered block out of order + 1
    rc = chain_compact(ws, num_blocks, capacity, crows, coff, host_scalars, stream);
    if (rc != SLAMEM_OK) return rc;
    rc = aln_after_chain(ws, bt, args, seg_boff, host_scalars, stream);
    if (rc != SLAMEM_OK) return rc;
    hipLaunchKernelGGL(k_map_fold, dim3(grid_for(num_queries + 1)), dim3(256), 0, stream, num_queries, strands,
                       (const uint64_t*)seg_boff, out_roff);
    MSTEP(hipGetLastError(), "k_map_fold");
    return SLAMEM_OK;
}
#undef MSTEP

}  // namespace slamem
