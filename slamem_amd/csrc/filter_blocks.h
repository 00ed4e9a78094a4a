// filter_blocks.h -- what every filter behind K9 shares (mum_filter.hip, smem_filter.hip, chain_filter.hip, ext_filter.hip,
// map_filter.hip; aln_filter.hip through filter_shared.h): the block helpers, the start of the workspace, and the end of every
// filter -- kept rows per block -> new block offsets, a lane per block copies its kept rows, two scalars go to the host.
// Everything sits in an unnamed namespace: each file that includes this gets its own kernels.
#pragma once
#include "common.h"
#include "prims.h"

namespace slamem {

namespace {

inline unsigned grid_for(uint64_t items, unsigned block = 256) { return items ? (unsigned)((items + block - 1) / block) : 1u; }
inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

__device__ __forceinline__ void clamp_block(const uint64_t* __restrict__ boff, uint64_t b, uint64_t cap, uint64_t& s, uint64_t& e) {
    // (a batch whose -mem list did not fit has offsets beyond the capacity: its result is refused, nothing is read past it)
    s = boff[b];
    e = boff[b + 1];
    if (s > cap) s = cap;
    if (e > cap) e = cap;
    if (e < s) e = s;
}

// the order every block must be in: q descending, then L non-increasing
__device__ __forceinline__ bool out_of_order(const slamem_mem& prev, const slamem_mem& r) {
    return r.query_pos > prev.query_pos || (r.query_pos == prev.query_pos && r.length > prev.length);
}

// The start of a filter's workspace.  ctr, rows and boff lie at the same place in every filter (filter_list_buffers,
// filters.hip, tells K9 where to place the -mem list without knowing the filter); the filter's sections per row follow keep,
// then the scan's room (scan_at), then the filter's lists.
struct FilterPrefix {
    uint64_t off_ctr, off_rows, off_boff, off_cnt, off_newoff, off_keep, off_scan, scan_bytes;
    uint64_t begin(uint64_t num_blocks, uint64_t capacity) {  // -> where the filter's own sections start
        uint64_t off = 0;
        off_ctr = off;    off = align_up(off + 64, 256);                                  // counters: the filter says which
        off_rows = off;   off = align_up(off + capacity * sizeof(slamem_mem) + 16, 256);  // the -mem list (K9 places it here)
        off_boff = off;   off = align_up(off + (num_blocks + 1) * 8, 256);                // ... and its block offsets
        off_cnt = off;    off = align_up(off + (num_blocks + 1) * 4, 256);                // kept rows per block
        off_newoff = off; off = align_up(off + (num_blocks + 1) * 8, 256);                // their exclusive sums
        off_keep = off;   off = align_up(off + capacity + 16, 256);                       // a byte per -mem row
        return off;
    }
    uint64_t scan_at(uint64_t off, uint64_t num_blocks) {  // -> behind the scan's room
        size_t need = 0;
        (void)scan_sum_exclusive_u32_u64(nullptr, need, nullptr, nullptr, num_blocks, 0);
        scan_bytes = need;
        off_scan = off;
        return align_up(off + need, 256);
    }
};

struct FilterBufs {
    unsigned long long* ctr;
    slamem_mem* rows;
    uint64_t* boff;
    uint32_t* cnt;
    uint64_t* newoff;
    uint8_t* keep;
    void* scan;
    size_t scan_bytes;
};

inline FilterBufs filter_bufs(void* ws, const FilterPrefix& m) {
    char* p = static_cast<char*>(ws);
    return FilterBufs{reinterpret_cast<unsigned long long*>(p + m.off_ctr), reinterpret_cast<slamem_mem*>(p + m.off_rows),
                      reinterpret_cast<uint64_t*>(p + m.off_boff),          reinterpret_cast<uint32_t*>(p + m.off_cnt),
                      reinterpret_cast<uint64_t*>(p + m.off_newoff),        reinterpret_cast<uint8_t*>(p + m.off_keep),
                      p + m.off_scan,                                       (size_t)m.scan_bytes};
}

// One lane per strand block: new offsets, and the kept rows of blocks of up to kLaneMax rows (larger ones: the filter's own
// list copy).  src: the rows to copy, by their place in the -mem list; kColumn: a uint32 per row goes with them (out_column may
// be null).  kGated (-mum): nothing is written while *gate is not 0 -- the counts are not final; gate null: the final pass.
// d stops at the block's new end: a refused batch may carry flags that its counts do not match.  (Not in -mum's copy, as
// before: k_mum_small counts exactly the flags it sets in the same call.)
template <uint32_t kLaneMax, bool kColumn, bool kGated>
__global__ void __launch_bounds__(256) k_filter_copy(const uint64_t* __restrict__ boff, uint64_t nb, uint64_t cap,
                                                     const slamem_mem* __restrict__ src, const uint32_t* __restrict__ column,
                                                     const uint8_t* __restrict__ keep, const uint64_t* __restrict__ newoff,
                                                     slamem_mem* __restrict__ out, uint32_t* __restrict__ out_column,
                                                     uint64_t* __restrict__ out_boff, const unsigned long long* __restrict__ gate) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b > nb) return;
    if (kGated && gate && *gate != 0ull) return;
    uint64_t d = newoff[b];
    out_boff[b] = d;
    if (b == nb) return;
    uint64_t s, e;
    clamp_block(boff, b, cap, s, e);
    if (e - s > kLaneMax) return;
    const uint64_t d_end = kGated ? ~0ull : newoff[b + 1];
    for (uint64_t i = s; i < e && d < d_end; i++) {
        if (!keep[i]) continue;
        if (d < cap) {
            out[d] = src[i];
            if (kColumn && out_column) out_column[d] = column[i];
        }
        d++;
    }
}

// The end of a filter: cnt -> newoff, then the lane copy.  The filter's list copy follows, then kept_scalars.
template <uint32_t kLaneMax, bool kColumn = false, bool kGated = false>
inline hipError_t compact_kept(const FilterBufs& w, uint64_t num_blocks, uint64_t capacity, const slamem_mem* src, slamem_mem* out_mems,
                               uint64_t* out_boff, hipStream_t stream, const uint32_t* column = nullptr, uint32_t* out_column = nullptr,
                               const unsigned long long* gate = nullptr) {
    size_t need = w.scan_bytes;
    const hipError_t e = scan_sum_exclusive_u32_u64(w.scan, need, w.cnt, w.newoff, num_blocks, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_filter_copy<kLaneMax, kColumn, kGated>), dim3(grid_for(num_blocks + 1)), dim3(256), 0, stream,
                       (const uint64_t*)w.boff, num_blocks, capacity, src, column, (const uint8_t*)w.keep, (const uint64_t*)w.newoff,
                       out_mems, out_column, out_boff, gate);
    return hipGetLastError();
}

// host_scalars[0] = rows kept, [1] = *second (the highest-numbered block out of the emission order + 1, 0: none; -mum: its large blocks)
inline hipError_t kept_scalars(const FilterBufs& w, uint64_t num_blocks, const unsigned long long* second, unsigned long long* host_scalars,
                               hipStream_t stream) {
    const hipError_t e = hipMemcpyAsync(host_scalars, w.newoff + num_blocks, 8, hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(host_scalars + 1, second, 8, hipMemcpyDeviceToHost, stream);
}

}  // namespace

}  // namespace slamem
