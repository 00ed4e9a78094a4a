// sam_filter.hip -- what -sam needs beyond -paf's mapping: the MD entries of every segment, the letters under
// `=` per segment and the primary segment per read.  An MD entry is one uint32 per reference letter under X or D,
//   m << 4 | d << 2 | c     m: the reference letters under `=` since the last entry (an I changes neither p nor m),
//                           d: 1 under D, c: the text's letter A C G T = 0..3 at that place
// and one closing entry m << 4 | 8 per segment.  All on the caller's stream behind slamem_find_maps_device's outputs:
//   k_md_count        a lane per segment: the entries it will emit, its letters under `=`; a segment of more than kSamLaneOps
//                     operations goes to a list (one atomic each)
//   scan              the entries' exclusive sums (scan.hip)
//   k_md_write        a lane per segment of up to kSamLaneOps operations: the entries, each letter from the text planes
//   k_md_write_wave   a wave per listed segment: 64 operations a trip, the entries' places by a wave prefix sum over the
//                     operations' entry counts, m carried across trips and across I
//   k_sam_primary     a lane per read: the segment with the most letters under `=`, the first on a tie
// No store goes at or behind md_capacity; the total comes back with one copy at the end.
#include "buffers.h"
#include "filter_blocks.h"
#include "pile_shared.h"

namespace slamem {

namespace {

// Operations of a segment that a lane walks alone.  A trip of the wave kernel costs three wave scans of six shuffle steps and a
// ballot whatever the trip holds, about what a lane spends on 32 operations of two or three instructions each; below that a wave
// would also leave more than half its lanes without an operation.  The pileup's walk over the same operations splits at the same
// place (kPileLaneOps).
constexpr uint32_t kSamLaneOps = 32;
constexpr unsigned kSamWaveGrid = 2048;  // one-wave workgroups that share the list
constexpr uint32_t kMdClose = 8u;

__device__ __forceinline__ uint32_t md_entry_step(uint32_t op) {  // entries an operation emits
    const uint32_t c = op & 15u;
    return (c == kOpX || c == kOpD) ? op >> 4 : 0u;
}
__device__ __forceinline__ uint32_t md_eq_step(uint32_t op) { return (op & 15u) == kOpEq ? op >> 4 : 0u; }

// the k entries of an X or D operation at reference place p, from entry `at`: the first carries m
__device__ __forceinline__ void md_emit(const TextPlanes* __restrict__ tpl, uint64_t n, uint32_t op, uint64_t p, uint32_t m, uint64_t at,
                                        uint64_t cap, uint32_t* __restrict__ md) {
    const uint32_t k = op >> 4, d = (op & 15u) == kOpD ? 4u : 0u;
    for (uint32_t j = 0; j < k; j++) {
        if (at + j >= cap) return;
        md[at + j] = ((j ? 0u : m) << 4) | d | md_text(tpl, n, p + j);
    }
}

__global__ void __launch_bounds__(256) k_md_count(uint64_t ns, const uint32_t* __restrict__ ops, const uint64_t* __restrict__ ooff,
                                                  uint32_t* __restrict__ cnt, uint32_t* __restrict__ seg_eq, uint64_t* __restrict__ list,
                                                  unsigned long long* __restrict__ ctr) {
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s > ns) return;
    if (s == ns) { cnt[ns] = 0u; return; }  // (the scan reads it)
    const uint64_t o0 = ooff[s], o1 = ooff[s + 1];
    uint32_t e = 1u, eq = 0u;
    for (uint64_t i = o0; i < o1; i++) {
        const uint32_t op = ops[i];
        e += md_entry_step(op);
        eq += md_eq_step(op);
    }
    cnt[s] = e;
    seg_eq[s] = eq;
    if (o1 > o0 && o1 - o0 > kSamLaneOps) list[atomicAdd(&ctr[0], 1ull)] = s;
}

__global__ void __launch_bounds__(256) k_md_write(uint64_t ns, const slamem_aln* __restrict__ segs, const uint32_t* __restrict__ ops,
                                                  const uint64_t* __restrict__ ooff, const TextPlanes* __restrict__ tpl, uint64_t n,
                                                  const uint64_t* __restrict__ moff, uint32_t* __restrict__ md, uint64_t cap) {
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s >= ns) return;
    const uint64_t o0 = ooff[s], o1 = ooff[s + 1];
    if (o1 > o0 && o1 - o0 > kSamLaneOps) return;
    uint64_t p = segs[s].ref_pos, at = moff[s];
    uint32_t m = 0;
    for (uint64_t i = o0; i < o1; i++) {
        const uint32_t op = ops[i], k = md_entry_step(op);
        if (k) {
            md_emit(tpl, n, op, p, m, at, cap, md);
            at += k;
            m = 0;
        } else {
            m += md_eq_step(op);
        }
        p += pile_ref_step(op);
    }
    if (at < cap) md[at] = (m << 4) | kMdClose;
}

__global__ void __launch_bounds__(64) k_md_write_wave(const uint64_t* __restrict__ list, const unsigned long long* __restrict__ ctr,
                                                      const slamem_aln* __restrict__ segs, const uint32_t* __restrict__ ops,
                                                      const uint64_t* __restrict__ ooff, const TextPlanes* __restrict__ tpl, uint64_t n,
                                                      const uint64_t* __restrict__ moff, uint32_t* __restrict__ md, uint64_t cap) {
    const uint32_t lane = threadIdx.x;
    const uint64_t nl = ctr[0];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t s = list[li];
        const uint64_t o0 = ooff[s], o1 = ooff[s + 1];
        uint64_t p = segs[s].ref_pos, at = moff[s];
        uint64_t carry = 0;  // reference letters under `=` since the last entry of the trips so far
        for (uint64_t base = o0; base < o1; base += 64u) {
            const bool have = base + lane < o1;
            const uint32_t op = have ? ops[base + lane] : 0u;
            const uint64_t rs = pile_ref_step(op), es = md_entry_step(op), qs = md_eq_step(op);
            const uint64_t ri = wave_scan_inclusive(rs, lane), ei = wave_scan_inclusive(es, lane), qi = wave_scan_inclusive(qs, lane);
            const unsigned long long emits = __ballot(es != 0u);
            // the last emitting operation in front of this one: the `=` letters up to it belong to its entries' predecessors
            const unsigned long long before = emits & ((1ull << lane) - 1ull);
            const int prev = before ? 63 - __builtin_clzll(before) : 0;
            const uint64_t q_prev = __shfl(qi, prev, 64);
            if (es) {
                const uint64_t m = before ? qi - q_prev : carry + qi;  // (an emitting operation adds nothing to qi)
                md_emit(tpl, n, op, p + ri - rs, (uint32_t)m, at + ei - es, cap, md);
            }
            const int last = emits ? 63 - __builtin_clzll(emits) : 0;
            const uint64_t q_all = __shfl(qi, 63, 64), q_last = __shfl(qi, last, 64);
            carry = emits ? q_all - q_last : carry + q_all;
            p += __shfl(ri, 63, 64);
            at += __shfl(ei, 63, 64);
        }
        if (lane == 0u && at < cap) md[at] = ((uint32_t)carry << 4) | kMdClose;
    }
}

__global__ void __launch_bounds__(256) k_sam_primary(uint64_t nq, uint64_t ns, const uint64_t* __restrict__ roff,
                                                     const uint32_t* __restrict__ seg_eq, uint32_t* __restrict__ primary) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= nq) return;
    uint64_t s0 = roff[r], s1 = roff[r + 1];
    if (s1 > ns) s1 = ns;
    uint32_t best = 0xFFFFFFFFu, best_eq = 0u;
    for (uint64_t s = s0; s < s1; s++) {
        const uint32_t e = seg_eq[s];
        if (best == 0xFFFFFFFFu || e > best_eq) { best = (uint32_t)(s - s0); best_eq = e; }
    }
    primary[r] = best;
}

struct MdLayout {
    uint64_t off_ctr, off_cnt, off_list, off_scan, scan_bytes, bytes;
};

MdLayout md_layout(uint64_t num_segs) {
    MdLayout m;
    uint64_t off = 0;
    m.off_ctr = off;  off = align_up(off + 64, 256);
    m.off_cnt = off;  off = align_up(off + (num_segs + 1) * 4, 256);
    m.off_list = off; off = align_up(off + (num_segs + 1) * 8, 256);
    size_t need = 0;
    (void)scan_sum_exclusive_u32_u64(nullptr, need, nullptr, nullptr, num_segs, 0);
    m.scan_bytes = need;
    m.off_scan = off; off = align_up(off + need, 256);
    m.bytes = off;
    return m;
}

}  // namespace

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_maps_md_workspace_bytes(uint64_t num_segs, uint32_t num_queries, uint64_t* bytes_out) {
    (void)num_queries;
    if (!bytes_out) { set_error("slamem_maps_md_workspace_bytes: null argument"); return SLAMEM_ERR_ARG; }
    if (num_segs >= 0xFFFFFFFFull) { set_error("slamem_maps_md_workspace_bytes: at most 2^32 - 2 segments a batch"); return SLAMEM_ERR_ARG; }
    *bytes_out = md_layout(num_segs).bytes;
    return SLAMEM_OK;
}

int slamem_maps_md_device(const slamem_index* idx, const slamem_aln* segs_dev, uint64_t num_segs, const uint64_t* read_offsets_dev,
                          uint32_t num_queries, const uint32_t* ops_dev, const uint64_t* op_offsets_dev, uint32_t* md_dev,
                          uint64_t md_capacity, uint64_t* md_offsets_dev, uint32_t* seg_eq_dev, uint32_t* primary_dev, void* workspace_dev,
                          uint64_t workspace_bytes, void* stream, uint64_t* md_total) {
    if (!idx || !md_total || !md_offsets_dev || (num_queries && (!read_offsets_dev || !primary_dev)) ||
        (num_segs && (!segs_dev || !ops_dev || !op_offsets_dev || !seg_eq_dev || !workspace_dev)) || (md_capacity && !md_dev)) {
        set_error("slamem_maps_md_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    *md_total = 0;
    if (!idx->view.tpl) {
        set_error("slamem_maps_md_device: the MD entries take the reference letters from the text planes of the index, and this index "
                  "has none (the compact layout, or one built with the seed sections switched off)");
        return SLAMEM_ERR_ARG;
    }
    if (num_segs >= 0xFFFFFFFFull) { set_error("slamem_maps_md_device: at most 2^32 - 2 segments a batch"); return SLAMEM_ERR_ARG; }
    const MdLayout m = md_layout(num_segs);
    if (num_segs && workspace_bytes < m.bytes) {
        set_error("slamem_maps_md_device: the workspace has %llu bytes, slamem_maps_md_workspace_bytes asks for %llu",
                  (unsigned long long)workspace_bytes, (unsigned long long)m.bytes);
        return SLAMEM_ERR_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t total = 0;
    if (num_segs == 0) {
        SLAMEM_HIP(hipMemsetAsync(md_offsets_dev, 0, 8, st));
    } else {
        char* p = static_cast<char*>(workspace_dev);
        unsigned long long* ctr = reinterpret_cast<unsigned long long*>(p + m.off_ctr);
        uint32_t* cnt = reinterpret_cast<uint32_t*>(p + m.off_cnt);
        uint64_t* list = reinterpret_cast<uint64_t*>(p + m.off_list);
        const TextPlanes* tpl = idx->view.tpl;
        const uint64_t n = idx->view.n;
        SLAMEM_HIP(hipMemsetAsync(ctr, 0, 64, st));
        hipLaunchKernelGGL(k_md_count, dim3(pile_grid(num_segs + 1, 256)), dim3(256), 0, st, num_segs, ops_dev, op_offsets_dev, cnt,
                           seg_eq_dev, list, ctr);
        SLAMEM_HIP(hipGetLastError());
        size_t need = m.scan_bytes;
        SLAMEM_HIP(scan_sum_exclusive_u32_u64(p + m.off_scan, need, cnt, md_offsets_dev, num_segs, st));
        hipLaunchKernelGGL(k_md_write, dim3(pile_grid(num_segs, 256)), dim3(256), 0, st, num_segs, segs_dev, ops_dev, op_offsets_dev, tpl,
                           n, (const uint64_t*)md_offsets_dev, md_dev, md_capacity);
        SLAMEM_HIP(hipGetLastError());
        const unsigned grid = num_segs < kSamWaveGrid ? (unsigned)num_segs : kSamWaveGrid;
        hipLaunchKernelGGL(k_md_write_wave, dim3(grid), dim3(64), 0, st, (const uint64_t*)list, (const unsigned long long*)ctr, segs_dev,
                           ops_dev, op_offsets_dev, tpl, n, (const uint64_t*)md_offsets_dev, md_dev, md_capacity);
        SLAMEM_HIP(hipGetLastError());
    }
    if (num_queries) {
        hipLaunchKernelGGL(k_sam_primary, dim3(pile_grid(num_queries, 256)), dim3(256), 0, st, (uint64_t)num_queries, num_segs,
                           read_offsets_dev, (const uint32_t*)seg_eq_dev, primary_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    if (num_segs) {
        SLAMEM_HIP(hipMemcpyAsync(&total, md_offsets_dev + num_segs, 8, hipMemcpyDeviceToHost, st));
        SLAMEM_HIP(hipStreamSynchronize(st));
    }
    *md_total = total;
    if (total > md_capacity) {
        set_error("slamem_maps_md_device: the batch has %llu MD entries, the buffer room for %llu", (unsigned long long)total,
                  (unsigned long long)md_capacity);
        return SLAMEM_ERR_CAPACITY;
    }
    return SLAMEM_OK;
}

// the MD pass over the arrays slamem_find_maps_host gave (uploaded again: this is the convenience path; a caller that minds the
// copies uses the device functions or a stream).  The entries' room is the sure bound, the sum of edits + the segments.
static int md_of_host_maps(const slamem_index* idx, uint32_t num_queries, const slamem_aln* segs, const uint64_t* read_offsets,
                           const uint32_t* ops, const uint64_t* op_offsets, const uint64_t* totals, uint32_t** md_out,
                           uint64_t** md_offsets_out, uint32_t** seg_eq_out, uint32_t** primary_out, uint64_t* md_total_out) {
    const uint64_t ns = totals[1], nops = totals[2];
    uint64_t cap = ns;
    for (uint64_t s = 0; s < ns; s++) cap += segs[s].edits;
    uint64_t ws_bytes = 0, total = 0;
    SLAMEM_TRY(slamem_maps_md_workspace_bytes(ns, num_queries, &ws_bytes));
    DevBuf<slamem_aln> d_segs;
    DevBuf<uint64_t> d_roff, d_ooff, d_moff;
    DevBuf<uint32_t> d_ops, d_md, d_eq, d_prim;
    DevBuf<char> d_ws;
    SLAMEM_HIP(hipSetDevice(idx->device));
    SLAMEM_TRY(d_segs.reserve(ns + 1));
    SLAMEM_TRY(d_roff.reserve((uint64_t)num_queries + 1));
    SLAMEM_TRY(d_ops.reserve(nops + 1));
    SLAMEM_TRY(d_ooff.reserve(ns + 1));
    SLAMEM_TRY(d_md.reserve(cap + 1));
    SLAMEM_TRY(d_moff.reserve(ns + 1));
    SLAMEM_TRY(d_eq.reserve(ns + 1));
    SLAMEM_TRY(d_prim.reserve((uint64_t)num_queries + 1));
    SLAMEM_TRY(d_ws.reserve(ws_bytes + 16));
    if (ns) SLAMEM_HIP(hipMemcpy(d_segs.get(), segs, ns * sizeof(slamem_aln), hipMemcpyHostToDevice));
    SLAMEM_HIP(hipMemcpy(d_roff.get(), read_offsets, ((uint64_t)num_queries + 1) * 8, hipMemcpyHostToDevice));
    if (nops) SLAMEM_HIP(hipMemcpy(d_ops.get(), ops, nops * 4, hipMemcpyHostToDevice));
    SLAMEM_HIP(hipMemcpy(d_ooff.get(), op_offsets, (ns + 1) * 8, hipMemcpyHostToDevice));
    SLAMEM_TRY(slamem_maps_md_device(idx, d_segs.get(), ns, d_roff.get(), num_queries, d_ops.get(), d_ooff.get(), d_md.get(), cap, d_moff.get(),
                                     d_eq.get(), d_prim.get(), d_ws.get(), ws_bytes, nullptr, &total));
    HostArray<uint32_t> h_md = host_array<uint32_t>(total + 1), h_eq = host_array<uint32_t>(ns + 1),
                        h_prim = host_array<uint32_t>((uint64_t)num_queries + 1);
    HostArray<uint64_t> h_moff = host_array<uint64_t>(ns + 1);
    if (!h_md || !h_moff || !h_eq || !h_prim) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    SLAMEM_HIP(hipDeviceSynchronize());
    if (total) SLAMEM_HIP(hipMemcpy(h_md.get(), d_md.get(), total * 4, hipMemcpyDeviceToHost));
    SLAMEM_HIP(hipMemcpy(h_moff.get(), d_moff.get(), (ns + 1) * 8, hipMemcpyDeviceToHost));
    if (ns) SLAMEM_HIP(hipMemcpy(h_eq.get(), d_eq.get(), ns * 4, hipMemcpyDeviceToHost));
    if (num_queries) SLAMEM_HIP(hipMemcpy(h_prim.get(), d_prim.get(), (uint64_t)num_queries * 4, hipMemcpyDeviceToHost));
    *md_out = h_md.release(); *md_offsets_out = h_moff.release(); *seg_eq_out = h_eq.release(); *primary_out = h_prim.release();
    *md_total_out = total;
    return SLAMEM_OK;
}

// slamem_find_maps_host, then the MD pass over its arrays; if the pass fails, the mapping's arrays go too
int slamem_find_maps_md_host(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries, uint32_t min_len,
                             int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits,
                             slamem_aln** segs_out, uint64_t** read_offsets_out, uint32_t** ops_out, uint64_t** op_offsets_out,
                             slamem_map** reads_out, uint64_t* totals_out, uint32_t** md_out, uint64_t** md_offsets_out,
                             uint32_t** seg_eq_out, uint32_t** primary_out, uint64_t* md_total_out) {
    return slamem_find_maps_md_host_gext(idx, queries, offsets, num_queries, min_len, both_strands, max_gap, mismatch_penalty, xdrop, max_edits,
                                         0, segs_out, read_offsets_out, ops_out, op_offsets_out, reads_out, totals_out, md_out, md_offsets_out,
                                         seg_eq_out, primary_out, md_total_out);
}

int slamem_find_maps_md_host_gext(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                                  uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop,
                                  uint32_t max_edits, uint32_t end_band, slamem_aln** segs_out, uint64_t** read_offsets_out,
                                  uint32_t** ops_out, uint64_t** op_offsets_out, slamem_map** reads_out, uint64_t* totals_out,
                                  uint32_t** md_out, uint64_t** md_offsets_out, uint32_t** seg_eq_out, uint32_t** primary_out,
                                  uint64_t* md_total_out) {
    if (!md_out || !md_offsets_out || !seg_eq_out || !primary_out || !md_total_out) {
        set_error("slamem_find_maps_md_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    *md_out = nullptr; *md_offsets_out = nullptr; *seg_eq_out = nullptr; *primary_out = nullptr; *md_total_out = 0;
    if (idx && !idx->view.tpl) {
        set_error("slamem_find_maps_md_host: the MD entries take the reference letters from the text planes of the index, and this "
                  "index has none (the compact layout, or one built with the seed sections switched off)");
        return SLAMEM_ERR_ARG;
    }
    int rc = slamem_find_maps_host_gext(idx, queries, offsets, num_queries, min_len, both_strands, max_gap, mismatch_penalty, xdrop, max_edits,
                                   end_band, segs_out, read_offsets_out, ops_out, op_offsets_out, reads_out, totals_out);
    if (rc != SLAMEM_OK) return rc;
    rc = md_of_host_maps(idx, num_queries, *segs_out, *read_offsets_out, *ops_out, *op_offsets_out, totals_out, md_out, md_offsets_out,
                         seg_eq_out, primary_out, md_total_out);
    if (rc != SLAMEM_OK) {
        slamem_host_free(*segs_out); slamem_host_free(*read_offsets_out); slamem_host_free(*ops_out); slamem_host_free(*op_offsets_out);
        slamem_host_free(*reads_out);
        *segs_out = nullptr; *read_offsets_out = nullptr; *ops_out = nullptr; *op_offsets_out = nullptr; *reads_out = nullptr;
    }
    return rc;
}

}  // extern "C"
