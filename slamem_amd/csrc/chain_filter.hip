// chain_filter.hip -- -chain (matchType 4): keep, of every strand block's -mem rows, the best collinear chain -- the rows a
// downstream aligner would join into one alignment -- and report its score.  DESIGN.md 4.12 has the definition; in short, with
// eq = q + L, ep = p + L and the maximum gap G:
//   j may precede i   iff  0 < q_i - q_j <= G,  0 < p_i - p_j <= G,  eq_j < eq_i,  ep_j < ep_i
//   link(j, i)        =    min(L_i, eq_i - eq_j, ep_i - ep_j) - |(p_i - q_i) - (p_j - q_j)|
//   f(i)              =    max(L_i, max over j that may precede i of f(j) + link(j, i))
// The predecessor of i is taken only if it gives more than L_i, the smallest index among the best; the chain ends in the row of
// the largest f, smallest index.  Both tie-breaks are one maximum of (score << 32) | ~index.  L_i <= f(i) <= eq_i: 32 bits.
//
// Inside a block the -mem rows come with the query start q descending (the emission order), so the rows that may
// precede row i lie BEHIND it in the list and, because q_i - q_j <= G, in one window that starts behind i's start group.  The
// DP therefore runs from the block's last row to its first, and row i scans forward until q_j < q_i - G.
//
// The filter runs on the -mem list K9 has placed in the workspace and writes the kept rows, in their order, to the caller's
// buffers -- all on the stream, no host read-back:
//   k_chain_lane        one lane per strand block of up to kChainLaneMax rows: pairs tested directly, f and the predecessors
//                       in the workspace (the lane reads back what it wrote: L1), then the backtrack; larger blocks go to a
//                       list (one atomic each)
//   k_chain_wave        a wave per listed block (a fixed grid of one-wave workgroups loops over the list): the rows and f of a
//                       tile of kChainTile rows in LDS, rows behind the tile and their f from global memory; per row the lanes
//                       share its window, the packed maximum is reduced with DPP and readlane, f and the predecessor go to
//                       LDS and, a tile at a time, to the workspace; then lane 0 walks the predecessors from the chain's end,
//                       staged in LDS tile by tile, and the lanes set the keep flags
//   scan                kept rows per block -> new block offsets (scan_sum_exclusive_u32_u64)
//   k_filter_copy / k_chain_list_copy  the kept rows, in order (listed blocks: a wave ranks 64 rows at a time with a ballot)
// Every row is checked against the one before it: a block out of the emission order fails the call (the highest-numbered
// such block, + 1, goes back with the batch's scalars: an atomic maximum) -- never wrong rows.
#include "filter_blocks.h"

namespace slamem {

namespace {

// A lane tests the pairs of blocks of up to this many rows: at most 496 pairs, of which a lane retires one in some tens of
// cycles, so the slowest lane holds its wave for tens of microseconds.  The work is quadratic: at 4.11's 256 rows one lane
// would hold its wave for milliseconds while a wave, which shares every window among 64 lanes, needs 256 short steps.
constexpr uint32_t kChainLaneMax = 32;
constexpr uint32_t kChainTile = 1024;     // rows of a listed block staged in LDS with f and predecessor: 20 KiB a wave, 8 waves a CU
constexpr unsigned kChainWaveGrid = 2048; // one-wave workgroups that share the list (8 per CU)
constexpr uint32_t kNoPred = 0xFFFFFFFFu;

struct ChainLayout : FilterPrefix {
    uint64_t off_f, off_pred, off_score, off_list, bytes;
};

ChainLayout chain_layout(uint64_t num_blocks, uint64_t capacity) {
    ChainLayout m;
    uint64_t off = m.begin(num_blocks, capacity);                                       // ctr: [0] listed blocks, [1] order violation
    m.off_f = off;      off = align_up(off + capacity * 4 + 16, 256);                   // f per -mem row
    m.off_pred = off;   off = align_up(off + capacity * 4 + 16, 256);                   // predecessor per -mem row (place in its block)
    m.off_score = off;  off = align_up(off + (num_blocks + 1) * 4, 256);                // block scores, when the caller wants none
    off = m.scan_at(off, num_blocks);
    m.off_list = off;   off = align_up(off + (capacity / (kChainLaneMax + 1) + 1) * 8, 256);  // listed strand blocks
    m.bytes = off;
    return m;
}

// f(j) + link(j, i) packed with j's place, or 0 when j may not precede i or gives no more than L_i.  dq = q_i - q_j is the
// caller's (it also ends the window).
__device__ __forceinline__ unsigned long long candidate(uint32_t pi, uint32_t li, uint32_t pj, uint32_t lj, uint32_t fj, int64_t dq,
                                                        int64_t gap, uint32_t j) {
    const int64_t dp = (int64_t)pi - (int64_t)pj;
    const int64_t de = (int64_t)li - (int64_t)lj;  // eq_i - eq_j = dq + de, ep_i - ep_j = dp + de
    const int64_t deq = dq + de, dep = dp + de;
    // (no early exit: the callers' loads stay unconditional and are issued together)
    const bool ok = (dq > 0) & (dq <= gap) & (dp > 0) & (dp <= gap) & (deq > 0) & (dep > 0);
    int64_t add = (int64_t)li;
    add = deq < add ? deq : add;
    add = dep < add ? dep : add;
    const int64_t drift = dp > dq ? dp - dq : dq - dp;
    const int64_t sc = (int64_t)fj + add - drift;
    const unsigned long long key = ((unsigned long long)sc << 32) | (unsigned long long)(~j);
    return (ok & (sc > (int64_t)li)) ? key : 0ull;
}

// one lane per strand block (and lane num_blocks keeps the scan's last input at 0)
__global__ void __launch_bounds__(256) k_chain_lane(const uint64_t* __restrict__ boff, uint64_t nb, const slamem_mem* __restrict__ rows,
                                                    uint64_t cap, uint32_t max_gap, uint32_t* __restrict__ cnt, uint8_t* __restrict__ keep,
                                                    uint32_t* f, uint32_t* pred, uint32_t* __restrict__ score,
                                                    uint64_t* __restrict__ list, unsigned long long* __restrict__ ctr) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b > nb) return;
    if (b == nb) { cnt[nb] = 0u; return; }
    uint64_t s, e;
    clamp_block(boff, b, cap, s, e);
    const uint32_t n = (uint32_t)(e - s);
    if (n > kChainLaneMax) {
        cnt[b] = 0u;  // (k_chain_wave writes it, and the score)
        list[atomicAdd(&ctr[0], 1ull)] = b;
        return;
    }
    if (n == 0u) { cnt[b] = 0u; score[b] = 0u; return; }
    const slamem_mem* R = rows + s;
    if (n == 1u) {  // (most blocks of a read batch)
        keep[s] = 1u;
        cnt[b] = 1u;
        score[b] = R[0].length;
        return;
    }
    uint32_t* F = f + s;
    uint32_t* P = pred + s;
    const int64_t gap = (int64_t)max_gap;
    unsigned long long end = 0;
    bool bad = false;
    for (uint32_t i = n; i-- > 0;) {
        const slamem_mem ri = R[i];
        unsigned long long best = 0;
        for (uint32_t j = i + 1; j < n; j++) {
            const slamem_mem rj = R[j];
            if (j == i + 1 && out_of_order(ri, rj)) bad = true;
            const int64_t dq = (int64_t)ri.query_pos - (int64_t)rj.query_pos;
            if (dq > gap) break;
            const unsigned long long c = candidate(ri.ref_pos, ri.length, rj.ref_pos, rj.length, F[j], dq, gap, j);
            if (c > best) best = c;
        }
        const uint32_t fi = best ? (uint32_t)(best >> 32) : ri.length;
        F[i] = fi;
        P[i] = best ? ~(uint32_t)best : kNoPred;
        keep[s + i] = 0u;
        const unsigned long long k = ((unsigned long long)fi << 32) | (unsigned long long)(~i);
        if (k > end) end = k;
    }
    uint32_t kept = 0;
    for (uint32_t i = ~(uint32_t)end; i < n; i = P[i]) {  // (kNoPred ends it: predecessors lie behind their row)
        keep[s + i] = 1u;
        kept++;
    }
    if (bad) {
        atomicMax(&ctr[1], (unsigned long long)b + 1ull);
        kept = 0u;
    }
    cnt[b] = kept;
    score[b] = bad ? 0u : (uint32_t)(end >> 32);
}

// ---- listed blocks: a wave each -------------------------------------------------------------------------------------------

// The maximum over the wave's 64 lanes, in every lane (all lanes active).  Four DPP steps make it uniform in each row of 16
// lanes (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror); the four rows meet through readlane.
template <int kCtrl>
__device__ __forceinline__ unsigned long long dpp_max_step(unsigned long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, kCtrl, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), kCtrl, 0xF, 0xF, true);
    const unsigned long long o = ((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo;
    return o > v ? o : v;
}

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int lane) {
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane) << 32) |
           (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    v = dpp_max_step<0xB1>(v);
    v = dpp_max_step<0x4E>(v);
    v = dpp_max_step<0x141>(v);
    v = dpp_max_step<0x140>(v);
    const unsigned long long a = readlane_u64(v, 0), b = readlane_u64(v, 16), c = readlane_u64(v, 32), d = readlane_u64(v, 48);
    const unsigned long long ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

// a one-wave workgroup per listed block; the grid loops over the list
__global__ void __launch_bounds__(64) k_chain_wave(const uint64_t* __restrict__ list, const unsigned long long* __restrict__ ctr_in,
                                                   const uint64_t* __restrict__ boff, const slamem_mem* __restrict__ rows, uint64_t cap,
                                                   uint32_t max_gap, uint8_t* __restrict__ keep, uint32_t* f, uint32_t* pred,
                                                   uint32_t* __restrict__ cnt, uint32_t* __restrict__ score,
                                                   unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t sp[kChainTile], sq[kChainTile], sl[kChainTile], sf[kChainTile], sv[kChainTile];
    const uint32_t lane = threadIdx.x;
    const uint64_t nl = ctr_in[0];
    const int64_t gap = (int64_t)max_gap;
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t b = list[li];
        uint64_t s, e;
        clamp_block(boff, b, cap, s, e);
        const uint32_t n = (uint32_t)(e - s);
        const slamem_mem* R = rows + s;
        uint32_t* F = f + s;
        uint32_t* P = pred + s;
        uint8_t* K = keep + s;
        bool bad = false;
        unsigned long long end = 0;
        // tiles from the block's end to its start; inside a tile, rows from its end to its start
        for (uint32_t hi = n; hi > 0;) {
            const uint32_t t0 = hi > kChainTile ? hi - kChainTile : 0u;
            __syncthreads();  // the f of the tiles behind are in global memory, and nobody reads the old tile any more
            for (uint32_t k = t0 + lane; k < hi; k += 64u) {
                const slamem_mem r = R[k];
                if (k + 1u < n && out_of_order(r, R[k + 1u])) bad = true;
                sp[k - t0] = r.ref_pos;
                sq[k - t0] = r.query_pos;
                sl[k - t0] = r.length;
                K[k] = 0u;
            }
            __syncthreads();
            for (uint32_t i = hi; i-- > t0;) {
                const uint32_t pi = sp[i - t0], qi = sq[i - t0], len = sl[i - t0];
                unsigned long long best = 0;
                for (uint32_t base = i + 1u; base < n; base += 64u) {
                    const uint32_t j = base + lane;
                    uint32_t pj, qj, lj, fj;
                    if (base + 64u <= hi) {  // (uniform) the 64 rows lie in the tile
                        const uint32_t k = j - t0;
                        pj = sp[k]; qj = sq[k]; lj = sl[k]; fj = sf[k];
                    } else {
                        // some lie behind the tile, or behind the block: both reads at a place that exists, then the choice
                        const bool tile = j < hi;
                        const uint32_t k = tile ? j - t0 : 0u, g = j < n ? j : n - 1u;
                        const slamem_mem rj = R[g];
                        const uint32_t fg = F[g];
                        pj = tile ? sp[k] : rj.ref_pos;
                        qj = tile ? sq[k] : rj.query_pos;
                        lj = tile ? sl[k] : rj.length;
                        fj = tile ? sf[k] : fg;
                    }
                    const int64_t dq = (int64_t)qi - (int64_t)qj;
                    const unsigned long long c = j < n ? candidate(pi, len, pj, lj, fj, dq, gap, j) : 0ull;
                    if (c > best) best = c;
                    // (q only falls behind row i: no row past the first one beyond the gap counts)
                    if (__any(j >= n || dq > gap)) break;
                }
                best = wave_max_u64(best);
                const uint32_t fi = best ? (uint32_t)(best >> 32) : len;
                // every lane stores the same word, so each lane's later read of it follows its own store.  (No global store
                // here: the next row's loads would wait for it.)
                sf[i - t0] = fi;
                sv[i - t0] = best ? ~(uint32_t)best : kNoPred;
                const unsigned long long k = ((unsigned long long)fi << 32) | (unsigned long long)(~i);
                if (k > end) end = k;
            }
            __syncthreads();
            for (uint32_t k = t0 + lane; k < hi; k += 64u) {  // the tile's f (for the tiles in front) and predecessors
                F[k] = sf[k - t0];
                P[k] = sv[k - t0];
            }
            hi = t0;
        }
        const int any_bad = __syncthreads_or(bad ? 1 : 0);  // (and the flags and predecessors are visible to every lane)
        // the backtrack, a tile at a time from the chain's end: the lanes stage the predecessors of the kChainTile rows
        // behind the current row in LDS, lane 0 walks them there (a chain mostly steps to a row nearby: a dependent LDS read
        // a step instead of a dependent global one), the lanes write the flags
        uint32_t kept = 0;
        for (uint32_t cur = any_bad ? n : ~(uint32_t)end; cur < n;) {
            const uint32_t tn = n - cur < kChainTile ? n - cur : kChainTile;
            __syncthreads();
            for (uint32_t k = lane; k < tn; k += 64u) {
                sp[k] = P[cur + k];
                sq[k] = 0u;
            }
            __syncthreads();
            if (lane == 0u) {
                uint32_t i = cur;
                while (i - cur < tn) {  // (kNoPred ends it: predecessors lie behind their row)
                    sq[i - cur] = 1u;
                    kept++;
                    i = sp[i - cur];
                }
                sf[0] = i;
            }
            __syncthreads();
            for (uint32_t k = lane; k < tn; k += 64u)
                if (sq[k]) K[cur + k] = 1u;
            cur = sf[0];
        }
        if (lane == 0u) {
            cnt[b] = kept;
            score[b] = any_bad ? 0u : (uint32_t)(end >> 32);
            if (any_bad) atomicMax(&ctr[1], (unsigned long long)b + 1ull);
        }
    }
}

// a listed block's kept rows, in order: a wave ranks 64 rows at a time
__global__ void __launch_bounds__(64) k_chain_list_copy(const uint64_t* __restrict__ list, const unsigned long long* __restrict__ ctr,
                                                        const uint64_t* __restrict__ boff, uint64_t cap, const slamem_mem* __restrict__ rows,
                                                        const uint8_t* __restrict__ keep, const uint32_t* __restrict__ cnt,
                                                        const uint64_t* __restrict__ newoff, slamem_mem* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const uint64_t nl = ctr[0];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t b = list[li];
        if (cnt[b] == 0u) continue;  // (uniform: the block was out of order)
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
                if (at < cap) out[at] = rows[s + i];
            }
            d += (uint64_t)__popcll(m);
        }
    }
}

}  // namespace

uint64_t chain_workspace_bytes(const FilterBatch& b, const FilterParams&) { return chain_layout(b.num_blocks(), b.capacity).bytes; }

#define CSTEP(call, what) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(e__, what, __FILE__, __LINE__); } while (0)

ChainBufs chain_buffers(void* ws, uint64_t num_blocks, uint64_t capacity) {
    const ChainLayout m = chain_layout(num_blocks, capacity);
    const FilterBufs w = filter_bufs(ws, m);
    char* p = static_cast<char*>(ws);
    return ChainBufs{w.ctr, w.rows, w.boff, w.cnt, w.keep, reinterpret_cast<uint32_t*>(p + m.off_score),
                     reinterpret_cast<uint64_t*>(p + m.off_list), w.scan, w.scan_bytes, kChainLaneMax, kChainWaveGrid};
}

// the DP and the backtrack: keep flags, kept rows and score per block
int chain_pass(void* ws, uint64_t num_blocks, uint64_t capacity, uint32_t max_gap, uint32_t* out_scores, hipStream_t stream) {
    const ChainLayout m = chain_layout(num_blocks, capacity);
    const FilterBufs w = filter_bufs(ws, m);
    char* p = static_cast<char*>(ws);
    uint32_t* f = reinterpret_cast<uint32_t*>(p + m.off_f);
    uint32_t* pred = reinterpret_cast<uint32_t*>(p + m.off_pred);
    uint32_t* score = out_scores ? out_scores : reinterpret_cast<uint32_t*>(p + m.off_score);
    uint64_t* list = reinterpret_cast<uint64_t*>(p + m.off_list);
    CSTEP(hipMemsetAsync(w.ctr, 0, 16, stream), "memset");
    hipLaunchKernelGGL(k_chain_lane, dim3(grid_for(num_blocks + 1)), dim3(256), 0, stream, (const uint64_t*)w.boff, num_blocks,
                       (const slamem_mem*)w.rows, capacity, max_gap, w.cnt, w.keep, f, pred, score, list, w.ctr);
    CSTEP(hipGetLastError(), "k_chain_lane");
    hipLaunchKernelGGL(k_chain_wave, dim3(kChainWaveGrid), dim3(64), 0, stream, (const uint64_t*)list, (const unsigned long long*)w.ctr,
                       (const uint64_t*)w.boff, (const slamem_mem*)w.rows, capacity, max_gap, w.keep, f, pred, w.cnt, score, w.ctr);
    CSTEP(hipGetLastError(), "k_chain_wave");
    return SLAMEM_OK;
}

// the kept rows of chain_pass, in their order, with new block offsets
int chain_compact(void* ws, uint64_t num_blocks, uint64_t capacity, slamem_mem* out_mems, uint64_t* out_boff,
                  unsigned long long* host_scalars, hipStream_t stream) {
    const ChainLayout m = chain_layout(num_blocks, capacity);
    const FilterBufs w = filter_bufs(ws, m);
    uint64_t* list = reinterpret_cast<uint64_t*>(static_cast<char*>(ws) + m.off_list);
    CSTEP(compact_kept<kChainLaneMax>(w, num_blocks, capacity, w.rows, out_mems, out_boff, stream), "compact_kept");
    hipLaunchKernelGGL(k_chain_list_copy, dim3(kChainWaveGrid), dim3(64), 0, stream, (const uint64_t*)list,
                       (const unsigned long long*)w.ctr, (const uint64_t*)w.boff, capacity, (const slamem_mem*)w.rows,
                       (const uint8_t*)w.keep, (const uint32_t*)w.cnt, (const uint64_t*)w.newoff, out_mems);
    CSTEP(hipGetLastError(), "k_chain_list_copy");
    CSTEP(kept_scalars(w, num_blocks, w.ctr + 1, host_scalars, stream), "memcpy");
    return SLAMEM_OK;
}

int chain_filter(void* ws, const FilterBatch& b, const FilterParams& p, slamem_mem* out_mems, uint64_t* out_boff,
                 unsigned long long* host_scalars, hipStream_t stream) {
    const int rc = chain_pass(ws, b.num_blocks(), b.capacity, p.max_gap, p.column_dev, stream);
    if (rc != SLAMEM_OK) return rc;
    return chain_compact(ws, b.num_blocks(), b.capacity, out_mems, out_boff, host_scalars, stream);
}
#undef CSTEP

}  // namespace slamem
