// smem_filter.hip -- -smem (matchType 3): keep the -mem rows of a strand block whose query interval no other row of the same
// block strictly contains -- the super-maximal exact matches read mappers seed with -- and, with an occurrence cap N
// (max_occ > 0), drop the SMEM rows whose query interval more than N rows of the block share (all copies together).
// DESIGN.md 4.11 has the definition and why, given the complete -mem list, it equals counting in the merged text.
//
// Inside a block the -mem rows come in the reference's emission order (slamem.c:114-193): query start q descending, then
// length L non-increasing; rows of equal (q, L) are adjacent (a "run": the occurrences of one interval).  So a row is strictly
// contained iff
//   (a) the first row of its start group (same q) is longer than it, or
//   (b) a row of a later start group (smaller q) ends at or beyond its end.
// With A = (~q, L) and B = (q + L, L), compared lexicographically, (a) is "the maximum A before the row is > its A" and (b) is
// "the maximum B after the row is > its B" (a row of its own run has the same B; a shorter row of its own group ends
// earlier; a later group's row that ends at the same place is longer).  Ends are 64-bit.
//
// The filter runs on the -mem list K9 has placed in the workspace and writes the kept rows, in their order, to the caller's
// buffers -- all on the stream, no host read-back:
//   k_smem_lane         one lane per strand block of up to kSmemLaneMax rows walks it backwards, a start group at a time;
//                       larger blocks go to a list (one atomic each)
//   k_smem_large        a workgroup per listed block (a fixed grid loops over the list): a forward pass (prefix max of A;
//                       with a cap, the start of each row's run) and a backward pass (suffix max of B; with a cap, the end
//                       of each row's run), in tiles of kSmemTile rows: kSmemItems consecutive rows a thread, a wave scan
//                       of the threads' aggregates, the running value carried from tile to tile
//   scan                kept rows per block -> new block offsets (scan_sum_exclusive_u32_u64)
//   k_filter_copy / k_smem_large_copy the kept rows, in order (large blocks: tiles ranked by a workgroup scan)
// Every row is checked against the one before it (one compare): a block out of that order fails the call (the highest-numbered
// such block, + 1, goes back with the batch's scalars: an atomic maximum) -- never wrong rows.
#include "filter_blocks.h"

namespace slamem {

namespace {

// a lane walks blocks of up to this many rows (two reads of each, L1-resident); reads at -l 20 have a handful
constexpr uint32_t kSmemLaneMax = 256;
constexpr uint32_t kSmemWg = 256, kSmemItems = 8, kSmemTile = kSmemWg * kSmemItems;
constexpr unsigned kSmemLargeGrid = 256;  // workgroups that share the list of large blocks (one per CU)

struct SmemLayout : FilterPrefix {
    uint64_t off_rstart, off_large, bytes;
};

SmemLayout smem_layout(uint64_t num_blocks, uint64_t capacity) {
    SmemLayout m;
    uint64_t off = m.begin(num_blocks, capacity);                                       // ctr: [0] large blocks, [1] order violation
    m.off_rstart = off; off = align_up(off + capacity * 4 + 16, 256);                   // large blocks, with a cap: run starts
    off = m.scan_at(off, num_blocks);
    m.off_large = off;  off = align_up(off + (capacity / (kSmemLaneMax + 1) + 1) * 8, 256);  // listed strand blocks
    m.bytes = off;
    return m;
}

__device__ __forceinline__ bool same_interval(const slamem_mem& x, const slamem_mem& y) {
    return x.query_pos == y.query_pos && x.length == y.length;
}

// one lane per strand block (and lane num_blocks keeps the scan's last input at 0)
__global__ void __launch_bounds__(256) k_smem_lane(const uint64_t* __restrict__ boff, uint64_t nb, const slamem_mem* __restrict__ rows,
                                                   uint64_t cap, uint32_t max_occ, uint32_t* __restrict__ cnt, uint8_t* __restrict__ keep,
                                                   uint64_t* __restrict__ large, unsigned long long* __restrict__ ctr) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b > nb) return;
    if (b == nb) { cnt[nb] = 0u; return; }
    uint64_t s, e;
    clamp_block(boff, b, cap, s, e);
    const uint32_t n = (uint32_t)(e - s);
    if (n > kSmemLaneMax) {
        cnt[b] = 0u;  // (k_smem_large writes it)
        large[atomicAdd(&ctr[0], 1ull)] = b;
        return;
    }
    const slamem_mem* R = rows + s;
    uint64_t max_after = 0;  // the largest end among the start groups behind the current one (every end is >= 1)
    uint32_t kept = 0, i = n;
    bool bad = false;
    while (i > 0) {
        // the start group [g, i): rows of one q, longest first
        const uint32_t q = R[i - 1].query_pos;
        uint32_t g = i - 1;
        while (g > 0 && R[g - 1].query_pos == q) g--;
        if (g > 0 && R[g - 1].query_pos < q) bad = true;
        const uint32_t lmax = R[g].length;
        for (uint32_t k = g; k < i;) {
            const uint32_t len = R[k].length;
            if (k > g && len > R[k - 1].length) bad = true;
            uint32_t k1 = k + 1;
            while (k1 < i && R[k1].length == len) k1++;
            const bool in = len < lmax || max_after >= (uint64_t)q + len;
            const bool keep_run = !in && (max_occ == 0u || k1 - k <= max_occ);
            for (uint32_t j = k; j < k1; j++) keep[s + j] = keep_run ? 1u : 0u;
            kept += keep_run ? k1 - k : 0u;
            k = k1;
        }
        const uint64_t end = (uint64_t)q + lmax;
        if (end > max_after) max_after = end;
        i = g;
    }
    if (bad) {
        atomicMax(&ctr[1], (unsigned long long)b + 1ull);
        kept = 0u;
    }
    cnt[b] = kept;
}

// ---- large blocks ----------------------------------------------------------------------------------------------------------

struct Key2 {  // compared lexicographically
    unsigned long long hi;
    uint32_t lo;
};

__device__ __forceinline__ bool key_less(const Key2& x, const Key2& y) { return x.hi < y.hi || (x.hi == y.hi && x.lo < y.lo); }
__device__ __forceinline__ Key2 key_max(const Key2& x, const Key2& y) { return key_less(x, y) ? y : x; }

// Exclusive max over the workgroup's threads (in thread order) of one key each, after `carry` (the tiles before);
// carry becomes the maximum over everything so far.  Called by every thread of the workgroup.
__device__ Key2 wg_exclusive_max(Key2 v, Key2* lds, Key2& carry) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    Key2 incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        Key2 o;
        o.hi = __shfl_up(incl.hi, d);
        o.lo = __shfl_up(incl.lo, d);
        if ((int)lane >= d) incl = key_max(incl, o);
    }
    Key2 up;
    up.hi = __shfl_up(incl.hi, 1);
    up.lo = __shfl_up(incl.lo, 1);
    if (lane == 63u) lds[w] = incl;
    __syncthreads();
    Key2 excl = carry;
    for (uint32_t q = 0; q < w; q++) excl = key_max(excl, lds[q]);
    if (lane) excl = key_max(excl, up);
    for (uint32_t q = 0; q < kSmemWg / 64u; q++) carry = key_max(carry, lds[q]);
    __syncthreads();
    return excl;
}

// Exclusive sum over the workgroup's threads, after `carry`; carry becomes the sum so far.
__device__ uint64_t wg_exclusive_sum(uint32_t v, uint32_t* lds, uint64_t& carry) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if ((int)lane >= d) incl += o;
    }
    if (lane == 63u) lds[w] = incl;
    __syncthreads();
    uint64_t excl = carry + incl - v;
    for (uint32_t q = 0; q < w; q++) excl += lds[q];
    for (uint32_t q = 0; q < kSmemWg / 64u; q++) carry += lds[q];
    __syncthreads();
    return excl;
}

__device__ __forceinline__ Key2 key_a(const slamem_mem& r) { return Key2{0xFFFFFFFFull - r.query_pos, r.length}; }
__device__ __forceinline__ Key2 key_b(const slamem_mem& r) { return Key2{(unsigned long long)r.query_pos + r.length, r.length}; }

// a workgroup per listed block; the grid loops over the list
__global__ void __launch_bounds__(kSmemWg) k_smem_large(const uint64_t* __restrict__ large, const unsigned long long* __restrict__ ctr_in,
                                                        const uint64_t* __restrict__ boff, const slamem_mem* __restrict__ rows, uint64_t cap,
                                                        uint32_t max_occ, uint8_t* __restrict__ keep, uint32_t* __restrict__ rstart,
                                                        uint32_t* __restrict__ cnt, unsigned long long* __restrict__ ctr) {
    __shared__ Key2 lds[kSmemWg / 64u];
    __shared__ uint32_t kept_total;
    const uint64_t nl = ctr_in[0];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t b = large[li];
        uint64_t s, e;
        clamp_block(boff, b, cap, s, e);
        const uint32_t n = (uint32_t)(e - s);
        const slamem_mem* R = rows + s;
        bool bad = false;
        uint32_t mine = 0;
        __syncthreads();
        if (threadIdx.x == 0) kept_total = 0;
        // forward: (a), and the start of each row's run
        Key2 carry_a{0, 0}, carry_s{0, 0};
        for (uint32_t t0 = 0; t0 < n; t0 += kSmemTile) {
            const uint32_t base = t0 + threadIdx.x * kSmemItems;
            slamem_mem r[kSmemItems];
#pragma unroll
            for (uint32_t k = 0; k < kSmemItems; k++)
                if (base + k < n) r[k] = R[base + k];
            slamem_mem prev = r[0];
            if (base > 0 && base < n) prev = R[base - 1];
            Key2 ex_a[kSmemItems];
            Key2 run_a{0, 0}, run_s{0, 0};
            uint32_t rs[kSmemItems];
#pragma unroll
            for (uint32_t k = 0; k < kSmemItems; k++) {
                const uint32_t i = base + k;
                ex_a[k] = run_a;
                rs[k] = 0;
                if (i < n) {
                    const slamem_mem& p = k ? r[k - 1] : prev;
                    if (i > 0 && out_of_order(p, r[k])) bad = true;
                    run_a = key_max(run_a, key_a(r[k]));
                    if (i == 0 || !same_interval(p, r[k])) run_s = key_max(run_s, Key2{i, 0});
                    rs[k] = (uint32_t)run_s.hi;
                }
            }
            const Key2 before_a = wg_exclusive_max(run_a, lds, carry_a);
            Key2 before_s{0, 0};
            if (max_occ) before_s = wg_exclusive_max(run_s, lds, carry_s);
#pragma unroll
            for (uint32_t k = 0; k < kSmemItems; k++) {
                const uint32_t i = base + k;
                if (i >= n) break;
                keep[s + i] = key_less(key_a(r[k]), key_max(before_a, ex_a[k])) ? 0u : 1u;
                // (a run that starts in an earlier thread's rows: its start is the latest start flagged before them)
                if (max_occ) rstart[s + i] = (uint32_t)key_max(before_s, Key2{rs[k], 0}).hi;
            }
        }
        __syncthreads();  // (keep and rstart of this block are read by other threads below)
        // backward: (b), and the end of each row's run; thread order runs from the block's last row to its first
        Key2 carry_b{0, 0}, carry_e{0, 0};
        for (uint32_t t0 = 0; t0 < n; t0 += kSmemTile) {
            const uint32_t base = t0 + threadIdx.x * kSmemItems;  // in reversed order: row n - 1 - (base + k)
            slamem_mem r[kSmemItems];
#pragma unroll
            for (uint32_t k = 0; k < kSmemItems; k++)
                if (base + k < n) r[k] = R[n - 1u - (base + k)];
            slamem_mem next = r[0];
            if (base > 0 && base < n) next = R[n - base];
            Key2 ex_b[kSmemItems];
            Key2 run_b{0, 0}, run_e{0, 0};
            uint32_t re[kSmemItems];
#pragma unroll
            for (uint32_t k = 0; k < kSmemItems; k++) {
                const uint32_t j = base + k;  // reversed position; the row is n - 1 - j
                ex_b[k] = run_b;
                re[k] = 0;
                if (j < n) {
                    const slamem_mem& nx = k ? r[k - 1] : next;
                    run_b = key_max(run_b, key_b(r[k]));
                    if (j == 0 || !same_interval(nx, r[k])) run_e = key_max(run_e, Key2{j, 0});
                    re[k] = (uint32_t)run_e.hi;
                }
            }
            const Key2 before_b = wg_exclusive_max(run_b, lds, carry_b);
            Key2 before_e{0, 0};
            if (max_occ) before_e = wg_exclusive_max(run_e, lds, carry_e);
#pragma unroll
            for (uint32_t k = 0; k < kSmemItems; k++) {
                const uint32_t j = base + k;
                if (j >= n) break;
                const uint32_t i = n - 1u - j;
                bool kp = keep[s + i] && !key_less(key_b(r[k]), key_max(before_b, ex_b[k]));
                if (max_occ && kp) {
                    const uint32_t last = n - 1u - (uint32_t)key_max(before_e, Key2{re[k], 0}).hi;  // the run's last row
                    kp = last - rstart[s + i] + 1u <= max_occ;
                }
                keep[s + i] = kp ? 1u : 0u;
                mine += kp ? 1u : 0u;
            }
        }
        atomicAdd(&kept_total, mine);
        const int any_bad = __syncthreads_or(bad ? 1 : 0);
        if (threadIdx.x == 0) {
            cnt[b] = any_bad ? 0u : kept_total;
            if (any_bad) atomicMax(&ctr[1], (unsigned long long)b + 1ull);
        }
    }
}

// a listed block's kept rows, in order: tiles of kSmemTile rows ranked with a workgroup scan
__global__ void __launch_bounds__(kSmemWg) k_smem_large_copy(const uint64_t* __restrict__ large, const unsigned long long* __restrict__ ctr,
                                                             const uint64_t* __restrict__ boff, uint64_t cap, const slamem_mem* __restrict__ rows,
                                                             const uint8_t* __restrict__ keep, const uint32_t* __restrict__ cnt,
                                                             const uint64_t* __restrict__ newoff, slamem_mem* __restrict__ out) {
    __shared__ uint32_t lds[kSmemWg / 64u];
    const uint64_t nl = ctr[0];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t b = large[li];
        if (cnt[b] == 0u) continue;  // (uniform: nothing kept, or the block was out of order)
        uint64_t s, e;
        clamp_block(boff, b, cap, s, e);
        const uint32_t n = (uint32_t)(e - s);
        uint64_t carry = newoff[b];
        for (uint32_t t0 = 0; t0 < n; t0 += kSmemTile) {
            const uint32_t base = t0 + threadIdx.x * kSmemItems;
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t k = 0; k < kSmemItems; k++)
                if (base + k < n) mine += keep[s + base + k];
            uint64_t d = wg_exclusive_sum(mine, lds, carry);
#pragma unroll
            for (uint32_t k = 0; k < kSmemItems; k++) {
                if (base + k < n && keep[s + base + k]) {
                    if (d < cap) out[d] = rows[s + base + k];
                    d++;
                }
            }
        }
    }
}

}  // namespace

uint64_t smem_workspace_bytes(const FilterBatch& b, const FilterParams&) { return smem_layout(b.num_blocks(), b.capacity).bytes; }

#define SSTEP(call, what) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(e__, what, __FILE__, __LINE__); } while (0)

int smem_filter(void* ws, const FilterBatch& b, const FilterParams& p, slamem_mem* out_mems, uint64_t* out_boff,
                unsigned long long* host_scalars, hipStream_t stream) {
    const uint64_t num_blocks = b.num_blocks(), capacity = b.capacity;
    const SmemLayout m = smem_layout(num_blocks, capacity);
    const FilterBufs w = filter_bufs(ws, m);
    uint32_t* rstart = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + m.off_rstart);
    uint64_t* large = reinterpret_cast<uint64_t*>(static_cast<char*>(ws) + m.off_large);
    SSTEP(hipMemsetAsync(w.ctr, 0, 16, stream), "memset");
    hipLaunchKernelGGL(k_smem_lane, dim3(grid_for(num_blocks + 1)), dim3(256), 0, stream, (const uint64_t*)w.boff, num_blocks,
                       (const slamem_mem*)w.rows, capacity, p.max_occ, w.cnt, w.keep, large, w.ctr);
    SSTEP(hipGetLastError(), "k_smem_lane");
    hipLaunchKernelGGL(k_smem_large, dim3(kSmemLargeGrid), dim3(kSmemWg), 0, stream, (const uint64_t*)large, (const unsigned long long*)w.ctr,
                       (const uint64_t*)w.boff, (const slamem_mem*)w.rows, capacity, p.max_occ, w.keep, rstart, w.cnt, w.ctr);
    SSTEP(hipGetLastError(), "k_smem_large");
    SSTEP(compact_kept<kSmemLaneMax>(w, num_blocks, capacity, w.rows, out_mems, out_boff, stream), "compact_kept");
    hipLaunchKernelGGL(k_smem_large_copy, dim3(kSmemLargeGrid), dim3(kSmemWg), 0, stream, (const uint64_t*)large,
                       (const unsigned long long*)w.ctr, (const uint64_t*)w.boff, capacity, (const slamem_mem*)w.rows,
                       (const uint8_t*)w.keep, (const uint32_t*)w.cnt, (const uint64_t*)w.newoff, out_mems);
    SSTEP(hipGetLastError(), "k_smem_large_copy");
    SSTEP(kept_scalars(w, num_blocks, w.ctr + 1, host_scalars, stream), "memcpy");
    return SLAMEM_OK;
}
#undef SSTEP

}  // namespace slamem
