// filter_shared.h -- what the filters behind K9 that read letters share (ext_filter.hip, aln_filter.hip): the batch as
// bit-planes (k_ext_units / k_ext_pack / k_ext_pack_long), the 64-letter windows of a strand and of the text and the X-drop
// walk over a mismatch mask, on top of filter_blocks.h.  Everything sits in an unnamed namespace: each file that includes this
// gets its own kernels.
#pragma once
#include "filter_blocks.h"

namespace slamem {

namespace {

constexpr uint32_t kExtPackLaneUnits = 16;  // units (of 64 letters) of a record one lane packs
constexpr unsigned kExtPackGrid = 1024;     // workgroups that share the list of longer records

// a unit of a packed record: the layout of TextPlanes without the occurs-once plane
struct __attribute__((aligned(32))) QueryUnit { uint64_t p0, p1, nm, pad; };
static_assert(sizeof(QueryUnit) == 32 && sizeof(TextPlanes) == 32, "units are two 16-byte loads");

// ---- the batch as planes -------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_ext_units(const uint64_t* __restrict__ offsets, uint64_t nq, uint32_t* __restrict__ ucnt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i > nq) return;
    ucnt[i] = i < nq ? (uint32_t)((offsets[i + 1] - offsets[i] + 63u) >> 6) : 0u;
}

// letters [at, at + 64) of a record of `len` letters that starts at byte address `rec` -> one unit.  Whole aligned 8-byte words
// are read, and only words that hold a letter of the record (the batch is readable up to the next multiple of 16 bytes).
__device__ __forceinline__ void pack_unit(uintptr_t rec, uint64_t len, uint64_t at, QueryUnit* __restrict__ out) {
    const uintptr_t first = rec + at, end = rec + len;
    const uint64_t* W = reinterpret_cast<const uint64_t*>(first & ~(uintptr_t)7);
    const uint32_t sh = (uint32_t)(first & 7u) * 8u;
    const uint64_t valid = len - at < 64u ? len - at : 64u;  // letters of this unit
    uint64_t p0 = 0, p1 = 0, nm = 0;
    uint64_t w = W[0];  // (holds the letter at `first`)
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) {
        const bool more = reinterpret_cast<uintptr_t>(W + k + 1u) < end;
        const uint64_t nx = more ? W[k + 1u] : 0ull;
        const uint64_t x = sh ? (w >> sh) | (nx << (64u - sh)) : w;  // letters 8k .. 8k+7 of the unit, the first in the lowest byte
        w = nx;
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) {
            const uint32_t u = (uint32_t)(x >> (8u * i)) & 0xDFu;        // (the classes of the search: case folded)
            const uint32_t y = (u >> 1) & 3u, code = y ^ (y >> 1);       // A 0, C 1, G 2, T 3
            const bool ok = ((0x54474341u >> (8u * code)) & 0xFFu) == u && 8u * k + i < valid;
            p0 |= (uint64_t)(ok ? code & 1u : 0u) << (8u * k + i);
            p1 |= (uint64_t)(ok ? code >> 1 : 0u) << (8u * k + i);
            nm |= (uint64_t)(ok ? 0u : 1u) << (8u * k + i);
        }
    }
    uint4* o = reinterpret_cast<uint4*>(out);
    o[0] = make_uint4((uint32_t)p0, (uint32_t)(p0 >> 32), (uint32_t)p1, (uint32_t)(p1 >> 32));
    o[1] = make_uint4((uint32_t)nm, (uint32_t)(nm >> 32), 0u, 0u);
}

// one lane per record; longer records go to a list (one atomic each)
__global__ void __launch_bounds__(256) k_ext_pack(const char* __restrict__ queries, const uint64_t* __restrict__ offsets, uint64_t nq,
                                                  const uint64_t* __restrict__ uoff, QueryUnit* __restrict__ units,
                                                  uint64_t* __restrict__ longs, unsigned long long* __restrict__ ctr) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= nq) return;
    const uint64_t o = offsets[r], len = offsets[r + 1] - o;
    const uint64_t nu = (len + 63u) >> 6;
    if (nu > kExtPackLaneUnits) { longs[atomicAdd(&ctr[2], 1ull)] = r; return; }
    const uintptr_t rec = reinterpret_cast<uintptr_t>(queries) + o;
    QueryUnit* U = units + uoff[r];
    for (uint64_t u = 0; u < nu; u++) pack_unit(rec, len, 64u * u, U + u);
}

// a workgroup per listed record (a fixed grid loops over the list), a lane per unit
__global__ void __launch_bounds__(256) k_ext_pack_long(const char* __restrict__ queries, const uint64_t* __restrict__ offsets,
                                                       const uint64_t* __restrict__ uoff, QueryUnit* __restrict__ units,
                                                       const uint64_t* __restrict__ longs, const unsigned long long* __restrict__ ctr) {
    const uint64_t nl = ctr[2];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t r = longs[li];
        const uint64_t o = offsets[r], len = offsets[r + 1] - o;
        const uint64_t nu = (len + 63u) >> 6;
        const uintptr_t rec = reinterpret_cast<uintptr_t>(queries) + o;
        QueryUnit* U = units + uoff[r];
        for (uint64_t u = threadIdx.x; u < nu; u += 256u) pack_unit(rec, len, 64u * u, U + u);
    }
}

struct Win { uint64_t p0, p1, bad; };

// Letters a .. a+63 (a of either sign) of a sequence of `len` letters held in `nunits` >= 1 units of 32 bytes {p0, p1, nm, ..}:
// two neighbouring units, each two 16-byte loads, funnel-shifted; positions outside the sequence come back as `bad`.  Both units
// are read at a place that exists, then the choice.
__device__ __forceinline__ Win window(const uint4* __restrict__ U, int64_t nunits, int64_t len, int64_t a) {
    const int64_t u = a >> 6;
    const uint32_t sh = (uint32_t)(a & 63);
    const bool in0 = u >= 0 && u < nunits, in1 = u + 1 >= 0 && u + 1 < nunits;
    const int64_t u0 = in0 ? u : 0, u1 = in1 ? u + 1 : 0;
    const uint4 a0 = U[2 * u0], b0 = U[2 * u0 + 1], a1 = U[2 * u1], b1 = U[2 * u1 + 1];
    const uint64_t l0 = in0 ? ((uint64_t)a0.y << 32) | a0.x : 0ull, l1 = in0 ? ((uint64_t)a0.w << 32) | a0.z : 0ull;
    const uint64_t ln = in0 ? ((uint64_t)b0.y << 32) | b0.x : ~0ull;
    const uint64_t h0 = in1 ? ((uint64_t)a1.y << 32) | a1.x : 0ull, h1 = in1 ? ((uint64_t)a1.w << 32) | a1.z : 0ull;
    const uint64_t hn = in1 ? ((uint64_t)b1.y << 32) | b1.x : ~0ull;
    Win w;
    w.p0 = sh ? (l0 >> sh) | (h0 << (64u - sh)) : l0;
    w.p1 = sh ? (l1 >> sh) | (h1 << (64u - sh)) : l1;
    w.bad = sh ? (ln >> sh) | (hn << (64u - sh)) : ln;
    const int64_t valid = len - a;  // letters of the window that lie in front of the sequence's end
    if (valid < 64) w.bad |= valid <= 0 ? ~0ull : ~0ull << valid;
    return w;
}

// the same of the scanned strand: the record itself, or (rev) its reverse complement -- the bit-reversed, complemented window
// of the forward strand that ends where this one starts
__device__ __forceinline__ Win strand_window(const uint4* __restrict__ U, int64_t nunits, int64_t len, bool rev, int64_t a) {
    if (!rev) return window(U, nunits, len, a);
    const Win f = window(U, nunits, len, len - 64 - a);
    Win w;
    w.p0 = ~__brevll(f.p0);
    w.p1 = ~__brevll(f.p1);
    w.bad = __brevll(f.bad);
    return w;
}

__device__ __forceinline__ Win mirrored(const Win& f) {
    Win w;
    w.p0 = __brevll(f.p0);
    w.p1 = __brevll(f.p1);
    w.bad = __brevll(f.bad);
    return w;
}

// one side of a row on its way: s and best as in the definition, pos = letters consumed into s so far + the run not yet added
struct Side {
    int64_t s, best;
    uint64_t ext, pos;
    uint32_t mm, mm_best;
};

// 64 more letters (distance t0 .. t0+63) of a side: bit k of `q`/`t` planes is the letter at distance t0 + k.  True: the side
// has ended.  The loop runs per MISMATCH: the matches in front of each are one addition.
__device__ __forceinline__ bool walk(Side& d, const Win& q, const Win& t, uint64_t t0, int64_t P, int64_t X) {
    const uint64_t bad = q.bad | t.bad;
    const uint32_t fb = bad ? (uint32_t)__builtin_ctzll(bad) : 64u;  // the step that ends the side in front of it
    uint64_t m = (q.p0 ^ t.p0) | (q.p1 ^ t.p1);
    if (fb < 64u) m &= (1ull << fb) - 1ull;
    while (m) {
        const uint64_t at = t0 + (uint64_t)__builtin_ctzll(m);
        m &= m - 1ull;
        d.s += (int64_t)(at - d.pos);  // the run of matches in front of the mismatch
        if (d.s > d.best) { d.best = d.s; d.ext = at; d.mm_best = d.mm; }
        d.s -= P;
        d.mm++;
        d.pos = at + 1ull;
        if (d.best - d.s > X) return true;
    }
    if (fb < 64u) {
        const uint64_t at = t0 + fb;
        d.s += (int64_t)(at - d.pos);
        if (d.s > d.best) { d.best = d.s; d.ext = at; d.mm_best = d.mm; }
        return true;
    }
    return false;
}

// ---- the batch as planes: the four launches ------------------------------------------------------------------------------------
// ucnt / uoff: num_queries + 1 entries; uscan: the scan's room; longs: query_bytes / (64 * kExtPackLaneUnits) + 1 entries; units:
// query_bytes / 64 + num_queries + 1 units; long_ctr: ctr[2] of a zeroed counter block
inline hipError_t pack_batch_planes(const char* queries, const uint64_t* offsets_dev, uint64_t num_queries, uint32_t* ucnt, uint64_t* uoff,
                                    void* uscan, size_t uscan_bytes, uint64_t* longs, QueryUnit* units, unsigned long long* ctr,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(k_ext_units, dim3(grid_for(num_queries + 1)), dim3(256), 0, stream, offsets_dev, num_queries, ucnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t need = uscan_bytes;
    e = scan_sum_exclusive_u32_u64(uscan, need, ucnt, uoff, num_queries, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ext_pack, dim3(grid_for(num_queries)), dim3(256), 0, stream, queries, offsets_dev, num_queries,
                       (const uint64_t*)uoff, units, longs, ctr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ext_pack_long, dim3(kExtPackGrid), dim3(256), 0, stream, queries, offsets_dev, (const uint64_t*)uoff, units,
                       (const uint64_t*)longs, (const unsigned long long*)ctr);
    return hipGetLastError();
}

}  // namespace

}  // namespace slamem
