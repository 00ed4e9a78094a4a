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
//   k_ext_copy / _list_copy the kept rows and their mismatches, in order
// Every row is checked against the one before it: a block out of the emission order fails the call -- never wrong rows.
#include "common.h"
#include "prims.h"

namespace slamem {

namespace {

inline unsigned grid_for(uint64_t items, unsigned block = 256) { return items ? (unsigned)((items + block - 1) / block) : 1u; }
inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

constexpr uint32_t kExtLaneMax = 32;        // rows of a block one lane de-duplicates
constexpr unsigned kExtWaveGrid = 2048;     // one-wave workgroups that share the list of larger blocks
constexpr uint32_t kExtPackLaneUnits = 16;  // units (of 64 letters) of a record one lane packs
constexpr unsigned kExtPackGrid = 1024;     // workgroups that share the list of longer records

// a unit of a packed record: the layout of TextPlanes without the occurs-once plane
struct __attribute__((aligned(32))) QueryUnit { uint64_t p0, p1, nm, pad; };
static_assert(sizeof(QueryUnit) == 32 && sizeof(TextPlanes) == 32, "units are two 16-byte loads");

struct ExtLayout {
    uint64_t off_ctr, off_rows, off_boff, off_cnt, off_newoff, off_keep, off_owner, off_xrows, off_xmm, off_scan, scan_bytes, off_list,
        off_ucnt, off_uoff, off_uscan, uscan_bytes, off_long, off_units, bytes;
};

ExtLayout ext_layout(uint64_t num_queries, uint64_t num_blocks, uint64_t query_bytes, uint64_t capacity) {
    ExtLayout m;
    uint64_t off = 0;
    m.off_ctr = off;    off = align_up(off + 64, 256);                                  // [0] listed blocks, [1] order violation, [2] listed records
    m.off_rows = off;   off = align_up(off + capacity * sizeof(slamem_mem) + 16, 256);  // the -mem list (K9 places it here)
    m.off_boff = off;   off = align_up(off + (num_blocks + 1) * 8, 256);                // ... and its block offsets
    m.off_cnt = off;    off = align_up(off + (num_blocks + 1) * 4, 256);                // kept rows per block
    m.off_newoff = off; off = align_up(off + (num_blocks + 1) * 8, 256);                // their exclusive sums
    m.off_keep = off;   off = align_up(off + capacity + 16, 256);                       // a byte per -mem row
    m.off_owner = off;  off = align_up(off + capacity * 4 + 16, 256);                   // the strand block of every -mem row
    m.off_xrows = off;  off = align_up(off + capacity * sizeof(slamem_mem) + 16, 256);  // the extended rows
    m.off_xmm = off;    off = align_up(off + capacity * 4 + 16, 256);                   // ... and their mismatches
    size_t need = 0;
    (void)scan_sum_exclusive_u32_u64(nullptr, need, nullptr, nullptr, num_blocks, 0);
    m.scan_bytes = need;
    m.off_scan = off;   off = align_up(off + need, 256);
    m.off_list = off;   off = align_up(off + (capacity / (kExtLaneMax + 1) + 1) * 8, 256);  // listed strand blocks
    m.off_ucnt = off;   off = align_up(off + (num_queries + 1) * 4, 256);               // units per record
    m.off_uoff = off;   off = align_up(off + (num_queries + 1) * 8, 256);               // their exclusive sums
    need = 0;
    (void)scan_sum_exclusive_u32_u64(nullptr, need, nullptr, nullptr, num_queries, 0);
    m.uscan_bytes = need;
    m.off_uscan = off;  off = align_up(off + need, 256);
    m.off_long = off;   off = align_up(off + (query_bytes / (64ull * kExtPackLaneUnits) + 1) * 8, 256);  // listed records
    m.off_units = off;  off = align_up(off + (query_bytes / 64 + num_queries + 1) * sizeof(QueryUnit), 256);  // the packed batch
    m.bytes = off;
    return m;
}

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

// one lane per strand block: new offsets, and the kept rows of blocks of up to kExtLaneMax rows
__global__ void __launch_bounds__(256) k_ext_copy(const uint64_t* __restrict__ boff, uint64_t nb, uint64_t cap,
                                                  const slamem_mem* __restrict__ xrows, const uint32_t* __restrict__ xmm,
                                                  const uint8_t* __restrict__ keep, const uint64_t* __restrict__ newoff,
                                                  slamem_mem* __restrict__ out, uint32_t* __restrict__ out_mm, uint64_t* __restrict__ out_boff) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b > nb) return;
    uint64_t d = newoff[b];
    out_boff[b] = d;
    if (b == nb) return;
    uint64_t s, e;
    clamp_block(boff, b, cap, s, e);
    if (e - s > kExtLaneMax) return;
    const uint64_t d_end = newoff[b + 1];
    for (uint64_t i = s; i < e && d < d_end; i++) {
        if (!keep[i]) continue;
        if (d < cap) {
            out[d] = xrows[i];
            if (out_mm) out_mm[d] = xmm[i];
        }
        d++;
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

uint64_t ext_workspace_bytes(uint64_t num_queries, uint64_t num_blocks, uint64_t query_bytes, uint64_t capacity) {
    return ext_layout(num_queries, num_blocks, query_bytes, capacity).bytes;
}

#define XSTEP(call, what) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(e__, what, __FILE__, __LINE__); } while (0)

void ext_list_buffers(void* ws, uint64_t num_queries, uint64_t num_blocks, uint64_t query_bytes, uint64_t capacity, slamem_mem** rows_out,
                      uint64_t** boff_out) {
    const ExtLayout m = ext_layout(num_queries, num_blocks, query_bytes, capacity);
    char* p = static_cast<char*>(ws);
    *rows_out = reinterpret_cast<slamem_mem*>(p + m.off_rows);
    *boff_out = reinterpret_cast<uint64_t*>(p + m.off_boff);
}

int ext_filter(void* ws, const IndexView& ix, const void* queries_dev, const uint64_t* offsets_dev, uint64_t num_queries, uint32_t strands,
               uint64_t query_bytes, uint64_t capacity, uint32_t penalty, uint32_t xdrop, slamem_mem* out_mems, uint64_t* out_boff,
               uint32_t* out_mm, unsigned long long* host_scalars, hipStream_t stream) {
    const uint64_t num_blocks = num_queries * strands;
    const ExtLayout m = ext_layout(num_queries, num_blocks, query_bytes, capacity);
    char* p = static_cast<char*>(ws);
    unsigned long long* ctr = reinterpret_cast<unsigned long long*>(p + m.off_ctr);
    const slamem_mem* rows = reinterpret_cast<const slamem_mem*>(p + m.off_rows);
    const uint64_t* boff = reinterpret_cast<const uint64_t*>(p + m.off_boff);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(p + m.off_cnt);
    uint64_t* newoff = reinterpret_cast<uint64_t*>(p + m.off_newoff);
    uint8_t* keep = reinterpret_cast<uint8_t*>(p + m.off_keep);
    uint32_t* owner = reinterpret_cast<uint32_t*>(p + m.off_owner);
    slamem_mem* xrows = reinterpret_cast<slamem_mem*>(p + m.off_xrows);
    uint32_t* xmm = reinterpret_cast<uint32_t*>(p + m.off_xmm);
    uint64_t* list = reinterpret_cast<uint64_t*>(p + m.off_list);
    uint32_t* ucnt = reinterpret_cast<uint32_t*>(p + m.off_ucnt);
    uint64_t* uoff = reinterpret_cast<uint64_t*>(p + m.off_uoff);
    uint64_t* longs = reinterpret_cast<uint64_t*>(p + m.off_long);
    QueryUnit* units = reinterpret_cast<QueryUnit*>(p + m.off_units);
    const char* queries = static_cast<const char*>(queries_dev);
    XSTEP(hipMemsetAsync(ctr, 0, 24, stream), "memset");
    // the batch as planes
    hipLaunchKernelGGL(k_ext_units, dim3(grid_for(num_queries + 1)), dim3(256), 0, stream, offsets_dev, num_queries, ucnt);
    XSTEP(hipGetLastError(), "k_ext_units");
    size_t need = m.uscan_bytes;
    XSTEP(scan_sum_exclusive_u32_u64(p + m.off_uscan, need, ucnt, uoff, num_queries, stream), "scan");
    hipLaunchKernelGGL(k_ext_pack, dim3(grid_for(num_queries)), dim3(256), 0, stream, queries, offsets_dev, num_queries,
                       (const uint64_t*)uoff, units, longs, ctr);
    XSTEP(hipGetLastError(), "k_ext_pack");
    hipLaunchKernelGGL(k_ext_pack_long, dim3(kExtPackGrid), dim3(256), 0, stream, queries, offsets_dev, (const uint64_t*)uoff, units,
                       (const uint64_t*)longs, (const unsigned long long*)ctr);
    XSTEP(hipGetLastError(), "k_ext_pack_long");
    // the rows
    hipLaunchKernelGGL(k_ext_mark, dim3(grid_for(num_blocks + 1)), dim3(256), 0, stream, boff, num_blocks, rows, capacity, owner, cnt, list,
                       ctr);
    XSTEP(hipGetLastError(), "k_ext_mark");
    hipLaunchKernelGGL(k_ext_mark_wave, dim3(kExtWaveGrid), dim3(64), 0, stream, (const uint64_t*)list, (const unsigned long long*)ctr, boff,
                       rows, capacity, owner, ctr);
    XSTEP(hipGetLastError(), "k_ext_mark_wave");
    hipLaunchKernelGGL(k_ext_extend, dim3(grid_for(capacity)), dim3(256), 0, stream, boff, num_blocks, rows, capacity,
                       (const uint32_t*)owner, offsets_dev, (const uint64_t*)uoff, (const QueryUnit*)units, ix.tpl, ix.n, strands, penalty,
                       xdrop, xrows, xmm);
    XSTEP(hipGetLastError(), "k_ext_extend");
    hipLaunchKernelGGL(k_ext_dedup, dim3(grid_for(num_blocks)), dim3(256), 0, stream, boff, num_blocks, rows, capacity,
                       (const slamem_mem*)xrows, keep, cnt);
    XSTEP(hipGetLastError(), "k_ext_dedup");
    hipLaunchKernelGGL(k_ext_dedup_wave, dim3(kExtWaveGrid), dim3(64), 0, stream, (const uint64_t*)list, (const unsigned long long*)ctr,
                       boff, rows, capacity, (const slamem_mem*)xrows, keep, cnt);
    XSTEP(hipGetLastError(), "k_ext_dedup_wave");
    need = m.scan_bytes;
    XSTEP(scan_sum_exclusive_u32_u64(p + m.off_scan, need, cnt, newoff, num_blocks, stream), "scan");
    hipLaunchKernelGGL(k_ext_copy, dim3(grid_for(num_blocks + 1)), dim3(256), 0, stream, boff, num_blocks, capacity,
                       (const slamem_mem*)xrows, (const uint32_t*)xmm, (const uint8_t*)keep, (const uint64_t*)newoff, out_mems, out_mm,
                       out_boff);
    XSTEP(hipGetLastError(), "k_ext_copy");
    hipLaunchKernelGGL(k_ext_list_copy, dim3(kExtWaveGrid), dim3(64), 0, stream, (const uint64_t*)list, (const unsigned long long*)ctr,
                       boff, capacity, (const slamem_mem*)xrows, (const uint32_t*)xmm, (const uint8_t*)keep, (const uint64_t*)newoff,
                       out_mems, out_mm);
    XSTEP(hipGetLastError(), "k_ext_list_copy");
    // [0] rows kept, [1] the first block out of order + 1 (0: none)
    XSTEP(hipMemcpyAsync(host_scalars, newoff + num_blocks, 8, hipMemcpyDeviceToHost, stream), "memcpy");
    XSTEP(hipMemcpyAsync(host_scalars + 1, ctr + 1, 8, hipMemcpyDeviceToHost, stream), "memcpy");
    return SLAMEM_OK;
}
#undef XSTEP

}  // namespace slamem
