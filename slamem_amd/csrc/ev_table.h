// ev_table.h -- the hash table that event_filter.hip (the indel events of -vcf) and sv_filter.hip (the junctions of
// -sv) both keep: the 24-byte slot, the two-CAS insert, the text's letters and the N screen of a range of rows, and
// the passes of the read-out that do not care what a key means (count per tile, emit at base + ballot rank, the second sort's key).
//
// A slot is 24 bytes: key0 (bit 63, pos in bits 0..39, kind in bit 40, bits 41..47 the table's own), key1 (bit 63, the rest the
// table's own), fwd, rev.  0 in a key word means empty.  An insert probes linearly from a hash of key0 and per probe does
// CAS(key0, 0 -> w0), on 0 or w0 CAS(key1, 0 -> w1), on 0 or w1 the atomic adds; otherwise the next slot; after kEvProbes probes
// the observation is counted in skipped[1].  No lane waits for another lane's store: no loop here has a bound that another lane can
// move (4.18 has the argument why equal keys meet in one slot and why no slot keeps a key0 without a key1).
#pragma once
#include "pile_shared.h"
#include "prims.h"

namespace slamem {

struct EvSlot {
    unsigned long long key0, key1;
    uint32_t fwd, rev;
};
static_assert(sizeof(EvSlot) == 24, "a slot is 24 bytes");

struct EvTable {
    EvSlot* slots;
    uint64_t nslots;              // a power of two, 64 to 2^31
    unsigned long long* skipped;  // the table's counters (3 for the events, 4 for the junctions)
    uint64_t* sel;                // the read-out's selected slots per tile: nslots / kEvTile + 2 words
    uint64_t *ka, *kb;            // the read-out's sort keys, nslots each
    uint32_t *va, *vb;            // ... and slot numbers
    void* tmp;                    // sort_pairs_u64_u32's scratch for nslots pairs
    size_t tmp_bytes;
};

namespace {

constexpr uint32_t kEvProbes = 128;   // slots an insert looks at before it gives up
constexpr uint32_t kEvTile = 2048;    // slots per workgroup of the read-out (256 lanes x 8)
constexpr unsigned long long kEvSet = 1ull << 63;
constexpr unsigned long long kEvPosMask = (1ull << 40) - 1ull;

struct EvAcc {
    const TextPlanes* tpl;
    EvSlot* slots;
    uint64_t mask;  // nslots - 1
    unsigned long long* skipped;
    uint64_t n;
};

// the text's letter at x (x < n): A 0, C 1, G 2, T 3; anything else 4
__device__ __forceinline__ uint32_t ev_text(const TextPlanes* __restrict__ tpl, uint64_t x) {
    const TextPlanes* u = tpl + (x >> 6);
    const uint32_t bit = (uint32_t)(x & 63u);
    if ((u->nm >> bit) & 1ull) return 4u;
    return (uint32_t)((u->p0 >> bit) & 1ull) | ((uint32_t)((u->p1 >> bit) & 1ull) << 1);
}

// is any of rows [p, p + k) (p + k <= n, k >= 1) none of A,C,G,T?
__device__ __forceinline__ bool ev_rows_bad(const TextPlanes* __restrict__ tpl, uint64_t p, uint64_t k) {
    const uint64_t e = p + k;
    uint64_t any = 0;
    for (uint64_t u = p >> 6; u <= (e - 1) >> 6; u++) {
        uint64_t m = tpl[u].nm;
        if (u == p >> 6) m &= ~0ull << (p & 63u);
        if (u == (e - 1) >> 6 && (e & 63u)) m &= (1ull << (e & 63u)) - 1ull;
        any |= m;
    }
    return any != 0;
}

__device__ __forceinline__ uint64_t ev_hash(uint64_t x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}

// the slot of the key (w0, w1), both with bit 63 set, gets `fwd` and `rev`; no room within kEvProbes probes: skipped[1]
__device__ __forceinline__ void ev_probe(const EvAcc& a, unsigned long long w0, unsigned long long w1, uint32_t fwd, uint32_t rev) {
    const uint64_t h = ev_hash(w0);
    const uint32_t probes = a.mask + 1u < kEvProbes ? (uint32_t)(a.mask + 1u) : kEvProbes;
    for (uint32_t i = 0; i < probes; i++) {
        EvSlot* s = a.slots + ((h + i) & a.mask);
        const unsigned long long r = atomicCAS(&s->key0, 0ull, w0);
        if (r != 0ull && r != w0) continue;
        const unsigned long long r1 = atomicCAS(&s->key1, 0ull, w1);  // (every lane that set or met w0 comes here: key1 never stays empty)
        if (r1 != 0ull && r1 != w1) continue;
        if (fwd) atomicAdd(&s->fwd, fwd);
        if (rev) atomicAdd(&s->rev, rev);
        return;
    }
    atomicAdd(&a.skipped[1], (unsigned long long)fwd + rev);
}

// a deletion of rows [p, p + k) (k >= 1, p + k <= n, the rows A,C,G,T) as far left as it goes: the row it then starts at.
// The loop runs at most p times: p is fixed before it starts.
__device__ __forceinline__ uint64_t ev_deletion_left(const TextPlanes* __restrict__ tpl, uint64_t p, uint64_t k) {
    for (uint64_t left = p; left > 0; left--) {
        const uint32_t c = ev_text(tpl, p - 1u);
        if (c >= 4u || c != ev_text(tpl, p + k - 1u)) break;
        p--;
    }
    return p;
}

// ---- read-out --------------------------------------------------------------------------------------------------------------

struct EvRule {
    uint64_t first, end;  // first <= pos < end
    uint64_t min_count;   // fwd + rev at least this (>= 1)
    uint64_t min_key1;    // kKey1: key1 without its marker at least this
};

template <bool kKey1>
__device__ __forceinline__ bool ev_selected(const EvSlot* __restrict__ slots, uint64_t x, uint64_t nslots, const EvRule& r) {
    if (x >= nslots) return false;
    const unsigned long long k0 = slots[x].key0;
    if (k0 == 0ull) return false;
    const uint64_t pos = k0 & kEvPosMask;
    if constexpr (kKey1) {
        if ((slots[x].key1 & ~kEvSet) < r.min_key1) return false;
    }
    return pos >= r.first && pos < r.end && (uint64_t)slots[x].fwd + slots[x].rev >= r.min_count;
}

// a workgroup of 256 per tile of slots: sel[blockIdx.x] = how many of them the rule selects
template <bool kKey1>
__device__ __forceinline__ void ev_count_body(const EvSlot* __restrict__ slots, uint64_t nslots, const EvRule& rule, uint64_t* __restrict__ sel) {
    __shared__ uint32_t wsum[4];
    const uint64_t base = (uint64_t)blockIdx.x * kEvTile;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kEvTile / 256u; j++) mine += ev_selected<kKey1>(slots, base + j * 256u + threadIdx.x, nslots, rule) ? 1u : 0u;
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) sel[blockIdx.x] = (uint64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// a workgroup of 256 per tile: key1 and the slot number of its selected slots at sel[blockIdx.x] + rank in the tile (the scheme of
// k_sites_emit: ballots and popcounts in a wave, the waves' totals through LDS).  room: the entries of keys / vals.
template <bool kKey1>
__device__ __forceinline__ void ev_emit_body(const EvSlot* __restrict__ slots, uint64_t nslots, const EvRule& rule, const uint64_t* __restrict__ sel,
                                             uint64_t room, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    constexpr uint32_t per = kEvTile / 256u;
    __shared__ uint32_t wcnt[per * 4u];
    const uint64_t out0 = sel[blockIdx.x];
    if (sel[blockIdx.x + 1] == out0) return;  // (the whole workgroup: nothing selected)
    const uint64_t base = (uint64_t)blockIdx.x * kEvTile;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool take[per];
    uint32_t below[per];
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        take[j] = ev_selected<kKey1>(slots, base + j * 256u + threadIdx.x, nslots, rule);
        const unsigned long long b = __ballot(take[j]);
        below[j] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0u) wcnt[j * 4u + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t run = 0;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            if (w == wave) mine = run;
            run += wcnt[j * 4u + w];
        }
        const uint64_t o = out0 + mine + below[j];
        if (!take[j] || o >= room) continue;
        const uint64_t x = base + j * 256u + threadIdx.x;
        keys[o] = slots[x].key1 & ~kEvSet;
        vals[o] = (uint32_t)x;
    }
}

// the second sort's key of entry i: pos, kind, bits 41..47 of key0 in this order of weight (key0 holds them the other way round)
__global__ void __launch_bounds__(256) k_ev_sort_key(const EvSlot* __restrict__ slots, uint64_t nslots, const uint32_t* __restrict__ vals,
                                                     uint64_t m, uint64_t* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint64_t x = vals[i];
    const unsigned long long k0 = x < nslots ? slots[x].key0 : 0ull;
    keys[i] = ((k0 & kEvPosMask) << 8) | (((k0 >> 40) & 1ull) << 7) | ((k0 >> 41) & 127ull);
}

inline uint64_t ev_tiles(uint64_t nslots) { return (nslots + kEvTile - 1) / kEvTile; }

// ---- the table's memory (host) -----------------------------------------------------------------------------------------------

// bytes of HBM a table of `slots` slots and `counters` skipped counters takes with its read-out's scratch; tmp_bytes: the sort's share
inline uint64_t ev_table_bytes(uint64_t slots, uint32_t counters, size_t* tmp_bytes) {
    *tmp_bytes = 0;
    (void)sort_pairs_u64_u32(nullptr, *tmp_bytes, nullptr, nullptr, nullptr, nullptr, (size_t)slots, 0, 8, nullptr);
    return slots * (sizeof(EvSlot) + 24) + (ev_tiles(slots) + 2) * 8 + *tmp_bytes + counters * 8;
}

inline void ev_table_release(EvTable* t) {
    if (t->slots) (void)hipFree(t->slots);
    if (t->skipped) (void)hipFree(t->skipped);
    if (t->sel) (void)hipFree(t->sel);
    if (t->ka) (void)hipFree(t->ka);
    if (t->kb) (void)hipFree(t->kb);
    if (t->va) (void)hipFree(t->va);
    if (t->vb) (void)hipFree(t->vb);
    if (t->tmp) (void)hipFree(t->tmp);
    *t = EvTable{};
}

// allocates and clears a table of `slots` slots and `counters` skipped counters; on a failure everything is released again
inline hipError_t ev_table_alloc(EvTable* t, uint64_t slots, size_t tmp_bytes, uint32_t counters) {
    *t = EvTable{};
    t->nslots = slots;
    t->tmp_bytes = tmp_bytes;
    const uint64_t tiles = ev_tiles(slots) + 2;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&t->slots), slots * sizeof(EvSlot));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->skipped), counters * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->sel), tiles * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->ka), slots * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->kb), slots * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->va), slots * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->vb), slots * 4);
    if (e == hipSuccess) e = hipMalloc(&t->tmp, tmp_bytes);
    if (e == hipSuccess) e = hipMemset(t->slots, 0, slots * sizeof(EvSlot));
    if (e == hipSuccess) e = hipMemset(t->skipped, 0, counters * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) ev_table_release(t);
    return e;
}

}  // namespace

}  // namespace slamem
