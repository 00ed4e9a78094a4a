// event_filter.hip -- the indel events of -vcf: what the pileup of 4.16 does not hold.  Every I and D operation
// of a contributing read (strand != 0, mapq >= min_mapq) is an observation of an event; the event is left-normalised against the
// text and counted per strand in a hash table in HBM, keyed by (pos, kind, len, inserted letters).
//
// The table, its 24-byte slot and its two-CAS insert are ev_table.h's, shared with sv_filter.hip; here key0 also holds len in bits
// 41..47 and key1 the inserted letters two bits each, the first one highest.
//   k_events_lane / k_events_wave   the walks of k_pile_lane / k_pile_wave (pile_filter.hip), acting on I and D alone
//   k_events_insert                 a lane per given event with its two counts: the merge of two tables, and the tests' planting tool
//   k_ev_count / k_ev_emit          the read-out: the slots of the range with enough observations per tile of kEvTile slots, and
//                                   (behind the scan of 4.17) their key1 and slot number at base + ballot rank: no atomics
//   k_ev_sort_key / k_ev_gather     the second sort's key (pos, kind, len from key0) and the slamem_event records in order
//   k_pile_rows_at                  rows of counts() at listed positions, a wave per position
#include "buffers.h"
#include "ev_table.h"

#include <new>

namespace slamem {

static_assert(sizeof(slamem_event) == 32, "a record is 32 bytes");

namespace {

constexpr uint32_t kEvMaxIns = 31, kEvMaxDel = 127;

// a valid event in canonical form: its slot gets `fwd` and `rev`; no room within kEvProbes probes: skipped[1]
__device__ __forceinline__ void ev_insert(const EvAcc& a, uint64_t pos, uint32_t kind, uint32_t len, uint64_t letters, uint32_t fwd,
                                          uint32_t rev) {
    ev_probe(a, kEvSet | ((unsigned long long)len << 41) | ((unsigned long long)kind << 40) | pos, kEvSet | letters, fwd, rev);
}

// a deletion of rows [p, p + k), valid (1 <= k <= kEvMaxDel, p + k <= n, the rows A,C,G,T): as far left as it goes, then inserted.
// The loop runs at most p times: p is fixed before it starts.
__device__ __forceinline__ void ev_deletion(const EvAcc& a, uint64_t p, uint32_t k, uint32_t fwd, uint32_t rev) {
    ev_insert(a, ev_deletion_left(a.tpl, p, k), 0u, k, 0ull, fwd, rev);
}

// an insertion of k letters S (1 <= k <= kEvMaxIns, letter i at bits 2 (k - 1 - i)) in front of row p < n
__device__ __forceinline__ void ev_insertion(const EvAcc& a, uint64_t p, uint32_t k, uint64_t S, uint32_t fwd, uint32_t rev) {
    for (uint64_t left = p; left > 0; left--) {
        const uint32_t c = ev_text(a.tpl, p - 1u);
        if (c >= 4u || c != (uint32_t)(S & 3ull)) break;
        S = ((uint64_t)c << (2u * (k - 1u))) | (S >> 2);
        p--;
    }
    ev_insert(a, p, 1u, k, S, fwd, rev);
}

// one operation of a read at (p, q): an I or a D is an observation of its strand
__device__ __forceinline__ void ev_op(const EvAcc& a, const PileRead& r, uint32_t op, uint64_t p, uint64_t q) {
    const uint32_t code = op & 15u, k = op >> 4;
    if ((code != kOpI && code != kOpD) || k == 0u) return;
    const uint32_t fwd = r.rev ? 0u : 1u, rev = r.rev ? 1u : 0u;
    if (code == kOpI) {
        if (k > kEvMaxIns) { atomicAdd(&a.skipped[0], 1ull); return; }
        uint64_t S = 0;
        bool bad = p >= a.n;
        for (uint32_t j = 0; j < k; j++) {
            const uint32_t c = pile_letter(r, q + j);
            bad |= c >= 4u;
            S = (S << 2) | (c & 3u);
        }
        if (bad) { atomicAdd(&a.skipped[2], 1ull); return; }
        ev_insertion(a, p, k, S, fwd, rev);
    } else {
        if (k > kEvMaxDel || p >= a.n || (uint64_t)k > a.n - p || ev_rows_bad(a.tpl, p, k)) { atomicAdd(&a.skipped[2], 1ull); return; }
        ev_deletion(a, p, k, fwd, rev);
    }
}

// a lane per read: its segments of up to kPileLaneOps operations (the walk of k_pile_lane)
__global__ void __launch_bounds__(256) k_events_lane(PileBatch b, EvAcc a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= b.nq) return;
    PileRead rd;
    if (!pile_contributes(b, r, rd)) return;
    const uint64_t s1 = b.roff[r + 1];
    for (uint64_t s = b.roff[r]; s < s1; s++) {
        const uint64_t o0 = b.ooff[s], o1 = b.ooff[s + 1];
        if (o1 <= o0 || o1 - o0 > kPileLaneOps) continue;
        const slamem_aln sg = b.segs[s];
        uint64_t p = sg.ref_pos, q = sg.query_pos;
        for (uint64_t i = o0; i < o1; i++) {
            const uint32_t op = b.ops[i];
            ev_op(a, rd, op, p, q);
            p += pile_ref_step(op);
            q += pile_query_step(op);
        }
    }
}

// a wave per 64 reads: the segments of more than kPileLaneOps operations, 64 operations at a time (the walk of k_pile_wave)
__global__ void __launch_bounds__(64) k_events_wave(PileBatch b, EvAcc a) {
    const uint32_t lane = threadIdx.x;
    const uint64_t chunks = (b.nq + 63u) >> 6;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t r = c * 64u + lane;
        bool big = false;
        PileRead mine;
        if (r < b.nq && pile_contributes(b, r, mine)) {
            const uint64_t s1 = b.roff[r + 1];
            for (uint64_t s = b.roff[r]; s < s1 && !big; s++) big = b.ooff[s + 1] - b.ooff[s] > kPileLaneOps && b.ooff[s + 1] > b.ooff[s];
        }
        unsigned long long todo = __ballot(big);
        while (todo) {
            const uint32_t src = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint64_t rr = c * 64u + src;
            PileRead rd;
            (void)pile_contributes(b, rr, rd);  // (it does: its lane said so)
            const uint64_t s1 = b.roff[rr + 1];
            for (uint64_t s = b.roff[rr]; s < s1; s++) {
                const uint64_t o0 = b.ooff[s], o1 = b.ooff[s + 1];
                if (o1 <= o0 || o1 - o0 <= kPileLaneOps) continue;
                const slamem_aln sg = b.segs[s];
                uint64_t p = sg.ref_pos, q = sg.query_pos;
                for (uint64_t base = o0; base < o1; base += 64u) {
                    const bool have = base + lane < o1;
                    const uint32_t op = have ? b.ops[base + lane] : 0u;
                    const uint64_t rs = pile_ref_step(op), qs = pile_query_step(op);
                    const uint64_t ri = wave_scan_inclusive(rs, lane), qi = wave_scan_inclusive(qs, lane);
                    if (have) ev_op(a, rd, op, p + ri - rs, q + qi - qs);
                    p += __shfl(ri, 63, 64);
                    q += __shfl(qi, 63, 64);
                }
            }
        }
    }
}

// a lane per given event: validated as an observation is, normalised (a canonical event stays as it is), inserted with its counts
__global__ void __launch_bounds__(256) k_events_insert(const slamem_event* __restrict__ ev, uint64_t m, EvAcc a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const slamem_event e = ev[i];
    const unsigned long long obs = (unsigned long long)e.fwd + e.rev;
    if (obs == 0ull) return;
    const uint32_t k = e.len;
    if (e.kind == 1u && k > kEvMaxIns) { atomicAdd(&a.skipped[0], obs); return; }
    bool bad = e.kind > 1u || k == 0u || e.pos >= a.n;
    if (!bad && e.kind == 1u) bad = (e.letters >> (2u * k)) != 0ull;
    if (!bad && e.kind == 0u) bad = k > kEvMaxDel || (uint64_t)k > a.n - e.pos || e.letters != 0ull || ev_rows_bad(a.tpl, e.pos, k);
    if (bad) { atomicAdd(&a.skipped[2], obs); return; }
    if (e.kind == 1u) ev_insertion(a, e.pos, k, e.letters, e.fwd, e.rev);
    else ev_deletion(a, e.pos, k, e.fwd, e.rev);
}

// ---- read-out --------------------------------------------------------------------------------------------------------------

// a workgroup per tile of slots: sel[blockIdx.x] = how many of them the rule selects (ev_table.h)
__global__ void __launch_bounds__(256) k_ev_count(const EvSlot* __restrict__ slots, uint64_t nslots, EvRule rule, uint64_t* __restrict__ sel) {
    ev_count_body<false>(slots, nslots, rule, sel);
}

// a workgroup per tile: key1 and the slot number of its selected slots at sel[blockIdx.x] + rank in the tile (ev_table.h)
__global__ void __launch_bounds__(256) k_ev_emit(const EvSlot* __restrict__ slots, uint64_t nslots, EvRule rule, const uint64_t* __restrict__ sel,
                                                 uint64_t room, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    ev_emit_body<false>(slots, nslots, rule, sel, room, keys, vals);
}

// record i (i < m, i < capacity) from the slot the sorts put there
__global__ void __launch_bounds__(256) k_ev_gather(const EvSlot* __restrict__ slots, uint64_t nslots, const uint32_t* __restrict__ vals,
                                                   uint64_t m, uint64_t capacity, slamem_event* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m || i >= capacity) return;
    const uint64_t x = vals[i];
    slamem_event e;
    e.pos = 0; e.letters = 0; e.fwd = 0; e.rev = 0; e.kind = 0; e.len = 0;
    for (int k = 0; k < 6; k++) e.pad[k] = 0;
    if (x < nslots) {
        const EvSlot s = slots[x];
        e.pos = s.key0 & kEvPosMask;
        e.kind = (uint8_t)((s.key0 >> 40) & 1ull);
        e.len = (uint8_t)((s.key0 >> 41) & 127ull);
        e.letters = s.key1 & ~kEvSet;
        e.fwd = s.fwd;
        e.rev = s.rev;
    }
    out[i] = e;
}

// a wave per listed position p: match[p] = the tile's base and the sum of diff from the tile's first entry to p (32 entries a
// lane), on top of cnt[p] in the column of the text's letter.  A position at or behind n: a row of zeros.
__global__ void __launch_bounds__(256) k_pile_rows_at(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                      const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t n,
                                                      const uint64_t* __restrict__ pos, uint64_t m, uint32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= m) return;  // (the whole wave)
    const uint64_t p = pos[i];
    if (p >= n) {
        if (lane < 6u) out[i * 6u + lane] = 0u;
        return;
    }
    const uint64_t t = p / kPileTile, base = t * kPileTile;
    constexpr uint32_t per = kPileTile / 64u;
    uint32_t v = 0;
#pragma unroll 8
    for (uint32_t j = 0; j < per; j++) {
        const uint64_t x = base + (uint64_t)lane * per + j;
        if (x <= p) v += (uint32_t)diff[x];
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v += __shfl_xor(v, d, 64);
    const uint32_t match = tile[t] + v, letter = ev_text(tpl, p);
    if (lane < 6u) out[i * 6u + lane] = cnt[p * 6u + lane] + (lane == letter ? match : 0u);
}

EvAcc ev_acc(const slamem_pileup* pile) {
    EvAcc a;
    a.tpl = pile->idx->view.tpl;
    a.slots = pile->ev->slots;
    a.mask = pile->ev->nslots - 1;
    a.skipped = pile->ev->skipped;
    a.n = pile->n;
    return a;
}

}  // namespace

int events_add(slamem_pileup* pile, const void* batch, hipStream_t stream) {
    const PileBatch b = *static_cast<const PileBatch*>(batch);
    const EvAcc a = ev_acc(pile);
    hipLaunchKernelGGL(k_events_lane, dim3(pile_grid(b.nq, 256)), dim3(256), 0, stream, b, a);
    SLAMEM_HIP(hipGetLastError());
    const unsigned chunks = pile_grid(b.nq, 64);
    hipLaunchKernelGGL(k_events_wave, dim3(chunks < kPileWaveGrid ? chunks : kPileWaveGrid), dim3(64), 0, stream, b, a);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int events_reset(slamem_pileup* pile) {
    SLAMEM_HIP(hipMemset(pile->ev->slots, 0, pile->ev->nslots * sizeof(EvSlot)));
    SLAMEM_HIP(hipMemset(pile->ev->skipped, 0, 3 * sizeof(unsigned long long)));
    return SLAMEM_OK;
}

void events_free(slamem_pileup* pile) {
    EvTable* t = pile->ev;
    if (!t) return;
    ev_table_release(t);
    delete t;
    pile->ev = nullptr;
}

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_pileup_enable_events(slamem_pileup* pile, uint64_t slots) {
    if (!pile) { set_error("slamem_pileup_enable_events: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_enable_events"));
    if (pile->ev) { set_error("slamem_pileup_enable_events: the events of this accumulator are enabled already"); return SLAMEM_ERR_ARG; }
    if (slots == 0) {  // the default: the smallest power of two that is at least max(65536, n / 16)
        const uint64_t want = (uint64_t)pile->n / 16 > 65536 ? (uint64_t)pile->n / 16 : 65536;
        for (slots = 65536; slots < want; slots <<= 1) {}
    }
    if (slots < 64 || slots > (1ull << 31) || (slots & (slots - 1)) != 0) {
        set_error("slamem_pileup_enable_events: the number of slots is a power of two from 64 to 2^31, not %llu", (unsigned long long)slots);
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_HIP(hipSetDevice(pile->device));
    size_t tmp_bytes = 0;
    const uint64_t need = ev_table_bytes(slots, 3, &tmp_bytes);
    size_t free_b = 0, total_b = 0;
    SLAMEM_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        set_error("slamem_pileup_enable_events: a table of %llu slots takes %llu bytes (24 per slot and as much again for the read-out's "
                  "sort), %llu are free on device %d", (unsigned long long)slots, (unsigned long long)need, (unsigned long long)free_b,
                  pile->device);
        return SLAMEM_ERR_NOMEM;
    }
    EvTable* t = new (std::nothrow) EvTable();
    if (!t) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    pile->ev = t;
    const hipError_t e = ev_table_alloc(t, slots, tmp_bytes, 3);
    if (e != hipSuccess) {
        events_free(pile);
        return hip_fail(e, "slamem_pileup_enable_events", __FILE__, __LINE__);
    }
    return SLAMEM_OK;
}

int slamem_pileup_add_events_device(slamem_pileup* pile, const slamem_event* events_dev, uint64_t m, void* stream) {
    if (!pile || (m && !events_dev)) { set_error("slamem_pileup_add_events_device: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_add_events_device"));
    if (!pile->ev) { set_error("slamem_pileup_add_events_device: the events of this accumulator are not enabled"); return SLAMEM_ERR_ARG; }
    if (m == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    pile->used.store(true, std::memory_order_relaxed);
    hipLaunchKernelGGL(k_events_insert, dim3(pile_grid(m, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), events_dev, m,
                       ev_acc(pile));
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int slamem_pileup_add_events_host(slamem_pileup* pile, const slamem_event* events, uint64_t m) {
    if (!pile || (m && !events)) { set_error("slamem_pileup_add_events_host: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_add_events_host"));
    if (!pile->ev) { set_error("slamem_pileup_add_events_host: the events of this accumulator are not enabled"); return SLAMEM_ERR_ARG; }
    if (m == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    DevBuf<slamem_event> d;
    SLAMEM_TRY(d.reserve(m));
    SLAMEM_HIP(hipMemcpy(d.get(), events, m * sizeof(slamem_event), hipMemcpyHostToDevice));
    SLAMEM_TRY(slamem_pileup_add_events_device(pile, d.get(), m, nullptr));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the buffer goes when this returns)
    return SLAMEM_OK;
}

int slamem_pileup_events_device(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t min_count, uint64_t capacity,
                                slamem_event* events_dev, uint64_t* skipped_out, uint64_t* total_out, void* stream) {
    if (!pile || !total_out || !skipped_out || (capacity && !events_dev)) {
        set_error("slamem_pileup_events_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    skipped_out[0] = skipped_out[1] = skipped_out[2] = 0;
    if (!pile->ev) { set_error("slamem_pileup_events_device: the events of this accumulator are not enabled"); return SLAMEM_ERR_ARG; }
    if (first > pile->n || count > pile->n - first) {
        set_error("slamem_pileup_events_device: rows %llu .. %llu + %llu lie outside the text's %u", (unsigned long long)first,
                  (unsigned long long)first, (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    if (min_count == 0u) { set_error("slamem_pileup_events_device: the least number of observations is at least 1"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    EvTable* t = pile->ev;
    const uint64_t tiles = ev_tiles(t->nslots);
    const EvRule rule{first, first + count, min_count, 0};
    hipLaunchKernelGGL(k_ev_count, dim3((unsigned)tiles), dim3(256), 0, st, (const EvSlot*)t->slots, t->nslots, rule, t->sel);
    SLAMEM_HIP(hipGetLastError());
    int rc = pile_scan_counts(t->sel, tiles, st);  // (tiles + 1 <= nslots / kEvTile + 2 words)
    if (rc != SLAMEM_OK) return rc;
    if (capacity) {
        hipLaunchKernelGGL(k_ev_emit, dim3((unsigned)tiles), dim3(256), 0, st, (const EvSlot*)t->slots, t->nslots, rule,
                           (const uint64_t*)t->sel, t->nslots, t->ka, t->va);
        SLAMEM_HIP(hipGetLastError());
    }
    uint64_t total = 0;  // the call's one host round trip: the sorts need the number of pairs
    unsigned long long skipped[3] = {0, 0, 0};
    SLAMEM_HIP(hipMemcpyAsync(&total, t->sel + tiles, 8, hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipMemcpyAsync(skipped, t->skipped, sizeof(skipped), hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipStreamSynchronize(st));
    *total_out = total;
    for (int k = 0; k < 3; k++) skipped_out[k] = skipped[k];
    if (capacity && total) {
        // two stable sorts: by the letters, then by (pos, kind, len); the slot numbers travel as values
        size_t tb = t->tmp_bytes;
        SLAMEM_HIP(sort_pairs_u64_u32(t->tmp, tb, t->ka, t->kb, t->va, t->vb, (size_t)total, 0, 62, st));
        hipLaunchKernelGGL(k_ev_sort_key, dim3(pile_grid(total, 256)), dim3(256), 0, st, (const EvSlot*)t->slots, t->nslots,
                           (const uint32_t*)t->vb, total, t->ka);
        SLAMEM_HIP(hipGetLastError());
        SLAMEM_HIP(sort_pairs_u64_u32(t->tmp, tb, t->ka, t->kb, t->vb, t->va, (size_t)total, 0, 48, st));
        hipLaunchKernelGGL(k_ev_gather, dim3(pile_grid(total < capacity ? total : capacity, 256)), dim3(256), 0, st,
                           (const EvSlot*)t->slots, t->nslots, (const uint32_t*)t->va, total, capacity, events_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    if (total > capacity) {
        set_error("slamem_pileup_events_device: %llu events are selected, the buffer holds %llu", (unsigned long long)total,
                  (unsigned long long)capacity);
        return SLAMEM_ERR_CAPACITY;
    }
    return SLAMEM_OK;
}

int slamem_pileup_events_host(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t min_count, uint64_t capacity,
                              slamem_event* events, uint64_t* skipped_out, uint64_t* total_out) {
    if (!pile || !total_out || !skipped_out || (capacity && !events)) {
        set_error("slamem_pileup_events_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    if (!pile->ev) { set_error("slamem_pileup_events_host: the events of this accumulator are not enabled"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    const uint64_t room = capacity < pile->ev->nslots ? capacity : pile->ev->nslots;  // (a table gives at most its slots)
    DevBuf<slamem_event> d;
    if (room) SLAMEM_TRY(d.reserve(room));
    const int rc = slamem_pileup_events_device(pile, first, count, min_count, room, d.get(), skipped_out, total_out, nullptr);
    if (rc != SLAMEM_OK && rc != SLAMEM_ERR_CAPACITY) return rc;
    // (the events that fitted go back with SLAMEM_ERR_CAPACITY too; the call's code comes before a failed copy's)
    const uint64_t got = *total_out < room ? *total_out : room;
    hipError_t e = hipDeviceSynchronize();
    if (got && e == hipSuccess) e = hipMemcpy(events, d.get(), got * sizeof(slamem_event), hipMemcpyDeviceToHost);
    if (rc == SLAMEM_OK && e != hipSuccess) return hip_fail(e, "hipMemcpy", __FILE__, __LINE__);
    return rc;
}

int slamem_pileup_rows_at_device(slamem_pileup* pile, const uint64_t* pos_dev, uint64_t m, uint32_t* out_dev, void* stream) {
    if (!pile || (m && (!pos_dev || !out_dev))) { set_error("slamem_pileup_rows_at_device: null argument"); return SLAMEM_ERR_ARG; }
    if (m == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = pile_tile_prefix(pile, pile->n, st);  // (the positions are on the device: the tiles of the whole text)
    if (rc != SLAMEM_OK) return rc;
    hipLaunchKernelGGL(k_pile_rows_at, dim3(pile_grid(m, 4)), dim3(256), 0, st, (const int32_t*)pile->diff, (const uint32_t*)pile->cnt,
                       (const uint32_t*)pile->tile, pile->idx->view.tpl, (uint64_t)pile->n, pos_dev, m, out_dev);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int slamem_pileup_rows_at_host(slamem_pileup* pile, const uint64_t* pos, uint64_t m, uint32_t* out) {
    if (!pile || (m && (!pos || !out))) { set_error("slamem_pileup_rows_at_host: null argument"); return SLAMEM_ERR_ARG; }
    uint64_t largest = 0;
    for (uint64_t i = 0; i < m; i++) {
        if (pos[i] >= pile->n) {
            set_error("slamem_pileup_rows_at_host: position %llu (entry %llu) lies outside the text's %u", (unsigned long long)pos[i],
                      (unsigned long long)i, pile->n);
            return SLAMEM_ERR_ARG;
        }
        if (pos[i] > largest) largest = pos[i];
    }
    if (m == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    DevBuf<uint64_t> d;  // m positions, then m rows of six uint32
    SLAMEM_TRY(d.reserve(m * 4));
    uint64_t* pd = d.get();
    uint32_t* od = reinterpret_cast<uint32_t*>(pd + m);
    SLAMEM_HIP(hipMemcpy(pd, pos, m * 8, hipMemcpyHostToDevice));
    SLAMEM_TRY(pile_tile_prefix(pile, largest + 1, nullptr));  // (up to the largest position)
    hipLaunchKernelGGL(k_pile_rows_at, dim3(pile_grid(m, 4)), dim3(256), 0, nullptr, (const int32_t*)pile->diff, (const uint32_t*)pile->cnt,
                       (const uint32_t*)pile->tile, pile->idx->view.tpl, (uint64_t)pile->n, (const uint64_t*)pd, m, od);
    SLAMEM_HIP(hipGetLastError());
    SLAMEM_HIP(hipMemcpy(out, od, m * 24, hipMemcpyDeviceToHost));
    return SLAMEM_OK;
}

}  // extern "C"
