// sv_filter.hip -- the junctions of -sv: the long deletions and insertions that lie between two segments of one
// read.  -aln closes a gap between two chain anchors up to -maxed edits; a gap that does not close ends a segment, and the pileup
// (4.16) and the events (4.18) see nothing of what lies between the two.  Every adjacent pair of segments (a, b) of a contributing
// read, in ascending order of the scanned strand, is a junction: dr text rows and dq read letters between a's end and b's start.
// The m = min(dr, dq) letters that both sides own are shared out between a's diagonal and b's where that costs the fewest
// mismatches (the smallest such split); what remains is a deletion of L = dr - dq rows or an insertion of L = dq - dr letters,
// left-normalised as 4.18 normalises and counted per strand in a table of ev_table.h's slots keyed by (pos, kind, len): key0 holds
// pos and kind, key1 the marker and len.  The inserted letters are not part of the key.
//   k_junctions          a lane per read of the batch, behind the pile kernels of an add; the screen of k_pile_lane
//   k_junctions_insert   a lane per given junction with its two counts: the merge of two tables, and the tests' planting tool
//   k_sv_count / k_sv_emit / k_ev_sort_key / k_sv_gather   the read-out: the passes of ev_table.h with the least length in the
//                        rule, two stable sorts (by len, then by pos and kind), the slamem_junction records in order
// Every loop has a bound that is fixed before it starts (the read's segments, m <= 64, dr, the row a normalisation starts at, the
// probes of an insert); no lane waits for another lane's store.
#include "buffers.h"
#include "ev_table.h"

#include <new>

namespace slamem {

static_assert(sizeof(slamem_junction) == 24, "a record is 24 bytes");

struct SvTable {
    EvTable t;
    uint32_t max_mis;  // mismatches the best split may have
};

namespace {

constexpr uint32_t kSvSlop = 64;  // letters both sides of a junction may own: one mask word

struct SvAcc {
    EvAcc e;
    uint32_t max_mis;
};

__device__ __forceinline__ uint64_t sv_low(uint32_t t) { return t >= 64u ? ~0ull : (1ull << t) - 1ull; }

// c letters (1 <= c <= 64) as two bit-planes and the mask of those that are none of A,C,G,T: bit i belongs to letter i
struct SvLetters {
    uint64_t p0, p1, bad;
};

// rows [x, x + c) of the text, x + c <= n: a window over two neighbouring units; the second one is loaded only when the window
// reaches into it, so that it holds row x + c - 1
__device__ __forceinline__ SvLetters sv_text(const TextPlanes* __restrict__ tpl, uint64_t x, uint32_t c) {
    const TextPlanes* u = tpl + (x >> 6);
    const uint32_t s = (uint32_t)(x & 63u);
    SvLetters w{u->p0 >> s, u->p1 >> s, u->nm >> s};
    if (s + c > 64u) {  // (s > 0 here)
        w.p0 |= u[1].p0 << (64u - s);
        w.p1 |= u[1].p1 << (64u - s);
        w.bad |= u[1].nm << (64u - s);
    }
    const uint64_t low = sv_low(c);
    w.p0 &= low; w.p1 &= low; w.bad &= low;
    return w;
}

// letters [q, q + c) of the scanned strand; a letter behind the read's end is none of A,C,G,T
__device__ __forceinline__ SvLetters sv_read(const PileRead& r, uint64_t q, uint32_t c) {
    SvLetters w{0, 0, 0};
    for (uint32_t i = 0; i < c; i++) {
        const uint64_t code = pile_letter(r, q + i);
        w.p0 |= (code & 1ull) << i;
        w.p1 |= ((code >> 1) & 1ull) << i;
        w.bad |= (code >> 2) << i;
    }
    return w;
}

__device__ __forceinline__ void sv_insert(const EvAcc& a, uint64_t pos, uint32_t kind, uint32_t len, uint32_t fwd, uint32_t rev) {
    ev_probe(a, kEvSet | ((unsigned long long)kind << 40) | pos, kEvSet | len, fwd, rev);
}

// the junction between a's end (pe, qe) and b's start (ps, qs) of a read of one strand
__device__ __forceinline__ void sv_junction(const SvAcc& a, const PileRead& rd, uint64_t pe, uint64_t qe, uint64_t ps, uint64_t qs) {
    const EvAcc& e = a.e;
    const uint32_t fwd = rd.rev ? 0u : 1u, rev = rd.rev ? 1u : 0u;
    if (ps < pe || qs < qe || ps >= e.n || qs > rd.len) { atomicAdd(&e.skipped[2], 1ull); return; }  // (no mapping of the engine's)
    const uint64_t dr = ps - pe, dq = qs - qe;
    if (dr == dq) { atomicAdd(&e.skipped[0], 1ull); return; }
    const uint64_t m64 = dr < dq ? dr : dq, len64 = dr < dq ? dq - dr : dr - dq;
    if (m64 > kSvSlop) { atomicAdd(&e.skipped[3], 1ull); return; }
    const uint32_t m = (uint32_t)m64, L = (uint32_t)len64;  // (dr <= n < 2^32; dq <= the read's length, which the key's 32 bits of len hold)
    if (len64 >> 32) { atomicAdd(&e.skipped[2], 1ull); return; }
    if (dr && ev_rows_bad(e.tpl, pe, dr)) { atomicAdd(&e.skipped[2], 1ull); return; }
    uint32_t t = 0;
    if (m) {
        // the first mask on a's diagonal, the second on b's
        const SvLetters r1 = sv_read(rd, qe, m), r2 = sv_read(rd, qs - m, m);
        if (r1.bad | r2.bad) { atomicAdd(&e.skipped[2], 1ull); return; }
        const SvLetters t1 = sv_text(e.tpl, pe, m), t2 = sv_text(e.tpl, ps - m, m);
        const uint64_t M1 = (r1.p0 ^ t1.p0) | (r1.p1 ^ t1.p1), M2 = (r2.p0 ^ t2.p0) | (r2.p1 ^ t2.p1), lowm = sv_low(m);
        uint32_t best = 65u;
        for (uint32_t k = 0; k <= m; k++) {  // (m <= 64)
            const uint64_t lk = sv_low(k);
            const uint32_t cost = (uint32_t)__popcll(M1 & lk) + (uint32_t)__popcll(M2 & ~lk & lowm);
            if (cost < best) { best = cost; t = k; }
        }
        if (best > a.max_mis) { atomicAdd(&e.skipped[3], 1ull); return; }
    }
    const uint64_t p0 = pe + t;
    if (dr > dq) {  // a deletion of rows [p0, p0 + L), inside [pe, ps): valid rows
        sv_insert(e, ev_deletion_left(e.tpl, p0, L), 0u, L, fwd, rev);
        return;
    }
    // an insertion of S = letters [qe + t, qe + t + L) of the scanned strand in front of row p0 < n.  4.18's loop without the
    // letters in a register: after j steps S is rows [p0 - j, p0) and then the first L - j letters of the read's; its last letter
    // is the read's while j < L and the text's afterwards.  The loop runs at most p0 times.
    uint64_t p = p0;
    for (uint64_t j = 0; j < p0; j++) {
        const uint32_t c = ev_text(e.tpl, p0 - j - 1u);
        const uint32_t last = j < L ? pile_letter(rd, qe + t + (L - 1u - j)) : ev_text(e.tpl, p0 - j + L - 1u);
        if (c >= 4u || c != last) break;
        p--;
    }
    sv_insert(e, p, 1u, L, fwd, rev);
}

// a lane per read: the adjacent pairs of its segments.  The engine writes a read's segments in descending order of the scanned
// strand: segment s + 1 ends in front of segment s.
__global__ void __launch_bounds__(256) k_junctions(PileBatch b, SvAcc a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= b.nq) return;
    PileRead rd;
    if (!pile_contributes(b, r, rd)) return;
    const uint64_t s0 = b.roff[r], s1 = b.roff[r + 1];
    if (s1 < s0 + 2u) return;
    slamem_aln hi = b.segs[s0];
    for (uint64_t s = s0 + 1u; s < s1; s++) {
        const slamem_aln lo = b.segs[s];
        sv_junction(a, rd, (uint64_t)lo.ref_pos + lo.ref_len, (uint64_t)lo.query_pos + lo.query_len, hi.ref_pos, hi.query_pos);
        hi = lo;
    }
}

// a lane per given junction: validated, a deletion normalised (a canonical one stays as it is), an insertion taken where it is
// given (its letters are not in the record), inserted with its counts
__global__ void __launch_bounds__(256) k_junctions_insert(const slamem_junction* __restrict__ jn, uint64_t m, EvAcc a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const slamem_junction j = jn[i];
    const unsigned long long obs = (unsigned long long)j.fwd + j.rev;
    if (obs == 0ull) return;
    bool bad = j.kind > 1u || j.len == 0u || j.pos >= a.n;
    if (!bad && j.kind == 0u) bad = (uint64_t)j.len > a.n - j.pos || ev_rows_bad(a.tpl, j.pos, j.len);
    if (bad) { atomicAdd(&a.skipped[2], obs); return; }
    sv_insert(a, j.kind == 0u ? ev_deletion_left(a.tpl, j.pos, j.len) : j.pos, j.kind, j.len, j.fwd, j.rev);
}

// ---- read-out (the passes of ev_table.h; the rule's min_key1 is the least length) ---------------------------------------------

__global__ void __launch_bounds__(256) k_sv_count(const EvSlot* __restrict__ slots, uint64_t nslots, EvRule rule, uint64_t* __restrict__ sel) {
    ev_count_body<true>(slots, nslots, rule, sel);
}

__global__ void __launch_bounds__(256) k_sv_emit(const EvSlot* __restrict__ slots, uint64_t nslots, EvRule rule, const uint64_t* __restrict__ sel,
                                                 uint64_t room, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    ev_emit_body<true>(slots, nslots, rule, sel, room, keys, vals);
}

// record i (i < m, i < capacity) from the slot the sorts put there
__global__ void __launch_bounds__(256) k_sv_gather(const EvSlot* __restrict__ slots, uint64_t nslots, const uint32_t* __restrict__ vals,
                                                   uint64_t m, uint64_t capacity, slamem_junction* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= m || i >= capacity) return;
    const uint64_t x = vals[i];
    slamem_junction j;
    j.pos = 0; j.len = 0; j.fwd = 0; j.rev = 0; j.kind = 0;
    for (int k = 0; k < 3; k++) j.pad[k] = 0;
    if (x < nslots) {
        const EvSlot s = slots[x];
        j.pos = s.key0 & kEvPosMask;
        j.kind = (uint8_t)((s.key0 >> 40) & 1ull);
        j.len = (uint32_t)(s.key1 & 0xFFFFFFFFull);
        j.fwd = s.fwd;
        j.rev = s.rev;
    }
    out[i] = j;
}

EvAcc sv_acc(const slamem_pileup* pile) {
    EvAcc a;
    a.tpl = pile->idx->view.tpl;
    a.slots = pile->sv->t.slots;
    a.mask = pile->sv->t.nslots - 1;
    a.skipped = pile->sv->t.skipped;
    a.n = pile->n;
    return a;
}

}  // namespace

int junctions_add(slamem_pileup* pile, const void* batch, hipStream_t stream) {
    const PileBatch b = *static_cast<const PileBatch*>(batch);
    const SvAcc a{sv_acc(pile), pile->sv->max_mis};
    hipLaunchKernelGGL(k_junctions, dim3(pile_grid(b.nq, 256)), dim3(256), 0, stream, b, a);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int junctions_reset(slamem_pileup* pile) {
    SLAMEM_HIP(hipMemset(pile->sv->t.slots, 0, pile->sv->t.nslots * sizeof(EvSlot)));
    SLAMEM_HIP(hipMemset(pile->sv->t.skipped, 0, 4 * sizeof(unsigned long long)));
    return SLAMEM_OK;
}

void junctions_free(slamem_pileup* pile) {
    SvTable* t = pile->sv;
    if (!t) return;
    ev_table_release(&t->t);
    delete t;
    pile->sv = nullptr;
}

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_pileup_enable_junctions(slamem_pileup* pile, uint64_t slots, uint32_t max_mis) {
    if (!pile) { set_error("slamem_pileup_enable_junctions: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_enable_junctions"));
    if (pile->sv) { set_error("slamem_pileup_enable_junctions: the junctions of this accumulator are enabled already"); return SLAMEM_ERR_ARG; }
    if (max_mis > kSvSlop) {
        set_error("slamem_pileup_enable_junctions: the mismatches of a split are 0 to %u, not %u", kSvSlop, max_mis);
        return SLAMEM_ERR_ARG;
    }
    if (slots == 0) {  // the default: the smallest power of two that is at least max(65536, n / 64)
        const uint64_t want = (uint64_t)pile->n / 64 > 65536 ? (uint64_t)pile->n / 64 : 65536;
        for (slots = 65536; slots < want; slots <<= 1) {}
    }
    if (slots < 64 || slots > (1ull << 31) || (slots & (slots - 1)) != 0) {
        set_error("slamem_pileup_enable_junctions: the number of slots is a power of two from 64 to 2^31, not %llu", (unsigned long long)slots);
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_HIP(hipSetDevice(pile->device));
    size_t tmp_bytes = 0;
    const uint64_t need = ev_table_bytes(slots, 4, &tmp_bytes);
    size_t free_b = 0, total_b = 0;
    SLAMEM_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        set_error("slamem_pileup_enable_junctions: a table of %llu slots takes %llu bytes (24 per slot and as much again for the "
                  "read-out's sort), %llu are free on device %d", (unsigned long long)slots, (unsigned long long)need,
                  (unsigned long long)free_b, pile->device);
        return SLAMEM_ERR_NOMEM;
    }
    SvTable* t = new (std::nothrow) SvTable();
    if (!t) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    t->max_mis = max_mis;
    pile->sv = t;
    const hipError_t e = ev_table_alloc(&t->t, slots, tmp_bytes, 4);
    if (e != hipSuccess) {
        junctions_free(pile);
        return hip_fail(e, "slamem_pileup_enable_junctions", __FILE__, __LINE__);
    }
    return SLAMEM_OK;
}

int slamem_pileup_add_junctions_device(slamem_pileup* pile, const slamem_junction* junctions_dev, uint64_t m, void* stream) {
    if (!pile || (m && !junctions_dev)) { set_error("slamem_pileup_add_junctions_device: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_add_junctions_device"));
    if (!pile->sv) { set_error("slamem_pileup_add_junctions_device: the junctions of this accumulator are not enabled"); return SLAMEM_ERR_ARG; }
    if (m == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    pile->used.store(true, std::memory_order_relaxed);
    hipLaunchKernelGGL(k_junctions_insert, dim3(pile_grid(m, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), junctions_dev, m,
                       sv_acc(pile));
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int slamem_pileup_add_junctions_host(slamem_pileup* pile, const slamem_junction* junctions, uint64_t m) {
    if (!pile || (m && !junctions)) { set_error("slamem_pileup_add_junctions_host: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_add_junctions_host"));
    if (!pile->sv) { set_error("slamem_pileup_add_junctions_host: the junctions of this accumulator are not enabled"); return SLAMEM_ERR_ARG; }
    if (m == 0) return SLAMEM_OK;
    SLAMEM_HIP(hipSetDevice(pile->device));
    DevBuf<slamem_junction> d;
    SLAMEM_TRY(d.reserve(m));
    SLAMEM_HIP(hipMemcpy(d.get(), junctions, m * sizeof(slamem_junction), hipMemcpyHostToDevice));
    SLAMEM_TRY(slamem_pileup_add_junctions_device(pile, d.get(), m, nullptr));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the buffer goes when this returns)
    return SLAMEM_OK;
}

int slamem_pileup_junctions_device(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t min_count, uint32_t min_len,
                                   uint64_t capacity, slamem_junction* junctions_dev, uint64_t* skipped_out, uint64_t* total_out,
                                   void* stream) {
    if (!pile || !total_out || !skipped_out || (capacity && !junctions_dev)) {
        set_error("slamem_pileup_junctions_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    for (int k = 0; k < 4; k++) skipped_out[k] = 0;
    if (!pile->sv) { set_error("slamem_pileup_junctions_device: the junctions of this accumulator are not enabled"); return SLAMEM_ERR_ARG; }
    if (first > pile->n || count > pile->n - first) {
        set_error("slamem_pileup_junctions_device: rows %llu .. %llu + %llu lie outside the text's %u", (unsigned long long)first,
                  (unsigned long long)first, (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    if (min_count == 0u) { set_error("slamem_pileup_junctions_device: the least number of observations is at least 1"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    EvTable* t = &pile->sv->t;
    const uint64_t tiles = ev_tiles(t->nslots);
    const EvRule rule{first, first + count, min_count, min_len};
    hipLaunchKernelGGL(k_sv_count, dim3((unsigned)tiles), dim3(256), 0, st, (const EvSlot*)t->slots, t->nslots, rule, t->sel);
    SLAMEM_HIP(hipGetLastError());
    int rc = pile_scan_counts(t->sel, tiles, st);  // (tiles + 1 <= nslots / kEvTile + 2 words)
    if (rc != SLAMEM_OK) return rc;
    if (capacity) {
        hipLaunchKernelGGL(k_sv_emit, dim3((unsigned)tiles), dim3(256), 0, st, (const EvSlot*)t->slots, t->nslots, rule,
                           (const uint64_t*)t->sel, t->nslots, t->ka, t->va);
        SLAMEM_HIP(hipGetLastError());
    }
    uint64_t total = 0;  // the call's one host round trip: the sorts need the number of pairs
    unsigned long long skipped[4] = {0, 0, 0, 0};
    SLAMEM_HIP(hipMemcpyAsync(&total, t->sel + tiles, 8, hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipMemcpyAsync(skipped, t->skipped, sizeof(skipped), hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipStreamSynchronize(st));
    *total_out = total;
    for (int k = 0; k < 4; k++) skipped_out[k] = skipped[k];
    if (capacity && total) {
        // two stable sorts: by len (key1 without its marker), then by (pos, kind); the slot numbers travel as values
        size_t tb = t->tmp_bytes;
        SLAMEM_HIP(sort_pairs_u64_u32(t->tmp, tb, t->ka, t->kb, t->va, t->vb, (size_t)total, 0, 32, st));
        hipLaunchKernelGGL(k_ev_sort_key, dim3(pile_grid(total, 256)), dim3(256), 0, st, (const EvSlot*)t->slots, t->nslots,
                           (const uint32_t*)t->vb, total, t->ka);
        SLAMEM_HIP(hipGetLastError());
        SLAMEM_HIP(sort_pairs_u64_u32(t->tmp, tb, t->ka, t->kb, t->vb, t->va, (size_t)total, 0, 48, st));
        hipLaunchKernelGGL(k_sv_gather, dim3(pile_grid(total < capacity ? total : capacity, 256)), dim3(256), 0, st,
                           (const EvSlot*)t->slots, t->nslots, (const uint32_t*)t->va, total, capacity, junctions_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    if (total > capacity) {
        set_error("slamem_pileup_junctions_device: %llu junctions are selected, the buffer holds %llu", (unsigned long long)total,
                  (unsigned long long)capacity);
        return SLAMEM_ERR_CAPACITY;
    }
    return SLAMEM_OK;
}

int slamem_pileup_junctions_host(slamem_pileup* pile, uint64_t first, uint64_t count, uint32_t min_count, uint32_t min_len,
                                 uint64_t capacity, slamem_junction* junctions, uint64_t* skipped_out, uint64_t* total_out) {
    if (!pile || !total_out || !skipped_out || (capacity && !junctions)) {
        set_error("slamem_pileup_junctions_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    if (!pile->sv) { set_error("slamem_pileup_junctions_host: the junctions of this accumulator are not enabled"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    const uint64_t room = capacity < pile->sv->t.nslots ? capacity : pile->sv->t.nslots;  // (a table gives at most its slots)
    DevBuf<slamem_junction> d;
    if (room) SLAMEM_TRY(d.reserve(room));
    const int rc = slamem_pileup_junctions_device(pile, first, count, min_count, min_len, room, d.get(), skipped_out, total_out, nullptr);
    if (rc != SLAMEM_OK && rc != SLAMEM_ERR_CAPACITY) return rc;
    // (the junctions that fitted go back with SLAMEM_ERR_CAPACITY too; the call's code comes before a failed copy's)
    const uint64_t got = *total_out < room ? *total_out : room;
    hipError_t e = hipDeviceSynchronize();
    if (got && e == hipSuccess) e = hipMemcpy(junctions, d.get(), got * sizeof(slamem_junction), hipMemcpyDeviceToHost);
    if (rc == SLAMEM_OK && e != hipSuccess) return hip_fail(e, "hipMemcpy", __FILE__, __LINE__);
    return rc;
}

}  // extern "C"
