// dedup_filter.hip -- -dedup: every copy of a fragment counts once in the pileup.  A read is a candidate iff it
// would contribute (strand != 0, mapq >= min_mapq, at least one segment); its key is (strand, u), u the unclipped 5' position in
// merged-text coordinates:
//   strand 1   L = the segment with the smallest query_pos:              u = ref_pos(L) - query_pos(L)               (may be < 0)
//   strand 2   R = the segment with the largest query_pos + query_len:   u = ref_pos(R) + ref_len(R) + (len - query_pos(R) - query_len(R))
// (the first such segment in storage order; the segments of a read are stored with the query start descending, and nothing here
// relies on that).  Packed: ((u + 2^32) << 1) | (strand - 1); all-ones is the empty slot.  A read's rank is seq << 32 | its index
// in the batch, seq the number of the dedup add on its accumulator; of the candidates of one key the one with the smallest rank
// is piled, the others are duplicates.
//
// The table is open addressing in HBM: a slot is 16 bytes {key, rank}, the slot count a power of two, cleared by one memset of
// 0xFF (an empty key, and a rank above every real one).  Linear probing from a hash of the key, at most kDdProbes slots, as
// event_filter.hip probes its table.  No lane waits for another lane's store: every loop is bounded by the probe limit.
//   k_dup_claim   a lane per read: CAS(key, empty -> mine) along the probes until the slot holds my key, then atomicMin(rank, mine);
//                 no such slot within the limit: the read claims nothing
//   k_dup_mark    a lane per read, behind k_dup_claim of the same add: the same probes find the slot again (a slot never changes its
//                 key), dup[r] = 0 kept or no candidate, 1 the slot's rank is another read's, 2 no room (kept); reads_keep[r] = the
//                 read's record with strand 0 where dup[r] == 1; four counters per wave by ballot, one atomic per wave and counter
// Two dedup adds on one accumulator must not overlap in these two kernels (a later add would mark before an earlier one has
// claimed): the host holds a mutex while it enqueues, numbers the add under it, and chains the pairs with an event.  The pile
// kernels behind the pair are atomics and overlap freely.
#include "buffers.h"
#include "pile_shared.h"

#include <mutex>
#include <new>

namespace slamem {

struct DdSlot {
    unsigned long long key, rank;
};
static_assert(sizeof(DdSlot) == 16, "a slot is 16 bytes");

struct DdTable {
    DdSlot* slots = nullptr;
    uint64_t nslots = 0;                  // a power of two, 64 to 2^32
    unsigned long long* stats = nullptr;  // candidates, duplicates, no room, slots newly claimed
    uint64_t seq = 0;                     // the number of the next dedup add (under mu)
    hipEvent_t last = nullptr;            // behind the claim and mark kernels of the add enqueued last (under mu)
    bool recorded = false;
    std::mutex mu;
};

namespace {

constexpr uint32_t kDdProbes = 128;  // slots a read looks at before it gives up
constexpr unsigned long long kDdEmpty = ~0ull;

struct DdAcc {
    DdSlot* slots;
    uint64_t mask;  // nslots - 1
    unsigned long long* stats;
    uint64_t seq;
};

__device__ __forceinline__ uint64_t dd_hash(uint64_t x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}

// the packed key of read r; false: the read is no candidate
__device__ __forceinline__ bool dd_key(const PileBatch& b, uint64_t r, unsigned long long& key) {
    const slamem_map m = b.reads[r];
    if (m.strand == 0u || m.mapq < b.min_mapq) return false;
    const uint64_t s0 = b.roff[r], s1 = b.roff[r + 1];
    if (s1 <= s0) return false;
    const int64_t len = (int64_t)(b.offsets[r + 1] - b.offsets[r]);
    int64_t u = 0;
    if (m.strand == 1u) {
        uint64_t best = ~0ull;
        for (uint64_t s = s0; s < s1; s++) {
            const slamem_aln g = b.segs[s];
            if ((uint64_t)g.query_pos < best) { best = g.query_pos; u = (int64_t)g.ref_pos - (int64_t)g.query_pos; }
        }
    } else {
        int64_t best = -1;
        for (uint64_t s = s0; s < s1; s++) {
            const slamem_aln g = b.segs[s];
            const int64_t e = (int64_t)g.query_pos + (int64_t)g.query_len;
            if (e > best) { best = e; u = (int64_t)g.ref_pos + (int64_t)g.ref_len + (len - e); }
        }
    }
    key = ((unsigned long long)(u + (1ll << 32)) << 1) | (unsigned long long)(m.strand == 2u ? 1u : 0u);
    return true;
}

__device__ __forceinline__ uint32_t dd_probes(const DdAcc& a) { return a.mask + 1u < kDdProbes ? (uint32_t)(a.mask + 1u) : kDdProbes; }

__global__ void __launch_bounds__(256) k_dup_claim(PileBatch b, DdAcc a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= b.nq) return;
    unsigned long long key;
    if (!dd_key(b, r, key)) return;
    const unsigned long long rank = (a.seq << 32) | r;
    const uint64_t h = dd_hash(key);
    const uint32_t probes = dd_probes(a);
    for (uint32_t i = 0; i < probes; i++) {
        DdSlot* s = a.slots + ((h + i) & a.mask);
        const unsigned long long was = atomicCAS(&s->key, kDdEmpty, key);
        if (was != kDdEmpty && was != key) continue;
        atomicMin(&s->rank, rank);
        return;
    }
}

__global__ void __launch_bounds__(256) k_dup_mark(PileBatch b, DdAcc a, slamem_map* __restrict__ keep, uint8_t* __restrict__ dup) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool have = r < b.nq;
    unsigned long long key = 0;
    const bool cand = have && dd_key(b, r, key);
    uint32_t flag = 0;
    bool mine = false;
    if (cand) {
        const unsigned long long rank = (a.seq << 32) | r;
        const uint64_t h = dd_hash(key);
        const uint32_t probes = dd_probes(a);
        flag = 2u;
        for (uint32_t i = 0; i < probes; i++) {
            DdSlot* s = a.slots + ((h + i) & a.mask);
            const unsigned long long k = __hip_atomic_load(&s->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == kDdEmpty) break;  // (a candidate's probes end at its key or run out: k_dup_claim has been there)
            if (k != key) continue;
            mine = __hip_atomic_load(&s->rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == rank;
            flag = mine ? 0u : 1u;
            break;
        }
    }
    if (have) {
        slamem_map m = b.reads[r];
        if (flag == 1u) m.strand = 0;
        keep[r] = m;
        if (dup) dup[r] = (uint8_t)flag;
    }
    // the wave's four counts: a ballot each, lane 0 adds what is not zero
    const unsigned long long c0 = __ballot(cand), c1 = __ballot(flag == 1u), c2 = __ballot(flag == 2u), c3 = __ballot(mine);
    if ((threadIdx.x & 63u) == 0u) {
        if (c0) atomicAdd(&a.stats[0], (unsigned long long)__popcll(c0));
        if (c1) atomicAdd(&a.stats[1], (unsigned long long)__popcll(c1));
        if (c2) atomicAdd(&a.stats[2], (unsigned long long)__popcll(c2));
        if (c3) atomicAdd(&a.stats[3], (unsigned long long)__popcll(c3));
    }
}

}  // namespace

int pileup_has_dedup(const slamem_pileup* pile) { return pile->dd != nullptr; }

int pileup_add_dedup(slamem_pileup* pile, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                     const slamem_aln* segs_dev, const uint64_t* read_offsets_dev, const uint32_t* ops_dev, const uint64_t* op_offsets_dev,
                     const slamem_map* reads_dev, uint32_t min_mapq, const uint64_t* lowq_dev, slamem_map* reads_keep_dev,
                     uint8_t* dup_out_dev, hipStream_t stream) {
    DdTable* t = pile->dd;
    {
        std::lock_guard<std::mutex> lk(t->mu);
        const uint64_t seq = t->seq++;
        if (num_queries == 0) return SLAMEM_OK;
        PileBatch b;
        b.queries = static_cast<const unsigned char*>(queries_dev);
        b.offsets = offsets_dev;
        b.segs = segs_dev;
        b.roff = read_offsets_dev;
        b.ops = ops_dev;
        b.ooff = op_offsets_dev;
        b.reads = reads_dev;
        b.nq = num_queries;
        b.min_mapq = min_mapq;
        const DdAcc a{t->slots, t->nslots - 1, t->stats, seq};
        if (t->recorded) SLAMEM_HIP(hipStreamWaitEvent(stream, t->last, 0));  // (behind the pair of the add in front of this one)
        hipLaunchKernelGGL(k_dup_claim, dim3(pile_grid(num_queries, 256)), dim3(256), 0, stream, b, a);
        SLAMEM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_dup_mark, dim3(pile_grid(num_queries, 256)), dim3(256), 0, stream, b, a, reads_keep_dev, dup_out_dev);
        SLAMEM_HIP(hipGetLastError());
        SLAMEM_HIP(hipEventRecord(t->last, stream));
        t->recorded = true;
    }
    return pileup_add_masked(pile, queries_dev, offsets_dev, num_queries, segs_dev, read_offsets_dev, ops_dev, op_offsets_dev,
                             reads_keep_dev, min_mapq, lowq_dev, stream);
}

int dedup_reset(slamem_pileup* pile) {
    DdTable* t = pile->dd;
    std::lock_guard<std::mutex> lk(t->mu);
    SLAMEM_HIP(hipMemset(t->slots, 0xFF, t->nslots * sizeof(DdSlot)));
    SLAMEM_HIP(hipMemset(t->stats, 0, 4 * sizeof(unsigned long long)));
    t->seq = 0;
    return SLAMEM_OK;
}

void dedup_free(slamem_pileup* pile) {
    DdTable* t = pile->dd;
    if (!t) return;
    if (t->slots) (void)hipFree(t->slots);
    if (t->stats) (void)hipFree(t->stats);
    if (t->last) (void)hipEventDestroy(t->last);
    delete t;
    pile->dd = nullptr;
}

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_pileup_enable_dedup(slamem_pileup* pile, uint64_t slots) {
    if (!pile) { set_error("slamem_pileup_enable_dedup: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_enable_dedup"));
    if (pile->dd) { set_error("slamem_pileup_enable_dedup: the duplicate filter of this accumulator is enabled already"); return SLAMEM_ERR_ARG; }
    if (slots == 0) {  // the default: the smallest power of two that is at least max(65536, n / 4)
        const uint64_t want = (uint64_t)pile->n / 4 > 65536 ? (uint64_t)pile->n / 4 : 65536;
        for (slots = 65536; slots < want; slots <<= 1) {}
    }
    if (slots < 64 || slots > (1ull << 32) || (slots & (slots - 1)) != 0) {
        set_error("slamem_pileup_enable_dedup: the number of slots is a power of two from 64 to 2^32, not %llu", (unsigned long long)slots);
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_HIP(hipSetDevice(pile->device));
    const uint64_t need = slots * sizeof(DdSlot) + 4 * sizeof(unsigned long long);
    size_t free_b = 0, total_b = 0;
    SLAMEM_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        set_error("slamem_pileup_enable_dedup: a table of %llu slots takes %llu bytes (16 per slot), %llu are free on device %d",
                  (unsigned long long)slots, (unsigned long long)need, (unsigned long long)free_b, pile->device);
        return SLAMEM_ERR_NOMEM;
    }
    DdTable* t = new (std::nothrow) DdTable();
    if (!t) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    t->nslots = slots;
    pile->dd = t;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&t->slots), slots * sizeof(DdSlot));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->stats), 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->last, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemsetAsync(t->slots, 0xFF, slots * sizeof(DdSlot), nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(t->stats, 0, 4 * sizeof(unsigned long long), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        dedup_free(pile);
        return hip_fail(e, "slamem_pileup_enable_dedup", __FILE__, __LINE__);
    }
    return SLAMEM_OK;
}

int slamem_pileup_add_dedup_device(slamem_pileup* pile, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                                   const slamem_aln* segs_dev, const uint64_t* read_offsets_dev, const uint32_t* ops_dev,
                                   const uint64_t* op_offsets_dev, const slamem_map* reads_dev, uint32_t min_mapq,
                                   const uint64_t* lowq_dev, slamem_map* reads_keep_dev, uint8_t* dup_out_dev, void* stream) {
    if (!pile || !offsets_dev || !read_offsets_dev || !op_offsets_dev || !reads_dev || !reads_keep_dev ||
        (num_queries && (!queries_dev || !segs_dev || !ops_dev))) {
        set_error("slamem_pileup_add_dedup_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_add_dedup_device"));
    SLAMEM_TRY(pile_refuse_quals(pile, "slamem_pileup_add_dedup_device"));
    if (!pile->dd) {
        set_error("slamem_pileup_add_dedup_device: the duplicate filter of this accumulator is not enabled (slamem_pileup_enable_dedup)");
        return SLAMEM_ERR_ARG;
    }
    if (min_mapq > 60u) { set_error("slamem_pileup_add_dedup_device: the minimum mapping quality is 0 to 60"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(pile->device));
    return pileup_add_dedup(pile, queries_dev, offsets_dev, num_queries, segs_dev, read_offsets_dev, ops_dev, op_offsets_dev, reads_dev,
                            min_mapq, lowq_dev, reads_keep_dev, dup_out_dev, static_cast<hipStream_t>(stream));
}

int slamem_pileup_dedup_stats(slamem_pileup* pile, uint64_t out[4]) {
    if (!pile || !out) { set_error("slamem_pileup_dedup_stats: null argument"); return SLAMEM_ERR_ARG; }
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!pile->dd) {
        set_error("slamem_pileup_dedup_stats: the duplicate filter of this accumulator is not enabled (slamem_pileup_enable_dedup)");
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are counted)
    unsigned long long v[4] = {0, 0, 0, 0};
    SLAMEM_HIP(hipMemcpy(v, pile->dd->stats, sizeof(v), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) out[k] = v[k];
    return SLAMEM_OK;
}

}  // extern "C"
