// qual_filter.hip -- -wq: the sum of the base qualities per row and letter, a second accumulator Q of the pileup's
// layout (int32 diff[n + 1], uint32 cnt[n][6]) that the owner keeps beside its counts.  A letter's quality is qv(b) = 0 when its
// byte b is below the Phred offset, else min(b - offset, 93).  Every read that contributes to the pileup of an add is walked once
// more with the same operations, and wherever the pileup's walk adds 1 to column A, C, G or T of a row, Q gets the letter's qv in
// the same column of the same row; D and I add nothing.
//
// The qualities of the letters under an `=` run are a step function over the run's rows, and a step function goes into a
// difference array with one atomic per step: + v where a stretch of level v starts, new - old where the level changes, - v where
// it ends.  Rows that the pileup gives nothing (the text's letter none of A,C,G,T, a masked letter, rows at or behind n) are of
// level 0.  Sequencers write few distinct values in long runs, so a run costs two atomics and one per change, not one per letter.
//   k_qual_lane / k_qual_lane_masked   a lane per read: its segments of up to kPileLaneOps operations
//   k_qual_wave / k_qual_wave_masked   a wave per 64 reads takes their longer segments one by one, 64 operations at a time (the
//                                      structure of pile_filter.hip's wave body)
// The pass is enqueued behind the pile kernels of the same add and reads the same batch -- under the duplicate filter the kept
// records.  Sums are taken modulo 2^32: with qv <= 93 < 2^7 a depth below 2^25 at a row is inside the contract.
#include "buffers.h"
#include "pile_shared.h"

namespace slamem {

namespace {

struct QualAcc {
    const TextPlanes* tpl;
    int32_t* diff;  // n + 1
    uint32_t* cnt;  // n x 6
    uint32_t n;
};

constexpr uint32_t kNoByte = 0x100u;  // no byte: the level is 0 because the row is excluded, not because of a letter

// an `=` run over rows [p, p + k) that shows letters [q, q + k) of the scanned strand, a text word (up to 64 rows) at a time as
// pile_eq_masked goes: `cur` is the level of the open stretch (0 outside one), `curb` the byte that set it.  An excluded row
// closes the stretch; a letter whose quality differs from cur moves the level by the difference; the run's end closes what is open.
template <bool kMasked>
__device__ __forceinline__ void qual_eq(const QualAcc& a, const QualRead& r, const PileLow& m, uint64_t p, uint64_t k, uint64_t q) {
    if (k == 0 || p >= a.n) return;
    if (p + k > a.n) k = a.n - p;
    if (q >= r.len) return;  // (a letter behind the read's end has no quality)
    if (r.len - q < k) k = r.len - q;
    const uint64_t e = p + k;  // <= n
    uint32_t cur = 0, curb = kNoByte;
    for (uint64_t x0 = p; x0 < e;) {
        const uint32_t sh = (uint32_t)(x0 & 63u);
        const uint32_t c = e - x0 < 64u - sh ? (uint32_t)(e - x0) : 64u - sh;
        const uint64_t in = c < 64u ? (1ull << c) - 1ull : ~0ull;
        const uint64_t t0 = q + (x0 - p);  // the letter of row x0
        uint64_t bad = a.tpl[x0 >> 6].nm >> sh;
        if constexpr (kMasked) bad |= lowq_letters(m, t0, c);
        bad &= in;  // bit i: row x0 + i
        uint32_t i = 0;
        while (i < c) {
            if ((bad >> i) & 1ull) {
                if (cur) atomicAdd(&a.diff[x0 + i], -(int32_t)cur);
                cur = 0;
                curb = kNoByte;
                const uint64_t good = ~bad & in & (~0ull << i);
                i = good ? (uint32_t)__builtin_ctzll(good) : c;
                continue;
            }
            const uint64_t stop = bad & (~0ull << i);
            const uint32_t lim = stop ? (uint32_t)__builtin_ctzll(stop) : c;  // the good rows from i on: [i, lim)
            if (curb != kNoByte) i += qual_same(r, t0 + i, lim - i, curb);
            if (i >= lim) continue;
            curb = qual_byte(r, t0 + i);
            const uint32_t v = qual_value(curb, r.off);
            if (v != cur) atomicAdd(&a.diff[x0 + i], (int32_t)(v - cur));
            cur = v;
            i++;
        }
        x0 += c;
    }
    if (cur) atomicAdd(&a.diff[e], -(int32_t)cur);
}

// one operation at (p, q): every write is checked against n.  D and I give Q nothing.
template <bool kMasked>
__device__ __forceinline__ void qual_op(const QualAcc& a, const PileRead& rd, const QualRead& r, const PileLow& m, uint32_t op, uint64_t p,
                                        uint64_t q) {
    const uint32_t code = op & 15u;
    const uint64_t k = op >> 4;
    if (code == kOpEq) {
        qual_eq<kMasked>(a, r, m, p, k, q);
    } else if (code == kOpX) {
        for (uint64_t j = 0; j < k && p + j < a.n; j++) {
            const uint32_t c = pile_letter(rd, q + j);  // (4 behind the read's end)
            if (c >= 4u) continue;
            if constexpr (kMasked) {
                if (lowq_letters(m, q + j, 1u)) continue;
            }
            const uint32_t v = qual_value(qual_byte(r, q + j), r.off);
            if (v) atomicAdd(&a.cnt[(p + j) * 6u + c], v);
        }
    }
}

template <bool kMasked>
__device__ __forceinline__ void qual_lane_body(const PileBatch& b, const QualAcc& a, const unsigned char* quals, uint32_t off,
                                               const uint64_t* lowq) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= b.nq) return;
    PileRead rd;
    if (!pile_contributes(b, r, rd)) return;
    const PileLow m = pile_low<kMasked>(b, rd, lowq);
    const QualRead qr = qual_read(b, rd, quals, off);
    const uint64_t s1 = b.roff[r + 1];
    for (uint64_t s = b.roff[r]; s < s1; s++) {
        const uint64_t o0 = b.ooff[s], o1 = b.ooff[s + 1];
        if (o1 <= o0 || o1 - o0 > kPileLaneOps) continue;
        const slamem_aln sg = b.segs[s];
        uint64_t p = sg.ref_pos, q = sg.query_pos;
        for (uint64_t i = o0; i < o1; i++) {
            const uint32_t op = b.ops[i];
            qual_op<kMasked>(a, rd, qr, m, op, p, q);
            p += pile_ref_step(op);
            q += pile_query_step(op);
        }
    }
}
__global__ void __launch_bounds__(256) k_qual_lane(PileBatch b, QualAcc a, const unsigned char* __restrict__ quals, uint32_t off) {
    qual_lane_body<false>(b, a, quals, off, nullptr);
}
__global__ void __launch_bounds__(256) k_qual_lane_masked(PileBatch b, QualAcc a, const unsigned char* __restrict__ quals, uint32_t off,
                                                          const uint64_t* __restrict__ lowq) {
    qual_lane_body<true>(b, a, quals, off, lowq);
}

template <bool kMasked>
__device__ __forceinline__ void qual_wave_body(const PileBatch& b, const QualAcc& a, const unsigned char* quals, uint32_t off,
                                               const uint64_t* lowq) {
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
            const PileLow m = pile_low<kMasked>(b, rd, lowq);
            const QualRead qr = qual_read(b, rd, quals, off);
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
                    if (have) qual_op<kMasked>(a, rd, qr, m, op, p + ri - rs, q + qi - qs);
                    p += __shfl(ri, 63, 64);
                    q += __shfl(qi, 63, 64);
                }
            }
        }
    }
}
__global__ void __launch_bounds__(64) k_qual_wave(PileBatch b, QualAcc a, const unsigned char* __restrict__ quals, uint32_t off) {
    qual_wave_body<false>(b, a, quals, off, nullptr);
}
__global__ void __launch_bounds__(64) k_qual_wave_masked(PileBatch b, QualAcc a, const unsigned char* __restrict__ quals, uint32_t off,
                                                         const uint64_t* __restrict__ lowq) {
    qual_wave_body<true>(b, a, quals, off, lowq);
}

}  // namespace

int pileup_has_quals(const slamem_pileup* pile) { return pile->qual != nullptr; }

int pileup_add_quals(slamem_pileup* pile, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                     const slamem_aln* segs_dev, const uint64_t* read_offsets_dev, const uint32_t* ops_dev, const uint64_t* op_offsets_dev,
                     const slamem_map* reads_dev, uint32_t min_mapq, const uint64_t* lowq_dev, const unsigned char* quals_dev,
                     uint32_t phred_offset, bool dedup, slamem_map* reads_keep_dev, uint8_t* dup_out_dev, hipStream_t stream) {
    if (dedup)
        SLAMEM_TRY(pileup_add_dedup(pile, queries_dev, offsets_dev, num_queries, segs_dev, read_offsets_dev, ops_dev, op_offsets_dev,
                                    reads_dev, min_mapq, lowq_dev, reads_keep_dev, dup_out_dev, stream));
    else
        SLAMEM_TRY(pileup_add_masked(pile, queries_dev, offsets_dev, num_queries, segs_dev, read_offsets_dev, ops_dev, op_offsets_dev,
                                     reads_dev, min_mapq, lowq_dev, stream));
    if (num_queries == 0) return SLAMEM_OK;
    PileBatch b;
    b.queries = static_cast<const unsigned char*>(queries_dev);
    b.offsets = offsets_dev;
    b.segs = segs_dev;
    b.roff = read_offsets_dev;
    b.ops = ops_dev;
    b.ooff = op_offsets_dev;
    b.reads = dedup ? reads_keep_dev : reads_dev;  // (the kept records: what the pile kernels of this add read)
    b.nq = num_queries;
    b.min_mapq = min_mapq;
    slamem_pileup* qp = pile->qual;
    const QualAcc a{pile->idx->view.tpl, qp->diff, qp->cnt, qp->n};
    const unsigned chunks = pile_grid(num_queries, 64);
    const dim3 lane_grid(pile_grid(num_queries, 256)), wave_grid(chunks < kPileWaveGrid ? chunks : kPileWaveGrid);
    qp->used.store(true, std::memory_order_relaxed);
    if (lowq_dev) {
        hipLaunchKernelGGL(k_qual_lane_masked, lane_grid, dim3(256), 0, stream, b, a, quals_dev, phred_offset, lowq_dev);
        SLAMEM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_qual_wave_masked, wave_grid, dim3(64), 0, stream, b, a, quals_dev, phred_offset, lowq_dev);
        SLAMEM_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_qual_lane, lane_grid, dim3(256), 0, stream, b, a, quals_dev, phred_offset);
        SLAMEM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_qual_wave, wave_grid, dim3(64), 0, stream, b, a, quals_dev, phred_offset);
        SLAMEM_HIP(hipGetLastError());
    }
    return SLAMEM_OK;
}

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_pileup_add_quals_device(slamem_pileup* pile, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                                   const slamem_aln* segs_dev, const uint64_t* read_offsets_dev, const uint32_t* ops_dev,
                                   const uint64_t* op_offsets_dev, const slamem_map* reads_dev, uint32_t min_mapq, const uint64_t* lowq_dev,
                                   const uint8_t* quals_dev, uint32_t phred_offset, int dedup, slamem_map* reads_keep_dev,
                                   uint8_t* dup_out_dev, void* stream) {
    if (!pile || !offsets_dev || !read_offsets_dev || !op_offsets_dev || !reads_dev || (dedup && !reads_keep_dev) ||
        (num_queries && (!queries_dev || !segs_dev || !ops_dev || !quals_dev))) {
        set_error("slamem_pileup_add_quals_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_pileup_add_quals_device"));
    if (!pile->qual) {
        set_error("slamem_pileup_add_quals_device: the quality sums of this accumulator are not enabled (slamem_pileup_enable_quals)");
        return SLAMEM_ERR_ARG;
    }
    if (dedup && !pile->dd) {
        set_error("slamem_pileup_add_quals_device: the duplicate filter of this accumulator is not enabled (slamem_pileup_enable_dedup)");
        return SLAMEM_ERR_ARG;
    }
    if (min_mapq > 60u) { set_error("slamem_pileup_add_quals_device: the minimum mapping quality is 0 to 60"); return SLAMEM_ERR_ARG; }
    if (phred_offset > 255u) { set_error("slamem_pileup_add_quals_device: the Phred offset is 0 to 255, not %u", phred_offset); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(pile->device));
    return pileup_add_quals(pile, queries_dev, offsets_dev, num_queries, segs_dev, read_offsets_dev, ops_dev, op_offsets_dev, reads_dev,
                            min_mapq, lowq_dev, quals_dev, phred_offset, dedup != 0, reads_keep_dev, dup_out_dev,
                            static_cast<hipStream_t>(stream));
}

}  // extern "C"
