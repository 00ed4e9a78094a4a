// stats_filter.hip -- -stats: the mapping QC table, SLAMEM_STATS_WORDS 64-bit counters in fixed sections (the
// table of include/slamem_hip.h), added up on the device behind the map kernels from the outputs of slamem_find_maps_device as
// they lie there.  Every number is a count, so the table is exact whatever the order of adds, streams and workgroups.
//
// One kernel, k_stats: a workgroup of 256 lanes takes 256 reads a trip, at least kStatsTrips trips (the grid is bounded by
// kStatsGrid), and keeps the whole table privately:
//   the sections behind TOTALS as 32-bit counters in LDS (12.4 KB), fed with LDS atomics;
//   TOTALS as sixteen 64-bit sums in each lane's registers, reduced by shuffles at the flush.
// A lane walks its read's segments of up to kPileLaneOps operations alone; the wave then takes the longer segments of its 64
// reads one by one, 64 operations a trip (the structure of pile_filter.hip's wave body), into the same LDS table.
//   `=` runs per cycle   a difference array in the CYC_ALN words: + 1 where the run's cycles start, - 1 behind their end, both
//                        below bin 511; the letters of cycle 511 and more go to a fold counter.  Scanned once at the flush.
//   X letters            one atomic each on CYC_MM (and SUB, Q_MM); CYC_ALN and Q_ALN get them at the flush, where
//                        CYC_ALN = scan(difference array) + CYC_MM and Q_ALN = (letters under `=`) + Q_MM.
//   qualities under `=`  the bytes are compared eight at a time (qual_same of pile_shared.h): one atomic per stretch of equal
//                        quality, with the stretch's length.
// The flush adds the non-zero bins to the global table with 64-bit atomicAdd.  OVERFLOW: every 32-bit bin is bounded by the
// weight of the reads walked since the last flush, weight = letters + operations + 3 per read; a workgroup sums the weights of a
// trip before it walks it, flushes first when the sum since the last flush would pass kStatsFlushAt = 2^31, and walks a trip
// that is heavier than that alone read by read with a flush behind each.
#include "buffers.h"
#include "pile_shared.h"

#include <stdlib.h>

struct slamem_stats {
    const slamem_index* idx;
    int device;
    unsigned long long* tab;  // SLAMEM_STATS_WORDS words on the device
    uint64_t flush_at;        // kStatsFlushAt (SLAMEM_STATS_FLUSH_AT: a smaller one, for tests of the flush in between)
};

namespace slamem {

namespace {

constexpr uint32_t kStatsBlock = 256;
constexpr uint32_t kStatsTrips = 4;     // trips a workgroup makes at least: a flush costs about what a few trips cost
constexpr unsigned kStatsGrid = 1024;   // workgroups at most: grid x SLAMEM_STATS_WORDS global atomics bound a batch's flushes
constexpr uint64_t kStatsFlushAt = 1ull << 31;

// the sections (words of the table)
constexpr uint32_t kTot = 0, kMapq = 24, kLen = 88, kNm = 600, kCycAln = 728, kCycMm = 1240, kCycIns = 1752, kCycDel = 2264, kSub = 2776,
                   kQAln = 2792, kQMm = 2888, kInsLen = 2984, kDelLen = 3048, kWords = 3112;
static_assert(kWords == SLAMEM_STATS_WORDS, "the sections fill the table");
constexpr uint32_t kLds = kWords - kMapq;  // the LDS table: word w of the table at w - kMapq
enum { T_READS, T_MAPPED, T_FWD, T_REV, T_COUNTED, T_SPLIT, T_SEGS, T_LETTERS, T_CLETTERS, T_EQ, T_X, T_INS, T_INSL, T_DEL, T_DELL, T_SEGL, T_N };

struct StatsCtx {
    uint32_t* tab;   // LDS
    uint32_t* fold;  // LDS: letters under `=` at cycle 511 and more
    const TextPlanes* tpl;
    uint64_t n;
    bool quals;
};

__device__ __forceinline__ void lds_add(const StatsCtx& c, uint32_t word, uint32_t v) { atomicAdd(&c.tab[word - kMapq], v); }

__device__ __forceinline__ uint32_t stats_bin(const PileRead& rd, uint64_t x) {  // the cycle's bin of letter x < len of the scanned strand
    const uint64_t cyc = rd.rev ? rd.len - 1u - x : x;
    return cyc < 511u ? (uint32_t)cyc : 511u;
}

// one operation at reference place p and letter q of the scanned strand.  Letters at or behind the read's end, which no
// mapping of the engine has, are not walked: no load leaves the read's own bytes.
__device__ __forceinline__ void stats_op(const StatsCtx& c, const PileRead& rd, const QualRead& qr, uint32_t op, uint64_t p, uint64_t q,
                                         uint64_t* t) {
    const uint32_t code = op & 15u;
    uint64_t k = op >> 4;
    if (code == kOpD) {
        t[T_DEL] += 1u;
        t[T_DELL] += k;
        lds_add(c, kDelLen + (k < 63u ? (uint32_t)k : 63u), 1u);
        if (q < rd.len) lds_add(c, kCycDel + stats_bin(rd, q), 1u);
        return;
    }
    if (code != kOpEq && code != kOpX && code != kOpI) return;
    if (code == kOpI) {
        t[T_INS] += 1u;
        t[T_INSL] += k;
        lds_add(c, kInsLen + (k < 63u ? (uint32_t)k : 63u), 1u);
    }
    if (q >= rd.len || k == 0) { if (code == kOpEq) t[T_EQ] += k; else if (code == kOpX) t[T_X] += k; return; }
    const uint64_t kw = rd.len - q < k ? rd.len - q : k;  // the letters walked
    if (code == kOpEq) {
        t[T_EQ] += k;
        // the cycles of letters [q, q + kw): [lo, hi]
        const uint64_t lo = rd.rev ? rd.len - q - kw : q, hi = lo + kw - 1u;
        if (lo >= 511u) {
            atomicAdd(c.fold, (uint32_t)kw);
        } else {
            lds_add(c, kCycAln + (uint32_t)lo, 1u);
            if (hi >= 511u) {
                lds_add(c, kCycAln + 511u, 0xFFFFFFFFu);
                atomicAdd(c.fold, (uint32_t)(hi - 510u));
            } else {
                lds_add(c, kCycAln + (uint32_t)hi + 1u, 0xFFFFFFFFu);
            }
        }
        if (c.quals) {
            for (uint64_t x = 0; x < kw;) {
                const uint32_t byte = qual_byte(qr, q + x);
                const uint64_t left = kw - x - 1u;
                uint32_t same = 1u;
                if (left) same += qual_same(qr, q + x + 1u, left < 0x40000000u ? (uint32_t)left : 0x40000000u, byte);
                lds_add(c, kQAln + qual_value(byte, qr.off), same);
                x += same;
            }
        }
    } else if (code == kOpX) {
        t[T_X] += k;
        for (uint64_t j = 0; j < kw; j++) {
            lds_add(c, kCycMm + stats_bin(rd, q + j), 1u);
            const uint32_t rl = pile_letter(rd, q + j);
            if (rl < 4u && p + j < c.n && !((c.tpl[(p + j) >> 6].nm >> ((p + j) & 63u)) & 1ull)) lds_add(c, kSub + 4u * md_text(c.tpl, c.n, p + j) + rl, 1u);
            if (c.quals) lds_add(c, kQMm + qual_value(qual_byte(qr, q + j), qr.off), 1u);
        }
    } else {
        for (uint64_t j = 0; j < kw; j++) lds_add(c, kCycIns + stats_bin(rd, q + j), 1u);
    }
}

// the segments of read r that a lane walks alone: those of up to kPileLaneOps operations
__device__ __forceinline__ void stats_lane_segments(const PileBatch& b, const StatsCtx& c, const PileRead& rd, const QualRead& qr, uint64_t r,
                                                    uint64_t* t) {
    const uint64_t s1 = b.roff[r + 1];
    for (uint64_t s = b.roff[r]; s < s1; s++) {
        const uint64_t o0 = b.ooff[s], o1 = b.ooff[s + 1];
        if (o1 <= o0 || o1 - o0 > kPileLaneOps) continue;
        const slamem_aln sg = b.segs[s];
        uint64_t p = sg.ref_pos, q = sg.query_pos;
        for (uint64_t i = o0; i < o1; i++) {
            const uint32_t op = b.ops[i];
            stats_op(c, rd, qr, op, p, q, t);
            p += pile_ref_step(op);
            q += pile_query_step(op);
        }
    }
}

// the longer segments of the wave's 64 reads, one by one, 64 operations a trip
__device__ __forceinline__ void stats_wave_segments(const PileBatch& b, const StatsCtx& c, const unsigned char* quals, uint32_t off, uint64_t r0,
                                                    bool big, uint32_t lane, uint64_t* t) {
    unsigned long long todo = __ballot(big);
    while (todo) {
        const uint32_t src = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint64_t rr = r0 + src;
        PileRead rd;
        (void)pile_contributes(b, rr, rd);  // (it does: its lane said so)
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
                if (have) stats_op(c, rd, qr, op, p + ri - rs, q + qi - qs, t);
                p += __shfl(ri, 63, 64);
                q += __shfl(qi, 63, 64);
            }
        }
    }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The workgroup's LDS table goes to the global one and is cleared; every lane of the workgroup calls it.  (Not inlined: three
// call sites, none of them hot.  The totals stay in their registers until the kernel's end: 64 bits do not overflow.)
__device__ __noinline__ void stats_flush(uint32_t* tab, uint32_t* fold, unsigned long long* g) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    __syncthreads();
    if (tid < 64u) {  // the difference array -> the letters under `=` per cycle below 511: eight entries a lane, then a wave scan
        uint32_t* d = tab + (kCycAln - kMapq) + 8u * lane;
        uint32_t v[8], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) { sum += d[i]; v[i] = sum; }
        const uint32_t before = (uint32_t)wave_scan_inclusive(sum, lane) - sum;
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) d[i] = v[i] + before;
    }
    __syncthreads();
    for (uint32_t w = tid; w < kLds; w += kStatsBlock) {
        const uint32_t word = w + kMapq;
        uint32_t v = tab[w];
        if (word >= kCycAln && word < kCycMm) v = (word == kCycAln + 511u ? *fold : v) + tab[w + (kCycMm - kCycAln)];  // (the scan ends at 0: every run is closed by bin 511)
        else if (word >= kQAln && word < kQMm) v += tab[w + (kQMm - kQAln)];
        if (v) atomicAdd(&g[word], (unsigned long long)v);
    }
    __syncthreads();
    for (uint32_t w = tid; w < kLds; w += kStatsBlock) tab[w] = 0u;
    if (tid == 0u) *fold = 0u;
    __syncthreads();
}

__global__ void __launch_bounds__(kStatsBlock) k_stats(PileBatch b, const TextPlanes* __restrict__ tpl, uint64_t n,
                                                       const unsigned char* __restrict__ quals, uint32_t off, uint64_t flush_at,
                                                       unsigned long long* __restrict__ g) {
    __shared__ uint32_t s_tab[kLds];
    __shared__ uint32_t s_fold;
    __shared__ unsigned long long s_trip, s_work;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t w = tid; w < kLds; w += kStatsBlock) s_tab[w] = 0u;
    if (tid == 0u) { s_fold = 0u; s_trip = 0ull; s_work = 0ull; }
    __syncthreads();
    const StatsCtx c{s_tab, &s_fold, tpl, n, quals != nullptr};
    uint64_t t[T_N];
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)T_N; i++) t[i] = 0;
    const uint64_t trips = (b.nq + kStatsBlock - 1u) / kStatsBlock;
    for (uint64_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const uint64_t r = trip * kStatsBlock + tid;
        // the read's own numbers, and its weight
        bool counted = false, big = false;
        PileRead rd = {nullptr, 0, false};
        uint64_t weight = 0;
        if (r < b.nq) {
            const slamem_map m = b.reads[r];
            const uint64_t len = b.offsets[r + 1] - b.offsets[r];
            t[T_READS] += 1u;
            t[T_LETTERS] += len;
            lds_add(c, kLen + (len < 511u ? (uint32_t)len : 511u), 1u);
            weight = 3u;  // (its own adds: LEN, MAPQ, NM)
            if (m.strand != 0u) {
                t[T_MAPPED] += 1u;
                t[T_FWD] += m.strand == 2u ? 0u : 1u;
                t[T_REV] += m.strand == 2u ? 1u : 0u;
                lds_add(c, kMapq + (m.mapq < 63u ? m.mapq : 63u), 1u);
            }
            counted = pile_contributes(b, r, rd);
            if (counted) {
                const uint64_t s0 = b.roff[r], s1 = b.roff[r + 1];
                uint64_t edits = 0, ql = 0;
                for (uint64_t s = s0; s < s1; s++) {
                    const slamem_aln sg = b.segs[s];
                    edits += sg.edits;
                    ql += sg.query_len;
                    big = big || (b.ooff[s + 1] > b.ooff[s] && b.ooff[s + 1] - b.ooff[s] > kPileLaneOps);
                }
                t[T_COUNTED] += 1u;
                t[T_SPLIT] += s1 - s0 > 1u ? 1u : 0u;
                t[T_SEGS] += s1 - s0;
                t[T_CLETTERS] += len;
                t[T_SEGL] += ql;
                lds_add(c, kNm + (edits < 127u ? (uint32_t)edits : 127u), 1u);
                weight += len + (s1 > s0 ? b.ooff[s1] - b.ooff[s0] : 0u);
            }
        }
        // OVERFLOW: the trip's weight, before it is walked
        const uint64_t wsum = wave_sum(weight);
        if (lane == 0u && wsum) atomicAdd(&s_trip, (unsigned long long)wsum);
        __syncthreads();
        const uint64_t tw = s_trip, work = s_work;
        const bool alone = tw > flush_at;
        if (work && work + tw > flush_at) stats_flush(s_tab, &s_fold, g);  // (uniform: every lane read the same two words)
        else __syncthreads();
        if (tid == 0u) { s_work = alone ? 0ull : (work && work + tw > flush_at) ? tw : work + tw; s_trip = 0ull; }
        const QualRead qr = qual_read(b, rd, quals, off);
        // a trip heavier than the bound: read by read, a flush behind each (the wave of the read takes its longer segments)
        const uint32_t rounds = alone ? kStatsBlock : 1u;
        for (uint32_t i = 0; i < rounds; i++) {
            const bool mine = !alone || tid == i;
            if (counted && mine) stats_lane_segments(b, c, rd, qr, r, t);
            stats_wave_segments(b, c, quals, off, trip * kStatsBlock + (tid & ~63u), big && mine, lane, t);
            if (alone) stats_flush(s_tab, &s_fold, g);
        }
        __syncthreads();
    }
    stats_flush(s_tab, &s_fold, g);
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)T_N; i++) {
        const uint64_t sum = wave_sum(t[i]);
        if (lane == 0u && sum) atomicAdd(&g[kTot + i], (unsigned long long)sum);
    }
}

__global__ void __launch_bounds__(256) k_stats_add_table(unsigned long long* __restrict__ g, const unsigned long long* __restrict__ src) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < kWords && src[w]) atomicAdd(&g[w], src[w]);
}

}  // namespace

int stats_device(const slamem_stats* st) { return st->device; }

int stats_add(slamem_stats* st, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries, const slamem_aln* segs_dev,
              const uint64_t* read_offsets_dev, const uint32_t* ops_dev, const uint64_t* op_offsets_dev, const slamem_map* reads_dev,
              const unsigned char* quals_dev, uint32_t phred_offset, uint32_t min_mapq, hipStream_t stream) {
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
    const uint64_t trips = ((uint64_t)num_queries + kStatsBlock - 1u) / kStatsBlock, want = (trips + kStatsTrips - 1u) / kStatsTrips;
    const unsigned grid = want < kStatsGrid ? (unsigned)want : kStatsGrid;
    hipLaunchKernelGGL(k_stats, dim3(grid), dim3(kStatsBlock), 0, stream, b, st->idx->view.tpl, (uint64_t)st->idx->view.n, quals_dev, phred_offset,
                       st->flush_at, st->tab);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_stats_create(const slamem_index* idx, slamem_stats** out) {
    if (!idx || !out) { set_error("slamem_stats_create: null argument"); return SLAMEM_ERR_ARG; }
    *out = nullptr;
    SLAMEM_HIP(hipSetDevice(idx->device));
    slamem_stats* st = new (std::nothrow) slamem_stats();
    if (!st) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    st->idx = idx;
    st->device = idx->device;
    st->tab = nullptr;
    st->flush_at = kStatsFlushAt;
    const char* v = getenv("SLAMEM_STATS_FLUSH_AT");
    if (v && atoll(v) > 0 && (uint64_t)atoll(v) < kStatsFlushAt) st->flush_at = (uint64_t)atoll(v);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->tab), kWords * 8u);
    if (e == hipSuccess) e = hipMemset(st->tab, 0, kWords * 8u);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (st->tab) (void)hipFree(st->tab);
        delete st;
        return hip_fail(e, "slamem_stats_create", __FILE__, __LINE__);
    }
    *out = st;
    return SLAMEM_OK;
}

int slamem_stats_free(slamem_stats* st) {
    if (!st) return SLAMEM_OK;
    (void)hipSetDevice(st->device);
    if (st->tab) (void)hipFree(st->tab);
    delete st;
    return SLAMEM_OK;
}

int slamem_stats_reset(slamem_stats* st) {
    if (!st) { set_error("slamem_stats_reset: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(st->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (adds of any stream that are still on their way belong to the table that goes)
    SLAMEM_HIP(hipMemset(st->tab, 0, kWords * 8u));
    SLAMEM_HIP(hipDeviceSynchronize());
    return SLAMEM_OK;
}

int slamem_stats_add_device(slamem_stats* st, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                            const slamem_aln* segs_dev, const uint64_t* read_offsets_dev, const uint32_t* ops_dev,
                            const uint64_t* op_offsets_dev, const slamem_map* reads_dev, const uint8_t* quals_dev, uint32_t phred_offset,
                            uint32_t min_mapq, void* stream) {
    if (!st || !offsets_dev || !read_offsets_dev || !op_offsets_dev || !reads_dev || (num_queries && (!queries_dev || !segs_dev || !ops_dev))) {
        set_error("slamem_stats_add_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    if (min_mapq > 60u) { set_error("slamem_stats_add_device: the minimum mapping quality is 0 to 60"); return SLAMEM_ERR_ARG; }
    if (phred_offset > 126u) { set_error("slamem_stats_add_device: the Phred offset is 0 to 126, not %u", phred_offset); return SLAMEM_ERR_ARG; }
    if (!st->idx->view.tpl) {
        set_error("slamem_stats_add_device: the substitution table takes the reference letters from the text planes of the index, and "
                  "this index has none (the compact layout, or one built with the seed sections switched off)");
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_HIP(hipSetDevice(st->device));
    return stats_add(st, queries_dev, offsets_dev, num_queries, segs_dev, read_offsets_dev, ops_dev, op_offsets_dev, reads_dev, quals_dev,
                     phred_offset, min_mapq, static_cast<hipStream_t>(stream));
}

int slamem_stats_table_device(slamem_stats* st, uint64_t* out_dev, void* stream) {
    if (!st || !out_dev) { set_error("slamem_stats_table_device: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(st->device));
    SLAMEM_HIP(hipMemcpyAsync(out_dev, st->tab, kWords * 8u, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return SLAMEM_OK;
}

int slamem_stats_table_host(slamem_stats* st, uint64_t* out) {
    if (!st || !out) { set_error("slamem_stats_table_host: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(st->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    SLAMEM_HIP(hipMemcpy(out, st->tab, kWords * 8u, hipMemcpyDeviceToHost));
    return SLAMEM_OK;
}

int slamem_stats_add_table_host(slamem_stats* st, const uint64_t* table) {
    if (!st || !table) { set_error("slamem_stats_add_table_host: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(st->device));
    DevBuf<unsigned long long> d;
    SLAMEM_TRY(d.reserve(kWords));
    SLAMEM_HIP(hipMemcpy(d.get(), table, kWords * 8u, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_stats_add_table, dim3((kWords + 255u) / 256u), dim3(256), 0, nullptr, st->tab, (const unsigned long long*)d.get());
    SLAMEM_HIP(hipGetLastError());
    SLAMEM_HIP(hipDeviceSynchronize());
    return SLAMEM_OK;
}

}  // extern "C"
