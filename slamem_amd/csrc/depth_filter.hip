// depth_filter.hip -- -depth: the depth of coverage d(p) = A+C+G+T+D of the pileup in its run-length form, and
// prefix sums of it at rows the caller names.  With levels t_1 < ... < t_m the value of a row is v(p) = #{i : t_i <= d(p)}, without
// levels v(p) = d(p); row p of the range [first, end) is a head iff p == first or v(p) != v(p - 1); the result is the heads in
// ascending p as records {pos, value}, and for every bound b the pair (sum of d, rows with d >= min_depth) over rows [first, b).
//   (pile_tile_prefix)   the sums of diff in front of every tile of kPileTile rows
//   k_depth_count        a workgroup per tile: d of its rows from diff, tile, cnt and the text's letter as k_pile_counts forms the
//                        rows, and three numbers: the heads, the sum of d, the rows with d >= min_depth (a lane takes 8 rows, a
//                        wave scan of the lanes' sums, the four waves through LDS)
//   (pile_scan_counts)   three times: each number's offset per tile, with the total behind them
//   k_depth_emit         a workgroup per tile: the same again, the waves' sums now as offsets, the heads below `capacity`, and cum[] of the
//                        bounds that lie in the tile (a binary search for the first of them, then a walk)
//   k_depth_bounds_edge  cum[] of a bound at `end`: the totals
// The first row of a tile needs v of the row in front of it: that row's match is the tile's exclusive prefix, its counters and
// its letter are one more row to read.  Nothing of the accumulator is written: the three numbers per tile are scratch of the
// read-out.
#include "buffers.h"
#include "pile_shared.h"

#include <new>

namespace slamem {

struct DepthScratch {
    uint64_t* num;   // 3 columns of n / kPileTile + 2 words: heads, sum of d, covered rows per tile; after the scans the offsets
    uint64_t words;  // of a column
};

namespace {

struct DepthLevels {
    uint32_t t[16];
    uint32_t m;
};

struct DepthTile {
    uint32_t match[kPileTile];  // the sum of diff[0 .. p]; afterwards the low word of d(p)
    uint8_t code[kPileTile];    // the text's letter, 4: none of A,C,G,T; afterwards the high word of d(p) (0 .. 4)
    uint64_t front;             // d of the row in front of the tile (base > first)
    uint64_t wsum[8];
};

// the text's letter at x (x < n): A 0, C 1, G 2, T 3; anything else 4
__device__ __forceinline__ uint32_t depth_text(const TextPlanes* __restrict__ tpl, uint64_t x) {
    const TextPlanes* u = tpl + (x >> 6);
    const uint32_t bit = (uint32_t)(x & 63u);
    if ((u->nm >> bit) & 1ull) return 4u;
    return (uint32_t)((u->p0 >> bit) & 1ull) | ((uint32_t)((u->p1 >> bit) & 1ull) << 1);
}

// d of row x: the five counters as the read-out gives them -- match on top of the column of the text's letter, modulo 2^32 as
// every counter -- summed in 64 bits
__device__ __forceinline__ uint64_t depth_row(const uint32_t* __restrict__ cnt, uint64_t x, uint32_t letter, uint32_t match) {
    const uint2* r = reinterpret_cast<const uint2*>(cnt + x * 6u);  // (24 bytes a row: 8-byte aligned)
    const uint2 a = r[0], b = r[1];
    uint32_t c[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) c[k] += letter == k ? match : 0u;
    return (uint64_t)c[0] + c[1] + c[2] + c[3] + r[2].x;
}

__device__ __forceinline__ uint64_t depth_value(uint64_t d, const DepthLevels& lv) {
    if (lv.m == 0u) return d;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16u; i++) v += i < lv.m && lv.t[i] <= d ? 1u : 0u;
    return v;
}

__device__ __forceinline__ uint64_t depth_at(const DepthTile& s, uint32_t at) { return ((uint64_t)s.code[at] << 32) | s.match[at]; }

// tile t of a read-out of rows [first, end) (end <= n): d of its rows inside the range into s.match / s.code (0 outside), d of the
// row in front of the tile into s.front.  The sums of diff are staged as pile_filter.hip stages them (a lane takes kPileTile / 256
// consecutive entries); the rows are then taken 256 apart, so a wave reads 64 neighbouring rows.  Ends with a barrier.
__device__ __forceinline__ void depth_tile_rows(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t t,
                                                uint64_t first, uint64_t end, DepthTile& s) {
    const uint64_t base = t * kPileTile;
    constexpr uint32_t per = kPileTile / 256u;
    uint32_t v[per], run = 0;
    const uint64_t x0 = base + (uint64_t)threadIdx.x * per;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        run += x0 + j < end ? (uint32_t)diff[x0 + j] : 0u;
        v[j] = run;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = run;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63u) s.wsum[wave] = inc;
    __syncthreads();
    uint32_t before = tile[t] + inc - run;
    for (uint32_t w = 0; w < wave; w++) before += (uint32_t)s.wsum[w];
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        const uint64_t x = x0 + j;
        const uint32_t at = threadIdx.x * per + j;
        s.match[at] = before + v[j];
        s.code[at] = (uint8_t)(x < end ? depth_text(tpl, x) : 4u);
    }
    if (threadIdx.x == 0 && base > first) s.front = depth_row(cnt, base - 1u, depth_text(tpl, base - 1u), tile[t]);  // (first < base < end)
    __syncthreads();
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        const uint32_t at = j * 256u + threadIdx.x;  // (this lane's entry alone: read, then replaced)
        const uint64_t x = base + at;
        const uint64_t d = x >= lo && x < hi ? depth_row(cnt, x, s.code[at], s.match[at]) : 0ull;
        s.match[at] = (uint32_t)d;
        s.code[at] = (uint8_t)(d >> 32);
    }
    __syncthreads();
}

// is row base + at (inside [lo, hi)) a head?  d: its depth
__device__ __forceinline__ bool depth_head(const DepthTile& s, uint64_t base, uint32_t at, uint64_t first, uint64_t d, const DepthLevels& lv) {
    if (base + at == first) return true;
    return depth_value(d, lv) != depth_value(at ? depth_at(s, at - 1u) : s.front, lv);
}

// what a lane's kPileTile / 256 consecutive rows of the staged tile add: d of each (0 outside [lo, hi)), bit j of `head` for a head
// among them, the heads and the rows with d >= min_depth as the two halves of hc (both at most kPileTile: one sum or scan serves
// the two), and the sum of d.  Both kernels take the rows this way, so what is counted is what is written.
__device__ __forceinline__ void depth_lane_rows(const DepthTile& s, uint64_t base, uint64_t lo, uint64_t hi, uint64_t first,
                                                const DepthLevels& lv, uint32_t min_depth, uint64_t (&d)[kPileTile / 256u], uint32_t& head,
                                                uint64_t& hc, uint64_t& sd) {
    constexpr uint32_t per = kPileTile / 256u;
    const uint32_t at0 = threadIdx.x * per;
    uint32_t nh = 0, nc = 0;
    head = 0;
    sd = 0;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        const uint32_t at = at0 + j;
        const bool in = base + at >= lo && base + at < hi;
        d[j] = depth_at(s, at);
        if (in && depth_head(s, base, at, first, d[j], lv)) { head |= 1u << j; nh++; }
        nc += in && d[j] >= min_depth ? 1u : 0u;
        sd += d[j];
    }
    hc = ((uint64_t)nh << 32) | nc;
}

// a workgroup per tile of rows: num[c * words + blockIdx.x] = the heads, the sum of d, the rows with d >= min_depth of the tile's
// rows inside [first, end)
__global__ void __launch_bounds__(256) k_depth_count(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t tile0,
                                                     uint64_t first, uint64_t end, DepthLevels lv, uint32_t min_depth,
                                                     uint64_t* __restrict__ num, uint64_t words) {
    __shared__ DepthTile s;
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile;
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    depth_tile_rows(diff, cnt, tile, tpl, t, first, end, s);
    uint64_t d[kPileTile / 256u], hc, sd;
    uint32_t head;
    depth_lane_rows(s, base, lo, hi, first, lv, min_depth, d, head, hc, sd);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t ihc = wave_scan_inclusive(hc, lane), isd = wave_scan_inclusive(sd, lane);
    if (lane == 63u) { s.wsum[wave] = ihc; s.wsum[4u + wave] = isd; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint64_t thc = s.wsum[0] + s.wsum[1] + s.wsum[2] + s.wsum[3];
    num[blockIdx.x] = thc >> 32;
    num[words + blockIdx.x] = s.wsum[4] + s.wsum[5] + s.wsum[6] + s.wsum[7];
    num[2u * words + blockIdx.x] = (uint32_t)thc;
}

// the first j with bounds[j] >= x (m: none); the same in every lane
__device__ __forceinline__ uint64_t depth_first_bound(const uint64_t* __restrict__ bounds, uint64_t m, uint64_t x) {
    uint64_t a = 0, b = m;
    while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (bounds[mid] < x) a = mid + 1u; else b = mid;
    }
    return a;
}

// a workgroup per tile: its heads go to num[blockIdx.x] + the heads of the tile in front of them, those at or behind `capacity`
// are dropped; cum[j] of every bound inside the tile's part of [first, end) is the pair of the tile's offsets plus what the tile's
// rows in front of the bound add
__global__ void __launch_bounds__(256) k_depth_emit(const int32_t* __restrict__ diff, const uint32_t* __restrict__ cnt,
                                                    const uint32_t* __restrict__ tile, const TextPlanes* __restrict__ tpl, uint64_t tile0,
                                                    uint64_t first, uint64_t end, DepthLevels lv, uint32_t min_depth,
                                                    const uint64_t* __restrict__ num, uint64_t words, uint64_t capacity,
                                                    slamem_depth_run* __restrict__ runs, const uint64_t* __restrict__ bounds, uint64_t m,
                                                    uint64_t* __restrict__ cum) {
    __shared__ DepthTile s;
    __shared__ uint64_t pre[kPileTile];  // the sum of d over the tile's rows of the range in front of the row
    __shared__ uint16_t prc[kPileTile];  // of those the rows with d >= min_depth
    const uint64_t t = tile0 + blockIdx.x, base = t * kPileTile;
    const uint64_t lo = base > first ? base : first, hi = base + kPileTile < end ? base + kPileTile : end;
    const uint64_t out0 = num[blockIdx.x];
    const uint64_t j0 = depth_first_bound(bounds, m, lo);
    const bool bound_here = j0 < m && bounds[j0] < hi;
    if (!bound_here && (num[blockIdx.x + 1] == out0 || out0 >= capacity)) return;  // (the whole workgroup: nothing to write)
    depth_tile_rows(diff, cnt, tile, tpl, t, first, end, s);
    constexpr uint32_t per = kPileTile / 256u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, at0 = threadIdx.x * per;
    uint64_t d[per], hc, sd;
    uint32_t head;
    depth_lane_rows(s, base, lo, hi, first, lv, min_depth, d, head, hc, sd);
    const uint64_t ihc = wave_scan_inclusive(hc, lane), isd = wave_scan_inclusive(sd, lane);
    if (lane == 63u) { s.wsum[wave] = ihc; s.wsum[4u + wave] = isd; }
    __syncthreads();
    uint64_t bhc = ihc - hc, bsd = isd - sd;
    for (uint32_t w = 0; w < wave; w++) { bhc += s.wsum[w]; bsd += s.wsum[4u + w]; }
    uint64_t o = out0 + (bhc >> 32);
    uint32_t c = (uint32_t)bhc;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        const uint32_t at = at0 + j;
        pre[at] = bsd;
        prc[at] = (uint16_t)c;
        if ((head >> j) & 1u) {
            if (o < capacity) runs[o] = slamem_depth_run{base + at, depth_value(d[j], lv)};
            o++;
        }
        bsd += d[j];
        c += base + at >= lo && base + at < hi && d[j] >= min_depth ? 1u : 0u;
    }
    if (!bound_here) return;
    __syncthreads();
    const uint64_t sum0 = num[words + blockIdx.x], cov0 = num[2u * words + blockIdx.x];
    for (uint64_t j = j0 + threadIdx.x; j < m; j += 256u) {
        const uint64_t b = bounds[j];
        if (b >= hi) break;  // (ascending: so are the bounds of the lanes behind this one)
        if (b < lo) continue;
        cum[2u * j] = sum0 + pre[b - base];
        cum[2u * j + 1u] = cov0 + prc[b - base];
    }
}

// a lane per bound: one at `end` gets the totals (0 without them: an empty range)
__global__ void __launch_bounds__(256) k_depth_bounds_edge(const uint64_t* __restrict__ bounds, uint64_t m, uint64_t end,
                                                           const uint64_t* __restrict__ sum, const uint64_t* __restrict__ cov,
                                                           uint64_t* __restrict__ cum) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= m || bounds[j] != end) return;
    cum[2u * j] = sum ? *sum : 0ull;
    cum[2u * j + 1u] = cov ? *cov : 0ull;
}

int depth_scratch(slamem_pileup* pile) {
    if (pile->depth) return SLAMEM_OK;
    DepthScratch* c = new (std::nothrow) DepthScratch();
    if (!c) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    c->num = nullptr;
    c->words = (uint64_t)pile->n / kPileTile + 2;
    pile->depth = c;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->num), c->words * 3 * sizeof(uint64_t));
    if (e != hipSuccess) {
        depth_free(pile);
        return hip_fail(e, "slamem_pileup_depth_runs_device", __FILE__, __LINE__);
    }
    return SLAMEM_OK;
}

// range, levels and least depth as both variants refuse them; `fn` names the caller in the message
int depth_check(const char* fn, const slamem_pileup* pile, uint64_t first, uint64_t count, const uint32_t* levels, uint32_t num_levels,
                uint32_t min_depth) {
    if (first > pile->n || count > pile->n - first) {
        set_error("%s: rows %llu .. %llu + %llu lie outside the text's %u", fn, (unsigned long long)first, (unsigned long long)first,
                  (unsigned long long)count, pile->n);
        return SLAMEM_ERR_ARG;
    }
    if (num_levels > 16u) { set_error("%s: at most 16 levels, not %u", fn, num_levels); return SLAMEM_ERR_ARG; }
    if (num_levels && !levels) { set_error("%s: null argument", fn); return SLAMEM_ERR_ARG; }
    for (uint32_t i = 0; i < num_levels; i++)
        if (levels[i] == 0u || (i && levels[i] <= levels[i - 1u])) {
            set_error("%s: the levels are at least 1 and ascend strictly; level %u is %u", fn, i, levels[i]);
            return SLAMEM_ERR_ARG;
        }
    if (min_depth == 0u || min_depth >= 0x80000000u) {
        set_error("%s: the least depth is 1 to 2^31 - 1, not %u", fn, min_depth);
        return SLAMEM_ERR_ARG;
    }
    return SLAMEM_OK;
}

}  // namespace

void depth_free(slamem_pileup* pile) {
    DepthScratch* c = pile->depth;
    if (!c) return;
    if (c->num) (void)hipFree(c->num);
    delete c;
    pile->depth = nullptr;
}

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_pileup_depth_runs_device(slamem_pileup* pile, uint64_t first, uint64_t count, const uint32_t* levels, uint32_t num_levels,
                                    uint32_t min_depth, uint64_t capacity, slamem_depth_run* runs_dev, const uint64_t* bounds_dev,
                                    uint64_t m, uint64_t* cum_dev, uint64_t* total_out, void* stream) {
    if (!pile || !total_out || (capacity && !runs_dev) || (m && (!bounds_dev || !cum_dev))) {
        set_error("slamem_pileup_depth_runs_device: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    int rc = depth_check("slamem_pileup_depth_runs_device", pile, first, count, levels, num_levels, min_depth);
    if (rc != SLAMEM_OK) return rc;
    SLAMEM_HIP(hipSetDevice(pile->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t end = first + count;
    if (count == 0) {  // no row, no run: every bound inside the range is `first`
        if (m) {
            hipLaunchKernelGGL(k_depth_bounds_edge, dim3(pile_grid(m, 256)), dim3(256), 0, st, bounds_dev, m, end, (const uint64_t*)nullptr,
                               (const uint64_t*)nullptr, cum_dev);
            SLAMEM_HIP(hipGetLastError());
        }
        return SLAMEM_OK;
    }
    rc = depth_scratch(pile);
    if (rc != SLAMEM_OK) return rc;
    DepthScratch* c = pile->depth;
    DepthLevels lv;
    for (uint32_t i = 0; i < 16u; i++) lv.t[i] = i < num_levels ? levels[i] : 0u;
    lv.m = num_levels;
    const uint64_t tiles = (end + kPileTile - 1) / kPileTile, tile0 = first / kPileTile, mine = tiles - tile0;  // (mine + 1 <= words)
    rc = pile_tile_prefix(pile, end, st);
    if (rc != SLAMEM_OK) return rc;
    const TextPlanes* tpl = pile->idx->view.tpl;
    hipLaunchKernelGGL(k_depth_count, dim3((unsigned)mine), dim3(256), 0, st, (const int32_t*)pile->diff, (const uint32_t*)pile->cnt,
                       (const uint32_t*)pile->tile, tpl, tile0, first, end, lv, min_depth, c->num, c->words);
    SLAMEM_HIP(hipGetLastError());
    for (uint32_t k = 0; k < 3u; k++) {
        rc = pile_scan_counts(c->num + k * c->words, mine, st);
        if (rc != SLAMEM_OK) return rc;
    }
    if (capacity || m) {  // heads behind `capacity` are dropped on the device, so the pass runs before the total is known
        hipLaunchKernelGGL(k_depth_emit, dim3((unsigned)mine), dim3(256), 0, st, (const int32_t*)pile->diff, (const uint32_t*)pile->cnt,
                           (const uint32_t*)pile->tile, tpl, tile0, first, end, lv, min_depth, (const uint64_t*)c->num, c->words, capacity,
                           runs_dev, bounds_dev, m, cum_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    if (m) {
        hipLaunchKernelGGL(k_depth_bounds_edge, dim3(pile_grid(m, 256)), dim3(256), 0, st, bounds_dev, m, end,
                           (const uint64_t*)(c->num + c->words + mine), (const uint64_t*)(c->num + 2 * c->words + mine), cum_dev);
        SLAMEM_HIP(hipGetLastError());
    }
    uint64_t total = 0;  // the call's one host round trip
    SLAMEM_HIP(hipMemcpyAsync(&total, c->num + mine, 8, hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipStreamSynchronize(st));
    *total_out = total;
    if (total > capacity) {
        set_error("slamem_pileup_depth_runs_device: the range has %llu runs, the buffer holds %llu", (unsigned long long)total,
                  (unsigned long long)capacity);
        return SLAMEM_ERR_CAPACITY;
    }
    return SLAMEM_OK;
}

int slamem_pileup_depth_runs_host(slamem_pileup* pile, uint64_t first, uint64_t count, const uint32_t* levels, uint32_t num_levels,
                                  uint32_t min_depth, uint64_t capacity, slamem_depth_run* runs, const uint64_t* bounds, uint64_t m,
                                  uint64_t* cum, uint64_t* total_out) {
    if (!pile || !total_out || (capacity && !runs) || (m && (!bounds || !cum))) {
        set_error("slamem_pileup_depth_runs_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    *total_out = 0;
    int rc = depth_check("slamem_pileup_depth_runs_host", pile, first, count, levels, num_levels, min_depth);
    if (rc != SLAMEM_OK) return rc;
    for (uint64_t j = 0; j < m; j++) {
        if (bounds[j] < first || bounds[j] > first + count || (j && bounds[j] < bounds[j - 1u])) {
            set_error("slamem_pileup_depth_runs_host: bound %llu (entry %llu) lies outside rows %llu .. %llu or in front of the bound before it",
                      (unsigned long long)bounds[j], (unsigned long long)j, (unsigned long long)first, (unsigned long long)(first + count));
            return SLAMEM_ERR_ARG;
        }
    }
    SLAMEM_HIP(hipSetDevice(pile->device));
    SLAMEM_HIP(hipDeviceSynchronize());  // (the adds of every stream so far are in the table that is read)
    const uint64_t room = capacity < count ? capacity : count;  // (a range has at most a run per row)
    DevBuf<slamem_depth_run> d;
    DevBuf<uint64_t> bd;  // the m bounds, then two words of sums for each
    if (room) SLAMEM_TRY(d.reserve(room));
    if (m) SLAMEM_TRY(bd.reserve(m * 3));
    uint64_t* bdev = bd.get();
    if (m) SLAMEM_HIP(hipMemcpy(bdev, bounds, m * 8, hipMemcpyHostToDevice));
    rc = slamem_pileup_depth_runs_device(pile, first, count, levels, num_levels, min_depth, room, d.get(), bdev, m, m ? bdev + m : nullptr,
                                         total_out, nullptr);
    if (rc != SLAMEM_OK && rc != SLAMEM_ERR_CAPACITY) return rc;
    // (the runs that fitted go back with SLAMEM_ERR_CAPACITY too; the call's code comes before a failed copy's)
    const uint64_t got = *total_out < room ? *total_out : room;
    hipError_t e = hipDeviceSynchronize();
    if (got && e == hipSuccess) e = hipMemcpy(runs, d.get(), got * sizeof(slamem_depth_run), hipMemcpyDeviceToHost);
    if (m && e == hipSuccess) e = hipMemcpy(cum, bdev + m, m * 16, hipMemcpyDeviceToHost);
    if (rc == SLAMEM_OK && e != hipSuccess) return hip_fail(e, "slamem_pileup_depth_runs_host", __FILE__, __LINE__);
    return rc;
}

}  // extern "C"
