// stream.hip -- host-to-host MEM retrieval, pipelined: the form of GetMatches' query loop (slamem.c:90-207) that a
// front end with its reads in HOST memory calls.  SURVEY.md 8(d) defines the path's metric on exactly this boundary
// ("reads resident in host memory -> MEM triples in host memory").
//
// A slamem_stream is a four-stage pipeline over `slots` (2-8) sets of buffers, each stage a host thread with its own HIP
// stream, each taking the batches in submission order:
//   UPLOAD    the batch's characters and offsets to the device (straight from the caller's memory: at full PCIe rate when
//             that memory is pinned, slamem_pinned_alloc)
//   PREPARE   work-item tables (the stage's one host round trip), K8a prefilter, work list, K7q packing
//   SEARCH    K8 and K9 of ALL batches back to back on one stream, with no host round trip in between: the thread only
//             enqueues (the preparation is awaited on the device, hipStreamWaitEvent) and never waits for a result
//   DOWNLOAD  waits for the batch's K9 (event), reads its totals, copies MEMs and block offsets into pinned host memory
// K8 is a persistent kernel that takes every wave slot of the chip; what it leaves idle is its tail (the last strands of
// its waves, ~1 ms whatever the batch size).  The preparation of the NEXT batches runs on its own stream, so the hardware
// puts its workgroups exactly where K8's waves retire, and the next K8 is already queued behind K9.  (Round 2 ran each
// batch's whole chain, with three host round trips, on one of two alternating search threads: the second thread's small
// kernels and memsets sat behind the first one's K8 until its tail and the chain after them was exposed -- 3.7 ms per
// million-read batch where the kernels need 2.9; measured with rocprofv3 --kernel-trace, profiles/r03_host_leg_timeline.txt.
// One thread per SLOT doing everything in turn was measured before that: the slots fall into lockstep, 62 ms.)
// -pile (match type 8) is -paf whose segments stay on the device: the download stage, once the batch's totals have shown that
// its result stands, enqueues the add to the accumulator (pile_filter.hip) on its stream and copies out the read records only.
// With -dedup (slamem_stream_set_dedup) that add goes through the duplicate filter (dedup_filter.hip) and a flag per read comes back.
// No CPU fallback: every batch is searched on the GPU.
//
// WHO OWNS WHAT.  Every buffer of a slot is a DevBuf or a PinnedBuf (buffers.h): freed by its destructor, grown by reserve(),
// which lets the old memory go first.  The stage that uses a buffer reserves it on the slot's first batch -- nothing is
// allocated at slamem_stream_create, and a batch no larger than the ones before allocates and frees nothing.
//   upload    the inputs: letters, record offsets, block offsets, read records (and planes, unit counts, mask words)
//   prepare   the outputs, sized by the inputs' room: rows, workspace, -ext's column, -aln's segments and operations
//   download  the MD arrays, -dedup's records and flags, and all pinned host memory; the outputs again when a batch's totals did not fit
// INPUTS REGROWN => OUTPUTS DROPPED: where the upload stage regrows a slot's inputs it drops every output buffer
// (drop_outputs), and the prepare stage, which finds no workspace, sizes them for the new room.
// The end of a stream (teardown(): destroy, and a create that failed half way): every HIP stream waited for, then the slots
// with their buffers, events and jobs, then the HIP streams.
#include "buffers.h"
#include "common.h"
#include "prims.h"

#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>

namespace slamem {

namespace {

enum SlotState { FREE = 0, QUEUED = 1, UPLOADED = 2, PREPARED = 3, LAUNCHED = 4, DONE = 5, RETURNED = 6,
                 K8_ISSUED = 7 };  // K8 enqueued with its lanes passed on; K9 follows behind the next batch's K8 (then LAUNCHED)
constexpr int kMaxSlots = 8;
constexpr int kThreads = 4;  // upload, prepare, search, download
enum { T_UP = 0, T_PREP = 1, T_SEARCH = 2, T_DOWN = 3 };

struct Slot {
    int state = FREE;
    // The batch's INPUTS on the device, allocated by the upload stage: letters (cap_chars of them behind kFront bytes), record
    // offsets, and the two arrays a record each that the search writes -- block offsets, -paf's read records -- (cap_q records).
    // cap_chars and cap_q are what the kernels and the prepare stage are told; both are 0 until all of these are there.
    DevBuf<char> d_q;
    DevBuf<uint64_t> d_off, d_boff;
    DevBuf<slamem_map> d_reads;
    uint64_t cap_chars = 0;
    uint32_t cap_q = 0;
    // a batch handed in as bit-planes (slamem_stream_submit_packed): 16-byte units {p0, p1}, the letters that are not A,C,G,T per
    // unit (cap_units of each), and the units per record with their prefix sums and the scan's scratch behind them (sized by cap_q)
    DevBuf<uint4> d_planes;
    DevBuf<uint64_t> d_other;
    DevBuf<uint32_t> d_ucnt;
    uint64_t cap_units = 0;
    // a batch handed in with a low-quality mask (slamem_stream_submit_masked): the words the batch touches --
    // d_lowq[0] is the caller's word offs[0] / 64
    DevBuf<uint64_t> d_lowq;
    // a batch handed in with its quality bytes (slamem_stream_submit_quals): the bytes of the batch's letters --
    // d_qual[0] is the caller's byte offs[0]
    DevBuf<unsigned char> d_qual;
    // The batch's OUTPUTS on the device, sized by the inputs' room and allocated by grow_outputs (prepare stage; download stage on
    // a capacity retry): -mem rows (room for `cap`) and the search's workspace; -ext: a uint32 per row; -aln: segments (room for
    // `cap`: a segment has at least one chain row), operations (room for `ops_cap`) and the operations' offsets per segment.
    // INPUTS REGROWN => OUTPUTS DROPPED (drop_outputs): the prepare stage sizes them again from the new room.
    DevBuf<slamem_mem> d_mems;
    DevBuf<char> d_ws;
    DevBuf<uint32_t> d_mm;
    DevBuf<slamem_aln> d_segs;
    DevBuf<uint32_t> d_ops;
    DevBuf<uint64_t> d_ooff;
    uint64_t cap = 0, ops_cap = 0;
    // -sam (slamem_stream_set_md), download stage: the MD entries (room for md_cap), their offsets and the letters under `=` per
    // segment, the primary segment per read, and the pass's workspace; nothing of it exists on a stream whose MD pass is off
    DevBuf<uint32_t> d_md, d_seg_eq, d_primary;
    DevBuf<uint64_t> d_md_off;
    DevBuf<char> d_md_ws;
    uint64_t md_cap = 0;
    // -dedup (slamem_stream_set_dedup), download stage: the read records the add kernels read (strand 0 where a read
    // is a duplicate) and a flag byte per read, room for cap_q + 1 each; nothing of it exists on a stream whose filter is off
    DevBuf<slamem_map> d_keep;
    DevBuf<uint8_t> d_dup;
    PinnedBuf<uint8_t> h_dup;
    // what slamem_stream_next and the getters hand out, in pinned host memory, allocated by the download stage as large as the
    // device buffer each is copied from; h_scal: the words K9's stream copies the batch's totals into (prepare stage)
    PinnedBuf<uint64_t> h_boff;
    PinnedBuf<slamem_mem> h_mems;
    PinnedBuf<uint32_t> h_mm;
    PinnedBuf<slamem_aln> h_segs;
    PinnedBuf<uint32_t> h_ops;
    PinnedBuf<uint64_t> h_ooff;
    PinnedBuf<slamem_map> h_reads;
    PinnedBuf<uint32_t> h_md, h_seg_eq, h_primary;
    PinnedBuf<uint64_t> h_md_off;
    PinnedBuf<unsigned long long> h_scal;
    // the batch
    uint64_t seq = 0;
    const char* chars = nullptr;
    const uint64_t* offs = nullptr;
    uint32_t nq = 0, min_len = 0;
    bool all_short = false;  // no record longer than a slice (seen by the upload stage while the copy engines work)
    const void* planes = nullptr;       // packed: letters 64u .. 64u+63 of a record per unit; a record starts a new unit
    const uint64_t* other = nullptr;    // packed: per unit, letters that are not A,C,G,T (nullptr: none)
    uint64_t units_hint = 0;            // packed: the batch's units as the caller counted them (0: count here)
    const uint64_t* lowq = nullptr;     // masked: the caller's words, indexed as its letters
    const uint8_t* quals = nullptr;     // -wq: the caller's quality bytes, indexed as its letters
    // its result
    uint64_t total = 0, ops_total = 0, md_total = 0;
    int rc = SLAMEM_OK;
    char err[512] = "";
    slamem_timings tm;
    // the batch on its way through the search (mem_search.hip) and the events the stages hand it over with
    SearchJob* job = nullptr;
    hipEvent_t ev_prep = nullptr, ev_done = nullptr, ev_k8 = nullptr;

    ~Slot() {  // (the buffers free themselves)
        if (ev_prep) (void)hipEventDestroy(ev_prep);
        if (ev_done) (void)hipEventDestroy(ev_done);
        if (ev_k8) (void)hipEventDestroy(ev_k8);
        if (job) search_job_delete(job);
    }
};

}  // namespace

}  // namespace slamem

using namespace slamem;

struct slamem_stream {
    const slamem_index* idx = nullptr;
    int device = 0;  // idx->device, kept so that slamem_stream_destroy does not read the index
    int nslots = 0, both = 0, match_type = 0;
    uint32_t max_occ = 0;  // -smem: the occurrence cap of every batch (slamem_stream_set_max_occ; 0: none)
    uint32_t max_gap = 0;  // -chain: the maximum gap of every batch (slamem_stream_set_max_gap; 0: the default)
    uint32_t ext_penalty = 0, ext_xdrop = kExtXdropUnset;  // -ext, -aln: penalty and drop of every batch (slamem_stream_set_ext_params)
    uint32_t end_band = 0;                // -aln: the band of the gapped outer ends (slamem_stream_set_end_band; 0: ungapped)
    uint32_t max_edits = kAlnEditsUnset;  // -aln: the most edits in a gap (slamem_stream_set_max_edits; kAlnEditsUnset: the default)
    slamem_pileup* pile = nullptr;          // -pile: the accumulator every batch is added to (slamem_stream_set_pileup)
    uint32_t min_mapq = 0;                  // -pile: the least mapping quality that counts
    bool md = false;                        // -sam: every batch also goes through the MD pass (slamem_stream_set_md)
    bool dedup = false;                     // -dedup: every batch is added with the duplicate filter (slamem_stream_set_dedup)
    bool quals = false;                     // -wq: every batch comes with its quality bytes (slamem_stream_set_quals)
    uint32_t phred_offset = 33;             // -wq: the Phred offset of those bytes
    slamem_stats* stats = nullptr;          // -stats: the table every batch is added to (slamem_stream_set_stats)
    uint32_t stats_min_mapq = 0;            // -stats: the least mapping quality that counts there
    bool stats_quals = false;               // -stats: batches may come through slamem_stream_submit_quals; their bytes feed the table
    uint64_t max_chars = 0;
    uint32_t max_q = 0;
    std::unique_ptr<Slot[]> slot;  // nslots of them; they go in teardown(), in front of the HIP streams
    std::thread th[kThreads];
    hipStream_t st[kThreads] = {};
    hipStream_t st_upx[3] = {nullptr, nullptr, nullptr};  // more copy streams of the upload stage (SLAMEM_STREAM_UPLOAD_SPLIT = 2..4)
    int upload_split = 2;
    int nthreads = kThreads;
    // SLAMEM_STREAM_CARRY=1: K8 without its tail (below).  Off by default: it does not pay -- every result then waits for the
    // NEXT batch's K8, and the carried lanes finish their strands at the head of that launch instead of the tail of this one
    // (headline workload, round 3: 39.5-40.0 ms against 38.5; a stream of 30 M reads 113.8 against 108.6 ms; the "steady rate" of
    // 868 M MEMs/s the first runs showed was an artefact of where the results' time stamps fall; profiles/r03_host_leg.jsonl)
    bool carry = false;
    Slot* pending = nullptr;     // search stage only: the batch whose K8 has passed its unfinished lanes on
    hipStream_t st_place = nullptr;    // K9 of every batch: behind the K8 that finished it, but not in front of the next K8
    hipStream_t st_search2 = nullptr;  // SLAMEM_STREAM_SEARCH_STREAMS=2: odd batches' K8 + K9 on a second stream (their K8 starts in the tail of the even one's)
    int search_streams = 1;
    uint32_t k8_waves = 2560;  // two search streams: waves of a K8 that has another batch behind it (SLAMEM_STREAM_K8_WAVES; the chip holds 4096)
    double mems_per_char = 0;  // the densest batch so far: sizes a slot's first output buffers (written by the download stage)
    std::mutex mu;
    std::condition_variable cv;
    uint64_t submitted = 0, returned = 0;  // batches handed in / handed back
    bool stop = false, trace = false;
    std::chrono::steady_clock::time_point t0;
};

namespace slamem {
namespace {

// Buffers are allocated by the stage that uses them, on a slot's first batch (and again if a batch needs more room):
// setting a stream up costs nothing, the allocations (pinned host memory above all: ~0.1 ms per MB) overlap with the
// other stages' work, and slots that are never used are never allocated.
// -aln and -paf share the segments' buffers, capacities and setters; -paf adds the read records and has offsets per read
// -pile is -paf whose segments stay on the device: the same job, buffers and setters; the download stage adds the batch to the
// accumulator where -paf copies its segments out
inline bool is_aln(const slamem_stream* s) { return s->match_type == 6 || s->match_type == 7 || s->match_type == 8; }
inline bool is_map(const slamem_stream* s) { return s->match_type == 7 || s->match_type == 8; }
inline int job_type(const slamem_stream* s) { return s->match_type == 8 ? 7 : s->match_type; }

// the stream's parameters (its setters have checked them) and the slot's buffers, as the filter takes them
FilterParams slot_params(const slamem_stream* s, const Slot& sl) {
    FilterParams p = {};  // (the setters have refused what the resolver refuses)
    (void)resolve_filter_params("slamem_stream", s->max_occ, s->max_gap, s->ext_penalty, s->ext_xdrop, s->max_edits, &p);
    (void)set_end_band("slamem_stream", s->end_band, &p);  // (both setters keep band and word consistent, so this cannot refuse)
    if (s->match_type == 5) p.column_dev = sl.d_mm.get();
    if (is_aln(s)) {
        p.segs = sl.d_segs.get(); p.segs_capacity = sl.cap;
        p.ops = sl.d_ops.get(); p.ops_capacity = sl.ops_cap;
        p.op_offsets = sl.d_ooff.get();
        p.reads = is_map(s) ? sl.d_reads.get() : nullptr;
    }
    return p;
}

// Every device buffer that is sized by the room of the slot's inputs.  Called where the outputs get another size AND where the
// upload stage regrows the inputs: a slot without d_ws is a slot whose outputs the prepare stage sizes anew.
void drop_outputs(Slot& sl) {
    sl.d_ws.release(); sl.d_mems.release(); sl.d_mm.release();
    sl.d_segs.release(); sl.d_ops.release(); sl.d_ooff.release();
}

// device output + workspace for `need_cap` rows (prepare stage; download stage on a capacity retry).  All of the old goes
// before any of the new is asked for; d_ws comes last, so that a slot that has it has them all.
int grow_outputs(slamem_stream* s, Slot& sl, uint64_t need_cap) {
    drop_outputs(sl);
    sl.cap = need_cap;
    if (is_aln(s)) {
        if (sl.ops_cap < 2 * sl.cap + 1024) sl.ops_cap = 2 * sl.cap + 1024;  // (a first guess; SLAMEM_ERR_CAPACITY tells the need)
        SLAMEM_TRY(sl.d_segs.reserve(sl.cap + 1));
        SLAMEM_TRY(sl.d_ops.reserve(sl.ops_cap + 1));
        SLAMEM_TRY(sl.d_ooff.reserve(sl.cap + 2));
    }
    SLAMEM_TRY(sl.d_mems.reserve(sl.cap, 16));
    if (s->match_type == 5) SLAMEM_TRY(sl.d_mm.reserve(sl.cap + 4));
    return sl.d_ws.reserve(search_workspace_bytes(sl.cap_q, s->both, sl.cap_chars, sl.cap, job_type(s), slot_params(s, sl)));
}

// stage 0: characters and offsets to the device.  The offsets go up as the caller holds them (absolute): the characters land
// at d_q + kFront + (base mod 16) and the kernels get the pointer that record offset `base` maps to -- 16-byte aligned like
// the caller's buffer start, so nothing is rebased on the host (a loop over a million offsets per batch made this stage
// the pipeline's bottleneck).
constexpr uint64_t kFront = 32;  // bytes in front of the characters: the kernels read whole aligned words around a record
inline const char* device_queries(const Slot& sl) {
    const uint64_t base = sl.offs[0];
    return sl.d_q.get() + kFront + (base & 15u) - base;
}
// Beside K8 -- which keeps the memory system at its random-request ceiling -- ONE copy engine moves 42 GB/s instead of the
// link's 57 (measured: 3.56 ms per 158 MB instead of 2.76, which made the upload the pipeline's period); the pieces of a
// batch go up on `upload_split` copy streams side by side.  Returns the streams used in *ways: the first is s->st[0], the
// caller waits for the others (s->st_upx[0 .. ways - 2]).
int copy_split(slamem_stream* s, void* dst, const void* src, uint64_t bytes, int* ways) {
    *ways = (s->upload_split > 1 && bytes >= (8u << 20)) ? s->upload_split : 1;
    uint64_t at = 0;
    for (int wy = 0; wy < *ways; wy++) {
        const uint64_t end = wy + 1 == *ways ? bytes : ((bytes * (uint64_t)(wy + 1) / (uint64_t)*ways) & ~(uint64_t)4095);
        hipStream_t cs = wy == 0 ? s->st[0] : s->st_upx[wy - 1];
        if (end > at)
            SLAMEM_HIP(hipMemcpyAsync(static_cast<char*>(dst) + at, static_cast<const char*>(src) + at, end - at, hipMemcpyHostToDevice, cs));
        at = end;
    }
    return SLAMEM_OK;
}
// while the copy engines work: is any record longer than a slice?  (if not, the prepare stage knows the number of work items
// without asking the device -- its one host round trip per batch goes away)
bool all_records_short(const Slot& sl) {
    uint64_t longest = 0;
    for (uint32_t i = 0; i < sl.nq; i++) {
        const uint64_t len = sl.offs[i + 1] - sl.offs[i];
        longest = len > longest ? len : longest;
    }
    return longest <= kSearchSliceLen;
}
// ---- reads that come as bit-planes (slamem_stream_submit_packed) -------------------------------------------------------------
// The link is what bounds the host-to-host path since the search takes 9 ms for 10 M reads (1.5 GB of letters: 26 ms at 57
// GB/s); a caller that holds its reads packed -- two bits a letter in the layout of the index's text planes, 48 bytes per 150
// letters -- sends a third of that.  On the device the letters are written out again (k_unpack_reads: 0.5 ms per 1.5 GB) and the
// batch goes the way of every other; letters that are not A,C,G,T travel as a third plane (or not at all: other = nullptr).
__global__ void __launch_bounds__(256) k_unit_counts(const uint64_t* __restrict__ offsets, uint32_t nq, uint32_t* __restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nq) return;
    cnt[i] = i < nq ? (uint32_t)((offsets[i + 1] - offsets[i] + 63u) >> 6) : 0u;  // cnt[nq] = 0: the scan leaves the total there
}
constexpr uint32_t kUnpackRecords = 128, kUnpackBytes = 32768;
// a block writes the letters of kUnpackRecords consecutive records: decoded into LDS (16 letters per lane and step), then out in
// aligned 16-byte pieces; records too long for the buffer are written letter by letter
__global__ void __launch_bounds__(256) k_unpack_reads(const uint4* __restrict__ planes, const uint64_t* __restrict__ other,
                                                      const uint32_t* __restrict__ uoff, const uint64_t* __restrict__ offsets, uint32_t nq,
                                                      char* __restrict__ out /* where record offset offsets[0] goes */) {
    __shared__ __attribute__((aligned(16))) char buf[kUnpackBytes + 16];
    const uint32_t r0 = blockIdx.x * kUnpackRecords, r1 = r0 + kUnpackRecords < nq ? r0 + kUnpackRecords : nq;
    if (r0 >= nq) return;
    const uint64_t base = offsets[0], lo = offsets[r0], hi = offsets[r1];
    char* dst = out + (lo - base);
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);  // buf[shift + x] is byte x of the range
    const bool staged = hi - lo <= kUnpackBytes;
    auto letter = [&](uint64_t p0, uint64_t p1, uint64_t ot, uint32_t bit) -> char {
        const uint32_t c = (uint32_t)((p0 >> bit) & 1ull) | ((uint32_t)((p1 >> bit) & 1ull) << 1);
        return ((ot >> bit) & 1ull) ? 'N' : "ACGT"[c];
    };
    // 2 lanes per record; a lane takes 16 letters at a time, 32 apart
    for (uint32_t r = r0 + (threadIdx.x >> 1); r < r1; r += 128u) {
        const uint64_t ro = offsets[r];
        const uint32_t len = (uint32_t)(offsets[r + 1] - ro);
        const uint32_t u0 = uoff[r];
        for (uint32_t x = (threadIdx.x & 1u) * 16u; x < len; x += 32u) {
            const uint4 pu = planes[u0 + (x >> 6)];
            const uint64_t p0 = ((uint64_t)pu.y << 32) | pu.x, p1 = ((uint64_t)pu.w << 32) | pu.z;
            const uint64_t ot = other ? other[u0 + (x >> 6)] : 0ull;
            const uint32_t n = len - x < 16u ? len - x : 16u;
            char* w = staged ? buf + shift + (uint32_t)(ro - lo) + x : dst + (ro - lo) + x;
            for (uint32_t i = 0; i < n; i++) w[i] = letter(p0, p1, ot, (x & 63u) + i);
        }
    }
    if (!staged) return;
    __syncthreads();
    const uint32_t nbytes = (uint32_t)(hi - lo);
    // bytes [0, nbytes) of the range sit at buf[shift ..]; global address dst - shift is 16-byte aligned
    const uint32_t first_full = shift ? 16u - shift : 0u;  // range bytes in front of the first aligned piece
    for (uint32_t i = threadIdx.x; i < first_full && i < nbytes; i += 256u) dst[i] = buf[shift + i];
    if (nbytes > first_full) {
        const uint32_t pieces = (nbytes - first_full) >> 4;
        uint4* g = reinterpret_cast<uint4*>(dst + first_full);
        const uint4* l = reinterpret_cast<const uint4*>(buf + shift + first_full);
        for (uint32_t i = threadIdx.x; i < pieces; i += 256u) g[i] = l[i];
        for (uint32_t i = first_full + (pieces << 4) + threadIdx.x; i < nbytes; i += 256u) dst[i] = buf[shift + i];
    }
}

int stage_upload_packed(slamem_stream* s, Slot& sl, char* dst) {
    // the units of the batch: as the caller says, or counted here (a pass over the offsets: ~1 ms per million records, in front
    // of the copies -- a caller that knows the number from slamem_pack_reads saves it)
    uint64_t units = sl.units_hint;
    if (units == 0)
        for (uint32_t i = 0; i < sl.nq; i++) units += (sl.offs[i + 1] - sl.offs[i] + 63u) >> 6;
    if (units >= 0xFFFFFFFFull) { set_error("slamem_stream_submit_packed: fewer than 2^32 units (64 letters) per batch"); return SLAMEM_ERR_ARG; }
    if (!sl.d_planes.get() || units > sl.cap_units) {
        sl.d_planes.release(); sl.d_other.release();
        sl.cap_units = 0;  // until both are there
        const uint64_t want = units > (s->max_chars >> 6) + s->max_q ? units : (s->max_chars >> 6) + s->max_q;
        SLAMEM_TRY(sl.d_planes.reserve(want + 1));
        SLAMEM_TRY(sl.d_other.reserve(want + 1));
        sl.cap_units = want;
    }
    SLAMEM_TRY(sl.d_ucnt.reserve((uint64_t)sl.cap_q + 2 + scan_u32_tmp_words((uint64_t)sl.cap_q + 1)));  // (goes with the inputs' room)
    hipStream_t st = s->st[0];
    SLAMEM_HIP(hipMemcpyAsync(sl.d_off.get(), sl.offs, ((uint64_t)sl.nq + 1) * 8, hipMemcpyHostToDevice, st));
    int ways = 1;  // the planes on the copy streams side by side (as the letters of an ordinary batch)
    SLAMEM_TRY(copy_split(s, sl.d_planes.get(), sl.planes, units * 16, &ways));
    if (sl.other && units) SLAMEM_HIP(hipMemcpyAsync(sl.d_other.get(), sl.other, units * 8, hipMemcpyHostToDevice, st));
    if (sl.nq) {
        hipLaunchKernelGGL(k_unit_counts, dim3((unsigned)(((uint64_t)sl.nq + 1 + 255) / 256)), dim3(256), 0, st, (const uint64_t*)sl.d_off.get(), sl.nq,
                           sl.d_ucnt.get());
        SLAMEM_HIP(exclusive_scan_u32(sl.d_ucnt.get(), sl.d_ucnt.get(), (uint64_t)sl.nq + 1, sl.d_ucnt.get() + sl.cap_q + 2, st));
    }
    sl.all_short = all_records_short(sl);
    for (int wy = 1; wy < ways; wy++) SLAMEM_HIP(hipStreamSynchronize(s->st_upx[wy - 1]));  // (the letters are written on st: every piece must be there)
    if (sl.nq) {
        hipLaunchKernelGGL(k_unpack_reads, dim3((sl.nq + kUnpackRecords - 1) / kUnpackRecords), dim3(256), 0, st, (const uint4*)sl.d_planes.get(),
                           sl.other ? (const uint64_t*)sl.d_other.get() : (const uint64_t*)nullptr, (const uint32_t*)sl.d_ucnt.get(),
                           (const uint64_t*)sl.d_off.get(), sl.nq, dst);
        SLAMEM_HIP(hipGetLastError());
    }
    SLAMEM_HIP(hipStreamSynchronize(st));
    return SLAMEM_OK;
}

int stage_upload(slamem_stream* s, Slot& sl) {
    const uint64_t base = sl.offs[0], qbytes = sl.offs[sl.nq] - base;
    if (!sl.d_q.get() || qbytes > sl.cap_chars || sl.nq > sl.cap_q) {
        // first batch of this slot, or a batch larger than the reservation (max_batch_* of slamem_stream_create are a hint).
        // INPUTS REGROWN => OUTPUTS DROPPED: what is sized by the inputs' room goes with them, all of it before anything new is
        // asked for, and the prepare stage (which finds no d_ws) sizes the outputs again
        const uint64_t nchars = qbytes > s->max_chars ? qbytes : s->max_chars;
        const uint32_t nrec = sl.nq > s->max_q ? sl.nq : s->max_q;
        const uint64_t nb = (uint64_t)nrec * (s->both ? 2 : 1);
        drop_outputs(sl);
        sl.d_q.release(); sl.d_off.release(); sl.d_boff.release(); sl.d_reads.release(); sl.d_ucnt.release();
        sl.cap_chars = 0; sl.cap_q = 0;  // until all are there: a failed allocation must not leave stale room behind
        SLAMEM_TRY(sl.d_q.reserve(nchars + 2 * kFront + 32));
        SLAMEM_TRY(sl.d_off.reserve((uint64_t)nrec + 1));
        SLAMEM_TRY(sl.d_boff.reserve(nb + 1));
        if (is_map(s)) SLAMEM_TRY(sl.d_reads.reserve((uint64_t)nrec + 1));
        sl.cap_chars = nchars;
        sl.cap_q = nrec;
    }
    char* dst = sl.d_q.get() + kFront + (base & 15u);
    if (sl.planes) return stage_upload_packed(s, sl, dst);
    int ways = 1;
    SLAMEM_TRY(copy_split(s, dst, sl.chars + base, qbytes, &ways));
    SLAMEM_HIP(hipMemcpyAsync(sl.d_off.get(), sl.offs, ((uint64_t)sl.nq + 1) * 8, hipMemcpyHostToDevice, s->st[0]));
    if (sl.lowq && qbytes) {
        // the mask's words that hold a bit of the batch: [base / 64, (base + qbytes + 63) / 64).  Nothing is shifted: the add gets
        // d_lowq - base / 64, so that bit offs[r] + i is letter i of read r there as it is in the caller's array
        const uint64_t w0 = base >> 6, nw = ((base + qbytes + 63u) >> 6) - w0;
        if (sl.d_lowq.count() < nw) SLAMEM_TRY(sl.d_lowq.reserve(nw > (sl.cap_chars >> 6) + 2 ? nw : (sl.cap_chars >> 6) + 2));
        SLAMEM_HIP(hipMemcpyAsync(sl.d_lowq.get(), sl.lowq + w0, nw * 8, hipMemcpyHostToDevice, s->st[0]));
    }
    if (sl.quals) {
        // the quality bytes of the batch's letters: [base, base + qbytes).  The add gets d_qual - base, so that byte offs[r] + i is
        // letter i of read r there as it is in the caller's array
        if (!sl.d_qual.get() || sl.d_qual.count() < qbytes) SLAMEM_TRY(sl.d_qual.reserve((qbytes > sl.cap_chars ? qbytes : sl.cap_chars) + 8));
        if (qbytes) SLAMEM_HIP(hipMemcpyAsync(sl.d_qual.get(), sl.quals + base, qbytes, hipMemcpyHostToDevice, s->st[0]));
    }
    sl.all_short = all_records_short(sl);
    SLAMEM_HIP(hipStreamSynchronize(s->st[0]));
    for (int wy = 1; wy < ways; wy++) SLAMEM_HIP(hipStreamSynchronize(s->st_upx[wy - 1]));
    return SLAMEM_OK;
}

// stage 1: work-item tables (one small host round trip on this stage's stream), then K8a, the work list and K7q, asynchronous
int job_setup(slamem_stream* s, Slot& sl) {
    const uint64_t qbytes = sl.offs[sl.nq] - sl.offs[0];
    if (!sl.d_ws.get()) {
        // first guess of the room for MEMs: what the densest batch so far would need, and never less than a MEM per 32
        // characters; grown when a batch needs more (SLAMEM_ERR_CAPACITY tells how much)
        const uint64_t nb = (uint64_t)sl.cap_q * (s->both ? 2 : 1);
        uint64_t guess = sl.cap_chars / 32 + nb + 1024;
        const uint64_t seen = (uint64_t)(1.25 * s->mems_per_char * (double)sl.cap_chars) + 1024;
        SLAMEM_TRY(grow_outputs(s, sl, seen > guess ? seen : guess));
    }
    if (!sl.job && !(sl.job = search_job_new())) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    if (!sl.ev_prep) SLAMEM_HIP(hipEventCreateWithFlags(&sl.ev_prep, hipEventDisableTiming));
    if (!sl.ev_done) SLAMEM_HIP(hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming));
    if (!sl.ev_k8) SLAMEM_HIP(hipEventCreateWithFlags(&sl.ev_k8, hipEventDisableTiming));
    SLAMEM_TRY(sl.h_scal.reserve(16));
    const FilterParams p = slot_params(s, sl);
    return search_job_init(sl.job, s->idx, device_queries(sl), sl.d_off.get(), sl.nq, qbytes, sl.min_len, s->both, job_type(s), sl.d_mems.get(),
                           sl.cap, sl.d_boff.get(), sl.d_ws.get(), sl.d_ws.count(), sl.h_scal.get(), &p);
}
int stage_prepare(slamem_stream* s, Slot& sl) {
    int rc = job_setup(s, sl);
    if (rc == SLAMEM_OK && sl.all_short) search_job_slices_hint(sl.job, sl.nq);
    if (rc == SLAMEM_OK) rc = search_job_tables(sl.job, s->st[T_PREP]);
    if (rc == SLAMEM_OK) rc = search_job_prep(sl.job, s->st[T_PREP]);
    if (rc == SLAMEM_OK) SLAMEM_HIP(hipEventRecord(sl.ev_prep, s->st[T_PREP]));
    return rc;
}

// stage 2: K8 + K9 behind the preparation, enqueued only: the search stream holds the K8s and K9s of all batches in flight,
// one behind the other.  K8 WITHOUT ITS TAIL: when another batch has been submitted behind this one, K8 ends as soon as its
// work list is empty and passes the unfinished lanes on (search_job_k8 carry_out); the next batch's K8 takes them in first,
// and only then this batch's K9 follows -- the chip never drains between two batches of a stream.  The last batch (nothing
// submitted behind it) runs to its end as before.  `failed`: the batch comes from an earlier stage with an error and only
// the batch waiting for it has to be finished.
void finish_pending(slamem_stream* s, hipStream_t st) {  // K9 of the batch whose lanes are all through now; hand it to the download stage
    Slot* p = s->pending;
    s->pending = nullptr;
    hipStream_t ps = s->st_place ? s->st_place : st;
    if (ps != st) { (void)hipEventRecord(p->ev_k8, st); (void)hipStreamWaitEvent(ps, p->ev_k8, 0); }
    int rc = search_job_place(p->job, ps);
    (void)hipEventRecord(p->ev_done, ps);
    if (rc != SLAMEM_OK) snprintf(p->err, sizeof(p->err), "%s", slamem_last_error_message());
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (rc != SLAMEM_OK) p->rc = rc;
        p->state = LAUNCHED;
    }
    s->cv.notify_all();
}
int stage_search(slamem_stream* s, Slot& sl, bool failed, bool* issued_only) {
    hipStream_t st = (s->search_streams > 1 && (sl.seq & 1u)) ? s->st_search2 : s->st[T_SEARCH];
    *issued_only = false;
    if (failed) {
        if (s->pending) {
            (void)search_job_flush(s->pending->job, st);
            finish_pending(s, st);
        }
        return SLAMEM_OK;
    }
    bool more, follows;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        follows = s->submitted > sl.seq + 1;
        more = s->carry && s->search_streams == 1 && follows;
    }
    // two search streams: a batch that has another one behind it takes only part of the chip for its K8, so that the next
    // batch's preparation and then its K8 start beside it instead of in its tail; the last batch of a stream takes all of it
    search_job_k8_wave_cap(sl.job, (s->search_streams > 1 && follows) ? s->k8_waves : 0u);
    SLAMEM_HIP(hipStreamWaitEvent(st, sl.ev_prep, 0));
    int rc;
    if (s->pending && search_job_can_carry_into(s->pending->job, sl.job)) {
        rc = search_job_k8(sl.job, st, s->pending->job, more);
        if (rc != SLAMEM_OK) (void)search_job_flush(s->pending->job, st);
        finish_pending(s, st);
    } else {
        if (s->pending) {
            (void)search_job_flush(s->pending->job, st);
            finish_pending(s, st);
        }
        rc = search_job_k8(sl.job, st, nullptr, more);
    }
    if (rc == SLAMEM_OK && search_job_carried_out(sl.job)) {
        s->pending = &sl;
        *issued_only = true;  // its K9 and its event follow behind the next batch's K8
        return SLAMEM_OK;
    }
    hipStream_t ps = s->st_place ? s->st_place : st;
    if (ps != st) { SLAMEM_HIP(hipEventRecord(sl.ev_k8, st)); SLAMEM_HIP(hipStreamWaitEvent(ps, sl.ev_k8, 0)); }
    if (rc == SLAMEM_OK) rc = search_job_place(sl.job, ps);
    // (recorded even after a failed launch: the download stage waits for whatever did get onto the stream)
    SLAMEM_HIP(hipEventRecord(sl.ev_done, ps));
    return rc;
}

// -sam: the MD pass over the batch's segments as they lie on the device (sam_filter.hip), and its four arrays to pinned host
// memory.  The entries' room starts at operations + segments (an entry per X or D letter: a first guess) and grows to what
// SLAMEM_ERR_CAPACITY tells.
int stage_md(slamem_stream* s, Slot& sl, hipStream_t st) {
    const uint64_t ns = sl.total;
    {   // a word per segment: as many as the slot has room for segments (ns <= cap), and one more
        const uint64_t segs = (sl.cap > ns ? sl.cap : ns) + 2;
        uint64_t ws_bytes = 0;
        SLAMEM_TRY(slamem_maps_md_workspace_bytes(segs - 1, sl.cap_q, &ws_bytes));
        SLAMEM_TRY(sl.d_md_off.reserve(segs));
        SLAMEM_TRY(sl.d_seg_eq.reserve(segs));
        SLAMEM_TRY(sl.d_md_ws.reserve(ws_bytes));
        SLAMEM_TRY(sl.h_md_off.reserve(segs));
        SLAMEM_TRY(sl.h_seg_eq.reserve(segs));
    }
    SLAMEM_TRY(sl.d_primary.reserve((uint64_t)sl.cap_q + 1));  // (nq <= cap_q)
    SLAMEM_TRY(sl.h_primary.reserve((uint64_t)sl.cap_q + 1));
    uint64_t want = sl.ops_total + ns + 1024;
    int rc = SLAMEM_OK;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (sl.md_cap < want) sl.md_cap = want;
        SLAMEM_TRY(sl.d_md.reserve(sl.md_cap + 1));
        rc = slamem_maps_md_device(s->idx, sl.d_segs.get(), ns, sl.d_boff.get(), sl.nq, sl.d_ops.get(), sl.d_ooff.get(), sl.d_md.get(), sl.md_cap,
                                   sl.d_md_off.get(), sl.d_seg_eq.get(), sl.d_primary.get(), sl.d_md_ws.get(), sl.d_md_ws.count(), st, &sl.md_total);
        if (rc != SLAMEM_ERR_CAPACITY) break;
        want = sl.md_total + sl.md_total / 8 + 1024;
    }
    if (rc != SLAMEM_OK) return rc;
    SLAMEM_TRY(sl.h_md.reserve(sl.md_cap + 1));
    if (sl.md_total) SLAMEM_HIP(hipMemcpyAsync(sl.h_md.get(), sl.d_md.get(), sl.md_total * 4, hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipMemcpyAsync(sl.h_md_off.get(), sl.d_md_off.get(), (ns + 1) * 8, hipMemcpyDeviceToHost, st));
    if (ns) SLAMEM_HIP(hipMemcpyAsync(sl.h_seg_eq.get(), sl.d_seg_eq.get(), ns * 4, hipMemcpyDeviceToHost, st));
    if (sl.nq) SLAMEM_HIP(hipMemcpyAsync(sl.h_primary.get(), sl.d_primary.get(), (uint64_t)sl.nq * 4, hipMemcpyDeviceToHost, st));
    return SLAMEM_OK;
}

// stage 3: the batch's totals, then MEMs and block offsets to pinned host memory
int stage_download(slamem_stream* s, Slot& sl) {
    hipStream_t st = s->st[T_DOWN];
    (void)slamem_reset_timings();
    SLAMEM_HIP(hipEventSynchronize(sl.ev_done));
    int rc = search_job_collect(sl.job, &sl.total);
    uint64_t at[3] = {0, 0, 0};  // -aln: -mem rows, segments, operations
    if (is_aln(s)) search_job_aln_totals(sl.job, at);
    for (int attempt = 0; rc == SLAMEM_ERR_CAPACITY && (sl.total > sl.cap || at[2] > sl.ops_cap) &&
                          attempt < (is_aln(s) ? 3 : 2); attempt++) {  // (-aln: the rows may not fit, then the operations)
        // rare (the first guess was too small): more room, and the batch once more, start to end, on this stage's stream
        if (is_aln(s)) {
            if (at[2] > sl.ops_cap) sl.ops_cap = at[2] + at[2] / 8 + 1024;
            rc = grow_outputs(s, sl, at[0] > sl.cap ? at[0] + at[0] / 8 + 1024 : sl.cap);
        } else
        rc = grow_outputs(s, sl, sl.total + sl.total / 8 + 1024);
        if (rc == SLAMEM_OK) rc = job_setup(s, sl);
        if (rc == SLAMEM_OK) rc = search_job_tables(sl.job, st);
        if (rc == SLAMEM_OK) rc = search_job_prep(sl.job, st);
        if (rc == SLAMEM_OK) rc = search_job_search(sl.job, st);
        SLAMEM_HIP(hipStreamSynchronize(st));
        if (rc == SLAMEM_OK) rc = search_job_collect(sl.job, &sl.total);
        if (is_aln(s)) search_job_aln_totals(sl.job, at);
    }
    sl.ops_total = at[2];
    if (rc == SLAMEM_OK) rc = search_job_finish(sl.job, st, &sl.total);  // -mum: a batch with a large block
    (void)slamem_get_timings(&sl.tm);
    if (rc != SLAMEM_OK) return rc;
    {
        const uint64_t chars = sl.offs[sl.nq] - sl.offs[0];
        const double d = chars ? (double)sl.total / (double)chars : 0.0;
        std::lock_guard<std::mutex> lk(s->mu);
        if (d > s->mems_per_char) s->mems_per_char = d;
    }
    // Pinned host memory for what goes back, each array as large as the device buffer it is copied from (so it follows that
    // buffer's growth, and a batch no larger than the ones before allocates nothing)
    const uint64_t strands = s->both ? 2 : 1, nb = (uint64_t)sl.nq * strands;
    SLAMEM_TRY(sl.h_boff.reserve((uint64_t)sl.cap_q * strands + 1));
    if (s->match_type == 8) {
        // -pile: the batch's result stands (its totals fitted), so it is added to the accumulator -- here and not behind K9,
        // where nobody knows yet whether the batch will be run again with more room.  Segments and operations stay on the device.
        // (a masked batch: the uploaded words start at the caller's word offs[0] / 64)
        const uint64_t* lowq = (sl.lowq && sl.d_lowq.get() && sl.offs[sl.nq] > sl.offs[0]) ? sl.d_lowq.get() - (sl.offs[0] >> 6) : nullptr;
        if (s->dedup) {  // (this stage takes the batches in submission order, and so the filter numbers them)
            SLAMEM_TRY(sl.d_keep.reserve((uint64_t)sl.cap_q + 1));
            SLAMEM_TRY(sl.d_dup.reserve((uint64_t)sl.cap_q + 1));
            SLAMEM_TRY(sl.h_dup.reserve((uint64_t)sl.cap_q + 1));
        }
        if (s->quals) {  // (the quality pass behind the pile kernels of the same batch)
            rc = pileup_add_quals(s->pile, device_queries(sl), sl.d_off.get(), sl.nq, sl.d_segs.get(), sl.d_boff.get(), sl.d_ops.get(),
                                  sl.d_ooff.get(), sl.d_reads.get(), s->min_mapq, lowq, sl.d_qual.get() - sl.offs[0], s->phred_offset,
                                  s->dedup, sl.d_keep.get(), sl.d_dup.get(), st);
            if (rc == SLAMEM_OK && s->dedup && sl.nq) SLAMEM_HIP(hipMemcpyAsync(sl.h_dup.get(), sl.d_dup.get(), sl.nq, hipMemcpyDeviceToHost, st));
        } else if (s->dedup) {
            rc = pileup_add_dedup(s->pile, device_queries(sl), sl.d_off.get(), sl.nq, sl.d_segs.get(), sl.d_boff.get(), sl.d_ops.get(),
                                  sl.d_ooff.get(), sl.d_reads.get(), s->min_mapq, lowq, sl.d_keep.get(), sl.d_dup.get(), st);
            if (rc == SLAMEM_OK && sl.nq) SLAMEM_HIP(hipMemcpyAsync(sl.h_dup.get(), sl.d_dup.get(), sl.nq, hipMemcpyDeviceToHost, st));
        } else {
            rc = pileup_add_masked(s->pile, device_queries(sl), sl.d_off.get(), sl.nq, sl.d_segs.get(), sl.d_boff.get(), sl.d_ops.get(),
                                   sl.d_ooff.get(), sl.d_reads.get(), s->min_mapq, lowq, st);
        }
        if (rc != SLAMEM_OK) return rc;
    } else {
        SLAMEM_TRY(sl.h_mems.reserve(sl.cap, 16));
    }
    if (s->stats) {  // (the batch's result stands; its counts go to the table, from the records as the search wrote them)
        const unsigned char* qb = (s->stats_quals && sl.quals && sl.d_qual.get()) ? sl.d_qual.get() - sl.offs[0] : nullptr;
        SLAMEM_TRY(stats_add(s->stats, device_queries(sl), sl.d_off.get(), sl.nq, sl.d_segs.get(), sl.d_boff.get(), sl.d_ops.get(),
                             sl.d_ooff.get(), sl.d_reads.get(), qb, s->phred_offset, s->stats_min_mapq, st));
    }
    if (sl.total && !is_aln(s))
        SLAMEM_HIP(hipMemcpyAsync(sl.h_mems.get(), sl.d_mems.get(), sl.total * sizeof(slamem_mem), hipMemcpyDeviceToHost, st));
    if (is_aln(s) && s->match_type != 8) {  // (sl.total: the segments)
        SLAMEM_TRY(sl.h_segs.reserve(sl.cap + 1));
        SLAMEM_TRY(sl.h_ooff.reserve(sl.cap + 2));
        SLAMEM_TRY(sl.h_ops.reserve(sl.ops_cap + 1));
        if (sl.total) SLAMEM_HIP(hipMemcpyAsync(sl.h_segs.get(), sl.d_segs.get(), sl.total * sizeof(slamem_aln), hipMemcpyDeviceToHost, st));
        if (sl.ops_total) SLAMEM_HIP(hipMemcpyAsync(sl.h_ops.get(), sl.d_ops.get(), sl.ops_total * 4, hipMemcpyDeviceToHost, st));
        SLAMEM_HIP(hipMemcpyAsync(sl.h_ooff.get(), sl.d_ooff.get(), (sl.total + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    if (s->md) SLAMEM_TRY(stage_md(s, sl, st));
    if (s->match_type == 5) {
        SLAMEM_TRY(sl.h_mm.reserve(sl.cap + 4));
        if (sl.total) SLAMEM_HIP(hipMemcpyAsync(sl.h_mm.get(), sl.d_mm.get(), sl.total * 4, hipMemcpyDeviceToHost, st));
    }
    if (is_map(s)) {  // (the offsets are per read)
        SLAMEM_TRY(sl.h_reads.reserve((uint64_t)sl.cap_q + 1));
        if (sl.nq) SLAMEM_HIP(hipMemcpyAsync(sl.h_reads.get(), sl.d_reads.get(), (uint64_t)sl.nq * sizeof(slamem_map), hipMemcpyDeviceToHost, st));
        SLAMEM_HIP(hipMemcpyAsync(sl.h_boff.get(), sl.d_boff.get(), ((uint64_t)sl.nq + 1) * 8, hipMemcpyDeviceToHost, st));
    } else
    SLAMEM_HIP(hipMemcpyAsync(sl.h_boff.get(), sl.d_boff.get(), (nb + 1) * 8, hipMemcpyDeviceToHost, st));
    SLAMEM_HIP(hipStreamSynchronize(st));
    return SLAMEM_OK;
}

// one thread per stage; each takes its batches in submission order
void worker(slamem_stream* s, int t) {
    static const int kWant[kThreads] = {QUEUED, UPLOADED, PREPARED, LAUNCHED};
    static const int kDone[kThreads] = {UPLOADED, PREPARED, LAUNCHED, DONE};
    static const char* const kName[kThreads] = {"upload", "prepare", "search", "download"};
    const int want = kWant[t], done = kDone[t];
    (void)hipSetDevice(s->device);
    for (uint64_t seq = 0;; seq++) {
        Slot& sl = s->slot[seq % (uint64_t)s->nslots];
        {
            std::unique_lock<std::mutex> lk(s->mu);
            s->cv.wait(lk, [&] { return s->stop || (sl.state == want && sl.seq == seq && seq < s->submitted); });
            if (s->stop) return;
        }
        int rc = sl.rc;  // a batch that failed in an earlier stage passes through untouched
        bool issued_only = false;
        const auto t_begin = std::chrono::steady_clock::now();
        if (rc == SLAMEM_OK) {
            rc = t == T_UP ? stage_upload(s, sl) : t == T_PREP ? stage_prepare(s, sl) : t == T_SEARCH ? stage_search(s, sl, false, &issued_only)
                                                                                                    : stage_download(s, sl);
            if (rc != SLAMEM_OK) snprintf(sl.err, sizeof(sl.err), "%s", slamem_last_error_message());  // the text is per thread
        } else if (t == T_SEARCH) {
            (void)stage_search(s, sl, true, &issued_only);
        } else if (t == T_DOWN && sl.ev_done) {
            (void)hipEventSynchronize(sl.ev_done);  // nothing of a failed batch may still run when its slot is handed back
        }
        if (s->trace) {  // SLAMEM_STREAM_TRACE=1: when every stage worked on every batch (ms since the stream was created)
            const auto t_end = std::chrono::steady_clock::now();
            fprintf(stderr, "[stream] batch %3llu %-8s %9.3f .. %9.3f ms\n", (unsigned long long)seq, kName[t],
                    std::chrono::duration<double, std::milli>(t_begin - s->t0).count(),
                    std::chrono::duration<double, std::milli>(t_end - s->t0).count());
        }
        {
            std::lock_guard<std::mutex> lk(s->mu);
            sl.rc = rc;
            sl.state = issued_only ? (int)K8_ISSUED : done;
        }
        s->cv.notify_all();
    }
}

// Steps 4 to 6 of a stream's end, for slamem_stream_destroy and for a slamem_stream_create that failed half way: the device is
// set, no thread runs.  Every copy and kernel of the stream's own HIP streams is through before buffers and streams go (the
// stages wait for their work batch by batch; this is for whatever a failed batch left behind, and for tools that watch the
// copies: a profiler waited 30 s at exit for completion callbacks of copies whose streams were destroyed under it,
// profiles/README.md); then the slots with their buffers, events and jobs; then the streams.
void teardown(slamem_stream* s) {
    hipStream_t all[kThreads + 3 + 2];
    int n = 0;
    for (int k = 0; k < kThreads; k++) all[n++] = s->st[k];
    for (int k = 0; k < 3; k++) all[n++] = s->st_upx[k];
    all[n++] = s->st_search2;
    all[n++] = s->st_place;
    for (int k = 0; k < n; k++)
        if (all[k]) (void)hipStreamSynchronize(all[k]);
    s->slot.reset();
    for (int k = 0; k < n; k++)
        if (all[k]) (void)hipStreamDestroy(all[k]);
}

// what every setter ends its checks with (s->mu held): the parameters of a stream are those of all its batches
bool has_batches(const slamem_stream* s, const char* who, const char* advice) {
    if (s->submitted == 0) return false;
    set_error("%s: the stream has batches already (%s before the first submit)", who, advice);
    return true;
}

// the slot of the batch slamem_stream_next returned last, for a getter (s->mu held); nullptr, with the message, if there is none
// or it failed: it would have had `things` to show
Slot* last_returned(slamem_stream* s, const char* who, const char* things) {
    if (s->returned == 0) { set_error("%s: no batch has been returned yet", who); return nullptr; }
    Slot& sl = s->slot[(s->returned - 1) % (uint64_t)s->nslots];
    if (sl.state != RETURNED || sl.rc != SLAMEM_OK) {
        set_error("%s: the batch slamem_stream_next returned last has no %s to show", who, things);
        return nullptr;
    }
    return &sl;
}

// a batch as one of slamem_stream_submit* takes it (which has checked its own arguments): letters or planes, never both
struct Batch {
    const char* chars = nullptr;
    const void* planes = nullptr;
    const uint64_t* other = nullptr;
    uint64_t units = 0;
    const uint64_t* lowq = nullptr;  // (nullptr: the batch is an unmasked one)
    const uint8_t* quals = nullptr;  // (nullptr: the batch has no quality bytes)
    const uint64_t* offs = nullptr;
    uint32_t nq = 0, min_len = 0;
};

int enqueue(slamem_stream* s, const char* who, const Batch& b) {
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->match_type == 8 && !s->pile) {
        set_error("%s: a stream of match type 8 (-pile) needs slamem_stream_set_pileup first", who);
        return SLAMEM_ERR_ARG;
    }
    if (s->pile && pileup_has_quals(s->pile) && !(s->quals && b.quals)) {
        set_error("%s: the stream's accumulator keeps quality sums (slamem_pileup_enable_quals), which a batch without quality bytes would "
                  "leave behind its counts: slamem_stream_set_quals, then slamem_stream_submit_quals", who);
        return SLAMEM_ERR_ARG;
    }
    Slot& sl = s->slot[s->submitted % (uint64_t)s->nslots];
    if (sl.state != FREE) {
        // a slot is released by the slamem_stream_next call AFTER the one that handed its result out: at most slots - 1
        // batches may be in flight beside the result the caller is working on.  Never blocks (a caller that both submits
        // and collects on one thread would wait for itself).
        set_error("%s: all %d slots are in use (collect a result with slamem_stream_next first)", who, s->nslots);
        return SLAMEM_ERR_ARG;
    }
    sl.seq = s->submitted;
    sl.chars = b.chars;
    sl.planes = b.planes;
    sl.other = b.other;
    sl.units_hint = b.units;
    sl.lowq = b.lowq;
    sl.quals = b.quals;
    sl.offs = b.offs;
    sl.nq = b.nq;
    sl.min_len = b.min_len;
    sl.rc = SLAMEM_OK;
    sl.err[0] = 0;
    sl.total = 0;
    sl.state = QUEUED;
    s->submitted++;
    lk.unlock();
    s->cv.notify_all();
    return SLAMEM_OK;
}

}  // namespace
}  // namespace slamem

extern "C" {

int slamem_pinned_alloc(void** out, uint64_t bytes) {
    if (!out) return SLAMEM_ERR_ARG;
    *out = nullptr;
    SLAMEM_HIP(hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault));
    return SLAMEM_OK;
}

// letters -> bit-planes on the host (what a caller without packed reads of its own puts in front of slamem_stream_submit_packed)
int slamem_pack_reads(const char* queries, const uint64_t* offsets, uint32_t num_queries, void* planes_out, uint64_t* other_out,
                      uint64_t* units_out, int threads) {
    if (!offsets || (num_queries && (!queries || !planes_out))) { set_error("slamem_pack_reads: null argument"); return SLAMEM_ERR_ARG; }
    // the first unit of every record: a prefix sum (one pass), then the records in ranges, a thread each
    std::vector<uint64_t> first((size_t)num_queries + 1);
    uint64_t units = 0;
    for (uint32_t i = 0; i < num_queries; i++) { first[i] = units; units += (offsets[i + 1] - offsets[i] + 63u) >> 6; }
    first[num_queries] = units;
    if (units_out) *units_out = units;
    uint64_t* pl = static_cast<uint64_t*>(planes_out);
    auto work = [&](uint32_t a, uint32_t b) {
        for (uint32_t r = a; r < b; r++) {
            const unsigned char* q = reinterpret_cast<const unsigned char*>(queries) + offsets[r];
            const uint64_t len = offsets[r + 1] - offsets[r];
            for (uint64_t u = 0; u * 64 < len; u++) {
                uint64_t p0 = 0, p1 = 0, ot = 0;
                const uint64_t n = len - u * 64 < 64 ? len - u * 64 : 64;
                for (uint64_t i = 0; i < n; i++) {
                    const unsigned c = q[u * 64 + i] & 0xDFu;  // upper case
                    const unsigned x = (c >> 1) & 3u, code = x ^ (x >> 1);  // A 0, C 1, G 2, T 3
                    const bool ok = c == 'A' || c == 'C' || c == 'G' || c == 'T';
                    if (ok) { p0 |= (uint64_t)(code & 1u) << i; p1 |= (uint64_t)(code >> 1) << i; } else ot |= 1ull << i;
                }
                pl[2 * (first[r] + u)] = p0;
                pl[2 * (first[r] + u) + 1] = p1;
                if (other_out) other_out[first[r] + u] = ot;
            }
        }
    };
    const int nt = threads < 1 ? 1 : threads > 64 ? 64 : threads;
    if (nt == 1 || num_queries < 4096u) work(0, num_queries);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++)
            th.emplace_back(work, (uint32_t)((uint64_t)num_queries * t / nt), (uint32_t)((uint64_t)num_queries * (t + 1) / nt));
        for (auto& x : th) x.join();
    }
    return SLAMEM_OK;
}

// device -> host copy for a front end that fills its (pinned) read buffers from device memory (bench.py, tools): one DMA into
// page-locked memory instead of the runtime's staged copy of pageable memory
int slamem_copy_to_host(void* dst_host, const void* src_dev, uint64_t bytes) {
    if (bytes && (!dst_host || !src_dev)) { set_error("slamem_copy_to_host: null argument"); return SLAMEM_ERR_ARG; }
    if (bytes) SLAMEM_HIP(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
    return SLAMEM_OK;
}

int slamem_pinned_free(void* p) {
    if (p) SLAMEM_HIP(hipHostFree(p));
    return SLAMEM_OK;
}

int slamem_stream_destroy(slamem_stream* s) {
    if (!s) return SLAMEM_OK;
    {
        std::unique_lock<std::mutex> lk(s->mu);
        // batches in flight finish first: never tear buffers down under a running kernel
        s->cv.wait(lk, [&] {
            for (int k = 0; k < s->nslots; k++)
                if (s->slot[k].state == QUEUED || s->slot[k].state == UPLOADED || s->slot[k].state == PREPARED ||
                    s->slot[k].state == LAUNCHED || s->slot[k].state == K8_ISSUED) return false;
            return true;
        });
        s->stop = true;
    }
    s->cv.notify_all();
    for (int k = 0; k < s->nthreads; k++)
        if (s->th[k].joinable()) s->th[k].join();
    (void)hipSetDevice(s->device);
    teardown(s);
    delete s;
    return SLAMEM_OK;
}

int slamem_stream_create(const slamem_index* idx, int slots, uint64_t max_batch_chars, uint32_t max_batch_queries,
                         int both_strands, int match_type, slamem_stream** out) {
    if (!idx || !out || slots < 2 || slots > kMaxSlots || max_batch_queries == 0 || (match_type < 0 || match_type > 8)) {
        set_error("slamem_stream_create: bad argument (2..8 slots, at least one query per batch, match type 0 to 8)");
        return SLAMEM_ERR_ARG;
    }
    *out = nullptr;
    SLAMEM_HIP(hipSetDevice(idx->device));
    slamem_stream* s = new (std::nothrow) slamem_stream();
    if (s) s->slot.reset(new (std::nothrow) Slot[slots]);
    if (!s || !s->slot) { delete s; set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    s->idx = idx;
    s->device = idx->device;
    s->trace = getenv("SLAMEM_STREAM_TRACE") != nullptr;
    s->t0 = std::chrono::steady_clock::now();
    s->nslots = slots;
    s->both = both_strands ? 1 : 0;
    s->match_type = match_type;
    s->max_chars = max_batch_chars;
    s->max_q = max_batch_queries;
    int rc = SLAMEM_OK;
    {
        int lo = 0, hi = 0;  // (numerically lower = higher priority)
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        const char* v = getenv("SLAMEM_STREAM_CARRY");
        if (v) s->carry = atoi(v) != 0;
        v = getenv("SLAMEM_STREAM_SEARCH_STREAMS");
        const bool two = v && atoi(v) == 2 && !s->carry;
        v = getenv("SLAMEM_STREAM_PREP_PRIORITY");
        const bool prio = v ? atoi(v) != 0 : two;
        for (int k = 0; k < s->nthreads; k++) {
            // the preparation's workgroups go first where K8's waves retire (it is what the next K8 waits for)
            hipError_t e = (prio && k == T_PREP) ? hipStreamCreateWithPriority(&s->st[k], hipStreamNonBlocking, hi)
                                                 : hipStreamCreateWithFlags(&s->st[k], hipStreamNonBlocking);
            if (e != hipSuccess) { rc = hip_fail(e, "hipStreamCreate", __FILE__, __LINE__); break; }
        }
        // K9 on a stream of its own (SLAMEM_STREAM_PLACE_STREAM=1) was measured and lost: behind a K8 that holds every wave
        // slot its small kernels wait for the next tail (43-44 ms against 38.5)
        v = getenv("SLAMEM_STREAM_PLACE_STREAM");
        if (rc == SLAMEM_OK && v && atoi(v) != 0) {
            hipError_t e = hipStreamCreateWithFlags(&s->st_place, hipStreamNonBlocking);
            if (e != hipSuccess) rc = hip_fail(e, "hipStreamCreate", __FILE__, __LINE__);
        }
        v = getenv("SLAMEM_STREAM_K8_WAVES");
        if (v && atoi(v) > 0) s->k8_waves = (uint32_t)atoi(v);
        // SLAMEM_STREAM_SEARCH_STREAMS=2 (measured at the end of round 3, not the default): even / odd batches on two search
        // streams, each K8 on 2560 of the chip's 4096 wave slots while another batch follows, the preparation on a high-priority
        // stream -- K8 (b+1) fills in as K8 (b) drains and the preparation of b+2 finds slots beside them.  Million-read batches
        // gain (headline stream 38.3 -> 37.5 ms, 30 M reads 109.0 -> 102.5 ms), two-million-read batches lose (102.3 -> 103.9 ms),
        // the command line does not move: profiles/r03_host_leg_two_streams.jsonl.
        if (rc == SLAMEM_OK && two) {
            hipError_t e = hipStreamCreateWithFlags(&s->st_search2, hipStreamNonBlocking);
            if (e != hipSuccess) rc = hip_fail(e, "hipStreamCreate", __FILE__, __LINE__);
            else s->search_streams = 2;
        }
    }
    {
        const char* v = getenv("SLAMEM_STREAM_UPLOAD_SPLIT");
        if (v && atoi(v) >= 1 && atoi(v) <= 4) s->upload_split = atoi(v);
        for (int k = 0; rc == SLAMEM_OK && k + 1 < s->upload_split; k++) {
            hipError_t e = hipStreamCreateWithFlags(&s->st_upx[k], hipStreamNonBlocking);
            if (e != hipSuccess) rc = hip_fail(e, "hipStreamCreate", __FILE__, __LINE__);
        }
    }
    if (rc != SLAMEM_OK) {
        teardown(s);  // (every HIP stream made so far, st_place and st_search2 among them)
        delete s;
        return rc;
    }
    for (int k = 0; k < s->nthreads; k++) s->th[k] = std::thread(worker, s, k);
    *out = s;
    return SLAMEM_OK;
}

int slamem_stream_set_max_occ(slamem_stream* s, uint32_t max_occ) {
    if (!s) { set_error("slamem_stream_set_max_occ: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->match_type != 3 && max_occ != 0) {
        set_error("slamem_stream_set_max_occ: an occurrence cap needs match type 3 (-smem)");
        return SLAMEM_ERR_ARG;
    }
    if (has_batches(s, "slamem_stream_set_max_occ", "set the cap")) return SLAMEM_ERR_ARG;
    s->max_occ = max_occ;
    return SLAMEM_OK;
}

int slamem_stream_set_max_gap(slamem_stream* s, uint32_t max_gap) {
    if (!s) { set_error("slamem_stream_set_max_gap: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->match_type != 4 && !is_aln(s) && max_gap != 0) {
        set_error("slamem_stream_set_max_gap: a maximum gap needs match type 4 (-chain)");
        return SLAMEM_ERR_ARG;
    }
    if (max_gap >= 0x80000000u) {
        set_error("slamem_stream_set_max_gap: the maximum gap must be below 2^31");
        return SLAMEM_ERR_ARG;
    }
    if (has_batches(s, "slamem_stream_set_max_gap", "set the gap")) return SLAMEM_ERR_ARG;
    s->max_gap = max_gap;
    return SLAMEM_OK;
}

int slamem_stream_set_ext_params(slamem_stream* s, uint32_t mismatch_penalty, uint32_t xdrop) {
    if (!s) { set_error("slamem_stream_set_ext_params: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->match_type != 5 && !is_aln(s) && (mismatch_penalty != 0 || xdrop != kExtXdropUnset)) {
        set_error("slamem_stream_set_ext_params: a mismatch penalty or an X-drop needs match type 5 (-ext)");
        return SLAMEM_ERR_ARG;
    }
    if (has_batches(s, "slamem_stream_set_ext_params", "set the parameters")) return SLAMEM_ERR_ARG;
    s->ext_penalty = mismatch_penalty;
    s->ext_xdrop = xdrop;
    return SLAMEM_OK;
}

int slamem_stream_set_max_edits(slamem_stream* s, uint32_t max_edits) {
    if (!s) { set_error("slamem_stream_set_max_edits: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    if (!is_aln(s) && max_edits != kAlnEditsUnset) {
        set_error("slamem_stream_set_max_edits: an edit limit needs match type 6 (-aln)");
        return SLAMEM_ERR_ARG;
    }
    AlnCosts costs;
    if (decode_aln_word("slamem_stream_set_max_edits", max_edits, &costs) != SLAMEM_OK) return SLAMEM_ERR_ARG;
    if (s->end_band && !costs.affine) {
        set_error("slamem_stream_set_max_edits: the stream has an end band (slamem_stream_set_end_band), which needs gap-affine costs in the word");
        return SLAMEM_ERR_ARG;
    }
    if (has_batches(s, "slamem_stream_set_max_edits", "set the limit")) return SLAMEM_ERR_ARG;
    s->max_edits = max_edits;
    return SLAMEM_OK;
}

int slamem_stream_set_end_band(slamem_stream* s, uint32_t end_band) {
    if (!s) { set_error("slamem_stream_set_end_band: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    if (!is_aln(s) && end_band) {
        set_error("slamem_stream_set_end_band: an end band needs match type 6 (-aln)");
        return SLAMEM_ERR_ARG;
    }
    FilterParams p = {};
    p.max_edits = s->max_edits == kAlnEditsUnset ? 0u : s->max_edits;
    if (set_end_band("slamem_stream_set_end_band", end_band, &p) != SLAMEM_OK) return SLAMEM_ERR_ARG;
    if (has_batches(s, "slamem_stream_set_end_band", "set the band")) return SLAMEM_ERR_ARG;
    s->end_band = end_band;
    return SLAMEM_OK;
}

int slamem_stream_alns(slamem_stream* s, const slamem_aln** segs_out, const uint32_t** ops_out, const uint64_t** op_offsets_out,
                       uint64_t* num_ops_out) {
    if (!s || !segs_out || !ops_out || !op_offsets_out || !num_ops_out) { set_error("slamem_stream_alns: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    *segs_out = nullptr; *ops_out = nullptr; *op_offsets_out = nullptr; *num_ops_out = 0;
    if (s->match_type == 8) { set_error("slamem_stream_alns: a stream of match type 8 (-pile) keeps its segments on the device"); return SLAMEM_ERR_ARG; }
    if (!is_aln(s)) { set_error("slamem_stream_alns: the stream's match type is not 6 (-aln)"); return SLAMEM_ERR_ARG; }
    const Slot* sl = last_returned(s, "slamem_stream_alns", "segments");
    if (!sl) return SLAMEM_ERR_ARG;
    *segs_out = sl->h_segs.get(); *ops_out = sl->h_ops.get(); *op_offsets_out = sl->h_ooff.get(); *num_ops_out = sl->ops_total;
    return SLAMEM_OK;
}

int slamem_stream_maps(slamem_stream* s, const slamem_map** reads_out) {
    if (!s || !reads_out) { set_error("slamem_stream_maps: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    *reads_out = nullptr;
    if (!is_map(s)) { set_error("slamem_stream_maps: the stream's match type is not 7 (-paf) or 8 (-pile)"); return SLAMEM_ERR_ARG; }
    const Slot* sl = last_returned(s, "slamem_stream_maps", "reads");
    if (!sl) return SLAMEM_ERR_ARG;
    *reads_out = sl->h_reads.get();
    return SLAMEM_OK;
}

int slamem_stream_set_md(slamem_stream* s, int on) {
    if (!s) { set_error("slamem_stream_set_md: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->match_type != 7) {
        set_error("slamem_stream_set_md: the MD pass needs match type 7 (-paf)");
        return SLAMEM_ERR_ARG;
    }
    if (has_batches(s, "slamem_stream_set_md", "switch the MD pass on")) return SLAMEM_ERR_ARG;
    if (on && !s->idx->view.tpl) {
        set_error("slamem_stream_set_md: the MD entries take the reference letters from the text planes of the index, and this index "
                  "has none (the compact layout, or one built with the seed sections switched off)");
        return SLAMEM_ERR_ARG;
    }
    s->md = on != 0;
    return SLAMEM_OK;
}

int slamem_stream_md(slamem_stream* s, const uint32_t** md_out, const uint64_t** md_offsets_out, const uint32_t** seg_eq_out,
                     const uint32_t** primary_out, uint64_t* num_md_out) {
    if (!s || !md_out || !md_offsets_out || !seg_eq_out || !primary_out || !num_md_out) {
        set_error("slamem_stream_md: null argument");
        return SLAMEM_ERR_ARG;
    }
    std::unique_lock<std::mutex> lk(s->mu);
    *md_out = nullptr; *md_offsets_out = nullptr; *seg_eq_out = nullptr; *primary_out = nullptr; *num_md_out = 0;
    if (!s->md) { set_error("slamem_stream_md: the stream's MD pass is not switched on (slamem_stream_set_md)"); return SLAMEM_ERR_ARG; }
    const Slot* sl = last_returned(s, "slamem_stream_md", "entries");
    if (!sl) return SLAMEM_ERR_ARG;
    *md_out = sl->h_md.get(); *md_offsets_out = sl->h_md_off.get(); *seg_eq_out = sl->h_seg_eq.get(); *primary_out = sl->h_primary.get();
    *num_md_out = sl->md_total;
    return SLAMEM_OK;
}

int slamem_stream_set_pileup(slamem_stream* s, slamem_pileup* pile, uint32_t min_mapq) {
    if (!s || !pile) { set_error("slamem_stream_set_pileup: null argument"); return SLAMEM_ERR_ARG; }
    SLAMEM_TRY(pile_refuse_child(pile, "slamem_stream_set_pileup"));
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->match_type != 8) {
        set_error("slamem_stream_set_pileup: an accumulator needs match type 8 (-pile)");
        return SLAMEM_ERR_ARG;
    }
    if (pileup_device(pile) != s->idx->device) {
        set_error("slamem_stream_set_pileup: the accumulator lives on device %d, the stream's index on device %d", pileup_device(pile),
                  s->idx->device);
        return SLAMEM_ERR_ARG;
    }
    if (min_mapq > 60u) {
        set_error("slamem_stream_set_pileup: the minimum mapping quality is 0 to 60");
        return SLAMEM_ERR_ARG;
    }
    if (has_batches(s, "slamem_stream_set_pileup", "set the accumulator")) return SLAMEM_ERR_ARG;
    if (s->dedup && !pileup_has_dedup(pile)) {
        set_error("slamem_stream_set_pileup: the stream's duplicate filter is on and this accumulator has none enabled");
        return SLAMEM_ERR_ARG;
    }
    s->pile = pile;
    s->min_mapq = min_mapq;
    return SLAMEM_OK;
}

int slamem_stream_set_dedup(slamem_stream* s, int on) {
    if (!s) { set_error("slamem_stream_set_dedup: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->match_type != 8) {
        set_error("slamem_stream_set_dedup: the duplicate filter needs match type 8 (-pile)");
        return SLAMEM_ERR_ARG;
    }
    if (has_batches(s, "slamem_stream_set_dedup", "switch the duplicate filter on")) return SLAMEM_ERR_ARG;
    if (on && (!s->pile || !pileup_has_dedup(s->pile))) {
        set_error("slamem_stream_set_dedup: the stream needs an accumulator whose duplicate filter is enabled (slamem_pileup_enable_dedup, "
                  "then slamem_stream_set_pileup)");
        return SLAMEM_ERR_ARG;
    }
    s->dedup = on != 0;
    return SLAMEM_OK;
}

int slamem_stream_set_quals(slamem_stream* s, uint32_t phred_offset) {
    if (!s) { set_error("slamem_stream_set_quals: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    if (has_batches(s, "slamem_stream_set_quals", "switch the quality sums on")) return SLAMEM_ERR_ARG;
    if (!s->pile || !pileup_has_quals(s->pile)) {
        set_error("slamem_stream_set_quals: the stream needs an accumulator whose quality sums are enabled (slamem_pileup_enable_quals, "
                  "then slamem_stream_set_pileup)");
        return SLAMEM_ERR_ARG;
    }
    if (phred_offset > 255u) { set_error("slamem_stream_set_quals: the Phred offset is 0 to 255, not %u", phred_offset); return SLAMEM_ERR_ARG; }
    s->quals = true;
    s->phred_offset = phred_offset;
    return SLAMEM_OK;
}

int slamem_stream_set_stats(slamem_stream* s, slamem_stats* st, uint32_t min_mapq, int with_quals) {
    if (!s || !st) { set_error("slamem_stream_set_stats: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    if (!is_map(s)) {
        set_error("slamem_stream_set_stats: a table needs match type 7 (-paf) or 8 (-pile)");
        return SLAMEM_ERR_ARG;
    }
    if (stats_device(st) != s->idx->device) {
        set_error("slamem_stream_set_stats: the table lives on device %d, the stream's index on device %d", stats_device(st), s->idx->device);
        return SLAMEM_ERR_ARG;
    }
    if (min_mapq > 60u) {
        set_error("slamem_stream_set_stats: the minimum mapping quality is 0 to 60");
        return SLAMEM_ERR_ARG;
    }
    if (has_batches(s, "slamem_stream_set_stats", "set the table")) return SLAMEM_ERR_ARG;
    if (!s->idx->view.tpl) {
        set_error("slamem_stream_set_stats: the substitution table takes the reference letters from the text planes of the index, and "
                  "this index has none (the compact layout, or one built with the seed sections switched off)");
        return SLAMEM_ERR_ARG;
    }
    s->stats = st;
    s->stats_min_mapq = min_mapq;
    s->stats_quals = with_quals != 0;
    return SLAMEM_OK;
}

int slamem_stream_dups(slamem_stream* s, const uint8_t** flags_out) {
    if (!s || !flags_out) { set_error("slamem_stream_dups: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    *flags_out = nullptr;
    if (!s->dedup) { set_error("slamem_stream_dups: the stream's duplicate filter is not switched on (slamem_stream_set_dedup)"); return SLAMEM_ERR_ARG; }
    const Slot* sl = last_returned(s, "slamem_stream_dups", "flags");
    if (!sl) return SLAMEM_ERR_ARG;
    *flags_out = sl->h_dup.get();
    return SLAMEM_OK;
}

int slamem_stream_mismatches(slamem_stream* s, const uint32_t** out) {
    if (!s || !out) { set_error("slamem_stream_mismatches: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    *out = nullptr;
    if (s->match_type != 5) { set_error("slamem_stream_mismatches: the stream's match type is not 5 (-ext)"); return SLAMEM_ERR_ARG; }
    const Slot* sl = last_returned(s, "slamem_stream_mismatches", "rows");
    if (!sl) return SLAMEM_ERR_ARG;
    *out = sl->h_mm.get();
    return SLAMEM_OK;
}

int slamem_stream_submit(slamem_stream* s, const char* queries, const uint64_t* offsets, uint32_t num_queries, uint32_t min_len) {
    if (!s || !offsets || (num_queries && !queries)) { set_error("slamem_stream_submit: null argument"); return SLAMEM_ERR_ARG; }
    if (min_len < 1) { set_error("slamem_stream_submit: minimum MEM length must be >= 1"); return SLAMEM_ERR_ARG; }
    Batch b;
    b.chars = queries; b.offs = offsets; b.nq = num_queries; b.min_len = min_len;
    return enqueue(s, "slamem_stream_submit", b);
}

int slamem_stream_submit_masked(slamem_stream* s, const char* queries, const uint64_t* lowq, const uint64_t* offsets, uint32_t num_queries,
                                uint32_t min_len) {
    if (!s || !offsets || (num_queries && !queries)) { set_error("slamem_stream_submit_masked: null argument"); return SLAMEM_ERR_ARG; }
    if (min_len < 1) { set_error("slamem_stream_submit_masked: minimum MEM length must be >= 1"); return SLAMEM_ERR_ARG; }
    if (s->match_type != 8) {  // (the match type is set once, at slamem_stream_create)
        set_error("slamem_stream_submit_masked: a low-quality mask needs match type 8 (-pile)");
        return SLAMEM_ERR_ARG;
    }
    Batch b;
    b.chars = queries; b.lowq = lowq; b.offs = offsets; b.nq = num_queries; b.min_len = min_len;
    return enqueue(s, "slamem_stream_submit_masked", b);
}

int slamem_stream_submit_quals(slamem_stream* s, const char* queries, const uint8_t* quals, const uint64_t* lowq, const uint64_t* offsets,
                               uint32_t num_queries, uint32_t min_len) {
    if (!s || !offsets || (num_queries && (!queries || !quals))) { set_error("slamem_stream_submit_quals: null argument"); return SLAMEM_ERR_ARG; }
    if (min_len < 1) { set_error("slamem_stream_submit_quals: minimum MEM length must be >= 1"); return SLAMEM_ERR_ARG; }
    if (!s->quals && !s->stats_quals) {  // (set before the first batch, and never taken back)
        set_error("slamem_stream_submit_quals: the stream's quality sums are not switched on (slamem_stream_set_quals, or "
                  "slamem_stream_set_stats with its quality sections)");
        return SLAMEM_ERR_ARG;
    }
    static const uint8_t none = 0;  // (a batch without reads has no bytes; the pointer only says that the batch came this way)
    Batch b;
    b.chars = queries; b.lowq = lowq; b.quals = quals ? quals : &none; b.offs = offsets; b.nq = num_queries; b.min_len = min_len;
    return enqueue(s, "slamem_stream_submit_quals", b);
}

int slamem_stream_submit_packed(slamem_stream* s, const void* planes, const uint64_t* other, const uint64_t* offsets, uint32_t num_queries,
                                uint64_t num_units, uint32_t min_len) {
    if (!s || !offsets || (num_queries && !planes)) { set_error("slamem_stream_submit_packed: null argument"); return SLAMEM_ERR_ARG; }
    if (((uintptr_t)planes & 15u) != 0) { set_error("slamem_stream_submit_packed: planes must be 16-byte aligned"); return SLAMEM_ERR_ARG; }
    if (min_len < 1) { set_error("slamem_stream_submit_packed: minimum MEM length must be >= 1"); return SLAMEM_ERR_ARG; }
    Batch b;
    b.planes = planes; b.other = other; b.units = num_units; b.offs = offsets; b.nq = num_queries; b.min_len = min_len;
    return enqueue(s, "slamem_stream_submit_packed", b);
}

int slamem_stream_next(slamem_stream* s, const slamem_mem** mems_out, const uint64_t** block_offsets_out, uint64_t* total_out,
                       uint32_t* num_queries_out, slamem_timings* timings_out) {
    if (!s || !mems_out || !block_offsets_out || !total_out) { set_error("slamem_stream_next: null argument"); return SLAMEM_ERR_ARG; }
    std::unique_lock<std::mutex> lk(s->mu);
    // the result handed out by the previous call goes back to the pool
    if (s->returned > 0) {
        Slot& prev = s->slot[(s->returned - 1) % (uint64_t)s->nslots];
        if (prev.state == RETURNED) { prev.state = FREE; s->cv.notify_all(); }
    }
    if (s->returned == s->submitted) { set_error("slamem_stream_next: no batch is pending"); return SLAMEM_ERR_ARG; }
    Slot& sl = s->slot[s->returned % (uint64_t)s->nslots];
    s->cv.wait(lk, [&] { return sl.state == DONE; });
    sl.state = RETURNED;
    s->returned++;
    *mems_out = sl.h_mems.get();
    *block_offsets_out = sl.h_boff.get();
    *total_out = sl.total;
    if (num_queries_out) *num_queries_out = sl.nq;
    if (timings_out) *timings_out = sl.tm;
    if (sl.rc != SLAMEM_OK) set_error("%s", sl.err);
    return sl.rc;
}

}  // extern "C"
