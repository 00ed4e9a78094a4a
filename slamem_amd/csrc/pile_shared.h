// pile_shared.h -- what pile_filter.hip (-pile and -sites), event_filter.hip (the indel events of -vcf,
// DESIGN.md 4.18), cons_filter.hip (the consensus of -cons), depth_filter.hip (the runs of -depth) and
// dedup_filter.hip (the duplicate filter of -dedup) and qual_filter.hip (the quality sums of -wq) and stats_filter.hip (the table of -stats) have in common: the accumulator's record, a batch as slamem_pileup_add_device takes it, the walk of a read's
// segments (letters of the scanned strand, the steps of an operation, the low-quality mask's window, the quality bytes, the text's letter), and the two entry points of the read-out's scratch that
// the event side borrows.
#pragma once
#include "common.h"

#include <atomic>

namespace slamem {

struct EvTable;  // ev_table.h: the hash table of the indel events, its counters and its read-out's scratch
struct SvTable;  // sv_filter.hip: the hash table of the junctions, the same table with its own counters
struct ConsScratch;  // cons_filter.hip: the consensus read-out's scratch (a flag byte per row, the sorted events and their marks)
struct DepthScratch;  // depth_filter.hip: the depth read-out's scratch (three numbers per tile)
struct DdTable;  // dedup_filter.hip: the hash table of the duplicate filter, its counters and the order of its adds

}  // namespace slamem

struct slamem_pileup {
    const slamem_index* idx;
    int device;
    uint32_t n;
    int32_t* diff;
    uint32_t* cnt;
    uint32_t* tile;  // the read-out's tile sums: n / kPileTile + 2 words
    uint64_t* sel;   // the sparse read-out's selected rows per tile: n / kPileTile + 2 words of 64 bits
    slamem::EvTable* ev;  // nullptr: events are not enabled
    slamem::SvTable* sv;  // nullptr: junctions are not enabled
    slamem::ConsScratch* cons;  // nullptr: no consensus was read yet
    slamem::DepthScratch* depth;  // nullptr: no depth runs were read yet
    slamem::DdTable* dd;  // nullptr: the duplicate filter is not enabled
    slamem_pileup* fwd;   // nullptr: strand counts are not enabled; else the forward accumulator, owned
    slamem_pileup* qual;  // nullptr: quality sums are not enabled; else the quality accumulator, owned
    bool child;           // this is the forward or the quality accumulator of another: no adds of reads, nothing to enable, freed by its owner
    bool child_qual;      // child: which of the two
    std::atomic<bool> used;  // something was added since creation or the last reset
};

namespace slamem {

namespace {

constexpr uint32_t kPileLaneOps = 32;   // operations of a segment a lane walks alone; more: the wave kernel
constexpr uint32_t kPileTile = 2048;    // entries of diff per workgroup of the read-out (256 lanes x 8)
constexpr unsigned kPileWaveGrid = 2048;
constexpr uint32_t kOpEq = 7, kOpX = 8, kOpI = 1, kOpD = 2;  // BAM's codes, as aln_filter.hip writes them

inline unsigned pile_grid(uint64_t items, unsigned block) { return items ? (unsigned)((items + block - 1) / block) : 1u; }

// A 0, C 1, G 2, T 3 (either case); anything else 4
__device__ __forceinline__ uint32_t pile_code(uint32_t byte) {
    const uint32_t u = byte & 0xDFu, y = (u >> 1) & 3u, code = y ^ (y >> 1);
    return ((0x54474341u >> (8u * code)) & 0xFFu) == u ? code : 4u;
}

// the read as the search saw it: letter x of the scanned strand
struct PileRead {
    const unsigned char* rec;
    uint64_t len;
    bool rev;
};
__device__ __forceinline__ uint32_t pile_letter(const PileRead& r, uint64_t x) {
    if (x >= r.len) return 4u;
    if (!r.rev) return pile_code(r.rec[x]);
    const uint32_t c = pile_code(r.rec[r.len - 1u - x]);
    return c < 4u ? 3u - c : 4u;
}

__device__ __forceinline__ uint32_t pile_ref_step(uint32_t op) {
    const uint32_t c = op & 15u;
    return (c == kOpEq || c == kOpX || c == kOpD) ? op >> 4 : 0u;
}
__device__ __forceinline__ uint32_t pile_query_step(uint32_t op) {
    const uint32_t c = op & 15u;
    return (c == kOpEq || c == kOpX || c == kOpI) ? op >> 4 : 0u;
}

struct PileBatch {
    const unsigned char* queries;
    const uint64_t* offsets;
    const slamem_aln* segs;
    const uint64_t* roff;
    const uint32_t* ops;
    const uint64_t* ooff;
    const slamem_map* reads;
    uint64_t nq;
    uint32_t min_mapq;
};

__device__ __forceinline__ bool pile_contributes(const PileBatch& b, uint64_t r, PileRead& out) {
    const slamem_map m = b.reads[r];
    if (m.strand == 0u || m.mapq < b.min_mapq) return false;
    const uint64_t o = b.offsets[r];
    out.rec = b.queries + o;
    out.len = b.offsets[r + 1] - o;
    out.rev = m.strand == 2u;
    return true;
}

// ---- the low-quality mask -----------------------------------------------------------------------------------
// bit off + i of `words` belongs to letter i of the read as given; every load below takes a word that holds a bit of the read
struct PileLow {
    const uint64_t* words;
    uint64_t off, len;
    bool rev;
};

// bits [at, at + c) of the mask, c in 1 .. 64, all of them letters of one read: bit i of the result is bit at + i.  The window
// comes from two neighbouring words (a funnel shift); the second one is loaded only when the window reaches into it, so that
// it holds bit at + c - 1 -- a letter of the read, never a word behind the mask's last.
__device__ __forceinline__ uint64_t lowq_window(const uint64_t* __restrict__ words, uint64_t at, uint32_t c) {
    const uint32_t s = (uint32_t)(at & 63u);
    uint64_t w = words[at >> 6] >> s;
    if (s + c > 64u) w |= words[(at >> 6) + 1u] << (64u - s);  // (s > 0 here)
    return c < 64u ? w & ((1ull << c) - 1ull) : w;
}

// the mask over letters [q, q + c) of the scanned strand, c in 1 .. 64: bit i belongs to letter q + i.  On strand 2 that is the
// given letter len - 1 - q - i: the window over the mirrored range, bit-reversed.  Letters behind the read's end have no bit.
__device__ __forceinline__ uint64_t lowq_letters(const PileLow& m, uint64_t q, uint32_t c) {
    if (q >= m.len) return 0ull;
    const uint32_t cv = m.len - q < c ? (uint32_t)(m.len - q) : c;
    if (!m.rev) return lowq_window(m.words, m.off + q, cv);
    return __brevll(lowq_window(m.words, m.off + (m.len - q - cv), cv)) >> (64u - cv);
}

template <bool kMasked>
__device__ __forceinline__ PileLow pile_low(const PileBatch& b, const PileRead& rd, const uint64_t* lowq) {
    PileLow m = {nullptr, 0, 0, false};
    if constexpr (kMasked) {
        m.words = lowq;
        m.off = (uint64_t)(rd.rec - b.queries);
        m.len = rd.len;
        m.rev = rd.rev;
    }
    return m;
}

// ---- the quality bytes of a read (qual_filter.hip and stats_filter.hip) ---------------------------------------
// the quality bytes of one read as given, and the Phred offset
struct QualRead {
    const unsigned char* qb;
    uint64_t len;
    uint32_t off;
    bool rev;
};

__device__ __forceinline__ uint32_t qual_value(uint32_t byte, uint32_t off) {
    const uint32_t v = byte < off ? 0u : byte - off;
    return v < 93u ? v : 93u;
}

// the byte of letter x of the scanned strand (x < len)
__device__ __forceinline__ uint32_t qual_byte(const QualRead& r, uint64_t x) { return r.qb[r.rev ? r.len - 1u - x : x]; }

// how many of the letters [x, x + c) of the scanned strand, from x on, carry the byte `byte`: eight at a time while eight are
// left -- the eight bytes XORed with the byte in every position are 0, or the first byte in scanned order that is not says where
// the stretch ends -- then one by one.  x + c <= len: every load lies inside the read's own bytes.  On strand 2 the letters
// x .. x + 7 are the given bytes len - 8 - x .. len - 1 - x, the first of them the highest.
__device__ __forceinline__ uint32_t qual_same(const QualRead& r, uint64_t x, uint32_t c, uint32_t byte) {
    const uint64_t all = 0x0101010101010101ull * byte;
    uint32_t i = 0;
    while (i + 8u <= c) {
        uint64_t w;
        __builtin_memcpy(&w, r.qb + (r.rev ? r.len - 8u - (x + i) : x + i), 8);
        w ^= all;
        if (w) return i + (uint32_t)(r.rev ? __builtin_clzll(w) : __builtin_ctzll(w)) / 8u;
        i += 8u;
    }
    while (i < c && qual_byte(r, x + i) == byte) i++;
    return i;
}

__device__ __forceinline__ QualRead qual_read(const PileBatch& b, const PileRead& rd, const unsigned char* quals, uint32_t off) {
    return QualRead{quals + (rd.rec - b.queries), rd.len, off, rd.rev};
}

// the text's letter at x as two bits (a place at or behind n, which no X or D reaches: 0); sam_filter.hip's MD entries and
// stats_filter.hip's substitution table take it from the text planes
__device__ __forceinline__ uint32_t md_text(const TextPlanes* __restrict__ tpl, uint64_t n, uint64_t x) {
    if (x >= n) return 0u;
    const TextPlanes* u = tpl + (x >> 6);
    const uint32_t bit = (uint32_t)(x & 63u);
    return (uint32_t)((u->p0 >> bit) & 1ull) | ((uint32_t)((u->p1 >> bit) & 1ull) << 1);
}

__device__ __forceinline__ uint64_t wave_scan_inclusive(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

}  // namespace

// pile_filter.hip, for the event side: pile->tile = the exclusive prefix sums of diff per tile of kPileTile entries below `end`
// (k_pile_tile_sums and k_pile_tile_scan), and the in-place exclusive scan of `tiles` 64-bit counts with the total behind them
// (k_sites_tile_scan)
int pile_tile_prefix(slamem_pileup* pile, uint64_t end, hipStream_t stream);
int pile_scan_counts(uint64_t* sel, uint64_t tiles, hipStream_t stream);

// event_filter.hip, for pile_filter.hip: the two event kernels behind the two pile kernels of an add (events enabled), and what
// reset and free do to the table
int events_add(slamem_pileup* pile, const void* batch /* PileBatch */, hipStream_t stream);
int events_reset(slamem_pileup* pile);
void events_free(slamem_pileup* pile);

// sv_filter.hip, for pile_filter.hip: the junction kernel behind the pile kernels of an add (junctions enabled), and what reset and
// free do to the table
int junctions_add(slamem_pileup* pile, const void* batch /* PileBatch */, hipStream_t stream);
int junctions_reset(slamem_pileup* pile);
void junctions_free(slamem_pileup* pile);

// cons_filter.hip, for pile_filter.hip: what free does to the consensus read-out's scratch
void cons_free(slamem_pileup* pile);

// depth_filter.hip, for pile_filter.hip: what free does to the depth read-out's scratch
void depth_free(slamem_pileup* pile);

// dedup_filter.hip, for pile_filter.hip: what reset and free do to the duplicate filter's table
int dedup_reset(slamem_pileup* pile);
void dedup_free(slamem_pileup* pile);

}  // namespace slamem
