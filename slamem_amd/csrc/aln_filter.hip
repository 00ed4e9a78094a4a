// aln_filter.hip -- -aln (matchType 6): per strand block the gapped alignment built on the block's best chain, as segments with
// an edit count and a CIGAR.  DESIGN.md 4.14 has the definition; in short: the rows of the best chain (4.12) are the anchors, a
// row that overlaps its predecessor is trimmed at its start, the letters between two consecutive anchors (a of the strand, b of
// the text) are aligned with unit costs, a gap closes iff both pieces are A,C,G,T only and the distance is at most E (-maxed),
// a maximal run of anchors joined by closed gaps is a segment, and the block's two outer ends are extended by 4.13's X-drop rule.
//
// All on the stream behind K9, no host read-back:
//   chain_pass / _compact   the chain's rows, compacted per block (chain_filter.hip, as it stands)
//   pack_batch_planes       the batch's letters as planes (filter_shared.h)
//   k_aln_geom              a lane per chain row: its block (binary search in the offsets), the trimming, the gap to its
//                           predecessor, the outer ends (walk), the runs of what it decides itself.  A gap with a == b <= 64 and
//                           at most two differing letters is decided here (distance = those letters); any other gap with
//                           |a - b| <= E goes to a list (one atomic each)
//   k_aln_wave              a wave per listed gap (a fixed grid of one-wave workgroups loops over the list): furthest-reaching
//                           points f[s][k] per edit count s and diagonal k = y - x, lanes hold the diagonals, the previous
//                           wavefront in LDS, every wavefront in the workgroup's slab for the traceback; the slide is the
//                           64-letter XOR compare.  The traceback needs f only: D[x][y] is the first s with f[s][k] >= x.
//   k_aln_wave_affine       the same for gap-affine costs (-affine): three furthest-reaching components per score
//                           s <= C = o + e E, earlier wavefronts read back from the workgroup's slab
//   k_aln_count / 3 scans   runs, edits and segment starts per row -> places
//   k_aln_segs / k_aln_write  block offsets, segment starts; a lane per row writes its runs (merged with the neighbours'), the
//                           segment's rightmost row writes the segment
#include "filter_shared.h"

namespace slamem {

namespace {

// One-wave workgroups that share the list of gaps.  A wave spends its time waiting for the next window, so the more the chip
// holds the better: up to 8,192 (32 a CU), fewer when the edit limit makes a workgroup's wavefront slab large -- the slabs of a
// call together stay within 64 MiB (8,192 workgroups at the default 31 edits, 514 at 127).
inline unsigned aln_wave_grid(uint32_t max_edits) {
    const uint64_t slab = (uint64_t)(max_edits + 1) * (2 * max_edits + 1) * 4, fit = (64ull << 20) / slab;
    return (unsigned)(fit > 8192 ? 8192 : fit < 256 ? 256 : fit);
}
// Gap-affine costs: the costs of a filter's max_edits word (resolve_filter_params has checked it), a workgroup's slab of three
// components for the scores 0 .. C over the diagonals |k| <= E, and the grid by the same 64 MiB rule (C <= kAlnMaxCost bounds a
// slab by 1.6 MB, so at least 41 workgroups fit; 1,286 at the default 31 edits and costs 4,6,2).
inline AlnCosts aln_costs(uint32_t word) {
    AlnCosts c;
    int affine = 0;
    (void)slamem_decode_aln_word(word, &c.E, &c.x, &c.o, &c.e, &affine);
    c.affine = affine != 0;
    c.C = c.o + c.e * c.E;
    return c;
}
inline uint64_t aln_affine_slab_words(const AlnCosts& c) { return 3ull * (c.C + 1) * (2 * c.E + 1); }
inline unsigned aln_affine_grid(const AlnCosts& c) {
    const uint64_t fit = (64ull << 20) / (aln_affine_slab_words(c) * 4);
    return (unsigned)(fit > 8192 ? 8192 : fit < 1 ? 1 : fit);
}
// Outer ends (-gext): three components for the scores 0 .. Cp over the diagonals |k| <= Z, the same rule (388 KB a
// workgroup at Z = 31: 173 workgroups; 641 at Z = 8)
inline uint64_t aln_end_slab_words(uint32_t band) { return 3ull * (kAlnMaxCost + 1) * (2 * band + 1); }
inline unsigned aln_end_grid(uint32_t band) {
    const uint64_t fit = (64ull << 20) / (aln_end_slab_words(band) * 4);
    return (unsigned)(fit > 8192 ? 8192 : fit < 1 ? 1 : fit);
}
// (the gap kernel and the end kernel run one after the other and share the room)
inline uint64_t aln_slabs_bytes(uint32_t word, uint32_t band) {
    const AlnCosts c = aln_costs(word);
    const uint64_t gaps = c.affine ? (uint64_t)aln_affine_grid(c) * aln_affine_slab_words(c) * 4
                                   : (uint64_t)aln_wave_grid(c.E) * (c.E + 1) * (2 * c.E + 1) * 4;
    const uint64_t ends = band ? (uint64_t)aln_end_grid(band) * aln_end_slab_words(band) * 4 : 0;
    return gaps > ends ? gaps : ends;
}
// Runs of an affine gap: every run but those of `=` costs at least min(x, e) >= 1 (L mismatches cost L x, a gap of L letters
// o + L e), so there are at most C of them, and two runs of `=` have one of the others between them: at most 2 C + 1 runs.
constexpr uint32_t kAffineRuns = 2 * kAlnMaxCost + 1;
constexpr uint32_t kOpEq = 7u, kOpX = 8u, kOpI = 1u, kOpD = 2u;  // BAM's codes
constexpr uint32_t kFirst = 1u, kLast = 2u, kClosed = 4u, kListed = 8u, kGapEq = 16u, kRev = 32u;
constexpr int32_t kNeg = -1;

// a chain row: the trimmed anchor, the gap to its predecessor (in front of it in the strand), its outer ends
struct AlnRow {
    uint32_t tp, tq, tl;    // the anchor as used
    uint32_t a, b;          // letters of the strand / of the text between the predecessor's end and the anchor
    uint32_t extl, extr;    // outer ends (the block's first / last chain row only)
    uint32_t flags;         // kFirst: first of its block in the list (the chain's LAST row); kLast: the chain's first row
    uint32_t nfl, nfr;      // runs of the outer ends
    uint32_t edl, edr;      // edits of the outer ends
    uint32_t extl_t, extr_t;  // the ends' letters of the text (extl, extr: of the strand; they differ in a replaced end only)
    uint32_t scl, scr;      // the ungapped sides' scores (4.13's best)
    uint32_t sll, slr;      // a replaced end's runs: where in the slab, left to right
    uint32_t repl, repr;    // 1: the end is the gapped attempt's (-gext)
    uint32_t gapn, gapd;    // a closed gap's runs and distance
    uint32_t slab;          // a listed gap's runs: where in the slab
    uint32_t rec;           // the record of the batch
};

struct AlnLayout {
    uint64_t chain_bytes, off_ctr, off_crows, off_coff, off_ucnt, off_uoff, off_uscan, uscan_bytes, off_long, off_units, off_rows,
        off_list, off_ends, off_n, off_flag, off_ed, off_sn, off_sflag, off_sed, off_scan, scan_bytes, off_segstart, off_slab, off_f, bytes;
};

AlnLayout aln_layout(const FilterBatch& b, const FilterParams& p) {
    const uint64_t num_queries = b.num_queries, num_blocks = b.num_blocks(), query_bytes = b.query_bytes, capacity = b.capacity;
    const uint64_t ops_capacity = p.ops_capacity;
    const uint32_t max_edits = p.max_edits;
    AlnLayout m;
    m.chain_bytes = align_up(chain_workspace_bytes(b, p), 256);  // (the -mem list K9 places lies in here)
    uint64_t off = m.chain_bytes;
    m.off_ctr = off;    off = align_up(off + 64, 256);                                  // [2] listed records, [3] listed gaps, [4] slab words, [5] listed ends, [6] ends replaced
    m.off_crows = off;  off = align_up(off + capacity * sizeof(slamem_mem) + 16, 256);  // the chains' rows
    m.off_coff = off;   off = align_up(off + (num_blocks + 1) * 8, 256);                // ... and their block offsets
    m.off_ucnt = off;   off = align_up(off + (num_queries + 1) * 4, 256);
    m.off_uoff = off;   off = align_up(off + (num_queries + 1) * 8, 256);
    size_t need = 0;
    (void)scan_sum_exclusive_u32_u64(nullptr, need, nullptr, nullptr, num_queries, 0);
    m.uscan_bytes = need;
    m.off_uscan = off;  off = align_up(off + need, 256);
    m.off_long = off;   off = align_up(off + (query_bytes / (64ull * kExtPackLaneUnits) + 1) * 8, 256);
    m.off_units = off;  off = align_up(off + (query_bytes / 64 + num_queries + 1) * sizeof(QueryUnit), 256);
    m.off_rows = off;   off = align_up(off + (capacity + 1) * sizeof(AlnRow), 256);
    m.off_list = off;   off = align_up(off + (capacity + 1) * 4, 256);                  // listed gaps (their rows)
    m.off_ends = off;   if (p.end_band) off = align_up(off + (capacity + 1) * 8, 256);  // listed ends (row << 1 | right), two a row at most
    m.off_n = off;      off = align_up(off + (capacity + 2) * 4, 256);                  // runs per row
    m.off_flag = off;   off = align_up(off + (capacity + 2) * 4, 256);                  // 1: the row is the rightmost of a segment
    m.off_ed = off;     off = align_up(off + (capacity + 2) * 4, 256);                  // edits per row
    m.off_sn = off;     off = align_up(off + (capacity + 2) * 8, 256);                  // their exclusive sums
    m.off_sflag = off;  off = align_up(off + (capacity + 2) * 8, 256);
    m.off_sed = off;    off = align_up(off + (capacity + 2) * 8, 256);
    need = 0;
    (void)scan_sum_exclusive_u32_u64(nullptr, need, nullptr, nullptr, capacity + 1, 0);
    m.scan_bytes = need;
    m.off_scan = off;   off = align_up(off + need, 256);
    m.off_segstart = off; off = align_up(off + (capacity + 2) * 4, 256);                // the rightmost row of every segment
    m.off_slab = off;   off = align_up(off + (ops_capacity + 1) * 4, 256);              // the runs of listed gaps
    m.off_f = off;      off = align_up(off + aln_slabs_bytes(max_edits, p.end_band), 256);          // wavefronts
    m.bytes = off;
    return m;
}

// what a lane knows of its block's sequences
struct Seqs {
    const uint4* Q;
    const uint4* T;
    int64_t qn, tn, len, n;
    bool rev;
};

__device__ __forceinline__ Seqs seqs_of(uint64_t rec, bool rev, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ uoff,
                                        const QueryUnit* __restrict__ units, const TextPlanes* __restrict__ tpl, uint32_t n) {
    Seqs s;
    s.len = (int64_t)(offsets[rec + 1] - offsets[rec]);
    s.qn = (s.len + 63) >> 6;
    s.n = (int64_t)n;
    s.tn = (s.n + 63) >> 6;
    s.Q = reinterpret_cast<const uint4*>(units + uoff[rec]);
    s.T = reinterpret_cast<const uint4*>(tpl);
    s.rev = rev;
    return s;
}

__device__ __forceinline__ uint64_t low_mask(int64_t k) { return k >= 64 ? ~0ull : (k <= 0 ? 0ull : (1ull << k) - 1ull); }

// runs of one operation, merged as they come; counts them, and writes them when asked to
struct Emit {
    uint32_t* out;
    uint64_t pos, cap;
    uint32_t code, len, n;
    bool write;
    __device__ __forceinline__ void flush() {
        if (len) {
            if (write && pos < cap) out[pos] = (len << 4) | code;
            pos++;
            n++;
        }
        len = 0;
        code = 0;
    }
    __device__ __forceinline__ void push(uint32_t c, uint32_t l) {
        if (!l) return;
        if (c != code) { flush(); code = c; }
        len += l;
    }
};

// the `=` / `X` runs of L letters of one diagonal, left to right (every letter inside both sequences and one of A,C,G,T)
__device__ __forceinline__ void diag_runs(const Seqs& s, int64_t q0, int64_t p0, int64_t L, Emit& em) {
    for (int64_t off = 0; off < L; off += 64) {
        const Win q = strand_window(s.Q, s.qn, s.len, s.rev, q0 + off), t = window(s.T, s.tn, s.n, p0 + off);
        const uint64_t m = (q.p0 ^ t.p0) | (q.p1 ^ t.p1);
        const uint32_t v = L - off < 64 ? (uint32_t)(L - off) : 64u;
        for (uint32_t i = 0; i < v;) {
            const uint64_t rest = m >> i;
            const bool mis = (rest & 1ull) != 0ull;
            const uint64_t x = mis ? ~rest : rest;
            uint32_t run = x ? (uint32_t)__builtin_ctzll(x) : 64u;
            if (run > v - i) run = v - i;
            em.push(mis ? kOpX : kOpEq, run);
            i += run;
        }
    }
}

// runs that a wave kernel left in the slab
__device__ __forceinline__ void slab_runs(const uint32_t* __restrict__ slab, uint64_t slab_cap, uint32_t from, uint32_t n, Emit& em) {
    for (uint32_t k = 0; k < n; k++) {
        const uint64_t at = (uint64_t)from + k;
        const uint32_t w = at < slab_cap ? slab[at] : 0u;
        em.push(w & 15u, w >> 4);
    }
}

// -gext, fact (c) of DESIGN.md 4.30: an attempt that beats the ungapped side holds a gap and scores at most a - (o + e), so a
// side that scores as much is kept here.  a is known when the walk ended at the strand's own end or bad letter (bit `fb` of the
// last window's bad mask, at distance t0 + fb = everything the walk looked at); any other end is listed.
__device__ __forceinline__ bool lists_end(uint64_t qbad, const Side& d, uint64_t t0, uint32_t gap_oe) {
    if (!qbad) return true;
    const uint64_t a = t0 + (uint64_t)__builtin_ctzll(qbad);
    return d.best + (int64_t)gap_oe < (int64_t)a;
}

// ---- a lane per chain row ----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_aln_geom(const uint64_t* __restrict__ coff, uint64_t nb, const slamem_mem* __restrict__ crows,
                                                  uint64_t cap, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ uoff,
                                                  const QueryUnit* __restrict__ units, const TextPlanes* __restrict__ tpl, uint32_t n,
                                                  uint32_t strands, uint32_t penalty, uint32_t xdrop, uint32_t max_edits,
                                                  uint32_t cost_x, uint32_t inline_d, uint32_t cost_bound, uint32_t end_band, uint32_t gap_oe, AlnRow* __restrict__ rows, uint32_t* __restrict__ list, uint32_t* __restrict__ ends, unsigned long long* __restrict__ ctr) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint64_t K = coff[nb];
    if (K > cap) K = cap;
    if (g >= K) return;
    uint64_t lo = 0, hi = nb;  // the smallest block whose end lies behind g
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (coff[mid + 1] <= g) lo = mid + 1; else hi = mid;
    }
    const uint64_t blk = lo < nb ? lo : nb - 1u;
    uint64_t s = coff[blk], e = coff[blk + 1];
    if (e > K) e = K;
    if (s > g) s = g;
    const uint64_t rec = blk / strands;
    const bool rev = (blk % strands) != 0u;
    const Seqs sq = seqs_of(rec, rev, offsets, uoff, units, tpl, n);
    const slamem_mem ri = crows[g];
    const bool has_gap = g + 1u < e;
    const slamem_mem rj = crows[has_gap ? g + 1u : g];
    const int64_t p = ri.ref_pos, q = ri.query_pos, L = ri.length;
    const int64_t eqj = (int64_t)rj.query_pos + rj.length, epj = (int64_t)rj.ref_pos + rj.length;
    int64_t o = 0;
    if (has_gap) {
        if (eqj - q > o) o = eqj - q;
        if (epj - p > o) o = epj - p;
        if (o >= L) o = L - 1;  // (never for rows that may follow one another)
    }
    AlnRow r;
    r.tp = (uint32_t)(p + o);
    r.tq = (uint32_t)(q + o);
    r.tl = (uint32_t)(L - o);
    r.flags = (g == s ? kFirst : 0u) | (g + 1u == e ? kLast : 0u) | (rev ? kRev : 0u);
    r.extl = r.extr = r.nfl = r.nfr = r.edl = r.edr = r.gapn = r.gapd = r.slab = 0u;
    r.extl_t = r.extr_t = r.scl = r.scr = r.sll = r.slr = r.repl = r.repr = 0u;
    r.rec = (uint32_t)rec;
    const int64_t a = has_gap ? q + o - eqj : 0, b = has_gap ? p + o - epj : 0;
    r.a = (uint32_t)a;
    r.b = (uint32_t)b;
    const bool inside = sq.qn > 0 && q + L <= sq.len && p + L <= sq.n && L > 0;  // (a row outside its sequences: nothing is read)
    const int64_t E = max_edits;
    if (has_gap && inside && a >= 0 && b >= 0 && (a > b ? a - b : b - a) <= E) {
        if (a == 0 && b == 0) {
            r.flags |= kClosed;
        } else if (a == b && a <= 64) {
            const Win wq = strand_window(sq.Q, sq.qn, sq.len, rev, eqj), wt = window(sq.T, sq.tn, sq.n, epj);
            const uint64_t mk = low_mask(a);
            const uint64_t bad = (wq.bad | wt.bad) & mk;
            const uint64_t m = ((wq.p0 ^ wt.p0) | (wq.p1 ^ wt.p1)) & mk;
            const uint32_t d = (uint32_t)__popcll(m);
            // Up to two differing letters on the diagonal: D = d, and the traceback stays on the diagonal.  Pieces of one length
            // cannot be one indel apart, so their distance is 0 (equal), 1 (one substitution, d = 1) or at least 2; with d <= 2
            // substitutions reach it, hence D = d.  The same holds for every pair of prefixes of one length (they have at most d
            // differing letters too), so D[x][x] = the differing letters in front of x, and the rule's diagonal step applies
            // at every cell of the diagonal.  (Three differing letters may cost 2: an inserted and a deleted letter.)
            // With costs x, o, e leaving the diagonal costs at least 2 (o + e), so d x <= 2 (o + e) letters stay
            // on it: inline_d = 2 (o + e) / x, closed iff d x <= C = o + e E.  Unit cost is x = 1, o = 0, e = 1: 2 and E, as above.
            if (!bad && d <= inline_d) {
                if (d * cost_x <= cost_bound) {
                    // runs of the mask: one per maximal stretch of equal bits
                    const uint64_t tr = (m ^ (m >> 1)) & low_mask(a - 1);
                    r.gapn = (uint32_t)__popcll(tr) + 1u;
                    r.gapd = d;
                    r.flags |= kClosed | (((m >> (a - 1)) & 1ull) ? 0u : kGapEq);
                }
            } else if (!bad) {
                r.flags |= kListed;
            }
        } else {
            r.flags |= kListed;
        }
        if (r.flags & kListed) list[atomicAdd(&ctr[3], 1ull)] = (uint32_t)g;
    }
    if (inside && (r.flags & (kFirst | kLast))) {
        const int64_t P = penalty, X = xdrop;
        Emit em = {nullptr, 0, 0, 0, 0, 0, false};
        if (r.flags & kLast) {  // (the chain's first row is not trimmed)
            Side left = {0, 0, 0, 0, 0, 0};
            Win ql = mirrored(strand_window(sq.Q, sq.qn, sq.len, rev, q - 64)), tl = mirrored(window(sq.T, sq.tn, sq.n, p - 64));
            uint64_t t0 = 0;
            while (!walk(left, ql, tl, t0, P, X)) {
                t0 += 64u;
                ql = mirrored(strand_window(sq.Q, sq.qn, sq.len, rev, q - 64 - (int64_t)t0));
                tl = mirrored(window(sq.T, sq.tn, sq.n, p - 64 - (int64_t)t0));
            }
            r.extl = r.extl_t = (uint32_t)left.ext;
            r.edl = left.mm_best;
            r.scl = (uint32_t)left.best;
            diag_runs(sq, q - (int64_t)left.ext, p - (int64_t)left.ext, (int64_t)left.ext, em);
            em.flush();
            r.nfl = em.n;
            if (end_band && g < 0x80000000ull && lists_end(ql.bad, left, t0, gap_oe)) ends[atomicAdd(&ctr[5], 1ull)] = (uint32_t)g << 1;
        }
        if (r.flags & kFirst) {
            Side right = {0, 0, 0, 0, 0, 0};
            Win qr = strand_window(sq.Q, sq.qn, sq.len, rev, q + L), tr = window(sq.T, sq.tn, sq.n, p + L);
            uint64_t t0 = 0;
            while (!walk(right, qr, tr, t0, P, X)) {
                t0 += 64u;
                qr = strand_window(sq.Q, sq.qn, sq.len, rev, q + L + (int64_t)t0);
                tr = window(sq.T, sq.tn, sq.n, p + L + (int64_t)t0);
            }
            r.extr = r.extr_t = (uint32_t)right.ext;
            r.edr = right.mm_best;
            r.scr = (uint32_t)right.best;
            const uint32_t before = em.n;
            diag_runs(sq, q + L, p + L, (int64_t)right.ext, em);
            em.flush();
            r.nfr = em.n - before;
            if (end_band && g < 0x80000000ull && lists_end(qr.bad, right, t0, gap_oe)) ends[atomicAdd(&ctr[5], 1ull)] = ((uint32_t)g << 1) | 1u;
        }
    }
    rows[g] = r;
}

// ---- a wave per listed gap -------------------------------------------------------------------------------------------------

// matching letters from (x, y) of the gap on, at most lim
__device__ __forceinline__ int64_t slide_fwd(const Seqs& s, int64_t qa, int64_t pb, int64_t x, int64_t y, int64_t lim) {
    int64_t done = 0;
    while (done < lim) {
        const Win q = strand_window(s.Q, s.qn, s.len, s.rev, qa + x + done), t = window(s.T, s.tn, s.n, pb + y + done);
        const uint64_t m = (q.p0 ^ t.p0) | (q.p1 ^ t.p1);
        const int64_t l = lim - done < 64 ? lim - done : 64;
        int64_t run = m ? (int64_t)__builtin_ctzll(m) : 64;
        if (run > l) run = l;
        done += run;
        if (run < 64) break;
    }
    return done;
}

// matching letters in front of (x, y), at most lim
__device__ __forceinline__ int64_t slide_back(const Seqs& s, int64_t qa, int64_t pb, int64_t x, int64_t y, int64_t lim) {
    int64_t done = 0;
    while (done < lim) {
        const Win q = mirrored(strand_window(s.Q, s.qn, s.len, s.rev, qa + x - done - 64));
        const Win t = mirrored(window(s.T, s.tn, s.n, pb + y - done - 64));
        const uint64_t m = (q.p0 ^ t.p0) | (q.p1 ^ t.p1);
        const int64_t l = lim - done < 64 ? lim - done : 64;
        int64_t run = m ? (int64_t)__builtin_ctzll(m) : 64;
        if (run > l) run = l;
        done += run;
        if (run < 64) break;
    }
    return done;
}

__global__ void __launch_bounds__(64) k_aln_wave(const uint32_t* __restrict__ list, const unsigned long long* __restrict__ ctr_in,
                                                 AlnRow* rows, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ uoff,
                                                 const QueryUnit* __restrict__ units, const TextPlanes* __restrict__ tpl, uint32_t n,
                                                 uint32_t max_edits, int32_t* fslab, uint32_t* __restrict__ slab, uint64_t slab_cap,
                                                 unsigned long long* __restrict__ ctr) {
    __shared__ int32_t wf[2][256];    // the last two wavefronts, by diagonal + E
    __shared__ uint32_t rbuf[256];    // the traceback's runs, last first
    __shared__ unsigned long long s_off;
    const uint32_t lane = threadIdx.x;
    const int32_t E = (int32_t)max_edits, W = 2 * E + 1;
    int32_t* F = fslab + (uint64_t)blockIdx.x * (uint64_t)(E + 1) * (uint64_t)W;
    const uint64_t nl = ctr_in[3];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint32_t g = list[li];
        const AlnRow r = rows[g];
        const Seqs sq = seqs_of(r.rec, (r.flags & kRev) != 0u, offsets, uoff, units, tpl, n);
        const int64_t a = r.a, b = r.b;
        const int64_t qa = (int64_t)r.tq - a, pb = (int64_t)r.tp - b;
        // a letter that is not A,C,G,T in either piece breaks the gap
        bool bad = false;
        for (int64_t w = lane; w * 64 < a; w += 64) {
            const Win q = strand_window(sq.Q, sq.qn, sq.len, sq.rev, qa + 64 * w);
            if (q.bad & low_mask(a - 64 * w)) bad = true;
        }
        for (int64_t w = lane; w * 64 < b; w += 64) {
            const Win t = window(sq.T, sq.tn, sq.n, pb + 64 * w);
            if (t.bad & low_mask(b - 64 * w)) bad = true;
        }
        __syncthreads();  // (nobody reads the last gap's LDS any more)
        for (uint32_t d = lane; d < 256u; d += 64u) { wf[0][d] = kNeg; wf[1][d] = kNeg; }
        if (__syncthreads_or(bad ? 1 : 0)) continue;
        const int32_t kfin = (int32_t)(b - a);
        int32_t s = 0;
        bool closed = false;
        for (;; s++) {
            const int32_t* prev = wf[(s + 1) & 1];
            int32_t* cur = wf[s & 1];
            bool fin = false;
            for (int32_t d = E - s + (int32_t)lane; d <= E + s; d += 64) {
                const int64_t k = d - E;
                int64_t c = kNeg;
                if (s == 0) {
                    c = 0;
                } else {
                    const int64_t fk = prev[d], fl = d > 0 ? prev[d - 1] : kNeg, fr = d + 1 < W ? prev[d + 1] : kNeg;
                    if (fk >= 0) {  // one more letter of both, or none at an end
                        c = fk + 1;
                        if (c > a) c = a;
                        if (c > b - k) c = b - k;
                    }
                    if (fl >= 0) {  // a text letter: from diagonal k - 1, x stays
                        int64_t v = fl < b - k ? fl : b - k;
                        const int64_t least = 1 - k > 0 ? 1 - k : 0;
                        if (v >= least && v > c) c = v;
                    }
                    if (fr >= 0) {  // a strand letter: from diagonal k + 1, x + 1
                        int64_t v = fr + 1 < a ? fr + 1 : a;
                        const int64_t least = -k - 1 > 0 ? -k - 1 : 0;
                        if (v - 1 >= least && v > c) c = v;
                    }
                }
                if (c >= 0) {
                    const int64_t lim = a - c < b - (c + k) ? a - c : b - (c + k);
                    if (lim > 0) c += slide_fwd(sq, qa, pb, c, c + k, lim);
                }
                cur[d] = (int32_t)c;
                F[(int64_t)s * W + d] = (int32_t)c;
                if (d == kfin + E && c >= a) fin = true;
            }
            if (__syncthreads_or(fin ? 1 : 0)) { closed = true; break; }
            if (s == E) break;
        }
        if (!closed) continue;
        // The traceback: D[x][y] is the first s with f[s][y - x] >= x.  Every lane runs it on the same values (a, b, the planes
        // and F are the same for all), so the lanes stay converged, their loads are one request, and the words they store to
        // rbuf[] are identical by construction.  F[] was written by other lanes through global memory: the __syncthreads_or that
        // ended the wavefront loop is the barrier (and the wait for the stores) that makes those words visible here.
        // Runs: every run but those of `=` holds an edit and two runs of `=` have one between them, so at most 2 s + 1 <= 255.
        bool overrun = false;
        int64_t x = a, y = b;
        int32_t d = s;
        uint32_t nr = 0, code = 0, len = 0;
        while (x > 0 || y > 0) {
            if (x > 0 && y > 0) {
                const int64_t run = slide_back(sq, qa, pb, x, y, x < y ? x : y);
                if (run) {
                    if (code != kOpEq) { if (len) rbuf[nr++] = (len << 4) | code; code = kOpEq; len = 0; }
                    len += (uint32_t)run;
                    x -= run;
                    y -= run;
                }
                if (x == 0 && y == 0) break;
            }
            const int32_t k = (int32_t)(y - x), sp = d - 1;
            const int32_t f_same = (sp >= 0 && k >= -sp && k <= sp) ? F[(int64_t)sp * W + k + E] : kNeg;
            const int32_t f_left = (sp >= 0 && k - 1 >= -sp && k - 1 <= sp) ? F[(int64_t)sp * W + k - 1 + E] : kNeg;
            uint32_t op;
            if (x > 0 && y > 0 && f_same >= 0 && (int64_t)f_same >= x - 1) { op = kOpX; x--; y--; }
            else if (y > 0 && (x == 0 || (f_left >= 0 && (int64_t)f_left >= x))) { op = kOpD; y--; }
            else { op = kOpI; x--; }  // (x > 0: with x == 0 there is y > 0, and the branch above was taken)
            d--;
            if (code != op) { if (len) rbuf[nr++] = (len << 4) | code; code = op; len = 0; }
            len++;
            if (nr >= 255u) { overrun = true; break; }  // (never, by the count above; if it were, the gap is left broken)
        }
        if (overrun) continue;  // (uniform)
        if (len) rbuf[nr++] = (len << 4) | code;
        if (lane == 0u) s_off = atomicAdd(&ctr[4], (unsigned long long)nr);
        __syncthreads();
        const uint64_t at = s_off;
        if (at + nr <= slab_cap)
            for (uint32_t t = lane; t < nr; t += 64u) slab[at + t] = rbuf[nr - 1u - t];
        if (lane == 0u) {
            AlnRow* o = rows + g;
            o->gapn = nr;
            o->gapd = (uint32_t)s;
            o->slab = (uint32_t)(at < 0xFFFFFFFFull ? at : 0xFFFFFFFFull);
            o->flags = r.flags | kClosed | ((nr && (rbuf[0] & 15u) == kOpEq) ? kGapEq : 0u);
        }
    }
}

// ---- a wave per listed gap, gap-affine costs -------------------------------------------------------------------

// The furthest-reaching points of three matrices per score s = 0 .. C and diagonal k = y - x, |k| <= E: M[s][k] the largest x with
// H[x][x + k] <= s, I and D the same for Im (the last step is a strand letter) and Dm (a text letter); -1: no such cell.  A score
// holds cells on the diagonals |k| <= (s - o) / e only (k = 0 below o + e), and nothing at all when none of its three sources
// s - x, s - o - e, s - e holds any: such a score is skipped, its part of the slab is never read (alive[]).  Earlier wavefronts are
// up to max(x, o + e) scores back; they are read from the workgroup's slab, behind the barrier that ends every score.
__global__ void __launch_bounds__(64) k_aln_wave_affine(const uint32_t* __restrict__ list, const unsigned long long* __restrict__ ctr_in,
                                                        AlnRow* rows, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ uoff,
                                                        const QueryUnit* __restrict__ units, const TextPlanes* __restrict__ tpl, uint32_t n,
                                                        uint32_t max_edits, uint32_t cost_x, uint32_t cost_o, uint32_t cost_e, int32_t* fslab,
                                                        uint32_t* __restrict__ slab, uint64_t slab_cap, unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t rbuf[kAffineRuns];       // the traceback's runs, last first
    __shared__ uint8_t alive[kAlnMaxCost + 1];   // per score: some cell of some component exists (and the slab holds the score)
    __shared__ unsigned long long s_off;
    const uint32_t lane = threadIdx.x;
    const int32_t E = (int32_t)max_edits, W = 2 * E + 1;
    const int32_t X = (int32_t)cost_x, O = (int32_t)(cost_o + cost_e), G = (int32_t)cost_e, C = (int32_t)(cost_o + cost_e * max_edits);
    const int64_t plane = (int64_t)(C + 1) * W;
    int32_t* FM = fslab + (uint64_t)blockIdx.x * 3u * (uint64_t)plane;
    int32_t* FI = FM + plane;
    int32_t* FD = FI + plane;
    // the diagonals of score sp: |k| <= kmax; a cell of the slab may be read iff it was written
    auto kmax_of = [&](int32_t sp) -> int32_t {
        if (sp < O) return 0;
        const int32_t v = (sp - (int32_t)cost_o) / G;
        return v < E ? v : E;
    };
    auto held = [&](int32_t sp, int32_t k) -> bool {
        if (sp < 0 || sp > C || !alive[sp]) return false;
        const int32_t km = kmax_of(sp);
        return k >= -km && k <= km;
    };
    const uint64_t nl = ctr_in[3];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint32_t g = list[li];
        const AlnRow r = rows[g];
        const Seqs sq = seqs_of(r.rec, (r.flags & kRev) != 0u, offsets, uoff, units, tpl, n);
        const int64_t a = r.a, b = r.b;
        const int64_t qa = (int64_t)r.tq - a, pb = (int64_t)r.tp - b;
        bool bad = false;
        for (int64_t w = lane; w * 64 < a; w += 64) {
            const Win q = strand_window(sq.Q, sq.qn, sq.len, sq.rev, qa + 64 * w);
            if (q.bad & low_mask(a - 64 * w)) bad = true;
        }
        for (int64_t w = lane; w * 64 < b; w += 64) {
            const Win t = window(sq.T, sq.tn, sq.n, pb + 64 * w);
            if (t.bad & low_mask(b - 64 * w)) bad = true;
        }
        // (nobody reads the last gap's LDS or slab any more: every lane stores the same alive[] and rbuf[] words, and reads them
        // behind a barrier)
        if (__syncthreads_or(bad ? 1 : 0)) continue;
        const int32_t kfin = (int32_t)(b - a);
        int32_t s = 0;
        bool closed = false;
        for (;; s++) {
            const int32_t sx = s - X, so = s - O, sg = s - G;
            const bool sources = s == 0 || (sx >= 0 && alive[sx]) || (so >= 0 && alive[so]) || (sg >= 0 && alive[sg]);
            if (!sources) {  // (uniform: alive[] is the same for every lane)
                alive[s] = 0;
                if (s == C) break;
                continue;
            }
            const int32_t km = kmax_of(s);
            bool fin = false, live = false;
            for (int32_t d = E - km + (int32_t)lane; d <= E + km; d += 64) {
                const int32_t k = d - E;
                int64_t ci = kNeg, cd = kNeg, c = kNeg;
                if (s == 0) {
                    c = 0;
                } else {
                    {  // a strand letter: from diagonal k + 1, x + 1; it opens a gap behind M or goes on in I
                        int64_t src = held(so, k + 1) ? FM[(int64_t)so * W + d + 1] : kNeg;
                        const int64_t go = held(sg, k + 1) ? FI[(int64_t)sg * W + d + 1] : kNeg;
                        if (go > src) src = go;
                        if (src >= 0) {
                            const int64_t v = src + 1 < a ? src + 1 : a, least = -k - 1 > 0 ? -k - 1 : 0;
                            if (v - 1 >= least) ci = v;
                        }
                    }
                    {  // a text letter: from diagonal k - 1, x stays
                        int64_t src = held(so, k - 1) ? FM[(int64_t)so * W + d - 1] : kNeg;
                        const int64_t go = held(sg, k - 1) ? FD[(int64_t)sg * W + d - 1] : kNeg;
                        if (go > src) src = go;
                        if (src >= 0) {
                            const int64_t v = src < b - k ? src : b - k, least = 1 - k > 0 ? 1 - k : 0;
                            if (v >= least) cd = v;
                        }
                    }
                    const int64_t fk = held(sx, k) ? FM[(int64_t)sx * W + d] : kNeg;
                    if (fk >= 0) {  // one more letter of both, or none at an end
                        c = fk + 1;
                        if (c > a) c = a;
                        if (c > b - k) c = b - k;
                    }
                    if (ci > c) c = ci;
                    if (cd > c) c = cd;
                }
                if (c >= 0) {
                    const int64_t lim = a - c < b - (c + k) ? a - c : b - (c + k);
                    if (lim > 0) c += slide_fwd(sq, qa, pb, c, c + k, lim);
                }
                FM[(int64_t)s * W + d] = (int32_t)c;
                FI[(int64_t)s * W + d] = (int32_t)ci;
                FD[(int64_t)s * W + d] = (int32_t)cd;
                if (c >= 0 || ci >= 0 || cd >= 0) live = true;
                if (k == kfin && c >= a) fin = true;
            }
            const bool any_live = __ballot(live) != 0ull, any_fin = __ballot(fin) != 0ull;
            alive[s] = any_live ? 1 : 0;
            __syncthreads();  // the score's cells are in the slab (and alive[s] in LDS) for every lane
            if (any_fin) { closed = true; break; }
            if (s == C) break;
        }
        if (!closed) continue;
        // The traceback of 4.29 from the stored points, uniform in the wave as k_aln_wave's: in state H the diagonal step on equal
        // letters (a slide backwards), X iff M[s - x][k] >= x - 1, else state D iff D[s][k] >= x, else state I; in state D a text
        // letter, and back to H iff M[s - o - e][k - 1] >= x, else s - e; state I the same with k + 1 and x - 1.
        bool overrun = false;
        int64_t x = a, y = b;
        int32_t sc = s;
        uint32_t state = 0, nr = 0, code = 0, len = 0, ned = 0;
        while (x > 0 || y > 0) {
            uint32_t op;
            const int32_t k = (int32_t)(y - x);
            if (state == 0u) {
                if (x > 0 && y > 0) {
                    const int64_t run = slide_back(sq, qa, pb, x, y, x < y ? x : y);
                    if (run) {
                        if (code != kOpEq) { if (len) rbuf[nr++] = (len << 4) | code; code = kOpEq; len = 0; }
                        len += (uint32_t)run;
                        x -= run;
                        y -= run;
                        if (nr >= kAffineRuns - 1u) { overrun = true; break; }
                        continue;
                    }
                }
                const int32_t m_same = held(sc - X, k) ? FM[(int64_t)(sc - X) * W + k + E] : kNeg;
                if (x > 0 && y > 0 && m_same >= 0 && (int64_t)m_same >= x - 1) { op = kOpX; x--; y--; sc -= X; }
                else {
                    const int32_t d_here = held(sc, k) ? FD[(int64_t)sc * W + k + E] : kNeg;
                    state = (y > 0 && (x == 0 || (d_here >= 0 && (int64_t)d_here >= x))) ? 1u : 2u;
                    continue;
                }
            } else if (state == 1u) {
                const int32_t m_open = held(sc - O, k - 1) ? FM[(int64_t)(sc - O) * W + k - 1 + E] : kNeg;
                op = kOpD;
                if (m_open >= 0 && (int64_t)m_open >= x) { sc -= O; state = 0u; } else { sc -= G; }
                y--;
            } else {
                const int32_t m_open = held(sc - O, k + 1) ? FM[(int64_t)(sc - O) * W + k + 1 + E] : kNeg;
                op = kOpI;
                if (m_open >= 0 && (int64_t)m_open >= x - 1) { sc -= O; state = 0u; } else { sc -= G; }
                x--;
            }
            ned++;
            if (code != op) { if (len) rbuf[nr++] = (len << 4) | code; code = op; len = 0; }
            len++;
            if (nr >= kAffineRuns - 1u || sc < 0 || x < 0 || y < 0) { overrun = true; break; }  // (never, by the count of runs; if it were, the gap is left broken)
        }
        if (overrun) continue;  // (uniform)
        if (len) rbuf[nr++] = (len << 4) | code;
        if (lane == 0u) s_off = atomicAdd(&ctr[4], (unsigned long long)nr);
        __syncthreads();
        const uint64_t at = s_off;
        if (at + nr <= slab_cap)
            for (uint32_t t = lane; t < nr; t += 64u) slab[at + t] = rbuf[nr - 1u - t];
        if (lane == 0u) {
            AlnRow* o = rows + g;
            o->gapn = nr;
            o->gapd = ned;
            o->slab = (uint32_t)(at < 0xFFFFFFFFull ? at : 0xFFFFFFFFull);
            o->flags = r.flags | kClosed | ((nr && (rbuf[0] & 15u) == kOpEq) ? kGapEq : 0u);
        }
        __syncthreads();  // rbuf[] and s_off are read before the next gap's traceback stores to them
    }
}

// ---- a wave per listed outer end (-gext) ------------------------------------------------------------------------

// Runs of an end: every run but those of `=` costs at least min(x', o' + e') >= 3 of the penalty p <= Cp, and two runs of `=` have
// one of the others between them.
constexpr uint32_t kEndRuns = 2 * (kAlnMaxCost / 3) + 1;

// The gapped X-drop attempt of one end on the penalty p with 2S = x + y - p (x' = 2P + 2, o' = 2o, e' = 2e + 1): 4.29's three
// components per score on the diagonals |k| <= Z (a lane each, 2Z + 1 <= 63), in the coordinates of the end -- x letters of the
// strand and y of the text away from the anchor, to the right, or to the left on the mirrored windows.  A cell whose start lies
// more than 2X under best2 is dead; best2 and the best cell are wave-uniform, and so are the pruning's inputs, alive[], the end
// of the attempt and the traceback.
__global__ void __launch_bounds__(64) k_aln_wave_ends(const uint32_t* __restrict__ ends, const unsigned long long* __restrict__ ctr_in,
                                                      AlnRow* rows, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ uoff,
                                                      const QueryUnit* __restrict__ units, const TextPlanes* __restrict__ tpl, uint32_t n,
                                                      uint32_t band, uint32_t penalty, uint32_t xdrop, uint32_t cost_o, uint32_t cost_e,
                                                      int32_t* fslab, uint32_t* __restrict__ slab, uint64_t slab_cap,
                                                      unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t rbuf[kEndRuns];          // the traceback's runs, the farthest from the anchor first
    __shared__ uint8_t alive[kAlnMaxCost + 1];   // per score: some cell is live (and the slab holds the score)
    __shared__ unsigned long long s_off;
    const uint32_t lane = threadIdx.x;
    const int32_t Z = (int32_t)band, W = 2 * Z + 1, C = (int32_t)kAlnMaxCost;
    const int32_t X = 2 * (int32_t)penalty + 2, G = 2 * (int32_t)cost_e + 1, o2 = 2 * (int32_t)cost_o, O = o2 + G;
    const int32_t back = X > O ? X : O;
    const int64_t drop2 = 2 * (int64_t)xdrop, kBias = 1ll << 34;
    const int64_t plane = (int64_t)(C + 1) * W;
    int32_t* FM = fslab + (uint64_t)blockIdx.x * 3u * (uint64_t)plane;
    int32_t* FI = FM + plane;
    int32_t* FD = FI + plane;
    auto kmax_of = [&](int32_t sp) -> int32_t {
        if (sp < O) return 0;
        const int32_t v = (sp - o2) / G;
        return v < Z ? v : Z;
    };
    auto held = [&](int32_t sp, int32_t k) -> bool {
        if (sp < 0 || sp > C || !alive[sp]) return false;
        const int32_t km = kmax_of(sp);
        return k >= -km && k <= km;
    };
    const uint64_t nl = ctr_in[5];
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint32_t en = ends[li], g = en >> 1;
        const bool right = (en & 1u) != 0u;
        const AlnRow r = rows[g];
        const Seqs sq = seqs_of(r.rec, (r.flags & kRev) != 0u, offsets, uoff, units, tpl, n);
        const int64_t q0 = (int64_t)r.tq + (right ? (int64_t)r.tl : 0), p0 = (int64_t)r.tp + (right ? (int64_t)r.tl : 0);
        // the pieces: letters up to the first that is not A,C,G,T or lies outside (window() calls those bad), 4,096 per trip
        auto piece_len = [&](bool text, int64_t limit) -> int64_t {
            for (int64_t w0 = 0;; w0 += 64) {
                const int64_t w = w0 + lane;
                Win v;
                if (text) v = right ? window(sq.T, sq.tn, sq.n, p0 + 64 * w) : mirrored(window(sq.T, sq.tn, sq.n, p0 - 64 - 64 * w));
                else v = right ? strand_window(sq.Q, sq.qn, sq.len, sq.rev, q0 + 64 * w)
                               : mirrored(strand_window(sq.Q, sq.qn, sq.len, sq.rev, q0 - 64 - 64 * w));
                const uint64_t hit = __ballot(v.bad != 0ull);
                if (hit) {
                    const int first = (int)__builtin_ctzll(hit);
                    const int64_t mine = 64 * w + (v.bad ? (int64_t)__builtin_ctzll(v.bad) : 0);
                    const int64_t len = __shfl(mine, first);
                    return len < limit ? len : limit;
                }
                if (64 * (w0 + 64) >= limit) return limit;
            }
        };
        const int64_t a = piece_len(false, (int64_t)1 << 40);
        const int64_t b = piece_len(true, a + Z);
        auto slide_out = [&](int64_t x, int64_t y, int64_t lim) -> int64_t {  // matching letters from (x, y) on, away from the anchor
            return right ? slide_fwd(sq, q0, p0, x, y, lim) : slide_back(sq, q0, p0, -x, -y, lim);
        };
        auto slide_in = [&](int64_t x, int64_t y, int64_t lim) -> int64_t {   // ... in front of (x, y), towards the anchor
            return right ? slide_back(sq, q0, p0, x, y, lim) : slide_fwd(sq, q0, p0, -x, -y, lim);
        };
        __syncthreads();  // (nobody reads the last end's LDS any more)
        int64_t best2 = 0, bx = 0;
        int32_t bs = 0, bk = 0, last_live = 0;
        for (int32_t s = 0; s <= C; s++) {
            if (s - last_live > back) break;  // (uniform)
            const int32_t sx = s - X, so = s - O, sg = s - G;
            const bool sources = s == 0 || (sx >= 0 && alive[sx]) || (so >= 0 && alive[so]) || (sg >= 0 && alive[sg]);
            if (!sources) { alive[s] = 0; continue; }
            const int32_t km = kmax_of(s), d = Z - km + (int32_t)lane, k = d - Z;
            long long key = -1;
            if (d <= Z + km) {
                int64_t ci = kNeg, cd = kNeg, c = kNeg;
                if (s == 0) {
                    c = 0;
                } else {
                    {  // a strand letter: from diagonal k + 1, x + 1
                        int64_t src = held(so, k + 1) ? FM[(int64_t)so * W + d + 1] : kNeg;
                        const int64_t go = held(sg, k + 1) ? FI[(int64_t)sg * W + d + 1] : kNeg;
                        if (go > src) src = go;
                        if (src >= 0) {
                            const int64_t v = src + 1 < a ? src + 1 : a, least = -k - 1 > 0 ? -k - 1 : 0;
                            if (v - 1 >= least) ci = v;
                        }
                    }
                    {  // a text letter: from diagonal k - 1, x stays
                        int64_t src = held(so, k - 1) ? FM[(int64_t)so * W + d - 1] : kNeg;
                        const int64_t go = held(sg, k - 1) ? FD[(int64_t)sg * W + d - 1] : kNeg;
                        if (go > src) src = go;
                        if (src >= 0) {
                            const int64_t v = src < b - k ? src : b - k, least = 1 - k > 0 ? 1 - k : 0;
                            if (v >= least) cd = v;
                        }
                    }
                    const int64_t fk = held(sx, k) ? FM[(int64_t)sx * W + d] : kNeg;
                    if (fk >= 0) {
                        c = fk + 1;
                        if (c > a) c = a;
                        if (c > b - k) c = b - k;
                    }
                    if (ci > c) c = ci;
                    if (cd > c) c = cd;
                }
                if (c >= 0 && best2 - (2 * c + k - s) > drop2) c = ci = cd = kNeg;  // dead
                if (c >= 0) {
                    const int64_t lim = a - c < b - (c + k) ? a - c : b - (c + k);
                    if (lim > 0) c += slide_out(c, c + k, lim);
                    const int32_t rank = k < 0 ? -2 * k - 1 : 2 * k;  // k = 0, -1, +1, -2, ..
                    key = ((long long)(2 * c + k - s + kBias) << 7) | (long long)(127 - rank);
                }
                FM[(int64_t)s * W + d] = (int32_t)c;
                FI[(int64_t)s * W + d] = (int32_t)ci;
                FD[(int64_t)s * W + d] = (int32_t)cd;
            }
            for (int m = 32; m; m >>= 1) {
                const long long other = __shfl_xor(key, m);
                if (other > key) key = other;
            }
            alive[s] = key >= 0 ? 1 : 0;
            __syncthreads();  // the score's cells are in the slab (and alive[s] in LDS) for every lane
            if (key >= 0) {
                last_live = s;
                const int64_t val = (int64_t)(key >> 7) - kBias;
                const int32_t rank = 127 - (int32_t)(key & 127), kb = (rank & 1) ? -(rank + 1) / 2 : rank / 2;
                if (val > best2) { best2 = val; bs = s; bk = kb; bx = (val - kb + s) / 2; }
            }
        }
        if (best2 <= 2 * (int64_t)(right ? r.scr : r.scl)) continue;  // (uniform) 4.13's side stays, a tie included
        // 4.29's traceback from the stored points, started at the best cell
        bool overrun = false;
        int64_t x = bx, y = bx + bk;
        int32_t sc = bs;
        uint32_t state = 0, nr = 0, code = 0, len = 0, ned = 0;
        while (x > 0 || y > 0) {
            uint32_t op;
            const int32_t k = (int32_t)(y - x);
            if (state == 0u) {
                if (x > 0 && y > 0) {
                    const int64_t run = slide_in(x, y, x < y ? x : y);
                    if (run) {
                        if (code != kOpEq) { if (len) rbuf[nr++] = (len << 4) | code; code = kOpEq; len = 0; }
                        len += (uint32_t)run;
                        x -= run;
                        y -= run;
                        if (nr >= kEndRuns - 1u) { overrun = true; break; }
                        continue;
                    }
                }
                const int32_t m_same = held(sc - X, k) ? FM[(int64_t)(sc - X) * W + k + Z] : kNeg;
                if (x > 0 && y > 0 && m_same >= 0 && (int64_t)m_same >= x - 1) { op = kOpX; x--; y--; sc -= X; }
                else {
                    const int32_t d_here = held(sc, k) ? FD[(int64_t)sc * W + k + Z] : kNeg;
                    state = (y > 0 && (x == 0 || (d_here >= 0 && (int64_t)d_here >= x))) ? 1u : 2u;
                    continue;
                }
            } else if (state == 1u) {
                const int32_t m_open = held(sc - O, k - 1) ? FM[(int64_t)(sc - O) * W + k - 1 + Z] : kNeg;
                op = kOpD;
                if (m_open >= 0 && (int64_t)m_open >= x) { sc -= O; state = 0u; } else { sc -= G; }
                y--;
            } else {
                const int32_t m_open = held(sc - O, k + 1) ? FM[(int64_t)(sc - O) * W + k + 1 + Z] : kNeg;
                op = kOpI;
                if (m_open >= 0 && (int64_t)m_open >= x - 1) { sc -= O; state = 0u; } else { sc -= G; }
                x--;
            }
            ned++;
            if (code != op) { if (len) rbuf[nr++] = (len << 4) | code; code = op; len = 0; }
            len++;
            if (nr >= kEndRuns - 1u || sc < 0 || x < 0 || y < 0) { overrun = true; break; }  // (never, by the count of runs)
        }
        // (the anchor is a MEM, so the letters next to it differ and the run next to it is never `=`; k_aln_count relies on it)
        if (overrun || code == kOpEq || !len) continue;  // (uniform)
        rbuf[nr++] = (len << 4) | code;
        if (lane == 0u) s_off = atomicAdd(&ctr[4], (unsigned long long)nr);
        __syncthreads();
        const uint64_t at = s_off;
        if (at + nr <= slab_cap)
            for (uint32_t t = lane; t < nr; t += 64u) slab[at + t] = rbuf[right ? nr - 1u - t : t];  // left to right in the strand
        if (lane == 0u) {
            AlnRow* o = rows + g;
            const uint32_t where = (uint32_t)(at < 0xFFFFFFFFull ? at : 0xFFFFFFFFull);
            if (right) { o->extr = (uint32_t)bx; o->extr_t = (uint32_t)(bx + bk); o->nfr = nr; o->edr = ned; o->slr = where; o->repr = 1u; }
            else { o->extl = (uint32_t)bx; o->extl_t = (uint32_t)(bx + bk); o->nfl = nr; o->edl = ned; o->sll = where; o->repl = 1u; }
            atomicAdd(&ctr[6], 1ull);
        }
    }
}

// ---- places ------------------------------------------------------------------------------------------------------------------

// a row's anchor goes into the run of the row to its left when its gap is closed and empty
__device__ __forceinline__ bool joins_left(const AlnRow& r) { return (r.flags & kClosed) && r.gapn == 0u; }

__global__ void __launch_bounds__(256) k_aln_count(const uint64_t* __restrict__ coff, uint64_t nb, uint64_t cap,
                                                   const AlnRow* __restrict__ rows, uint32_t* __restrict__ nruns, uint32_t* __restrict__ flag,
                                                   uint32_t* __restrict__ ed) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g > cap + 1u) return;
    uint64_t K = coff[nb];
    if (K > cap) K = cap;
    if (g >= K) { nruns[g] = 0u; flag[g] = 0u; ed[g] = 0u; return; }
    const AlnRow r = rows[g];
    const bool closed = (r.flags & kClosed) != 0u;
    const bool own_anchor = !(closed && (r.gapn == 0u || (r.flags & kGapEq)));
    nruns[g] = r.nfl + r.nfr + (closed ? r.gapn : 0u) + (own_anchor ? 1u : 0u);
    ed[g] = r.edl + r.edr + (closed ? r.gapd : 0u);
    // the gap to the right of row g is row g - 1's
    flag[g] = ((r.flags & kFirst) || !(rows[g - 1u].flags & kClosed)) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_aln_segs(const uint64_t* __restrict__ coff, uint64_t nb, uint64_t cap,
                                                  const uint32_t* __restrict__ flag, const uint64_t* __restrict__ sflag,
                                                  const uint64_t* __restrict__ sn, uint32_t* __restrict__ segstart,
                                                  uint64_t* __restrict__ out_boff, uint64_t* __restrict__ op_off, uint64_t seg_cap) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint64_t K = coff[nb];
    if (K > cap) K = cap;
    if (i <= nb) {
        const uint64_t c = coff[i] < K ? coff[i] : K;
        out_boff[i] = sflag[c];
    }
    if (i < K && flag[i]) segstart[sflag[i]] = (uint32_t)i;
    if (i == K) {
        const uint64_t nseg = sflag[K];
        segstart[nseg] = (uint32_t)K;
        if (nseg <= seg_cap) op_off[nseg] = sn[K];
    }
}

__global__ void __launch_bounds__(256) k_aln_write(const uint64_t* __restrict__ coff, uint64_t nb, uint64_t cap,
                                                   const AlnRow* __restrict__ rows, const uint64_t* __restrict__ offsets,
                                                   const uint64_t* __restrict__ uoff, const QueryUnit* __restrict__ units,
                                                   const TextPlanes* __restrict__ tpl, uint32_t n, const uint64_t* __restrict__ sflag,
                                                   const uint64_t* __restrict__ sn, const uint64_t* __restrict__ sed,
                                                   const uint32_t* __restrict__ segstart, const uint32_t* __restrict__ slab,
                                                   uint64_t slab_cap, slamem_aln* __restrict__ segs, uint64_t seg_cap,
                                                   uint32_t* __restrict__ ops, uint64_t ops_cap, uint64_t* __restrict__ op_off) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint64_t K = coff[nb];
    if (K > cap) K = cap;
    if (g >= K) return;
    const AlnRow r = rows[g];
    const uint64_t sg = sflag[g + 1u] - 1u;
    const uint64_t g0 = segstart[sg], g1p = segstart[sg + 1u];
    const Seqs sq = seqs_of(r.rec, (r.flags & kRev) != 0u, offsets, uoff, units, tpl, n);
    Emit em = {ops, sn[g0] + (sn[g1p] - sn[g + 1u]), ops_cap, 0, 0, 0, true};
    if (!(joins_left(r) && g + 1u < g1p)) {
        if ((r.flags & kLast) && r.repl) slab_runs(slab, slab_cap, r.sll, r.nfl, em);
        else if ((r.flags & kLast) && r.extl) diag_runs(sq, (int64_t)r.tq - r.extl, (int64_t)r.tp - r.extl, r.extl, em);
        if ((r.flags & kClosed) && r.gapn) {
            if (r.flags & kListed) {
                slab_runs(slab, slab_cap, r.slab, r.gapn, em);
            } else {
                diag_runs(sq, (int64_t)r.tq - r.a, (int64_t)r.tp - r.b, r.a, em);
            }
        }
        uint32_t len = r.tl;
        for (uint64_t k = g; k > g0;) {  // anchors to the right that join this run (their gap is closed and empty)
            k--;
            const AlnRow rk = rows[k];
            if (!joins_left(rk)) break;
            len += rk.tl;
        }
        em.push(kOpEq, len);
    }
    if ((r.flags & kFirst) && r.repr) slab_runs(slab, slab_cap, r.slr, r.nfr, em);
    else if ((r.flags & kFirst) && r.extr) diag_runs(sq, (int64_t)r.tq + r.tl, (int64_t)r.tp + r.tl, r.extr, em);
    em.flush();
    if (g == g0 && sg < seg_cap) {
        const AlnRow rl = rows[g1p - 1u];
        slamem_aln o;
        o.ref_pos = rl.tp - rl.extl_t;
        o.query_pos = rl.tq - rl.extl;
        o.ref_len = r.tp + r.tl + r.extr_t - o.ref_pos;
        o.query_len = r.tq + r.tl + r.extr - o.query_pos;
        o.edits = (uint32_t)(sed[g1p] - sed[g0]);
        segs[sg] = o;
        op_off[sg] = sn[g0];
    }
}

}  // namespace

uint64_t aln_workspace_bytes(const FilterBatch& b, const FilterParams& p) { return aln_layout(b, p).bytes; }
uint64_t aln_counters_offset(const FilterBatch& b, const FilterParams& p) { return aln_layout(b, p).off_ctr; }

#define ASTEP(call, what) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(e__, what, __FILE__, __LINE__); } while (0)

void aln_chain_buffers(void* ws, const FilterBatch& b, const FilterParams& args, slamem_mem** crows_out, uint64_t** coff_out) {
    const AlnLayout m = aln_layout(b, args);
    char* p = static_cast<char*>(ws);
    *crows_out = reinterpret_cast<slamem_mem*>(p + m.off_crows);
    *coff_out = reinterpret_cast<uint64_t*>(p + m.off_coff);
}

int aln_filter(void* ws, const FilterBatch& b, const FilterParams& args, slamem_mem*, uint64_t* out_boff, unsigned long long* host_scalars,
               hipStream_t stream) {
    slamem_mem* crows;
    uint64_t* coff;
    aln_chain_buffers(ws, b, args, &crows, &coff);
    // the chains: [0] rows kept (replaced below), [1] the highest-numbered block out of order + 1
    int rc = chain_pass(ws, b.num_blocks(), b.capacity, args.max_gap, nullptr, stream);
    if (rc == SLAMEM_OK) rc = chain_compact(ws, b.num_blocks(), b.capacity, crows, coff, host_scalars, stream);
    if (rc != SLAMEM_OK) return rc;
    return aln_after_chain(ws, b, args, out_boff, host_scalars, stream);
}

int aln_after_chain(void* ws, const FilterBatch& b, const FilterParams& args, uint64_t* out_boff, unsigned long long* host_scalars,
                    hipStream_t stream) {
    const IndexView& ix = *b.ix;
    const uint64_t* offsets_dev = b.offsets_dev;
    const uint64_t num_queries = b.num_queries, num_blocks = b.num_blocks(), capacity = b.capacity;
    const uint32_t strands = b.strands;
    const AlnLayout m = aln_layout(b, args);
    const AlnCosts costs = aln_costs(args.max_edits);
    char* p = static_cast<char*>(ws);
    unsigned long long* ctr = reinterpret_cast<unsigned long long*>(p + m.off_ctr);
    slamem_mem* crows = reinterpret_cast<slamem_mem*>(p + m.off_crows);
    uint64_t* coff = reinterpret_cast<uint64_t*>(p + m.off_coff);
    uint32_t* ucnt = reinterpret_cast<uint32_t*>(p + m.off_ucnt);
    uint64_t* uoff = reinterpret_cast<uint64_t*>(p + m.off_uoff);
    uint64_t* longs = reinterpret_cast<uint64_t*>(p + m.off_long);
    QueryUnit* units = reinterpret_cast<QueryUnit*>(p + m.off_units);
    AlnRow* rows = reinterpret_cast<AlnRow*>(p + m.off_rows);
    uint32_t* list = reinterpret_cast<uint32_t*>(p + m.off_list);
    uint32_t* ends = reinterpret_cast<uint32_t*>(p + m.off_ends);
    uint32_t* nruns = reinterpret_cast<uint32_t*>(p + m.off_n);
    uint32_t* flag = reinterpret_cast<uint32_t*>(p + m.off_flag);
    uint32_t* ed = reinterpret_cast<uint32_t*>(p + m.off_ed);
    uint64_t* sn = reinterpret_cast<uint64_t*>(p + m.off_sn);
    uint64_t* sflag = reinterpret_cast<uint64_t*>(p + m.off_sflag);
    uint64_t* sed = reinterpret_cast<uint64_t*>(p + m.off_sed);
    uint32_t* segstart = reinterpret_cast<uint32_t*>(p + m.off_segstart);
    uint32_t* slab = reinterpret_cast<uint32_t*>(p + m.off_slab);
    int32_t* fslab = reinterpret_cast<int32_t*>(p + m.off_f);
    const char* queries = static_cast<const char*>(b.queries_dev);
    ASTEP(hipMemsetAsync(ctr, 0, 64, stream), "memset");
    ASTEP(pack_batch_planes(queries, offsets_dev, num_queries, ucnt, uoff, p + m.off_uscan, m.uscan_bytes, longs, units, ctr, stream),
          "pack_batch_planes");
    if (num_blocks) {
        hipLaunchKernelGGL(k_aln_geom, dim3(grid_for(capacity)), dim3(256), 0, stream, (const uint64_t*)coff, num_blocks,
                           (const slamem_mem*)crows, capacity, offsets_dev, (const uint64_t*)uoff, (const QueryUnit*)units, ix.tpl, ix.n,
                           strands, args.penalty, args.xdrop, costs.E, costs.x, 2u * (costs.o + costs.e) / costs.x, costs.C,
                           args.end_band, costs.o + costs.e, rows, list, ends, ctr);
        ASTEP(hipGetLastError(), "k_aln_geom");
        if (costs.affine) {
            hipLaunchKernelGGL(k_aln_wave_affine, dim3(aln_affine_grid(costs)), dim3(64), 0, stream, (const uint32_t*)list,
                               (const unsigned long long*)ctr, rows, offsets_dev, (const uint64_t*)uoff, (const QueryUnit*)units, ix.tpl, ix.n,
                               costs.E, costs.x, costs.o, costs.e, fslab, slab, args.ops_capacity, ctr);
            ASTEP(hipGetLastError(), "k_aln_wave_affine");
            if (args.end_band) {
                hipLaunchKernelGGL(k_aln_wave_ends, dim3(aln_end_grid(args.end_band)), dim3(64), 0, stream, (const uint32_t*)ends,
                                   (const unsigned long long*)ctr, rows, offsets_dev, (const uint64_t*)uoff, (const QueryUnit*)units, ix.tpl,
                                   ix.n, args.end_band, args.penalty, args.xdrop, costs.o, costs.e, fslab, slab, args.ops_capacity, ctr);
                ASTEP(hipGetLastError(), "k_aln_wave_ends");
            }
        } else {
            hipLaunchKernelGGL(k_aln_wave, dim3(aln_wave_grid(costs.E)), dim3(64), 0, stream, (const uint32_t*)list, (const unsigned long long*)ctr, rows,
                               offsets_dev, (const uint64_t*)uoff, (const QueryUnit*)units, ix.tpl, ix.n, costs.E, fslab, slab,
                               args.ops_capacity, ctr);
            ASTEP(hipGetLastError(), "k_aln_wave");
        }
    }
    hipLaunchKernelGGL(k_aln_count, dim3(grid_for(capacity + 2)), dim3(256), 0, stream, (const uint64_t*)coff, num_blocks, capacity,
                       (const AlnRow*)rows, nruns, flag, ed);
    ASTEP(hipGetLastError(), "k_aln_count");
    size_t need = m.scan_bytes;
    ASTEP(scan_sum_exclusive_u32_u64(p + m.off_scan, need, nruns, sn, capacity + 1, stream), "scan");
    need = m.scan_bytes;
    ASTEP(scan_sum_exclusive_u32_u64(p + m.off_scan, need, flag, sflag, capacity + 1, stream), "scan");
    need = m.scan_bytes;
    ASTEP(scan_sum_exclusive_u32_u64(p + m.off_scan, need, ed, sed, capacity + 1, stream), "scan");
    const uint64_t most = capacity > num_blocks ? capacity : num_blocks;
    hipLaunchKernelGGL(k_aln_segs, dim3(grid_for(most + 1)), dim3(256), 0, stream, (const uint64_t*)coff, num_blocks, capacity,
                       (const uint32_t*)flag, (const uint64_t*)sflag, (const uint64_t*)sn, segstart, out_boff, args.op_offsets,
                       args.segs_capacity);
    ASTEP(hipGetLastError(), "k_aln_segs");
    hipLaunchKernelGGL(k_aln_write, dim3(grid_for(capacity)), dim3(256), 0, stream, (const uint64_t*)coff, num_blocks, capacity,
                       (const AlnRow*)rows, offsets_dev, (const uint64_t*)uoff, (const QueryUnit*)units, ix.tpl, ix.n,
                       (const uint64_t*)sflag, (const uint64_t*)sn, (const uint64_t*)sed, (const uint32_t*)segstart, (const uint32_t*)slab,
                       args.ops_capacity, args.segs, args.segs_capacity, args.ops, args.ops_capacity, args.op_offsets);
    ASTEP(hipGetLastError(), "k_aln_write");
    // [0] segments, [1] (chain_filter's) the highest-numbered block out of order + 1, [2] operations
    ASTEP(hipMemcpyAsync(host_scalars, sflag + capacity + 1, 8, hipMemcpyDeviceToHost, stream), "memcpy");
    ASTEP(hipMemcpyAsync(host_scalars + 2, sn + capacity + 1, 8, hipMemcpyDeviceToHost, stream), "memcpy");
    return SLAMEM_OK;
}
#undef ASTEP

}  // namespace slamem
