// filters.hip -- the filters behind K9 as the search sees them: one row per match type 2..7, the one place that
// turns the placeholders of the public interface into values, and where K9 places the -mem list in a filter's workspace.
#include "filter_blocks.h"

namespace slamem {

namespace {

constexpr uint64_t kRows32 = 0xFFFFFFFFull, kRowsTiled = 0xFFFF0000ull;  // row places are 32-bit; ... and counted in tiles
const char kAlnLimits[] = "slamem_find_alns_device: at most 2^32 - 2^16 MEMs and operations of capacity and 2^32 - 2 strand blocks per call";

// name, flag, noun, limits, capacity_end, bounds_blocks, needs_planes, column_per_row, segments, needs_reads, scalars,
// workspace_bytes, run, finish
// (-paf shares -aln's bounds and their message; -mum alone finishes on the host's word)
const FilterDesc kFilters[6] = {
    {"slamem_find_mums_device", "-mum", nullptr, "slamem_find_mums_device: at most 2^32 - 2 MEMs of capacity per call", kRows32, false, false,
     false, false, false, 2, mum_workspace_bytes, mum_filter_small, mum_filter_large},
    {"slamem_find_smems_device", "-smem", "SMEMs", "slamem_find_smems_device: at most 2^32 - 2^16 MEMs of capacity per call", kRowsTiled, false,
     false, false, false, false, 2, smem_workspace_bytes, smem_filter, nullptr},
    {"slamem_find_chains_device", "-chain", "chains", "slamem_find_chains_device: at most 2^32 - 2^16 MEMs of capacity per call", kRowsTiled,
     false, false, false, false, false, 2, chain_workspace_bytes, chain_filter, nullptr},
    {"slamem_find_exts_device", "-ext", "extended MEMs",
     "slamem_find_exts_device: at most 2^32 - 2^16 MEMs of capacity and 2^32 - 2 strand blocks per call", kRowsTiled, true, true, true, false,
     false, 2, ext_workspace_bytes, ext_filter, nullptr},
    {"slamem_find_alns_device", "-aln", "alignments", kAlnLimits, kRowsTiled, true, true, false, true, false, 3,
     aln_workspace_bytes, aln_filter, nullptr},
    {"slamem_find_maps_device", "-paf", "alignments", kAlnLimits, kRowsTiled, true, true, false, true, true, 3,
     map_workspace_bytes, map_filter, nullptr},
};

}  // namespace

const FilterDesc* filter_for(int match_type) { return match_type >= 2 && match_type <= 7 ? &kFilters[match_type - 2] : nullptr; }

int resolve_filter_params(const char* who, uint32_t max_occ, uint32_t max_gap, uint32_t penalty, uint32_t xdrop, uint32_t max_edits,
                          FilterParams* out) {
    if (max_gap >= 0x80000000u) {
        set_error("%s: the maximum gap must be below 2^31 (0: the default, %u)", who, kChainDefaultGap);
        return SLAMEM_ERR_ARG;
    }
    AlnCosts c;
    if (int bad = decode_aln_word(who, max_edits, &c)) return bad;
    *out = FilterParams{max_occ, max_gap ? max_gap : kChainDefaultGap, penalty ? penalty : kExtDefaultPenalty,
                        xdrop == kExtXdropUnset ? kExtDefaultXdrop : xdrop, c.word(), nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr};
    return SLAMEM_OK;
}

int set_end_band(const char* who, uint32_t end_band, FilterParams* p) {
    if (end_band > kAlnMaxEndBand) {
        set_error("%s: the end band is %u, above %u", who, end_band, kAlnMaxEndBand);
        return SLAMEM_ERR_ARG;
    }
    if (end_band && !(p->max_edits >> 8)) {
        set_error("%s: an end band needs gap-affine costs in the max_edits word (SLAMEM_ALN_AFFINE)", who);
        return SLAMEM_ERR_ARG;
    }
    p->end_band = end_band;
    return SLAMEM_OK;
}

int decode_aln_word(const char* who, uint32_t word, AlnCosts* out) {
    int affine = 0;
    const int bad = slamem_decode_aln_word(word, &out->E, &out->x, &out->o, &out->e, &affine);
    out->affine = affine != 0;
    out->C = out->o + out->e * out->E;
    switch (bad) {
    case 0: return SLAMEM_OK;
    case 1: set_error("%s: at most %u edits a gap (SLAMEM_ALN_EDITS_DEFAULT: the default, %u)", who, kAlnMaxEdits, kAlnDefaultEdits); break;
    case 2: set_error("%s: the cost of a mismatch is %u, outside 1 to 31 (SLAMEM_ALN_AFFINE)", who, out->x); break;
    case 3: set_error("%s: the cost of a gap opened is %u, above 63 (SLAMEM_ALN_AFFINE)", who, out->o); break;
    case 4: set_error("%s: the cost of a gap letter is %u, outside 1 to 31 (SLAMEM_ALN_AFFINE)", who, out->e); break;
    default: set_error("%s: the bound on a gap's cost, o + e E = %u + %u * %u, is above %u", who, out->o, out->e, out->E, kAlnMaxCost); break;
    }
    return SLAMEM_ERR_ARG;
}

void filter_list_buffers(void* ws, uint64_t num_blocks, uint64_t capacity, slamem_mem** rows_out, uint64_t** boff_out) {
    FilterPrefix m;
    (void)m.begin(num_blocks, capacity);
    *rows_out = reinterpret_cast<slamem_mem*>(static_cast<char*>(ws) + m.off_rows);
    *boff_out = reinterpret_cast<uint64_t*>(static_cast<char*>(ws) + m.off_boff);
}

uint64_t search_workspace_bytes(uint64_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity, int match_type,
                                const FilterParams& params) {
    const uint64_t mem = find_mems_workspace_bytes(num_queries, both_strands, query_bytes, mems_capacity);
    const FilterDesc* f = filter_for(match_type);
    const FilterBatch b = {nullptr, nullptr, nullptr, num_queries, both_strands ? 2u : 1u, query_bytes, mems_capacity};
    return f ? mem + f->workspace_bytes(b, params) : mem;
}

}  // namespace slamem
