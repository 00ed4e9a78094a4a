"""ctypes binding of libslamem_hip.so -- the C ABI declared in include/slamem_hip.h.

Loading is lazy so that CPU-only tooling (FASTA helpers, the synthetic generator) can import the
package on a machine without the library; every compute entry point goes through :func:`lib`, which
raises if the HIP library is missing.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SLAMEM_HIP_LIB: another build of the same library (tools/variants.sh builds A/B variants of a kernel beside the product's
# library instead of over it; the product path never sets it)
LIB_PATH = os.environ.get("SLAMEM_HIP_LIB") or os.path.join(_HERE, "csrc", "libslamem_hip.so")
SYNTH_PATH = os.path.join(_HERE, "csrc", "libslamem_synth.so")

SLAMEM_OK = 0
SLAMEM_ERR_ARG = 1
SLAMEM_ERR_HIP = 2
SLAMEM_ERR_NOMEM = 3
SLAMEM_ERR_CAPACITY = 4
SLAMEM_ERR_FORMAT = 5
SLAMEM_ERR_IO = 6
SLAMEM_ERR_NO_DEVICE = 7

ARRAY_SA, ARRAY_BWT, ARRAY_LCP, ARRAY_PSV, ARRAY_NSV = range(5)
LAYOUT_AUTO, LAYOUT_FULL, LAYOUT_COMPACT = 0, 1, 2

# every symbol include/slamem_hip.h declares (tests check that the library exports all of them)
ABI_SYMBOLS = (
    "slamem_abi_version", "slamem_strerror", "slamem_last_error_message", "slamem_device_count",
    "slamem_get_timings", "slamem_reset_timings", "slamem_device_warmup", "slamem_device_pci_bus_id",
    "slamem_index_build", "slamem_index_build_device", "slamem_index_build_layout", "slamem_index_build_device_layout",
    "slamem_index_build_bytes", "slamem_device_mem_info", "slamem_index_free", "slamem_index_get_info",
    "slamem_index_arena", "slamem_index_export", "slamem_index_attach", "slamem_index_adopt_arena", "slamem_index_save", "slamem_index_load",
    "slamem_index_validate_header", "slamem_search_stats_enable", "slamem_get_search_stats", "slamem_get_search_clock",
    "slamem_index_download", "slamem_index_sampled_lcp_stats",
    "slamem_follow_letter_batch", "slamem_enclosing_interval_batch", "slamem_position_in_text_batch",
    "slamem_char_at_bwt_pos_batch",
    "slamem_find_mems_workspace_bytes", "slamem_find_mems_device", "slamem_find_mems_host", "slamem_host_free",
    "slamem_find_mams_device", "slamem_find_mams_host",
    "slamem_find_mums_workspace_bytes", "slamem_find_mums_device", "slamem_find_mums_host",
    "slamem_find_smems_workspace_bytes", "slamem_find_smems_device", "slamem_find_smems_host",
    "slamem_find_chains_workspace_bytes", "slamem_find_chains_device", "slamem_find_chains_host",
    "slamem_find_exts_workspace_bytes", "slamem_find_exts_device", "slamem_find_exts_host",
    "slamem_stream_set_ext_params", "slamem_stream_mismatches",
    "slamem_find_alns_workspace_bytes", "slamem_find_alns_device", "slamem_find_alns_host",
    "slamem_stream_set_max_edits", "slamem_stream_alns",
    "slamem_find_alns_workspace_bytes_gext", "slamem_find_alns_device_gext", "slamem_find_alns_host_gext",
    "slamem_find_maps_workspace_bytes_gext", "slamem_find_maps_device_gext", "slamem_find_maps_host_gext",
    "slamem_find_maps_md_host_gext", "slamem_stream_set_end_band", "slamem_find_alns_end_counts_device",
    "slamem_find_maps_workspace_bytes", "slamem_find_maps_device", "slamem_find_maps_host", "slamem_stream_maps",
    "slamem_maps_md_workspace_bytes", "slamem_maps_md_device", "slamem_find_maps_md_host", "slamem_stream_set_md", "slamem_stream_md",
    "slamem_pileup_create", "slamem_pileup_free", "slamem_pileup_reset", "slamem_pileup_add_device",
    "slamem_pileup_counts_device", "slamem_pileup_counts_host", "slamem_stream_set_pileup",
    "slamem_pileup_sites_device", "slamem_pileup_sites_host", "slamem_pileup_add_counts_device", "slamem_pileup_add_counts_host",
    "slamem_pileup_enable_events", "slamem_pileup_events_device", "slamem_pileup_events_host", "slamem_pileup_add_events_device",
    "slamem_pileup_add_events_host", "slamem_pileup_rows_at_device", "slamem_pileup_rows_at_host",
    "slamem_pileup_consensus_device", "slamem_pileup_consensus_host", "slamem_pileup_consensus_gt_device",
    "slamem_pileup_consensus_gt_host", "slamem_pileup_depth_runs_device", "slamem_pileup_depth_runs_host",
    "slamem_stream_create", "slamem_stream_set_max_occ", "slamem_stream_set_max_gap", "slamem_stream_submit", "slamem_stream_submit_packed", "slamem_pack_reads", "slamem_stream_next",
    "slamem_pack_lowq_device", "slamem_pack_lowq", "slamem_pileup_add_masked_device", "slamem_stream_submit_masked",
    "slamem_pileup_enable_dedup", "slamem_pileup_add_dedup_device", "slamem_pileup_dedup_stats", "slamem_stream_set_dedup", "slamem_stream_dups",
    "slamem_gt_costs", "slamem_pileup_genotypes_device", "slamem_pileup_genotypes_host", "slamem_pileup_genotype_events_device",
    "slamem_pileup_genotype_events_host",
    "slamem_pileup_enable_strands", "slamem_pileup_forward", "slamem_fisher_strand", "slamem_fisher_strand_table",
    "slamem_pileup_enable_quals", "slamem_pileup_quality", "slamem_pileup_add_quals_device", "slamem_pileup_genotypes_weighted_device",
    "slamem_pileup_genotypes_weighted_host", "slamem_stream_set_quals", "slamem_stream_submit_quals",
    "slamem_stats_create", "slamem_stats_free", "slamem_stats_reset", "slamem_stats_add_device", "slamem_stats_table_device",
    "slamem_stats_table_host", "slamem_stats_add_table_host", "slamem_stream_set_stats",
    "slamem_pileup_enable_junctions", "slamem_pileup_junctions_device", "slamem_pileup_junctions_host",
    "slamem_pileup_add_junctions_device", "slamem_pileup_add_junctions_host",
    "slamem_stream_destroy",
    "slamem_pinned_alloc", "slamem_pinned_free", "slamem_copy_to_host",
)


class SlamemError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"slamem error {code}: {message}")
        self.code = code


class Mem(C.Structure):
    _fields_ = [("ref_pos", C.c_uint32), ("query_pos", C.c_uint32), ("length", C.c_uint32)]


class IndexInfo(C.Structure):
    _fields_ = [("text_length", C.c_uint32), ("bwt_size", C.c_uint32), ("num_n_rows", C.c_uint32),
                ("dollar_row", C.c_uint32), ("max_lcp", C.c_uint32), ("sort_rounds", C.c_uint32),
                ("arena_bytes", C.c_uint64), ("device", C.c_int32), ("owns_arena", C.c_int32),
                ("filter_k", C.c_uint32), ("layout", C.c_uint32), ("seed_k", C.c_uint32), ("reserved1", C.c_uint32)]


class SslcpStats(C.Structure):
    _fields_ = [("num_samples", C.c_uint64), ("num_oversized_lcp", C.c_uint64), ("sum_lcp", C.c_int64),
                ("max_lcp", C.c_uint32), ("pad", C.c_uint32), ("num_oversized_links", C.c_uint64),
                ("sum_link_distance", C.c_uint64), ("max_link_distance", C.c_uint64)]


class Timings(C.Structure):
    _fields_ = [("build_total_ms", C.c_float), ("build_pack_ms", C.c_float), ("build_sort_ms", C.c_float),
                ("build_bwt_ms", C.c_float), ("build_lcp_ms", C.c_float), ("build_links_ms", C.c_float),
                ("search_kernel_ms", C.c_float), ("search_total_ms", C.c_float),
                ("search_launches", C.c_uint64), ("search_kernel_ms_sum", C.c_double),
                ("prefilter_ms", C.c_float), ("k8_ms", C.c_float), ("prefilter_ms_sum", C.c_double),
                ("k8_ms_sum", C.c_double), ("seed_ms", C.c_float), ("mum_filter_ms", C.c_float), ("seed_ms_sum", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SearchStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in (
        "fm_lines_top", "fm_lines_bottom", "rec_lines_fail", "rec_lines_pend", "rec_lines_flush", "query_loads",
        "lane_trips", "wave_trips", "positions", "enum_jobs", "prefilter_probes", "prefilter_query_loads",
        "prefilter_items", "items", "survivors", "mems", "overflow_records", "valid", "dir_sa_lines", "dir_group_loads",
        "dir_rec_lines", "dir_letters", "jump_lines", "skip_group_loads", "skip_probe_lines", "skip_attempts", "skips",
        "enum_row_steps", "enum_levels", "enum_wave_us")] + [("state_lane_trips", C.c_uint64 * 11),
                                                               ("state_wave_trips", C.c_uint64 * 11)] + [
        (k, C.c_uint64) for k in ("seed_windows", "seed_compares", "seed_letter_masks", "seed_mems", "seed_strands_left",
                                  "seed_reads", "seed_query_bytes")] + [("seed_left_why", C.c_uint64 * 7), ("seed_once_reads", C.c_uint64)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if (k.startswith("state_") or k == "seed_left_why") else int(getattr(self, k))) for k, _ in self._fields_}


_LIB = None
_SYNTH = None


class GtParams(C.Structure):
    """slamem_gt_params (-gt)"""
    _fields_ = [("ploidy", C.c_uint32), ("match_cost", C.c_uint32), ("het_cost", C.c_uint32), ("err_cost", C.c_uint32),
                ("het_prior", C.c_uint32), ("min_depth", C.c_uint32), ("min_qual", C.c_uint32)]


class ConsGtParams(C.Structure):
    """slamem_cons_gt_params (the consensus by genotype likelihood)"""
    _fields_ = [("row", GtParams), ("event", GtParams), ("min_depth", C.c_uint32), ("min_gq", C.c_uint32), ("weighted", C.c_uint32)]


def _declare(L):
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.slamem_abi_version.restype = i32
    L.slamem_strerror.restype = C.c_char_p
    L.slamem_strerror.argtypes = [i32]
    L.slamem_last_error_message.restype = C.c_char_p
    L.slamem_device_count.argtypes = [C.POINTER(i32)]
    L.slamem_device_pci_bus_id.argtypes = [i32, C.c_char_p, i32]
    L.slamem_get_timings.argtypes = [C.POINTER(Timings)]
    L.slamem_index_build.argtypes = [C.c_char_p, u32, i32, C.POINTER(vp)]
    L.slamem_index_build_device.argtypes = [vp, u32, i32, vp, C.POINTER(vp)]
    L.slamem_index_build_layout.argtypes = [C.c_char_p, u32, i32, i32, C.POINTER(vp)]
    L.slamem_index_build_device_layout.argtypes = [vp, u32, i32, vp, i32, C.POINTER(vp)]
    L.slamem_index_build_bytes.argtypes = [u32, i32, C.POINTER(u64), C.POINTER(u64)]
    L.slamem_device_mem_info.argtypes = [i32, C.POINTER(u64), C.POINTER(u64)]
    L.slamem_index_free.argtypes = [vp]
    L.slamem_index_get_info.argtypes = [vp, C.POINTER(IndexInfo)]
    L.slamem_index_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.slamem_index_export.argtypes = [vp, vp, u64, vp]
    L.slamem_index_attach.argtypes = [vp, u64, i32, C.POINTER(vp)]
    L.slamem_index_adopt_arena.argtypes = [vp]
    L.slamem_index_save.argtypes = [vp, C.c_char_p]
    L.slamem_index_load.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.slamem_index_validate_header.argtypes = [vp, u64, u64]
    L.slamem_search_stats_enable.argtypes = [i32]
    L.slamem_get_search_stats.argtypes = [C.POINTER(SearchStats)]
    L.slamem_get_search_clock.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.slamem_index_download.argtypes = [vp, i32, vp, u64]
    L.slamem_index_sampled_lcp_stats.argtypes = [vp, C.POINTER(SslcpStats)]
    L.slamem_follow_letter_batch.argtypes = [vp, vp, vp, vp, vp, u64, vp]
    L.slamem_enclosing_interval_batch.argtypes = [vp, vp, vp, vp, u64, vp]
    L.slamem_position_in_text_batch.argtypes = [vp, vp, vp, u64, vp]
    L.slamem_char_at_bwt_pos_batch.argtypes = [vp, vp, vp, u64, vp]
    L.slamem_find_mems_workspace_bytes.argtypes = [u32, i32, u64, u64, C.POINTER(u64)]
    L.slamem_find_mems_device.argtypes = [vp, vp, vp, u32, u64, u32, i32, vp, u64, vp, vp, u64, vp, C.POINTER(u64)]
    L.slamem_find_mems_host.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, C.POINTER(C.POINTER(Mem)),
                                        C.POINTER(C.POINTER(u64)), C.POINTER(u64)]
    L.slamem_find_mams_device.argtypes = L.slamem_find_mems_device.argtypes
    L.slamem_find_mams_host.argtypes = L.slamem_find_mems_host.argtypes
    L.slamem_find_mums_workspace_bytes.argtypes = L.slamem_find_mems_workspace_bytes.argtypes
    L.slamem_find_mums_device.argtypes = L.slamem_find_mems_device.argtypes
    L.slamem_find_mums_host.argtypes = L.slamem_find_mems_host.argtypes
    L.slamem_find_smems_workspace_bytes.argtypes = L.slamem_find_mems_workspace_bytes.argtypes
    L.slamem_find_smems_device.argtypes = [vp, vp, vp, u32, u64, u32, i32, u32, vp, u64, vp, vp, u64, vp, C.POINTER(u64)]
    L.slamem_find_smems_host.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, u32, C.POINTER(C.POINTER(Mem)),
                                         C.POINTER(C.POINTER(u64)), C.POINTER(u64)]
    L.slamem_stream_create.argtypes = [vp, i32, u64, u32, i32, i32, C.POINTER(vp)]
    L.slamem_stream_set_max_occ.argtypes = [vp, u32]
    L.slamem_find_chains_workspace_bytes.argtypes = L.slamem_find_mems_workspace_bytes.argtypes
    L.slamem_find_chains_device.argtypes = [vp, vp, vp, u32, u64, u32, i32, u32, vp, u64, vp, vp, vp, u64, vp, C.POINTER(u64)]
    L.slamem_find_chains_host.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, u32, C.POINTER(C.POINTER(Mem)),
                                          C.POINTER(C.POINTER(u64)), C.POINTER(C.POINTER(u32)), C.POINTER(u64)]
    L.slamem_stream_set_max_gap.argtypes = [vp, u32]
    L.slamem_find_exts_workspace_bytes.argtypes = L.slamem_find_mems_workspace_bytes.argtypes
    L.slamem_find_exts_device.argtypes = [vp, vp, vp, u32, u64, u32, i32, u32, u32, vp, u64, vp, vp, vp, u64, vp, C.POINTER(u64)]
    L.slamem_find_exts_host.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, u32, u32, C.POINTER(C.POINTER(Mem)),
                                        C.POINTER(C.POINTER(u64)), C.POINTER(C.POINTER(u32)), C.POINTER(u64)]
    L.slamem_stream_set_ext_params.argtypes = [vp, u32, u32]
    L.slamem_stream_set_max_edits.argtypes = [vp, u32]
    L.slamem_stream_alns.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.slamem_find_alns_workspace_bytes.argtypes = [u32, i32, u64, u64, u64, u32, C.POINTER(u64)]
    L.slamem_find_alns_device.argtypes = [vp, vp, vp, u32, u64, u32, i32, u32, u32, u32, u32, u64, vp, u64, vp, vp, u64, vp, vp, u64,
                                          vp, C.POINTER(u64)]
    L.slamem_find_alns_host.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(vp),
                                        C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.slamem_find_maps_workspace_bytes.argtypes = [u32, i32, u64, u64, u64, u32, C.POINTER(u64)]
    L.slamem_find_maps_device.argtypes = [vp, vp, vp, u32, u64, u32, i32, u32, u32, u32, u32, u64, vp, u64, vp, vp, u64, vp, vp, vp,
                                          u64, vp, C.POINTER(u64)]
    L.slamem_find_maps_host.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(vp),
                                        C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.slamem_stream_maps.argtypes = [vp, C.POINTER(vp)]
    # the forms with end_band behind max_edits (-gext)
    L.slamem_stream_set_end_band.argtypes = [vp, u32]
    L.slamem_find_alns_end_counts_device.argtypes = [u32, i32, u64, u64, u64, u32, u32, vp, vp, C.POINTER(u64)]
    L.slamem_find_maps_md_host_gext.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, u32, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(vp),
                                                C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(vp),
                                                C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.slamem_find_alns_workspace_bytes_gext.argtypes = [u32, i32, u64, u64, u64, u32, u32, C.POINTER(u64)]
    L.slamem_find_maps_workspace_bytes_gext.argtypes = [u32, i32, u64, u64, u64, u32, u32, C.POINTER(u64)]
    L.slamem_find_alns_device_gext.argtypes = [vp, vp, vp, u32, u64, u32, i32, u32, u32, u32, u32, u32, u64, vp, u64, vp, vp, u64, vp,
                                               vp, u64, vp, C.POINTER(u64)]
    L.slamem_find_maps_device_gext.argtypes = [vp, vp, vp, u32, u64, u32, i32, u32, u32, u32, u32, u32, u64, vp, u64, vp, vp, u64, vp,
                                               vp, vp, u64, vp, C.POINTER(u64)]
    L.slamem_find_alns_host_gext.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, u32, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(vp),
                                             C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.slamem_find_maps_host_gext.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, u32, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(vp),
                                             C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.slamem_maps_md_workspace_bytes.argtypes = [u64, u32, C.POINTER(u64)]
    L.slamem_maps_md_device.argtypes = [vp, vp, u64, vp, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, C.POINTER(u64)]
    L.slamem_find_maps_md_host.argtypes = [vp, C.c_char_p, vp, u32, u32, i32, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(vp),
                                           C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(vp),
                                           C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.slamem_stream_set_md.argtypes = [vp, i32]
    L.slamem_stream_md.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.slamem_pileup_create.argtypes = [vp, C.POINTER(vp)]
    L.slamem_pileup_free.argtypes = [vp]
    L.slamem_pileup_reset.argtypes = [vp]
    L.slamem_pileup_add_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp]
    L.slamem_pileup_add_masked_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp]
    L.slamem_pack_lowq_device.argtypes = [vp, u64, u32, u32, vp, vp]
    L.slamem_pack_lowq.argtypes = [vp, u64, u32, u32, vp, i32]
    L.slamem_stream_submit_masked.argtypes = [vp, vp, vp, vp, u32, u32]
    L.slamem_pileup_counts_device.argtypes = [vp, u64, u64, vp, vp]
    L.slamem_pileup_counts_host.argtypes = [vp, u64, u64, vp]
    L.slamem_pileup_sites_device.argtypes = [vp, u64, u64, u32, u32, u32, u64, vp, vp, vp, C.POINTER(u64), vp]
    L.slamem_pileup_sites_host.argtypes = [vp, u64, u64, u32, u32, u32, u64, vp, vp, vp, C.POINTER(u64)]
    L.slamem_pileup_add_counts_device.argtypes = [vp, u64, u64, vp, vp]
    L.slamem_pileup_add_counts_host.argtypes = [vp, u64, u64, vp]
    L.slamem_pileup_enable_events.argtypes = [vp, u64]
    L.slamem_pileup_events_device.argtypes = [vp, u64, u64, u32, u64, vp, C.POINTER(u64), C.POINTER(u64), vp]
    L.slamem_pileup_events_host.argtypes = [vp, u64, u64, u32, u64, vp, C.POINTER(u64), C.POINTER(u64)]
    L.slamem_pileup_add_events_device.argtypes = [vp, vp, u64, vp]
    L.slamem_pileup_add_events_host.argtypes = [vp, vp, u64]
    L.slamem_pileup_enable_junctions.argtypes = [vp, u64, u32]
    L.slamem_pileup_junctions_device.argtypes = [vp, u64, u64, u32, u32, u64, vp, C.POINTER(u64), C.POINTER(u64), vp]
    L.slamem_pileup_junctions_host.argtypes = [vp, u64, u64, u32, u32, u64, vp, C.POINTER(u64), C.POINTER(u64)]
    L.slamem_pileup_add_junctions_device.argtypes = [vp, vp, u64, vp]
    L.slamem_pileup_add_junctions_host.argtypes = [vp, vp, u64]
    L.slamem_pileup_rows_at_device.argtypes = [vp, vp, u64, vp, vp]
    L.slamem_pileup_rows_at_host.argtypes = [vp, vp, u64, vp]
    L.slamem_pileup_consensus_device.argtypes = [vp, u64, u64, u32, u64, vp, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp]
    L.slamem_pileup_consensus_host.argtypes = [vp, u64, u64, u32, u64, vp, vp, u64, vp, C.POINTER(u64), C.POINTER(u64)]
    L.slamem_pileup_consensus_gt_device.argtypes = [vp, u64, u64, C.POINTER(ConsGtParams), u64, vp, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp]
    L.slamem_pileup_consensus_gt_host.argtypes = [vp, u64, u64, C.POINTER(ConsGtParams), u64, vp, vp, u64, vp, C.POINTER(u64), C.POINTER(u64)]
    L.slamem_pileup_depth_runs_device.argtypes = [vp, u64, u64, vp, u32, u32, u64, vp, vp, u64, vp, C.POINTER(u64), vp]
    L.slamem_pileup_depth_runs_host.argtypes = [vp, u64, u64, vp, u32, u32, u64, vp, vp, u64, vp, C.POINTER(u64)]
    L.slamem_stream_set_pileup.argtypes = [vp, vp, u32]
    L.slamem_pileup_enable_dedup.argtypes = [vp, u64]
    L.slamem_pileup_add_dedup_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    L.slamem_pileup_dedup_stats.argtypes = [vp, C.POINTER(u64)]
    L.slamem_stream_set_dedup.argtypes = [vp, i32]
    L.slamem_gt_costs.argtypes = [u32, C.POINTER(u32)]
    L.slamem_pileup_genotypes_device.argtypes = [vp, u64, u64, C.POINTER(GtParams), u64, vp, vp, vp, C.POINTER(u64), vp]
    L.slamem_pileup_genotypes_host.argtypes = [vp, u64, u64, C.POINTER(GtParams), u64, vp, vp, vp, C.POINTER(u64)]
    L.slamem_pileup_genotype_events_device.argtypes = [vp, vp, vp, u64, C.POINTER(GtParams), vp, vp, vp]
    L.slamem_pileup_genotype_events_host.argtypes = [vp, vp, vp, u64, C.POINTER(GtParams), vp, vp]
    L.slamem_pileup_enable_strands.argtypes = [vp]
    L.slamem_pileup_forward.argtypes = [vp, C.POINTER(vp)]
    L.slamem_pileup_enable_quals.argtypes = [vp]
    L.slamem_pileup_quality.argtypes = [vp, C.POINTER(vp)]
    L.slamem_pileup_add_quals_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, C.c_int, vp, vp, vp]
    L.slamem_pileup_genotypes_weighted_device.argtypes = [vp, u64, u64, C.POINTER(GtParams), u64, vp, vp, vp, vp, C.POINTER(u64), vp]
    L.slamem_pileup_genotypes_weighted_host.argtypes = [vp, u64, u64, C.POINTER(GtParams), u64, vp, vp, vp, vp, C.POINTER(u64)]
    L.slamem_stream_set_quals.argtypes = [vp, u32]
    L.slamem_stream_submit_quals.argtypes = [vp, vp, vp, vp, vp, u32, u32]
    L.slamem_stats_create.argtypes = [vp, C.POINTER(vp)]
    L.slamem_stats_free.argtypes = [vp]
    L.slamem_stats_reset.argtypes = [vp]
    L.slamem_stats_add_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, u32, u32, vp]
    L.slamem_stats_table_device.argtypes = [vp, vp, vp]
    L.slamem_stats_table_host.argtypes = [vp, vp]
    L.slamem_stats_add_table_host.argtypes = [vp, vp]
    L.slamem_stream_set_stats.argtypes = [vp, vp, u32, i32]
    L.slamem_fisher_strand.argtypes = [C.POINTER(u32)]
    L.slamem_fisher_strand.restype = C.c_double
    L.slamem_fisher_strand_table.argtypes = [C.POINTER(u32), C.POINTER(u32)]
    L.slamem_fisher_strand_table.restype = None
    L.slamem_stream_dups.argtypes = [vp, C.POINTER(vp)]
    L.slamem_stream_mismatches.argtypes = [vp, C.POINTER(C.POINTER(u32))]
    L.slamem_stream_submit.argtypes = [vp, vp, vp, u32, u32]
    L.slamem_copy_to_host.argtypes = [vp, vp, u64]
    L.slamem_stream_submit_packed.argtypes = [vp, vp, vp, vp, u32, u64, u32]
    L.slamem_pack_reads.argtypes = [vp, vp, u32, vp, vp, C.POINTER(u64), i32]
    L.slamem_stream_next.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u32), C.POINTER(Timings)]
    L.slamem_stream_destroy.argtypes = [vp]
    L.slamem_pinned_alloc.argtypes = [C.POINTER(vp), u64]
    L.slamem_pinned_free.argtypes = [vp]
    L.slamem_host_free.argtypes = [vp]
    L.slamem_host_free.restype = None
    for name in ABI_SYMBOLS:
        f = getattr(L, name)
        if f.restype is C.c_int and name not in ("slamem_abi_version",):
            f.restype = i32


def _load_torch_runtime_first():
    # torch bundles its own libamdhip64; if libslamem_hip.so pulls in /opt/rocm's copy BEFORE torch loads its
    # own, the process ends up with two HIP runtimes and the second one sees no device.  Loading torch first
    # makes both share one runtime (the C front end never loads torch and simply uses /opt/rocm's).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib():
    """The loaded HIP library; raises (loudly) if it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C slamem_amd/csrc`).  slamem_amd has no CPU fallback.")
        _load_torch_runtime_first()
        L = C.CDLL(LIB_PATH)
        _declare(L)
        if L.slamem_abi_version() != 4:
            raise ImportError("libslamem_hip.so ABI version mismatch")
        _LIB = L
    return _LIB


def synth_lib():
    global _SYNTH
    if _SYNTH is None:
        if not os.path.exists(SYNTH_PATH):
            raise ImportError(f"{SYNTH_PATH} is missing: run __graft_entry__.build()")
        _load_torch_runtime_first()
        S = C.CDLL(SYNTH_PATH)
        S.slamem_synth_reference.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        S.slamem_synth_reads.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                         C.c_double, C.c_uint64, C.c_uint32, C.c_void_p]
        S.slamem_gather_modes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        S.slamem_gather_bench.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        S.slamem_synth_plant_repeats.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
        S.slamem_synth_reads_avoid.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                               C.c_double, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
        S.slamem_synth_plant_genome_like.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
        _SYNTH = S
    return _SYNTH


def check(code: int):
    if code != SLAMEM_OK:
        raise SlamemError(code, lib().slamem_last_error_message().decode(errors="replace"))
