// capi.hip -- the extern "C" surface of libslamem_hip.so (include/slamem_hip.h).
// Plain pointers and sizes only.  There is no CPU fallback anywhere in this library: without a
// usable gfx950 device every compute entry point fails with SLAMEM_ERR_NO_DEVICE / SLAMEM_ERR_HIP.
#include "buffers.h"
#include "common.h"
#include "../../include/slamem_fisher.h"

#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

namespace slamem {

static thread_local char g_err[512] = "";
static thread_local Timings g_tm;

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    const char* base = strrchr(file, '/');
    set_error("HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, base ? base + 1 : file, line);
    if (e == hipErrorOutOfMemory) return SLAMEM_ERR_NOMEM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return SLAMEM_ERR_NO_DEVICE;
    return SLAMEM_ERR_HIP;
}

Timings& thread_timings() { return g_tm; }
static thread_local bool g_want_stats = false;
static thread_local slamem_search_stats g_stats;
bool search_stats_wanted() { return g_want_stats; }
slamem_search_stats& last_search_stats() { return g_stats; }
static thread_local double g_clock[3];
double* last_search_clock() { return g_clock; }

int download_array(const slamem_index* idx, int which, void* host_dst, uint64_t count);
int sampled_lcp_stats(const slamem_index* idx, slamem_sslcp_stats* out);
int follow_letter_batch(const slamem_index*, const char*, uint32_t*, uint32_t*, uint32_t*, uint64_t, hipStream_t);
int enclosing_interval_batch(const slamem_index*, uint32_t*, uint32_t*, int32_t*, uint64_t, hipStream_t);
int position_in_text_batch(const slamem_index*, const uint32_t*, uint32_t*, uint64_t, hipStream_t);
int char_at_bwt_pos_batch(const slamem_index*, const uint32_t*, char*, uint64_t, hipStream_t);

static int check_device(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device available (%s): libslamem_hip has no CPU path", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return SLAMEM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        set_error("device %d out of range (0..%d)", device, count - 1);
        return SLAMEM_ERR_ARG;
    }
    return SLAMEM_OK;
}

// Every section the kernels will index must lie inside the arena, in order, aligned for the paired 64-byte FM blocks:
// a truncated, stale or corrupted file / peer buffer is refused here instead of faulting on the GPU.
static int header_ok(const ArenaHeader& h, uint64_t bytes) {
    if (h.magic_lo != kArenaMagicLo || h.magic_hi != kArenaMagicHi || h.version != kArenaVersion) {
        set_error("not a slamem index arena (bad magic / version)");
        return SLAMEM_ERR_FORMAT;
    }
    if (h.total_bytes > bytes || h.total_bytes < kHeaderBytes) {
        set_error("index arena truncated: header says %llu bytes, got %llu", (unsigned long long)h.total_bytes,
                  (unsigned long long)bytes);
        return SLAMEM_ERR_FORMAT;
    }
    const uint64_t R = (uint64_t)h.n + 1;
    const char* bad = nullptr;
    uint64_t end = kHeaderBytes;  // end of the previous section
    auto section = [&](uint64_t off, uint64_t size, const char* name) {
        if (bad) return;
        if ((off & 127u) != 0 || off < end || off > h.total_bytes || size > h.total_bytes - off) bad = name;
        end = off + size;
    };
    if (h.n == 0 || h.n > 0xFFFFFFF0u) bad = "text length";
    if (!bad && h.nblocks != (uint32_t)((R + 1 + kFmRows - 1) >> kFmRowsLog2)) bad = "FM block count";
    if (!bad && h.off_fm != kHeaderBytes) bad = "FM block offset";
    section(h.off_fm, (uint64_t)h.nblocks * sizeof(FMBlock), "FM blocks");
    section(h.off_rec, (R + 1) * sizeof(RowRec), "row records");
    section(h.off_sa, R * 4, "suffix array");
    if (!bad && h.num_n > h.n) bad = "N row count";
    section(h.off_nrows, (uint64_t)(h.num_n ? h.num_n : 1) * 4, "N row list");
    if (h.off_kfilter) {
        if (!bad && (h.kfilter_log2 < 10 || h.kfilter_log2 > 40 || h.kfilter_k < 4 || h.kfilter_k > 26 ||
                     (h.kfilter_levels != 0u && h.kfilter_levels != 2u && h.kfilter_levels != 3u))) bad = "presence filter parameters";
        if (!bad) section(h.off_kfilter, 8ull << h.kfilter_log2, "presence filter");
    }
    if (h.off_tgrp || h.off_prec) {
        section(h.off_tgrp, ((R >> 4) + 2) * sizeof(TextGroup), "text groups");
        section(h.off_prec, R * sizeof(TextRec), "text-ordered records");
    }
    if (h.off_kjump) {
        if (!bad && (h.kjump_k < 1 || h.kjump_k > 12)) bad = "jump table K";
        if (!bad) section(h.off_kjump, 8ull << (2u * h.kjump_k), "jump table");
    }
    if (h.off_kbits) {
        if (!bad && (h.kbits_k < 8 || h.kbits_k > 16)) bad = "occurrence bitmap k";
        if (!bad) section(h.off_kbits, (1ull << (2u * h.kbits_k)) >> 3, "occurrence bitmap");
    }
    if (h.off_seed || h.off_tpl || h.off_spill) {
        const uint64_t units = text_units(h.n);
        if (!bad && (h.seed_k < 4 || h.seed_k > kSeedMaxK || h.seed_log2 < 10 || h.seed_log2 > 30 || 2u * h.seed_k < h.seed_log2 ||
                     2u * h.seed_k - h.seed_log2 > 7u)) bad = "seed table parameters";
        if (!bad) section(h.off_seed, sizeof(SeedBucket) << h.seed_log2, "seed table");
        section(h.off_tpl, units * sizeof(TextPlanes), "text units");
        if (!bad && (h.spill_cap != seed_spill_entries(h.n) || h.spill_used > h.spill_cap)) bad = "seed spill list size";
        section(h.off_spill, (uint64_t)h.spill_cap * 8, "seed spill list");
    }
    if (!bad && (h.off_tnm || h.off_tnb || h.off_tuq)) bad = "reserved section offsets";
    if (!bad && h.dollar_row > h.n) bad = "'$' row";
    if (bad) {
        set_error("index arena is corrupt or truncated: bad %s", bad);
        return SLAMEM_ERR_FORMAT;
    }
    return SLAMEM_OK;
}

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_abi_version(void) { return SLAMEM_ABI_VERSION; }

const char* slamem_strerror(int code) {
    switch (code) {
    case SLAMEM_OK: return "ok";
    case SLAMEM_ERR_ARG: return "bad argument";
    case SLAMEM_ERR_HIP: return "HIP runtime error";
    case SLAMEM_ERR_NOMEM: return "out of memory";
    case SLAMEM_ERR_CAPACITY: return "output capacity too small";
    case SLAMEM_ERR_FORMAT: return "not a slamem index";
    case SLAMEM_ERR_IO: return "I/O error";
    case SLAMEM_ERR_NO_DEVICE: return "no usable GPU (there is no CPU fallback)";
    default: return "unknown error";
    }
}

const char* slamem_last_error_message(void) { return g_err; }

// -gt: the three costs of a letter at a constant error rate of Phred q.  Host arithmetic in doubles, one
// operation after the other as engine.gt_costs and tests/gt_spec.py write them, rounded half up.
int slamem_gt_costs(uint32_t q, uint32_t out[3]) {
    if (!out) { set_error("slamem_gt_costs: null argument"); return SLAMEM_ERR_ARG; }
    if (q < 1u || q > 93u) { set_error("slamem_gt_costs: the error rate is 1 to 93 Phred, not %u", q); return SLAMEM_ERR_ARG; }
    // (volatile: every intermediate is rounded to a double of its own, never fused with the next operation)
    const volatile double e = pow(10.0, -(double)q / 10.0);
    const volatile double hom = 1.0 - e, half = hom / 2.0, sixth = e / 6.0, het = half + sixth, third = e / 3.0;
    out[0] = (uint32_t)floor(-10000.0 * log10(hom) + 0.5);
    out[1] = (uint32_t)floor(-10000.0 * log10(het) + 0.5);
    out[2] = (uint32_t)floor(-10000.0 * log10(third) + 0.5);
    return SLAMEM_OK;
}

// -sb: FS of a strand table and the table as the test sees it; include/slamem_fisher.h has the one definition
double slamem_fisher_strand(const uint32_t t[4]) {
    uint32_t norm[4];
    return t ? slamem_fisher_strand_of(t, norm) : 0.0;
}

void slamem_fisher_strand_table(const uint32_t t[4], uint32_t out[4]) {
    if (t && out) (void)slamem_fisher_strand_of(t, out);
}

int slamem_device_count(int* count_out) {
    if (!count_out) return SLAMEM_ERR_ARG;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count_out = 0; return hip_fail(e, "hipGetDeviceCount", __FILE__, __LINE__); }
    *count_out = c;
    return SLAMEM_OK;
}

int slamem_device_warmup(int device) {
    SLAMEM_HIP(hipSetDevice(device));
    SLAMEM_HIP(hipFree(nullptr));
    return SLAMEM_OK;
}

int slamem_device_pci_bus_id(int device, char* out, int out_bytes) {
    if (!out || out_bytes < 16) return SLAMEM_ERR_ARG;
    int rc = check_device(device);
    if (rc) return rc;
    SLAMEM_HIP(hipDeviceGetPCIBusId(out, out_bytes, device));
    return SLAMEM_OK;
}

int slamem_get_timings(slamem_timings* out) {
    if (!out) return SLAMEM_ERR_ARG;
    *out = g_tm.t;
    return SLAMEM_OK;
}

int slamem_search_stats_enable(int on) {
    g_want_stats = on != 0;
    return SLAMEM_OK;
}

int slamem_get_search_stats(slamem_search_stats* out) {
    if (!out) return SLAMEM_ERR_ARG;
    *out = g_stats;
    return SLAMEM_OK;
}

int slamem_get_search_clock(double* us_to_empty_list, double* us_tail, double* us_wave_sum) {
    if (us_to_empty_list) *us_to_empty_list = g_clock[0];
    if (us_tail) *us_tail = g_clock[1];
    if (us_wave_sum) *us_wave_sum = g_clock[2];
    return SLAMEM_OK;
}

int slamem_reset_timings(void) {
    memset(&g_tm.t, 0, sizeof(g_tm.t));
    return SLAMEM_OK;
}

int slamem_device_mem_info(int device, uint64_t* free_out, uint64_t* total_out) {
    int rc = check_device(device);
    if (rc) return rc;
    SLAMEM_HIP(hipSetDevice(device));
    size_t f = 0, t = 0;
    SLAMEM_HIP(hipMemGetInfo(&f, &t));
    if (free_out) *free_out = f;
    if (total_out) *total_out = t;
    return SLAMEM_OK;
}

int slamem_index_build_bytes(uint32_t n, int layout, uint64_t* arena_bytes_out, uint64_t* peak_bytes_out) {
    return estimate_build_bytes(n, layout, arena_bytes_out, peak_bytes_out);
}

int slamem_index_build_device(const void* text_dev, uint32_t n, int device, void* stream, slamem_index** out) {
    return slamem_index_build_device_layout(text_dev, n, device, stream, SLAMEM_LAYOUT_AUTO, out);
}

int slamem_index_build_device_layout(const void* text_dev, uint32_t n, int device, void* stream, int layout,
                                     slamem_index** out) {
    int rc = check_device(device);
    if (rc) return rc;
    return build_index_device(text_dev, n, device, static_cast<hipStream_t>(stream), layout, out);
}

int slamem_index_build(const char* text_host, uint32_t n, int device, slamem_index** out) {
    return slamem_index_build_layout(text_host, n, device, SLAMEM_LAYOUT_AUTO, out);
}

int slamem_index_build_layout(const char* text_host, uint32_t n, int device, int layout, slamem_index** out) {
    if (!text_host || !out || n == 0) { set_error("slamem_index_build: empty text"); return SLAMEM_ERR_ARG; }
    int rc = check_device(device);
    if (rc) return rc;
    SLAMEM_HIP(hipSetDevice(device));
    void* d = nullptr;
    SLAMEM_HIP(hipMalloc(&d, (size_t)n + 16));
    hipError_t e = hipMemcpy(d, text_host, n, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(e, "hipMemcpy(text)", __FILE__, __LINE__); }
    rc = build_index_device(d, n, device, nullptr, layout, out);
    (void)hipFree(d);
    return rc;
}

int slamem_index_free(slamem_index* idx) {
    if (!idx) return SLAMEM_OK;
    if (idx->owns_arena && idx->arena) {
        (void)hipSetDevice(idx->device);
        (void)hipFree(idx->arena);
    }
    free(idx);
    return SLAMEM_OK;
}

int slamem_index_get_info(const slamem_index* idx, slamem_index_info* out) {
    if (!idx || !out) return SLAMEM_ERR_ARG;
    out->text_length = idx->hdr.n;
    out->bwt_size = idx->hdr.n + 1;
    out->num_n_rows = idx->hdr.num_n;
    out->dollar_row = idx->hdr.dollar_row;
    out->max_lcp = idx->hdr.max_lcp;
    out->sort_rounds = idx->hdr.sort_rounds;
    out->arena_bytes = idx->arena_bytes;
    out->device = idx->device;
    out->owns_arena = idx->owns_arena;
    out->filter_k = idx->hdr.off_kfilter ? idx->hdr.kfilter_k : 0u;
    out->seed_k = idx->hdr.off_seed ? idx->hdr.seed_k : 0u;
    out->reserved1 = 0u;
    out->layout = idx->hdr.layout == 2u ? SLAMEM_LAYOUT_COMPACT : SLAMEM_LAYOUT_FULL;
    return SLAMEM_OK;
}

int slamem_index_arena(const slamem_index* idx, void** arena_dev_out, uint64_t* bytes_out) {
    if (!idx || !arena_dev_out || !bytes_out) return SLAMEM_ERR_ARG;
    *arena_dev_out = idx->arena;
    *bytes_out = idx->arena_bytes;
    return SLAMEM_OK;
}

int slamem_index_export(const slamem_index* idx, void* dst_dev, uint64_t dst_bytes, void* stream) {
    if (!idx || !dst_dev) return SLAMEM_ERR_ARG;
    if (dst_bytes < idx->arena_bytes) { set_error("slamem_index_export: destination too small"); return SLAMEM_ERR_ARG; }
    SLAMEM_HIP(hipSetDevice(idx->device));
    SLAMEM_HIP(hipMemcpyAsync(dst_dev, idx->arena, idx->arena_bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    SLAMEM_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return SLAMEM_OK;
}

int slamem_index_attach(void* arena_dev, uint64_t bytes, int device, slamem_index** out) {
    if (!arena_dev || !out || bytes < kHeaderBytes) { set_error("slamem_index_attach: bad arena"); return SLAMEM_ERR_ARG; }
    if (((uintptr_t)arena_dev & 127u) != 0) { set_error("slamem_index_attach: the arena must be 128-byte aligned"); return SLAMEM_ERR_ARG; }
    int rc = check_device(device);
    if (rc) return rc;
    SLAMEM_HIP(hipSetDevice(device));
    ArenaHeader h;
    SLAMEM_HIP(hipMemcpy(&h, arena_dev, sizeof(h), hipMemcpyDeviceToHost));
    rc = header_ok(h, bytes);
    if (rc) return rc;
    slamem_index* idx = static_cast<slamem_index*>(calloc(1, sizeof(slamem_index)));
    if (!idx) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    idx->hdr = h;
    idx->arena = arena_dev;
    idx->arena_bytes = h.total_bytes;
    idx->device = device;
    idx->owns_arena = 0;
    make_view(idx);
    *out = idx;
    return SLAMEM_OK;
}

int slamem_index_adopt_arena(slamem_index* idx) {
    if (!idx) return SLAMEM_ERR_ARG;
    idx->owns_arena = 1;
    return SLAMEM_OK;
}

int slamem_index_save(const slamem_index* idx, const char* path) {
    if (!idx || !path) return SLAMEM_ERR_ARG;
    SLAMEM_HIP(hipSetDevice(idx->device));
    FILE* f = fopen(path, "wb");
    if (!f) { set_error("cannot create <%s>", path); return SLAMEM_ERR_IO; }
    const uint64_t chunk = 64ull << 20;
    char* buf = static_cast<char*>(malloc(chunk));
    if (!buf) { fclose(f); set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    int rc = SLAMEM_OK;
    for (uint64_t off = 0; off < idx->arena_bytes; off += chunk) {
        uint64_t len = idx->arena_bytes - off < chunk ? idx->arena_bytes - off : chunk;
        hipError_t e = hipMemcpy(buf, static_cast<char*>(idx->arena) + off, len, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { rc = hip_fail(e, "hipMemcpy(save)", __FILE__, __LINE__); break; }
        if (fwrite(buf, 1, len, f) != len) { set_error("short write to <%s>", path); rc = SLAMEM_ERR_IO; break; }
    }
    free(buf);
    if (fclose(f) != 0 && rc == SLAMEM_OK) { set_error("cannot close <%s>", path); rc = SLAMEM_ERR_IO; }
    return rc;
}

int slamem_index_validate_header(const void* header, uint64_t header_bytes, uint64_t available_bytes) {
    if (!header || header_bytes < sizeof(ArenaHeader)) { set_error("slamem_index_validate_header: need the first %zu bytes", sizeof(ArenaHeader)); return SLAMEM_ERR_ARG; }
    ArenaHeader h;
    memcpy(&h, header, sizeof(h));
    return header_ok(h, available_bytes);
}

int slamem_index_load(const char* path, int device, slamem_index** out) {
    if (!path || !out) return SLAMEM_ERR_ARG;
    int rc;
    FILE* f = fopen(path, "rb");
    if (!f) { set_error("cannot open <%s>", path); return SLAMEM_ERR_IO; }
    ArenaHeader h;
    if (fread(&h, 1, sizeof(h), f) != sizeof(h)) { fclose(f); set_error("<%s> is too short", path); return SLAMEM_ERR_FORMAT; }
    uint64_t file_bytes = 0;
    if (fseeko(f, 0, SEEK_END) == 0) { off_t e2 = ftello(f); if (e2 > 0) file_bytes = (uint64_t)e2; }
    rc = header_ok(h, file_bytes);  // before any device call: a bad file is reported as such on any machine
    if (rc == SLAMEM_OK) rc = check_device(device);
    if (rc) { fclose(f); return rc; }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { fclose(f); return hip_fail(e, "hipSetDevice", __FILE__, __LINE__); }
    void* arena = nullptr;
    e = hipMalloc(&arena, h.total_bytes);
    if (e != hipSuccess) { fclose(f); return hip_fail(e, "hipMalloc(load)", __FILE__, __LINE__); }
    const uint64_t chunk = 64ull << 20;
    char* buf = static_cast<char*>(malloc(chunk));
    rewind(f);
    rc = buf ? SLAMEM_OK : SLAMEM_ERR_NOMEM;
    for (uint64_t off = 0; rc == SLAMEM_OK && off < h.total_bytes; off += chunk) {
        uint64_t len = h.total_bytes - off < chunk ? h.total_bytes - off : chunk;
        if (fread(buf, 1, len, f) != len) { set_error("<%s> is truncated", path); rc = SLAMEM_ERR_FORMAT; break; }
        e = hipMemcpy(static_cast<char*>(arena) + off, buf, len, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy(load)", __FILE__, __LINE__);
    }
    free(buf);
    fclose(f);
    if (rc) { (void)hipFree(arena); return rc; }
    slamem_index* idx = static_cast<slamem_index*>(calloc(1, sizeof(slamem_index)));
    if (!idx) { (void)hipFree(arena); set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    idx->hdr = h;
    idx->arena = arena;
    idx->arena_bytes = h.total_bytes;
    idx->device = device;
    idx->owns_arena = 1;
    make_view(idx);
    *out = idx;
    return SLAMEM_OK;
}

int slamem_index_download(const slamem_index* idx, int which, void* host_dst, uint64_t count) {
    if (!idx || !host_dst) return SLAMEM_ERR_ARG;
    return download_array(idx, which, host_dst, count);
}

int slamem_index_sampled_lcp_stats(const slamem_index* idx, slamem_sslcp_stats* out) {
    if (!idx || !out) return SLAMEM_ERR_ARG;
    return sampled_lcp_stats(idx, out);
}

int slamem_follow_letter_batch(const slamem_index* idx, const char* letters_dev, uint32_t* top_dev, uint32_t* bottom_dev,
                               uint32_t* size_out_dev, uint64_t count, void* stream) {
    if (!idx || (count && (!letters_dev || !top_dev || !bottom_dev || !size_out_dev))) return SLAMEM_ERR_ARG;
    return follow_letter_batch(idx, letters_dev, top_dev, bottom_dev, size_out_dev, count, static_cast<hipStream_t>(stream));
}

int slamem_enclosing_interval_batch(const slamem_index* idx, uint32_t* top_dev, uint32_t* bottom_dev,
                                    int32_t* depth_out_dev, uint64_t count, void* stream) {
    if (!idx || (count && (!top_dev || !bottom_dev || !depth_out_dev))) return SLAMEM_ERR_ARG;
    return enclosing_interval_batch(idx, top_dev, bottom_dev, depth_out_dev, count, static_cast<hipStream_t>(stream));
}

int slamem_position_in_text_batch(const slamem_index* idx, const uint32_t* rows_dev, uint32_t* pos_out_dev,
                                  uint64_t count, void* stream) {
    if (!idx || (count && (!rows_dev || !pos_out_dev))) return SLAMEM_ERR_ARG;
    return position_in_text_batch(idx, rows_dev, pos_out_dev, count, static_cast<hipStream_t>(stream));
}

int slamem_char_at_bwt_pos_batch(const slamem_index* idx, const uint32_t* rows_dev, char* chars_out_dev, uint64_t count,
                                 void* stream) {
    if (!idx || (count && (!rows_dev || !chars_out_dev))) return SLAMEM_ERR_ARG;
    return char_at_bwt_pos_batch(idx, rows_dev, chars_out_dev, count, static_cast<hipStream_t>(stream));
}

int slamem_find_mems_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                     uint64_t* bytes_out) {
    if (!bytes_out) return SLAMEM_ERR_ARG;
    *bytes_out = find_mems_workspace_bytes(num_queries, both_strands, query_bytes, mems_capacity);
    return SLAMEM_OK;
}

int slamem_find_mems_device(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev,
                            uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands,
                            slamem_mem* mems_dev, uint64_t mems_capacity, uint64_t* block_offsets_dev, void* workspace_dev,
                            uint64_t workspace_bytes, void* stream, uint64_t* total_out) {
    return find_mems_device(idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands, 0, mems_dev,
                            mems_capacity, block_offsets_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream),
                            total_out, nullptr, nullptr);
}

int slamem_find_mams_device(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev,
                            uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands,
                            slamem_mem* mems_dev, uint64_t mems_capacity, uint64_t* block_offsets_dev, void* workspace_dev,
                            uint64_t workspace_bytes, void* stream, uint64_t* total_out) {
    return find_mems_device(idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands, 1, mems_dev,
                            mems_capacity, block_offsets_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream),
                            total_out, nullptr, nullptr);
}

// The filtered searches: the placeholders of the public interface -> values (resolve_filter_params), then the one search.
static int filter_workspace_bytes(const char* who, int match_type, uint32_t num_queries, int both_strands, uint64_t query_bytes,
                                  uint64_t mems_capacity, uint64_t ops_capacity, uint32_t max_edits, uint64_t* bytes_out, uint32_t end_band = 0) {
    if (!bytes_out) return SLAMEM_ERR_ARG;
    FilterParams p;
    if (int bad = resolve_filter_params(who, 0, 0, 0, kExtXdropUnset, max_edits, &p)) return bad;
    if (int bad = set_end_band(who, end_band, &p)) return bad;
    p.ops_capacity = ops_capacity;
    *bytes_out = search_workspace_bytes(num_queries, both_strands, query_bytes, mems_capacity, match_type, p);
    return SLAMEM_OK;
}

int slamem_find_mums_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                     uint64_t* bytes_out) {
    return filter_workspace_bytes("slamem_find_mums_workspace_bytes", 2, num_queries, both_strands, query_bytes, mems_capacity, 0,
                                  kAlnEditsUnset, bytes_out);
}

int slamem_find_mums_device(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev,
                            uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands,
                            slamem_mem* mems_dev, uint64_t mems_capacity, uint64_t* block_offsets_dev, void* workspace_dev,
                            uint64_t workspace_bytes, void* stream, uint64_t* total_out) {
    FilterParams p;
    if (int bad = resolve_filter_params("slamem_find_mums_device", 0, 0, 0, kExtXdropUnset, kAlnEditsUnset, &p)) return bad;
    return find_mems_device(idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands, 2, mems_dev,
                            mems_capacity, block_offsets_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream),
                            total_out, &p, nullptr);
}

int slamem_find_smems_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                      uint64_t* bytes_out) {
    return filter_workspace_bytes("slamem_find_smems_workspace_bytes", 3, num_queries, both_strands, query_bytes, mems_capacity, 0,
                                  kAlnEditsUnset, bytes_out);
}

int slamem_find_smems_device(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev,
                             uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_occ,
                             slamem_mem* mems_dev, uint64_t mems_capacity, uint64_t* block_offsets_dev, void* workspace_dev,
                             uint64_t workspace_bytes, void* stream, uint64_t* total_out) {
    FilterParams p;
    if (int bad = resolve_filter_params("slamem_find_smems_device", max_occ, 0, 0, kExtXdropUnset, kAlnEditsUnset, &p)) return bad;
    return find_mems_device(idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands, 3, mems_dev,
                            mems_capacity, block_offsets_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream),
                            total_out, &p, nullptr);
}

int slamem_find_chains_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                       uint64_t* bytes_out) {
    return filter_workspace_bytes("slamem_find_chains_workspace_bytes", 4, num_queries, both_strands, query_bytes, mems_capacity, 0,
                                  kAlnEditsUnset, bytes_out);
}

int slamem_find_chains_device(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev,
                              uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap,
                              slamem_mem* mems_dev, uint64_t mems_capacity, uint64_t* block_offsets_dev,
                              uint32_t* block_scores_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream,
                              uint64_t* total_out) {
    FilterParams p;
    if (int bad = resolve_filter_params("slamem_find_chains_device", 0, max_gap, 0, kExtXdropUnset, kAlnEditsUnset, &p)) return bad;
    p.column_dev = block_scores_dev;
    return find_mems_device(idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands, 4, mems_dev,
                            mems_capacity, block_offsets_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream),
                            total_out, &p, nullptr);
}

int slamem_find_exts_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                     uint64_t* bytes_out) {
    return filter_workspace_bytes("slamem_find_exts_workspace_bytes", 5, num_queries, both_strands, query_bytes, mems_capacity, 0,
                                  kAlnEditsUnset, bytes_out);
}

int slamem_find_exts_device(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                            uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t mismatch_penalty, uint32_t xdrop,
                            slamem_mem* mems_dev, uint64_t mems_capacity, uint64_t* block_offsets_dev, uint32_t* mismatches_dev,
                            void* workspace_dev, uint64_t workspace_bytes, void* stream, uint64_t* total_out) {
    FilterParams p;
    if (int bad = resolve_filter_params("slamem_find_exts_device", 0, 0, mismatch_penalty, xdrop, kAlnEditsUnset, &p)) return bad;
    p.column_dev = mismatches_dev;
    return find_mems_device(idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands, 5, mems_dev,
                            mems_capacity, block_offsets_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream),
                            total_out, &p, nullptr);
}

int slamem_find_alns_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                     uint64_t ops_capacity, uint32_t max_edits, uint64_t* bytes_out) {
    return slamem_find_alns_workspace_bytes_gext(num_queries, both_strands, query_bytes, mems_capacity, ops_capacity, max_edits, 0, bytes_out);
}

int slamem_find_alns_workspace_bytes_gext(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                          uint64_t ops_capacity, uint32_t max_edits, uint32_t end_band, uint64_t* bytes_out) {
    return filter_workspace_bytes("slamem_find_alns_workspace_bytes", 6, num_queries, both_strands, query_bytes, mems_capacity,
                                  ops_capacity, max_edits, bytes_out, end_band);
}

int slamem_find_maps_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                     uint64_t ops_capacity, uint32_t max_edits, uint64_t* bytes_out) {
    return slamem_find_maps_workspace_bytes_gext(num_queries, both_strands, query_bytes, mems_capacity, ops_capacity, max_edits, 0, bytes_out);
}

int slamem_find_maps_workspace_bytes_gext(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                          uint64_t ops_capacity, uint32_t max_edits, uint32_t end_band, uint64_t* bytes_out) {
    return filter_workspace_bytes("slamem_find_maps_workspace_bytes", 7, num_queries, both_strands, query_bytes, mems_capacity,
                                  ops_capacity, max_edits, bytes_out, end_band);
}

// -gext: the two counters the kernels of the last call left in its workspace (sized by the same arguments)
int slamem_find_alns_end_counts_device(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                       uint64_t ops_capacity, uint32_t max_edits, uint32_t end_band, const void* workspace_dev,
                                       void* stream, uint64_t* counts_out) {
    const char* who = "slamem_find_alns_end_counts_device";
    if (!workspace_dev || !counts_out) { set_error("%s: null argument", who); return SLAMEM_ERR_ARG; }
    FilterParams p;
    if (int bad = resolve_filter_params(who, 0, 0, 0, kExtXdropUnset, max_edits, &p)) return bad;
    if (int bad = set_end_band(who, end_band, &p)) return bad;
    p.ops_capacity = ops_capacity;
    const FilterBatch b = {nullptr, nullptr, nullptr, num_queries, both_strands ? 2u : 1u, query_bytes, mems_capacity};
    const char* ctr = static_cast<const char*>(workspace_dev) + find_mems_workspace_bytes(num_queries, both_strands, query_bytes, mems_capacity) +
                      aln_counters_offset(b, p);
    unsigned long long h[2] = {0, 0};
    SLAMEM_HIP(hipMemcpyAsync(h, ctr + 5 * 8, 16, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    SLAMEM_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    counts_out[0] = h[0];
    counts_out[1] = h[1];
    return SLAMEM_OK;
}

// -aln and -paf (reads_dev: -paf's record per read, then offsets_out_dev takes num_queries + 1 read offsets)
static int find_segments_device(const char* who, const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev,
                                uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap,
                                uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits, uint64_t mems_capacity, slamem_aln* segs_dev,
                                uint64_t segs_capacity, uint64_t* offsets_out_dev, uint32_t* ops_dev, uint64_t ops_capacity,
                                uint64_t* op_offsets_dev, slamem_map* reads_dev, int match_type, void* workspace_dev,
                                uint64_t workspace_bytes, void* stream, uint64_t* totals_out, uint32_t end_band) {
    if (!totals_out) { set_error("%s: null argument", who); return SLAMEM_ERR_ARG; }
    totals_out[0] = totals_out[1] = totals_out[2] = 0;
    FilterParams p;
    if (int bad = resolve_filter_params(who, 0, max_gap, mismatch_penalty, xdrop, max_edits, &p)) return bad;
    if (int bad = set_end_band(who, end_band, &p)) return bad;
    p.segs = segs_dev;
    p.segs_capacity = segs_capacity;
    p.ops = ops_dev;
    p.ops_capacity = ops_capacity;
    p.op_offsets = op_offsets_dev;
    p.reads = reads_dev;
    uint64_t total = 0;
    return find_mems_device(idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands, match_type, nullptr,
                            mems_capacity, offsets_out_dev, workspace_dev, workspace_bytes, static_cast<hipStream_t>(stream), &total, &p,
                            totals_out);
}

int slamem_find_alns_device(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                            uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty,
                            uint32_t xdrop, uint32_t max_edits, uint64_t mems_capacity, slamem_aln* segs_dev, uint64_t segs_capacity,
                            uint64_t* block_offsets_dev, uint32_t* ops_dev, uint64_t ops_capacity, uint64_t* op_offsets_dev,
                            void* workspace_dev, uint64_t workspace_bytes, void* stream, uint64_t* totals_out) {
    return slamem_find_alns_device_gext(idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands, max_gap,
                                        mismatch_penalty, xdrop, max_edits, 0, mems_capacity, segs_dev, segs_capacity, block_offsets_dev,
                                        ops_dev, ops_capacity, op_offsets_dev, workspace_dev, workspace_bytes, stream, totals_out);
}

int slamem_find_alns_device_gext(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                                 uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty,
                                 uint32_t xdrop, uint32_t max_edits, uint32_t end_band, uint64_t mems_capacity, slamem_aln* segs_dev,
                                 uint64_t segs_capacity, uint64_t* block_offsets_dev, uint32_t* ops_dev, uint64_t ops_capacity,
                                 uint64_t* op_offsets_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream, uint64_t* totals_out) {
    return find_segments_device("slamem_find_alns_device", idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands,
                                max_gap, mismatch_penalty, xdrop, max_edits, mems_capacity, segs_dev, segs_capacity, block_offsets_dev,
                                ops_dev, ops_capacity, op_offsets_dev, nullptr, 6, workspace_dev, workspace_bytes, stream, totals_out, end_band);
}

int slamem_find_maps_device(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                            uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty,
                            uint32_t xdrop, uint32_t max_edits, uint64_t mems_capacity, slamem_aln* segs_dev, uint64_t segs_capacity,
                            uint64_t* read_offsets_dev, uint32_t* ops_dev, uint64_t ops_capacity, uint64_t* op_offsets_dev,
                            slamem_map* reads_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream, uint64_t* totals_out) {
    return slamem_find_maps_device_gext(idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands, max_gap,
                                        mismatch_penalty, xdrop, max_edits, 0, mems_capacity, segs_dev, segs_capacity, read_offsets_dev,
                                        ops_dev, ops_capacity, op_offsets_dev, reads_dev, workspace_dev, workspace_bytes, stream, totals_out);
}

int slamem_find_maps_device_gext(const slamem_index* idx, const void* queries_dev, const uint64_t* offsets_dev, uint32_t num_queries,
                                 uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty,
                                 uint32_t xdrop, uint32_t max_edits, uint32_t end_band, uint64_t mems_capacity, slamem_aln* segs_dev,
                                 uint64_t segs_capacity, uint64_t* read_offsets_dev, uint32_t* ops_dev, uint64_t ops_capacity,
                                 uint64_t* op_offsets_dev, slamem_map* reads_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream,
                                 uint64_t* totals_out) {
    return find_segments_device("slamem_find_maps_device", idx, queries_dev, offsets_dev, num_queries, query_bytes, min_len, both_strands,
                                max_gap, mismatch_penalty, xdrop, max_edits, mems_capacity, segs_dev, segs_capacity, read_offsets_dev,
                                ops_dev, ops_capacity, op_offsets_dev, reads_dev, 7, workspace_dev, workspace_bytes, stream, totals_out, end_band);
}

// -aln and -paf for a caller with host memory (reads_out: -paf; then the offsets are per read).  Four attempts: the -mem rows,
// the segments and the operations may each not fit once.
static int find_segments_host(const char* who, const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                              uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop,
                              uint32_t max_edits, slamem_aln** segs_out, uint64_t** offsets_out, uint32_t** ops_out,
                              uint64_t** op_offsets_out, slamem_map** reads_out, uint64_t* totals_out, uint32_t end_band) {
    *segs_out = nullptr; *offsets_out = nullptr; *ops_out = nullptr; *op_offsets_out = nullptr;
    if (reads_out) *reads_out = nullptr;
    totals_out[0] = totals_out[1] = totals_out[2] = 0;
    FilterParams checked;
    if (int bad = resolve_filter_params(who, 0, max_gap, mismatch_penalty, xdrop, max_edits, &checked)) return bad;
    if (int bad = set_end_band(who, end_band, &checked)) return bad;
    const uint64_t qbytes = offsets[num_queries] - offsets[0];
    const uint64_t num_blocks = (uint64_t)num_queries * (both_strands ? 2u : 1u);
    const uint64_t noff = (reads_out ? (uint64_t)num_queries : num_blocks) + 1;  // offsets that go back
    const char* q0 = queries ? queries + offsets[0] : nullptr;
    HostArray<uint64_t> rel = host_array<uint64_t>((uint64_t)num_queries + 1);
    if (!rel) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    for (uint64_t i = 0; i <= num_queries; i++) rel[i] = offsets[i] - offsets[0];
    uint64_t cap = 2 * qbytes / (min_len ? min_len : 1) + 4 * num_blocks + 1024;  // the -mem list
    uint64_t scap = num_blocks + 1024, ocap = 4 * num_blocks + 4096;                // segments, operations
    DevBuf<char> d_q, d_ws;
    DevBuf<uint64_t> d_off, d_boff, d_ooff;
    DevBuf<slamem_aln> d_segs;
    DevBuf<uint32_t> d_ops;
    DevBuf<slamem_map> d_reads;
    SLAMEM_HIP(hipSetDevice(idx->device));
    SLAMEM_TRY(d_q.reserve(qbytes + 16));
    SLAMEM_TRY(d_off.reserve((uint64_t)num_queries + 1));
    SLAMEM_TRY(d_boff.reserve(noff));
    if (reads_out) SLAMEM_TRY(d_reads.reserve((uint64_t)num_queries + 1));
    if (qbytes) SLAMEM_HIP(hipMemcpy(d_q.get(), q0, qbytes, hipMemcpyHostToDevice));
    SLAMEM_HIP(hipMemcpy(d_off.get(), rel.get(), ((uint64_t)num_queries + 1) * 8, hipMemcpyHostToDevice));
    int rc = SLAMEM_OK;
    for (int attempt = 0; attempt < 4; attempt++) {
        uint64_t ws_bytes = 0;
        SLAMEM_TRY(filter_workspace_bytes(reads_out ? "slamem_find_maps_workspace_bytes" : "slamem_find_alns_workspace_bytes", reads_out ? 7 : 6,
                                          num_queries, both_strands, qbytes, cap, ocap, max_edits, &ws_bytes, end_band));
        SLAMEM_TRY(d_segs.reserve(scap + 1));
        SLAMEM_TRY(d_ops.reserve(ocap + 1));
        SLAMEM_TRY(d_ooff.reserve(scap + 2));
        SLAMEM_TRY(d_ws.reserve(ws_bytes));
        rc = find_segments_device(reads_out ? "slamem_find_maps_device" : "slamem_find_alns_device", idx, d_q.get(), d_off.get(), num_queries,
                                  qbytes, min_len, both_strands, max_gap, mismatch_penalty, xdrop, max_edits, cap, d_segs.get(), scap,
                                  d_boff.get(), d_ops.get(), ocap, d_ooff.get(), d_reads.get(), reads_out ? 7 : 6, d_ws.get(), ws_bytes, nullptr,
                                  totals_out, end_band);
        if (rc != SLAMEM_ERR_CAPACITY) break;
        d_segs.release(); d_ops.release(); d_ooff.release(); d_ws.release();  // all of the old before any of the new
        if (totals_out[0] > cap) cap = totals_out[0] + 1024;
        if (totals_out[1] > scap) scap = totals_out[1] + 1024;
        if (totals_out[2] > ocap) ocap = totals_out[2] + 1024;
    }
    if (rc) return rc;
    HostArray<slamem_aln> h_segs = host_array<slamem_aln>(totals_out[1] + 1);
    HostArray<uint64_t> h_boff = host_array<uint64_t>(noff), h_ooff = host_array<uint64_t>(totals_out[1] + 1);
    HostArray<uint32_t> h_ops = host_array<uint32_t>(totals_out[2] + 1);
    HostArray<slamem_map> h_reads;
    if (reads_out) h_reads = host_array<slamem_map>((uint64_t)num_queries + 1);
    if (!h_segs || !h_boff || !h_ops || !h_ooff || (reads_out && !h_reads)) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    if (totals_out[1]) SLAMEM_HIP(hipMemcpy(h_segs.get(), d_segs.get(), totals_out[1] * sizeof(slamem_aln), hipMemcpyDeviceToHost));
    SLAMEM_HIP(hipMemcpy(h_boff.get(), d_boff.get(), noff * 8, hipMemcpyDeviceToHost));
    if (reads_out && num_queries) SLAMEM_HIP(hipMemcpy(h_reads.get(), d_reads.get(), (uint64_t)num_queries * sizeof(slamem_map), hipMemcpyDeviceToHost));
    if (totals_out[2]) SLAMEM_HIP(hipMemcpy(h_ops.get(), d_ops.get(), totals_out[2] * 4, hipMemcpyDeviceToHost));
    SLAMEM_HIP(hipMemcpy(h_ooff.get(), d_ooff.get(), (totals_out[1] + 1) * 8, hipMemcpyDeviceToHost));
    *segs_out = h_segs.release(); *offsets_out = h_boff.release(); *ops_out = h_ops.release(); *op_offsets_out = h_ooff.release();
    if (reads_out) *reads_out = h_reads.release();
    return SLAMEM_OK;
}

int slamem_find_alns_host(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries, uint32_t min_len,
                          int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits,
                          slamem_aln** segs_out, uint64_t** block_offsets_out, uint32_t** ops_out, uint64_t** op_offsets_out,
                          uint64_t* totals_out) {
    return slamem_find_alns_host_gext(idx, queries, offsets, num_queries, min_len, both_strands, max_gap, mismatch_penalty, xdrop, max_edits, 0,
                                      segs_out, block_offsets_out, ops_out, op_offsets_out, totals_out);
}

int slamem_find_alns_host_gext(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries, uint32_t min_len,
                               int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits,
                               uint32_t end_band, slamem_aln** segs_out, uint64_t** block_offsets_out, uint32_t** ops_out,
                               uint64_t** op_offsets_out, uint64_t* totals_out) {
    if (!idx || !offsets || !segs_out || !block_offsets_out || !ops_out || !op_offsets_out || !totals_out || (num_queries && !queries)) {
        set_error("slamem_find_alns_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    return find_segments_host("slamem_find_alns_host", idx, queries, offsets, num_queries, min_len, both_strands, max_gap, mismatch_penalty,
                              xdrop, max_edits, segs_out, block_offsets_out, ops_out, op_offsets_out, nullptr, totals_out, end_band);
}

int slamem_find_maps_host(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries, uint32_t min_len,
                          int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits,
                          slamem_aln** segs_out, uint64_t** read_offsets_out, uint32_t** ops_out, uint64_t** op_offsets_out,
                          slamem_map** reads_out, uint64_t* totals_out) {
    return slamem_find_maps_host_gext(idx, queries, offsets, num_queries, min_len, both_strands, max_gap, mismatch_penalty, xdrop, max_edits, 0,
                                      segs_out, read_offsets_out, ops_out, op_offsets_out, reads_out, totals_out);
}

int slamem_find_maps_host_gext(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries, uint32_t min_len,
                               int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits,
                               uint32_t end_band, slamem_aln** segs_out, uint64_t** read_offsets_out, uint32_t** ops_out,
                               uint64_t** op_offsets_out, slamem_map** reads_out, uint64_t* totals_out) {
    if (!idx || !offsets || !segs_out || !read_offsets_out || !ops_out || !op_offsets_out || !reads_out || !totals_out || (num_queries && !queries)) {
        set_error("slamem_find_maps_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    return find_segments_host("slamem_find_maps_host", idx, queries, offsets, num_queries, min_len, both_strands, max_gap, mismatch_penalty,
                              xdrop, max_edits, segs_out, read_offsets_out, ops_out, op_offsets_out, reads_out, totals_out, end_band);
}

void slamem_host_free(void* p) { free(p); }

static int find_matches_host(const char* who, const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                             uint32_t min_len, int both_strands, int match_type, slamem_mem** mems_out, uint64_t** block_offsets_out,
                             uint64_t* total_out, uint32_t max_occ, uint32_t max_gap, uint32_t** column_out, uint32_t ext_penalty,
                             uint32_t ext_xdrop);

int slamem_find_mems_host(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                          uint32_t min_len, int both_strands, slamem_mem** mems_out, uint64_t** block_offsets_out,
                          uint64_t* total_out) {
    return find_matches_host("slamem_find_mems_host", idx, queries, offsets, num_queries, min_len, both_strands, 0, mems_out,
                             block_offsets_out, total_out, 0, 0, nullptr, 0, kExtXdropUnset);
}

int slamem_find_mams_host(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                          uint32_t min_len, int both_strands, slamem_mem** mems_out, uint64_t** block_offsets_out,
                          uint64_t* total_out) {
    return find_matches_host("slamem_find_mams_host", idx, queries, offsets, num_queries, min_len, both_strands, 1, mems_out,
                             block_offsets_out, total_out, 0, 0, nullptr, 0, kExtXdropUnset);
}

int slamem_find_mums_host(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                          uint32_t min_len, int both_strands, slamem_mem** mems_out, uint64_t** block_offsets_out,
                          uint64_t* total_out) {
    return find_matches_host("slamem_find_mums_host", idx, queries, offsets, num_queries, min_len, both_strands, 2, mems_out,
                             block_offsets_out, total_out, 0, 0, nullptr, 0, kExtXdropUnset);
}

int slamem_find_smems_host(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                           uint32_t min_len, int both_strands, uint32_t max_occ, slamem_mem** mems_out,
                           uint64_t** block_offsets_out, uint64_t* total_out) {
    return find_matches_host("slamem_find_smems_host", idx, queries, offsets, num_queries, min_len, both_strands, 3, mems_out,
                             block_offsets_out, total_out, max_occ, 0, nullptr, 0, kExtXdropUnset);
}

int slamem_find_chains_host(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                            uint32_t min_len, int both_strands, uint32_t max_gap, slamem_mem** mems_out,
                            uint64_t** block_offsets_out, uint32_t** block_scores_out, uint64_t* total_out) {
    return find_matches_host("slamem_find_chains_host", idx, queries, offsets, num_queries, min_len, both_strands, 4, mems_out,
                             block_offsets_out, total_out, 0, max_gap, block_scores_out, 0, kExtXdropUnset);
}

int slamem_find_exts_host(const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                          uint32_t min_len, int both_strands, uint32_t mismatch_penalty, uint32_t xdrop, slamem_mem** mems_out,
                          uint64_t** block_offsets_out, uint32_t** mismatches_out, uint64_t* total_out) {
    return find_matches_host("slamem_find_exts_host", idx, queries, offsets, num_queries, min_len, both_strands, 5, mems_out,
                             block_offsets_out, total_out, 0, 0, mismatches_out, mismatch_penalty, xdrop);
}

// (column_out: -chain's uint32 per strand block, or -ext's uint32 per returned row.  `who` names the caller in the resolver's
// messages only: the null-argument message has always named slamem_find_mems_host, and callers may match on it)
static int find_matches_host(const char* who, const slamem_index* idx, const char* queries, const uint64_t* offsets, uint32_t num_queries,
                             uint32_t min_len, int both_strands, int match_type, slamem_mem** mems_out, uint64_t** block_offsets_out,
                             uint64_t* total_out, uint32_t max_occ, uint32_t max_gap, uint32_t** column_out, uint32_t ext_penalty,
                             uint32_t ext_xdrop) {
    FilterParams p;
    if (int bad = resolve_filter_params(who, max_occ, max_gap, ext_penalty, ext_xdrop, kAlnEditsUnset, &p)) return bad;
    if (!idx || !offsets || !mems_out || !block_offsets_out || !total_out || (num_queries && !queries)) {
        set_error("slamem_find_mems_host: null argument");
        return SLAMEM_ERR_ARG;
    }
    SLAMEM_HIP(hipSetDevice(idx->device));
    const FilterDesc* filter = filter_for(match_type);
    const bool per_row = filter && filter->column_per_row;  // (the column grows with the capacity)
    const uint64_t qbytes = offsets[num_queries];
    const uint64_t num_blocks = (uint64_t)num_queries * (both_strands ? 2 : 1);
    DevBuf<char> d_q, d_ws;
    DevBuf<uint64_t> d_off, d_boff;
    DevBuf<slamem_mem> d_mems;
    DevBuf<uint32_t> d_score;
    uint64_t cap = qbytes / 16 + 4 * (uint64_t)num_blocks + 1024;  // first guess; grown on SLAMEM_ERR_CAPACITY
    SLAMEM_TRY(d_q.reserve(qbytes + 16));
    SLAMEM_TRY(d_off.reserve((uint64_t)num_queries + 1));
    SLAMEM_TRY(d_boff.reserve(num_blocks + 1));
    if (column_out && !per_row) SLAMEM_TRY(d_score.reserve(num_blocks + 1));
    SLAMEM_HIP(hipMemcpy(d_q.get(), queries, qbytes, hipMemcpyHostToDevice));
    SLAMEM_HIP(hipMemcpy(d_off.get(), offsets, ((uint64_t)num_queries + 1) * 8, hipMemcpyHostToDevice));
    int rc = SLAMEM_OK;
    for (int attempt = 0; attempt < 3; attempt++) {
        const uint64_t ws_bytes = search_workspace_bytes(num_queries, both_strands, qbytes, cap, match_type, p);
        SLAMEM_TRY(d_mems.reserve(cap, 16));
        SLAMEM_TRY(d_ws.reserve(ws_bytes));
        if (column_out && per_row) SLAMEM_TRY(d_score.reserve(cap + 1));
        p.column_dev = d_score.get();
        rc = find_mems_device(idx, d_q.get(), d_off.get(), num_queries, qbytes, min_len, both_strands, match_type, d_mems.get(), cap,
                              d_boff.get(), d_ws.get(), ws_bytes, nullptr, total_out, filter ? &p : nullptr, nullptr);
        if (rc != SLAMEM_ERR_CAPACITY) break;
        d_mems.release(); d_ws.release();  // both of the old before either of the new
        cap = *total_out;
    }
    if (rc) return rc;
    HostArray<slamem_mem> h_mems = host_array<slamem_mem>(*total_out ? *total_out : 1);
    HostArray<uint64_t> h_boff = host_array<uint64_t>(num_blocks + 1);
    HostArray<uint32_t> h_score;
    if (column_out) h_score = host_array<uint32_t>((per_row ? *total_out : num_blocks) + 1);
    if (!h_mems || !h_boff || (column_out && !h_score)) { set_error("out of host memory"); return SLAMEM_ERR_NOMEM; }
    if (*total_out) SLAMEM_HIP(hipMemcpy(h_mems.get(), d_mems.get(), *total_out * sizeof(slamem_mem), hipMemcpyDeviceToHost));
    SLAMEM_HIP(hipMemcpy(h_boff.get(), d_boff.get(), (num_blocks + 1) * 8, hipMemcpyDeviceToHost));
    if (column_out) {
        const uint64_t nscore = per_row ? *total_out : num_blocks;
        if (nscore) SLAMEM_HIP(hipMemcpy(h_score.get(), d_score.get(), nscore * 4, hipMemcpyDeviceToHost));
        *column_out = h_score.release();
    }
    *mems_out = h_mems.release();
    *block_offsets_out = h_boff.release();
    return SLAMEM_OK;
}

}  // extern "C"
