// filters_shim.hip -- TEST INFRASTRUCTURE ONLY: one extern "C" door to the list filters behind K9 (-mum, -smem, -chain:
// FilterDesc::needs_planes == false, they read neither index nor reads), so that tests/filters.py can run a filter on a GIVEN
// -mem list (tests/test_gpu_filter_lists.py).  No kernels here: the code under test is the product's, linked from
// libslamem_hip.so and reached the way the search reaches it -- filter_for, resolve_filter_params, workspace_bytes,
// filter_list_buffers, run, finish.  Everything runs on the null stream and is synchronised before the door returns, so a fault
// inside a kernel comes back as this call's error.
#include "../../slamem_amd/csrc/common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kHipBase = 1000;  // a HIP error of the shim's own calls comes back as kHipBase + hipError_t

struct DevBuf {  // the workspace: freed on every way out
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

const slamem::FilterDesc* list_filter(int match_type) {
    const slamem::FilterDesc* f = slamem::filter_for(match_type);
    return f && !f->needs_planes && !f->segments ? f : nullptr;
}

}  // namespace

extern "C" {

// the filter's workspace for a list of `capacity` rows in `num_blocks` strand blocks (0: not a list filter)
uint64_t filters_workspace_bytes(int match_type, uint64_t num_blocks, uint64_t capacity, uint32_t max_occ, uint32_t max_gap) {
    const slamem::FilterDesc* f = list_filter(match_type);
    slamem::FilterParams params;
    if (!f || slamem::resolve_filter_params(f->name, max_occ, max_gap, 0, slamem::kExtXdropUnset, slamem::kAlnEditsUnset, &params) != SLAMEM_OK)
        return 0;
    const slamem::FilterBatch batch = {nullptr, nullptr, nullptr, num_blocks, 1, 0, capacity};
    return f->workspace_bytes(batch, params);
}

// rows_dev: num_rows -mem rows (num_rows <= capacity), boff_dev: num_blocks + 1 offsets into them.  out_rows_dev: capacity rows,
// out_boff_dev: num_blocks + 1 words, column_dev: a uint32 per block (-chain's scores) or null.  scalars_out[0..1]: what run()
// sent to the host ([1] of -mum: its large blocks, before finish()); *total_out: the rows kept (-mum: after finish()).
// Returns the SLAMEM_* code of the filter, or kHipBase + the hipError_t of a call of the shim's own.
int filters_run(int match_type, const void* rows_dev, const uint64_t* boff_dev, uint64_t num_rows, uint64_t num_blocks, uint64_t capacity,
                uint32_t max_occ, uint32_t max_gap, void* out_rows_dev, uint64_t* out_boff_dev, uint32_t* column_dev,
                unsigned long long* scalars_out, uint64_t* total_out) {
    const slamem::FilterDesc* f = list_filter(match_type);
    if (!f || !scalars_out || !total_out || num_rows > capacity || capacity >= f->capacity_end) return SLAMEM_ERR_ARG;
    slamem::FilterParams params;
    int rc = slamem::resolve_filter_params(f->name, max_occ, max_gap, 0, slamem::kExtXdropUnset, slamem::kAlnEditsUnset, &params);
    if (rc != SLAMEM_OK) return rc;
    params.column_dev = column_dev;
    const slamem::FilterBatch batch = {nullptr, nullptr, nullptr, num_blocks, 1, 0, capacity};
    DevBuf ws;
    hipError_t e = hipMalloc(&ws.p, f->workspace_bytes(batch, params));
    if (e != hipSuccess) return kHipBase + (int)e;
    slamem_mem* rows = nullptr;
    uint64_t* boff = nullptr;
    slamem::filter_list_buffers(ws.p, num_blocks, capacity, &rows, &boff);
    if (num_rows && (e = hipMemcpyAsync(rows, rows_dev, num_rows * sizeof(slamem_mem), hipMemcpyDeviceToDevice, nullptr)) != hipSuccess)
        return kHipBase + (int)e;
    if ((e = hipMemcpyAsync(boff, boff_dev, (num_blocks + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, nullptr)) != hipSuccess)
        return kHipBase + (int)e;
    scalars_out[0] = scalars_out[1] = 0;
    rc = f->run(ws.p, batch, params, static_cast<slamem_mem*>(out_rows_dev), out_boff_dev, scalars_out, nullptr);
    e = hipStreamSynchronize(nullptr);
    if (rc != SLAMEM_OK) return rc;
    if (e != hipSuccess) return kHipBase + (int)e;
    *total_out = scalars_out[0];
    if (f->finish && scalars_out[1]) {
        rc = f->finish(ws.p, batch, scalars_out[1], static_cast<slamem_mem*>(out_rows_dev), out_boff_dev, nullptr, total_out);
        e = hipStreamSynchronize(nullptr);
        if (rc != SLAMEM_OK) return rc;
        if (e != hipSuccess) return kHipBase + (int)e;
    }
    return SLAMEM_OK;
}

}  // extern "C"
