// prims_shim.hip -- TEST INFRASTRUCTURE ONLY: extern "C" doors to the functions of slamem_amd/csrc/prims.h, so that
// tests/prims.py can call each primitive on its own with raw device pointers (tests/test_gpu_prims.py).  No kernels here:
// the code under test is the product's, linked from libslamem_hip.so.  Everything runs on the null stream; a call that
// did work (tmp != nullptr) synchronises it before returning, so a fault inside a kernel comes back as this call's error.
#include "../../slamem_amd/csrc/prims.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

inline int done(hipError_t e, bool ran) {
    if (!ran) return (int)e;
    hipError_t s = hipStreamSynchronize(nullptr);
    return (int)(e != hipSuccess ? e : s);
}

}  // namespace

extern "C" {

int prims_sort_pairs_u64_u32(void* tmp, uint64_t* tmp_bytes, uint64_t* keys_in, uint64_t* keys_out, uint32_t* vals_in,
                             uint32_t* vals_out, uint64_t n, int begin_bit, int end_bit) {
    size_t b = (size_t)*tmp_bytes;
    hipError_t e = slamem::sort_pairs_u64_u32(tmp, b, keys_in, keys_out, vals_in, vals_out, (size_t)n, begin_bit, end_bit, nullptr);
    *tmp_bytes = b;
    return done(e, tmp != nullptr);
}

// exclusive_scan_u32 takes no size of its tmp: the caller sizes it with scan_u32_tmp_words
uint64_t prims_scan_u32_tmp_words(uint64_t n) { return slamem::scan_u32_tmp_words(n); }

int prims_exclusive_scan_u32(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* tmp) {
    return done(slamem::exclusive_scan_u32(in, out, n, tmp, nullptr), true);
}

int prims_scan_max_inclusive_u32(void* tmp, uint64_t* tmp_bytes, const uint32_t* in, uint32_t* out, uint64_t n) {
    size_t b = (size_t)*tmp_bytes;
    hipError_t e = slamem::scan_max_inclusive_u32(tmp, b, in, out, (size_t)n, nullptr);
    *tmp_bytes = b;
    return done(e, tmp != nullptr);
}

int prims_scan_sum_exclusive_u32_u64(void* tmp, uint64_t* tmp_bytes, const uint32_t* in, uint64_t* out, uint64_t n) {
    size_t b = (size_t)*tmp_bytes;
    hipError_t e = slamem::scan_sum_exclusive_u32_u64(tmp, b, in, out, (size_t)n, nullptr);
    *tmp_bytes = b;
    return done(e, tmp != nullptr);
}

int prims_scan_sum_exclusive_u64(void* tmp, uint64_t* tmp_bytes, const uint64_t* in, uint64_t* out, uint64_t n) {
    size_t b = (size_t)*tmp_bytes;
    hipError_t e = slamem::scan_sum_exclusive_u64(tmp, b, in, out, (size_t)n, nullptr);
    *tmp_bytes = b;
    return done(e, tmp != nullptr);
}

int prims_scan_sum_exclusive_uint4(void* tmp, uint64_t* tmp_bytes, const void* in, void* out, uint64_t n) {
    size_t b = (size_t)*tmp_bytes;
    hipError_t e = slamem::scan_sum_exclusive_uint4(tmp, b, static_cast<const uint4*>(in), static_cast<uint4*>(out), (size_t)n, nullptr);
    *tmp_bytes = b;
    return done(e, tmp != nullptr);
}

int prims_select_flagged_u32(void* tmp, uint64_t* tmp_bytes, const uint32_t* in, const uint8_t* flags, uint32_t* out,
                             uint32_t* count_out, uint64_t n) {
    size_t b = (size_t)*tmp_bytes;
    hipError_t e = slamem::select_flagged_u32(tmp, b, in, flags, out, count_out, (size_t)n, nullptr);
    *tmp_bytes = b;
    return done(e, tmp != nullptr);
}

int prims_select_indices_u32(void* tmp, uint64_t* tmp_bytes, const uint8_t* flags, uint32_t* out, uint32_t* count_out, uint64_t n) {
    size_t b = (size_t)*tmp_bytes;
    hipError_t e = slamem::select_indices_u32(tmp, b, flags, out, count_out, (size_t)n, nullptr);
    *tmp_bytes = b;
    return done(e, tmp != nullptr);
}

}  // extern "C"
