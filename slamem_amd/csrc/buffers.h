// buffers.h -- the two owning buffer types of the host code (internal, host only): device memory and pinned host memory that
// is freed by its owner's destructor and grows only.  Ownership is written here once: a function that holds its memory in these
// may return early, and a struct of them needs no list of frees.
#pragma once
#include "common.h"

#include <memory>
#include <stdlib.h>

namespace slamem {

struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void* p) { return hipFree(p); }
    static constexpr const char* kCall = "hipMalloc(&p, bytes)";
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
    static constexpr const char* kCall = "hipHostMalloc(&p, bytes, hipHostMallocDefault)";
};

template <typename T, typename Mem>
class Buf {
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }

    T* get() const { return p_; }
    uint64_t count() const { return n_; }  // elements last reserved (0: no buffer)

    // Room for `count` elements and `pad_bytes` behind them (kernels read whole aligned words past the logical end).  Nothing
    // happens if the buffer holds that many; otherwise the old memory goes BEFORE the new is asked for -- a batch's buffers are up
    // to gigabytes, and the two must never exist side by side -- and the content is lost.  A failed allocation leaves no buffer;
    // its message names the call site.
    int reserve(uint64_t count, uint64_t pad_bytes = 0, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
        if (p_ && n_ >= count) return SLAMEM_OK;
        release();
        void* p = nullptr;
        const hipError_t e = Mem::alloc(&p, count * sizeof(T) + pad_bytes);
        if (e != hipSuccess) return hip_fail(e, Mem::kCall, file, line);
        p_ = static_cast<T*>(p);
        n_ = count;
        return SLAMEM_OK;
    }
    void release() {
        if (p_) (void)Mem::free(p_);
        p_ = nullptr;
        n_ = 0;
    }

private:
    T* p_ = nullptr;
    uint64_t n_ = 0;
};

template <typename T> using DevBuf = Buf<T, DeviceMem>;
template <typename T> using PinnedBuf = Buf<T, PinnedMem>;

// A malloc'ed array on its way to a caller of the C interface, who frees it with slamem_host_free: free()d here unless
// release()d to the caller.  host_array gives a null one when the memory is not to be had.
struct HostFree {
    void operator()(void* p) const { free(p); }
};
template <typename T> using HostArray = std::unique_ptr<T[], HostFree>;
template <typename T> HostArray<T> host_array(uint64_t count) { return HostArray<T>(static_cast<T*>(malloc(count * sizeof(T)))); }

// `return rc` of a reserve (or of any call that gives a SLAMEM_* code) unless it is SLAMEM_OK
#define SLAMEM_TRY(call)                       \
    do {                                       \
        const int rc__ = (call);               \
        if (rc__ != SLAMEM_OK) return rc__;    \
    } while (0)

}  // namespace slamem
