// lowq_filter.hip -- the low-quality mask of a batch: a bit per letter of the batch's letter buffer, set where
// the letter's base quality is below the threshold.  Letter j is low iff max(0, qual[j] - phred_offset) < min_bq; bit j is bit
// j % 64 of word j / 64, and the unused bits of the last word are 0.  The mask knows nothing of reads: the masked add
// (pile_filter.hip) finds a read's bits at its offset.
//   k_lowq_pack            quality bytes in device memory -> the mask: a lane per letter, a wave ballot per word
//   slamem_pack_lowq       the same on the host (what a front end puts in front of slamem_stream_submit_masked: the link then
//                          carries an eighth of a byte per letter)
#include "common.h"

#include <thread>
#include <vector>

namespace slamem {

namespace {

constexpr unsigned kLowqGrid = 4096;  // workgroups of four waves; a wave takes words blockIdx * 4 + wave, + 4 * gridDim, ...

// a wave per word: lane i reads byte 64 w + i (the wave 64 consecutive bytes), the ballot is the word, lane 0 writes it.  Lanes
// behind `total` read nothing and vote 0, so the tail word's unused bits are 0; nothing at or behind word (total + 63) / 64 is
// written.
__global__ void __launch_bounds__(256) k_lowq_pack(const unsigned char* __restrict__ quals, uint64_t total, uint32_t min_bq,
                                                   uint32_t phred_offset, uint64_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t words = (total + 63u) >> 6;
    for (uint64_t w = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); w < words; w += (uint64_t)gridDim.x * 4u) {  // (wave-uniform)
        const uint64_t j = w * 64u + lane;
        bool low = false;
        if (j < total) {
            const uint32_t v = quals[j];
            low = (v > phred_offset ? v - phred_offset : 0u) < min_bq;
        }
        const unsigned long long word = __ballot(low);
        if (lane == 0u) out[w] = word;
    }
}

bool lowq_args_ok(const char* who, uint32_t min_bq, uint32_t phred_offset) {
    if (min_bq > 93u) { set_error("%s: the minimum base quality is 0 to 93, not %u", who, min_bq); return false; }
    if (phred_offset > 126u) { set_error("%s: the quality offset is 0 to 126, not %u", who, phred_offset); return false; }
    return true;
}

}  // namespace

}  // namespace slamem

using namespace slamem;

extern "C" {

int slamem_pack_lowq_device(const void* quals_dev, uint64_t total_letters, uint32_t min_bq, uint32_t phred_offset, uint64_t* mask_out_dev,
                            void* stream) {
    if (total_letters && (!quals_dev || !mask_out_dev)) { set_error("slamem_pack_lowq_device: null argument"); return SLAMEM_ERR_ARG; }
    if (!lowq_args_ok("slamem_pack_lowq_device", min_bq, phred_offset)) return SLAMEM_ERR_ARG;
    if (total_letters == 0) return SLAMEM_OK;
    const uint64_t words = (total_letters + 63u) >> 6, groups = (words + 3u) / 4u;
    hipLaunchKernelGGL(k_lowq_pack, dim3((unsigned)(groups < kLowqGrid ? groups : kLowqGrid)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned char*>(quals_dev), total_letters, min_bq, phred_offset, mask_out_dev);
    SLAMEM_HIP(hipGetLastError());
    return SLAMEM_OK;
}

int slamem_pack_lowq(const char* quals, uint64_t total_letters, uint32_t min_bq, uint32_t phred_offset, uint64_t* mask_out, int threads) {
    if (total_letters && (!quals || !mask_out)) { set_error("slamem_pack_lowq: null argument"); return SLAMEM_ERR_ARG; }
    if (!lowq_args_ok("slamem_pack_lowq", min_bq, phred_offset)) return SLAMEM_ERR_ARG;
    const uint64_t words = (total_letters + 63u) >> 6;
    const unsigned char* q = reinterpret_cast<const unsigned char*>(quals);
    auto work = [&](uint64_t w0, uint64_t w1) {
        for (uint64_t w = w0; w < w1; w++) {
            const uint64_t at = w * 64u, n = total_letters - at < 64u ? total_letters - at : 64u;
            uint64_t word = 0;
            for (uint64_t i = 0; i < n; i++) {
                const uint32_t v = q[at + i];
                word |= (uint64_t)((v > phred_offset ? v - phred_offset : 0u) < min_bq) << i;
            }
            mask_out[w] = word;
        }
    };
    const int nt = threads < 1 ? 1 : threads > 64 ? 64 : threads;
    if (nt == 1 || words < 65536u) work(0, words);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++) th.emplace_back(work, words * (uint64_t)t / (uint64_t)nt, words * (uint64_t)(t + 1) / (uint64_t)nt);
        for (auto& x : th) x.join();
    }
    return SLAMEM_OK;
}

}  // extern "C"
