// Structured training negatives drawn on the device (dl_sample_negatives): one thread per entry, counter-based randomness.
//
// Entry e = r * m + j pairs the source src[r] of training edge row r with a partner k drawn uniformly over [0, N), rejected
// while (src[r], k) stands in the exclusion CSR (ascending columns per row: the pair_exclusion normal form the scans read)
// or, with exclude_self, while k == src[r].  That is the rule of splits.structured_negatives: an edge row of the whole
// dataset — validation and test rows included — is never a negative.
//
// Randomness: Philox4x32-10 (Salmon et al., SC'11) written out below, key = the two halves of `seed`, counter =
// (e, attempt, epoch low, epoch high); k = (uint64(word 0) * N) >> 32.  The draw is therefore a pure function of
// (seed, epoch, e): it does not depend on the grid, on wave order or on which call makes it.  The multiply-high map is
// biased by at most N / 2^32 per value (a value receives floor or ceil of 2^32 / N of the 2^32 words).
// `epoch` is read from device memory: the training loop advances it with a tensor add, no host value changes between epochs.
// At most DL_SAMPLE_ATTEMPTS = 64 attempts per entry; an entry that exhausts them writes k = -1 and adds 1 to *n_failed
// (an integer atomic: the sum does not depend on order) and the trainers give it weight 0.
// Duplicated draws inside an epoch are KEPT as separate entries (the fixed split de-duplicates; here nothing does).
#include "dl_sample.h"

namespace dl {

// (Philox and the rejection rule: sample_partner, dl_sample.h — shared with dl_sample_hard.hip, whose candidate 0 is this draw)
__global__ __launch_bounds__(BLOCK) void sample_negatives_kernel(const int32_t* __restrict__ src, int n_rows, int m, int N,
                                                                 const int32_t* __restrict__ ex_rowptr,
                                                                 const int32_t* __restrict__ ex_col, uint32_t seed_lo,
                                                                 uint32_t seed_hi, const uint64_t* __restrict__ epoch_dev,
                                                                 int exclude_self, int32_t* __restrict__ k_out,
                                                                 uint32_t* __restrict__ n_failed) {
    const long long e = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= (long long)n_rows * m) return;
    const uint64_t epoch = epoch_dev[0];
    const int result = sample_partner((uint32_t)e, 0u, epoch, seed_lo, seed_hi, src[e / m], N, ex_rowptr, ex_col, exclude_self);
    k_out[e] = result;
    if (result < 0) atomicAdd(n_failed, 1u);
}

}  // namespace dl

extern "C" int dl_sample_negatives(const int32_t* src, int n_rows, int m, int N, const int32_t* ex_rowptr,
                                   const int32_t* ex_col, uint64_t seed, const uint64_t* epoch_dev, int exclude_self,
                                   int32_t* k_out, uint32_t* n_failed, void* stream) {
    using namespace dl;
    DL_REQUIRE(n_rows >= 0 && m >= 1 && N >= 1, "dl_sample_negatives: n_rows=%d m=%d N=%d", n_rows, m, N);
    DL_REQUIRE((long long)n_rows * m <= 0x7fffffffLL, "dl_sample_negatives: %d x %d entries exceed 2^31 - 1", n_rows, m);
    DL_REQUIRE(epoch_dev != nullptr && n_failed != nullptr, "NULL argument");
    if (n_rows == 0) return DL_OK;
    DL_REQUIRE(src && k_out, "NULL argument");
    const long long n = (long long)n_rows * m;
    hipLaunchKernelGGL(sample_negatives_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                       src, n_rows, m, N, ex_rowptr, ex_col, (uint32_t)seed, (uint32_t)(seed >> 32), epoch_dev, exclude_self,
                       k_out, n_failed);
    return check_launch("dl_sample_negatives");
}
