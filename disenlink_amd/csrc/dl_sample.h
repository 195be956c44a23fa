// The draw of the device samplers (dl_sample.hip, dl_sample_hard.hip): Philox4x32-10 written out and the rejection rule of
// dl_sample_negatives, as one __device__ function both kernels call, so that both draw the same bits.
#pragma once
#include "dl_common.h"

namespace dl {

constexpr int SAMPLE_ATTEMPTS = 64;

__device__ __forceinline__ uint32_t philox4x32_10_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                        uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// One partner for the source u of entry e: at most SAMPLE_ATTEMPTS words of counter (e, counter1 + attempt, epoch low, epoch
// high), k = (word * N) >> 32, rejected while k stands in the exclusion row of u (ascending columns) or, with exclude_self,
// while k == u.  -1 once the attempts are spent, and for a u outside [0, N), whose row is never read.
__device__ __forceinline__ int sample_partner(uint32_t e, uint32_t counter1, uint64_t epoch, uint32_t seed_lo, uint32_t seed_hi, int u,
                                              int N, const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col,
                                              int exclude_self) {
    if (u < 0 || u >= N) return -1;                                     // (a source outside the table: a failed entry, never a read)
    const int beg = ex_rowptr ? ex_rowptr[u] : 0, end = ex_rowptr ? ex_rowptr[u + 1] : 0;
    for (int attempt = 0; attempt < SAMPLE_ATTEMPTS; ++attempt) {
        const uint32_t word = philox4x32_10_word0(e, counter1 + (uint32_t)attempt, (uint32_t)epoch, (uint32_t)(epoch >> 32), seed_lo,
                                                  seed_hi);
        const int k = (int)(((uint64_t)word * (uint64_t)(uint32_t)N) >> 32);
        bool bad = exclude_self && k == u;
        int lo = beg, hi = end;                                         // first column >= k of the row
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (ex_col[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        bad = bad || (lo < end && ex_col[lo] == k);
        if (!bad) return k;
    }
    return -1;
}

}  // namespace dl
