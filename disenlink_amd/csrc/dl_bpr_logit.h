// The pair logit over gathered rows that one wave forms, x(u, k) = sum_f (h_f[u].h_f[k]) exp(z_f[u].z_f[k] / t), in the two
// lane geometries of the ranking trainer (dl_train_bpr.hip) — shared with the hard-negative sampler (dl_sample_hard.hip), so
// that the logit the sampler ranks a candidate by is, bit for bit, the neg_logit the trainer then forms for that pair.
#pragma once
#include "dl_fast.h"

namespace dl {
namespace bpr {

// ---- d = 64, K = 4 NJ: lane l holds the float4s j * 64 + l of a row, i.e. elements 4 (l & 15) .. of factor (l >> 4) + 4 j
template <int NJ>
__device__ __forceinline__ void load_row_d64(const float* __restrict__ T, int node, int lane, float4 (&out)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) out[j] = *reinterpret_cast<const float4*>(T + (size_t)node * (NJ * 256) + (j * 64 + lane) * 4);
}

// -> x(u, k), the same value in every lane; ex[j] = e_f and ttv[j] = (h.h)_f e_f of this lane's factors f = (lane >> 4) + 4 j.
// The sums over the DPP row run in the order of TransposedReduce<16, 8> (xor 8, 4, 2, 1): sampled_d64_kernel's bits
// (dl_train_sampled.hip); then the lane's factors, then (rows 0 + 1) + (rows 2 + 3).
template <int NJ>
__device__ __forceinline__ float logit_d64(const float4 (&uz)[NJ], const float4 (&uh)[NJ], const float4 (&zv)[NJ], const float4 (&hv)[NJ],
                                           float t, float (&ex)[NJ], float (&ttv)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float zz = butterfly_down<8, 1>(fast::dot4_packed(uz[j], zv[j]));
        const float hh = butterfly_down<8, 1>(fast::dot4_packed(uh[j], hv[j]));
        ex[j] = expf(div_t(zz, t));
        ttv[j] = hh * ex[j];
    }
    float term = ttv[0];
    if constexpr (NJ == 2) term += ttv[1];
    return add_xor<32>(add_xor<16>(term));                          // (rows 0 + 1) + (rows 2 + 3): all factors
}

// ---- any K, d: element x = f d + lane + 64 n of a row belongs to lane `lane`; factor f of the pair whose rows start at
// zu, hu, zk, hk -> (h.h)_f e_f with e_f left in ex, and added onto `logit`: per-factor wave all-reduces, the caller walks the
// factors in ascending order (sampled_generic_kernel's order).  The product is rounded before it is added (no contraction
// into an FMA on the running sum: a caller that uses nothing but the sum would otherwise get other bits than one that keeps
// the term as well).
__device__ __forceinline__ float factor_term_generic(const float* zu, const float* hu, const float* zk, const float* hk, int f, int d,
                                                     int lane, float t, float& ex, float& logit) {
#pragma clang fp contract(off)
    float pz = 0.0f, ph = 0.0f;
    for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) {
        pz = fmaf(zu[x], zk[x], pz);
        ph = fmaf(hu[x], hk[x], ph);
    }
    const float zz = wave_allreduce_sum(pz), hh = wave_allreduce_sum(ph);
    ex = expf(div_t(zz, t));
    const float ttv = hh * ex;
    logit = logit + ttv;
    return ttv;
}

}  // namespace bpr
}  // namespace dl
