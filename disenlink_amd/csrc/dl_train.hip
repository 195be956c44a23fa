// One-pass training scorer in probability space (the kernels: dl_train.h) and the pair-list BCE of either score space.
// (one of the tuned-kernel translation units; the shared pieces and the design notes are in dl_fast.h)
#include "dl_train.h"

namespace dl {
namespace fast {

// ---------------------------------------------------------------------------- pair-list BCE
// loss = sum_q w[q] * bce(prob[q], y[q]),  g[q] = dloss/dprob[q], in PROBABILITY space exactly as
// F.binary_cross_entropy does it (main_disentangled.py:195): log clamped at -100, gradient
// (p - y) / max(p (1 - p), 1e-12).  Saturated fp32 sigmoids keep their zero gradient downstream because the
// scorer backward multiplies by p (1 - p).  Deterministic two-stage reduction (no float atomics).
constexpr int BCE_BLOCKS = 1024;     // 4 workgroups per CU (256 left one: 12.8 us for 1.1M pairs, latency-bound)

__global__ __launch_bounds__(BLOCK) void pair_bce_kernel(const float* __restrict__ prob, const float* __restrict__ y,
                                                         const float* __restrict__ w, int n, float* __restrict__ g,
                                                         float* __restrict__ partial) {
    __shared__ float red[WAVES_PER_BLOCK];
    float acc = 0.0f;
    for (int q = blockIdx.x * BLOCK + threadIdx.x; q < n; q += BCE_BLOCKS * BLOCK) {
        const float p = prob[q], yy = y[q], ww = w[q];
        // a NaN probability must stay visible as a NaN loss (fmaxf would turn its log into -100 and hide it; torch's
        // BCE refuses such input outright)
        const float lg = logf(p), lg1 = logf(1.0f - p);
        const float lp = lg < -100.0f ? -100.0f : lg, l1p = lg1 < -100.0f ? -100.0f : lg1;
        // weight 0 = "not part of the loss" (e.g. validation pairs riding along): exactly nothing, even for a NaN p
        acc += ww == 0.0f ? 0.0f : ww * -(yy * lp + (1.0f - yy) * l1p);
        g[q] = ww == 0.0f ? 0.0f : ww * (p - yy) / fmaxf(p * (1.0f - p), 1e-12f);
    }
    acc = wave_allreduce_sum(acc);
    if (lane_id() == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
        for (int i = 1; i < WAVES_PER_BLOCK; ++i) t += red[i];
        partial[blockIdx.x] = t;
    }
}

// The same loss in LOGIT space (dl_pair_bce_logits): loss = sum_q w[q] (max(x, 0) - x y + log1p(exp(-|x|))), g[q] = d loss / d x[q] =
// w[q] (sigma(x) - y) through sigmoid_minus_label — no log of a rounded probability, no clamp, a gradient for every finite x.
// max(x, 0) - x y is formed as (1 - y) max(x, 0) + y max(-x, 0) with a zero factor dropping its term: the same value for every
// finite x (one rounding apart), and x = +-inf costs 0 under the agreeing label and inf under the other instead of inf - inf.
// Same grid, same 1,024 fixed-order partial sums and the same finish kernel as pair_bce_kernel.
__global__ __launch_bounds__(BLOCK) void pair_bce_logits_kernel(const float* __restrict__ logit, const float* __restrict__ y,
                                                                const float* __restrict__ w, int n, float* __restrict__ g,
                                                                float* __restrict__ partial) {
    __shared__ float red[WAVES_PER_BLOCK];
    float acc = 0.0f;
    for (int q = blockIdx.x * BLOCK + threadIdx.x; q < n; q += BCE_BLOCKS * BLOCK) {
        const float x = logit[q], yy = y[q], ww = w[q];
        const float ny = 1.0f - yy;
        const float lin = (ny == 0.0f ? 0.0f : ny * fmaxf(x, 0.0f)) + (yy == 0.0f ? 0.0f : yy * fmaxf(-x, 0.0f));
        // (x != x keeps a NaN logit visible: fmaxf drops it)
        const float l = x != x ? x : lin + log1pf(expf(-fabsf(x)));
        // weight 0 = "not part of the loss": exactly nothing, even for a NaN logit
        acc += ww == 0.0f ? 0.0f : ww * l;
        g[q] = ww == 0.0f ? 0.0f : ww * sigmoid_minus_label(x, yy);
    }
    acc = wave_allreduce_sum(acc);
    if (lane_id() == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
        for (int i = 1; i < WAVES_PER_BLOCK; ++i) t += red[i];
        partial[blockIdx.x] = t;
    }
}

__global__ void pair_bce_finish_kernel(const float* __restrict__ partial, float* __restrict__ loss) {
    const int lane = threadIdx.x;                           // one wave
    float acc = 0.0f;
    for (int i = lane; i < BCE_BLOCKS; i += DL_WAVE) acc += partial[i];
    acc = wave_allreduce_sum(acc);
    if (lane == 0) loss[0] = acc;
}

}  // namespace fast

int pair_bce(const float* prob, const float* y, const float* w, int n, float* loss, float* g, float* partial,
             hipStream_t st) {
    hipLaunchKernelGGL(fast::pair_bce_kernel, dim3(fast::BCE_BLOCKS), dim3(BLOCK), 0, st, prob, y, w, n, g, partial);
    hipLaunchKernelGGL(fast::pair_bce_finish_kernel, dim3(1), dim3(DL_WAVE), 0, st, partial, loss);
    return check_launch("pair_bce");
}

int pair_bce_logits(const float* logit, const float* y, const float* w, int n, float* loss, float* g, float* partial,
                    hipStream_t st) {
    hipLaunchKernelGGL(fast::pair_bce_logits_kernel, dim3(fast::BCE_BLOCKS), dim3(BLOCK), 0, st, logit, y, w, n, g, partial);
    hipLaunchKernelGGL(fast::pair_bce_finish_kernel, dim3(1), dim3(DL_WAVE), 0, st, partial, loss);
    return check_launch("pair_bce_logits");
}

int fast_score_pairs_train(const dl_pair_incidence* inc, const void* Z, const void* H, int K, int d, int dtype, float t,
                           const float* y, const float* w, float* prob, float* dZ, float* dH, float* part, hipStream_t st) {
    return score_pairs_train_space<false>(inc, Z, H, K, d, dtype, t, y, w, prob, dZ, dH, part, st);
}

}  // namespace dl
