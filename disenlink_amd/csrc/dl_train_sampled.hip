// Training scorer over SAMPLED partners (dl_score_sampled_train, dl_score_sampled_train_logits): the negatives of an epoch
// drawn by dl_sample_negatives, trained without a plan build.
//
// Entry e pairs u_e = src[e / m] (src ascending: the u side is a fixed CSR, u_rowptr counts ENTRIES) with the partner k[e]
// (-1 = a failed draw: weight 0), label 0, weight w:
//   x_e = sum_f (h_f[u].h_f[k]) exp(z_f[u].z_f[k] / t),    loss = sum_e  -w max(log(1 - sigma(x)), -100)     (probability space)
//                                                                        w (max(x, 0) + log1p(exp(-|x|)))   (logit space)
// and dZ, dH = d loss / d (Z, H), every pair in BOTH endpoints' rows, without float atomics:
//   pass A (row side): the entry list is cut into chunks of SEG = 64 consecutive entries, one wave per chunk.  The wave walks
//     its entries in order, gathers z[k], h[k], forms the score and the 2K coefficients c_f = g e_f, b_f = g (h.h)_f e_f / t
//     (g = d loss / d x; the arithmetic of score_train_wave_kernel, dl_train.h, clamps included), writes both to memory and
//     accumulates dH[u] += c_f h_f[k], dZ[u] += b_f z_f[k] on chip.  Where the row changes inside the chunk the sum is written
//     out: straight to the row's place if the whole row lies inside the chunk, else to one of the chunk's two partial slots
//     (2 chunk: the row began in an earlier chunk; 2 chunk + 1: it began here and goes on).
//   pass B (partner side): the same walk over `order` (the stable ascending sort of k, the -1 entries first and skipped)
//     with k_rowptr [N+1]: reads the coefficients, gathers z[u], h[u], accumulates dH[k] += c_f h_f[u], dZ[k] += b_f z_f[u].
//     A partner nobody names has no entries; one with more than 64 spans chunks and sums through the slots.
//   finish: one wave per node: B (direct row or its partial slots in chunk order) + A (likewise), B first, written to dZ / dH or
//     added onto them (accumulate != 0: the positive list's gradients and these sum without another launch).  Rows without an
//     entry on either side read exactly 0 (or stay what they were when accumulating).
// Every sum has a fixed order that depends on the lists alone: the same bits on every call, whatever the grid.
// k == u is legal: both passes then contribute to the same row, which is simply the sum.
//
// Kernels: d = 64 with K in {4, 8} (K = 8 is the benchmark's form) takes the lane geometry of score_train_wave_kernel — lane l
// holds float4 number j * 64 + l of a row, a DPP row of 16 lanes holds one factor slice, the per-factor dot products are
// butterflies over the DPP row in the order of that kernel's transposed reduction and the factors are added in its order:
// the scores are its bits.  The other tuned fp32 shapes but K = 16, d = 128 run pass A in the lane geometry of their own pair-list
// trainer (sampled_geo_kernel: its bits again); every other fp32 shape with K d <= 2048 takes the generic kernels
// (accumulators in LDS).
#include "dl_fast.h"

namespace dl {
namespace sampled {

using fast::dot4_packed;
using fast::store4;

constexpr int SEG = 64;                 // entries per chunk = lanes of the wave that preloads their indices
constexpr float FMAX = 3.402823466e38f;
constexpr int LOSS_BLOCKS = 1024;

struct Lists {
    const int32_t* src;                 // [n_rows] ascending
    const int32_t* k;                   // [E]
    const int32_t* order;               // [E] (pass B)
    const int32_t* rowptr;              // [N+1] of the side walked, in list positions
    int m, E, N;
};

// the indices of the chunk's entries, one per lane: (entry, row walked, partner gathered); row = -1: skipped
template <bool SIDE_B>
__device__ __forceinline__ void load_chunk(const Lists& L, int pos0, int lane, int& my_e, int& my_row, int& my_partner) {
    my_e = 0;
    my_row = -1;
    my_partner = -1;
    const int pos = pos0 + lane;
    if (pos < L.E) {
        int e = pos;
        if constexpr (SIDE_B) e = L.order[pos];
        if (e >= 0 && e < L.E) {
            int u = L.src[e / L.m], k = L.k[e];
            if (u < 0 || u >= L.N) u = -1;
            if (k < 0 || k >= L.N) k = -1;
            my_e = e;
            if constexpr (SIDE_B) {
                my_row = u < 0 ? -1 : k;
                my_partner = u;
            } else {
                my_row = u;
                my_partner = k;
            }
        }
    }
}

// where the sum of row `cur` over this chunk goes: its own place, or one of the chunk's two slots
__device__ __forceinline__ float* flush_dst(const Lists& L, int cur, int chunk, int pos0, float* buf, float* part, int ROW) {
    const int rb = L.rowptr[cur], re = L.rowptr[cur + 1];
    const bool before = rb < pos0, after = re > pos0 + SEG;
    if (!before && !after) return buf + (size_t)cur * 2 * ROW;
    return part + ((size_t)2 * chunk + (before ? 0 : 1)) * 2 * ROW;
}

// g = d loss / d x of a negative with weight w, and the stored score
template <bool LOGIT>
__device__ __forceinline__ float grad_coef(float logit, float w, float& p) {
    if constexpr (LOGIT) {
        p = logit;
        return w == 0.0f ? 0.0f : w * sigmoid_minus_label(logit, 0.0f);
    } else {
        p = sigmoid_ref(logit);
        const float pr = p * (1.0f - p);                            // dl_pair_bce's gradient times the sigmoid backward
        return w == 0.0f ? 0.0f : w * p * (pr >= 1e-12f ? 1.0f : pr * 1e12f);
    }
}

// ---------------------------------------------------------------------------- d = 64, K = 4 NJ
template <int NJ, bool LOGIT, bool SIDE_B>
__global__ __launch_bounds__(BLOCK) void sampled_d64_kernel(const float* __restrict__ Z, const float* __restrict__ H, float t,
                                                            Lists L, float w, float* __restrict__ score, float* rec,
                                                            float* __restrict__ buf, float* __restrict__ part) {
    constexpr int K = 4 * NJ, ROW = K * 64;
    const int wave = wave_index(), lane = lane_id();
    const int chunk = blockIdx.x * WAVES_PER_BLOCK + wave;
    const int pos0 = chunk * SEG;
    if (pos0 >= L.E) return;                                        // (no barrier in this kernel)
    const int n = min(SEG, L.E - pos0);
    int my_e, my_row, my_partner;
    load_chunk<SIDE_B>(L, pos0, lane, my_e, my_row, my_partner);
    const int fbase = lane >> 4;                                    // this lane's factors: fbase + 4 j
    float4 az[NJ], ah[NJ], uz[NJ], uh[NJ];
    int cur = -1;
    auto flush = [&]() {
        float* dst = flush_dst(L, cur, chunk, pos0, buf, part, ROW);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            store4(dst + 4 * (j * 64 + lane), az[j]);
            store4(dst + ROW + 4 * (j * 64 + lane), ah[j]);
        }
    };
    for (int s = 0; s < n; ++s) {
        const int e = __builtin_amdgcn_readlane(my_e, s), row = __builtin_amdgcn_readlane(my_row, s);
        const int v = __builtin_amdgcn_readlane(my_partner, s);
        if (row < 0) {                                              // pass A: a source outside the table; pass B: a failed draw
            if constexpr (!SIDE_B) {
                if (pos0 + s < L.E && lane == 0) score[pos0 + s] = 0.0f;
                if (lane < 2 * K) rec[(size_t)(pos0 + s) * 2 * K + lane] = 0.0f;
            }
            continue;
        }
        if (row != cur) {
            if (cur >= 0) flush();
            cur = row;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                az[j] = ah[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (!SIDE_B) {
                    uz[j] = *reinterpret_cast<const float4*>(Z + (size_t)row * ROW + (j * 64 + lane) * 4);
                    uh[j] = *reinterpret_cast<const float4*>(H + (size_t)row * ROW + (j * 64 + lane) * 4);
                }
            }
        }
        float c[NJ], b[NJ];
        if constexpr (!SIDE_B) {
            if (v < 0) {                                            // a failed draw: weight 0, score 0, nothing gathered
                if (lane == 0) score[e] = 0.0f;
                if (lane < 2 * K) rec[(size_t)e * 2 * K + lane] = 0.0f;
                continue;
            }
        }
        float4 zv[NJ], hv[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            zv[j] = *reinterpret_cast<const float4*>(Z + (size_t)v * ROW + (j * 64 + lane) * 4);
            hv[j] = *reinterpret_cast<const float4*>(H + (size_t)v * ROW + (j * 64 + lane) * 4);
        }
        if constexpr (SIDE_B) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                c[j] = rec[(size_t)e * 2 * K + fbase + 4 * j];
                b[j] = rec[(size_t)e * 2 * K + K + fbase + 4 * j];
            }
        } else {
            float ex[NJ], ttv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                // sums over the DPP row in the order of TransposedReduce<16, 8> (xor 8, 4, 2, 1): score_train_wave_kernel's bits
                const float zz = butterfly_down<8, 1>(dot4_packed(uz[j], zv[j]));
                const float hh = butterfly_down<8, 1>(dot4_packed(uh[j], hv[j]));
                ex[j] = expf(div_t(zz, t));
                ttv[j] = hh * ex[j];
            }
            float term = ttv[0];
            if constexpr (NJ == 2) term += ttv[1];
            const float logit = add_xor<32>(add_xor<16>(term));     // (rows 0 + 1) + (rows 2 + 3): all factors
            float p;
            const float gl = grad_coef<LOGIT>(logit, w, p);
            if (lane == 0) score[e] = p;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                // 0 * inf must stay 0 (an overflowed exponent saturates p): clamp the factors to the largest finite value first
                c[j] = gl * fminf(ex[j], FMAX);
                b[j] = gl * __builtin_amdgcn_fmed3f(div_t(ttv[j], t), -FMAX, FMAX);
                if ((lane & 15) == 0) {
                    rec[(size_t)e * 2 * K + fbase + 4 * j] = c[j];
                    rec[(size_t)e * 2 * K + K + fbase + 4 * j] = b[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            ah[j].x = fmaf(c[j], hv[j].x, ah[j].x); ah[j].y = fmaf(c[j], hv[j].y, ah[j].y);
            ah[j].z = fmaf(c[j], hv[j].z, ah[j].z); ah[j].w = fmaf(c[j], hv[j].w, ah[j].w);
            az[j].x = fmaf(b[j], zv[j].x, az[j].x); az[j].y = fmaf(b[j], zv[j].y, az[j].y);
            az[j].z = fmaf(b[j], zv[j].z, az[j].z); az[j].w = fmaf(b[j], zv[j].w, az[j].w);
        }
    }
    if (cur >= 0) flush();
}

// ---------------------------------------------------------------------------- any K, d with K d <= 2048: accumulators in LDS
// One wave per chunk as above; the wave's [dZ row | dH row] accumulators live in its LDS region (2 K d floats), element
// i = lane + 64 n of a row belongs to lane `lane`.  The per-factor dot products are wave all-reduces, the factors are added
// in ascending order.  The coefficients go through `rec` in memory in both passes (every lane stores the same value and
// reads back what it stored itself: no exchange between lanes is involved).
template <bool LOGIT, bool SIDE_B>
__global__ __launch_bounds__(BLOCK) void sampled_generic_kernel(const float* __restrict__ Z, const float* __restrict__ H, int K,
                                                                int d, float t, Lists L, float w, float* __restrict__ score,
                                                                float* rec, float* __restrict__ buf, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ROW = K * d;
    const int wave = wave_index(), lane = lane_id();
    const int chunk = blockIdx.x * WAVES_PER_BLOCK + wave;
    const int pos0 = chunk * SEG;
    if (pos0 >= L.E) return;                                        // (no barrier in this kernel)
    const int n = min(SEG, L.E - pos0);
    float* const acc = lds + (size_t)wave * 2 * ROW;                // [dZ row | dH row]
    int my_e, my_row, my_partner;
    load_chunk<SIDE_B>(L, pos0, lane, my_e, my_row, my_partner);
    int cur = -1;
    auto flush = [&]() {
        float* dst = flush_dst(L, cur, chunk, pos0, buf, part, ROW);
        for (int f = 0; f < K; ++f)                                 // (every element by the lane that accumulates it)
            for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) {
                dst[x] = acc[x];
                dst[ROW + x] = acc[ROW + x];
            }
    };
    for (int s = 0; s < n; ++s) {
        const int e = __builtin_amdgcn_readlane(my_e, s), row = __builtin_amdgcn_readlane(my_row, s);
        const int v = __builtin_amdgcn_readlane(my_partner, s);
        if (row < 0) {
            if constexpr (!SIDE_B) {
                if (lane == 0) score[pos0 + s] = 0.0f;
                for (int f = lane; f < 2 * K; f += DL_WAVE) rec[(size_t)(pos0 + s) * 2 * K + f] = 0.0f;
            }
            continue;
        }
        if (row != cur) {
            if (cur >= 0) flush();
            cur = row;
            for (int f = 0; f < K; ++f)
                for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) acc[x] = acc[ROW + x] = 0.0f;
        }
        float* const r = rec + (size_t)e * 2 * K;
        if constexpr (!SIDE_B) {
            if (v < 0) {
                if (lane == 0) score[e] = 0.0f;
                for (int f = lane; f < 2 * K; f += DL_WAVE) r[f] = 0.0f;
                continue;
            }
            const float* zu = Z + (size_t)row * ROW;
            const float* hu = H + (size_t)row * ROW;
            const float* zk = Z + (size_t)v * ROW;
            const float* hk = H + (size_t)v * ROW;
            float logit = 0.0f;
            for (int f = 0; f < K; ++f) {
                float pz = 0.0f, ph = 0.0f;
                for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) {
                    pz = fmaf(zu[x], zk[x], pz);
                    ph = fmaf(hu[x], hk[x], ph);
                }
                const float zz = wave_allreduce_sum(pz), hh = wave_allreduce_sum(ph);
                const float ex = expf(div_t(zz, t));
                const float ttv = hh * ex;
                logit += ttv;
                r[f] = fminf(ex, FMAX);                             // (the clamps: see the d = 64 kernel)
                r[K + f] = __builtin_amdgcn_fmed3f(div_t(ttv, t), -FMAX, FMAX);
            }
            float p;
            const float gl = grad_coef<LOGIT>(logit, w, p);
            if (lane == 0) score[e] = p;
            for (int f = 0; f < K; ++f) {                           // every lane: its own stores, read back, scaled, stored
                const float cf = gl * r[f], bf = gl * r[K + f];
                r[f] = cf;
                r[K + f] = bf;
            }
        }
        const float* zp = Z + (size_t)v * ROW;
        const float* hp = H + (size_t)v * ROW;
        for (int f = 0; f < K; ++f) {
            const float cf = r[f], bf = r[K + f];
            for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) {
                acc[x] = fmaf(bf, zp[x], acc[x]);
                acc[ROW + x] = fmaf(cf, hp[x], acc[ROW + x]);
            }
        }
    }
    if (cur >= 0) flush();
}

// ---------------------------------------------------------------------------- pass A at the group-per-entry shapes
// The shapes whose pair-list trainer is the group-per-entry kernel (score_bwd_seg_kernel, dl_score_bwd.h): pass A forms a
// pair's dot products, exponentials and factor sum in THAT kernel's lane geometry and order (G = D / 4 lanes hold a factor
// slice, one transposed reduction per table, the factors added by a butterfly over the group), so the scores are its bits.
// Every group of the wave works on the same entry; coefficients and accumulators are the generic kernel's (LDS, `rec`).
// Pass B of these shapes is the generic kernel: it only reads the stored coefficients.
template <int K, int D, bool LOGIT>
__global__ __launch_bounds__(BLOCK) void sampled_geo_kernel(const float* __restrict__ Z, const float* __restrict__ H, float t,
                                                            Lists L, float w, float* __restrict__ score, float* rec,
                                                            float* __restrict__ buf, float* __restrict__ part) {
    using GE = fast::Geo<K, D, float>;
    using FL = typename GE::FL;
    constexpr int VEC = GE::VEC, G = GE::G, KP = FL::KP, VPL = FL::VPL, ROW = GE::ROW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = wave_index(), lane = lane_id();
    const int chunk = blockIdx.x * WAVES_PER_BLOCK + wave;
    const int pos0 = chunk * SEG;
    if (pos0 >= L.E) return;                                        // (no barrier in this kernel)
    const int n = min(SEG, L.E - pos0);
    float* const acc = lds + (size_t)wave * 2 * ROW;                // [dZ row | dH row]
    const int c = lane % G;
    int my_e, my_row, my_partner;
    load_chunk<false>(L, pos0, lane, my_e, my_row, my_partner);
    int cur = -1;
    auto flush = [&]() {
        float* dst = flush_dst(L, cur, chunk, pos0, buf, part, ROW);
#pragma unroll
        for (int f = 0; f < K; ++f)
            for (int x = f * D + lane; x < (f + 1) * D; x += DL_WAVE) {
                dst[x] = acc[x];
                dst[ROW + x] = acc[ROW + x];
            }
    };
    auto zero = [&]() {                                             // (every element by the lane that accumulates it)
#pragma unroll
        for (int f = 0; f < K; ++f)
            for (int x = f * D + lane; x < (f + 1) * D; x += DL_WAVE) acc[x] = acc[ROW + x] = 0.0f;
    };
    for (int s = 0; s < n; ++s) {
        const int e = __builtin_amdgcn_readlane(my_e, s), row = __builtin_amdgcn_readlane(my_row, s);
        const int v = __builtin_amdgcn_readlane(my_partner, s);
        float* const r = rec + (size_t)e * 2 * K;
        if (row < 0 || v < 0) {
            if (row >= 0 && row != cur) {
                if (cur >= 0) flush();
                cur = row;
                zero();
            }
            if (lane == 0) score[e] = 0.0f;
            for (int f = lane; f < 2 * K; f += DL_WAVE) r[f] = 0.0f;
            continue;
        }
        if (row != cur) {
            if (cur >= 0) flush();
            cur = row;
            zero();
        }
        const float* zu = Z + (size_t)row * ROW;
        const float* hu = H + (size_t)row * ROW;
        const float* zp = Z + (size_t)v * ROW;
        const float* hp = H + (size_t)v * ROW;
        float pq[KP], ps[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const int kk = k < K ? k : 0;
            pq[k] = k < K ? fast::dot(fast::load_f32<VEC>(hu + kk * D + c * VEC), fast::Tab<float>::load(hp + kk * D + c * VEC)) : 0.0f;
            ps[k] = k < K ? fast::dot(fast::load_f32<VEC>(zu + kk * D + c * VEC), fast::Tab<float>::load(zp + kk * D + c * VEC)) : 0.0f;
        }
        TransposedReduce<KP, G / 2>::run(pq, c);
        TransposedReduce<KP, G / 2>::run(ps, c);
        float ek_lane[VPL], ch_lane[VPL], cz_lane[VPL];
#pragma unroll
        for (int i = 0; i < VPL; ++i) ek_lane[i] = expf(div_t(ps[i], t));
        float term = 0.0f;
#pragma unroll
        for (int i = 0; i < VPL; ++i)
            if (FL::primary(c) && FL::factor_base(c) + i < K) term += pq[i] * ek_lane[i];
        const float logit = group_allreduce_sum<G>(term);
        float p;
        const float gl = grad_coef<LOGIT>(logit, w, p);
        if (lane == 0) score[e] = p;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {                             // that kernel's coefficients: 0 for gl == 0, whatever e_k is
            const float ek = ek_lane[i];
            ch_lane[i] = gl == 0.0f ? 0.0f : gl * ek;
            cz_lane[i] = gl == 0.0f ? 0.0f : div_t(gl * pq[i] * ek, t);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float ch = group_bcast<G>(ch_lane[FL::src_slot(k)], FL::src_lane(k));
            const float cz = group_bcast<G>(cz_lane[FL::src_slot(k)], FL::src_lane(k));
            r[k] = ch;                                              // (every lane stores the same value)
            r[K + k] = cz;
            for (int x = k * D + lane; x < (k + 1) * D; x += DL_WAVE) {
                acc[x] = fmaf(cz, zp[x], acc[x]);
                acc[ROW + x] = fmaf(ch, hp[x], acc[ROW + x]);
            }
        }
    }
    if (cur >= 0) flush();
}

// the shapes of DL_FAST_SHAPES_F32 whose one-pass trainer is score_bwd_seg_kernel (not the wave-per-entry forms)
#define DL_SAMPLED_GEO_SHAPES(X) X(4, 32) X(5, 32) X(5, 64) X(10, 32) X(10, 64) X(20, 32) X(8, 32) X(4, 8) X(8, 8) X(3, 8)

// ---------------------------------------------------------------------------- finish: B + A per node, in a fixed order
struct Side {
    const int32_t* rowptr;
    const float* buf;
    const float* part;
};

__device__ __forceinline__ float side_sum(const Side& sd, int node, int E, int ROW, int i) {
    int rb = sd.rowptr[node], re = sd.rowptr[node + 1];
    rb = max(0, min(rb, E));
    re = max(0, min(re, E));
    if (re <= rb) return 0.0f;
    const int c0 = rb / SEG, c1 = (re - 1) / SEG;
    if (c0 == c1) return sd.buf[(size_t)node * 2 * ROW + i];
    float v = sd.part[((size_t)2 * c0 + 1) * 2 * ROW + i];          // began in c0 and goes on
    for (int c = c0 + 1; c <= c1; ++c) v += sd.part[(size_t)2 * c * 2 * ROW + i];
    return v;
}

__global__ __launch_bounds__(BLOCK) void sampled_finish_kernel(Side A, Side B, int N, int E, int ROW, int accumulate,
                                                               float* __restrict__ dZ, float* __restrict__ dH) {
    const int node = blockIdx.x * WAVES_PER_BLOCK + wave_index();
    if (node >= N) return;
    for (int i = lane_id(); i < 2 * ROW; i += DL_WAVE) {
        const float total = side_sum(B, node, E, ROW, i) + side_sum(A, node, E, ROW, i);      // B first, then A
        float* out = i < ROW ? dZ + (size_t)node * ROW + i : dH + (size_t)node * ROW + (i - ROW);
        *out = accumulate ? *out + total : total;
    }
}

// ---------------------------------------------------------------------------- the loss value: 1,024 partial sums in a fixed order
template <bool LOGIT>
__global__ __launch_bounds__(BLOCK) void sampled_loss_kernel(const float* __restrict__ score, Lists L, float w,
                                                             float* __restrict__ partial) {
    __shared__ float red[WAVES_PER_BLOCK];
    float acc = 0.0f;
    for (int e = blockIdx.x * BLOCK + threadIdx.x; e < L.E; e += LOSS_BLOCKS * BLOCK) {
        const int u = L.src[e / L.m], k = L.k[e];
        if (w == 0.0f || u < 0 || u >= L.N || k < 0 || k >= L.N) continue;
        const float x = score[e];
        float l;
        if constexpr (LOGIT) {
            l = bce_logits_term(x, 0.0f);
        } else {
            const float lg1 = logf(1.0f - x);                       // (a NaN score stays a NaN loss, as in pair_bce_kernel)
            l = -(lg1 < -100.0f ? -100.0f : lg1);
        }
        acc += w * l;
    }
    acc = wave_allreduce_sum(acc);
    if (lane_id() == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = red[0];
        for (int i = 1; i < WAVES_PER_BLOCK; ++i) s += red[i];
        partial[blockIdx.x] = s;
    }
}

__global__ void sampled_loss_finish_kernel(const float* __restrict__ partial, float* __restrict__ loss) {
    const int lane = threadIdx.x;                                   // one wave
    float acc = 0.0f;
    for (int i = lane; i < LOSS_BLOCKS; i += DL_WAVE) acc += partial[i];
    acc = wave_allreduce_sum(acc);
    if (lane == 0) loss[0] = acc;
}

// ---------------------------------------------------------------------------- host
static bool supported(int K, int d, int dtype) {
    return dtype == DL_F32 && K >= 1 && K <= DL_MAX_FACTORS && d >= 1 && (long long)K * d <= 2048;
}

static int n_chunks(int E) { return (E + SEG - 1) / SEG; }

// workspace: rec [E][2K] | bufA [N][2 ROW] | bufB [N][2 ROW] | partA [2 chunks][2 ROW] | partB likewise | loss partials
struct Carve {
    float *rec, *bufA, *bufB, *partA, *partB, *loss_part;
    size_t bytes;
};

static Carve carve(int E, int N, int K, int d, void* ws) {
    const size_t row2 = (size_t)2 * K * d * sizeof(float);
    const size_t rec = align256((size_t)E * 2 * K * sizeof(float)), buf = align256((size_t)N * row2);
    const size_t part = align256((size_t)2 * n_chunks(E) * row2), lp = align256(LOSS_BLOCKS * sizeof(float));
    char* base = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    Carve c;
    c.rec = (float*)base;
    c.bufA = (float*)(base + rec);
    c.bufB = (float*)(base + rec + buf);
    c.partA = (float*)(base + rec + 2 * buf);
    c.partB = (float*)(base + rec + 2 * buf + part);
    c.loss_part = (float*)(base + rec + 2 * buf + 2 * part);
    c.bytes = rec + 2 * buf + 2 * part + lp + 256;
    return c;
}

template <bool LOGIT>
static int run(const float* Z, const float* H, int N, int K, int d, float t, const Lists& LA, const int32_t* k_rowptr,
               float w, float* score, float* loss, float* dZ, float* dH, int accumulate, const Carve& c, hipStream_t st) {
    const int E = LA.E, ROW = K * d;
    Lists LB = LA;
    LB.rowptr = k_rowptr;
    const dim3 grid(wave_blocks(n_chunks(E))), block(BLOCK);
    if (d == 64 && (K == 4 || K == 8)) {
        if (K == 8) {
            hipLaunchKernelGGL((sampled_d64_kernel<2, LOGIT, false>), grid, block, 0, st, Z, H, t, LA, w, score, c.rec, c.bufA, c.partA);
            hipLaunchKernelGGL((sampled_d64_kernel<2, LOGIT, true>), grid, block, 0, st, Z, H, t, LB, w, score, c.rec, c.bufB, c.partB);
        } else {
            hipLaunchKernelGGL((sampled_d64_kernel<1, LOGIT, false>), grid, block, 0, st, Z, H, t, LA, w, score, c.rec, c.bufA, c.partA);
            hipLaunchKernelGGL((sampled_d64_kernel<1, LOGIT, true>), grid, block, 0, st, Z, H, t, LB, w, score, c.rec, c.bufB, c.partB);
        }
    } else {
        const size_t lds = (size_t)WAVES_PER_BLOCK * 2 * ROW * sizeof(float);
        bool geo = false;
#define X(KK, DD)                                                                                                              \
        if (K == KK && d == DD) {                                                                                              \
            hipLaunchKernelGGL((sampled_geo_kernel<KK, DD, LOGIT>), grid, block, lds, st, Z, H, t, LA, w, score, c.rec, c.bufA, \
                               c.partA);                                                                                       \
            geo = true;                                                                                                        \
        }
        DL_SAMPLED_GEO_SHAPES(X)
#undef X
        if (!geo)
            hipLaunchKernelGGL((sampled_generic_kernel<LOGIT, false>), grid, block, lds, st, Z, H, K, d, t, LA, w, score, c.rec, c.bufA, c.partA);
        hipLaunchKernelGGL((sampled_generic_kernel<LOGIT, true>), grid, block, lds, st, Z, H, K, d, t, LB, w, score, c.rec, c.bufB, c.partB);
    }
    const Side A = {LA.rowptr, c.bufA, c.partA}, B = {k_rowptr, c.bufB, c.partB};
    hipLaunchKernelGGL(sampled_finish_kernel, dim3(wave_blocks(N)), block, 0, st, A, B, N, E, ROW, accumulate, dZ, dH);
    hipLaunchKernelGGL((sampled_loss_kernel<LOGIT>), dim3(LOSS_BLOCKS), block, 0, st, score, LA, w, c.loss_part);
    hipLaunchKernelGGL(sampled_loss_finish_kernel, dim3(1), dim3(DL_WAVE), 0, st, c.loss_part, loss);
    return check_launch(LOGIT ? "dl_score_sampled_train_logits" : "dl_score_sampled_train");
}

static int entry(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* src, int n_rows,
                 int m, const int32_t* u_rowptr, const int32_t* k, const int32_t* order, const int32_t* k_rowptr, float w,
                 float* score, float* loss, float* dZ, float* dH, int accumulate, void* ws, size_t ws_bytes, bool logit,
                 void* stream) {
    const char* const name = logit ? "dl_score_sampled_train_logits" : "dl_score_sampled_train";
    DL_REQUIRE(supported(K, d, (int)dtype), "%s serves fp32 tables with 1 <= K <= 64 and K d <= 2048 (got K=%d d=%d dtype=%d: %s_supported)",
               name, K, d, (int)dtype, name);
    DL_REQUIRE(N >= 1 && n_rows >= 0 && m >= 1, "%s: N=%d n_rows=%d m=%d", name, N, n_rows, m);
    DL_REQUIRE((long long)n_rows * m <= 0x7fffffffLL / (2 * K), "%s: %d x %d entries x %d coefficients exceed 2^31 - 1", name, n_rows, m, 2 * K);
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    DL_REQUIRE(Z && H && dZ && dH && loss && u_rowptr && k_rowptr, "NULL argument");
    const int E = n_rows * m;
    if (E > 0) DL_REQUIRE(src && k && order && score, "NULL list argument");
    const Carve c = carve(E, N, K, d, ws);
    if (!ws || ws_bytes < c.bytes) {
        set_error("workspace too small: have %zu, need %zu (%s_workspace_bytes)", ws ? ws_bytes : (size_t)0, c.bytes, name);
        return DL_E_WORKSPACE;
    }
    const Lists LA = {src, k, order, u_rowptr, m, E, N};
    if (logit) return run<true>((const float*)Z, (const float*)H, N, K, d, t, LA, k_rowptr, w, score, loss, dZ, dH, accumulate, c, (hipStream_t)stream);
    return run<false>((const float*)Z, (const float*)H, N, K, d, t, LA, k_rowptr, w, score, loss, dZ, dH, accumulate, c, (hipStream_t)stream);
}

}  // namespace sampled
}  // namespace dl

extern "C" {

int dl_score_sampled_train_supported(int K, int d, dl_dtype dtype) { return dl::sampled::supported(K, d, (int)dtype) ? 1 : 0; }
int dl_score_sampled_train_logits_supported(int K, int d, dl_dtype dtype) { return dl_score_sampled_train_supported(K, d, dtype); }

size_t dl_score_sampled_train_workspace_bytes(int n_entries, int N, int K, int d) {
    if (n_entries < 0 || N < 1 || !dl::sampled::supported(K, d, DL_F32)) return 0;
    return dl::sampled::carve(n_entries, N, K, d, nullptr).bytes;
}
size_t dl_score_sampled_train_logits_workspace_bytes(int n_entries, int N, int K, int d) {
    return dl_score_sampled_train_workspace_bytes(n_entries, N, K, d);
}

int dl_score_sampled_train(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* src,
                           int n_rows, int m, const int32_t* u_rowptr, const int32_t* k, const int32_t* order,
                           const int32_t* k_rowptr, float w, float* score, float* loss, float* dZ, float* dH, int accumulate,
                           void* ws, size_t ws_bytes, void* stream) {
    return dl::sampled::entry(Z, H, N, K, d, dtype, t, src, n_rows, m, u_rowptr, k, order, k_rowptr, w, score, loss, dZ, dH,
                              accumulate, ws, ws_bytes, false, stream);
}

int dl_score_sampled_train_logits(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* src,
                                  int n_rows, int m, const int32_t* u_rowptr, const int32_t* k, const int32_t* order,
                                  const int32_t* k_rowptr, float w, float* score, float* loss, float* dZ, float* dH,
                                  int accumulate, void* ws, size_t ws_bytes, void* stream) {
    return dl::sampled::entry(Z, H, N, K, d, dtype, t, src, n_rows, m, u_rowptr, k, order, k_rowptr, w, score, loss, dZ, dH,
                              accumulate, ws, ws_bytes, true, stream);
}

}  // extern "C"
