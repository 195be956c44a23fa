// Pairwise ranking trainer (BPR) over SAMPLED partners (dl_score_sampled_bpr_train): a training edge row (u_r, v_r) must score
// above (u_r, k_rj) for the m negatives k_rj of the row drawn by dl_sample_negatives, trained without a plan build.
//
// Row r has the positive (src[r], dst[r]) and the entries e = r m + j, j < m, with partners k[e] (-1 = a failed draw: no term):
//   x(a, b) = sum_f (h_f[a].h_f[b]) exp(z_f[a].z_f[b] / t),    delta_rj = x(u_r, k_rj) - x(u_r, v_r)    (taken in fp32),
//   loss = sum_{r, j live} w (max(delta, 0) + log1p(exp(-|delta|))),    g_rj = w sigma(delta_rj),    G_r = sum_j g_rj (ascending j),
//   d loss / d x(u_r, k_rj) = g_rj,    d loss / d x(u_r, v_r) = -G_r
// and dZ, dH = d loss / d (Z, H), every one of the (m + 1) pairs of a row in BOTH endpoints' rows, without float atomics:
//   row pass: the row list is cut into chunks of RPC = floor(64 / (m + 1)) consecutive rows (1 <= m <= 63), one wave per chunk;
//     lane rr (m + 1) + jj preloads partner jj of the chunk's row rr (jj = 0: dst).  Per row the wave gathers z[v], h[v] FIRST,
//     forms x+ and keeps the positive's per-factor e_f and (h.h)_f e_f (d = 64: in registers with z[v], h[v]; generic: in the
//     positive's coefficient record), then walks the m negatives in ascending j: x-, delta, g, the 2K coefficients c_f = g e_f,
//     b_f = g (h.h)_f e_f / t (the arithmetic and the finite clamps of dl_train_sampled.hip), written to memory, and
//     dH[u] += c_f h_f[k], dZ[u] += b_f z_f[k] on chip; last the positive with -G_r (exactly 0 where G_r == 0: a row whose
//     draws all failed, or w == 0, contributes nothing).  Consecutive rows of the same u share the accumulator; where u changes
//     the sum is written out: to the node's place if all rows of u lie inside the chunk, else to one of the chunk's two partial
//     slots (2 chunk: u began in an earlier chunk; 2 chunk + 1: it began here and goes on).
//   partner passes (two launches of one kernel): the k side walks `order` (the stable ascending sort of k, the -1 entries first
//     and skipped) with k_rowptr, the positives' partner side walks dst_order (the stable ascending sort of dst) with dst_rowptr,
//     both in chunks of 64 list positions: read the stored coefficients, gather z[u], h[u], accumulate dH[p] += c_f h_f[u],
//     dZ[p] += b_f z_f[u]; direct place or partial slots as above.
//   finish: one wave per node: k side + positives' partner side + row side, in THAT order, each side its direct place or its
//     partial slots in chunk order; written to dZ / dH or added onto them (accumulate != 0).  A node no list names reads exactly 0.
//   loss: 1,024 partial sums over the entries in a fixed order (delta re-formed from the stored logits: the same fp32
//     subtraction), then one wave.
// Every sum has an order that the lists alone fix: the same bits on every call, whatever the grid.
// k == v, k == u and v == u are legal: the passes then contribute to the same row, which is simply the sum.
//
// Kernels: d = 64 with K in {4, 8} takes the lane geometry and reduction order of sampled_d64_kernel (dl_train_sampled.hip), so
// x+ and x- are that kernel's bits; every other fp32 shape with K d <= 2048 takes the generic form (accumulators in LDS,
// per-factor wave all-reduces, factors added in ascending order: sampled_generic_kernel's order).
// Resources (gfx950, -O3, -Rpass-analysis=kernel-resource-usage; no kernel uses scratch) -> waves per SIMD:
//   bpr_row_d64_kernel<2>       142 VGPRs, no LDS -> 3       bpr_partner_d64_kernel<2, *>   58 VGPRs, no LDS -> 8
//   bpr_row_d64_kernel<1>        88 VGPRs, no LDS -> 5       bpr_partner_d64_kernel<1, *>   36 VGPRs, no LDS -> 8
//   bpr_row_generic_kernel       47 VGPRs -> 7 by registers; 32 K d bytes of dynamic LDS per workgroup of 4 waves (64 KiB at
//   bpr_partner_generic_kernel   26 VGPRs -> 8               K d = 2048: two workgroups per CU) bound it first from K d = 640 on
// (sampled_d64_kernel<2> has 108 VGPRs and 4 waves: z[v], h[v] and the positive's 2 NJ factors held across the walk cost the
// K = 8 row pass one wave; a launch bound of 4 waves spills 64 bytes per lane, so it is not set.)
#include "dl_bpr_logit.h"

namespace dl {
namespace bpr {

using fast::store4;

constexpr int SEG = 64;                 // list positions per chunk of a partner pass; lanes that preload a row chunk's indices
constexpr int MAX_M = 63;
constexpr float FMAX = 3.402823466e38f;
constexpr int LOSS_BLOCKS = 1024;

struct Lists {
    const int32_t* src;                 // [n_rows] ascending
    const int32_t* dst;                 // [n_rows]
    const int32_t* k;                   // [n_rows m]
    const int32_t* order;               // the list a partner pass walks: order [E] or dst_order [n_rows]
    const int32_t* rowptr;              // [N+1] of the side walked: u_rowptr (ENTRIES), k_rowptr, dst_rowptr
    int m, n_rows, N;
    int rpc;                            // rows per chunk of the row pass
};

// where the sum of node `cur` over this chunk goes: [rb, re) = the node's range and [c0, c0 + len) the chunk's, in the same unit
__device__ __forceinline__ float* flush_dst(int cur, int rb, int re, int chunk, int c0, int len, float* buf, float* part, int ROW) {
    const bool before = rb < c0, after = re > c0 + len;
    if (!before && !after) return buf + (size_t)cur * 2 * ROW;
    return part + ((size_t)2 * chunk + (before ? 0 : 1)) * 2 * ROW;
}

// the row pass's indices, one per lane: lane rr (m + 1) + jj holds (src, partner jj) of the chunk's row rr; -1 = outside the table
__device__ __forceinline__ void load_rows(const Lists& L, int row0, int nr, int lane, int& my_u, int& my_p) {
    my_u = my_p = -1;
    const int rr = lane / (L.m + 1), jj = lane - rr * (L.m + 1);
    if (rr < nr) {
        const int r = row0 + rr;
        int u = L.src[r], p = jj == 0 ? L.dst[r] : L.k[r * L.m + jj - 1];
        if (u < 0 || u >= L.N) u = -1;
        if (p < 0 || p >= L.N) p = -1;
        my_u = u;
        my_p = p;
    }
}

// a partner pass's indices, one per lane: (record, node walked, node gathered); node walked = -1: skipped
template <bool POS>
__device__ __forceinline__ void load_partner(const Lists& L, int n, int pos0, int lane, int& my_i, int& my_row, int& my_partner) {
    my_i = 0;
    my_row = my_partner = -1;
    const int pos = pos0 + lane;
    if (pos < n) {
        const int i = L.order[pos];
        if (i >= 0 && i < n) {
            const int r = POS ? i : i / L.m;
            const int u = L.src[r], v = L.dst[r], p = POS ? v : L.k[i];
            if (u >= 0 && u < L.N && v >= 0 && v < L.N && p >= 0 && p < L.N) {
                my_i = i;
                my_row = p;
                my_partner = u;
            }
        }
    }
}

__device__ __forceinline__ float bpr_coef(float delta, float w) { return w == 0.0f ? 0.0f : w * sigmoid_minus_label(delta, 0.0f); }

// ---------------------------------------------------------------------------- d = 64, K = 4 NJ: the row pass
template <int NJ>
__global__ __launch_bounds__(BLOCK) void bpr_row_d64_kernel(const float* __restrict__ Z, const float* __restrict__ H, float t, Lists L,
                                                            float w, float* __restrict__ pos_logit, float* __restrict__ neg_logit,
                                                            float* __restrict__ rec_neg, float* __restrict__ rec_pos,
                                                            float* __restrict__ buf, float* __restrict__ part) {
    constexpr int K = 4 * NJ, ROW = K * 64;
    const int wave = wave_index(), lane = lane_id();
    const int chunk = blockIdx.x * WAVES_PER_BLOCK + wave;
    const int row0 = chunk * L.rpc;
    if (row0 >= L.n_rows) return;                                   // (no barrier in this kernel)
    const int nr = min(L.rpc, L.n_rows - row0), m = L.m;
    int my_u, my_p;
    load_rows(L, row0, nr, lane, my_u, my_p);
    const int fbase = lane >> 4;                                    // this lane's factors: fbase + 4 j
    float4 az[NJ], ah[NJ], uz[NJ], uh[NJ];
    int cur = -1;
    auto flush = [&]() {
        float* dst = flush_dst(cur, L.rowptr[cur] / m, L.rowptr[cur + 1] / m, chunk, row0, L.rpc, buf, part, ROW);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            store4(dst + 4 * (j * 64 + lane), az[j]);
            store4(dst + ROW + 4 * (j * 64 + lane), ah[j]);
        }
    };
    auto accumulate = [&](const float* c, const float* b, const float4* zv, const float4* hv) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            ah[j].x = fmaf(c[j], hv[j].x, ah[j].x); ah[j].y = fmaf(c[j], hv[j].y, ah[j].y);
            ah[j].z = fmaf(c[j], hv[j].z, ah[j].z); ah[j].w = fmaf(c[j], hv[j].w, ah[j].w);
            az[j].x = fmaf(b[j], zv[j].x, az[j].x); az[j].y = fmaf(b[j], zv[j].y, az[j].y);
            az[j].z = fmaf(b[j], zv[j].z, az[j].z); az[j].w = fmaf(b[j], zv[j].w, az[j].w);
        }
    };
    for (int rr = 0; rr < nr; ++rr) {
        const int r = row0 + rr, base = rr * (m + 1), e0 = r * m;
        const int u = __builtin_amdgcn_readlane(my_u, base), v = __builtin_amdgcn_readlane(my_p, base);
        if (u < 0 || v < 0) {                                       // an endpoint outside the table: the row is no term at all
            if (lane == 0) pos_logit[r] = 0.0f;
            if (lane < 2 * K) rec_pos[(size_t)r * 2 * K + lane] = 0.0f;
            for (int i = lane; i < m; i += DL_WAVE) neg_logit[e0 + i] = 0.0f;
            for (int i = lane; i < m * 2 * K; i += DL_WAVE) rec_neg[(size_t)e0 * 2 * K + i] = 0.0f;
            continue;
        }
        if (u != cur) {
            if (cur >= 0) flush();
            cur = u;
#pragma unroll
            for (int j = 0; j < NJ; ++j) az[j] = ah[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            load_row_d64<NJ>(Z, u, lane, uz);
            load_row_d64<NJ>(H, u, lane, uh);
        }
        // the positive first: its logit, and e_f, (h.h)_f e_f kept with z[v], h[v] until G_r is known
        float4 zp[NJ], hp[NJ];
        load_row_d64<NJ>(Z, v, lane, zp);
        load_row_d64<NJ>(H, v, lane, hp);
        float exp_[NJ], ttp[NJ];
        const float xp = logit_d64<NJ>(uz, uh, zp, hp, t, exp_, ttp);       // (the lane geometry and the order: dl_bpr_logit.h)
        if (lane == 0) pos_logit[r] = xp;
        float G = 0.0f;
#pragma unroll 1
        for (int jn = 0; jn < m; ++jn) {
            const int e = e0 + jn, kk = __builtin_amdgcn_readlane(my_p, base + 1 + jn);
            if (kk < 0) {                                           // a failed draw: no term, score 0, nothing gathered
                if (lane == 0) neg_logit[e] = 0.0f;
                if (lane < 2 * K) rec_neg[(size_t)e * 2 * K + lane] = 0.0f;
                continue;
            }
            float4 zv[NJ], hv[NJ];
            load_row_d64<NJ>(Z, kk, lane, zv);
            load_row_d64<NJ>(H, kk, lane, hv);
            float ex[NJ], ttv[NJ], c[NJ], b[NJ];
            const float xn = logit_d64<NJ>(uz, uh, zv, hv, t, ex, ttv);
            const float gl = bpr_coef(xn - xp, w);
            G += gl;
            if (lane == 0) neg_logit[e] = xn;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                // 0 * inf must stay 0: clamp the factors to the largest finite value first (dl_train_sampled.hip)
                c[j] = gl * fminf(ex[j], FMAX);
                b[j] = gl * __builtin_amdgcn_fmed3f(div_t(ttv[j], t), -FMAX, FMAX);
                if ((lane & 15) == 0) {
                    rec_neg[(size_t)e * 2 * K + fbase + 4 * j] = c[j];
                    rec_neg[(size_t)e * 2 * K + K + fbase + 4 * j] = b[j];
                }
            }
            accumulate(c, b, zv, hv);
        }
        const float gp = G == 0.0f ? 0.0f : -G;                     // d loss / d x+; exactly nothing where no negative pulled
        float c[NJ], b[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            c[j] = gp * fminf(exp_[j], FMAX);
            b[j] = gp * __builtin_amdgcn_fmed3f(div_t(ttp[j], t), -FMAX, FMAX);
            if ((lane & 15) == 0) {
                rec_pos[(size_t)r * 2 * K + fbase + 4 * j] = c[j];
                rec_pos[(size_t)r * 2 * K + K + fbase + 4 * j] = b[j];
            }
        }
        accumulate(c, b, zp, hp);
    }
    if (cur >= 0) flush();
}

// ---------------------------------------------------------------------------- d = 64, K = 4 NJ: a partner pass
template <int NJ, bool POS>
__global__ __launch_bounds__(BLOCK) void bpr_partner_d64_kernel(const float* __restrict__ Z, const float* __restrict__ H, Lists L, int n,
                                                                const float* __restrict__ rec, float* __restrict__ buf,
                                                                float* __restrict__ part) {
    constexpr int K = 4 * NJ, ROW = K * 64;
    const int wave = wave_index(), lane = lane_id();
    const int chunk = blockIdx.x * WAVES_PER_BLOCK + wave;
    const int pos0 = chunk * SEG;
    if (pos0 >= n) return;                                          // (no barrier in this kernel)
    const int cnt = min(SEG, n - pos0);
    int my_i, my_row, my_partner;
    load_partner<POS>(L, n, pos0, lane, my_i, my_row, my_partner);
    const int fbase = lane >> 4;
    float4 az[NJ], ah[NJ];
    int cur = -1;
    auto flush = [&]() {
        float* dst = flush_dst(cur, L.rowptr[cur], L.rowptr[cur + 1], chunk, pos0, SEG, buf, part, ROW);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            store4(dst + 4 * (j * 64 + lane), az[j]);
            store4(dst + ROW + 4 * (j * 64 + lane), ah[j]);
        }
    };
    for (int s = 0; s < cnt; ++s) {
        const int i = __builtin_amdgcn_readlane(my_i, s), row = __builtin_amdgcn_readlane(my_row, s);
        const int u = __builtin_amdgcn_readlane(my_partner, s);
        if (row < 0) continue;                                      // a failed draw, or an endpoint outside the table
        if (row != cur) {
            if (cur >= 0) flush();
            cur = row;
#pragma unroll
            for (int j = 0; j < NJ; ++j) az[j] = ah[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float4 zu = *reinterpret_cast<const float4*>(Z + (size_t)u * ROW + (j * 64 + lane) * 4);
            const float4 hu = *reinterpret_cast<const float4*>(H + (size_t)u * ROW + (j * 64 + lane) * 4);
            const float c = rec[(size_t)i * 2 * K + fbase + 4 * j], b = rec[(size_t)i * 2 * K + K + fbase + 4 * j];
            ah[j].x = fmaf(c, hu.x, ah[j].x); ah[j].y = fmaf(c, hu.y, ah[j].y);
            ah[j].z = fmaf(c, hu.z, ah[j].z); ah[j].w = fmaf(c, hu.w, ah[j].w);
            az[j].x = fmaf(b, zu.x, az[j].x); az[j].y = fmaf(b, zu.y, az[j].y);
            az[j].z = fmaf(b, zu.z, az[j].z); az[j].w = fmaf(b, zu.w, az[j].w);
        }
    }
    if (cur >= 0) flush();
}

// ---------------------------------------------------------------------------- any K, d with K d <= 2048: accumulators in LDS
// One wave per chunk as above; the wave's [dZ row | dH row] accumulators live in its LDS region (2 K d floats), element
// i = lane + 64 n of a factor slice belongs to lane `lane`.  The per-factor dot products are wave all-reduces, the factors are
// added in ascending order.  The coefficients go through the records in memory (every lane stores the same value and reads
// back what it stored itself: no exchange between lanes is involved); the positive's record holds its clamped e_f and
// (h.h)_f e_f / t until G_r is known and is then scaled in place.
__global__ __launch_bounds__(BLOCK) void bpr_row_generic_kernel(const float* __restrict__ Z, const float* __restrict__ H, int K, int d,
                                                                float t, Lists L, float w, float* __restrict__ pos_logit,
                                                                float* __restrict__ neg_logit, float* rec_neg, float* rec_pos,
                                                                float* __restrict__ buf, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ROW = K * d;
    const int wave = wave_index(), lane = lane_id();
    const int chunk = blockIdx.x * WAVES_PER_BLOCK + wave;
    const int row0 = chunk * L.rpc;
    if (row0 >= L.n_rows) return;                                   // (no barrier in this kernel)
    const int nr = min(L.rpc, L.n_rows - row0), m = L.m;
    float* const acc = lds + (size_t)wave * 2 * ROW;                // [dZ row | dH row]
    int my_u, my_p;
    load_rows(L, row0, nr, lane, my_u, my_p);
    int cur = -1;
    auto flush = [&]() {
        float* dst = flush_dst(cur, L.rowptr[cur] / m, L.rowptr[cur + 1] / m, chunk, row0, L.rpc, buf, part, ROW);
        for (int f = 0; f < K; ++f)                                 // (every element by the lane that accumulates it)
            for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) {
                dst[x] = acc[x];
                dst[ROW + x] = acc[ROW + x];
            }
    };
    // the logit of (u, p), its clamped e_f and (h.h)_f e_f / t left in the record r
    auto score = [&](const float* zu, const float* hu, int p, float* r) {
        const float* zk = Z + (size_t)p * ROW;
        const float* hk = H + (size_t)p * ROW;
        float logit = 0.0f;
        for (int f = 0; f < K; ++f) {
            float ex;
            const float ttv = factor_term_generic(zu, hu, zk, hk, f, d, lane, t, ex, logit);   // (the order: dl_bpr_logit.h)
            r[f] = fminf(ex, FMAX);                                 // (the clamps: see the d = 64 kernel)
            r[K + f] = __builtin_amdgcn_fmed3f(div_t(ttv, t), -FMAX, FMAX);
        }
        return logit;
    };
    // scale the record by g (every lane: its own stores, read back, scaled, stored) and add the pair to the u row
    auto apply = [&](float g, int p, float* r) {
        const float* zk = Z + (size_t)p * ROW;
        const float* hk = H + (size_t)p * ROW;
        for (int f = 0; f < K; ++f) {
            const float cf = g * r[f], bf = g * r[K + f];
            r[f] = cf;
            r[K + f] = bf;
            for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) {
                acc[x] = fmaf(bf, zk[x], acc[x]);
                acc[ROW + x] = fmaf(cf, hk[x], acc[ROW + x]);
            }
        }
    };
    for (int rr = 0; rr < nr; ++rr) {
        const int r = row0 + rr, base = rr * (m + 1), e0 = r * m;
        const int u = __builtin_amdgcn_readlane(my_u, base), v = __builtin_amdgcn_readlane(my_p, base);
        float* const rp = rec_pos + (size_t)r * 2 * K;
        if (u < 0 || v < 0) {
            if (lane == 0) pos_logit[r] = 0.0f;
            for (int f = lane; f < 2 * K; f += DL_WAVE) rp[f] = 0.0f;
            for (int i = lane; i < m; i += DL_WAVE) neg_logit[e0 + i] = 0.0f;
            for (int i = lane; i < m * 2 * K; i += DL_WAVE) rec_neg[(size_t)e0 * 2 * K + i] = 0.0f;
            continue;
        }
        if (u != cur) {
            if (cur >= 0) flush();
            cur = u;
            for (int f = 0; f < K; ++f)
                for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) acc[x] = acc[ROW + x] = 0.0f;
        }
        const float* zu = Z + (size_t)u * ROW;
        const float* hu = H + (size_t)u * ROW;
        const float xp = score(zu, hu, v, rp);
        if (lane == 0) pos_logit[r] = xp;
        float G = 0.0f;
        for (int jn = 0; jn < m; ++jn) {
            const int e = e0 + jn, kk = __builtin_amdgcn_readlane(my_p, base + 1 + jn);
            float* const rn = rec_neg + (size_t)e * 2 * K;
            if (kk < 0) {
                if (lane == 0) neg_logit[e] = 0.0f;
                for (int f = lane; f < 2 * K; f += DL_WAVE) rn[f] = 0.0f;
                continue;
            }
            const float xn = score(zu, hu, kk, rn);
            const float gl = bpr_coef(xn - xp, w);
            G += gl;
            if (lane == 0) neg_logit[e] = xn;
            apply(gl, kk, rn);
        }
        apply(G == 0.0f ? 0.0f : -G, v, rp);
    }
    if (cur >= 0) flush();
}

template <bool POS>
__global__ __launch_bounds__(BLOCK) void bpr_partner_generic_kernel(const float* __restrict__ Z, const float* __restrict__ H, int K,
                                                                    int d, Lists L, int n, const float* __restrict__ rec,
                                                                    float* __restrict__ buf, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ROW = K * d;
    const int wave = wave_index(), lane = lane_id();
    const int chunk = blockIdx.x * WAVES_PER_BLOCK + wave;
    const int pos0 = chunk * SEG;
    if (pos0 >= n) return;                                          // (no barrier in this kernel)
    const int cnt = min(SEG, n - pos0);
    float* const acc = lds + (size_t)wave * 2 * ROW;
    int my_i, my_row, my_partner;
    load_partner<POS>(L, n, pos0, lane, my_i, my_row, my_partner);
    int cur = -1;
    auto flush = [&]() {
        float* dst = flush_dst(cur, L.rowptr[cur], L.rowptr[cur + 1], chunk, pos0, SEG, buf, part, ROW);
        for (int f = 0; f < K; ++f)
            for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) {
                dst[x] = acc[x];
                dst[ROW + x] = acc[ROW + x];
            }
    };
    for (int s = 0; s < cnt; ++s) {
        const int i = __builtin_amdgcn_readlane(my_i, s), row = __builtin_amdgcn_readlane(my_row, s);
        const int u = __builtin_amdgcn_readlane(my_partner, s);
        if (row < 0) continue;
        if (row != cur) {
            if (cur >= 0) flush();
            cur = row;
            for (int f = 0; f < K; ++f)
                for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) acc[x] = acc[ROW + x] = 0.0f;
        }
        const float* r = rec + (size_t)i * 2 * K;
        const float* zu = Z + (size_t)u * ROW;
        const float* hu = H + (size_t)u * ROW;
        for (int f = 0; f < K; ++f) {
            const float cf = r[f], bf = r[K + f];
            for (int x = f * d + lane; x < (f + 1) * d; x += DL_WAVE) {
                acc[x] = fmaf(bf, zu[x], acc[x]);
                acc[ROW + x] = fmaf(cf, hu[x], acc[ROW + x]);
            }
        }
    }
    if (cur >= 0) flush();
}

// ---------------------------------------------------------------------------- finish: k side + positives' side + row side
struct Side {
    const int32_t* rowptr;
    const float* buf;
    const float* part;
    int unit;                           // rowptr counts `unit` list positions per position of this side (the row side: m)
    int seg;                            // positions per chunk
    int n;                              // positions in all
};

__device__ __forceinline__ float side_sum(const Side& sd, int node, int ROW, int i) {
    int rb = sd.rowptr[node] / sd.unit, re = sd.rowptr[node + 1] / sd.unit;
    rb = max(0, min(rb, sd.n));
    re = max(0, min(re, sd.n));
    if (re <= rb) return 0.0f;
    const int c0 = rb / sd.seg, c1 = (re - 1) / sd.seg;
    if (c0 == c1) return sd.buf[(size_t)node * 2 * ROW + i];
    float v = sd.part[((size_t)2 * c0 + 1) * 2 * ROW + i];          // began in c0 and goes on
    for (int c = c0 + 1; c <= c1; ++c) v += sd.part[(size_t)2 * c * 2 * ROW + i];
    return v;
}

__global__ __launch_bounds__(BLOCK) void bpr_finish_kernel(Side SK, Side SP, Side SA, int N, int ROW, int accumulate,
                                                           float* __restrict__ dZ, float* __restrict__ dH) {
    const int node = blockIdx.x * WAVES_PER_BLOCK + wave_index();
    if (node >= N) return;
    for (int i = lane_id(); i < 2 * ROW; i += DL_WAVE) {
        const float total = (side_sum(SK, node, ROW, i) + side_sum(SP, node, ROW, i)) + side_sum(SA, node, ROW, i);
        float* out = i < ROW ? dZ + (size_t)node * ROW + i : dH + (size_t)node * ROW + (i - ROW);
        *out = accumulate ? *out + total : total;
    }
}

// ---------------------------------------------------------------------------- the loss value: 1,024 partial sums in a fixed order
__global__ __launch_bounds__(BLOCK) void bpr_loss_kernel(const float* __restrict__ pos_logit, const float* __restrict__ neg_logit,
                                                         Lists L, float w, float* __restrict__ partial) {
    __shared__ float red[WAVES_PER_BLOCK];
    const int E = L.n_rows * L.m;
    float acc = 0.0f;
    for (int e = blockIdx.x * BLOCK + threadIdx.x; e < E; e += LOSS_BLOCKS * BLOCK) {
        const int r = e / L.m;
        const int u = L.src[r], v = L.dst[r], k = L.k[e];
        if (w == 0.0f || u < 0 || u >= L.N || v < 0 || v >= L.N || k < 0 || k >= L.N) continue;
        acc += w * bce_logits_term(neg_logit[e] - pos_logit[r], 0.0f);      // (a NaN difference stays a NaN loss)
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

__global__ void bpr_loss_finish_kernel(const float* __restrict__ partial, float* __restrict__ loss) {
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

static int chunks(int n, int seg) { return (n + seg - 1) / seg; }
static int rows_per_chunk(int m) { return SEG / (m + 1); }

// workspace: rec_neg [E][2K] | rec_pos [n_rows][2K] | bufA, bufK, bufP [N][2 ROW] | partA [2 row chunks][2 ROW] |
//            partK [2 chunks of E][2 ROW] | partP [2 chunks of n_rows][2 ROW] | loss partials
struct Carve {
    float *rec_neg, *rec_pos, *bufA, *bufK, *bufP, *partA, *partK, *partP, *loss_part;
    size_t bytes;
};

static Carve carve(int n_rows, int m, int N, int K, int d, void* ws) {
    const size_t row2 = (size_t)2 * K * d * sizeof(float), E = (size_t)n_rows * m;
    const size_t sizes[9] = {align256(E * 2 * K * sizeof(float)), align256((size_t)n_rows * 2 * K * sizeof(float)),
                             align256((size_t)N * row2), align256((size_t)N * row2), align256((size_t)N * row2),
                             align256((size_t)2 * chunks(n_rows, rows_per_chunk(m)) * row2),
                             align256((size_t)2 * chunks((int)E, SEG) * row2), align256((size_t)2 * chunks(n_rows, SEG) * row2),
                             align256(LOSS_BLOCKS * sizeof(float))};
    char* p = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    float* at[9];
    size_t total = 256;
    for (int i = 0; i < 9; ++i) {
        at[i] = (float*)p;
        p += sizes[i];
        total += sizes[i];
    }
    return {at[0], at[1], at[2], at[3], at[4], at[5], at[6], at[7], at[8], total};
}

static int run(const float* Z, const float* H, int N, int K, int d, float t, const Lists& LA, const int32_t* dst_order,
               const int32_t* dst_rowptr, const int32_t* order, const int32_t* k_rowptr, float w, float* pos_logit,
               float* neg_logit, float* loss, float* dZ, float* dH, int accumulate, const Carve& c, hipStream_t st) {
    const int n_rows = LA.n_rows, E = n_rows * LA.m, ROW = K * d;
    Lists LK = LA, LP = LA;
    LK.order = order;
    LK.rowptr = k_rowptr;
    LP.order = dst_order;
    LP.rowptr = dst_rowptr;
    const dim3 block(BLOCK);
    const dim3 gA(wave_blocks(chunks(n_rows, LA.rpc))), gK(wave_blocks(chunks(E, SEG))), gP(wave_blocks(chunks(n_rows, SEG)));
    if (n_rows > 0) {                                               // (an empty list launches nothing: the finish writes zeros)
        if (d == 64 && K == 8) {
            hipLaunchKernelGGL((bpr_row_d64_kernel<2>), gA, block, 0, st, Z, H, t, LA, w, pos_logit, neg_logit, c.rec_neg, c.rec_pos, c.bufA, c.partA);
            hipLaunchKernelGGL((bpr_partner_d64_kernel<2, false>), gK, block, 0, st, Z, H, LK, E, c.rec_neg, c.bufK, c.partK);
            hipLaunchKernelGGL((bpr_partner_d64_kernel<2, true>), gP, block, 0, st, Z, H, LP, n_rows, c.rec_pos, c.bufP, c.partP);
        } else if (d == 64 && K == 4) {
            hipLaunchKernelGGL((bpr_row_d64_kernel<1>), gA, block, 0, st, Z, H, t, LA, w, pos_logit, neg_logit, c.rec_neg, c.rec_pos, c.bufA, c.partA);
            hipLaunchKernelGGL((bpr_partner_d64_kernel<1, false>), gK, block, 0, st, Z, H, LK, E, c.rec_neg, c.bufK, c.partK);
            hipLaunchKernelGGL((bpr_partner_d64_kernel<1, true>), gP, block, 0, st, Z, H, LP, n_rows, c.rec_pos, c.bufP, c.partP);
        } else {
            const size_t lds = (size_t)WAVES_PER_BLOCK * 2 * ROW * sizeof(float);
            hipLaunchKernelGGL(bpr_row_generic_kernel, gA, block, lds, st, Z, H, K, d, t, LA, w, pos_logit, neg_logit, c.rec_neg, c.rec_pos, c.bufA, c.partA);
            hipLaunchKernelGGL((bpr_partner_generic_kernel<false>), gK, block, lds, st, Z, H, K, d, LK, E, c.rec_neg, c.bufK, c.partK);
            hipLaunchKernelGGL((bpr_partner_generic_kernel<true>), gP, block, lds, st, Z, H, K, d, LP, n_rows, c.rec_pos, c.bufP, c.partP);
        }
    }
    const Side SK = {k_rowptr, c.bufK, c.partK, 1, SEG, E}, SP = {dst_rowptr, c.bufP, c.partP, 1, SEG, n_rows};
    const Side SA = {LA.rowptr, c.bufA, c.partA, LA.m, LA.rpc, n_rows};
    hipLaunchKernelGGL(bpr_finish_kernel, dim3(wave_blocks(N)), block, 0, st, SK, SP, SA, N, ROW, accumulate, dZ, dH);
    hipLaunchKernelGGL(bpr_loss_kernel, dim3(LOSS_BLOCKS), block, 0, st, pos_logit, neg_logit, LA, w, c.loss_part);
    hipLaunchKernelGGL(bpr_loss_finish_kernel, dim3(1), dim3(DL_WAVE), 0, st, c.loss_part, loss);
    return check_launch("dl_score_sampled_bpr_train");
}

}  // namespace bpr
}  // namespace dl

extern "C" {

int dl_score_sampled_bpr_train_supported(int K, int d, dl_dtype dtype) { return dl::bpr::supported(K, d, (int)dtype) ? 1 : 0; }

size_t dl_score_sampled_bpr_train_workspace_bytes(int n_rows, int m, int N, int K, int d) {
    if (n_rows < 0 || m < 1 || m > dl::bpr::MAX_M || N < 1 || !dl::bpr::supported(K, d, DL_F32)) return 0;
    if ((long long)n_rows * m > 0x7fffffffLL / (2 * K)) return 0;
    return dl::bpr::carve(n_rows, m, N, K, d, nullptr).bytes;
}

int dl_score_sampled_bpr_train(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* src,
                               const int32_t* dst, int n_rows, int m, const int32_t* u_rowptr, const int32_t* dst_order,
                               const int32_t* dst_rowptr, const int32_t* k, const int32_t* order, const int32_t* k_rowptr, float w,
                               float* pos_logit, float* neg_logit, float* loss, float* dZ, float* dH, int accumulate, void* ws,
                               size_t ws_bytes, void* stream) {
    using namespace dl;
    const char* const name = "dl_score_sampled_bpr_train";
    DL_REQUIRE(bpr::supported(K, d, (int)dtype), "%s serves fp32 tables with 1 <= K <= 64 and K d <= 2048 (got K=%d d=%d dtype=%d: %s_supported)",
               name, K, d, (int)dtype, name);
    DL_REQUIRE(N >= 1 && n_rows >= 0, "%s: N=%d n_rows=%d", name, N, n_rows);
    DL_REQUIRE(m >= 1 && m <= bpr::MAX_M, "%s serves 1 <= m <= %d negatives per row (a chunk of 64 lanes holds whole rows of m + 1 partners), got m=%d",
               name, bpr::MAX_M, m);
    DL_REQUIRE((long long)n_rows * m <= 0x7fffffffLL / (2 * K), "%s: %d x %d entries x %d coefficients exceed 2^31 - 1", name, n_rows, m, 2 * K);
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    DL_REQUIRE(Z && H && dZ && dH && loss && u_rowptr && dst_rowptr && k_rowptr, "NULL argument");
    if (n_rows > 0) DL_REQUIRE(src && dst && k && dst_order && order && pos_logit && neg_logit, "NULL list argument");
    const bpr::Carve c = bpr::carve(n_rows, m, N, K, d, ws);
    if (!ws || ws_bytes < c.bytes) {
        set_error("workspace too small: have %zu, need %zu (%s_workspace_bytes)", ws ? ws_bytes : (size_t)0, c.bytes, name);
        return DL_E_WORKSPACE;
    }
    const bpr::Lists LA = {src, dst, k, nullptr, u_rowptr, m, n_rows, N, bpr::rows_per_chunk(m)};
    return bpr::run((const float*)Z, (const float*)H, N, K, d, t, LA, dst_order, dst_rowptr, order, k_rowptr, w, pos_logit, neg_logit,
                    loss, dZ, dH, accumulate, c, (hipStream_t)stream);
}

}  // extern "C"
