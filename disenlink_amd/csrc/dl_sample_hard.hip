// Hard training negatives drawn on the device (dl_sample_negatives_hard): c candidates per entry by the rule of
// dl_sample_negatives, the one the CURRENT tables score highest is kept — dynamic negative sampling without a plan build.
//
// Entry e = r m + j has the source u = src[r] and the candidates i < c (1 <= c <= 64): candidate i is sample_partner
// (dl_sample.h) with the Philox counter (e, i 64 + attempt, epoch low, epoch high) and the seed as key, so candidate 0 is, bit
// for bit, the draw dl_sample_negatives makes for e; a candidate that spends its 64 attempts is dead.  Kept: the live candidate
// with the largest x(u, k) = sum_f (h_f[u].h_f[k]) exp(z_f[u].z_f[k] / t) (fp32); ties go to the lowest i; a NaN logit ranks
// below every number, -inf included, and where every live logit is NaN the first live candidate is kept.  All c dead, or a
// src outside [0, N) (never read): k = -1, logit 0, one count in *n_failed (entries, not candidates).  Duplicated candidates
// are the same node with the same logit.  The result is a pure function of (seed, epoch, e, Z, H, t): the same bits on every
// call, whatever the grid; the one atomic is the integer n_failed (one add per wave).
//
// One wave owns a chunk of EPC = floor(64 / c) consecutive entries.  Lane ee c + i draws candidate i of the chunk's entry ee;
// the wave then walks its slots in order with readlane (as bpr_row_d64_kernel walks its rows): z[u], h[u] are loaded only where
// u changes (src is ascending), z[k], h[k] gathered per live candidate, the logit formed by the functions of dl_bpr_logit.h —
// d = 64 with K in {4, 8}: the lane geometry and reduction order of bpr_row_d64_kernel; every other shape: the generic order
// (per-factor wave all-reduce, factors added ascending) — so x_out is the ranking trainer's neg_logit for the same (u, k).  The
// running best is wave-uniform (lane 0's bits); lane ee keeps entry ee's result and the chunk is written with one store per
// array.  A plain serial walk: nothing of the next candidate is in flight while one is scored.
//
// Resources (gfx950, -O3, -Rpass-analysis=kernel-resource-usage; no scratch, no LDS) -> waves per SIMD:
//   sample_hard_d64_kernel<2>    46 VGPRs -> 8       sample_hard_d64_kernel<1>    26 VGPRs -> 8
//   sample_hard_generic_kernel   20 VGPRs -> 8
// (bpr_row_d64_kernel<2>: 142 VGPRs, 3 waves — no coefficients and no accumulators are held here.)
#include "dl_bpr_logit.h"
#include "dl_sample.h"

namespace dl {
namespace hard {

using bpr::factor_term_generic;
using bpr::load_row_d64;
using bpr::logit_d64;

struct Draw {
    const int32_t* src;                 // [n_rows] ascending
    const int32_t* ex_rowptr;           // [N+1] or NULL
    const int32_t* ex_col;
    const uint64_t* epoch_dev;
    int32_t* k_out;                     // [n_rows m]
    float* x_out;                       // [n_rows m] or NULL
    uint32_t* n_failed;
    uint32_t seed_lo, seed_hi;
    int n_entries, m, c, N, exclude_self;
    int epc;                            // entries per chunk: floor(64 / c)
};

// lane ee c + i: (the source, candidate i) of the chunk's entry ee; -1 = no entry, a source outside the table, a dead candidate
__device__ __forceinline__ void draw_candidates(const Draw& D, int e0, int ne, int lane, int& my_u, int& my_k) {
    my_u = my_k = -1;
    const int ee = lane / D.c, i = lane - ee * D.c;
    if (ee < ne) {
        const int e = e0 + ee;
        const int u = D.src[e / D.m];
        my_k = sample_partner((uint32_t)e, (uint32_t)i * SAMPLE_ATTEMPTS, D.epoch_dev[0], D.seed_lo, D.seed_hi, u, D.N, D.ex_rowptr,
                              D.ex_col, D.exclude_self);
        my_u = (u >= 0 && u < D.N) ? u : -1;
    }
}

// the order of the selection: x replaces the best so far where it is larger, or where the best is a NaN and x is not
__device__ __forceinline__ bool better(float x, float best) { return x > best || (best != best && x == x); }

// the chunk's results, entry ee in lane ee: one store per array, and one integer add for the wave's failed entries
__device__ __forceinline__ void write_chunk(const Draw& D, int e0, int ne, int lane, int res_k, float res_x) {
    const bool mine = lane < ne;
    if (mine) {
        D.k_out[e0 + lane] = res_k;
        if (D.x_out) D.x_out[e0 + lane] = res_x;
    }
    const int failed = __popcll(__ballot(mine && res_k < 0));
    if (lane == 0 && failed > 0) atomicAdd(D.n_failed, (uint32_t)failed);
}

// ---------------------------------------------------------------------------- d = 64, K = 4 NJ
template <int NJ>
__global__ __launch_bounds__(BLOCK) void sample_hard_d64_kernel(const float* __restrict__ Z, const float* __restrict__ H, float t, Draw D) {
    const int wave = wave_index(), lane = lane_id();
    const long long first = ((long long)blockIdx.x * WAVES_PER_BLOCK + wave) * D.epc;
    if (first >= D.n_entries) return;                               // (no barrier in this kernel)
    const int e0 = (int)first, ne = min(D.epc, D.n_entries - e0), c = D.c;
    int my_u, my_k;
    draw_candidates(D, e0, ne, lane, my_u, my_k);
    float4 uz[NJ], uh[NJ];
    int cur = -1, res_k = -1;
    float res_x = 0.0f;
    for (int ee = 0; ee < ne; ++ee) {
        const int u = __builtin_amdgcn_readlane(my_u, ee * c);
        int best_k = -1;
        float best_x = 0.0f;
        if (u >= 0) {
            if (u != cur) {
                cur = u;
                load_row_d64<NJ>(Z, u, lane, uz);
                load_row_d64<NJ>(H, u, lane, uh);
            }
#pragma unroll 1
            for (int i = 0; i < c; ++i) {
                const int kk = __builtin_amdgcn_readlane(my_k, ee * c + i);
                if (kk < 0) continue;                               // a dead candidate: nothing gathered
                float4 zv[NJ], hv[NJ];
                load_row_d64<NJ>(Z, kk, lane, zv);
                load_row_d64<NJ>(H, kk, lane, hv);
                float ex[NJ], ttv[NJ];
                const float x = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(logit_d64<NJ>(uz, uh, zv, hv, t, ex, ttv))));
                if (best_k < 0 || better(x, best_x)) {
                    best_k = kk;
                    best_x = x;
                }
            }
        }
        if (lane == ee) {
            res_k = best_k;
            res_x = best_x;
        }
    }
    write_chunk(D, e0, ne, lane, res_k, res_x);
}

// ---------------------------------------------------------------------------- any K, d with K d <= 2048
__global__ __launch_bounds__(BLOCK) void sample_hard_generic_kernel(const float* __restrict__ Z, const float* __restrict__ H, int K, int d,
                                                                    float t, Draw D) {
    const int ROW = K * d;
    const int wave = wave_index(), lane = lane_id();
    const long long first = ((long long)blockIdx.x * WAVES_PER_BLOCK + wave) * D.epc;
    if (first >= D.n_entries) return;                               // (no barrier in this kernel)
    const int e0 = (int)first, ne = min(D.epc, D.n_entries - e0), c = D.c;
    int my_u, my_k;
    draw_candidates(D, e0, ne, lane, my_u, my_k);
    int res_k = -1;
    float res_x = 0.0f;
    for (int ee = 0; ee < ne; ++ee) {
        const int u = __builtin_amdgcn_readlane(my_u, ee * c);
        int best_k = -1;
        float best_x = 0.0f;
        if (u >= 0) {
            const float* zu = Z + (size_t)u * ROW;
            const float* hu = H + (size_t)u * ROW;
            for (int i = 0; i < c; ++i) {
                const int kk = __builtin_amdgcn_readlane(my_k, ee * c + i);
                if (kk < 0) continue;
                const float* zk = Z + (size_t)kk * ROW;
                const float* hk = H + (size_t)kk * ROW;
                float logit = 0.0f;
                for (int f = 0; f < K; ++f) {
                    float ex;
                    factor_term_generic(zu, hu, zk, hk, f, d, lane, t, ex, logit);
                }
                const float x = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(logit)));
                if (best_k < 0 || better(x, best_x)) {
                    best_k = kk;
                    best_x = x;
                }
            }
        }
        if (lane == ee) {
            res_k = best_k;
            res_x = best_x;
        }
    }
    write_chunk(D, e0, ne, lane, res_k, res_x);
}

static bool supported(int K, int d, int dtype) {
    return dtype == DL_F32 && K >= 1 && K <= DL_MAX_FACTORS && d >= 1 && (long long)K * d <= 2048;
}

}  // namespace hard
}  // namespace dl

extern "C" {

int dl_sample_negatives_hard_supported(int K, int d, dl_dtype dtype) { return dl::hard::supported(K, d, (int)dtype) ? 1 : 0; }

int dl_sample_negatives_hard(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* src,
                             int n_rows, int m, int c, const int32_t* ex_rowptr, const int32_t* ex_col, uint64_t seed,
                             const uint64_t* epoch_dev, int exclude_self, int32_t* k_out, float* x_out, uint32_t* n_failed,
                             void* stream) {
    using namespace dl;
    const char* const name = "dl_sample_negatives_hard";
    DL_REQUIRE(hard::supported(K, d, (int)dtype), "%s serves fp32 tables with 1 <= K <= 64 and K d <= 2048 (got K=%d d=%d dtype=%d: %s_supported)",
               name, K, d, (int)dtype, name);
    DL_REQUIRE(n_rows >= 0 && m >= 1 && N >= 1, "%s: n_rows=%d m=%d N=%d", name, n_rows, m, N);
    DL_REQUIRE(c >= 1 && c <= DL_WAVE, "%s serves 1 <= c <= 64 candidates per entry (one lane draws one candidate), got c=%d", name, c);
    DL_REQUIRE((long long)n_rows * m <= 0x7fffffffLL, "%s: %d x %d entries exceed 2^31 - 1", name, n_rows, m);
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    DL_REQUIRE(Z && H && epoch_dev != nullptr && n_failed != nullptr, "NULL argument");
    if (n_rows == 0) return DL_OK;
    DL_REQUIRE(src && k_out, "NULL argument");
    const int E = n_rows * m, epc = DL_WAVE / c;
    const hard::Draw D = {src, ex_rowptr, ex_col, epoch_dev, k_out, x_out, n_failed, (uint32_t)seed, (uint32_t)(seed >> 32),
                          E, m, c, N, exclude_self, epc};
    const long long n_chunks = ((long long)E + epc - 1) / epc;
    const dim3 grid((unsigned)((n_chunks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)), block(BLOCK);
    const hipStream_t st = (hipStream_t)stream;
    if (d == 64 && K == 8) hipLaunchKernelGGL((hard::sample_hard_d64_kernel<2>), grid, block, 0, st, (const float*)Z, (const float*)H, t, D);
    else if (d == 64 && K == 4) hipLaunchKernelGGL((hard::sample_hard_d64_kernel<1>), grid, block, 0, st, (const float*)Z, (const float*)H, t, D);
    else hipLaunchKernelGGL(hard::sample_hard_generic_kernel, grid, block, 0, st, (const float*)Z, (const float*)H, K, d, t, D);
    return check_launch(name);
}

}  // extern "C"
