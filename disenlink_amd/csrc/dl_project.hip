// Factor projection Z[n][k][:] = MLP_k(x[n]) on the matrix cores (model.py:13-15, 24-27, 106) — the
// only dense contraction of the path.  fp32 in / fp32 results: both layers as six exact bf16 products per term
// from three bf16 planes per operand (dl_tiles.h; fp32-grade accuracy), or — without a workspace or with
// DL_PROJECT_FP32_MFMA=1 — v_mfma_f32_32x32x2_f32, which is bit-for-bit a k-ordered fmaf chain; either way
// the result keeps the reference's fp32 semantics up to rounding / summation order.
//
// Two-layer form (Factor2), one kernel per arithmetic: project2_fwd_planes_kernel and project2_fwd_f32_kernel.  In both,
// one workgroup = 8 waves = 128 nodes x ONE factor k, looping over (a group
// of) 128-unit chunks of the hidden layer.  Waves are 4 x 2: node quarter wn, hidden half wh; each wave
// owns a (64 hidden) x (32 nodes) tile = two independent accumulators; two waves share a SIMD, so one
// wave's LDS reads and barrier waits hide behind the other's MFMA chain.
//   layer 1 (transposed):  hidT[hidden][node] = W1_k[hidden][F] . x^T            A = W1 rows, B = x rows
//   bias + ReLU in the accumulator registers
//   layer 2:               Z^T[d][node] += W2_k[d][hidden] . hidT                 B = the accumulator itself
// A 32x32 accumulator has its column on the lane and its rows in the 16 registers, which is exactly
// the B-operand shape of the next MFMA when that product sums over the accumulator's ROW index
// (register r supplies the k-pair {acc_row(r,0), acc_row(r,1)}); so the hidden activations never leave
// the register file — no [N, K*nhid] tensor is written to HBM and re-read, unlike two library GEMMs.
// The layer-1 operand tiles ([128 rows][32 features]: three bf16 planes at an 80-byte row pitch, or fp32 at
// 36 / 68 floats: aligned, conflict-free b128 reads) are double-buffered in LDS; the next step's tiles are copied
// there behind the current step's MFMAs (bf16 planes by LDS-DMA, PlaneDma; fp32 tiles through registers).  The
// fp32 path's W2 operand (A[i = d][k = hidden], 4 consecutive hidden units per register quad) is read straight
// from global memory, one d-tile ahead of its use.  The two hidden halves of a node's Z are added through LDS at
// the end (fixed order).
// Small graphs: the hidden chunks are split over G workgroups per (node tile, k) whose partial Z go to
// G slabs, added in slab order by z_slab_sum_kernel (no atomics; needs the workspace).
#include <algorithm>
#include <cstdlib>
#include "dl_common.h"
#include "dl_kernels.h"
#include "dl_project.h"

namespace dl {
namespace project {

constexpr int TH = 128;       // hidden units per chunk (2 wave halves x 64)

// stage rows [row0, row0+rows) x cols [col0, col0+cols) of a row-major [n_rows][n_cols] matrix into
// LDS with leading dimension ld (zero fill outside the matrix)
__device__ __forceinline__ void stage_tile(float* lds, int ld, const float* __restrict__ src, int n_rows, int n_cols,
                                           int row0, int col0, int rows, int cols) {
    for (int i = threadIdx.x; i < rows * cols; i += blockDim.x) {
        const int r = i / cols, c = i - r * cols;
        const int gr = row0 + r, gc = col0 + c;
        lds[r * ld + c] = (gr < n_rows && gc < n_cols) ? src[(size_t)gr * n_cols + gc] : 0.0f;
    }
}

// 4 consecutive floats src[base .. base+3] of a vector of length n, loaded unconditionally from a clamped
// address; zero4() afterwards clears what lies outside the vector.  Two steps so that the s_waitcnt of the
// load lands at the use, not at the issue.  VEC: n % 4 == 0 and base % 4 == 0 (one aligned dwordx4).
template <bool VEC>
__device__ __forceinline__ float4 load4_raw(const float* __restrict__ src, int base, int n) {
    if constexpr (VEC) {
        return *reinterpret_cast<const float4*>(src + (base < n ? base : 0));
    } else {
        float e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = src[base + i < n ? base + i : 0];
        return make_float4(e[0], e[1], e[2], e[3]);
    }
}
template <bool VEC>
__device__ __forceinline__ float4 zero4(const float4& q, int base, int n) {
    if constexpr (VEC) {
        const unsigned m = base < n ? 0xFFFFFFFFu : 0u;
        return make_float4(mask_bits(q.x, m), mask_bits(q.y, m), mask_bits(q.z, m), mask_bits(q.w, m));
    } else {
        return make_float4(mask_bits(q.x, base + 0 < n ? 0xFFFFFFFFu : 0u), mask_bits(q.y, base + 1 < n ? 0xFFFFFFFFu : 0u),
                           mask_bits(q.z, base + 2 < n ? 0xFFFFFFFFu : 0u), mask_bits(q.w, base + 3 < n ? 0xFFFFFFFFu : 0u));
    }
}

// The W2 operand of layer 2 for one hidden chunk, staged through LDS (round 5).  The planes of W2 lie in global memory as
// [3][K*D][nhid_p] bf16 with the hidden units in layer 2's k-slot order; a chunk's slice — D rows x 128 hidden x 3 planes —
// was read straight from there by every wave, one K = 16 group ahead of its use: 16 bytes per lane from 32 different rows
// per instruction (a quarter of every 128-byte line used), and a global round trip per group that no prefetch depth hid
// (stamps: 9,000 cycles per chunk for 48 MFMAs = 1,536 cycles of issue).  Now the whole workgroup
// copies the slice with fully coalesced 16-byte loads (issued between the MFMA blocks of the chunk's last layer-1 step) into
// the LDS tile buffer that step has just finished reading, and layer 2 takes its A operands from there with ds_read_b128.
template <int D, int THREADS>
struct W2Stage {
    static constexpr int PIECES = 3 * D * 16;                  // 16-byte pieces: 3 planes x D rows x (128 hidden / 8)
    static constexpr int PER = PIECES / THREADS;
    static constexpr int PITCH = 128 + 8;                      // LDS row pitch (bf16): 68 dwords -> conflict-free b128 reads
    static_assert(PIECES % THREADS == 0, "the slice divides over the workgroup");
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    u32x4 v[PER];
    __device__ __forceinline__ void fetch(const __bf16* __restrict__ w2, size_t plane_stride, size_t row0, int nhid_p, int col0, int tid) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int q = tid + THREADS * j, p = q / (D * 16), r = (q % (D * 16)) / 16, c = (q % 16) * 8;
            v[j] = *reinterpret_cast<const u32x4*>(w2 + p * plane_stride + (row0 + r) * nhid_p + col0 + c);
        }
    }
    __device__ __forceinline__ void stash(__bf16* lds, int tid) const {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int q = tid + THREADS * j, p = q / (D * 16), r = (q % (D * 16)) / 16, c = (q % 16) * 8;
            *reinterpret_cast<u32x4*>(lds + (p * D + r) * PITCH + c) = v[j];
        }
    }
};

// Layer-1 tiles by LDS-DMA (round 6; it replaced a register-staged form).  A [3][128][32] bf16 plane tile
// (24 KB, contiguous in the plane array) goes to its padded LDS image — 384 rows of 80 bytes: 4 data pieces + 1 pad piece of
// 16 bytes — by 30 global_load_lds_dwordx4 wave-instructions: the LDS side of such an instruction is linear (wave-uniform
// base + 16 bytes per lane), the GLOBAL address is per lane, so lane l of instruction i fetches the piece that belongs at
// padded position i * 64 + l (a pad position fetches its row's last piece again: a fifth of the requests buy nothing, all of
// them L2 hits).  No staging registers (the register form held a whole tile pair: 30 registers), no ds_write pass, and no
// vmcnt(0) in the middle of a step waiting for the tile loads: stamps of the register form showed 1,000-2,200 of a step's
// 3,800 cycles in "stash" + "fetch issue".  Wave w issues instructions w, w + 8, w + 16, w + 24 of each tile.
struct PlaneDma {
    static constexpr int PIECES = 3 * PLANE_ROWS * 5;           // padded 16-byte positions of a tile
    static constexpr int INSTR = PIECES / DL_WAVE;               // 30
    static constexpr int PER_WAVE = (INSTR + NTHR / DL_WAVE - 1) / (NTHR / DL_WAVE);
    static_assert(PIECES % DL_WAVE == 0 && SPLIT_COLS == 32 && SPLIT_PITCH == 40, "80-byte LDS rows of 64-byte tile rows");
    unsigned off[PER_WAVE];                                     // byte offset of this lane's piece inside the global tile
    __device__ __forceinline__ void init(int wave, int lane) {
#pragma unroll
        for (int j = 0; j < PER_WAVE; ++j) {
            const unsigned pos = (unsigned)((wave + (NTHR / DL_WAVE) * j) * DL_WAVE + lane), row = pos / 5u, slot = pos - row * 5u;
            off[j] = (row * 4u + (slot < 4u ? slot : 3u)) * 16u;
        }
    }
    __device__ __forceinline__ void issue(const __bf16* __restrict__ tile, __bf16* lds_tile, int wave) const {
        typedef const __attribute__((address_space(1))) void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
#pragma unroll
        for (int j = 0; j < PER_WAVE; ++j) {
            const int i = wave + (NTHR / DL_WAVE) * j;           // wave-uniform
            if (i < INSTR)
                __builtin_amdgcn_global_load_lds((gptr_t)(reinterpret_cast<const char*>(tile) + off[j]),
                                                 (lptr_t)(reinterpret_cast<char*>(lds_tile) + i * (DL_WAVE * 16)), 16, 0, 0);
        }
    }
};

// ---- what the two forward kernels share ----------------------------------------------------------------------
// Both take one argument list (one launcher, one dispatch): W1 [K][nhid][F], b1 [K][nhid], W2 [K][D][nhid], b2 [K][D];
// 1-D grid of xcd_grid(node tiles of 128, K * G hidden-chunk groups); out: Z [N][K][D] with b2 != nullptr (G == 1), or slab
// [G][N][K][D] of partial sums with b2 == nullptr; hid_out != nullptr: the hidden layer is kept, hidT [K][nhid][ldh].
struct FwdPlanes {
    const __bf16* x; const __bf16* w; size_t w_batch; int ncb;     // tile-major planes of x and of the K matrices W1_k
    const __bf16* w2; size_t w2_ps; int nhid_p;                    // planes [3][K*D][nhid_p] of W2 in layer 2's k-slot order
};

// bias + ReLU on hidT (row = hidden unit, column = node) in the accumulator registers: quad g of a tile = its hidden rows
// 8g + 4*half .. +3, b their biases (zero past nhid)
__device__ __forceinline__ void bias_relu(f32x16& acc, int g, const float4& b) {
    acc[4 * g + 0] = fmaxf(acc[4 * g + 0] + b.x, 0.0f);
    acc[4 * g + 1] = fmaxf(acc[4 * g + 1] + b.y, 0.0f);
    acc[4 * g + 2] = fmaxf(acc[4 * g + 2] + b.z, 0.0f);
    acc[4 * g + 3] = fmaxf(acc[4 * g + 3] + b.w, 0.0f);
}

// Z hand-over, after the last step's barrier.  The two hidden halves (wh = 0, 1) of a node quarter hold partial Z sums: wave
// wh = 1 hands its half over through LDS (z_give; red is [wn][dt][16][64]), the workgroup meets at a barrier, and wave wh = 0
// adds (fixed order), adds b2 (nullptr: a slab of partial sums) and stores its node's row orow of factor k (z_take;
// registers 4g..4g+3 are 4 consecutive dd of node column li).
template <int DT>
__device__ __forceinline__ void z_give(float* red, const f32x16 (&zacc)[DT], int wn, int lane) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[((wn * DT + dt) * 16 + r) * 64 + lane] = zacc[dt][r];
}
// registers 4g .. 4g+3 of acc + the four values handed over for them (rows row .. row+3 of red) + bb -> 4 consecutive dd at o4
__device__ __forceinline__ void z_take(float* o4, const f32x16& acc, int g, const float* red, int row, int lane, const float4& bb) {
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = acc[4 * g + j] + red[(row + j) * 64 + lane];
    *reinterpret_cast<float4*>(o4) = make_float4(o[0] + bb.x, o[1] + bb.y, o[2] + bb.z, o[3] + bb.w);
}

// ---- the bf16-plane forward ----------------------------------------------------------------------------------
// Both layers on the bf16 matrix path from three bf16 planes per operand (dl_tiles.h: fp32-grade accuracy at a multiple of
// the fp32 MFMA rate).  x and W1 arrive as padded, tile-major plane arrays (dl_planes.hip) and their [128][32] tiles are
// copied without masks, so no instantiation depends on the alignment of F or nhid; of the fp32 arguments only the biases
// are read.  LDS: two parity buffers, each [3][TN][SPLIT_PITCH] (x tile) followed by [3][TH][SPLIT_PITCH] (W1 tile) — one
// buffer is one contiguous block, it also takes the W2 slice of a chunk's layer 2 (W2Stage) — and behind them bias_s, the
// 128 biases of the current hidden chunk.
constexpr size_t project2_planes_lds(int D) {
    const size_t red = sizeof(float) * 4 * (D / 32) * 16 * 64;                 // the Z hand-over at the end
    const size_t stage = sizeof(__bf16) * 2 * 3 * (TN + TH) * SPLIT_PITCH + sizeof(float) * TH;
    return stage > red ? stage : red;
}

template <int D>
__global__ __launch_bounds__(NTHR) void project2_fwd_planes_kernel(const float* __restrict__ /* x */, int N, int /* F */, int nhid,
                                                                   const float* __restrict__ /* W1 */, const float* __restrict__ b1,
                                                                   const float* __restrict__ /* W2 */, const float* __restrict__ b2,
                                                                   float* __restrict__ out, int K, int G, int chunks_per_group,
                                                                   float* __restrict__ hid_out, int ldh, FwdPlanes P) {
    constexpr int DT = D / 32;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int XBUF = 3 * TN * SPLIT_PITCH, PBUF = 3 * (TN + TH) * SPLIT_PITCH;
    __bf16* pbuf = reinterpret_cast<__bf16*>(lds);
    constexpr bool W2LDS = D <= 64 && (size_t)W2Stage<D, NTHR>::PITCH * 3 * D <= (size_t)PBUF;
    float* bias_s = reinterpret_cast<float*>(pbuf + 2 * PBUF);
    float bias_q = 0.0f;
    const XcdItem item = xcd_item(blockIdx.x, (N + TN - 1) / TN, K * G);
    if (!item.valid) return;
    const int k = item.b % K, grp = item.b / K;
    const int n0 = item.a * TN;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, half = lane >> 5;
    const int wn = wave >> 1, wh = wave & 1;
    const float* b1k = b1 + (size_t)k * nhid;
    const int nfc = P.ncb, nhc = (nhid + TH - 1) / TH;
    const int hc0 = grp * chunks_per_group;
    const int steps = nfc * max(0, min(chunks_per_group, nhc - hc0));

    static_assert(TN == PLANE_ROWS && TH == PLANE_ROWS, "tiles of the plane arrays");
    PlaneDma dma;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    dma.init(wave_s, lane);
    // both tiles of step s straight into its parity buffer (which every wave left at the barrier before)
    auto dma_tile = [&](int s) {
        const int hc = hc0 + s / nfc, fc = s % nfc;
        dma.issue(P.x + plane_tile<SPLIT_COLS>(item.a, fc, P.ncb), pbuf + (s & 1) * PBUF, wave_s);
        dma.issue(P.w + (size_t)k * P.w_batch + plane_tile<SPLIT_COLS>(hc, fc, P.ncb), pbuf + (s & 1) * PBUF + XBUF, wave_s);
    };

    f32x16 hacc[2], zacc[DT];
#pragma unroll
    for (int ht = 0; ht < 2; ++ht) zero_acc(hacc[ht]);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) zero_acc(zacc[dt]);

    if (steps > 0) {
        dma_tile(0);                                              // tiles 0 and 1 on their way into the two buffers together
        if (steps > 1) dma_tile(1);
    }
    wait_vmem();
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int hc = hc0 + s / nfc, fc = s % nfc;
        const bool last = fc == nfc - 1;
        const int hbase = hc * TH + wh * 64;                    // first hidden unit of this wave's tile
        // tile s + 1 into the other buffer — free since the barrier that ended step s - 1 — with the whole step to land
        // (tile 1 left in the prologue); the barrier at the end of this step waits for it (vmcnt(0) + s_barrier)
        if (s >= 1 && s + 1 < steps) dma_tile(s + 1);
        // Apart from the tile, nothing is requested from global memory at the top of a step.  s_waitcnt vmcnt counts in
        // issue order, and the compiler cannot tell loads apart at the join of the `last` branch (it waits for vmcnt(0)): with
        // the register-staged tiles this kernel had before LDS-DMA, a load issued HERE made the mid-step stash of the next tile
        // sit out a whole global round trip (stamps: +2,800 cycles in every chunk's last step).  The chunk's biases and the
        // W2 slice are requested between the step's MFMA blocks instead (below); the biases — asked for a step ahead — go to
        // LDS here, at the top of the chunk's last step.  (F <= 32, one step per chunk: requested here, staged before their use.)
        if (tid < TH) {
            if (nfc == 1) {
                const int h = hc * TH + tid;
                bias_q = b1k[h < nhid ? h : 0];
                bias_q = h < nhid ? bias_q : 0.0f;
            } else if (last) {
                bias_s[tid] = bias_q;
            }
        }
        // the A operand of layer 2 for group grp = (d-tile, hidden tile, K = 16 block): one 16-byte load per plane
        auto load_w2p = [&](bf16x8 (&a)[3], int grp) {
            const int dt = grp >> 2, ht = (grp >> 1) & 1, b = grp & 1;
            if constexpr (W2LDS) {                               // the slice staged in this step's (already read) tile buffer
                const __bf16* src = pbuf + (s & 1) * PBUF + (dt * 32 + li) * W2Stage<D, NTHR>::PITCH + wh * 64 + ht * 32 + 16 * b + 8 * half;
#pragma unroll
                for (int p = 0; p < 3; ++p) a[p] = *reinterpret_cast<const bf16x8*>(src + p * D * W2Stage<D, NTHR>::PITCH);
            } else {
                const __bf16* src = P.w2 + ((size_t)k * D + dt * 32 + li) * P.nhid_p + hbase + ht * 32 + 16 * b + 8 * half;
#pragma unroll
                for (int p = 0; p < 3; ++p) a[p] = *reinterpret_cast<const bf16x8*>(src + p * P.w2_ps);
            }
        };
        constexpr int W2PF = 1;     // groups in flight (the first issued a layer-1 step ahead; three measured no faster)
        bf16x8 w2a[W2PF + 1][3];
        W2Stage<D, NTHR> w2st;
        // lane half h supplies features 8h .. 8h+7 of each 16-wide block: A = W1 rows (two hidden tiles), B = x rows
        const __bf16* xb = pbuf + (s & 1) * PBUF + (wn * 32 + li) * SPLIT_PITCH + half * 8;
        const __bf16* wb = pbuf + (s & 1) * PBUF + XBUF + (wh * 64 + li) * SPLIT_PITCH + half * 8;
        // both K = 16 blocks of the chunk are read up front: block 1's LDS latency hides behind block 0's MFMAs
        bf16x8 a0[2][3], a1[2][3], b[2][3];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                b[kb][p] = *reinterpret_cast<const bf16x8*>(xb + p * TN * SPLIT_PITCH + kb * 16);
                a0[kb][p] = *reinterpret_cast<const bf16x8*>(wb + p * TH * SPLIT_PITCH + kb * 16);
                a1[kb][p] = *reinterpret_cast<const bf16x8*>(wb + (p * TH + 32) * SPLIT_PITCH + kb * 16);
            }
        mfma_split6(hacc[0], a0[0], b[0]);
        mfma_split6(hacc[1], a1[0], b[0]);
        // the step's other global requests, between the two MFMA blocks (see the top of the step): the chunk's 128
        // biases — one float per thread of the first two waves, a step ahead of their use — and, in the chunk's last
        // step, the W2 operand of layer 2.  (Staging in waves 4..7 before their first MFMA block instead, beside their
        // SIMD partners' MFMAs, measured slower: 90.7 -> 95.4 us at the bench shape, 675 -> 748 at F = 2,088, 845 -> 868
        // at d = 128.)  Kept a lambda: written inline, the same code compiles to a different register allocation.
        auto stage_work = [&]() {
            if (nfc >= 2 && fc == nfc - 2 && tid < TH) {
                const int h = hc * TH + tid;
                bias_q = b1k[h < nhid ? h : 0];
                bias_q = h < nhid ? bias_q : 0.0f;
            }
            if (last) {
                if constexpr (W2LDS) {
                    w2st.fetch(P.w2, P.w2_ps, (size_t)k * D, P.nhid_p, hc * TH, tid);  // coalesced; lands under the rest of the step
                } else {
#pragma unroll
                    for (int q = 0; q < W2PF; ++q) load_w2p(w2a[q], q);
                }
            }
        };
        stage_work();
        mfma_split6(hacc[0], a0[1], b[1]);
        mfma_split6(hacc[1], a1[1], b[1]);
        if (last) {
            if (nfc == 1 && tid < TH) bias_s[tid] = bias_q;
            __syncthreads();        // the biases are staged; every wave has this step's operands in registers: the tile buffer is free
            float4 bias[2][4];                                  // staged as zeros past nhid
#pragma unroll
            for (int ht = 0; ht < 2; ++ht)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    bias[ht][g] = *reinterpret_cast<const float4*>(bias_s + wh * 64 + ht * 32 + 8 * g + 4 * half);
#pragma unroll
            for (int ht = 0; ht < 2; ++ht)
#pragma unroll
                for (int g = 0; g < 4; ++g) bias_relu(hacc[ht], g, bias[ht][g]);
            if (hid_out != nullptr) {                           // keep the hidden layer for the backward: hidT[k][h][n]
                const int n = n0 + wn * 32 + li;
#pragma unroll
                for (int ht = 0; ht < 2; ++ht)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int h = hbase + ht * 32 + acc_row(r, half);
                        if (h < nhid && n < N) hid_out[((size_t)k * nhid + h) * ldh + n] = hacc[ht][r];
                    }
            }
            // layer 2 straight from the registers, on the bf16 matrix path too: the post-ReLU accumulators split into
            // their three planes (slot s of block b = register 8b + s), W2 comes pre-split in the matching order.  Written out,
            // not split_acc_block (dl_project.h): through it the d <= 64 forms lose two waits and d = 64 takes four more registers.
            bf16x8 hp[2][2][3];
#pragma unroll
            for (int ht = 0; ht < 2; ++ht)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int s8 = 0; s8 < 8; ++s8) {
                        __bf16 hi, mid, lo;
                        split3(hacc[ht][8 * b + s8], hi, mid, lo);
                        hp[ht][b][0][s8] = hi; hp[ht][b][1][s8] = mid; hp[ht][b][2][s8] = lo;
                    }
            if constexpr (W2LDS) {
                // the slice was requested between this step's MFMA blocks (half a layer-1 step, the bias / ReLU and the plane split ago)
                w2st.stash(pbuf + (s & 1) * PBUF, tid);
                __syncthreads();                                 // the staged slice is complete
#pragma unroll
                for (int q = 0; q < W2PF; ++q) load_w2p(w2a[q], q);
            }
#pragma unroll
            for (int grp = 0; grp < 4 * DT; ++grp) {
                if (grp + W2PF < 4 * DT) load_w2p(w2a[(grp + W2PF) % (W2PF + 1)], grp + W2PF);
                mfma_split6(zacc[grp >> 2], w2a[grp % (W2PF + 1)], hp[(grp >> 1) & 1][grp & 1]);
            }
#pragma unroll
            for (int ht = 0; ht < 2; ++ht) zero_acc(hacc[ht]);
        }
        // LDS-DMA data is ordered for a ds_read only by the issuing wave's vmcnt followed by a barrier the reader has passed;
        // the workgroup fence of __syncthreads() waits for LDS operations only.  (hipcc already emitted this wait here, for
        // the pending bias load: written out so that the tile of step s + 1 does not depend on that.)
        wait_vmem();
        __syncthreads();
    }
    if (wh == 1) z_give<DT>(lds, zacc, wn, lane);
    __syncthreads();
    const int n = n0 + wn * 32 + li;
    if (wh == 0 && n < N) {
        float* orow = out + (((size_t)grp * N + n) * K + k) * D;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = dt * 32 + 8 * g + 4 * half;
                float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
                if (b2 != nullptr) bb = *reinterpret_cast<const float4*>(b2 + (size_t)k * D + dd);
                z_take(orow + dd, zacc[dt], g, lds, (wn * DT + dt) * 16 + 4 * g, lane, bb);
            }
    }
}

// ---- the fp32-MFMA forward -----------------------------------------------------------------------------------
// Both layers by v_mfma_f32_32x32x2_f32, straight from x, W1 and W2 (no workspace, no planes).  VEC: F % 4 == 0 and
// nhid % 4 == 0 (tile rows, W2 rows and b1 are sequences of aligned quads).  LDS: xs [2][TN][LDT], w1s [2][TH][LDT].
constexpr size_t project2_f32_lds(int D) {
    const size_t red = sizeof(float) * 4 * (D / 32) * 16 * 64;                 // the Z hand-over at the end
    const size_t stage = sizeof(float) * (2 * TN + 2 * TH) * (fwd_fc(D) + 4);
    return stage > red ? stage : red;
}

template <int D, bool VEC>
__global__ __launch_bounds__(NTHR) void project2_fwd_f32_kernel(const float* __restrict__ x, int N, int F, int nhid,
                                                                const float* __restrict__ W1, const float* __restrict__ b1,
                                                                const float* __restrict__ W2, const float* __restrict__ b2,
                                                                float* __restrict__ out, int K, int G, int chunks_per_group,
                                                                float* __restrict__ hid_out, int ldh, FwdPlanes /* none */) {
    constexpr int DT = D / 32;
    constexpr int FC = fwd_fc(D), LDT = FC + 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* xs = lds;
    float* w1s = xs + 2 * TN * LDT;
    const XcdItem item = xcd_item(blockIdx.x, (N + TN - 1) / TN, K * G);
    if (!item.valid) return;
    const int k = item.b % K, grp = item.b / K;
    const int n0 = item.a * TN;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, half = lane >> 5;
    const int wn = wave >> 1, wh = wave & 1;
    const float* W1k = W1 + (size_t)k * nhid * F;
    const float* W2k = W2 + (size_t)k * D * nhid;
    const float* b1k = b1 + (size_t)k * nhid;
    const int nfc = (F + FC - 1) / FC, nhc = (nhid + TH - 1) / TH;
    const int hc0 = grp * chunks_per_group;
    const int steps = nfc * max(0, min(chunks_per_group, nhc - hc0));

    // the fp32 tiles of step s into registers, and from there into its parity buffer
    TileStage<TN, FC, VEC, NTHR> xt;
    TileStage<TH, FC, VEC, NTHR> wt;
    auto fetch = [&](int s) {
        const int hc = hc0 + s / nfc, fc = s % nfc;
        xt.fetch(x + (size_t)n0 * F + fc * FC, F, N - n0, F - fc * FC, tid);
        wt.fetch(W1k + (size_t)hc * TH * F + fc * FC, F, nhid - hc * TH, F - fc * FC, tid);
    };
    auto stash = [&](int s) {
        xt.template stash<LDT>(xs + (s & 1) * TN * LDT, tid);
        wt.template stash<LDT>(w1s + (s & 1) * TH * LDT, tid);
    };
    // W2_k[dt*32 + li][hidden quad g of tile ht]: the A operand of layer 2 for d-tile dt
    auto load_w2 = [&](float4 (&wv)[2][4], int dt, int hbase) {
#pragma unroll
        for (int ht = 0; ht < 2; ++ht)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                wv[ht][g] = load4_raw<VEC>(W2k + (size_t)(dt * 32 + li) * nhid, hbase + ht * 32 + 8 * g + 4 * half, nhid);
    };

    f32x16 hacc[2], zacc[DT];
#pragma unroll
    for (int ht = 0; ht < 2; ++ht) zero_acc(hacc[ht]);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) zero_acc(zacc[dt]);

    // Software pipeline (one register set per tile, write-after-barrier): during step s the registers hold
    // tile s+1, whose global loads were issued one step earlier; it goes to the other LDS buffer in the shadow
    // of the first MFMA block of step s (every wave left that buffer at the barrier before), and the loads of
    // tile s+2 are issued right behind it.
    if (steps > 0) {
        fetch(0);
        stash(0);
        if (steps > 1) fetch(1);
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int hc = hc0 + s / nfc, fc = s % nfc;
        const bool last = fc == nfc - 1;
        const int hbase = hc * TH + wh * 64;                    // first hidden unit of this wave's tile
        float4 bias[2][4], wnext[2][4];                         // quad g of tile ht = hidden rows 8g+4*half .. +3
        if (last) {                                             // raw loads, a whole step ahead; zero4 at the use
#pragma unroll
            for (int ht = 0; ht < 2; ++ht)
#pragma unroll
                for (int g = 0; g < 4; ++g) bias[ht][g] = load4_raw<VEC>(b1k, hbase + ht * 32 + 8 * g + 4 * half, nhid);
            load_w2(wnext, 0, hbase);
        }
        Layer1F32<FC, LDT, 2, false> l1{xs + (s & 1) * TN * LDT + (wn * 32 + li) * LDT + half * (FC / 2),
                                        w1s + (s & 1) * TH * LDT + (wh * 64 + li) * LDT + half * (FC / 2)};
        l1.read_block(0);
#pragma unroll
        for (int j = 0; j < l1.NB; ++j) {
            if (j + 1 < l1.NB) l1.read_block(j + 1);
            l1.mfma_block(hacc, j);
            if (j == 0) {
                if (s + 1 < steps) stash(s + 1);
                if (s + 2 < steps) fetch(s + 2);
            }
        }
        if (last) {
#pragma unroll
            for (int ht = 0; ht < 2; ++ht)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bias[ht][g] = zero4<VEC>(bias[ht][g], hbase + ht * 32 + 8 * g + 4 * half, nhid);
                    bias_relu(hacc[ht], g, bias[ht][g]);
                }
            if (hid_out != nullptr) {                           // keep the hidden layer for the backward: hidT[k][h][n]
                const int n = n0 + wn * 32 + li;
#pragma unroll
                for (int ht = 0; ht < 2; ++ht)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int h = hbase + ht * 32 + acc_row(r, half);
                        if (h < nhid && n < N) hid_out[((size_t)k * nhid + h) * ldh + n] = hacc[ht][r];
                    }
            }
            // layer 2 straight from the registers
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                float4 wv[2][4];
#pragma unroll
                for (int ht = 0; ht < 2; ++ht)
#pragma unroll
                    for (int g = 0; g < 4; ++g) wv[ht][g] = zero4<VEC>(wnext[ht][g], hbase + ht * 32 + 8 * g + 4 * half, nhid);
                if (dt + 1 < DT) load_w2(wnext, dt + 1, hbase);
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int ht = 0; ht < 2; ++ht) {
                        DL_MFMA(zacc[dt], wv[ht][g].x, hacc[ht][4 * g + 0]);
                        DL_MFMA(zacc[dt], wv[ht][g].y, hacc[ht][4 * g + 1]);
                        DL_MFMA(zacc[dt], wv[ht][g].z, hacc[ht][4 * g + 2]);
                        DL_MFMA(zacc[dt], wv[ht][g].w, hacc[ht][4 * g + 3]);
                    }
            }
#pragma unroll
            for (int ht = 0; ht < 2; ++ht) zero_acc(hacc[ht]);
        }
        __syncthreads();
    }
    if (wh == 1) z_give<DT>(lds, zacc, wn, lane);
    __syncthreads();
    const int n = n0 + wn * 32 + li;
    if (wh == 0 && n < N) {
        float* orow = out + (((size_t)grp * N + n) * K + k) * D;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = dt * 32 + 8 * g + 4 * half;
                float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
                if (b2 != nullptr) bb = *reinterpret_cast<const float4*>(b2 + (size_t)k * D + dd);
                z_take(orow + dd, zacc[dt], g, lds, (wn * DT + dt) * 16 + 4 * g, lane, bb);
            }
    }
}

// Z[n][c] = b2[c] + sum_g slab[g][n][c] (g ascending), c over K*D; 4 columns per thread.
__global__ __launch_bounds__(256) void z_slab_sum_kernel(const float* __restrict__ slab, int G, size_t NC, int C,
                                                         const float* __restrict__ b2, float* __restrict__ Z) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= NC) return;
    float4 acc = *reinterpret_cast<const float4*>(b2 + i % C);
    for (int g = 0; g < G; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(slab + (size_t)g * NC + i);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(Z + i) = acc;
}

// Single-layer projection (Factor): W [K][D][F], b [K][D]:  Z[n][k][:] = W_k x[n] + b_k.
template <int D>
__global__ __launch_bounds__(256) void project1_fwd_kernel(const float* __restrict__ x, int N, int F,
                                                           const float* __restrict__ W, const float* __restrict__ b,
                                                           float* __restrict__ Z, int K) {
    constexpr int DT = D / 32;
    constexpr int TILE_N = 128;                               // nodes per workgroup (4 waves x 32)
    constexpr int FC = D == 128 ? 32 : 64;                    // keep xs + ws inside 64 KiB of static LDS
    __shared__ float xs[TILE_N * (FC + 1)];
    __shared__ float ws[D * (FC + 1)];
    const int k = blockIdx.y;
    const int n0 = blockIdx.x * TILE_N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 31, half = lane >> 5;
    const float* Wk = W + (size_t)k * D * F;
    f32x16 zacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) zacc[dt][r] = 0.0f;
    for (int f0 = 0; f0 < F; f0 += FC) {
        __syncthreads();
        stage_tile(xs, FC + 1, x, N, F, n0, f0, TILE_N, FC);
        stage_tile(ws, FC + 1, Wk, D, F, 0, f0, D, FC);
        __syncthreads();
        const float* xa = xs + (wave * 32 + li) * (FC + 1) + half;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const float* wa = ws + (dt * 32 + li) * (FC + 1) + half;
#pragma unroll 8
            for (int s = 0; s < FC / 2; ++s)
                zacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[2 * s], xa[2 * s], zacc[dt], 0, 0, 0);
        }
    }
    const int n = n0 + wave * 32 + li;
    if (n < N) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int dd = dt * 32 + 8 * g4 + 4 * half;
                const float4 bb = *reinterpret_cast<const float4*>(b + (size_t)k * D + dd);
                float4 o;
                o.x = zacc[dt][4 * g4 + 0] + bb.x;
                o.y = zacc[dt][4 * g4 + 1] + bb.y;
                o.z = zacc[dt][4 * g4 + 2] + bb.z;
                o.w = zacc[dt][4 * g4 + 3] + bb.w;
                *reinterpret_cast<float4*>(Z + ((size_t)n * K + k) * D + dd) = o;
            }
        }
    }
}

}  // namespace project

// Layer-1 products from three bf16 planes per operand (default) or plain fp32 MFMA (DL_PROJECT_FP32_MFMA=1).
bool split_products() {
    return !config().project_fp32_mfma;
}

bool project_supported(int d) { return d == 32 || d == 64 || d == 128; }

// Hidden-chunk groups per (node tile, factor): 1 when the grid already covers the 256 CUs twice over, else
// enough groups to get there (each group = whole 128-unit chunks; measured at N=5,201: 2 groups beat 1 and 4).
static int project2_groups(int N, int K, int nhid) {
    const long long wg = (long long)((N + project::TN - 1) / project::TN) * K;
    const int nhc = (nhid + project::TH - 1) / project::TH;
    if (config().fwd_groups > 0) return std::max(1, std::min(nhc, config().fwd_groups));           // DL_FWD_GROUPS: tuning knob
    if (wg >= 512) return 1;
    const int cpg = std::max(1, (int)(nhc / std::min<long long>(nhc, (512 + wg - 1) / wg)));
    return (nhc + cpg - 1) / cpg;
}

// Node block of the two-layer forward: the x planes are made per block of rows, so the workspace does not grow with
// the graph (2.9M nodes x 288 features would be 5 GB of planes).  Large graphs only — they never use the group split.
static int fwd_block_rows(int N) {
    long long rows = 1 << 17;
    if (config().fwd_block_rows > 0) rows = config().fwd_block_rows * project::TN;                  // DL_FWD_BLOCK_ROWS (tests: force blocking)
    return N <= 2 * rows ? N : (int)rows;
}

// Workspace of the two-layer forward: [Z slabs of the G groups][x planes of one node block][W1 planes]
struct FwdLayout { int G, R, nhid_p; size_t off_xp, off_wp, off_w2p, bytes; };
static FwdLayout fwd_layout(int N, int F, int K, int nhid, int d) {
    FwdLayout L{};
    L.R = fwd_block_rows(N);
    L.G = L.R < N ? 1 : project2_groups(N, K, nhid);
    size_t off = L.G > 1 ? align256(sizeof(float) * (size_t)L.G * N * K * d) : 0;
    L.off_xp = off;
    if (split_products()) {
        off += align256(sizeof(__bf16) * project::plane_array_elems(L.R, F, project::SPLIT_COLS));
        L.off_wp = off;
        off += align256(sizeof(__bf16) * K * project::plane_array_elems(nhid, F, project::SPLIT_COLS));
        L.off_w2p = off;
        L.nhid_p = (int)project::round_up(nhid, project::TH);
        off += align256(sizeof(__bf16) * 3 * (size_t)K * d * L.nhid_p);
    }
    L.bytes = off;
    return L;
}

size_t project_fwd_workspace_bytes(int N, int F, int K, int nhid, int d, bool two_layer) {
    if (!two_layer || N <= 0) return 0;
    return fwd_layout(N, F, K, nhid, d).bytes;
}

// What the two-layer forward does with a workspace of ws_bytes: which kernel runs (split: project2_fwd_planes_kernel<D>,
// where vec selects nothing; else project2_fwd_f32_kernel<D, vec>), over how many hidden-chunk groups, in how many launches of
// how many rows, and whether persistent x planes serve it.  project_fwd dispatches on exactly this.  A layout of 0 bytes (fp32 MFMA, one group) needs no workspace, so it fits with or without one:
// the form then does not depend on whether the caller's empty workspace has an address.
struct FwdForm { bool fits, split, vec, xplanes; int G, cpg, R, launches; };
static FwdForm fwd_form(const FwdLayout& L, int N, int F, int nhid, bool have_ws, size_t ws_bytes, bool have_xplanes) {
    FwdForm f{};
    f.fits = (have_ws || L.bytes == 0) && ws_bytes >= L.bytes;
    f.split = split_products() && f.fits;                   // no workspace: fp32 MFMA straight from x and W1
    f.vec = (f.split || F % 4 == 0) && (nhid % 4 == 0);     // quads never straddle a row end
    f.G = f.fits ? L.G : 1;                                 // no workspace: one group
    const int nhc = (nhid + project::TH - 1) / project::TH;
    f.cpg = (nhc + f.G - 1) / f.G;
    f.R = f.fits ? L.R : N;                                 // rows per launch (G == 1 whenever R < N)
    f.launches = f.R > 0 ? (N + f.R - 1) / f.R : 0;
    f.xplanes = f.split && f.R >= N && have_xplanes;        // one node block on planes: x was split once for the run
    return f;
}

// ws_bytes = 0 stands for "no workspace" (ws == nullptr in project_fwd).
void project_fwd_form(int N, int F, int K, int nhid, int d, bool two_layer, size_t ws_bytes, bool have_xplanes, int* out) {
    if (!two_layer) {                                       // project1_fwd_kernel<d>: one launch, no workspace, no planes
        const int one[7] = {0, 0, 1, 0, N, 1, 0};
        std::copy(one, one + 7, out);
        return;
    }
    const FwdLayout L = fwd_layout(N, F, K, nhid, d);
    const FwdForm f = fwd_form(L, N, F, nhid, ws_bytes > 0, ws_bytes, have_xplanes);
    const int two[7] = {f.split, f.vec, f.G, f.cpg, f.R, f.launches, f.xplanes};
    std::copy(two, two + 7, out);
}

template <auto KERNEL, size_t LDS>
static void launch2_t(int N, int K, int G, int cpg, hipStream_t st, const float* x, int F, int nhid, const float* W1,
                      const float* b1, const float* W2, const float* b2, float* out, float* hid_out, int ldh,
                      project::FwdPlanes P) {
    using namespace project;
    static unsigned long long lds_done = 0;
    ensure_dynamic_lds(reinterpret_cast<const void*>(KERNEL), LDS, lds_done);
    const dim3 grid((unsigned)xcd_grid((N + TN - 1) / TN, K * G));
    hipLaunchKernelGGL(KERNEL, grid, dim3(NTHR), LDS, st, x, N, F, nhid, W1, b1, W2, b2, out, K, G, cpg, hid_out, ldh, P);
}

// Persistent planes of the (constant) feature matrix: [x planes, 32-column tiles | x^T planes, 16-column tiles], both
// tile-major and zero-padded like the per-call arrays (dl_tiles.h).  Only single-block problems use them (fwd_block_rows,
// bwd_block_rows): a blocked run re-splits the block it works on.
size_t project_xplanes_bytes(int N, int F) {
    using namespace project;
    if (N <= 0 || F <= 0) return 0;
    return align256(sizeof(__bf16) * plane_array_elems(N, F, SPLIT_COLS)) + align256(sizeof(__bf16) * plane_array_elems(F, N, PLANE_ROWS));
}
static size_t xplanes_xT_offset(int N, int F) {
    using namespace project;
    return align256(sizeof(__bf16) * plane_array_elems(N, F, SPLIT_COLS));
}
const void* project_xplanes_xT(const void* xplanes, int N, int F) {
    return xplanes ? static_cast<const char*>(xplanes) + xplanes_xT_offset(N, F) : nullptr;
}
int project_xplanes_build(const float* x, int N, int F, void* xplanes, hipStream_t st) {
    using namespace project;
    char* base = static_cast<char*>(xplanes);
    split_rows(x, 1, N, F, F, 0, reinterpret_cast<__bf16*>(base), st);
    split_transposed(x, N, F, F, reinterpret_cast<__bf16*>(base + xplanes_xT_offset(N, F)), st);
    return check_launch("project_xplanes_build");
}

int project_fwd(const float* x, int N, int F, int K, int nhid, int d, const float* W1, const float* b1,
                const float* W2, const float* b2, float* Z, void* ws, size_t ws_bytes, float* hid_out, hipStream_t st,
                const void* xplanes) {
    using namespace project;
    const int ldh = (N + 3) & ~3;
    if (W2 == nullptr) {          // single Linear(F -> d): W1 is [K][d][F], b1 is [K][d]
        const dim3 grid((unsigned)((N + 127) / 128), (unsigned)K), block(256);
        if (d == 32) hipLaunchKernelGGL(project1_fwd_kernel<32>, grid, block, 0, st, x, N, F, W1, b1, Z, K);
        else if (d == 64) hipLaunchKernelGGL(project1_fwd_kernel<64>, grid, block, 0, st, x, N, F, W1, b1, Z, K);
        else hipLaunchKernelGGL(project1_fwd_kernel<128>, grid, block, 0, st, x, N, F, W1, b1, Z, K);
        return check_launch("project_fwd");
    }
    const FwdLayout L = fwd_layout(N, F, K, nhid, d);
    const FwdForm form = fwd_form(L, N, F, nhid, ws != nullptr, ws_bytes, xplanes != nullptr);
    const bool split = form.split, vec = form.vec;
    const int G = form.G;
    FwdPlanes P{};
    if (split) {
        char* base = static_cast<char*>(ws);
        __bf16* xP = reinterpret_cast<__bf16*>(base + L.off_xp);
        __bf16* wP = reinterpret_cast<__bf16*>(base + L.off_wp);
        __bf16* w2P = reinterpret_cast<__bf16*>(base + L.off_w2p);
        if (form.R >= N) {                                  // one node block: all three operand splits in one launch
            if (form.xplanes) xP = const_cast<__bf16*>(static_cast<const __bf16*>(xplanes));     // x was split once for the run
            split_fwd_operands(form.xplanes ? nullptr : x, N, F, xP, W1, K, nhid, wP, W2, d, w2P, L.nhid_p, st);
        } else {
            split_rows(W1, K, nhid, F, F, (size_t)nhid * F, wP, st);
            split_w2(W2, K * d, nhid, w2P, L.nhid_p, st);
        }
        P = FwdPlanes{xP, wP, plane_array_elems(nhid, F, SPLIT_COLS), plane_chunks<SPLIT_COLS>(F, SPLIT_COLS),
                      w2P, (size_t)K * d * L.nhid_p, L.nhid_p};
    }
    const int cpg = form.cpg;
    float* out = G > 1 ? static_cast<float*>(ws) : Z;
    const float* bias2 = G > 1 ? nullptr : b2;
    const int R = form.R;
    for (int row0 = 0; row0 < N; row0 += R) {
        const int rows = std::min(R, N - row0);
        const float* xb = x + (size_t)row0 * F;
        float* ob = out + (size_t)row0 * K * d;
        float* hb = hid_out ? hid_out + row0 : nullptr;
        if (split && form.R < N) split_rows(xb, 1, rows, F, F, 0, const_cast<__bf16*>(P.x), st);
#define DL_P2(DD)                                                                                       \
    if (d == DD) {                                                                                      \
        if (split) launch2_t<project2_fwd_planes_kernel<DD>, project2_planes_lds(DD)>(rows, K, G, cpg, st, xb, F, nhid, W1, b1, W2, bias2, ob, hb, ldh, P);   \
        else if (vec) launch2_t<project2_fwd_f32_kernel<DD, true>, project2_f32_lds(DD)>(rows, K, G, cpg, st, xb, F, nhid, W1, b1, W2, bias2, ob, hb, ldh, P);  \
        else launch2_t<project2_fwd_f32_kernel<DD, false>, project2_f32_lds(DD)>(rows, K, G, cpg, st, xb, F, nhid, W1, b1, W2, bias2, ob, hb, ldh, P);          \
    }
        DL_P2(32) DL_P2(64) DL_P2(128)
#undef DL_P2
    }
    if (G > 1) {
        const size_t NC = (size_t)N * K * d;
        hipLaunchKernelGGL(z_slab_sum_kernel, dim3((unsigned)((NC / 4 + 255) / 256)), dim3(256), 0, st, out, G, NC, K * d, b2, Z);
    }
    return check_launch("project_fwd");
}

}  // namespace dl
