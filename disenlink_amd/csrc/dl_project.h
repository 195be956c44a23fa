// What the two-layer projection forward (dl_project.hip) and kernel A of its backward (dl_project_bwd.hip) share: the
// shape of a workgroup and the steps both run.  Register layout: dl_tiles.h.
#pragma once
#include "dl_common.h"
#include "dl_tiles.h"

namespace dl {
namespace project {

// One workgroup = 8 waves = 128 nodes: node quarter wn = wave >> 1 (32 nodes) x hidden half wh = wave & 1.
constexpr int TN = 128;
constexpr int NTHR = 512;
// Feature chunk of an fp32 layer-1 step (LDS row pitch of its operand tiles = chunk + 4 floats).  Forward: 64 (one barrier
// per 64 MFMAs of a wave) where the registers allow, else 32.  Kernel A: 32.
constexpr int fwd_fc(int D) { return D <= 64 ? 64 : 32; }
constexpr int BFC = 32;

// The pipelined fp32 layer-1 step on LDS tiles of FC features at a row pitch of LD floats:
//   acc[t] += (x rows of this node quarter) . (W1 rows of tile t)^T,  t < NT tiles of 32 hidden units.
// xb / wb = this lane's x row / its row of W1 tile 0, at the feature offset of its lane half (half * FC / 2): a lane half owns
// FC / 2 features of the chunk.  MFMA block j of NB takes 2 quads of them per operand row (1 + NT ds_read_b128 per quad,
// 8 * NT MFMAs).  X_IS_A: x is the A operand, the accumulator is [node][hidden] (kernel A); else W1 is, the accumulator is
// [hidden][node] (the forward).  The step, as both kernels write it:
//     l1.read_block(0);
//     for j < NB (unrolled):  if (j + 1 < NB) l1.read_block(j + 1);  l1.mfma_block(acc, j);  if (j == 0) { stash(s + 1); fetch(s + 2); }
// block j + 1's reads are issued ahead of block j's MFMAs, and the kernel's staging runs behind the first block's MFMAs, in
// the shadow of the others.  The loop and the staging stay in the kernel's own text: inside a helper their branches are
// simplified apart from the kernel's and the step compiles to another schedule.
template <int FC, int LD, int NT, bool X_IS_A>
struct Layer1F32 {
    static constexpr int NB = FC / 16;
    const float* xb; const float* wb;
    float4 xq[2][2], wq[2][NT][2];                              // [parity of block][...][quad]
    __device__ __forceinline__ void read_block(int j) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            xq[j & 1][q] = *reinterpret_cast<const float4*>(xb + 8 * j + 4 * q);
#pragma unroll
            for (int t = 0; t < NT; ++t) wq[j & 1][t][q] = *reinterpret_cast<const float4*>(wb + t * 32 * LD + 8 * j + 4 * q);
        }
    }
    __device__ __forceinline__ void mfma(f32x16& acc, float w, float x) const {
        if constexpr (X_IS_A) DL_MFMA(acc, x, w);
        else DL_MFMA(acc, w, x);
    }
    __device__ __forceinline__ void mfma_block(f32x16 (&acc)[NT], int j) const {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int t = 0; t < NT; ++t) mfma(acc[t], wq[j & 1][t][q].x, xq[j & 1][q].x);
#pragma unroll
            for (int t = 0; t < NT; ++t) mfma(acc[t], wq[j & 1][t][q].y, xq[j & 1][q].y);
#pragma unroll
            for (int t = 0; t < NT; ++t) mfma(acc[t], wq[j & 1][t][q].z, xq[j & 1][q].z);
#pragma unroll
            for (int t = 0; t < NT; ++t) mfma(acc[t], wq[j & 1][t][q].w, xq[j & 1][q].w);
        }
    }
};

// K = 16 block b of a 16-register accumulator (or of 16 floats in its layout) as a B operand on the bf16 matrix path, split in
// place into its three planes: slot s of the block = register 8b + s.
template <class Acc>
__device__ __forceinline__ void split_acc_block(const Acc& acc, int b, bf16x8 (&out)[3]) {
    bf16x8 p0, p1, p2;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        __bf16 hi, mid, lo;
        split3(acc[8 * b + s], hi, mid, lo);
        p0[s] = hi; p1[s] = mid; p2[s] = lo;
    }
    out[0] = p0; out[1] = p1; out[2] = p2;
}

}  // namespace project
}  // namespace dl
