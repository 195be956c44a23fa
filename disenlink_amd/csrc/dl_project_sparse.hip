// Factor projection of SPARSE features (model.py:13-15, 24-27 fanned out at model.py:106): the feature matrix is
//     x~[i][f] = scale[i] * X[i][f] + shift[i],   X a CSR (dl_sparse_features, include/disenlink_hip.h),
// so layer 1 is a gather of W1^T rows and dW1 a gather of dhid rows over the CSC view of X — no product with zeros and no
// dense [N][F] matrix.
//
//   forward   W1 [C][F] -> W1T [F][Cp] (+ csum[c] = sum_f W1[c][f] when shift is given)        transpose / csum kernels
//             acc[i][c] = sum_{e in row i} val_e W1T[col_e][c];  pre = scale_i acc + shift_i csum[c] + b1[c]
//             two-layer: hid = relu(pre) -> hidT [K][nhid][ldh];  single layer: Z = pre          sparse_l1_fwd_kernel
//             Z[n][k][:] = W2_k hid[n][k][:] + b2_k from hidT on the matrix cores                sparse_l2_fwd_kernel
//   backward  dW2, db1, db2, dhid [N][C]: kernel A of dl_project_bwd.hip, kept fp32 form         project_bwd_kept
//             partial[s][c] = sum_{e in segment s} (scale_i val_e) dhid[i][c]                    sparse_dw1_seg_kernel
//             gpart[r][c] = sum_{i in node range r} shift_i dhid[i][c]                           sparse_shift_colsum_kernel
//             dW1[c][f] = sum_{s in column f} partial[s][c] + sum_r gpart[r][c]                  sparse_dw1_finish_kernel
// C = K * nhid (single layer: K * d), Cp = C rounded up to 4.  A lane owns 4 consecutive columns c (16-byte loads of the
// gathered rows), a wave 256.  Every sum has a fixed order and no float atomics are used: bitwise reproducible, and a row's
// hidden layer depends on that row alone.
#include <algorithm>
#include "dl_common.h"
#include "dl_kernels.h"
#include "dl_tiles.h"

namespace dl {
namespace sparse {

using project::XcdItem;
using project::xcd_grid;
using project::xcd_item;

constexpr int CHUNK = 256;        // columns of one wave: 64 lanes x 4
constexpr int ROWS = 32;          // node rows of one forward workgroup (4 waves x 8 rows)
constexpr int TP = 33;            // LDS pitch of the transposing tiles
constexpr int DEFAULT_SEG = 512;  // entries of a column segment

// ---------------------------------------------------------------------------------------------- W1 -> W1T, csum
__global__ __launch_bounds__(256) void sparse_w1t_kernel(const float* __restrict__ W1, int C, int F, int Cp,
                                                         float* __restrict__ W1T) {
    __shared__ float tile[32][TP];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int f0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + ty + 8 * j, f = f0 + tx;
        tile[ty + 8 * j][tx] = (c < C && f < F) ? W1[(size_t)c * F + f] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = f0 + ty + 8 * j, c = c0 + tx;
        if (f < F && c < Cp) W1T[(size_t)f * Cp + c] = tile[tx][ty + 8 * j];     // columns C .. Cp-1 are written as zero
    }
}

// csum[c] = sum_f W1[c][f]: one wave per c, tiles of 128 features (two per lane, then the butterfly), the tile sums added
// in tile order.
__global__ __launch_bounds__(256) void sparse_csum_kernel(const float* __restrict__ W1, int C, int F,
                                                          float* __restrict__ csum) {
    const int c = (int)blockIdx.x * 4 + wave_index(), lane = lane_id();
    if (c >= C) return;
    const float* row = W1 + (size_t)c * F;
    float total = 0.0f;
    for (int t0 = 0; t0 < F; t0 += 128) {
        const int fa = t0 + lane, fb = t0 + 64 + lane;
        const float a = fa < F ? row[fa] : 0.0f, b = fb < F ? row[fb] : 0.0f;
        total += wave_allreduce_sum(a + b);
    }
    if (lane == 0) csum[c] = total;
}

// ---------------------------------------------------------------------------------------------- layer 1: the gather
// 1-D grid of xcd_grid(column chunks, row tiles of 32): the workgroups of one XCD at a time work on few column chunks of W1T.
// Wave w owns rows 8w .. 8w+7 of the tile, one after the other; per row the entries are walked in steps of 8 (8 index /
// value pairs by scalar loads, 8 row loads of 16 bytes per lane in flight, then the 8 fmas in entry order).
template <bool TWO>
__global__ __launch_bounds__(256) void sparse_l1_fwd_kernel(dl_sparse_features sf, const float* __restrict__ W1T, int C, int Cp,
                                                            const float* __restrict__ csum, const float* __restrict__ b1,
                                                            float* __restrict__ out, int ldh, int n_chunks, int n_tiles) {
    __shared__ float tile[TWO ? CHUNK * TP : 1];
    const XcdItem item = xcd_item(blockIdx.x, n_chunks, n_tiles);
    if (!item.valid) return;
    const int chunk = item.a, rt = item.b;
    const int wave = wave_index(), lane = lane_id();
    const int c0 = chunk * CHUNK + lane * 4;
    const bool cv = c0 < Cp;
    const float* wcol = W1T + (cv ? c0 : 0);
    float cs[4], bb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = c0 + j < C;
        bb[j] = ok ? b1[c0 + j] : 0.0f;
        cs[j] = (ok && csum != nullptr) ? csum[c0 + j] : 0.0f;
    }
    for (int rr = 0; rr < ROWS / 4; ++rr) {
        const int rl = wave * (ROWS / 4) + rr, i = rt * ROWS + rl;       // wave-uniform
        if (i >= sf.N) break;
        const int beg = sf.rowptr[i], end = sf.rowptr[i + 1];
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        int e = beg;
        for (; e + 8 <= end; e += 8) {
            int cj[8];
            float vj[8];
            float4 w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                cj[j] = sf.col[e + j];
                vj[j] = sf.val != nullptr ? sf.val[e + j] : 1.0f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = *reinterpret_cast<const float4*>(wcol + (size_t)cj[j] * Cp);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc.x = fmaf(vj[j], w[j].x, acc.x);
                acc.y = fmaf(vj[j], w[j].y, acc.y);
                acc.z = fmaf(vj[j], w[j].z, acc.z);
                acc.w = fmaf(vj[j], w[j].w, acc.w);
            }
        }
        for (; e < end; ++e) {
            const int cj = sf.col[e];
            const float vj = sf.val != nullptr ? sf.val[e] : 1.0f;
            const float4 w = *reinterpret_cast<const float4*>(wcol + (size_t)cj * Cp);
            acc.x = fmaf(vj, w.x, acc.x);
            acc.y = fmaf(vj, w.y, acc.y);
            acc.z = fmaf(vj, w.z, acc.z);
            acc.w = fmaf(vj, w.w, acc.w);
        }
        const float sc = sf.scale != nullptr ? sf.scale[i] : 1.0f;
        const float sh = sf.shift != nullptr ? sf.shift[i] : 0.0f;
        float pre[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float affine = sf.shift != nullptr ? fmaf(sh, cs[j], bb[j]) : bb[j];
            pre[j] = fmaf(sc, pre[j], affine);
        }
        if constexpr (TWO) {
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[(lane * 4 + j) * TP + rl] = fmaxf(pre[j], 0.0f);
        } else {
            float* o = out + (size_t)i * C + c0;
            if ((C & 3) == 0) {
                if (c0 < C) *reinterpret_cast<float4*>(o) = make_float4(pre[0], pre[1], pre[2], pre[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < C) o[j] = pre[j];
            }
        }
    }
    if constexpr (TWO) {
        // hidT [C][ldh]: 32 consecutive nodes of one hidden unit per half wave; the columns N .. ldh-1 are written as zero
        __syncthreads();
        const int r = threadIdx.x & 31, cg = threadIdx.x >> 5;
        const int n = rt * ROWS + r;
#pragma unroll 4
        for (int j = 0; j < 32; ++j) {
            const int cl = cg * 32 + j, c = chunk * CHUNK + cl;
            if (c < C && n < ldh) out[(size_t)c * ldh + n] = n < sf.N ? tile[cl * TP + r] : 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------- layer 2 from hidT
// Z[n][k][:] = W2_k . hid[n][k][:] + b2_k.  Grid (node tiles of 128, K); 4 waves, wave w owns nodes 32w .. 32w+31 and all
// D output columns (D/32 accumulators).  Per step of 32 hidden units the hidT tile [32 h][128 n] and the W2 tile [D][32 h]
// are split into three bf16 planes on their way into LDS ([3][rows][32 + 8], the image of dl_tiles.h) and contracted by
// mfma_split6: A rows = nodes, B rows = output columns, so a lane holds output column (lane % 32) of 16 nodes.
template <int D>
__global__ __launch_bounds__(256) void sparse_l2_fwd_kernel(const float* __restrict__ hidT, int N, int ldh, int K, int nhid,
                                                            const float* __restrict__ W2, const float* __restrict__ b2,
                                                            float* __restrict__ Z) {
    using namespace project;
    constexpr int P = SPLIT_PITCH, DT = D / 32;
    __shared__ __attribute__((aligned(16))) __bf16 hp[3 * 128 * P];
    __shared__ __attribute__((aligned(16))) __bf16 wp[3 * D * P];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, half = lane >> 5;
    const int n0 = blockIdx.x * 128, k = blockIdx.y;
    const float* hk = hidT + (size_t)k * nhid * ldh;
    const float* wk = W2 + (size_t)k * D * nhid;
    f32x16 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) zero_acc(acc[dt]);
    for (int h0 = 0; h0 < nhid; h0 += 32) {
        // global -> registers: hid pairs (h, h+1) of one node; W2 pairs (h, h+1) of one output column
        float ha[8][2], wa[D / 16][2];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = tid + 256 * j, nl = i & 127, hq = i >> 7;
            const int n = n0 + nl, h = h0 + 2 * hq;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const bool ok = n < N && h + t < nhid;
                const float v = hk[ok ? (size_t)(h + t) * ldh + n : 0];
                ha[j][t] = ok ? v : 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < D / 16; ++j) {
            const int i = tid + 256 * j, hq = i & 15, dd = i >> 4;
            const int h = h0 + 2 * hq;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const bool ok = h + t < nhid;
                const float v = wk[ok ? (size_t)dd * nhid + h + t : 0];
                wa[j][t] = ok ? v : 0.0f;
            }
        }
        __syncthreads();                                        // every wave is past the previous step's LDS reads
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = tid + 256 * j, nl = i & 127, hq = i >> 7;
            __bf16 p0[2], p1[2], p2[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) split3(ha[j][t], p0[t], p1[t], p2[t]);
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<bf16x2*>(hp + (0 * 128 + nl) * P + 2 * hq) = bf16x2{p0[0], p0[1]};
            *reinterpret_cast<bf16x2*>(hp + (1 * 128 + nl) * P + 2 * hq) = bf16x2{p1[0], p1[1]};
            *reinterpret_cast<bf16x2*>(hp + (2 * 128 + nl) * P + 2 * hq) = bf16x2{p2[0], p2[1]};
        }
#pragma unroll
        for (int j = 0; j < D / 16; ++j) {
            const int i = tid + 256 * j, hq = i & 15, dd = i >> 4;
            __bf16 p0[2], p1[2], p2[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) split3(wa[j][t], p0[t], p1[t], p2[t]);
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<bf16x2*>(wp + (0 * D + dd) * P + 2 * hq) = bf16x2{p0[0], p0[1]};
            *reinterpret_cast<bf16x2*>(wp + (1 * D + dd) * P + 2 * hq) = bf16x2{p1[0], p1[1]};
            *reinterpret_cast<bf16x2*>(wp + (2 * D + dd) * P + 2 * hq) = bf16x2{p2[0], p2[1]};
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            bf16x8 a[3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
                a[p] = *reinterpret_cast<const bf16x8*>(hp + (p * 128 + wave * 32 + li) * P + kb * 16 + 8 * half);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                bf16x8 b[3];
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    b[p] = *reinterpret_cast<const bf16x8*>(wp + (p * D + dt * 32 + li) * P + kb * 16 + 8 * half);
                mfma_split6(acc[dt], a, b);
            }
        }
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const float bias = b2[k * D + dt * 32 + li];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + wave * 32 + acc_row(r, half);
            if (n < N) Z[((size_t)n * K + k) * D + dt * 32 + li] = acc[dt][r] + bias;
        }
    }
}

// ---------------------------------------------------------------------------------------------- dW1: the CSC gather
// One wave per (segment, column chunk): partial[s][c] = sum over the entries of segment s, rows ascending, of
// (scale_i val_e) Y[i][c], Y = dhid [N][C] (single layer: dZ).  VEC: C % 4 == 0, rows of Y are aligned quads.
template <bool VEC>
__global__ __launch_bounds__(256) void sparse_dw1_seg_kernel(dl_sparse_features sf, const float* __restrict__ Y, int C, int Cp,
                                                             int n_chunks, float* __restrict__ partial) {
    const long long item = (long long)blockIdx.x * 4 + wave_index();
    if (item >= (long long)sf.n_seg * n_chunks) return;
    const int s = (int)(item / n_chunks), chunk = (int)(item - (long long)s * n_chunks);
    const int lane = lane_id(), c0 = chunk * CHUNK + lane * 4;
    if (c0 >= Cp) return;
    const int f = sf.seg_col[s];
    const int beg = sf.colptr[f] + (s - sf.colseg[f]) * sf.seg_len, end = min(sf.colptr[f + 1], beg + sf.seg_len);
    auto load = [&](int i) {
        const float* y = Y + (size_t)i * C + c0;
        if constexpr (VEC) {
            return *reinterpret_cast<const float4*>(y);
        } else {
            float4 q;
            q.x = y[0];                                                          // c0 < Cp and C > Cp - 4: c0 < C
            q.y = c0 + 1 < C ? y[1] : 0.0f;
            q.z = c0 + 2 < C ? y[2] : 0.0f;
            q.w = c0 + 3 < C ? y[3] : 0.0f;
            return q;
        }
    };
    auto weight = [&](int e, int i) {
        const float v = sf.val != nullptr ? sf.val[sf.csc_entry[e]] : 1.0f;
        return sf.scale != nullptr ? sf.scale[i] * v : v;
    };
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int e = beg;
    for (; e + 8 <= end; e += 8) {
        int ij[8];
        float wj[8];
        float4 y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) ij[j] = sf.csc_row[e + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = load(ij[j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) wj[j] = weight(e + j, ij[j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc.x = fmaf(wj[j], y[j].x, acc.x);
            acc.y = fmaf(wj[j], y[j].y, acc.y);
            acc.z = fmaf(wj[j], y[j].z, acc.z);
            acc.w = fmaf(wj[j], y[j].w, acc.w);
        }
    }
    for (; e < end; ++e) {
        const int i = sf.csc_row[e];
        const float4 y = load(i);
        const float w = weight(e, i);
        acc.x = fmaf(w, y.x, acc.x);
        acc.y = fmaf(w, y.y, acc.y);
        acc.z = fmaf(w, y.z, acc.z);
        acc.w = fmaf(w, y.w, acc.w);
    }
    *reinterpret_cast<float4*>(partial + (size_t)s * Cp + c0) = acc;
}

// gpart[r][c] = sum over the nodes i of range r of shift_i Y[i][c] (colsum_kernel of dl_project_bwd.hip with a weight):
// block = 64 columns x 4 row lanes, grid (column blocks, ranges).
__global__ __launch_bounds__(256) void sparse_shift_colsum_kernel(const float* __restrict__ Y, const float* __restrict__ shift,
                                                                  int N, int C, int Cp, int rows_per_range,
                                                                  float* __restrict__ gpart) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int r0 = blockIdx.y * rows_per_range, r1 = min(N, r0 + rows_per_range);
    float v = 0.0f;
    if (c < C)
        for (int r = r0 + rl; r < r1; r += 4) v = fmaf(shift[r], Y[(size_t)r * C + c], v);
    red[rl][cl] = v;
    __syncthreads();
    if (rl == 0 && c < C) gpart[(size_t)blockIdx.y * Cp + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// dW1[c][f] = (partials of column f in segment order) + (g[c] = gpart ranges in order); every (c, f) is written, columns
// without entries too.  Block = 32 features x 256 columns c; thread t sums for column c0 + t, the tile leaves through LDS
// so that the stores run along f.
__global__ __launch_bounds__(256) void sparse_dw1_finish_kernel(dl_sparse_features sf, const float* __restrict__ partial, int C,
                                                                int Cp, const float* __restrict__ gpart, int S, int n_chunks,
                                                                float* __restrict__ dW1) {
    __shared__ float tile[CHUNK * TP];
    const int chunk = blockIdx.x % n_chunks, ft = blockIdx.x / n_chunks;
    const int tid = threadIdx.x, c = chunk * CHUNK + tid;
    const int F = sf.F;
    float g = 0.0f;
    if (gpart != nullptr && c < C)
        for (int r = 0; r < S; ++r) g += gpart[(size_t)r * Cp + c];
    for (int fl = 0; fl < 32; ++fl) {
        const int f = ft * 32 + fl;
        float v = 0.0f;
        if (f < F && c < C) {
            const int s0 = sf.colseg[f], s1 = sf.colseg[f + 1];
            for (int s = s0; s < s1; ++s) v += partial[(size_t)s * Cp + c];
            if (gpart != nullptr) v += g;
        }
        tile[tid * TP + fl] = v;
    }
    __syncthreads();
    const int fl = tid & 31, cg = tid >> 5, f = ft * 32 + fl;
#pragma unroll 4
    for (int j = 0; j < 32; ++j) {
        const int cl = cg * 32 + j, cc = chunk * CHUNK + cl;
        if (cc < C && f < F) dW1[(size_t)cc * F + f] = tile[cl * TP + fl];
    }
}

// ---------------------------------------------------------------------------------------------- host side

struct Shape { int C, Cp, n_chunks; };
static Shape shape_of(int K, int nhid, int d, bool two) {
    Shape s;
    s.C = K * (two ? nhid : d);
    s.Cp = (s.C + 3) & ~3;
    s.n_chunks = ceil_div(s.Cp, CHUNK);
    return s;
}

// node ranges of g: enough workgroups for the chip, never fewer than 64 rows per range
static void g_ranges(int N, int C, int& S, int& rows_per_range) {
    const int colblocks = ceil_div(C, 64);
    S = (int)std::max(1LL, std::min<long long>(ceil_div(N, 64), ceil_div(768, colblocks)));
    rows_per_range = ceil_div(N, S);
    S = ceil_div(N, rows_per_range);
}

struct FwdLayout { size_t off_w1t, off_csum, bytes; };
static FwdLayout fwd_layout(int F, const Shape& s) {
    FwdLayout L;
    size_t off = 0;
    L.off_w1t = off;   off += align256(sizeof(float) * (size_t)F * s.Cp);
    L.off_csum = off;  off += align256(sizeof(float) * (size_t)s.Cp);
    L.bytes = off;
    return L;
}

struct BwdLayout { size_t off_kept, off_dhid, off_partial, off_gpart, bytes; int S, rows_per_range; };
static BwdLayout bwd_layout(int N, int n_seg, int K, int nhid, int d, bool two, const Shape& s) {
    BwdLayout L;
    g_ranges(N, s.C, L.S, L.rows_per_range);
    size_t off = 0;
    L.off_kept = off;     off += align256(project_bwd_kept_workspace_bytes(N, K, nhid, d, two));
    L.off_dhid = off;     off += two ? align256(sizeof(float) * (size_t)N * s.C) : 0;
    L.off_partial = off;  off += align256(sizeof(float) * (size_t)std::max(n_seg, 1) * s.Cp);
    L.off_gpart = off;    off += align256(sizeof(float) * (size_t)L.S * s.Cp);
    L.bytes = off;
    return L;
}

}  // namespace sparse

int sparse_seg_len() { return config().sparse_seg > 0 ? config().sparse_seg : sparse::DEFAULT_SEG; }

size_t project_sparse_fwd_workspace_bytes(const dl_sparse_features* x, int K, int nhid, int d, bool two) {
    return sparse::fwd_layout(x->F, sparse::shape_of(K, nhid, d, two)).bytes;
}

size_t project_sparse_bwd_workspace_bytes(const dl_sparse_features* x, int K, int nhid, int d, bool two) {
    return sparse::bwd_layout(x->N, x->n_seg, K, nhid, d, two, sparse::shape_of(K, nhid, d, two)).bytes;
}

void project_sparse_form(int N, int F, int K, int nhid, int d, bool two, bool affine, int max_col_len, int* out) {
    using namespace sparse;
    (void)F;
    const Shape s = shape_of(K, nhid, d, two);
    int S, rpr, kept[3];
    g_ranges(N, s.C, S, rpr);
    project_bwd_kept_form(N, K, nhid, d, two, kept);
    const int seg = sparse_seg_len();
    const int v[DL_PROJECT_SPARSE_FORM_LEN] = {s.n_chunks, s.Cp - (s.n_chunks - 1) * CHUNK, affine ? 1 : 0,
                                               ceil_div(max_col_len, seg), seg, two ? 1 : 0, two ? d : 0,
                                               s.C % 4 == 0 ? 1 : 0, kept[0], affine ? S : 0};
    std::copy(v, v + DL_PROJECT_SPARSE_FORM_LEN, out);
}

int project_sparse_fwd(const dl_sparse_features* x, int K, int nhid, int d, const float* W1, const float* b1, const float* W2,
                       const float* b2, float* Z, float* hid_out, void* ws, hipStream_t st) {
    using namespace sparse;
    const bool two = W2 != nullptr;
    const int N = x->N, F = x->F;
    const Shape s = shape_of(K, nhid, d, two);
    const FwdLayout L = fwd_layout(F, s);
    char* base = static_cast<char*>(ws);
    float* W1T = reinterpret_cast<float*>(base + L.off_w1t);
    float* csum = x->shift != nullptr ? reinterpret_cast<float*>(base + L.off_csum) : nullptr;
    hipLaunchKernelGGL(sparse_w1t_kernel, dim3((unsigned)ceil_div(F, 32), (unsigned)ceil_div(s.Cp, 32)), dim3(256), 0, st, W1,
                       s.C, F, s.Cp, W1T);
    if (csum != nullptr)
        hipLaunchKernelGGL(sparse_csum_kernel, dim3((unsigned)ceil_div(s.C, 4)), dim3(256), 0, st, W1, s.C, F, csum);
    const int n_tiles = ceil_div(N, ROWS), ldh = (N + 3) & ~3;
    const dim3 grid((unsigned)xcd_grid(s.n_chunks, n_tiles));
    if (two) {
        hipLaunchKernelGGL(sparse_l1_fwd_kernel<true>, grid, dim3(256), 0, st, *x, W1T, s.C, s.Cp, csum, b1, hid_out, ldh,
                           s.n_chunks, n_tiles);
        const dim3 g2((unsigned)ceil_div(N, 128), (unsigned)K);
        if (d == 32) hipLaunchKernelGGL(sparse_l2_fwd_kernel<32>, g2, dim3(256), 0, st, hid_out, N, ldh, K, nhid, W2, b2, Z);
        if (d == 64) hipLaunchKernelGGL(sparse_l2_fwd_kernel<64>, g2, dim3(256), 0, st, hid_out, N, ldh, K, nhid, W2, b2, Z);
        if (d == 128) hipLaunchKernelGGL(sparse_l2_fwd_kernel<128>, g2, dim3(256), 0, st, hid_out, N, ldh, K, nhid, W2, b2, Z);
    } else {
        hipLaunchKernelGGL(sparse_l1_fwd_kernel<false>, grid, dim3(256), 0, st, *x, W1T, s.C, s.Cp, csum, b1, Z, 0, s.n_chunks,
                           n_tiles);
    }
    return check_launch("project_sparse_fwd");
}

int project_sparse_bwd(const dl_sparse_features* x, int K, int nhid, int d, const float* b1, const float* W2, const float* dZ,
                       const float* hid, float* dW1, float* db1, float* dW2, float* db2, void* ws, hipStream_t st) {
    using namespace sparse;
    const bool two = W2 != nullptr;
    const int N = x->N, F = x->F;
    const Shape s = shape_of(K, nhid, d, two);
    const BwdLayout L = bwd_layout(N, x->n_seg, K, nhid, d, two, s);
    char* base = static_cast<char*>(ws);
    float* dhid = reinterpret_cast<float*>(base + L.off_dhid);
    float* partial = reinterpret_cast<float*>(base + L.off_partial);
    float* gpart = x->shift != nullptr ? reinterpret_cast<float*>(base + L.off_gpart) : nullptr;
    project_bwd_kept(N, K, nhid, d, b1, W2, dZ, hid, dhid, db1, dW2, db2, base + L.off_kept, st);
    const float* Y = two ? dhid : dZ;                           // [N][C]
    if (gpart != nullptr)
        hipLaunchKernelGGL(sparse_shift_colsum_kernel, dim3((unsigned)ceil_div(s.C, 64), (unsigned)L.S), dim3(256), 0, st, Y,
                           x->shift, N, s.C, s.Cp, L.rows_per_range, gpart);
    if (x->n_seg > 0) {
        const dim3 grid((unsigned)ceil_div((long long)x->n_seg * s.n_chunks, 4));
        if (s.C % 4 == 0) hipLaunchKernelGGL(sparse_dw1_seg_kernel<true>, grid, dim3(256), 0, st, *x, Y, s.C, s.Cp, s.n_chunks, partial);
        else hipLaunchKernelGGL(sparse_dw1_seg_kernel<false>, grid, dim3(256), 0, st, *x, Y, s.C, s.Cp, s.n_chunks, partial);
    }
    hipLaunchKernelGGL(sparse_dw1_finish_kernel, dim3((unsigned)(ceil_div(F, 32) * s.n_chunks)), dim3(256), 0, st, *x, partial,
                       s.C, s.Cp, gpart, L.S, s.n_chunks, dW1);
    return check_launch("project_sparse_bwd");
}

}  // namespace dl

// ---------------------------------------------------------------------------------------------- C ABI
using namespace dl;

static int check_sparse(const dl_sparse_features* x, int K, int nhid, int d, bool two) {
    DL_REQUIRE(x != nullptr, "sparse features are NULL");
    DL_REQUIRE(K >= 1 && K <= DL_MAX_FACTORS, "K=%d outside 1..%d", K, DL_MAX_FACTORS);
    DL_REQUIRE(project_supported(d), "projection kernel supports d in {32, 64, 128}, got %d", d);
    DL_REQUIRE(x->N >= 0 && x->F >= 1 && x->nnz >= 0 && nhid >= 1, "bad size N=%d F=%d nnz=%d nhid=%d", x->N, x->F, x->nnz, nhid);
    DL_REQUIRE(two || nhid == 1, "single layer: nhid must be 1");
    DL_REQUIRE((long long)K * (two ? nhid : d) <= (1 << 21) && (long long)x->F * K * (two ? nhid : d) < (1LL << 40),
               "projection sizes out of range");
    if (x->N == 0) return DL_OK;
    DL_REQUIRE(x->rowptr && x->colptr && x->colseg, "NULL index array");
    DL_REQUIRE(x->nnz == 0 || (x->col && x->csc_row && x->csc_entry && x->seg_col), "NULL entry array");
    DL_REQUIRE(x->seg_len == sparse_seg_len(), "the segment plan was built for segments of %d entries, the library cuts at %d "
               "(dl_sparse_seg_len; DL_SPARSE_SEG)", x->seg_len, sparse_seg_len());
    DL_REQUIRE(x->n_seg >= 0 && x->n_seg <= x->nnz, "bad segment count %d", x->n_seg);
    return DL_OK;
}

extern "C" {

int dl_sparse_seg_len(void) { return sparse_seg_len(); }

size_t dl_project_sparse_fwd_workspace_bytes(const dl_sparse_features* x, int K, int nhid, int d, int two_layer) {
    if (x == nullptr || x->N <= 0 || x->F < 1 || K < 1 || nhid < 1 || d < 1) return 0;
    return project_sparse_fwd_workspace_bytes(x, K, two_layer ? nhid : 1, d, two_layer != 0);
}

size_t dl_project_sparse_bwd_workspace_bytes(const dl_sparse_features* x, int K, int nhid, int d, int two_layer) {
    if (x == nullptr || x->N <= 0 || x->F < 1 || K < 1 || nhid < 1 || d < 1 || !project_supported(d)) return 0;
    return project_sparse_bwd_workspace_bytes(x, K, two_layer ? nhid : 1, d, two_layer != 0);
}

int dl_project_sparse_form(int N, int F, int K, int nhid, int d, int two_layer, int affine, int max_col_len, int* out) {
    DL_REQUIRE(out != nullptr && project_supported(d) && N >= 1 && F >= 1 && K >= 1 && nhid >= 1 && max_col_len >= 0,
               "bad argument");
    project_sparse_form(N, F, K, two_layer ? nhid : 1, d, two_layer != 0, affine != 0, max_col_len, out);
    return DL_OK;
}

int dl_project_sparse_fwd(const dl_sparse_features* x, int K, int nhid, int d, const float* W1, const float* b1,
                          const float* W2, const float* b2, float* Z, float* hid_out, void* ws, size_t ws_bytes,
                          void* stream) {
    DL_REQUIRE((W2 == nullptr) == (b2 == nullptr), "W2 and b2 must both be given (two-layer) or both NULL");
    const bool two = W2 != nullptr;
    if (!two) nhid = 1;
    if (int rc = check_sparse(x, K, nhid, d, two)) return rc;
    if (x->N == 0) return DL_OK;
    DL_REQUIRE(W1 && b1 && Z, "NULL argument");
    DL_REQUIRE(!two || hid_out != nullptr, "the two-layer form keeps the hidden layer: hid_out is required");
    DL_REQUIRE(two || hid_out == nullptr, "hid_out is for the two-layer form only");
    const size_t need = project_sparse_fwd_workspace_bytes(x, K, nhid, d, two);
    DL_REQUIRE(ws != nullptr && ws_bytes >= need && ((uintptr_t)ws & 15) == 0,
               "workspace too small: %zu < %zu bytes (dl_project_sparse_fwd_workspace_bytes)", ws_bytes, need);
    return project_sparse_fwd(x, K, nhid, d, W1, b1, W2, b2, Z, hid_out, ws, (hipStream_t)stream);
}

int dl_project_sparse_bwd(const dl_sparse_features* x, int K, int nhid, int d, const float* W1, const float* b1,
                          const float* W2, const float* dZ, const float* hid, float* dW1, float* db1, float* dW2,
                          float* db2, void* ws, size_t ws_bytes, void* stream) {
    (void)W1;                                                   // the gradients do not depend on W1 once hid is given
    const bool two = W2 != nullptr;
    if (!two) nhid = 1;
    if (int rc = check_sparse(x, K, nhid, d, two)) return rc;
    DL_REQUIRE(dW1 && db1 && (!two || (dW2 && db2)), "NULL gradient output");
    hipStream_t st = (hipStream_t)stream;
    if (x->N == 0) {                                            // no nodes: every gradient is zero
        const size_t m = two ? (size_t)nhid : (size_t)d;
        hipError_t e = hipMemsetAsync(dW1, 0, sizeof(float) * K * m * x->F, st);
        if (e == hipSuccess) e = hipMemsetAsync(db1, 0, sizeof(float) * K * m, st);
        if (two && e == hipSuccess) e = hipMemsetAsync(dW2, 0, sizeof(float) * (size_t)K * d * nhid, st);
        if (two && e == hipSuccess) e = hipMemsetAsync(db2, 0, sizeof(float) * (size_t)K * d, st);
        DL_REQUIRE(e == hipSuccess, "hipMemsetAsync failed");
        return DL_OK;
    }
    DL_REQUIRE(dZ != nullptr && b1 != nullptr, "NULL argument");
    DL_REQUIRE(!two || hid != nullptr, "the sparse backward has no recompute form: hid is required");
    DL_REQUIRE(two || hid == nullptr, "hid is for the two-layer form only");
    const size_t need = project_sparse_bwd_workspace_bytes(x, K, nhid, d, two);
    DL_REQUIRE(ws != nullptr && ws_bytes >= need && ((uintptr_t)ws & 15) == 0,
               "workspace too small: %zu < %zu bytes (dl_project_sparse_bwd_workspace_bytes)", ws_bytes, need);
    return project_sparse_bwd(x, K, nhid, d, b1, W2, dZ, hid, dW1, db1, dW2, db2, ws, st);
}

}  // extern "C"
