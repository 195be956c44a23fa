// Dense backward of the [N][N] link scorer on the matrix cores: the gradient of ANY loss on link_pred
// (autograd of model.py:109-113 + sigmoid under main_disentangled.py:198), without a pair plan.  With
//   G = g_prob o prob o (1 - prob)   (sigmoid backward on the forward's saved output),   G^ = G + G^T,
// and per factor k  S = Z_k Z_k^T, E = exp(S / t), Q = H_k H_k^T:
//   dH_k = (G^ o E) . H_k                 dZ_k = (G^ o Q o E / t) . Z_k             (the diagonal included as written).
// That is the forward's two Gram products per tile (no symmetry to exploit: every (u tile, v tile) pair is formed)
// plus two [128 x 128] x [128 x d] products per tile: 4x the FLOP of the forward's executed products.
//
// Three stages (+ one combine launch when the v range is sliced), all on the caller's stream, no atomics, no host read:
//   1. ghat_kernel: G^ as Np x Np floats (Np = N rounded up to 128, zero outside N) — the transposed read of g_prob
//      goes through LDS, so both reads are coalesced.
//   2. planes: split_rows (dl_planes.hip) gives the row planes of Z_k, H_k for the Gram products; split_cols_kernel
//      gives the planes of Z_k^T, H_k^T in the exact operand order of the second products.
//   3. score_dense_bwd_kernel: one workgroup = 8 waves owns a 128-row u tile of one factor and walks v tiles of 128.
//      Per v tile: S and Q as in the forward (gram_block_split6, wave = 32 u x 64 v), the two weight tiles in the
//      accumulator registers, written to LDS as three bf16 planes each (one 64-v half at a time: the images alias the
//      Gram staging buffers), then wave (u quarter, o) multiplies weight o (0: G^ o E, 1: G^ o Q o E / t) against the
//      v rows of H_k (Z_k) into its resident [32 u x d] accumulator, six exact bf16 products per term.  Stored once.
// NO tile is skipped and no zero weight short-cuts a product: a zero of G^ against an overflowed E = inf gives NaN, as
// the reference's autograd does.
#include <algorithm>
#include <type_traits>
#include "dl_common.h"
#include "dl_kernels.h"
#include "dl_scan.h"
#include "dl_tiles.h"

namespace dl {
namespace dense_bwd {

using namespace project;       // PlaneStage, f32x16, acc_row, split3 planes

constexpr int TT = 128;        // tile edge (u and v)
constexpr int BTHR = 512;
constexpr int SDC = SPLIT_COLS, SLD = SPLIT_PITCH;
constexpr int STAGE = 3 * TT * SLD;            // bf16 elements of one staged operand tile [3][128][32 + 8]
constexpr int VH = 64;                         // v extent of a weight image (half a v tile)
constexpr int WLD = VH + 8;                    // its row pitch (144 bytes: conflict-free b128 reads)
constexpr int WIMG = 3 * TT * WLD;             // one weight: [3 planes][128 u][WLD]
constexpr size_t LDS_BYTES = (size_t)4 * STAGE * sizeof(__bf16);
static_assert(2 * WIMG <= 4 * STAGE, "the weight images alias the Gram staging buffers");
// One-plane tables (P = 1, bf16): the staging buffers are a third of that, [2][1][128][SLD] per operand, while the weights are
// fp32 values formed in registers and keep their three planes: the two weight images no longer fit over the staging buffers,
// so the dynamic LDS of a form is the larger of the two and the images still start where the staging buffers start.
constexpr size_t lds_bytes(int P) { return sizeof(__bf16) * (size_t)std::max(4 * (STAGE / 3) * P, 2 * WIMG); }
static_assert(lds_bytes(3) == LDS_BYTES, "the three-plane form keeps its LDS");
static_assert(lds_bytes(1) == sizeof(__bf16) * (size_t)2 * WIMG && 4 * (STAGE / 3) <= 2 * WIMG && lds_bytes(1) <= LDS_BYTES,
              "one plane: the weight images cover the Gram staging buffers, and the form needs no more LDS than three planes");
constexpr int KB = TT / 16;                    // K = 16 blocks of a v tile

// ---- 1. G^ = G + G^T, G = g o p o (1 - p), zero-filled out to Np x Np ---------------------------------------------
// LOGIT: g is d loss / d logit, so G = g as it stands and prob is not read (dl_score_allpairs_logits_bwd_dense).
template <bool LOGIT = false>
__global__ __launch_bounds__(256) void ghat_kernel(const float* __restrict__ prob, const float* __restrict__ g, int N, int Np,
                                                   float* __restrict__ ghat) {
    __shared__ float mir[64][65];
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tc = threadIdx.x & 63, tr = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {                              // the mirrored tile: rows j0.., columns i0..
        const int r = 4 * i + tr, row = j0 + r, col = i0 + tc;
        float x = 0.0f;
        if (row < N && col < N) {
            const size_t o = (size_t)row * N + col;
            if constexpr (LOGIT) {
                x = g[o];
            } else {
                const float p = prob[o];
                x = g[o] * p * (1.0f - p);                      // sigmoid backward p(1-p)
            }
        }
        mir[r][tc] = x;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = 4 * i + tr, row = i0 + r, col = j0 + tc;
        float x = 0.0f;
        if (row < N && col < N) {
            const size_t o = (size_t)row * N + col;
            if constexpr (LOGIT) {
                x = g[o];
            } else {
                const float p = prob[o];
                x = g[o] * p * (1.0f - p);
            }
        }
        ghat[(size_t)row * Np + col] = x + mir[tc][r];          // G[row][col] + G[col][row]: symmetric bit for bit
    }
}

// ---- 2. planes of Z_k^T and H_k^T in operand order ----------------------------------------------------------------
// Per factor: [v tile][K = 16 block kb (8)][plane (3)][c (dp)][16 v] bf16 — the B operand of one MFMA (lane = column c,
// lane half h supplies v = 16 kb + 8 h .. + 7) is one 16-byte load, and a wave's 32 columns are 1 KiB contiguous.
// Zero outside N and d.  grid (nvt * dp / 32, K, 2 tables).
struct ColsJob { const float* Z; const float* H; __bf16* zT; __bf16* hT; int N, K, d, dp; size_t batch; };
__global__ __launch_bounds__(256) void split_cols_kernel(ColsJob j) {
    __shared__ float tile[TT][33];
    const int ncb = j.dp / 32;
    const int vt = blockIdx.x / ncb, cb = blockIdx.x % ncb, k = blockIdx.y;
    const float* __restrict__ src = (blockIdx.z ? j.H : j.Z) + (size_t)k * j.d;
    __bf16* __restrict__ dst = (blockIdx.z ? j.hT : j.zT) + (size_t)k * j.batch;
    const int ld = j.K * j.d;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int idx = threadIdx.x + 256 * i, r = idx >> 5, c = idx & 31;
        const int v = vt * TT + r, col = cb * 32 + c;
        tile[r][c] = (v < j.N && col < j.d) ? src[(size_t)v * ld + col] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = threadIdx.x + 256 * i, half = idx & 1, c = (idx >> 1) & 31, kb = idx >> 6;
        bf16x8 p0, p1, p2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            __bf16 h, m, l;
            split3(tile[kb * 16 + 8 * half + e][c], h, m, l);
            p0[e] = h; p1[e] = m; p2[e] = l;
        }
        __bf16* o = dst + ((size_t)(vt * KB + kb) * 3 * j.dp + cb * 32 + c) * 16 + half * 8;
        *reinterpret_cast<bf16x8*>(o) = p0;
        *reinterpret_cast<bf16x8*>(o + (size_t)j.dp * 16) = p1;
        *reinterpret_cast<bf16x8*>(o + (size_t)2 * j.dp * 16) = p2;
    }
}

// The same operand order from bf16 tables, which are their own single plane: [v tile][kb (8)][c (dp)][16 v], no arithmetic on
// the values.  Zero outside N and d; the same grid, the same coalesced reads through LDS and 16-byte stores.
struct CopyColsJob { const __bf16* Z; const __bf16* H; __bf16* zT; __bf16* hT; int N, K, d, dp; size_t batch; };
__global__ __launch_bounds__(256) void copy_cols_kernel(CopyColsJob j) {
    __shared__ __bf16 tile[TT][34];                             // 17-word rows: the column reads below spread over the banks
    const int ncb = j.dp / 32;
    const int vt = blockIdx.x / ncb, cb = blockIdx.x % ncb, k = blockIdx.y;
    const __bf16* __restrict__ src = (blockIdx.z ? j.H : j.Z) + (size_t)k * j.d;
    __bf16* __restrict__ dst = (blockIdx.z ? j.hT : j.zT) + (size_t)k * j.batch;
    const int ld = j.K * j.d;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int idx = threadIdx.x + 256 * i, r = idx >> 5, c = idx & 31;
        const int v = vt * TT + r, col = cb * 32 + c;
        tile[r][c] = (v < j.N && col < j.d) ? src[(size_t)v * ld + col] : (__bf16)0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = threadIdx.x + 256 * i, half = idx & 1, c = (idx >> 1) & 31, kb = idx >> 6;
        bf16x8 p;
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] = tile[kb * 16 + 8 * half + e][c];
        *reinterpret_cast<bf16x8*>(dst + ((size_t)(vt * KB + kb) * j.dp + cb * 32 + c) * 16 + half * 8) = p;
    }
}

// ---- 3. the main kernel -------------------------------------------------------------------------------------------
struct BwdArgs {
    const __bf16 *zp, *hp;     // row planes (split_rows): per factor plane_array_elems(N, d, 32) elements
    const __bf16 *zT, *hT;     // transposed planes (split_cols_kernel), the same size per factor
    size_t batch;
    const float* ghat;         // [Np][Np], or a strip of it: the rows of the u tiles from ut0 on
    int N, Np, K, d;
    float t;
    float *dZ, *dH;            // slice s writes at + s * slice_stride
    int nslice;
    size_t slice_stride;
    int ut0;                   // STRIP: first u tile of the launch
};

// NCB: 32-column chunks of the padded factor width.  STRIP (dl_score_recon.hip): the launch covers the u tiles from ut0 on
// and ghat holds their rows only; everything a workgroup computes for its u tile is the same.
// P: planes per table operand, 3 (fp32 tables) or 1 (bf16 tables: copy_rows / copy_cols_kernel planes, batch = Np dp).  With one
// plane the Gram products are gram_block<1> and the second products weight (3 planes) x table^T (1 plane) = mfma_split3: on
// bf16-exact finite tables the bits of the three-plane form, which multiplies the same values against planes of zeros.
template <int NCB, bool STRIP = false, int P = 3>
__global__ __launch_bounds__(BTHR) void score_dense_bwd_kernel(BwdArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int PSTAGE = P * TT * SLD;                       // one staged operand tile of this form (STAGE for P = 3)
    __bf16* us = reinterpret_cast<__bf16*>(lds);               // [2][P][TT][SLD]
    __bf16* vs = us + 2 * PSTAGE;
    __bf16* wim = us;                                          // [2 weights][3][TT][WLD], aliasing us / vs between Gram phases
    constexpr int nd = NCB, steps = 2 * nd, dp = 32 * NCB;
    const int nvt = A.Np / TT;
    const int slice = blockIdx.x % A.nslice, rest = blockIdx.x / A.nslice;
    const int k0 = rest % A.K, ut_0 = STRIP ? A.ut0 + rest / A.K : rest / A.K;
    // (one plane: the division runs on the vector unit; its uniform results go to scalar registers, see `wave` below)
    const int k = P == 1 ? __builtin_amdgcn_readfirstlane(k0) : k0, ut = P == 1 ? __builtin_amdgcn_readfirstlane(ut_0) : ut_0;
    const int vt_beg = (int)((long long)slice * nvt / A.nslice), vt_end = (int)((long long)(slice + 1) * nvt / A.nslice);
    const int u0 = ut * TT;
    // (one plane: the wave index as a scalar, so that what depends on it alone — the table pointer of the second products, the
    // store pointer, row offsets — lives in scalar registers; the three-plane forms keep their text as measured)
    const int tid = threadIdx.x, wave = P == 1 ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6, lane = tid & 63;
    const int li = lane & 31, half = lane >> 5;
    const int wu = wave >> 1, wv = wave & 1;                   // Gram: u quarter, v half; second products: u quarter, weight wv
    const __bf16* zsrc = A.zp + (size_t)k * A.batch;
    const __bf16* hsrc = A.hp + (size_t)k * A.batch;
    const __bf16* tsrc = (wv ? A.zT : A.hT) + (size_t)k * A.batch + (size_t)li * 16 + half * 8;

    PlaneStage<BTHR, SDC, P> uq, vq;
    static_assert(TT == PLANE_ROWS, "tiles of the plane arrays");
    f32x16 out[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) zero_acc(out[cb]);

    for (int vt = vt_beg; vt < vt_end; ++vt) {
        auto fetch = [&](int s) {
            const __bf16* src = s < nd ? zsrc : hsrc;
            const int dc = s < nd ? s : s - nd;
            uq.fetch(src + plane_tile<SDC, P>(ut, dc, nd), tid);
            vq.fetch(src + plane_tile<SDC, P>(vt, dc, nd), tid);
        };
        auto stash = [&](int s) {
            uq.stash(us + (s & 1) * PSTAGE, tid);
            vq.stash(vs + (s & 1) * PSTAGE, tid);
        };
        fetch(0);
        stash(0);                                               // (the previous tile's last barrier freed the buffers)
        fetch(1);                                               // steps >= 2
        f32x16 acc[2];
        float e[2][16], gh[2][16];                              // gh: G^ in accumulator layout (lane = v, registers = u)
        zero_acc(acc[0]);
        zero_acc(acc[1]);
        __syncthreads();
        auto gram_step = [&](int s, auto last_tag) {
            constexpr bool LAST = decltype(last_tag)::value;
            const __bf16* ub = us + (s & 1) * PSTAGE + (wu * 32 + li) * SLD + half * 8;
            const __bf16* vb = vs + (s & 1) * PSTAGE + (wv * 64 + li) * SLD + half * 8;
#pragma unroll
            for (int kb = 0; kb < SDC / 16; ++kb) {
                gram_block<P>(acc, ub, vb, kb);                 // dl_tiles.h: the forward's products in the forward's order
                if (kb == 0) {
                    if constexpr (!LAST) {
                        stash(s + 1);
                        fetch(min(s + 2, steps - 1));           // unconditional: see TileStage (dl_tiles.h)
                    } else if constexpr (P == 1) {
                        // One plane frees 2 staging registers, not 24, for the 32 values of G^.  Each address is a uniform
                        // 64-bit row pointer (scalar registers) plus ONE 32-bit lane offset — 4 ((4 half) Np + column) < 32 Np bytes,
                        // far under 2^32 for every N <= DL_SCORE_RECON_MAX_N — instead of a 64-bit address per row, which
                        // is what keeps this form out of scratch.
                        const float* gb = A.ghat + (size_t)((STRIP ? u0 - A.ut0 * TT : u0) + wu * 32) * A.Np + (size_t)vt * TT + wv * 64;
                        unsigned go = 4u * ((unsigned)(4 * half) * (unsigned)A.Np + (unsigned)li);      // in bytes
                        asm volatile("" : "+v"(go));            // (formed here: folded into a pointer outside the loop, it is 64-bit again)
#pragma unroll
                        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                            for (int q = 0; q < 16; ++q) {
                                const float* row = gb + (size_t)((q & 3) + 8 * (q >> 2)) * A.Np + bb * 32;
                                gh[bb][q] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(row) + go);
                            }
                    } else {                                    // the staging registers are free: G^ arrives under the last products
                        const float* gp = A.ghat + (size_t)((STRIP ? u0 - A.ut0 * TT : u0) + wu * 32 + 4 * half) * A.Np + (size_t)vt * TT + wv * 64 + li;
#pragma unroll
                        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                            for (int q = 0; q < 16; ++q) gh[bb][q] = gp[(size_t)((q & 3) + 8 * (q >> 2)) * A.Np + bb * 32];
                    }
                }
            }
            if (s == nd - 1) {                                  // S complete: e = exp(S / t)
#pragma unroll
                for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) e[bb][q] = expf(div_t(acc[bb][q], A.t));
                    zero_acc(acc[bb]);
                }
            }
            __syncthreads();
        };
        // (a rolled loop, as in the forward: unrolled over all steps the scheduler hoists LDS reads until it spills)
#pragma unroll 1
        for (int s = 0; s < steps - 1; ++s) gram_step(s, std::false_type{});
        gram_step(steps - 1, std::true_type{});
        // weights, in place: acc = Q -> G^ o Q o E / t (autograd's order: (g * q) * e, then / t);  e -> G^ o E
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                acc[bb][q] = div_t((gh[bb][q] * acc[bb][q]) * e[bb][q], A.t);
                e[bb][q] = gh[bb][q] * e[bb][q];
            }
        }
#pragma unroll
        for (int hv = 0; hv < 2; ++hv) {
            if (wv == hv) {                                     // the four waves that hold this half of the v tile
#pragma unroll
                for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int o = (wu * 32 + acc_row(q, half)) * WLD + bb * 32 + li;
                        __bf16 h, m, l;
                        split3(e[bb][q], h, m, l);
                        wim[o] = h; wim[TT * WLD + o] = m; wim[2 * TT * WLD + o] = l;
                        split3(acc[bb][q], h, m, l);
                        wim[WIMG + o] = h; wim[WIMG + TT * WLD + o] = m; wim[WIMG + 2 * TT * WLD + o] = l;
                    }
                }
            }
            __syncthreads();
            // A = weight wv, rows of this u quarter, 16 v per block; B = the v rows of H_k (wv = 0) / Z_k (wv = 1), transposed
            const __bf16* wa = wim + wv * WIMG + (wu * 32 + li) * WLD + half * 8;
            const __bf16* tb = tsrc + (size_t)(vt * KB + hv * (VH / 16)) * P * dp * 16;
#pragma unroll
            for (int kb = 0; kb < VH / 16; ++kb) {
                bf16x8 a[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) a[p] = *reinterpret_cast<const bf16x8*>(wa + p * TT * WLD + kb * 16);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    if constexpr (P == 3) {
                        bf16x8 b[3];
#pragma unroll
                        for (int p = 0; p < 3; ++p)
                            b[p] = *reinterpret_cast<const bf16x8*>(tb + ((kb * 3 + p) * dp + cb * 32) * 16);
                        mfma_split6(out[cb], a, b);             // six products, smallest terms first
                    } else {                                    // the table is its own plane: the three products against it
                        mfma_split3(out[cb], a, *reinterpret_cast<const bf16x8*>(tb + (kb * dp + cb * 32) * 16));
                    }
                }
            }
            __syncthreads();
        }
    }
    // out[cb]: lane = column c, registers = u rows.  Every (u < N, k, c < d) is written by exactly one lane.
    float* dst = (wv ? A.dZ : A.dH) + (size_t)slice * A.slice_stride;
    int sli = li, shalf = half;                                 // the lane's column and row half of the stores
    if constexpr (P == 1) {                                     // read anew (every lane is active here): nothing of the lane index
        const int l = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));     // is kept across the v loop
        sli = l & 31;
        shalf = l >> 5;
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int c = cb * 32 + sli;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int u = u0 + wu * 32 + acc_row(q, shalf);
            if (u < A.N && c < A.d) dst[((size_t)u * A.K + k) * A.d + c] = out[cb][q];
        }
    }
}

// slices of the v range summed in slice order: dZ | dH = sum_s part[s]
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ part, size_t n, int nslice, float* __restrict__ dZ,
                                                      float* __restrict__ dH) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * n) return;
    float s = part[i];
    for (int j = 1; j < nslice; ++j) s += part[(size_t)j * 2 * n + i];
    if (i < n) dZ[i] = s; else dH[i - n] = s;
}


// How many slices the v range is cut into: a function of (N, K, d) only.  A workgroup per (u tile, factor) leaves most
// of the 256 CUs idle on small graphs; aim at two workgroups per CU, at least one v tile per slice, at most 16 slices.
static int slices(int N, int K) {
    const int nt = (N + TT - 1) / TT, items = nt * K;
    if (items >= 512) return 1;
    return max(1, min(min(nt, 16), (512 + items - 1) / items));
}

struct Layout { size_t ghat, zp, hp, zT, hT, part, bytes; int Np, dp, nslice; size_t batch; };
static Layout layout(int N, int K, int d) {
    Layout L;
    L.Np = (int)round_up(N, TT);
    L.dp = (int)round_up(d, SDC);
    L.nslice = slices(N, K);
    L.batch = plane_array_elems(N, d, SDC);                    // 3 * Np * dp
    const size_t planes = align256(sizeof(__bf16) * (size_t)K * L.batch);
    L.ghat = 0;
    L.zp = align256(sizeof(float) * (size_t)L.Np * L.Np);
    L.hp = L.zp + planes;
    L.zT = L.hp + planes;
    L.hT = L.zT + planes;
    L.part = L.hT + planes;
    // the slices' partial sums: nslice * N rows at most 16 N and at most 65536 / K + N (nslice <= 512 / (nt K) + 1) — the
    // smaller of the two bounds is reserved whatever nslice is, so that the size never shrinks as N grows
    const size_t rows = std::min<size_t>((size_t)16 * N, (size_t)(65536 / K) + 1 + N);
    L.bytes = L.part + align256(sizeof(float) * rows * 2 * K * d) + 256;
    return L;
}

}  // namespace dense_bwd

bool dense_bwd_supported(int d) { return d >= 1 && d <= 128; }

size_t dense_bwd_workspace_bytes(int N, int K, int d) { return dense_bwd::layout(N, K, d).bytes; }

// out = Np, NCB, nslice (from layout, which the launch calls), and the v tiles of the shortest and of the longest slice:
// a host restatement of the split the kernel takes in device code (slice s walks the tiles [s nvt / nslice, (s + 1) nvt / nslice))
void dense_bwd_form(int N, int K, int d, int* out) {
    const dense_bwd::Layout L = dense_bwd::layout(N, K, d);
    const int nvt = L.Np / dense_bwd::TT;
    int lo = nvt, hi = 0;
    for (int s = 0; s < L.nslice; ++s) {
        const int n = (int)((long long)(s + 1) * nvt / L.nslice) - (int)((long long)s * nvt / L.nslice);
        lo = std::min(lo, n);
        hi = std::max(hi, n);
    }
    out[0] = L.Np;
    out[1] = L.dp / dense_bwd::SDC;
    out[2] = L.nslice;
    out[3] = lo;
    out[4] = hi;
}

// The planes of Z_k^T and H_k^T (stage 2) into zT / hT, K * plane_array_elems(N, d, 32) elements each
void dense_bwd_cols(const float* Z, const float* H, int N, int K, int d, __bf16* zT, __bf16* hT, hipStream_t st) {
    using namespace dense_bwd;
    const int nt = (int)round_up(N, TT) / TT, dp = (int)round_up(d, SDC);
    hipLaunchKernelGGL(split_cols_kernel, dim3((unsigned)(nt * (dp / SDC)), (unsigned)K, 2u), dim3(256), 0, st,
                       ColsJob{Z, H, zT, hT, N, K, d, dp, plane_array_elems(N, d, SDC)});
}

// ... of bf16 tables: the one plane, K * plane_array_elems<1>(N, d, 32) elements each
void copy_cols(const __bf16* Z, const __bf16* H, int N, int K, int d, __bf16* zT, __bf16* hT, hipStream_t st) {
    using namespace dense_bwd;
    const int nt = (int)round_up(N, TT) / TT, dp = (int)round_up(d, SDC);
    hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)(nt * (dp / SDC)), (unsigned)K, 2u), dim3(256), 0, st,
                       CopyColsJob{Z, H, zT, hT, N, K, d, dp, plane_array_elems<1>(N, d, SDC)});
}

int dense_bwd_nslice(int N, int K) { return dense_bwd::slices(N, K); }

// floats of the slices' partial sums (0 where the v range is not cut)
size_t dense_bwd_part_floats(int N, int K, int d) {
    const int ns = dense_bwd::slices(N, K);
    return ns > 1 ? (size_t)ns * 2 * N * K * d : 0;
}

// Stage 3 over the u tiles [ut0, ut0 + n_ut): ghat = the Np-wide rows of G^ from row ut0 * 128 on (`strip`), or the whole
// matrix (ut0 = 0, n_ut = Np / 128: the dense entry's instantiation).  The v range is cut into dense_bwd_nslice(N, K) slices whatever the u range; with more than
// one, the rows of the launch go to `part` (dense_bwd_part_floats) and dense_bwd_combine sums them once every row is there.
// dt = DL_BF16: zp .. hT are one-plane arrays (copy_rows, copy_cols) and the launch is the one-plane form, which exists as a
// strip launch only (the whole matrix is the strip from ut0 = 0).
void dense_bwd_tiles(const __bf16* zp, const __bf16* hp, const __bf16* zT, const __bf16* hT, dl_dtype dt, const float* ghat, int N,
                     int K, int d, float t, int ut0, int n_ut, bool strip, float* part, float* dZ, float* dH, hipStream_t st) {
    using namespace dense_bwd;
    const int ncb = (int)round_up(d, SDC) / SDC, nslice = slices(N, K);
    const size_t n = (size_t)N * K * d;
    BwdArgs A;
    A.zp = zp; A.hp = hp; A.zT = zT; A.hT = hT;
    A.batch = scan::table_plane_elems(dt, N, d);
    A.ghat = ghat;
    A.N = N; A.Np = (int)round_up(N, TT); A.K = K; A.d = d;
    A.ut0 = ut0;
    A.t = t;
    A.nslice = nslice;
    A.dZ = nslice > 1 ? part : dZ;
    A.dH = nslice > 1 ? part + n : dH;
    A.slice_stride = nslice > 1 ? 2 * n : 0;
    const unsigned grid = (unsigned)((size_t)n_ut * K * nslice);
#define DL_LAUNCH_BWD(NCB)                                                                                               \
    do {                                                                                                                 \
        if (dt == DL_BF16) scan::launch_lds<score_dense_bwd_kernel<NCB, true, 1>>(grid, BTHR, lds_bytes(1), st, A);      \
        else if (strip) scan::launch_lds<score_dense_bwd_kernel<NCB, true>>(grid, BTHR, LDS_BYTES, st, A);               \
        else scan::launch_lds<score_dense_bwd_kernel<NCB>>(grid, BTHR, LDS_BYTES, st, A);                                \
    } while (0)
    switch (ncb) {
        case 1: DL_LAUNCH_BWD(1); break;
        case 2: DL_LAUNCH_BWD(2); break;
        case 3: DL_LAUNCH_BWD(3); break;
        default: DL_LAUNCH_BWD(4); break;
    }
#undef DL_LAUNCH_BWD
}

void dense_bwd_combine(const float* part, int N, int K, int d, float* dZ, float* dH, hipStream_t st) {
    using namespace dense_bwd;
    const int nslice = slices(N, K);
    const size_t n = (size_t)N * K * d;
    if (nslice > 1)
        hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, st, part, n, nslice, dZ, dH);
}

// prob == NULL: g_prob is the gradient with respect to the LOGITS (dl_score_allpairs_logits_bwd_dense), G^ = g + g^T
int dense_bwd_score_allpairs(const float* Z, const float* H, int N, int K, int d, float t, const float* prob, const float* g_prob,
                             float* dZ, float* dH, void* ws, hipStream_t st) {
    using namespace dense_bwd;
    const Layout L = layout(N, K, d);
    char* base = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    float* ghat = (float*)(base + L.ghat);
    __bf16 *zp = (__bf16*)(base + L.zp), *hp = (__bf16*)(base + L.hp), *zT = (__bf16*)(base + L.zT), *hT = (__bf16*)(base + L.hT);
    float* part = (float*)(base + L.part);

    const dim3 ggrid((unsigned)(L.Np / 64), (unsigned)(L.Np / 64));
    if (prob == nullptr) hipLaunchKernelGGL(ghat_kernel<true>, ggrid, dim3(256), 0, st, prob, g_prob, N, L.Np, ghat);
    else hipLaunchKernelGGL(ghat_kernel<false>, ggrid, dim3(256), 0, st, prob, g_prob, N, L.Np, ghat);
    project::split_rows(Z, K, N, d, K * d, (size_t)d, zp, st);
    project::split_rows(H, K, N, d, K * d, (size_t)d, hp, st);
    dense_bwd_cols(Z, H, N, K, d, zT, hT, st);
    dense_bwd_tiles(zp, hp, zT, hT, DL_F32, ghat, N, K, d, t, 0, L.Np / TT, false, part, dZ, dH, st);
    dense_bwd_combine(part, N, K, d, dZ, dH, st);
    return check_launch("score_allpairs_bwd_dense");
}

}  // namespace dl
