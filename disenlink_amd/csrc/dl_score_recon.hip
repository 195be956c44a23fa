// Whole-graph reconstruction loss and its gradient with nothing of size N x N in memory (dl_score_recon).
//
// Contract.  Included pairs: all unordered {u, v}, u != v, outside the ignored set.  For an included pair
//   s = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t),  p = sigmoid(s),  y = 1 if it is a positive, else 0,
//   w = w_pos (y = 1) or w_neg (y = 0)      (the caller's pos_weight / C and 1 / C, C = the number of included pairs),
//   loss = sum w BCE(p, y)                  (F.binary_cross_entropy's clamp of the logs at -100, as dl_pair_bce),
//   d loss / d s = w (p - y)                (the one-pass scorer's form with its max(p (1 - p), 1e-12) clamp: a saturated
//                                            pair contributes exactly 0).
// The gradient depends on the pair alone, so G^ (dl_score_dense_bwd.hip) is formed where the logit is formed, one strip of
// block_rows rows at a time:
//   1. planes of Z, H (split_rows) and of their transposes (split_cols_kernel), once per call — bf16 tables (DL_BF16) are
//      their own single plane, copied into the same layouts (copy_rows, copy_cols_kernel), and 2. runs in its one-plane forms;
//   2. per strip: the ranking scan in its RECON mode (dl_score_rank.hip) over the strip's rows against ALL candidate tiles
//      writes the strip of G^ (zero for ignored pairs, the diagonal and outside N) and, per (row, candidate tile), one loss
//      cell and one count cell, each exactly once; row_sum_kernel adds a row's cells in tile order (fp64, integers);
//      score_dense_bwd_kernel runs over the strip's u tiles with the strip as its G^.  The v range is cut as a function of
//      the WHOLE N and K, so a row of dZ / dH has the same bits whatever the strip height;
//   3. the slices' partial sums are combined, and finish_kernel adds the rows in one fixed order and halves: every unordered
//      pair was visited from both of its rows (halving is exact).
// No tile is skipped: as in the dense backward, a zero of G^ against an overflowed E = inf gives NaN in dZ / dH.
// Logit space (dl_score_recon_logits): the same sets, weights, strips and launches with, per included pair,
//   loss term = w l(s, y),  l = (1 - y) max(s, 0) + y max(-s, 0) + log1p(exp(-|s|))   (bce_logits_term, dl_common.h),
//   d loss / d s = w (sigmoid(s) - y)                                                  (sigmoid_minus_label: no clamp factor),
// so a saturated pair keeps its cost and its gradient; a non-finite logit gives a non-finite loss and gradient.
// Node-group rule (dl_score_recon_filtered, dl_score_recon_logits_filtered; dl_node_filter, NULL = none): the included pairs are
// further those the rule admits, allow[group[u]] bit group[v], which the caller gives in its symmetric (unordered) form.  A
// denied pair behaves exactly like an ignored one, edge or not: no loss term, G^ = 0, not counted; the caller's w_pos, w_neg
// are taken over the pairs that remain.  The scan's RECON x FILT instantiations form the rule's 128 x 128 deny mask of a
// candidate tile into the ignored mask; strips, launches, workspace and every guarantee below are the unfiltered call's, and
// no tile is skipped under a rule either (a tile pair denied whole still writes its zeros of G^ and is still multiplied).
// No float atomics, no host read, everything on the caller's stream; the same bits on every call, for every block_rows and
// for every slice count of the scan (DL_RANK_SLICES).
#include <algorithm>
#include "dl_common.h"
#include "dl_kernels.h"
#include "dl_scan.h"

namespace dl {
namespace recon {

using namespace scan;

constexpr int TT = PLANE_ROWS;
constexpr size_t STRIP_BYTES = (size_t)1 << 30;               // the default strip stays at or under this

__global__ __launch_bounds__(256) void row_sum_kernel(const float* __restrict__ lcell, const unsigned* __restrict__ ccell, int rows,
                                                      int nt, int q0, double* __restrict__ rowloss, u64* __restrict__ rowcnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    double s = 0.0;
    u64 np = 0, nn = 0;
    for (int c = 0; c < nt; ++c) {
        s += (double)lcell[(size_t)i * nt + c];
        const unsigned x = ccell[(size_t)i * nt + c];
        np += x & 0xFFFFu;
        nn += x >> 16;
    }
    rowloss[q0 + i] = s;
    rowcnt[2 * (size_t)(q0 + i)] = np;
    rowcnt[2 * (size_t)(q0 + i) + 1] = nn;
}

// one workgroup: thread j adds the rows j, j + 256, ... in order, then a tree over the threads; halved
__global__ __launch_bounds__(256) void finish_kernel(const double* __restrict__ rowloss, const u64* __restrict__ rowcnt, int N,
                                                     double* __restrict__ loss, int64_t* __restrict__ counts) {
    __shared__ double sl[256];
    __shared__ u64 sp[256], sn[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    u64 np = 0, nn = 0;
    for (int i = tid; i < N; i += 256) {
        s += rowloss[i];
        np += rowcnt[2 * (size_t)i];
        nn += rowcnt[2 * (size_t)i + 1];
    }
    sl[tid] = s; sp[tid] = np; sn[tid] = nn;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            sl[tid] += sl[tid + w];
            sp[tid] += sp[tid + w];
            sn[tid] += sn[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        loss[0] = 0.5 * sl[0];
        counts[0] = (int64_t)(sp[0] / 2);
        counts[1] = (int64_t)(sn[0] / 2);
    }
}

struct Plan { int Np, nt, block_rows, strips, nslice; size_t batch; };
static Plan plan(int N, int K, int d, dl_dtype dt, int block_rows) {
    Plan p;
    p.Np = (int)round_up(N, TT);
    p.nt = p.Np / TT;
    if (block_rows <= 0) block_rows = (int)std::max<size_t>(TT, STRIP_BYTES / ((size_t)p.Np * 4) / TT * TT);
    p.block_rows = std::min(block_rows, p.Np);
    p.strips = (p.Np + p.block_rows - 1) / p.block_rows;
    p.nslice = dense_bwd_nslice(N, K);
    p.batch = table_plane_elems(dt, N, d);                     // the one thing of a plan that depends on the table type
    return p;
}

// Workspace (256-byte aligned blocks): planes of Z | H | Z^T | H^T (2 K 3 Np dp bytes each; bf16 tables: 2 K Np dp) | one strip of G^ (4 block_rows Np)
// | loss cells | count cells (4 block_rows Np / 128 each) | row losses (8 N) | row counts (16 N) | the dense backward's slice
// partials (4 nslice 2 N K d, none for nslice = 1).  Nothing of size N x N.
struct Ws {
    __bf16 *zp, *hp, *zT, *hT;
    float *ghat, *lcell, *part;
    unsigned* ccell;
    double* rowloss;
    u64* rowcnt;
    size_t bytes;
};
static Ws carve(const Plan& p, int N, int K, int d, void* ws) {
    Ws w = {};
    Carver c(ws);
    w.zp = c.take<__bf16>((size_t)K * p.batch);
    w.hp = c.take<__bf16>((size_t)K * p.batch);
    w.zT = c.take<__bf16>((size_t)K * p.batch);
    w.hT = c.take<__bf16>((size_t)K * p.batch);
    w.ghat = c.take<float>((size_t)p.block_rows * p.Np);
    w.lcell = c.take<float>((size_t)p.block_rows * p.nt);
    w.ccell = c.take<unsigned>((size_t)p.block_rows * p.nt);
    w.rowloss = c.take<double>((size_t)N);
    w.rowcnt = c.take<u64>((size_t)2 * N);
    w.part = c.take<float>(dense_bwd_part_floats(N, K, d));
    w.bytes = c.bytes();
    return w;
}

}  // namespace recon

bool score_recon_supported(int K, int d) { return score_rank_supported(K, d) && dense_bwd_supported(d); }

// out = Np, strips, rows per strip, slices of the dense backward's v range
void score_recon_form(int N, int K, int d, dl_dtype dt, int block_rows, int* out) {
    const recon::Plan p = recon::plan(N, K, d, dt, block_rows);
    out[0] = p.Np;
    out[1] = p.strips;
    out[2] = p.block_rows;
    out[3] = p.nslice;
}

size_t score_recon_workspace_bytes(int N, int K, int d, dl_dtype dt, int block_rows) {
    return recon::carve(recon::plan(N, K, d, dt, block_rows), N, K, d, nullptr).bytes;
}

// logit: the scan's epilogue takes the loss term and G^ in logit space (the contract below); every launch behind it is the same.
// dt: the type of Z and H.  DL_BF16: the tables are their own single plane (copy_rows, copy_cols), the scan and the backward
// run in their one-plane forms, everything behind them is the same.  nf: the node-group rule of the scan, NULL = none.
int score_recon(const void* Z, const void* H, int N, int K, int d, dl_dtype dt, float t, const int32_t* pos_rowptr,
                const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg, int block_rows,
                bool logit, double* loss, int64_t* counts, float* dZ, float* dH, void* ws, hipStream_t st, const dl_node_filter* nf) {
    using namespace recon;
    const Plan p = plan(N, K, d, dt, block_rows);
    const Ws w = carve(p, N, K, d, ws);
    table_planes(Z, dt, nullptr, N, K, d, w.zp, st);
    table_planes(H, dt, nullptr, N, K, d, w.hp, st);
    if (dt == DL_BF16) copy_cols((const __bf16*)Z, (const __bf16*)H, N, K, d, w.zT, w.hT, st);
    else dense_bwd_cols((const float*)Z, (const float*)H, N, K, d, w.zT, w.hT, st);
    for (int q0 = 0; q0 < N; q0 += p.block_rows) {
        const int rows = std::min(p.block_rows, N - q0);
        score_recon_strip(w.zp, w.hp, dt, N, K, d, t, q0, rows, pos_rowptr, pos_col, ign_rowptr, ign_col, w_pos, w_neg, logit, nf, w.ghat, w.lcell,
                          w.ccell, st);
        hipLaunchKernelGGL(row_sum_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, w.lcell, w.ccell, rows, p.nt, q0,
                           w.rowloss, w.rowcnt);
        dense_bwd_tiles(w.zp, w.hp, w.zT, w.hT, dt, w.ghat, N, K, d, t, q0 / TT, (rows + TT - 1) / TT, true, w.part, dZ, dH, st);
    }
    dense_bwd_combine(w.part, N, K, d, dZ, dH, st);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, st, w.rowloss, w.rowcnt, N, loss, counts);
    return check_launch("score_recon");
}

}  // namespace dl
