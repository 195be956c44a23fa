// Ranking of all candidate links of a set of query nodes on the matrix cores: top-k per query row (dl_score_topk) and
// filtered rank counts of target pairs (dl_score_ranks), with the logit of the dense scorer (dl_score_dense.hip),
//   s(u, v) = sum_k (h_k[u].h_k[v]) * exp(z_k[u].z_k[v] / t),
// and nothing of size Q x N in memory.
//
// Scan: one workgroup = 8 waves = a tile of 128 query rows against a SLICE of consecutive 128-row candidate tiles; per
// candidate tile the Gram products run exactly as in the dense scorer (gram_block_split6 of dl_tiles.h: three bf16 planes
// per operand, six exact products, double-buffered LDS staging, the query as the A operand).  The query rows are gathered
// into a compact array and split once per call; the candidates are read from the plane arrays of Z and H (split_rows).
// Work items (query tile x slice) are dealt to the XCDs by xcd_item.  What follows the products per candidate tile:
//   * exclusion: a 128-bit mask per query row, from the row's ascending excluded columns (a cursor that only moves forward
//     through the tiles of a slice: one binary search per row and workgroup).
//   * node groups (the FILT instantiations; dl_score_topk_filtered, dl_score_ranks_filtered): a rule on the groups of the
//     row's and the candidate's node, formed into the same mask ahead of the exclusion (see rank_scan_kernel).
//   * top-k: a per-(row, slice) list in global memory of cap = k + 64 keys.  A candidate is appended only if its key beats
//     the row's running threshold (the k-th best key of the list after its last compaction; kept in LDS).  A round of
//     appends adds at most 64 keys per row (two waves x 32 lanes); a list that could overflow in the next round is
//     compacted by one wave: its sorted prefix (the previous compaction's output) and the new keys are ranked against each
//     other and the first k written back in order.  A merge kernel combines the slices' sorted lists by rank.
//   * ranks: each query row's target logits, sorted once, live in global memory; a candidate that reaches the smallest
//     of them finds its place by binary search and adds 1 to an integer counter (a difference array summed at the end).
// Keys order the logits totally: larger first, +inf above every finite value, -inf below, NaN below everything; equal
// values by candidate index, smaller first.  Everything selected or counted is a function of the logits alone, and the
// logit of a pair does not depend on where in a tile its rows sit: results are independent of the slicing and of the run.
// Given pairs (dl_score_pair_logits, dl_score_pair_terms): the DIAG and TERMS instantiations, a tile of 128 pairs against itself
// with the diagonal kept.  DIAG writes the logit; TERMS writes, per factor, what the pass holds on the way to it: e = exp(S / t),
// q = h.h and the running sum, whose last column has the logit's bits ("which factor makes this link").
// Reconstruction loss (dl_score_recon, driven by dl_score_recon.hip): the RECON instantiation, a strip of consecutive rows as
// the queries against all candidate tiles; its epilogue writes, per value, the loss gradient into a strip of G^ for the dense
// backward's kernel and, per (row, candidate tile), one loss cell and one count cell (recon_epilogue).
// bf16 tables (the *_dtype entries with DL_BF16): the P = 1 instantiations, one plane per operand (copy_rows, which also
// gathers the query rows) and one product per block; on the same values, the bits of the three-plane scan.
#include "dl_common.h"
#include "dl_kernels.h"
#include "dl_scan.h"

namespace dl {
namespace rank {

using namespace project;       // PlaneStage, gram_block_split6, f32x16, acc_row, xcd_item, plane arrays
using namespace scan;          // ord_key / ord_value / make_key, the exclusion search of the target kernels, host scaffolding

constexpr int TT = 128;        // tile edge (query rows and candidate rows)
constexpr int RTHR = 512;
constexpr int SDC = SPLIT_COLS, SLD = SPLIT_PITCH;
constexpr int MAX_K = 128;
constexpr int ROUND = 64;      // keys one round of appends can add to a row's list
constexpr int MAX_CAP = MAX_K + ROUND;
constexpr int MAX_SLICES = 32;
enum { TOPK = 0, RANKS = 1, DIAG = 2, TERMS = 3, RECON = 4 };

struct ScanArgs {
    const __bf16 *qz, *qh;  size_t qbatch;     // planes of the gathered query rows (per factor: qbatch elements)
    const __bf16 *cz, *ch;  size_t cbatch;     // planes of Z and H (the candidates)
    int Q, N, K, nd;  float t;
    const int32_t* qnode;                      // [Q] node of each query row
    const int32_t *ex_rowptr, *ex_col;         // exclusion CSR over nodes (ascending columns), or NULL
    int exclude_self;
    int slices, tiles_per_slice;
    int k, cap;  u64* lists;  int* counts;     // TOPK: lists [Q][slices][cap], counts [Q][slices]
    const int32_t* tptr;  const unsigned* tord;  u64* gcnt;  u64* tcnt;   // RANKS
    const int32_t *trow, *tdst;  int T;  float* tlogit;                 // DIAG: target i = (query row trow[i], node tdst[i])
    FilterArgs filt;                                                    // FILT: the node-group rule (dl_tiles.h)
    float *te, *tq, *tcum;                     // TERMS: [T][K] each, NULL = not wanted (targets as in DIAG)
};
// RECON has arguments of its own behind them (the other modes' kernels keep their argument block): query row i is node
// q0 + i (no qnode array); ex_* = the positives, ig_* = the ignored pairs (NULL: none), both symmetric CSRs; ghat
// [>= 128 qtiles][128 nt] and one cell per (row, candidate tile): the row's loss over the tile and its positives | negatives << 16
struct ReconArgs : ScanArgs {
    int q0;
    const int32_t *ig_rowptr, *ig_col;
    float w_pos, w_neg;
    float* ghat;  float* lcell;  unsigned* ccell;
};
template <int MODE> struct ModeArgs { typedef ScanArgs type; };
template <> struct ModeArgs<RECON> { typedef ReconArgs type; };

// LDS with P planes per operand (bytes): the two double-buffered staging images, the logits' way through LDS, then the
// exclusion mask, per-row bookkeeping, per-wave compaction scratch.  The epilogue passes each wave's logits through 4 KiB of
// LDS: with three planes that is the staging image the step has finished reading (30 KiB, four waves each); a one-plane
// image (10 KiB) is too small for that, so the one-plane instantiations keep 8 x 4 KiB of their own behind the images.
// RECON's epilogue reads its values back transposed and keeps a pitch of its own (RPITCH), a little more per wave: `recon`.
constexpr size_t LG_WAVE = 16 * DL_WAVE;                       // floats per wave
constexpr int RPITCH = DL_WAVE + 1, RLG = 16 * RPITCH;         // RECON: the pitch and the floats per wave (recon_epilogue)
constexpr size_t lg_bytes(int P, bool recon = false) { return P == 3 ? 0 : 8 * (recon ? (size_t)RLG : LG_WAVE) * 4; }
constexpr size_t lds_bytes(int P, bool recon = false) {
    return (size_t)2 * 2 * P * TT * SLD * 2 + lg_bytes(P, recon) + TT * 4 * 4 + 6 * TT * 4 + TT * 8 + 8 * MAX_CAP * 8;
}
static_assert(lds_bytes(1, true) % 16 == 0 && lg_bytes(3, true) == 0, "RECON: three planes as before, one plane aligned");
static_assert(lds_bytes(3) % 16 == 0 && lds_bytes(1) % 16 == 0 && lds_bytes(3) + FILTER_LDS_BYTES <= 160 * 1024, "LDS of a CU");
static_assert(lds_bytes(1, true) + FILTER_LDS_BYTES <= 160 * 1024, "LDS of a CU: RECON x FILT on one plane (three planes: lds_bytes(3))");
static_assert(4 * LG_WAVE * 4 <= (size_t)3 * TT * SLD * 2, "four waves' logits fit a three-plane image");

// A PlaneStage tile whose 128 rows are gathered: row r of the tile is row rows[min(base + r, n - 1)] of the plane array.
template <int P>
__device__ __forceinline__ void gather_fetch(PlaneStage<RTHR, SDC, P>& st, const __bf16* __restrict__ planes, const int32_t* rows,
                                             int base, int n, int dc, int nd, int tid) {
    static_assert(PlaneStage<RTHR, SDC, P>::PER == 1, "one 16-byte piece per plane and thread");
    const int r = tid / (SDC / 8), c = (tid % (SDC / 8)) * 8;
    const int row = rows[min(base + r, n - 1)];
    const __bf16* src = planes + plane_tile<SDC, P>(row / PLANE_ROWS, dc, nd) + (row % PLANE_ROWS) * SDC + c;
#pragma unroll
    for (int p = 0; p < P; ++p)
        st.v[p] = *reinterpret_cast<const typename PlaneStage<RTHR, SDC, P>::u32x4*>(src + (size_t)p * PLANE_ROWS * SDC);
}

// TERMS: which of a lane's 2 x 16 accumulator elements lies on the tile's diagonal (DIAG's ul == vl), as bb * 16 + q, or -1:
// at most one per lane.  Found once per workgroup, so that a store is a tree of selects on the bits of the index and the
// 32 values stay in registers.
__device__ __forceinline__ int diagonal_element(int wu, int wv, int li, int half) {
    int sel = -1;
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (wu * 32 + acc_row(q, half) == wv * 64 + bb * 32 + li) sel = bb * 16 + q;
    }
    return sel;
}
// x[sel >> 4][sel & 15], sel in [0, 32).  Every value passes an empty asm on its way into a select: the compiler would
// otherwise turn selects of array elements into one load at a selected address, which puts the array into scratch.
__device__ __forceinline__ float in_register(float v) {
    asm("" : "+v"(v));
    return v;
}
__device__ __forceinline__ float pick2(bool odd, float even_v, float odd_v) { return in_register(odd ? odd_v : even_v); }
template <class V>
__device__ __forceinline__ float pick16(const V& x, bool b0, bool b1, bool b2, bool b3) {
#define DL_PAIR(j) pick2(b0, in_register(x[2 * (j)]), in_register(x[2 * (j) + 1]))
    const float c0 = pick2(b2, pick2(b1, DL_PAIR(0), DL_PAIR(1)), pick2(b1, DL_PAIR(2), DL_PAIR(3)));
    const float c1 = pick2(b2, pick2(b1, DL_PAIR(4), DL_PAIR(5)), pick2(b1, DL_PAIR(6), DL_PAIR(7)));
#undef DL_PAIR
    return pick2(b3, c0, c1);
}
template <class V>
__device__ __forceinline__ float pick_element(const V (&x)[2], int sel) {
    const bool b0 = sel & 1, b1 = sel & 2, b2 = sel & 4, b3 = sel & 8;
    return pick2(sel & 16, pick16(x[0], b0, b1, b2, b3), pick16(x[1], b0, b1, b2, b3));
}

// Rank one row's list against itself and write its best min(n, k) keys back in order (one wave; between barriers).
// Keys [0, srt) are sorted (descending) from the previous compaction, keys [srt, n) are new.
__device__ __forceinline__ void compact_row(u64* __restrict__ L, u64* S, int n, int srt, int k, int lane, u64* thr_out,
                                            int* cnt_out, int* srt_out) {
    for (int i = lane; i < n; i += DL_WAVE) S[i] = L[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    constexpr int E = (MAX_CAP + DL_WAVE - 1) / DL_WAVE;
    u64 mine[E];
    int rk[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + DL_WAVE * e;
        mine[e] = i < n ? S[i] : 0ull;
        rk[e] = 0;
    }
    for (int j = srt; j < n; ++j) {                             // against the new keys
        const u64 x = S[j];
#pragma unroll
        for (int e = 0; e < E; ++e) rk[e] += x > mine[e] ? 1 : 0;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + DL_WAVE * e;
        if (i < srt) {
            rk[e] += i;                                         // the old keys above it: its position
        } else {                                                // old keys above a new one: binary search
            int lo = 0, hi = srt;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (S[mid] > mine[e]) lo = mid + 1; else hi = mid;
            }
            rk[e] += lo;
        }
    }
    const int keep = min(n, k);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + DL_WAVE * e;
        if (i < n && rk[e] < keep) L[rk[e]] = mine[e];
        if (i < n && n >= k && rk[e] == k - 1) *thr_out = mine[e];
    }
    if (lane == 0) {
        *cnt_out = keep;
        *srt_out = keep;
    }
}

// RECON: the whole-graph reconstruction loss of a candidate tile (dl_score_recon.hip has the contract).  Two masks per row,
// positives and ignored (the second one and the sums of the two v halves live where the top-k modes keep their compaction
// scratch); per value p = sigmoid(s), the weighted BCE term with F.binary_cross_entropy's clamps and g = w (p - y) in the
// one-pass scorer's form (dl_train.h), written to the strip of G^ — zero where the pair carries no loss: ignored, the
// diagonal, outside N.  As in the other modes the values go through LDS so that the loop over a lane's 16 rows stays rolled
// (lg: RLG floats of the wave's own, pitch 65: the transposed read below is conflict-free); the loss terms come back the
// same way and the 128 terms of a row are added in one fixed order — 16 consecutive columns by one lane, the two halves of a
// 32-column block, the two blocks of a wave, the two waves — so a cell is a function of its logits alone.  Counts: ballots.
// LOGIT (dl_score_recon_logits): per value the term w l(s, y) of BCE-with-logits (bce_logits_term) and g = w (sigmoid(s) - y)
// without a clamp (sigmoid_minus_label), both of dl_common.h; masks, stores, sums and counts are the same text.
// FILT (dl_score_recon_filtered): a pair the node-group rule denies is an ignored pair.  The scan has put the rule's deny words
// of the tile into igm (see rank_scan_kernel), so the row threads OR the ignored columns and the diagonal into them where the
// unfiltered epilogue starts from zero; everything behind the masks is the same text.
static_assert(4 * RLG * 4 <= 3 * TT * SLD * 2, "four waves' terms fit a three-plane image");
template <bool LOGIT, bool FILT>
__device__ __forceinline__ void recon_epilogue(const ReconArgs& A, const f32x16 (&term)[2], float* lg, unsigned* pom, unsigned* scr,
                                               int* pocur, int* igcur, const int* rnode, int qt, int ct, int nt, int tid) {
    unsigned* igm = scr;                                        // [TT][4]: ignored columns of the tile, the diagonal among them
    float* redl = reinterpret_cast<float*>(scr + TT * 4);       // [2 v halves][TT]
    unsigned* redc = scr + TT * 4 + 2 * TT;                     // [2][TT]
    const int wave = tid >> 6, lane = tid & 63, li = lane & 31, half = lane >> 5, wu = wave >> 1, wv = wave & 1;
    const int v0 = ct * TT;
    if (tid < TT) {
        const int node = rnode[tid];
        unsigned *m = pom + tid * 4, *g = igm + tid * 4;
        m[0] = m[1] = m[2] = m[3] = 0u;
        if constexpr (!FILT) g[0] = g[1] = g[2] = g[3] = 0u;
        if (node >= 0) {
            pocur[tid] = exclusion_mask(A.ex_col, pocur[tid], A.ex_rowptr[node + 1], v0, m);
            if (A.ig_rowptr != nullptr) igcur[tid] = exclusion_mask(A.ig_col, igcur[tid], A.ig_rowptr[node + 1], v0, g);
            if (node >= v0 && node < v0 + TT) g[(node - v0) >> 5] |= 1u << ((node - v0) & 31);
        }
    }
    __syncthreads();
    const size_t Np = (size_t)nt * TT;
    const int sq = lane & 15, sh = (lane >> 4) & 1, sp = lane >> 5;   // the sums: row (sq, sh), columns 16 sp .. 16 sp + 15 of a block
    float racc = 0.0f;
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const int w = wv * 2 + bb;                              // the mask word of this 32-column block: bit li
        const bool inside = v0 + w * 32 + li < A.N;
#pragma unroll
        for (int q = 0; q < 16; ++q) lg[q * RPITCH + lane] = term[bb][q];
#pragma unroll 1
        for (int q = 0; q < 16; ++q) {
            const int row = wu * 32 + acc_row(q, half);
            const bool live = inside && rnode[row] >= 0 && !((igm[row * 4 + w] >> li) & 1u);
            const bool pos = (pom[row * 4 + w] >> li) & 1u;
            float bce, gl;
            if constexpr (LOGIT) {                              // logit space: the pair objective's term and gradient, no clamp
                const float x = lg[q * RPITCH + lane], y = pos ? 1.0f : 0.0f, ww = pos ? A.w_pos : A.w_neg;
                bce = ww * bce_logits_term(x, y);
                gl = ww * sigmoid_minus_label(x, y);
            } else {
                const float p = sigmoid_ref(lg[q * RPITCH + lane]);
                const float lgp = logf(pos ? p : 1.0f - p);     // F.binary_cross_entropy: the log clamped at -100 (dl_pair_bce)
                const float ww = pos ? A.w_pos : A.w_neg, r = p * (1.0f - p);
                bce = ww * -(lgp < -100.0f ? -100.0f : lgp);
                gl = ww * (p - (pos ? 1.0f : 0.0f)) * (r >= 1e-12f ? 1.0f : r * 1e12f);
            }
            A.ghat[((size_t)qt * TT + row) * Np + v0 + w * 32 + li] = live ? gl : 0.0f;
            lg[q * RPITCH + lane] = live ? bce : 0.0f;
            const u64 mp = __ballot(live && pos), mn = __ballot(live && !pos);
            if (li == 0) {
                const unsigned c = __popc((unsigned)(mp >> (32 * half))) | ((unsigned)__popc((unsigned)(mn >> (32 * half))) << 16);
                redc[wv * TT + row] = bb == 0 ? c : redc[wv * TT + row] + c;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) a += lg[sq * RPITCH + sh * 32 + sp * 16 + i];
        a += __shfl_xor(a, 32);
        racc = bb == 0 ? a : racc + a;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane < 32) redl[wv * TT + wu * 32 + acc_row(sq, sh)] = racc;
    __syncthreads();
    if (tid < TT) {                                             // every cell written once, zeros included
        const size_t cell = ((size_t)qt * TT + tid) * nt + ct;
        A.lcell[cell] = redl[tid] + redl[TT + tid];
        A.ccell[cell] = redc[tid] + redc[TT + tid];
    }
}

// FILT: the node-group rule on top of the exclusion.  All 512 threads form the tile's mask from the rule, one word each, in
// the tile's last pipeline step (the candidates' groups were staged one step earlier: a tile has K * 2 * nd >= 2 steps, and
// every reader of the previous tile's mask and groups is behind a barrier by then); the row threads then OR the exclusion
// into it where the unfiltered kernel starts from zero.  The epilogue is the unfiltered one.
// RECON x FILT (dl_score_recon_filtered): exm holds the positives there, and a denied pair is an IGNORED one, so the words go to
// the ignored mask igm, the first [TT][4] words of scr.  The same ordering holds for it: the only readers of igm are the value
// loops of the previous tile's recon_epilogue, which lie before that epilogue's last __syncthreads, and the words are written
// in step per_tile - 1 >= 1 of this tile, behind that barrier and the one that ends step 0; what the epilogue keeps in scr
// behind igm (redl, redc) is not touched.  The first tile of a work item has no earlier reader, and all TT * 4 words are
// written, so igm never holds what the last work item left.  The barrier that ends the step stands between the 512 writers and
// the row threads that OR the ignored columns and the diagonal in.  A row outside the strip (rnode < 0) takes group 0 and a
// column >= N group 0: either word is formed and never read as live (the epilogue tests rnode and N itself).
// P: planes per operand, 3 (fp32 tables) or 1 (bf16 tables: one bf16x8 and one MFMA per operand and block, gram_block<1>); the
// step keeps its 32 columns, so the k-blocks of a product are added in the same ascending order in both.
// LOGIT (RECON only): the loss term and the gradient of the epilogue in logit space (dl_score_recon_logits).
template <int MODE, bool FILT = false, int P = 3, bool LOGIT = false>
__global__ __launch_bounds__(RTHR) void rank_scan_kernel(typename ModeArgs<MODE>::type A) {
    static_assert(!LOGIT || MODE == RECON, "only the reconstruction epilogue has a logit-space form");
    static_assert(!(FILT && (MODE == DIAG || MODE == TERMS)), "the target passes have no mask");
    constexpr bool PAIRS = MODE == DIAG || MODE == TERMS;      // TERMS: DIAG's geometry and gathers, other stores
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __bf16* us = reinterpret_cast<__bf16*>(lds);               // [2][P][TT][SLD]
    __bf16* vs = us + 2 * P * TT * SLD;
    float* lgs = reinterpret_cast<float*>(vs + 2 * P * TT * SLD);         // P = 1: [8][LG_WAVE], see lg_bytes
    unsigned* exm = reinterpret_cast<unsigned*>(lgs + lg_bytes(P, MODE == RECON) / 4);   // [TT][4]: excluded columns of the tile
    int* cnt = reinterpret_cast<int*>(exm + TT * 4);           // TOPK: keys in the row's list
    int* srt = cnt + TT;                                        // TOPK: of which sorted
    int* excur = srt + TT;                                      // next exclusion entry of the row
    int* rnode = excur + TT;                                    // node of the row (-1: no row)
    int* rbase = rnode + TT;                                    // RANKS: first target of the row
    int* rm = rbase + TT;                                       // RANKS: targets of the row
    u64* thr = reinterpret_cast<u64*>(rm + TT);                 // TOPK: threshold key; RANKS: smallest target order
    u64* scr = thr + TT;                                        // [8][MAX_CAP]: compaction scratch of each wave
    u64* fal = scr + 8 * MAX_CAP;                               // FILT: allow [64] | cgrp [TT] | rgrp [TT]
    unsigned char* cgrp = reinterpret_cast<unsigned char*>(fal + 64);
    unsigned char* rgrp = cgrp + TT;

    const int nrows = PAIRS ? A.T : A.Q;
    const int qtiles = (nrows + TT - 1) / TT;
    const int nslices = PAIRS ? 1 : A.slices;
    const XcdItem it = xcd_item((int)blockIdx.x, qtiles, nslices);
    if (!it.valid) return;
    const int qt = it.a, sl = it.b;
    const int nt = (A.N + TT - 1) / TT;
    int ct0 = qt, ntl = 1;
    if constexpr (!PAIRS) {
        ct0 = sl * A.tiles_per_slice;
        ntl = max(0, min(nt, ct0 + A.tiles_per_slice) - ct0);
    }
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, half = lane >> 5;
    const int wu = wave >> 1, wv = wave & 1;
    const int nd = A.nd;
    const int per_tile = A.K * 2 * nd;
    const int steps = ntl * per_tile;

    if constexpr (!PAIRS) {
        if (tid < TT) {
            const int qi = qt * TT + tid;
            int node = -1;
            if constexpr (MODE == RECON) node = qi < A.Q ? A.q0 + qi : -1;
            else node = qi < A.Q ? A.qnode[qi] : -1;
            rnode[tid] = node;
            cnt[tid] = 0;
            srt[tid] = 0;
            thr[tid] = 0ull;
            if constexpr (FILT) {
                rgrp[tid] = node >= 0 ? A.filt.group[node] : (unsigned char)0;
                if (tid < 64) fal[tid] = tid < A.filt.n_groups ? A.filt.allow[tid] : 0ull;
            }
            if (node >= 0 && A.ex_rowptr != nullptr) {          // first excluded column >= the slice's first candidate
                int lo = A.ex_rowptr[node], hi = A.ex_rowptr[node + 1];
                const int v0 = ct0 * TT;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (A.ex_col[mid] < v0) lo = mid + 1; else hi = mid;
                }
                excur[tid] = lo;
            }
            if constexpr (MODE == RECON) {                       // cnt: the cursor into the row's ignored columns
                if (node >= 0 && A.ig_rowptr != nullptr)
                    cnt[tid] = first_col_at_least(A.ig_col, A.ig_rowptr[node], A.ig_rowptr[node + 1], ct0 * TT);
            }
            if constexpr (MODE == RANKS) {
                const int b = node >= 0 ? A.tptr[qi] : 0, m = node >= 0 ? A.tptr[qi + 1] - b : 0;
                rbase[tid] = b;
                rm[tid] = m;
                thr[tid] = m > 0 ? (u64)A.tord[b] : 0ull;
            }
        }
    }

    int tsel = -1;                                              // TERMS: the lane's diagonal element and its pair's row [K]
    size_t tcell = 0;
    if constexpr (MODE == TERMS) {
        tsel = diagonal_element(wu, wv, li, half);
        const int i = qt * TT + wv * 64 + (tsel >> 4) * 32 + li;
        if (i >= A.T) tsel = -1;
        tcell = (size_t)i * A.K;
    }

    PlaneStage<RTHR, SDC, P> uq, vq;
    static_assert(TT == PLANE_ROWS, "tiles of the plane arrays");
    auto fetch = [&](int s) {
        const int j = s / per_tile, rem = s - j * per_tile;
        const int k = rem / (2 * nd), r = rem - k * 2 * nd;
        const int dc = r < nd ? r : r - nd;
        const __bf16* qsrc = (r < nd ? A.qz : A.qh) + (size_t)k * A.qbatch;
        const __bf16* csrc = (r < nd ? A.cz : A.ch) + (size_t)k * A.cbatch;
        if constexpr (PAIRS) {
            gather_fetch(uq, qsrc, A.trow, qt * TT, A.T, dc, nd, tid);
            gather_fetch(vq, csrc, A.tdst, qt * TT, A.T, dc, nd, tid);
        } else {
            uq.fetch(qsrc + plane_tile<SDC, P>(qt, dc, nd), tid);
            vq.fetch(csrc + plane_tile<SDC, P>(ct0 + j, dc, nd), tid);
        }
    };
    auto stash = [&](int s) {
        uq.stash(us + (s & 1) * P * TT * SLD, tid);
        vq.stash(vs + (s & 1) * P * TT * SLD, tid);
    };

    f32x16 acc[2], term[2];
    float e[2][16];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        zero_acc(acc[b]);
        zero_acc(term[b]);
    }
    if (steps > 0) {
        fetch(0);
        stash(0);
        fetch(min(1, steps - 1));
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int rem = s % per_tile;
        const int r = rem % (2 * nd);
        unsigned char gb = 0;                                   // FILT: group of candidate tid of this tile, on its way to LDS
        if constexpr (FILT) {
            const int v = (ct0 + s / per_tile) * TT + tid;
            if (rem == per_tile - 2 && tid < TT && v < A.N) gb = A.filt.group[v];
        }
        const __bf16* ub = us + (s & 1) * P * TT * SLD + (wu * 32 + li) * SLD + half * 8;
        const __bf16* vb = vs + (s & 1) * P * TT * SLD + (wv * 64 + li) * SLD + half * 8;
#pragma unroll
        for (int kb = 0; kb < SDC / 16; ++kb) {
            gram_block<P>(acc, ub, vb, kb);                     // the dense scorer's products (dl_tiles.h)
            if (kb == 0) {
                if (s + 1 < steps) stash(s + 1);
                fetch(min(s + 2, steps - 1));                   // unconditional: see TileStage (dl_tiles.h)
            }
        }
        if (r == nd - 1) {                                      // S complete: e = exp(S / t)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
                for (int q = 0; q < 16; ++q) e[bb][q] = expf(div_t(acc[bb][q], A.t));
                zero_acc(acc[bb]);
            }
            if constexpr (MODE == TERMS) {
                if (A.te != nullptr && tsel >= 0) A.te[tcell + rem / (2 * nd)] = pick_element(e, tsel);
            }
        } else if (r == 2 * nd - 1) {                           // Q complete: term += Q * e
            if constexpr (MODE == TERMS) {
                if (A.tq != nullptr && tsel >= 0) A.tq[tcell + rem / (2 * nd)] = pick_element(acc, tsel);
            }
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
                for (int q = 0; q < 16; ++q) term[bb][q] += acc[bb][q] * e[bb][q];
                zero_acc(acc[bb]);
            }
            if constexpr (MODE == TERMS) {                      // the running sum: column K - 1 has DIAG's bits
                if (A.tcum != nullptr && tsel >= 0) A.tcum[tcell + rem / (2 * nd)] = pick_element(term, tsel);
            }
        }
        if constexpr (FILT) {
            if (rem == per_tile - 2) {
                if (tid < TT) cgrp[tid] = gb;
            } else if (rem == per_tile - 1) {                   // word tid & 3 of row tid >> 2
                unsigned* fm = MODE == RECON ? reinterpret_cast<unsigned*>(scr) : exm;      // RECON: igm, see above
                fm[tid] = filter_word(fal[rgrp[tid >> 2] & 63], cgrp + (tid & 3) * 32);
            }
        }
        __syncthreads();
        if (rem != per_tile - 1) continue;

        // ---- candidate tile complete: term[bb][q] = s(query row wu*32 + acc_row(q, half), candidate vl = wv*64 + bb*32 + li)
        const int v0 = (ct0 + s / per_tile) * TT;
        if constexpr (MODE == TERMS) {                          // everything was written on the way
        } else if constexpr (MODE == DIAG) {
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int ul = wu * 32 + acc_row(q, half), vl = wv * 64 + bb * 32 + li;
                    const int i = qt * TT + ul;
                    if (ul == vl && i < A.T) A.tlogit[i] = term[bb][q];
                }
            }
        } else if constexpr (MODE == RECON) {
            float* lg = P == 3 ? reinterpret_cast<float*>((wave < 4 ? us : vs) + (s & 1) * 3 * TT * SLD) + (wave & 3) * (3 * TT * SLD / 8)
                               : lgs + wave * RLG;              // one plane: the wave's own RLG floats behind the images
            recon_epilogue<LOGIT, FILT>(A, term, lg, exm, reinterpret_cast<unsigned*>(scr), excur, cnt, rnode, qt, ct0 + s / per_tile, nt, tid);
        } else {
            if (tid < TT) {                                     // this tile's excluded columns of row tid
                const int node = rnode[tid];
                unsigned* m = exm + tid * 4;
                if constexpr (!FILT) m[0] = m[1] = m[2] = m[3] = 0u;
                if (node >= 0 && A.ex_rowptr != nullptr) {
                    int c = excur[tid];
                    const int end = A.ex_rowptr[node + 1];
                    for (; c < end; ++c) {
                        const int col = A.ex_col[c] - v0;
                        if (col >= TT) break;
                        m[col >> 5] |= 1u << (col & 31);
                    }
                    excur[tid] = c;
                }
                if (node >= 0 && A.exclude_self && node >= v0 && node < v0 + TT) m[(node - v0) >> 5] |= 1u << ((node - v0) & 31);
            }
            __syncthreads();
            // The logits go through LDS, one lane's own 16 values per round (no exchange between lanes), so that the
            // candidate loop below need not be unrolled over the registers: into the staging image this step has finished
            // reading (the next write to it is the stash in step s + 1, behind the barriers at the end of this epilogue).
            float* lg = P == 3 ? reinterpret_cast<float*>((wave < 4 ? us : vs) + (s & 1) * 3 * TT * SLD) + (wave & 3) * 16 * DL_WAVE
                               : lgs + wave * LG_WAVE;          // one plane: the wave's own 4 KiB behind the images
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const int vl = wv * 64 + bb * 32 + li, v = v0 + vl;
#pragma unroll
                for (int q = 0; q < 16; ++q) lg[q * DL_WAVE + lane] = term[bb][q];
#pragma unroll 1
                for (int q = 0; q < 16; ++q) {
                    const int row = wu * 32 + acc_row(q, half);
                    const bool ok = rnode[row] >= 0 && v < A.N && !((exm[row * 4 + (vl >> 5)] >> (vl & 31)) & 1u);
                    if (!ok) continue;
                    const int qi = qt * TT + row;
                    const float x = lg[q * DL_WAVE + lane];
                    if constexpr (MODE == TOPK) {
                        const u64 key = make_key(x, v);
                        if (key > thr[row]) {
                            const int slot = atomicAdd(&cnt[row], 1);
                            A.lists[((size_t)qi * A.slices + sl) * A.cap + slot] = key;
                        }
                    } else {
                        const unsigned o = ord_key(x);
                        const int m = rm[row];
                        if (m > 0 && (u64)o >= thr[row]) {      // reaches the row's smallest target
                            const unsigned* to = A.tord + rbase[row];
                            int lo = 0, hi = m;                 // targets below o: [0, lo)
                            while (lo < hi) {
                                const int mid = (lo + hi) >> 1;
                                if (to[mid] < o) lo = mid + 1; else hi = mid;
                            }
                            int lo2 = lo, hi2 = m;              // equal to o: [lo, lo2)
                            while (lo2 < hi2) {
                                const int mid = (lo2 + hi2) >> 1;
                                if (to[mid] <= o) lo2 = mid + 1; else hi2 = mid;
                            }
                            if (lo > 0) atomicAdd(&A.gcnt[rbase[row] + qi + lo], 1ull);
                            if (lo2 > lo) atomicAdd(&A.tcnt[rbase[row] + lo], 1ull);
                        }
                    }
                }
                if constexpr (MODE == TOPK) {                   // lists that could overflow in the next round
                    __syncthreads();
                    for (int row = wave; row < TT; row += 8) {
                        const int n = cnt[row];
                        if (n > A.cap - ROUND)
                            compact_row(A.lists + ((size_t)(qt * TT + row) * A.slices + sl) * A.cap, scr + wave * MAX_CAP, n,
                                        srt[row], A.k, lane, &thr[row], &cnt[row], &srt[row]);
                    }
                    __syncthreads();
                }
            }
            if constexpr (MODE == RANKS) __syncthreads();
        }
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) zero_acc(term[bb]);
    }
    if constexpr (MODE == TOPK) {                               // every list of the work item sorted and truncated to k
        __syncthreads();
        for (int row = wave; row < TT; row += 8) {
            const int qi = qt * TT + row;
            if (qi >= A.Q) continue;
            const int n = cnt[row];
            if (n > srt[row])
                compact_row(A.lists + ((size_t)qi * A.slices + sl) * A.cap, scr + wave * MAX_CAP, n, srt[row], A.k, lane,
                            &thr[row], &cnt[row], &srt[row]);
            if (lane == 0) A.counts[(size_t)qi * A.slices + sl] = min(n, A.k);
        }
    }
}

// One workgroup per query row: the slices' sorted lists are merged by rank (position in its own list + keys above it in
// every other list, by binary search); ranks are unique (keys are), so every output slot is written once.
__global__ __launch_bounds__(256) void topk_merge_kernel(const u64* __restrict__ lists, const int* __restrict__ counts,
                                                         int slices, int cap, int k, int64_t* __restrict__ index,
                                                         float* __restrict__ logit, float* __restrict__ prob) {
    __shared__ u64 sm[MAX_SLICES * MAX_K];
    __shared__ int off[MAX_SLICES + 1];
    const int qi = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int o = 0;
        for (int s = 0; s < slices; ++s) {
            off[s] = o;
            o += counts[(size_t)qi * slices + s];
        }
        off[slices] = o;
    }
    __syncthreads();
    for (int s = 0; s < slices; ++s) {
        const int n = off[s + 1] - off[s];
        const u64* L = lists + ((size_t)qi * slices + s) * cap;
        for (int i = tid; i < n; i += 256) sm[off[s] + i] = L[i];
    }
    __syncthreads();
    const int total = off[slices];
    for (int e = tid; e < total; e += 256) {
        const u64 x = sm[e];
        int rank = 0;
        for (int s = 0; s < slices; ++s) {
            const int b = off[s], n = off[s + 1] - b;
            if (e >= b && e < b + n) {
                rank += e - b;
                continue;
            }
            int lo = 0, hi = n;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sm[b + mid] > x) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            const float val = ord_value((unsigned)(x >> 32));
            const size_t o = (size_t)qi * k + rank;
            index[o] = (int64_t)(0xFFFFFFFFu - (unsigned)x);
            logit[o] = val;
            prob[o] = sigmoid_ref(val);
        }
    }
    for (int r = total + tid; r < k; r += 256) {                // fewer than k candidates: padding
        const size_t o = (size_t)qi * k + r;
        index[o] = -1;
        logit[o] = __uint_as_float(0x7FC00000u);
        prob[o] = __uint_as_float(0x7FC00000u);
    }
}

__global__ void gather_rows_kernel(const float* __restrict__ Z, const float* __restrict__ H, const int32_t* __restrict__ rows,
                                   int Q, int w, float* __restrict__ zq, float* __restrict__ hq) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)Q * w) return;
    const size_t r = g / w, c = g % w;
    const size_t src = (size_t)rows[r] * w + c;
    zq[g] = Z[src];
    hq[g] = H[src];
}

// per target: its query row, from the CSR of targets by query
__global__ void target_rows_kernel(const int32_t* __restrict__ tptr, int Q, int32_t* __restrict__ trow) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    for (int i = tptr[q]; i < tptr[q + 1]; ++i) trow[i] = q;
}

// sort each row's target logits (ascending by value order; rows are short): position and first position of its value
__global__ void target_sort_kernel(const int32_t* __restrict__ tptr, const int32_t* __restrict__ trow, const float* __restrict__ tlogit,
                                   int T, unsigned* __restrict__ tord, int32_t* __restrict__ spos, int32_t* __restrict__ sfirst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const int q = trow[i], b = tptr[q], e = tptr[q + 1];
    const unsigned o = ord_key(tlogit[i]);
    int lt = 0, pos = 0;
    for (int j = b; j < e; ++j) {
        const unsigned oj = ord_key(tlogit[j]);
        lt += oj < o ? 1 : 0;
        pos += (oj < o || (oj == o && j < i)) ? 1 : 0;
    }
    tord[b + pos] = o;
    spos[i] = pos;
    sfirst[i] = lt;
}

__global__ void target_finish_kernel(const int32_t* __restrict__ tptr, const int32_t* __restrict__ trow, const int32_t* __restrict__ tdst,
                                     const int32_t* __restrict__ qnode, const int32_t* __restrict__ spos, const int32_t* __restrict__ sfirst,
                                     const u64* __restrict__ gcnt, const u64* __restrict__ tcnt, const int32_t* __restrict__ ex_rowptr,
                                     const int32_t* __restrict__ ex_col, int T, int64_t* __restrict__ greater, int64_t* __restrict__ ties) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const int q = trow[i], b = tptr[q], m = tptr[q + 1] - b;
    u64 g = 0;
    for (int p = spos[i] + 1; p <= m; ++p) g += gcnt[b + q + p];
    u64 tie = tcnt[b + sfirst[i]];
    const int node = qnode[q], v = tdst[i];
    bool counted = v != node;                                   // the scan counted the target itself among the ties
    if (counted && ex_rowptr != nullptr) {
        const int lo = first_col_at_least(ex_col, ex_rowptr[node], ex_rowptr[node + 1], v);
        counted = !(lo < ex_rowptr[node + 1] && ex_col[lo] == v);
    }
    greater[i] = (int64_t)g;
    ties[i] = (int64_t)tie - (counted ? 1 : 0);
}

// Under a node-group rule the scan counted a target itself only where the rule allows it: behind target_finish_kernel, give
// a target the rule does not allow the 1 back that was taken from its ties.
__global__ void target_unallowed_kernel(const int32_t* __restrict__ trow, const int32_t* __restrict__ tdst,
                                        const int32_t* __restrict__ qnode, const int32_t* __restrict__ ex_rowptr,
                                        const int32_t* __restrict__ ex_col, int T, FilterArgs filt, int64_t* __restrict__ ties) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const int node = qnode[trow[i]], v = tdst[i];
    if (v == node || ((filt.allow[filt.group[node]] >> (filt.group[v] & 63)) & 1ull)) return;
    if (ex_rowptr != nullptr) {
        const int lo = first_col_at_least(ex_col, ex_rowptr[node], ex_rowptr[node + 1], v);
        if (lo < ex_rowptr[node + 1] && ex_col[lo] == v) return;       // excluded: nothing was taken
    }
    ties[i] += 1;
}

}  // namespace rank

using namespace rank;

bool score_rank_supported(int K, int d) { return K >= 1 && K <= DL_MAX_FACTORS && d >= 1 && d <= 128; }

// Slicing of the candidate tiles: as many slices as keep one work item per CU busy (one workgroup per CU fits the LDS),
// at most MAX_SLICES, never an empty slice.  DL_RANK_SLICES (test knob) forces the count; results do not depend on it.
struct RankPlan { int nd, qtiles, nt, slices, tps, cap; size_t qbatch, cbatch; dl_dtype dt; };
static RankPlan rank_plan(int N, int d, int Q, int k, dl_dtype dt = DL_F32) {
    RankPlan p;
    p.nd = (d + SDC - 1) / SDC;
    p.qtiles = (Q + TT - 1) / TT;
    p.nt = (N + TT - 1) / TT;
    const int want = config().rank_slices > 0 ? config().rank_slices : device_cus() / max(1, p.qtiles);
    const int s = max(1, min(min(want, MAX_SLICES), p.nt));
    p.tps = (p.nt + s - 1) / s;
    p.slices = (p.nt + p.tps - 1) / p.tps;
    p.cap = k + ROUND;
    p.qbatch = table_plane_elems(dt, Q, d);                    // only the plane arrays depend on the table type
    p.cbatch = table_plane_elems(dt, N, d);
    p.dt = dt;
    return p;
}

// out = nd, qtiles, slices, tiles per slice, tiles of the last slice, cap: rank_plan under the current configuration
void score_topk_form(int N, int d, int Q, int k, int* out) {
    const RankPlan p = rank_plan(N, d, Q, k);
    out[0] = p.nd;
    out[1] = p.qtiles;
    out[2] = p.slices;
    out[3] = p.tps;
    out[4] = p.nt - (p.slices - 1) * p.tps;
    out[5] = p.cap;
}

// Workspace (256-byte aligned blocks): gathered query rows (fp32 tables only: bf16 rows are gathered by the copy into their
// plane) | their planes | planes of Z and H | TOPK: lists, counts | RANKS: per-target arrays and the two counter arrays.
struct RankWs {
    float *zq, *hq, *tlogit;
    __bf16 *qz, *qh, *cz, *ch;
    u64 *lists, *gcnt, *tcnt;
    int *counts;
    int32_t *trow, *spos, *sfirst;
    unsigned* tord;
    size_t bytes;
};
static RankWs rank_carve(const RankPlan& p, int Q, int K, int d, int k, int T, void* ws) {
    RankWs w = {};
    Carver c(ws);
    if (p.dt == DL_F32) {
        w.zq = c.take<float>((size_t)Q * K * d);
        w.hq = c.take<float>((size_t)Q * K * d);
    }
    w.qz = c.take<__bf16>((size_t)K * p.qbatch);
    w.qh = c.take<__bf16>((size_t)K * p.qbatch);
    w.cz = c.take<__bf16>((size_t)K * p.cbatch);
    w.ch = c.take<__bf16>((size_t)K * p.cbatch);
    if (k > 0) {
        w.lists = c.take<u64>((size_t)Q * p.slices * p.cap);
        w.counts = c.take<int>((size_t)Q * p.slices);
    }
    if (T > 0) {
        w.trow = c.take<int32_t>((size_t)T);
        w.spos = c.take<int32_t>((size_t)T);
        w.sfirst = c.take<int32_t>((size_t)T);
        w.tlogit = c.take<float>((size_t)T);
        w.tord = c.take<unsigned>((size_t)T);
        w.gcnt = c.take<u64>((size_t)T + Q);
        w.tcnt = c.take<u64>((size_t)T);
    }
    w.bytes = c.bytes();
    return w;
}

size_t score_rank_workspace_bytes(int N, int K, int d, int Q, int k, int T, dl_dtype dt) {
    return rank_carve(rank_plan(N, d, Q, k, dt), Q, K, d, k, T, nullptr).bytes;
}

// the query rows gathered and split, the candidate tables split: the scan's operands
static ScanArgs scan_operands(const RankPlan& p, const RankWs& w, const void* Z, const void* H, int N, int K, int d, float t,
                              const int32_t* queries, int Q, const int32_t* exr, const int32_t* exc, hipStream_t st) {
    if (p.dt == DL_BF16) {                                      // the gather is part of the copy into the plane
        table_planes(Z, p.dt, queries, Q, K, d, w.qz, st);
        table_planes(H, p.dt, queries, Q, K, d, w.qh, st);
    } else {
        const size_t n = (size_t)Q * K * d;
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)Z, (const float*)H,
                           queries, Q, K * d, w.zq, w.hq);
        split_rows(w.zq, K, Q, d, K * d, (size_t)d, w.qz, st);
        split_rows(w.hq, K, Q, d, K * d, (size_t)d, w.qh, st);
    }
    table_planes(Z, p.dt, nullptr, N, K, d, w.cz, st);
    table_planes(H, p.dt, nullptr, N, K, d, w.ch, st);
    ScanArgs a = {};
    a.qz = w.qz; a.qh = w.qh; a.qbatch = p.qbatch;
    a.cz = w.cz; a.ch = w.ch; a.cbatch = p.cbatch;
    a.Q = Q; a.N = N; a.K = K; a.nd = p.nd; a.t = t;
    a.qnode = queries;
    a.ex_rowptr = exr; a.ex_col = exc;
    a.slices = p.slices; a.tiles_per_slice = p.tps;
    return a;
}

// the scan in its three-plane or one-plane instantiation (FILT where there is a rule and the mode has one)
template <int MODE>
static void launch_rank(dl_dtype dt, const dl_node_filter* nf, unsigned grid, hipStream_t st, const ScanArgs& a) {
    if constexpr (MODE == DIAG) {
        if (dt == DL_BF16) launch_lds<rank_scan_kernel<DIAG, false, 1>>(grid, RTHR, lds_bytes(1), st, a);
        else launch_lds<rank_scan_kernel<DIAG>>(grid, RTHR, lds_bytes(3), st, a);
    } else {
        if (dt == DL_BF16)
            launch_scan<rank_scan_kernel<MODE, false, 1>, rank_scan_kernel<MODE, true, 1>>(nf, grid, RTHR, lds_bytes(1), st, a);
        else
            launch_scan<rank_scan_kernel<MODE>, rank_scan_kernel<MODE, true>>(nf, grid, RTHR, lds_bytes(3), st, a);
    }
}

int score_topk(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* queries, int Q, int k,
               const int32_t* exr, const int32_t* exc, int exclude_self, int64_t* index, float* logit, float* prob, void* ws,
               hipStream_t st, const dl_node_filter* nf) {
    const RankPlan p = rank_plan(N, d, Q, k, dt);
    const RankWs w = rank_carve(p, Q, K, d, k, 0, ws);
    ScanArgs a = scan_operands(p, w, Z, H, N, K, d, t, queries, Q, exr, exc, st);
    a.exclude_self = exclude_self ? 1 : 0;
    a.k = k; a.cap = p.cap; a.lists = w.lists; a.counts = w.counts;
    a.filt = filter_args(nf);
    launch_rank<TOPK>(dt, nf, (unsigned)xcd_grid(p.qtiles, p.slices), st, a);
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)Q), dim3(256), 0, st, w.lists, w.counts, p.slices, p.cap, k, index,
                       logit, prob);
    return check_launch("score_topk");
}

int score_ranks(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* queries, int Q,
                const int32_t* tptr, const int32_t* tdst, int T, const int32_t* exr, const int32_t* exc, int64_t* greater, int64_t* ties,
                void* ws, hipStream_t st, const dl_node_filter* nf) {
    const RankPlan p = rank_plan(N, d, Q, 0, dt);
    const RankWs w = rank_carve(p, Q, K, d, 0, T, ws);
    ScanArgs a = scan_operands(p, w, Z, H, N, K, d, t, queries, Q, exr, exc, st);
    hipLaunchKernelGGL(target_rows_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, tptr, Q, w.trow);
    // the targets' own logits, from the scan's arithmetic with the query as the A operand: tile i of the targets against
    // itself, the diagonal kept
    ScanArgs g = a;
    g.trow = w.trow; g.tdst = tdst; g.T = T; g.tlogit = w.tlogit;
    launch_rank<DIAG>(dt, nullptr, (unsigned)xcd_grid((T + TT - 1) / TT, 1), st, g);
    const unsigned tb = (unsigned)((T + 255) / 256);
    hipLaunchKernelGGL(target_sort_kernel, dim3(tb), dim3(256), 0, st, tptr, w.trow, w.tlogit, T, w.tord, w.spos, w.sfirst);
    hipError_t e = hipMemsetAsync(w.gcnt, 0, sizeof(u64) * ((size_t)T + Q), st);
    if (e == hipSuccess) e = hipMemsetAsync(w.tcnt, 0, sizeof(u64) * (size_t)T, st);
    DL_REQUIRE(e == hipSuccess, "hipMemsetAsync: %s", hipGetErrorString(e));
    a.exclude_self = 1;
    a.tptr = tptr; a.tord = w.tord; a.gcnt = w.gcnt; a.tcnt = w.tcnt;
    a.filt = filter_args(nf);
    launch_rank<RANKS>(dt, nf, (unsigned)xcd_grid(p.qtiles, p.slices), st, a);
    hipLaunchKernelGGL(target_finish_kernel, dim3(tb), dim3(256), 0, st, tptr, w.trow, tdst, queries, w.spos, w.sfirst, w.gcnt,
                       w.tcnt, exr, exc, T, greater, ties);
    if (nf != nullptr)
        hipLaunchKernelGGL(target_unallowed_kernel, dim3(tb), dim3(256), 0, st, w.trow, tdst, queries, exr, exc, T, a.filt, ties);
    return check_launch("score_ranks");
}

// ---- the RECON scan of one strip of rows (dl_score_recon.hip drives it): rows [q0, q0 + rows) of the graph, q0 a multiple of
// 128, as the query tiles — read where they stand in the plane arrays of Z and H, which are the candidates too — against all
// candidate tiles.  ghat: rows x Np floats and the cells [rows rounded up to 128][Np / 128], all of it written.
// dt: the planes are three per operand (DL_F32, split_rows) or the one of a bf16 table (DL_BF16, copy_rows): the P = 1 form.
// nf (NULL: none): a symmetric node-group rule; a pair it denies is ignored (the RECON x FILT instantiations).
void score_recon_strip(const __bf16* cz, const __bf16* ch, dl_dtype dt, int N, int K, int d, float t, int q0, int rows,
                       const int32_t* pos_rowptr, const int32_t* pos_col, const int32_t* ig_rowptr, const int32_t* ig_col, float w_pos,
                       float w_neg, bool logit, const dl_node_filter* nf, float* ghat, float* lcell, unsigned* ccell, hipStream_t st) {
    const RankPlan p = rank_plan(N, d, rows, 0, dt);
    ReconArgs a = {};
    const size_t first = dt == DL_BF16 ? plane_tile<SDC, 1>(q0 / TT, 0, p.nd) : plane_tile<SDC, 3>(q0 / TT, 0, p.nd);
    a.qz = cz + first; a.qh = ch + first; a.qbatch = p.cbatch;
    a.cz = cz; a.ch = ch; a.cbatch = p.cbatch;
    a.Q = rows; a.N = N; a.K = K; a.nd = p.nd; a.t = t;
    a.ex_rowptr = pos_rowptr; a.ex_col = pos_col;
    a.slices = p.slices; a.tiles_per_slice = p.tps;
    a.q0 = q0;
    a.ig_rowptr = ig_rowptr; a.ig_col = ig_col;
    a.w_pos = w_pos; a.w_neg = w_neg;
    a.ghat = ghat; a.lcell = lcell; a.ccell = ccell;
    a.filt = filter_args(nf);
    const unsigned grid = (unsigned)xcd_grid(p.qtiles, p.slices);
    if (logit) {                                               // the same LDS: the epilogue keeps nothing more there
        if (dt == DL_BF16)
            launch_scan<rank_scan_kernel<RECON, false, 1, true>, rank_scan_kernel<RECON, true, 1, true>>(nf, grid, RTHR, lds_bytes(1, true), st, a);
        else
            launch_scan<rank_scan_kernel<RECON, false, 3, true>, rank_scan_kernel<RECON, true, 3, true>>(nf, grid, RTHR, lds_bytes(3), st, a);
    } else if (dt == DL_BF16) {
        launch_scan<rank_scan_kernel<RECON, false, 1>, rank_scan_kernel<RECON, true, 1>>(nf, grid, RTHR, lds_bytes(1, true), st, a);
    } else {
        launch_scan<rank_scan_kernel<RECON>, rank_scan_kernel<RECON, true>>(nf, grid, RTHR, lds_bytes(3), st, a);
    }
}

// ---- dl_score_pair_logits: the DIAG pass on its own, with the plane arrays of Z and H as BOTH sides: pair i = (row a[i] as
// the A operand, row b[i]), tile i of the pairs against itself, the diagonal kept.  Workspace: planes of Z and H.
struct PairWs { __bf16 *cz, *ch; size_t cbatch, bytes; };
static PairWs pair_carve(int N, int K, int d, dl_dtype dt, void* ws) {
    PairWs w = {};
    w.cbatch = table_plane_elems(dt, N, d);
    Carver c(ws);
    w.cz = c.take<__bf16>((size_t)K * w.cbatch);
    w.ch = c.take<__bf16>((size_t)K * w.cbatch);
    w.bytes = c.bytes();
    return w;
}

size_t score_pair_logits_workspace_bytes(int N, int K, int d, dl_dtype dt) { return pair_carve(N, K, d, dt, nullptr).bytes; }

// the tables split into the workspace, and the pass's operands and pairs; what the pass writes is its caller's
static ScanArgs pair_operands(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* a, const int32_t* b,
                              int T, void* ws, hipStream_t st) {
    const PairWs w = pair_carve(N, K, d, dt, ws);
    table_planes(Z, dt, nullptr, N, K, d, w.cz, st);
    table_planes(H, dt, nullptr, N, K, d, w.ch, st);
    ScanArgs g = {};
    g.qz = w.cz; g.qh = w.ch; g.qbatch = w.cbatch;
    g.cz = w.cz; g.ch = w.ch; g.cbatch = w.cbatch;
    g.N = N; g.K = K; g.nd = (d + SDC - 1) / SDC; g.t = t;
    g.trow = a; g.tdst = b; g.T = T;
    return g;
}

int score_pair_logits(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* a, const int32_t* b,
                      int T, float* logit, void* ws, hipStream_t st) {
    ScanArgs g = pair_operands(Z, H, dt, N, K, d, t, a, b, T, ws, st);
    g.tlogit = logit;
    launch_rank<DIAG>(dt, nullptr, (unsigned)xcd_grid((T + TT - 1) / TT, 1), st, g);
    return check_launch("score_pair_logits");
}

// ---- dl_score_pair_terms: the same pass in its TERMS instantiation, which writes what the pass holds per factor (e, q, the
// running sum) for the pair on the diagonal instead of the final sum alone.  Same workspace, same operands, same products.
int score_pair_terms(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* a, const int32_t* b,
                     int T, float* e, float* q, float* cum, void* ws, hipStream_t st) {
    ScanArgs g = pair_operands(Z, H, dt, N, K, d, t, a, b, T, ws, st);
    g.te = e; g.tq = q; g.tcum = cum;
    const unsigned grid = (unsigned)xcd_grid((T + TT - 1) / TT, 1);
    if (dt == DL_BF16) launch_lds<rank_scan_kernel<TERMS, false, 1>>(grid, RTHR, lds_bytes(1), st, g);
    else launch_lds<rank_scan_kernel<TERMS>>(grid, RTHR, lds_bytes(3), st, g);
    return check_launch("score_pair_terms");
}

}  // namespace dl
