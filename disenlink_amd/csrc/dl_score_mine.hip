// Mining of the graph's m most likely missing links (dl_score_mine): an exact, deterministic global top-m over the logits
//   s(u, v) = sum_k (h_k[u].h_k[v]) * exp(z_k[u].z_k[v] / t)
// of all unordered pairs u < v, with nothing of size N x N in memory.
//
// Scan: the tile loop of the ranking scan (dl_score_rank.hip) over the tile pairs (u tile <= v tile) of the dense scorer: one
// workgroup = 8 waves = a run of consecutive tile pairs in row-major order, per pair the Gram products of gram_block_split6
// (dl_tiles.h) from the plane arrays of Z and H (split_rows), the rows of the SMALLER endpoint as the A operand — the bits
// dl_score_topk forms for query u, candidate v.  A candidate is a pair u < v < N outside the exclusion CSR (a 128-bit
// mask per u row and tile, as in the ranking scan) whose logit reaches the floor; NaN reaches no floor.
//
// Selection: a radix select over the 64-bit key  (order key of the logit) << 32 | ~(u N + v)  (keys are distinct; a larger
// key ranks first).  Up to six HISTOGRAM scans, one per digit (11, 11, 10 bits of the value, then of the index), count the
// candidates whose higher digits equal the threshold's so far (LDS-private bins, flushed with integer atomics); a
// one-workgroup kernel picks the digit in which the m-th best key lies.  As soon as the keys with the chosen prefix are
// exactly the ones still needed (always, once the prefix holds a single key), a device flag ends the search: the
// remaining histogram scans return at workgroup start.  One EMIT scan appends every candidate at or above the threshold to
// a key array (exactly count = min(m, candidates) of them, in arbitrary order), and a rank-by-counting kernel puts them
// in order and writes the outputs and the padding.
// EVERY scan recomputes the logits with the same instruction stream (scan_tiles below, one body for all modes), and the
// logit of a pair does not depend on where in a tile its rows sit or on which workgroup forms it: the keys are the same
// bits in every scan, which is what makes the histograms, the threshold and the emitted set consistent.  Nothing is keyed
// on a float sum or on an arrival order, so the outputs are the same bits on every call and under every geometry.
//
// Counting (dl_score_pair_ranks, mode COUNT of the same body): where T given target pairs stand among ALL candidates.  The
// caller passes the targets' order keys in ascending order; every candidate (NaN logits included, no floor) finds lo = the
// number of target keys strictly below its own — a table of <= SEPS separators in LDS (every stride-th key), then a binary
// search among the <= stride keys between two separators in global memory — and adds 1 to the 64-bit difference array
// gcnt[lo] and, if the key at lo equals its own, to tcnt[lo]; candidates below the smallest key add nothing, those above the
// largest are summed per lane and added once per wave, and a wave whose lanes all found the same place adds once.  ncand
// receives the number of candidates.  Suffix sums and the correction for the target itself are the caller's (ops.py).
//
// Link graph (dl_score_links_count / dl_score_links_fill, modes DEG and FILL of the same body): EVERY candidate at or above
// the floor, however many, as a symmetric CSR with ascending columns, with no atomics and no arrival order on the output
// path.  When a tile pair (qt, ct) completes, the waves form its 128 x 128 pass mask with ballots, row-major and
// column-major (2 KB each, where the bins are in the other modes).  DEG: the row threads write popc of the rows to cell
// (u, ct) of cnt [N][nt] and popc of the columns to cell (v, qt); on a diagonal pair both sides of a node are one cell, the
// smaller neighbours first.  Every cell is written exactly once, by the workgroup that forms its tile pair, zeros included:
// nothing is cleared beforehand and nothing is added.  Offsets: a wave per node turns its cells into their exclusive
// prefix, and one workgroup scans the degrees into rowptr (64-bit).  FILL: the same scan and the same masks again; every
// value that passed goes to slot rowptr[u] + cnt[u][ct] + (passed columns of its row below v), and likewise for (v, u);
// a slot >= the caller's nnz is not written.  The walk of the tile pairs and its cap N <= 46,340 are the mining's.
//
// Budgeted link graph (dl_score_links_top_count / _fill, modes DEG_TOP and FILL_TOP): the m best candidates, ANY m, as that
// CSR.  The radix select above runs unchanged (its counts are 32-bit and the candidates number < 2^32, so it finds the m-th
// key for every m; only EMIT and the ordering need m <= 65,536, and neither runs) and leaves the threshold key in
// State::prefix; the link modes then pass a pair only if its 64-bit key also reaches that threshold.  Keys are distinct, so
// exactly min(m, candidates) pairs pass: the set dl_score_mine would list without its cap, a class of tied logits cut where
// it cuts it (smaller u N + v first).  Nothing is read back between the select and the count.
//
// Two node sets (dl_score_mine_between, dl_score_links_between_count / _fill; the modes HIST_RECT, EMIT_RECT, DEG_RECT,
// FILL_RECT): rows of a table A against rows of a table B, every tile pair of the ntA x ntB grid, the pair index a nB + b
// local to the rectangle (nA, nB <= 46,340).  The select, the ordering, the offsets and the epilogues are the ones above;
// there is no u < v and no diagonal, and the link modes keep cells and a CSR per side.  A graph of any size is the union of
// its diagonal blocks (the entries above, on row slices) and of such rectangles; the caller merges them (scans.py).
//
// Node groups (the FILT instantiations; dl_score_mine_filtered, dl_score_pair_ranks_filtered): a symmetric rule on the groups
// of u and v, formed into the row mask ahead of the exclusion; a candidate passes both.  The epilogues do not change.
//
// bf16 tables (the *_dtype entries with DL_BF16; the P = 1 instantiations): the table is its own single plane (copy_rows), a
// step stages one plane per operand and issues one product per block (gram_block<1>).  On the same values the logits are the
// bits of the three-plane scan (dl_tiles.h), so everything above holds unchanged; only the plane arrays of the workspace shrink.
//
// Host side (behind namespace mine): every entry is made of the same parts — the Plan of the tile walk (a triangle is the
// rectangle whose B is A; the run length and DL_MINE_TILES live there), carve (the workspace as the select's blocks, the planes
// and the link cells, in that order), split_tables, scan_args (either kind of rule), launch<MODE> (RECT, P and FILT from the
// plan), select (the histogram rounds) and link_offsets (cells, then rowptr, per side).  A new mode adds its epilogue and its
// part of ScanArgs on the device side, and on the host side a driver that names its passes.
#include <cstddef>
#include "dl_common.h"
#include "dl_config.h"
#include "dl_kernels.h"
#include "dl_scan.h"

namespace dl {
namespace mine {

using namespace scan;         // the step arithmetic, keys, exclusion walk and host scaffolding of the scans

constexpr int TT = 128;
constexpr int MTHR = 512;
constexpr int SDC = SPLIT_COLS, SLD = SPLIT_PITCH;
constexpr int BINS = 2048;                 // the widest digit
constexpr int PASSES = 6;
constexpr int MAX_M = 65536;
enum { HIST = 0, EMIT = 1, COUNT = 2, DEG = 3, FILL = 4, DEG_TOP = 5, FILL_TOP = 6,      // *_TOP: DEG / FILL under the selected key
       HIST_RECT = 7, EMIT_RECT = 8, DEG_RECT = 9, FILL_RECT = 10 };                     // *_RECT: rows of A against rows of B
constexpr int rect_mode(int mode) { return mode == HIST ? HIST_RECT : mode == EMIT ? EMIT_RECT : mode == DEG ? DEG_RECT : FILL_RECT; }
constexpr int base_mode(int mode) { return mode == HIST_RECT ? HIST : mode == EMIT_RECT ? EMIT : mode == DEG_RECT ? DEG : mode == FILL_RECT ? FILL : mode; }
constexpr int SEPS = 4096;                 // COUNT: first-level separators of the sorted targets, in LDS

// the digits of the key, from the top: value 11 + 11 + 10 bits, index 11 + 11 + 10 bits
__host__ __device__ inline int digit_shift(int p) { return p == 0 ? 53 : p == 1 ? 42 : p == 2 ? 32 : p == 3 ? 21 : p == 4 ? 10 : 0; }
__host__ __device__ inline int digit_bits(int p) { return (p == 2 || p == 5) ? 10 : 11; }

// Selection state in the workspace (device memory; the library's host code never reads it)
struct State {
    u64 prefix;            // the threshold key's digits chosen so far, lower bits zero
    unsigned need;         // keys still to take among those with this prefix
    unsigned done;         // 1: prefix is the final threshold
    unsigned count;        // min(m, candidates), once done
    unsigned emitted;      // EMIT: keys appended
    unsigned scans;        // scans that ran (a measurement: tools/mine_time.py)
    unsigned pad;
};

// One kernel argument: what every scan reads, then what one family of modes reads
struct SelectArgs {                            // HIST / EMIT (dl_score_mine)
    int m, pass;                               // pass: HIST's digit
    unsigned* hist;  u64* keys;
};
struct CountArgs {                             // COUNT (dl_score_pair_ranks): the ascending order keys of the T targets, every
    const unsigned* tord;                      // stride-th of them a separator, and the 64-bit counters: gcnt [T+1] (difference
    int T, stride, nsep;                       // array of "greater"), tcnt [T+1] (equal range, at its first place), ncand [1]
    u64 *gcnt, *tcnt, *ncand;
};
struct LinkArgs {                              // DEG / FILL (dl_score_links): cnt [N][nt], the eligible pairs of node r with
    unsigned* cnt;                             // partners in tile t (DEG writes the counts, the offsets kernel turns each row into
    const int64_t* rowptr;  long long nnz;     // its exclusive prefix, FILL reads that), and FILL's CSR (slots >= nnz are skipped)
    int32_t* col;  float *logit, *prob;
};
struct RectArgs {                              // RECT (dl_score_*_between): the v side is a table B of its own — its planes, rows
    const __bf16 *cz, *ch;  size_t cbatch;     // and tiles, the groups of its rows (FILT), and the cells and the CSR of its side
    int N, nt;                                 // (DEG / FILL: cnt [nB][ntA], columns = rows of A)
    const unsigned char* group;
    LinkArgs link;
};
struct ScanArgs {
    const __bf16 *cz, *ch;  size_t cbatch;     // planes of Z and H
    int N, K, nd, nt;  float t;
    const int32_t *ex_rowptr, *ex_col;
    float min_logit;                           // the floor (COUNT has none)
    int pairs, per_wg;                         // tile pairs, tile pairs per workgroup
    FilterArgs filt;                           // FILT: the node-group rule (dl_tiles.h); symmetric, so the u row decides
    State* state;                              // HIST / EMIT / COUNT: the selection state and the count of scans; DEG / FILL: none;
                                               // DEG_TOP / FILL_TOP: the state the select left (prefix = the threshold key)
    SelectArgs sel;
    CountArgs cnt;
    LinkArgs link;
    RectArgs rect;                             // last: the offsets of everything above are those of the triangular scans
};

// LDS of an instantiation with P planes per operand: the two double-buffered images, the exclusion mask, the mode's table
constexpr size_t lds_bytes(int mode, int P) { return (size_t)2 * 2 * P * TT * SLD * 2 + TT * 4 * 4 + (mode == COUNT ? SEPS : BINS) * 4; }
static_assert(lds_bytes(HIST, 3) % 16 == 0 && lds_bytes(COUNT, 3) % 16 == 0 && lds_bytes(HIST, 1) % 16 == 0 &&
              lds_bytes(COUNT, 1) % 16 == 0 && lds_bytes(COUNT, 3) + FILTER_LDS_BYTES <= 160 * 1024, "LDS of a CU");

__device__ __forceinline__ u64 wave_sum(u64 x) {
#pragma unroll
    for (int o = DL_WAVE / 2; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)x, o, DL_WAVE), hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), o, DL_WAVE);
        x += ((u64)hi << 32) | lo;
    }
    return x;
}

// ---- the epilogues: what a mode does with a complete tile pair.  term[bb][q] = s(u, v) of row L.row(q) and column L.col(bb)
// of the pair's 128 x 128 tile, exm its [128][4] mask of columns a row may not take (exclusion and, FILT, the group rule).
struct Lane {
    int wu, wv, li, half, lane;
    __device__ __forceinline__ int row(int q) const { return wu * 32 + acc_row(q, half); }
    __device__ __forceinline__ int col(int bb) const { return wv * 64 + bb * 32 + li; }
};
struct Tile { int u0, v0, N, nu; };           // first node of the u tile and of the v tile; nodes of the graph (RECT: rows of
                                              // B, which the pair index a nB + b counts in, and nu = rows of A)
template <bool RECT = false>
__device__ __forceinline__ bool eligible(const unsigned* exm, const Tile T, int row, int vl) {
    const bool in = RECT ? T.u0 + row < T.nu : T.u0 + row < T.v0 + vl;      // a rectangle has no u < v and no diagonal
    return in && T.v0 + vl < T.N && !((exm[row * 4 + (vl >> 5)] >> (vl & 31)) & 1u);
}

// HIST: the digit of pass `pass` of the keys that carry the threshold's higher digits, counted in the LDS bins
struct Digit { int shift, hs; unsigned dmask; u64 prefix; };      // hs: bits below the chosen prefix
template <bool RECT = false>
__device__ __forceinline__ void hist_epilogue(const f32x16 (&term)[2], const unsigned* exm, unsigned* bins, const Lane L, const Tile T,
                                              float min_logit, const Digit D) {
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const int vl = L.col(bb);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = L.row(q);
            const float x = term[bb][q];
            bool ok = eligible<RECT>(exm, T, row, vl) && x >= min_logit;
            const u64 key = make_key(x, (unsigned)(T.u0 + row) * (unsigned)T.N + (unsigned)(T.v0 + vl));
            if (D.hs < 64) ok = ok && (key >> D.hs) == (D.prefix >> D.hs);
            const unsigned dg = (unsigned)(key >> D.shift) & D.dmask;
            const u64 act = __ballot(ok);
            if (act != 0ull) {                                  // wave-uniform: logits cluster, so one bin per wave is common
                const int first = __ffsll((long long)act) - 1;
                const unsigned d0 = (unsigned)__shfl((int)dg, first, DL_WAVE);
                if (__ballot(ok && dg == d0) == act) {
                    if (L.lane == first) atomicAdd(&bins[d0], (unsigned)__popcll(act));
                } else if (ok) {
                    atomicAdd(&bins[dg], 1u);
                }
            }
        }
    }
}
__device__ __forceinline__ void hist_flush(const unsigned* bins, unsigned* hist, int tid) {
    __syncthreads();
    for (int i = tid; i < BINS; i += MTHR) {
        const unsigned c = bins[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// EMIT: every candidate at or above the threshold key, appended in arrival order (order_kernel sorts)
template <bool RECT = false>
__device__ __forceinline__ void emit_epilogue(const f32x16 (&term)[2], const unsigned* exm, const Lane L, const Tile T, float min_logit,
                                              u64 threshold, State* state, u64* keys, int m) {
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const int vl = L.col(bb);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = L.row(q);
            const float x = term[bb][q];
            const bool ok = eligible<RECT>(exm, T, row, vl) && x >= min_logit;
            const u64 key = make_key(x, (unsigned)(T.u0 + row) * (unsigned)T.N + (unsigned)(T.v0 + vl));
            if (ok && key >= threshold) {
                const unsigned slot = atomicAdd(&state->emitted, 1u);
                if (slot < (unsigned)m) keys[slot] = key;
            }
        }
    }
}

// COUNT, at the end of the kernel: one add per wave
__device__ __forceinline__ void count_flush(const CountArgs& C, u64 ncount, u64 nabove, int lane) {
    ncount = wave_sum(ncount);
    nabove = wave_sum(nabove);
    if (lane == 0) {
        if (ncount) atomicAdd(C.ncand, ncount);
        if (nabove) atomicAdd(&C.gcnt[C.T], nabove);
    }
}

// One body for all modes: every scan forms the logits with this loop (fetch, stash, products, factor update), so that the
// keys are the same bits in every scan; a mode's epilogue is a function above (HIST, EMIT) or, where that spilled or ran
// slower, a block of the body (COUNT, the link modes).  A new mode adds an epilogue and its part of ScanArgs, not a loop.
// FILT: the node-group rule on top of the exclusion, as in the ranking scan (dl_score_rank.hip): the groups of the pair's v
// and u nodes are staged in the pair's last step but one, all 512 threads form the mask from the rule, one word each, in its
// last step, and the row threads OR the exclusion into it where the unfiltered kernel starts from zero.
// P: planes per operand, 3 (fp32 tables, split_rows) or 1 (bf16 tables, copy_rows); it reaches the staging and the products
// only.  The one-plane step keeps the 32-column width: k-blocks are added in ascending k exactly as in the three-plane step.
// RECT (dl_score_mine_between, dl_score_links_between; the modes HIST_RECT, EMIT_RECT, DEG_RECT, FILL_RECT — further values
// of the mode, not a further template parameter, so that no existing kernel changes its name): the u side reads table A
// (A.N rows, A.nt tiles), the v side table B (A.rect), every tile pair of the ntA x ntB grid in row-major order.  A pair is in range iff a < nA and
// b < nB: no u < v, no diagonal; the exclusion CSR has the rows of A and B-local columns, the rule reads the groups of A for
// the rows and of B for the columns, the pair index is a nB + b, and the link modes keep one cell array and one CSR per side.
template <int MODE_, bool FILT = false, int P = 3>
__global__ __launch_bounds__(MTHR) void scan_tiles(ScanArgs A) {
    constexpr bool RECT = MODE_ >= HIST_RECT;                  // the rectangular form of ...
    constexpr int MODE = base_mode(MODE_);                     // ... this mode, which is all the body below asks for
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __bf16* us = reinterpret_cast<__bf16*>(lds);               // [2][P][TT][SLD]
    __bf16* vs = us + 2 * P * TT * SLD;
    unsigned* exm = reinterpret_cast<unsigned*>(vs + 2 * P * TT * SLD);   // [TT][4]: excluded columns of the tile
    unsigned* bins = exm + TT * 4;                              // HIST: [BINS]; COUNT: [SEPS] separators; DEG / FILL: masks, bases
    u64* fal = reinterpret_cast<u64*>(bins + (MODE == COUNT ? SEPS : BINS));           // FILT: allow [64] | cgrp [TT] | rgrp [TT]
    unsigned char* cgrp = reinterpret_cast<unsigned char*>(fal + 64);
    constexpr bool KEYED = MODE == DEG_TOP || MODE == FILL_TOP;       // dl_score_links_top: a pair also has to reach the selected key
    constexpr bool DEGS = MODE == DEG || MODE == DEG_TOP, FILLS = MODE == FILL || MODE == FILL_TOP;
    constexpr bool LINKS = DEGS || FILLS;                      // dl_score_links: no selection state, masks where the bins are
    static_assert(2 * TT * 4 * 4 + 2 * TT * 8 <= BINS * 4, "the link masks and bases fit where the bins are");

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // device-side state, read at workgroup start: a finished search makes the remaining histogram scans return at once
    Digit D = {};
    if constexpr (MODE == HIST || MODE == EMIT) {
        const State S = *A.state;
        if (MODE == HIST && S.done) return;
        D.prefix = S.prefix;
    }
    if constexpr (!LINKS)
        if (blockIdx.x == 0 && tid == 0) atomicAdd(&A.state->scans, 1u);
    // KEYED: the threshold key the select left (uniform; complete at the launch boundary, pick_kernel has finished)
    u64 threshold = 0ull;
    if constexpr (KEYED) threshold = A.state->prefix;
    const int p0 = (int)blockIdx.x * A.per_wg;
    // COUNT serves tile-pair counts close to 2^31, where p0 + per_wg would overflow; the other modes keep their form (N <= 46,340)
    const int ntl = MODE == COUNT || RECT ? max(0, min(A.per_wg, A.pairs - p0)) : max(0, min(A.pairs, p0 + A.per_wg) - p0);
    if (ntl == 0) return;
    // tile pair p0 in the row-major order of (qt, ct >= qt); RECT: of the whole ntA x ntB grid
    const int ntc = RECT ? A.rect.nt : A.nt;                    // tiles of the v side
    int qt = 0, ct = 0;
    if constexpr (RECT) {
        qt = p0 / ntc;
        ct = p0 - qt * ntc;
    } else {
        int rest = p0;
        while (rest >= A.nt - qt) {
            rest -= A.nt - qt;
            ++qt;
        }
        ct = qt + rest;
    }
    int qt2 = ct + 1 < ntc ? qt : qt + 1, ct2 = ct + 1 < ntc ? ct + 1 : RECT ? 0 : qt + 1;      // the pair after it

    const int li = lane & 31, half = lane >> 5;
    const int wu = wave >> 1, wv = wave & 1;
    const int nd = A.nd;
    const int per_tile = A.K * 2 * nd;
    const int steps = ntl * per_tile;
    if constexpr (MODE == HIST) {
        D.shift = digit_shift(A.sel.pass);
        D.dmask = (1u << digit_bits(A.sel.pass)) - 1u;
        D.hs = D.shift + digit_bits(A.sel.pass);
        for (int i = tid; i < BINS; i += MTHR) bins[i] = 0u;
    }
    // COUNT: separator j = target j * stride; the smallest and the largest target bound the candidates that need a search
    unsigned tmin = 0xFFFFFFFFu, tmax = 0u;
    u64 ncount = 0ull, nabove = 0ull;
    if constexpr (MODE == COUNT) {
        for (int i = tid; i < A.cnt.nsep; i += MTHR) bins[i] = A.cnt.tord[(size_t)i * A.cnt.stride];
        if (A.cnt.T > 0) {
            tmin = A.cnt.tord[0];
            tmax = A.cnt.tord[A.cnt.T - 1];
        }
    }
    if constexpr (FILT)
        if (tid < 64) fal[tid] = tid < A.filt.n_groups ? A.filt.allow[tid] : 0ull;

    PlaneStage<MTHR, SDC, P> uq, vq;
    static_assert(TT == PLANE_ROWS, "tiles of the plane arrays");
    int jcur = 0;                                               // tile pair (of this workgroup) the products are in
    auto fetch = [&](int s) {
        const int j = s / per_tile, rem = s - j * per_tile;
        const int k = rem / (2 * nd), r = rem - k * 2 * nd;
        const int dc = r < nd ? r : r - nd;
        const __bf16* src = (r < nd ? A.cz : A.ch) + (size_t)k * A.cbatch;
        const int fq = j == jcur ? qt : qt2, fc = j == jcur ? ct : ct2;      // a fetch runs at most one pair ahead
        uq.fetch(src + plane_tile<SDC, P>(fq, dc, nd), tid);
        if constexpr (RECT) {
            const __bf16* srb = (r < nd ? A.rect.cz : A.rect.ch) + (size_t)k * A.rect.cbatch;
            vq.fetch(srb + plane_tile<SDC, P>(fc, dc, nd), tid);
        } else {
            vq.fetch(src + plane_tile<SDC, P>(fc, dc, nd), tid);
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
    fetch(0);
    stash(0);
    fetch(min(1, steps - 1));
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int rem = s % per_tile;
        const int r = rem % (2 * nd);
        unsigned char gb = 0;                                   // FILT: group of node tid of (v tile | u tile), on its way to LDS
        if constexpr (FILT) {
            const int node = (tid < TT ? ct * TT : (qt - 1) * TT) + tid;
            if constexpr (RECT) {                               // each side against its own length, from its own array
                if (rem == per_tile - 2 && tid < 2 * TT && node < (tid < TT ? A.rect.N : A.N))
                    gb = (tid < TT ? A.rect.group : A.filt.group)[node];
            } else {
                if (rem == per_tile - 2 && tid < 2 * TT && node < A.N) gb = A.filt.group[node];
            }
        }
        const __bf16* ub = gram_operand<P>(us, s, wu * 32 + li, half);
        const __bf16* vb = gram_operand<P>(vs, s, wv * 64 + li, half);
#pragma unroll
        for (int kb = 0; kb < SDC / 16; ++kb) {
            gram_block<P>(acc, ub, vb, kb);                     // the ranking scan's products (dl_tiles.h)
            if (kb == 0) {
                if (s + 1 < steps) stash(s + 1);
                fetch(min(s + 2, steps - 1));                   // unconditional: see TileStage (dl_tiles.h)
            }
        }
        factor_update(acc, e, term, r, nd, A.t);                // S complete: e = exp(S / t); Q complete: term += Q * e
        if constexpr (FILT) {
            if (rem == per_tile - 2) {
                if (tid < 2 * TT) cgrp[tid] = gb;
            } else if (rem == per_tile - 1) {                   // word tid & 3 of row tid >> 2
                exm[tid] = filter_word(fal[cgrp[TT + (tid >> 2)] & 63], cgrp + (tid & 3) * 32);
            }
        }
        __syncthreads();
        if (rem != per_tile - 1) continue;

        // ---- tile pair complete: term[bb][q] = s(u = qt*128 + wu*32 + acc_row(q, half), v = ct*128 + wv*64 + bb*32 + li)
        const Tile T = {qt * TT, ct * TT, RECT ? A.rect.N : A.N, A.N};
        if (tid < TT) {                                         // this tile's excluded columns of row u0 + tid
            unsigned* m = exm + tid * 4;
            if constexpr (!FILT) m[0] = m[1] = m[2] = m[3] = 0u;
            const int node = T.u0 + tid;
            if (node < A.N && A.ex_rowptr != nullptr) {
                const int end = A.ex_rowptr[node + 1];
                exclusion_mask(A.ex_col, first_col_at_least(A.ex_col, A.ex_rowptr[node], end, T.v0), end, T.v0, m);
            }
        }
        if constexpr (FILLS) {                                  // where the cells of this tile pair start in the CSR
            long long* ubase = reinterpret_cast<long long*>(bins + 2 * TT * 4), *vbase = ubase + TT;
            if (tid < TT) {
                const int node = T.u0 + tid;
                ubase[tid] = node < A.N ? (long long)A.link.rowptr[node] + (long long)A.link.cnt[(size_t)node * ntc + ct] : 0ll;
            } else if (tid < 2 * TT) {
                const int node = T.v0 + tid - TT;
                if constexpr (RECT)                             // the B side's own CSR: cell (b, qt) of cnt [nB][ntA]
                    vbase[tid - TT] = node < A.rect.N ? (long long)A.rect.link.rowptr[node] +
                                                        (long long)A.rect.link.cnt[(size_t)node * A.nt + qt] : 0ll;
                else
                    vbase[tid - TT] = node < A.N ? (long long)A.link.rowptr[node] + (long long)A.link.cnt[(size_t)node * A.nt + qt] : 0ll;
            }
        }
        __syncthreads();
        if constexpr (LINKS) {                                  // in the body: as functions FILL measured 0.7-1.0 % slower
            unsigned* pm = bins;                                // [TT][4] pass mask, bit v of row u
            unsigned* pmt = bins + TT * 4;                      // [TT][4] its transpose, bit u of column v
            const long long* ubase = reinterpret_cast<const long long*>(bins + 2 * TT * 4);    // FILL: [TT] first slot of cell (u, ct)
            const long long* vbase = ubase + TT;                // FILL: [TT] first slot of cell (v, qt)
            // The tile's pass mask, row-major and column-major, without atomics: a ballot holds 32 columns of two rows (one
            // per half of the wave), and a lane gathers the 16 rows of its half for its column, the other half's by a swap.
            // Ranks come from these masks, never from the order of lanes or of acc_row.
            // Wave-uniform and constant terms are kept apart from the lane's (rows of a lane: rbase + acc_row(q, 0)), so that
            // nothing per q is loop-invariant and held in registers across the product loop.
            const int swu = __builtin_amdgcn_readfirstlane(wu), swv = __builtin_amdgcn_readfirstlane(wv);
            const int hs4 = half * 4, rbase = swu * 32 + hs4;
            unsigned okm = 0u;                                  // bit bb * 16 + q: this lane's value passed
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const int vw = swv * 2 + bb, vl = vw * 32 + li, v = T.v0 + vl;
                unsigned rows = 0u;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = rbase + acc_row(q, 0), u = T.u0 + row;
                    bool ok = (RECT ? u < A.N && v < A.rect.N : u < v && v < A.N) && !((exm[row * 4 + vw] >> li) & 1u) &&
                              term[bb][q] >= A.min_logit;
                    if constexpr (KEYED) ok = ok && make_key(term[bb][q], (unsigned)u * (unsigned)A.N + (unsigned)v) >= threshold;
                    const u64 b = __ballot(ok);
                    if (li == 0) pm[row * 4 + vw] = half ? (unsigned)(b >> 32) : (unsigned)b;
                    rows |= ok ? 1u << acc_row(q, 0) : 0u;
                    okm |= ok ? 1u << (bb * 16 + q) : 0u;
                }
                rows <<= hs4;
                rows |= (unsigned)__shfl_xor((int)rows, 32, DL_WAVE);
                if (half == 0) pmt[vl * 4 + swu] = rows;
            }
            __syncthreads();
            const bool diag = !RECT && qt == ct;                // RECT: never; its diag branches fold away
            if constexpr (DEGS) {
                // cell (u, ct) from the rows, cell (v, qt) from the columns; on the diagonal both sides of a node are one cell.
                // Every cell of every node < N is written once, by the one workgroup that forms its tile pair, zeros included.
                if (tid < TT) {
                    const int node = T.u0 + tid;
                    const unsigned* w = pm + tid * 4;
                    unsigned c = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
                    if (diag) {
                        const unsigned* wt = pmt + tid * 4;
                        c += __popc(wt[0]) + __popc(wt[1]) + __popc(wt[2]) + __popc(wt[3]);
                    }
                    if (node < A.N) A.link.cnt[(size_t)node * ntc + ct] = c;
                } else if (tid < 2 * TT && !diag) {
                    const int node = T.v0 + tid - TT;
                    const unsigned* wt = pmt + (tid - TT) * 4;
                    if constexpr (RECT) {                       // cell (b, qt) of the B side's cnt [nB][ntA]
                        if (node < A.rect.N)
                            A.rect.link.cnt[(size_t)node * A.nt + qt] = __popc(wt[0]) + __popc(wt[1]) + __popc(wt[2]) + __popc(wt[3]);
                    } else {
                        if (node < A.N) A.link.cnt[(size_t)node * A.nt + qt] = __popc(wt[0]) + __popc(wt[1]) + __popc(wt[2]) + __popc(wt[3]);
                    }
                }
            } else {
                // slot of (u, v) in row u: the cell's start, on the diagonal the smaller neighbours of u first, then the passed
                // columns below v; in row v: the cell's start and the passed rows below u.  Columns ascend within a row.
#pragma unroll
                for (int bb = 0; bb < 2; ++bb) {
                    const int vw = swv * 2 + bb, vl = vw * 32 + li, v = T.v0 + vl;
                    const unsigned* wt = pmt + vl * 4;
                    const unsigned vword = wt[swu], vsh = vword >> hs4;
                    const long long vb = vbase[vl] + (swu > 0 ? __popc(wt[0]) : 0) + (swu > 1 ? __popc(wt[1]) : 0) +
                                         (swu > 2 ? __popc(wt[2]) : 0) + __popc(vword & ((1u << hs4) - 1u));
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        if (!((okm >> (bb * 16 + q)) & 1u)) continue;
                        const int row = rbase + acc_row(q, 0), u = T.u0 + row;
                        const unsigned* w = pm + row * 4;
                        long long su = ubase[row] + (vw > 0 ? __popc(w[0]) : 0) + (vw > 1 ? __popc(w[1]) : 0) + (vw > 2 ? __popc(w[2]) : 0) +
                                       __popc(w[vw] & ((1u << li) - 1u));
                        if (diag) {
                            const unsigned* ut = pmt + row * 4;
                            su += __popc(ut[0]) + __popc(ut[1]) + __popc(ut[2]) + __popc(ut[3]);
                        }
                        const long long sv = vb + __popc(vsh & ((1u << acc_row(q, 0)) - 1u));
                        const float x = term[bb][q] == 0.0f ? 0.0f : term[bb][q];      // -0 is reported as +0
                        const float pr = A.link.prob != nullptr ? sigmoid_ref(x) : 0.0f;
                        if ((u64)su < (u64)A.link.nnz) {
                            A.link.col[su] = v;
                            A.link.logit[su] = x;
                            if (A.link.prob != nullptr) A.link.prob[su] = pr;
                        }
                        if constexpr (RECT) {                   // (b, a) in the B side's CSR, under its own nnz
                            if ((u64)sv < (u64)A.rect.link.nnz) {
                                A.rect.link.col[sv] = u;
                                A.rect.link.logit[sv] = x;
                                if (A.link.prob != nullptr) A.rect.link.prob[sv] = pr;
                            }
                        } else if ((u64)sv < (u64)A.link.nnz) {
                            A.link.col[sv] = u;
                            A.link.logit[sv] = x;
                            if (A.link.prob != nullptr) A.link.prob[sv] = pr;
                        }
                    }
                }
            }
        } else {
            const Lane L = {wu, wv, li, half, lane};
            if constexpr (MODE == HIST) hist_epilogue<RECT>(term, exm, bins, L, T, A.min_logit, D);
            else if constexpr (MODE == EMIT) emit_epilogue<RECT>(term, exm, L, T, A.min_logit, D.prefix, A.state, A.sel.keys, A.sel.m);
            else {
                // COUNT: the place of every candidate among the sorted targets: lo = targets strictly below it (they count it
                // as "greater": +1 at gcnt[lo], summed from the top on the host), and the equal range, if any, starts at lo.
                // Kept in the kernel body: as a function of its own it takes the instantiation from 250 to 256 VGPRs and spills.
#pragma unroll
                for (int bb = 0; bb < 2; ++bb) {
                    const int vl = wv * 64 + bb * 32 + li;
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int row = wu * 32 + acc_row(q, half), u = T.u0 + row, v = T.v0 + vl;
                        const bool ok = u < v && v < T.N && !((exm[row * 4 + (vl >> 5)] >> (vl & 31)) & 1u);
                        const unsigned o = ord_key(term[bb][q]);
                        ncount += ok ? 1ull : 0ull;
                        nabove += (ok && o > tmax) ? 1ull : 0ull;
                        const bool in = ok && o >= tmin && o <= tmax;
                        int lo = 0;
                        bool tie = false;
                        if (in) {
                            int a = 0, b = A.cnt.nsep;              // separators below o: [0, a)
                            while (a < b) {
                                const int mid = (a + b) >> 1;
                                if (bins[mid] < o) a = mid + 1; else b = mid;
                            }
                            if (a > 0) {                        // target (a-1) stride < o <= target a stride (or the end)
                                int l = (a - 1) * A.cnt.stride + 1, h = min(a * A.cnt.stride, A.cnt.T);
                                while (l < h) {
                                    const int mid = (l + h) >> 1;
                                    if (A.cnt.tord[mid] < o) l = mid + 1; else h = mid;
                                }
                                lo = l;
                            }
                            tie = A.cnt.tord[lo] == o;              // lo < T: o <= tmax
                        }
                        const u64 act = __ballot(in);
                        if (act != 0ull) {                      // wave-uniform; one place per wave where the logits cluster
                            const int first = __ffsll((long long)act) - 1;
                            const int l0 = __shfl(lo, first, DL_WAVE);
                            if (__ballot(in && lo == l0) == act) {
                                const u64 eq = __ballot(in && tie);
                                if (lane == first) {
                                    if (l0 > 0) atomicAdd(&A.cnt.gcnt[l0], (u64)__popcll(act));
                                    if (eq != 0ull) atomicAdd(&A.cnt.tcnt[l0], (u64)__popcll(eq));
                                }
                            } else if (in) {
                                if (lo > 0) atomicAdd(&A.cnt.gcnt[lo], 1ull);
                                if (tie) atomicAdd(&A.cnt.tcnt[lo], 1ull);
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) zero_acc(term[bb]);
        ++jcur;                                                 // on to the next pair (uniform; fetches are already there)
        qt = qt2;
        ct = ct2;
        qt2 = ct + 1 < ntc ? qt : qt + 1;
        ct2 = ct + 1 < ntc ? ct + 1 : RECT ? 0 : qt + 1;
    }
    if constexpr (MODE == HIST) hist_flush(bins, A.sel.hist, tid);
    if constexpr (MODE == COUNT) count_flush(A.cnt, ncount, nabove, lane);
}

__global__ __launch_bounds__(256) void init_kernel(State* st, unsigned* hist, int m) {
    for (int i = threadIdx.x; i < BINS; i += 256) hist[i] = 0u;
    if (threadIdx.x == 0) {
        State s = {};
        s.need = (unsigned)m;
        *st = s;
    }
}

// One workgroup: the digit of pass `pass` in which the need-th best key with the current prefix lies.  Counts are integers
// and complete (the launch boundary), so the choice is a function of the candidates alone.
__global__ __launch_bounds__(256) void pick_kernel(State* st, unsigned* hist, int pass, int m) {
    __shared__ unsigned part[256];
    __shared__ unsigned chunk[3];                               // all taken?, chunk of the digit, keys above the chunk
    const int tid = threadIdx.x;
    const State s0 = *st;
    if (s0.done) return;
    const int nb = 1 << digit_bits(pass);
    constexpr int PER = BINS / 256;
    unsigned mine[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {                             // thread tid: bins nb-1 - (tid*PER + j), from the top
        const int b = nb - 1 - (tid * PER + j);
        mine[j] = b >= 0 ? hist[b] : 0u;
        sum += mine[j];
    }
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned total = 0;
        for (int i = 0; i < 256; ++i) total += part[i];
        unsigned above = 0;
        int c = 0;
        if (total >= s0.need)
            while (c < 255 && above + part[c] < s0.need) above += part[c++];
        chunk[0] = total < s0.need ? 1u : 0u;
        chunk[1] = (unsigned)c;
        chunk[2] = above;
    }
    __syncthreads();
    if (chunk[0]) {                                             // (first pass only) fewer candidates than m: all of them
        if (tid == 0) {
            State s = s0;
            s.prefix = 0ull;
            unsigned total = 0;
            for (int i = 0; i < 256; ++i) total += part[i];
            s.count = total;
            s.need = 0;
            s.done = 1;
            *st = s;
        }
    } else if (tid == (int)chunk[1]) {
        State s = s0;
        unsigned above = chunk[2], cnt = 0;
        int sel = -1;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (sel < 0) {
                if (above + mine[j] >= s.need) {
                    sel = j;
                    cnt = mine[j];
                } else {
                    above += mine[j];
                }
            }
        }
        const int b = max(0, nb - 1 - (tid * PER + max(sel, 0)));
        s.prefix |= (u64)(unsigned)b << digit_shift(pass);
        s.need -= above;
        if (cnt == s.need) {                                    // every key with this prefix is taken: the threshold
            s.done = 1;
            s.count = (unsigned)m;
        }
        *st = s;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {                             // the next pass counts from zero
        const int b = nb - 1 - (tid * PER + j);
        if (b >= 0) hist[b] = 0u;
    }
}

// Rank by counting: the emitted keys are distinct, so the ranks are a permutation of [0, count).  Every element of every
// output is written: thread i < count writes slot rank(i), thread i >= count writes the padding of slot i.
__global__ __launch_bounds__(256) void order_kernel(const State* st, const u64* __restrict__ keys, int N, int m, int32_t* src,
                                                    int32_t* dst, float* logit, float* prob, int64_t* count) {
    __shared__ u64 sm[1024];
    const int count_ = (int)min(st->count, (unsigned)m);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) count[0] = (int64_t)count_;
    if ((int)blockIdx.x * 256 >= count_) {                      // a workgroup of padding only (uniform)
        if (i < m) {
            src[i] = -1;
            dst[i] = -1;
            logit[i] = __uint_as_float(0x7FC00000u);
            prob[i] = __uint_as_float(0x7FC00000u);
        }
        return;
    }
    const u64 x = i < count_ ? keys[i] : 0ull;
    int rank = 0;
    for (int b = 0; b < count_; b += 1024) {
        __syncthreads();
        for (int j = threadIdx.x; j < 1024; j += 256) sm[j] = b + j < count_ ? keys[b + j] : 0ull;
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < 1024; ++j) rank += sm[j] > x ? 1 : 0;
    }
    if (i < count_) {
        const float val = ord_value((unsigned)(x >> 32));
        const unsigned pair = 0xFFFFFFFFu - (unsigned)x;
        src[rank] = (int32_t)(pair / (unsigned)N);
        dst[rank] = (int32_t)(pair % (unsigned)N);
        logit[rank] = val;
        prob[rank] = sigmoid_ref(val);
    } else if (i < m) {
        src[i] = -1;
        dst[i] = -1;
        logit[i] = __uint_as_float(0x7FC00000u);
        prob[i] = __uint_as_float(0x7FC00000u);
    }
}

// ---- dl_score_links: the offsets between the DEG and the FILL scan
// One wave per node: its nt cells become their exclusive prefix in place (at most N - 1 < 2^16 in all), the total its degree.
__global__ __launch_bounds__(256) void link_cells_kernel(unsigned* cnt, unsigned* deg, int N, int nt) {
    const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;                                       // wave-uniform
    unsigned* c = cnt + (size_t)row * nt;
    unsigned run = 0u;
    for (int b = 0; b < nt; b += DL_WAVE) {
        const int i = b + lane;
        const unsigned x = i < nt ? c[i] : 0u;
        unsigned inc = x;
#pragma unroll
        for (int o = 1; o < DL_WAVE; o <<= 1) {
            const unsigned y = (unsigned)__shfl_up((int)inc, o, DL_WAVE);
            if (lane >= o) inc += y;
        }
        if (i < nt) c[i] = run + inc - x;
        run += (unsigned)__shfl((int)inc, DL_WAVE - 1, DL_WAVE);
    }
    if (lane == 0) deg[row] = run;
}

// One workgroup: rowptr = the exclusive 64-bit prefix of the degrees, rowptr[N] = nnz.  Thread i sums a run of consecutive
// nodes, the 1,024 sums are scanned in LDS, and the thread walks its run again.  scanned = 0 (N < 2): no pair, all zeros.
__global__ __launch_bounds__(1024) void link_rowptr_kernel(const unsigned* __restrict__ deg, int64_t* rowptr, int N, int scanned) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x, per = (N + 1023) / 1024;
    const int lo = min(N, tid * per), hi = min(N, lo + per);
    long long sum = 0;
    if (scanned)
        for (int i = lo; i < hi; ++i) sum += (long long)deg[i];
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const long long y = tid >= o ? part[tid - o] : 0ll;
        __syncthreads();
        part[tid] += y;
        __syncthreads();
    }
    long long run = part[tid] - sum;
    for (int i = lo; i < hi; ++i) {
        rowptr[i] = (int64_t)run;
        if (scanned) run += (long long)deg[i];
    }
    if (tid == 1023) rowptr[N] = (int64_t)part[1023];
}

}  // namespace mine

using namespace mine;

// ---- The parts every driver below is made of: the plan of the tile walk, the carving of the workspace, the tables' planes,
// the builder of ScanArgs, the launcher, the select and the offsets step.  A driver names its passes.

// The tile walk of rows of a table A against rows of a table B, over tables of one shape (K, d) and type.  A triangle is the
// case "B is A": the tile pairs u tile <= v tile, none for N < 2; a rectangle walks every tile pair of the ntA x ntB grid.
// Tile pairs per workgroup: eight workgroups' worth of pairs per CU (one workgroup per CU fits the LDS; short runs keep the
// tail of the grid short, consecutive pairs of a run share their u tile).  DL_MINE_TILES (test knob) forces the run length;
// results do not depend on it.
struct Plan { bool rect; int nA, nB, K, d, nd, ntA, ntB, pairs, per_wg, grid; size_t cbatchA, cbatchB; dl_dtype dt; };
static Plan tile_plan(bool rect, int nA, int nB, int K, int d, dl_dtype dt) {
    Plan p = {};
    p.rect = rect; p.nA = nA; p.nB = nB; p.K = K; p.d = d; p.dt = dt;
    p.nd = (d + SDC - 1) / SDC;
    p.ntA = (nA + TT - 1) / TT;
    p.ntB = (nB + TT - 1) / TT;
    // 64-bit: nt (nt + 1) / 2 fits an int32 up to nt = 65,535 (the callers' limit on N), its intermediates do not; a
    // rectangle has <= 363^2
    const long long pairs = rect ? (long long)p.ntA * p.ntB : nA >= 2 ? (long long)p.ntA * (p.ntA + 1) / 2 : 0;
    p.pairs = (int)pairs;
    const long long per_cu = 8LL * device_cus();
    const int want = config().mine_tiles > 0 ? config().mine_tiles : (int)((pairs + per_cu - 1) / per_cu);
    p.per_wg = max(1, min(want, max(1, p.pairs)));
    p.grid = (int)((pairs + p.per_wg - 1) / p.per_wg);
    p.cbatchA = table_plane_elems(dt, nA, d);                  // the one thing of a plan that depends on the table type
    p.cbatchB = table_plane_elems(dt, nB, d);
    return p;
}
// what every *_form reports of a plan: out = nd, tiles (of A, then of B: rectangle), tile pairs, tile pairs per workgroup,
// workgroups of a scan
static void plan_form(const Plan& p, int* out) {
    *out++ = p.nd;
    *out++ = p.ntA;
    if (p.rect) *out++ = p.ntB;
    *out++ = p.pairs;
    *out++ = p.per_wg;
    *out++ = p.grid;
}
static Plan triangle(int N, int K, int d, dl_dtype dt = DL_F32) { return tile_plan(false, N, N, K, d, dt); }
static Plan rectangle(int nA, int nB, int K, int d, dl_dtype dt = DL_F32) { return tile_plan(true, nA, nB, K, d, dt); }

// The workspace (256-byte aligned blocks), always in this order, of the pieces a driver names:
//   the select's:    selection state | histogram | keys [keys]          (WS_STATE: the state alone; keys = 0: no key array)
//   the planes:      of Z and H (triangle), of ZA, HA, ZB, HB (rectangle); three per fp32 table, the one of a bf16 table
//   the link cells:  cnt [N][nt] | deg [N] (triangle), cnt_a [nA][ntB] | cnt_b [nB][ntA] | deg_a [nA] | deg_b [nB] (rectangle)
enum { WS_STATE = 1, WS_HIST = 2, WS_SELECT = WS_STATE | WS_HIST, WS_CELLS = 4 };
struct Ws { State* state; unsigned* hist; u64* keys; __bf16 *za, *ha, *zb, *hb; unsigned *cnt_a, *cnt_b, *deg_a, *deg_b; size_t bytes; };
static Ws carve(const Plan& p, int pieces, size_t keys, void* ws) {
    Ws w = {};
    Carver c(ws);
    if (pieces & WS_STATE) w.state = c.take<State>(1);
    if (pieces & WS_HIST) w.hist = c.take<unsigned>(BINS);
    if (keys > 0) w.keys = c.take<u64>(keys);
    w.zb = w.za = c.take<__bf16>((size_t)p.K * p.cbatchA);     // a triangle's B is its A
    w.hb = w.ha = c.take<__bf16>((size_t)p.K * p.cbatchA);
    if (p.rect) {
        w.zb = c.take<__bf16>((size_t)p.K * p.cbatchB);
        w.hb = c.take<__bf16>((size_t)p.K * p.cbatchB);
    }
    if (pieces & WS_CELLS) {
        w.cnt_a = c.take<unsigned>((size_t)p.nA * p.ntB);      // <= 46,340 * 363 cells
        if (p.rect) w.cnt_b = c.take<unsigned>((size_t)p.nB * p.ntA);
        w.deg_a = c.take<unsigned>((size_t)p.nA);
        if (p.rect) w.deg_b = c.take<unsigned>((size_t)p.nB);
    }
    w.bytes = c.bytes();
    return w;
}

// The tables of a scan (a triangle has no ZB, HB) and their split into the planes of the workspace
struct Tables { const void *ZA, *HA, *ZB, *HB; };
static void split_tables(const Plan& p, const Ws& w, const Tables& T, hipStream_t st) {
    table_planes(T.ZA, p.dt, nullptr, p.nA, p.K, p.d, w.za, st);
    table_planes(T.HA, p.dt, nullptr, p.nA, p.K, p.d, w.ha, st);
    if (!p.rect) return;
    table_planes(T.ZB, p.dt, nullptr, p.nB, p.K, p.d, w.zb, st);
    table_planes(T.HB, p.dt, nullptr, p.nB, p.K, p.d, w.hb, st);
}

// Either kind of node-group rule as the kernels take it: the groups of the rows (of A) and the allow table, and the groups
// of the rows of B where B has its own
struct Rule { bool on; FilterArgs filt; const unsigned char* group_b; };
static Rule rule_of(const dl_node_filter* nf) { return Rule{nf != nullptr, filter_args(nf), nullptr}; }
static Rule rule_of(const dl_node_filter_between* nf) {
    if (nf == nullptr) return Rule{false, FilterArgs{nullptr, nullptr, 0}, nullptr};
    return Rule{true, FilterArgs{nf->group_a, (const u64*)nf->allow, nf->n_groups}, nf->group_b};
}

// What every scan of the family reads; a mode's own part of ScanArgs is its driver's
static ScanArgs scan_args(const Plan& p, const Ws& w, float t, const int32_t* exr, const int32_t* exc, float min_logit, const Rule& r) {
    ScanArgs a = {};
    a.cz = w.za; a.ch = w.ha; a.cbatch = p.cbatchA;
    a.N = p.nA; a.K = p.K; a.nd = p.nd; a.nt = p.ntA; a.t = t;
    a.ex_rowptr = exr; a.ex_col = exc;
    a.min_logit = min_logit;
    a.pairs = p.pairs; a.per_wg = p.per_wg;
    a.filt = r.filt;
    if (p.rect) {
        a.rect.cz = w.zb; a.rect.ch = w.hb; a.rect.cbatch = p.cbatchB;
        a.rect.N = p.nB; a.rect.nt = p.ntB;
        a.rect.group = r.group_b;
    }
    return a;
}

// The instantiations of scan_tiles, named once in the order in which the code object holds them.  The compiler emits kernels
// in the order of their first use, so with this list a change of the host code below leaves the device assembly of the unit
// the same text, which is how such a change is checked (hipcc -S --cuda-device-only, before and after).
#define DL_SCAN_FORMS(MODE, F0, F1) scan_tiles<MODE, F0, 1>, scan_tiles<MODE, F1, 1>, scan_tiles<MODE, F0, 3>, scan_tiles<MODE, F1, 3>
[[maybe_unused]] static void (*const SCAN_FORMS[])(ScanArgs) = {
    DL_SCAN_FORMS(HIST, false, true), DL_SCAN_FORMS(EMIT, false, true), DL_SCAN_FORMS(COUNT, false, true),
    DL_SCAN_FORMS(DEG, false, true), DL_SCAN_FORMS(FILL, false, true),
    DL_SCAN_FORMS(HIST_RECT, true, false), DL_SCAN_FORMS(EMIT_RECT, true, false), DL_SCAN_FORMS(DEG_RECT, true, false),
    DL_SCAN_FORMS(FILL_RECT, true, false), DL_SCAN_FORMS(DEG_TOP, false, true), DL_SCAN_FORMS(FILL_TOP, false, true)};
#undef DL_SCAN_FORMS

// One scan in the instantiation the plan asks for: the RECT form of the mode on a rectangle (HIST, EMIT, DEG and FILL have
// one), one plane per operand on bf16 tables, FILT (which keeps FILTER_LDS_BYTES behind the mode's LDS) under a rule
constexpr bool has_rect(int mode) { return mode == HIST || mode == EMIT || mode == DEG || mode == FILL; }
template <int MODE, int P>
static void launch_planes(const Plan& p, const ScanArgs& a, bool filtered, hipStream_t st) {
    const unsigned grid = (unsigned)p.grid;
    const size_t lds = lds_bytes(MODE, P) + (filtered ? FILTER_LDS_BYTES : 0);
    if constexpr (has_rect(MODE)) {
        if (p.rect) {
            if (filtered) launch_lds<scan_tiles<rect_mode(MODE), true, P>>(grid, MTHR, lds, st, a);
            else launch_lds<scan_tiles<rect_mode(MODE), false, P>>(grid, MTHR, lds, st, a);
            return;
        }
    }
    if (filtered) launch_lds<scan_tiles<MODE, true, P>>(grid, MTHR, lds, st, a);
    else launch_lds<scan_tiles<MODE, false, P>>(grid, MTHR, lds, st, a);
}
template <int MODE>
static void launch(const Plan& p, const ScanArgs& a, bool filtered, hipStream_t st) {
    if (p.dt == DL_BF16) launch_planes<MODE, 1>(p, a, filtered, st);
    else launch_planes<MODE, 3>(p, a, filtered, st);
}

// The radix select of the `need` best keys: the state and the histogram cleared, the tables split, then one HIST scan and one
// pick per digit.  It leaves the threshold key in State::prefix and the select's part of `a` filled in; without a tile pair
// only the state is set (no candidate, count 0).
static void select(const Plan& p, const Ws& w, const Tables& T, ScanArgs& a, int need, bool filtered, hipStream_t st) {
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(256), 0, st, w.state, w.hist, need);
    if (p.pairs == 0) return;
    split_tables(p, w, T, st);
    a.state = w.state;
    a.sel.m = need; a.sel.hist = w.hist; a.sel.keys = w.keys;
    for (int pass = 0; pass < PASSES; ++pass) {
        a.sel.pass = pass;
        launch<HIST>(p, a, filtered, st);
        hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(256), 0, st, w.state, w.hist, pass, need);
    }
}

// The offsets of one side of a link graph, between its count and its fill: every node's cells [n][nt] into their exclusive
// prefix and its degree, then the degrees into rowptr.  scanned = false (no tile pair wrote a cell): rowptr is all zero.
static void link_offsets(unsigned* cnt, unsigned* deg, int n, int nt, bool scanned, int64_t* rowptr, hipStream_t st) {
    if (scanned) hipLaunchKernelGGL(link_cells_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, cnt, deg, n, nt);
    hipLaunchKernelGGL(link_rowptr_kernel, dim3(1), dim3(1024), 0, st, deg, rowptr, n, scanned ? 1 : 0);
}

// The count pass of a link graph over split tables: the DEG scan (DEG_TOP: under the key a select left), then the offsets of
// the A side and, on a rectangle, of the B side
template <int MODE>
static void count_links(const Plan& p, const Ws& w, ScanArgs& a, bool filtered, int64_t* rowptr_a, int64_t* rowptr_b, hipStream_t st) {
    if (p.pairs > 0) {
        a.link.cnt = w.cnt_a;
        if (p.rect) a.rect.link.cnt = w.cnt_b;
        launch<MODE>(p, a, filtered, st);
    }
    link_offsets(w.cnt_a, w.deg_a, p.nA, p.ntB, p.pairs > 0, rowptr_a, st);
    if (p.rect) link_offsets(w.cnt_b, w.deg_b, p.nB, p.ntA, p.pairs > 0, rowptr_b, st);
}

// The fill pass over the planes and cells the count left: the CSR of the A side and, on a rectangle, of the B side.  A side
// of length 0 takes no write (every slot is >= its nnz); nothing to write at all: no scan.
template <int MODE>
static void fill_links(const Plan& p, ScanArgs& a, bool filtered, const LinkArgs& side_a, const LinkArgs& side_b, hipStream_t st) {
    if (p.pairs == 0 || (side_a.nnz <= 0 && side_b.nnz <= 0)) return;
    a.link = side_a;
    if (p.rect) a.rect.link = side_b;
    launch<MODE>(p, a, filtered, st);
}

// The m best pairs of a plan, in order: the select, an EMIT scan of the keys at or above its threshold, the ordering, which
// decodes the pair index with the row length of the walk (N; nB on a rectangle: src A-local, dst B-local)
static int mine_pairs(const char* what, const Plan& p, const Tables& T, float t, const int32_t* exr, const int32_t* exc, float min_logit,
                      int m, const Rule& r, int32_t* src, int32_t* dst, float* logit, float* prob, int64_t* count, void* ws,
                      hipStream_t st) {
    const Ws w = carve(p, WS_SELECT, (size_t)m, ws);
    ScanArgs a = scan_args(p, w, t, exr, exc, min_logit, r);
    select(p, w, T, a, m, r.on, st);
    if (p.pairs > 0) launch<EMIT>(p, a, r.on, st);
    hipLaunchKernelGGL(order_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, w.state, w.keys, p.rect ? p.nB : max(p.nA, 1),
                       m, src, dst, logit, prob, count);
    return check_launch(what);
}

// ---- dl_score_mine: the m best unordered pairs u < v of one table
bool score_mine_supported(int K, int d) { return score_rank_supported(K, d); }

// out = nd, tiles, tile pairs, tile pairs per workgroup, workgroups of a scan, scans at most (digits + emit), byte offset of
// the 32-bit count of scans that ran inside the (256-byte aligned) workspace
void score_mine_form(int N, int d, int m, int* out) {
    (void)m;
    const Plan p = triangle(N, 0, d);
    plan_form(p, out);
    out[5] = p.pairs > 0 ? PASSES + 1 : 0;
    out[6] = (int)offsetof(State, scans);
}

size_t score_mine_workspace_bytes(int N, int K, int d, int m, dl_dtype dt) {
    return carve(triangle(N, K, d, dt), WS_SELECT, (size_t)m, nullptr).bytes;
}

int score_mine(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* exr, const int32_t* exc,
               float min_logit, int m, int32_t* src, int32_t* dst, float* logit, float* prob, int64_t* count, void* ws, hipStream_t st,
               const dl_node_filter* nf) {
    return mine_pairs("score_mine", triangle(N, K, d, dt), Tables{Z, H, nullptr, nullptr}, t, exr, exc, min_logit, m, rule_of(nf), src,
                      dst, logit, prob, count, ws, st);
}

// ---- dl_score_pair_ranks: ONE counting scan (scan_tiles<COUNT>) over the sorted order keys of T target pairs
struct PairRankPlan { Plan m; int stride, nsep, lds_levels, global_levels; };
static int search_levels(int n) {                               // iterations of a lower-bound search over n elements, at most
    int l = 0;
    while (n > 0) {
        ++l;
        n >>= 1;
    }
    return l;
}
static PairRankPlan pair_rank_plan(int N, int K, int d, int T, dl_dtype dt = DL_F32) {
    PairRankPlan p;
    p.m = triangle(N, K, d, dt);
    p.stride = max(1, (T + SEPS - 1) / SEPS);
    p.nsep = (T + p.stride - 1) / p.stride;
    p.lds_levels = search_levels(p.nsep);
    p.global_levels = search_levels(p.stride - 1);
    return p;
}

// out = nd, tiles, tile pairs, tile pairs per workgroup, workgroups, separators in LDS, targets per separator, search
// levels in LDS, search levels in global memory
void score_pair_ranks_form(int N, int d, int T, int* out) {
    const PairRankPlan p = pair_rank_plan(N, 0, d, T);
    plan_form(p.m, out);
    out[5] = p.nsep;
    out[6] = p.stride;
    out[7] = p.lds_levels;
    out[8] = p.global_levels;
}

size_t score_pair_ranks_workspace_bytes(int N, int K, int d, dl_dtype dt) { return carve(triangle(N, K, d, dt), WS_STATE, 0, nullptr).bytes; }

int score_pair_ranks(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* exr, const int32_t* exc,
                     const unsigned* tord, int T, u64* gcnt, u64* tcnt, u64* ncand, void* ws, hipStream_t st,
                     const dl_node_filter* nf) {
    const PairRankPlan p = pair_rank_plan(N, K, d, T, dt);
    const Ws w = carve(p.m, WS_STATE, 0, ws);
    hipError_t e = hipMemsetAsync(w.state, 0, sizeof(State), st);
    if (e == hipSuccess) e = hipMemsetAsync(gcnt, 0, sizeof(u64) * ((size_t)T + 1), st);
    if (e == hipSuccess) e = hipMemsetAsync(tcnt, 0, sizeof(u64) * ((size_t)T + 1), st);
    if (e == hipSuccess) e = hipMemsetAsync(ncand, 0, sizeof(u64), st);
    DL_REQUIRE(e == hipSuccess, "hipMemsetAsync: %s", hipGetErrorString(e));
    if (p.m.pairs > 0) {
        const Rule r = rule_of(nf);
        split_tables(p.m, w, Tables{Z, H, nullptr, nullptr}, st);
        ScanArgs a = scan_args(p.m, w, t, exr, exc, 0.0f, r);
        a.state = w.state;
        a.cnt = CountArgs{tord, T, p.stride, p.nsep, gcnt, tcnt, ncand};
        launch<COUNT>(p.m, a, r.on, st);
    }
    return check_launch("score_pair_ranks");
}

// ---- dl_score_links: every eligible pair as a symmetric CSR — a DEG scan, the offsets, then (second call) a FILL scan
bool score_links_supported(int K, int d) { return score_mine_supported(K, d); }

// out = nd, tiles, tile pairs, tile pairs per workgroup, workgroups of a scan, scans of count + fill, cells of cnt
void score_links_form(int N, int d, int* out) {
    const Plan p = triangle(N, 0, d);
    plan_form(p, out);
    out[5] = p.pairs > 0 ? 2 : 0;
    out[6] = N * p.ntA;                                         // <= 46,340 * 363
}

size_t score_links_workspace_bytes(int N, int K, int d, dl_dtype dt) { return carve(triangle(N, K, d, dt), WS_CELLS, 0, nullptr).bytes; }

int score_links_count(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* exr, const int32_t* exc,
                      float min_logit, const dl_node_filter* nf, void* ws, int64_t* rowptr, hipStream_t st) {
    const Plan p = triangle(N, K, d, dt);
    const Ws w = carve(p, WS_CELLS, 0, ws);
    const Rule r = rule_of(nf);
    if (p.pairs > 0) split_tables(p, w, Tables{Z, H, nullptr, nullptr}, st);
    ScanArgs a = scan_args(p, w, t, exr, exc, min_logit, r);
    count_links<DEG>(p, w, a, r.on, rowptr, nullptr, st);
    return check_launch("score_links_count");
}

int score_links_fill(dl_dtype dt, int N, int K, int d, float t, const int32_t* exr, const int32_t* exc, float min_logit,
                     const dl_node_filter* nf, void* ws, const int64_t* rowptr, long long nnz, int32_t* col, float* logit, float* prob,
                     hipStream_t st) {
    const Plan p = triangle(N, K, d, dt);
    const Ws w = carve(p, WS_CELLS, 0, ws);
    const Rule r = rule_of(nf);
    ScanArgs a = scan_args(p, w, t, exr, exc, min_logit, r);
    fill_links<FILL>(p, a, r.on, LinkArgs{w.cnt_a, rowptr, nnz, col, logit, prob}, LinkArgs{}, st);
    return check_launch("score_links_fill");
}

// ---- dl_score_links_top: the m best candidates as that CSR — the select of score_mine (no EMIT, no ordering), then the link
// scans under the threshold key it left on the device
// out = the fields of score_links_form with scans at most = digits + count + fill, then the byte offset of the 32-bit count
// of HISTOGRAM scans that ran inside the (256-byte aligned) workspace
void score_links_top_form(int N, int d, int* out) {
    score_links_form(N, d, out);
    out[5] = out[2] > 0 ? PASSES + 2 : 0;
    out[7] = (int)offsetof(State, scans);
}

size_t score_links_top_workspace_bytes(int N, int K, int d, dl_dtype dt) {
    return carve(triangle(N, K, d, dt), WS_SELECT | WS_CELLS, 0, nullptr).bytes;
}

int score_links_top_count(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* exr,
                          const int32_t* exc, float min_logit, long long m, const dl_node_filter* nf, void* ws, int64_t* rowptr,
                          hipStream_t st) {
    const Plan p = triangle(N, K, d, dt);
    const Ws w = carve(p, WS_SELECT | WS_CELLS, 0, ws);
    const Rule r = rule_of(nf);
    // a budget above all pairs means every candidate; what is left fits the select's 32-bit counts (N <= 46,340)
    const long long all = (long long)N * (N - 1) / 2;
    const int need = (int)(m < all ? m : all);
    static_assert((long long)DL_SCORE_LINKS_MAX_N * (DL_SCORE_LINKS_MAX_N - 1) / 2 <= 2147483647LL, "pairs fit the select's need");
    ScanArgs a = scan_args(p, w, t, exr, exc, min_logit, r);
    select(p, w, Tables{Z, H, nullptr, nullptr}, a, need, r.on, st);
    count_links<DEG_TOP>(p, w, a, r.on, rowptr, nullptr, st);
    return check_launch("score_links_top_count");
}

int score_links_top_fill(dl_dtype dt, int N, int K, int d, float t, const int32_t* exr, const int32_t* exc, float min_logit,
                         const dl_node_filter* nf, void* ws, const int64_t* rowptr, long long nnz, int32_t* col, float* logit,
                         float* prob, hipStream_t st) {
    const Plan p = triangle(N, K, d, dt);
    const Ws w = carve(p, WS_SELECT | WS_CELLS, 0, ws);
    const Rule r = rule_of(nf);
    ScanArgs a = scan_args(p, w, t, exr, exc, min_logit, r);
    a.state = w.state;                                          // the threshold the count's select left
    fill_links<FILL_TOP>(p, a, r.on, LinkArgs{w.cnt_a, rowptr, nnz, col, logit, prob}, LinkArgs{}, st);
    return check_launch("score_links_top_fill");
}

// ---- dl_score_mine_between / dl_score_links_between: rows of a table A against rows of a table B (the RECT instantiations).
// The same passes over the ntA x ntB grid of tile pairs, the pair index a nB + b local to the rectangle; a graph past the cap
// of the triangular walk is the union of its diagonal blocks (the entries above on row slices) and of such rectangles, merged
// by the caller (scans.py).
// out = nd, tiles of A, tiles of B, tile pairs, tile pairs per workgroup, workgroups of a scan, scans at most (digits + emit),
// byte offset of the 32-bit count of scans that ran inside the (256-byte aligned) workspace
void score_mine_between_form(int nA, int nB, int d, int* out) {
    plan_form(rectangle(nA, nB, 0, d), out);
    out[6] = PASSES + 1;
    out[7] = (int)offsetof(State, scans);
}

size_t score_mine_between_workspace_bytes(int nA, int nB, int K, int d, int m, dl_dtype dt) {
    return carve(rectangle(nA, nB, K, d, dt), WS_SELECT, (size_t)m, nullptr).bytes;
}

int score_mine_between(const void* ZA, const void* HA, const void* ZB, const void* HB, dl_dtype dt, int nA, int nB, int K, int d, float t,
                       const int32_t* exr, const int32_t* exc, float min_logit, int m, int32_t* src, int32_t* dst, float* logit,
                       float* prob, int64_t* count, void* ws, hipStream_t st, const dl_node_filter_between* nf) {
    return mine_pairs("score_mine_between", rectangle(nA, nB, K, d, dt), Tables{ZA, HA, ZB, HB}, t, exr, exc, min_logit, m, rule_of(nf),
                      src, dst, logit, prob, count, ws, st);
}

// out = the first six fields of score_mine_between_form, scans of count + fill, cells of the A side, cells of the B side
void score_links_between_form(int nA, int nB, int d, int* out) {
    score_mine_between_form(nA, nB, d, out);
    out[6] = 2;
    out[7] = nA * out[2];                                       // <= 46,340 * 363
    out[8] = nB * out[1];
}

size_t score_links_between_workspace_bytes(int nA, int nB, int K, int d, dl_dtype dt) {
    return carve(rectangle(nA, nB, K, d, dt), WS_CELLS, 0, nullptr).bytes;
}

int score_links_between_count(const void* ZA, const void* HA, const void* ZB, const void* HB, dl_dtype dt, int nA, int nB, int K, int d,
                              float t, const int32_t* exr, const int32_t* exc, float min_logit, const dl_node_filter_between* nf,
                              void* ws, int64_t* rowptr_a, int64_t* rowptr_b, hipStream_t st) {
    const Plan p = rectangle(nA, nB, K, d, dt);
    const Ws w = carve(p, WS_CELLS, 0, ws);
    const Rule r = rule_of(nf);
    split_tables(p, w, Tables{ZA, HA, ZB, HB}, st);
    ScanArgs a = scan_args(p, w, t, exr, exc, min_logit, r);
    count_links<DEG>(p, w, a, r.on, rowptr_a, rowptr_b, st);
    return check_launch("score_links_between_count");
}

int score_links_between_fill(dl_dtype dt, int nA, int nB, int K, int d, float t, const int32_t* exr, const int32_t* exc, float min_logit,
                             const dl_node_filter_between* nf, void* ws, const int64_t* rowptr_a, const int64_t* rowptr_b,
                             long long nnz_a, int32_t* col_a, float* logit_a, float* prob_a, long long nnz_b, int32_t* col_b,
                             float* logit_b, float* prob_b, hipStream_t st) {
    const Plan p = rectangle(nA, nB, K, d, dt);
    const Ws w = carve(p, WS_CELLS, 0, ws);
    const Rule r = rule_of(nf);
    ScanArgs a = scan_args(p, w, t, exr, exc, min_logit, r);
    fill_links<FILL>(p, a, r.on, LinkArgs{w.cnt_a, rowptr_a, nnz_a, col_a, logit_a, prob_a},
                     LinkArgs{w.cnt_b, rowptr_b, nnz_b, col_b, logit_b, prob_b}, st);
    return check_launch("score_links_between_fill");
}

}  // namespace dl
