// Routing: exp-Gram softmax over K, first-max arg-max per edge, row sums of the winning weights (model.py:56-72).
// (one of the tuned-kernel translation units; the shared pieces and the design notes are in dl_fast.h)
#include "dl_fast.h"
#include "dl_hub.h"

namespace dl {
namespace fast {

// ---------------------------------------------------------------------------- route
// p[e], a[e] for the entries of the plan's segments.  MIRROR: the plan covers col >= row only and
// every result is also written to the reverse entry (routing is symmetric, bitwise).
template <int K, int D, typename T, bool MIRROR>
__global__ __launch_bounds__(BLOCK, (K <= 8 && sizeof(T) == 4) ? 8 : (K <= 10 ? 6 : (K <= 16 ? 4 : 1))) void route_seg_kernel(dl_csr_plan g, const int32_t* __restrict__ rev,
                                                          const T* __restrict__ Z, float t,
                                                          uint8_t* __restrict__ p, float* __restrict__ a) {
    using GE = Geo<K, D, T>;
    using FL = typename GE::FL;
    constexpr int VEC = GE::VEC, G = GE::G, EPW = GE::EPW, KP = FL::KP, VPL = FL::VPL;
    const WaveSeg ws = load_wave_seg(g);
    if (!ws.active) return;
    const SegInfo si = ws.si;
    const int lane = lane_id();
    const int c = lane % G, grp = lane / G;
    const int kb = FL::factor_base(c);

    Chunk<VEC> zi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) zi[k] = Tab<T>::load(Z + (size_t)si.grow * GE::ROW + k * D + c * VEC);

    int my_col = si.grow, my_rev = 0;
    if (si.beg + lane < si.end) {
        my_col = g.col[si.beg + lane];
        if (MIRROR) my_rev = rev[si.beg + lane];
    }
    for (int base = si.beg; base < si.end; base += EPW) {
        const int e = base + grp;
        const bool live = e < si.end;
        const int j = entry_scalar<EPW>(my_col, base - si.beg, grp);
        float part[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k)
            part[k] = k < K ? dot(zi[k < K ? k : 0], Tab<T>::load(Z + (size_t)j * GE::ROW + (k < K ? k : 0) * D + c * VEC))
                            : 0.0f;
        float ex[VPL];
        const float S = lane_exps<K, G>(part, c, t, ex);
        float best = 0.0f;
        int win = 255;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const float al = ex[i] / S;
            if (kb + i < K && (win == 255 || beats(al, best))) { best = al; win = kb + i; }
        }
        group_argmax_first<G>(best, win);             // (an arg-max by wave ballots measured slower, round 4)
        if (MIRROR) {
            const int r = entry_scalar<EPW>(my_rev, base - si.beg, grp);
            if (live && c == 0) { p[e] = (uint8_t)win; a[e] = best; }
            if (live && c == 1 % G && r != e) { p[r] = (uint8_t)win; a[r] = best; }
        } else {
            if (live && c == 0) { p[e] = (uint8_t)win; a[e] = best; }
        }
    }
}

// ---------------------------------------------------------------------------- route over a hub plan
// The kernel above gathers one whole Z row per entry with col >= row and is bound by those bytes (15.6 TB/s out of the L2 on
// squirrel).  On a skewed graph most of them are repeats: the routing hub plan (dl_graph.route_hub, graph.py) hands every
// undirected edge to its endpoint of larger degree, cuts those owners into blocks of 16 rows, and a workgroup that holds a
// block's Z rows in LDS (32 KB at K = 8) gathers a partner row ONCE for up to four of them.  Item, staging, walk and batch
// counter are those of every kernel over a hub plan (dl_hub.h, with the plan contract); the step is that of
// hub::score_fwd_wave_kernel (dl_score.h) on one table: scalar row bases, every gather of a step issued before the first
// wait, a chunk's LDS reads issued together.
// Lane l holds float4 number j * 64 + l of a row: a DPP row of 16 lanes is one factor slice (factor 4 j + r, r = l >> 4), and
// lane i of it holds the elements 4 i .. 4 i + 3 — the elements lane c = i of a group holds in the kernel above.
// Bits.  A pair's results are those of the kernel above, operation for operation:
//   - the partial of (factor, lane) is dl::fast::dot — x0 * y0, then three fmaf; symmetric in its rows, so it does not
//     matter which endpoint is the block row;
//   - the 16 partials of a factor are added by the butterfly in stage order 8, 4, 2, 1 (TransposedReduce: the same tree
//     whichever value index a sum sits at; an add's operands may swap sides, IEEE addition commutes);
//   - S = group_allreduce_sum<16> over the primary lanes there adds the factors as ((e_f + e_f^4) + (e_f^2 + e_f^6)) +
//     ((e_f^1 + e_f^5) + (e_f^3 + e_f^7)) at K = 8 and (e_f + e_f^2) + (e_f^1 + e_f^3) at K = 4, then zeros; here factor
//     bit 2 is the chunk (lane ^ 8), bit 1 the DPP row pair (lane ^ 32), bit 0 the DPP row (lane ^ 16): the same tree;
//   - al = ex / S is the IEEE division, and the winner is the first maximal QUOTIENT under `beats` (a total preorder with
//     ties to the lower factor: which lanes are compared in which order cannot change the winner).
// A step ends at its reduction: 16 / NVAL = NB lanes of a DPP row then hold the same sum, so the wave keeps the sums of NB of
// its steps side by side — lane i keeps those of the batch's step number i & (NB - 1) — and runs ONE tail (expf, S, division,
// arg-max, stores) per NB steps and one behind its last step; none of the tail's exchanges (lane ^ 8, ^ 16, ^ 32) crosses
// these lanes.  The chunk-0 lanes of DPP row 0 store (p, a) at the entry, those of row 1 at the reverse entry (-1: a self-loop,
// or a dead slot), at indices they read per lane from the plan when the batch opened.  The base name is that of the kernel above on purpose: the per-phase accounting of
// the benchmark matches kernels by base name.
namespace hub {
constexpr bool route_shape_ok(int K, int D) { return D == 64 && (K == 4 || K == 8); }
template <int K, int D>
struct RouteGeo {
    static constexpr bool ok = route_shape_ok(K, D);
    static constexpr int NJ = K * D / 256;            // float4 of a row per lane (chunks)
    static constexpr int NVAL = 4 * NJ;               // partial dot products per lane and step: index = chunk * 4 + slot
    static constexpr int SH = K == 8 ? 1 : 2;         // 1 << SH = 16 / NVAL lanes of a DPP row end up with the same sum
};
// waves per SIMD the register allocation aims at: 71 registers, three workgroups per CU.  Pinned at 4 / 6 / 8 (8: 64 registers,
// no scratch) route_fwd alone takes 27.4 / 25.8 / 26.2 us on squirrel at one slice, and the per-step tail instead of the batched
// one 27.9 (profiles/r14_route_hub.txt)
constexpr int ROUTE_MAXW = 6;

struct RouteWords { dl_vi4 v, u; };                   // the plan words a step runs on: partner rows and u_local of its four slots

__device__ __forceinline__ float dot4_chain(const float4& x, const float4& y) {      // dl::fast::dot on float4
    float r = x.x * y.x;
    r = fmaf(x.y, y.y, r);
    r = fmaf(x.z, y.z, r);
    return fmaf(x.w, y.w, r);
}

// one exchange of the first-max arg-max: every lane holds a candidate (of a different factor than its partner lane's), both
// lanes of a pair end with the same one.  `beats`, written without short-circuits: selects, no branches.
template <int OFF>
__device__ __forceinline__ void argmax_xor(float& best, int& win) {
    const float ob = xor_lane<OFF>(best);
    const int ow = xor_lane_i<OFF>(win);
    const bool o_nan = ob != ob, b_nan = best != best;
    const bool o_beats = (ob > best) | (o_nan & !b_nan), b_beats = (best > ob) | (b_nan & !o_nan);
    const bool take = o_beats | (!b_beats & (ow < win));
    best = take ? ob : best;
    win = take ? ow : win;
}

template <int K, int D, bool T1>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, ROUTE_MAXW))) void route_seg_kernel(
    dl_pair_hub h, const float* __restrict__ Z, float t, uint8_t* __restrict__ p, float* __restrict__ a) {
    using RG = RouteGeo<K, D>;
    constexpr int NJ = RG::NJ, NVAL = RG::NVAL, SH = RG::SH, ROW = K * D, R4 = ROW / 4;      // R4: float4 of one Z row
    static_assert(RG::ok, "one DPP row of 16 lanes per factor slice, one or two chunks");
    __shared__ __attribute__((aligned(16))) float4 urow[DL_HUB_W * R4];
    int it;
    if (!workgroup_item<true>(h, it)) return;                        // (a routing plan has one stream of items)
    const int wave = wave_index(), lane = lane_id();
    const int i = lane & 15, r = lane >> 4;
    const int blk = h.item_block[it];                                // asked for first: block, rows, LDS is the chain to the barrier
    const ItemSteps st = item_steps(h, it);
    auto fetch = [&](const int step) {
        const int s = __builtin_amdgcn_readfirstlane(step);
        RouteWords w;
        w.v = plan_words(h.step_v, s), w.u = plan_words(h.step_u, s);
        return w;
    };
    // after the reduction lane i of a DPP row holds the sum number i >> SH = chunk * 4 + slot of its row's factors
    constexpr int NB = 1 << SH;                                      // steps per batch
    const int e_me = (i >> SH) & 3;                                  // this lane's slot
    const int k_me = 4 * (i >> (SH + 2)) + r;                        // and factor (chunk j holds the factors 4 j + r)
    const int b_me = i & (NB - 1);                                   // and step of the batch
    const bool writer = (i >> (SH + 2)) == 0 && r < 2;               // chunk 0 of row 0: the entry, of row 1: the reverse entry
    // the pending sums of up to NB of the wave's steps (s0, s0 + 8, ...).  The store indices of a batch are asked for per
    // lane when it opens and are there long before the flush.
    float sg = 0.0f;
    int dst = -1;
    Batch<NB, false> batch;
    const int32_t* const my_q = r == 0 ? h.step_q : h.step_q2;
    auto open = [&](const int s0) {
        const int sb = s0 + WAVES * b_me;
        dst = -1;
        if (writer && sb < st.end) dst = my_q[4 * sb + e_me];
    };
    auto flush = [&]() {                                             // one tail for the whole batch
        const float ex = expf(T1 ? sg : sg / t);
        float S = ex;
        if constexpr (NJ == 2) S = add_xor<8>(S);
        S = add_xor<16>(add_xor<32>(S));
        float best = ex / S;
        int win = k_me;
        if constexpr (NJ == 2) argmax_xor<8>(best, win);
        argmax_xor<32>(best, win);
        argmax_xor<16>(best, win);
        if (dst >= 0) {                                              // -1: no writer lane, a dead slot, no reverse entry, no step
            p[dst] = (uint8_t)win;
            a[dst] = best;
        }
    };
    auto do_step = [&](const RouteWords& w, auto shape, auto last) {
        constexpr int NV = decltype(shape)::value;                   // gathered partner rows: 4 (A), 2 (B), 1 (C)
        constexpr bool LAST = decltype(last)::value;                 // dead partner rows: dl_hub.h
        const int sv[4] = {w.v.x, w.v.y, w.v.z, w.v.w}, su[4] = {w.u.x, w.u.y, w.u.z, w.u.w};
        float4 zv[NV][NJ];
#pragma unroll
        for (int n = 0; n < NV; ++n) {
            if (!LAST || sv[n] >= 0) {                               // wave-uniform
                const auto* zr = uniform_row<dl_vf4>(Z, (size_t)(unsigned)sv[n] * ROW * sizeof(float));
#pragma unroll
                for (int j = 0; j < NJ; ++j) zv[n][j] = as_float4(zr[(unsigned)(lane + j * 64)]);
            } else {
#pragma unroll
                for (int j = 0; j < NJ; ++j) zv[n][j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        float val[NVAL];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float4 u4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) u4[e] = urow[(su[e] & (DL_HUB_W - 1)) * R4 + j * 64 + lane];      // this slot's own u row
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) val[j * 4 + e] = dot4_chain(u4[e], zv[e * NV / 4][j]);
            __builtin_amdgcn_sched_barrier(0);
        }
        TransposedReduce<NVAL, 8>::run(val, i);
        sg = b_me == batch.nb ? val[0] : sg;                         // the lanes of this step's place in the batch keep it
        ++batch.nb;
    };
    // The words of the wave's first step and the store indices of its first batch are requested with the block's rows, ahead
    // of the staging loads — not behind the barrier.
    const int s = st.a + wave;
    RouteWords nxt = {};
    if (s < st.end) nxt = fetch(s);
    open(s);
    stage_block<NJ, 1>((lds_vf4*)urow, h, blk, wave, lane, {Z});
    __syncthreads();                                                 // the only one: nothing below waits for another wave
    walk(s, st, nxt, fetch, [&](const RouteWords& w, const int step, auto shape, auto last) {
        do_step(w, shape, last);
        batch.tick(step, flush, open);
    });
    batch.close(flush);
}
}  // namespace hub

// s[i][k] = sum_{e in row i, p[e]=k} a[e] (raw; model.py:70-71).  Four LANES per segment position (a wavefront per
// segment would leave most lanes idle and spend its time in K all-reduces; one thread per segment walks 32 entries in
// eight dependent round trips): lane `sub` of a position adds the entries sub, sub + 4, ... of the segment in order and
// keeps the K sums in registers; the four lanes are then added as (0 + 1) + (2 + 3), and the (<= 4) positions of a unit —
// one aligned group of 16 lanes, a DPP row — in segment order by the unit's first position.  All exchanges are DPP
// (quad_perm, row_shl): no LDS.  KP = K rounded up to 4 / 8 / 16 / 32.
constexpr int ROWSUM_SUB = 4;                                   // lanes per segment position
constexpr int ROWSUM_POS_PER_BLOCK = BLOCK / ROWSUM_SUB;

template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_move_i(int v) {
    return __builtin_amdgcn_update_dpp(-1, v, CTRL, 0xF, 0xF, false);     // lanes shifted in from outside the row keep -1
}

//
// Rows of SEVERAL units (slot >= 0; more than DL_UNIT_SEGS segments) are not summed from their units at all (round 2
// wrote one partial per unit and launched a combine kernel for a handful of rows: 5 us of launch for microseconds of
// work): the workgroups behind the first n_reg_blocks take one such row per WAVE — lane l adds the entries l, l + 64,
// ... of the row in order (loads in batches of four), then the 64 lanes are added by the wave butterfly.  One launch;
// the order depends on the row alone.
template <int KP>
__global__ __launch_bounds__(BLOCK) void s_rowsum_thread_kernel(dl_csr_plan g, int K, const uint8_t* __restrict__ p,
                                                                const float* __restrict__ a, float* __restrict__ s,
                                                                int n_reg_blocks) {
    if ((int)blockIdx.x >= n_reg_blocks) {
        const int m = ((int)blockIdx.x - n_reg_blocks) * WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);
        if (m >= g.n_multi) return;
        const int lane = lane_id();
        const int row = g.multi_row[m];
        const int beg = g.rowptr[row], end = g.rowptr[row + 1];
        float acc[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[k] = 0.0f;
        for (int e = beg + lane; e < end; e += 4 * DL_WAVE) {
            int k[4];
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = min(e + j * DL_WAVE, end - 1);
                k[j] = e + j * DL_WAVE < end ? (int)p[i] : 255;
                v[j] = a[i];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int kk = 0; kk < KP; ++kk) acc[kk] += k[j] == kk ? v[j] : 0.0f;
        }
        float mine = 0.0f;
#pragma unroll
        for (int kk = 0; kk < KP; ++kk) {
            const float tot = wave_allreduce_sum(acc[kk]);
            if (lane == kk) mine = tot;
        }
        if (lane < K) s[((size_t)row + g.row_offset) * K + lane] = mine;
        return;
    }
    const int seg = blockIdx.x * ROWSUM_POS_PER_BLOCK + (int)(threadIdx.x / ROWSUM_SUB);
    const int sub = threadIdx.x % ROWSUM_SUB;
    const int row = seg < g.n_seg ? g.seg_row[seg] : -1;
    int beg = 0, end = 0, slot = -1;
    if (row >= 0) { beg = g.seg_beg[seg]; end = g.seg_end[seg]; slot = g.seg_slot[seg]; }
    if (slot >= 0) beg = end = 0;                                 // a row of several units: summed by its own wave (above)
    float acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.0f;
    for (int e = beg + sub; e < end; e += 4 * ROWSUM_SUB) {     // four entries in flight per lane (clamped loads), added in order
        int k[4];
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = min(e + j * ROWSUM_SUB, end - 1);
            k[j] = e + j * ROWSUM_SUB < end ? (int)p[i] : 255;
            v[j] = a[i];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int kk = 0; kk < KP; ++kk) acc[kk] += k[j] == kk ? v[j] : 0.0f;
    }
    // segment sum over the four lanes of the position: (0 + 1) + (2 + 3), every lane of the quad gets it
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) acc[kk] = add_xor<2>(add_xor<1>(acc[kk]));
    // unit sum: the 4 positions of a workgroup-sized group are the 4 quads of one DPP row; a unit is a run of equal rows
    // among them, added in segment order by its first position (row_shl:4q brings quad +q)
    const int pos_in_grp = (threadIdx.x / ROWSUM_SUB) % WAVES_PER_BLOCK;
    // (a unit = same row AND same slot: plans with one segment per unit give every segment of a row its own slot)
    const int prev_row = dpp_move_i<0x114>(row);                 // row_shr:4: the previous position's row (-1 at the group's start)
    const int prev_slot = dpp_move_i<0x114>(slot);
    const bool head = row >= 0 && (pos_in_grp == 0 || prev_row != row || prev_slot != slot);
    const int r1 = dpp_move_i<0x104>(row), r2 = dpp_move_i<0x108>(row), r3 = dpp_move_i<0x10C>(row);   // row_shl:4 / 8 / 12
    const int t1 = dpp_move_i<0x104>(slot), t2 = dpp_move_i<0x108>(slot), t3 = dpp_move_i<0x10C>(slot);
    const bool ok1 = r1 == row && t1 == slot, ok2 = ok1 && r2 == row && t2 == slot, ok3 = ok2 && r3 == row && t3 == slot;
    float tot[KP];
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
        const float v1 = dpp_move<0x104>(acc[kk]), v2 = dpp_move<0x108>(acc[kk]), v3 = dpp_move<0x10C>(acc[kk]);
        tot[kk] = acc[kk];
        tot[kk] += ok1 ? v1 : 0.0f;
        tot[kk] += ok2 ? v2 : 0.0f;
        tot[kk] += ok3 ? v3 : 0.0f;
    }
    if (!head || sub != 0 || slot >= 0) return;
    float* dst = s + ((size_t)row + g.row_offset) * K;
#pragma unroll
    for (int kk = 0; kk < KP; ++kk)
        if (kk < K) dst[kk] = tot[kk];
}

// Per multi-segment row: out[grow][k] = f(sum of the K-vectors of its slots, in slot order).
// One wave per row: lane handles factor k = lane % KP of slot (lane / KP), stride 64/KP.
// mode 0: plain sum (s);  mode 1: ds_from_acc(sum, s_raw[grow][k]) (normaliser gradient).
__global__ __launch_bounds__(BLOCK) void vec_combine_kernel(dl_csr_plan g, int K, int KP,
                                                            const float* __restrict__ part, int mode,
                                                            const float* __restrict__ s_raw,
                                                            float* __restrict__ out) {
    const int m = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (m >= g.n_multi) return;
    const int lane = lane_id();
    const int k = lane % KP, sl = lane / KP, step = DL_WAVE / KP;
    float acc = 0.0f;
    if (k < K)
        for (int slot = g.multi_slot0[m] + sl; slot < g.multi_slot0[m + 1]; slot += step)
            acc += part[(size_t)slot * K + k];
    for (int off = KP; off < DL_WAVE; off <<= 1) acc += __shfl_xor(acc, off, DL_WAVE);
    if (lane < K) {
        const size_t o = ((size_t)g.multi_row[m] + g.row_offset) * K + lane;
        out[o] = mode == 0 ? acc : ds_from_acc(acc, s_raw[o]);
    }
}

static void launch_s_rowsum(const dl_csr_plan* g, int K, const uint8_t* p, const float* a, float* s, hipStream_t st) {
    if (g->n_seg <= 0) return;
    const int reg = (g->n_seg + ROWSUM_POS_PER_BLOCK - 1) / ROWSUM_POS_PER_BLOCK;
    const dim3 grid((unsigned)reg + wave_blocks(g->n_multi)), block(BLOCK);
    if (K <= 4) hipLaunchKernelGGL(s_rowsum_thread_kernel<4>, grid, block, 0, st, *g, K, p, a, s, reg);
    else if (K <= 8) hipLaunchKernelGGL(s_rowsum_thread_kernel<8>, grid, block, 0, st, *g, K, p, a, s, reg);
    else if (K <= 16) hipLaunchKernelGGL(s_rowsum_thread_kernel<16>, grid, block, 0, st, *g, K, p, a, s, reg);
    else hipLaunchKernelGGL(s_rowsum_thread_kernel<32>, grid, block, 0, st, *g, K, p, a, s, reg);   // tuned shapes: K <= 32
}

void launch_vec_combine(const dl_csr_plan* g, int K, const float* part, int mode, const float* s_raw,
                        float* out, hipStream_t st) {
    if (g->n_multi <= 0) return;
    hipLaunchKernelGGL(vec_combine_kernel, dim3(wave_blocks(g->n_multi)), dim3(BLOCK), 0, st, *g, K, pow2_at_least(K),
                       part, mode, s_raw, out);
}

template <int K, int D, typename T>
struct RouteOps {
    // `route`: the (possibly sliced / upper-triangle) plan the routing kernel walks, NULL = g itself;
    // mirror: it covers col >= row only and every result is also written through rev
    // hp: the routing hub plan (every entry with col >= row, both directions written), NULL = none
    static int route_fwd(const dl_csr_plan* g, const dl_csr_plan* route, bool mirror, const int32_t* rev,
                         const dl_pair_hub* hp, const void* Z, float t, uint8_t* p, float* a, float* s, float* s_part,
                         hipStream_t st) {
        if constexpr (std::is_same<T, float>::value && hub::RouteGeo<K, D>::ok) {
            if (hp != nullptr) {
                const dim3 grid((unsigned)hp->n_slices * (unsigned)hp->slice_max_item), block(hub::THREADS);
                if (t == 1.0f)
                    hipLaunchKernelGGL((hub::route_seg_kernel<K, D, true>), grid, block, 0, st, *hp, (const float*)Z, t, p, a);
                else
                    hipLaunchKernelGGL((hub::route_seg_kernel<K, D, false>), grid, block, 0, st, *hp, (const float*)Z, t, p, a);
                launch_s_rowsum(g, K, p, a, s, st);
                return check_launch("route_fwd(fast, hub blocks)");
            }
        }
        const dl_csr_plan* rp = route ? route : g;
        if (mirror)
            hipLaunchKernelGGL((route_seg_kernel<K, D, T, true>), dim3(seg_blocks(rp)), dim3(BLOCK), 0, st, *rp, rev,
                               (const T*)Z, t, p, a);
        else
            hipLaunchKernelGGL((route_seg_kernel<K, D, T, false>), dim3(seg_blocks(rp)), dim3(BLOCK), 0, st, *rp, rev,
                               (const T*)Z, t, p, a);
        (void)s_part;
        launch_s_rowsum(g, K, p, a, s, st);
        return check_launch("route_fwd(fast)");
    }
};

}  // namespace fast

bool fast_supported(int K, int d, int dtype) {
#define X(KK, DD) if (K == KK && d == DD) return true;
    if (dtype == DL_F32) { DL_FAST_SHAPES_F32(X) }
    if (dtype == DL_BF16) { DL_FAST_SHAPES_BF16(X) }
#undef X
    return false;
}

// the shapes hub::route_seg_kernel is instantiated for (those of the hub scorer)
bool fast_route_hub_supported(int K, int d, int dtype) { return dtype == DL_F32 && fast::hub::route_shape_ok(K, d); }

int fast_route_fwd(const dl_csr_plan* g, const dl_csr_plan* route, bool mirror, const int32_t* rev, const dl_pair_hub* hub,
                   const void* Z, int K, int d, int dtype, float t, uint8_t* p, float* a, float* s, float* s_part,
                   hipStream_t st) {
#define X_F32(KK, DD) \
    if (K == KK && d == DD) return fast::RouteOps<KK, DD, float>::route_fwd(g, route, mirror, rev, hub, Z, t, p, a, s, s_part, st);
#define X_BF16(KK, DD)      \
    if (K == KK && d == DD) \
        return fast::RouteOps<KK, DD, fast::bf16_t>::route_fwd(g, route, mirror, rev, hub, Z, t, p, a, s, s_part, st);
    DL_DISPATCH(X)
#undef X_F32
#undef X_BF16
}

}  // namespace dl
