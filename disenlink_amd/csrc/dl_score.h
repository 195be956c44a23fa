// Pair scorer (model.py:109-113 on a pair list), the gather-form dense scorer, and the separate scorer backward: the kernels and
// their launch choice.  Instantiated by dl_score.hip (probability space) and by dl_pair_logits.hip (logit space).
// (the shared pieces and the design notes are in dl_fast.h)
#pragma once
#include "dl_fast.h"
#include "dl_hub.h"
#include "dl_score_bwd.h"

namespace dl {
namespace fast {

// One wave per segment of the "pairs by first endpoint" plan: the u rows of Z and H are staged once
// in LDS, every lane group then scores one pair per iteration from the gathered v rows.
// LOGIT (dl_score_pairs_logits_fwd; the forms without stored terms): `prob` receives the logit, not its sigmoid — in this
// kernel, the wave-per-entry kernel and the hub kernel below; nothing else differs, so a pair's logit is the value the
// probability form feeds its sigmoid.
template <int K, int D, typename T, bool COEF, bool LOGIT = false>
// (4 waves per SIMD: pinned at 5 / 6 / 8 hipcc keeps fewer row gathers in flight per wave — 301 / 543 / 612 us against
// 170 on squirrel; whether the u rows sit in registers or are re-read from LDS every iteration makes no difference:
// the kernel is bound by the vector-L1 / L2 pipeline, 4.3 GB through 256 x 64 B/clk.)
__global__ __launch_bounds__(BLOCK, K <= 8 ? 4 : 1) void score_fwd_seg_kernel(dl_csr_plan g, const int32_t* __restrict__ pair_id,
                                                              const int32_t* __restrict__ pair_id2,
                                                              const T* __restrict__ Z, const T* __restrict__ H,
                                                              float t, float* __restrict__ prob,
                                                              float* __restrict__ coef_e,
                                                              float* __restrict__ coef_q) {
    using GE = Geo<K, D, T>;
    constexpr int VEC = GE::VEC, G = GE::G, EPW = GE::EPW, ROW = GE::ROW;
    constexpr int KB = K > 8 ? 8 : K;                        // factor block
    using FLB = FactorLanes<G, KB>;
    constexpr int KBP = FLB::KP;
    __shared__ __attribute__((aligned(16))) float urow[WAVES_PER_BLOCK][2 * ROW];
    const WaveSeg ws = load_wave_seg(g);
    const SegInfo si = ws.si;
    const int wave = ws.wave, lane = lane_id();
    const bool active = ws.active;
    if (active) stage_u_rows<K, D, T>(urow[wave], Z, H, (size_t)si.grow);
    __syncthreads();
    if (!active) return;
    const int c = lane % G, grp = lane / G;
    const int kbb = FLB::factor_base(c);
    int my_col = si.grow, my_pair = 0, my_pair2 = -1;                // pair_id2: the mirrored pair an entry also scores (-1 = none)
    if (si.beg + lane < si.end) {
        my_col = g.col[si.beg + lane];
        my_pair = pair_id[si.beg + lane];
        if (pair_id2 != nullptr) my_pair2 = pair_id2[si.beg + lane];
    }
    for (int base = si.beg; base < si.end; base += EPW) {
        const int it = base + grp;
        const bool live = it < si.end;
        const size_t v = (size_t)entry_scalar<EPW>(my_col, base - si.beg, grp);
        const int q = entry_scalar<EPW>(my_pair, base - si.beg, grp);
        const int q2 = entry_scalar<EPW>(my_pair2, base - si.beg, grp);
        // factors are processed in blocks of KB <= 8: at most 2*KB row chunks live at a time, whatever K is
        float term = 0.0f;
#pragma unroll
        for (int b0 = 0; b0 < K; b0 += KB) {
            float pq[KBP], ps[KBP];
#pragma unroll
            for (int k = 0; k < KBP; ++k) {
                const bool in = k < KB && b0 + k < K;
                const int kk = in ? b0 + k : 0;
                pq[k] = in ? dot(load_f32<VEC>(&urow[wave][ROW + kk * D + c * VEC]), Tab<T>::load(H + v * ROW + kk * D + c * VEC)) : 0.0f;
                ps[k] = in ? dot(load_f32<VEC>(&urow[wave][kk * D + c * VEC]), Tab<T>::load(Z + v * ROW + kk * D + c * VEC)) : 0.0f;
            }
            TransposedReduce<KBP, G / 2>::run(pq, c);
            TransposedReduce<KBP, G / 2>::run(ps, c);
#pragma unroll
            for (int i = 0; i < FLB::VPL; ++i) {
                const int k = b0 + kbb + i;
                if (FLB::primary(c) && kbb + i < KB && k < K) {
                    const float ek = expf(div_t(ps[i], t));
                    const float qe = pq[i] * ek;
                    term += qe;
                    if (COEF && live) {                         // per-factor logit terms for the backward
                        coef_e[(size_t)q * K + k] = ek;
                        coef_q[(size_t)q * K + k] = qe;
                        if (q2 >= 0) {
                            coef_e[(size_t)q2 * K + k] = ek;
                            coef_q[(size_t)q2 * K + k] = qe;
                        }
                    }
                }
            }
        }
        const float logit = group_allreduce_sum<G>(term);
        if (live && c == 0) {
            const float p = LOGIT ? logit : sigmoid_ref(logit);
            prob[q] = p;
            if (q2 >= 0) prob[q2] = p;
        }
    }
}

// ---------------------------------------------------------------------------- forward scorer, wave per entry (round 6)
// The forward pass in the geometry of the one-pass training scorer (dl_train.h: score_train_wave_kernel) for d = 64,
// K in {4, 8}, fp32 tables: the 64 lanes share ONE pair, lane l holds float4 number j * 64 + l of a row (a DPP row of 16
// lanes = one factor slice), the row base is a scalar (readlane of the segment's columns) and the lane offset a constant,
// the u rows are re-read from the wave's LDS region every step, U = 4 pairs per step, the 16 partial dot products reduced
// over the DPP row by one transposed reduction: one expf and one sigmoid per step.  No accumulators, so fewer registers
// than the training kernel; the arithmetic up to the probability is that kernel's, operation for operation — the two give the
// same bits.  The group-per-entry kernel above stays for every other shape (and as the reference form: DL_FWD_GROUP_KERNEL=1).
// Why: the training kernel's bound build ran these very gathers, without arithmetic, at 0.86 of the L2 peak; the
// group-per-entry forward reached 0.79.
constexpr int FWD_WAVE_MAXW = 6;      // waves per SIMD the register allocation aims at (4 / 5 / 6 measured: 156.6 / 156.8 / 154.4 us, profiles/r7n_*)
template <int K, int D>
struct FwdWave {
    static constexpr bool ok = D == 64 && (K == 4 || K == 8);
    static constexpr int NJ = K * D / 256, U = 4;
};

// (amdgpu_waves_per_eu(4, 5): left to itself hipcc aims at 8 waves per SIMD = 64 registers — exactly the 16 gathered float4 of a
// step — by requesting only 12 of them up front and the rest behind three more vmcnt(0) round trips per step.)
// FOLD: the plan folds mirrored pairs (dl_pair_incidence.inc_pair2) — an entry's probability and terms go to a second pair id
// as well, from the lanes that store the first; same arithmetic, same bits.  The last step of a segment issues no gathers
// for the entries past its end (a wave-uniform branch per entry; their lanes compute on zeros and store nothing): the
// padding of squirrel's short segments was 5.9 % of all gathers and, although it hit in the vector L1, 7.7 % of the
// kernel's time (154.3 -> 142.5 us; folding 151.6; both 139.9 — profiles/r9_fwd_fold_bound.txt).
template <int K, int D, bool T1, bool COEF, bool FOLD, bool LOGIT = false>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, FWD_WAVE_MAXW))) void score_fwd_wave_kernel(dl_csr_plan g, const int32_t* __restrict__ pair_id,
                                                                  const int32_t* __restrict__ pair_id2,
                                                                  const float* __restrict__ Z, const float* __restrict__ H, float t,
                                                                  float* __restrict__ prob, float* __restrict__ coef_e,
                                                                  float* __restrict__ coef_q) {
    using FW = FwdWave<K, D>;
    constexpr int NJ = FW::NJ, U = FW::U, ROW = K * D;
    static_assert(D == 64 && NJ >= 1 && U * NJ <= 8, "one DPP row of 16 lanes per factor slice; at most 8 exponents per row and step");
    __shared__ __attribute__((aligned(16))) float4 urow[WAVES_PER_BLOCK][2 * ROW / 4];      // [Z row | H row] of the segment's u
    __shared__ int ent_q[WAVES_PER_BLOCK][(FOLD ? 2 : 1) * DL_WAVE];
    const WaveSeg ws = load_wave_seg(g);
    if (!ws.active) return;                                         // no barrier in this kernel: every region is its wave's own
    const SegInfo si = ws.si;
    const int wave = ws.wave, lane = lane_id();
    const int i = lane & 15, r = lane >> 4;                         // position in the DPP row; the row holds the factors r, r + 4
    float4* const mine = urow[wave];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        mine[j * 64 + lane] = *reinterpret_cast<const float4*>(Z + (size_t)si.grow * ROW + (j * 64 + lane) * 4);
        mine[ROW / 4 + j * 64 + lane] = *reinterpret_cast<const float4*>(H + (size_t)si.grow * ROW + (j * 64 + lane) * 4);
    }
    int my_col = si.grow, my_q = 0, my_q2 = -1;
    if (si.beg + lane < si.end) {
        my_col = g.col[si.beg + lane];
        my_q = pair_id[si.beg + lane];
        if constexpr (FOLD) my_q2 = pair_id2[si.beg + lane];
    }
    ent_q[wave][lane] = my_q;                                       // written and read by this wave only
    if constexpr (FOLD) ent_q[wave][DL_WAVE + lane] = my_q2;
    const int len = si.end - si.beg;
    // one step = U entries; n_live of them are gathered (all U, known at compile time, in every step but a segment's last)
    auto do_step = [&](const int step, auto tail, const int n_live) {
        constexpr bool TAIL = decltype(tail)::value;
        float4 zv[U][NJ], hv[U][NJ];
#pragma unroll
        for (int e = 0; e < U; ++e) {
            if (!TAIL || e < n_live) {                              // wave-uniform
                const size_t v = (size_t)(unsigned)__builtin_amdgcn_readlane(my_col, (step * U + e) & 63);
                const auto* zr = uniform_row<dl_vf4>(Z, v * ROW * sizeof(float));     // row base in SGPRs (dl_fast.h)
                const auto* hr = uniform_row<dl_vf4>(H, v * ROW * sizeof(float));
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    zv[e][j] = as_float4(zr[(unsigned)(lane + j * 64)]);
                    hv[e][j] = as_float4(hr[(unsigned)(lane + j * 64)]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NJ; ++j) zv[e][j] = hv[e][j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        float val[16];                                              // index = table * 8 + chunk * 4 + entry
#pragma unroll
        for (int x = 0; x < 16; ++x) val[x] = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float4 a4 = mine[j * 64 + lane], b4 = mine[ROW / 4 + j * 64 + lane];
#pragma unroll
            for (int e = 0; e < U; ++e) {
                val[j * 4 + e] = dot4_packed(a4, zv[e][j]);
                val[8 + j * 4 + e] = dot4_packed(b4, hv[e][j]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        TransposedReduce<16, 8>::run(val, i);                       // lane i: sum number i — below 8: z_u . z_v of (chunk i / 4, entry i % 4), above: h_u . h_v
        const float mine_v = val[0];
        const float ex = expf(T1 ? mine_v : mine_v / t);
        const float ttv = mine_v * xor_lane<8>(ex);                 // lanes 8..15: (h.h) e^(z.z / t) of (chunk, entry)
        float term = ttv;
        if constexpr (NJ == 2) term += xor_lane<4>(ttv);
        const float logit = add_xor<32>(add_xor<16>(term));         // over the 4 DPP rows: all factors
        const float p = LOGIT ? logit : sigmoid_ref(logit);
        const int idx = step * U + (i & 3);
        const bool live = idx < len;
        const int qq = ent_q[wave][idx & 63];
        int qq2 = -1;
        if constexpr (FOLD) qq2 = ent_q[wave][DL_WAVE + (idx & 63)];
        if (lane >= 8 && lane < 12 && live) {
            prob[qq] = p;
            if (FOLD && qq2 >= 0) prob[qq2] = p;
        }
        if constexpr (COEF) {                                       // per-factor terms for the separate backward: e_k, q_k e_k
            const int k = 4 * ((i & 7) >> 2) + r;                   // the factor this lane's sum belongs to (chunk j holds the factors 4 j + r)
            if (live && (NJ == 2 || (i & 7) < 4)) {
                if (i < 8) coef_e[(size_t)qq * K + k] = ex;
                else coef_q[(size_t)qq * K + k] = ttv;
                if (FOLD && qq2 >= 0) {
                    if (i < 8) coef_e[(size_t)qq2 * K + k] = ex;
                    else coef_q[(size_t)qq2 * K + k] = ttv;
                }
            }
        }
    };
    const int nfull = len / U;
    for (int step = 0; step < nfull; ++step) do_step(step, std::false_type{}, U);
    if (len % U != 0) do_step(nfull, std::true_type{}, len % U);
}

// ---------------------------------------------------------------------------- forward scorer over a hub plan
// The wave-per-entry kernel above gathers one [Z row | H row] pair per entry and is bound by those bytes.  On a skewed pair
// list most entries sit in a few long rows that score against many of the SAME partner rows: a workgroup that holds a
// block of 16 such rows in LDS (dl_pair_hub, disenlink_hip.h) gathers a partner row once for up to four of them.
// Item, staging (64 KB at K = 8: two workgroups per CU), walk and batch counter are those of every kernel over a hub plan
// (dl_hub.h, with the plan contract).  A step is the step of the kernel above — 4 / 2 / 1 partner rows gathered into
// registers through a scalar row base, 16 float4 in flight before anything waits, the same dot4_packed calls into
// val[table * 8 + chunk * 4 + slot], the same reduction, expf and sigmoid — except that every slot reads ITS OWN u row from
// LDS, and that the partner registers a slot uses are fixed by the step's shape (NV = gathered rows: slot e uses the set
// its shape's row map names, dl_hub.h).  The value of a slot never meets another slot's, and the reduction adds the same 16 lanes in the same order
// whichever slot a value sits in: every pair gets the bits of the kernel above.
// Without per-factor terms (COEF == false) a step ends at its logit: a step yields 4 of them and a wave has 64 lanes, so the
// wave keeps the logits of 16 steps in its lanes and runs ONE sigmoid and ONE store pass per batch (and one behind its last
// step), with pair ids it read per lane when the batch opened — no second expf, no IEEE division, no pair-id selects and no
// store on the chain a wave must finish before its next gathers go out (the scorer alone on squirrel: 116.9 -> 112.1 us; with the
// bank-masked reduction below 107.8, profiles/r13_fwd_hub_tail.txt).
// The base name is that kernel's on purpose: the per-phase accounting of the benchmark matches kernels by base name.
namespace hub {
// The 16 plan words of one step: partner rows, u_local, pair id and second pair id of its four slots.
struct StepWords { dl_vi4 v, u, q, p; };

// TransposedReduce<16, 8> with the stages OFF = 8 and OFF = 4 as two bank-masked DPP adds per output: the select bit of a
// stage is constant within a bank of 4 lanes, so "keep + (send of lane ^ OFF)" is one add written under the banks whose bit is
// clear and one under the others — the same two addends per lane (IEEE addition commutes: the same bits), without the two
// v_cndmask per output and, at OFF = 4, without the v_mov_dpp.  The builtins cannot say "the second add keeps the lanes of the
// first", hence asm; one statement per stage, outputs early-clobber, and an s_nop 1 at its head: the hazard recogniser does not
// see inside asm, and a DPP read of a VGPR needs two wait states behind the VALU write of it (store4_sc1 is the precedent).
// Every lane must be active.
__device__ __forceinline__ void transposed_reduce16_masked(float* v, int c) {
    float a[8], b[4];
    asm volatile("s_nop 1\n\t"
                 "v_add_f32_dpp %0, %8, %8 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %1, %9, %9 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %2, %10, %10 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %3, %11, %11 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %4, %12, %12 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %5, %13, %13 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %6, %14, %14 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %7, %15, %15 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %0, %16, %16 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %1, %17, %17 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %2, %18, %18 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %3, %19, %19 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %4, %20, %20 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %5, %21, %21 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %6, %22, %22 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %7, %23, %23 row_ror:8 row_mask:0xf bank_mask:0xc"
                 : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3]), "=&v"(a[4]), "=&v"(a[5]), "=&v"(a[6]), "=&v"(a[7])
                 : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]), "v"(v[8]), "v"(v[9]),
                   "v"(v[10]), "v"(v[11]), "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]));
    asm volatile("s_nop 1\n\t"
                 "v_add_f32_dpp %0, %4, %4 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %1, %5, %5 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %2, %6, %6 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %3, %7, %7 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %0, %8, %8 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
                 "v_add_f32_dpp %1, %9, %9 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
                 "v_add_f32_dpp %2, %10, %10 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
                 "v_add_f32_dpp %3, %11, %11 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
                 "s_nop 1"                                           // the next stage's DPP reads are the compiler's: it does not know of these writes
                 : "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
                 : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]));
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = b[q];
    TransposedReduce<4, 2>::run(v, c);
}

// MIXED: h is the plan of a dl_pair_hub_mixed — five lists per item, walked by the five-list walk of dl_hub.h, whose two further
// shapes differ from A, B and C in nothing but the number of gathered rows and the slot -> row map below.  A partner row is
// then gathered once per remainder of its group, and a slot's hub row is the heavier endpoint of its pair: fewer gathered
// rows for the same steps, the same LDS reads and the same arithmetic (profiles/r17_fwd_hub_mixed.txt).
template <int K, int D, bool T1, bool COEF, bool FOLD, bool LOGIT = false, bool MIXED = false>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void score_fwd_wave_kernel(
    dl_pair_hub h, const float* __restrict__ Z, const float* __restrict__ H, float t, float* __restrict__ prob,
    float* __restrict__ coef_e, float* __restrict__ coef_q) {
    using FW = FwdWave<K, D>;
    constexpr int NJ = FW::NJ, U = FW::U, ROW = K * D, R4 = 2 * ROW / 4;      // R4: float4 of one [Z row | H row]
    static_assert(D == 64 && NJ >= 1 && U == 4 && U * NJ <= 8, "the step geometry of score_fwd_wave_kernel");
    static_assert(!(LOGIT && COEF), "the logit form has no stored terms");
    constexpr bool BATCH = !COEF;      // the forms with per-factor terms store per step and per lane anyway: they keep the per-step tail
    __shared__ __attribute__((aligned(16))) float4 urow[DL_HUB_W * R4];
    int it;
    if (!workgroup_item<false>(h, it)) return;
    const int wave = wave_index(), lane = lane_id();
    const int i = lane & 15, r = lane >> 4;
    const int blk = h.item_block[it];
    const std::conditional_t<MIXED, MixedItemSteps, ItemSteps> st = [&] {      // asked for with the block, ahead of the staging loads
        if constexpr (MIXED) return mixed_item_steps(h, it);
        else return item_steps(h, it);
    }();
    stage_block<NJ, 2>((lds_vf4*)urow, h, blk, wave, lane, {Z, H});
    __syncthreads();                                                 // the only one: nothing below waits for another wave
    // a step's 16 words through the scalar cache (the plan is read-only for the whole launch)
    auto fetch = [&](const int step) {
        const int s = __builtin_amdgcn_readfirstlane(step);
        StepWords w;
        w.v = plan_words(h.step_v, s), w.u = plan_words(h.step_u, s);
        w.q = w.p = dl_vi4{-1, -1, -1, -1};
        if constexpr (!BATCH) {                                      // a batched tail reads the pair ids per lane, once per 16 steps
            w.q = plan_words(h.step_q, s);
            if constexpr (FOLD) w.p = plan_words(h.step_q2, s);
        }
        return w;
    };
    // BATCH: the pending logits of up to 16 of the wave's steps, one per lane — lane L holds slot L & 3 of the batch's step
    // number L >> 2 (the steps s0, s0 + 8, ...).  The pair ids of a batch are asked for per lane when it opens (a wave takes
    // every step s0 + 8 b below the item's end) and are there long before the flush.
    const int slot_step = lane >> 2;
    float lg = 0.0f;
    int pq = -1, pq2 = -1;
    Batch<16, true> batch;
    auto open = [&](const int s0) {
        const int sb = s0 + WAVES * slot_step;
        pq = pq2 = -1;
        if (sb < st.end) {
            pq = h.step_q[4 * sb + (lane & 3)];
            if constexpr (FOLD) pq2 = h.step_q2[4 * sb + (lane & 3)];
        }
    };
    auto flush = [&]() {                                             // one sigmoid (LOGIT: none) and one store pass for the whole batch
        const float p = LOGIT ? lg : sigmoid_ref(lg);
        if (pq >= 0) prob[pq] = p;                                   // a dead slot's id is -1 in the plan, like a dead lane's here
        if (FOLD && pq2 >= 0) prob[pq2] = p;
    };
    auto do_step = [&](const StepWords& w, auto shape, auto last) {
        using SH = decltype(shape);
        constexpr int NV = SH::value;                                // gathered partner rows: 4 (A), 3 (A211), 2 (B, B31), 1 (C)
        constexpr bool LAST = decltype(last)::value;                 // dead partner rows: dl_hub.h; the kernel above's TAIL
        const int sv[4] = {w.v.x, w.v.y, w.v.z, w.v.w}, su[4] = {w.u.x, w.u.y, w.u.z, w.u.w}, sq[4] = {w.q.x, w.q.y, w.q.z, w.q.w},
                  sq2[4] = {w.p.x, w.p.y, w.p.z, w.p.w};
        float4 zv[NV][NJ], hv[NV][NJ];
#pragma unroll
        for (int n = 0; n < NV; ++n) {
            if (!LAST || sv[n] >= 0) {                               // wave-uniform
                const size_t v = (size_t)(unsigned)sv[n];
                const auto* zr = uniform_row<dl_vf4>(Z, v * ROW * sizeof(float));
                const auto* hr = uniform_row<dl_vf4>(H, v * ROW * sizeof(float));
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    zv[n][j] = as_float4(zr[(unsigned)(lane + j * 64)]);
                    hv[n][j] = as_float4(hr[(unsigned)(lane + j * 64)]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NJ; ++j) zv[n][j] = hv[n][j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        float val[16];                                              // index = table * 8 + chunk * 4 + slot
#pragma unroll
        for (int q = 0; q < 16; ++q) val[q] = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            // the chunk's eight LDS reads are issued together, ahead of its dot products: left in one loop with them, the reads
            // of the second chunk go out one or two at a time, each behind the wait of the one before (profiles/r12_*)
            float4 a4[U], b4[U];
#pragma unroll
            for (int e = 0; e < U; ++e) {
                const float4* mine = urow + (su[e] & (DL_HUB_W - 1)) * R4;     // this slot's own u row
                a4[e] = mine[j * 64 + lane], b4[e] = mine[ROW / 4 + j * 64 + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < U; ++e) {
                // (A, B and C: row(e) == e * NV / 4 — the three-list forms keep that expression and with it their register allocation)
                const int rw = MIXED ? SH::row(e) : e * NV / 4;
                val[j * 4 + e] = dot4_packed(a4[e], zv[rw][j]);
                val[8 + j * 4 + e] = dot4_packed(b4[e], hv[rw][j]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        transposed_reduce16_masked(val, i);                         // TransposedReduce<16, 8>::run(val, i) in fewer instructions
        const float mine_v = val[0];
        const float ex = expf(T1 ? mine_v : mine_v / t);
        const float ttv = mine_v * xor_lane<8>(ex);
        float term = ttv;
        if constexpr (NJ == 2) term += xor_lane<4>(ttv);
        if constexpr (BATCH) {
            // term is valid in the lanes 8..11 of a DPP row: copied under bank masks into the other lanes of the row, the two adds
            // over the rows leave the logit of slot lane & 3 in EVERY lane — the same addends in the same order as in lanes
            // 8..11 — and the lanes of this step's batch slot keep it.  (At NJ == 2 the lanes 12..15 hold the same two addends the
            // other way round, but hipcc contracts `ttv + xor_lane<4>(ttv)` into an FMA on the lane's own product: the halves of
            // the row differ in the last bit of some pairs, and only 8..11 are the reference's bits.)
            int tb = __float_as_int(term);
            tb = __builtin_amdgcn_update_dpp(tb, tb, 0x114, 0xF, 0x8, false);                             // row_shr:4 -> lanes 12..15
            tb = __builtin_amdgcn_update_dpp(tb, tb, 0x128, 0xF, 0x3, false);                             // row_ror:8 -> lanes 0..7
            const float logit = add_xor<32>(add_xor<16>(__int_as_float(tb)));
            lg = slot_step == batch.nb ? logit : lg;
            ++batch.nb;
        } else {
            const float logit = add_xor<32>(add_xor<16>(term));
            const float p = sigmoid_ref(logit);
            const int e_me = i & 3;
            const int qq = e_me == 0 ? sq[0] : e_me == 1 ? sq[1] : e_me == 2 ? sq[2] : sq[3];
            const int qq2 = e_me == 0 ? sq2[0] : e_me == 1 ? sq2[1] : e_me == 2 ? sq2[2] : sq2[3];
            const bool live = qq >= 0;
            if (lane >= 8 && lane < 12 && live) {
                prob[qq] = p;
                if (FOLD && qq2 >= 0) prob[qq2] = p;
            }
            if constexpr (COEF) {
                const int k = 4 * ((i & 7) >> 2) + r;
                if (live && (NJ == 2 || (i & 7) < 4)) {
                    if (i < 8) coef_e[(size_t)qq * K + k] = ex;
                    else coef_q[(size_t)qq * K + k] = ttv;
                    if (FOLD && qq2 >= 0) {
                        if (i < 8) coef_e[(size_t)qq2 * K + k] = ex;
                        else coef_q[(size_t)qq2 * K + k] = ttv;
                    }
                }
            }
        }
    };
    const int s = st.a + wave;
    StepWords nxt = {};
    if (s < st.end) nxt = fetch(s);
    if constexpr (BATCH) open(s);
    walk(s, st, nxt, fetch, [&](const StepWords& w, const int step, auto shape, auto last) {
        do_step(w, shape, last);
        if constexpr (BATCH) batch.tick(step, flush, open);
    });
    if constexpr (BATCH) batch.close(flush);
}
}  // namespace hub

// Dense [N][N] scorer (the reference's link_pred, model.py:109-113): no pair list at all.  One wave = one
// row u x one chunk of <= VCH consecutive columns; the column space is cut into n_slices XCD slices exactly
// like the pair plans (workgroup b serves slice b % n_slices), so an XCD's L2 holds the v rows it gathers.
template <int K, int D, typename T>
__global__ __launch_bounds__(BLOCK) void score_allpairs_kernel(const T* __restrict__ Z, const T* __restrict__ H, int N,
                                                               float t, int n_slices, int slice_w, int chunks_per_u,
                                                               float* __restrict__ prob) {
    using GE = Geo<K, D, T>;
    constexpr int VEC = GE::VEC, G = GE::G, EPW = GE::EPW, ROW = GE::ROW;
    constexpr int KB = K > 8 ? 8 : K;
    using FLB = FactorLanes<G, KB>;
    constexpr int KBP = FLB::KP;
    constexpr int VCH = 256;
    __shared__ __attribute__((aligned(16))) float urow[WAVES_PER_BLOCK][2 * ROW];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int x = blockIdx.x % n_slices;
    const int item = (blockIdx.x / n_slices) * WAVES_PER_BLOCK + wave;
    const int u = item / chunks_per_u, ch = item - u * chunks_per_u;
    const int v0 = x * slice_w + ch * VCH;
    const int v1 = min(min(v0 + VCH, (x + 1) * slice_w), N);
    const bool active = u < N && v0 < v1;
    if (active) stage_u_rows<K, D, T>(urow[wave], Z, H, (size_t)u);
    __syncthreads();
    if (!active) return;
    const int c = lane % G, grp = lane / G;
    const int kbb = FLB::factor_base(c);
    for (int base = v0; base < v1; base += EPW) {
        const int vi = base + grp;
        const bool live = vi < v1;
        const size_t v = (size_t)(live ? vi : v0);
        float term = 0.0f;
#pragma unroll
        for (int b0 = 0; b0 < K; b0 += KB) {
            float pq[KBP], ps[KBP];
#pragma unroll
            for (int k = 0; k < KBP; ++k) {
                const bool in = k < KB && b0 + k < K;
                const int kk = in ? b0 + k : 0;
                pq[k] = in ? dot(load_f32<VEC>(&urow[wave][ROW + kk * D + c * VEC]), Tab<T>::load(H + v * ROW + kk * D + c * VEC)) : 0.0f;
                ps[k] = in ? dot(load_f32<VEC>(&urow[wave][kk * D + c * VEC]), Tab<T>::load(Z + v * ROW + kk * D + c * VEC)) : 0.0f;
            }
            TransposedReduce<KBP, G / 2>::run(pq, c);
            TransposedReduce<KBP, G / 2>::run(ps, c);
#pragma unroll
            for (int i = 0; i < FLB::VPL; ++i)
                if (FLB::primary(c) && kbb + i < KB && b0 + kbb + i < K) term += pq[i] * expf(div_t(ps[i], t));
        }
        const float logit = group_allreduce_sum<G>(term);
        if (live && c == 0) prob[(size_t)u * N + vi] = sigmoid_ref(logit);
    }
}

// Scorer backward from stored per-factor terms: a weighted row gather, one launch per output.
//   PASS 0: dZ[u] = sum_inc (gl/t) * (q_k e_k) * Z[v][k]      PASS 1: dH[u] = sum_inc gl * e_k * H[v][k]
template <int K, int D, typename T, int PASS>
__global__ __launch_bounds__(BLOCK) void score_bwd_coef_seg_kernel(dl_csr_plan g, const int32_t* __restrict__ inc_pair,
                                                                   const T* __restrict__ X, float t,
                                                                   const float* __restrict__ prob,
                                                                   const float* __restrict__ g_prob,
                                                                   const float* __restrict__ coef,
                                                                   float* __restrict__ out, float* __restrict__ part) {
    using GE = Geo<K, D, T>;
    constexpr int VEC = GE::VEC, G = GE::G, EPW = GE::EPW, ROW = GE::ROW;
    using US = Stage<K, D, T, 1>;
    __shared__ __attribute__((aligned(16))) float red[US::FLOATS];
    const WaveSeg ws = load_wave_seg(g);
    const SegInfo si = ws.si;
    const int lane = lane_id();
    const int c = lane % G, grp = lane / G;
    if (ws.active) {
        Chunk<VEC> acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = zero_chunk<VEC>();
        int my_col = si.grow, my_pair = 0;
        float my_gl = 0.0f;
        if (si.beg + lane < si.end) {
            my_col = g.col[si.beg + lane];
            my_pair = inc_pair[si.beg + lane];
            const float pr = prob[my_pair];
            my_gl = g_prob[my_pair] * pr * (1.0f - pr);      // sigmoid backward p(1-p)
            if (PASS == 0) my_gl = div_t(my_gl, t);
        }
        for (int base = si.beg; base < si.end; base += EPW) {
            const int idx = base + grp - si.beg;
            const size_t v = (size_t)__shfl(my_col, idx, DL_WAVE);
            const int q = __shfl(my_pair, idx, DL_WAVE);
            const float gl = __shfl(my_gl, idx, DL_WAVE);     // 0 past the segment end
            float ck[K];
            if constexpr (K % 4 == 0) {
#pragma unroll
                for (int k = 0; k < K; k += 4) {
                    const float4 t4 = *reinterpret_cast<const float4*>(coef + (size_t)q * K + k);
                    ck[k] = t4.x; ck[k + 1] = t4.y; ck[k + 2] = t4.z; ck[k + 3] = t4.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k) ck[k] = coef[(size_t)q * K + k];
            }
            // gathers in blocks of <= 8 factor slices: bounded live registers for any K
#pragma unroll
            for (int b0 = 0; b0 < K; b0 += 8) {
                Chunk<VEC> xv[8];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (b0 + k < K) xv[k] = Tab<T>::load(X + v * ROW + (b0 + k) * D + c * VEC);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (b0 + k < K) fma_chunk(acc[b0 + k], gl * ck[b0 + k], xv[k]);
            }
        }
        US::put(red, ws.wave, grp, c, acc, 0);
    }
    __syncthreads();
    if (!ws.head) return;
    float4 r[US::NQ];
    US::sum(red, ws.wave, ws.n_unit, lane, r);
    float* o = si.slot < 0 ? out + (size_t)si.grow * ROW : part + (size_t)si.slot * ROW;
#pragma unroll
    for (int q = 0; q < US::NQ; ++q) {
        const int x = q * DL_WAVE + lane;
        if (x < US::F4) store4(o + 4 * x, r[q]);
    }
}

// Launch geometry of score_allpairs_kernel for rows of row_bytes bytes: slice the columns 8 ways only while a slice of
// Z+H can live in an XCD's L2 (like graph.auto_slices).  Shared by the launch and by fast_score_allpairs_form.
struct AllpairsGeo { int n_slices, slice_w, chunks_per_u; long long items; unsigned blocks; };
static AllpairsGeo allpairs_geo(int N, size_t row_bytes) {
    AllpairsGeo g;
    const double table = 2.0 * N * (double)row_bytes;
    g.n_slices = table <= 8.0 * 8.0 * (4 << 20) && N >= 64 ? 8 : 1;
    g.slice_w = (N + g.n_slices - 1) / g.n_slices;
    g.chunks_per_u = (g.slice_w + 255) / 256;
    g.items = (long long)N * g.chunks_per_u;
    g.blocks = (unsigned)(g.n_slices * ((g.items + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK));
    return g;
}

template <int K, int D, typename T>
struct ScoreOps {
    static constexpr int ROW = K * D;
    template <bool LOGIT = false>
    static int score_fwd(const dl_pair_incidence* by_u, const void* Z, const void* H, float t, float* prob,
                         float* coef, hipStream_t st) {
        const dl_csr_plan* g = &by_u->csr;
        float* coef_q = coef ? coef + (size_t)by_u->n_pairs * K : nullptr;
        if constexpr (std::is_same<T, float>::value && FwdWave<K, D>::ok) {
            if (g->seg_len <= 64 && g->seg_len % FwdWave<K, D>::U == 0 && !config().fwd_group_kernel) {
                // the three flags of both wave kernels: temperature 1, stored terms, folded mirrors
                auto pick = [&](auto launch) {
                    auto fold = [&](auto t1, auto cf) {
                        if (by_u->inc_pair2) launch(t1, cf, std::true_type{});
                        else launch(t1, cf, std::false_type{});
                    };
                    if constexpr (!LOGIT) {                          // (the logit form has no stored terms: its coef is NULL)
                        if (coef) {
                            if (t == 1.0f) fold(std::true_type{}, std::true_type{}); else fold(std::false_type{}, std::true_type{});
                            return;
                        }
                    }
                    if (t == 1.0f) fold(std::true_type{}, std::false_type{}); else fold(std::false_type{}, std::false_type{});
                };
                auto wave_plan = [&](const dl_csr_plan* c, const int32_t* pair, const int32_t* pair2) {
                    pick([&](auto t1, auto cf, auto fo) {
                        hipLaunchKernelGGL((score_fwd_wave_kernel<K, D, decltype(t1)::value, decltype(cf)::value, decltype(fo)::value, LOGIT>),
                                           dim3(seg_blocks(c)), dim3(BLOCK), 0, st, *c, pair, pair2, (const float*)Z,
                                           (const float*)H, t, prob, coef, coef_q);
                    });
                };
                const dl_pair_hub* hp = config().fwd_hub ? by_u->hub : nullptr;
                const dl_pair_hub* hm = config().fwd_hub && config().score_hub_mixed && by_u->hub_mixed ? &by_u->hub_mixed->hub : nullptr;
                if (hm != nullptr && hm->n_items > 0) {
                    // the same, over the mixed plan: five step shapes, and its own residual plan
                    pick([&](auto t1, auto cf, auto fo) {
                        hipLaunchKernelGGL((hub::score_fwd_wave_kernel<K, D, decltype(t1)::value, decltype(cf)::value, decltype(fo)::value, LOGIT, true>),
                                           dim3((unsigned)hm->n_slices * (unsigned)hm->slice_max_item), dim3(hub::THREADS), 0,
                                           st, *hm, (const float*)Z, (const float*)H, t, prob, coef, coef_q);
                    });
                    if (hm->rest.n_entries > 0) wave_plan(&hm->rest, hm->rest_pair, hm->rest_pair2);
                    return check_launch("score_pairs_fwd(fast, mixed hub blocks + wave per entry)");
                }
                if (hp != nullptr && hp->n_items > 0) {
                    // hub rows by blocks of 16 (hub::score_fwd_wave_kernel), then every other row as before
                    pick([&](auto t1, auto cf, auto fo) {
                        hipLaunchKernelGGL((hub::score_fwd_wave_kernel<K, D, decltype(t1)::value, decltype(cf)::value, decltype(fo)::value, LOGIT>),
                                           dim3((unsigned)hp->n_slices * (unsigned)hp->slice_max_item), dim3(hub::THREADS), 0,
                                           st, *hp, (const float*)Z, (const float*)H, t, prob, coef, coef_q);
                    });
                    if (hp->rest.n_entries > 0) wave_plan(&hp->rest, hp->rest_pair, hp->rest_pair2);
                    return check_launch("score_pairs_fwd(fast, hub blocks + wave per entry)");
                }
                wave_plan(g, by_u->inc_pair, by_u->inc_pair2);
                return check_launch("score_pairs_fwd(fast, wave per entry)");
            }
        }
        if constexpr (!LOGIT) {
            if (coef) {
                hipLaunchKernelGGL((score_fwd_seg_kernel<K, D, T, true>), dim3(seg_blocks(g)), dim3(BLOCK), 0, st, *g,
                                   by_u->inc_pair, by_u->inc_pair2, (const T*)Z, (const T*)H, t, prob, coef, coef_q);
                return check_launch("score_pairs_fwd(fast)");
            }
        }
        hipLaunchKernelGGL((score_fwd_seg_kernel<K, D, T, false, LOGIT>), dim3(seg_blocks(g)), dim3(BLOCK), 0, st, *g,
                               by_u->inc_pair, by_u->inc_pair2, (const T*)Z, (const T*)H, t, prob, coef, coef_q);
        return check_launch("score_pairs_fwd(fast)");
    }

    static int score_allpairs(const void* Z, const void* H, int N, float t, float* prob, hipStream_t st) {
        const AllpairsGeo g = allpairs_geo(N, ROW * sizeof(T));
        hipLaunchKernelGGL((score_allpairs_kernel<K, D, T>), dim3(g.blocks), dim3(BLOCK), 0, st, (const T*)Z, (const T*)H, N,
                           t, g.n_slices, g.slice_w, g.chunks_per_u, prob);
        return check_launch("score_allpairs_fwd(fast)");
    }

    template <bool LOGIT = false>
    static int score_bwd(const dl_pair_incidence* inc, const void* Z, const void* H, float t, const float* prob,
                         const float* g_prob, const float* coef, float* dZ, float* dH, float* part, hipStream_t st) {
        const dl_csr_plan* g = &inc->csr;
        const float* no_x = nullptr;
        if constexpr (!LOGIT) {                                  // (the logit form has no stored terms: it recomputes)
        if (coef) {
            const float* coef_q = coef + (size_t)inc->n_pairs * K;
            float* part_h = part + (size_t)g->n_slots * ROW;
            hipLaunchKernelGGL((score_bwd_coef_seg_kernel<K, D, T, 0>), dim3(seg_blocks(g)), dim3(BLOCK), 0, st, *g,
                               inc->inc_pair, (const T*)Z, t, prob, g_prob, coef_q, dZ, part);
            hipLaunchKernelGGL((score_bwd_coef_seg_kernel<K, D, T, 1>), dim3(seg_blocks(g)), dim3(BLOCK), 0, st, *g,
                               inc->inc_pair, (const T*)H, t, prob, g_prob, coef, dH, part_h);
            if (g->n_multi > 0)
                hipLaunchKernelGGL((row_combine_kernel<ROW, float, float>), dim3(g->n_multi, 2), dim3(BLOCK), 0, st, *g,
                                   part, ROW, no_x, 0.0f, 1.0f, dZ, 0, part_h, dH);
            return check_launch("score_pairs_bwd(fast, stored terms)");
        }
        }
        hipLaunchKernelGGL((score_bwd_seg_kernel<K, D, T, false, LOGIT>), dim3(seg_blocks(g)), dim3(BLOCK), 0, st, *g, inc->inc_pair,
                           (const T*)Z, (const T*)H, t, prob, g_prob, dZ, dH, part);
        if (g->n_multi > 0)
            hipLaunchKernelGGL((row_combine_kernel<ROW, float, float>), dim3(g->n_multi, 2), dim3(BLOCK), 0, st, *g, part,
                               2 * ROW, no_x, 0.0f, 1.0f, dZ, 0, part + ROW, dH);
        return check_launch("score_pairs_bwd(fast)");
    }
};

}  // namespace fast

}  // namespace dl
