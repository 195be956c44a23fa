// What a kernel over a hub plan (dl_pair_hub, disenlink_hip.h) shares: hub::score_fwd_wave_kernel (dl_score.h) and
// hub::route_seg_kernel (dl_route.hip).  A workgroup of eight waves takes one work item: it stages the 16 rows of the item's
// block in LDS, ONE barrier, and from there on wave w runs the steps s_a + w, + 8, ... of the item on its own, counted through
// the three lists [A | B | C] so that no two waves differ by more than one step.
// THE PLAN CONTRACT (stated in disenlink_hip.h at dl_pair_hub; graph.HubPlan.check refuses any other plan before it is bound):
//   - dead partner rows (-1) stand only in the LAST step of list A and of list B of an item: LAST is compiled into those two
//     steps alone, every other step gathers its rows without a sign test and without a zero fill, and a C step has none;
//   - an item's steps are [item_step[0], item_step[3]): the walk requests the words of a wave's next step one step ahead and
//     never past the item's last step, and a batch asks for no word of a step past it;
//   - every lane is active at a step's reduction: the walk's branches are wave-uniform (a wave takes a step or does not).
// A mixed plan (dl_pair_hub_mixed; graph.HubPlan.build_mixed, the forward scorer only) has five lists [A | A211 | B | B31 | C]
// under the same contract: dead partner rows only in the last step of each of its first four lists.
#pragma once
#include "dl_fast.h"

namespace dl::fast::hub {
constexpr int WAVES = 8, THREADS = WAVES * DL_WAVE;
static_assert(DL_HUB_W == 2 * WAVES, "every wave stages two rows of the block");

// Four consecutive plan words at a wave-uniform index, as ONE scalar load: the pointer is typed constant address space, which
// is what lets hipcc use the scalar cache for a load that follows the kernel's own stores (to prob, p, a — never to a plan array).
typedef int dl_vi4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ dl_vi4 plan_words(const int32_t* a, int idx) {
    const auto* g = (const __attribute__((address_space(1))) int32_t*)a;
    return reinterpret_cast<const __attribute__((address_space(4))) dl_vi4*>((const __attribute__((address_space(4))) int32_t*)g)[idx];
}

// The workgroup's item: workgroup b serves stream b % n_slices.  false: none — the whole workgroup returns, before the barrier.
// ONE_STREAM: a plan with one stream takes the workgroup's index, without a round trip to the stream table.
template <bool ONE_STREAM>
__device__ __forceinline__ bool workgroup_item(const dl_pair_hub& h, int& it) {
    it = (int)blockIdx.x;
    if (ONE_STREAM && h.n_slices == 1) return it < h.n_items;
    const int x = blockIdx.x % h.n_slices;
    it = h.slice_item0[x] + (int)(blockIdx.x / h.n_slices);
    return it < h.slice_item0[x + 1];
}

struct ItemSteps { int a, b, c, end; };                              // list A: [a, b), B: [b, c), C: [c, end)
__device__ __forceinline__ ItemSteps item_steps(const dl_pair_hub& h, int it) {
    return {h.item_step[4 * it], h.item_step[4 * it + 1], h.item_step[4 * it + 2], h.item_step[4 * it + 3]};
}

// The block's 16 rows of NTAB tables into urow[16][NTAB][NJ * 64] float4, two rows per wave.  The caller's barrier follows.
// (urow is typed LDS: through a generic pointer hipcc orders these stores against the plan's loads, and stages row by row.)
typedef __attribute__((address_space(3))) dl_vf4 lds_vf4;
template <int NJ, int NTAB>
__device__ __forceinline__ void stage_block(lds_vf4* urow, const dl_pair_hub& h, int blk, int wave, int lane,
                                            const float* const (&tab)[NTAB]) {
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int ul = 2 * wave + rr;
        const int row = h.block_row[blk * DL_HUB_W + ul];            // wave-uniform; -1: the last block is short
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            dl_vf4 x[NTAB];
#pragma unroll
            for (int n = 0; n < NTAB; ++n) x[n] = dl_vf4{0.0f, 0.0f, 0.0f, 0.0f};
            if (row >= 0) {
#pragma unroll
                for (int n = 0; n < NTAB; ++n)
                    x[n] = *reinterpret_cast<const dl_vf4*>(tab[n] + (size_t)row * (NJ * 256) + (j * 64 + lane) * 4);
            }
#pragma unroll
            for (int n = 0; n < NTAB; ++n) urow[(ul * NTAB + n) * (NJ * 64) + j * 64 + lane] = x[n];
        }
    }
}

// The walk of wave w = (s - st.a): step(words, s, shape, last) for each of its steps, in order.  shape: gathered partner rows
// (value) and which of them each of the four slots scores against (row).
using FULL = std::false_type;
using LAST = std::true_type;                                         // the step may hold dead partner rows
template <int NV, int R0, int R1, int R2, int R3>
struct Shape {
    static constexpr int value = NV;
    static constexpr int row(int e) { return e == 0 ? R0 : e == 1 ? R1 : e == 2 ? R2 : R3; }
};
constexpr Shape<4, 0, 1, 2, 3> SHAPE_A{};
constexpr Shape<2, 0, 0, 1, 1> SHAPE_B{};
constexpr Shape<1, 0, 0, 0, 0> SHAPE_C{};
constexpr Shape<3, 0, 0, 1, 2> SHAPE_A211{};                         // the two shapes only a mixed plan has (dl_pair_hub_mixed)
constexpr Shape<2, 0, 0, 0, 1> SHAPE_B31{};
// nxt: the words of step s, requested by the caller (if s < st.end) as early as it likes; those of the wave's NEXT step are
// requested at the top of the current one, into a second set of SGPRs — not behind a round trip at the head of its chain.
template <typename Words, typename Fetch, typename Step>
__device__ __forceinline__ void walk(int s, const ItemSteps& st, Words nxt, Fetch&& fetch, Step&& step) {
    auto take = [&](const int cur) {
        const Words w = nxt;
        if (cur + WAVES < st.end) nxt = fetch(cur + WAVES);
        return w;
    };
    for (; s < st.b - 1; s += WAVES) step(take(s), s, SHAPE_A, FULL{});
    if (s == st.b - 1) step(take(s), s, SHAPE_A, LAST{}), s += WAVES;
    for (; s < st.c - 1; s += WAVES) step(take(s), s, SHAPE_B, FULL{});
    if (s == st.c - 1) step(take(s), s, SHAPE_B, LAST{}), s += WAVES;
    for (; s < st.end; s += WAVES) step(take(s), s, SHAPE_C, FULL{});
}

// The same over the five lists [A | A211 | B | B31 | C] of a mixed plan (dl_pair_hub_mixed: item_step has six boundaries).
struct MixedItemSteps { int a, a211, b, b31, c, end; };
__device__ __forceinline__ MixedItemSteps mixed_item_steps(const dl_pair_hub& h, int it) {
    return {h.item_step[6 * it],     h.item_step[6 * it + 1], h.item_step[6 * it + 2],
            h.item_step[6 * it + 3], h.item_step[6 * it + 4], h.item_step[6 * it + 5]};
}
template <typename Words, typename Fetch, typename Step>
__device__ __forceinline__ void walk(int s, const MixedItemSteps& st, Words nxt, Fetch&& fetch, Step&& step) {
    auto take = [&](const int cur) {
        const Words w = nxt;
        if (cur + WAVES < st.end) nxt = fetch(cur + WAVES);
        return w;
    };
    for (; s < st.a211 - 1; s += WAVES) step(take(s), s, SHAPE_A, FULL{});
    if (s == st.a211 - 1) step(take(s), s, SHAPE_A, LAST{}), s += WAVES;
    for (; s < st.b - 1; s += WAVES) step(take(s), s, SHAPE_A211, FULL{});
    if (s == st.b - 1) step(take(s), s, SHAPE_A211, LAST{}), s += WAVES;
    for (; s < st.b31 - 1; s += WAVES) step(take(s), s, SHAPE_B, FULL{});
    if (s == st.b31 - 1) step(take(s), s, SHAPE_B, LAST{}), s += WAVES;
    for (; s < st.c - 1; s += WAVES) step(take(s), s, SHAPE_B31, FULL{});
    if (s == st.c - 1) step(take(s), s, SHAPE_B31, LAST{}), s += WAVES;
    for (; s < st.end; s += WAVES) step(take(s), s, SHAPE_C, FULL{});
}

// A wave whose step ends in fewer lanes than it has keeps the results of NB steps side by side and runs ONE tail per batch:
// nb (wave-uniform) counts the steps captured since the last flush.  What a lane keeps, what open(first step) asks for — per
// lane, -1 for a step past the item's end: exactly the lanes that capture nothing — and what flush() does is the kernel's.
template <int NB, bool RARE_FLUSH>                                   // RARE_FLUSH: lay the flush out of line (a long batch)
struct Batch {
    int nb = 0;
    // behind every step: at NB captured steps flush, and open the batch that starts with the wave's next step
    template <typename Flush, typename Open>
    __device__ __forceinline__ void tick(int step, Flush&& flush, Open&& open) {
        if (RARE_FLUSH ? __builtin_expect(nb == NB, 0) : nb == NB) {
            flush(), nb = 0, open(step + WAVES);
        }
    }
    template <typename Flush>
    __device__ __forceinline__ void close(Flush&& flush) { if (nb > 0) flush(); }      // a wave with no step flushes nothing
};
}  // namespace dl::fast::hub
