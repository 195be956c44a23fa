"""The batched tail of hub::score_fwd_wave_kernel against the wave-per-entry kernel (PairList.build(hub_rows=0)): every
pair keeps its BITS — torch.equal of prob, and with want_coef of both arrays of terms.  No tolerance.

Without want_coef a wave of that kernel keeps the logits of up to 16 of its steps (s, s + 8, ...) in its lanes — lane L holds
slot L & 3 of the batch's step number L >> 2 — and runs one sigmoid and one store pass per batch: when 16 steps are captured
and once behind its last step.  The pair ids of a batch are read per lane when the batch opens.  What can go wrong depends
on how many steps a wave has and on where in a batch a list ends, so the lists here are chosen by the steps per wave
they give: 0, 1 and 2 (a rest only), 15, 16 (one full batch whose flush coincides with the end of the item), 17, 31, 32, 33
(two flushes and a rest of one), 35 and 36 with the transitions A -> B -> C inside batches, an item of 129 steps over all
three lists (one more than 8 waves x 16: besides 127 and 128 the lengths at which the closing flush changes — the walk and
the batch counter are dl_hub.h's, shared with the routing kernel), the last steps of A and of B and
a C step as a wave's 16th and 17th (dead slots at a batch's end and start), and many short items.  With want_coef the kernel
stores per step as before; those cases run the same lists.

Written like test_gpu_score_hub_pipeline.py: one block of 16 hub rows (0..15), one column slice, one work item per list
(HUB_ITEM_ROWS patched to 4096 and restored; 8 for the list of short items); the partners are node ids from 16 up: nA listed
by one row each (round robin: slots of A steps), nB by the rows (2i, 2i + 1) mod 16 (halves of B steps), nC by the rows
4i .. 4i + 3 mod 16 (C steps).  Every third listed pair is listed in the other direction too: folded, its entry carries a
second pair id; unfolded, the mirrors are entries of the rows that are no hub rows.  The steps per wave are asserted on a CPU
copy of item_step, so that a change of the plan builder fails here instead of silently covering less.  d = 64, K in {4, 8},
t in {1, 2}, folded and not, with and without want_coef.

The bits do not change with the batched tail: this test passes on the kernel with the per-step tail as well."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D = 640, 64

# name -> ((nA, nB, nC), work item length)
LISTS = {
    "512/0/0": ((512, 0, 0), 4096),
    "0/0/130": ((0, 0, 130), 4096),
    "0/0/264": ((0, 0, 264), 4096),
    "100/120/200": ((100, 120, 200), 4096),
    "509/3/1": ((509, 3, 1), 4096),
    "61/0/0": ((61, 0, 0), 4096),
    "0/0/3": ((0, 0, 3), 4096),
    "0/0/127": ((0, 0, 127), 4096),
    "0/0/255": ((0, 0, 255), 4096),
    "100/120/44": ((100, 120, 44), 4096),
    "20/16/12, items of 8": ((20, 16, 12), 8),
}
# steps per wave the issue's plans give (the first seven lists), and by arithmetic the next two
WANT_PER_WAVE = {"512/0/0": {16}, "0/0/130": {16, 17}, "0/0/264": {33}, "100/120/200": {35, 36}, "509/3/1": {16, 17},
                 "61/0/0": {2}, "0/0/3": {0, 1}, "0/0/127": {15, 16}, "0/0/255": {31, 32}, "100/120/44": {16, 17}}
WANT_ITEM_STEP = {"100/120/200": [0, 25, 85, 285], "509/3/1": [0, 128, 130, 131], "100/120/44": [0, 25, 85, 129]}
_lists, _tabs, _refs = {}, {}, {}


def _pairs(nA, nB, nC):
    pu, pv, v = [], [], 16
    for i in range(nA):
        pu.append(i % 16), pv.append(v)
        v += 1
    for i in range(nB):
        pu += [(2 * i) % 16, (2 * i + 1) % 16]
        pv += [v, v]
        v += 1
    for i in range(nC):
        pu += [(4 * i + j) % 16 for j in range(4)]
        pv += [v] * 4
        v += 1
    assert v <= N
    pu, pv = np.array(pu), np.array(pv)
    back = np.arange(0, pu.size, 3)                                 # every third pair in the other direction too
    pu, pv = np.concatenate([pu, pv[back]]), np.concatenate([pv, pu[back]])
    perm = np.random.default_rng(pu.size).permutation(pu.size)
    return pu[perm], pv[perm]


def _build(name, fold, hub=True, dev=DEV):
    from disenlink_amd import graph
    (nA, nB, nC), item_rows = LISTS[name]
    pu, pv = _pairs(nA, nB, nC)
    tu, tv = torch.from_numpy(pu).to(dev), torch.from_numpy(pv).to(dev)
    old = graph.HUB_ITEM_ROWS
    try:
        graph.HUB_ITEM_ROWS = item_rows
        return graph.PairList.build(tu, tv, N, n_slices=1, hub_rows=16 if hub else 0, fold_mirrors=fold)
    finally:
        graph.HUB_ITEM_ROWS = old


def steps_per_wave(item_step):
    """The numbers of steps of the 8 waves of every item (wave w takes the steps a + w, a + w + 8, ... below e)."""
    return {len(range(a + w, e, 8)) for a, b, c, e in item_step for w in range(8)}


def _plans(fold):
    if fold not in _lists:
        plans = {name: _build(name, fold) for name in LISTS}
        per_wave, lengths = set(), set()
        for name, pl in plans.items():
            h = pl.hub
            assert h is not None and h.n_blocks == 1, name
            (nA, nB, nC), item_rows = LISTS[name]
            st = h.item_step.cpu().tolist()
            assert (len(st) == 1) == (item_rows == 4096), name
            waves = steps_per_wave(st)
            if name in WANT_PER_WAVE:
                assert waves == WANT_PER_WAVE[name], (name, waves)
            if name in WANT_ITEM_STEP:
                assert st == [WANT_ITEM_STEP[name]], (name, st)
            per_wave |= waves
            lengths |= {e - a for a, b, c, e in st}
            assert (int((h.step_q2 >= 0).sum()) > 0) if fold else h.step_q2 is None, name
            if nA + nB + nC >= 16:                                   # (0, 0, 3) lists 12 of the 16 rows: unfolded, three partners are hub rows too
                assert h.block_row.cpu().tolist() == list(range(16)), name
                assert st[-1][3] == h.n_steps == (nA + 3) // 4 + (nB + 1) // 2 + nC, name
                assert h.n_entries == nA + 2 * nB + 4 * nC and (h.rest is None) == fold, name
        assert {0, 1, 2, 15, 16, 17, 31, 32, 33} <= per_wave and max(per_wave) >= 35, per_wave
        assert {127, 128, 129} <= lengths, lengths                  # 8 waves x 16 steps, one less, one more
        _lists[fold] = plans
    return _lists[fold]


def _tables(K):
    if K not in _tabs:
        from disenlink_amd import ops
        from disenlink_amd.graph import Graph
        rng = np.random.default_rng(700 + K)
        g = Graph.from_edge_rows(torch.from_numpy(rng.integers(0, N, 4000)), torch.from_numpy(rng.integers(0, N, 4000)), N).to(DEV)
        Z = (torch.randn(N, K, D, generator=torch.Generator().manual_seed(31 + K)) * 0.35).to(DEV).contiguous()
        H = ops.aggregate_fwd(g, Z, 0.5, *ops.route_fwd(g, Z, 1.0))
        _tabs[K] = (Z, H)
    return _tabs[K]


def _score(pl, K, t, want_coef):
    from disenlink_amd import ops
    Z, H = _tables(K)
    # prob is torch.empty: the allocator may hand back the block of an earlier result of the same list, which holds the right
    # bits already.  Blocks of that size are filled with NaN and freed first, so that a pair no lane stored is likely to show.
    junk = [torch.full((pl.pu.numel(),), float("nan"), device=DEV) for _ in range(4)]
    del junk
    out = ops.score_pairs_fwd(Z, H, pl.pu, pl.pv, t, pl, want_coef=want_coef)
    torch.cuda.synchronize()
    return out


def _ref(name, fold, K, t):
    """prob and terms of the plan without hub rows — computed once per case and left unchanged."""
    key = (LISTS[name][0], fold, K, t)
    if key not in _refs:
        plain = _build(name, fold, hub=False)
        assert plain.hub is None
        p, c = _score(plain, K, t, True)
        assert torch.equal(_score(plain, K, t, False), p) and bool(torch.isfinite(p).all()) and float(p.std()) > 0.02
        _refs[key] = (p.clone(), c[0].clone(), c[1].clone())
    return _refs[key]


@pytest.mark.parametrize("want_coef", [False, True], ids=["prob", "terms"])
@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("t", [1.0, 2.0])
@pytest.mark.parametrize("K", [4, 8])
def test_batched_tail_gives_the_bits_of_the_plain_plan(K, t, fold, want_coef):
    for name, pl in _plans(fold).items():
        ref_p, ref_e, ref_q = _ref(name, fold, K, t)
        if want_coef:
            got_p, got_c = _score(pl, K, t, True)
            assert torch.equal(got_p, ref_p), name
            assert torch.equal(got_c[0], ref_e) and torch.equal(got_c[1], ref_q), name
        else:
            got = _score(pl, K, t, False)
            assert torch.equal(got, ref_p), f"{name}: prob differs at {int((got != ref_p).sum())} of {ref_p.numel()} pairs"
