"""What one wave of hub::score_fwd_wave_kernel carries from a step to its next one (s, s + 8), against the wave-per-entry
kernel (PairList.build(hub_rows=0)): every pair keeps its BITS — torch.equal of prob, and with want_coef of both arrays of
terms.  No tolerance.

Written for a kernel that gathers the partner rows of step s + 8 between the dot products and the tail of step s, into
the registers step s has just read, and the rows of a wave's first step ahead of the staging barrier.  That kernel gave
these bits and no time (profiles/r12_fwd_hub_pipeline.txt) and is not the one in the tree; the
shipped kernel keeps the plan words of step s + 8 across step s and nothing else.  Any form that keeps more — registers,
loads in flight — depends on the pair (form of step s, form of step s + 8) of one wave, which the plans of
test_gpu_score_hub_steps.py barely hold, so the lists here are built to hold every such pair.  One block of 16 hub rows (0..15), one column slice, one work item per list (HUB_ITEM_ROWS patched to 4096 and
restored); the partners are node ids from 16 up: nA listed by one row each (round robin: slots of A steps), nB by the rows
(2i, 2i + 1) mod 16 (halves of B steps), nC by the rows 4i .. 4i + 3 mod 16 (C steps).  Asserted on a CPU copy of
item_step: all thirteen pairs of forms (A, A-last, B, B-last, C; a list's last step never precedes a step of the same
list), waves with no step, one step, exactly two steps and four or more, an item of at most 8 steps (no rotation at all)
and, with HUB_ITEM_ROWS = 8, several items the last of which ends on the last row of the step arrays.  Every third listed
pair is listed in the other direction too: folded, its entry carries a second pair id; unfolded, the mirrors are entries of
the rows that are no hub rows.  d = 64, K in {4, 8}, t in {1, 2}, folded and not, with and without want_coef."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D = 272, 64

# name -> ((nA, nB, nC), work item length)
LISTS = {
    "190/40/20": ((190, 40, 20), 4096),
    "20/16/12": ((20, 16, 12), 4096),
    "12/22/0": ((12, 22, 0), 4096),
    "81/0/30": ((81, 0, 30), 4096),
    "0/40/3": ((0, 40, 3), 4096),
    "8/14/4": ((8, 14, 4), 4096),
    "20/16/12, items of 8": ((20, 16, 12), 8),
}
FORMS = ("A", "A-last", "B", "B-last", "C")
WANT_PAIRS = {("A", "A"), ("A", "A-last"), ("A", "B"), ("A", "B-last"), ("A", "C"), ("A-last", "B"), ("A-last", "B-last"),
              ("A-last", "C"), ("B", "B"), ("B", "B-last"), ("B", "C"), ("B-last", "C"), ("C", "C")}
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


def _build(name, fold, hub=True):
    from disenlink_amd import graph
    (nA, nB, nC), item_rows = LISTS[name]
    pu, pv = _pairs(nA, nB, nC)
    tu, tv = torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV)
    old = graph.HUB_ITEM_ROWS
    try:
        graph.HUB_ITEM_ROWS = item_rows
        return graph.PairList.build(tu, tv, N, n_slices=1, hub_rows=16 if hub else 0, fold_mirrors=fold)
    finally:
        graph.HUB_ITEM_ROWS = old


def form(n, b, c):
    return "A" if n < b - 1 else "A-last" if n == b - 1 else "B" if n < c - 1 else "B-last" if n == c - 1 else "C"


def wave_walks(item_step):
    """(pairs of forms (step s, step s + 8), steps per wave, steps per item) over all waves of all items."""
    pairs, per_wave, per_item = set(), set(), []
    for a, b, c, e in item_step:
        per_item.append(e - a)
        for w in range(8):
            steps = list(range(a + w, e, 8))
            per_wave.add(len(steps))
            pairs |= {(form(s, b, c), form(t, b, c)) for s, t in zip(steps, steps[1:])}
    return pairs, per_wave, per_item


def _plans(fold):
    if fold not in _lists:
        plans = {name: _build(name, fold) for name in LISTS}
        pairs, per_wave, short = set(), set(), False
        for name, pl in plans.items():
            h = pl.hub
            assert h is not None and h.n_blocks == 1 and h.block_row.cpu().tolist() == list(range(16)), name
            (nA, nB, nC), item_rows = LISTS[name]
            st = h.item_step.cpu().tolist()
            assert st[-1][3] == h.n_steps == (nA + 3) // 4 + (nB + 1) // 2 + nC, name
            assert (len(st) == 1) == (item_rows == 4096), name
            got, waves, per_item = wave_walks(st)
            pairs |= got
            per_wave |= waves
            short |= min(per_item) <= 8
            assert h.n_entries == nA + 2 * nB + 4 * nC and (h.rest is None) == fold, name
            assert (int((h.step_q2 >= 0).sum()) > 0) if fold else h.step_q2 is None, name
        assert pairs == WANT_PAIRS, (WANT_PAIRS - pairs, pairs - WANT_PAIRS)
        assert {0, 1, 2} <= per_wave and max(per_wave) >= 4 and short, per_wave
        _lists[fold] = plans
    return _lists[fold]


def _tables(K):
    if K not in _tabs:
        from disenlink_amd import ops
        from disenlink_amd.graph import Graph
        rng = np.random.default_rng(500 + K)
        g = Graph.from_edge_rows(torch.from_numpy(rng.integers(0, N, 2000)), torch.from_numpy(rng.integers(0, N, 2000)), N).to(DEV)
        Z = (torch.randn(N, K, D, generator=torch.Generator().manual_seed(29 + K)) * 0.35).to(DEV).contiguous()
        H = ops.aggregate_fwd(g, Z, 0.5, *ops.route_fwd(g, Z, 1.0))
        _tabs[K] = (Z, H)
    return _tabs[K]


def _score(pl, K, t, want_coef):
    from disenlink_amd import ops
    Z, H = _tables(K)
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
def test_rotated_steps_give_the_bits_of_the_plain_plan(K, t, fold, want_coef):
    for name, pl in _plans(fold).items():
        ref_p, ref_e, ref_q = _ref(name, fold, K, t)
        if want_coef:
            got_p, got_c = _score(pl, K, t, True)
            assert torch.equal(got_p, ref_p), name
            assert torch.equal(got_c[0], ref_e) and torch.equal(got_c[1], ref_q), name
        else:
            got = _score(pl, K, t, False)
            assert torch.equal(got, ref_p), f"{name}: prob differs at {int((got != ref_p).sum())} of {ref_p.numel()} pairs"
