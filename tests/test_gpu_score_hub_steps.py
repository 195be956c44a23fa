"""The step forms of hub::score_fwd_wave_kernel against the wave-per-entry kernel (PairList.build(hub_rows=0)): full steps
run without dead-row handling (no sign test, no zero fill, gathers unconditional), the last step of an item's A list and B
list with it, and the plan words of a wave's next step are requested one step ahead, never past the item's end — and every
pair keeps its BITS: torch.equal of prob, and with want_coef of both arrays of terms.

N = 96, d = 64, K in {4, 8}, t in {1, 2}, mirrors folded and not, with and without want_coef, on two lists (about 2,000 and
150 pairs) under four plans that are asserted to hold, among their work items: an A list of 0 steps, of 1 step, of exactly
4 k live slots (no dead row in its last step), last A steps of 1, 2 and 3 live rows, a B list of an odd number of halves, an
item of C steps only, A steps on one u row next to mixed ones, a block of fewer than 16 rows, an item of fewer than 8 steps
(some waves get none) and an item of a single step.  A plan whose A slots are shuffled after the build gives the same bits:
the kernel asks nothing of their order.
("A steps on one u row next to mixed ones" exercises no path of its own in the shipped kernel, where every slot reads its own
u row: a one-row step form was measured and not kept, DESIGN.md section 8.  The case stays for such a form.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D = 96, 64


def _wide():
    """37 hub rows (a last block of 5) over a shared pool, rows 0 and 1 with partners of their own, mirrors, self pairs."""
    rng = np.random.default_rng(23)
    pu, pv = [], []
    pool = np.arange(30, 70)
    for u in range(N):
        k = int(rng.integers(40, 58)) if u < 16 else int(rng.integers(28, 36)) if u < 32 else int(rng.integers(18, 22)) if u < 37 \
            else int(rng.integers(0, 9))
        v = rng.choice(pool if u < 37 else N, size=min(k, pool.size if u < 37 else N), replace=False)
        pu += [u] * v.size
        pv += v.tolist()
    for u, own in ((0, range(70, 96)), (1, range(72, 90))):          # partners no other row of the block lists
        pu += [u] * len(own)
        pv += list(own)
    pu += [5, 20, 33, 50]
    pv += [5, 20, 33, 50]
    pu, pv = np.array(pu), np.array(pv)
    pick = rng.choice(pu.size, size=500, replace=False)             # listed in both directions
    pu, pv = np.concatenate([pu, pv[pick]]), np.concatenate([pv, pu[pick]])
    keep = np.unique(np.stack([pu, pv], 1), axis=0, return_index=True)[1]
    keep.sort()
    perm = rng.permutation(keep.size)
    return pu[keep][perm], pv[keep][perm]


def _c_only():
    """16 rows that all list the same 8 partners (C steps only), and a few rows outside the hub rows."""
    u, v = np.meshgrid(np.arange(16), np.arange(40, 48), indexing="ij")
    pu, pv = u.reshape(-1).tolist(), v.reshape(-1).tolist()
    for w in range(60, 70):
        pu += [w, w]
        pv += [w - 50, w + 10]
    return np.array(pu), np.array(pv)


# name -> (list, hub rows, column slices, work item length)
PLANS = {
    "wide": (_wide, 37, 8, 256),
    "wide, items of 8": (_wide, 37, 8, 8),
    "wide, one slice, items of 24": (_wide, 37, 1, 24),
    "C only": (_c_only, 16, 1, 256),
}
_lists, _tabs, _refs = {}, {}, {}


def _build(name, fold, dev=DEV, hub=True):
    from disenlink_amd import graph
    make, T, n_slices, item_rows = PLANS[name]
    pu, pv = make()
    tu, tv = torch.from_numpy(pu).to(dev), torch.from_numpy(pv).to(dev)
    old = graph.HUB_ITEM_ROWS
    try:
        graph.HUB_ITEM_ROWS = item_rows
        return graph.PairList.build(tu, tv, N, n_slices=n_slices, hub_rows=T if hub else 0, fold_mirrors=fold)
    finally:
        graph.HUB_ITEM_ROWS = old


def features(plans):
    """What the items of these plans hold, as a set of names (on a CPU copy of the plan arrays)."""
    got = set()
    for pl in plans:
        h = pl.hub
        st, sv, su, sq = h.item_step.cpu(), h.step_v.cpu(), h.step_u.cpu(), h.step_q.cpu()
        if int((h.block_row.cpu().reshape(-1, 16) >= 0).sum(1).min()) < 16:
            got.add("short block")
        for a, b, c, e in st.tolist():
            got.add(f"A list of {b - a} steps" if b - a < 2 else "A list of several steps")
            if b > a:
                n = int((sv[b - 1] >= 0).sum())
                got.add(f"last A step of {n} live rows")
            if c > b and int((sv[c - 1, :2] >= 0).sum()) == 1:
                got.add("odd B halves")
            if a == b == c and e > c:
                got.add("C only")
            if e - a < 8:
                got.add("fewer than 8 steps")
            if e - a == 1:
                got.add("single step")
            one = [len(set(su[s].tolist())) == 1 and bool((sq[s] >= 0).all()) for s in range(a, b)]
            if any(x != y for x, y in zip(one, one[1:])):
                got.add("same-row next to mixed")
    return got


WANT = {"short block", "A list of 0 steps", "A list of 1 steps", "A list of several steps", "last A step of 1 live rows",
        "last A step of 2 live rows", "last A step of 3 live rows", "last A step of 4 live rows", "odd B halves", "C only",
        "fewer than 8 steps", "single step", "same-row next to mixed"}


def _plans(fold):
    if fold not in _lists:
        plans = {name: _build(name, fold) for name in PLANS}
        assert all(pl.hub is not None for pl in plans.values())
        missing = WANT - features(plans.values())
        assert not missing, missing
        assert 1000 < plans["wide"].n_pairs < 4000
        if fold:
            assert int((plans["wide"].hub.step_q2 >= 0).sum()) > 50
        _lists[fold] = plans
    return _lists[fold]


def _tables(K):
    if K not in _tabs:
        from disenlink_amd import ops
        from disenlink_amd.graph import Graph
        rng = np.random.default_rng(300 + K)
        g = Graph.from_edge_rows(torch.from_numpy(rng.integers(0, N, 700)), torch.from_numpy(rng.integers(0, N, 700)), N).to(DEV)
        Z = (torch.randn(N, K, D, generator=torch.Generator().manual_seed(17 + K)) * 0.35).to(DEV).contiguous()
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
    key = (PLANS[name][0], PLANS[name][2], fold, K, t)
    if key not in _refs:
        plain = _build(name, fold, hub=False)
        assert plain.hub is None
        p, c = _score(plain, K, t, True)
        assert torch.equal(_score(plain, K, t, False), p) and bool(torch.isfinite(p).all()) and float(p.std()) > 0.05
        _refs[key] = (p.clone(), c[0].clone(), c[1].clone())
    return _refs[key]


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("t", [1.0, 2.0])
@pytest.mark.parametrize("K", [4, 8])
def test_step_forms_give_the_bits_of_the_plain_plan(K, t, fold):
    for name, pl in _plans(fold).items():
        ref_p, ref_e, ref_q = _ref(name, fold, K, t)
        got = _score(pl, K, t, False)
        assert torch.equal(got, ref_p), f"{name}: prob differs at {int((got != ref_p).sum())} of {ref_p.numel()} pairs"
        got_p, got_c = _score(pl, K, t, True)
        assert torch.equal(got_p, ref_p), name
        assert torch.equal(got_c[0], ref_e) and torch.equal(got_c[1], ref_q), name


@pytest.mark.parametrize("name", ["wide", "wide, one slice, items of 24"])
def test_shuffled_a_slots_give_the_same_bits(name):
    """The live A slots of every item permuted after the build (the list stays packed: dead rows only in its last step)."""
    K, t = 8, 1.0
    pl = _build(name, True)
    h = pl.hub
    rng = np.random.default_rng(5)
    st = h.item_step.cpu().tolist()
    arrays = [h.step_v, h.step_u, h.step_q, h.step_q2]
    moved = n_a = 0
    for a, b, _, _ in st:
        if b > a:
            flat = [x[a:b].reshape(-1) for x in arrays]
            n = int((flat[2] >= 0).sum())
            perm = torch.from_numpy(rng.permutation(n)).to(DEV)
            moved += int((perm != torch.arange(n, device=DEV)).sum())
            n_a += n
            for x, f in zip(arrays, flat):
                f[:n] = f[:n][perm]
                x[a:b] = f.reshape(-1, 4)
    assert n_a >= 40 and moved >= n_a // 2                      # a random permutation leaves about one slot per item in place
    ref_p, ref_e, ref_q = _ref(name, True, K, t)
    got_p, got_c = _score(pl, K, t, True)
    assert torch.equal(got_p, ref_p) and torch.equal(got_c[0], ref_e) and torch.equal(got_c[1], ref_q)
    assert torch.equal(_score(pl, K, t, False), ref_p)
