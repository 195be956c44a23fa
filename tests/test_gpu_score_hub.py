"""The forward scorer over a hub plan (graph.HubPlan, dl_pair_hub; hub::score_fwd_wave_kernel) against the same call on the
plan without hub rows (PairList.build(hub_rows=0), the wave-per-entry kernel alone): the probabilities, and with
want_coef both arrays of stored terms, must be the same BITS — a hub slot runs the arithmetic of an entry, only the row it
scores against is shared with up to three other slots.

N = 96, d = 64, K in {4, 8}, t in {1, 2}, 1 and 8 column slices, fp32, on ONE list of about 3 k pairs whose hub plan (37 hub
rows) is asserted to hold: a last block of 5 rows; partner rows with 1, 2, 3, 4, 5, 7 and 16 slots inside one block; A lists
that end on 1, 2 and 3 live slots and a B list that ends on a single half (a C step has four live slots by construction); work
items with an empty A, B or C list; second pair ids (mirrored pairs); self pairs in hub rows and in residual rows; rows left to the residual
plan; and, with the item length cut to 8 partner rows, (block, slice) lists cut into several work items.  Also: a list
without hubs gets no hub plan and the call is what it was; two calls give the same bits; DL_FWD_HUB=0 walks the whole
forward plan and gives them too; and a call into sentinel-filled buffers writes every listed id once and nothing else."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D, T_HUB = 96, 64, 37
SENTINEL = -7.0


def _pair_list():
    rng = np.random.default_rng(11)
    pu, pv = [], []

    def add(u, v):
        pu.extend(np.atleast_1d(u).tolist())
        pv.extend(np.atleast_1d(v).tolist())

    shared = {40: 16, 41: 7, 42: 5, 43: 4, 44: 3, 45: 2, 46: 1}     # partner row -> how many of the rows 0..15 list it
    for u in range(N):
        if u < 16:
            k, lo = int(rng.integers(62, 70)), 17                   # the first block: the longest rows
        elif u < 32:
            k, lo = int(rng.integers(50, 57)), 0
        elif u < T_HUB:
            k, lo = int(rng.integers(24, 28)), 0                    # the five rows of the last block
        else:
            k, lo = int(rng.integers(0, 17)), 0                     # residual rows, some of them empty
        pool = np.setdiff1d(np.arange(lo, N), list(shared)) if u < 16 else np.arange(lo, N)
        v = rng.choice(pool, size=k, replace=False)
        if u < 16:
            v = np.concatenate([v, [w for w, c in shared.items() if u < c]])
        add(np.full(v.size, u), v)
    add([5, 20, 33], [5, 20, 33])                                   # self pairs in hub rows
    keep = np.unique(np.stack([pu, pv], 1), axis=0, return_index=True)[1]
    keep.sort()
    pu, pv = np.array(pu)[keep], np.array(pv)[keep]
    perm = rng.permutation(pu.size)
    return pu[perm], pv[perm]


def _check_features(pl, cut):
    """The list is what the docstring says (all on the CPU copy of the plan; list tails and empty lists counted over the
    plan and its copy with short work items — one slice has only three (block, slice) lists)."""
    a_tail, b_tail, empty = set(), set(), set()
    for h in (pl.hub, cut.hub):
        live = h.step_q.cpu() >= 0
        for a, b, c, e in h.item_step.cpu().tolist():
            if b > a: a_tail.add(int(live[b - 1].sum()))
            if c > b: b_tail.add(int(live[c - 1].sum()))
            empty |= {n for n, (lo, hi) in zip("ABC", ((a, b), (b, c), (c, e))) if hi == lo}
    assert {1, 2, 3} <= a_tail and 2 in b_tail, (a_tail, b_tail)
    assert empty == {"A", "B", "C"}, empty
    h = pl.hub
    assert h is not None and h.n_rows == T_HUB and h.n_blocks == 3
    block_row = h.block_row.cpu().reshape(-1, 16)
    assert int((block_row[2] >= 0).sum()) == 5 and sorted(block_row[0].tolist()) == list(range(16))
    steps, sv, sq, sq2 = h.item_step.cpu(), h.step_v.cpu(), h.step_q.cpu(), h.step_q2.cpu()
    live = sq >= 0
    mult = {}
    for it in range(h.n_items):
        a, b, c, e = steps[it].tolist()
        if int(h.item_block[it]) == 0:
            for s in range(a, e):
                nv = 4 if s < b else 2 if s < c else 1
                for slot in range(4):
                    if live[s, slot]:
                        v = int(sv[s, slot * nv // 4])
                        mult[v] = mult.get(v, 0) + 1
    assert {40: 16, 41: 7, 42: 5, 43: 4, 44: 3, 45: 2, 46: 1}.items() <= mult.items(), mult
    assert int((sq2 >= 0).sum()) > 20                              # mirrored pairs inside the hub steps
    assert h.rest is not None and h.rest.n_entries > 100 and int((h.rest_pair2 >= 0).sum()) > 0
    pu, pv = pl.pu.cpu(), pl.pv.cpu()
    self_ids = set(torch.nonzero(pu == pv).reshape(-1).tolist())
    assert len(self_ids & set(sq[live].tolist())) >= 3 and len(self_ids & set(h.rest_pair.cpu().tolist())) >= 1


_shared = {}


def _lists(n_slices):
    """(pu, pv, hub plan, the same with short work items, no hub rows) for this slicing — built once."""
    if n_slices not in _shared:
        from disenlink_amd import graph
        pu, pv = _pair_list()
        assert 2500 <= pu.size <= 3500
        tu, tv = torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV)
        hub = graph.PairList.build(tu, tv, N, n_slices=n_slices, hub_rows=T_HUB)
        plain = graph.PairList.build(tu, tv, N, n_slices=n_slices, hub_rows=0)
        old = graph.HUB_ITEM_ROWS
        try:
            graph.HUB_ITEM_ROWS = 8
            cut = graph.PairList.build(tu, tv, N, n_slices=n_slices, hub_rows=T_HUB)
        finally:
            graph.HUB_ITEM_ROWS = old
        assert plain.hub is None and hub.fwd is not None and cut.hub.n_items > hub.hub.n_items
        _check_features(hub, cut)
        _shared[n_slices] = (pu, pv, hub, cut, plain)
    return _shared[n_slices]


_tabs = {}


def _tables(K):
    if K not in _tabs:
        from disenlink_amd import ops
        from disenlink_amd.graph import Graph
        rng = np.random.default_rng(200 + K)
        g = Graph.from_edge_rows(torch.from_numpy(rng.integers(0, N, 700)), torch.from_numpy(rng.integers(0, N, 700)), N).to(DEV)
        Z = (torch.randn(N, K, D, generator=torch.Generator().manual_seed(7 + K)) * 0.35).to(DEV).contiguous()
        H = ops.aggregate_fwd(g, Z, 0.5, *ops.route_fwd(g, Z, 1.0))
        _tabs[K] = (Z, H)
    return _tabs[K]


def _score(pl, K, t, want_coef):
    from disenlink_amd import ops
    Z, H = _tables(K)
    out = ops.score_pairs_fwd(Z, H, pl.pu, pl.pv, t, pl, want_coef=want_coef)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n_slices", [1, 8])
@pytest.mark.parametrize("t", [1.0, 2.0])
@pytest.mark.parametrize("K", [4, 8])
def test_hub_plan_gives_the_bits_of_the_plain_plan(K, t, n_slices):
    pu, pv, hub, cut, plain = _lists(n_slices)
    ref = _score(plain, K, t, False)
    ref_p, ref_c = _score(plain, K, t, True)
    assert torch.equal(ref, ref_p) and bool(torch.isfinite(ref).all()) and float(ref.std()) > 0.05      # (self pairs saturate to 1)
    for pl in (hub, cut):
        got = _score(pl, K, t, False)
        assert torch.equal(got, ref), f"prob differs at {int((got != ref).sum())} of {ref.numel()} pairs"
        got_p, got_c = _score(pl, K, t, True)
        assert torch.equal(got_p, ref)
        assert torch.equal(got_c[0], ref_c[0]) and torch.equal(got_c[1], ref_c[1])


def test_twice_the_same_and_switch_off():
    from disenlink_amd import _lib
    pu, pv, hub, cut, plain = _lists(8)
    a, b = _score(hub, 8, 1.0, False), _score(hub, 8, 1.0, False)
    assert torch.equal(a, b)
    os.environ["DL_FWD_HUB"] = "0"
    _lib.config_reload()
    try:
        off = _score(hub, 8, 1.0, False)
    finally:
        del os.environ["DL_FWD_HUB"]
        _lib.config_reload()
    assert torch.equal(off, a) and torch.equal(_score(plain, 8, 1.0, False), a)


@pytest.mark.parametrize("want_coef", [False, True])
def test_writes_every_listed_id_and_nothing_else(want_coef):
    """Straight into the library with sentinel-filled buffers of P + 7 slots."""
    from disenlink_amd import _lib, ops
    pu, pv, hub, cut, plain = _lists(8)
    K, P = 8, pu.size
    Z, H = _tables(K)
    lib = _lib.load()
    outs = []
    for pl in (hub, plain):
        prob = torch.full((P + 7,), SENTINEL, device=DEV)
        cf = torch.full((2, P, K), SENTINEL, device=DEV) if want_coef else None
        _lib.check(lib.dl_score_pairs_fwd(Z.data_ptr(), H.data_ptr(), N, K, D, _lib.DL_F32, 1.0, pl.pu.data_ptr(),
                                          pl.pv.data_ptr(), P, pl.c_struct_by_u(), prob.data_ptr(),
                                          cf.data_ptr() if cf is not None else None, ops._stream()), "dl_score_pairs_fwd")
        torch.cuda.synchronize()
        assert bool((prob[P:] == SENTINEL).all()) and bool((prob[:P] != SENTINEL).all())
        if cf is not None:
            assert bool((cf != SENTINEL).all())
        outs.append((prob, cf))
    assert torch.equal(outs[0][0], outs[1][0])
    if want_coef:
        assert torch.equal(outs[0][1], outs[1][1])


def test_list_without_hubs_is_unchanged():
    """Automatic selection on a uniform sparse list: no hub plan, the forward plan and the call are what hub_rows=0 gives."""
    from disenlink_amd.graph import PairList
    u = np.arange(N)                                               # two partners per row, no partner twice in 16 rows
    pu = torch.from_numpy(np.repeat(u, 2)).to(DEV)
    pv = torch.from_numpy(np.stack([(u + 1) % N, (u + 17) % N], 1).reshape(-1)).to(DEV)
    auto, off = PairList.build(pu, pv, N), PairList.build(pu, pv, N, hub_rows=0)
    assert auto.hub is None
    for f in ("seg_row", "seg_beg", "seg_end", "col"):
        assert torch.equal(getattr(auto.fwd or auto.by_u, f), getattr(off.fwd or off.by_u, f))
    assert not bool(auto.c_struct_by_u()._obj.hub)
    assert torch.equal(_score(auto, 8, 1.0, False), _score(off, 8, 1.0, False))
