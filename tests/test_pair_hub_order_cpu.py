"""The hub plan (graph.HubPlan.build) as the forward kernel relies on it, on the CPU.  hub::score_fwd_wave_kernel gathers the
partner rows of every step but a list's last WITHOUT looking at them, so a dead partner row anywhere else would be a read
outside the tables.  The lists hold hub rows over a shared pool, rows with partners of their own (long A lists), a K4-like
clique listed in both directions, duplicate pairs and self pairs; the work items are cut at 8 (one list: 32) gathered
partner rows so that every list has many of them.

Checked: the plan decodes to the multiset of (u, v, q, q2) of the forward plan; dead partner rows sit only in the last
step of an item's A list and B list, behind the live ones; and n_gathered, n_steps and item_step are what the packing rule
gives (recomputed here in numpy from the forward plan alone), with every list in partner-row order inside its item.
(Sorting the A slots of an item by u_local for a one-row step form was measured and not kept — DESIGN.md section 8 — so
no order by u_local is asserted.)"""
import numpy as np
import pytest
import torch

from disenlink_amd import graph as G
from disenlink_amd.graph import HUB_W, PairList

ITEM_ROWS = 8


def _list(seed, n_nodes, n_hub, mirrors, private=0):
    rng = np.random.default_rng(seed)
    pu, pv = [], []
    order = rng.permutation(n_nodes)
    pool = order[:40]
    for u in range(2):                                              # partners no other row lists: A slots of ONE row
        pu += [u] * private
        pv += order[40 + u * private:40 + (u + 1) * private].tolist()
    for u in range(n_nodes):
        k = int(rng.integers(18, 36)) if u < n_hub else int(rng.integers(0, 4))
        v = rng.choice(pool if u < n_hub else n_nodes, size=k, replace=False)
        pu += [u] * k
        pv += v.tolist()
    clique = [n_hub, n_hub + 1, n_hub + 2, n_hub + 3]               # K4, every edge in both directions
    for a in clique:
        for b in clique:
            if a != b:
                pu.append(a), pv.append(b)
    pu += [0, 0, 3, 3, 3, n_hub + 5]                                # duplicate pairs
    pv += [int(pool[0]), int(pool[0]), int(pool[1]), int(pool[1]), int(pool[1]), 7]
    pu += [1, 2, n_hub + 7, n_nodes - 1]                            # self pairs, in hub rows and outside
    pv += [1, 2, n_hub + 7, n_nodes - 1]
    pu, pv = np.array(pu), np.array(pv)
    if mirrors:
        pick = rng.choice(pu.size, size=mirrors, replace=False)
        pu, pv = np.concatenate([pu, pv[pick]]), np.concatenate([pv, pu[pick]])
    perm = rng.permutation(pu.size)
    return torch.from_numpy(pu[perm]), torch.from_numpy(pv[perm])


LISTS = {
    "hubs, 8 slices": dict(seed=1, n_nodes=120, n_hub=40, mirrors=0, n_slices=8, hub_rows=None),
    "hubs, mirrored, 4 slices": dict(seed=2, n_nodes=100, n_hub=30, mirrors=300, n_slices=4, hub_rows=45),
    "hubs, one slice, short block": dict(seed=3, n_nodes=80, n_hub=21, mirrors=50, n_slices=1, hub_rows=21),
    "private partners, items of 32": dict(seed=4, n_nodes=90, n_hub=20, mirrors=0, n_slices=2, hub_rows=20, private=22, item_rows=32),
}
_built = {}


def build(name):
    if name not in _built:
        a = LISTS[name]
        pu, pv = _list(a["seed"], a["n_nodes"], a["n_hub"], a["mirrors"], a.get("private", 0))
        old = G.HUB_ITEM_ROWS
        try:
            G.HUB_ITEM_ROWS = a.get("item_rows", ITEM_ROWS)
            pl = PairList.build(pu, pv, a["n_nodes"], n_slices=a["n_slices"], hub_rows=a["hub_rows"],
                                **({} if a["hub_rows"] is not None else {"row_bytes": 2048}))
        finally:
            G.HUB_ITEM_ROWS = old
        assert pl.hub is not None and pl.hub.n_items >= 4
        _built[name] = pl
    return _built[name]


def fwd_entries(pl):
    """(u, v, q, q2) of every entry of the forward plan."""
    f = pl.fwd or pl.by_u
    u = torch.repeat_interleave(torch.arange(f.n_rows), (f.rowptr[1:] - f.rowptr[:-1]).long()) + f.row_offset
    q = (pl.fwd_pair if pl.fwd is not None else pl.by_u_pair).long()
    q2 = pl.fwd_pair2.long() if pl.fwd is not None and pl.fwd_pair2 is not None else torch.full_like(q, -1)
    return torch.stack([u, f.col.long(), q, q2], 1)


def hub_entries(pl):
    """(u, v, q, q2) of every live slot of the hub plan and every entry of its residual plan."""
    h = pl.hub
    rows = []
    for it in range(h.n_items):
        a, b, c, e = h.item_step[it].tolist()
        blk = int(h.item_block[it])
        for s in range(a, e):
            nv = 4 if s < b else 2 if s < c else 1
            for slot in range(4):
                q = int(h.step_q[s, slot])
                if q >= 0:
                    rows.append((int(h.block_row[blk * HUB_W + int(h.step_u[s, slot])]), int(h.step_v[s, slot * nv // 4]), q,
                                 int(h.step_q2[s, slot]) if h.step_q2 is not None else -1))
    if h.rest is not None:
        r = h.rest
        u = torch.repeat_interleave(torch.arange(r.n_rows), (r.rowptr[1:] - r.rowptr[:-1]).long()) + r.row_offset
        q2 = h.rest_pair2.tolist() if h.rest_pair2 is not None else [-1] * r.n_entries
        rows += list(zip(u.tolist(), r.col.tolist(), h.rest_pair.tolist(), q2))
    return rows


@pytest.mark.parametrize("name", list(LISTS))
def test_same_multiset_as_the_forward_plan(name):
    pl = build(name)
    want = sorted(map(tuple, fwd_entries(pl).tolist()))
    got = sorted(hub_entries(pl))
    assert got == want
    assert len({w[:2] for w in want}) < len(want)                   # duplicate pairs are in the list
    assert any(w[0] == w[1] for w in want)                          # and self pairs
    if "mirrored" in name:
        assert sum(w[3] >= 0 for w in want) > 20


@pytest.mark.parametrize("name", list(LISTS))
def test_dead_rows_only_close_a_list(name):
    h = build(name).hub
    tails = set()
    for it in range(h.n_items):
        a, b, c, e = h.item_step[it].tolist()
        assert bool((h.step_v[a:max(a, b - 1)] >= 0).all())                    # A: four rows in every step but the last
        assert bool((h.step_v[b:max(b, c - 1), :2] >= 0).all())                # B: two
        assert bool((h.step_v[c:e, 0] >= 0).all())                             # C: one, always
        for lo, hi, nv in ((a, b, 4), (b, c, 2)):
            if hi > lo:
                live = h.step_v[hi - 1, :nv] >= 0
                n = int(live.sum())
                assert n >= 1 and bool(live[:n].all())                         # dead rows behind the live ones
                tails.add((nv, n))
    if "private" not in name:
        assert {(4, 1), (4, 2), (4, 3), (4, 4), (2, 1), (2, 2)} <= tails, tails    # every tail length occurs


def _rule(pl, name):
    """(item_step rows as a sorted list, n_steps, n_gathered) from the forward plan and the packing rule alone: c slots of a
    (block, slice) on one partner row = c // 4 C steps, a B half for a remainder of 2 or 3, an A slot for 1 or 3; a new item
    where the groups before it have gathered a multiple of HUB_ITEM_ROWS partner rows."""
    h = pl.hub
    ent = fwd_entries(pl).numpy()
    n = pl.n_nodes
    cnt = np.bincount(ent[:, 0], minlength=n)
    rank = np.empty(n, np.int64)
    rank[np.argsort(-cnt, kind="stable")] = np.arange(n)
    m = rank[ent[:, 0]] < h.n_rows
    blk, v = rank[ent[m, 0]] // HUB_W, ent[m, 1]
    # the slice of a partner row, from the list's own column boundaries: the forward entries' columns cut into n_slices
    # runs of equal entry count (slice q = [bounds[q - 1], bounds[q])) — recomputed here, not read off the plan
    n_sl = LISTS[name]["n_slices"]
    cols = np.sort(ent[:, 1])
    bounds = cols[(np.arange(1, n_sl) * cols.size) // n_sl]
    sl = np.searchsorted(bounds, v, side="right")
    for it in range(h.n_items):                                     # and the plan puts every item's partner rows there
        a, b, c, e = h.item_step[it].tolist()
        w = h.step_v[a:e].reshape(-1).numpy()
        assert bool((np.searchsorted(bounds, w[w >= 0], side="right") == int(h.item_slice[it])).all())
    key, c = np.unique((blk * n_sl + sl) * n + v, return_counts=True)
    bs = key // n
    nC, hasB, hasA = c // 4, (c % 4 >= 2).astype(np.int64), (c % 2 == 1).astype(np.int64)
    gath = nC + hasB + hasA
    items, n_gathered = [], int(gath.sum())
    for g in np.unique(bs):
        idx = np.nonzero(bs == g)[0]
        cum = np.cumsum(gath[idx]) - gath[idx]
        part = cum // LISTS[name].get("item_rows", ITEM_ROWS)
        for p in np.unique(part):
            j = idx[part == p]
            items.append((int((hasA[j].sum() + 3) // 4), int((hasB[j].sum() + 1) // 2), int(nC[j].sum())))
    return sorted(items), sum(sum(i) for i in items), n_gathered


@pytest.mark.parametrize("name", list(LISTS))
def test_sizes_are_the_packing_rules(name):
    pl = build(name)
    h = pl.hub
    items, n_steps, n_gathered = _rule(pl, name)
    st = h.item_step
    got = sorted(zip((st[:, 1] - st[:, 0]).tolist(), (st[:, 2] - st[:, 1]).tolist(), (st[:, 3] - st[:, 2]).tolist()))
    assert got == items
    assert h.n_steps == n_steps and h.n_gathered == n_gathered
    assert torch.equal(st[1:, 0], st[:-1, 3]) and int(st[0, 0]) == 0 and int(st[-1, 3]) == h.n_steps
    # every list comes in partner-row order inside its item; an item holds a partner row at most once per list
    for it in range(h.n_items):
        a, b, c, e = st[it].tolist()
        vb = h.step_v[b:c, :2].reshape(-1)
        vb = vb[vb >= 0]
        assert bool((vb[1:] > vb[:-1]).all())
        vc = h.step_v[c:e, 0]
        assert bool((vc[1:] >= vc[:-1]).all())
        va = h.step_v[a:b].reshape(-1)
        va = va[va >= 0]
        assert bool((va[1:] > va[:-1]).all()) and (b - a) == (va.numel() + 3) // 4


@pytest.mark.parametrize("name", list(LISTS))
def test_check_refuses_a_dead_row_the_kernel_would_gather(name):
    """HubPlan.check (run when the plan is bound) passes what the builder emits and raises on a dead partner row in a full
    A or B step, in a C step, or in front of a live row of a list's last step."""
    import copy
    h = build(name).hub
    h.check()
    st = h.item_step.tolist()
    spots = []
    for a, b, c, e in st:
        if b - a > 1: spots.append((a, 3))                          # a full A step
        if c - b > 1: spots.append((b, 1))                          # a full B step
        if e > c: spots.append((e - 1, 0))                          # a C step
        if b > a and int((h.step_v[b - 1] >= 0).sum()) > 1: spots.append((b - 1, 0))     # dead in front of live
    kinds = {(s < b, s < c) for a, b, c, e in st for s, _ in spots if a <= s < e}
    assert len(spots) >= 4 and len(kinds) == 3
    for s, row in spots[:40]:
        bad = copy.copy(h)
        bad.step_v = h.step_v.clone()
        bad.step_v[s, row] = -1
        with pytest.raises(ValueError):
            bad.check()
