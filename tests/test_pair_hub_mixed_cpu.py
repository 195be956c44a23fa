"""The mixed hub plan of the forward scorer (graph.HubPlan.build_mixed, dl_pair_hub_mixed) as a data structure, on the CPU:
every listed pair is scored exactly once on its own two endpoints with the hub row the owner rule names, every (item,
partner row) is gathered once per C step and once for its remainder, every step has the slots of its list's shape with dead
slots and rows only where the kernel allows them, the plan is a function of the list alone, building it leaves
PairList.hub what it was, and on the benchmark's own list it gathers what the rule says: about 0.80 of the three-list plan.
Everything is compared on integers."""
import numpy as np
import pytest
import torch

from disenlink_amd import graph as G
from disenlink_amd.graph import HUB_W, HubPlan, PairList
from test_pair_hub_plan_cpu import LISTS as PLAN_LISTS

A, A211, B, B31, C = range(5)
SIZES = {A: (1, 1, 1, 1), A211: (2, 1, 1), B: (2, 2), B31: (3, 1), C: (4,)}      # slots per gathered row of every shape


def remainder_list():
    """Two blocks of 16 hub rows; each holds, three times over, groups of c = 1 ... 9 and 13 slots on one partner row, and one
    more group of 2 (an odd 2-piece): 3-pieces and 1-pieces for B31, 2-pieces for B, the odd one for A211, 1-pieces for A."""
    pu, pv, v = [], [], 32
    for blk in range(2):
        for rep in range(3):
            for c in (1, 2, 3, 4, 5, 6, 7, 8, 9, 13) + ((2,) if rep == 0 else ()):
                pu += [blk * 16 + (v + i) % 16 for i in range(c)]
                pv += [v] * c
                v += 1
    for u in range(32):                           # private partners: the 32 rows are the owners, and 0 .. 15 rank first
        k = 16 if u < 16 else 4
        pu += [u] * k
        pv += list(range(v, v + k))
        v += k
    return torch.tensor(pu), torch.tensor(pv), v, 1, 32


LISTS = dict(PLAN_LISTS, remainders=remainder_list)


def build(name, **kw):
    pu, pv, n, slices, T = LISTS[name]()
    return PairList.build(pu, pv, n, n_slices=slices, hub_rows=T, **kw), pu, pv


def forward_entries(pl):
    f = pl.fwd or pl.by_u
    row = np.repeat(np.arange(f.n_rows), np.diff(f.rowptr.numpy()))
    return row.astype(np.int64), f.col.numpy().astype(np.int64)


def owner_rule(fu, fv, n):
    """The owner rule in numpy: the endpoint with more forward entries over both endpoints, ties to the smaller id."""
    deg = np.bincount(np.concatenate([fu, fv]), minlength=n)
    swap = (deg[fv] > deg[fu]) | ((deg[fv] == deg[fu]) & (fv < fu))
    return np.where(swap, fv, fu), np.where(swap, fu, fv)


def decode(h):
    """list and item of every step; (step, slot, hub row, partner row) of every live slot"""
    assert h.mixed and tuple(h.item_step.shape) == (h.n_items, 6)
    list_of = torch.empty(h.n_steps, dtype=torch.long)
    item_of = torch.empty(h.n_steps, dtype=torch.long)
    for it in range(h.n_items):
        b = h.item_step[it].tolist()
        assert all(x <= y for x, y in zip(b, b[1:])) and b[5] > b[0]
        item_of[b[0]:b[5]] = it
        for l in range(5):
            list_of[b[l]:b[l + 1]] = l
    step, slot = torch.nonzero(h.step_q >= 0, as_tuple=True)
    smap = torch.tensor(G.HUB_MIXED_SHAPES)[list_of]                 # [n_steps, 4] slot -> row
    v = h.step_v[step, smap[step, slot]].long()
    u = h.block_row[h.item_block[item_of[step]].long() * HUB_W + h.step_u[step, slot].long()].long()
    return list_of, item_of, step, slot, u, v


def scored(pl):
    """(pair id, hub row, partner row) of everything the mixed plan and its residual score; second ids as (id, v, u)"""
    h = pl.hub_mixed
    _, _, step, slot, u, v = decode(h)
    ids, us, vs = [h.step_q[step, slot].long()], [u], [v]
    if h.step_q2 is not None:
        two = h.step_q2[step, slot] >= 0
        ids.append(h.step_q2[step, slot][two].long()); us.append(v[two]); vs.append(u[two])
    if h.rest is not None:
        r = h.rest
        row = torch.repeat_interleave(torch.arange(r.n_rows), (r.rowptr[1:] - r.rowptr[:-1]).long()) + r.row_offset
        ids.append(h.rest_pair.long()); us.append(row); vs.append(r.col.long())
        if h.rest_pair2 is not None:
            two = h.rest_pair2 >= 0
            ids.append(h.rest_pair2[two].long()); us.append(r.col.long()[two]); vs.append(row[two])
    return torch.cat(ids), torch.cat(us), torch.cat(vs)


@pytest.mark.parametrize("name", list(LISTS))
def test_every_pair_once_owner_is_hub_row(name):
    pl, pu, pv = build(name)
    h = pl.hub_mixed
    assert h is not None and h.n_items > 0 and pl.hub is not None
    ids, us, vs = scored(pl)
    assert ids.numel() == pu.numel() and torch.equal(torch.sort(ids).values, torch.arange(pu.numel()))
    listed = (us == pu[ids]) & (vs == pv[ids])
    swapped = (us == pv[ids]) & (vs == pu[ids])
    assert bool((listed | swapped).all())                             # on its own two endpoints, in either order
    assert h.n_entries + (h.rest.n_entries if h.rest is not None else 0) == (pl.fwd or pl.by_u).n_entries
    # the hub row of a FIRST id (hub slot or residual entry) is the endpoint the owner rule names
    fu, fv = forward_entries(pl)
    ou, _ = owner_rule(fu, fv, pl.n_nodes)
    f = pl.fwd or pl.by_u
    first = (pl.fwd_pair if pl.fwd is not None else pl.by_u_pair).long()
    want = torch.full((pu.numel(),), -1, dtype=torch.long)
    want[first] = torch.from_numpy(ou)
    n_first = h.n_entries + (h.rest.n_entries if h.rest is not None else 0)
    _, _, step, slot, u, _ = decode(h)
    assert torch.equal(u, want[h.step_q[step, slot].long()])
    if h.rest is not None:
        r = h.rest
        row = torch.repeat_interleave(torch.arange(r.n_rows), (r.rowptr[1:] - r.rowptr[:-1]).long()) + r.row_offset
        assert torch.equal(row, want[h.rest_pair.long()])
    assert n_first == f.n_entries
    if name in ("skewed", "mirrored"):
        assert int((ou != fu).sum()) > 0                              # some entry's owner is its second endpoint
    if name == "mirrored":
        assert h.step_q2 is not None and int((h.step_q2 >= 0).sum()) > 0


@pytest.mark.parametrize("name", list(LISTS))
def test_one_gather_per_remainder(name):
    pl, _, _ = build(name)
    h = pl.hub_mixed
    list_of, item_of, step, slot, u, v = decode(h)
    n = pl.n_nodes
    key, c = np.unique((item_of[step] * n + v).numpy(), return_counts=True)          # slots per (item, partner row)
    srow, sidx = torch.nonzero(h.step_v >= 0, as_tuple=True)
    gkey, g = np.unique((item_of[srow] * n + h.step_v[srow, sidx].long()).numpy(), return_counts=True)
    assert np.array_equal(key, gkey) and np.array_equal(g, c // 4 + (c % 4 > 0))
    # the total, by the rule alone: owners, ranks and blocks in numpy from the forward entries
    fu, fv = forward_entries(pl)
    ou, ov = owner_rule(fu, fv, n)
    cnt = np.bincount(ou, minlength=n)
    rank = np.empty(n, np.int64)
    rank[np.argsort(-cnt, kind="stable")] = np.arange(n)
    m = rank[ou] < h.n_rows
    _, cc = np.unique((rank[ou[m]] // HUB_W) * n + ov[m], return_counts=True)
    assert h.n_gathered == int((cc // 4 + (cc % 4 > 0)).sum())
    assert (h.rest.n_entries if h.rest is not None else 0) == int((~m).sum())
    if name == "remainders":
        # every item holds the groups it was built from, and all five lists
        per_item = {it: sorted(c[key // n == it].tolist()) for it in range(h.n_items)}
        assert h.n_items == 2 and all(sorted(set(x)) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 13] for x in per_item.values())
        assert bool(((h.item_step[:, 1:] - h.item_step[:, :-1]) > 0).all())
    # cutting long (block, slice) lists into work items changes neither
    old = G.HUB_MIXED_ITEM_ROWS
    try:
        G.HUB_MIXED_ITEM_ROWS = 8
        cut, pu, pv = build(name)
    finally:
        G.HUB_MIXED_ITEM_ROWS = old
    assert cut.hub_mixed.n_items > h.n_items and cut.hub_mixed.n_gathered == h.n_gathered
    assert torch.equal(torch.sort(scored(cut)[0]).values, torch.arange(pu.numel()))
    cut.hub_mixed.check()


def shape_errors(h):
    """What the contract forbids, counted: (steps whose slots do not match their list's shape, dead slots or rows elsewhere
    than at the end of the last step of a non-C list — or in the fourth slot of a C step, slots of one row with two partners)."""
    list_of, item_of, step, slot, u, v = decode(h)
    live = h.step_q >= 0
    smap = torch.tensor(G.HUB_MIXED_SHAPES)[list_of]
    nv = smap[:, 3] + 1
    used = torch.arange(4)[None, :] < nv[:, None]
    row_live = (h.step_v >= 0)
    bad_shape = int((row_live & ~used).sum())                          # a row the shape does not gather
    # a row is gathered exactly where its slots are live: all of them, or none
    slots_of_row = torch.stack([(smap == r) & live for r in range(4)], dim=1).sum(2)       # [n_steps, 4] live slots per row
    size = torch.stack([(smap == r).sum(1) for r in range(4)], dim=1)
    partial = (slots_of_row > 0) & (slots_of_row < size)
    is_c = list_of == C
    bad_shape += int((partial & ~is_c[:, None]).sum()) + int(((slots_of_row > 0) != row_live).sum())
    # C: row 0 alive, four live slots — or three, for a 3-piece without a partner
    bad_shape += int((is_c & ~(live[:, :3].all(1))).sum())
    last = torch.zeros(h.n_steps, dtype=torch.bool)
    for it in range(h.n_items):
        b = h.item_step[it].tolist()
        for l in range(4):
            if b[l + 1] > b[l]:
                last[b[l + 1] - 1] = True
    dead = ~live
    misplaced = int((dead.any(1) & ~last & ~is_c).sum()) + int((live[:, 1:] & dead[:, :-1]).sum()) + int(dead[:, 0].sum())
    return bad_shape, misplaced


@pytest.mark.parametrize("name", list(LISTS))
def test_shapes_and_dead_slots(name):
    pl, _, _ = build(name)
    h = pl.hub_mixed
    assert bool((h.step_u >= 0).all()) and bool((h.step_u < HUB_W).all())
    if h.step_q2 is not None:
        assert not bool(((h.step_q2 >= 0) & (h.step_q < 0)).any())
    assert shape_errors(h) == (0, 0)
    h.check()                                                       # accepts the builder's plan
    # every slot of a block names a row the block has
    list_of, item_of, step, slot, u, v = decode(h)
    assert bool((u >= 0).all())
    # steps are stored item by item without gaps; streams partition the items, slice by slice, largest first
    assert torch.equal(h.item_step[1:, 0], h.item_step[:-1, 5]) and int(h.item_step[-1, 5]) == h.n_steps
    s0 = h.slice_item0.tolist()
    assert s0[0] == 0 and s0[-1] == h.n_items and h.slice_max_item == max(y - x for x, y in zip(s0, s0[1:]))
    size = (h.item_step[:, 5] - h.item_step[:, 0]).tolist()
    for x in range(h.n_slices):
        key = [(int(h.item_slice[i]), -size[i]) for i in range(s0[x], s0[x + 1])]
        assert key == sorted(key) and all(k[0] % h.n_slices == x for k in key)


def test_check_refuses_a_dead_row_in_a_full_step():
    pl, _, _ = build("remainders")
    h = pl.hub_mixed
    a, a211 = int(h.item_step[0, 0]), int(h.item_step[0, 1])
    assert a211 - a >= 2                                              # list A of the first item has a full step
    for col in (3, 0):
        bad = h.to("cpu")
        bad.step_v = h.step_v.clone()
        bad.step_v[a, col] = -1
        with pytest.raises(ValueError):
            bad.check()
    # a live slot against a dead row of a LAST step is refused too (it would score against zeros)
    b31_last = int(h.item_step[0, 4]) - 1
    bad = h.to("cpu")
    bad.step_v = h.step_v.clone()
    bad.step_v[b31_last, 1] = -1
    bad.step_q = h.step_q.clone()
    bad.step_q[b31_last, 3] = 5
    with pytest.raises(ValueError):
        bad.check()
    # and a mixed plan is not bound where a three-list plan belongs
    with pytest.raises(ValueError):
        pl.hub.c_value_mixed()


def test_leftover_pieces():
    """An item with 3-pieces and no 1-piece: one closes list B31 with a dead second row, the others are C steps whose fourth
    slot is dead; an odd 2-piece without a 1-piece closes list B; with one 1-piece the A211 step has a dead third row."""
    def plan(groups):
        pu, pv, v = [], [], 16
        for c in groups:
            pu += list(range(c)); pv += [v] * c
            v += 1
        for u in range(16):                                           # 20 private partners keep the 16 rows the owners
            pu += [u] * 20; pv += list(range(v, v + 20))
            v += 20
        # items are cut at 4 gathered rows: the first item holds the groups whose gathers start below 4 — the private
        # partners, 1-pieces all, come behind them
        old = G.HUB_MIXED_ITEM_ROWS
        try:
            G.HUB_MIXED_ITEM_ROWS = 4
            h = PairList.build(torch.tensor(pu), torch.tensor(pv), v, n_slices=1, hub_rows=16).hub_mixed
        finally:
            G.HUB_MIXED_ITEM_ROWS = old
        assert shape_errors(h) == (0, 0)
        h.check()
        it = int((h.item_step[:, 0] == 0).nonzero()[0, 0])
        return h, h.item_step[it].tolist(), (h.item_step[it, 1:] - h.item_step[it, :-1]).tolist()
    live = lambda h, s: (h.step_q[s] >= 0).tolist()
    rows = lambda h, s: (h.step_v[s] >= 0).tolist()
    # groups 3, 3, 3, 7 (gathers start at 0, 1, 2, 3): four 3-pieces, no 1-piece, one C step of the 7
    h, b, lens = plan([3, 3, 3, 7])
    assert lens == [0, 0, 0, 1, 4]
    assert rows(h, b[3]) == [True, False, False, False] and live(h, b[3]) == [True, True, True, False]
    assert live(h, b[4]) == [True] * 4
    for s in range(b[4] + 1, b[5]):
        assert rows(h, s) == [True, False, False, False] and live(h, s) == [True, True, True, False]
    # groups 2, 2, 2, 4: the odd 2-piece finds no 1-piece and closes list B with a dead second row
    h, b, lens = plan([2, 2, 2, 4])
    assert lens == [0, 0, 2, 0, 1]
    assert rows(h, b[2]) == [True, True, False, False] and live(h, b[2]) == [True] * 4
    assert rows(h, b[2] + 1) == [True, False, False, False] and live(h, b[2] + 1) == [True, True, False, False]
    # groups 2, 2, 2 and the first private partner: the odd 2-piece and one 1-piece, an A211 step with a dead third row
    h, b, lens = plan([2, 2, 2])
    assert lens == [0, 1, 1, 0, 0]
    assert rows(h, b[1]) == [True, True, False, False] and live(h, b[1]) == [True, True, True, False]


@pytest.mark.parametrize("name", list(LISTS))
def test_same_plan_twice_and_hub_untouched(name):
    a, _, _ = build(name)
    b, _, _ = build(name)
    off, _, _ = build(name, hub_mixed=False)
    assert off.hub_mixed is None
    fields = ("block_row", "slice_item0", "item_block", "item_slice", "item_step", "step_v", "step_u", "step_q", "step_q2")
    same = lambda x, y: (x is None and y is None) or torch.equal(x, y)
    for f in fields:
        assert same(getattr(a.hub_mixed, f), getattr(b.hub_mixed, f)), f
        assert same(getattr(a.hub, f), getattr(off.hub, f)), f          # PairList.hub is what it is without the mixed plan
    for f in ("n_rows", "n_blocks", "n_items", "n_slices", "slice_max_item", "n_entries"):
        assert getattr(a.hub_mixed, f) == getattr(b.hub_mixed, f) and getattr(a.hub, f) == getattr(off.hub, f), f
    for x, y in ((a.hub_mixed, b.hub_mixed), (a.hub, off.hub)):
        assert (x.rest is None) == (y.rest is None)
        if x.rest is not None:
            for f in ("rowptr", "col", "seg_row", "seg_beg", "seg_end", "slice_seg0"):
                assert torch.equal(getattr(x.rest, f), getattr(y.rest, f)), f
            assert torch.equal(x.rest_pair, y.rest_pair) and same(x.rest_pair2, y.rest_pair2)


def test_no_hub_plan_no_mixed_plan():
    rng = np.random.default_rng(7)
    n = 4000
    pu = torch.from_numpy(np.repeat(np.arange(n), 6))
    pv = torch.from_numpy(rng.integers(0, n, size=pu.numel()))
    pl = PairList.build(pu, pv, n)
    assert pl.hub is None and pl.hub_mixed is None
    with pytest.raises(ValueError):
        PairList.build(pu, pv, n, hub_mixed=True)


def test_todays_packing_in_the_mixed_layout():
    """build_mixed(mixed=False), the A/B arm: the three-list packing — as many gathered rows as PairList.hub on the same
    orientation — in the five-list layout, lists A211 and B31 empty."""
    old = G.HUB_MIXED_OWNER, G.HUB_MIXED_SHAPES_ON
    try:
        G.HUB_MIXED_OWNER, G.HUB_MIXED_SHAPES_ON = False, False
        pl, pu, pv = build("skewed")
    finally:
        G.HUB_MIXED_OWNER, G.HUB_MIXED_SHAPES_ON = old
    h = pl.hub_mixed
    h.check()
    assert h.n_gathered == pl.hub.n_gathered and h.n_steps == pl.hub.n_steps and h.n_entries == pl.hub.n_entries
    lens = h.item_step[:, 1:] - h.item_step[:, :-1]
    assert int(lens[:, A211].sum()) == 0 and int(lens[:, B31].sum()) == 0
    ids, us, vs = scored(pl)
    assert torch.equal(torch.sort(ids).values, torch.arange(pu.numel())) and torch.equal(us, pu[ids]) and torch.equal(vs, pv[ids])


def test_squirrel_counts():
    """The benchmark's pair list (squirrel_real, the split of bench.build_workload, every row a hub row): 971,841 folded
    entries in ceil(971,841 / 4) = 242,961 steps plus the short last steps of the items' lists; the gathered row pairs are
    recomputed here by the rule alone (owners, ranks on the owners' entry counts, blocks of 16, one gather per C step and
    one per remainder) and come to 474,307 — below 0.82 of what PairList.hub gathers (589,665)."""
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.splits import make_link_split
    sg = synthetic_graph("squirrel_real", seed=0)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=0)
    pu = np.concatenate([split.pos_train.u, split.neg_train.u])
    pv = np.concatenate([split.pos_train.v, split.neg_train.v])
    order = np.lexsort((pv, pu))
    pl = PairList.build(torch.from_numpy(pu[order]), torch.from_numpy(pv[order]), sg.n_nodes)
    h, N = pl.hub_mixed, sg.n_nodes
    assert pl.n_pairs == 1009603 and pl.fwd.n_entries == 971841
    assert h is not None and h.rest is None and pl.hub.rest is None and h.n_entries == 971841
    assert int((h.step_q >= 0).sum()) == 971841
    lists = 4 * h.n_items                                             # each non-C list of an item may end in a short step
    print(f"squirrel_real: {h.n_steps} steps in {h.n_items} items")
    assert 242961 <= h.n_steps <= 242961 + lists
    fu, fv = forward_entries(pl)
    ou, ov = owner_rule(fu, fv, N)
    cnt = np.bincount(ou, minlength=N)
    rank = np.empty(N, np.int64)
    rank[np.argsort(-cnt, kind="stable")] = np.arange(N)
    _, c = np.unique((rank[ou] // 16) * N + ov, return_counts=True)
    want = int((c // 4 + (c % 4 > 0)).sum())
    print(f"squirrel_real: {want} gathered row pairs, {pl.hub.n_gathered} on the three-list plan = {want / pl.hub.n_gathered:.3f}")
    assert h.n_gathered == want
    assert want / pl.hub.n_gathered < 0.82
    assert shape_errors(h) == (0, 0)
    h.check()
