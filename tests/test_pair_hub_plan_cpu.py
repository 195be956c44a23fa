"""The hub plan of the forward scorer (graph.HubPlan, dl_pair_hub) as a data structure, on the CPU: every listed pair is
scored exactly once by a hub slot or a residual entry, every slot sits on its own endpoints, the three step shapes keep
their slots on the right partner row, dead slots only close a list, the plan is a function of the list alone, and the
block rule gives the counts the kernel's design was argued from on the benchmark's own pair list."""
import numpy as np
import pytest
import torch

from disenlink_amd import graph as G
from disenlink_amd.graph import HUB_W, PairList


def skewed_list(n_nodes, n_hub, hub_deg, tail_deg, seed, mirrors=0):
    """n_hub rows of about hub_deg pairs that share a pool of partners, every other row tail_deg random ones."""
    rng = np.random.default_rng(seed)
    pu, pv = [], []
    pool = rng.permutation(n_nodes)[: max(4, 2 * hub_deg)]
    for u in range(n_nodes):
        if u < n_hub:
            k = max(1, int(hub_deg * (0.5 + rng.random())))
            v = rng.choice(pool, size=min(k, pool.size), replace=False)
        else:
            v = rng.choice(n_nodes, size=tail_deg, replace=False)
        pu += [u] * len(v)
        pv += list(v)
    pu, pv = np.array(pu), np.array(pv)
    if mirrors:                                    # list some pairs in both directions: folded entries carry second ids
        pick = rng.choice(pu.size, size=mirrors, replace=False)
        pu, pv = np.concatenate([pu, pv[pick]]), np.concatenate([pv, pu[pick]])
    keep = np.unique(np.stack([pu, pv], 1), axis=0, return_index=True)[1]      # no pair twice
    keep.sort()
    return torch.from_numpy(pu[keep]), torch.from_numpy(pv[keep])


LISTS = {
    "skewed": lambda: (*skewed_list(300, 40, 60, 3, 1), 300, 8, 37),
    "skewed, one slice": lambda: (*skewed_list(200, 21, 40, 2, 2), 200, 1, None),
    "mirrored": lambda: (*skewed_list(150, 30, 30, 2, 3, mirrors=400), 150, 4, 32),
    "fewer than 16 rows": lambda: (*skewed_list(64, 9, 20, 0, 4), 64, 2, 9),
}


def build(name, hub_rows="list"):
    pu, pv, n, slices, T = LISTS[name]()
    return PairList.build(pu, pv, n, n_slices=slices, hub_rows=T if hub_rows == "list" else hub_rows), pu, pv


def scored(pl):
    """(pair id, u, v) of everything the hub plan and its residual score, second ids included."""
    h = pl.hub
    live = h.step_q >= 0
    step, slot = torch.nonzero(live, as_tuple=True)
    item_of_step = torch.empty(h.n_steps, dtype=torch.long)
    shape_of_step = torch.empty(h.n_steps, dtype=torch.long)
    for it in range(h.n_items):
        a, b, c, e = h.item_step[it].tolist()
        item_of_step[a:e] = it
        shape_of_step[a:b], shape_of_step[b:c], shape_of_step[c:e] = 4, 2, 1
    nv = shape_of_step[step]
    vset = slot * nv // 4                                       # A: the slot, B: slot // 2, C: 0
    v = h.step_v[step, vset].long()
    u = h.block_row[h.item_block[item_of_step[step]].long() * HUB_W + h.step_u[step, slot].long()].long()
    ids, us, vs = [h.step_q[step, slot].long()], [u], [v]
    if h.step_q2 is not None:
        two = h.step_q2[step, slot] >= 0
        ids.append(h.step_q2[step, slot][two].long()); us.append(v[two]); vs.append(u[two])    # the mirror: endpoints swapped
    if h.rest is not None:
        r = h.rest
        row = torch.repeat_interleave(torch.arange(r.n_rows), (r.rowptr[1:] - r.rowptr[:-1]).long()) + r.row_offset
        ids.append(h.rest_pair.long()); us.append(row); vs.append(r.col.long())
        if h.rest_pair2 is not None:
            two = h.rest_pair2 >= 0
            ids.append(h.rest_pair2[two].long()); us.append(r.col.long()[two]); vs.append(row[two])
        # the residual plan's segments cover each of its entries once
        cover = torch.zeros(r.n_entries, dtype=torch.long)
        for s in torch.nonzero((r.seg_row >= 0) & (r.seg_end > r.seg_beg)).reshape(-1).tolist():
            cover[int(r.seg_beg[s]):int(r.seg_end[s])] += 1
            assert int(r.seg_row[s]) + r.row_offset == int(row[int(r.seg_beg[s])])
        assert bool((cover == 1).all())
    return torch.cat(ids), torch.cat(us), torch.cat(vs), shape_of_step, item_of_step


@pytest.mark.parametrize("name", list(LISTS))
def test_every_pair_once_on_its_endpoints(name):
    pl, pu, pv = build(name)
    assert pl.hub is not None and pl.hub.n_items > 0
    ids, us, vs, _, _ = scored(pl)
    assert ids.numel() == pu.numel()
    assert torch.equal(torch.sort(ids).values, torch.arange(pu.numel()))
    assert torch.equal(us, pu[ids]) and torch.equal(vs, pv[ids])
    assert pl.hub.n_entries + (pl.hub.rest.n_entries if pl.hub.rest is not None else 0) == (pl.fwd or pl.by_u).n_entries
    if name == "mirrored":
        assert pl.hub.step_q2 is not None and int((pl.hub.step_q2 >= 0).sum()) > 0


@pytest.mark.parametrize("name", list(LISTS))
def test_shapes_and_dead_slots(name):
    pl, _, _ = build(name)
    h = pl.hub
    live = h.step_q >= 0
    assert bool((h.step_u >= 0).all()) and bool((h.step_u < HUB_W).all())
    if h.step_q2 is not None:
        assert not bool(((h.step_q2 >= 0) & ~live).any())            # a second id only beside a first
    n_rows_in_block = (h.block_row.reshape(-1, HUB_W) >= 0).sum(1)
    assert bool((n_rows_in_block[:-1] == HUB_W).all()) and int(n_rows_in_block[-1]) == (h.n_rows - 1) % HUB_W + 1
    for it in range(h.n_items):
        a, b, c, e = h.item_step[it].tolist()
        assert a <= b <= c <= e and e > a
        blk = int(h.item_block[it])
        # a live slot names a row the block has
        assert bool((h.step_u[a:e][live[a:e]] < n_rows_in_block[blk]).all())
        # A: slot e on partner row e; the row is gathered exactly where the slot is live
        assert torch.equal(h.step_v[a:b] >= 0, live[a:b])
        # B: two slots per gathered row, both live or both dead; rows 2 and 3 unused
        assert torch.equal(live[b:c, 0], live[b:c, 1]) and torch.equal(live[b:c, 2], live[b:c, 3])
        assert torch.equal(h.step_v[b:c, 0] >= 0, live[b:c, 0]) and torch.equal(h.step_v[b:c, 1] >= 0, live[b:c, 2])
        assert bool((h.step_v[b:c, 2:] < 0).all())
        # C: one row, four live slots
        assert bool((h.step_v[c:e, 0] >= 0).all()) and bool((h.step_v[c:e, 1:] < 0).all()) and bool(live[c:e].all())
        # dead slots close a list, and never lead a step
        for lo, hi in ((a, b), (b, c), (c, e)):
            if hi > lo:
                assert bool(live[lo:hi - 1].all()) and bool(live[hi - 1, 0])
                n_live = int(live[hi - 1].sum())
                assert bool(live[hi - 1, :n_live].all())
    # items of a stream: slice by slice, largest first; streams partition the items
    s0 = h.slice_item0.tolist()
    assert s0[0] == 0 and s0[-1] == h.n_items and h.slice_max_item == max(y - x for x, y in zip(s0, s0[1:]))
    size = (h.item_step[:, 3] - h.item_step[:, 0]).tolist()
    for x in range(h.n_slices):
        key = [(int(h.item_slice[i]), -size[i]) for i in range(s0[x], s0[x + 1])]
        assert key == sorted(key) and all(k[0] % h.n_slices == x for k in key)
    # steps are stored item by item without gaps
    assert torch.equal(h.item_step[1:, 0], h.item_step[:-1, 3]) and int(h.item_step[-1, 3]) == h.n_steps


def test_partner_rows_packed_as_counted():
    """The steps gather what hub_block_counts says: c slots on a partner row = c // 4 C steps, a B half for a remainder of
    2 or 3, an A slot for 1 or 3 — and cutting long (block, slice) lists into work items does not change it."""
    pl, pu, pv = build("skewed")
    f = pl.fwd or pl.by_u
    row = torch.repeat_interleave(torch.arange(f.n_rows), (f.rowptr[1:] - f.rowptr[:-1]).long())
    entries, gathers = G.hub_block_counts(row, f.col.long(), pl.n_nodes)
    nb = pl.hub.n_blocks
    full = pl.hub.n_rows // HUB_W
    assert pl.hub.n_gathered >= int(gathers[:full].sum()) and pl.hub.n_gathered <= int(gathers[:nb].sum())
    old = G.HUB_ITEM_ROWS
    try:
        G.HUB_ITEM_ROWS = 8
        cut, _, _ = build("skewed")
    finally:
        G.HUB_ITEM_ROWS = old
    assert cut.hub.n_items > pl.hub.n_items and cut.hub.n_gathered == pl.hub.n_gathered
    ids, us, vs, _, _ = scored(cut)
    assert torch.equal(torch.sort(ids).values, torch.arange(pu.numel())) and torch.equal(us, pu[ids]) and torch.equal(vs, pv[ids])
    c = torch.tensor([1, 2, 3, 4, 5, 7, 16])
    assert G.hub_gathers(c).tolist() == [1, 1, 2, 1, 2, 3, 4]


@pytest.mark.parametrize("name", list(LISTS))
def test_same_plan_twice(name):
    a, _, _ = build(name)
    b, _, _ = build(name)
    for f in ("block_row", "slice_item0", "item_block", "item_slice", "item_step", "step_v", "step_u", "step_q", "step_q2"):
        x, y = getattr(a.hub, f), getattr(b.hub, f)
        assert (x is None and y is None) or torch.equal(x, y), f
    if a.hub.rest is not None:
        for f in ("col", "seg_row", "seg_beg", "seg_end", "slice_seg0"):
            assert torch.equal(getattr(a.hub.rest, f), getattr(b.hub.rest, f)), f
        assert torch.equal(a.hub.rest_pair, b.hub.rest_pair)


def test_no_hubs_no_plan():
    """A uniform sparse list has no block at the threshold: no hub plan, and the forward plan is what hub_rows=0 builds."""
    rng = np.random.default_rng(7)
    n = 4000
    pu = torch.from_numpy(np.repeat(np.arange(n), 6))
    pv = torch.from_numpy(rng.integers(0, n, size=pu.numel()))
    auto = PairList.build(pu, pv, n)
    off = PairList.build(pu, pv, n, hub_rows=0)
    assert auto.hub is None and off.hub is None
    assert torch.equal((auto.fwd or auto.by_u).seg_beg, (off.fwd or off.by_u).seg_beg)
    assert G.auto_hub_rows(pu, pv, n) == 0
    # a row shard never gets one, and asking for one there is an error
    assert PairList.build(pu[:600], pv[:600], n, by_u_range=(0, 100)).hub is None
    with pytest.raises(ValueError):
        PairList.build(pu[:600], pv[:600], n, by_u_range=(0, 100), hub_rows=16)


def test_auto_rule():
    """A first block at or above HUB_MIN_SHARE entries per gathered row pair puts every row with entries into the hub plan
    (no residual plan); a first block below it gives no plan."""
    pu, pv, n, slices, _ = LISTS["skewed"]()
    pl = PairList.build(pu, pv, n, n_slices=slices)
    f = pl.fwd or pl.by_u
    row = torch.repeat_interleave(torch.arange(f.n_rows), (f.rowptr[1:] - f.rowptr[:-1]).long())
    entries, gathers = G.hub_block_counts(row, f.col.long(), n)
    n_live = int((torch.bincount(row, minlength=n) > 0).sum())
    assert float(entries[0]) / float(gathers[0]) >= G.HUB_MIN_SHARE
    assert G.auto_hub_rows(row, f.col.long(), n) == n_live
    assert pl.hub is not None and pl.hub.n_rows == n_live and pl.hub.rest is None and pl.hub.n_entries == f.n_entries
    assert G.auto_hub_rows(row, f.col.long(), n, min_share=float(entries[0]) / float(gathers[0]) + 0.01) == 0
    ids, us, vs, _, _ = scored(pl)
    assert torch.equal(torch.sort(ids).values, torch.arange(pu.numel())) and torch.equal(us, pu[ids]) and torch.equal(vs, pv[ids])


def test_squirrel_counts():
    """The benchmark's pair list (squirrel_real, the split of bench.build_workload): 971,841 folded entries; blocks of 16
    over the 2,048 rows with the most entries gather 596,545 partner row pairs, residual entries included (0.614 of one
    per entry) with mirrored pairs folded into the row of the smaller endpoint, as the forward plan folds them
    (graph.mirror_partners); folding each into the orientation listed first would give 596,319.  The figure is recomputed here from the forward plan alone, by the rule and without the plan builder, and the steps the
    builder emits must gather exactly that."""
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.splits import make_link_split
    sg = synthetic_graph("squirrel_real", seed=0)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=0)
    pu = np.concatenate([split.pos_train.u, split.neg_train.u])
    pv = np.concatenate([split.pos_train.v, split.neg_train.v])
    order = np.lexsort((pv, pu))
    pl = PairList.build(torch.from_numpy(pu[order]), torch.from_numpy(pv[order]), sg.n_nodes, hub_rows=2048)
    assert pl.n_pairs == 1009603 and pl.fwd.n_entries == 971841
    h = pl.hub
    assert h.n_rows == 2048 and h.n_blocks == 128
    assert int((h.step_q >= 0).sum()) == h.n_entries and h.n_entries + h.rest.n_entries == 971841
    # the rule, in numpy, from the forward plan's rows and columns
    f, N = pl.fwd, sg.n_nodes
    fu = np.repeat(np.arange(f.n_rows), np.diff(f.rowptr.numpy()))
    fv = f.col.numpy().astype(np.int64)
    cnt = np.bincount(fu, minlength=N)
    rank = np.empty(N, np.int64)
    rank[np.argsort(-cnt, kind="stable")] = np.arange(N)
    m = rank[fu] < 2048
    _, c = np.unique((rank[fu[m]] // 16) * N + fv[m], return_counts=True)
    hub_gathers = int((c // 4).sum() + (c % 4 >= 2).sum() + (c % 2 == 1).sum())
    assert h.n_gathered == hub_gathers and h.rest.n_entries == int((~m).sum())
    total = hub_gathers + int((~m).sum())
    print(f"squirrel_real, T 2048, W 16: {total} gathered row pairs of {fu.size} entries = {total / fu.size:.3f}")
    assert total == 596545
    # and the top 1,024 rows hold about three quarters of the entries
    assert 0.73 < float((rank[fu] < 1024).mean()) < 0.75
