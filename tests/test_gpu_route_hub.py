"""Routing over a hub plan (Graph.route_hub; hub::route_seg_kernel) against the same call on the graph built from the same
edges with route_hub=False (route_seg_kernel over the mirrored routing plan): p equal, a and s equal as int32 views — the
same BITS, NaN included.  d = 64, K in {4, 8}, t in {1, 2}, fp32.

Graphs (all N <= 600).  The three small graphs of test_route_hub_plan_cpu.py, forced (route_hub=True), at the routing plan's
own item length and column slices, and in one slice with the items cut to 8 gathered rows (many short items; n17's second
block holds one row).  An item of 8
gathered rows has at most a dozen steps, so no wave of those plans has more than two: the waves of 15, 16, 17 and 33 steps (and 35, 36) —
a wave keeps the sums of two (K = 8) or four (K = 4) of its steps before it runs its tail, so what can go wrong depends on
the steps per wave — come from engineered graphs in one work item, the lists of test_gpu_score_hub_tail.py as graphs (16
hub rows that own every edge; nA partners on one hub, nB on two, nC on four): an item with only A steps, one with only C
steps, A lists that end on 1, 2 and 3 live rows, a B list that ends on one live half, a block of 3 rows.  The walk and the
batch counter are shared code (dl_hub.h), so the items also hold every length at which the closing flush changes: a multiple
of 8 waves x the batch (16 steps at K = 8, 32 at K = 4: 128 does for both), one less (127) and one more (129, an item with
all three lists), besides items of fewer than 8 steps (waves with none), without A, without B and of C steps only.  All of it is
asserted on CPU copies of the plans, so that a change of the plan builder fails here instead of silently covering less.

Tables: random; all zero (every quotient 1 / K: p is 0 everywhere); factor 1 an exact copy of factor 0 (the lower index
wins); one hub row scaled by 1e20 (inf / inf: NaN — why floats are compared as integers).

Also: the whole squirrel_real step at K = 8, t = 1 (all 342,129 entries, then H and the scorer's probabilities); a bf16
table and d = 32 on a graph that carries a plan (the old kernel runs); DL_ROUTE_HUB=0 in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import route_hub_graphs as rg
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 64
ENGINEERED = {"512/0/0": (512, 0, 0), "0/0/130": (0, 0, 130), "0/0/264": (0, 0, 264), "0/0/127": (0, 0, 127),
              "61/0/0": (61, 0, 0), "3/0/0": (3, 0, 0), "102/121/200": (102, 121, 200), "100/120/44": (100, 120, 44)}
WANT_PER_WAVE = {"512/0/0": {16}, "0/0/130": {16, 17}, "0/0/264": {33}, "0/0/127": {15, 16}, "61/0/0": {2}, "3/0/0": {0, 1},
                 "102/121/200": {35, 36}, "100/120/44": {16, 17}}
WANT_ITEM_STEP = {"512/0/0": [0, 128, 128, 128], "0/0/130": [0, 0, 0, 130], "61/0/0": [0, 16, 16, 16], "3/0/0": [0, 1, 1, 1],
                  "102/121/200": [0, 26, 87, 287], "100/120/44": [0, 25, 85, 129]}
_graphs = {}


def steps_per_wave(item_step):
    """The numbers of steps of the 8 waves of every item (wave w takes the steps a + w, a + w + 8, ... below e)."""
    return {len(range(a + w, e, 8)) for a, b, c, e in item_step for w in range(8)}


def _pair(src, dst, n, item_rows):
    """(graph with a forced hub plan, the same edges without one), on the GPU.  item_rows: None = the routing plan's own
    item length and slices, else that item length in ONE slice."""
    from disenlink_amd import graph
    old = graph.ROUTE_HUB_ITEM_ROWS, graph.ROUTE_HUB_SLICES
    ts, td = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)
    try:
        if item_rows is not None:
            graph.ROUTE_HUB_ITEM_ROWS, graph.ROUTE_HUB_SLICES = item_rows, 1
        hub = graph.Graph.from_edge_rows(ts, td, n, route_hub=True)
    finally:
        graph.ROUTE_HUB_ITEM_ROWS, graph.ROUTE_HUB_SLICES = old
    plain = graph.Graph.from_edge_rows(ts, td, n, route_hub=False)
    assert hub.route_hub is not None and plain.route_hub is None and n <= 600
    return hub, plain


def _all_graphs():
    """name -> (hub graph, plain graph); the plans hold what the docstring says."""
    if _graphs:
        return _graphs
    out, per_wave, a_tail, b_tail, lengths, lists = {}, set(), set(), set(), set(), set()
    for name, maker in rg.SMALL.items():
        out[name] = _pair(*maker(), None)
        out[name + ", items of 8"] = _pair(*maker(), 8)
        assert out[name][0].route_hub.n_slices > 1 and out[name + ", items of 8"][0].route_hub.n_slices == 1, name
        if name != "n17":
            assert out[name + ", items of 8"][0].route_hub.n_items > out[name][0].route_hub.n_items, name
    for name, (nA, nB, nC) in ENGINEERED.items():
        out[name] = _pair(*rg.engineered(nA, nB, nC), 4096)
        h = out[name][0].route_hub
        st = h.item_step.cpu().tolist()
        assert h.n_blocks == 1 and len(st) == 1 and h.n_entries == nA + 2 * nB + 4 * nC, name
        assert steps_per_wave(st) == WANT_PER_WAVE[name], (name, steps_per_wave(st))
        if name in WANT_ITEM_STEP:
            assert st == [WANT_ITEM_STEP[name]], (name, st)
    for name, (g, _) in out.items():
        h = g.route_hub
        st, v = h.item_step.cpu().tolist(), h.step_v.cpu().numpy()
        per_wave |= steps_per_wave(st)
        for a, b, c, e in st:
            lengths.add(e - a)
            lists.add((b > a, c > b, e > c))                         # which of the lists A, B, C the item has
            if b > a:
                a_tail.add(int((v[b - 1] >= 0).sum()))              # live rows of the A list's last step
            if c > b:
                b_tail.add(int((v[c - 1, :2] >= 0).sum()))          # live halves of the B list's last step
    assert {0, 1, 2, 15, 16, 17, 33} <= per_wave, per_wave
    assert {127, 128, 129} <= lengths and min(lengths) < 8, lengths  # 8 waves x 2 or 4 steps divides 128: nb == 0 at the closing flush
    assert {(True, True, True), (False, True, True), (True, False, True), (False, False, True), (True, False, False)} <= lists, lists
    assert {1, 2, 3, 4} <= a_tail and {1, 2} <= b_tail, (a_tail, b_tail)
    short = [int((g.route_hub.block_row[-16:] >= 0).sum()) for g, _ in out.values()]
    assert 1 in short and 3 in short, short                          # blocks with fewer than 16 rows
    assert any(g.route_hub.n_items >= 20 for g, _ in out.values())
    _graphs.update(out)
    return _graphs


def _tables(n, K, hub_row):
    gen = torch.Generator().manual_seed(1000 * K + n)
    Z = (torch.randn(n, K, D, generator=gen) * 0.35).contiguous()
    same = Z.clone()
    same[:, 1] = same[:, 0]
    big = Z.clone()
    big[hub_row] *= 1e20
    return {"random": Z.to(DEV), "zero": torch.zeros(n, K, D, device=DEV), "factor 1 == factor 0": same.to(DEV),
            "row * 1e20": big.to(DEV)}


def _route(g, Z, t):
    from disenlink_amd import ops
    p = torch.full((g.n_edges,), 255, dtype=torch.uint8, device=DEV)
    a = torch.full((g.n_edges,), -3.0, dtype=torch.float32, device=DEV)
    s = torch.zeros(Z.shape[0], Z.shape[1], dtype=torch.float32, device=DEV)
    ops.route_fwd(g, Z, t, s_out=s, p_out=p, a_out=a)
    torch.cuda.synchronize()
    return p, a, s


def _same(got, ref, what):
    for name, x, y in zip("pas", got, ref):
        if name == "p":
            assert torch.equal(x, y), f"{what}: p differs at {int((x != y).sum())} of {x.numel()} entries"
        else:
            xi, yi = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(xi, yi), f"{what}: {name} differs at {int((xi != yi).sum())} of {xi.numel()} values"


@pytest.mark.parametrize("t", [1.0, 2.0])
@pytest.mark.parametrize("K", [4, 8])
def test_hub_plan_gives_the_bits_of_the_routing_plan(K, t):
    for name, (hub, plain) in _all_graphs().items():
        owner = int(hub.route_hub.block_row[0])
        for tab, Z in _tables(hub.n_nodes, K, owner).items():
            ref = _route(plain, Z, t)
            assert int((ref[0] == 255).sum()) == 0, (name, tab)      # the reference wrote every entry
            if tab == "zero":
                assert int(ref[0].max()) == 0 and bool((ref[1] == 1.0 / K).all()), name
            if tab == "factor 1 == factor 0":
                assert int((ref[0] == 1).sum()) == 0, name
            if tab == "row * 1e20":
                assert bool(torch.isnan(ref[1]).any()), name
            _same(_route(hub, Z, t), ref, f"{name}, {tab}, K={K}, t={t}")


def test_whole_squirrel_step():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph
    K, t = 8, 1.0
    sg, split, g, pairs, model, x, Z = bench.build_workload("squirrel_real", DEV, K, D, 512)
    plain = Graph.from_edge_rows(torch.from_numpy(split.train_src).to(DEV), torch.from_numpy(split.train_dst).to(DEV),
                                 sg.n_nodes, row_bytes=K * D * 4, route_hub=False)
    h = g.route_hub
    assert h is not None and h.rest is None and g.n_edges == plain.n_edges == 342129 and h.n_entries == 171127
    assert h.n_gathered == 78062                                     # 0.456 gathered rows per entry
    ref, got = _route(plain, Z, t), _route(g, Z, t)
    _same(got, ref, "squirrel_real")
    H_ref, H_got = ops.aggregate_fwd(plain, Z, 0.5, *ref), ops.aggregate_fwd(g, Z, 0.5, *got)
    assert torch.equal(H_got, H_ref)
    prob = lambda H: ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs)
    assert torch.equal(prob(H_got), prob(H_ref))


@pytest.mark.parametrize("form", ["bf16", "d=32"])
def test_other_tables_run_the_routing_plan(form):
    hub, plain = _all_graphs()["power_law_300"]
    n = hub.n_nodes
    gen = torch.Generator().manual_seed(5)
    if form == "bf16":
        Z = (torch.randn(n, 8, D, generator=gen) * 0.35).to(DEV).to(torch.bfloat16).contiguous()
    else:
        Z = (torch.randn(n, 8, 32, generator=gen) * 0.35).to(DEV).contiguous()
    ref = _route(plain, Z, 1.0)
    assert int((ref[0] == 255).sum()) == 0 and len(set(ref[0].cpu().tolist())) > 1
    _same(_route(hub, Z, 1.0), ref, form)


_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import route_hub_graphs as rg
from disenlink_amd import ops
from disenlink_amd.graph import Graph
src, dst, n = rg.power_law_300()
g = Graph.from_edge_rows(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), n, route_hub=True)
assert g.route_hub is not None
Z = (torch.randn(n, 8, 64, generator=torch.Generator().manual_seed(77)) * 0.35).cuda().contiguous()
p, a, s = ops.route_fwd(g, Z, 1.0)
torch.cuda.synchronize()
np.savez({out!r}, p=p.cpu().numpy(), a=a.cpu().numpy().view(np.int32), s=s.cpu().numpy().view(np.int32))
"""


def test_switch_off_in_a_child_process(tmp_path):
    """DL_ROUTE_HUB=0: the library ignores the plan and walks the routing plan — the same arrays."""
    outs = []
    for value in ("0", "1"):
        out = str(tmp_path / f"route_{value}.npz")
        env = dict(os.environ, DL_ROUTE_HUB=value)
        code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(out))
    for k in ("p", "a", "s"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert len(set(outs[0]["p"].tolist())) > 1
