"""Routing over a hub plan (graph.route_hub_plan; hub::route_seg_kernel) against the graph built from the same edges with
route_hub=False (route_seg_kernel over the mirrored routing plan), route_fwd called alone on the benchmark's inputs.
All forms interleaved in one process: 12 rounds, order reversed every other round, HIP events around 100 calls after 50
warm-up calls per form; median / min / max per form, torch.equal of p / a / s (floats as int32) against route_hub=False,
and the project's keep rule (worst of the form below the reference's best, gain above twice the reference's min-max spread).
The times are those of the whole call: the routing launch and the row-sum launch behind it.
usage: python tools/route_hub_ab.py [workload] [K] [d] [t]      (the forms: the sweep of graph.ROUTE_HUB_ITEM_ROWS at the default
graph.ROUTE_HUB_SLICES, and the slices at the default item length)"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from disenlink_amd import graph, ops
from disenlink_amd.graph import Graph
args = [a for a in sys.argv[1:] if not a.startswith("--")]
dev = torch.device("cuda:0")
name = args[0] if len(args) > 0 else "squirrel_real"
K = int(args[1]) if len(args) > 1 else 8
d = int(args[2]) if len(args) > 2 else 64
t = float(args[3]) if len(args) > 3 else 1.0
sg, split, g, pairs, model, x, Z = bench.build_workload(name, dev, K, d, 512)
src, dst = torch.from_numpy(split.train_src).to(dev), torch.from_numpy(split.train_dst).to(dev)
build = lambda hub: Graph.from_edge_rows(src, dst, sg.n_nodes, row_bytes=K * d * 4, route_hub=hub)
REF = "route_hub=False"
forms = {REF: build(False)}
default = graph.ROUTE_HUB_ITEM_ROWS
auto = g.route_hub is not None
slices = graph.ROUTE_HUB_SLICES
for cap in (32, 64, 96, 128, 160, 256):                     # the item-length sweep at the default slices
    graph.ROUTE_HUB_ITEM_ROWS = cap
    forms[f"item<={cap}, {slices} slices" + (" (default)" if cap == default else "")] = build(True)
graph.ROUTE_HUB_ITEM_ROWS = default
for n in (1, 2, 4, 8):                                      # the slices at the default item length
    if n != slices:
        graph.ROUTE_HUB_SLICES = n
        forms[f"item<={default}, {n} slice" + ("s" if n > 1 else "")] = build(True)
graph.ROUTE_HUB_SLICES = slices
walked = int((forms[REF].route.seg_end - forms[REF].route.seg_beg).sum())
print(f"{name} K={K} d={d} t={t}: {g.n_edges} entries, {walked} walked by the routing plan (col >= row) in "
      f"{int((forms[REF].route.seg_row >= 0).sum())} segments; automatic rule: {'a hub plan' if auto else 'no hub plan'}")
for k, f in forms.items():
    h = f.route_hub
    if h is not None:
        st = h.item_step.long()
        size = (st[:, 3] - st[:, 0]).cpu()
        print(f"  {k}: {h.n_blocks} blocks, {h.n_slices} streams, {h.n_items} items (steps max {int(size.max())} median {int(size.median())}), {h.n_steps} steps "
              f"(A / B / C {int((st[:, 1] - st[:, 0]).sum())} / {int((st[:, 2] - st[:, 1]).sum())} / {int((st[:, 3] - st[:, 2]).sum())}), "
              f"{h.n_entries} entries on {h.n_gathered} gathered rows ({h.n_gathered / h.n_entries:.3f} per entry)")
run = lambda f: ops.route_fwd(f, Z, t)
bits = lambda out: (out[0].clone(), out[1].view(torch.int32).clone(), out[2].view(torch.int32).clone())
ref = bits(run(forms[REF]))
same = {k: all(torch.equal(x, y) for x, y in zip(bits(run(f)), ref)) for k, f in forms.items()}
times = {k: [] for k in forms}
for k, f in forms.items():
    for _ in range(50): run(f)
torch.cuda.synchronize()
order = list(forms)
for r in range(12):
    for k in (order if r % 2 == 0 else order[::-1]):
        f = forms[k]
        run(f)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100): run(f)
        e1.record(); e1.synchronize()
        times[k].append(e0.elapsed_time(e1) / 100 * 1e3)
p = times[REF]
print(f"us per call (route + row sums)      median      min      max   bits == {REF}")
for k in forms:
    v = times[k]
    keep = "" if k == REF else ("   keep" if max(v) < min(p) and np.median(p) - np.median(v) > 2 * (max(p) - min(p)) else "   NOT kept")
    print(f"  {k:32s} {np.median(v):8.2f} {min(v):8.2f} {max(v):8.2f}   {same[k]}{keep}")
print("raw (us per call, round by round):")
for k in forms:
    print(f"  {k:32s} " + " ".join(f"{v:.2f}" for v in times[k]))
