"""Forward scorer over a hub plan (graph.HubPlan; hub::score_fwd_wave_kernel + the residual plan) against the plan without hub
rows (PairList.build(hub_rows=0): the wave-per-entry kernel alone), the scorer called alone on the benchmark's inputs.
All forms interleaved in one process: 12 rounds, order reversed every other round, HIP events around 100 calls after 50
warm-up calls per form; median / min / max per form, torch.equal of all probabilities against hub_rows=0, and the
project's keep rule (worst of the form below the reference's best, gain above twice the reference's min-max spread).
usage: python tools/fwd_hub_ab.py [workload] [K] [d] [t] [--items [--auto] | --mixed]     (--items: sweep graph.HUB_ITEM_ROWS at
T = 2048 instead of T; with --auto at the automatic hub rows, the plan the benchmark runs.  --mixed: the mixed plan
(HubPlan.build_mixed) and each of its two parts alone against the three-list plan at the automatic hub rows)"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from disenlink_amd import graph, ops
from disenlink_amd.graph import PairList
args = [a for a in sys.argv[1:] if not a.startswith("--")]
dev = torch.device("cuda:0")
name = args[0] if len(args) > 0 else "squirrel_real"
K = int(args[1]) if len(args) > 1 else 8
d = int(args[2]) if len(args) > 2 else 64
t = float(args[3]) if len(args) > 3 else 1.0
sg, split, g, pairs, model, x, Z = bench.build_workload(name, dev, K, d, 512)
H = ops.aggregate_fwd(g, Z, 0.5, *ops.route_fwd(g, Z, t))
pu, pv, N = pairs.pu.long(), pairs.pv.long(), sg.n_nodes
f = pairs.fwd or pairs.by_u
row = torch.repeat_interleave(torch.arange(f.n_rows, device=dev), (f.rowptr[1:] - f.rowptr[:-1]).long())
entries, gathers = graph.hub_block_counts(row, f.col.long(), N)
share = (entries.double() / gathers.double()).cpu().numpy()
n_live = int((torch.bincount(row, minlength=N) > 0).sum())
auto = graph.auto_hub_rows(row, f.col.long(), N)
low = np.nonzero(share < graph.HUB_MIN_SHARE)[0]
at_thr = min(n_live, 16 * int(low[0] if low.size else share.size))
print(f"{name} K={K} d={d} t={t}: {f.n_entries} forward entries in {n_live} rows; automatic hub rows (first block at >= {graph.HUB_MIN_SHARE}): {auto}; every block at >= {graph.HUB_MIN_SHARE}: {at_thr}")
print("  entries per gathered row pair of block 0, 16, 32, ...: " + " ".join(f"{s:.2f}" for s in share[::16]))
build = lambda T, **kw: PairList.build(pu, pv, N, row_bytes=K * d * 4, hub_rows=T, hub_mixed=kw.pop("hub_mixed", False), **kw)
forms = {"hub_rows=0": build(0)}
REF = "hub_rows=0"                 # the form the keep rule measures against
if "--mixed" in sys.argv:
    # the mixed plan and its two parts, each alone, against the three-list plan the benchmark ran before it
    REF = "three lists (auto)"
    forms[REF] = build(None)
    if "--items" in sys.argv:                                   # ... or the mixed plan at several item lengths
        for cap in (192, 256, 320, 384, 448, 512):
            graph.HUB_MIXED_ITEM_ROWS = cap
            forms[f"mixed item<={cap}"] = build(None, hub_mixed=True)
    else:
        for label, owner, shapes in (("mixed shapes, listed orientation", False, True), ("owner, three-list shapes", True, False),
                                     ("mixed: owner + shapes", True, True)):
            graph.HUB_MIXED_OWNER, graph.HUB_MIXED_SHAPES_ON = owner, shapes
            forms[label] = build(None, hub_mixed=True)
        graph.HUB_MIXED_OWNER = graph.HUB_MIXED_SHAPES_ON = True
elif "--items" in sys.argv:
    T_items = auto if "--auto" in sys.argv else 2048
    for cap in (64, 128, 256, 384, 512, 768, 1024, 1 << 30):
        graph.HUB_ITEM_ROWS = cap
        forms[f"T={T_items} item<={cap}"] = build(T_items)
else:
    for T in sorted({512, 1024, 2048, at_thr, auto, n_live} - {0}):
        forms[f"T={T}" + (" (auto)" if T == auto else "") + (" (all rows)" if T == n_live else "")] = build(T)
for k, pl in forms.items():
    if pl.hub is not None:
        h = pl.hub_mixed or pl.hub                              # the plan the scorer walks
        size = (h.item_step[:, -1] - h.item_step[:, 0]).cpu()
        rest = h.rest.n_entries if h.rest is not None else 0
        print(f"  {k}: {h.n_blocks} blocks, {h.n_items} items (steps max {int(size.max())} median {int(size.median())}), {h.n_steps} steps, "
              f"{h.n_entries} hub entries on {h.n_gathered} gathered row pairs + {rest} residual = {h.n_gathered + rest} "
              f"({(h.n_gathered + rest) / f.n_entries:.3f} of one per entry)")
fwd = lambda pl: ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pl)
ref = fwd(forms["hub_rows=0"]).clone()
same = {k: torch.equal(fwd(pl), ref) for k, pl in forms.items()}
times = {k: [] for k in forms}
for k, pl in forms.items():
    for _ in range(50): fwd(pl)
torch.cuda.synchronize()
order = list(forms)
for r in range(12):
    for k in (order if r % 2 == 0 else order[::-1]):
        pl = forms[k]
        fwd(pl)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100): fwd(pl)
        e1.record(); e1.synchronize()
        times[k].append(e0.elapsed_time(e1) / 100 * 1e3)
p = times[REF]
print(f"us per call (keep rule against: {REF})   median      min      max   bits == hub_rows=0")
for k in forms:
    v = times[k]
    keep = "" if k in ("hub_rows=0", REF) else ("   keep" if max(v) < min(p) and np.median(p) - np.median(v) > 2 * (max(p) - min(p)) else "   NOT kept")
    print(f"  {k:32s} {np.median(v):8.2f} {min(v):8.2f} {max(v):8.2f}   {same[k]}{keep}")
print("raw (us per call, round by round):")
for k in forms:
    print(f"  {k:32s} " + " ".join(f"{v:.2f}" for v in times[k]))
