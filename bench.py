#!/usr/bin/env python3
"""edges/sec (aggregate+score) at K=8, d=64 — the metric of BASELINE.json — on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
                    [--workload squirrel|chameleon|penn94|snap_patents|...] [--dtype f32|bf16] [--scaling weak|strong]
                    [--sections all|headline,hbm_bound,...]

One "step" = one forward pass of the hot path over the whole training graph with inputs
resident in HBM: route (model.py:56-72) + aggregate (model.py:73-75) over the E_sym directed
non-zeros of the training adjacency, + the pair scorer (model.py:109-113) over the P scored
training pairs.  value = (E_sym + P) / step time  (SURVEY.md §8d headline rate).  The
projection GEMM and the one-time CSR construction are outside the timed region, as §8d says.

Timing: W warm-up steps, then warm-up BY TIME (blocks of min(K, 50) steps until at least 0.3 s have passed and three
consecutive blocks agree within 2 % — a fresh GPU ramps its clocks for tens of milliseconds, far longer than any
sensible W at 0.2 ms per step), then exactly K timed steps between two device synchronisations; ms_per_step is their
time / K.  --dump-outputs DIR writes what the last timed step computed (DIR/<name>.npy, float32).  A plain run stops
there and prints the line.

--full adds everything else: the per-kernel roofline table (a second pass of R blocks of K steps, R >= --repeats and
>= 1 s in total, with HIP events on the phases; min / median / max of those blocks are in the line), the extra
sections (--sections), the CPU baselines and `parity`: the timed GPU outputs against the CPU oracle's dense pass on
the same Z (max |dprob| over the scored pairs, AUC on both sides; exit 4 when they do not match).

Roofline accounting.  Two byte counts per kernel phase:
  * algorithmic_bytes — SURVEY.md §8(d)'s per-unit figures (no cache credit, every directed edge, the u rows of the
    scorer counted per pair): the nominal size of the problem;
  * moved_bytes — what the kernels actually request from the memory system per launch: rows gathered (routing walks
    each undirected edge once; the scorer stages the u rows once per segment in LDS and gathers only v rows), per-entry
    scalars, per-segment descriptors, outputs and the partial-slot round trips.
`roofline.achieved` = moved_bytes / kernel time.  On the default workload (squirrel: Z+H = 21 MB) those bytes come out
of the XCD L2s / the Infinity Cache, not HBM, so the bound that applies is the L2 bandwidth (MI355X_MICROARCH.md §L2:
34.5 TB/s) and `roofline.bound` says "l2"; the HBM-side traffic measured by rocprofv3 PMC passes rides along as
`traffic`.  The `hbm_bound` block repeats the measurement IN THE SAME RUN on a workload whose tables (>= 1 GiB) cannot
sit in any cache, where the 8 TB/s HBM roofline is the bound: that is the number the north star's "fraction of the HBM
roofline on the K-factor edge-scatter" refers to.

N > 1: one rank per GPU over RCCL (disenlink_amd/dist.py, dist_bench.py).  Started under torch.distributed.run the
process is a rank; started plainly (`python bench.py --gpus N`) it LAUNCHES its N ranks itself as child processes —
before it has made any GPU call, relaying rank 0's JSON line and the children's exit code.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
L2_PEAK_GBS = 34500.0      # MI355X_MICROARCH.md §L2 (per XCD): ~34.5 TB/s aggregate over the 8 XCDs
L2_GATHER_REF_GBS = (16800.0, 18800.0)   # ibid. §Indexed rows: L2-resident row gather into LDS, measured lower bounds
FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 = 256 FLOP/clk/CU x 256 CUs x 2.4 GHz
BF16_MFMA_PEAK_TFLOPS = 2500.0  # ibid.: dense bf16 MFMA
# kernels launched by each phase of the step (names as rocprofv3 reports them, template arguments stripped)
PHASE_KERNELS = {"route": ("route_seg_kernel", "s_rowsum_thread_kernel"),
                 "aggregate": ("aggregate_cls_kernel", "row_combine_kernel"),
                 "score": ("score_fwd_seg_kernel", "score_fwd_wave_kernel")}
PMC_SUMMARY = os.path.join(ROOT, "profiles", "pmc_traffic_latest.json")
NAMES = ("route", "aggregate", "score")


def kernel_source_hash() -> str:
    """sha256 over the HIP sources: a PMC summary collected for other kernels is not this build's traffic."""
    h = hashlib.sha256()
    src = os.path.join(ROOT, "disenlink_amd", "csrc")
    for name in sorted(os.listdir(src)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            h.update(open(os.path.join(src, name), "rb").read())
    return h.hexdigest()[:16]


TRAIN_PHASE_KERNELS = {"scorer": ("score_train_wave_kernel", "score_train_wide_kernel", "score_bwd_seg_kernel", "score_bwd_coef_seg_kernel"),
                       "bwd_phase1": ("bwd_phase1_seg_kernel",), "bwd_phase2": ("bwd_phase2_seg_kernel",),
                       "route": ("route_seg_kernel", "s_rowsum_thread_kernel"), "aggregate": ("aggregate_cls_kernel",)}


def pmc_traffic(workload_key: str, phases=None):
    """HBM-side bytes per launch and phase from the committed rocprofv3 PMC passes (tools/pmc_traffic.py: FETCH_SIZE x2
    gfx950 correction + WRITE_SIZE, separate passes of `bench.py --sections <...>`), or None when no summary exists for
    this workload or it was collected for different kernel sources."""
    try:
        table = json.load(open(PMC_SUMMARY))
    except (OSError, ValueError):
        return None, "no PMC summary committed"
    entry = table.get(workload_key)
    if not entry:
        return None, f"no PMC passes committed for {workload_key}"
    if entry.get("kernel_source_hash") != kernel_source_hash():
        return None, (f"PMC passes in profiles/ were collected for kernel sources {entry.get('kernel_source_hash')}, "
                      f"this build is {kernel_source_hash()}: not reported")
    out = {}
    for phase, kernels in (phases or PHASE_KERNELS).items():
        tot = 0.0
        for kname, v in entry["kernels"].items():
            base = kname.split("<")[0].split("::")[-1]
            if base in kernels and v.get("phase", phase) == phase:
                tot += v["traffic_bytes"] * v.get("launches_per_step", 1.0)
        out[phase] = tot
    return out, entry.get("source", "profiles/pmc_traffic_latest.json")


PMC_L2_SUMMARY = os.path.join(ROOT, "profiles", "pmc_l2_latest.json")


def pmc_l2(workload_key: str, phases=None):
    """Bytes the compute units REQUESTED from the XCD L2s per launch and phase (rocprofv3 TCC_READ / TCC_WRITE passes,
    tools/pmc_l2_run.sh: reads x 128 B + writes x 64 B) — the counter behind `moved_bytes` — with the L2 hit rate, or None
    when no pass exists for this workload or it belongs to other kernel sources."""
    try:
        entry = json.load(open(PMC_L2_SUMMARY)).get(workload_key)
    except (OSError, ValueError):
        return None
    if not entry or entry.get("kernel_source_hash") != kernel_source_hash():
        return None
    out = {}
    for phase, kernels in (phases or PHASE_KERNELS).items():
        tot, hit, miss = 0.0, 0.0, 0.0
        for kname, v in entry["kernels"].items():
            if kname.split("<")[0].split("::")[-1] in kernels:
                tot += v["l2_bytes"]
                hit += v["hit"]
                miss += v["miss"]
        out[phase] = dict(l2_bytes=tot, hit_rate=hit / (hit + miss) if hit + miss > 0 else None)
    return out


HBM_ACHIEVABLE_FRAC = 6.3 / 8.0     # MI355X_MICROARCH.md §HBM: ~6.3 of the 8 TB/s are achievable


def memory_bound(table_bytes, mbytes, traffic):
    """Which roof prices the gather kernels of this workload -> (bound, peak GB/s, how it was decided).
    MEASURED where rocprofv3 PMC passes exist for this build and workload: if the bytes that left the XCD L2s
    (FETCH_SIZE x2 + WRITE_SIZE, Infinity-Cache hits included) are less than half of what the kernels request, the
    requests are served by the caches and the L2 bandwidth is the roof; otherwise HBM is.  Without counters the table
    size decides (Z+H within 128 MiB: cache) and the line says so; an HBM fraction above what HBM can deliver is then
    flagged, never presented as a measurement."""
    if traffic is not None and sum(mbytes.values()) > 0:
        ratio = sum(traffic.values()) / sum(mbytes.values())
        bound = "l2" if ratio < 0.5 else "hbm"
        how = f"measured: PMC traffic / moved bytes = {ratio:.2f} ({'< 0.5: cache-served' if ratio < 0.5 else '>= 0.5: HBM-served'})"
    else:
        bound = "l2" if table_bytes <= 128 << 20 else "hbm"
        how = "table size (no PMC passes for this build and workload: Z+H %s 128 MiB)" % ("<=" if bound == "l2" else ">")
    return bound, (L2_PEAK_GBS if bound == "l2" else HBM_PEAK_GBS), how


def algorithmic_bytes(K, d, n_nodes, n_edges, n_pairs, w=4):
    """SURVEY.md §8(d), no cache credit: per edge route K*d*w+4+1+4, aggregate d*w+4+1+4+4;
    per node 2*K*d*w (z_i in both passes) + K*d*w (h_i) + 2*K*4 (s) + 8 (rowptr); per pair 4*K*d*w+8+4."""
    route = n_edges * (K * d * w + 9) + n_nodes * (K * d * w + K * 4 + 4)
    aggregate = n_edges * (d * w + 13) + n_nodes * (2 * K * d * w + K * 4 + 4)
    score = n_pairs * (4 * K * d * w + 12)
    return dict(route=route, aggregate=aggregate, score=score)


def moved_bytes(graph, pairs, K, d, w=4):
    """Bytes the kernels request per launch: gathered rows count every time they are gathered, rows staged
    in LDS or held in registers count once per segment, partial slots count their write and their read-back."""
    row = K * d * w
    plan, rp, pu = graph.plan, graph.route, pairs.by_u
    E, N = plan.n_entries, plan.n_rows
    walked = int((rp.seg_end.long() - rp.seg_beg.long()).sum()) if rp is not None else E
    n_rseg = rp.n_seg if rp is not None else plan.n_seg
    mirror = 2 if graph.route_mirror else 1
    route = (walked * (row + 4 + (4 if graph.route_mirror else 0)) + mirror * walked * 5      # gathers, col, rev; p, a out
             + n_rseg * (row + 16)                                                              # z_i + descriptor
             + E * 5 + plan.n_seg * 16 + N * K * 4)                                             # row sums of (p, a) -> s
    aggregate = (E * (d * w + 4 + 1 + 4 + 4) + plan.n_seg * 16                                  # slice gather, col, p, a, s[col]
                 + N * 2 * row                                                                  # z_i in, h_i out
                 + plan.n_slots * K * d * 4 * 2)                                                # partial rows: written, read back
    P = pairs.n_pairs
    score = P * (2 * row + 4 + 4 + 4) + pu.n_seg * (2 * row + 16)                               # v rows; u rows once per segment
    return dict(route=route, aggregate=aggregate, score=score)


def build_workload(name, device, K, d, nhid, seed=0, m=5, scale=1.0, elem_bytes=4):
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.graph import Graph, PairList
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    sg = synthetic_graph(name, seed=seed, scale=scale)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=m, seed=seed)
    graph = Graph.from_edge_rows(torch.from_numpy(split.train_src).to(device),
                                 torch.from_numpy(split.train_dst).to(device), sg.n_nodes, row_bytes=K * d * elem_bytes)
    pu = np.concatenate([split.pos_train.u, split.neg_train.u])
    pv = np.concatenate([split.pos_train.v, split.neg_train.v])
    order = np.lexsort((pv, pu))                      # pair list laid out by u: long runs share the u rows
    pu, pv = pu[order], pv[order]
    pairs = PairList.build(torch.from_numpy(pu).to(device), torch.from_numpy(pv).to(device), sg.n_nodes,
                           row_bytes=K * d * elem_bytes)
    pairs.bench_label = np.concatenate([split.pos_train.label, split.neg_train.label])[order].astype(np.float32)
    torch.manual_seed(seed)
    model = Disentangle(sg.n_feat, nhid, d, nfactor=K, beta=0.5, t=1).to(device)
    x = torch.from_numpy(sg.features()).to(device)
    with torch.no_grad():
        Z = model.project(x).contiguous()
    return sg, split, graph, pairs, model, x, Z


def cpu_baseline(Z_cpu, graph_cpu, n_units, beta, t, budget_s=45.0, parity=None, fwd_bwd_budget_s=30.0):
    """The oracle's dense restatement (same op sequence as model.py:56-76,109-113) timed on the host
    cores: one warm-up, then THREE timed passes (their median is the value) unless the budget runs out first — the
    sample text then says how many passes were timed and claims no median.  `parity` = (pu, pv, label, prob_gpu) of
    the timed GPU step: the warm-up pass's probabilities at those pairs become the line's parity block."""
    from oracle import dense_ref
    N = Z_cpu.shape[0]
    adj = torch.zeros(N, N)
    src = torch.repeat_interleave(torch.arange(N), (graph_cpu.rowptr[1:] - graph_cpu.rowptr[:-1]).long())
    adj[src, graph_cpu.col.long()] = 1
    Zk = Z_cpu.permute(1, 0, 2).contiguous()
    times = []
    t_all = time.perf_counter()
    with torch.no_grad():
        for it in range(4):
            t0 = time.perf_counter()
            H, e, _att, _p, _s = dense_ref.route_aggregate(Zk, adj, beta, t)
            P = dense_ref.score_allpairs(H, e)
            dt = time.perf_counter() - t0
            if it == 0 and parity is not None:
                par = parity_block(P[parity[0].long(), parity[1].long()].numpy(), *parity[2:])
            del H, e, _att, P
            if it > 0:
                times.append(dt)
            if len(times) >= 3 or (time.perf_counter() - t_all > budget_s and times):
                break
    med = float(np.median(times))
    how = f"median of {len(times)} timed passes" if len(times) >= 3 else \
        f"{len(times)} timed pass{'es' if len(times) > 1 else ''} (the {budget_s:.0f} s budget ran out: no median claimed)"
    out = dict(value=n_units / med, unit="edges/s", cores=torch.get_num_threads(), kind="port",
               sample=f"whole workload, dense [K,N,N] forward (route+aggregate+all-pairs score) of oracle/dense_ref.py, "
                      f"{how} after 1 warm-up, {med:.2f} s per pass",
               seconds_per_pass=med, timed_passes=len(times), seconds_per_pass_all=[round(v, 3) for v in times])
    # forward + backward ("forward and forward+backward reported separately"): one pass of the same
    # dense op sequence under autograd with the weighted BCE of main_disentangled.py:195 on the scored pairs — what the
    # reference's loss.backward() does to the path (the projection excluded on both sides), timed once (it holds ~10
    # [K,N,N] tensors; a second pass would double the bench's CPU time)
    if parity is not None and fwd_bwd_budget_s > 0:
        try:
            from disenlink_amd.metrics import pair_bce_weights
            pu, pv, label = parity[0].long(), parity[1].long(), torch.from_numpy(parity[2])
            n_pos = int(label.sum())
            w = torch.where(label > 0, torch.tensor(1.0 / max(n_pos, 1)), torch.tensor(1.0 / (5 * max(label.numel() - n_pos, 1))))
            Zg = Zk.clone().requires_grad_(True)
            t0 = time.perf_counter()
            H, e, _att, _p, _s = dense_ref.route_aggregate(Zg, adj, beta, t)
            P = dense_ref.score_allpairs(H, e)
            loss = torch.nn.functional.binary_cross_entropy(P[pu, pv], label, weight=w, reduction="sum")
            loss.backward()
            dt = time.perf_counter() - t0
            del H, e, _att, P, loss
            out["fwd_bwd"] = dict(value=n_units / dt, unit="edges/s", seconds_per_pass=dt,
                                  sample="one pass of the same dense forward under autograd + weighted BCE on the scored pairs + "
                                         "backward to Z (no warm-up of its own)")
        except MemoryError as ex:                                   # the host cannot hold the autograd tape
            out["fwd_bwd"] = {"value": None, "error": f"{type(ex).__name__}: {ex}"}
    return (out, par) if parity is not None else out


def parity_block(prob_cpu, label, prob_gpu, tol_prob=1e-5, what=None, routing=None):
    """The metric's "link-pred AUC parity vs CPU ref" for the outputs of the TIMED GPU step: max |dprob| over the scored
    pairs against the oracle's dense pass on the same Z, and the tie-averaged AUC of either side (the oracle's numpy AUC
    for the CPU probabilities, the library's device AUC — dl_auc_pair_counts — for the GPU's)."""
    from disenlink_amd.metrics import AucPlan
    from oracle import metrics_ref
    pg = prob_gpu.detach().float()
    if label is None:                                               # no labels at hand (sharded blocks): the probabilities alone
        dmax = float(np.max(np.abs(pg.cpu().numpy().astype(np.float64) - prob_cpu.astype(np.float64))))
        return {"max_abs_dprob": dmax, "pairs": int(prob_cpu.size), "tolerance": {"max_abs_dprob": tol_prob},
                "ok": bool(dmax <= tol_prob), "what": what}
    lab = torch.from_numpy(label).to(pg.device)
    auc_gpu = float(AucPlan(lab).auc(pg))
    auc_cpu = float(metrics_ref.auc_tie_avg(label, prob_cpu))
    pgh = pg.cpu().numpy()
    diff = np.abs(pgh.astype(np.float64) - prob_cpu.astype(np.float64))
    dmax = float(np.max(diff))
    beyond = int((diff > tol_prob).sum())
    out = {"max_abs_dprob": dmax, "auc_gpu": auc_gpu, "auc_cpu": auc_cpu, "abs_dauc": abs(auc_gpu - auc_cpu),
           "pairs": int(label.size), "pairs_beyond_tolerance": beyond,
           "saturated_frac": float(((pgh == 0.0) | (pgh == 1.0)).mean()),      # a check on all-saturated scores says little: see parity_unsaturated
           "tolerance": {"max_abs_dprob": tol_prob, "abs_dauc": 1e-4},
           "what": what or "timed GPU step (route+aggregate+score on the scored train pairs) vs oracle/dense_ref.py on the same Z"}
    # Routing is an arg-max over K softmax weights (model.py:61): where two weights tie to the last bits, the GPU's and the
    # CPU's summation orders may pick different factors for that edge — the reference against itself on another BLAS does
    # the same.  `routing` = (edges routed differently, largest |a_gpu - a_cpu| among them): with flips present, isolated
    # pairs beyond the tolerance are theirs; the metric's criterion (AUC within 1e-4) and a bound on their number stay.
    flips, flip_gap = routing[:2] if routing is not None else (0, 0.0)
    near_tie = False
    if routing is not None:
        out["routing_flips"] = {"edges": int(flips), "max_abs_da_at_flips": float(flip_gap)}
        if flips > 0 and len(routing) > 3 and beyond > 0:
            # a flipped edge (r, c) changes the normalisers s[r], s[c] (model.py:69-72), hence the aggregation weights of every
            # edge pointing at r or c (model.py:73: att[i, j] = alpha1[i, j] / s[j]), hence H of r, c and all their neighbours
            # (routing[2]: that node set) — and every scored pair touching one of those nodes.  Nothing else may differ.
            touched, (pu, pv) = routing[2], routing[3]
            far = diff > tol_prob
            explained = touched[pu[far]] | touched[pv[far]]
            out["routing_flips"].update(nodes_whose_H_changes=int(touched.sum()), pairs_beyond_tolerance_touching_them=int(explained.sum()))
            near_tie = bool(flip_gap <= 1e-5 and explained.all())
    out["ok"] = bool(abs(auc_gpu - auc_cpu) <= 1e-4 and (dmax <= tol_prob or near_tie))
    return out


def routing_flips(p_gpu, a_gpu, p_cpu, a_cpu, rowptr, col, pairs_uv):
    """-> (edges the GPU and the oracle routed to different factors, largest |a_gpu - a_cpu| among them, bool[N] of the nodes
    whose H such a flip changes: its endpoints and their neighbours, (pu, pv))."""
    pg, ag = p_gpu.cpu().numpy(), a_gpu.float().cpu().numpy()
    fl = np.flatnonzero(pg != p_cpu)
    n = rowptr.size - 1
    touched = np.zeros(n, dtype=bool)
    if fl.size:
        rows = np.searchsorted(rowptr, fl, side="right") - 1
        ends = np.unique(np.concatenate([rows, col[fl]]))
        touched[ends] = True
        for u in ends:
            touched[col[rowptr[u]:rowptr[u + 1]]] = True
    gap = float(np.abs(ag[fl] - a_cpu[fl]).max()) if fl.size else 0.0
    return (int(fl.size), gap, touched, pairs_uv)


def cpu_baseline_sparse(Z_cpu, graph_cpu, pairs_cpu, n_units, beta, t, budget_s=30.0, label=None, parity=None, bf16=False):
    """Baseline B: the multi-threaded C restatement of the edge-list form, for graphs whose
    dense [K,N,N] form cannot exist.  Whole workload, three timed passes after one warm-up (fewer if the budget runs out:
    the sample text says so).  `parity` = (label, prob_gpu) of the timed GPU step: the warm-up pass's probabilities become
    the line's parity block (returned second).  bf16: Z_cpu holds the bf16-rounded table and the oracle's H is rounded to
    bf16 before scoring, as the GPU stores it — what is left is fp32 summation order and bf16 rounding flips of H."""
    from oracle import c_ref
    Zh = Z_cpu.numpy()
    par = None
    rnd = (lambda a: torch.from_numpy(a).to(torch.bfloat16).float().numpy()) if bf16 else (lambda a: a)
    rowptr, col = graph_cpu.rowptr.numpy(), graph_cpu.col.numpy()
    pu, pv = pairs_cpu[0].numpy(), pairs_cpu[1].numpy()
    times = []
    t_all = time.perf_counter()
    for it in range(4):
        t0 = time.perf_counter()
        p, a, s = c_ref.route(Zh, rowptr, col, t)
        H = c_ref.aggregate(Zh, rowptr, col, p, a, s, beta)
        prob_c = c_ref.score_pairs(Zh, rnd(H) if (bf16 and it == 0 and parity is not None) else H, pu, pv, t)
        dt = time.perf_counter() - t0
        if it == 0 and parity is not None:
            routing = None
            if len(parity) > 3 and parity[2] is not None:           # the GPU's routing of the same step: near-tie flips and what they touch
                routing = routing_flips(parity[2], parity[3], p, a, rowptr, col, (pu, pv))
            par = parity_block(prob_c, parity[0], parity[1], tol_prob=2e-2 if bf16 else 1e-5, routing=routing,
                               what="timed GPU step (route+aggregate+score on the scored train pairs) vs oracle/c/sparse_ref.c "
                                    "(edge-list form, OpenMP) on the same Z" + (" — bf16-rounded tables on both sides, the oracle's H "
                                                                               "rounded to bf16 before scoring" if bf16 else ""))
        del prob_c
        if it > 0:
            times.append(dt)
        if len(times) >= 3 or (time.perf_counter() - t_all > budget_s and times):
            break
    med = float(np.median(times))
    how = f"median of {len(times)} timed passes" if len(times) >= 3 else \
        f"{len(times)} timed pass{'es' if len(times) > 1 else ''} (the {budget_s:.0f} s budget ran out: no median claimed)"
    out = dict(value=n_units / med, unit="edges/s", cores=os.cpu_count(), kind="port",
               sample=f"whole workload, edge-list forward (route+aggregate+score_pairs) of oracle/c/sparse_ref.c with "
                      f"OpenMP on all host cores (Baseline B of BASELINE.md: the form that also runs where the reference's "
                      f"dense [K,N,N] cannot exist), {how} after 1 warm-up, {med:.2f} s per pass",
               seconds_per_pass=med, timed_passes=len(times), seconds_per_pass_all=[round(v, 3) for v in times])
    if label is not None:                                           # forward + backward of the same path, edge-list form
        n_pos = int(label.sum())
        w = np.where(label > 0, 1.0 / max(n_pos, 1), 1.0 / (5 * max(label.size - n_pos, 1))).astype(np.float32)
        tb = []
        for it in range(2):
            t0 = time.perf_counter()
            p, a, s = c_ref.route(Zh, rowptr, col, t)
            H = c_ref.aggregate(Zh, rowptr, col, p, a, s, beta)
            prob = c_ref.score_pairs(Zh, H, pu, pv, t)
            g = (w * (prob - label) / np.maximum(prob * (1 - prob), np.float32(1e-12))).astype(np.float32)
            _dZs, dH = c_ref.score_pairs_bwd(Zh, H, pu, pv, t, prob, g)
            c_ref.route_aggregate_bwd(Zh, rowptr, col, p, a, s, beta, t, dH)
            tb.append(time.perf_counter() - t0)
            if time.perf_counter() - t_all > 2 * budget_s:
                break
        out["fwd_bwd"] = dict(value=n_units / tb[-1], unit="edges/s", seconds_per_pass=tb[-1],
                              sample="edge-list forward + weighted BCE gradient + scorer / routing / aggregation backward of "
                                     f"oracle/c/sparse_ref.c, pass {len(tb)} of {len(tb)}")
    return (out, par) if parity is not None else out


EVENT_OVERHEAD_US = [0.0]     # the empty event-to-event interval of the last time_forward (reported, not subtracted)
WARM_S = [0.3]          # --warm-s / --min-region-s (profiler passes set both to 0: a PMC pass serialises every launch)
REGION_S = [1.0]


def steady_warmup(run_block, min_s=None, tol=0.02, max_s=4.0):
    """Blocks of the step (run_block() -> seconds for one block, synchronised) until >= min_s have elapsed AND three
    consecutive blocks agree within tol (or max_s is up) -> (blocks run, seconds spent, settled?)."""
    min_s = WARM_S[0] if min_s is None else min(min_s, WARM_S[0])
    hist, t0 = [], time.perf_counter()
    while True:
        hist.append(run_block())
        el = time.perf_counter() - t0
        last = hist[-3:]
        settled = len(last) == 3 and (max(last) - min(last)) <= tol * min(last)
        if (el >= min_s and (settled or min_s == 0.0)) or el >= max_s:
            return len(hist), el, settled


def time_steps(step, steps, warmup):
    """The headline's timing -> (seconds per timed step, the last timed step's outputs, warm-up info).  `warmup` steps,
    warm-up by time (steady_warmup over blocks of at most 50 steps, so that it stays within its bound whatever --steps
    is), then exactly `steps` steps between two device synchronisations."""
    for _ in range(warmup):
        step()
    n_block = max(1, min(steps, 50))

    def block():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_block):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n_block
    n_warm, warm_s, settled = steady_warmup(block)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / steps
    return sec, out, dict(warmup_blocks=n_warm, warmup_block_steps=n_block, warmup_s=warm_s,
                          warmup_settled=bool(settled), timed_region_s=sec * steps)


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """`--dump-outputs DIR`: each array as DIR/<name>.npy in float32.  When all of them together exceed 64 MB, every array
    above an equal share of that budget is replaced by a fixed sample of its flattened elements (seed 0, sorted, repeats
    removed), the same on every run with the same arguments -> {name: shape written, or the sampled count}."""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.numel() for a in arrays.values()) * 4
    share = DUMP_BUDGET_BYTES // 4 // len(arrays)
    written = {}
    for name, a in arrays.items():
        a = a.detach()
        if total > DUMP_BUDGET_BYTES and a.numel() > share:
            idx = np.unique(np.random.default_rng(0).integers(0, a.numel(), share))
            a = a.reshape(-1)[torch.from_numpy(idx).to(a.device)]
            written[name] = {"sampled": int(idx.size), "of": int(arrays[name].numel()), "shape": list(arrays[name].shape)}
        else:
            written[name] = {"shape": list(a.shape)}
        np.save(os.path.join(out_dir, name + ".npy"), a.float().cpu().numpy())
    return written


def time_forward(ops, graph, pairs, Z, beta, t, steps, warmup, repeats, min_region_s=None, info=None):
    """-> (per-block seconds per step, per-phase kernel seconds (HIP events on the launch stream, median)).
    W warm-up steps, warm-up by time (steady_warmup), then max(repeats, enough for min_region_s) blocks of exactly
    `steps` steps."""
    def step():
        p, a, s = ops.route_fwd(graph, Z, t)
        H = ops.aggregate_fwd(graph, Z, beta, p, a, s)
        return ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs)

    def block():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    min_region_s = REGION_S[0] if min_region_s is None else min(min_region_s, REGION_S[0])
    for _ in range(warmup):
        step()
    n_warm, warm_s, settled = steady_warmup(block)
    est = block()
    n_blocks = int(min(2000, max(repeats, np.ceil(min_region_s / max(est * steps, 1e-9)))))
    blocks = [block() for _ in range(n_blocks)]
    if info is not None:
        info.update(warmup_blocks=n_warm, warmup_s=warm_s, warmup_settled=bool(settled), timed_region_s=float(sum(blocks)) * steps)
    # per-kernel durations with HIP events on the launch stream (torch's current stream), same loop
    n_ev = min(max(steps, 20), 50)
    # ... taken INSIDE a running loop of the step: one step in EVERY of them carries the four event markers, the others keep
    # the GPU in the steady state of the timed region (clocks, caches) and the host ahead of it.  Bracketing every step of a
    # short loop of its own made the host the slower side on some boxes (three launches + four event records against 0.2 ms
    # of GPU work): the intervals then contained idle time and the phases summed to 1.2x the step while rocprofv3's durations
    # had not moved; queueing that loop behind a long memory-bound kernel measured 10 % too long as well (clocks).
    # An interval between two markers also contains the markers' own cost (a barrier packet each): a fifth marker right
    # behind the fourth measures the EMPTY interval in the same loop (EVENT_OVERHEAD_US[0], reported in the line as
    # `event_overhead_us`).  It is NOT taken off the phases: two markers back to back cost more than a marker adds to a busy
    # interval (subtracting it put route and aggregate 2-3 us UNDER rocprofv3's kernel durations), so the phase times stay
    # upper bounds — a few per cent above rocprofv3's.
    EVERY = 8
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(n_ev)]
    torch.cuda.synchronize()
    for _ in range(2 * EVERY):
        step()
    for i in range(n_ev):
        for _ in range(EVERY - 1):
            step()
        ev[i][0].record()
        p, a, s = ops.route_fwd(graph, Z, t)
        ev[i][1].record()
        H = ops.aggregate_fwd(graph, Z, beta, p, a, s)
        ev[i][2].record()
        ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs)
        ev[i][3].record()
        ev[i][4].record()
    torch.cuda.synchronize()
    empty = float(np.median([ev[i][3].elapsed_time(ev[i][4]) for i in range(n_ev)])) * 1e-3
    EVENT_OVERHEAD_US[0] = empty * 1e6
    ktime = {n: float(np.median([ev[i][j].elapsed_time(ev[i][j + 1]) for i in range(n_ev)])) * 1e-3
             for j, n in enumerate(NAMES)}
    return blocks, ktime


def phase_table(ktime, abytes, mbytes, peak, traffic=None, l2=None):
    out = {}
    for n in NAMES:
        out[n] = dict(avg_us=ktime[n] * 1e6, algorithmic_bytes=abytes[n], moved_bytes=mbytes[n],
                      achieved_GBs=mbytes[n] / ktime[n] / 1e9, frac=mbytes[n] / ktime[n] / 1e9 / peak,
                      algorithmic_GBs=abytes[n] / ktime[n] / 1e9)
        if traffic is not None:
            out[n]["traffic"] = traffic[n]
            out[n]["hbm_GBs"] = traffic[n] / ktime[n] / 1e9
            out[n]["hbm_frac"] = traffic[n] / ktime[n] / 1e9 / HBM_PEAK_GBS
        if l2 is not None and n in l2:
            out[n]["l2_traffic"] = l2[n]["l2_bytes"]                       # counted at the L2s' request side
            out[n]["l2_traffic_over_moved"] = l2[n]["l2_bytes"] / mbytes[n] if mbytes[n] else None
            out[n]["l2_hit_rate"] = l2[n]["hit_rate"]
            out[n]["l2_GBs"] = l2[n]["l2_bytes"] / ktime[n] / 1e9
            out[n]["l2_frac"] = l2[n]["l2_bytes"] / ktime[n] / 1e9 / L2_PEAK_GBS
    return out


def scatter_entry(kernels, E, peak):
    t_ = (kernels["route"]["avg_us"] + kernels["aggregate"]["avg_us"]) * 1e-6
    mb = kernels["route"]["moved_bytes"] + kernels["aggregate"]["moved_bytes"]
    ab = kernels["route"]["algorithmic_bytes"] + kernels["aggregate"]["algorithmic_bytes"]
    out = {"kernels": "route+aggregate", "avg_us": t_ * 1e6, "algorithmic_bytes": ab, "moved_bytes": mb,
           "achieved_GBs": mb / t_ / 1e9, "frac": mb / t_ / 1e9 / peak, "edges_per_s": E / t_}
    if "traffic" in kernels["route"]:
        tr = kernels["route"]["traffic"] + kernels["aggregate"]["traffic"]
        out.update(traffic=tr, hbm_GBs=tr / t_ / 1e9, hbm_frac=tr / t_ / 1e9 / HBM_PEAK_GBS)
    return out


def hbm_bound_section(ops, device, K, d, nhid, steps, warmup, repeats, workload="snap_patents", scale=0.25, dtype="f32"):
    """The same forward on a graph whose Z and H tables are far larger than every cache (snap-patents-shaped,
    a quarter of its size: N = 731k, tables 2 x 1.5 GB in fp32): here the HBM roofline is the bound."""
    wb = 2 if dtype == "bf16" else 4
    sg, split, graph, pairs, model, x, Z = build_workload(workload, device, K, d, nhid, scale=scale, elem_bytes=wb)
    if dtype == "bf16":
        Z = Z.to(torch.bfloat16)
    del model, x
    E, P, N = graph.n_edges, pairs.n_pairs, graph.n_nodes
    blocks, ktime = time_forward(ops, graph, pairs, Z, 0.5, 1.0, steps, warmup, repeats)
    ab, mb = algorithmic_bytes(K, d, N, E, P, w=wb), moved_bytes(graph, pairs, K, d, w=wb)
    key = f"{workload}x{scale:g}_K{K}_d{d}_{dtype}"
    traffic, src = pmc_traffic(key)
    _bound, _peak, bound_how = memory_bound(2 * N * K * d * wb, mb, traffic)
    kernels = phase_table(ktime, ab, mb, HBM_PEAK_GBS, traffic, pmc_l2(key))
    dom = max(NAMES, key=lambda n: ktime[n])
    med = float(np.median(blocks))
    out = {"workload": f"{workload}-synthetic x{scale:g} (seed 0): N={N}, E_sym={E}, P={P}, K={K}, d={d}, {dtype}; "
                       f"Z+H = {2 * N * K * d * wb / 2**30:.2f} GiB",
           "pmc_key": key, "table_bytes": 2 * N * K * d * wb, "n_nodes": N, "E_sym": E, "P": P,
           "steps": steps, "repeats": repeats, "ms_per_step": med * 1e3, "ms_per_step_blocks": [b * 1e3 for b in blocks],
           "edges_per_s": (E + P) / med,
           "roofline": {"bound": "hbm", "bound_decided_by": bound_how, "kernel": dom,
                        "achieved": kernels[dom]["achieved_GBs"], "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": kernels[dom]["frac"], "traffic": kernels[dom].get("traffic"),
                        "traffic_source": src, "moved_bytes": kernels[dom]["moved_bytes"],
                        "algorithmic_bytes": kernels[dom]["algorithmic_bytes"], "avg_us": kernels[dom]["avg_us"]},
           "edge_scatter": scatter_entry(kernels, E, HBM_PEAK_GBS),
           "kernels": kernels,
           "step_bytes_over_time_GBs": sum(mb.values()) / med / 1e9}
    del graph, pairs, Z
    torch.cuda.empty_cache()
    return out


def under_launcher() -> bool:
    from disenlink_amd.launch import under_launcher as f
    return f()


def self_launch(n_gpus: int, argv) -> int:
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks as CHILD processes
    (disenlink_amd/launch.py: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <same
    arguments>`), pass their stderr through, relay rank 0's JSON line on stdout and return the children's exit code
    (non-zero when any rank failed or no line came back).  This process makes NO GPU / HIP call — it neither asks
    torch.cuda anything nor loads the library — and replaces no running program (no os.exec*)."""
    from disenlink_amd.launch import launch_ranks
    # the arguments travel in the environment: torch.distributed.run's parser classifies every "--option" on its command
    # line before it reaches the script's remainder, and e.g. "--d" is an ambiguous prefix of its "--duplicate-*-filters"
    return launch_ranks(n_gpus, [os.path.abspath(__file__)], [], cwd=ROOT, result_marker='"metric"',
                        env_extra={"DL_BENCH_SELF_LAUNCHED": "1", "DL_BENCH_ARGV": json.dumps(list(argv))})


def launch_check(rank: int, world: int) -> int:
    """DL_BENCH_LAUNCH_CHECK=1 (CPU tests of the launch path, no GPU needed): every rank joins a gloo group, one
    all-reduce proves the rendezvous, rank 0 prints a line marked as a launch check.  =fail makes the last rank exit
    non-zero before the rendezvous, to prove that a failing child fails the launch."""
    import torch.distributed as dist
    mode = os.environ["DL_BENCH_LAUNCH_CHECK"]
    if mode == "fail" and rank == world - 1:
        return 3
    dist.init_process_group("gloo", rank=rank, world_size=world)
    v = torch.tensor([float(rank + 1)])
    dist.all_reduce(v)
    if rank == 0:
        print(json.dumps({"metric": "launch check only (no measurement)", "launch_check": True, "n_gpus": world,
                          "rank_sum": float(v), "self_launched": bool(os.environ.get("DL_BENCH_SELF_LAUNCHED"))}), flush=True)
    dist.destroy_process_group()
    return 0


def training_epoch_section(device, K, d, nhidden, split, x, workload, epochs=150):
    """One epoch of the training loop end to end (main_disentangled.py:191-214 through train.run_link_prediction: projection,
    route, aggregate, one-pass scorer, loss, backward, Adam, validation AUC, early-stopping bookkeeping) on the headline
    workload's own graph, link split (m = 5) and features — wall time per epoch, eager and replayed from a HIP graph.  An
    extra of the line, not the headline metric."""
    from disenlink_amd import native
    from disenlink_amd.model import Disentangle
    from disenlink_amd.train import prepare_run, run_link_prediction
    run = prepare_run(split, device, row_bytes=K * d * 4)
    n_feat = int(x.shape[1])
    out = {"workload": f"{workload}: the headline's graph and link split (m=5): {run.n_pos + run.n_neg} train + "
                       f"{run.label_val.numel()} validation pairs, F={n_feat} K={K} d={d} nhid={nhidden}",
           "epochs": epochs, "compiled_binding": bool(native.available()),
           "bookkeeping": "device (dl_epoch_finish; history read one epoch behind)"
           if os.environ.get("DL_DEVICE_EARLY_STOP", "1") != "0" else "host (read back every epoch)"}
    for key, use_graph in (("eager_ms", False), ("replayed_ms", True)):
        best = None
        for _rep in range(2):
            torch.manual_seed(0)
            model = Disentangle(n_feat, nhidden, d, nfactor=K, beta=0.5, t=1).to(device)
            run_link_prediction(model, x, run, epochs=3, lr=1e-4, use_graph=use_graph)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = run_link_prediction(model, x, run, epochs=epochs, lr=1e-4, use_graph=use_graph)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / max(res.epochs_run, 1) * 1e3     # (incl. the graph capture when replayed)
            best = dt if best is None else min(best, dt)
        out[key] = best
    return out


def dropin_epoch_section(device, K, d, nhidden, split, x, edges, workload, epochs=40, static_masks=(False, True)):
    """The epoch a DisenLink user gets from the ONE-LINE swap (`from disenlink_amd.model import Disentangle` inside the
    unchanged script): the reference's loop of main_disentangled.py:192-214 as it is written — dense adj_sym, dense masks
    built like :134-190, `model(x, adj_sym)` -> boolean-mask gathers of the [N,N] prediction -> F.binary_cross_entropy ->
    backward -> torch.optim.Adam -> a_pred[all_val_adj == 1].cpu() -> sklearn.roc_auc_score — around the drop-in module.
    Wall time per epoch, a per-stage table from a second pass with a synchronisation after every stage, the dense scorer
    backward (dl_score_allpairs_bwd) by HIP events, with and without `model.assume_static_loss_masks(pos, neg)` (the one
    optional extra line that removes the backward's host read)."""
    import torch.nn.functional as F
    from sklearn.metrics import roc_auc_score
    from disenlink_amd import ops
    from disenlink_amd.model import Disentangle
    n = split.n_nodes
    dev = device

    def dense(u, v, summed=False):                                  # torch.sparse_coo_tensor(idx, ones).to_dense()
        a = torch.zeros(n, n, device=dev)
        idx = (torch.as_tensor(u, device=dev).long(), torch.as_tensor(v, device=dev).long())
        if summed:
            a.index_put_(idx, torch.ones(idx[0].numel(), device=dev), accumulate=True)
        else:
            a[idx] = 1.0
        return a
    ori_adj = dense(edges[0], edges[1])
    adj = dense(split.train_src, split.train_dst)
    adj_sym = ((adj + adj.t()) != 0).float()
    pos_train_adj = dense(split.train_src, split.train_dst, summed=True)       # :176-179: summed, never binarised
    neg_raw = split.raw["neg_train"] if getattr(split, "raw", None) else (split.neg_train.u, split.neg_train.v)
    neg_train_adj = dense(neg_raw[0], neg_raw[1], summed=True)
    all_val_adj = dense(split.val.u, split.val.v)
    m = split.m
    n_feat = int(x.shape[1])
    out = {"workload": f"{workload}: N={n}, dense [N,N] masks ({n * n * 4 / 1e6:.0f} MB each), "
                       f"{int((pos_train_adj == 1).sum())} + {int((neg_train_adj == 1).sum())} train entries, "
                       f"{int((all_val_adj == 1).sum())} validation entries, F={n_feat} K={K} d={d} nhid={nhidden}",
           "loop": "main_disentangled.py:192-214 verbatim (dense masks, F.binary_cross_entropy, torch.optim.Adam, "
                   "sklearn.roc_auc_score on .cpu())", "epochs": epochs}

    def run(static, n_epochs, stages=None):
        torch.manual_seed(0)
        model = Disentangle(n_feat, nhidden, d, nfactor=K, beta=0.5, t=1).to(dev)
        if static:
            model.assume_static_loss_masks(pos_train_adj, neg_train_adj)
        optimizer = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-4)
        best_auc, stale, weights = 0, 0, None
        from copy import deepcopy

        def mark(name, t0):
            if stages is None:
                return t0
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            stages[name] = stages.get(name, 0.0) + (t1 - t0)
            return t1
        for _epoch in range(n_epochs):
            t0 = time.perf_counter() if stages is not None else 0.0
            model.train()
            h_all_factor, a_pred = model(x, adj_sym)
            t0 = mark("forward: model(x, adj_sym)", t0)
            loss = F.binary_cross_entropy(a_pred[pos_train_adj == 1].unsqueeze(0), ori_adj[pos_train_adj == 1].unsqueeze(0)) + \
                F.binary_cross_entropy(a_pred[neg_train_adj == 1].unsqueeze(0), ori_adj[neg_train_adj == 1].unsqueeze(0)) / m
            t0 = mark("loss: 4 boolean-mask gathers of [N,N] + 2 BCE", t0)
            optimizer.zero_grad()
            loss.backward()
            t0 = mark("backward", t0)
            optimizer.step()
            t0 = mark("optimizer.step (torch.optim.Adam over 4K parameters)", t0)
            model.eval()
            pred_score = a_pred[all_val_adj == 1]
            link_label = ori_adj[all_val_adj == 1]
            auc = roc_auc_score(link_label.cpu().detach().numpy(), pred_score.cpu().detach().numpy())
            t0 = mark("validation: 2 mask gathers + .cpu() + sklearn.roc_auc_score", t0)
            if auc > best_auc:
                stale, best_auc, weights = 0, auc, deepcopy(model.state_dict())
            else:
                stale += 1
            if stages is not None:
                loss.item()
            t0 = mark("bookkeeping: deepcopy(state_dict) on improvement, loss.item()", t0)
        return model, best_auc

    for static in static_masks:
        key = "static_masks" if static else "default"
        run(static, 3)                                              # warm-up: plans, planes, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _model, best = run(static, epochs)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / epochs * 1e3
        stages = {}
        run(static, 10, stages)
        out[key] = {"ms_per_epoch": ms, "best_val_auc": float(best), "pair_plan_builds_in_the_timed_epochs": int(_model._dense_plan.rebuilds),
                    "stages_ms_synchronised": {k: v / 10 * 1e3 for k, v in stages.items()},
                    "extra_line": "model.assume_static_loss_masks(pos_train_adj, neg_train_adj)" if static else None}
    # the dense scorer backward on its own (dl_score_allpairs_bwd on the support of the two train masks)
    model, _ = run(True, 1)
    with torch.no_grad():
        Z = model.project(x).contiguous()
        from disenlink_amd.graph import Graph
        g = Graph.from_dense(adj_sym, row_bytes=K * d * 4)
        H = ops.aggregate_fwd(g, Z, 0.5, *ops.route_fwd(g, Z, 1.0))
        prob = ops.score_allpairs_fwd(Z, H, 1.0)
        gp = torch.zeros_like(prob)
        sup = (pos_train_adj != 0) | (neg_train_adj != 0)
        gp[sup] = 1e-6
        plan = model._dense_plan.pairs
        for _ in range(2):
            ops.score_allpairs_bwd(Z, H, plan, 1.0, prob, gp)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        for i in range(5):
            ops.score_allpairs_bwd(Z, H, plan, 1.0, prob, gp)
            ev[i + 1].record()
        torch.cuda.synchronize()
        out["dl_score_allpairs_bwd_us"] = float(np.mean([ev[i].elapsed_time(ev[i + 1]) for i in range(5)])) * 1e3
        out["dl_score_allpairs_bwd_pairs"] = int(plan.n_pairs)
    return out

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5,
                    help="--full: blocks of --steps steps of the per-kernel pass (ms_per_step_min_median_max)")
    ap.add_argument("--workload", default="auto",
                    help="N=1: auto = squirrel_real (the real geom-gcn edge list shipped as the parity fixture) when the "
                         "fixture is present, else the seeded squirrel-shaped graph.  N>1: auto = the three blocks of "
                         "disenlink_amd/dist_bench.py (snap_patents strong, penn94 bf16 strong, squirrel weak); a name = "
                         "that workload alone with --scaling / --K / --d / --dtype")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--nhidden", type=int, default=512)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="N > 1: weak = the graph grows with the GPU count, strong = the same graph on every count")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-generic", action="store_true")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32",
                    help="storage type of the gathered Z/H tables (arithmetic is fp32 either way)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: its per-kernel roofline table, the extra sections (--sections), the CPU "
                         "baselines and the parity of the timed step against the CPU oracle (exit 4 on a mismatch)")
    ap.add_argument("--sections", default="all",
                    help="with --full: comma list of headline, hbm_bound, fwd_bwd, scorer_train, projection, dense, epoch, "
                         "dropin, cpu (default all)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (route p, a, s; H; the pair probabilities) as "
                         "DIR/<name>.npy in float32, at most 64 MB in all (a fixed seeded sample of larger outputs)")
    ap.add_argument("--hbm-scale", type=float, default=0.25, help="scale of the snap_patents graph of the hbm_bound block")
    ap.add_argument("--hbm-steps", type=int, default=5)
    ap.add_argument("--warm-s", type=float, default=0.3, help="warm up by time for at least this long (0: --warmup steps only)")
    ap.add_argument("--min-region-s", type=float, default=1.0,
                    help="--full: the blocks of the per-kernel pass last at least this long (0: --repeats blocks)")
    argv = json.loads(os.environ["DL_BENCH_ARGV"]) if os.environ.get("DL_BENCH_ARGV") and under_launcher() else None
    args = ap.parse_args(argv)                                 # (self-launched ranks: see self_launch)
    WARM_S[0], REGION_S[0] = args.warm_s, args.min_region_s
    want = lambda s: args.sections == "all" or s in args.sections.split(",")
    if args.sections != "all" and not args.full:
        ap.error("--sections selects among the --full measurements: add --full")
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.dump_outputs and not want("headline"):
        ap.error("--dump-outputs writes the headline's outputs: --sections must include headline")
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and not under_launcher():                 # BEFORE any GPU call: the parent only starts and waits
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's rank count and --gpus disagree")
    if os.environ.get("DL_BENCH_LAUNCH_CHECK"):
        raise SystemExit(launch_check(rank, world))
    one = world == 1 and not os.environ.get("DL_FORCE_SHARDED")
    if args.workload == "auto" and one:
        args.workload = "squirrel_real" if os.path.exists(os.path.join(ROOT, "tests", "golden", "real_squirrel.npz")) \
            else "squirrel"
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    # DL_REHEARSE_ON_ONE_GPU=1: every rank uses cuda:0 and the collectives go through gloo — a functional
    # rehearsal of the N>1 code on a one-GPU box (RCCL refuses two ranks on one device); never a measurement.
    rehearse = bool(os.environ.get("DL_REHEARSE_ON_ONE_GPU"))
    if rehearse and world > 1 and args.scale == 1.0 and not os.environ.get("DL_REHEARSE_FULL_SIZE"):
        # gloo carries a device table through host memory: at full snap-patents size one gather takes seconds.  The
        # rehearsal is functional only, so it runs the same blocks at 2 % of their size (the line says so).
        args.scale = 0.02
    dev_index = 0 if rehearse else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    sharded = world > 1 or bool(os.environ.get("DL_FORCE_SHARDED"))     # the env var rehearses the N>1 code on 1 GPU
    if sharded:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        from disenlink_amd.launch import stdout_to_stderr
        with stdout_to_stderr():        # backends print connection banners from C++ on fd 1: stdout is ONE JSON line
            if rehearse:
                dist.init_process_group("gloo", rank=rank, world_size=world)
            else:
                if os.environ.get("NCCL_DEBUG", "VERSION").upper() == "VERSION":      # RCCL's version banner (this image's default)
                    os.environ["NCCL_DEBUG"] = "WARN"
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
                dist.barrier()          # (communicators come up here, not inside the first timed collective)

    from disenlink_amd import _lib, ops
    lib = _lib.load()
    if args.force_generic:
        lib.dl_set_force_generic(1)

    K, d = args.K, args.d
    beta, t = 0.5, 1.0
    if sharded:
        import torch.distributed as dist
        from disenlink_amd import dist_bench
        if args.dump_outputs:
            raise SystemExit("--dump-outputs covers the one-GPU path only")
        result = dist_bench.bench_sharded(args, rank, world, device)
        if rank == 0:
            print(json.dumps(result), flush=True)
        dist.destroy_process_group()
        return

    wbytes = 2 if args.dtype == "bf16" else 4
    sg, split, graph, pairs, model, x, Z = build_workload(args.workload, device, K, d, args.nhidden, scale=args.scale,
                                                          elem_bytes=wbytes)
    E, P, N = graph.n_edges, pairs.n_pairs, graph.n_nodes
    if args.dtype == "bf16":
        Z = Z.to(torch.bfloat16)

    table_bytes = 2 * N * K * d * wbytes
    units = E + P

    def step():
        p, a, s = ops.route_fwd(graph, Z, t)
        H = ops.aggregate_fwd(graph, Z, beta, p, a, s)
        return p, a, s, H, ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs)
    step_s, last, tinfo = float("nan"), None, {}
    if want("headline"):
        step_s, last, tinfo = time_steps(step, args.steps, args.warmup)
    result = {
        "metric": "edges/sec (aggregate+score) at K=8 d=64",
        "value": units / step_s,
        "unit": "edges/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": step_s * 1e3,
        "timing": {**tinfo, "note": "warm-up = --warmup steps, then blocks of min(--steps, 50) steps until >= 0.3 s AND three "
                                    "consecutive blocks within 2 %; timed region = exactly --steps steps between two device "
                                    "synchronisations, ms_per_step = its time / --steps"},
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.dtype, "data": "real edge rows, synthetic features" if args.workload.endswith("_real") else "synthetic",
        "config": {"workload": f"{args.workload + ' (edge list of the parity fixture)' if args.workload.endswith('_real') else args.workload + '-synthetic'}(seed 0): N={N}, edge rows={sg.src.size}, 85/5/10 split, "
                               f"E_sym={E}, scored train pairs P={P} (m=5), K={K}, d={d}, beta={beta}, t={t}; "
                               "forward route+aggregate+score_pairs",
                   "K": K, "d": d, "n_nodes": N, "E_sym": E, "P": P, "fast_path": bool(lib.dl_has_fast_path(K, d))
                   and not args.force_generic},
    }
    if args.dump_outputs:
        result["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dump_outputs(
            args.dump_outputs, dict(zip(("route_p", "route_a", "route_s", "H", "prob"), last)))}
    del last
    if not args.full:
        print(json.dumps(result), flush=True)
        return

    # --full: everything beyond the headline figure
    tinfo = {}
    if want("headline"):
        blocks, ktime = time_forward(ops, graph, pairs, Z, beta, t, args.steps, args.warmup, args.repeats, info=tinfo)
        ev_over_us = EVENT_OVERHEAD_US[0]
        route_timed = ops.route_fwd(graph, Z, t)
        prob_timed = ops.score_pairs_fwd(Z, ops.aggregate_fwd(graph, Z, beta, *route_timed),
                                         pairs.pu, pairs.pv, t, pairs).clone()       # the timed step's output, for `parity`
        route_timed = (route_timed[0].clone(), route_timed[1].clone())
    else:
        blocks, ktime, prob_timed, ev_over_us, route_timed = [float("nan")], {n: float("nan") for n in NAMES}, None, None, (None, None)
    abytes, mbytes = algorithmic_bytes(K, d, N, E, P, w=wbytes), moved_bytes(graph, pairs, K, d, w=wbytes)
    pmc_key = f"{args.workload}x{args.scale:g}_K{K}_d{d}_{args.dtype}"
    traffic, traffic_src = pmc_traffic(pmc_key)
    bound, peak, bound_how = memory_bound(table_bytes, mbytes, traffic)
    in_cache = bound == "l2"
    l2 = pmc_l2(pmc_key)
    kernels = phase_table(ktime, abytes, mbytes, peak, traffic, l2)
    kernels["score"]["pairs_per_s"] = P / ktime["score"]                  # P / t_score
    dom = max(NAMES, key=lambda n: ktime[n])

    # extra: forward+backward of the same path (what one training epoch adds on top), not the headline — with its own
    # per-kernel roofline table (the training kernels are 70 % of an epoch's GPU time)
    fb_ms, fb_kernels = None, None
    if want("fwd_bwd"):
        gp = torch.full((P,), 1.0 / P, device=device)
        yb_ = (torch.rand(P, device=device) < 0.2).float()
        # the training loop's own choice (ops.one_pass_scorer_wanted, shared with model.forward_pairs_loss and dist)
        one_pass_fb = ops.one_pass_scorer_wanted(torch.float32 if args.dtype == "f32" else torch.bfloat16, N, K, d) and \
            ops.score_pairs_train_supported(pairs, K, d, ops._lib.DL_F32 if args.dtype == "f32" else ops._lib.DL_BF16)
        def train_step(ev=None):
            rec = (lambda i: ev[i].record()) if ev is not None else (lambda i: None)
            rec(0)
            p, a, s = ops.route_fwd(graph, Z, t)
            rec(1)
            H = ops.aggregate_fwd(graph, Z, beta, p, a, s)
            rec(2)
            if one_pass_fb:
                _prob, dZs, dH = ops.score_pairs_train(Z, H, pairs, t, yb_, gp)
            else:
                prob, coef = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs, want_coef=True)
                dZs, dH = ops.score_pairs_bwd(Z, H, pairs, t, prob, gp, coef=coef)
            rec(3)
            if ev is None:
                return ops.route_aggregate_bwd(graph, Z, beta, t, p, a, s, dH, dZ_accum=dZs)
            ds = torch.empty((N, K), dtype=torch.float32, device=device)
            rec(4)
            dw, dwr = ops.route_aggregate_bwd_phase1(graph, Z, beta, p, a, s, dH, ds)
            rec(5)
            ops.route_aggregate_bwd_phase2(graph, Z, beta, t, p, a, s, dH, dw, dwr, ds, dZs, True)
            rec(6)
        for _ in range(3):
            train_step()
        def fb_block(nb=max(5, args.steps // 4)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(nb):
                train_step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / nb
        steady_warmup(fb_block, min_s=0.2)
        fb_blocks = [fb_block() for _ in range(5)]
        fb_ms = float(np.median(fb_blocks)) * 1e3
        n_ev = 20
        evs = [[torch.cuda.Event(enable_timing=True) for _ in range(7)] for _ in range(n_ev)]
        for i in range(n_ev):                                   # (as in time_forward: the marked step inside a running loop)
            for _ in range(3):
                train_step()
            train_step(evs[i])
        torch.cuda.synchronize()
        med = lambda i, j: float(np.median([e[i].elapsed_time(e[j]) for e in evs])) * 1e-3
        row = K * d * wbytes
        inc = pairs.inc
        plan = graph.plan
        fb_model = {
            # one pass over the incidence rows: every pair slot (2 per pair) gathers the partner's Z and H rows and the
            # pair's label / weight; per segment the node's own Z, H rows + descriptors; per node dZ, dH rows out; per pair prob
            # out; partial slots written and read back (2 rows each)
            "scorer_one_pass" if one_pass_fb else "scorer_fwd_terms_plus_bwd":
                (med(2, 3), 2 * P * (2 * row + 4 + 8) + inc.n_seg * (2 * row + 16) + N * 2 * K * d * 4 + P * 4
                 + inc.n_slots * 2 * K * d * 4 * 2 if one_pass_fb else None,
                 2 * P * (2 * row + 16) + N * 2 * K * d * 4 if one_pass_fb else None),
            # phase 1 per edge 2*d*4*2+17, own rows; phase 2 per edge K*d*4 + d*4 + 25, per node 3*K*d*4
            "bwd_phase1": (med(4, 5), E * (2 * d * 4 * 2 + 17) + N * 2 * K * d * 4 + plan.n_seg * 16,
                           E * (2 * d * 4 * 2 + 17) + N * 2 * K * d * 4),
            "bwd_phase2": (med(5, 6), E * (row + d * 4 + 25) + N * 3 * K * d * 4 + plan.n_seg * 16 + plan.n_slots * 2 * K * d * 4,
                           E * (row + d * 4 + 25) + N * 3 * K * d * 4),
            "route": (med(0, 1), mbytes["route"], abytes["route"]),
            "aggregate": (med(1, 2), mbytes["aggregate"], abytes["aggregate"]),
        }
        fb_traffic, fb_traffic_src = pmc_traffic(pmc_key + "_train", phases=TRAIN_PHASE_KERNELS)
        fb_l2 = pmc_l2(pmc_key + "_train", phases=TRAIN_PHASE_KERNELS)
        fb_kernels = {}
        for name, (sec, mv, ab) in fb_model.items():
            e = {"avg_us": sec * 1e6, "moved_bytes": mv, "algorithmic_bytes": ab}
            if mv is not None:
                e.update(achieved_GBs=mv / sec / 1e9, frac=mv / sec / 1e9 / peak, bound=bound)
            key = "scorer" if name.startswith("scorer") else name
            if fb_traffic is not None and key in fb_traffic:
                e.update(traffic=fb_traffic[key], hbm_frac=fb_traffic[key] / sec / 1e9 / HBM_PEAK_GBS)
            if fb_l2 is not None and key in fb_l2 and fb_l2[key]["l2_bytes"] > 0:
                e.update(l2_traffic=fb_l2[key]["l2_bytes"], l2_hit_rate=fb_l2[key]["hit_rate"],
                         l2_traffic_over_moved=fb_l2[key]["l2_bytes"] / mv if mv else None,
                         l2_frac_by_counter=fb_l2[key]["l2_bytes"] / sec / 1e9 / L2_PEAK_GBS)
            fb_kernels[name] = e
        fb_kernels["_sum_of_kernels_us"] = sum(v[0] for v in fb_model.values()) * 1e6
        fb_kernels["_traffic_source"] = fb_traffic_src

    # extra: the scorer's training step in its two forms: forward storing terms + two backward passes,
    # and dl_score_pairs_train (forward, loss gradient and backward in one pass; the default for tables that live in HBM)
    scorer_train = None
    if want("scorer_train") and args.dtype == "f32":
        from disenlink_amd.metrics import pair_bce_weights
        gp = torch.full((P,), 1.0 / P, device=device)
        Hs = ops.aggregate_fwd(graph, Z, beta, *ops.route_fwd(graph, Z, t))
        yb = (torch.rand(P, device=device) < 0.2).float()
        wb = pair_bce_weights(P // 6, P - P // 6, 5, device)
        def separate():
            prob, coef = ops.score_pairs_fwd(Z, Hs, pairs.pu, pairs.pv, t, pairs, want_coef=True)
            return ops.score_pairs_bwd(Z, Hs, pairs, t, prob, gp, coef=coef)
        def one_pass():
            return ops.score_pairs_train(Z, Hs, pairs, t, yb, wb)
        times = {}
        for name, fn in (("separate_us", separate), ("one_pass_us", one_pass)):
            if name == "one_pass_us" and not ops.score_pairs_train_supported(pairs, K, d, ops._lib.DL_F32 if args.dtype == "f32" else ops._lib.DL_BF16):
                continue
            for _ in range(2):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                fn()
            e1.record()
            e1.synchronize()
            times[name] = e0.elapsed_time(e1) / 5 * 1e3
        scorer_train = {**times, "pairs": P, "forward_us": ktime["score"] * 1e6,
                        "note": "separate = dl_score_pairs_fwd(coef) + dl_score_pairs_bwd; one pass = dl_score_pairs_train"}

    # extra: the projection (excluded from the headline) — the path's only MFMA-bound kernels.
    # fp32 in / fp32 results; layer 1 and the dW1 contraction run as six exact bf16 products per term from three bf16
    # planes per operand (fp32-grade accuracy).  Two fractions: fp32-equivalent FLOP/s against the fp32
    # matrix peak (what a caller gets), and the bf16 MFMA FLOP/s actually issued (6x) against the bf16 matrix peak (how
    # busy the pipe that is used is).
    proj = None
    if want("projection") and ops.project_supported(d) and not model.single_layer:
        st = model._stacked
        W1, b1 = st[("mlp1", "weight")], st[("mlp1", "bias")]
        W2, b2 = st[("mlp2", "weight")], st[("mlp2", "bias")]
        gZ = torch.randn(N, K, d, device=device)
        def ev_time(fn, reps=10):
            for _ in range(2):
                fn()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
            e[0].record()
            for i in range(reps):
                fn()
                e[i + 1].record()
            torch.cuda.synchronize()
            return float(np.mean([e[i].elapsed_time(e[i + 1]) for i in range(reps)])) * 1e-3
        Fx, nh = x.shape[1], W1.shape[1]
        t_f = ev_time(lambda: ops.project_fwd(x, W1, b1, W2, b2))
        t_b = ev_time(lambda: ops.project_bwd(x, W1, b1, W2, gZ))
        _Zk, hid_kept = ops.project_fwd(x, W1, b1, W2, b2, keep_hid=True)
        t_fk = ev_time(lambda: ops.project_fwd(x, W1, b1, W2, b2, keep_hid=True))
        t_bk = ev_time(lambda: ops.project_bwd(x, W1, b1, W2, gZ, hid=hid_kept))
        fl_f = 2.0 * N * K * nh * (Fx + d)
        fl_b = 2.0 * N * K * nh * (2 * Fx + 2 * d)              # recomputed layer 1, dW1, dhid, dW2
        fl_bk = 2.0 * N * K * nh * (Fx + 2 * d)                 # kept hidden layer: dW1, dhid, dW2
        planes = not os.environ.get("DL_PROJECT_FP32_MFMA")
        def both(fl, tt):
            e = {"avg_us": tt * 1e6, "achieved": fl / tt / 1e12, "frac": fl / tt / 1e12 / FP32_MFMA_PEAK_TFLOPS}
            if planes:
                e["bf16_pipe_TFLOPs"] = 6.0 * fl / tt / 1e12
                e["bf16_pipe_frac"] = 6.0 * fl / tt / 1e12 / BF16_MFMA_PEAK_TFLOPS
            return e
        proj = {"bound": "mfma", "dtype": "f32" if not planes else
                "f32 results; products from three bf16 planes per operand (six exact bf16 MFMA products per term)",
                "peak": FP32_MFMA_PEAK_TFLOPS, "bf16_peak": BF16_MFMA_PEAK_TFLOPS,
                "unit": "TFLOP/s (fp32-equivalent against the fp32 matrix peak; bf16_pipe_* = issued bf16 MFMA flops, "
                        "6 per fp32 flop, against the dense bf16 peak — an upper bound: the recompute form's kernel A (layer 1 "
                        "again, dW2, dhid) still runs fp32 MFMA)",
                "shape": {"N": N, "F": Fx, "K": K, "nhid": nh, "d": d},
                "fwd": both(fl_f, t_f),
                # `bwd`: the RECOMPUTE form (layer 1 again; what graphs too large to keep the hidden layer take);
                # `bwd_from_kept_hidden`: the form the training loop runs whenever the hidden layer fits (ops.keep_hidden)
                "bwd": dict(both(fl_b, t_b), form="recompute (hidden layer not kept: graphs beyond ops.keep_hidden)"),
                "fwd_keeping_hidden": {"avg_us": t_fk * 1e6},
                "bwd_from_kept_hidden": dict(both(fl_bk, t_bk), form="kept hidden layer"),
                # what an epoch of the training loop runs at this shape (ops.keep_hidden: the forward keeps the hidden layer,
                # the backward starts from it; round 5: kernel A of that backward on the bf16 matrix path too, d <= 64)
                "training_loop": {"form": "kept hidden layer" if ops.keep_hidden(N, Fx, K, nh) else "recompute",
                                  "fwd_us": (t_fk if ops.keep_hidden(N, Fx, K, nh) else t_f) * 1e6,
                                  "bwd_us": (t_bk if ops.keep_hidden(N, Fx, K, nh) else t_b) * 1e6}}

    # extra: the dense [N,N] scorer of the drop-in forward (model.py:109-113 as written): Gram products on MFMA
    dense = None
    if want("dense") and N <= 12000 and args.dtype == "f32":
        Hd = ops.aggregate_fwd(graph, Z, beta, *ops.route_fwd(graph, Z, t))
        for _ in range(2):
            ops.score_allpairs_fwd(Z, Hd, t)
        evd = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        evd[0].record()
        for i in range(5):
            ops.score_allpairs_fwd(Z, Hd, t)
            evd[i + 1].record()
        torch.cuda.synchronize()
        t_d = float(np.mean([evd[i].elapsed_time(evd[i + 1]) for i in range(5)])) * 1e-3
        nt = (N + 127) // 128                                   # 128x128 tiles; only u tile <= v tile is computed
        fl_d = 4.0 * K * d * 128 * 128 * (nt * (nt + 1) // 2)   # MFMA flops executed (P is symmetric: half mirrored)
        split_d = not os.environ.get("DL_DENSE_FP32_MFMA")
        dense = {"bound": "mfma", "dtype": "f32 results from three bf16 planes per operand (six exact products per term)"
                 if split_d else "f32", "peak": FP32_MFMA_PEAK_TFLOPS,
                 "unit": "TFLOP/s (fp32-equivalent, against the fp32 matrix peak)", "pairs": N * N,
                 "avg_us": t_d * 1e6, "achieved": fl_d / t_d / 1e12, "frac": fl_d / t_d / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                 "effective": 4.0 * N * N * K * d / t_d / 1e12, "pairs_per_s": N * N / t_d}
        if split_d:
            dense["bf16_pipe_frac"] = 6.0 * fl_d / t_d / 1e12 / BF16_MFMA_PEAK_TFLOPS

    bound_note = ("Z+H (%.0f MB) sit in the XCD L2s / the Infinity Cache: the bytes the kernels move come from L2, priced "
                  "against the L2 bandwidth (MI355X_MICROARCH.md: 34.5 TB/s; its L2-resident row-gather rates are "
                  "16.8-18.8 TB/s, lower bounds); hbm_* = HBM-side bytes of the rocprofv3 PMC passes against 8 TB/s; "
                  "the HBM-bound measurement is the hbm_bound block" % (table_bytes / 1e6)) if in_cache else \
                 "the kernels' requests are served from HBM: HBM roofline"
    result.update({
        "repeats": len(blocks),
        "ms_per_step_min_median_max": [float(np.min(blocks)) * 1e3, float(np.median(blocks)) * 1e3, float(np.max(blocks)) * 1e3],
        "ms_per_step_blocks": [round(b * 1e3, 5) for b in (blocks if len(blocks) <= 24 else
                                                            blocks[:8] + blocks[len(blocks) // 2 - 4:len(blocks) // 2 + 4] + blocks[-8:])],
        "ms_per_step_blocks_note": "all blocks" if len(blocks) <= 24 else "first 8, middle 8, last 8 of %d blocks" % len(blocks),
        "block_timing": {"blocks_of_steps": args.steps, **tinfo,
                         "note": "the per-kernel pass (--full), after the headline's timed steps: warm-up = --warmup steps, "
                                 "then blocks until >= 0.3 s AND three consecutive blocks within 2 %; R blocks of exactly "
                                 "--steps steps, R >= --repeats and >= 1 s in total; ms_per_step_* = per-step time of those "
                                 "blocks"},
        "roofline": {"bound": bound, "bound_decided_by": bound_how, "kernel": dom,
                     "achieved": kernels[dom]["achieved_GBs"],
                     "peak": peak, "unit": "GB/s", "frac": kernels[dom]["frac"],
                     "traffic": kernels[dom].get("traffic"), "traffic_source": traffic_src,
                     "hbm_frac": kernels[dom].get("hbm_frac"),
                     "l2_traffic": kernels[dom].get("l2_traffic"), "l2_traffic_over_moved": kernels[dom].get("l2_traffic_over_moved"),
                     "l2_hit_rate": kernels[dom].get("l2_hit_rate"), "l2_frac_by_counter": kernels[dom].get("l2_frac"),
                     "l2_traffic_source": "profiles/pmc_l2_latest.json (rocprofv3 TCC_READ x 128 B + TCC_WRITE x 64 B per launch)"
                     if l2 is not None else "no L2-request passes committed for this build and workload",
                     "moved_bytes": kernels[dom]["moved_bytes"], "algorithmic_bytes": kernels[dom]["algorithmic_bytes"],
                     "avg_us": kernels[dom]["avg_us"], "l2_gather_reference_GBs": list(L2_GATHER_REF_GBS),
                     "note": bound_note},
        "edge_scatter": scatter_entry(kernels, E, peak),
        "kernels": kernels,
        "kernels_note": "avg_us of a phase = HIP events around its launches on the launch stream, in every 8th step of a "
                        "running loop of the step (steady clocks, host ahead of the GPU); event_overhead_us = the EMPTY "
                        "event-to-event interval of the same loop (not subtracted: the phase times are upper bounds, a few "
                        "per cent above rocprofv3's kernel durations); the phases sum to phase_sum_over_step x ms_per_step "
                        "(the timed blocks carry no events)",
        "event_overhead_us": ev_over_us,
        "phase_sum_over_step": sum(kernels[n]["avg_us"] for n in NAMES) * 1e-6 / step_s,
        "step_bytes_over_time_GBs": sum(mbytes.values()) / step_s / 1e9,
        "kernel_source_hash": kernel_source_hash(),
    })
    if bound == "hbm" and kernels[dom]["frac"] > HBM_ACHIEVABLE_FRAC:
        result["roofline"]["frac_unverified"] = (
            "above the ~6.3 TB/s HBM can deliver: part of these bytes are served by the 256 MiB Infinity Cache " +
            ("(the fabric-side PMC counters count its hits as traffic: they cannot separate it from HBM)" if traffic is not None
             else "or the L2s, and no PMC passes exist for this build and workload") +
            "; this is NOT a fraction of the HBM roofline — the hbm_bound block (tables far beyond every cache) is")
    if fb_ms is not None:
        result["fwd_bwd"] = {"ms_per_step": fb_ms, "ms_per_step_blocks": [b * 1e3 for b in fb_blocks],
                             "edges_per_s": units / (fb_ms * 1e-3), "kernels": fb_kernels,
                             "scorer": "one pass (dl_score_pairs_train)" if one_pass_fb else
                             "dl_score_pairs_fwd storing terms + dl_score_pairs_bwd"}
    result["scorer_training_step"] = scorer_train
    result["projection"] = proj
    result["dense_allpairs"] = dense
    gcpu = graph.to("cpu") if want("cpu") and not args.no_cpu_baseline else None
    Zc = Z.float().cpu() if gcpu is not None else None
    pcpu = (pairs.pu.cpu(), pairs.pv.cpu()) if gcpu is not None else None
    label_cpu = pairs.bench_label
    if want("epoch") and args.dtype == "f32" and (args.K, args.d) == (8, 64):
        result["training_epoch"] = training_epoch_section(device, args.K, args.d, args.nhidden, split, x, args.workload)
    if want("dropin") and args.dtype == "f32" and N <= 12000:
        result["dropin_epoch"] = dropin_epoch_section(device, args.K, args.d, args.nhidden, split, x, (sg.src, sg.dst), args.workload)
        if result.get("training_epoch"):
            te = result["training_epoch"]
            result["dropin_epoch"]["over_pair_list_epoch"] = {
                k: result["dropin_epoch"][k]["ms_per_epoch"] / te["eager_ms"] for k in ("default", "static_masks") if k in result["dropin_epoch"]}
    if want("hbm_bound"):
        del graph, pairs, Z, model, x
        torch.cuda.empty_cache()
        result["hbm_bound"] = hbm_bound_section(ops, device, 8, 64, args.nhidden, args.hbm_steps, 2, args.repeats,
                                                scale=args.hbm_scale)
    if gcpu is not None:
        if N <= 12000:                                          # dense [K,N,N] fits: the reference's own form
            par_in = (pcpu[0], pcpu[1], label_cpu, prob_timed) if prob_timed is not None else None
            got = cpu_baseline(Zc, gcpu, units, beta, t, parity=par_in)
            result["cpu_baseline"], result["parity"] = got if par_in is not None else (got, None)
            # Baseline B beside it ("also reported for 1-3"): seconds, not tens of seconds
            result["cpu_baseline_sparse"] = cpu_baseline_sparse(Zc, gcpu, pcpu, units, beta, t, budget_s=8.0, label=label_cpu)
        else:                                                   # Baseline B is the baseline (configs 4-5) — with parity
            par_in = (label_cpu, prob_timed, route_timed[0], route_timed[1]) if prob_timed is not None else None
            got = cpu_baseline_sparse(Zc, gcpu, pcpu, units, beta, t, label=label_cpu, parity=par_in, bf16=args.dtype == "bf16",
                                      budget_s=90.0)
            result["cpu_baseline"], result["parity"] = got if par_in is not None else (got, None)
            if result["parity"] is not None and result["parity"].get("saturated_frac", 0.0) > 0.5:
                # the workload's random-init scores saturate (every probability 1.0: the check above is then vacuous): the
                # same step once more, UNTIMED, on the tables scaled down until the scores spread, against the same oracle
                from oracle import c_ref
                sc = 1.0
                for _try in range(6):
                    sc *= 0.5
                    Zs = (Z.float() * sc).to(Z.dtype)
                    rs = ops.route_fwd(graph, Zs, t)
                    ps = ops.score_pairs_fwd(Zs, ops.aggregate_fwd(graph, Zs, beta, *rs), pairs.pu, pairs.pv, t, pairs)
                    if float(((ps == 0) | (ps == 1)).float().mean()) < 0.05:
                        break
                Zsh = Zs.float().cpu().numpy()
                rp, cl = gcpu.rowptr.numpy(), gcpu.col.numpy()
                p_c, a_c, s_c = c_ref.route(Zsh, rp, cl, t)
                H_c = c_ref.aggregate(Zsh, rp, cl, p_c, a_c, s_c, beta)
                if args.dtype == "bf16":
                    H_c = torch.from_numpy(H_c).to(torch.bfloat16).float().numpy()
                prob_c = c_ref.score_pairs(Zsh, H_c, pcpu[0].numpy(), pcpu[1].numpy(), t)
                result["parity_unsaturated"] = parity_block(
                    prob_c, label_cpu, ps, tol_prob=2e-2 if args.dtype == "bf16" else 1e-5,
                    routing=routing_flips(rs[0], rs[1], p_c, a_c, rp, cl, (pcpu[0].numpy(), pcpu[1].numpy())),
                    what=f"the same step, untimed, on Z x {sc:g} (the workload's own random-init scores saturate) vs oracle/c/sparse_ref.c")
                result["parity_unsaturated"]["z_scale"] = sc
    print(json.dumps(result), flush=True)
    if any(result.get(k) is not None and not result[k]["ok"] for k in ("parity", "parity_unsaturated")):
        print("bench.py: the timed step's outputs do NOT match the CPU oracle (parity.ok = false)", file=sys.stderr)
        sys.exit(4)


if __name__ == "__main__":
    main()
