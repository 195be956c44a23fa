"""Per-epoch training time with the negatives (a) fixed, as the split drew them, (b) drawn anew each epoch on the device
(sampler + sort + the two passes of the sampled trainer) and (c) drawn anew on the host and planned with PairList.build every
epoch — what a user had before (b) existed.  An epoch = forward, loss, backward and the Adam step on the synthetic workload.

    python tools/resample_time.py [--workloads squirrel,chameleon] [--rounds 7] [--epochs 10] [--out profiles/resample_time.jsonl]

The three arms run interleaved in one process, round after round; the figure of an arm is the MEDIAN over the rounds of the
time per epoch, from HIP events around the round's epochs (`gpu_us`) and from the host clock around the same epochs with a
synchronisation at the end (`wall_us`: arm (c) spends most of its time on the host, which events do not see)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disenlink_amd import ops                                     # noqa: E402
from disenlink_amd.data import synthetic_graph                    # noqa: E402
from disenlink_amd.graph import PairList                          # noqa: E402
from disenlink_amd.model import Disentangle                       # noqa: E402
from disenlink_amd.splits import _unique, make_link_split, structured_negatives      # noqa: E402
from disenlink_amd.train import _loss_vectors, _make_adam, prepare_run              # noqa: E402


def arms(name, dev, K, d, nhid, m, seed):
    sg = synthetic_graph(name, seed=seed)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=m, seed=seed)
    run = prepare_run(split, dev, row_bytes=K * d * 4, resample_negatives=True)
    x = torch.from_numpy(sg.features()).to(dev)
    torch.manual_seed(seed)
    model = Disentangle(sg.n_feat, nhid, d, nfactor=K, beta=0.5, t=1).to(dev)
    opt = _make_adam(model, True, 1e-4, 5e-4)
    N, sp, pv_pairs = sg.n_nodes, run.sampled, run.pos_val_pairs
    a, n_val = run.n_pos, run.label_val.numel()
    label_all, weight_all = _loss_vectors(run, dev)
    label_pv = torch.cat([run.label_pos, run.label_val])
    weight_pv = torch.cat([torch.full((a,), 1.0 / a, device=dev), torch.zeros(n_val, device=dev)])
    neg_w = 1.0 / (m * sp.n_entries)
    epoch_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(seed)
    edge_keys = _unique(np.asarray(sg.src, dtype=np.int64) * N + np.asarray(sg.dst, dtype=np.int64))
    train_src = np.sort(split.train_src.astype(np.int64))

    def finish(loss):
        opt.zero_grad()
        loss.backward()
        opt.step()

    def fixed():
        _emb, _prob, loss = model.forward_pairs_loss(x, run.graph, run.train_val_pairs, label_all, weight_all)
        finish(loss)

    def resampled():
        k, _ = ops.sample_negatives(sp, seed=seed, epoch=epoch_dev, n_failed=n_failed)
        order, k_rowptr = ops.sampled_order(k, N)
        _emb, _s, _n, loss = model.forward_pairs_resampled_loss(x, run.graph, pv_pairs, label_pv, weight_pv, sp, k, neg_w,
                                                                order, k_rowptr)
        epoch_dev.add_(1)
        finish(loss)

    def host_rebuild():
        ks = np.concatenate([structured_negatives(train_src, N, edge_keys, rng) for _ in range(m)])
        us = np.tile(train_src, m)
        pu = torch.cat([pv_pairs.pu.long(), torch.from_numpy(us).to(dev)])
        pv = torch.cat([pv_pairs.pv.long(), torch.from_numpy(ks).to(dev)])
        pairs = PairList.build(pu, pv, N, row_bytes=K * d * 4)
        label = torch.cat([label_pv, torch.zeros(us.size, device=dev)])
        weight = torch.cat([weight_pv, torch.full((us.size,), neg_w, device=dev)])
        _emb, _prob, loss = model.forward_pairs_loss(x, run.graph, pairs, label, weight)
        finish(loss)

    info = dict(workload=name, N=N, K=K, d=d, m=m, train_rows=int(train_src.size), fixed_pairs=run.train_val_pairs.n_pairs,
                pos_val_pairs=pv_pairs.n_pairs, sampled_entries=sp.n_entries)
    return info, (("a_fixed", fixed), ("b_resampled", resampled), ("c_host_rebuild", host_rebuild)), n_failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="squirrel,chameleon")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "resample_time.jsonl"))
    ap.add_argument("--arms", default="a_fixed,b_resampled,c_host_rebuild", help="a subset, e.g. for a kernel trace in a run of its own")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name in args.workloads.split(","):
        info, fns, n_failed = arms(name, dev, 8, 64, 512, 5, 0)
        fns = tuple(f for f in fns if f[0] in args.arms.split(","))
        for _name, fn in fns:                                       # warm-up: allocations, plans, bound labels
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        gpu = {n: [] for n, _ in fns}
        wall = {n: [] for n, _ in fns}
        for _round in range(args.rounds):
            for arm, fn in fns:
                reps = args.epochs if arm != "c_host_rebuild" else max(1, args.epochs // 5)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                wall[arm].append((time.perf_counter() - t0) / reps * 1e6)
                gpu[arm].append(e0.elapsed_time(e1) / reps * 1e3)
        for arm, _fn in fns:
            rows.append(dict(info, arm=arm, rounds=args.rounds, gpu_us=round(statistics.median(gpu[arm]), 1),
                             wall_us=round(statistics.median(wall[arm]), 1), gpu_us_min=round(min(gpu[arm]), 1),
                             gpu_us_max=round(max(gpu[arm]), 1), failed_draws=int(n_failed[0])))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print("| workload | arm | epoch, HIP events [us] (min .. max) | epoch, host clock [us] |")
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['workload']} | {r['arm']} | {r['gpu_us']} ({r['gpu_us_min']} .. {r['gpu_us_max']}) | {r['wall_us']} |")


if __name__ == "__main__":
    main()
