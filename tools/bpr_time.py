"""What the pairwise ranking trainer (dl_score_sampled_bpr_train) costs, at the synthetic squirrel workload (N 5,201, K 8, d 64,
the split's own training edge rows and m = 5), against (1) the BCE sampled trainer on the same draws and (2) the hand-rolled
ranking step a user had before it existed.

    python tools/bpr_time.py [--workload squirrel] [--rounds 7] [--reps 20] [--out profiles/bpr_time.jsonl]

Arms, interleaved in one process round after round; the figure of an arm is the MEDIAN over the rounds of the time per call,
from HIP events around the round's calls (`gpu_us`) and from the host clock around the same calls with a synchronisation at the
end (`wall_us`: the plan build of the hand-rolled arm is host work, which events do not see):
  trainer_bpr       ops.score_sampled_bpr_train on fixed tables, the epoch's k, order and k_rowptr given
  trainer_sampled   ops.score_sampled_train(logits=True) on the same tables, k, order and k_rowptr
  step_bpr          model.forward_bpr_loss + backward (projection, routing and aggregation included)
  step_hand         PairList.build([edge rows | live entries]) for the epoch, model.forward_pair_logits, torch softplus of the
                    differences, backward — the same loss, the only way to it at the parent commit
  hand_plan_build   the PairList.build of step_hand alone
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disenlink_amd import ops                                     # noqa: E402
from disenlink_amd.data import synthetic_graph                    # noqa: E402
from disenlink_amd.graph import PairList                          # noqa: E402
from disenlink_amd.model import Disentangle                       # noqa: E402
from disenlink_amd.splits import make_link_split                  # noqa: E402
from disenlink_amd.train import prepare_run                       # noqa: E402


def arms(name, dev, K, d, nhid, m, seed):
    sg = synthetic_graph(name, seed=seed)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=m, seed=seed)
    run = prepare_run(split, dev, row_bytes=K * d * 4, resample_negatives=True)
    x = torch.from_numpy(sg.features()).to(dev)
    torch.manual_seed(seed)
    model = Disentangle(sg.n_feat, nhid, d, nfactor=K, beta=0.5, t=1).to(dev)
    N, sp = sg.n_nodes, run.sampled
    w = 1.0 / sp.n_entries
    k, failed = ops.sample_negatives(sp, seed=seed, epoch=0)
    order, k_rowptr = ops.sampled_order(k, N)
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (0.1 * torch.randn(N, K, d, generator=g)).to(dev)
    H = (0.1 * torch.randn(N, K, d, generator=g)).to(dev)
    live = k >= 0
    row = (torch.arange(sp.n_entries, device=dev) // m)[live]
    pu = torch.cat([sp.src.long(), sp.src.long()[row]])
    pv = torch.cat([sp.dst.long(), k.long()[live]])

    def trainer_bpr():
        ops.score_sampled_bpr_train(Z, H, 1.0, sp, k, w, order, k_rowptr)

    def trainer_sampled():
        ops.score_sampled_train(Z, H, 1.0, sp, k, w, True, order, k_rowptr)

    def step_bpr():
        _emb, _p, _n, _v, loss = model.forward_bpr_loss(x, run.graph, sp, k, w, None, order, k_rowptr)
        model.zero_grad()
        loss.backward()

    def hand_plan_build():
        return PairList.build(pu, pv, N, row_bytes=K * d * 4)

    def step_hand():
        pairs = hand_plan_build()
        _emb, logit = model.forward_pair_logits(x, run.graph, pairs)
        loss = (w * F.softplus(logit[sp.n_rows:] - logit[:sp.n_rows][row])).sum()
        model.zero_grad()
        loss.backward()

    info = dict(workload=name, N=N, K=K, d=d, m=m, n_rows=sp.n_rows, entries=sp.n_entries, failed_draws=int(failed),
                hand_pairs=int(pu.numel()))
    return info, (("trainer_bpr", trainer_bpr, 1), ("trainer_sampled", trainer_sampled, 1), ("step_bpr", step_bpr, 1),
                  ("step_hand", step_hand, 5), ("hand_plan_build", hand_plan_build, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="squirrel")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "bpr_time.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    info, fns = arms(args.workload, dev, 8, 64, 512, 5, 0)
    for _name, fn, _div in fns:                                     # warm-up: allocations, plans, workspace
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    gpu = {n: [] for n, _f, _d in fns}
    wall = {n: [] for n, _f, _d in fns}
    for _round in range(args.rounds):
        for arm, fn, div in fns:
            reps = max(1, args.reps // div)
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
    rows = [dict(info, arm=arm, rounds=args.rounds, gpu_us=round(statistics.median(gpu[arm]), 1),
                 wall_us=round(statistics.median(wall[arm]), 1), gpu_us_min=round(min(gpu[arm]), 1),
                 gpu_us_max=round(max(gpu[arm]), 1)) for arm, _f, _d in fns]
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print(json.dumps(info))
    print("| arm | per call, HIP events [us] (min .. max) | per call, host clock [us] |")
    print("|---|---|---|")
    for r in rows:
        print(f"| {r['arm']} | {r['gpu_us']} ({r['gpu_us_min']} .. {r['gpu_us_max']}) | {r['wall_us']} |")


if __name__ == "__main__":
    main()
