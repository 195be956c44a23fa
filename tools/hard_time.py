"""What hard negatives cost (dl_sample_negatives_hard), at the synthetic squirrel workload (N 5,201, K 8, d 64, the split's own
training edge rows and m = 5), for c = 1, 2, 4, 8 candidates per entry, against the plain sampler, the ranking trainer that
then trains on the draw, and the hand-rolled selection a user had before it existed.

    python tools/hard_time.py [--workload squirrel] [--rounds 7] [--reps 20] [--out profiles/hard_time.jsonl]

Arms, interleaved in one process round after round; the figure of an arm is the MEDIAN over the rounds of the time per call,
from HIP events around the round's calls (`gpu_us`) and from the host clock around the same calls with a synchronisation at the
end (`wall_us`: the plan build of the hand-rolled arm is host work, which events do not see):
  sampler           ops.sample_negatives alone (one uniform draw per entry)
  draw_c{c}         ops.sample_hard_negatives on fixed tables; `gathered_GBps` = c E 2 K d 4 bytes over its time, and
                    `of_l2_peak` = that over the 34.5 TB/s of the XCD L2s (what the sampled trainers' row
                    passes are held against)
  trainer_bpr       ops.score_sampled_bpr_train on the same tables and the k of draw_c4, order and k_rowptr given
  step_plain        the loop's epoch with uniform negatives: ops.sample_negatives, ops.sampled_order, model.forward_bpr_loss +
                    backward (projection, routing and aggregation included)
  step_hard_c{c}    the same with an ops.HardDraw(c): the draw and the sort happen inside the forward
  hand_c{c}         the selection by hand: ops.sample_negatives with m c draws per row, PairList.build of the live pairs,
                    model.forward_pair_logits (no gradient), torch argmax per entry
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disenlink_amd import ops                                     # noqa: E402
from disenlink_amd.data import synthetic_graph                    # noqa: E402
from disenlink_amd.graph import PairList                          # noqa: E402
from disenlink_amd.model import Disentangle                       # noqa: E402
from disenlink_amd.splits import make_link_split                  # noqa: E402
from disenlink_amd.train import prepare_run                       # noqa: E402

CANDIDATES = (1, 2, 4, 8)
L2_PEAK_GBPS = 34500.0


def arms(name, dev, K, d, nhid, m, seed):
    sg = synthetic_graph(name, seed=seed)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=m, seed=seed)
    run = prepare_run(split, dev, row_bytes=K * d * 4, resample_negatives=True)
    x = torch.from_numpy(sg.features()).to(dev)
    torch.manual_seed(seed)
    model = Disentangle(sg.n_feat, nhid, d, nfactor=K, beta=0.5, t=1).to(dev)
    N, sp = sg.n_nodes, run.sampled
    E = sp.n_entries
    w = 1.0 / E
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (0.1 * torch.randn(N, K, d, generator=g)).to(dev)
    H = (0.1 * torch.randn(N, K, d, generator=g)).to(dev)
    k4, _x, failed = ops.sample_hard_negatives(Z, H, 1.0, sp, 4, seed=seed, epoch=0)
    order, k_rowptr = ops.sampled_order(k4, N)
    ex = (sp.ex_rowptr, sp.ex_col)
    entry_u = sp.entry_u().long()

    def sampler():
        ops.sample_negatives(sp, seed=seed, epoch=0)

    def draw(c):
        return lambda: ops.sample_hard_negatives(Z, H, 1.0, sp, c, seed=seed, epoch=0)

    def trainer_bpr():
        ops.score_sampled_bpr_train(Z, H, 1.0, sp, k4, w, order, k_rowptr)

    def step(k, o=None, r=None):
        _emb, _p, _n, _v, loss = model.forward_bpr_loss(x, run.graph, sp, k, w, None, o, r)
        model.zero_grad()
        loss.backward()

    def step_plain():
        k, _f = ops.sample_negatives(sp, seed=seed, epoch=0)
        o, r = ops.sampled_order(k, N)
        step(k, o, r)

    def step_hard(c):
        return lambda: step(ops.HardDraw(c, seed, 0))

    def hand(c):
        def fn():
            kc, _f = ops.sample_negatives(sp.src, m * c, N, ex, seed=seed, epoch=0)       # [n_rows, m c] = [E, c]
            live = kc >= 0
            pu, pv = entry_u.repeat_interleave(c)[live], kc.long()[live]
            pairs = PairList.build(pu, pv, N, row_bytes=K * d * 4)
            with torch.no_grad():
                _emb, logit = model.forward_pair_logits(x, run.graph, pairs)
            full = torch.full((E * c,), float("-inf"), device=dev)
            full[live] = logit
            best = full.view(E, c).argmax(dim=1, keepdim=True)
            return kc.view(E, c).gather(1, best)
        return fn

    info = dict(workload=name, N=N, K=K, d=d, m=m, n_rows=sp.n_rows, entries=E, failed_entries_c4=int(failed))
    fns = [("sampler", sampler, 1)] + [(f"draw_c{c}", draw(c), 1) for c in CANDIDATES] + [("trainer_bpr", trainer_bpr, 1),
                                                                                           ("step_plain", step_plain, 1)]
    fns += [(f"step_hard_c{c}", step_hard(c), 1) for c in CANDIDATES] + [(f"hand_c{c}", hand(c), 10) for c in CANDIDATES]
    return info, fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="squirrel")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "hard_time.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K, d, m = 8, 64, 5
    info, fns = arms(args.workload, dev, K, d, 512, m, 0)
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
    rows = []
    for arm, _f, _d in fns:
        r = dict(info, arm=arm, rounds=args.rounds, gpu_us=round(statistics.median(gpu[arm]), 1),
                 wall_us=round(statistics.median(wall[arm]), 1), gpu_us_min=round(min(gpu[arm]), 1), gpu_us_max=round(max(gpu[arm]), 1))
        if arm.startswith("draw_c"):
            c = int(arm[len("draw_c"):])
            gbps = c * info["entries"] * 2 * K * d * 4 / (r["gpu_us"] * 1e-6) / 1e9
            r.update(gathered_GBps=round(gbps, 1), of_l2_peak=round(gbps / L2_PEAK_GBPS, 3))
        rows.append(r)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print(json.dumps(info))
    print("| arm | per call, HIP events [us] (min .. max) | per call, host clock [us] | gathered [GB/s] (of the L2 peak) |")
    print("|---|---|---|---|")
    for r in rows:
        extra = f"{r['gathered_GBps']} ({r['of_l2_peak']})" if "gathered_GBps" in r else ""
        print(f"| {r['arm']} | {r['gpu_us']} ({r['gpu_us_min']} .. {r['gpu_us_max']}) | {r['wall_us']} | {extra} |")


if __name__ == "__main__":
    main()
