#!/usr/bin/env python3
"""usage: tools/rank_time.py [--reps R] [--skip-snap]  -> one JSON line per shape: ops.score_topk / ops.score_ranks against
the dense scorer (ops.score_allpairs_fwd) and dense + torch.topk, timed in the same process (events, after warm-up).
Shapes: the bench graph (squirrel synthetic, N = 5,201, K = 8, d = 64, every node a query, k = 100) and the snap-patents
synthetic (N = 2,923,922, 4,096 queries, k = 100; no dense comparison: [N,N] cannot exist).  FLOP rates: the dense scorer
counts the tiles it computes, 4 (nt(nt+1)/2 128^2) K d; the scan 4 Q N K d."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disenlink_amd import ops  # noqa: E402
from disenlink_amd.data import SPECS  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def tables(N, K, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(N, K, d, device="cuda", generator=g) / d ** 0.5,
            torch.randn(N, K, d, device="cuda", generator=g) / d ** 0.5)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    K, d, k = 8, 64, 100
    N = SPECS["squirrel"]["N"]
    Z, H = tables(N, K, d, 0)
    q = torch.arange(N, device="cuda")
    src = torch.randint(0, N, (20000,), device="cuda")
    dst = torch.randint(0, N, (20000,), device="cuda")

    def dense_topk():
        p = ops.score_allpairs_fwd(Z, H, 1.0)
        p.fill_diagonal_(-1.0)
        return torch.topk(p, k, dim=1)
    t_dense = timed(lambda: ops.score_allpairs_fwd(Z, H, 1.0), reps)
    t_dense_topk = timed(dense_topk, reps)
    t_topk = timed(lambda: ops.score_topk(Z, H, 1.0, q, k), reps)
    t_ranks = timed(lambda: ops.score_ranks(Z, H, 1.0, src, dst), reps)
    nt = (N + 127) // 128
    dense_rate = 4.0 * (nt * (nt + 1) / 2 * 128 ** 2) * K * d / (t_dense * 1e-3) / 1e12
    scan_rate = 4.0 * N * N * K * d / (t_topk * 1e-3) / 1e12
    print(json.dumps({"shape": "squirrel", "N": N, "K": K, "d": d, "Q": N, "k": k, "dense_ms": round(t_dense, 4),
                      "dense_topk_ms": round(t_dense_topk, 4), "topk_ms": round(t_topk, 4), "ranks_20k_ms": round(t_ranks, 4),
                      "topk_over_dense": round(t_topk / t_dense, 3), "dense_tflops": round(dense_rate, 1),
                      "scan_tflops": round(scan_rate, 1)}), flush=True)
    del Z, H
    if "--skip-snap" in sys.argv:
        return
    N = SPECS["snap_patents"]["N"]
    Z, H = tables(N, K, d, 1)
    Q = 4096
    q = torch.randperm(N, device="cuda")[:Q]
    src, dst = q.repeat_interleave(4), torch.randint(0, N, (4 * Q,), device="cuda")
    r = max(1, reps // 5)
    t_topk = timed(lambda: ops.score_topk(Z, H, 1.0, q, k), r)
    t_ranks = timed(lambda: ops.score_ranks(Z, H, 1.0, src, dst), r)
    ws = int(ops._lib.load().dl_score_topk_workspace_bytes(N, K, d, Q, k, 0))
    print(json.dumps({"shape": "snap_patents", "N": N, "K": K, "d": d, "Q": Q, "k": k, "topk_ms": round(t_topk, 3),
                      "ranks_16k_ms": round(t_ranks, 3), "scan_tflops": round(4.0 * Q * N * K * d / (t_topk * 1e-3) / 1e12, 1),
                      "scan_over_dense_rate": round(4.0 * Q * N * K * d / (t_topk * 1e-3) / 1e12 / dense_rate, 3),
                      "workspace_bytes": ws}), flush=True)


if __name__ == "__main__":
    main()
