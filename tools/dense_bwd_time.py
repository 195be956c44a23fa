#!/usr/bin/env python3
"""usage: tools/dense_bwd_time.py [--seconds S]  -> JSON lines: the dense backward of link_pred (ops.score_allpairs_bwd_dense)
against the dense forward and the pair-plan backward, interleaved in ONE process (HIP events; every candidate is
repeated for at least S = 1 second in all after warm-up, in rounds that alternate between the candidates).
  squirrel shape (N = 5,201, K = 8, d = 64, seeded tables):
    (a) dense forward  (b) dense backward, whole-matrix gradient
    (c) pair-plan backward on the declared support of the real squirrel train masks (tests/golden/real_squirrel.npz)
  whole-matrix gradient at N = 2,048, K = 8, d = 64:
    (d) pair-plan backward on an all-ones plan (the plan build is not timed) against the dense backward.
GATE: in (d) the dense backward must not be slower than the plan backward; the exit status is 1 otherwise.  Any failing
step (a call that raises, a non-finite result) ends the run there."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disenlink_amd import ops  # noqa: E402
from disenlink_amd.splits import make_link_split  # noqa: E402


def interleaved(cands, seconds, reps):
    """cands: {name: fn}.  -> {name: (mean ms, best round's mean ms, repetitions)}; rounds of reps[name] calls per candidate,
    alternating, until every candidate has run for `seconds` in all."""
    for fn in cands.values():                                   # warm-up: workspaces, LDS attributes, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    total = {n: 0.0 for n in cands}
    count = {n: 0 for n in cands}
    best = {n: float("inf") for n in cands}
    while min(total.values()) < seconds * 1e3:
        for n, fn in cands.items():
            if total[n] >= seconds * 1e3:
                continue
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps[n]):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            total[n] += ms
            count[n] += reps[n]
            best[n] = min(best[n], ms / reps[n])
    return {n: (total[n] / count[n], best[n], count[n]) for n in cands}


def tables(N, K, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(N, K, d, device="cuda", generator=g) / d ** 0.5,
            torch.randn(N, K, d, device="cuda", generator=g) / d ** 0.5)


def finite(*ts):
    for t in ts:
        if not bool(torch.isfinite(t).all()):
            raise RuntimeError("non-finite result")


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    dev = torch.device("cuda", torch.cuda.current_device())
    K, d, t = 8, 64, 1.0
    note = "HIP events, interleaved rounds in one process, >= %.1f s of repetitions per candidate after warm-up" % seconds

    # ---- squirrel shape: (a) forward, (b) dense backward, (c) plan backward on the real train masks
    g = np.load(os.path.join(ROOT, "tests", "golden", "real_squirrel.npz"))
    m = json.loads(str(g["meta"]))
    edges = g["edges"].astype(np.int64)
    N = int(m["N"])
    split = make_link_split(edges[:, 0], edges[:, 1], N, m=m["m"], seed=m["split_seed"])
    cache = ops.DensePairPlanCache()
    cache.set_pairs(N, dev, (split.pos_train.u, split.pos_train.v), (split.neg_train.u, split.neg_train.v))
    n_plan = int(cache.flat.numel())
    Z, H = tables(N, K, d, 0)
    prob = ops.score_allpairs_fwd(Z, H, t)
    gen = torch.Generator(device="cuda").manual_seed(1)
    g_full = torch.randn(N, N, device="cuda", generator=gen) / (N * N)
    mask = torch.zeros(N * N, device="cuda")
    mask[cache.flat] = 1.0
    g_mask = g_full * mask.view(N, N)
    finite(*ops.score_allpairs_bwd_dense(Z, H, t, prob, g_full), *ops.score_allpairs_bwd(Z, H, cache.pairs, t, prob, g_mask))
    r = interleaved({"fwd": lambda: ops.score_allpairs_fwd(Z, H, t),
                     "dense_bwd": lambda: ops.score_allpairs_bwd_dense(Z, H, t, prob, g_full),
                     "plan_bwd_masks": lambda: ops.score_allpairs_bwd(Z, H, cache.pairs, t, prob, g_mask)},
                    seconds, {"fwd": 100, "dense_bwd": 25, "plan_bwd_masks": 25})
    nt = (N + 127) // 128
    flop_bwd = 8.0 * (nt * 128) ** 2 * K * d                  # two Gram products + two weight products per tile, all tiles
    print(json.dumps({"shape": "squirrel", "N": N, "K": K, "d": d, "plan_pairs": n_plan,
                      "a_dense_fwd_ms": round(r["fwd"][0], 4), "b_dense_bwd_ms": round(r["dense_bwd"][0], 4),
                      "c_plan_bwd_train_masks_ms": round(r["plan_bwd_masks"][0], 4),
                      "best_round_ms": {n: round(v[1], 4) for n, v in r.items()}, "repetitions": {n: v[2] for n, v in r.items()},
                      "b_over_a": round(r["dense_bwd"][0] / r["fwd"][0], 3),
                      "b_over_c": round(r["dense_bwd"][0] / r["plan_bwd_masks"][0], 3),
                      "dense_bwd_tflops": round(flop_bwd / (r["dense_bwd"][0] * 1e-3) / 1e12, 1),
                      "workspace_bytes": int(ops._lib.load().dl_score_allpairs_bwd_dense_workspace_bytes(N, K, d)),
                      "measured": note}), flush=True)
    del Z, H, prob, g_full, g_mask, mask, cache

    # ---- (d) whole-matrix gradient at N = 2048: plan on an all-ones mask against dense
    N = 2048
    Z, H = tables(N, K, d, 2)
    prob = ops.score_allpairs_fwd(Z, H, t)
    g_full = torch.randn(N, N, device="cuda", generator=gen) / (N * N)
    cache = ops.DensePairPlanCache()
    cache.set_pairs(N, dev, torch.ones(N, N, device="cuda"))  # built here, outside the timed region
    a, b = ops.score_allpairs_bwd_dense(Z, H, t, prob, g_full), ops.score_allpairs_bwd(Z, H, cache.pairs, t, prob, g_full)
    finite(*a, *b)
    scale = max(float(b[0].abs().max()), float(b[1].abs().max()))
    diff = max(float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()))
    if not diff <= 1e-4 * scale:
        raise RuntimeError(f"dense and plan backwards disagree: {diff} against scale {scale}")
    r = interleaved({"dense_bwd": lambda: ops.score_allpairs_bwd_dense(Z, H, t, prob, g_full),
                     "plan_bwd_all": lambda: ops.score_allpairs_bwd(Z, H, cache.pairs, t, prob, g_full)},
                    seconds, {"dense_bwd": 50, "plan_bwd_all": 5})
    ok = r["dense_bwd"][0] <= r["plan_bwd_all"][0]
    print(json.dumps({"shape": "whole-matrix gradient", "N": N, "K": K, "d": d, "plan_pairs": int(cache.flat.numel()),
                      "d_dense_bwd_ms": round(r["dense_bwd"][0], 4), "d_plan_bwd_all_ones_ms": round(r["plan_bwd_all"][0], 4),
                      "best_round_ms": {n: round(v[1], 4) for n, v in r.items()}, "repetitions": {n: v[2] for n, v in r.items()},
                      "plan_over_dense": round(r["plan_bwd_all"][0] / r["dense_bwd"][0], 2),
                      "max_abs_difference_over_scale": diff / scale,
                      "gate_dense_not_slower_than_plan": bool(ok), "measured": note}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
