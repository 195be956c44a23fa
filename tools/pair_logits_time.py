#!/usr/bin/env python3
"""usage: tools/pair_logits_time.py [--seconds S] [--workload squirrel] [--out FILE]  -> one JSON line: the probability and the
logit forms of the one-pass training scorer (dl_score_pairs_train / dl_score_pairs_train_logits) and of the forward scorer
(dl_score_pairs_fwd / dl_score_pairs_logits_fwd, no stored terms) at the benchmark's shape (the squirrel synthetic workload of
bench.build_workload, K = 8, d = 64, fp32 tables), interleaved in ONE process: HIP events, rounds that alternate between the four
candidates until each has run for S = 1 second in all after warm-up; the MEDIAN round counts, every round is listed.
EXPECTATION: the logit forms are no slower (the forward runs one expf and one division less per batch; the training step swaps
the sigmoid and its clamp factor for sigmoid_minus_label).
ACCEPTANCE (exit status 1 when missed): the logit form's median <= the probability form's WORST round of the same run, i.e. it
lies within the probability form's own round-to-round spread, or below it.
The line also says whether the two forward forms agree as prob == sigmoid(logit) to 2 ulp of 1 and whether the forward and the
training logits are the same bits."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from disenlink_amd import ops  # noqa: E402
from disenlink_amd.metrics import pair_bce_weights  # noqa: E402

K, D, T, BETA, REPS = 8, 64, 1.0, 0.5, 200


def interleaved(cands, seconds):
    """cands: {name: fn} -> {name: the rounds' mean times in ms} (a round = REPS calls: 20 to 70 ms here)."""
    for fn in cands.values():                                   # warm-up: workspaces, code objects, clocks
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    rounds = {n: [] for n in cands}
    while min(sum(v) * REPS for v in rounds.values()) < seconds * 1e3:
        for n, fn in cands.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(REPS):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            rounds[n].append(ev[0].elapsed_time(ev[1]) / REPS)
    return rounds


def main():
    arg = lambda k, dflt: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else dflt
    seconds, workload, out = float(arg("--seconds", "1.0")), arg("--workload", "squirrel"), arg("--out", None)
    dev = torch.device("cuda:0")
    _sg, _split, graph, pairs, _model, _x, Z = bench.build_workload(workload, dev, K, D, 512, elem_bytes=4)
    H = ops.aggregate_fwd(graph, Z, BETA, *ops.route_fwd(graph, Z, T))
    P = pairs.n_pairs
    y = (torch.rand(P, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) < 0.2).float()
    w = pair_bce_weights(P // 6, P - P // 6, 5, dev)
    cands = {
        "train_prob": lambda: ops.score_pairs_train(Z, H, pairs, T, y, w),
        "train_logit": lambda: ops.score_pairs_train_logits(Z, H, pairs, T, y, w),
        "fwd_prob": lambda: ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, T, pairs),
        "fwd_logit": lambda: ops.score_pairs_logits_fwd(Z, H, pairs.pu, pairs.pv, T, pairs),
    }
    prob, logit, train_logit = cands["fwd_prob"](), cands["fwd_logit"](), cands["train_logit"]()[0]
    if not bool(torch.isfinite(logit).all()):
        raise RuntimeError("non-finite logits")
    agree = float((prob - torch.sigmoid(logit)).abs().max())
    rounds = interleaved(cands, seconds)
    med = {n: statistics.median(v) for n, v in rounds.items()}
    verdict = {kind: bool(med[kind + "_logit"] <= max(rounds[kind + "_prob"])) for kind in ("train", "fwd")}
    line = {"workload": workload, "K": K, "d": D, "n_pairs": P, "hub_plan": pairs.hub is not None,
            "median_us": {n: round(1e3 * v, 2) for n, v in med.items()},
            "best_round_us": {n: round(1e3 * min(v), 2) for n, v in rounds.items()},
            "worst_round_us": {n: round(1e3 * max(v), 2) for n, v in rounds.items()},
            "rounds_us": {n: [round(1e3 * x, 2) for x in v] for n, v in rounds.items()}, "repetitions_per_round": REPS,
            "logit_over_prob": {kind: round(med[kind + "_logit"] / med[kind + "_prob"], 4) for kind in ("train", "fwd")},
            "logit_median_within_prob_spread_or_below": verdict,
            "max_abs_prob_minus_sigmoid_of_logit": agree, "prob_is_sigmoid_of_logit_to_2_ulp": bool(agree <= 2 * 2.0 ** -24),
            "train_logits_equal_forward_logits_bitwise": bool(torch.equal(train_logit, logit)),
            "measured": "HIP events, interleaved rounds in one process, median round, >= %.1f s per candidate after warm-up" % seconds}
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(text + "\n")
    return 0 if all(verdict.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
