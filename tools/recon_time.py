#!/usr/bin/env python3
"""usage: tools/recon_time.py [--seconds S] [--shapes bench,penn94] [--rows dense,bf16] [--out FILE]  -> JSON lines: the whole-graph
reconstruction loss (ops.score_recon_loss) against the dense [N,N] path, interleaved in ONE process (HIP events; rounds
that alternate between the candidates until each has run for S = 1 second in all after warm-up; the MEDIAN round counts):
  (a) score_recon_loss: loss, dZ, dH by strips, nothing of size N x N
  (b) the dense forward alone (ops.score_allpairs_fwd)
  (c) dense forward + whole-matrix weighted F.binary_cross_entropy + its gradient + ops.score_allpairs_bwd_dense
at the bench shape (N = 5,201, K = 8, d = 64) and a Penn94-shaped one (N = 41,554), on seeded tables and a seeded random
graph of ~16 edges per node with 2 N held-out pairs ignored.  Peak allocation of (a) and (c) is taken in a pass of its own
(torch.cuda.max_memory_allocated over a call that starts from an empty workspace and an empty cache, minus what was
resident before the call: tables and pair sets).
PREDICTION (no gate): (a) ~ 2 x (b) + the dense backward, from the product count — the scan cannot use the symmetry the
dense forward uses.  The line says "met" when (a) <= 1.1 x that sum, else "missed".
GATE (exit status 1): peak allocation of (a) <= dl_score_recon_workspace_bytes + outputs + the allocator's rounding (torch's
caching allocator rounds a block up to 512 bytes and hands out a whole fresh segment, a multiple of 2 MiB, when what would be
left of it is 1 MiB or less: 2 MiB for each of the workspace, dZ and dH, 512 bytes for each of loss and counts), and below
that of (c).  Any failing step ends the run there.
The bf16 row of a size (--rows bf16; tools/scan_bf16_time.py's comparison for the scans): the bf16 entry
(table_dtype=torch.bfloat16 on bf16 tensors) against the fp32 entry on the SAME rounded tables widened to fp32, interleaved
the same way; time (median, best and worst round, every round listed), peak allocation and workspace bytes of both, and
whether all four outputs have the same bits.  KEEP RULE (reported, no gate): worst bf16 round <= best fp32 round.
PREDICTION (no gate; a lower bound on the bf16 time, there being no timing-bound split of these kernels into matrix-core
time and the rest): fp32 time x 10 / 36, the ratio of the matrix-core products issued per (tile pair, factor, K block) —
scan Gram 2 of 12, backward Gram 2 of 12, second products 6 of 12; exp, epilogue, the weights' split3, the LDS images
and the G^ traffic are the same in both.  "met" when the bf16 median is within 1.1 x of it."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disenlink_amd import _dev, _lib, ops  # noqa: E402

SHAPES = {"bench": 5201, "penn94": 41554}
K, D, T = 8, 64, 1.0
ALLOCATOR_SLACK = 3 * (2 << 20) + 2 * 512


def interleaved(cands, seconds, reps):
    """cands: {name: fn} -> {name: (median ms of a round's mean, best, repetitions)}."""
    for fn in cands.values():                                   # warm-up: workspaces, LDS attributes, clocks
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rounds = {n: [] for n in cands}
    while min(sum(v) * reps[n] for n, v in rounds.items()) < seconds * 1e3:
        for n, fn in cands.items():
            if sum(rounds[n]) * reps[n] >= seconds * 1e3:
                continue
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps[n]):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            rounds[n].append(ev[0].elapsed_time(ev[1]) / reps[n])
    return {n: (statistics.median(v), min(v), len(v) * reps[n], v) for n, v in rounds.items()}


def problem(N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Z = torch.randn(N, K, D, device="cuda", generator=g) * 0.5 / D ** 0.5
    H = torch.randn(N, K, D, device="cuda", generator=g) * 0.5 / D ** 0.5
    n_edges, n_ign = 8 * N, 2 * N
    pos = tuple(torch.randint(0, N, (n_edges,), device="cuda", generator=g) for _ in range(2))
    ign = tuple(torch.randint(0, N, (n_ign,), device="cuda", generator=g) for _ in range(2))
    return Z, H, ops.recon_sets(pos, ign, N, Z.device)


def dense_masks(sets, N, w_pos, w_neg):
    """y and weight [N,N] fp32 of the same included pairs, over the upper triangle (built once, outside the timed region)."""
    def upper(rowptr, col):
        m = torch.zeros(N, N, dtype=torch.bool, device="cuda")
        if rowptr is not None:
            rows = torch.repeat_interleave(torch.arange(N, device="cuda"), (rowptr[1:] - rowptr[:-1]).long())
            m[rows, col.long()] = True
        return torch.triu(m, diagonal=1)
    pos = upper(sets.pos_rowptr, sets.pos_col)
    inc = torch.triu(torch.ones(N, N, dtype=torch.bool, device="cuda"), diagonal=1) & ~upper(sets.ign_rowptr, sets.ign_col)
    weight = torch.where(pos, w_pos, w_neg) * inc
    return pos.float(), weight.float()


def peak_of(fn):
    """bytes allocated at the peak of fn() above what was resident before it, from an empty workspace and cache"""
    _dev._ws.buf.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def run(name, N, seconds):
    Z, H, sets = problem(N, seed=N)
    w_pos, w_neg = ops.recon_weights(sets)
    y, weight = dense_masks(sets, N, w_pos, w_neg)

    def a():
        return ops.score_recon_loss(Z, H, T, sets)

    def b():
        return ops.score_allpairs_fwd(Z, H, T)

    def c():
        prob = ops.score_allpairs_fwd(Z, H, T).requires_grad_(True)
        loss = F.binary_cross_entropy(prob, y, weight=weight, reduction="sum")
        (g,) = torch.autograd.grad(loss, prob)
        return (loss,) + ops.score_allpairs_bwd_dense(Z, H, T, prob.detach(), g)

    def bwd_only(prob, g):
        return lambda: ops.score_allpairs_bwd_dense(Z, H, T, prob, g)

    la, dZa, dHa, counts = a()
    lc, dZc, dHc = c()
    for x in (la, dZa, dHa, lc, dZc, dHc):
        if not bool(torch.isfinite(x).all()):
            raise RuntimeError("non-finite result")
    ops.check_recon_counts(counts, sets)
    scale = max(float(dZc.abs().max()), float(dHc.abs().max()))
    diff = max(float((dZa - dZc).abs().max()), float((dHa - dHc).abs().max()))
    if not (diff <= 1e-4 * scale and abs(float(la) - float(lc.detach())) <= 1e-4 * abs(float(lc.detach()))):
        raise RuntimeError(f"the two paths disagree: gradients {diff} against scale {scale}, losses {float(la)} / {float(lc.detach())}")
    del la, dZa, dHa, lc, dZc, dHc
    prob = ops.score_allpairs_fwd(Z, H, T)
    g = torch.full((N, N), 1.0 / (N * N), device="cuda")
    big = N > 20000
    reps = {"a": 1 if big else 5, "b": 1 if big else 20, "c": 1 if big else 5, "dense_bwd": 1 if big else 5}
    r = interleaved({"a": a, "b": b, "c": c, "dense_bwd": bwd_only(prob, g)}, seconds, reps)
    del prob, g
    peak_c = peak_of(c)
    peak_a = peak_of(a)
    lib = _lib.load()
    ws = int(lib.dl_score_recon_workspace_bytes(N, K, D, 0))
    outputs = 2 * N * K * D * 4 + 8 + 16
    form = _lib.score_recon_form(N, K, D, 0)
    predicted = 2 * r["b"][0] + r["dense_bwd"][0]
    gate = peak_a <= ws + outputs + ALLOCATOR_SLACK and peak_a < peak_c
    line = {"shape": name, "N": N, "K": K, "d": D, "n_pos": sets.n_pos, "n_neg": sets.n_neg, "n_ignored": sets.n_ignored,
            "strips": form["strips"], "block_rows": form["block_rows"],
            "a_recon_ms": round(r["a"][0], 4), "b_dense_fwd_ms": round(r["b"][0], 4), "c_dense_fwd_bce_bwd_ms": round(r["c"][0], 4),
            "dense_bwd_ms": round(r["dense_bwd"][0], 4), "a_over_c": round(r["a"][0] / r["c"][0], 3),
            "predicted_a_ms": round(predicted, 4), "a_over_predicted": round(r["a"][0] / predicted, 3),
            "prediction": "met" if r["a"][0] <= 1.1 * predicted else "missed",
            "best_round_ms": {n: round(v[1], 4) for n, v in r.items()}, "repetitions": {n: v[2] for n, v in r.items()},
            "peak_bytes_a": peak_a, "peak_bytes_c": peak_c, "workspace_bytes_a": ws, "output_bytes_a": outputs, "allocator_slack_bytes": ALLOCATOR_SLACK,
            "max_abs_gradient_difference_over_scale": diff / scale, "gate_peak_allocation": bool(gate),
            "measured": "HIP events, interleaved rounds in one process, median round, >= %.1f s per candidate after warm-up; "
                        "peaks from torch.cuda.max_memory_allocated in a pass of their own" % seconds}
    return line, gate


def run_bf16(name, N, seconds):
    Z, H, sets = problem(N, seed=N)
    Zb, Hb = Z.to(torch.bfloat16), H.to(torch.bfloat16)
    Zf, Hf = Zb.float(), Hb.float()
    del Z, H

    def f32():
        return ops.score_recon_loss(Zf, Hf, T, sets)

    def bf16():
        return ops.score_recon_loss(Zb, Hb, T, sets, table_dtype=torch.bfloat16)

    want, got = f32(), bf16()
    ops.check_recon_counts(got[3], sets)
    if not all(bool(torch.isfinite(x).all()) for x in want[:3]):
        raise RuntimeError("non-finite result")
    same = all(torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32 if a.dtype == torch.float32 else a.dtype),
                           b.view(torch.int64 if b.dtype == torch.float64 else torch.int32 if b.dtype == torch.float32 else b.dtype))
               for a, b in zip(want, got))
    del want, got
    reps = {"f32": 1 if N > 20000 else 5, "bf16": 1 if N > 20000 else 5}
    r = interleaved({"f32": f32, "bf16": bf16}, seconds, reps)
    peak = {"f32": peak_of(f32), "bf16": peak_of(bf16)}
    lib = _lib.load()
    ws = {"f32": int(lib.dl_score_recon_workspace_bytes_dtype(N, K, D, _lib.DL_F32, 0)),
          "bf16": int(lib.dl_score_recon_workspace_bytes_dtype(N, K, D, _lib.DL_BF16, 0))}
    Np, dp = -(-N // 128) * 128, -(-D // 32) * 32
    predicted = r["f32"][0] * 10 / 36
    line = {"row": "bf16", "shape": name, "N": N, "K": K, "d": D, "n_pos": sets.n_pos, "n_neg": sets.n_neg, "n_ignored": sets.n_ignored,
            "f32_ms": round(r["f32"][0], 4), "bf16_ms": round(r["bf16"][0], 4), "bf16_over_f32": round(r["bf16"][0] / r["f32"][0], 3),
            "best_round_ms": {n: round(v[1], 4) for n, v in r.items()}, "worst_round_ms": {n: round(max(v[3]), 4) for n, v in r.items()},
            "rounds_ms": {n: [round(x, 4) for x in v[3]] for n, v in r.items()}, "repetitions_per_round": reps,
            "keep_rule_worst_bf16_le_best_f32": bool(max(r["bf16"][3]) <= r["f32"][1]),
            "predicted_lower_bound_bf16_ms": round(predicted, 4), "bf16_over_predicted": round(r["bf16"][0] / predicted, 3),
            "prediction": "met" if r["bf16"][0] <= 1.1 * predicted else "missed",
            "peak_bytes": peak, "workspace_bytes": ws, "workspace_difference": ws["f32"] - ws["bf16"],
            "workspace_difference_is_16_K_Np_dp": ws["f32"] - ws["bf16"] == 16 * K * Np * dp, "same_bits": bool(same),
            "measured": "HIP events, interleaved rounds in one process, >= %.1f s per candidate after warm-up; peaks from "
                        "torch.cuda.max_memory_allocated in a pass of their own" % seconds}
    return line, bool(same)


def main():
    arg = lambda k, dflt: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else dflt
    seconds = float(arg("--seconds", "1.0"))
    out = arg("--out", None)
    ok = True
    rows = arg("--rows", "dense,bf16").split(",")
    for name in arg("--shapes", "bench,penn94").split(","):
        for row, fn in (("dense", run), ("bf16", run_bf16)):
            if row not in rows:
                continue
            line, gate = fn(name, SHAPES[name], seconds)
            text = json.dumps(line)
            print(text, flush=True)
            if out:
                with open(out, "a") as fh:
                    fh.write(text + "\n")
            ok = ok and gate
            _dev._ws.buf.clear()
            torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
