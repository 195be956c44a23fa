#!/usr/bin/env python3
"""usage: tools/recon_logits_time.py [--seconds S] [--out FILE]  -> JSON lines: the logit-space entries against the probability
entries they stand beside, interleaved in ONE process (HIP events; rounds that alternate between the candidates until each has
run for S = 1 second in all after warm-up; the MEDIAN round counts; every round is listed), at the bench shape (N = 5,201,
K = 8, d = 64) on tools/recon_time.py's seeded tables and pair sets:
  row "recon f32":   ops.score_recon_loss against ops.score_recon_logits_loss on fp32 tables
  row "recon bf16":  the same on bf16 tables (table_dtype=torch.bfloat16)
  row "dense fwd":   ops.score_allpairs_fwd against ops.score_allpairs_logits_fwd
The yardstick is the probability entry in the same process: its kernels are not under test.  Each pair issues the same
matrix-core products and differs in the epilogue only (sigmoid_ref + logf against expf + a hardware reciprocal + log1pf per
value; the dense forward: no sigmoid at all), so the EXPECTATION (reported, no gate, no number fixed in advance) is that the
logit entry's median lies within the probability entry's own round-to-round span of the run: "inside" / "outside", and by
how much of the probability entry's median when outside."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disenlink_amd import ops  # noqa: E402
from recon_time import K, D, T, SHAPES, interleaved, problem  # noqa: E402


def row(name, prob_fn, logit_fn, seconds, reps):
    r = interleaved({"prob": prob_fn, "logit": logit_fn}, seconds, {"prob": reps, "logit": reps})
    lo, hi = min(r["prob"][3]), max(r["prob"][3])
    med = r["logit"][0]
    inside = lo <= med <= hi
    return {"row": name, "N": SHAPES["bench"], "K": K, "d": D,
            "prob_ms": round(r["prob"][0], 4), "logit_ms": round(med, 4), "logit_over_prob": round(med / r["prob"][0], 4),
            "prob_span_ms": [round(lo, 4), round(hi, 4)], "logit_median_in_prob_span": "inside" if inside else "outside",
            "outside_by_of_prob_median": 0.0 if inside else round((med - hi if med > hi else med - lo) / r["prob"][0], 4),
            "rounds_ms": {n: [round(x, 4) for x in v[3]] for n, v in r.items()}, "repetitions_per_round": reps,
            "measured": "HIP events, interleaved rounds in one process, median round, >= %.1f s per candidate after warm-up" % seconds}


def main():
    arg = lambda k, dflt: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else dflt
    seconds = float(arg("--seconds", "1.0"))
    out = arg("--out", None)
    N = SHAPES["bench"]
    Z, H, sets = problem(N, seed=N)
    Zb, Hb = Z.to(torch.bfloat16), H.to(torch.bfloat16)
    rows = (
        ("recon f32", lambda: ops.score_recon_loss(Z, H, T, sets), lambda: ops.score_recon_logits_loss(Z, H, T, sets), 5),
        ("recon bf16", lambda: ops.score_recon_loss(Zb, Hb, T, sets, table_dtype=torch.bfloat16),
         lambda: ops.score_recon_logits_loss(Zb, Hb, T, sets, table_dtype=torch.bfloat16), 5),
        ("dense fwd", lambda: ops.score_allpairs_fwd(Z, H, T), lambda: ops.score_allpairs_logits_fwd(Z, H, T), 20),
    )
    for name, p, l, reps in rows:
        a, b = p(), l()
        if name.startswith("recon"):
            ops.check_recon_counts(b[3], sets)
            # nothing saturates on these tables: the two objectives are the same function there (1e-4, the module tolerance)
            if not (abs(float(a[0]) - float(b[0])) <= 1e-4 * abs(float(a[0])) and bool(torch.isfinite(b[1]).all())
                    and float((a[2] - b[2]).abs().max()) <= 1e-4 * float(a[2].abs().max())):
                raise RuntimeError(f"{name}: the two entries disagree on unsaturated tables")
        elif not float((torch.sigmoid(b.double()) - a.double()).abs().max()) <= 3e-7:
            raise RuntimeError("dense fwd: sigmoid(logit) is not the probability entry's output")
        del a, b
        text = json.dumps(row(name, p, l, seconds, reps))
        print(text, flush=True)
        if out:
            with open(out, "a") as fh:
                fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
