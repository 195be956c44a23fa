#!/usr/bin/env python3
"""usage: tools/recon_filter_time.py [--seconds S] [--shapes bench,penn94] [--out FILE]  -> JSON lines: the whole-graph
reconstruction loss under a node-group rule (ops.score_recon_loss on sets prepared with ``node_filter``;
dl_score_recon_filtered) against the call without a rule, interleaved in ONE process (tools/recon_time.py's method: HIP
events, rounds that alternate between the candidates until each has run for S = 1 second in all after warm-up; the MEDIAN
round counts), with the rule ``NodeFilter.between`` on the two halves of the nodes (a balanced users x items graph):
  (a) the unfiltered call                         every pair outside ``ignore`` is charged
  (b) the filtered call                           only user-item pairs are charged
  (c) the only way without the rule on the loss   the unfiltered call with every denied pair listed in ``ignore``
at the bench shape (N = 5,201, K = 8, d = 64) and a Penn94-shaped one (N = 41,554), on tools/recon_time.py's seeded tables
and random graph.  (c) is built at N = 5,201 only; at 41,554 the line reports the bytes its ignored CSR would take
(int32 rowptr [N + 1] and both orientations of every denied pair) instead of building it.  Peak allocation of each candidate
is taken in a pass of its own (torch.cuda.max_memory_allocated over a call that starts from an empty workspace and an
empty cache, minus what was resident before the call: the tables and the candidate's own prepared sets), and the bytes of
the prepared sets are reported beside it.
EXPECTATION (no gate): (b) is at (a) — the rule costs one mask word per thread and candidate tile, and no tile is skipped —
within the +-3-5 % box spread the project quotes for such pairs; (b) is below (c) in time and far below it in resident bytes.
The line says "met" when |b / a - 1| <= 0.05 and, where (c) was built, b <= c.
GATE (exit status 1): (b) and (c) return the same bits (loss, dZ, dH, counts), and the counts of (b) are the host's."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disenlink_amd import _dev, ops  # noqa: E402
from recon_time import D, K, SHAPES, T, interleaved, peak_of  # noqa: E402

LIST_MAX_N = 8192            # (c) is built up to here: its ignored CSR is of order N^2


def raw_sets(N, seed):
    """tools/recon_time.py's problem with the raw pair lists kept: tables, positives, ignored pairs."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    Z = torch.randn(N, K, D, device="cuda", generator=g) * 0.5 / D ** 0.5
    H = torch.randn(N, K, D, device="cuda", generator=g) * 0.5 / D ** 0.5
    pos = tuple(torch.randint(0, N, (8 * N,), device="cuda", generator=g) for _ in range(2))
    ign = tuple(torch.randint(0, N, (2 * N,), device="cuda", generator=g) for _ in range(2))
    return Z, H, pos, ign


def sets_bytes(sets):
    return sum(x.numel() * x.element_size() for x in (sets.pos_rowptr, sets.pos_col, sets.ign_rowptr, sets.ign_col) if x is not None)


def same_bits(a, b):
    view = lambda x: x.view(torch.int64 if x.dtype == torch.float64 else torch.int32 if x.dtype == torch.float32 else x.dtype)
    return all(torch.equal(view(x), view(y)) for x, y in zip(a, b))


def run(name, N, seconds):
    Z, H, pos, ign = raw_sets(N, seed=N)
    users = torch.arange(N, device="cuda") < N // 2
    nf = ops.NodeFilter.between(users, ~users, device="cuda")
    plain = ops.recon_sets(pos, ign, N, Z.device)
    ruled = ops.recon_sets(pos, ign, N, Z.device, node_filter=nf)
    n_denied = (N // 2) * (N // 2 - 1) // 2 + (N - N // 2) * (N - N // 2 - 1) // 2
    cands = {"a": lambda: ops.score_recon_loss(Z, H, T, plain), "b": lambda: ops.score_recon_loss(Z, H, T, ruled)}
    listed = None
    if N <= LIST_MAX_N:
        same_side = users[:, None] == users[None, :]
        iu, iv = ign
        same_side[iu, iv] = True
        same_side[iv, iu] = True
        listed = ops.recon_sets(pos, same_side, N, Z.device)
        del same_side
        cands["c"] = lambda: ops.score_recon_loss(Z, H, T, listed)
    out = {n: fn() for n, fn in cands.items()}
    ops.check_recon_counts(out["b"][3], ruled)
    ok = all(bool(torch.isfinite(x).all()) for o in out.values() for x in o[:3])
    bits = None
    if listed is not None:
        bits = same_bits(out["b"], out["c"]) and (listed.n_pos, listed.n_neg) == (ruled.n_pos, ruled.n_neg)
        ok = ok and bits
    del out
    reps = {n: 1 if N > 20000 else 5 for n in cands}
    r = interleaved(cands, seconds, reps)
    peak = {n: peak_of(fn) for n, fn in cands.items()}
    resident = {"a": sets_bytes(plain), "b": sets_bytes(ruled) + N + 8 * nf.n_groups}
    if listed is not None:
        resident["c"] = sets_bytes(listed)
    met = abs(r["b"][0] / r["a"][0] - 1.0) <= 0.05 and (listed is None or r["b"][0] <= r["c"][0])
    line = {"shape": name, "N": N, "K": K, "d": D, "rule": "between, two halves",
            "counts": {"a": [plain.n_pos, plain.n_neg, plain.n_ignored], "b": [ruled.n_pos, ruled.n_neg, ruled.n_ignored]},
            "denied_pairs": n_denied, "listed_ignore_csr_bytes": 4 * (N + 1) + 8 * (n_denied + ruled.n_ignored),
            "ms": {n: round(v[0], 4) for n, v in r.items()}, "b_over_a": round(r["b"][0] / r["a"][0], 4),
            "b_over_c": round(r["b"][0] / r["c"][0], 4) if "c" in r else None,
            "best_round_ms": {n: round(v[1], 4) for n, v in r.items()}, "worst_round_ms": {n: round(max(v[3]), 4) for n, v in r.items()},
            "repetitions": {n: v[2] for n, v in r.items()}, "peak_bytes_of_the_call": peak, "prepared_set_bytes": resident,
            "b_and_c_same_bits": bits, "expectation": "met" if met else "missed",
            "measured": "HIP events, interleaved rounds in one process, median round, >= %.1f s per candidate after warm-up; "
                        "peaks from torch.cuda.max_memory_allocated in a pass of their own" % seconds}
    return line, bool(ok)


def main():
    arg = lambda k, dflt: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else dflt
    seconds = float(arg("--seconds", "1.0"))
    out = arg("--out", None)
    ok = True
    for name in arg("--shapes", "bench,penn94").split(","):
        line, gate = run(name, SHAPES[name], seconds)
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
