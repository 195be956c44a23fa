#!/usr/bin/env python3
"""usage: tools/mine_time.py [--seconds S] [--skip-penn94]  -> one JSON line per (shape, m), appended to
profiles/mine_time.jsonl: (a) ops.score_mine (dl_score_mine), (b) the dense forward alone (ops.score_allpairs_fwd) and
(c) dense forward + exclusion mask + torch.topk of the strict upper triangle, the route there was before.  The three are
interleaved in one process, round after round, until each has run for at least S seconds (default 1) after a warm-up;
times are HIP events around each call, the median of the rounds.  Peak allocator memory of (a) and (c) is taken in
separate single calls ((a): ops.score_mine's allocations plus the workspace it holds).  (c) is skipped where it does not fit.  `scans` is the number of scans of the tile pairs that
ran in the last call (the histogram scans the device flag did not cut short, plus the emit scan), read from the
workspace word dl_score_mine_form points at.
Shapes: the bench graph (N = 5,201, K = 8, d = 64) and a Penn94-shaped seeded table (N = 41,554), m = 100 and 10,000;
the known pairs are 25 N seeded random edges."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disenlink_amd import _lib, ops, scans  # noqa: E402


def tables(N, K, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(N, K, d, device="cuda", generator=g) / d ** 0.5,
            torch.randn(N, K, d, device="cuda", generator=g) / d ** 0.5)


def once(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def interleaved(fns, seconds):
    """{name: [ms per call]}: rounds of one call each, in turn, until every candidate has run `seconds` in all"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    while any(sum(v) < seconds * 1e3 for v in times.values()):
        for k, fn in fns.items():
            times[k].append(once(fn))
    return times


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def scans_ran(ws, N, K, d, m):
    off = (-ws.data_ptr()) % 256 + _lib.score_mine_form(N, K, d, m)["scans_offset"]
    return int(ws[off:off + 4].view(torch.int32).item())


def shape(name, N, K, d, seed, seconds, out):
    Z, H = tables(N, K, d, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    rows = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    cols = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    ex = scans._unordered_exclusion_csr((rows, cols), N, Z.device)      # the CSR once, as a caller with a fixed graph would
    ptr = ex[0].to(torch.int64)
    ex_pairs = (torch.repeat_interleave(torch.arange(N, device="cuda"), ptr[1:] - ptr[:-1]), ex[1].to(torch.int64))
    for m in (100, 10000):
        lib = _lib.load()
        ws = ops._ws.get(int(lib.dl_score_mine_workspace_bytes(N, K, d, m)), Z.device)
        outs = [torch.empty(m, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
        count = torch.empty(1, dtype=torch.int64, device="cuda")

        def mine():                                                   # the library call itself: no host read, no allocation
            _lib.check(lib.dl_score_mine(Z.data_ptr(), H.data_ptr(), N, K, d, 1.0, ex[0].data_ptr(), ex[1].data_ptr(),
                                         float("-inf"), m, *[o.data_ptr() for o in outs], count.data_ptr(), ws.data_ptr(),
                                         ws.numel(), ops._stream()), "dl_score_mine")

        def dense():
            return ops.score_allpairs_fwd(Z, H, 1.0)

        def dense_topk():
            p = ops.score_allpairs_fwd(Z, H, 1.0)
            bad = torch.ones(N, N, dtype=torch.bool, device="cuda").tril_()
            bad[ex_pairs[0], ex_pairs[1]] = True
            p.masked_fill_(bad, -1.0)
            del bad
            v, i = torch.topk(p.view(-1), m)
            return torch.div(i, N, rounding_mode="floor"), i % N, v

        fns = {"mine": mine, "dense": dense, "dense_topk": dense_topk}
        try:
            peak_c = peak_of(dense_topk)
        except torch.OutOfMemoryError:
            peak_c = None
            del fns["dense_topk"]
            torch.cuda.empty_cache()
        peak_a = peak_of(lambda: ops.score_mine(Z, H, 1.0, m, exclude=ex_pairs)) + ws.numel()      # its workspace was there before
        t = {k: statistics.median(v) for k, v in interleaved(fns, seconds).items()}
        mine()
        torch.cuda.synchronize()
        rec = {"shape": name, "N": N, "K": K, "d": d, "m": m, "known_pairs": int(ex[1].numel()),
               "mine_ms": round(t["mine"], 3), "dense_ms": round(t["dense"], 3),
               "dense_topk_ms": round(t["dense_topk"], 3) if "dense_topk" in t else None,
               "mine_over_dense": round(t["mine"] / t["dense"], 3), "scans": scans_ran(ws, N, K, d, m), "count": int(count.item()),
               "mine_peak_bytes": peak_a, "dense_topk_peak_bytes": peak_c,
               "workspace_bytes": int(_lib.load().dl_score_mine_workspace_bytes(N, K, d, m))}
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as fh:
            fh.write(line + "\n")


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    out = os.path.join(ROOT, "profiles", "mine_time.jsonl")
    shape("bench", 5201, 8, 64, 0, seconds, out)
    if "--skip-penn94" not in sys.argv:
        shape("penn94_shaped", 41554, 8, 64, 1, seconds, out)


if __name__ == "__main__":
    main()
