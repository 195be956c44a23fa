#!/usr/bin/env python3
"""usage: tools/pair_rank_time.py [--seconds S] [--skip-penn94] [--skip-dense-sort]  -> one JSON line per shape, appended
to profiles/pair_rank_time.jsonl: (a) ops.score_pair_ranks (one target pass, the torch sort, ONE counting scan, the suffix
sums; the exclusion set prepared once with ops.pair_exclusion, as a caller with a fixed graph would), (b) the dense forward
alone (ops.score_allpairs_fwd) and (c) dense forward + upper-triangle / exclusion mask + torch.sort + searchsorted, the
[N,N] route.  `scan` is the counting scan alone (dl_score_pair_ranks on sorted keys).  The candidates are interleaved in one
process, round after round, until each has run for at least S seconds (default 1) after a warm-up; times are HIP events
around each call, the median of the rounds.  Peak allocator memory of (a) and (c) is taken in separate single calls ((a):
its allocations plus the workspace it holds).  (c) is skipped where it does not fit.  `count_ok`: the candidates the device
counted equal N (N - 1) / 2 - excluded pairs.  `scan_floor` is the same counting scan with target keys above every
candidate (all +inf): every candidate is scored, masked and counted, none searches or adds, so scan - scan_floor is the
measured cost of the search and the adds together.  Exit status 1 if the device's count is wrong or the peak memory of (a) is
not below that of (c) where (c) ran: the one gate.
Shapes: the bench graph (N = 5,201, K = 8, d = 64; targets = the test positives of the seeded squirrel split, exclusion =
every dataset edge) and a Penn94-shaped seeded table (N = 41,554; 100,000 seeded targets, 25 N seeded known pairs)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disenlink_amd import _lib, ops, scans  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mine_time import interleaved, peak_of, tables  # noqa: E402


def shape(name, N, K, d, seed, src, dst, known, seconds, out, dense_sort=True):
    Z, H = tables(N, K, d, seed)
    ex = ops.pair_exclusion(known, N, Z.device)
    ptr = ex.rowptr.to(torch.int64)
    ex_pairs = (torch.repeat_interleave(torch.arange(N, device="cuda"), ptr[1:] - ptr[:-1]), ex.col.to(torch.int64))
    lo, hi = torch.minimum(src, dst), torch.maximum(src, dst)
    T = int(src.numel())
    lib = _lib.load()
    tord = torch.sort(scans._order_keys(ops.score_pair_logits(Z, H, 1.0, lo, hi))).values
    tord = torch.where(tord >= 0x80000000, tord - 0x100000000, tord).to(torch.int32).contiguous()
    cnt = torch.empty(2 * (T + 1) + 1, dtype=torch.int64, device="cuda")
    ws = ops._ws.get(int(lib.dl_score_pair_ranks_workspace_bytes(N, K, d)), Z.device)

    def ranks():
        return ops.score_pair_ranks_counted(Z, H, 1.0, src, dst, exclude=ex)

    def scan():                                                       # the library call itself
        _lib.check(lib.dl_score_pair_ranks(Z.data_ptr(), H.data_ptr(), N, K, d, 1.0, ex.rowptr.data_ptr(), ex.col.data_ptr(),
                                           tord.data_ptr(), T, cnt.data_ptr(), cnt[T + 1:].data_ptr(), cnt[2 * T + 2:].data_ptr(),
                                           ws.data_ptr(), ws.numel(), ops._stream()), "dl_score_pair_ranks")

    def dense():
        return ops.score_allpairs_fwd(Z, H, 1.0)

    def dense_sort_route():
        p = ops.score_allpairs_fwd(Z, H, 1.0)
        tp = p[lo, hi]
        bad = torch.ones(N, N, dtype=torch.bool, device="cuda").tril_()
        bad[ex_pairs[0], ex_pairs[1]] = True
        vals = p[~bad]
        del bad, p
        vals = torch.sort(vals).values
        below = torch.searchsorted(vals, tp, right=False)
        upto = torch.searchsorted(vals, tp, right=True)
        return vals.numel() - upto, upto - below

    top = torch.full((T,), 0xFF800000 - 0x100000000, dtype=torch.int32, device="cuda")      # the key of +inf

    def scan_floor():                                                 # no candidate reaches a target: the scan without its epilogue's work
        _lib.check(lib.dl_score_pair_ranks(Z.data_ptr(), H.data_ptr(), N, K, d, 1.0, ex.rowptr.data_ptr(), ex.col.data_ptr(),
                                           top.data_ptr(), T, cnt.data_ptr(), cnt[T + 1:].data_ptr(), cnt[2 * T + 2:].data_ptr(),
                                           ws.data_ptr(), ws.numel(), ops._stream()), "dl_score_pair_ranks")

    fns = {"ranks": ranks, "scan": scan, "scan_floor": scan_floor, "dense": dense}
    peak_c = None
    if dense_sort:
        try:
            peak_c = peak_of(dense_sort_route)
            fns["dense_sort"] = dense_sort_route
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
    peak_a = peak_of(ranks) + ws.numel()                              # its workspace was there before
    t = {k: statistics.median(v) for k, v in interleaved(fns, seconds).items()}
    counted = int(ranks()[4])
    want = N * (N - 1) // 2 - int(ex.n_pairs)
    form = _lib.score_pair_ranks_form(N, K, d, T)
    rec = {"shape": name, "N": N, "K": K, "d": d, "targets": T, "excluded_pairs": int(ex.n_pairs),
           "ranks_ms": round(t["ranks"], 3), "scan_ms": round(t["scan"], 3), "scan_floor_ms": round(t["scan_floor"], 3),
           "dense_ms": round(t["dense"], 3),
           "dense_sort_ms": round(t["dense_sort"], 3) if "dense_sort" in t else None,
           "ranks_over_dense": round(t["ranks"] / t["dense"], 3), "scan_over_dense": round(t["scan"] / t["dense"], 3),
           "scan_floor_over_dense": round(t["scan_floor"] / t["dense"], 3),
           "one_scan_met": bool(t["ranks"] <= 1.1 * t["dense"]),
           "faster_than_dense_sort": bool(t["ranks"] < t["dense_sort"]) if "dense_sort" in t else None,
           "ranks_peak_bytes": peak_a, "dense_sort_peak_bytes": peak_c,
           "peak_below_dense_sort": bool(peak_a < peak_c) if peak_c is not None else None,
           "candidates_counted": counted, "count_ok": counted == want,
           "lds_levels": form["lds_levels"], "global_levels": form["global_levels"], "grid": form["grid"]}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")
    return rec["count_ok"] and rec["peak_below_dense_sort"] is not False


def bench_targets():
    """the test positives and every edge (both directions) of the seeded synthetic squirrel graph of bench.py"""
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.splits import make_link_split
    sg = synthetic_graph("squirrel", seed=0)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=0)
    pos = split.test.label > 0.5
    src = torch.from_numpy(np.ascontiguousarray(split.test.u[pos])).cuda().long()
    dst = torch.from_numpy(np.ascontiguousarray(split.test.v[pos])).cuda().long()
    src, dst = src[src != dst], dst[src != dst]                      # a self loop is no pair
    s, t = torch.from_numpy(np.asarray(sg.src)).long().cuda(), torch.from_numpy(np.asarray(sg.dst)).long().cuda()
    return sg.n_nodes, src, dst, (torch.cat([s, t]), torch.cat([t, s]))


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = os.path.join(ROOT, "profiles", "pair_rank_time.jsonl")
    dense_sort = "--skip-dense-sort" not in sys.argv
    N, src, dst, known = bench_targets()
    ok = shape("bench", N, 8, 64, 0, src, dst, known, seconds, out, dense_sort)
    if "--skip-penn94" not in sys.argv:
        N = 41554
        g = torch.Generator(device="cuda").manual_seed(101)
        src = torch.randint(0, N, (100000,), device="cuda", generator=g)
        dst = (src + 1 + torch.randint(0, N - 1, (100000,), device="cuda", generator=g)) % N
        known = (torch.randint(0, N, (25 * N,), device="cuda", generator=g), torch.randint(0, N, (25 * N,), device="cuda", generator=g))
        ok = shape("penn94_shaped", N, 8, 64, 1, src, dst, known, seconds, out, dense_sort) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
