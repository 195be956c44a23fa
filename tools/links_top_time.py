#!/usr/bin/env python3
"""usage: tools/links_top_time.py [--seconds S] [--skip-penn94]  -> one JSON line per (shape, M), appended to
profiles/links_top_time.jsonl: the budgeted link graph (a) dl_score_links_top_count_dtype + dl_score_links_top_fill_dtype
at M links against (p) dl_score_links_count + dl_score_links_fill at the floor that yields the same links (the M-th logit:
what a caller pays who already knew the threshold) and (c) dense forward + mask + torch.topk of the upper triangle, the
route without the scans, where it fits.
The candidates are interleaved in one process, round after round, until each has run for at least S seconds (default 1)
after a warm-up; times are HIP events around each call, the median of the rounds (the conventions of tools/links_time.py,
whose shapes, tables and known pairs these are: the bench graph N = 5,201, K = 8, d = 64 and a Penn94-shaped seeded table
N = 41,554, 25 N seeded random edges as known pairs).  M: the link counts tools/links_time.py reports at these shapes.
The library calls run on preallocated arrays (no host read, no allocation); `top_op_ms` is ops.score_top_links as a user
calls it with a prepared ops.pair_exclusion, the read of rowptr[N] and the allocations included.  `hist_scans` is the number
of histogram scans that ran (State::scans in the workspace), `scans` that plus count and fill; `expected_ratio` =
(scans) / 2, what (a) / (p) would be if every scan cost the same.
Exit status 1 if (a) does not hold exactly M links, if (p) at the M-th logit differs from (a) by anything but the ties of
that logit which the budget cuts off, if more than six histogram scans ran, or if the peak allocator memory of
ops.score_top_links exceeds that of ops.score_links at the same result size by more than the extra workspace (the
selection state and the histogram, in the allocator's 512-byte blocks).  The times gate nothing."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disenlink_amd import _lib, ops, scans  # noqa: E402
from mine_time import interleaved, peak_of, tables  # noqa: E402

F32 = _lib.DL_F32


def shape(name, N, K, d, seed, budgets, seconds, out):
    lib = _lib.load()
    Z, H = tables(N, K, d, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    rows = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    cols = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    prepared = scans.pair_exclusion((rows, cols), N, Z.device)          # once, as a caller with a fixed graph would
    ptr = prepared.rowptr.to(torch.int64)
    ex_pairs = (torch.repeat_interleave(torch.arange(N, device="cuda"), ptr[1:] - ptr[:-1]), prepared.col.to(torch.int64))
    form = _lib.score_links_top_form(N, K, d)
    ws_top_bytes = int(lib.dl_score_links_top_workspace_bytes_dtype(N, K, d, F32))
    ws_links_bytes = int(lib.dl_score_links_workspace_bytes(N, K, d))
    ok = True
    for M in budgets:
        ws = torch.empty(ws_top_bytes, dtype=torch.uint8, device="cuda")
        rowptr = torch.empty(N + 1, dtype=torch.int64, device="cuda")
        head = (Z.data_ptr(), H.data_ptr(), N, K, d, F32, 1.0, prepared.rowptr.data_ptr(), prepared.col.data_ptr(), float("-inf"),
                M, None, ws.data_ptr(), ws.numel(), rowptr.data_ptr())

        def top_count():
            _lib.check(lib.dl_score_links_top_count_dtype(*head, ops._stream()), "dl_score_links_top_count_dtype")

        top_count()
        nnz = int(rowptr[-1].item())
        off = (-ws.data_ptr()) % 256 + form["scans_offset"]
        hist_scans = int(ws[off:off + 4].view(torch.int32).item())
        col = torch.empty(nnz, dtype=torch.int32, device="cuda")
        logit = torch.empty(nnz, dtype=torch.float32, device="cuda")
        prob = torch.empty(nnz, dtype=torch.float32, device="cuda")

        def top_fill():
            _lib.check(lib.dl_score_links_top_fill_dtype(*head, nnz, col.data_ptr(), logit.data_ptr(), prob.data_ptr(), ops._stream()),
                       "dl_score_links_top_fill_dtype")

        top_fill()
        floor = float(logit.min()) if nnz else float("inf")            # the M-th logit: the floor a caller would have had to know
        ties_a = int((logit == floor).sum()) // 2

        ws_p = torch.empty(ws_links_bytes, dtype=torch.uint8, device="cuda")
        rowptr_p = torch.empty(N + 1, dtype=torch.int64, device="cuda")
        head_p = (Z.data_ptr(), H.data_ptr(), N, K, d, 1.0, prepared.rowptr.data_ptr(), prepared.col.data_ptr(), floor, None,
                  ws_p.data_ptr(), ws_p.numel(), rowptr_p.data_ptr())

        def links_count():
            _lib.check(lib.dl_score_links_count(*head_p, ops._stream()), "dl_score_links_count")

        links_count()
        nnz_p = int(rowptr_p[-1].item())
        col_p = torch.empty(nnz_p, dtype=torch.int32, device="cuda")
        logit_p = torch.empty(nnz_p, dtype=torch.float32, device="cuda")
        prob_p = torch.empty(nnz_p, dtype=torch.float32, device="cuda")

        def links_fill():
            _lib.check(lib.dl_score_links_fill(*head_p, nnz_p, col_p.data_ptr(), logit_p.data_ptr(), prob_p.data_ptr(), ops._stream()),
                       "dl_score_links_fill")

        links_fill()
        ties_p = int((logit_p == floor).sum()) // 2

        def top_op():
            return ops.score_top_links(Z, H, 1.0, M, exclude=prepared)

        def dense():
            return ops.score_allpairs_fwd(Z, H, 1.0)

        def dense_topk():
            p = ops.score_allpairs_fwd(Z, H, 1.0)
            keep = torch.ones(N, N, dtype=torch.bool, device="cuda").triu_(1)
            keep[ex_pairs[0], ex_pairs[1]] = False
            p.masked_fill_(~keep, -1.0)                                # below every probability
            return torch.topk(p.view(-1), M, sorted=False)

        fns = {"top_count": top_count, "top_fill": top_fill, "links_count": links_count, "links_fill": links_fill,
               "top_op": top_op, "dense": dense, "dense_topk": dense_topk}
        try:
            peak_c = peak_of(dense_topk)
            n_c = int((dense_topk()[0] >= 0).sum())
        except (torch.OutOfMemoryError, RuntimeError) as e:            # it does not fit, or topk does not take the size
            print(f"# dense + topk skipped at {name}, M = {M}: {type(e).__name__}", flush=True)
            peak_c = n_c = None
            del fns["dense_topk"]
            torch.cuda.empty_cache()
        # like with like: both normalise the same pair list inside the call, both allocate their workspace and outputs
        peak_a = peak_of(lambda: ops.score_top_links(Z, H, 1.0, M, exclude=ex_pairs))
        peak_p = peak_of(lambda: ops.score_links(Z, H, 1.0, floor, exclude=ex_pairs))
        # the extra workspace, and a 512-byte block of the allocator for each of the three outputs where their sizes differ
        allow = -(-(ws_top_bytes - ws_links_bytes) // 512) * 512 + 3 * 512
        peak_within = peak_a - 12 * nnz <= peak_p - 12 * nnz_p + allow
        t = {k: statistics.median(v) for k, v in interleaved(fns, seconds).items()}
        a, p = t["top_count"] + t["top_fill"], t["links_count"] + t["links_fill"]
        rec = {"shape": name, "N": N, "K": K, "d": d, "M": M, "links": nnz // 2, "mth_logit": round(floor, 6),
               "ties_at_cut_taken": ties_a, "links_at_floor": nnz_p // 2, "ties_at_floor": ties_p, "links_dense_route": n_c,
               "hist_scans": hist_scans, "scans": hist_scans + 2, "max_scans": form["scans"],
               "top_count_ms": round(t["top_count"], 3), "top_fill_ms": round(t["top_fill"], 3), "top_ms": round(a, 3),
               "links_count_ms": round(t["links_count"], 3), "links_fill_ms": round(t["links_fill"], 3), "links_ms": round(p, 3),
               "top_op_ms": round(t["top_op"], 3), "dense_ms": round(t["dense"], 3),
               "dense_topk_ms": round(t["dense_topk"], 3) if "dense_topk" in t else None,
               "top_over_links": round(a / p, 3), "expected_ratio": (hist_scans + 2) / 2,
               "top_peak_bytes": peak_a, "links_peak_bytes": peak_p, "dense_topk_peak_bytes": peak_c,
               "workspace_bytes": ws_top_bytes, "workspace_extra_bytes": ws_top_bytes - ws_links_bytes,
               "peak_within_extra": bool(peak_within)}
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as fh:
            fh.write(line + "\n")
        total = N * (N - 1) // 2
        if nnz // 2 != min(M, total - int(prepared.n_pairs.item())) or nnz_p // 2 - ties_p != nnz // 2 - ties_a or ties_p < ties_a:
            ok = False
        if hist_scans > 6 or not peak_within:
            ok = False
        del ws, ws_p, col, logit, prob, col_p, logit_p, prob_p
    return ok


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    out = os.path.join(ROOT, "profiles", "links_top_time.jsonl")
    ok = shape("bench", 5201, 8, 64, 0, (128048, 1284175), seconds, out)
    if "--skip-penn94" not in sys.argv:
        ok = shape("penn94_shaped", 41554, 8, 64, 1, (1036497, 10381773), seconds, out) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
