#!/usr/bin/env python3
"""usage: tools/links_time.py [--seconds S] [--skip-penn94]  -> one JSON line per (shape, floor), appended to
profiles/links_time.jsonl: the thresholded link graph (dl_score_links_count + dl_score_links_fill) against (b) the dense
forward alone (ops.score_allpairs_fwd) and (c) dense forward + mask + torch.nonzero, the route there was before.
count, fill, (b) and (c) are interleaved in one process, round after round, until each has run for at least S seconds
(default 1) after a warm-up; times are HIP events around each call, the median of the rounds.  count and fill are the
library calls themselves on preallocated arrays (no host read, no allocation); `links_op_ms` is ops.score_links as a user
calls it, with the normalisation of the exclusion, the read of rowptr[N] and the allocations.  Peak allocator memory of
ops.score_links (its workspace included) and of (c) is taken in separate single calls; (c) is skipped where it does not fit.
Shapes: the bench graph (N = 5,201, K = 8, d = 64) and a Penn94-shaped seeded table (N = 41,554); the known pairs are 25 N
seeded random edges.  Floors: the logit above which about as many pairs lie as there are known pairs (from a sample of
4 M scored pairs), and the one above which ten times as many lie.
Exit status 1 if a result disagrees with (c) in its number of links, or if at the Penn94 shape the peak memory of
ops.score_links is not below that of (c)."""
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


def floor_for(Z, H, share, seed):
    """the logit that a `share` of all unordered pairs reaches, from 4 M sampled pairs"""
    N = Z.shape[0]
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randint(0, N, (1 << 22,), device="cuda", generator=g)
    b = torch.randint(0, N, (1 << 22,), device="cuda", generator=g)
    keep = a != b
    x = ops.score_pair_logits(Z, H, 1.0, torch.minimum(a, b)[keep], torch.maximum(a, b)[keep])
    k = max(1, int(round(share * x.numel())))
    return float(torch.topk(x, k).values[-1])


def shape(name, N, K, d, seed, seconds, out):
    lib = _lib.load()
    Z, H = tables(N, K, d, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    rows = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    cols = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    ex = scans._unordered_exclusion_csr((rows, cols), N, Z.device)      # the CSR once, as a caller with a fixed graph would
    ptr = ex[0].to(torch.int64)
    ex_pairs = (torch.repeat_interleave(torch.arange(N, device="cuda"), ptr[1:] - ptr[:-1]), ex[1].to(torch.int64))
    known = int((ex_pairs[0] < ex_pairs[1]).sum())
    total = N * (N - 1) // 2
    ok = True
    for label, mult in (("edges", 1), ("ten_times", 10)):
        floor = floor_for(Z, H, mult * known / total, seed + 200)
        ws = torch.empty(int(lib.dl_score_links_workspace_bytes(N, K, d)), dtype=torch.uint8, device="cuda")
        rowptr = torch.empty(N + 1, dtype=torch.int64, device="cuda")
        head = (Z.data_ptr(), H.data_ptr(), N, K, d, 1.0, ex[0].data_ptr(), ex[1].data_ptr(), floor, None, ws.data_ptr(),
                ws.numel(), rowptr.data_ptr())

        def count():
            _lib.check(lib.dl_score_links_count(*head, ops._stream()), "dl_score_links_count")

        count()
        nnz = int(rowptr[-1].item())
        col = torch.empty(nnz, dtype=torch.int32, device="cuda")
        logit = torch.empty(nnz, dtype=torch.float32, device="cuda")
        prob = torch.empty(nnz, dtype=torch.float32, device="cuda")

        def fill():
            _lib.check(lib.dl_score_links_fill(*head, nnz, col.data_ptr(), logit.data_ptr(), prob.data_ptr(), ops._stream()),
                       "dl_score_links_fill")

        def links_op():
            return ops.score_links(Z, H, 1.0, floor, exclude=ex_pairs)

        def dense():
            return ops.score_allpairs_fwd(Z, H, 1.0)

        p_floor = float(torch.sigmoid(torch.tensor(floor, dtype=torch.float64)))

        def dense_nonzero():
            p = ops.score_allpairs_fwd(Z, H, 1.0)
            keep = (p >= p_floor).triu_(1)
            keep[ex_pairs[0], ex_pairs[1]] = False
            idx = torch.nonzero(keep)
            return idx, p[keep]

        fns = {"count": count, "fill": fill, "links_op": links_op, "dense": dense, "dense_nonzero": dense_nonzero}
        try:
            peak_c = peak_of(dense_nonzero)
            n_c = int(dense_nonzero()[0].shape[0])
        except torch.OutOfMemoryError:
            peak_c = n_c = None
            del fns["dense_nonzero"]
            torch.cuda.empty_cache()
        peak_a = peak_of(links_op)                                    # its workspace is allocated inside the call
        t = {k: statistics.median(v) for k, v in interleaved(fns, seconds).items()}
        both = t["count"] + t["fill"]
        rec = {"shape": name, "N": N, "K": K, "d": d, "floor": label, "min_logit": round(floor, 6), "known_pairs": known,
               "links": nnz // 2, "links_dense_route": n_c,
               "count_ms": round(t["count"], 3), "fill_ms": round(t["fill"], 3), "count_fill_ms": round(both, 3),
               "links_op_ms": round(t["links_op"], 3), "dense_ms": round(t["dense"], 3),
               "dense_nonzero_ms": round(t["dense_nonzero"], 3) if "dense_nonzero" in t else None,
               "count_fill_over_dense": round(both / t["dense"], 3),
               "links_peak_bytes": peak_a, "dense_nonzero_peak_bytes": peak_c,
               "peak_below_dense_route": bool(peak_a < peak_c) if peak_c is not None else None,
               "workspace_bytes": int(ws.numel())}
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as fh:
            fh.write(line + "\n")
        # the dense route rounds differently (fp32 sigmoid of the dense scorer's logits): counts agree to a few pairs at the floor
        if n_c is not None and abs(n_c - nnz // 2) > max(10, 1e-3 * n_c):
            ok = False
        if name == "penn94_shaped" and rec["peak_below_dense_route"] is False:
            ok = False
        del ws, col, logit, prob
    return ok


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    out = os.path.join(ROOT, "profiles", "links_time.jsonl")
    ok = shape("bench", 5201, 8, 64, 0, seconds, out)
    if "--skip-penn94" not in sys.argv:
        ok = shape("penn94_shaped", 41554, 8, 64, 1, seconds, out) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
