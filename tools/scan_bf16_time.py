#!/usr/bin/env python3
"""usage: tools/scan_bf16_time.py [--seconds S] [--skip-penn94]  -> one JSON line per (shape, scan), appended to
profiles/scan_bf16_time.jsonl: the all-pairs scans on bf16 tables (dl_score_*_dtype with DL_BF16: one plane per operand, one
matrix-core product per block) against the fp32 entries (three planes, six products) on the same tables, rounded to bf16 and
widened, so that both do the same selection work.
Per scan three candidates are interleaved in one process, round after round, until each has run for at least S seconds
(default 1) after a warm-up: (a) the fp32 entry, (b) the bf16 entry, (a2) the fp32 entry again — the spread of the process
itself is |a - a2|.  Times are HIP events around each call, the median of the rounds.  mine, links (count + fill) and top-k
are the library calls themselves on preallocated arrays; pair ranks is ops.score_pair_ranks with a prepared exclusion (its
target pass and host-side sort included, the same for both).  Peak allocator memory is that of one ops call per candidate
with the shared workspace dropped beforehand, so it includes the workspace.
Shapes: the bench graph (N = 5,201, K = 8, d = 64) and a Penn94-shaped seeded table (N = 41,554); the known pairs are 25 N
seeded random edges.  Scans: mine (m = 100 and 10,000), pair ranks (4,096 targets), links (count + fill at the floor above
which about as many pairs lie as there are known pairs), top-k (all nodes at the bench shape, 4,096 queries at Penn94; k = 100).
Exit status 1 if (b)'s peak allocation is not below (a)'s, or if at the Penn94 shape (b) is slower than (a) by more than the
spread the two (a) runs show (|a - a2|, at least 1 % of a)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disenlink_amd import _lib, ops  # noqa: E402
from links_time import floor_for  # noqa: E402
from mine_time import interleaved, tables  # noqa: E402

F32, BF16 = _lib.DL_F32, _lib.DL_BF16
NINF = float("-inf")


def peak_fresh(fn):
    """peak allocator bytes of one call that allocates its own workspace (the shared grow-only one is dropped first)"""
    ops._ws.buf.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ops._ws.buf.clear()
    return peak


def record(out, name, N, K, d, scan, t, peaks, ws, extra=None):
    a, b, a2 = (statistics.median(t[k]) for k in ("a", "b", "a2"))
    spread = abs(a - a2)
    rec = {"shape": name, "N": N, "K": K, "d": d, "scan": scan, "f32_ms": round(a, 3), "bf16_ms": round(b, 3),
           "f32_again_ms": round(a2, 3), "spread_ms": round(spread, 3), "f32_over_bf16": round(min(a, a2) / b, 3),
           "rounds": len(t["b"]), "f32_peak_bytes": peaks[0], "bf16_peak_bytes": peaks[1],
           "f32_workspace_bytes": ws[0], "bf16_workspace_bytes": ws[1]}
    rec.update(extra or {})
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")
    ok = peaks[1] < peaks[0]
    if name == "penn94_shaped" and b > max(a, a2) + max(spread, 0.01 * a):
        ok = False
    return ok


def shape(name, N, K, d, seed, seconds, out, n_queries):
    lib = _lib.load()
    Z, H = tables(N, K, d, seed)
    Zb, Hb = Z.bfloat16().contiguous(), H.bfloat16().contiguous()
    Zw, Hw = Zb.float(), Hb.float()                                  # (a) and (b) see the same values
    del Z, H
    tab = {F32: (Zw, Hw), BF16: (Zb, Hb)}
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    rows = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    cols = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    pex = ops.pair_exclusion((rows, cols), N, Zw.device)             # the CSR once, as a caller with a fixed graph would
    exr, exc = pex.rowptr, pex.col
    ex_pairs = (torch.div(pex.key, N, rounding_mode="floor"), pex.key % N)
    known = int(pex.n_pairs)
    stream = ops._stream
    ok = True

    def three(make):
        fa, fb = make(F32), make(BF16)
        return interleaved({"a": fa, "b": fb, "a2": fa}, seconds)

    # ---- mine
    for m in (100, 10000):
        outs = [torch.empty(m, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
        count = torch.empty(1, dtype=torch.int64, device="cuda")
        wsb = [int(lib.dl_score_mine_workspace_bytes_dtype(N, K, d, dt, m)) for dt in (F32, BF16)]
        ws = torch.empty(wsb[0], dtype=torch.uint8, device="cuda")

        def make(dt):
            Zc, Hc = tab[dt]
            return lambda: _lib.check(lib.dl_score_mine_dtype(
                Zc.data_ptr(), Hc.data_ptr(), N, K, d, dt, 1.0, exr.data_ptr(), exc.data_ptr(), NINF, m,
                *[o.data_ptr() for o in outs], count.data_ptr(), ws.data_ptr(), ws.numel(), stream(), None), "dl_score_mine_dtype")

        t = three(make)
        del ws
        peaks = [peak_fresh(lambda: ops.score_mine(Zw, Hw, 1.0, m, exclude=ex_pairs)),
                 peak_fresh(lambda: ops.score_mine(Zb, Hb, 1.0, m, exclude=ex_pairs, table_dtype=torch.bfloat16))]
        ok = record(out, name, N, K, d, f"mine_m{m}", t, peaks, wsb, {"count": int(count.item())}) and ok

    # ---- pair ranks
    gt = torch.Generator(device="cuda").manual_seed(seed + 300)
    ts = torch.randint(0, N, (4096,), device="cuda", generator=gt)
    td = (ts + 1 + torch.randint(0, N - 1, (4096,), device="cuda", generator=gt)) % N
    wsb = [int(lib.dl_score_pair_ranks_workspace_bytes_dtype(N, K, d, dt)) for dt in (F32, BF16)]
    t = three(lambda dt: (lambda: ops.score_pair_ranks(*tab[dt], 1.0, ts, td, exclude=pex,
                                                       table_dtype=torch.bfloat16 if dt == BF16 else torch.float32)))
    peaks = [peak_fresh(lambda: ops.score_pair_ranks(Zw, Hw, 1.0, ts, td, exclude=pex)),
             peak_fresh(lambda: ops.score_pair_ranks(Zb, Hb, 1.0, ts, td, exclude=pex, table_dtype=torch.bfloat16))]
    ok = record(out, name, N, K, d, "pair_ranks", t, peaks, wsb, {"targets": 4096}) and ok

    # ---- links: count + fill
    floor = floor_for(Zw, Hw, known / (N * (N - 1) // 2), seed + 200)
    wsb = [int(lib.dl_score_links_workspace_bytes_dtype(N, K, d, dt)) for dt in (F32, BF16)]
    ws = torch.empty(wsb[0], dtype=torch.uint8, device="cuda")
    rowptr = torch.empty(N + 1, dtype=torch.int64, device="cuda")

    def head(dt):
        Zc, Hc = tab[dt]
        return (Zc.data_ptr(), Hc.data_ptr(), N, K, d, dt, 1.0, exr.data_ptr(), exc.data_ptr(), floor, None, ws.data_ptr(),
                ws.numel(), rowptr.data_ptr())

    _lib.check(lib.dl_score_links_count_dtype(*head(F32), stream()), "dl_score_links_count_dtype")
    nnz = int(rowptr[-1].item())
    col = torch.empty(nnz, dtype=torch.int32, device="cuda")
    logit = torch.empty(nnz, dtype=torch.float32, device="cuda")
    prob = torch.empty(nnz, dtype=torch.float32, device="cuda")

    def make(dt):
        h = head(dt)

        def both():
            _lib.check(lib.dl_score_links_count_dtype(*h, stream()), "dl_score_links_count_dtype")
            _lib.check(lib.dl_score_links_fill_dtype(*h, nnz, col.data_ptr(), logit.data_ptr(), prob.data_ptr(), stream()),
                       "dl_score_links_fill_dtype")
        return both

    t = three(make)
    del ws, col, logit, prob
    peaks = [peak_fresh(lambda: ops.score_links(Zw, Hw, 1.0, floor, exclude=ex_pairs)),
             peak_fresh(lambda: ops.score_links(Zb, Hb, 1.0, floor, exclude=ex_pairs, table_dtype=torch.bfloat16))]
    ok = record(out, name, N, K, d, "links_count_fill", t, peaks, wsb, {"links": nnz // 2, "min_logit": round(floor, 6)}) and ok

    # ---- top-k
    Q, k = n_queries, 100
    q = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + 400))[:Q].to(torch.int32)
    q = q.sort().values.contiguous()
    ex_csr = ops.exclusion_csr((torch.cat([ex_pairs[0], ex_pairs[1]]), torch.cat([ex_pairs[1], ex_pairs[0]])), N, Zw.device)
    index = torch.empty(Q, k, dtype=torch.int64, device="cuda")
    lg = torch.empty(Q, k, dtype=torch.float32, device="cuda")
    pr = torch.empty(Q, k, dtype=torch.float32, device="cuda")
    wsb = [int(lib.dl_score_topk_workspace_bytes_dtype(N, K, d, dt, Q, k, 0)) for dt in (F32, BF16)]
    ws = torch.empty(wsb[0], dtype=torch.uint8, device="cuda")

    def make(dt):
        Zc, Hc = tab[dt]
        return lambda: _lib.check(lib.dl_score_topk_dtype(
            Zc.data_ptr(), Hc.data_ptr(), N, K, d, dt, 1.0, q.data_ptr(), Q, k, ex_csr[0].data_ptr(), ex_csr[1].data_ptr(), 1,
            index.data_ptr(), lg.data_ptr(), pr.data_ptr(), ws.data_ptr(), ws.numel(), stream(), None), "dl_score_topk_dtype")

    t = three(make)
    del ws
    both_ways = (torch.cat([ex_pairs[0], ex_pairs[1]]), torch.cat([ex_pairs[1], ex_pairs[0]]))
    peaks = [peak_fresh(lambda: ops.score_topk(Zw, Hw, 1.0, q, k, exclude=both_ways)),
             peak_fresh(lambda: ops.score_topk(Zb, Hb, 1.0, q, k, exclude=both_ways, table_dtype=torch.bfloat16))]
    ok = record(out, name, N, K, d, "topk_k100", t, peaks, wsb, {"queries": Q}) and ok
    return ok


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    out = os.path.join(ROOT, "profiles", "scan_bf16_time.jsonl")
    ok = shape("bench", 5201, 8, 64, 0, seconds, out, 5201)
    if "--skip-penn94" not in sys.argv:
        ok = shape("penn94_shaped", 41554, 8, 64, 1, seconds, out, 4096) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
