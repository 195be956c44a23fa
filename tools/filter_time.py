#!/usr/bin/env python3
"""usage: tools/filter_time.py [--seconds S] [--skip-penn94]  -> one JSON line per (shape, scan), appended to
profiles/filter_time.jsonl: what the node-group rule (ops.NodeFilter, dl_score_*_filtered) costs on top of the unfiltered
scan, and what it replaces.  Per scan — score_mine (m = 100), score_pair_ranks (the targets of tools/pair_rank_time.py) and
score_topk (every node a query, k = 100) — the library calls themselves, interleaved in one process, round after round,
until each has run for at least S seconds (default 1) after a warm-up; HIP events around each call, medians:
  (a) the unfiltered scan with the known pairs as its exclusion CSR;
  (b) the same with the filter: two seeded balanced groups under the rule `different`;
  (c) at the bench shape only, what a caller had to do before: the unfiltered scan with the pairs the rule does not allow
      LISTED in the exclusion CSR beside the known ones — the scan alone (c_ms), and with the listing and the CSR build in
      front of it (c_with_build_ms); peak allocator bytes of (b) (filter construction + call) and of (c) (listing + call).
At the Penn94 shape (c) is not run: the line reports the pairs and the CSR bytes it would need.
Shapes: the bench graph (N = 5,201, K = 8, d = 64) and a Penn94-shaped seeded table (N = 41,554); known pairs: 25 N seeded
random edges.  Exit status: 0 iff at the bench shape (b) is faster than (c) with its build and peaks lower, for every scan."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disenlink_amd import _lib, ops  # noqa: E402
from disenlink_amd.scans import _order_keys, _unordered_exclusion_csr  # noqa: E402
from mine_time import interleaved, peak_of, tables  # noqa: E402


def ptrs(rowptr, col):
    return rowptr.data_ptr(), col.data_ptr()


def scans(Z, H, N, K, d, known, src, dst):
    """name -> (call(csr, nf), csr of a pair list, ordered?): the raw library calls, no host read, no allocation"""
    lib = _lib.load()
    dev = Z.device
    m, k = 100, 100
    ws = ops._ws.get(max(int(lib.dl_score_mine_workspace_bytes(N, K, d, m)), int(lib.dl_score_pair_ranks_workspace_bytes(N, K, d)),
                         int(lib.dl_score_topk_workspace_bytes(N, K, d, N, k, 0))), dev)
    z, h, w, wn = Z.data_ptr(), H.data_ptr(), ws.data_ptr(), ws.numel()
    mo = [torch.empty(m, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
    count = torch.empty(1, dtype=torch.int64, device=dev)

    def mine(csr, nf):
        if nf is None:
            rc = lib.dl_score_mine(z, h, N, K, d, 1.0, *ptrs(*csr), float("-inf"), m, *[o.data_ptr() for o in mo], count.data_ptr(),
                                   w, wn, ops._stream())
        else:
            rc = lib.dl_score_mine_filtered(z, h, N, K, d, 1.0, *ptrs(*csr), float("-inf"), m, *[o.data_ptr() for o in mo],
                                            count.data_ptr(), w, wn, ops._stream(), nf)
        _lib.check(rc, "dl_score_mine")

    lo, hi = torch.minimum(src, dst), torch.maximum(src, dst)
    key = torch.sort(_order_keys(ops.score_pair_logits(Z, H, 1.0, lo, hi))).values
    tord = torch.where(key >= 0x80000000, key - 0x100000000, key).to(torch.int32).contiguous()
    T = int(tord.numel())
    above, equal = (torch.empty(T + 1, dtype=torch.int64, device=dev) for _ in range(2))
    ncand = torch.empty(1, dtype=torch.int64, device=dev)

    def pair_ranks(csr, nf):
        args = (z, h, N, K, d, 1.0, *ptrs(*csr), tord.data_ptr(), T, above.data_ptr(), equal.data_ptr(), ncand.data_ptr(), w, wn,
                ops._stream())
        _lib.check(lib.dl_score_pair_ranks(*args) if nf is None else lib.dl_score_pair_ranks_filtered(*args, nf), "dl_score_pair_ranks")

    q = torch.arange(N, dtype=torch.int32, device=dev)
    index = torch.empty(N, k, dtype=torch.int64, device=dev)
    logit, prob = (torch.empty(N, k, dtype=torch.float32, device=dev) for _ in range(2))

    def topk(csr, nf):
        args = (z, h, N, K, d, 1.0, q.data_ptr(), N, k, *ptrs(*csr), 1, index.data_ptr(), logit.data_ptr(), prob.data_ptr(), w, wn,
                ops._stream())
        _lib.check(lib.dl_score_topk(*args) if nf is None else lib.dl_score_topk_filtered(*args, nf), "dl_score_topk")

    unordered = lambda pairs: _unordered_exclusion_csr(pairs, N, dev)          # noqa: E731
    ordered = lambda pairs: ops.exclusion_csr((torch.cat([pairs[0], pairs[1]]), torch.cat([pairs[1], pairs[0]])), N, dev)    # noqa: E731
    return {"score_mine": (mine, unordered, ncand), "score_pair_ranks": (pair_ranks, unordered, ncand), "score_topk": (topk, ordered, None)}


def shape(name, N, K, d, seed, src, dst, seconds, out, listed):
    Z, H = tables(N, K, d, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    known = (torch.randint(0, N, (25 * N,), device="cuda", generator=g), torch.randint(0, N, (25 * N,), device="cuda", generator=g))
    groups = (torch.randperm(N, device="cuda", generator=g) % 2).to(torch.uint8)
    filt = ops.NodeFilter.different(groups)
    sizes = torch.bincount(groups.long(), minlength=2).tolist()
    n_listed = sum(c * (c - 1) // 2 for c in sizes)                    # unordered pairs the rule does not allow
    ok = True
    for scan, (call, make_csr, ncand) in scans(Z, H, N, K, d, known, src, dst).items():
        csr = make_csr(known)
        nf, _keep = filt._c_arg(N, Z.device, scan != "score_topk")

        def listing():                                                # the pairs the rule does not allow, beside the known ones
            same = groups[:, None] == groups[None, :]
            r, c = torch.nonzero(same, as_tuple=True)
            return make_csr((torch.cat([known[0], r]), torch.cat([known[1], c])))

        fns = {"a": lambda: call(csr, None), "b": lambda: call(csr, nf)}
        rec = {"shape": name, "N": N, "K": K, "d": d, "scan": scan, "known_pairs": int(known[0].numel()), "group_sizes": sizes,
               "pairs_not_allowed": n_listed}
        if listed:
            big = listing()
            fns["c"] = lambda: call(big, None)
            fns["c_with_build"] = lambda: call(listing(), None)
            rec["c_csr_bytes"] = int(big[0].numel() + big[1].numel()) * 4

            def fresh_filter():                                       # the filter made from the group array, then the call
                f = ops.NodeFilter.different(groups)
                call(csr, f._c_arg(N, Z.device, scan != "score_topk")[0])
                torch.cuda.synchronize()

            rec["b_peak_bytes"] = peak_of(fresh_filter)
            rec["c_peak_bytes"] = peak_of(lambda: call(listing(), None))
        else:                                                         # what (c) would need: rowptr + one int32 per listed pair
            per = 1 if scan != "score_topk" else 2
            rec["c_csr_bytes_needed"] = 4 * (N + 1) + 4 * per * (n_listed + int(known[0].numel()))
        t = {k: statistics.median(v) for k, v in interleaved(fns, seconds).items()}
        if listed and ncand is not None and scan == "score_pair_ranks":          # the same candidates either way
            call(csr, nf)
            n_b = int(ncand.item())
            call(big, None)
            rec["candidates"] = n_b
            rec["candidates_agree"] = n_b == int(ncand.item())
            ok = ok and rec["candidates_agree"]
        rec.update({f"{k}_ms": round(v, 3) for k, v in t.items()})
        rec["b_over_a"] = round(t["b"] / t["a"], 4)
        if listed:
            rec["b_faster_than_c_with_build"] = t["b"] < t["c_with_build"]
            rec["b_peak_below_c"] = rec["b_peak_bytes"] < rec["c_peak_bytes"]
            ok = ok and rec["b_faster_than_c_with_build"] and rec["b_peak_below_c"]
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as fh:
            fh.write(line + "\n")
    return ok


def main():
    from pair_rank_time import bench_targets
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = os.path.join(ROOT, "profiles", "filter_time.jsonl")
    N, src, dst, _known = bench_targets()
    ok = shape("bench", N, 8, 64, 0, src, dst, seconds, out, listed=True)
    if "--skip-penn94" not in sys.argv:
        N = 41554
        g = torch.Generator(device="cuda").manual_seed(101)
        src = torch.randint(0, N, (100000,), device="cuda", generator=g)
        dst = (src + 1 + torch.randint(0, N - 1, (100000,), device="cuda", generator=g)) % N
        ok = shape("penn94_shaped", N, 8, 64, 1, src, dst, seconds, out, listed=False) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
