#!/usr/bin/env python3
"""usage: tools/pair_terms_time.py [--seconds S] [--skip-penn94]  -> one JSON line per (shape, pairs, table type), appended
to profiles/pair_terms_time.jsonl: the per-factor terms of given pairs (dl_score_pair_terms, all three arrays, and `cum`
alone) against dl_score_pair_logits, the pass they come from, which does the same gathers and products and writes one value
per pair instead of 3 K.
The candidates are interleaved in one process, round after round, until each has run for at least S seconds (default 1)
after a warm-up; times are HIP events around each call, the median of the rounds.  They are the library calls themselves on
preallocated arrays (no host read, no allocation); `terms_op_ms` / `logits_op_ms` are ops.score_pair_terms /
ops.score_pair_logits as a user calls them.  Before anything is timed, cum[:, K-1] is compared with the logits bit for bit
at the timed size.
Shapes: the bench graph (N = 5,201, K = 8, d = 64) with 2^20 pairs and a Penn94-shaped seeded table (N = 41,554) with 2^20
and 10.4 M pairs, seeded random pairs, in fp32 and in bf16 tables.
Last line (Penn94 shape, fp32): ops.score_links at the floor above which about as many pairs lie as there are known pairs
(25 N seeded random edges), and ops.score_pair_terms of every link it lists: what explaining a whole predicted graph costs
beside the two scans that produced it.
There is no gate on the times.  Exit status 1 if cum[:, K-1] and the logits differ anywhere."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disenlink_amd import _lib, ops, scans  # noqa: E402
from links_time import floor_for  # noqa: E402
from mine_time import interleaved, tables  # noqa: E402


def same_bits(a, b):
    a, b = (torch.where(x == 0, torch.zeros_like(x), x) for x in (a, b))
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")


def pairs_case(name, Z, H, n_pairs, table, seed, seconds, out):
    lib = _lib.load()
    N, K, d = Z.shape
    dt = _lib.DL_BF16 if table == "bf16" else _lib.DL_F32
    tdt = torch.bfloat16 if table == "bf16" else torch.float32
    Zt, Ht = (Z.bfloat16(), H.bfloat16()) if table == "bf16" else (Z, H)
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randint(0, N, (n_pairs,), device="cuda", generator=g, dtype=torch.int32)
    b = torch.randint(0, N, (n_pairs,), device="cuda", generator=g, dtype=torch.int32)
    ws = torch.empty(int(lib.dl_score_pair_terms_workspace_bytes_dtype(N, K, d, dt)), dtype=torch.uint8, device="cuda")
    logit = torch.empty(n_pairs, dtype=torch.float32, device="cuda")
    e, q, cum = (torch.empty(n_pairs, K, dtype=torch.float32, device="cuda") for _ in range(3))
    head = (Zt.data_ptr(), Ht.data_ptr(), N, K, d, dt, 1.0, a.data_ptr(), b.data_ptr(), n_pairs)
    tail = (ws.data_ptr(), ws.numel())

    def logits():
        _lib.check(lib.dl_score_pair_logits_dtype(*head, logit.data_ptr(), *tail, ops._stream()), "dl_score_pair_logits_dtype")

    def terms():
        _lib.check(lib.dl_score_pair_terms_dtype(*head, e.data_ptr(), q.data_ptr(), cum.data_ptr(), *tail, ops._stream()),
                   "dl_score_pair_terms_dtype")

    def cum_only():
        _lib.check(lib.dl_score_pair_terms_dtype(*head, None, None, cum.data_ptr(), *tail, ops._stream()),
                   "dl_score_pair_terms_dtype")

    def logits_op():
        return ops.score_pair_logits(Zt, Ht, 1.0, a, b, table_dtype=tdt)

    def terms_op():
        return ops.score_pair_terms(Zt, Ht, 1.0, a, b, table_dtype=tdt)

    logits()
    terms()
    ok = same_bits(cum[:, -1], logit)
    fns = {"logits": logits, "terms": terms, "cum_only": cum_only, "logits_op": logits_op, "terms_op": terms_op}
    t = {k: statistics.median(v) for k, v in interleaved(fns, seconds).items()}
    emit({"shape": name, "N": N, "K": K, "d": d, "pairs": n_pairs, "tables": table,
          "logits_ms": round(t["logits"], 3), "terms_ms": round(t["terms"], 3), "cum_only_ms": round(t["cum_only"], 3),
          "terms_over_logits": round(t["terms"] / t["logits"], 3), "cum_only_over_logits": round(t["cum_only"] / t["logits"], 3),
          "logits_op_ms": round(t["logits_op"], 3), "terms_op_ms": round(t["terms_op"], 3),
          "bytes_written_terms": 3 * 4 * K * n_pairs, "last_cum_is_the_logit": ok}, out)
    return ok


def links_case(name, Z, H, seed, seconds, out):
    """ops.score_links at the 'edges' floor of tools/links_time.py, and the terms of every link it lists"""
    N, K, d = Z.shape
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    rows = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    cols = torch.randint(0, N, (25 * N,), device="cuda", generator=g)
    ex = scans._unordered_exclusion_csr((rows, cols), N, Z.device)
    ptr = ex[0].to(torch.int64)
    ex_pairs = (torch.repeat_interleave(torch.arange(N, device="cuda"), ptr[1:] - ptr[:-1]), ex[1].to(torch.int64))
    known = int((ex_pairs[0] < ex_pairs[1]).sum())
    floor = floor_for(Z, H, known / (N * (N - 1) // 2), seed + 200)
    rowptr, col, logit, _ = ops.score_links(Z, H, 1.0, floor, exclude=ex_pairs)
    r = torch.repeat_interleave(torch.arange(N, device="cuda"), rowptr[1:] - rowptr[:-1])
    keep = r < col
    src, dst, want = r[keep].to(torch.int32), col[keep].contiguous(), logit[keep]

    def links_op():
        return ops.score_links(Z, H, 1.0, floor, exclude=ex_pairs)

    def explain_op():
        return ops.score_pair_terms(Z, H, 1.0, src, dst)

    ok = same_bits(explain_op().logit, want)
    t = {k: statistics.median(v) for k, v in interleaved({"links_op": links_op, "explain_op": explain_op}, seconds).items()}
    emit({"shape": name, "N": N, "K": K, "d": d, "tables": "f32", "what": "explain every link of score_links",
          "min_logit": round(floor, 6), "links": int(src.numel()), "links_op_ms": round(t["links_op"], 3),
          "explain_op_ms": round(t["explain_op"], 3), "explain_over_links": round(t["explain_op"] / t["links_op"], 3),
          "explained_logit_is_the_listed_one": ok}, out)
    return ok


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    out = os.path.join(ROOT, "profiles", "pair_terms_time.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    ok = True
    cases = [("bench", 5201, 0, (1 << 20,))]
    if "--skip-penn94" not in sys.argv:
        cases.append(("penn94_shaped", 41554, 1, (1 << 20, 10_400_000)))
    for name, N, seed, sizes in cases:
        Z, H = tables(N, 8, 64, seed)
        for n_pairs in sizes:
            for table in ("f32", "bf16"):
                ok = pairs_case(name, Z, H, n_pairs, table, seed + 7, seconds, out) and ok
        if name == "penn94_shaped":
            ok = links_case(name, Z, H, seed, seconds, out) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
