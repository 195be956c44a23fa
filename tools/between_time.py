#!/usr/bin/env python3
"""usage: tools/between_time.py [--seconds S] [--skip-penn94] [--skip-large]  -> JSON lines appended to
profiles/between_time.jsonl: the link scans between two node sets and by blocks.
(a) ops.score_mine_between (m = 10,000) and ops.score_links_between on the two halves of a table, against (b) the
    triangular ops.score_mine / ops.score_links on the whole table under NodeFilter.between, which gives the same result;
    at the bench shape (N = 5,201, K = 8, d = 64) and a Penn94-shaped seeded table (N = 41,554).  The floor of the link
    graph is the logit that about 25 N pairs reach (tools/links_time.py's, from a sample).
(c) ops.score_mine_blocks (m = 10,000) at N = 41,554 with blocks of N / 2 and N / 4 rows (rounded up to 128), against the
    unblocked ops.score_mine.
(d) ops.score_mine_blocks, m = 10,000, default blocks, on a seeded table of N = 169,343 (the size of arxiv-year), K = 8,
    d = 64: four blocks, ten windows.
All candidates of a line are interleaved in one process, round after round, until each has run for at least S seconds
(default 1) after a warm-up; times are HIP events around each call (the calls as a user makes them, host reads included),
the median of the rounds.  Each line carries the expectation it is to be read against (`expect`); none of them is a
threshold.  Exit status 1 only if (a) and (b), or (c) and the unblocked call, disagree in a single bit, if (a) is slower
than (b), or if a blocked call allocates more than 64 (N + 8 m) bytes beside the shared workspace, which it sizes once for
its largest window (`window_workspace_bytes`, from the sizers; the buffer is grow-only and outlives the call, so the
allocator's peak is taken with it in place)."""
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
from mine_time import interleaved, peak_of, tables  # noqa: E402

M = 10000


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")


def halves(name, N, K, d, seed, seconds, out):
    """(a) against (b)"""
    Z, H = tables(N, K, d, seed)
    nA = N // 2
    ZA, HA, ZB, HB = Z[:nA], H[:nA], Z[nA:], H[nA:]
    in_a = torch.arange(N, device="cuda") < nA
    nf = ops.NodeFilter.between(in_a, ~in_a, device="cuda")
    floor = floor_for(Z, H, 25 * N / (N * (N - 1) // 2), seed + 200)

    def mine_between():
        return ops.score_mine_between(ZA, HA, ZB, HB, 1.0, M)

    def mine_filtered():
        return ops.score_mine(Z, H, 1.0, M, node_filter=nf)

    def links_between():
        return ops.score_links_between(ZA, HA, ZB, HB, 1.0, floor)

    def links_filtered():
        return ops.score_links(Z, H, 1.0, floor, node_filter=nf)

    a, b = mine_between(), mine_filtered()
    equal = same(a, (b[0], b[1] - nA, b[2], b[3]))
    la, lb = links_between(), links_filtered()
    cut = int(lb[0][nA])
    equal = equal and same(la.ab, (lb[0][:nA + 1], lb[1][:cut] - nA, lb[2][:cut], lb[3][:cut])) and \
        same(la.ba, (lb[0][nA:] - cut, lb[1][cut:], lb[2][cut:], lb[3][cut:]))
    links = int(la.ab[0][-1])
    del a, b, la, lb
    t = {k: statistics.median(v) for k, v in interleaved({"mine_between": mine_between, "mine_filtered": mine_filtered,
                                                          "links_between": links_between, "links_filtered": links_filtered},
                                                         seconds).items()}
    fb = _lib.score_mine_between_form(nA, N - nA, K, d, M)
    rec = {"part": "a_vs_b", "shape": name, "N": N, "nA": nA, "nB": N - nA, "K": K, "d": d, "m": M, "min_logit": round(floor, 6),
           "links": links, "tile_pairs_between": fb["pairs"], "tile_pairs_triangle": _lib.score_mine_form(N, K, d, M)["pairs"],
           "mine_between_ms": round(t["mine_between"], 3), "mine_filtered_ms": round(t["mine_filtered"], 3),
           "mine_ratio": round(t["mine_between"] / t["mine_filtered"], 3),
           "links_between_ms": round(t["links_between"], 3), "links_filtered_ms": round(t["links_filtered"], 3),
           "links_ratio": round(t["links_between"] / t["links_filtered"], 3),
           "expect": "ratios about 0.5: half the tile pairs are walked", "equal_bits": bool(equal)}
    emit(out, rec)
    return equal and t["mine_between"] <= t["mine_filtered"] and t["links_between"] <= t["links_filtered"]


def window_ws(N, K, d, block):
    """the largest workspace of one window of a blocked mining call"""
    lib = _lib.load()
    n0 = min(block, N)
    need = int(lib.dl_score_mine_workspace_bytes_dtype(n0, K, d, _lib.DL_F32, M))
    if N > block:
        need = max(need, int(lib.dl_score_mine_between_workspace_bytes_dtype(n0, min(block, N - block), K, d, _lib.DL_F32, M)))
    return need


def blocked(N, K, d, seed, seconds, out):
    """(c): blocks of N / 2 and N / 4 against the unblocked call"""
    Z, H = tables(N, K, d, seed)
    up = lambda v, q: (v + q - 1) // q                                # ceil(v / q)
    sizes = {f"blocks_{k}": up(up(N, k), 128) * 128 for k in (2, 4)}
    fns = {"unblocked": lambda: ops.score_mine(Z, H, 1.0, M)}
    for name, bn in sizes.items():
        fns[name] = (lambda bn: lambda: ops.score_mine_blocks(Z, H, 1.0, M, block_nodes=bn))(bn)
    ref = fns["unblocked"]()
    equal = all(same(ref, fns[name]()) for name in sizes)
    peaks = {name: peak_of(fns[name]) for name in sizes}
    bound = 64 * (N + 8 * M)
    del ref
    t = {k: statistics.median(v) for k, v in interleaved(fns, seconds).items()}
    rec = {"part": "c_blocks", "N": N, "K": K, "d": d, "m": M, "unblocked_ms": round(t["unblocked"], 3), "equal_bits": bool(equal),
           "expect": "blocked within the extra launches and the per-window selects of the unblocked call"}
    for name, bn in sizes.items():
        nb = -(-N // bn)
        rec[name] = {"block_nodes": bn, "windows": nb * (nb + 1) // 2, "ms": round(t[name], 3),
                     "over_unblocked": round(t[name] / t["unblocked"], 3), "window_workspace_bytes": window_ws(N, K, d, bn),
                     "peak_bytes_beside_workspace": peaks[name], "peak_bound_bytes": bound}
    emit(out, rec)
    return equal and all(peaks[n] <= bound for n in sizes)


def large(N, K, d, seed, seconds, out):
    """(d): a graph past the cap of the triangular walk"""
    Z, H = tables(N, K, d, seed)

    def run():
        return ops.score_mine_blocks(Z, H, 1.0, M)

    src, dst, logit, _ = run()
    sane = len(src) == M and bool((src < dst).all()) and bool((logit[:-1] >= logit[1:]).all())
    peak = peak_of(run)
    bound = 64 * (N + 8 * M)
    t = statistics.median(interleaved({"run": run}, seconds)["run"])
    nb = -(-N // ops.BLOCK_NODES)
    penn = [json.loads(ln) for ln in open(os.path.join(ROOT, "profiles", "mine_time.jsonl"))]
    penn = [r for r in penn if r.get("shape") == "penn94_shaped" and r.get("m") == M]
    expect_ms = round(penn[-1]["mine_ms"] * (N / penn[-1]["N"]) ** 2, 1) if penn else None
    emit(out, {"part": "d_large", "N": N, "K": K, "d": d, "m": M, "block_nodes": ops.BLOCK_NODES, "windows": nb * (nb + 1) // 2,
               "mine_blocks_ms": round(t, 3), "expect_ms": expect_ms,
               "expect": "(N / 41,554)^2 x the Penn94 figure of profiles/mine_time.jsonl", "window_workspace_bytes": window_ws(N, K, d, ops.BLOCK_NODES), "peak_bytes_beside_workspace": peak,
               "peak_bound_bytes": bound, "sorted_and_full": bool(sane)})
    return sane and peak <= bound


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    out = os.path.join(ROOT, "profiles", "between_time.jsonl")
    ok = halves("bench", 5201, 8, 64, 0, seconds, out)
    if "--skip-penn94" not in sys.argv:
        ok = halves("penn94_shaped", 41554, 8, 64, 1, seconds, out) and ok
        ok = blocked(41554, 8, 64, 1, seconds, out) and ok
    if "--skip-large" not in sys.argv:
        ok = large(169343, 8, 64, 2, seconds, out) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
