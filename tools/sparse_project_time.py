#!/usr/bin/env python3
"""usage: tools/sparse_project_time.py [--seconds S]  -> JSON lines: the projection forward + backward on a SparseFeatures
input (ops.project_sparse_fwd / _bwd: layer 1 and dW1 as gathers) against the dense kernels on its to_dense()
(ops.project_fwd(keep_hid=True) / project_bwd, persistent x planes in use), interleaved in ONE process (HIP events; every
candidate is repeated for at least S = 1 second in all after warm-up, in rounds that alternate between the candidates).
  cora     the Cora fixture (tests/golden/real_cora.npz: N = 2,708, F = 1,433, binary, unstandardised) at its recipe
           K = 10, d = 64, nhid = 256
  penn94   a seeded Penn94-shaped input: N = 41,554, F = 4,814, seven ones per row (one per categorical block), rows
           standardised; K = 8, d = 64, nhid = 512 (the benchmark's defaults for the penn94 workload)
Peak device memory of both forms is recorded at the penn94 shape (allocator peak over one forward + backward, the inputs
included).  GATE: the exit status is 1 where the sparse path is slower than the dense one at either shape.  Any failing step
(a call that raises, a non-finite result, a disagreement of the two forms) ends the run there."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disenlink_amd import ops  # noqa: E402
from disenlink_amd.features import SparseFeatures  # noqa: E402
from tools.dense_bwd_time import finite, interleaved  # noqa: E402


def weights(F, K, nhid, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    return r(K, nhid, F) / 8.0, r(K, nhid) * 0.1, r(K, d, nhid) / nhid ** 0.5, r(K, d) * 0.1


def penn94_like(seed=0):
    """Seven one-hot blocks over 4,814 columns (block widths as uneven as categorical flags are: one block of 2 columns — a
    flag that holds about half of the nodes each — up to one of thousands)."""
    N, widths = 41_554, (2, 6, 12, 60, 230, 1_500, 3_004)
    assert sum(widths) == 4_814
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(N), len(widths))
    cols = np.stack([off + rng.integers(0, w, N) for off, w in zip(np.cumsum((0,) + widths[:-1]), widths)], axis=1).reshape(-1)
    return SparseFeatures.from_coo(rows, cols, (N, sum(widths)), standardise=True)


def one_shape(name, sf, K, nhid, d, seconds, reps, want_memory):
    sf = sf.to("cuda")
    N, F = sf.shape
    W1, b1, W2, b2 = weights(F, K, nhid, d, 1)
    dZ = torch.randn(N, K, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) / N

    def sparse():
        Z, hid = ops.project_sparse_fwd(sf, W1, b1, W2, b2)
        return (Z,) + ops.project_sparse_bwd(sf, W1, b1, W2, dZ, hid=hid)

    mem = {}
    if want_memory:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = sparse()
        torch.cuda.synchronize()
        mem["sparse_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        mem["sparse_features_bytes"] = int(sum(t.numel() * t.element_size() for t in sf._tensors() if t is not None))
        del out
    x = sf.to_dense()
    ops.xplanes_for(x, force=True)                              # the dense path as a training run has it: planes of x built once

    def dense():
        Z, hid = ops.project_fwd(x, W1, b1, W2, b2, keep_hid=True)
        return (Z,) + ops.project_bwd(x, W1, b1, W2, dZ, hid=hid)

    if want_memory:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = dense()
        torch.cuda.synchronize()
        mem["dense_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        mem["dense_x_bytes"] = int(x.numel() * 4)
        mem["bytes_before"] = int(base)
        del out
    # agreement: Z of the two forwards; the gradients of the two backwards FROM ONE hidden layer (the sparse forward's — the
    # two forwards round differently, so a few of the N K nhid pre-activations next to zero fall on different sides of the
    # ReLU, and each such flip moves whole rows of dW1; the flips are counted and reported)
    Zs, hid_s = ops.project_sparse_fwd(sf, W1, b1, W2, b2)
    Zd, hid_d = ops.project_fwd(x, W1, b1, W2, b2, keep_hid=True)
    ld = (N + 3) // 4 * 4                                       # hidT [K][nhid][ld]: the columns N .. ld-1 are padding
    flips = int(((hid_s.view(K, nhid, ld)[:, :, :N] > 0) != (hid_d.view(K, nhid, ld)[:, :, :N] > 0)).sum())
    a = (Zs,) + ops.project_sparse_bwd(sf, W1, b1, W2, dZ, hid=hid_s)
    b = (Zd,) + ops.project_bwd(x, W1, b1, W2, dZ, hid=hid_s)
    finite(*a, *b)
    worst = 0.0
    for s_, d_ in zip(a, b):
        scale = max(float(d_.abs().max()), 1e-30)
        worst = max(worst, float((s_ - d_).abs().max()) / scale)
    if not worst <= 1e-4:
        raise RuntimeError(f"{name}: sparse and dense projections disagree: {worst} of the largest entry")
    del a, b, Zs, Zd, hid_s, hid_d
    r = interleaved({"sparse": sparse, "dense": dense}, seconds, reps)
    ok = r["sparse"][0] <= r["dense"][0]
    note = "HIP events, interleaved rounds in one process, >= %.1f s of repetitions per candidate after warm-up" % seconds
    print(json.dumps({"shape": name, "N": N, "F": F, "nnz": sf.nnz, "density": sf.nnz / (N * F), "standardised": sf.shift is not None,
                      "K": K, "d": d, "nhid": nhid, "sparse_fwd_bwd_ms": round(r["sparse"][0], 4),
                      "dense_fwd_bwd_ms": round(r["dense"][0], 4), "best_round_ms": {n: round(v[1], 4) for n, v in r.items()},
                      "repetitions": {n: v[2] for n, v in r.items()}, "dense_over_sparse": round(r["dense"][0] / r["sparse"][0], 2),
                      "max_abs_difference_over_scale": worst, "relu_mask_flips": flips,
                      "hidden_elements": N * K * nhid, **mem, "gate_sparse_not_slower_than_dense": bool(ok),
                      "measured": note}), flush=True)
    return ok


def main():
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0
    g = np.load(os.path.join(ROOT, "tests", "golden", "real_cora.npz"))
    shape = tuple(int(v) for v in g["feat_shape"])
    cora = SparseFeatures.from_coo(g["feat_row"].astype(np.int64), g["feat_col"].astype(np.int64), shape)
    ok = one_shape("cora", cora, 10, 256, 64, seconds, {"sparse": 20, "dense": 20}, False)
    torch.cuda.empty_cache()
    ok = one_shape("penn94-shaped", penn94_like(), 8, 512, 64, seconds, {"sparse": 3, "dense": 3}, True) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
