"""fp64 reference of the global top-m link mining (ops.score_mine / dl_score_mine) and the case list of its GPU test,
shared by tests/test_mine_cpu.py (which checks the reference itself and what the case list reaches) and
tests/test_gpu_mine.py."""
import itertools

import numpy as np
import torch

# the shapes of test_gpu_mine.py::test_valid_global_top_m
GPU_N = (2, 5, 127, 128, 129, 300)
GPU_KD = ((1, 8), (3, 40), (8, 64), (2, 96), (2, 128))
GPU_T = (1, 2)
GPU_CASES = list(itertools.product(GPU_N, GPU_KD, GPU_T))


def gpu_m_values(N):
    """m = 1, 7, 1,000 and more than all candidates"""
    return (1, 7, 1000, N * (N - 1) // 2 + 5)


def select_top(S, m, excluded=None, min_logit=-np.inf):
    """The selection dl_score_mine specifies, made from a matrix of logits S [N,N] (any float dtype, S[u,v] for u < v is
    what counts): candidates are the pairs u < v with excluded[u,v] false (the caller symmetrises), a logit that is not NaN
    and >= min_logit; the first m of them by larger logit first (+inf above everything finite, -0 equal to +0), equal
    logits by u * N + v, the smaller first.  -> (src, dst, logit) int64, int64, S.dtype."""
    N = S.shape[0]
    ok = torch.triu(torch.ones(N, N, dtype=torch.bool, device=S.device), 1)
    if excluded is not None:
        ok &= ~excluded.to(S.device).bool()
    ok &= ~torch.isnan(S) & (S >= min_logit)
    u, v = torch.nonzero(ok, as_tuple=True)                      # ascending u * N + v
    val = S[u, v]
    val = torch.where(val == 0, torch.zeros_like(val), val)     # -0 ranks as +0
    order = torch.sort(val, descending=True, stable=True).indices[:m]
    return u[order], v[order], S[u, v][order]


def logits64(Z, H, t):
    """fp64 s(u, v) = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t) for all pairs, and test_gpu_rank.py::logits64's error
    band 1e-5 * sum_k exp(z.z / t) (|h|.|h| + |h.h| |z|.|z| / t)."""
    Zd, Hd = Z.double(), H.double()
    zz = torch.einsum("qkd,nkd->qnk", Zd, Zd)
    hh = torch.einsum("qkd,nkd->qnk", Hd, Hd)
    za = torch.einsum("qkd,nkd->qnk", Zd.abs(), Zd.abs())
    ha = torch.einsum("qkd,nkd->qnk", Hd.abs(), Hd.abs())
    e = torch.exp(zz / t)
    return (hh * e).sum(-1), 1e-5 * (e * (ha + hh.abs() * za / t)).sum(-1)


def mine64(Z, H, t, ex, min_logit, m):
    """fp64 reference of ops.score_mine: ex = None or a bool [N,N] mask of excluded pairs (either orientation)."""
    S, _ = logits64(Z, H, t)
    if ex is not None:
        ex = ex.bool() | ex.bool().T
    return select_top(S, m, ex, min_logit)
