"""What the pairwise ranking trainer (dl_score_sampled_bpr_train) is checked against.  TEST INFRASTRUCTURE: torch on the CPU.

Edge row r = (src[r], dst[r]) with m entries e = r m + j and partners k[e] (-1: a failed draw, no term):

  x(a, b)   = sum_f (h_f[a].h_f[b]) exp(z_f[a].z_f[b] / t)                       (ref64.logit64)
  delta_rj  = x(src[r], k[r m + j]) - x(src[r], dst[r])
  loss      = sum_{live} w softplus(delta)        g_rj = w sigma(delta_rj)       G_r = sum_j g_rj
  d loss / d x-_rj = g_rj                         d loss / d x+_r = -G_r

`step64` is that in fp64 (softplus by logit_ref.softplus64; dZ, dH by autograd of the two logit lists with the coefficients
above); `step32` restates it in fp32: fp32 tables and logits, delta TAKEN IN FP32, g by the kernels' form of the sigmoid
(logit_ref.sigmoid_minus_label32), G_r SUMMED IN FP32 — so the bound carries the cancellation of x- - x+.  `bound` is the
project's rule: 4 x the error of the fp32 restatement against fp64, measured on the caller's own cases, with the figures of
sample_ref.figures: ref64.row_ratio for gradients, relative error for the loss, relative error with a median floor for scores.
"""
from __future__ import annotations

import numpy as np
import torch

import logit_ref
import ref64

F64 = torch.float64


def triples(src, dst, m: int, k):
    """-> (src, dst int64 [n_rows], pu, pk int64 [L], row int64 [L], live bool [E]): the positives, and the entries with k >= 0
    listed in entry order with the edge row each belongs to."""
    src, dst = torch.as_tensor(np.asarray(src), dtype=torch.int64), torch.as_tensor(np.asarray(dst), dtype=torch.int64)
    k = torch.as_tensor(np.asarray(k), dtype=torch.int64)
    assert k.numel() == src.numel() * m and dst.numel() == src.numel()
    live = k >= 0
    row = torch.arange(k.numel()) // m
    return src, dst, src[row[live]], k[live], row[live], live


def loss64(xp, xn, row, w: float):
    """The written-out loss in fp64: sum w softplus(x- - x+[row])."""
    return (float(w) * logit_ref.softplus64(xn - xp[row])).sum()


def step64(Z, H, src, dst, m: int, k, t: float, w: float):
    """-> (pos64 [n_rows], neg64 [L], loss, dZ, dH) in fp64."""
    src, dst, pu, pk, row, _live = triples(src, dst, m, k)
    Zr, Hr = Z.detach().to(F64).clone().requires_grad_(True), H.detach().to(F64).clone().requires_grad_(True)
    xp, xn = ref64.logit64(Zr, Hr, src, dst, t), ref64.logit64(Zr, Hr, pu, pk, t)
    delta = (xn - xp[row]).detach()
    g = float(w) * torch.sigmoid(delta)
    G = torch.zeros(src.numel(), dtype=F64).index_add_(0, row, g)
    dZ, dH = torch.autograd.grad([xn, xp], (Zr, Hr), [g, -G])
    return xp.detach(), xn.detach(), float(loss64(xp.detach(), xn.detach(), row, w)), dZ, dH


def step32(Z, H, src, dst, m: int, k, t: float, w: float):
    """step64 restated in fp32 on ONE thread (the backward of a gather adds rows in thread order: one order for a recorded
    figure): fp32 logits, delta and G_r in fp32, the loss by the loss kernel's formula summed in fp32 by torch."""
    src, dst, pu, pk, row, _live = triples(src, dst, m, k)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        Zr, Hr = Z.float().requires_grad_(True), H.float().requires_grad_(True)
        xp, xn = ref64.logit64(Zr, Hr, src, dst, float(t)), ref64.logit64(Zr, Hr, pu, pk, float(t))
        delta = (xn - xp[row]).detach()                              # fp32
        wv = torch.tensor(float(w), dtype=torch.float32)
        g = wv * logit_ref.sigmoid_minus_label32(delta, torch.zeros_like(delta))
        G = torch.zeros(src.numel(), dtype=torch.float32).index_add_(0, row, g)
        loss = (wv * (delta.clamp(min=0) + torch.log1p(torch.exp(-delta.abs())))).sum()
        dZ, dH = torch.autograd.grad([xn, xp], (Zr, Hr), [g, -G])
    finally:
        torch.set_num_threads(threads)
    return xp.detach(), xn.detach(), float(loss), dZ, dH


def _score_fig(got, ref) -> float:
    ref, got = ref.double(), torch.as_tensor(got).double()
    if ref.numel() == 0:
        return 0.0
    floor = ref.abs().median().clamp_min(1e-300)
    return float(((got - ref).abs() / torch.maximum(ref.abs(), floor)).max())


def figures(ref, got):
    """{"pos", "neg", "loss", "dZ", "dH"} of (pos, neg_live, loss, dZ, dH) `got` against the fp64 `ref`."""
    return {"pos": _score_fig(got[0], ref[0]), "neg": _score_fig(got[1], ref[1]),
            "loss": abs(float(got[2]) - ref[2]) / abs(ref[2]),
            "dZ": ref64.row_ratio(got[3], ref[3]), "dH": ref64.row_ratio(got[4], ref[4])}


def bound(Z, H, src, dst, m: int, k, t: float, w: float):
    """-> (the fp64 tuple, the fp32 restatement's figures against it); the bound is 4 x the figures."""
    ref = step64(Z, H, src, dst, m, k, t, w)
    return ref, figures(ref, step32(Z, H, src, dst, m, k, t, w))
