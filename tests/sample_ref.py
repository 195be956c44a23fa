"""What the device sampler and the sampled trainer are checked against.  TEST INFRASTRUCTURE: numpy and torch on the CPU.

Sampler: Philox-N x W with 10 rounds in numpy (`philox`, W = 32 is the kernel's, W = 64 is numpy's own generator and exists
here so that the SAME round function can be checked against ``numpy.random.Philox``) and the rule of dl_sample_negatives
(`sample`): counter (e, attempt, epoch low, epoch high), key (seed low, seed high), k = (word 0 * N) >> 32, at most 64 attempts,
reject k in the exclusion row of src[e // m] (and k == src with exclude_self), -1 once the attempts are spent.

Trainer: the loss of the sampled negatives and its gradients in fp64 (`step64`) and restated in fp32 (`step32`) on a LISTED
copy of the entries (u_e, k_e) — label 0, one weight, entries with k = -1 dropped — from the pieces of ref64 / logit_ref /
label_weight_ref; `bound` is the project's rule, 4 x the error of the fp32 restatement against fp64, measured where it is used.
"""
from __future__ import annotations

import numpy as np
import torch

import label_weight_ref as lw
import logit_ref
import ref64

ATTEMPTS = 64
_CONST = {32: (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85),
          64: (0xD2E7470EE14C6C93, 0xCA5A826395121157, 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B)}


def philox(ctr, key, W: int = 32):
    """Philox4xW-10: ctr [..., 4], key [..., 2] (python ints or arrays, broadcast) -> [..., 4] uint64 words below 2^W."""
    m0, m1, w0, w1 = _CONST[W]
    mask = (1 << W) - 1
    c = [np.asarray(ctr[..., i], dtype=object) for i in range(4)] if isinstance(ctr, np.ndarray) else [np.asarray(v, dtype=object) for v in ctr]
    k = [np.asarray(v, dtype=object) for v in key]
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [((p1 >> W) ^ c[1] ^ k[0]) & mask, p1 & mask, ((p0 >> W) ^ c[3] ^ k[1]) & mask, p0 & mask]
        k = [(k[0] + w0) & mask, (k[1] + w1) & mask]
    return np.stack([np.asarray(v, dtype=object) for v in np.broadcast_arrays(*c)], axis=-1)


def exclusion_graph(N: int = 70, seed: int = 3):
    """-> (N, rowptr int32, col int32, rows): an exclusion CSR with an EMPTY row (node 0), a row that excludes 68 of the 70
    nodes (node 1: many rejections), a row that excludes ALL nodes (node 2: every draw fails) and 1 .. 11 columns elsewhere."""
    rng = np.random.default_rng(seed)
    rows = [[] for _ in range(N)]
    rows[1] = sorted(rng.choice(N, N - 2, replace=False).tolist())
    rows[2] = list(range(N))
    for n in range(3, N):
        rows[n] = sorted(rng.choice(N, int(rng.integers(1, 12)), replace=False).tolist())
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    return N, rowptr, col, rows


def sample(src, m: int, N: int, ex_rowptr, ex_col, seed: int, epoch: int, exclude_self: bool = False, entries=None):
    """-> (k int32 [len(src) m], n_failed): dl_sample_negatives on the CPU.  ``entries``: draw these entries only (the others
    stay -1 and are not counted): an entry's draw depends on nothing but (seed, epoch, e)."""
    src = np.asarray(src, dtype=np.int64)
    E = src.size * m
    k = np.full(E, -1, dtype=np.int32)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    rows = [set() for _ in range(N)] if ex_rowptr is None else \
        [set(int(c) for c in ex_col[ex_rowptr[n]:ex_rowptr[n + 1]]) for n in range(N)]
    todo = np.arange(E) if entries is None else np.asarray(entries, dtype=np.int64)
    for attempt in range(ATTEMPTS):
        if todo.size == 0:
            break
        words = philox((todo.astype(object), attempt, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF), key)[..., 0]
        cand = np.array([(int(w) * N) >> 32 for w in words], dtype=np.int64)
        u = src[todo // m]
        ok = np.array([(c not in rows[a]) and not (exclude_self and c == a) for c, a in zip(cand.tolist(), u.tolist())], dtype=bool)
        k[todo[ok]] = cand[ok]
        todo = todo[~ok]
    return k, int(todo.size)


def listed(src, m: int, k):
    """(pu, pv) int64 tensors of the entries with k >= 0, in entry order."""
    u = np.repeat(np.asarray(src, dtype=np.int64), m)
    k = np.asarray(k, dtype=np.int64)
    live = k >= 0
    return torch.from_numpy(u[live]), torch.from_numpy(k[live]), live


def step64(Z, H, pu, pv, t: float, w: float, space: str):
    """-> score64 [P], loss, dZ, dH in fp64 for label 0 and weight w on every listed pair: probability space by
    label_weight_ref.prob_step64 (the coefficient at the fp32 probability, as the kernels and dl_pair_bce have it), logit space
    by logit_ref.step64."""
    y = torch.zeros(pu.numel(), dtype=torch.float64)
    wv = torch.full((pu.numel(),), float(w), dtype=torch.float64)
    if space == "logit":
        x, loss, _g, dZ, dH = logit_ref.step64(Z, H, pu, pv, t, y, wv)
        return x, float(loss), dZ, dH
    x, p32, _g, dZ, dH = lw.prob_step64(Z, H, pu, pv, t, y, wv)
    return p32, float((wv * lw.prob_loss_terms64(p32, y)).sum()), dZ, dH


def step32(Z, H, pu, pv, t: float, w: float, space: str):
    """The same step restated in fp32 (logit_ref.step32 / label_weight_ref.prob_step32) -> score32, loss32, dZ32, dH32."""
    y = torch.zeros(pu.numel(), dtype=torch.float64)
    wv = torch.full((pu.numel(),), float(w), dtype=torch.float64)
    if space == "logit":
        x, loss, _g, dZ, dH = logit_ref.step32(Z, H, pu, pv, t, y, wv)
        return x, float(loss), dZ, dH
    _x, p, loss, _g, dZ, dH = lw.prob_step32(Z, H, pu, pv, t, y, wv)
    return p, float(loss), dZ, dH


def figures(ref, got):
    """{"dZ", "dH", "loss", "score"} of (score, loss, dZ, dH) `got` against the fp64 `ref`: ref64.row_ratio for the gradients,
    relative error for the loss, the largest |difference| / max(|ref|, the median |ref|) for the scores."""
    s_ref, s_got = ref[0].double(), torch.as_tensor(got[0]).double()
    floor = s_ref.abs().median().clamp_min(1e-300)
    return {"dZ": ref64.row_ratio(got[2], ref[2]), "dH": ref64.row_ratio(got[3], ref[3]),
            "loss": abs(float(got[1]) - ref[1]) / abs(ref[1]),
            "score": float(((s_got - s_ref).abs() / torch.maximum(s_ref.abs(), floor)).max())}


def bound(Z, H, pu, pv, t: float, w: float, space: str):
    """-> (ref64 tuple, {"dZ", "dH", "loss", "score"} bounds): 4 x the error of the fp32 restatement against fp64 on exactly
    these sums (ref64's rule and its reason: another equally valid fp32 summation order and a hardware exp)."""
    ref = step64(Z, H, pu, pv, t, w, space)
    fp32 = figures(ref, step32(Z, H, pu, pv, t, w, space))
    return ref, {name: 4.0 * v for name, v in fp32.items()}, fp32
