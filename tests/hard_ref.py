"""What the hard-negative sampler (dl_sample_negatives_hard) is checked against.  TEST INFRASTRUCTURE: numpy and torch on the CPU.

The rule, restated.  Entry e = r m + j has the source u = src[r] and c candidates.  Candidate i is the draw of
dl_sample_negatives (sample_ref.sample) with the Philox counter (e, i 64 + attempt, epoch low, epoch high) and the seed as key:
k = (word 0 * N) >> 32, at most 64 attempts, rejected while k stands in the exclusion row of u (or k == u with exclude_self); a
candidate that spends its attempts is dead (-1), as is every candidate of a u outside [0, N).  Kept: the live candidate with the
largest logit x(u, k) = sum_f (h_f[u].h_f[k]) exp(z_f[u].z_f[k] / t) (ref64.logit64), ties to the lowest i, a NaN below every
number, -inf included (all NaN: the first live candidate); no live candidate: k = -1, one failed ENTRY.

`candidates` draws, `logits` scores (fp64, or the same formula restated in fp32), `select` keeps.  `tolerance` is the project's
rule — 4 x the error of the fp32 restatement against fp64, with the figure of sample_ref.figures for scores — and `decisive`
marks the entries whose fp64 argmax any fp32 evaluation within that tolerance must reproduce.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import ref64
import sample_ref as sr

MAX_CANDIDATES = 64
# the inputs of tests/test_gpu_hard.py (the CPU tests check the reference itself on the same ones): the lists of
# tests/test_gpu_sample.py under sample_ref.exclusion_graph(), the shapes of tests/test_gpu_bpr.py
SHAPES = ((8, 64), (4, 64), (3, 20), (4, 32))
TEMPS = (1.0, 2.0)
MC = ((3, 4), (3, 3), (3, 5), (1, 16), (1, 64))       # (m, c): c dividing 64 and not, a whole wave per entry
SEED, EPOCH = 1, 7
MAX_NON_DECISIVE = 0.01


@functools.lru_cache(maxsize=None)
def _candidates(src: tuple, m: int, N: int, ex: tuple, seed: int, epoch: int, c: int, exclude_self: bool):
    src = np.asarray(src, dtype=np.int64)
    E = src.size * m
    cand = np.full((E, c), -1, dtype=np.int32)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    rows = [set(r) for r in ex] if ex else [set() for _ in range(N)]
    u_of = np.repeat(src, m)
    ok_u = (u_of >= 0) & (u_of < N)
    ee, ii = np.meshgrid(np.arange(E), np.arange(c), indexing="ij")
    todo_e, todo_i = ee[ok_u].reshape(-1), ii[ok_u].reshape(-1)
    for attempt in range(sr.ATTEMPTS):
        if todo_e.size == 0:
            break
        ctr1 = (todo_i * sr.ATTEMPTS + attempt).astype(object)
        words = sr.philox((todo_e.astype(object), ctr1, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF), key)[..., 0]
        k = np.array([(int(w) * N) >> 32 for w in words], dtype=np.int64)
        u = u_of[todo_e]
        ok = np.array([(b not in rows[a]) and not (exclude_self and b == a) for b, a in zip(k.tolist(), u.tolist())], dtype=bool)
        cand[todo_e[ok], todo_i[ok]] = k[ok]
        todo_e, todo_i = todo_e[~ok], todo_i[~ok]
    cand.setflags(write=False)
    return cand


def candidates(src, m: int, N: int, ex_rowptr, ex_col, seed: int, epoch: int, c: int, exclude_self: bool = False):
    """-> int32 [len(src) m, c]: candidate i of every entry, -1 = dead.  Column 0 is sample_ref.sample's k."""
    assert 1 <= c <= MAX_CANDIDATES
    ex = () if ex_rowptr is None else tuple(tuple(int(v) for v in ex_col[ex_rowptr[n]:ex_rowptr[n + 1]]) for n in range(N))
    return _candidates(tuple(int(v) for v in src), int(m), int(N), ex, int(seed), int(epoch), int(c), bool(exclude_self))


def logits(Z, H, src, m: int, cand, t: float, dtype=torch.float64):
    """-> [E, c] tensor of `dtype`: x(u_e, cand[e, i]) by ref64.logit64 on the tables cast to `dtype`; 0 where the candidate is dead."""
    cand = np.asarray(cand)
    E, c = cand.shape
    live = torch.from_numpy(cand >= 0)
    u = torch.from_numpy(np.repeat(np.asarray(src, dtype=np.int64), m))[:, None].expand(E, c)[live]
    k = torch.from_numpy(cand.astype(np.int64))[live]
    out = torch.zeros(E, c, dtype=dtype)
    if k.numel():
        out[live] = ref64.logit64(Z.to(dtype), H.to(dtype), u, k, float(t))
    return out


def select(cand, x):
    """-> (k int32 [E], which int64 [E], n_failed): the rule's choice on the logits x [E, c]; which = the candidate index, -1."""
    cand, x = np.asarray(cand), np.asarray(x, dtype=np.float64)
    E, c = cand.shape
    k, which = np.full(E, -1, dtype=np.int32), np.full(E, -1, dtype=np.int64)
    for e in range(E):
        best = -1
        for i in range(c):
            if cand[e, i] < 0:
                continue
            if best < 0 or x[e, i] > x[e, best] or (np.isnan(x[e, best]) and not np.isnan(x[e, i])):
                best = i
        if best >= 0:
            k[e], which[e] = cand[e, best], best
    return k, which, int((k < 0).sum())


def score_figure(got, ref, live) -> float:
    """The largest |got - ref| / max(|ref|, the median |ref|) over the live candidates (sample_ref.figures' score figure)."""
    live = torch.as_tensor(np.asarray(live))
    ref, got = torch.as_tensor(ref).double()[live], torch.as_tensor(got).double()[live]
    if ref.numel() == 0:
        return 0.0
    floor = ref.abs().median().clamp_min(1e-300)
    return float(((got - ref).abs() / torch.maximum(ref.abs(), floor)).max())


def tolerance(Z, H, src, m: int, cand, t: float):
    """-> (x64 [E, c], tol, fp32 figure): tol = 4 x the error of the fp32 restatement of these logits against fp64."""
    x64 = logits(Z, H, src, m, cand, t)
    fig = score_figure(logits(Z, H, src, m, cand, t, torch.float32), x64, np.asarray(cand) >= 0)
    return x64, 4.0 * fig, fig


def decisive(cand, x64, tol: float):
    """-> (decisive bool [E], node int32 [E]): node = the fp64 choice; an entry is decisive when the logits of its best and of
    its best OTHER node differ by more than `tol`, relative to max(|best|, the median |x| of the live candidates with a finite
    logit) — or when it has no other node; a +inf best is decisive against anything smaller, a NaN among the others ranks below
    every number (it is no matter of rounding).  Entries without a live candidate are not decisive (node -1)."""
    cand, x = np.asarray(cand), np.asarray(x64, dtype=np.float64)
    live = cand >= 0
    finite = live & np.isfinite(x)
    median = float(np.median(np.abs(x[finite]))) if finite.any() else 0.0
    node, which, _failed = select(cand, x)
    out = np.zeros(cand.shape[0], dtype=bool)
    for e in np.flatnonzero(node >= 0):
        other = live[e] & (cand[e] != node[e])
        if not other.any():
            out[e] = True
            continue
        best = x[e, which[e]]
        numbers = x[e][other][~np.isnan(x[e][other])]
        if numbers.size == 0:                                         # every other node scores NaN: below any number
            out[e] = not np.isnan(best)
            continue
        second = np.max(numbers)
        if np.isposinf(best):
            out[e] = second < best
        else:
            out[e] = (best - second) > tol * max(abs(best), median)   # (a NaN best: False)
    return out, node


def non_decisive_share(cand, x64, tol: float) -> float:
    """The share of the entries with a live candidate that are not decisive."""
    dec, node = decisive(cand, x64, tol)
    n_live = int((node >= 0).sum())
    return 0.0 if n_live == 0 else float(((node >= 0) & ~dec).sum()) / n_live
