"""What the tests of the per-factor terms (dl_score_pair_terms, ops.score_pair_terms, Disentangle.explain_links, --explain)
share: the numpy restatement of ``PairTerms.contrib`` / ``.factor``, the derived tables whose ``ops.score_pair_logits`` is the
expected value of every cell, and the comparison of bits.

Every expected value is a logit of ``ops.score_pair_logits`` (pinned to fp64 by test_gpu_dense_fp64.py) on tables DERIVED
from the ones under test, so nothing is compared within a tolerance:
  cum[:, k]  the logit of the tables cut to factors 0..k                     (prefix_tables)
  q[:, k]    the logit of factor k alone with Z = 0: e = expf(0) = 1, 0 + q * 1 = q      (gram_tables)
  e[:, k]    the logit of factor k alone with H = a unit vector: h.h = 1, 0 + 1 * e = e   (weight_tables)
"""
import numpy as np
import torch


def contrib(cum: np.ndarray) -> np.ndarray:
    """fp32 [P, K]: column 0 is cum[:, 0], column k is cum[:, k] - cum[:, k-1] (fp32 subtraction)"""
    cum = np.asarray(cum, dtype=np.float32)
    out = cum.copy()
    with np.errstate(invalid="ignore"):
        out[:, 1:] = cum[:, 1:] - cum[:, :-1]
    return out


def factor(cum: np.ndarray) -> np.ndarray:
    """int64 [P]: the first index of the largest contribution of the row, -1 where a contribution is NaN"""
    c = contrib(cum)
    if c.shape[1] == 0:
        return np.full(c.shape[0], -1, np.int64)
    bad = np.isnan(c).any(axis=1)
    best = np.argmax(np.where(np.isnan(c), -np.inf, c), axis=1).astype(np.int64)      # np.argmax: the first of equals
    return np.where(bad, -1, best)


def _canon(x) -> np.ndarray:
    """int32 bits of fp32 values with -0 as +0 and every NaN as one NaN"""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    x = np.where(x == 0, np.float32(0), x)
    x = np.where(np.isnan(x), np.float32("nan"), x).astype(np.float32)
    return np.ascontiguousarray(x).view(np.int32)


def same_bits(a, b) -> bool:
    """the fp32 arrays agree bit for bit (-0 taken as +0, any NaN equal to any NaN); no tolerance"""
    a, b = _canon(a), _canon(b)
    return a.shape == b.shape and bool((a == b).all())


def prefix_tables(Z, H, k):
    return Z[:, :k + 1].contiguous(), H[:, :k + 1].contiguous()


def gram_tables(Z, H, k):
    return torch.zeros_like(Z[:, k:k + 1]).contiguous(), H[:, k:k + 1].contiguous()


def weight_tables(Z, H, k):
    N, _, d = Z.shape
    U = torch.zeros(N, 1, d, dtype=H.dtype, device=H.device)
    U[:, 0, 0] = 1.0
    return Z[:, k:k + 1].contiguous(), U


# (N, K, d, t, n_pairs): n_pairs around the 128-pair tile (its tail, the clamped gather), N from the self pair to three table
# tiles, d with 1..4 chunks of 32 columns, both forms of the division by t
GPU_CASES = [
    (1, 1, 1, 1.0, 1),
    (1, 2, 32, 0.5, 127),
    (2, 2, 32, 0.5, 127),
    (2, 5, 33, 1.0, 128),
    (129, 1, 64, 1.0, 129),
    (129, 2, 33, 1.0, 1),
    (129, 5, 65, 0.5, 300),
    (300, 2, 128, 1.0, 300),
    (300, 5, 64, 0.5, 129),
    (300, 1, 1, 0.5, 128),
]


def case_pairs(N: int, n_pairs: int, seed: int):
    """int64 (a, b) on the CPU: random pairs in either orientation, with a self pair, a repeated pair and the table's corners"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randint(0, N, (n_pairs,), generator=g)
    b = torch.randint(0, N, (n_pairs,), generator=g)
    fixed = [(0, 0), (N - 1, 0), (0, N - 1), (N - 1, N - 1), (N // 2, N // 2)]
    for i, (u, v) in enumerate(fixed[:max(0, n_pairs - 2)]):
        a[i], b[i] = u, v
    if n_pairs >= 2:
        a[-1], b[-1] = a[0], b[0]                                       # a duplicated pair, in the last (partial) tile
    return a, b
