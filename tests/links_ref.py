"""Reference of the thresholded link graph (ops.score_links / dl_score_links_count + dl_score_links_fill) and the case list
of its GPU test, shared by tests/test_links_cpu.py (which checks the reference itself and the seeds of the case list) and
tests/test_gpu_links.py."""
import itertools

import numpy as np
import torch

import mine_ref

# the shapes of test_gpu_links.py: a single diagonal tile (1, 2, 5, 127, 128), a second tile of one row (129), three tiles
# with off-diagonal tile pairs and a 44-row tail (300)
GPU_N = (1, 2, 5, 127, 128, 129, 300)
GPU_KD = mine_ref.GPU_KD
GPU_T = (1, 2)
GPU_CASES = list(itertools.product(GPU_N, GPU_KD, GPU_T))


# min_prob per golden case (tests/golden/case_*.npz, the reference model's own link_pred): both sides of the threshold are
# populated wherever the fixture allows it — k16_d128 and k5_d64 are saturated (link_pred = 1 within its tolerance for nearly
# every pair, so no p separates them and they check the all-pairs side) — and at most 1 % of the candidates lie within
# test_gpu_parity.py's tolerance for link_pred of p (golden_doubt; test_links_cpu.py confirms the cap on the fixtures)
GOLDEN_P = {"k16_d128": 0.999, "k3_d8_hub": 0.99, "k4_d32": 0.99, "k4_d8": 0.99, "k5_d64": 0.999, "k8_d32": 0.99,
            "k8_d64": 0.999, "k8_d8_t2": 0.9, "tiny_k1": 0.5, "tiny_k3": 0.9}


def golden_doubt(link_pred, p):
    """pairs whose reference probability lies within rtol = atol = 1e-5 (test_gpu_parity.py, link_pred) of the threshold p"""
    return np.abs(link_pred.astype(np.float64) - p) <= 1e-5 + 1e-5 * np.abs(link_pred)


def case_seed(N, K, d, t):
    """the seeds of test_gpu_mine.py::test_valid_global_top_m"""
    return N * 131 + K * 7 + d + t


def tables(N, K, d, seed=0, scale=1.0, device="cpu"):
    """test_gpu_mine.py's tables: drawn on the CPU, the same numbers on every device"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (torch.randn(N, K, d, generator=g) * scale / d ** 0.5).to(device)
    H = (torch.randn(N, K, d, generator=g) / d ** 0.5).to(device)
    return Z, H


def select_links(S, excluded=None, min_logit=-np.inf):
    """The selection dl_score_links specifies, made from a matrix of logits S [N,N] (any float dtype; S[u,v] for u < v is
    what counts): a pair u < v is eligible iff neither excluded[u,v] nor excluded[v,u] is set, its logit is not NaN and is
    >= min_logit (-0 reaches a floor of 0).  -> (rowptr int64 [N+1], col int64 [nnz], logit S.dtype [nnz]), the symmetric
    CSR over all N nodes: every eligible pair as (u, v) and as (v, u) with the logit S[u,v] (-0 reported as +0), columns
    ascending within a row.  The conventions are mine_ref.select_top's."""
    N = S.shape[0]
    upper = torch.triu(torch.ones(N, N, dtype=torch.bool, device=S.device), 1)
    ok = upper.clone()
    if excluded is not None:
        ex = excluded.to(S.device).bool()
        ok &= ~(ex | ex.T)
    ok &= ~torch.isnan(S) & (S >= min_logit)
    val = torch.where(S == 0, torch.zeros_like(S), S)              # -0 is reported as +0
    both = ok | ok.T
    sym = torch.where(upper, val, val.T)
    rows, cols = torch.nonzero(both, as_tuple=True)                # row-major: ascending columns within a row
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=S.device)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), dim=0)
    return rowptr, cols, sym[rows, cols]


def upper_pairs(rowptr, col, *values):
    """(src, dst, *values) of the CSR's entries with src < dst, in ascending src * N + dst order"""
    N = rowptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(N, device=rowptr.device), rowptr[1:] - rowptr[:-1])
    keep = rows < col.long()
    return (rows[keep], col.long()[keep]) + tuple(v[keep] for v in values)


def workspace_bytes(N, K, form):
    """dl_score_links_workspace_bytes from the plan of dl_score_links_form: the three bf16 planes of Z and of H (rows padded
    to 128-row tiles, columns to 32-column chunks), cnt (4 bytes per cell), the degrees (4 bytes per node), each rounded up
    to 256 bytes, and 256 bytes to align the caller's pointer"""
    up = lambda b: (b + 255) // 256 * 256
    planes = 2 * K * 3 * (form["tiles"] * 128) * (form["nd"] * 32)
    return 2 * up(planes) + up(4 * form["cells"]) + up(4 * N) + 256
