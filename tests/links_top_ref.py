"""Reference of the budgeted link graph (ops.score_top_links / dl_score_links_top_count + dl_score_links_top_fill) and the
case list of its GPU test, shared by tests/test_links_top_cpu.py (which checks the reference itself and the budgets chosen
for the golden fixtures) and tests/test_gpu_links_top.py."""
import numpy as np
import torch

import links_ref
import mine_ref

# the shapes of test_gpu_links.py, with the budgets of test_gpu_mine.py and one in the middle of the candidates
GPU_CASES = links_ref.GPU_CASES


def gpu_m_values(N):
    """m = 1, 7, 1,000, more than all candidates, and half of the pairs"""
    return tuple(dict.fromkeys(mine_ref.gpu_m_values(N) + (max(1, N * (N - 1) // 4),)))


# beyond the cap of the mining (65,536): the smallest round N with more pairs than that, two budgets above the cap
BIG_N, BIG_KD, BIG_M = 400, ((1, 8), (3, 40)), (65537, 70000)
assert BIG_N * (BIG_N - 1) // 2 == 79800 > 65536

# m per golden case (tests/golden/case_*.npz, the reference model's own link_pred).  With p* the m-th largest reference
# probability among the candidates, the pairs within test_gpu_parity.py's tolerance for link_pred of p* may fall on either
# side of the cut; m is chosen so that they are at most 1 % of the candidates — or one pair, the m-th itself, which always
# lies in its own band (the floor of test_gpu_links.py::test_against_fp64's cap) — with and without the fixture's edges as
# candidates (test_links_top_cpu.py confirms it on the fixtures).  k16_d128 and k5_d64 are saturated: link_pred = 1 within
# the tolerance for nearly every pair, no m meets the cap, and they check the count and the layout only.
GOLDEN_M = {"k16_d128": 100, "k3_d8_hub": 300, "k4_d32": 310, "k4_d8": 290, "k5_d64": 200, "k8_d32": 500, "k8_d64": 400,
            "k8_d8_t2": 880, "tiny_k1": 6, "tiny_k3": 20}
GOLDEN_SATURATED = ("k16_d128", "k5_d64")


def golden_cut(link_pred, cand, m):
    """(p*, doubt): the m-th largest reference probability among the candidates ``cand`` (a bool [N,N] mask of pairs u < v)
    and the candidates within rtol = atol = 1e-5 of it (links_ref.golden_doubt)"""
    x = np.sort(link_pred[cand].astype(np.float64))[::-1]
    p = float(x[min(m, x.size) - 1])
    return p, links_ref.golden_doubt(link_pred, p) & cand


def doubt_cap(n_candidates):
    return max(1, int(0.01 * n_candidates))


def chosen_pairs(S, m, excluded=None, min_logit=-np.inf):
    """bool [N,N], upper triangle: the set mine_ref.select_top chooses (``excluded`` in either orientation)"""
    N = S.shape[0]
    ex = None
    if excluded is not None:
        ex = excluded.to(S.device).bool()
        ex = ex | ex.T
    u, v, _ = mine_ref.select_top(S, m, ex, min_logit)
    keep = torch.zeros(N, N, dtype=torch.bool, device=S.device)
    keep[u, v] = True
    return keep


def select_top_links(S, m, excluded=None, min_logit=-np.inf):
    """The selection dl_score_links_top specifies, made from a matrix of logits S [N,N]: the set of mine_ref.select_top (the
    first m candidates by larger logit, equal logits by u * N + v) as the CSR of links_ref.select_links restricted to it
    -> (rowptr int64 [N+1], col int64 [nnz], logit S.dtype [nnz]), nnz = 2 min(m, candidates)."""
    keep = chosen_pairs(S, m, excluded, min_logit)
    return links_ref.select_links(S, ~(keep | keep.T), -np.inf)
