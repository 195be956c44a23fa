"""Reference of the global rank counts of target pairs among all unordered pairs of a graph (ops.score_pair_ranks /
dl_score_pair_ranks), written from the contract on ANY matrix of logits, and the case lists of its GPU test; shared by
tests/test_pair_ranks_cpu.py (which checks the reference itself and what the case lists reach) and
tests/test_gpu_pair_ranks.py."""
import torch

import mine_ref

# test_gpu_pair_ranks.py: the enumerated cases are the mining's, the geometry case forces the run length of a workgroup
GPU_CASES = mine_ref.GPU_CASES
GEOMETRY = dict(N=700, K=3, d=40, tiles=(1, 4, 21))                  # 6 tiles = 21 tile pairs: one, a few, all per workgroup
EDGE_PAIRS = ((0, 1), (0, -1), (126, 127), (127, 128), (128, 129), (-2, -1))      # negative: from N


def above(c, x):
    """c ranks strictly above x by value: larger first, NaN below everything"""
    return torch.where(torch.isnan(x), ~torch.isnan(c), c > x)


def equal(c, x):
    """-0 equals +0, inf equals inf, NaN equals NaN only"""
    return (c == x) | (torch.isnan(c) & torch.isnan(x))


def candidates(N, excluded=None, device="cpu"):
    """bool [N,N]: the unordered pairs u < v outside the exclusion set (a mask read in either orientation)"""
    cand = torch.triu(torch.ones(N, N, dtype=torch.bool, device=device), 1)
    if excluded is not None:
        ex = excluded.to(device).bool()
        cand &= ~(ex | ex.T)
    return cand


def pair_ranks(S, src, dst, excluded=None):
    """-> (greater, ties, n_others) int64 [T] for the unordered target pairs {src[i], dst[i]}: S[u, v] for u < v is the
    logit of pair {u, v}; candidates are the pairs u < v outside ``excluded``; target i = S[min, max] is ranked whether or
    not it is excluded; greater / ties count the candidates OTHER than the target pair itself strictly above / equal to it
    by value; n_others = candidates - [the target is one]."""
    N = S.shape[0]
    src, dst = torch.as_tensor(src).reshape(-1).long(), torch.as_tensor(dst).reshape(-1).long()
    assert src.numel() == dst.numel() and not bool((src == dst).any())
    cand = candidates(N, excluded, S.device)
    cu, cv = torch.nonzero(cand, as_tuple=True)
    cval = S[cu, cv]
    lo, hi = torch.minimum(src, dst).to(S.device), torch.maximum(src, dst).to(S.device)
    T = lo.numel()
    if T == 0:
        e = torch.zeros(0, dtype=torch.int64)
        return e, e.clone(), e.clone()
    x = S[lo, hi]
    other = ~((cu[None, :] == lo[:, None]) & (cv[None, :] == hi[:, None]))          # [T, |C|]: not the target pair itself
    greater = (above(cval[None, :], x[:, None]) & other).sum(1)
    ties = (equal(cval[None, :], x[:, None]) & other).sum(1)
    return greater.cpu(), ties.cpu(), other.sum(1).cpu()


def order_key(x):
    """int64 order keys of fp32 values: the device's total order (NaN -> 0, -0 as +0, larger value = larger key)"""
    x = x.float()
    z = torch.where(x == 0, torch.zeros_like(x), x)
    b = z.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b + 0x80000000)
    return torch.where(torch.isnan(x), torch.zeros_like(key), key)


def counts_from_list(list_logit, n_nan, tgt_logit, tgt_in_c):
    """Expected (greater, ties) of targets from an enumeration of the candidates: ``list_logit`` holds the logit of EVERY
    non-NaN candidate (ops.score_mine with m = all), ``n_nan`` the number of NaN candidates; integer comparisons of order
    keys only.  ``tgt_in_c`` [T] bool: the target is itself among the candidates (counted once among its ties)."""
    ck = torch.sort(order_key(list_logit)).values
    tk = order_key(tgt_logit)
    ge = ck.numel() - torch.searchsorted(ck, tk, right=False)          # candidates with key >= the target's
    gt = ck.numel() - torch.searchsorted(ck, tk, right=True)
    nan = tk == 0
    greater = torch.where(nan, torch.full_like(gt, ck.numel()), gt)
    ties = torch.where(nan, torch.full_like(gt, int(n_nan)), ge - gt) - tgt_in_c.to(torch.int64)
    return greater, ties


def targets_for(N, seed, n=200):
    """The targets of the enumerated GPU test: every pair for N <= 5, else ``n`` seeded pairs and the tile-edge pairs that
    exist; some repeated, every third given in the other orientation.  -> (src, dst) int64 CPU tensors, src != dst."""
    if N <= 5:
        u, v = torch.triu_indices(N, N, 1)
    else:
        g = torch.Generator().manual_seed(seed)
        u = torch.randint(0, N, (n,), generator=g)
        v = (u + 1 + torch.randint(0, N - 1, (n,), generator=g)) % N
        edge = [(a % N, b % N) for a, b in EDGE_PAIRS if max(a, b) < N and a % N != b % N]
        u = torch.cat([u, torch.tensor([a for a, _ in edge], dtype=torch.int64)])
        v = torch.cat([v, torch.tensor([b for _, b in edge], dtype=torch.int64)])
    u, v = torch.cat([u, u[:7]]), torch.cat([v, v[:7]])                 # duplicates of a target
    flip = torch.arange(u.numel()) % 3 == 1
    return torch.where(flip, v, u), torch.where(flip, u, v)
