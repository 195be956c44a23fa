"""Plain float64 reference of the hot path (route, normaliser, aggregate, pair scorer) and the inputs it is run on.
TEST INFRASTRUCTURE: torch, float64, CPU.

Written from the formulas alone (the header of oracle/sparse_ref.py; model.py:56-75, 110-113):

  route        e_k = exp(z_k[i].z_k[j] / t), alpha = e / sum_k e, p = argmax_k alpha, a = alpha_p      per edge (i, j)
  normaliser   s_k[i] = sum_{j in N(i), p_ij = k} a_ij ; 0 -> 1
  aggregate    h_k[i] = beta z_k[i] + (1 - beta) sum_{j in N(i), p_ij = k} a_ij / s_k[j] z_k[j]       (s of the NEIGHBOUR)
  score        logit(u, v) = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t),  prob = sigmoid(logit)

There is no hand-derived backward in this file: every gradient is torch.autograd through the forward above, with the
routing index p a constant (argmax carries no gradient).  Each forward has an "absolute-sum companion": the same sum with
every product replaced by its magnitude (and every exp by exp times one plus the magnitude of its argument) — what fp32
rounding of that output scales with.  The bands of tests/test_gpu_hotpath_fp64.py are `c * 2^-24 * companion`.

ORACLE holds the largest errors the fp32 numpy oracle (oracle/sparse_ref.py) shows against this reference on the
cases of `hotpath_cases`, as measured by tests/test_ref64_cpu.py (which measures them again on every run); BOUND is 4x that: a
different but equally valid fp32 summation order and a hardware exp.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24                                                   # fp32 unit roundoff

# -------------------------------------------------------------------------------------------------- the reference


def edge_src(rowptr: torch.Tensor) -> torch.Tensor:
    rowptr = rowptr.long()
    return torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr[1:] - rowptr[:-1])


def alpha64(Z, rowptr, col, t):
    """[E, K] routing softmax of every edge (no max subtraction: model.py:57-60)."""
    src, dst = edge_src(rowptr), col.long()
    e = torch.exp((Z[src] * Z[dst]).sum(-1) / t)
    return e / e.sum(1, keepdim=True)


def forward64(Z, rowptr, col, p, beta, t):
    """-> a [E] (= alpha[e, p_e]), s_raw [N, K] (before zero -> 1), H [N, K, d]."""
    N, K, d = Z.shape
    src, dst, p = edge_src(rowptr), col.long(), p.long()
    a = alpha64(Z, rowptr, col, t).gather(1, p[:, None])[:, 0]
    s_raw = torch.zeros(N, K, dtype=Z.dtype).index_put((src, p), a, accumulate=True)
    return a, s_raw, aggregate64(Z, rowptr, col, p, a, s_raw, beta)


def aggregate64(Z, rowptr, col, p, a, s_raw, beta):
    """H from given routing weights and raw normalisers (what the aggregation kernel is handed)."""
    src, dst, p = edge_src(rowptr), col.long(), p.long()
    s = torch.where(s_raw == 0, torch.ones_like(s_raw), s_raw)
    w = a / s[dst, p]
    acc = torch.zeros_like(Z).index_put((src, p), w[:, None] * Z[dst, p], accumulate=True)
    return beta * Z + (1 - beta) * acc


def logit64(Z, H, pu, pv, t):
    pu, pv = pu.long(), pv.long()
    return ((H[pu] * H[pv]).sum(-1) * torch.exp((Z[pu] * Z[pv]).sum(-1) / t)).sum(-1)


def score_bwd64(Z, H, pu, pv, t, g_prob, prob=None):
    """dZ_score, dH of sum_q g_prob[q] prob[q].  `prob` given: the sigmoid backward is taken at THAT probability
    (g_logit = g_prob prob (1 - prob): the scorer backward is handed the fp32 probabilities of the forward); None:
    autograd through the sigmoid as well."""
    Zr, Hr = Z.detach().clone().requires_grad_(True), H.detach().clone().requires_grad_(True)
    x = logit64(Zr, Hr, pu, pv, t)
    if prob is None:
        loss = (torch.sigmoid(x) * g_prob).sum()
    else:
        loss = (x * (g_prob * prob * (1 - prob))).sum()
    dZ, dH = torch.autograd.grad(loss, (Zr, Hr))
    return dZ, dH


def route_aggregate_bwd64(Z, rowptr, col, p, beta, t, dH):
    """dZ from dH through aggregate -> normaliser -> routing softmax."""
    Zr = Z.detach().clone().requires_grad_(True)
    _a, _s, H = forward64(Zr, rowptr, col, p, beta, t)
    (dZ,) = torch.autograd.grad(H, Zr, dH)
    return dZ


# ---- absolute-sum companions
def route_abs64(Z, rowptr, col, p, t):
    """Companions of a [E] and s_raw [N, K].  a = e_p / sum_k e_k with e_k = exp(x_k): a rounding error dx_k of an
    exponent's argument moves a by a |[k = p] - alpha_k| dx_k, and dx_k scales with sum |z_i| |z_j| / t; the 1 stands
    for the exp, the sum and the division themselves.  s is a sum of positive terms: the sum of their companions."""
    N, K, _d = Z.shape
    src, dst, p = edge_src(rowptr), col.long(), p.long()
    alpha = alpha64(Z, rowptr, col, t)
    xa = (Z[src].abs() * Z[dst].abs()).sum(-1) / t
    onehot = torch.zeros_like(alpha).scatter_(1, p[:, None], 1.0)
    a_abs = alpha.gather(1, p[:, None])[:, 0] * (1 + ((onehot - alpha).abs() * xa).sum(1))
    s_abs = torch.zeros(N, K, dtype=Z.dtype).index_put((src, p), a_abs, accumulate=True)
    return a_abs, s_abs


def aggregate_abs64(Z, rowptr, col, p, a, s_raw, beta):
    return aggregate64(Z.abs(), rowptr, col, p, a, s_raw, beta)


def logit_abs64(Z, H, pu, pv, t):
    """sum_k exp(z.z / t) (|h|.|h| + |h.h| |z|.|z| / t): tests/test_gpu_rank.py's measure."""
    pu, pv = pu.long(), pv.long()
    e = torch.exp((Z[pu] * Z[pv]).sum(-1) / t)
    hh = (H[pu] * H[pv]).sum(-1).abs()
    ha = (H[pu].abs() * H[pv].abs()).sum(-1)
    za = (Z[pu].abs() * Z[pv].abs()).sum(-1)
    return (e * (ha + hh * za / t)).sum(-1)


def sigmoid32(x64):
    """The fp32 probability of an fp64 logit, formed as the oracle and the kernels form it: 1 / (1 + exp(-x)) in fp32
    (exactly 1 from x = 24 ln 2 on, where exp(-x) no longer moves the 1)."""
    x = x64.float()
    return (1.0 / (1.0 + torch.exp(-x))).double()


# ---- the measures of the comparison
def band_ratio(got, ref, companion):
    """max over elements of |got - ref| / (2^-24 companion): the constant c of a forward band."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    err, den = (got - ref).abs(), U * companion
    bad = (den == 0) & (err > 0)
    if bool(bad.any()):
        return math.inf
    return float((err / den.clamp_min(1e-300)).max()) if err.numel() else 0.0


def row_ratio(got, ref):
    """Gradients, per node (one [K, d] block): err_i = max |got_i - ref_i|, scale_i = max(max |ref_i|, the median over the
    non-zero rows of max |ref_j|) -> max_i err_i / scale_i.  The median floor keeps a near-zero row from being judged
    against itself, and no hub sets the scale for anyone else."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    n = ref.shape[0]
    err = (got - ref).abs().reshape(n, -1).max(1).values
    mag = ref.abs().reshape(n, -1).max(1).values
    nz = mag[mag > 0]
    if nz.numel() == 0:
        return 0.0 if float(err.max()) == 0 else math.inf
    return float((err / torch.maximum(mag, nz.median())).max())


def bf16_half_ulp(x_abs):
    """Half a bf16 unit in the last place at magnitude x_abs (8 significant bits): 2^(floor(log2 x) - 8); 0 at 0."""
    _m, e = torch.frexp(x_abs)                                       # x = m 2^e, 0.5 <= m < 1: floor(log2 x) = e - 1
    return torch.where(x_abs > 0, torch.ldexp(torch.ones_like(x_abs), e - 9), torch.zeros_like(x_abs))


def prob_band(x64, logit_band, eps):
    """|sigmoid(x + dx) - sigmoid(x)| <= max sigma' over [x - b, x + b] * b, plus eps for the sigmoid's own rounding."""
    near = torch.clamp(x64.abs() - logit_band, min=0.0)              # the point of the interval closest to 0
    sp = torch.sigmoid(near) * (1 - torch.sigmoid(near))
    return sp * logit_band + eps


# Largest error of the fp32 numpy oracle against this reference over all cases, as measured (three significant digits):
# forward outputs in units of 2^-24 * companion, gradients as row_ratio.  tests/test_ref64_cpu.py measures them again on
# every run and holds them within CPU_SLACK of these figures (another host's numpy may sum in another order); the slack
# is for that re-assertion only and no part of the GPU bounds, which are 4x the figures below.
ORACLE = {
    "a": 3.17, "s": 4.41, "H": 5.07, "logit": 2.54, "prob_eps": 1.51,
    "dZ_score": 6.43e-6, "dH": 2.61e-6, "dZ_route": 1.12e-6,
}
CPU_SLACK = 1.1
BOUND = {k: 4.0 * v for k, v in ORACLE.items()}

# -------------------------------------------------------------------------------------------------- the inputs
LADDER_DEGREES = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 290)
LADDER_PAIRS = (0, 1, 63, 64, 65, 255, 256, 257, 300)              # pairs whose FIRST endpoint is the ladder node
N_POOL = 300
N_NODES = N_POOL + len(LADDER_DEGREES)
MARGIN = 1e-5                                                     # tests/test_gpu_parity.py:_decisive
SATURATED = 15.0
P_ONE = 24 * math.log(2.0)                                        # fp32 sigmoid is exactly 1 from here on

Structure = namedtuple("Structure", "graph pairs rowptr col pu pv ladder pair_ladder isolated dup_pairs")


@functools.lru_cache(maxsize=None)
def structure(seed: int = 2024) -> Structure:
    """One graph and one pair list on N_NODES nodes (CPU plans with the default parameters; .to(device) for the GPU).
    Ladder nodes (scattered over the id range) connect only to distinct pool nodes and have exactly LADDER_DEGREES
    neighbours; nine of them are the first endpoint of exactly LADDER_PAIRS pairs and never a second endpoint."""
    from disenlink_amd.graph import Graph, PairList
    rng = np.random.default_rng(seed)
    ids = rng.permutation(N_NODES)
    pool, ladder = ids[:N_POOL], ids[N_POOL:]
    src, dst = [rng.choice(pool, 420)], [rng.choice(pool, 420)]
    keep = src[0] != dst[0]                                          # the two self-loops are added on purpose below
    src, dst = [src[0][keep]], [dst[0][keep]]
    for node, deg in zip(ladder, LADDER_DEGREES):
        src.append(np.full(deg, node))
        dst.append(rng.choice(pool, deg, replace=False))
    src, dst = np.concatenate(src), np.concatenate(dst)
    dup = rng.choice(src.size, 30, replace=False)                    # duplicated edges, half of them reversed
    src, dst = np.r_[src, src[dup[:15]], dst[dup[15:]]], np.r_[dst, dst[dup[:15]], src[dup[15:]]]
    loops = rng.choice(pool, 2, replace=False)
    src, dst = np.r_[src, loops], np.r_[dst, loops]
    order = rng.permutation(src.size)
    graph = Graph.from_edge_rows(torch.from_numpy(src[order]), torch.from_numpy(dst[order]), N_NODES)
    deg = (graph.rowptr[1:] - graph.rowptr[:-1]).long().numpy()
    assert tuple(deg[ladder]) == LADDER_DEGREES, deg[ladder]
    isolated = int(ladder[0])
    col = graph.col.long()
    assert int((col == edge_src(graph.rowptr)).sum()) == 2           # the self-loops

    pair_ladder = ladder[1:1 + len(LADDER_PAIRS)]
    others = np.setdiff1d(ids, pair_ladder)
    pu, pv = [rng.choice(others, 1500)], [rng.choice(others, 1500)]
    for node, cnt in zip(pair_ladder, LADDER_PAIRS):
        pu.append(np.full(cnt, node))
        pv.append(rng.choice(others, cnt, replace=False))
    pu, pv = np.concatenate(pu), np.concatenate(pv)
    same = rng.choice(others, 4, replace=False)                      # u == v pairs
    iso_mate = rng.choice(pool, 4, replace=False)                    # pairs touching the isolated node, both ways
    pu = np.r_[pu, same, isolated, isolated, iso_mate[2:]]
    pv = np.r_[pv, same, iso_mate[:2], isolated, isolated]
    dup = rng.choice(1500, 20, replace=False)                        # exact duplicates (of pairs among the other nodes)
    n0 = pu.size
    pu, pv = np.r_[pu, pu[dup]], np.r_[pv, pv[dup]]
    dup_pairs = np.stack([dup, n0 + np.arange(20)], 1)
    order = rng.permutation(pu.size)
    inv = np.argsort(order)
    pu, pv, dup_pairs = pu[order], pv[order], inv[dup_pairs]
    pairs = PairList.build(torch.from_numpy(pu), torch.from_numpy(pv), N_NODES)
    first = (pairs.by_u.rowptr[1:] - pairs.by_u.rowptr[:-1]).long().numpy()
    inc = (pairs.inc.rowptr[1:] - pairs.inc.rowptr[:-1]).long().numpy()
    assert tuple(first[pair_ladder]) == LADDER_PAIRS and tuple(inc[pair_ladder]) == LADDER_PAIRS, (first[pair_ladder], inc[pair_ladder])
    assert not np.isin(pv, pair_ladder).any()
    assert (pu[dup_pairs[:, 0]] == pu[dup_pairs[:, 1]]).all() and (pv[dup_pairs[:, 0]] == pv[dup_pairs[:, 1]]).all()
    assert int((pu == pv).sum()) >= 4 and int(((pu == isolated) | (pv == isolated)).sum()) >= 4
    return Structure(graph, pairs, graph.rowptr.long(), col, torch.from_numpy(pu), torch.from_numpy(pv),
                     ladder, pair_ladder, isolated, dup_pairs)


Case = namedtuple("Case", "K d dtype t beta generic")
TEMPERATURES, BETAS = (1.0, 2.0, 0.5), (0.6, 0.3, 0.9)
UNTUNED = ((3, 5), (2, 1), (7, 16))


def case_id(c: Case) -> str:
    return f"{c.dtype}-K{c.K}-d{c.d}-t{c.t:g}" + ("-generic" if c.generic else "")


def tuned_shapes(lib, dtype: str):
    from disenlink_amd import _lib
    code = {"f32": _lib.DL_F32, "bf16": _lib.DL_BF16}[dtype]
    return [(K, d) for K in range(1, 65) for d in (4, 8, 16, 32, 64, 128) if lib.dl_has_fast_path_dtype(K, d, code)]


def hotpath_cases(lib):
    """Every shape the library reports a tuned kernel for, in both table types (fp32 shapes once more on the generic
    kernels), three fp32 shapes without a tuned kernel, and the benchmark's (8, 64) at all three temperatures; t and
    beta cycle with the case index."""
    cases, i = [], 0
    for dtype in ("f32", "bf16"):
        shapes = tuned_shapes(lib, dtype)
        assert (8, 64) in shapes, f"the benchmark's shape (8, 64) has no tuned {dtype} kernel"
        for K, d in shapes + (list(UNTUNED) if dtype == "f32" else []):
            assert dtype == "bf16" or ((K, d) in UNTUNED) == ((K, d) not in shapes)
            ts = TEMPERATURES if (K, d) == (8, 64) else (TEMPERATURES[i % 3],)
            for t in ts:
                beta = BETAS[i % 3]
                cases.append(Case(K, d, dtype, t, beta, False))
                if dtype == "f32" and (K, d) in shapes and t == ts[0]:
                    cases.append(Case(K, d, dtype, t, beta, True))
                i += 1
    return cases


def _round_table(x64, dtype):
    return (x64.float() if dtype == "f32" else x64.to(torch.bfloat16)).double()


@functools.lru_cache(maxsize=4)
def reference(K: int, d: int, dtype: str, t: float, beta: float):
    """Tables for one case and everything the fp64 reference says about them (a dict of CPU tensors).

    Z is drawn at the amplitude of test_dense_scorer_on_the_matrix_cores_matches_the_pair_scorer and rounded to the table
    type; the scorer's H input is the reference's own H rounded to the table type, the scorer backward's prob input the
    fp32 sigmoid of the reference's logit, and the routing backward's (a, s, dH) inputs the reference's cast to fp32:
    every kernel is handed exactly rounded inputs, so no kernel's error leaks into the check of the next.

    Conditions on the reference alone (asserted; a case that misses one gets another seed or another amplitude from the
    deterministic search below, never a looser condition):
      * every edge's top-2 routing margin exceeds MARGIN, so p must be the fp64 argmax on EVERY edge;
      * between 3 pairs and 5 % of the pairs have |logit| > SATURATED;
      * everything is finite, in fp32 too (largest exponent argument below 80);
      * no pair's logit lies within 1e-3 (and 64 bands) of 24 ln 2, where the fp32 probability becomes exactly 1 and the
        clamped BCE gradient of a label-0 pair jumps from w to 0 (SURVEY.md §0 finding 4): on either side of the jump
        kernel and reference agree, at the jump itself either answer is right.
    """
    st = structure()
    N, P = N_NODES, st.pu.numel()
    amp0 = 0.3 * (32 / d) ** 0.5 * (4 / K) ** 0.25
    why, scale, margin_misses = [], 1.0, 0
    for step in range(48):
        seed = 7919 * K + 31 * d + int(10 * t) + 1000 * step + (500 if dtype == "bf16" else 0)
        g = torch.Generator().manual_seed(seed)
        Z = _round_table(torch.randn(N, K, d, generator=g, dtype=F64) * (amp0 * scale), dtype)
        alpha = alpha64(Z, st.rowptr, st.col, t)
        top = torch.sort(alpha, dim=1).values
        margin = float((top[:, -1] - top[:, -2]).min()) if K > 1 else 1.0
        p = torch.argmax(alpha, dim=1)
        a, s_raw, H = forward64(Z, st.rowptr, st.col, p, beta, t)
        H_in = _round_table(H, dtype)
        x = logit64(Z, H_in, st.pu, st.pv, t)
        x_abs = logit_abs64(Z, H_in, st.pu, st.pv, t)
        n_sat = int((x.abs() > SATURATED).sum())
        arg_max = float(((Z[st.pu.long()] * Z[st.pv.long()]).sum(-1).abs().max()) / t)
        arg_max = max(arg_max, float((Z[edge_src(st.rowptr)] * Z[st.col]).sum(-1).abs().max()) / t)
        finite = bool(torch.isfinite(x).all() and torch.isfinite(H).all()) and arg_max < 80 and float(x.abs().max()) < 1e30
        gap = float(((x - P_ONE).abs() - 64 * 4 * U * x_abs).min())
        why.append((seed, round(scale, 3), margin, n_sat, arg_max, gap))
        if not finite or n_sat > 0.05 * P:                            # too loud: lower the amplitude
            scale, margin_misses = scale * 0.85, 0
        elif n_sat < 3:                                               # too quiet
            scale, margin_misses = scale * 1.1, 0
        elif margin <= MARGIN or gap <= 1e-3:                         # another draw; a shape that keeps missing is too flat
            margin_misses += 1
            if margin_misses == 3:
                scale, margin_misses = scale * 1.25, 0
        else:
            break
    else:
        raise AssertionError(f"no admissible tables for K={K} d={d} {dtype} t={t}: {why}")
    assert margin > MARGIN and 3 <= n_sat <= 0.05 * P and finite and gap > 1e-3, (margin, n_sat, P, finite, gap)

    a_abs, s_abs = route_abs64(Z, st.rowptr, st.col, p, t)
    a32, s32 = a.float().double(), s_raw.float().double()
    assert bool((s32[st.isolated] == 0).all())
    ref = dict(Z=Z, seed=seed, scale=scale, margin=margin, n_sat=n_sat, p=p, a=a, a_abs=a_abs, s=s_raw, s_abs=s_abs,
               a32=a32, s32=s32, H_in=H_in, logit=x, logit_abs=x_abs)
    # aggregation: from the fp32 (a, s) it is handed
    ref["H"] = aggregate64(Z, st.rowptr, st.col, p, a32, s32, beta)
    ref["H_abs"] = aggregate_abs64(Z, st.rowptr, st.col, p, a32, s32, beta)
    # scorer backward from a random g_prob at the fp32 probabilities
    rng = np.random.default_rng(seed)
    prob32 = sigmoid32(x)
    g_prob = torch.from_numpy((rng.standard_normal(P) * 0.1).astype(np.float32)).double()
    ref["prob32"], ref["g_prob"] = prob32, g_prob
    ref["dZ_score"], ref["dH"] = score_bwd64(Z, H_in, st.pu, st.pv, t, g_prob, prob32)
    # one-pass training scorer: weighted BCE of (label, weight), weight-0 pairs included; the gradient in probability space with
    # F.binary_cross_entropy's clamp, at the fp32 probability (test_one_pass_training_scorer_matches_the_oracle_directly)
    label = torch.from_numpy((rng.random(P) < 0.3).astype(np.float32)).double()
    weight = torch.from_numpy((rng.uniform(0.2, 1.0, P) / 64).astype(np.float32)).double()
    weight[torch.from_numpy(rng.choice(P, P // 8, replace=False))] = 0.0
    r32 = (prob32.float() * (1 - prob32.float())).double()
    g_bce = weight * (prob32 - label) / torch.clamp(r32, min=1e-12)
    ref["label"], ref["weight"] = label, weight
    ref["dZ_train"], ref["dH_train"] = score_bwd64(Z, H_in, st.pu, st.pv, t, g_bce, prob32)
    ref["g_bce"] = g_bce
    # routing / aggregation backward from the reference's dH cast to fp32
    dH32 = ref["dH"].float().double()
    ref["dH32"] = dH32
    ref["dZ_route"] = route_aggregate_bwd64(Z, st.rowptr, st.col, p, beta, t, dH32)
    return ref
