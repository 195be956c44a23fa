"""Operators of the DisenLink hot path over libdisenlink_hip.so.

Raw wrappers (``route_fwd`` ...) take/return device tensors and launch on torch's current
stream; the ``autograd.Function``s stitch them into the graph so that the reference's
training loop (``loss.backward()``, main_disentangled.py:198) works unchanged.

There is no fallback: tensors must be CUDA(HIP) fp32 tensors and the library must be built.
"""
from __future__ import annotations

import os

import torch

from . import _lib
from ._dev import (                                                     # noqa: F401
    _POISON, _Workspace, _empty, _empty_like, _f32c, _need_cuda, _nkd, _stream, _tab, _ws, table_code)
from .graph import Graph, PairList
from .link_pred import (                                                # noqa: F401  (the dense link_pred: ops.* as before)
    DensePairPlanCache, LinkPred, ScoreAllPairs, ScoreAllPairsDense, ScoreAllPairsLogits, as_link_pred, score_allpairs_bwd,
    score_allpairs_bwd_dense, score_allpairs_bwd_dense_supported, score_allpairs_fwd, score_allpairs_logits_bwd_dense,
    score_allpairs_logits_fwd)
from .project import (                                                  # noqa: F401  (the projection: ops.project_* as before)
    Project, _pad_features, _XPlanes, keep_hidden, padded_features, project_bwd, project_fwd, project_sparse_bwd,
    project_sparse_fwd, project_supported, project_tile_width, xplanes_for)
from .recon import (                                                    # noqa: F401  (the whole-graph reconstruction loss)
    ReconLogitsLoss, ReconLoss, ReconSets, check_recon_counts, recon_sets, recon_weights, score_recon_logits_loss,
    score_recon_loss)
from .sampled import (                                                  # noqa: F401  (fresh training negatives every epoch)
    SampledLogitsLoss, SampledLoss, SampledNegatives, sample_negatives, sampled_order, score_sampled_logits_loss,
    score_sampled_loss, score_sampled_supported, score_sampled_train,
    SampledBprLoss, score_sampled_bpr_loss, score_sampled_bpr_supported, score_sampled_bpr_train,   # (... the ranking objective)
    HardDraw, check_hard_draw, sample_hard_negatives, sample_hard_supported)                        # (... hard negatives)
from .scans import (                                                    # noqa: F401  (the all-pairs scans: ops.score_* as before)
    BETWEEN_MAX_N, BLOCK_NODES, BLOCKS_MAX_N, LINKS_MAX_N, MINE_MAX_M, MINE_MAX_N, RANK_MAX_K, LinksBetween, NodeFilter,
    PairExclusion, PairTerms, bipartite_exclusion_csr, exclusion_csr, pair_exclusion, score_link_degrees,
    score_link_degrees_blocks, score_links, score_links_between, score_links_blocks, score_mine, score_mine_between,
    score_mine_blocks, score_pair_logits, score_pair_ranks, score_pair_ranks_counted, score_pair_terms, score_ranks,
    score_top_links, score_topk)


_bce_ws: dict = {}


def _ws_bce(device) -> torch.Tensor:
    """dl_pair_bce's 8 KiB of scratch: a buffer of its own (the shared grow-only workspace is handed to the plans' kernels
    in the same step; the compiled binding passes all three scratch tensors into one call).  DL_POISON=1 fills it like
    the shared one."""
    t = _bce_ws.get(device)
    if t is None:
        t = _bce_ws[device] = torch.empty(8192, dtype=torch.uint8, device=device)
    if _POISON:
        t.fill_(0xFF)
    return t


def _workspace(owner, device, K: int, d: int) -> torch.Tensor:
    """The device's shared scratch, at least what the plan of ``owner`` (a Graph or a PairList) needs at (K, d)."""
    return _ws.get(owner.workspace_bytes(K, d), device)


def _check_rows(g: Graph, Z: torch.Tensor):
    N, K, d = _nkd(Z)
    if N != g.n_nodes:
        raise ValueError(f"Z has {N} rows, graph has {g.n_nodes} nodes")
    return N, K, d


def _plan_check(owner, Z: torch.Tensor, *operands: torch.Tensor):
    """The refusals the plan entries share, ahead of a wrapper's own: the table, the operands and the plan on the GPU, and
    (a Graph) as many rows as the graph has nodes -> (N, K, d)."""
    if isinstance(owner, Graph):
        _need_cuda(Z, *operands, owner.rowptr)
        return _check_rows(owner, Z)
    _need_cuda(Z, *operands, owner.inc.rowptr)
    return _nkd(Z)


def _plan_call(entry: str, owner, Z: torch.Tensor, dt: int, *mid, H: torch.Tensor | None = None) -> None:
    """The one call path of the entries that walk a plan: ``entry``(head, *mid, tail) with ``mid`` in the entry's own order.
    head = (the graph's struct, Z, K, d, dt) for the entries of a Graph, (Z, H, K, d, dt) for those of a PairList, whose
    struct rides in ``mid`` where the entry has it; tail = (the owner's workspace, its size, the stream)."""
    K, d = Z.shape[1], Z.shape[2]
    ws = _workspace(owner, Z.device, K, d)
    head = (owner.c_struct(), Z.data_ptr()) if H is None else (Z.data_ptr(), H.data_ptr())
    _lib.check(getattr(_lib.load(), entry)(*head, K, d, dt, *mid, ws.data_ptr(), ws.numel(), _stream()), entry)


# ---------------------------------------------------------------------- raw wrappers
def route_fwd(g: Graph, Z: torch.Tensor, t: float, s_out: torch.Tensor | None = None, p_out: torch.Tensor | None = None,
              a_out: torch.Tensor | None = None):
    """-> p uint8[E], a f32[E], s f32[N,K] (raw sums; only the graph's rows are written).
    model.py:56-72 on the edges of adj.  p_out / a_out: write into existing per-entry arrays (a graph whose routing plan
    covers only SOME entries — dist.Shard.route_by_peer — fills its part of them; the row sums are taken over the
    arrays as they stand, so they are final after the last part)."""
    Z, dt = _tab(Z)
    N, K, d = _plan_check(g, Z)
    if (p_out is None) != (a_out is None):
        raise ValueError("p_out and a_out come together")
    if p_out is not None and (p_out.dtype != torch.uint8 or a_out.dtype != torch.float32 or p_out.numel() != g.n_edges
                              or a_out.numel() != g.n_edges or not p_out.is_contiguous() or not a_out.is_contiguous()):
        raise ValueError("p_out / a_out must be contiguous uint8 / float32 arrays of n_edges entries")
    p = _empty(g.n_edges, torch.uint8, Z.device) if p_out is None else p_out
    a = _empty(g.n_edges, torch.float32, Z.device) if a_out is None else a_out
    s = _empty((N, K), torch.float32, Z.device) if s_out is None else s_out
    _plan_call("dl_route_fwd", g, Z, dt, float(t), p.data_ptr(), a.data_ptr(), s.data_ptr())
    return p, a, s


def aggregate_fwd(g: Graph, Z: torch.Tensor, beta: float, p, a, s, H_out: torch.Tensor | None = None):
    """-> H f32[N,K,d] (only the graph's rows are written).  model.py:73-75."""
    Z, dt = _tab(Z)
    _plan_check(g, Z, p, a, s)
    H = _empty_like(Z) if H_out is None else H_out
    if H.dtype != Z.dtype:
        raise TypeError("H must have the storage type of Z")
    _plan_call("dl_aggregate_fwd", g, Z, dt, float(beta), p.data_ptr(), a.data_ptr(), s.data_ptr(), H.data_ptr())
    return H


def score_terms_available(K: int, d: int, dt: int) -> bool:
    """Whether dl_score_pairs_fwd hands out the per-factor logit terms the backward can reuse (the tuned scorer only)."""
    lib = _lib.load()
    return bool(lib.dl_has_fast_path_dtype(K, d, dt)) and not lib.dl_set_force_generic(-1)


def score_pairs_fwd(Z, H, pu, pv, t: float, pairs: PairList | None = None, want_coef: bool = False):
    """-> prob f32[P].  model.py:109-113 at the listed pairs.  ``pairs`` (the PairList the index arrays
    belong to) enables the LDS-staged, XCD-sliced kernel; without it every pair is scored on its own."""
    lib = _lib.load()
    (Z, dt), (H, dth) = _tab(Z), _tab(H)
    _need_cuda(Z, H, pu, pv)
    N, K, d = _nkd(Z)
    if H.shape != Z.shape or dt != dth:
        raise ValueError("Z and H differ in shape or storage type")
    if pu.dtype != torch.int32 or pv.dtype != torch.int32:
        raise TypeError("pair indices must be int32")
    P = int(pu.numel())
    prob = _empty(P, torch.float32, Z.device)
    by_u = pairs.c_struct_by_u() if pairs is not None else None
    # per-factor logit terms for the backward: only the tuned scorer produces them
    coef = None
    if want_coef and pairs is not None and score_terms_available(K, d, dt):
        coef = _empty((2, P, K), torch.float32, Z.device)
    _lib.check(lib.dl_score_pairs_fwd(Z.data_ptr(), H.data_ptr(), N, K, d, dt, float(t), pu.data_ptr(), pv.data_ptr(),
                                      P, by_u, prob.data_ptr(), coef.data_ptr() if coef is not None else None,
                                      _stream()), "dl_score_pairs_fwd")
    return (prob, coef) if want_coef else prob


def score_pairs_bwd(Z, H, pairs: PairList, t: float, prob, g_prob, dZ_out=None, dH_out=None, coef=None):
    """-> dZ, dH f32[N,K,d] (rows of the incidence plan are written)."""
    (Z, dt), (H, _dth), prob, g_prob = _tab(Z), _tab(H), _f32c(prob), _f32c(g_prob)
    N, K, d = _plan_check(pairs, Z, H, prob, g_prob)
    if prob.numel() != g_prob.numel():
        raise ValueError("prob / g_prob lengths differ")
    dZ = _empty(Z.shape, torch.float32, Z.device) if dZ_out is None else dZ_out
    dH = _empty(Z.shape, torch.float32, Z.device) if dH_out is None else dH_out
    if coef is not None and tuple(coef.shape) != (2, prob.numel(), K):
        raise ValueError("coef must be the [2, P, K] array of score_pairs_fwd for the same pair list")
    _plan_call("dl_score_pairs_bwd", pairs, Z, dt, float(t), pairs.c_struct(int(prob.numel())), prob.data_ptr(),
               g_prob.data_ptr(), coef.data_ptr() if coef is not None else None, dZ.data_ptr(), dH.data_ptr(), H=H)
    return dZ, dH


def one_pass_scorer_wanted(table_dtype, n_nodes: int, K: int, d: int) -> bool:
    """The training step's choice between the one-pass scorer (dl_score_pairs_train: 8 KB of partner rows per pair at K = 8,
    d = 64) and forward-with-stored-terms + two coefficient gathers (12 KB per pair) — ONE rule for model.forward_pairs_loss,
    dist.sharded_forward_loss and bench.py (DL_ONE_PASS_SCORER=0/1 forces either).  Measured (tools/score_train_time.py):
    one pass wins or ties wherever a wave-per-entry kernel exists (K in {4, 8} at d = 64; K = 16, d = 128 in both table types
    since round 5: Penn94-shaped bf16 15.9 vs 22.3 ms, fp32 29.9 vs 45.1) and for every fp32 shape (squirrel 387 vs 553 us);
    what remains for the separate kernels is a WIDE row (K d >= 2048) of bf16 tables that sit in the caches and has only
    the group-per-entry kernel (one wave per SIMD there)."""
    mode = os.environ.get("DL_ONE_PASS_SCORER", "auto")
    if mode in ("0", "1"):
        return mode == "1"
    if table_dtype == torch.float32 or K * d < 2048 or (K, d) == (16, 128):
        return True
    return 2 * n_nodes * K * d * 2 > (512 << 20)


def score_pairs_train_supported(pairs: PairList, K: int, d: int, dt: int) -> bool:
    return bool(_lib.load().dl_score_pairs_train_supported(pairs.c_struct(pairs.n_pairs), K, d, dt))


def _train_pairs(pairs: PairList, label, weight):
    """What a training step hands dl_score_pairs_train of its pair list, here and in the compiled binding (native.py):
    label and weight must cover the list; they are bound per entry once the same tensors come back (graph.py)
    -> the incidence struct."""
    P = int(label.numel())
    if weight.numel() != P or P != pairs.n_pairs:
        raise ValueError("label / weight must cover the pair list")
    pairs.bind_labels(label, weight, P)
    return pairs.c_struct(P)


def score_pairs_train(Z, H, pairs: PairList, t: float, label, weight):
    """-> prob f32[P], dZ, dH f32[N,K,d]: scorer forward, the weighted-BCE gradient of (label, weight) and the scorer
    backward in ONE pass over the incidence plan (dl_score_pairs_train; tuned (K, d) only).  dZ / dH are the
    gradients of sum_q weight BCE(prob, label)."""
    (Z, dt), (H, _dth), label, weight = _tab(Z), _tab(H), _f32c(label), _f32c(weight)
    _plan_check(pairs, Z, H, label, weight)
    inc = _train_pairs(pairs, label, weight)
    prob = _empty(pairs.n_pairs, torch.float32, Z.device)
    dZ = _empty(Z.shape, torch.float32, Z.device)
    dH = _empty(Z.shape, torch.float32, Z.device)
    _plan_call("dl_score_pairs_train", pairs, Z, dt, float(t), inc, label.data_ptr(), weight.data_ptr(), prob.data_ptr(),
               dZ.data_ptr(), dH.data_ptr(), H=H)
    return prob, dZ, dH


def pair_bce(prob, label, weight):
    """-> (loss, d loss / d prob f32[P]) of loss = sum_q weight[q] BCE(prob[q], label[q]) with torch's clamps, both from ONE
    kernel (dl_pair_bce) on its own scratch (``_ws_bce``)."""
    prob, label, weight = _f32c(prob), _f32c(label), _f32c(weight)
    _need_cuda(prob, label, weight)
    if not (prob.numel() == label.numel() == weight.numel()):
        raise ValueError("prob, label and weight differ in length")
    loss = _empty(1, torch.float32, prob.device)
    g = _empty_like(prob)
    ws = _ws_bce(prob.device)
    _lib.check(_lib.load().dl_pair_bce(prob.data_ptr(), label.data_ptr(), weight.data_ptr(), prob.numel(), loss.data_ptr(),
                                       g.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "dl_pair_bce")
    return loss[0], g


# ---- the same four in LOGIT space (include/disenlink_hip.h: "The pair-list objective in LOGIT space")
def score_pairs_logits_fwd(Z, H, pu, pv, t: float, pairs: PairList | None = None):
    """-> logit f32[P]: the value ``score_pairs_fwd`` feeds its sigmoid, at the listed pairs (dl_score_pairs_logits_fwd; no
    stored terms — the logit-space backward recomputes)."""
    lib = _lib.load()
    (Z, dt), (H, dth) = _tab(Z), _tab(H)
    _need_cuda(Z, H, pu, pv)
    N, K, d = _nkd(Z)
    if H.shape != Z.shape or dt != dth:
        raise ValueError("Z and H differ in shape or storage type")
    if pu.dtype != torch.int32 or pv.dtype != torch.int32:
        raise TypeError("pair indices must be int32")
    P = int(pu.numel())
    logit = _empty(P, torch.float32, Z.device)
    by_u = pairs.c_struct_by_u() if pairs is not None else None
    _lib.check(lib.dl_score_pairs_logits_fwd(Z.data_ptr(), H.data_ptr(), N, K, d, dt, float(t), pu.data_ptr(), pv.data_ptr(),
                                             P, by_u, logit.data_ptr(), _stream()), "dl_score_pairs_logits_fwd")
    return logit


def score_pairs_logits_bwd(Z, H, pairs: PairList, t: float, g_logit, dZ_out=None, dH_out=None):
    """-> dZ, dH f32[N,K,d] (rows of the incidence plan are written) from d loss / d logit per pair."""
    (Z, dt), (H, _dth), g_logit = _tab(Z), _tab(H), _f32c(g_logit)
    N, K, d = _plan_check(pairs, Z, H, g_logit)
    if g_logit.numel() != pairs.n_pairs:
        raise ValueError("g_logit must cover the pair list")
    dZ = _empty(Z.shape, torch.float32, Z.device) if dZ_out is None else dZ_out
    dH = _empty(Z.shape, torch.float32, Z.device) if dH_out is None else dH_out
    _plan_call("dl_score_pairs_logits_bwd", pairs, Z, dt, float(t), pairs.c_struct(int(g_logit.numel())), g_logit.data_ptr(),
               dZ.data_ptr(), dH.data_ptr(), H=H)
    return dZ, dH


def score_pairs_train_logits_supported(pairs: PairList, K: int, d: int, dt: int) -> bool:
    return bool(_lib.load().dl_score_pairs_train_logits_supported(pairs.c_struct(pairs.n_pairs), K, d, dt))


def score_pairs_train_logits(Z, H, pairs: PairList, t: float, label, weight):
    """-> logit f32[P], dZ, dH f32[N,K,d]: ``score_pairs_train`` in logit space (dl_score_pairs_train_logits) — dZ / dH are the
    gradients of sum_q weight BCE-with-logits(logit, label); a saturated pair keeps its gradient."""
    (Z, dt), (H, _dth), label, weight = _tab(Z), _tab(H), _f32c(label), _f32c(weight)
    _plan_check(pairs, Z, H, label, weight)
    inc = _train_pairs(pairs, label, weight)
    logit = _empty(pairs.n_pairs, torch.float32, Z.device)
    dZ = _empty(Z.shape, torch.float32, Z.device)
    dH = _empty(Z.shape, torch.float32, Z.device)
    _plan_call("dl_score_pairs_train_logits", pairs, Z, dt, float(t), inc, label.data_ptr(), weight.data_ptr(), logit.data_ptr(),
               dZ.data_ptr(), dH.data_ptr(), H=H)
    return logit, dZ, dH


def pair_bce_logits(logit, label, weight):
    """-> (loss, d loss / d logit f32[P]) of loss = sum_q weight[q] (max(x, 0) - x label + log1p(exp(-|x|))), both from ONE
    kernel (dl_pair_bce_logits) on dl_pair_bce's scratch."""
    logit, label, weight = _f32c(logit), _f32c(label), _f32c(weight)
    _need_cuda(logit, label, weight)
    if not (logit.numel() == label.numel() == weight.numel()):
        raise ValueError("logit, label and weight differ in length")
    loss = _empty(1, torch.float32, logit.device)
    g = _empty_like(logit)
    ws = _ws_bce(logit.device)
    _lib.check(_lib.load().dl_pair_bce_logits(logit.data_ptr(), label.data_ptr(), weight.data_ptr(), logit.numel(),
                                              loss.data_ptr(), g.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "dl_pair_bce_logits")
    return loss[0], g


def route_aggregate_bwd(g: Graph, Z, beta: float, t: float, p, a, s, dH, dZ_accum=None) -> torch.Tensor:
    """-> dZ f32[N,K,d] (added onto ``dZ_accum`` in place when given).  Unsharded graphs only."""
    (Z, dt), dH = _tab(Z), _f32c(dH)
    _plan_check(g, Z, dH, p, a, s)
    if dZ_accum is None:
        dZ, acc = _empty(Z.shape, torch.float32, Z.device), 0
    else:
        if not dZ_accum.is_contiguous() or dZ_accum.shape != Z.shape or dZ_accum.dtype != torch.float32:
            raise ValueError("dZ_accum must be a contiguous fp32 [N,K,d] tensor")
        dZ, acc = dZ_accum, 1
    _plan_call("dl_route_aggregate_bwd", g, Z, dt, float(beta), float(t), p.data_ptr(), a.data_ptr(), s.data_ptr(),
               dH.data_ptr(), dZ.data_ptr(), acc)
    return dZ


def route_aggregate_bwd_phase1(g: Graph, Z, beta: float, p, a, s, dH, ds_out: torch.Tensor):
    """-> dw, dwr f32[E]; writes ds[N,K] rows of the graph (all-gather ds before phase 2 when sharded)."""
    (Z, dt), dH = _tab(Z), _f32c(dH)
    _plan_check(g, Z, dH, p, a, s, ds_out)
    dw = _empty(g.n_edges, torch.float32, Z.device)
    dwr = _empty(g.n_edges, torch.float32, Z.device)
    _plan_call("dl_route_aggregate_bwd_phase1", g, Z, dt, float(beta), p.data_ptr(), a.data_ptr(), s.data_ptr(),
               dH.data_ptr(), dw.data_ptr(), dwr.data_ptr(), ds_out.data_ptr())
    return dw, dwr


def route_aggregate_bwd_phase2(g: Graph, Z, beta: float, t: float, p, a, s, dH, dw, dwr, ds, dZ_out: torch.Tensor,
                               accumulate: bool):
    (Z, dt), dH = _tab(Z), _f32c(dH)
    _plan_check(g, Z, dH, p, a, s, ds, dZ_out)
    _plan_call("dl_route_aggregate_bwd_phase2", g, Z, dt, float(beta), float(t), p.data_ptr(), a.data_ptr(), s.data_ptr(),
               dH.data_ptr(), dw.data_ptr(), dwr.data_ptr(), ds.data_ptr(), dZ_out.data_ptr(), 1 if accumulate else 0)
    return dZ_out


def route_aggregate_bwd_scaled(g: Graph, Z, beta: float, t: float, p, a, s, dH, dZ_in, scale) -> torch.Tensor:
    """-> dZ = scale * (dZ_in + backward(dH)), a NEW tensor: dH and dZ_in are only read (they may be an autograd node's
    saved tensors), scale is a 0-dim / 1-element fp32 tensor on the device (an upstream d/dloss).  dl_route_aggregate_bwd_scaled:
    the backward is linear in (dH, dZ_in), so a caller holding UNSCALED gradients needs no scaling passes."""
    (Z, dt), dH, dZ_in = _tab(Z), _f32c(dH), _f32c(dZ_in)
    scale = scale.to(device=Z.device, dtype=torch.float32).reshape(1)
    _plan_check(g, Z, dH, dZ_in, p, a, s)
    if dZ_in.shape != Z.shape or dH.shape != Z.shape:
        raise ValueError("dH and dZ_in must be [N,K,d] like Z")
    dZ = _empty(Z.shape, torch.float32, Z.device)
    _plan_call("dl_route_aggregate_bwd_scaled", g, Z, dt, float(beta), float(t), p.data_ptr(), a.data_ptr(), s.data_ptr(),
               dH.data_ptr(), dZ_in.data_ptr(), scale.data_ptr(), dZ.data_ptr())
    return dZ


# ---------------------------------------------------------------------- autograd
def step_tables(graph: Graph, Z, beta: float, t: float, table_dtype):
    """The tables of a step -> (Zt, p, a, s, H): Z (fp32) stored as ``table_dtype``, routed and aggregated from THAT table,
    H in the same storage type.  The one spelling of it: the training Functions and the ranking tables of
    Disentangle._rank_tables all come through here."""
    Zt = _f32c(Z) if table_dtype == torch.float32 else _f32c(Z).to(table_dtype)
    p, a, s = route_fwd(graph, Zt, t)
    return Zt, p, a, s, aggregate_fwd(graph, Zt, beta, p, a, s)


def _step_backward_tail(ctx, Zt, a, s, dZ, dH, g_emb):
    """How both step Functions end their backward: a gradient arriving on emb joins dH, then routing and aggregation add
    their dZ onto the scorer's, in place -> dZ."""
    if g_emb is not None:
        dH += g_emb
    return route_aggregate_bwd(ctx.graph, Zt, ctx.beta, ctx.t, ctx.p, a, s, dH, dZ_accum=dZ)


class RouteAggregate(torch.autograd.Function):
    """Z [N,K,d] -> H [N,K,d]: Disentangle_layer.forward (model.py:55-77) on the CSR of adj."""

    @staticmethod
    def forward(ctx, Z, graph: Graph, beta: float, t: float):
        Z, p, a, s, H = step_tables(graph, Z, beta, t, torch.float32)
        ctx.graph, ctx.beta, ctx.t = graph, beta, t
        ctx.save_for_backward(Z, a, s)
        ctx.p = p
        return H

    @staticmethod
    def backward(ctx, dH):
        Z, a, s = ctx.saved_tensors
        dZ = route_aggregate_bwd(ctx.graph, Z, ctx.beta, ctx.t, ctx.p, a, s, dH.contiguous())
        return dZ, None, None, None


class PairBCE(torch.autograd.Function):
    """loss = sum_q w[q] BCE(prob[q], label[q]) with torch's clamps, loss and d loss / d prob from ONE kernel
    (main_disentangled.py:195 on pair lists; see metrics.pair_bce_weights)."""

    @staticmethod
    def forward(ctx, prob, label, weight):
        loss, g = pair_bce(prob, label, weight)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        (g,) = ctx.saved_tensors
        return g * g_loss, None, None


class HotPathPairs(torch.autograd.Function):
    """Z [N,K,d] fp32 -> (emb [N,K,d] fp32, prob [P]): route + aggregate + pair scorer as ONE autograd node.
    ``table_dtype`` (torch.float32 / torch.bfloat16) is the storage type of the gathered Z and H tables;
    arithmetic and every gradient stay fp32 (the cast of Z happens inside, so dZ comes back in fp32)."""

    @staticmethod
    def forward(ctx, Z, graph: Graph, pairs: PairList, beta: float, t: float, table_dtype):
        ctx.set_materialize_grads(False)        # an unused output (emb in the training loss) arrives as None, not zeros
        Zt, p, a, s, H = step_tables(graph, Z, beta, t, table_dtype)
        if ctx.needs_input_grad[0]:
            prob, coef = score_pairs_fwd(Zt, H, pairs.pu, pairs.pv, t, pairs, want_coef=True)
        else:
            prob, coef = score_pairs_fwd(Zt, H, pairs.pu, pairs.pv, t, pairs), None
        ctx.graph, ctx.pairs, ctx.beta, ctx.t, ctx.p, ctx.coef = graph, pairs, beta, t, p, coef
        ctx.save_for_backward(Zt, H, a, s, prob)
        return H.float(), prob

    @staticmethod
    def backward(ctx, g_emb, g_prob):
        Zt, H, a, s, prob = ctx.saved_tensors
        g_prob = torch.zeros_like(prob) if g_prob is None else g_prob.contiguous()
        dZ, dH = score_pairs_bwd(Zt, H, ctx.pairs, ctx.t, prob, g_prob, coef=ctx.coef)
        _step_backward_tail(ctx, Zt, a, s, dZ, dH, g_emb)
        return dZ, None, None, None, None, None


class HotPathPairsLoss(torch.autograd.Function):
    """Z [N,K,d] fp32 -> (emb, prob [P], loss): route + aggregate + pair scorer + weighted BCE of (label, weight) as ONE
    autograd node whose scorer part runs forward AND backward in a single pass (score_pairs_train): the gradients of
    the loss w.r.t. the scorer's inputs are ready when the forward returns, and the backward only scales them by the
    incoming d/dloss and continues into aggregation and routing.  A gradient arriving on ``prob`` (another loss on the
    same scores) is added through the ordinary scorer backward."""

    @staticmethod
    def forward(ctx, Z, graph: Graph, pairs: PairList, beta: float, t: float, table_dtype, label, weight):
        ctx.set_materialize_grads(False)
        Zt, p, a, s, H = step_tables(graph, Z, beta, t, table_dtype)
        prob, dZs, dHs = score_pairs_train(Zt, H, pairs, t, label, weight)
        loss, _g = pair_bce(prob, label, weight)                # dl_pair_bce's gradient output: the loss VALUE is what is used
        ctx.graph, ctx.pairs, ctx.beta, ctx.t, ctx.p = graph, pairs, beta, t, p
        ctx.save_for_backward(Zt, H, a, s, prob, dZs, dHs)
        return H.float(), prob, loss

    @staticmethod
    def backward(ctx, g_emb, g_prob, g_loss):
        Zt, H, a, s, prob, dZs, dHs = ctx.saved_tensors
        if g_loss is not None and g_prob is None and g_emb is None and g_loss.numel() == 1:
            # the usual case (loss.backward()): everything downstream is linear in the scorer's gradients, so d/dloss
            # scales the RESULT inside the last kernel — no scaling passes over the two [N,K,d] arrays, which stay unwritten
            return (route_aggregate_bwd_scaled(ctx.graph, Zt, ctx.beta, ctx.t, ctx.p, a, s, dHs, dZs, g_loss),
                    None, None, None, None, None, None, None)
        if g_loss is not None:
            dZ, dH = dZs * g_loss, dHs * g_loss
        else:
            dZ, dH = torch.zeros_like(dZs), torch.zeros_like(dHs)
        if g_prob is not None:                                   # some other function of the scores
            dZ2, dH2 = score_pairs_bwd(Zt, H, ctx.pairs, ctx.t, prob, g_prob.contiguous())
            dZ += dZ2
            dH += dH2
        _step_backward_tail(ctx, Zt, a, s, dZ, dH, g_emb)
        return dZ, None, None, None, None, None, None, None


class PairBCELogits(torch.autograd.Function):
    """loss = sum_q w[q] BCE-with-logits(logit[q], label[q]), loss and d loss / d logit from ONE kernel (pair_bce_logits)."""

    @staticmethod
    def forward(ctx, logit, label, weight):
        loss, g = pair_bce_logits(logit, label, weight)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        (g,) = ctx.saved_tensors
        return g * g_loss, None, None


class HotPathPairLogits(torch.autograd.Function):
    """Z [N,K,d] fp32 -> (emb [N,K,d] fp32, logit [P]): ``HotPathPairs`` with the LOGITS out; the backward takes d loss / d logit
    and recomputes the per-factor terms (score_pairs_logits_bwd)."""

    @staticmethod
    def forward(ctx, Z, graph: Graph, pairs: PairList, beta: float, t: float, table_dtype):
        ctx.set_materialize_grads(False)
        Zt, p, a, s, H = step_tables(graph, Z, beta, t, table_dtype)
        logit = score_pairs_logits_fwd(Zt, H, pairs.pu, pairs.pv, t, pairs)
        ctx.graph, ctx.pairs, ctx.beta, ctx.t, ctx.p = graph, pairs, beta, t, p
        ctx.save_for_backward(Zt, H, a, s)
        return H.float(), logit

    @staticmethod
    def backward(ctx, g_emb, g_logit):
        Zt, H, a, s = ctx.saved_tensors
        g_logit = torch.zeros(ctx.pairs.n_pairs, dtype=torch.float32, device=Zt.device) if g_logit is None else g_logit.contiguous()
        dZ, dH = score_pairs_logits_bwd(Zt, H, ctx.pairs, ctx.t, g_logit)
        _step_backward_tail(ctx, Zt, a, s, dZ, dH, g_emb)
        return dZ, None, None, None, None, None


class HotPathPairLogitsLoss(torch.autograd.Function):
    """Z [N,K,d] fp32 -> (emb, logit [P], loss): ``HotPathPairsLoss`` in logit space — the one-pass scorer with
    gl = w (sigma(x) - y) (score_pairs_train_logits) and the loss value of pair_bce_logits.  The backward is that node's: d/dloss
    scales the result inside the last kernel; a gradient arriving on ``logit`` goes through score_pairs_logits_bwd."""

    @staticmethod
    def forward(ctx, Z, graph: Graph, pairs: PairList, beta: float, t: float, table_dtype, label, weight):
        ctx.set_materialize_grads(False)
        Zt, p, a, s, H = step_tables(graph, Z, beta, t, table_dtype)
        logit, dZs, dHs = score_pairs_train_logits(Zt, H, pairs, t, label, weight)
        loss, _g = pair_bce_logits(logit, label, weight)         # the loss VALUE is what is used
        ctx.graph, ctx.pairs, ctx.beta, ctx.t, ctx.p = graph, pairs, beta, t, p
        ctx.save_for_backward(Zt, H, a, s, dZs, dHs)
        return H.float(), logit, loss

    @staticmethod
    def backward(ctx, g_emb, g_logit, g_loss):
        Zt, H, a, s, dZs, dHs = ctx.saved_tensors
        if g_loss is not None and g_logit is None and g_emb is None and g_loss.numel() == 1:
            return (route_aggregate_bwd_scaled(ctx.graph, Zt, ctx.beta, ctx.t, ctx.p, a, s, dHs, dZs, g_loss),
                    None, None, None, None, None, None, None)
        if g_loss is not None:
            dZ, dH = dZs * g_loss, dHs * g_loss
        else:
            dZ, dH = torch.zeros_like(dZs), torch.zeros_like(dHs)
        if g_logit is not None:                                  # some other function of the scores
            dZ2, dH2 = score_pairs_logits_bwd(Zt, H, ctx.pairs, ctx.t, g_logit.contiguous())
            dZ += dZ2
            dH += dH2
        _step_backward_tail(ctx, Zt, a, s, dZ, dH, g_emb)
        return dZ, None, None, None, None, None, None, None


class HotPathPairsResampledLoss(torch.autograd.Function):
    """Z [N,K,d] fp32 -> (emb, score [P], neg_score [E], loss): ``HotPathPairsLoss`` (``logit``: ``HotPathPairLogitsLoss``) over
    the POSITIVE list ``pairs`` with (label, weight), plus this epoch's sampled negatives (``sampled``, ``k``, one weight
    ``neg_weight``) through ``score_sampled_train``, over ONE routing / aggregation forward and one backward: the sampled
    trainer adds its gradients onto the positive list's in its finishing launch, and loss = positive part + negative part.
    The backward takes a gradient on the loss (and on emb); the scores carry none.  fp32 tables only.
    ``k``: the epoch's partners, or a ``HardDraw`` — the sampled trainer then draws them from the (Zt, H) of this forward."""

    @staticmethod
    def forward(ctx, Z, graph: Graph, pairs: PairList, beta: float, t: float, label, weight, sampled, k, neg_weight: float,
                logit: bool, order=None, k_rowptr=None):
        check_hard_draw(k, order, k_rowptr)
        ctx.set_materialize_grads(False)
        Zt, p, a, s, H = step_tables(graph, Z, beta, t, torch.float32)
        if logit:
            score, dZs, dHs = score_pairs_train_logits(Zt, H, pairs, t, label, weight)
            loss_pos, _g = pair_bce_logits(score, label, weight)
        else:
            score, dZs, dHs = score_pairs_train(Zt, H, pairs, t, label, weight)
            loss_pos, _g = pair_bce(score, label, weight)
        loss_neg, neg_score, dZs, dHs = score_sampled_train(Zt, H, t, sampled, k, neg_weight, logit, order, k_rowptr,
                                                            dZ_accum=dZs, dH_accum=dHs)
        ctx.graph, ctx.beta, ctx.t, ctx.p = graph, beta, t, p
        ctx.save_for_backward(Zt, a, s, dZs, dHs)
        ctx.mark_non_differentiable(score, neg_score)
        return H.float(), score, neg_score, loss_pos + loss_neg

    @staticmethod
    def backward(ctx, g_emb, _g_score, _g_neg, g_loss):
        Zt, a, s, dZs, dHs = ctx.saved_tensors
        none = (None,) * 12
        if g_loss is not None and g_emb is None and g_loss.numel() == 1:
            return (route_aggregate_bwd_scaled(ctx.graph, Zt, ctx.beta, ctx.t, ctx.p, a, s, dHs, dZs, g_loss),) + none
        if g_loss is not None:
            dZ, dH = dZs * g_loss, dHs * g_loss
        else:
            dZ, dH = torch.zeros_like(dZs), torch.zeros_like(dHs)
        _step_backward_tail(ctx, Zt, a, s, dZ, dH, g_emb)
        return (dZ,) + none


class HotPathBprLoss(torch.autograd.Function):
    """Z [N,K,d] fp32 -> (emb, pos_logit [n_rows], neg_logit [E], val_logit [P] or an empty tensor, loss): one routing /
    aggregation forward, the pairwise ranking loss of ``score_sampled_bpr_train`` over ``sampled`` (built with ``dst``) and this
    epoch's partners ``k`` with the one weight ``weight``, and — ``val_pairs`` given — the logits of that list through
    ``score_pairs_logits_fwd``, forward only.  The backward is ``HotPathPairsResampledLoss``'s: a gradient on the loss (scaled
    inside the last kernel) and on emb; the logits carry none.  fp32 tables only.
    ``k``: the epoch's partners, or a ``HardDraw`` — the ranking trainer then draws them from the (Zt, H) of this forward."""

    @staticmethod
    def forward(ctx, Z, graph: Graph, beta: float, t: float, sampled, k, weight: float, val_pairs=None, order=None, k_rowptr=None):
        check_hard_draw(k, order, k_rowptr)
        ctx.set_materialize_grads(False)
        Zt, p, a, s, H = step_tables(graph, Z, beta, t, torch.float32)
        loss, pos, neg, dZs, dHs = score_sampled_bpr_train(Zt, H, t, sampled, k, weight, order, k_rowptr)
        if val_pairs is None:
            val = torch.empty(0, dtype=torch.float32, device=Zt.device)
        else:
            val = score_pairs_logits_fwd(Zt, H, val_pairs.pu, val_pairs.pv, t, val_pairs)
        ctx.graph, ctx.beta, ctx.t, ctx.p = graph, beta, t, p
        ctx.save_for_backward(Zt, a, s, dZs, dHs)
        ctx.mark_non_differentiable(pos, neg, val)
        return H.float(), pos, neg, val, loss

    @staticmethod
    def backward(ctx, g_emb, _g_pos, _g_neg, _g_val, g_loss):
        Zt, a, s, dZs, dHs = ctx.saved_tensors
        none = (None,) * 9
        if g_loss is not None and g_emb is None and g_loss.numel() == 1:
            return (route_aggregate_bwd_scaled(ctx.graph, Zt, ctx.beta, ctx.t, ctx.p, a, s, dHs, dZs, g_loss),) + none
        if g_loss is not None:
            dZ, dH = dZs * g_loss, dHs * g_loss
        else:
            dZ, dH = torch.zeros_like(dZs), torch.zeros_like(dHs)
        _step_backward_tail(ctx, Zt, a, s, dZ, dH, g_emb)
        return (dZ,) + none


class HotPathRecon(torch.autograd.Function):
    """Z [N,K,d] fp32 -> (emb [N,K,d] fp32, loss): route + aggregate + the whole-graph reconstruction loss as ONE autograd
    node on tables stored as ``table_dtype`` — the step of a bf16 module, in the shape of ``HotPathPairsLoss``: the cast of Z
    happens inside (so dZ comes back in fp32), H is routed and aggregated from THAT table, and ``score_recon_loss`` has the
    gradients of the loss with respect to both tables ready when the forward returns.  The backward scales them by the
    incoming d/dloss, adds a gradient arriving on ``emb`` to dH and continues into aggregation and routing.  ``sets``: a
    prepared ``recon_sets(...)``, whose node filter, if it has one, is the rule of the loss; the device counts stand in
    ``ReconLoss.last_counts``."""
    _loss, _counts = staticmethod(score_recon_loss), ReconLoss

    @classmethod
    def forward(cls, ctx, Z, graph: Graph, sets: ReconSets, beta: float, t: float, table_dtype, pos_weight=None, block_rows=None):
        ctx.set_materialize_grads(False)
        Zt, p, a, s, H = step_tables(graph, Z, beta, t, table_dtype)
        loss, dZs, dHs, counts = cls._loss(Zt, H, t, sets, None, pos_weight, block_rows, table_dtype=table_dtype)
        ctx.graph, ctx.beta, ctx.t, ctx.p = graph, beta, t, p
        ctx.save_for_backward(Zt, a, s, dZs, dHs)
        cls._counts.last_counts = counts
        return H.float(), loss.to(torch.float32)

    @staticmethod
    def backward(ctx, g_emb, g_loss):
        Zt, a, s, dZs, dHs = ctx.saved_tensors
        if g_loss is not None:
            dZ, dH = dZs * g_loss, dHs * g_loss
        else:
            dZ, dH = torch.zeros_like(dZs), torch.zeros_like(dHs)
        _step_backward_tail(ctx, Zt, a, s, dZ, dH, g_emb)
        return dZ, None, None, None, None, None, None, None


class HotPathReconLogits(HotPathRecon):
    """``HotPathRecon`` with the loss in logit space (``score_recon_logits_loss``): the same single node; the device counts
    stand in ``ReconLogitsLoss.last_counts``."""
    _loss, _counts = staticmethod(score_recon_logits_loss), ReconLogitsLoss


class ScorePairs(torch.autograd.Function):
    """(Z, H) -> prob[P] at the listed pairs: model.py:109-113 + sigmoid."""

    @staticmethod
    def forward(ctx, Z, H, pairs: PairList, t: float):
        Z, H = _f32c(Z), _f32c(H)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        prob, coef = score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs, want_coef=True) if need else \
            (score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs), None)
        ctx.pairs, ctx.t, ctx.coef = pairs, t, coef
        ctx.save_for_backward(Z, H, prob)
        return prob

    @staticmethod
    def backward(ctx, g_prob):
        Z, H, prob = ctx.saved_tensors
        dZ, dH = score_pairs_bwd(Z, H, ctx.pairs, ctx.t, prob, g_prob.contiguous(), coef=ctx.coef)
        return dZ, dH, None, None
