"""Fresh training negatives every epoch, drawn and trained on the device (csrc/dl_sample.hip, csrc/dl_train_sampled.hip).

The fixed split draws m negatives per training edge row ONCE (``splits.structured_negatives``) and trains on that list for the
whole run.  Here the same rule — for the source u of a training edge row a node k, uniform over [0, N), with (u, k) not an
edge row of the whole dataset — is drawn anew each epoch by ``sample_negatives`` (counter-based Philox4x32-10: a pure
function of (seed, epoch, entry)) and trained by ``score_sampled_train`` without a plan build: the u side of the list is fixed
for the run (``SampledNegatives``), the partner side needs one stable device sort (``sampled_order``).  No host read and no
synchronisation in the epoch.

Hard negatives (csrc/dl_sample_hard.hip): ``sample_hard_negatives`` draws c candidates per entry by the same rule and keeps the
one the current tables score highest; a ``HardDraw`` handed to a trainer or a step in place of ``k`` makes that draw inside the
step, on the tables the loss is taken on.

What differs from the fixed split: duplicated draws inside an epoch are KEPT as separate loss terms (the fixed split keeps only
the pairs drawn once); an entry whose 64 attempts all hit excluded partners is k = -1, weight 0, and counted in ``n_failed``.
fp32 tables only (bf16 tables raise).

The same draws also serve the pairwise ranking objective (csrc/dl_train_bpr.hip): ``SampledNegatives(..., dst=...)`` keeps the
positives' other end, and ``score_sampled_bpr_train`` trains every edge row (u, v) to score above (u, k) for its m draws.
"""
from __future__ import annotations

import torch

from . import _lib
from ._dev import _empty, _f32c, _need_cuda, _nkd, _stream, _ws
from .scans import _csr_args, exclusion_csr


class SampledNegatives:
    """The fixed side of the resampled negatives, built once per run: ``src`` int32 [n_rows] ascending (the sources of the
    training edge rows, duplicates kept), ``m`` draws per row, ``u_rowptr`` int32 [N+1] (the CSR of the u side, in ENTRIES:
    entry e = r m + j belongs to src[r]) and the exclusion CSR (``ops.exclusion_csr`` normal form: ascending distinct columns
    per row, directed — (u, k) excluded says nothing about (k, u)).  ``exclusion``: what ``ops.exclusion_csr`` takes (a
    ``(rows, cols)`` pair, a dense mask, a ``Graph``) or None.
    ``dst`` (aligned with ``src``; what the pairwise ranking trainer ``score_sampled_bpr_train`` needs): the other end of every
    edge row, carried through a STABLE sort by ``src`` and kept as ``.dst`` int32 [n_rows], with ``.dst_order`` int32 [n_rows]
    (the stable ascending sort of ``.dst`` over the rows) and ``.dst_rowptr`` int32 [N+1] (the number of rows with dst < n),
    built once.  Without it the three are None and everything else is what it was."""

    def __init__(self, src, m: int, n_nodes: int, exclusion=None, device=None, dst=None):
        src = torch.as_tensor(src)
        device = src.device if device is None else torch.device(device)
        if src.dim() != 1 or src.dtype.is_floating_point:
            raise ValueError("src must be a 1-D integer array")
        if int(m) < 1 or int(n_nodes) < 1:
            raise ValueError(f"m and n_nodes must be positive, got {m}, {n_nodes}")
        self.dst = self.dst_order = self.dst_rowptr = None
        if dst is None:
            src = torch.sort(src.to(device=device, dtype=torch.int64)).values
        else:
            dst = torch.as_tensor(dst)
            if dst.dim() != 1 or dst.dtype.is_floating_point or dst.numel() != src.numel():
                raise ValueError("dst must be a 1-D integer array aligned with src")
            src, perm = torch.sort(src.to(device=device, dtype=torch.int64), stable=True)
            dst = dst.to(device=device, dtype=torch.int64)[perm]
            if dst.numel() and (int(dst.min()) < 0 or int(dst.max()) >= n_nodes):
                raise ValueError(f"dst outside [0, {n_nodes})")
            sd, order = torch.sort(dst, stable=True)
            self.dst = dst.to(torch.int32).contiguous()
            self.dst_order = order.to(torch.int32).contiguous()
            self.dst_rowptr = torch.searchsorted(sd, torch.arange(int(n_nodes) + 1, device=device, dtype=torch.int64)) \
                .to(torch.int32).contiguous()
        if src.numel() and (int(src[0]) < 0 or int(src[-1]) >= n_nodes):          # built once: the one host read
            raise ValueError(f"src outside [0, {n_nodes})")
        if src.numel() * int(m) > (2 ** 31 - 1) // 128:
            raise ValueError("too many entries for 32-bit list positions")
        self.n_nodes, self.m, self.n_rows = int(n_nodes), int(m), int(src.numel())
        self.src = src.to(torch.int32).contiguous()
        nodes = torch.arange(self.n_nodes + 1, device=device, dtype=torch.int64)
        self.u_rowptr = (torch.searchsorted(src, nodes) * self.m).to(torch.int32).contiguous()
        self.ex_rowptr, self.ex_col = exclusion_csr(exclusion, self.n_nodes, device)
        self.device = device

    @property
    def n_entries(self) -> int:
        return self.n_rows * self.m

    def entry_u(self) -> torch.Tensor:
        """int32 [n_entries]: the u of every entry (a listed copy, for tests and comparisons)."""
        return self.src.repeat_interleave(self.m)


def _epoch_tensor(epoch, device) -> torch.Tensor:
    if torch.is_tensor(epoch):
        if epoch.dtype != torch.int64 or epoch.numel() != 1 or epoch.device != device:
            raise ValueError("epoch must be an int or a 1-element int64 tensor on the device")
        return epoch
    if int(epoch) < 0:
        raise ValueError("epoch must be >= 0")
    return torch.tensor([int(epoch)], dtype=torch.int64, device=device)


def sample_negatives(src, m: int = None, n_nodes: int = None, exclusion=None, seed: int = 0, epoch=0, exclude_self: bool = False,
                     n_failed: torch.Tensor | None = None):
    """-> (k int32 [n_rows m], n_failed int32 [1]): one partner per entry e = r m + j, uniform over [0, n_nodes), with
    (src[r], k) not in ``exclusion`` (and k != src[r] if ``exclude_self``) — dl_sample_negatives.  ``src``: a prepared
    ``SampledNegatives`` (then m, n_nodes and exclusion are its own) or an int32 device tensor with ``exclusion`` = a
    ``(rowptr, col)`` CSR in ``ops.exclusion_csr`` form or None.  ``epoch``: an int, or a 1-element int64 DEVICE tensor that
    the kernel reads (a loop advances it with ``add_(1)``: no host value changes between epochs).  The draw is a pure function
    of (seed, epoch, e) — Philox4x32-10, k = (word * n_nodes) >> 32, biased by at most n_nodes / 2^32 — and the same bits on
    every call.  An entry that fails 64 attempts is -1 and counted in ``n_failed`` (``n_failed`` given: added onto it).
    Duplicated draws are kept.  No host read, no synchronisation."""
    if isinstance(src, SampledNegatives):
        s = src
        src, m, n_nodes, ex = s.src, s.m, s.n_nodes, (s.ex_rowptr, s.ex_col)
    else:
        ex = (None, None) if exclusion is None else tuple(exclusion)
        if m is None or n_nodes is None:
            raise ValueError("m and n_nodes are required with a raw src array")
    _need_cuda(src)
    if src.dtype != torch.int32 or not src.is_contiguous():
        raise TypeError("src must be a contiguous int32 tensor")
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 bits")
    dev = src.device
    for a in ex:
        if a is not None and (a.dtype != torch.int32 or a.device != dev):
            raise TypeError("the exclusion CSR must be int32 tensors on the device of src")
    ep = _epoch_tensor(epoch, dev)
    k = _empty(src.numel() * int(m), torch.int32, dev)
    if n_failed is None:
        n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
    er, ec, keep = _csr_args(ex[0], ex[1], dev)
    _lib.check(_lib.load().dl_sample_negatives(src.data_ptr(), src.numel(), int(m), int(n_nodes), er, ec, int(seed), ep.data_ptr(),
                                               int(bool(exclude_self)), k.data_ptr(), n_failed.data_ptr(), _stream()),
               "dl_sample_negatives")
    del keep
    return k, n_failed


def sampled_order(k: torch.Tensor, n_nodes: int):
    """-> (order int32 [E], k_rowptr int32 [N+1]) of an epoch's partners: the STABLE ascending sort of k over the entries (the
    -1 entries first) and k_rowptr[n] = the number of entries with k < n.  Device work only (one sort, one search)."""
    sk, order = torch.sort(k, stable=True)
    nodes = torch.arange(int(n_nodes) + 1, device=k.device, dtype=k.dtype)
    return order.to(torch.int32), torch.searchsorted(sk, nodes).to(torch.int32)


# ------------------------------------------------------------------------------------------------ hard negatives
HARD_MAX_CANDIDATES = 64                 # one lane of a wave draws one candidate


def _check_candidates(candidates) -> int:
    c = int(candidates)
    if not 1 <= c <= HARD_MAX_CANDIDATES:
        raise ValueError(f"candidates must be 1 .. {HARD_MAX_CANDIDATES} per entry, got {candidates}")
    return c


def sample_hard_supported(K: int, d: int, dtype=torch.float32) -> bool:
    code = _lib.DL_F32 if dtype == torch.float32 else _lib.DL_BF16 if dtype == torch.bfloat16 else -1
    return code >= 0 and bool(_lib.load().dl_sample_negatives_hard_supported(int(K), int(d), code))


def sample_hard_negatives(Z, H, t: float, src, candidates: int, m: int = None, n_nodes: int = None, exclusion=None, seed: int = 0,
                          epoch=0, exclude_self: bool = False, n_failed: torch.Tensor | None = None):
    """-> (k int32 [n_rows m], logit f32 [n_rows m], n_failed int32 [1]): hard negatives (dynamic negative sampling) —
    ``candidates`` = c draws per entry instead of one (1 <= c <= 64), each by the rule of ``sample_negatives`` with the Philox
    counter (e, i 64 + attempt, epoch), and the live candidate that the tables ``Z``, ``H`` [N,K,d] score highest is kept:
    x(u, k) = sum_f (h_f[u].h_f[k]) exp(z_f[u].z_f[k] / t) in fp32, ties to the lowest candidate index, a NaN below every number
    (all NaN: the first live candidate) — dl_sample_negatives_hard.  Candidate 0 is ``sample_negatives``' draw for the entry, so
    c = 1 returns its k.  ``logit``: the kept candidate's logit, the bits ``score_sampled_bpr_train`` returns as ``neg_logit``
    for the same pair; 0 where k = -1 (all c candidates failed, or a src outside the table), which counts ONCE in ``n_failed``
    (given: added onto it).  ``src``, ``m``, ``n_nodes``, ``exclusion``, ``epoch``: as in ``sample_negatives``.  A pure function of
    (seed, epoch, entry, Z, H, t): the same bits on every call; no host read, no synchronisation.  The selection favours
    unobserved TRUE links where the graph has many.  fp32 tables with K d <= 2048; bf16 tables raise."""
    c = _check_candidates(candidates)
    if Z.dtype != torch.float32 or H.dtype != torch.float32:
        raise TypeError(f"the hard-negative sampler takes fp32 tables, got {Z.dtype} / {H.dtype} (bf16 tables are not served)")
    if isinstance(src, SampledNegatives):
        s = src
        src, m, n_nodes, ex = s.src, s.m, s.n_nodes, (s.ex_rowptr, s.ex_col)
    else:
        ex = (None, None) if exclusion is None else tuple(exclusion)
        if m is None or n_nodes is None:
            raise ValueError("m and n_nodes are required with a raw src array")
    if t == 0:
        raise ValueError("temperature is 0")
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 bits")
    Z, H = _f32c(Z), _f32c(H)
    _need_cuda(Z, H, src)
    N, K, d = _nkd(Z)
    if tuple(H.shape) != tuple(Z.shape):
        raise ValueError("Z and H differ in shape")
    if N != int(n_nodes):
        raise ValueError(f"tables of {N} nodes, negatives over {n_nodes}")
    if src.dtype != torch.int32 or not src.is_contiguous():
        raise TypeError("src must be a contiguous int32 tensor")
    lib = _lib.load()
    if not lib.dl_sample_negatives_hard_supported(K, d, _lib.DL_F32):
        raise _lib.DisenlinkHipError(f"the hard-negative sampler serves fp32 tables with K <= 64 and K d <= 2048 (got K={K}, d={d}); "
                                     "there is no eager fallback")
    dev = src.device
    for a in ex:
        if a is not None and (a.dtype != torch.int32 or a.device != dev):
            raise TypeError("the exclusion CSR must be int32 tensors on the device of src")
    ep = _epoch_tensor(epoch, dev)
    E = src.numel() * int(m)
    k = _empty(E, torch.int32, dev)
    logit = _empty(E, torch.float32, dev)
    if n_failed is None:
        n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
    er, ec, keep = _csr_args(ex[0], ex[1], dev)
    _lib.check(lib.dl_sample_negatives_hard(Z.data_ptr(), H.data_ptr(), N, K, d, _lib.DL_F32, float(t), src.data_ptr(), src.numel(),
                                            int(m), c, er, ec, int(seed), ep.data_ptr(), int(bool(exclude_self)), k.data_ptr(),
                                            logit.data_ptr(), n_failed.data_ptr(), _stream()), "dl_sample_negatives_hard")
    del keep
    return k, logit, n_failed


class HardDraw:
    """What a training step takes in place of this epoch's ``k`` to train on hard negatives: ``candidates`` draws per entry
    (1 .. 64), ``seed``, ``epoch`` (an int, or the 1-element int64 DEVICE tensor a loop advances), ``n_failed`` (an int32 [1]
    device tensor the failed entries are added onto; None: the record makes its own at the first draw) and ``exclude_self``.
    The step — ``score_sampled_train`` / ``score_sampled_bpr_train`` and everything built on them — calls ``draw`` on the tables
    its loss is taken on, under no_grad; afterwards ``.k`` and ``.logit`` hold that step's draw (None before the first)."""

    def __init__(self, candidates: int, seed: int = 0, epoch=0, n_failed: torch.Tensor | None = None, exclude_self: bool = False):
        self.candidates = _check_candidates(candidates)
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must fit 64 bits")
        self.seed, self.epoch, self.n_failed, self.exclude_self = int(seed), epoch, n_failed, bool(exclude_self)
        self.k = self.logit = None

    def draw(self, Z, H, t: float, sampled: SampledNegatives) -> torch.Tensor:
        """``sample_hard_negatives`` for the entries of ``sampled`` on (Z, H) -> k; kept in ``.k`` / ``.logit``."""
        with torch.no_grad():
            self.k, self.logit, self.n_failed = sample_hard_negatives(
                Z.detach(), H.detach(), t, sampled, self.candidates, seed=self.seed, epoch=self.epoch,
                exclude_self=self.exclude_self, n_failed=self.n_failed)
        return self.k


def check_hard_draw(k, order, k_rowptr) -> None:
    """A ``HardDraw`` draws its partners inside the step, so their sort cannot exist beforehand: ``order`` / ``k_rowptr`` raise."""
    if isinstance(k, HardDraw) and (order is not None or k_rowptr is not None):
        raise ValueError("with a HardDraw the partners are drawn inside the step: order / k_rowptr cannot be given")


def score_sampled_supported(K: int, d: int, dtype=torch.float32) -> bool:
    code = _lib.DL_F32 if dtype == torch.float32 else _lib.DL_BF16 if dtype == torch.bfloat16 else -1
    return code >= 0 and bool(_lib.load().dl_score_sampled_train_supported(int(K), int(d), code))


def score_sampled_train(Z, H, t: float, sampled: SampledNegatives, k, weight: float, logits: bool = False, order=None,
                        k_rowptr=None, dZ_accum=None, dH_accum=None):
    """-> (loss f32 [], score f32 [E], dZ, dH f32 [N,K,d]) for the entries (u_e, k_e) of ``sampled`` with this epoch's
    partners ``k``, label 0 and ONE weight: score = sigmoid(x) (``logits``: x), loss = sum_e -weight max(log(1 - score), -100)
    (``logits``: sum_e weight (max(x, 0) + log1p(exp(-|x|)))), dZ / dH its gradient, every pair in both endpoints' rows
    (dl_score_sampled_train / _logits).  ``dZ_accum`` / ``dH_accum`` (both or neither): the gradient is ADDED onto them in
    place, in the finishing launch.  Every row is written; an entry with k = -1 has score 0 and no part in the loss.
    Duplicates are separate terms.  No float atomics, no host read, no synchronisation; the same bits on every call.
    fp32 tables with K d <= 2048; bf16 tables raise.
    ``k`` may be a ``HardDraw``: the partners are then drawn here, from (Z, H), and ``order`` / ``k_rowptr`` cannot be given."""
    check_hard_draw(k, order, k_rowptr)
    lib = _lib.load()
    if Z.dtype != torch.float32 or H.dtype != torch.float32:
        raise TypeError(f"the sampled trainer takes fp32 tables, got {Z.dtype} / {H.dtype} (bf16 tables are not served)")
    Z, H = _f32c(Z), _f32c(H)
    _need_cuda(Z, H, *(() if isinstance(k, HardDraw) else (k,)))
    N, K, d = _nkd(Z)
    if tuple(H.shape) != tuple(Z.shape):
        raise ValueError("Z and H differ in shape")
    if N != sampled.n_nodes:
        raise ValueError(f"tables of {N} nodes, sampled negatives of {sampled.n_nodes}")
    if isinstance(k, HardDraw):
        k = k.draw(Z, H, t, sampled)
    if not lib.dl_score_sampled_train_supported(K, d, _lib.DL_F32):
        raise _lib.DisenlinkHipError(f"the sampled trainer serves fp32 tables with K <= 64 and K d <= 2048 (got K={K}, d={d}); "
                                     "there is no eager fallback")
    E = sampled.n_entries
    if k.dtype != torch.int32 or k.numel() != E or not k.is_contiguous():
        raise ValueError(f"k must be a contiguous int32 tensor of {E} entries")
    if (order is None) != (k_rowptr is None):
        raise ValueError("order and k_rowptr come together")
    if order is None:
        order, k_rowptr = sampled_order(k, N)
    if order.dtype != torch.int32 or order.numel() != E or k_rowptr.dtype != torch.int32 or k_rowptr.numel() != N + 1:
        raise ValueError("order must be int32 [E] and k_rowptr int32 [N + 1]")
    if (dZ_accum is None) != (dH_accum is None):
        raise ValueError("dZ_accum and dH_accum come together")
    dev = Z.device
    if dZ_accum is None:
        dZ, dH, acc = _empty(Z.shape, torch.float32, dev), _empty(Z.shape, torch.float32, dev), 0
    else:
        for g in (dZ_accum, dH_accum):
            if g.dtype != torch.float32 or tuple(g.shape) != tuple(Z.shape) or not g.is_contiguous():
                raise ValueError("dZ_accum / dH_accum must be contiguous fp32 [N,K,d] tensors")
        dZ, dH, acc = dZ_accum, dH_accum, 1
    score = _empty(E, torch.float32, dev)
    loss = _empty(1, torch.float32, dev)
    entry = "dl_score_sampled_train_logits" if logits else "dl_score_sampled_train"
    ws = _ws.get(max(256, int(getattr(lib, entry + "_workspace_bytes")(E, N, K, d))), dev)
    _lib.check(getattr(lib, entry)(Z.data_ptr(), H.data_ptr(), N, K, d, _lib.DL_F32, float(t), sampled.src.data_ptr(),
                                   sampled.n_rows, sampled.m, sampled.u_rowptr.data_ptr(), k.data_ptr(), order.data_ptr(),
                                   k_rowptr.data_ptr(), float(weight), score.data_ptr(), loss.data_ptr(), dZ.data_ptr(),
                                   dH.data_ptr(), acc, ws.data_ptr(), ws.numel(), _stream()), entry)
    return loss.reshape(()), score, dZ, dH


class SampledLoss(torch.autograd.Function):
    """(Z, H) -> (loss, score [E]) of ``score_sampled_train``; the forward keeps dZ, dH and the backward scales them by the
    gradient arriving on the loss (the scores carry none)."""
    _logits = False

    @classmethod
    def forward(cls, ctx, Z, H, t: float, sampled: SampledNegatives, k, weight: float):
        loss, score, dZ, dH = score_sampled_train(Z, H, t, sampled, k, weight, cls._logits)
        ctx.save_for_backward(dZ, dH)
        ctx.mark_non_differentiable(score)
        return loss, score

    @staticmethod
    def backward(ctx, g_loss, _g_score):
        dZ, dH = ctx.saved_tensors
        return dZ * g_loss, dH * g_loss, None, None, None, None


class SampledLogitsLoss(SampledLoss):
    """``SampledLoss`` in logit space (dl_score_sampled_train_logits): the scores are logits."""
    _logits = True


def score_sampled_loss(Z, H, t: float, sampled: SampledNegatives, k, weight: float):
    """-> (loss, prob [E]), differentiable in (Z, H): the sampled negatives' BCE in probability space (``SampledLoss``)."""
    return SampledLoss.apply(Z, H, float(t), sampled, k, float(weight))


def score_sampled_logits_loss(Z, H, t: float, sampled: SampledNegatives, k, weight: float):
    """-> (loss, logit [E]), differentiable in (Z, H): the same in logit space (``SampledLogitsLoss``)."""
    return SampledLogitsLoss.apply(Z, H, float(t), sampled, k, float(weight))


# ------------------------------------------------------------------------------------------------ pairwise ranking (BPR)
BPR_MAX_M = 63                           # a chunk of the row pass holds floor(64 / (m + 1)) whole rows


def score_sampled_bpr_supported(K: int, d: int, dtype=torch.float32) -> bool:
    code = _lib.DL_F32 if dtype == torch.float32 else _lib.DL_BF16 if dtype == torch.bfloat16 else -1
    return code >= 0 and bool(_lib.load().dl_score_sampled_bpr_train_supported(int(K), int(d), code))


def score_sampled_bpr_train(Z, H, t: float, sampled: SampledNegatives, k, weight: float, order=None, k_rowptr=None, dZ_accum=None,
                            dH_accum=None):
    """-> (loss f32 [], pos_logit f32 [n_rows], neg_logit f32 [E], dZ, dH f32 [N,K,d]): the pairwise ranking loss (BPR) of
    ``sampled`` (built with ``dst``) and this epoch's partners ``k`` — edge row r = (src[r], dst[r]) must score above
    (src[r], k[r m + j]) for its m draws: loss = sum weight softplus(neg_logit - pos_logit[row]) over the entries with k >= 0,
    dZ / dH its gradient, every pair in both endpoints' rows (dl_score_sampled_bpr_train).  Logit space only.  ``pos_logit`` is
    written for every row, ``neg_logit`` is 0 for k = -1; a row whose draws all failed has no loss and no gradient.
    ``dZ_accum`` / ``dH_accum`` (both or neither): the gradient is ADDED onto them in place, in the finishing launch.
    Duplicates are separate terms; k == dst, k == src and dst == src are legal.  No float atomics, no host read, no
    synchronisation; the same bits on every call.  fp32 tables with K d <= 2048 and m <= 63; bf16 tables raise.
    ``k`` may be a ``HardDraw``: the partners are then drawn here, from (Z, H), and ``order`` / ``k_rowptr`` cannot be given."""
    check_hard_draw(k, order, k_rowptr)
    lib = _lib.load()
    if Z.dtype != torch.float32 or H.dtype != torch.float32:
        raise TypeError(f"the ranking trainer takes fp32 tables, got {Z.dtype} / {H.dtype} (bf16 tables are not served)")
    Z, H = _f32c(Z), _f32c(H)
    _need_cuda(Z, H, *(() if isinstance(k, HardDraw) else (k,)))
    N, K, d = _nkd(Z)
    if tuple(H.shape) != tuple(Z.shape):
        raise ValueError("Z and H differ in shape")
    if N != sampled.n_nodes:
        raise ValueError(f"tables of {N} nodes, sampled negatives of {sampled.n_nodes}")
    if sampled.dst is None:
        raise ValueError("the ranking trainer needs the positives: build SampledNegatives(..., dst=...)")
    if sampled.m > BPR_MAX_M:
        raise ValueError(f"the ranking trainer serves m <= {BPR_MAX_M} negatives per row, got m = {sampled.m}")
    if not lib.dl_score_sampled_bpr_train_supported(K, d, _lib.DL_F32):
        raise _lib.DisenlinkHipError(f"the ranking trainer serves fp32 tables with K <= 64 and K d <= 2048 (got K={K}, d={d}); "
                                     "there is no eager fallback")
    if isinstance(k, HardDraw):
        k = k.draw(Z, H, t, sampled)
    E = sampled.n_entries
    if k.dtype != torch.int32 or k.numel() != E or not k.is_contiguous():
        raise ValueError(f"k must be a contiguous int32 tensor of {E} entries")
    if (order is None) != (k_rowptr is None):
        raise ValueError("order and k_rowptr come together")
    if order is None:
        order, k_rowptr = sampled_order(k, N)
    if order.dtype != torch.int32 or order.numel() != E or k_rowptr.dtype != torch.int32 or k_rowptr.numel() != N + 1:
        raise ValueError("order must be int32 [E] and k_rowptr int32 [N + 1]")
    if (dZ_accum is None) != (dH_accum is None):
        raise ValueError("dZ_accum and dH_accum come together")
    dev = Z.device
    if dZ_accum is None:
        dZ, dH, acc = _empty(Z.shape, torch.float32, dev), _empty(Z.shape, torch.float32, dev), 0
    else:
        for g in (dZ_accum, dH_accum):
            if g.dtype != torch.float32 or tuple(g.shape) != tuple(Z.shape) or not g.is_contiguous():
                raise ValueError("dZ_accum / dH_accum must be contiguous fp32 [N,K,d] tensors")
        dZ, dH, acc = dZ_accum, dH_accum, 1
    pos = _empty(sampled.n_rows, torch.float32, dev)
    neg = _empty(E, torch.float32, dev)
    loss = _empty(1, torch.float32, dev)
    ws = _ws.get(max(256, int(lib.dl_score_sampled_bpr_train_workspace_bytes(sampled.n_rows, sampled.m, N, K, d))), dev)
    _lib.check(lib.dl_score_sampled_bpr_train(
        Z.data_ptr(), H.data_ptr(), N, K, d, _lib.DL_F32, float(t), sampled.src.data_ptr(), sampled.dst.data_ptr(), sampled.n_rows,
        sampled.m, sampled.u_rowptr.data_ptr(), sampled.dst_order.data_ptr(), sampled.dst_rowptr.data_ptr(), k.data_ptr(),
        order.data_ptr(), k_rowptr.data_ptr(), float(weight), pos.data_ptr(), neg.data_ptr(), loss.data_ptr(), dZ.data_ptr(),
        dH.data_ptr(), acc, ws.data_ptr(), ws.numel(), _stream()), "dl_score_sampled_bpr_train")
    return loss.reshape(()), pos, neg, dZ, dH


class SampledBprLoss(torch.autograd.Function):
    """(Z, H) -> (loss, pos_logit [n_rows], neg_logit [E]) of ``score_sampled_bpr_train``; the forward keeps dZ, dH and the
    backward scales them by the gradient arriving on the loss (the logits carry none)."""

    @staticmethod
    def forward(ctx, Z, H, t: float, sampled: SampledNegatives, k, weight: float, order=None, k_rowptr=None):
        loss, pos, neg, dZ, dH = score_sampled_bpr_train(Z, H, t, sampled, k, weight, order, k_rowptr)
        ctx.save_for_backward(dZ, dH)
        ctx.mark_non_differentiable(pos, neg)
        return loss, pos, neg

    @staticmethod
    def backward(ctx, g_loss, _g_pos, _g_neg):
        dZ, dH = ctx.saved_tensors
        return dZ * g_loss, dH * g_loss, None, None, None, None, None, None


def score_sampled_bpr_loss(Z, H, t: float, sampled: SampledNegatives, k, weight: float, order=None, k_rowptr=None):
    """-> (loss, pos_logit [n_rows], neg_logit [E]), differentiable in (Z, H): the pairwise ranking loss (``SampledBprLoss``)."""
    return SampledBprLoss.apply(Z, H, float(t), sampled, k, float(weight), order, k_rowptr)
