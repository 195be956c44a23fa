"""The whole-graph reconstruction objective over libdisenlink_hip.so (dl_score_recon): every non-edge is a negative, the
positives are up-weighted, and loss and gradient come from one call that forms nothing of size N x N.  A leaf beside
``scans``: it imports ``_dev``, ``_lib`` and the set normalisation of ``scans``; ``ops`` re-exports the public names.

The contract (restated in fp64 by tests/recon_ref.py).  Included pairs: all unordered {u, v}, u != v, outside ``ignore``;
a pair listed in both sets is ignored.  For an included pair, with s = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t) and
p = sigmoid(s):  y = 1 if the pair is in ``positives`` else 0;  w = pos_weight / C for y = 1, else 1 / C, with
C = n_pos + n_neg the number of included pairs;  loss = sum w BCE(p, y) with F.binary_cross_entropy's clamps;
d loss / d s = w (p - y) in the one-pass scorer's form (saturated pairs contribute exactly 0).  No tile of the scan is
skipped: a zero gradient against an overflowed exp(z.z / t) = inf gives NaN in dZ / dH, exactly as the dense backward
(``score_allpairs_bwd_dense``) documents — it is the same kernel.

bf16 tables (``table_dtype=torch.bfloat16``, the scans' keyword and convention): the tables are their own single bf16
plane, so scan and backward issue 10 matrix-core products per (tile pair, factor, K block) instead of 36 and the workspace
is 16 K Np dp bytes smaller (dl_score_recon_dtype with DL_BF16).  Every finite output has the bits of the fp32 call on the
same tables widened to fp32; gradients are fp32, with respect to the rounded tables.

Node-group rule (``node_filter``, an ``ops.NodeFilter``; dl_score_recon_filtered, dl_score_recon_logits_filtered): the
included pairs are further those the UNORDERED rule admits, ``node_filter.allowed(u, v, unordered=True)`` — a rule with no
symmetric form raises ValueError before any launch, as in ``score_mine``.  A denied pair behaves exactly like an ignored one,
whether it is an edge or not: no loss term, G^ = 0, not counted.  C = n_pos + n_neg counts included pairs only, so w_pos, w_neg
and the default pos_weight = n_neg / n_pos come from the filtered counts; with nothing included the loss is 0, the gradients
are zero and the counts (0, 0).  No tile is skipped under a rule either, and every guarantee below holds with one.  The rule
travels in the prepared sets (``ReconSets.node_filter``): whatever takes prepared sets reads it from there.

Logit space (``score_recon_logits_loss``, ``ReconLogitsLoss``; dl_score_recon_logits, restated by tests/recon_logits_ref.py):
the same pairs, labels and weights with loss = sum w (max(s, 0) - s y + log1p(exp(-|s|))) and d loss / d s =
w (sigmoid(s) - y), neither clamped: what the fp32 sigmoid saturates (s > 16.64; p (1 - p) < 1e-12 below -27.6) keeps its
cost and its gradient.  The probability and logit forms share every body here through a private flag.
"""
from __future__ import annotations

from collections import namedtuple

from types import SimpleNamespace

import torch

from . import _lib
from ._dev import _empty, _need_cuda, _nkd, _stream, _ws
from .scans import _csr_args, _csr_rows, _exclusion_arg, _filter_arg, _filter_check, _scan_dtype, exclusion_csr


ReconSets = namedtuple("ReconSets", ["n_nodes", "pos_rowptr", "pos_col", "ign_rowptr", "ign_col", "n_pos", "n_neg", "n_ignored",
                                     "node_filter"], defaults=(None,))
ReconSets.__doc__ = """The two pair sets of the reconstruction loss, normalised once (``recon_sets``): symmetric CSRs (int32, every
pair in both of its rows, columns ascending and distinct) of the positives that are not ignored and of the ignored pairs
(``ign_*`` None where there are none), and the host's counts: ``n_pos`` included positives, ``n_neg`` = N (N - 1) / 2 -
n_ignored - n_pos included negatives.  ``node_filter`` (None: no rule): the node-group rule the sets were normalised under;
no pair it denies stands in either CSR, ``n_ignored`` counts the ignored pairs it admits and ``n_neg`` = the pairs it admits -
n_ignored - n_pos.  A caller with fixed sets passes the result instead of the raw sets and skips the
normalisation, and its host read, per call."""


def _unordered_keys(pairs, N: int, device) -> torch.Tensor:
    """int64 keys u * N + v, u < v, ascending and distinct, of a set of unordered pairs in any form ``pair_exclusion``
    takes (a ``Graph``, a dense [N,N] mask, ``(rows, cols)`` or a prepared ``PairExclusion``): either orientation, duplicates
    collapsed, self pairs dropped."""
    if pairs is None:
        return torch.zeros(0, dtype=torch.int64, device=device)
    ex = _exclusion_arg(pairs, N, torch.device(device), keyed=False)
    if ex.rowptr is None:
        return torch.zeros(0, dtype=torch.int64, device=device)
    rows, cols = _csr_rows(ex.rowptr), ex.col.to(torch.int64)          # column max(a, b) of row min(a, b)
    keep = cols > rows
    return rows[keep] * N + cols[keep]


def _symmetric_csr(key: torch.Tensor, N: int, device):
    u = torch.div(key, N, rounding_mode="floor")
    v = key - u * N
    return exclusion_csr((torch.cat([u, v]), torch.cat([v, u])), N, device)


def _admitted(key: torch.Tensor, N: int, node_filter) -> torch.Tensor:
    """bool per key u * N + v: does the unordered rule admit the pair?"""
    u = torch.div(key, N, rounding_mode="floor")
    return node_filter.allowed(u, key - u * N, unordered=True)


def _first(key: torch.Tensor, keep: torch.Tensor, n: int) -> torch.Tensor:
    """The n keys that ``keep`` marks, in their order, where n is already known on the host (no further read)."""
    return key[torch.argsort(~keep, stable=True)[:n]]


def recon_sets(positives, ignore, N: int, device, node_filter=None) -> ReconSets:
    """Normalise ``positives`` and ``ignore`` (each whatever ``pair_exclusion`` accepts; ``ignore`` may be None) for
    ``score_recon_loss``: self pairs and duplicates go, an asymmetric listing is symmetrised, a pair in both sets is ignored.
    ``node_filter`` (an ``ops.NodeFilter`` over the N nodes, on ``device``): pairs its unordered rule denies go from both
    sets, the counts are those of the pairs it admits, and the sets carry it; an asymmetric rule, a filter of another node
    count or on another device raises ValueError.  ONE host read (the two set sizes and, under a rule, the number of pairs
    it admits, together)."""
    N, device = int(N), torch.device(device)
    _filter_check(node_filter, SimpleNamespace(shape=(N,)), True)
    pos, ign = _unordered_keys(positives, N, device), _unordered_keys(ignore, N, device)
    if node_filter is not None and node_filter.groups.device != pos.device:      # (pos.device: "cuda" with its index)
        raise ValueError(f"node filter on {node_filter.groups.device}, reconstruction sets on {pos.device}: use NodeFilter.to(device)")
    if node_filter is None:
        if ign.numel() and pos.numel():
            pos = pos[~torch.isin(pos, ign)]
        n_pos, n_ign = int(pos.numel()), int(ign.numel())               # (sizes of device tensors: the host read)
        n_pairs = N * (N - 1) // 2
    else:
        keep_p, keep_i = _admitted(pos, N, node_filter), _admitted(ign, N, node_filter)
        if ign.numel() and pos.numel():
            keep_p &= ~torch.isin(pos, ign)
        n_pos, n_ign, n_pairs = (int(c) for c in torch.cat([keep_p.sum().reshape(1), keep_i.sum().reshape(1),
                                                            node_filter._n_pairs_allowed()]).tolist())     # the host read
        pos, ign = _first(pos, keep_p, n_pos), _first(ign, keep_i, n_ign)
    pr, pc = _symmetric_csr(pos, N, device)
    ir, ic = _symmetric_csr(ign, N, device) if n_ign else (None, None)
    return ReconSets(N, pr, pc, ir, ic, n_pos, n_pairs - n_ign - n_pos, n_ign, node_filter)


def _own_filter(sets, node_filter) -> None:
    """A node filter beside prepared sets must be the sets' own object (or None)."""
    if isinstance(sets, ReconSets) and node_filter is not None and node_filter is not sets.node_filter:
        raise ValueError("prepared ReconSets carry their node filter (recon_sets(..., node_filter=...)): pass "
                         "node_filter=None or the sets' own")


def _sets_arg(positives, ignore, N: int, device, node_filter=None) -> ReconSets:
    if isinstance(positives, ReconSets):
        if ignore is not None:
            raise ValueError("prepared ReconSets carry their ignored pairs: pass ignore=None")
        _own_filter(positives, node_filter)
        if positives.n_nodes != N:
            raise ValueError(f"reconstruction sets of {positives.n_nodes} nodes, tables of {N}")
        if positives.pos_rowptr.device != device:
            raise ValueError(f"reconstruction sets on {positives.pos_rowptr.device}, tables on {device}")
        return positives
    return recon_sets(positives, ignore, N, device, node_filter)


def _recon_tables(Z, H, table_dtype=torch.float32):
    """[N,K,d] tables on the device with 1 <= d <= 128 -> (Z, H, N, K, d, dl_dtype); anything else raises (there is no
    fallback).  ``table_dtype=torch.float32`` (the default): fp32 tensors, nothing else.  ``torch.bfloat16``: Z and H are both
    bf16 tensors, used as they are, or both fp32 tensors, rounded to nearest-even here (``scans._rank_tables``' rule)."""
    dt = _scan_dtype(table_dtype)
    if dt == _lib.DL_F32:
        if Z.dtype != torch.float32 or H.dtype != torch.float32:
            raise TypeError(f"the reconstruction loss takes fp32 tables, got {Z.dtype} / {H.dtype} "
                            f"(bf16 tables: table_dtype=torch.bfloat16)")
    else:
        if Z.dtype != H.dtype or Z.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"table_dtype=torch.bfloat16 takes Z and H both bf16 or both fp32, got {Z.dtype} / {H.dtype}")
        _need_cuda(Z, H)
        Z, H = Z.to(torch.bfloat16), H.to(torch.bfloat16)
    _need_cuda(Z, H)
    N, K, d = _nkd(Z)
    if tuple(H.shape) != tuple(Z.shape):
        raise ValueError("Z and H differ in shape")
    if N < 1 or not _lib.load().dl_score_recon_supported(K, d):
        raise _lib.DisenlinkHipError(f"the reconstruction loss serves N >= 1, K <= 64 and 1 <= d <= 128 (got N={N}, K={K}, "
                                     f"d={d}); there is no eager fallback")
    return Z.contiguous(), H.contiguous(), N, K, d, dt


def recon_weights(sets: ReconSets, pos_weight=None):
    """(w_pos, w_neg) = (pos_weight / C, 1 / C), C = n_pos + n_neg; ``pos_weight`` defaults to n_neg / n_pos (1 where
    there is no positive).  No included pair at all: (0, 0)."""
    C = sets.n_pos + sets.n_neg
    if C <= 0:
        return 0.0, 0.0
    if pos_weight is None:
        pos_weight = sets.n_neg / sets.n_pos if sets.n_pos else 1.0
    return float(pos_weight) / C, 1.0 / C


def _block_rows(block_rows) -> int:
    b = 0 if block_rows is None else int(block_rows)
    if b < 0 or b % 128:
        raise ValueError(f"block_rows must be a positive multiple of 128 (or None for the default), got {block_rows}")
    return b


def score_recon_loss(Z, H, t: float, positives, ignore=None, pos_weight=None, block_rows=None, table_dtype=torch.float32,
                     node_filter=None):
    """-> (loss f64 [], dZ f32 [N,K,d], dH f32 [N,K,d], counts int64 [2]): the whole-graph reconstruction loss of the
    module docstring and its gradient with respect to the tables, by strips of ``block_rows`` rows (None: the largest
    multiple of 128 whose strip of G^ stays at or under 1 GiB — the whole graph where that fits).  ``positives`` /
    ``ignore``: unordered pair sets as ``pair_exclusion`` takes them, or ``positives`` = a prepared ``recon_sets(...)`` (then
    no host read happens here).  ``counts`` = the included positives and negatives the scan saw, DEVICE values to compare
    with the sets' ``n_pos`` / ``n_neg`` wherever the caller synchronises anyway (``check_recon_counts``).  fp32 tables
    with 1 <= d <= 128, anything else raises; ``table_dtype=torch.bfloat16``: bf16 tables (both tensors bf16, or both fp32 and
    rounded to nearest-even here; a mix raises TypeError), the one-plane kernels, the bits of the fp32 call on the rounded
    tables, and dZ / dH (fp32) with respect to the rounded tables.  ``node_filter`` (raw sets only: prepared sets carry their
    own, and another beside them raises ValueError): the node-group rule of the module docstring — a denied pair is an ignored
    one, counts, weights and the default ``pos_weight`` are those of the admitted pairs.  No float atomics, no host read and no synchronisation in
    the call; launches follow the current stream; the same bits on every call, for every ``block_rows`` and every
    DL_RANK_SLICES."""
    return _score_recon(Z, H, t, positives, ignore, pos_weight, block_rows, table_dtype, False, node_filter)


def score_recon_logits_loss(Z, H, t: float, positives, ignore=None, pos_weight=None, block_rows=None, table_dtype=torch.float32,
                            node_filter=None):
    """``score_recon_loss`` in LOGIT space (dl_score_recon_logits): the same sets, rule, weights, strips, outputs and guarantees,
    with loss = sum w l(s, y), l = max(s, 0) - s y + log1p(exp(-|s|)) (``F.binary_cross_entropy_with_logits``) and
    d loss / d s = w (sigmoid(s) - y) without a clamp: a pair past the saturation of the fp32 sigmoid (s > 16.64, or
    s < -27.6 on a positive) keeps its cost and its gradient, where the probability form charges 100 w and returns exactly 0.
    Logit space does not cure an overflowed exp(z.z / t): a non-finite logit gives a non-finite loss and gradients."""
    return _score_recon(Z, H, t, positives, ignore, pos_weight, block_rows, table_dtype, True, node_filter)


def _score_recon(Z, H, t, positives, ignore, pos_weight, block_rows, table_dtype, logits, node_filter=None):
    _filter_check(node_filter, Z, True)                                # the rule's refusals, ahead of the tables' own
    _own_filter(positives, node_filter)
    Z, H, N, K, d, dt = _recon_tables(Z, H, table_dtype)
    sets = _sets_arg(positives, ignore, N, Z.device, node_filter)
    return _recon_call(Z, H, N, K, d, float(t), sets, recon_weights(sets, pos_weight), _block_rows(block_rows), dt, logits)


def _recon_call(Z, H, N, K, d, t, sets, weights, block_rows, dt=_lib.DL_F32, logits=False):
    lib = _lib.load()
    entry = "dl_score_recon_logits" if logits else "dl_score_recon_dtype"     # one argument list, one workspace
    dev = Z.device
    rule = ()
    if sets.node_filter is not None:                                    # the sets' rule: the _filtered entry, the rule last
        entry = "dl_score_recon_logits_filtered" if logits else "dl_score_recon_filtered"
        nf, keep_f = _filter_arg(sets.node_filter, N, dev, True)
        rule = (nf,)
    loss = _empty((1,), torch.float64, dev)
    counts = _empty((2,), torch.int64, dev)
    dZ, dH = _empty(Z.shape, torch.float32, dev), _empty(Z.shape, torch.float32, dev)
    pr, pc, keep_p = _csr_args(sets.pos_rowptr, sets.pos_col, dev)
    ir, ic, keep_i = _csr_args(sets.ign_rowptr, sets.ign_col, dev)
    ws = _ws.get(max(256, int(lib.dl_score_recon_workspace_bytes_dtype(N, K, d, dt, block_rows))), dev)
    _lib.check(getattr(lib, entry)(Z.data_ptr(), H.data_ptr(), N, K, d, dt, t, pr, pc, ir, ic, weights[0], weights[1],
                                   block_rows, loss.data_ptr(), counts.data_ptr(), dZ.data_ptr(), dH.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _stream(), *rule), entry)
    del keep_p, keep_i, rule
    return loss.reshape(()), dZ, dH, counts


def check_recon_counts(counts, sets: ReconSets) -> None:
    """The scans' "exact count" check: ``counts`` (a host list or a tensor: then this synchronises) against the host's
    n_pos and n_neg = N (N - 1) / 2 - |ignored| - n_pos (under the sets' node filter: the pairs it admits in place of
    N (N - 1) / 2, the ignored and the positives among them); a mismatch raises."""
    got = [int(c) for c in (counts.tolist() if torch.is_tensor(counts) else counts)]
    if got != [sets.n_pos, sets.n_neg]:
        raise _lib.DisenlinkHipError(f"the reconstruction scan saw {got[0]} positives and {got[1]} negatives, the host counts "
                                     f"{sets.n_pos} and {sets.n_neg}")


class ReconLoss(torch.autograd.Function):
    """(Z, H) -> loss (fp32 scalar) of ``score_recon_loss``; the forward keeps dZ, dH and the backward scales them by the
    incoming scalar.  ``sets``: a prepared ``recon_sets(...)``, whose node filter, if it has one, is the rule of the loss.  ``table_dtype=torch.bfloat16``: the tables as
    ``score_recon_loss`` takes them; the rounding passes the gradient straight through (as ``ops.HotPathPairs``).  The device
    counts of the last forward stand in ``ReconLoss.last_counts`` for ``check_recon_counts``."""
    last_counts = None
    _logits = False

    @classmethod
    def forward(cls, ctx, Z, H, t: float, sets: ReconSets, pos_weight=None, block_rows=None, table_dtype=torch.float32):
        Z, H, N, K, d, dt = _recon_tables(Z, H, table_dtype)
        sets = _sets_arg(sets, None, N, Z.device)
        loss, dZ, dH, counts = _recon_call(Z, H, N, K, d, float(t), sets, recon_weights(sets, pos_weight), _block_rows(block_rows),
                                           dt, cls._logits)
        ctx.save_for_backward(dZ, dH)
        cls.last_counts = counts
        return loss.to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        dZ, dH = ctx.saved_tensors
        return dZ * g, dH * g, None, None, None, None, None


class ReconLogitsLoss(ReconLoss):
    """``ReconLoss`` over ``score_recon_logits_loss``: the same node, the logit-space entry; its device counts stand in
    ``ReconLogitsLoss.last_counts``."""
    last_counts = None
    _logits = True
