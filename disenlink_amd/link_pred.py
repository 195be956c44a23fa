"""The dense ``link_pred`` of ``Disentangle.forward(x, adj)``: the [N,N] scorer, its two backwards — on the pair plan of the
caller's loss masks (``DensePairPlanCache``, ``LinkPred``) and on the matrix cores for any gradient — and the autograd
Functions over them.  A leaf: it imports ``_dev``, ``_lib`` and ``graph`` only; ``ops`` re-exports every name.
"""
from __future__ import annotations

import os
import weakref

import torch

from . import _lib
from ._dev import _empty, _f32c, _need_cuda, _nkd, _stream, _tab, _ws
from .graph import PairList


# ---------------------------------------------------------------------- raw wrappers
def score_allpairs_fwd(Z, H, t: float) -> torch.Tensor:
    """-> prob f32[N,N] for all ordered pairs: model.py:109-113 as written, without a pair list."""
    lib = _lib.load()
    (Z, dt), (H, dth) = _tab(Z), _tab(H)
    _need_cuda(Z, H)
    N, K, d = _nkd(Z)
    if H.shape != Z.shape or dt != dth:
        raise ValueError("Z and H differ in shape or storage type")
    prob = _empty((N, N), torch.float32, Z.device)
    ws = _ws.get(int(lib.dl_score_allpairs_workspace_bytes(N, K, d, dt)), Z.device)
    _lib.check(lib.dl_score_allpairs_fwd(Z.data_ptr(), H.data_ptr(), N, K, d, dt, float(t), prob.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream()), "dl_score_allpairs_fwd")
    return prob


def score_allpairs_logits_fwd(Z, H, t: float) -> torch.Tensor:
    """-> logit f32[N,N] for all ordered pairs: model.py:109-113 without its sigmoid (dl_score_allpairs_logits_fwd), the
    tensor ``F.binary_cross_entropy_with_logits`` is written on.  fp32 tables, every d (the matrix-core kernel from planes,
    which pad d to a multiple of 32); symmetric bit for bit.  bf16 tables raise: there is no fallback."""
    lib = _lib.load()
    if Z.dtype != torch.float32 or H.dtype != torch.float32:
        raise TypeError(f"the dense logits take fp32 tables, got {Z.dtype} / {H.dtype}")
    _need_cuda(Z, H)
    Z, H = Z.contiguous(), H.contiguous()
    N, K, d = _nkd(Z)
    if H.shape != Z.shape:
        raise ValueError("Z and H differ in shape")
    logit = _empty((N, N), torch.float32, Z.device)
    ws = _ws.get(max(256, int(lib.dl_score_allpairs_logits_workspace_bytes(N, K, d))), Z.device)
    _lib.check(lib.dl_score_allpairs_logits_fwd(Z.data_ptr(), H.data_ptr(), N, K, d, _lib.DL_F32, float(t), logit.data_ptr(),
                                                ws.data_ptr(), ws.numel(), _stream()), "dl_score_allpairs_logits_fwd")
    return logit


def score_allpairs_bwd(Z, H, pairs: PairList, t: float, prob, g_prob):
    """-> dZ, dH f32[N,K,d]: backward of score_allpairs_fwd on the fixed pair plan ``pairs`` (the support of the
    caller's loss masks); prob and g_prob are the dense [N,N] arrays."""
    lib = _lib.load()
    (Z, dt), (H, _dth), prob, g_prob = _tab(Z), _tab(H), _f32c(prob), _f32c(g_prob)
    _need_cuda(Z, H, prob, g_prob, pairs.inc.rowptr)
    N, K, d = _nkd(Z)
    if tuple(prob.shape) != (N, N) or tuple(g_prob.shape) != (N, N):
        raise ValueError("prob / g_prob must be the dense [N, N] arrays")
    dZ = _empty(Z.shape, torch.float32, Z.device)
    dH = _empty(Z.shape, torch.float32, Z.device)
    P = pairs.n_pairs
    ws = _ws.get(pairs.workspace_bytes(K, d), Z.device)
    _lib.check(lib.dl_score_allpairs_bwd(Z.data_ptr(), H.data_ptr(), N, K, d, dt, float(t), pairs.c_struct(P),
                                         pairs.pu.data_ptr(), pairs.pv.data_ptr(), P, prob.data_ptr(), g_prob.data_ptr(),
                                         dZ.data_ptr(), dH.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "dl_score_allpairs_bwd")
    return dZ, dH


def score_allpairs_bwd_dense_supported(K: int, d: int) -> bool:
    """fp32 tables with 1 <= d <= 128."""
    return bool(_lib.load().dl_score_allpairs_bwd_dense_supported(int(K), int(d)))


def score_allpairs_bwd_dense(Z, H, t: float, prob, g_prob):
    """-> dZ, dH f32[N,K,d]: backward of score_allpairs_fwd for ANY dense gradient ``g_prob`` [N,N] (not necessarily
    symmetric, possibly expanded or transposed: it is made contiguous fp32 here) on the matrix cores
    (dl_score_dense_bwd.hip) — no pair plan, no host read.  ``prob`` is the forward's output.  Every element of dZ and dH
    is written."""
    return _bwd_dense(Z, H, t, prob, g_prob)


def score_allpairs_logits_bwd_dense(Z, H, t: float, g_logit):
    """-> dZ, dH f32[N,K,d]: backward of score_allpairs_logits_fwd for ANY dense gradient ``g_logit`` [N,N] with respect to
    the logits (dl_score_allpairs_logits_bwd_dense): G^ = g + g^T with no p (1 - p) factor and no saved forward output;
    everything else, limits included, is ``score_allpairs_bwd_dense``."""
    return _bwd_dense(Z, H, t, None, g_logit)


def _bwd_dense(Z, H, t, prob, g):
    """The dense backward of either score space; ``prob`` None: ``g`` is the gradient with respect to the logits."""
    lib = _lib.load()
    logits = prob is None
    Z, H = _f32c(Z), _f32c(H)
    if not logits:
        prob = _f32c(prob)
    _need_cuda(Z, H, g, *(() if logits else (prob,)))
    N, K, d = _nkd(Z)
    if H.shape != Z.shape:
        raise ValueError("Z and H differ in shape")
    if logits:
        if tuple(g.shape) != (N, N):
            raise ValueError("g_logit must be the dense [N, N] array")
    elif tuple(prob.shape) != (N, N) or tuple(g.shape) != (N, N):
        raise ValueError("prob / g_prob must be the dense [N, N] arrays")
    if not lib.dl_score_allpairs_bwd_dense_supported(K, d):
        raise _lib.DisenlinkHipError(f"the dense backward of link_pred serves fp32 tables with 1 <= d <= 128 (got K = {K}, "
                                     f"d = {d}); there is no eager fallback")
    g = g.to(torch.float32).contiguous()                        # stride-0 (mean()) and transposed gradients arrive here
    dZ = _empty(Z.shape, torch.float32, Z.device)
    dH = _empty(Z.shape, torch.float32, Z.device)
    ws = _ws.get(int(lib.dl_score_allpairs_bwd_dense_workspace_bytes(N, K, d)), Z.device)
    if logits:
        _lib.check(lib.dl_score_allpairs_logits_bwd_dense(Z.data_ptr(), H.data_ptr(), N, K, d, float(t), g.data_ptr(),
                                                          dZ.data_ptr(), dH.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                   "dl_score_allpairs_logits_bwd_dense")
    else:
        _lib.check(lib.dl_score_allpairs_bwd_dense(Z.data_ptr(), H.data_ptr(), N, K, d, float(t), prob.data_ptr(),
                                                   g.data_ptr(), dZ.data_ptr(), dH.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   _stream()), "dl_score_allpairs_bwd_dense")
    return dZ, dH


# ---------------------------------------------------------------------- the pair plan of the caller's loss
class DensePairPlanCache:
    """Pair plan of the dense [N,N] score gradient's support — owned by ONE module (no process-wide state).

    The reference's caller takes its loss on ``link_pred[mask == 1]`` with masks that are fixed for a run
    (main_disentangled.py:167-190,195), so d loss / d link_pred can be non-zero only on the masks' support.  The plan
    must be keyed on THAT support, not on the entries of the gradient that happen to be non-zero: a saturated positive
    (p == 1.0 in fp32, y == 1) has exactly zero BCE gradient in one epoch and a non-zero one in the next (SURVEY.md §0
    finding 4), so the gradient's non-zero set moves under fixed masks.

      * ``set_pairs(masks ...)`` (Disentangle.set_loss_pairs / assume_static_loss_masks(mask, ...)): the plan IS the
        support of the caller's masks; entries whose gradient is zero cost a little arithmetic and add exactly zero.
      * no masks given: the plan is learnt — first from the caller's own INDEXING of link_pred (round 6: forward returns
        a LinkPred, a Tensor subclass whose only difference is that ``link_pred[mask]`` / ``link_pred[rows, cols]`` tells
        this cache the support of the index before handing over to torch: main_disentangled.py:195, 202 index it with
        the fixed masks every epoch, so after the first epoch the plan is their union and never changes again), and, as
        the safety net behind that, from the gradients: a backward whose non-zero entries are not all inside the cached
        set extends it by the new ones (union) and rebuilds; it never shrinks to the current non-zero set.  (Learning
        from the gradients ALONE rebuilt the plan in every one of the first 40 epochs on squirrel and chameleon — each
        epoch desaturates a few more pairs — 4 ms per epoch: profiles/r7d_dropin_*.)
      * validation: non-zeros(g) must be a SUBSET of the plan.  Default: two device counters are read back per backward
        (one 16-byte host read; the reference's own loop reads back the validation scores and the loss every epoch,
        main_disentangled.py:204,214).  ``static=True`` (needs masks): no host read — the same two counters stay on
        the device and become a validity factor, 1 if the subset relation holds, NaN if not, multiplied into the
        gradients: a caller that promised fixed masks and takes a loss elsewhere gets NaN gradients at once, never
        silently wrong ones."""

    def __init__(self):
        self.pairs = None        # PairList of the cached index set
        self.flat = None         # int64 [n] row-major positions, ascending
        self.key = None          # (N, device)
        self.static = False
        self.from_masks = False  # the set is the caller's declared support (never extended behind their back)
        self.rebuilds = 0        # how often the plan was (re)built: a learnt plan is rebuilt whenever new entries carry gradient
        self._seen_index = set() # fingerprints of the index masks link_pred was indexed with (note_index)
        self._seen_ij = []       # (rows, cols) index tensors seen: weak references + version counters
        self._pending = []       # flat positions learnt from indexing, not yet in the plan
        self._hash_vec = None

    # ---- the caller's declared support
    def set_pairs(self, N: int, device, *supports):
        """``supports``: dense [N,N] masks (entries != 0 belong to the support: the caller's summed train masks hold
        2, 3, ... where index pairs repeat, main_disentangled.py:176-179 — those entries are outside the loss and get
        zero gradient, which is harmless here) and / or (rows, cols) index tuples.  The plan is the union."""
        flats = []
        for sup in supports:
            if isinstance(sup, (tuple, list)):
                r, c = (torch.as_tensor(v, device=device).reshape(-1).long() for v in sup)
                if r.numel() != c.numel():
                    raise ValueError("(rows, cols) differ in length")
                if r.numel() and (int(r.min()) < 0 or int(c.min()) < 0 or int(r.max()) >= N or int(c.max()) >= N):
                    raise ValueError("pair index outside [0, N)")
                flats.append(r * N + c)
            else:
                m = torch.as_tensor(sup, device=device)
                if m.dim() != 2 or m.shape[0] != N or m.shape[1] != N:
                    raise ValueError(f"a loss mask must be [N, N] = [{N}, {N}], got {tuple(m.shape)}")
                flats.append(torch.nonzero(m.reshape(-1)).reshape(-1))
        if not flats:
            raise ValueError("no loss masks / pairs given")
        self._install(torch.unique(torch.cat(flats)), N, device)
        self.from_masks = True

    def clear(self):
        self.pairs = self.flat = self.key = None
        self.from_masks = False
        self._seen_index, self._seen_ij, self._pending = set(), [], []

    # ---- learnt from the caller's indexing of link_pred (LinkPred.__torch_function__)
    def note_index(self, N: int, index) -> None:
        """``link_pred[index]`` is about to be evaluated: remember the support of a boolean [N,N] mask or of a
        (rows, cols) pair of index tensors.  A mask is recognised by a fingerprint (count, hashed row sums, hashed
        column sums: two reductions over the mask and one 24-byte read — the indexing that follows synchronises anyway),
        so the masks the loop passes every epoch cost a nonzero() once."""
        if self.from_masks or self.static:
            return                                                  # the caller declared the support: nothing to learn
        try:
            if torch.is_tensor(index) and index.dtype == torch.bool and tuple(index.shape) == (N, N) and index.is_cuda:
                # the mask's bytes as 8-byte words against a fixed random int64 vector (wrapping multiply-add): one fused pass over
                # N*N bytes (the first form — row and column sums of the bool matrix — cost 1.2 ms per epoch on squirrel)
                flat = index.reshape(-1)
                n8 = flat.numel() // 8
                if self._hash_vec is None or self._hash_vec.numel() != n8 or self._hash_vec.device != index.device:
                    g = torch.Generator().manual_seed(0x5eed)
                    self._hash_vec = torch.randint(-(1 << 62), 1 << 62, (n8,), generator=g, dtype=torch.int64).to(index.device)
                words = flat[:n8 * 8].view(torch.int64)
                fp = tuple(torch.stack([(words * self._hash_vec).sum(),
                                        words.sum(), flat[n8 * 8:].sum()]).tolist())
                if fp in self._seen_index:
                    return
                self._seen_index.add(fp)
                self._pending.append(torch.nonzero(index.reshape(-1)).reshape(-1))
            elif isinstance(index, tuple) and len(index) == 2 and all(torch.is_tensor(v) and v.dtype == torch.int64 and v.dim() == 1
                                                                        for v in index) and index[0].is_cuda:
                # recognised by the tensor OBJECTS and their version counters (no device read: this form of indexing does not
                # synchronise) — not by addresses: index tensors made afresh every epoch come back at the address of the ones
                # just freed, with other contents
                rows, cols = index
                for r0, r1, v0, v1 in self._seen_ij:
                    if r0() is rows and r1() is cols and (v0, v1) == (rows._version, cols._version):
                        return
                self._seen_ij.append((weakref.ref(rows), weakref.ref(cols), rows._version, cols._version))
                del self._seen_ij[:-16]
                self._pending.append((rows % N) * N + (cols % N))
            if len(self._pending) > 32:                             # many gathers between two backwards: keep one merged set
                self._pending = [torch.unique(torch.cat(self._pending))]
        except RuntimeError:                                        # an index torch itself will reject: let torch say so
            return

    def _install(self, flat: torch.Tensor, N: int, device):
        self.flat = flat
        # (only the incidence plan is walked by dl_score_allpairs_bwd: the forward plan of the list is not built)
        self.pairs = PairList.build(torch.div(flat, N, rounding_mode="floor"), flat % N, N, build_by_u=False)
        self.key = (N, device)
        self.rebuilds += 1

    # ---- per backward
    def lookup(self, g_prob: torch.Tensor):
        """-> (pairs, validity factor or None)"""
        N = g_prob.shape[0]
        g_flat = g_prob.reshape(-1)
        key = (N, g_prob.device)
        if self.pairs is not None and self.key != key:
            if self.from_masks:
                raise ValueError(f"the loss pairs were declared for {self.key}, the gradient is for {key}")
            self.clear()
        if self._pending and not self.from_masks:                   # supports learnt from the caller's indexing since the last backward
            known = [self.flat] if self.flat is not None and self.key == key else []
            self._install(torch.unique(torch.cat(known + self._pending)), N, g_prob.device)
            self._pending = []
        if self.pairs is None:
            if self.static:
                raise RuntimeError("assume_static_loss_masks() needs the masks (or index pairs) the loss is taken on: "
                                   "the support of a loss cannot be read off one gradient")
            self._install(torch.nonzero(g_flat).reshape(-1), N, g_prob.device)
            return self.pairs, None
        # non-zeros(g) inside the plan == non-zeros(g) anywhere  <=>  subset
        probe = torch.stack([torch.count_nonzero(g_flat), torch.count_nonzero(g_flat[self.flat])])
        if self.static:
            return self.pairs, torch.where(probe[0] == probe[1], 1.0, float("nan")).to(torch.float32)
        cnt, kept = probe.tolist()
        if cnt != kept:
            if self.from_masks:
                raise RuntimeError(f"{cnt - kept} entries of d loss / d link_pred lie outside the declared loss pairs "
                                   "(Disentangle.set_loss_pairs): declare every mask the loss indexes link_pred with")
            self._install(torch.unique(torch.cat([self.flat, torch.nonzero(g_flat).reshape(-1)])), N, g_prob.device)
        return self.pairs, None


class LinkPred(torch.Tensor):
    """The dense link_pred of Disentangle.forward(x, adj): a torch.Tensor in every respect, except that indexing it —
    ``a_pred[pos_train_adj == 1]`` (main_disentangled.py:195, 202, 217) — first tells the owning module's DensePairPlanCache
    which entries are being taken (note_index), so that the dense backward knows the support of the caller's loss without
    a declaration and without learning it from gradients whose zero pattern moves.  Every operation, indexing included, is
    then torch's own, and every result is a plain torch.Tensor."""
    _dl_cache = None

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        if func is torch.Tensor.__getitem__ and len(args) == 2 and isinstance(args[0], LinkPred):
            cache = args[0]._dl_cache
            # (only where a backward can follow: an evaluation loop under no_grad indexes without end and never consumes
            # what it reported)
            if cache is not None and args[0].dim() == 2 and args[0].requires_grad and torch.is_grad_enabled():
                cache.note_index(int(args[0].shape[0]), args[1])
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **(kwargs or {}))

    # Copies and serialised forms are DATA: plain tensors, without the owning module's cache (torch's default __deepcopy__
    # refuses a subclass without new_empty(); pickling the subclass would drag the cache along and break weights_only loads).
    def __deepcopy__(self, memo):
        return self.as_subclass(torch.Tensor).__deepcopy__(memo)

    def __reduce_ex__(self, proto):
        return self.as_subclass(torch.Tensor).__reduce_ex__(proto)


def as_link_pred(prob: torch.Tensor, cache: "DensePairPlanCache") -> torch.Tensor:
    if os.environ.get("DL_LINK_PRED_SUBCLASS", "1") == "0":        # plain tensor: the plan is learnt from the gradients alone
        return prob
    out = prob.as_subclass(LinkPred)
    out._dl_cache = cache
    return out


# ---------------------------------------------------------------------- autograd
def _forward(ctx, Z, H, t: float) -> torch.Tensor:
    """The forward of both Functions: link_pred of fp32 tables, kept with them for the backward."""
    Z, H = _f32c(Z), _f32c(H)
    prob = score_allpairs_fwd(Z, H, t)
    ctx.t = t
    ctx.save_for_backward(Z, H, prob)
    return prob


class ScoreAllPairs(torch.autograd.Function):
    """(Z, H) -> prob [N,N], the dense output the reference's caller indexes with masks
    (main_disentangled.py:195).  Backward: dl_score_allpairs_bwd on the pair plan of ``cache`` (the calling module's
    DensePairPlanCache: the support of the caller's loss masks)."""

    @staticmethod
    def forward(ctx, Z, H, t: float, cache: "DensePairPlanCache | None" = None):
        ctx.cache = cache if cache is not None else DensePairPlanCache()
        return _forward(ctx, Z, H, t)

    @staticmethod
    def backward(ctx, g_prob):
        Z, H, prob = ctx.saved_tensors
        pairs, valid = ctx.cache.lookup(g_prob)
        dZ, dH = score_allpairs_bwd(Z, H, pairs, ctx.t, prob, g_prob)
        if valid is not None:
            dZ, dH = dZ * valid, dH * valid
        return dZ, dH, None, None


class ScoreAllPairsDense(torch.autograd.Function):
    """ScoreAllPairs' forward with the dense backward: the gradient of whatever the caller does with link_pred, as the
    reference's autograd gives it (model.py:109-113, main_disentangled.py:198) — no plan, no declaration, no host read."""

    @staticmethod
    def forward(ctx, Z, H, t: float):
        return _forward(ctx, Z, H, t)

    @staticmethod
    def backward(ctx, g_prob):
        Z, H, prob = ctx.saved_tensors
        dZ, dH = score_allpairs_bwd_dense(Z, H, ctx.t, prob, g_prob)
        return dZ, dH, None


class ScoreAllPairsLogits(torch.autograd.Function):
    """(Z, H) -> logit [N,N] (score_allpairs_logits_fwd), a plain tensor for ``F.binary_cross_entropy_with_logits``; the
    backward is the dense one (score_allpairs_logits_bwd_dense) and the only one: there is no pair plan in logit space.
    Shapes the dense backward does not serve (d > 128) and non-fp32 tables raise in the forward."""

    @staticmethod
    def forward(ctx, Z, H, t: float):
        if Z.dtype != torch.float32 or H.dtype != torch.float32:
            raise TypeError(f"link_logits takes fp32 tables, got {Z.dtype} / {H.dtype}")
        N, K, d = _nkd(Z)
        if not score_allpairs_bwd_dense_supported(K, d):
            raise _lib.DisenlinkHipError(f"link_logits serves fp32 tables with 1 <= d <= 128, the shapes of its dense backward "
                                         f"(got K = {K}, d = {d}); there is no eager fallback")
        Z, H = Z.contiguous(), H.contiguous()
        ctx.t = t
        ctx.save_for_backward(Z, H)
        return score_allpairs_logits_fwd(Z, H, t)

    @staticmethod
    def backward(ctx, g_logit):
        Z, H = ctx.saved_tensors
        dZ, dH = score_allpairs_logits_bwd_dense(Z, H, ctx.t, g_logit)
        return dZ, dH, None
