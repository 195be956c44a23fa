"""The projection Z [N,K,d] = K MLPs of x (model.py:13-15 / 24-27 / 106) over libdisenlink_hip.so: the caches of what the
kernels read for a feature tensor (its zero-padded copy, its persistent bf16 planes), the raw wrappers of the dense and the
sparse kernels, and the one ``autograd.Function`` over them.  ``ops`` re-exports every name (``ops.project_fwd`` as before).

Three things are written once here and used by all four wrappers: the tile width (``_tile`` refuses d > 128, ``_at_tile``
zero-pads the LAST layer's output rows to 32 / 64 / 128, ``_trim_grads`` cuts the results back to d), the carve of the
gradients out of one allocation (``_carve``) and the choice of weights and saved state in ``Project``.
"""
from __future__ import annotations

import os
import weakref

import torch

from . import _lib
from ._dev import _empty, _f32c, _need_cuda, _stream, _ws
from .features import SparseFeatures


class _PaddedFeatures:
    """Zero-padded copies of feature matrices whose row length is not a multiple of 4, one per source TENSOR and version
    counter.  Entries are keyed by the tensor OBJECT (its id, checked against a weak reference: an address — or an id —
    can be reused by another tensor once this one is gone, a live object cannot) and are dropped when their tensor dies.
    The padded copy is what the kernels — and any captured HIP graph — read, so it must live exactly as long as the
    caller's x does: with one entry per tensor, a second model, an evaluation on other features or a second run in the
    same process cannot evict the copy a live graph still replays (train._graphed_epoch also holds it)."""

    def __init__(self):
        self._by_id: dict = {}

    def get(self, x: torch.Tensor, Fp: int) -> torch.Tensor:
        key = id(x)
        hit = self._by_id.get(key)
        if hit is None or hit[0]() is not x or hit[1] != x._version or hit[2].shape[1] != Fp:
            ref = weakref.ref(x, lambda _r, k=key, d=self._by_id: d.pop(k, None) if d.get(k, (None,))[0] is _r else None)
            hit = (ref, x._version, torch.nn.functional.pad(x, (0, Fp - x.shape[1])))
            self._by_id[key] = hit
        return hit[2]


_xpad = _PaddedFeatures()


def padded_features(x: torch.Tensor) -> torch.Tensor:
    """The tensor project_fwd / project_bwd actually read for x (x itself when its rows are 16-byte aligned; a
    SparseFeatures passes through untouched: the sparse kernels read its arrays)."""
    if isinstance(x, SparseFeatures):
        return x
    F = x.shape[1]
    Fp = (F + 3) // 4 * 4
    return x if Fp == F else _xpad.get(x, Fp)


class _XPlanes:
    """Persistent bf16 planes of a feature matrix and of its transpose (dl_project_xplanes_build), one entry per feature
    TENSOR (object identity + version counter, like _PaddedFeatures): model.py:106 evaluates the MLPs on the same x every
    epoch, and the projection kernels otherwise split x (forward) and x^T (backward) into their three bf16 planes on every
    call.  An entry is made the SECOND time a tensor is seen (a one-off call splits inside its own workspace, as before),
    only for graphs the kernels process as one node block, and dies with its tensor.
    CONTRACT: the planes follow the tensor's identity and VERSION COUNTER — a write that bypasses the counter (``x.data``,
    a raw-pointer kernel) leaves stale planes in use; write through torch (any in-place op bumps the version) or set
    DL_X_PLANES=0.  Up to MAX_BYTES (1 GiB, about 3x the size of x) of device memory per cached tensor."""
    MAX_ROWS = 2 << 17              # fwd_block_rows: larger graphs are processed in node blocks that re-split themselves
    MAX_BYTES = 1 << 30

    def __init__(self):
        self._by_id: dict = {}

    def get(self, x: torch.Tensor, force: bool = False):
        if os.environ.get("DL_X_PLANES", "1") == "0" or x.shape[0] > self.MAX_ROWS or not x.is_cuda:
            return None
        # no version counter to watch (inference-mode tensors raise on ._version), or a view made for this call (a row chunk of
        # the sharded path: a new tensor object every epoch, it would never be seen twice): split per call, as before the cache
        if x.is_inference() or x._base is not None:
            return None
        key = id(x)
        hit = self._by_id.get(key)
        if hit is not None and (hit[0]() is not x or hit[1] != x._version):
            hit = None
        if hit is None:
            ref = weakref.ref(x, lambda _r, k=key, d=self._by_id: d.pop(k, None) if d.get(k, (None,))[0] is _r else None)
            hit = (ref, x._version, None)
            self._by_id[key] = hit
            if not force:
                return None                                         # first sight: remember the tensor, build next time
        if hit[2] is None:
            lib = _lib.load()
            N, F = x.shape
            nbytes = int(lib.dl_project_xplanes_bytes(N, F))
            if nbytes == 0 or nbytes > self.MAX_BYTES:
                return None
            buf = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            _lib.check(lib.dl_project_xplanes_build(x.data_ptr(), N, F, buf.data_ptr(), nbytes, _stream()), "dl_project_xplanes_build")
            hit = (hit[0], hit[1], buf)
            self._by_id[key] = hit
        return hit[2]


_xplanes = _XPlanes()


def xplanes_for(x: torch.Tensor, force: bool = False):
    """The persistent planes of the tensor the projection kernels read for x (its zero-padded copy when F % 4 != 0), or
    None (first sight of the tensor, a blocked graph, DL_X_PLANES=0, a SparseFeatures: the sparse kernels use no planes of
    x).  force=True builds them now (before a graph capture)."""
    if isinstance(x, SparseFeatures):
        return None
    return _xplanes.get(padded_features(_f32c(x)), force)


def _pad_features(x, W1):
    """Rows of F floats with F % 4 != 0 have no common 16-byte alignment, which would force the kernels onto
    scalar loads.  Zero-pad the feature axis of x (once per tensor: the features are constant data) and of W1
    (per call: one small copy) to a multiple of 4; zero columns add nothing to any product."""
    F = x.shape[1]
    Fp = (F + 3) // 4 * 4
    if Fp == F:
        return x, W1
    return padded_features(x), torch.nn.functional.pad(W1, (0, Fp - F))


def keep_hidden(N: int, F: int, K: int, nhid: int) -> bool:
    """Should the forward keep the hidden layer for the backward?  Recomputing it costs 2*F FLOP per hidden unit
    against 8 bytes of traffic: measured faster at every width tried (F = 128: fwd+bwd 0.35 -> 0.30 ms, F = 2089:
    2.9 -> 2.0 ms, tools/project_keep_times.py; snap-patents-sized, 45 GiB of hidden layer: epoch 445 -> 393 ms) — while
    the [K,nhid,N] buffer stays within a quarter of the device's memory, at most 64 GiB (of 288 GB on an MI355X); past
    that the recompute is what keeps large graphs in memory."""
    mode = os.environ.get("DL_KEEP_HIDDEN", "auto")
    if mode in ("0", "1"):
        return mode == "1"
    return N * K * nhid * 4 <= _keep_hidden_limit()


_KEEP_LIMIT = None


def _keep_hidden_limit() -> int:
    global _KEEP_LIMIT
    if _KEEP_LIMIT is None:
        total = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory if torch.cuda.is_available() else 0
        _KEEP_LIMIT = min(64 << 30, total // 4)
    return _KEEP_LIMIT


# ---------------------------------------------------------------------- the tile width, once
_TILE_WIDTHS = (32, 64, 128)          # factor widths d the matrix-core projection kernels are instantiated for


def project_tile_width(d: int) -> int | None:
    """The kernels' own widths serve themselves; any other d <= 128 runs at the next width with zero-padded output
    weights (zero rows of the LAST layer: they add nothing to any product and cost (dp - d) / dp of the smaller GEMM);
    None beyond 128 (the library GEMMs then)."""
    for w in _TILE_WIDTHS:
        if d <= w:
            return w
    return None


def project_supported(d: int) -> bool:
    """Do the matrix-core projection kernels serve factor width d?  (Natively 32 / 64 / 128; every other d <= 128 at the
    next of those widths through zero-padded output weights, project_tile_width.)"""
    return project_tile_width(int(d)) is not None


def _pad_out_rows(W, b, dp):
    """Zero-pad dim 1 of W [K,d,*] and b [K,d] (None: the backward has no use for it) to dp."""
    d = W.shape[1]
    return torch.nn.functional.pad(W, (0, 0, 0, dp - d)), None if b is None else torch.nn.functional.pad(b, (0, dp - d))


def _tile(W1, W2):
    """(d, dp): the width of the last layer's output and the tile width it runs at; the refusal beyond the widest tile."""
    d = W1.shape[1] if W2 is None else W2.shape[1]
    dp = project_tile_width(d)
    if dp is None:
        raise _lib.DisenlinkHipError(f"projection kernels serve d <= {_TILE_WIDTHS[-1]}, got {d}")
    return d, dp


def _at_tile(dp, W1, b1, W2, b2=None):
    """(W1, b1, W2, b2) as the kernels take them: fp32-contiguous, the last layer's output rows zero-padded to dp.  The
    padded columns of Z come out as zeros' products and carry zero gradient in; _trim_grads cuts the results back."""
    if W2 is None:
        return (W1, b1, None, None) if W1.shape[1] == dp else (*_pad_out_rows(W1, b1, dp), None, None)
    W2, b2 = _f32c(W2), None if b2 is None else _f32c(b2)
    return (W1, b1, W2, b2) if W2.shape[1] == dp else (W1, b1, *_pad_out_rows(W2, b2, dp))


def _trim_grads(grads, d, dp):
    """The gradients of the last layer at its true width d (contiguous copies: at a padded width they are no longer
    back to back)."""
    if dp == d:
        return grads
    dW1, db1, dW2, db2 = grads
    if dW2 is None:
        return dW1[:, :d].contiguous(), db1[:, :d].contiguous(), None, None
    return dW1, db1, dW2[:, :d].contiguous(), db2[:, :d].contiguous()


def _carve(shapes, device, one_allocation: bool):
    """fp32 outputs of `shapes`: views of ONE flat buffer, back to back, when asked for and every size is a multiple of 4
    floats (every piece 16-byte aligned: the sharded training step all-reduces them as one flat tensor without packing,
    dist.allreduce_gradients), else separate tensors."""
    sizes = [int(torch.Size(sh).numel()) for sh in shapes]
    if not (one_allocation and all(n % 4 == 0 for n in sizes)):
        return [_empty(sh, torch.float32, device) for sh in shapes]
    flat = _empty((sum(sizes),), torch.float32, device)
    parts, off = [], 0
    for sh, n in zip(shapes, sizes):
        parts.append(flat[off:off + n].view(sh))
        off += n
    return parts


# ---------------------------------------------------------------------- raw wrappers
def project_fwd(x, W1, b1, W2=None, b2=None, pad: bool = True, keep_hid: bool = False):
    """Z [N,K,d] = K MLPs of x on the matrix cores.  Two-layer: W1 [K,nhid,F], b1 [K,nhid], W2 [K,d,nhid],
    b2 [K,d]; single layer: W1 [K,d,F], b1 [K,d], W2 = b2 = None.  model.py:13-15 / 24-27 / 106.
    keep_hid=True (two-layer): returns (Z, hid) with hid the kept hidden layer for project_bwd.
    Any d <= 128: widths other than 32 / 64 / 128 run at the next of those (project_tile_width)."""
    lib = _lib.load()
    x, W1, b1 = _f32c(x), _f32c(W1), _f32c(b1)
    _need_cuda(x, W1, b1)
    if W1.shape[2] != x.shape[1]:
        raise ValueError("W1 does not match the feature count of x")
    d_true, d = _tile(W1, W2)
    two = W2 is not None
    W1, b1, W2, b2 = _at_tile(d, W1, b1, W2, b2)
    if pad:
        x, W1 = _pad_features(x, W1)
    N, F = x.shape
    K = W1.shape[0]
    nhid = W1.shape[1] if two else 1
    if two and (W2.shape != (K, d, nhid) or b2.shape != (K, d) or b1.shape != (K, nhid)):
        raise ValueError("inconsistent projection weight shapes")
    if W1.shape[2] != F:
        raise ValueError("W1 does not match the feature count of x")
    Z = _empty((N, K, d), torch.float32, x.device)
    hid = None
    if keep_hid and two:
        hid = _empty(int(lib.dl_project_hidden_floats(N, K, nhid)), torch.float32, x.device)
    ws = _ws.get(int(lib.dl_project_fwd_workspace_bytes(N, F, K, nhid, d, int(two))), x.device)
    xp = _xplanes.get(x) if two else None                      # x's planes, split once for the run (second call on)
    _lib.check(lib.dl_project_fwd_xp(x.data_ptr(), N, F, K, nhid, d, W1.data_ptr(), b1.data_ptr(),
                                     W2.data_ptr() if two else None, b2.data_ptr() if two else None,
                                     Z.data_ptr(), hid.data_ptr() if hid is not None else None, ws.data_ptr(), ws.numel(),
                                     xp.data_ptr() if xp is not None else None, _stream()), "dl_project_fwd")
    if d != d_true:                                            # hand back the first d columns
        Z = Z[:, :, :d_true].contiguous()
    # (a single layer at a padded width hands back Z alone, asked for the hidden layer it does not have or not)
    return (Z, hid) if keep_hid and (two or d == d_true) else Z


def project_bwd(x, W1, b1, W2, dZ, pad: bool = True, hid=None, one_allocation: bool = True):
    """Weight / bias gradients of the projection from dZ [N,K,d]: (dW1, db1, dW2, db2), shaped like the weights
    (dW2 = db2 = None for the single layer).  autograd of model.py:13-15 / 24-27.  hid: the hidden layer kept
    by project_fwd(keep_hid=True), else it is recomputed.  one_allocation: the gradients are views of ONE flat buffer (the
    sharded step all-reduces it as it is); False gives four separate tensors (registered operators may not return
    outputs that share storage)."""
    lib = _lib.load()
    x, W1, b1, dZ = _f32c(x), _f32c(W1), _f32c(b1), _f32c(dZ)
    _need_cuda(x, W1, b1, dZ)
    if W1.shape[2] != x.shape[1]:
        raise ValueError("inconsistent projection shapes")
    d_true, d = _tile(W1, W2)
    if d != d_true and dZ.shape[2] != d_true:
        raise ValueError("inconsistent projection shapes")
    two = W2 is not None
    W1, b1, W2, _b2 = _at_tile(d, W1, b1, W2)
    F_true = x.shape[1]
    if pad:
        x, W1 = _pad_features(x, W1)
    N, F = x.shape
    K = W1.shape[0]
    nhid = W1.shape[1] if two else 1
    if dZ.shape != (N, K, d_true) or W1.shape[2] != F:
        raise ValueError("inconsistent projection shapes")
    if d != d_true:                                            # zero-padded output columns carry zero gradient in
        dZ = torch.nn.functional.pad(dZ, (0, d - d_true))
    # with a zero-padded feature axis the kernels write dW1 at the padded width into a buffer of its own and the columns
    # that exist are copied into the first piece — the one copy the trim costs anyway — so the four gradients stay
    # adjacent at EVERY feature width: snap-patents' F = 269 gave four collectives in round 4
    trimmed = F != F_true
    shapes = [tuple(W1.shape[:2]) + (F_true,), tuple(b1.shape)] + ([tuple(W2.shape), (K, d)] if two else [])
    dW1_out, db1, dW2, db2 = _carve(shapes, x.device, one_allocation) + ([] if two else [None, None])
    dW1 = _empty(tuple(W1.shape), torch.float32, x.device) if trimmed else dW1_out
    ws = _ws.get(int(lib.dl_project_bwd_workspace_bytes(N, F, K, nhid, d, int(two))), x.device)
    xp = _xplanes.get(x) if two else None
    _lib.check(lib.dl_project_bwd_xp(x.data_ptr(), N, F, K, nhid, d, W1.data_ptr(), b1.data_ptr(),
                                     W2.data_ptr() if two else None, dZ.data_ptr(),
                                     hid.data_ptr() if (two and hid is not None) else None, dW1.data_ptr(), db1.data_ptr(),
                                     dW2.data_ptr() if two else None, db2.data_ptr() if two else None,
                                     ws.data_ptr(), ws.numel(), xp.data_ptr() if xp is not None else None, _stream()),
               "dl_project_bwd")
    if trimmed:
        dW1_out.copy_(dW1[..., :F_true])
    return _trim_grads((dW1_out, db1, dW2, db2), d_true, d)


def _sparse_shapes(sf, W1, b1, W2, b2=None):
    """The checks both sparse wrappers make -> (the weights at the tile width, N, K, nhid, d_true, d, two)."""
    if not isinstance(sf, SparseFeatures) or not sf.is_cuda:
        raise _lib.DisenlinkHipError("the sparse projection kernels take a SparseFeatures on the GPU")
    W1, b1 = _f32c(W1), _f32c(b1)
    _need_cuda(W1, b1)
    N, F = sf.shape
    K = W1.shape[0]
    if W1.shape[2] != F:
        raise ValueError("W1 does not match the feature count of x")
    d_true, d = _tile(W1, W2)
    two = W2 is not None
    nhid = W1.shape[1] if two else 1
    if two:
        W2 = _f32c(W2)
        if W2.shape != (K, d_true, nhid) or b1.shape != (K, nhid) or (b2 is not None and b2.shape != (K, d_true)):
            raise ValueError("inconsistent projection weight shapes")
    return _at_tile(d, W1, b1, W2, b2), N, K, nhid, d_true, d, two


def project_sparse_fwd(sf, W1, b1, W2=None, b2=None):
    """project_fwd for a SparseFeatures input (dl_project_sparse_fwd): layer 1 as a gather over the CSR of x.  Two-layer:
    returns (Z, hid) — the hidden layer is always kept, the backward has no recompute form; single layer: Z.
    Any d <= 128, as project_fwd."""
    lib = _lib.load()
    (W1, b1, W2, b2), N, K, nhid, d_true, d, two = _sparse_shapes(sf, W1, b1, W2, b2)
    Z = _empty((N, K, d), torch.float32, sf.device)
    hid = _empty(int(lib.dl_project_hidden_floats(N, K, nhid)), torch.float32, sf.device) if two else None
    ref = sf.c_struct()
    ws = _ws.get(int(lib.dl_project_sparse_fwd_workspace_bytes(ref, K, nhid, d, int(two))), sf.device)
    _lib.check(lib.dl_project_sparse_fwd(ref, K, nhid, d, W1.data_ptr(), b1.data_ptr(), W2.data_ptr() if two else None,
                                         b2.data_ptr() if two else None, Z.data_ptr(), hid.data_ptr() if two else None,
                                         ws.data_ptr(), ws.numel(), _stream()), "dl_project_sparse_fwd")
    if d != d_true:                                            # hand back the first d columns
        Z = Z[:, :, :d_true].contiguous()
    return (Z, hid) if two else Z


def project_sparse_bwd(sf, W1, b1, W2, dZ, hid=None):
    """project_bwd for a SparseFeatures input (dl_project_sparse_bwd): (dW1, db1, dW2, db2) from dZ [N,K,d] and the hidden
    layer project_sparse_fwd kept; dW1 as a gather over the CSC view of x.  The gradients are views of one flat buffer where
    their sizes allow, like project_bwd's."""
    lib = _lib.load()
    (W1, b1, W2, _b2), N, K, nhid, d_true, d, two = _sparse_shapes(sf, W1, b1, W2)
    dZ = _f32c(dZ)
    _need_cuda(dZ)
    if dZ.shape != (N, K, d_true):
        raise ValueError("inconsistent projection shapes")
    if d != d_true:                                            # zero-padded output columns carry zero gradient in
        dZ = torch.nn.functional.pad(dZ, (0, d - d_true))
    if two and hid is None:
        raise _lib.DisenlinkHipError("the sparse backward has no recompute form: pass the hidden layer project_sparse_fwd kept")
    shapes = [tuple(W1.shape), tuple(b1.shape)] + ([tuple(W2.shape), (K, d)] if two else [])
    dW1, db1, dW2, db2 = _carve(shapes, sf.device, True) + ([] if two else [None, None])
    ref = sf.c_struct()
    ws = _ws.get(int(lib.dl_project_sparse_bwd_workspace_bytes(ref, K, nhid, d, int(two))), sf.device)
    _lib.check(lib.dl_project_sparse_bwd(ref, K, nhid, d, W1.data_ptr(), b1.data_ptr(), W2.data_ptr() if two else None,
                                         dZ.data_ptr(), hid.data_ptr() if two else None, dW1.data_ptr(), db1.data_ptr(),
                                         dW2.data_ptr() if two else None, db2.data_ptr() if two else None,
                                         ws.data_ptr(), ws.numel(), _stream()), "dl_project_sparse_bwd")
    return _trim_grads((dW1, db1, dW2, db2), d_true, d)


# ---------------------------------------------------------------------- autograd
class Project(torch.autograd.Function):
    """Z = MLP_k(x) for all k: ``Project.apply(x, bufs, K, *params)``.  x: a dense fp32 tensor (the fused MFMA kernels of
    dl_project_fwd / dl_project_bwd) or a SparseFeatures (features.py: dl_project_sparse_fwd / _bwd); it is data and gets no
    gradient.  Weights, in one of two forms:
    * bufs = the module's shared [K, ...] buffers (W1, b1, W2, b2; Disentangle._restack), params = the 4K (single layer:
      2K) per-factor Parameters that view them.  The Parameters are the autograd inputs, the kernel reads their common
      storage — no stacking copy — and each parameter's gradient is a slice of the stacked gradient;
    * bufs = None, params = the four stacked tensors themselves (W2 = b2 = None for the single layer).
    The hidden layer is kept for the backward when a gradient is wanted and keep_hidden says so (else dl_project_bwd
    recomputes it on the matrix cores); always on sparse features, whose backward has no recompute form."""

    @staticmethod
    def forward(ctx, x, bufs, K, *params):
        W1, b1, W2, b2 = params if bufs is None else bufs
        ctx.sparse, ctx.stacked, ctx.two_layer = isinstance(x, SparseFeatures), bufs is not None, W2 is not None
        if ctx.sparse:
            ctx.x, ctx.weights = x, (W1, b1, W2)
            keep = ctx.two_layer
            out = project_sparse_fwd(x, W1, b1, W2, b2)
        else:
            if ctx.stacked:                                     # buffers are no autograd inputs: held as they are
                ctx.weights = (W1, b1, W2)
                ctx.save_for_backward(x)
            else:
                ctx.save_for_backward(x, W1, b1, W2 if ctx.two_layer else x.new_empty(0))
            keep = ctx.two_layer and any(ctx.needs_input_grad) and keep_hidden(x.shape[0], x.shape[1], K, W1.shape[1])
            out = project_fwd(x, W1, b1, W2, b2, keep_hid=keep)
        Z, ctx.hid = out if keep else (out, None)
        return Z

    @staticmethod
    def backward(ctx, dZ):
        if ctx.sparse:
            x, (W1, b1, W2) = ctx.x, ctx.weights
        elif ctx.stacked:
            (x,), (W1, b1, W2) = ctx.saved_tensors, ctx.weights
        else:
            x, W1, b1, W2 = ctx.saved_tensors
            W2 = W2 if ctx.two_layer else None
        grads = (project_sparse_bwd if ctx.sparse else project_bwd)(x, W1, b1, W2, dZ.contiguous(), hid=ctx.hid)
        ctx.hid = None
        if ctx.stacked:                                         # every parameter's gradient: its slice of the stacked one
            grads = [g_k for g in grads if g is not None for g_k in g.unbind(0)]
        return (None, None, None, *grads)
