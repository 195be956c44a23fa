"""Drop-in ``Disentangle`` module: same constructor, ``forward(x, adj)`` signature and
``state_dict`` keys as the reference's ``model.Disentangle`` (model.py:91-114), with the
routing / aggregation / scoring path running on libdisenlink_hip.so.

    from disenlink_amd.model import Disentangle          # instead of: from model import Disentangle
    model = Disentangle(nfeat, nhidden, nembed, nfactor=K, beta=b, t=t).to(device)
    emb, a_pred = model(x, adj_sym)                       # main_disentangled.py:194

For graphs where ``[N,N]`` cannot exist, ``forward_pairs(x, graph, pairs)`` scores a pair
list instead; the reference has no counterpart for it.  Neither has ranking:
``topk_links`` (the k most likely links of query nodes) and ``link_ranks`` (filtered ranks of target pairs among all
nodes, for MRR / Hits@K) score every candidate on the matrix cores without an ``[N,N]`` tensor, and
``top_missing_links`` mines the m most likely links of the whole graph that are not known yet the same way.
"""
from __future__ import annotations

import math
import os
import weakref
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .features import SparseFeatures
from .graph import Graph, PairList
from .recon import _own_filter


TopLinks = namedtuple("TopLinks", ["index", "logit", "prob"])
MinedLinks = namedtuple("MinedLinks", ["src", "dst", "logit", "prob"])
PairRanks = namedtuple("PairRanks", ["greater", "ties", "logit", "n_others"])


class PredictedLinks(namedtuple("PredictedLinks", ["rowptr", "col", "logit", "prob"])):
    """The predicted graph of ``Disentangle.predicted_links``: a symmetric CSR over all nodes (rowptr int64 [N+1], col int32
    [nnz], logit / prob f32 [nnz]); every link {u, v} is stored as (u, v) and as (v, u), columns ascending within a row."""
    __slots__ = ()

    @property
    def n_nodes(self) -> int:
        return int(self.rowptr.numel()) - 1

    @property
    def degree(self) -> torch.Tensor:
        """int64 [N]: the predicted degree of every node."""
        return self.rowptr[1:] - self.rowptr[:-1]

    def _rows(self) -> torch.Tensor:
        return torch.repeat_interleave(torch.arange(self.n_nodes, device=self.rowptr.device), self.degree)

    def pairs(self):
        """(src int64 [P], dst int64 [P], logit f32 [P], prob f32 [P]): every link once, src < dst, in ascending
        src * N + dst order (the order of the CSR's upper triangle)."""
        rows, cols = self._rows(), self.col.long()
        keep = rows < cols
        return rows[keep], cols[keep], self.logit[keep], self.prob[keep]

    def to_graph(self) -> Graph:
        """The links as a graph.Graph, as ``Disentangle.forward`` takes it."""
        return Graph.from_edge_rows(self._rows(), self.col.long(), self.n_nodes, symmetrise=False)


class Factor(nn.Module):
    """One Linear(F -> d); used when nhid == 1 (model.py:7-15, :94-95)."""

    def __init__(self, nfeat, nhid):
        super().__init__()
        self.mlp = nn.Linear(nfeat, nhid)

    def forward(self, x):
        return self.mlp(x)


class Factor2(nn.Module):
    """Linear(F -> nmid) -> ReLU -> Linear(nmid -> d) (model.py:16-27, :96-97)."""

    def __init__(self, nfeat, nmid, nhid):
        super().__init__()
        self.mlp1 = nn.Linear(nfeat, nmid)
        self.mlp2 = nn.Linear(nmid, nhid)

    def forward(self, x):
        return self.mlp2(F.relu(self.mlp1(x)))


class Disentangle(nn.Module):
    def __init__(self, nfeat, nhid, nebed, nfactor, beta, t=1, table_dtype=torch.float32, projection="auto",
                 use_torch_ops=False, link_pred_backward="plan"):
        """Extensions (the reference has neither):
        ``table_dtype``: storage type of the gathered Z / H tables in ``forward_pairs`` — torch.float32
        (reference precision) or torch.bfloat16 (half the gather bytes, fp32 arithmetic and gradients).
        ``projection``: "mfma" = the fused matrix-core kernels of libdisenlink_hip.so (forward and backward; fp32
        results — layer 1 and the dW1 contraction run as six exact bf16 products per term; the hidden
        layer is written once, transposed, for the backward while it fits a quarter of the device memory (at most
        64 GiB) and recomputed beyond that),
        "library" = library GEMMs (rocBLAS through torch), "auto" = the kernels wherever they support the factor width
        (any d <= 128; widths other than 32 / 64 / 128 run at the next of those): measured equal or faster than the library path at every feature width (squirrel epoch
        1.64 vs 1.75 ms at F=128, 1.93 vs 2.06 at 512, 2.17 vs 2.36 at 1024, 2.74 vs 3.20 at 2089; real Cora
        (F=1433) 1.32 vs 1.60; tools/epoch_time.py), and they never materialise the [N,K,nhid] activations.
        ``use_torch_ops``: ``forward_pairs`` goes through the REGISTERED operators ``torch.ops.disenlink.*``
        (disenlink_amd/torch_ops.py: schema + fake + autograd via torch.library over the same C ABI) instead of the
        ctypes-calling autograd.Functions — same kernels and bits; what it buys is dispatcher visibility:
        ``torch.compile(model.forward_pairs)`` traces the whole step without graph breaks.
        ``link_pred_backward``: how ``forward(x, adj)``'s dense link_pred is differentiated.  "plan" = on the pair plan of
        the caller's loss masks (declared with set_loss_pairs / assume_static_loss_masks, or learnt from the indexing of
        link_pred): the cheapest backward for the reference's masked loss.  "dense" = the gradient of ANY loss on
        link_pred — a whole-matrix reconstruction loss, ``link_pred.mean()``, a regulariser — by the dense matrix-core
        backward (ops.score_allpairs_bwd_dense): link_pred is a plain tensor, nothing is declared or learnt, no host
        read; it costs the same whatever the loss touches (INTEGRATION.md §1 on which to choose)."""
        super().__init__()
        if link_pred_backward not in ("plan", "dense"):
            raise ValueError("link_pred_backward must be 'plan' or 'dense'")
        self.link_pred_backward = link_pred_backward
        self.use_torch_ops = bool(use_torch_ops)
        if projection not in ("auto", "mfma", "library"):
            raise ValueError("projection must be 'auto', 'mfma' or 'library'")
        self.table_dtype = table_dtype
        self.projection = projection
        # creation order == the reference's (model.py:93-99), so a seeded init draws the same stream
        if nhid == 1:
            factors = [Factor(nfeat, nebed) for _ in range(nfactor)]
        else:
            factors = [Factor2(nfeat, nhid, nebed) for _ in range(nfactor)]
        for i, f in enumerate(factors):
            self.add_module("factor_{}".format(i), f)
        self.single_layer = nhid == 1
        self.temperature = t
        self.nfactor = nfactor
        self.nebed = nebed
        self.beta = beta
        self._graph_cache = None
        self._dense_plan = ops.DensePairPlanCache()      # backward of the dense link_pred: this module's own cache
        self._stacked = {}
        self._restack()

    # ------------------------------------------------------------------ stacked parameter storage
    # The K factor modules keep their own Parameters (and state_dict keys), but every group of K same-shaped
    # parameters shares ONE contiguous [K, ...] buffer: parameter i's .data is the view buf[i].  The projection
    # kernel reads the buffers directly — no torch.stack copies per call — and Adam / load_state_dict, which
    # update parameters in place, keep the buffers current.
    def _param_groups(self):
        names = ("mlp",) if self.single_layer else ("mlp1", "mlp2")
        for name in names:
            for attr in ("weight", "bias"):
                yield (name, attr), [getattr(getattr(f, name), attr) for f in self.factors]

    def _param_slots(self):
        """(key, [(owning module's _parameters dict, attribute name)]) per group: where the LIVE Parameter objects are
        registered — the fast path checks identity against these slots, so a replaced Parameter object
        (load_state_dict(assign=True), setattr, weight tying) is seen."""
        names = ("mlp",) if self.single_layer else ("mlp1", "mlp2")
        for name in names:
            for attr in ("weight", "bias"):
                yield (name, attr), [(getattr(f, name)._parameters, attr) for f in self.factors]

    def _restack(self):
        # (owner's _parameters dict, attribute, parameter, expected data pointer, expected shape) of every view
        self._stacked_check = []
        for key, slots in self._param_slots():
            ps = [reg[attr] for reg, attr in slots]
            buf = torch.stack([p.data for p in ps]).contiguous()
            for i, (p, (reg, attr)) in enumerate(zip(ps, slots)):
                p.data = buf[i]
                self._stacked_check.append((reg, attr, p, p.data_ptr(), tuple(p.shape)))
            self._stacked[key] = buf

    def _apply(self, fn, *args, **kwargs):                     # .to(device) / .float() replace .data: re-stack
        out = super()._apply(fn, *args, **kwargs)
        self._restack()
        return out

    def snapshot_state(self):
        """deepcopy(state_dict()) (main_disentangled.py:209) with one clone per shared buffer instead of one per
        parameter; the result loads back with load_state_dict like any state_dict."""
        if self._stacked_params() is None:
            from copy import deepcopy
            return deepcopy(self.state_dict())
        clones = {key: buf.clone() for key, buf in self._stacked.items()}
        out = {}
        for i in range(self.nfactor):
            for (name, attr), buf in clones.items():
                out[f"factor_{i}.{name}.{attr}"] = buf[i]
        return {k: out[k] for k in self.state_dict().keys()}

    def _stacked_params(self):
        """The flat parameter list if every parameter still aliases its place in the shared buffers, else None.  Runs
        every forward: compares each parameter's data pointer with the one recorded when the buffers were built (indexing
        the buffers here — 4K tiny view tensors per call — cost the eager loop ~50 us of host time per epoch)."""
        chk = self.__dict__.get("_stacked_check")
        if chk and all(reg.get(attr) is p and p.data_ptr() == ptr and tuple(p.shape) == shape
                       for reg, attr, p, ptr, shape in chk):
            return [c[2] for c in chk]
        # pointers moved (a deep copy, an unpickled module) or a Parameter object was replaced: look at the LIVE
        # parameters and the buffers themselves, and record anew
        fresh = []
        for key, slots in self._param_slots():
            buf = self._stacked.get(key)
            ps = [reg.get(attr) for reg, attr in slots]
            if buf is None or any(p is None or p.data_ptr() != buf[i].data_ptr() or p.shape != buf[i].shape
                                  for i, p in enumerate(ps)):
                return None
            fresh += [(reg, attr, p, p.data_ptr(), tuple(p.shape)) for p, (reg, attr) in zip(ps, slots)]
        self._stacked_check = fresh
        return [c[2] for c in fresh]

    def restack(self):
        """Re-establish the shared [K, ...] buffers from the LIVE parameters (after load_state_dict(assign=True) or any
        other replacement of Parameter objects, which leaves project() on the slower stacking path until this is
        called).  Optimisers built over the old Parameter objects must be rebuilt, as torch requires after assign."""
        self._restack()
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """torch's load_state_dict; with ``assign=True`` — which REPLACES the Parameter objects instead of copying into
        them — the shared buffers are rebuilt from the new parameters afterwards, so the kernels, snapshot_state() and
        the live state_dict keep reading the same storage."""
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        if assign:
            self._restack()
        return out

    def train(self, mode: bool = True):
        """No layer of this model depends on the mode (main_disentangled.py:193,201 call train()/eval() every
        epoch as no-ops): set the flag without walking the K factor modules."""
        self.training = mode
        return self

    @property
    def factors(self):
        return [getattr(self, "factor_{}".format(i)) for i in range(self.nfactor)]

    # ------------------------------------------------------------------ projection (model.py:106)
    def project(self, x: torch.Tensor) -> torch.Tensor:
        """Z [N,K,d] = K independent MLPs of x.  On the GPU: the fused MFMA kernels of libdisenlink_hip.so (d <= 128).
        The library-GEMM form (one wide GEMM + one K-batched GEMM: the reference's own ops) runs ONLY when asked for —
        ``Disentangle(projection="library")``, kept for timing comparisons — or for CPU tensors, which no product path
        serves (the CPU tests of the host logic and of the sharding choreography use it with the oracle as the backend);
        a CUDA tensor whose shape the kernels do not serve raises instead of falling back."""
        K, d = self.nfactor, self.nebed
        sparse = isinstance(x, SparseFeatures)
        if sparse:
            # features.py: scale * X + shift with X a CSR.  On the GPU layer 1 and dW1 are gathers (dl_project_sparse_fwd / _bwd)
            # and there is never a dense product; a CPU object takes the GEMM branch on to_dense() (host tests only)
            if not x.is_cuda:
                return self.project(x.to_dense())
            if not ops.project_supported(d):
                raise ops._lib.DisenlinkHipError(f"the sparse projection kernels serve factor widths d <= 128 (got d = {d})")
        elif not x.is_cuda or self.projection == "library":
            return self._project_gemm(x)
        elif not (x.dtype == torch.float32 and ops.project_supported(d)):
            raise ops._lib.DisenlinkHipError(
                f"the projection kernels serve fp32 features and factor widths d <= 128 (got {x.dtype}, d = {d}); "
                "there is no eager fallback on the GPU — construct the module with projection=\"library\" to use the library GEMMs")
        bufs, params = self._project_weights()
        if bufs is not None and not sparse:
            from . import native
            if native.project_ok(x, d, self.single_layer):       # the same kernels from a C++ autograd node (no Python in the backward)
                return native.project_stacked(x, bufs, params)
        return ops.Project.apply(x, bufs, K, *params)

    def _stacked_weights(self):
        """(W1, b1, W2, b2) stacked from the K factors' LIVE Parameters, one copy each (W2 = b2 = None for the single layer)."""
        fs = self.factors
        if self.single_layer:
            return torch.stack([f.mlp.weight for f in fs]), torch.stack([f.mlp.bias for f in fs]), None, None
        return (torch.stack([f.mlp1.weight for f in fs]), torch.stack([f.mlp1.bias for f in fs]),
                torch.stack([f.mlp2.weight for f in fs]), torch.stack([f.mlp2.bias for f in fs]))

    def _project_weights(self):
        """The weights of one projection call, as ops.Project takes them: (the shared [K, ...] buffers, the flat list of
        per-factor Parameters) while every Parameter still aliases its place in the buffers — zero-copy: the kernel reads
        the buffers — else (None, the four stacked tensors): the caller re-pointed a Parameter, one stacking copy per call."""
        flat = self._stacked_params()
        if flat is None:
            return None, self._stacked_weights()
        st = self._stacked
        if self.single_layer:
            return (st[("mlp", "weight")], st[("mlp", "bias")], None, None), flat
        return (st[("mlp1", "weight")], st[("mlp1", "bias")], st[("mlp2", "weight")], st[("mlp2", "bias")]), flat

    def _project_gemm(self, x):
        """project() as library GEMMs (one wide GEMM + one K-batched GEMM), differentiated by autograd."""
        fs = self.factors
        K, d = self.nfactor, self.nebed
        if self.single_layer:
            W = torch.cat([f.mlp.weight for f in fs], dim=0)             # [K*d, F]
            b = torch.cat([f.mlp.bias for f in fs], dim=0)
            return F.linear(x, W, b).view(-1, K, d)
        W1 = torch.cat([f.mlp1.weight for f in fs], dim=0)               # [K*nhid, F]
        b1 = torch.cat([f.mlp1.bias for f in fs], dim=0)
        hid = F.relu(F.linear(x, W1, b1)).view(x.shape[0], K, -1)        # [N,K,nhid]
        W2 = torch.stack([f.mlp2.weight for f in fs], dim=0)             # [K,d,nhid]
        b2 = torch.stack([f.mlp2.bias for f in fs], dim=0)               # [K,d]
        Z = torch.einsum("nkh,kdh->nkd", hid, W2) + b2
        return Z.contiguous()

    # ------------------------------------------------------------------ graph cache
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_graph_cache"] = None              # holds a weak reference: not copyable / picklable, and only a cache
        state["_dense_plan"] = ops.DensePairPlanCache()     # a copy starts without a plan (declare the masks again)
        return state

    def set_loss_pairs(self, *supports, n_nodes: int | None = None):
        """Declare where the caller takes its loss on the dense ``link_pred`` of ``forward(x, adj)``: dense [N,N] masks
        (the reference's ``pos_train_adj``, ``neg_train_adj``; entries != 0 count, main_disentangled.py:167-190) and / or
        ``(rows, cols)`` index tuples (then give ``n_nodes`` unless a mask comes along).  Their union becomes the pair
        plan of the dense backward (dl_score_allpairs_bwd), built once, on the module's device.  Without it the plan is
        learnt from the gradients (it grows until it covers the masks; ops.DensePairPlanCache).
        ``set_loss_pairs()`` with no argument forgets a declared set."""
        self._no_declaration_in_dense_mode("set_loss_pairs")
        if not supports:
            self._dense_plan.clear()
            return self
        for sup in supports:
            if torch.is_tensor(sup) and sup.dim() == 2 and n_nodes is None:
                n_nodes = sup.shape[0]
        if n_nodes is None:
            raise ValueError("index pairs alone do not say how many nodes there are: pass n_nodes=")
        self._dense_plan.set_pairs(int(n_nodes), next(self.parameters()).device, *supports)
        return self

    def assume_static_loss_masks(self, *masks, static: bool = True):
        """``assume_static_loss_masks(pos_train_adj, neg_train_adj)``: the caller promises that every step's loss is
        taken inside these masks (the reference builds them once per run, main_disentangled.py:167-190).  The dense
        backward then runs on their support without any host read: the subset check "no gradient outside the plan"
        stays on the device and turns the gradients into NaN — not into something silently wrong — should the promise
        be broken.  The masks are REQUIRED (here or through set_loss_pairs before): the support of a loss cannot be
        inferred from a gradient, whose non-zero set moves with fp32 sigmoid saturation.
        ``assume_static_loss_masks(static=False)`` returns to the validated mode (one 16-byte read per backward)."""
        self._no_declaration_in_dense_mode("assume_static_loss_masks")
        if len(masks) == 1 and isinstance(masks[0], bool):        # round-2 spelling: assume_static_loss_masks(False)
            static, masks = masks[0], ()
        if masks:
            self.set_loss_pairs(*masks)
        if static and not self._dense_plan.from_masks:
            raise ValueError("assume_static_loss_masks needs the loss masks: assume_static_loss_masks(pos_train_adj, "
                             "neg_train_adj), or call set_loss_pairs(...) first")
        self._dense_plan.static = bool(static)
        return self

    def _no_declaration_in_dense_mode(self, what: str):
        if getattr(self, "link_pred_backward", "plan") == "dense":
            raise ValueError(f"{what}: link_pred_backward=\"dense\" differentiates every entry of link_pred and needs no "
                             "declaration of where the loss is taken")

    def _graph_of(self, adj) -> Graph:
        """``adj`` as the methods below take it: a prebuilt Graph, or the dense adj_sym."""
        return adj if isinstance(adj, Graph) else self._graph_for(adj)

    def _graph_for(self, adj: torch.Tensor) -> Graph:
        """CSR + plans of a dense adjacency, built once per adjacency tensor: keyed on the tensor OBJECT (weak
        reference) and its version counter — an address can be reused by a different tensor, an object cannot."""
        hit = self._graph_cache
        if hit is None or hit[0]() is not adj or hit[1] != adj._version:
            hit = (weakref.ref(adj), adj._version, Graph.from_dense(adj, row_bytes=self.nfactor * self.nebed * 4))
            self._graph_cache = hit
        return hit[2]

    # ------------------------------------------------------------------ forward
    def forward(self, x, adj):
        """(emb [N,K*d], link_pred [N,N]) exactly as model.py:105-114; ``adj`` is the dense adj_sym
        (or a prebuilt ``Graph``)."""
        graph = self._graph_of(adj)
        Z = self.project(x)
        H = ops.RouteAggregate.apply(Z, graph, float(self.beta), float(self.temperature))
        if getattr(self, "link_pred_backward", "plan") == "dense":
            if not (Z.dtype == torch.float32 and ops.score_allpairs_bwd_dense_supported(self.nfactor, self.nebed)):
                raise ops._lib.DisenlinkHipError(
                    f"link_pred_backward=\"dense\" serves fp32 tables and factor widths d <= 128 (got {Z.dtype}, "
                    f"d = {self.nebed}); there is no eager fallback — use link_pred_backward=\"plan\"")
            return H.view(H.shape[0], -1), ops.ScoreAllPairsDense.apply(Z, H, float(self.temperature))
        link_pred = ops.ScoreAllPairs.apply(Z, H, float(self.temperature), self._dense_plan)
        # (a Tensor whose indexing reports the entries taken to this module's pair-plan cache: ops.LinkPred)
        return H.view(H.shape[0], -1), ops.as_link_pred(link_pred, self._dense_plan)

    def forward_logits(self, x, adj):
        """(emb [N,K*d], link_logits [N,N]): ``forward`` with the dense scores left in LOGIT space — a plain tensor, for
        ``F.binary_cross_entropy_with_logits(link_logits[mask], ...)`` or any other loss; ``emb`` has ``forward``'s bits.  Its
        backward is the dense one (ops.ScoreAllPairsLogits: the gradient of whatever is done with it, no declaration of
        where the loss is taken), so it raises where that does not serve — d > 128, non-fp32 tables — as
        ``link_pred_backward="dense"`` does.  ``forward`` itself is untouched."""
        if not (self.table_dtype == torch.float32 and ops.score_allpairs_bwd_dense_supported(self.nfactor, self.nebed)):
            raise ops._lib.DisenlinkHipError(
                f"forward_logits serves fp32 tables and factor widths d <= 128 (got {self.table_dtype}, d = {self.nebed}); "
                f"there is no eager fallback")
        graph = self._graph_of(adj)
        Z = self.project(x)
        H = ops.RouteAggregate.apply(Z, graph, float(self.beta), float(self.temperature))
        return H.view(H.shape[0], -1), ops.ScoreAllPairsLogits.apply(Z, H, float(self.temperature))

    def forward_pairs_loss(self, x, graph: Graph, pairs: PairList, label, weight):
        """(emb [N,K*d], prob [P], loss) with loss = sum_q weight BCE(prob, label) (main_disentangled.py:195 on a pair
        list; metrics.pair_bce_weights): the training step's scorer runs forward and backward in one pass
        (ops.HotPathPairsLoss).  Falls back to forward_pairs + the fused loss where no tuned kernel exists."""
        Z = self.project(x)
        dt = ops.table_code(self.table_dtype)
        one_pass = ops.one_pass_scorer_wanted(self.table_dtype, Z.shape[0], Z.shape[1], Z.shape[2])     # the rule and its numbers: there
        if one_pass and ops.score_pairs_train_supported(pairs, Z.shape[1], Z.shape[2], dt):
            if Z.dtype == torch.float32 and graph.n_rows == graph.n_nodes:
                from . import native                            # the compiled binding: the same step as ONE C++ autograd node
                if native.available():
                    H, prob, loss = native.hot_path_pairs_loss(Z, graph, pairs, float(self.beta), float(self.temperature),
                                                               label, weight, self.table_dtype)
                    return H.view(H.shape[0], -1), prob, loss
            H, prob, loss = ops.HotPathPairsLoss.apply(Z, graph, pairs, float(self.beta), float(self.temperature),
                                                       self.table_dtype, label, weight)
            return H.view(H.shape[0], -1), prob, loss
        H, prob = ops.HotPathPairs.apply(Z, graph, pairs, float(self.beta), float(self.temperature), self.table_dtype)
        return H.view(H.shape[0], -1), prob, ops.PairBCE.apply(prob, label, weight)

    def forward_pair_logits(self, x, graph: Graph, pairs: PairList):
        """(emb [N,K*d], logit [P]): ``forward_pairs`` with the scores left in LOGIT space — the value the sigmoid is taken
        of, differentiable (ops.HotPathPairLogits).  A fp32 probability is exactly 1 from logit 16.64 on; the logit keeps its
        order (AUC, ranking) and its gradient there."""
        Z = self.project(x)
        H, logit = ops.HotPathPairLogits.apply(Z, graph, pairs, float(self.beta), float(self.temperature), self.table_dtype)
        return H.view(H.shape[0], -1), logit

    def forward_pair_logits_loss(self, x, graph: Graph, pairs: PairList, label, weight):
        """(emb [N,K*d], logit [P], loss) with loss = sum_q weight BCE-with-logits(logit, label): ``forward_pairs_loss`` in
        logit space, with its dispatch rule — one pass (ops.HotPathPairLogitsLoss, or the compiled node) where
        ``one_pass_scorer_wanted`` and the shape say so, forward_pair_logits + ops.PairBCELogits otherwise.  A saturated pair
        keeps its gradient and its loss; an overflowed exp is NOT cured (its gradient is huge, infinite or NaN)."""
        if label.numel() != pairs.n_pairs or weight.numel() != pairs.n_pairs:
            raise ValueError("label / weight must cover the pair list")
        Z = self.project(x)
        dt = ops.table_code(self.table_dtype)
        one_pass = ops.one_pass_scorer_wanted(self.table_dtype, Z.shape[0], Z.shape[1], Z.shape[2])
        if one_pass and ops.score_pairs_train_logits_supported(pairs, Z.shape[1], Z.shape[2], dt):
            if Z.dtype == torch.float32 and graph.n_rows == graph.n_nodes:
                from . import native
                if native.available():
                    H, logit, loss = native.hot_path_pair_logits_loss(Z, graph, pairs, float(self.beta), float(self.temperature),
                                                                      label, weight, self.table_dtype)
                    return H.view(H.shape[0], -1), logit, loss
            H, logit, loss = ops.HotPathPairLogitsLoss.apply(Z, graph, pairs, float(self.beta), float(self.temperature),
                                                             self.table_dtype, label, weight)
            return H.view(H.shape[0], -1), logit, loss
        H, logit = ops.HotPathPairLogits.apply(Z, graph, pairs, float(self.beta), float(self.temperature), self.table_dtype)
        return H.view(H.shape[0], -1), logit, ops.PairBCELogits.apply(logit, label, weight)

    def forward_pairs_resampled_loss(self, x, graph: Graph, pos_pairs: PairList, label, weight, sampled, k, neg_weight: float,
                                     order=None, k_rowptr=None):
        """(emb [N,K*d], prob [P], neg_prob [E], loss): the positive list ``pos_pairs`` with (label, weight) through the one-pass
        scorer, plus this epoch's sampled negatives — ``sampled`` (an ``ops.SampledNegatives``) with the partners ``k`` of
        ``ops.sample_negatives``, label 0 and the one weight ``neg_weight`` — through ``ops.score_sampled_train``, over one
        hot-path forward and one backward (ops.HotPathPairsResampledLoss).  Duplicated draws are separate loss terms and a
        failed draw (k = -1) is no term.  fp32 tables only; a shape without a one-pass scorer runs the positive list through
        forward_pairs' node and the sampled trainer as a node of its own.
        ``k`` may be an ``ops.HardDraw`` in place of a tensor (hard negatives): the forward then draws its candidates, under
        no_grad, from the tables it has just computed and keeps the highest-scoring one per entry; ``order`` / ``k_rowptr``
        cannot be given with it; afterwards ``k.k`` and ``k.logit`` hold the draw."""
        return self._forward_resampled(x, graph, pos_pairs, label, weight, sampled, k, neg_weight, False, order, k_rowptr)

    def forward_pair_logits_resampled_loss(self, x, graph: Graph, pos_pairs: PairList, label, weight, sampled, k,
                                           neg_weight: float, order=None, k_rowptr=None):
        """``forward_pairs_resampled_loss`` in LOGIT space: the scores are logits, the loss BCE with logits on both lists."""
        return self._forward_resampled(x, graph, pos_pairs, label, weight, sampled, k, neg_weight, True, order, k_rowptr)

    def _forward_resampled(self, x, graph, pos_pairs, label, weight, sampled, k, neg_weight, logit, order, k_rowptr):
        ops.check_hard_draw(k, order, k_rowptr)
        if self.table_dtype != torch.float32:
            raise TypeError("resampled negatives are trained on fp32 tables only (bf16 tables are not served)")
        if label.numel() != pos_pairs.n_pairs or weight.numel() != pos_pairs.n_pairs:
            raise ValueError("label / weight must cover the pair list")
        Z = self.project(x)
        K, d = Z.shape[1], Z.shape[2]
        if not ops.score_sampled_supported(K, d):
            raise ops._lib.DisenlinkHipError(f"the sampled trainer serves K <= 64 and K d <= 2048 (got K={K}, d={d}); there is no "
                                             "eager fallback")
        ok = ops.score_pairs_train_logits_supported if logit else ops.score_pairs_train_supported
        if not ok(pos_pairs, K, d, ops.table_code(torch.float32)):
            # no one-pass scorer for the positive list at this shape: forward_pairs' node and the fused loss for it, the
            # sampled trainer as a node of its own over (Z, H) — its gradient on H arrives at the first node as d/d emb
            beta, t = float(self.beta), float(self.temperature)
            if logit:
                H, score = ops.HotPathPairLogits.apply(Z, graph, pos_pairs, beta, t, torch.float32)
                loss = ops.PairBCELogits.apply(score, label, weight)
            else:
                H, score = ops.HotPathPairs.apply(Z, graph, pos_pairs, beta, t, torch.float32)
                loss = ops.PairBCE.apply(score, label, weight)
            node = ops.SampledLogitsLoss if logit else ops.SampledLoss
            loss_neg, neg_score = node.apply(Z, H, t, sampled, k, float(neg_weight))
            return H.view(H.shape[0], -1), score, neg_score, loss + loss_neg
        H, score, neg_score, loss = ops.HotPathPairsResampledLoss.apply(
            Z, graph, pos_pairs, float(self.beta), float(self.temperature), label, weight, sampled, k, float(neg_weight),
            logit, order, k_rowptr)
        return H.view(H.shape[0], -1), score, neg_score, loss

    def forward_bpr_loss(self, x, graph: Graph, sampled, k, weight: float, val_pairs: PairList = None, order=None, k_rowptr=None):
        """(emb [N,K*d], pos_logit [n_rows], neg_logit [E], val_logit [P] | None, loss): the pairwise ranking objective (BPR) —
        every training edge row (src, dst) of ``sampled`` (an ``ops.SampledNegatives`` built with ``dst``) must score above
        (src, k) for its m partners ``k`` of ``ops.sample_negatives``: loss = sum weight softplus(neg_logit - pos_logit[row])
        over the entries with k >= 0, through ``ops.score_sampled_bpr_train`` over one hot-path forward and one backward
        (ops.HotPathBprLoss).  ``val_pairs``: a list whose logits come out of the same forward (forward only: no gradient).
        Duplicated draws are separate terms, a failed draw (k = -1) is none.  fp32 tables only, logit space only.
        ``k`` may be an ``ops.HardDraw`` (hard negatives: the forward draws from its own tables; no ``order`` / ``k_rowptr``)."""
        ops.check_hard_draw(k, order, k_rowptr)
        if self.table_dtype != torch.float32:
            raise TypeError("the ranking objective is trained on fp32 tables only (bf16 tables are not served)")
        Z = self.project(x)
        K, d = Z.shape[1], Z.shape[2]
        if not ops.score_sampled_bpr_supported(K, d):
            raise ops._lib.DisenlinkHipError(f"the ranking trainer serves K <= 64 and K d <= 2048 (got K={K}, d={d}); there is no "
                                             "eager fallback")
        H, pos, neg, val, loss = ops.HotPathBprLoss.apply(Z, graph, float(self.beta), float(self.temperature), sampled, k,
                                                          float(weight), val_pairs, order, k_rowptr)
        return H.view(H.shape[0], -1), pos, neg, (None if val_pairs is None else val), loss

    def forward_recon_loss(self, x, graph: Graph, ignore=None, pos_weight=None, block_rows=None, node_filter=None):
        """(emb [N,K*d], loss): the whole-graph reconstruction loss (ops.score_recon_loss) of project -> RouteAggregate ->
        ops.ReconLoss (a bf16 module, ``table_dtype=torch.bfloat16``: project -> ops.HotPathRecon, one node that routes,
        aggregates and scores on the bf16 tables the module is evaluated, ranked and mined on) — every pair of nodes that is not an edge of ``graph`` is a negative, the edges are up-weighted by
        ``pos_weight`` (default n_neg / n_pos), pairs in ``ignore`` (held-out validation / test pairs) carry no loss —
        with nothing of size N x N in memory.  ``graph``: the training graph the model routes over; its edges are the
        positives.  ``ignore`` may be a prepared ``ops.recon_sets(graph, ignore, N, device)``, which then supplies both
        sets and skips the normalisation (and its host read) per call.  No tile is skipped: a zero gradient against an
        overflowed exp gives NaN, as with ``link_pred_backward="dense"``.  d <= 128; anything else raises.
        ``node_filter`` (an ``ops.NodeFilter``): only pairs its unordered rule admits carry loss — a denied pair, edge or not,
        is an ignored one, and the default ``pos_weight`` is that of the admitted pairs; it goes into ``ops.recon_sets`` where
        ``ignore`` is not already prepared sets, which carry their own (another beside them raises ValueError)."""
        return self._forward_recon(x, graph, ignore, pos_weight, block_rows, ops.ReconLoss, ops.HotPathRecon, node_filter)

    def forward_recon_logits_loss(self, x, graph: Graph, ignore=None, pos_weight=None, block_rows=None, node_filter=None):
        """(emb [N,K*d], loss): ``forward_recon_loss`` in LOGIT space (ops.score_recon_logits_loss), with its arguments and its
        dispatch — fp32: RouteAggregate + ops.ReconLogitsLoss, bf16: ops.HotPathReconLogits.  A pair past the saturation of
        the fp32 sigmoid keeps its cost and its gradient (a non-edge scored at +20 is pushed back; the probability form
        charges it 100 w with gradient exactly 0); an overflowed exp is NOT cured: loss and gradients are then non-finite.
        The device counts stand in ``ops.ReconLogitsLoss.last_counts``."""
        return self._forward_recon(x, graph, ignore, pos_weight, block_rows, ops.ReconLogitsLoss, ops.HotPathReconLogits, node_filter)

    def _forward_recon(self, x, graph, ignore, pos_weight, block_rows, loss_node, hot_node, node_filter=None):
        _own_filter(ignore, node_filter)                               # beside prepared sets: their own, or none
        Z = self.project(x)
        sets = ignore if isinstance(ignore, ops.ReconSets) else ops.recon_sets(graph, ignore, Z.shape[0], Z.device, node_filter)
        if self.table_dtype == torch.bfloat16:
            H, loss = hot_node.apply(Z, graph, sets, float(self.beta), float(self.temperature), self.table_dtype,
                                     pos_weight, block_rows)
            return H.view(H.shape[0], -1), loss
        H = ops.RouteAggregate.apply(Z, graph, float(self.beta), float(self.temperature))
        loss = loss_node.apply(Z, H, float(self.temperature), sets, pos_weight, block_rows)
        return H.view(H.shape[0], -1), loss

    def forward_pairs(self, x, graph: Graph, pairs: PairList):
        """(emb [N,K*d], prob [P]) — the same model evaluated on a pair list only."""
        if self.use_torch_ops and isinstance(x, SparseFeatures):
            raise TypeError("use_torch_ops=True: the registered torch.ops.disenlink operators take dense features; a "
                            "SparseFeatures input runs through the autograd.Functions (use_torch_ops=False)")
        if self.use_torch_ops and not self.single_layer and self.table_dtype == torch.float32 and x.is_cuda \
                and ops.project_supported(self.nebed):
            from . import torch_ops
            return torch_ops.forward_pairs(self, x, torch_ops.register_graph(graph), torch_ops.register_pairs(pairs))
        Z = self.project(x)
        H, prob = ops.HotPathPairs.apply(Z, graph, pairs, float(self.beta), float(self.temperature), self.table_dtype)
        return H.view(H.shape[0], -1), prob

    # ------------------------------------------------------------------ ranking (inference only)
    def _rank_tables(self, x, adj, table_dtype=None):
        """Z and H of forward(x, adj) — the same projection and routing / aggregation, under no_grad.  ``table_dtype``:
        None = fp32 tables; torch.bfloat16 = the tables the training step of a bf16 module gathers from (ops.step_tables,
        which ops.HotPathPairs.forward calls too): Z rounded to bf16, H routed and aggregated from THAT Z and stored as bf16."""
        graph = self._graph_of(adj)
        with torch.no_grad():
            Z = self.project(x)
            if table_dtype is None or table_dtype is torch.float32:
                return Z, ops.RouteAggregate.apply(Z, graph, float(self.beta), float(self.temperature))
            if table_dtype is not torch.bfloat16:
                raise TypeError(f"table_dtype must be None, torch.float32 or torch.bfloat16, got {table_dtype!r}")
            Zt, _p, _a, _s, H = ops.step_tables(graph, Z, float(self.beta), float(self.temperature), table_dtype)
            return Zt, H

    @staticmethod
    def _scan_dtype(table_dtype):
        """The ``table_dtype`` keyword of the ops scans for this one (None = fp32)."""
        return torch.float32 if table_dtype is None else table_dtype

    @staticmethod
    def _logit_floor(min_prob) -> float:
        """``min_prob`` in [0, 1] as the logit floor of the scans (0.5 -> 0.0; None = no floor)."""
        if min_prob is None:
            return float("-inf")
        p = float(min_prob)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"min_prob={p} outside [0, 1]")
        return float("-inf") if p == 0.0 else float("inf") if p == 1.0 else math.log(p) - math.log1p(-p)

    def topk_links(self, x, adj, queries, k: int, exclude=None, exclude_self: bool = True, node_filter=None,
                   table_dtype=None) -> TopLinks:
        """The k most likely links of every node in ``queries``: TopLinks(index int64 [Q,k], logit, prob f32 [Q,k]),
        ranked by the pre-sigmoid logit of link_pred (prob = link_pred's value).  ``adj`` as in forward; ``exclude``: a
        Graph, a dense [N,N] mask or (rows, cols) of pairs that are not candidates; ``node_filter``: an ops.NodeFilter, a
        rule on node groups that candidates must pass as well (ops.score_topk).  ``table_dtype`` (here and in the four
        methods below): None = fp32 tables; torch.bfloat16 = the scan runs on the bf16 tables the training step gathers
        from (a module trained with ``table_dtype=torch.bfloat16`` passes ``model.table_dtype`` to rank the model it
        trained; on an fp32-trained module it is an approximation: operands rounded to bf16, exact arithmetic on them)."""
        Z, H = self._rank_tables(x, adj, table_dtype)
        return TopLinks(*ops.score_topk(Z, H, float(self.temperature), queries, k, exclude, exclude_self, node_filter,
                                        self._scan_dtype(table_dtype)))

    def link_ranks(self, x, adj, src, dst, exclude=None, node_filter=None, table_dtype=None):
        """(greater, ties) int64 per target pair (src[i], dst[i]) among all nodes except src[i] and its exclusion set
        and, with ``node_filter`` (an ops.NodeFilter), the nodes its group may not take
        (ops.score_ranks; metrics.ranking_metrics turns them into MRR / Hits@K)."""
        Z, H = self._rank_tables(x, adj, table_dtype)
        return ops.score_ranks(Z, H, float(self.temperature), src, dst, exclude, node_filter, self._scan_dtype(table_dtype))

    def top_missing_links(self, x, adj, m: int, exclude=None, min_prob=None, node_filter=None, table_dtype=None,
                          block_nodes=None) -> MinedLinks:
        """The m most likely links of the WHOLE graph that are not known yet: MinedLinks(src, dst int32 [c], logit, prob
        f32 [c]) with src < dst, c = min(m, eligible pairs), ranked by the pre-sigmoid logit of link_pred over all
        unordered pairs (ops.score_mine; nothing of size N x N is formed).  ``exclude``: the known pairs, as a Graph, a
        dense [N,N] mask or (rows, cols), in either orientation; None = the edges of ``adj`` itself.  ``min_prob``: keep
        only pairs with link_pred >= min_prob (turned into a logit floor on the host: 0.5 -> 0.0).  ``node_filter``: a
        symmetric ops.NodeFilter, a rule on node groups that pairs must pass as well.  Graphs of more than 46,340 nodes
        (or any graph, with ``block_nodes``: rows per block, a multiple of 128) are scanned by blocks
        (ops.score_mine_blocks): the same list, equal logits ordered by the 64-bit src * N + dst."""
        graph = self._graph_of(adj)
        Z, H = self._rank_tables(x, graph, table_dtype)
        floor = self._logit_floor(min_prob)
        known = graph if exclude is None else exclude
        with torch.no_grad():
            if block_nodes is not None or int(Z.shape[0]) > ops.MINE_MAX_N:
                return MinedLinks(*ops.score_mine_blocks(Z, H, float(self.temperature), m, known, floor, node_filter,
                                                         self._scan_dtype(table_dtype), block_nodes))
            return MinedLinks(*ops.score_mine(Z, H, float(self.temperature), m, known, floor, node_filter,
                                              self._scan_dtype(table_dtype)))

    def predicted_links(self, x, adj, min_prob, exclude=None, node_filter=None, table_dtype=None,
                        block_nodes=None) -> PredictedLinks:
        """The predicted graph: EVERY unordered pair whose link_pred reaches ``min_prob`` and that is not known yet, as
        PredictedLinks(rowptr, col, logit, prob), a symmetric CSR over all nodes with ``.degree``, ``.pairs()`` and
        ``.to_graph()`` (ops.score_links: two scans, nothing of size N x N is formed, no cap on the number of links).
        ``exclude``: the known pairs, as a Graph, a dense [N,N] mask or (rows, cols), in either orientation; None = the
        edges of ``adj`` itself.  ``min_prob`` in [0, 1] is turned into a logit floor on the host, as in
        ``top_missing_links`` (0.5 -> 0.0).  ``node_filter``: a symmetric ops.NodeFilter that pairs must pass as well.
        Graphs of more than 46,340 nodes (or any graph, with ``block_nodes``: rows per block, a multiple of 128) are
        scanned by blocks (ops.score_links_blocks): the same CSR."""
        graph = self._graph_of(adj)
        Z, H = self._rank_tables(x, graph, table_dtype)
        floor = self._logit_floor(float(min_prob))
        known = graph if exclude is None else exclude
        with torch.no_grad():
            if block_nodes is not None or int(Z.shape[0]) > ops.LINKS_MAX_N:
                return PredictedLinks(*ops.score_links_blocks(Z, H, float(self.temperature), floor, known, node_filter,
                                                              self._scan_dtype(table_dtype), block_nodes))
            return PredictedLinks(*ops.score_links(Z, H, float(self.temperature), floor, known, node_filter,
                                                   self._scan_dtype(table_dtype)))

    def top_predicted_links(self, x, adj, m: int, exclude=None, min_prob=None, node_filter=None,
                            table_dtype=None) -> PredictedLinks:
        """The predicted graph under a BUDGET: the m most likely links that are not known yet, for any m >= 1 ("the 1 % most
        likely pairs", "five million links"), as the PredictedLinks of ``predicted_links`` — the pairs ``top_missing_links``
        would list if it had no cap on m, in the layout of a graph (ops.score_top_links: the select of the mining, then the
        two scans of ``predicted_links``; nothing of size N x N is formed and no threshold has to be known).  There are
        exactly min(m, eligible pairs) links; tied logits across the cut are taken by ascending src * N + dst.  ``exclude``,
        ``min_prob`` and ``node_filter`` as in ``top_missing_links`` (``exclude`` may also be a prepared
        ``ops.pair_exclusion``); ``min_prob`` and the budget both hold.  N <= 46,340."""
        graph = self._graph_of(adj)
        Z, H = self._rank_tables(x, graph, table_dtype)
        floor = self._logit_floor(min_prob)
        with torch.no_grad():
            return PredictedLinks(*ops.score_top_links(Z, H, float(self.temperature), m, graph if exclude is None else exclude,
                                                       floor, node_filter, self._scan_dtype(table_dtype)))

    def explain_links(self, x, adj, src, dst, table_dtype=None) -> "ops.PairTerms":
        """Which factor makes the links (src[i], dst[i]): ops.PairTerms(e, q, cum) f32 [P, K] with ``.logit``, ``.contrib``
        [P, K] and ``.factor`` int64 [P] (ops.score_pair_terms: the pass of the scans with its per-factor terms written
        out).  Row src[i] is the A operand: pass the pairs as ``top_missing_links`` or ``predicted_links().pairs()``
        list them (src < dst) and ``.logit`` has the bits they report."""
        Z, H = self._rank_tables(x, adj, table_dtype)
        with torch.no_grad():
            return ops.score_pair_terms(Z, H, float(self.temperature), src, dst, self._scan_dtype(table_dtype))

    def missing_link_ranks(self, x, adj, src, dst, exclude=None, node_filter=None, table_dtype=None) -> PairRanks:
        """Where the unordered pairs {src[i], dst[i]} stand among ALL unordered pairs of the graph, in the order
        ``top_missing_links`` lists from the top: PairRanks(greater, ties int64 [T], logit f32 [T], n_others int64 [T])
        (ops.score_pair_ranks: one target pass and one scan, nothing of size N x N; metrics.global_ranking_metrics turns
        them into the AUC against every non-edge, MRR and recall@M).  ``exclude``: the pairs that are no candidates, as
        in ``top_missing_links``; None = the edges of ``adj``.  ``node_filter``: a symmetric ops.NodeFilter that candidates
        must pass as well.  A target is ranked whether or not it is excluded or allowed."""
        graph = self._graph_of(adj)
        Z, H = self._rank_tables(x, graph, table_dtype)
        with torch.no_grad():
            return PairRanks(*ops.score_pair_ranks(Z, H, float(self.temperature), src, dst, graph if exclude is None else exclude,
                                                   node_filter, self._scan_dtype(table_dtype)))
