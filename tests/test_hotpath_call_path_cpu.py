"""The call path of the training step's operators without a GPU: a recording stand-in takes the library's place, and what
the raw wrappers and the autograd Functions of disenlink_amd.ops hand to the C ABI is held against the prototypes in
_lib.EXPORTS — the entry sequence of every Function, forward and backward, the head (struct, Z, K, d, table code) and the
tail (workspace, its size, stream) of every plan entry, the per-factor terms exactly where they exist, one question to the
workspace sizer per (owner, K, d), and refusals before any entry runs.  Graph.from_edge_rows and PairList.build run as
they are, on CPU tensors: a path graph of 9 nodes and 4 pairs."""
import ast
import ctypes as C
import inspect

import pytest
import torch

from disenlink_amd import _dev, _lib, link_pred, ops
from disenlink_amd.graph import Graph, PairList

N, K, D, P = 9, 4, 8, 4
BETA, T, STREAM = 0.6, 1.0, 77
SIZER = "dl_workspace_bytes"
GRAPH_ENTRIES = ("dl_route_fwd", "dl_aggregate_fwd", "dl_route_aggregate_bwd", "dl_route_aggregate_bwd_scaled",
                 "dl_route_aggregate_bwd_phase1", "dl_route_aggregate_bwd_phase2")
PAIR_ENTRIES = ("dl_score_pairs_bwd", "dl_score_pairs_train")


class Recorder:
    """Stands for the loaded library: every symbol is a function that notes (name, args); entries return 0 (DL_OK),
    sizers 4096 bytes, dl_has_fast_path_dtype ``fast``, dl_score_pairs_train_supported 1, dl_set_force_generic 0.  A plan
    entry must end in (the device's shared workspace, its size, the stream)."""

    def __init__(self):
        self.calls = []
        self.fast = 1

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name in GRAPH_ENTRIES + PAIR_ENTRIES:                     # the tail: the shared workspace as it is NOW
                ws = ops._ws.buf[torch.device("cpu")]
                assert args[-3:] == (ws.data_ptr(), ws.numel(), STREAM) and ws.numel() >= 4096, (name, args[-3:])
            if "_bytes" in name:
                return 4096
            return self.fast if name == "dl_has_fast_path_dtype" else 1 if name == "dl_score_pairs_train_supported" else 0
        return fn

    def entries(self):
        """Names of the recorded calls without the sizer's."""
        return [n for n, _ in self.calls if n != SIZER]

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    for mod in (_dev, ops, link_pred):
        monkeypatch.setattr(mod, "_need_cuda", lambda *tensors: None)
        monkeypatch.setattr(mod, "_stream", lambda: STREAM)
        monkeypatch.setattr(mod, "_empty", lambda shape, dtype, device: torch.zeros(shape, dtype=dtype, device=device))
        if hasattr(mod, "_empty_like"):
            monkeypatch.setattr(mod, "_empty_like", torch.zeros_like)
    return r


def _graph(n=N):
    src = torch.arange(n - 1)
    return Graph.from_edge_rows(src, src + 1, n)


def _pairs():
    return PairList.build(torch.tensor([0, 2, 5, 7]), torch.tensor([3, 8, 1, 4]), N)


def _Z(grad=True, n=N):
    return (torch.randn(n, K, D, generator=torch.Generator().manual_seed(3)) * 0.3).requires_grad_(grad)


def _yw():
    return torch.tensor([1.0, 0.0, 1.0, 0.0]), torch.full((P,), 0.25)


def _check(calls, Z=None, owner_of=None, code=_lib.DL_F32):
    """Every recorded entry has its prototype's argument count; plan entries have the head of the call path (the tail is
    checked by the stand-in, at the time of the call)."""
    for name, args in calls:
        assert len(args) == len(_lib.EXPORTS[name][1]), name
        if name in GRAPH_ENTRIES:
            assert type(args[0]).__name__ == "CArgObject", name
            if owner_of is not None:
                assert args[0]._obj is owner_of[name]._struct, name
            assert args[2:5] == (K, D, code), (name, args[2:5])
            if Z is not None:
                assert args[1] == Z.data_ptr(), name
        if name in PAIR_ENTRIES:
            assert args[2:5] == (K, D, code) and type(args[5]) is float, (name, args[2:6])
            assert type(args[6]).__name__ == "CArgObject", name
            if Z is not None:
                assert args[0] == Z.data_ptr(), name


# ------------------------------------------------------------------------------------------------ entry sequences
def test_hot_path_pairs_sequence_head_and_tail(rec):
    g, pairs, Z = _graph(), _pairs(), _Z()
    emb, prob = ops.HotPathPairs.apply(Z, g, pairs, BETA, T, torch.float32)
    fwd = rec.take()
    assert [n for n, _ in fwd if n != SIZER] == ["dl_route_fwd", "dl_aggregate_fwd", "dl_has_fast_path_dtype",
                                                 "dl_set_force_generic", "dl_score_pairs_fwd"]
    _check(fwd, Z, {"dl_route_fwd": g, "dl_aggregate_fwd": g})
    assert dict(fwd)["dl_score_pairs_fwd"][12] is not None              # coef: a gradient is wanted, the terms are there
    assert tuple(emb.shape) == (N, K, D) and tuple(prob.shape) == (P,)
    (prob.sum() + emb.sum()).backward()
    bwd = rec.take()
    assert [n for n, _ in bwd if n != SIZER] == ["dl_score_pairs_bwd", "dl_route_aggregate_bwd"]
    _check(bwd, Z, {"dl_route_aggregate_bwd": g})
    assert dict(bwd)["dl_score_pairs_bwd"][9] is not None               # ... and reaches the backward
    assert dict(bwd)["dl_route_aggregate_bwd"][12] == 1                 # onto the scorer's dZ
    assert Z.grad is not None and Z.grad.shape == Z.shape


@pytest.mark.parametrize("grad,fast", [(False, 1), (True, 0)], ids=["nograd", "noterms"])
def test_coef_is_null_without_a_gradient_or_without_terms(rec, grad, fast):
    rec.fast = fast
    g, pairs, Z = _graph(), _pairs(), _Z(grad)
    _emb, prob = ops.HotPathPairs.apply(Z, g, pairs, BETA, T, torch.float32)
    calls = rec.take()
    assert dict(calls)["dl_score_pairs_fwd"][12] is None
    assert ("dl_has_fast_path_dtype" in [n for n, _ in calls]) == grad
    if grad:
        prob.sum().backward()
        assert dict(rec.take())["dl_score_pairs_bwd"][9] is None


def test_hot_path_pairs_loss_sequences(rec):
    g, pairs = _graph(), _pairs()
    label, weight = _yw()
    Z = _Z()
    _emb, _prob, loss = ops.HotPathPairsLoss.apply(Z, g, pairs, BETA, T, torch.float32, label, weight)
    fwd = rec.take()
    assert [n for n, _ in fwd if n != SIZER] == ["dl_route_fwd", "dl_aggregate_fwd", "dl_score_pairs_train", "dl_pair_bce"]
    _check(fwd, Z, {"dl_route_fwd": g, "dl_aggregate_fwd": g})
    assert dict(fwd)["dl_score_pairs_train"][6]._obj is pairs._struct
    loss.backward()                                                     # loss only: d/dloss inside the last kernel
    bwd = rec.take()
    assert [n for n, _ in bwd if n != SIZER] == ["dl_route_aggregate_bwd_scaled"]
    _check(bwd, Z, {"dl_route_aggregate_bwd_scaled": g})
    Z2 = _Z()
    emb, prob, loss = ops.HotPathPairsLoss.apply(Z2, g, pairs, BETA, T, torch.float32, label, weight)
    rec.take()
    (loss + prob.sum() + emb.sum()).backward()                          # every gradient at once
    bwd = rec.take()
    assert [n for n, _ in bwd if n != SIZER] == ["dl_score_pairs_bwd", "dl_route_aggregate_bwd"]
    _check(bwd, Z2, {"dl_route_aggregate_bwd": g})
    assert dict(bwd)["dl_score_pairs_bwd"][9] is None                   # the one-pass scorer keeps no terms


def test_route_aggregate_and_pair_bce_sequences(rec):
    g, Z = _graph(), _Z()
    H = ops.RouteAggregate.apply(Z, g, BETA, T)
    fwd = rec.take()
    assert [n for n, _ in fwd if n != SIZER] == ["dl_route_fwd", "dl_aggregate_fwd"]
    _check(fwd, Z, {"dl_route_fwd": g, "dl_aggregate_fwd": g})
    H.sum().backward()
    bwd = rec.take()
    assert [n for n, _ in bwd if n != SIZER] == ["dl_route_aggregate_bwd"]
    _check(bwd, Z, {"dl_route_aggregate_bwd": g})
    assert dict(bwd)["dl_route_aggregate_bwd"][12] == 0                 # a dZ of its own
    label, weight = _yw()
    prob = torch.full((P,), 0.5, requires_grad=True)
    loss = ops.PairBCE.apply(prob, label, weight)
    calls = rec.take()
    assert [n for n, _ in calls] == ["dl_pair_bce"]
    _check(calls)
    args = calls[0][1]
    assert args[:4] == (prob.data_ptr(), label.data_ptr(), weight.data_ptr(), P) and args[7] >= 8192 and args[8] == STREAM
    loss.backward()
    assert rec.take() == [] and prob.grad.shape == prob.shape


def test_raw_backward_phases_follow_the_call_path(rec):
    g = _graph()
    Z = _Z(False)
    p, a, s = ops.route_fwd(g, Z, T)
    dH, ds = torch.zeros_like(Z), torch.zeros(N, K)
    dw, dwr = ops.route_aggregate_bwd_phase1(g, Z, BETA, p, a, s, dH, ds)
    dZ = torch.zeros_like(Z)
    assert ops.route_aggregate_bwd_phase2(g, Z, BETA, T, p, a, s, dH, dw, dwr, ds, dZ, True) is dZ
    calls = rec.take()
    assert [n for n, _ in calls if n != SIZER] == ["dl_route_fwd", "dl_route_aggregate_bwd_phase1",
                                                   "dl_route_aggregate_bwd_phase2"]
    _check(calls, Z, {n: g for n in GRAPH_ENTRIES})
    assert dict(calls)["dl_route_aggregate_bwd_phase2"][15] == 1        # accumulate


def test_bf16_tables_reach_every_entry_as_code_1(rec):
    g, pairs = _graph(), _pairs()
    label, weight = _yw()
    emb, prob, loss = ops.HotPathPairsLoss.apply(_Z(), g, pairs, BETA, T, torch.bfloat16, label, weight)
    loss.backward()
    emb, prob = ops.HotPathPairs.apply(_Z(), g, pairs, BETA, T, torch.bfloat16)
    (prob.sum() + emb.sum()).backward()
    calls = rec.take()
    _check(calls, code=_lib.DL_BF16)
    seen = [n for n, _ in calls]
    assert set(GRAPH_ENTRIES[:4]) | set(PAIR_ENTRIES) <= set(seen)
    assert all(args[5] == _lib.DL_BF16 for n, args in calls if n == "dl_score_pairs_fwd")
    assert all(args[2] == _lib.DL_BF16 for n, args in calls if n == "dl_has_fast_path_dtype")
    assert emb.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ the workspace sizer
def test_the_sizer_is_asked_once_per_owner_and_shape(rec):
    g1, g2, pairs = _graph(), _graph(12), _pairs()
    label, weight = _yw()
    Z12 = _Z(False, 12)
    for _ in range(3):                                                  # two graphs and a pair list, alive at once, in turn
        ops.HotPathPairsLoss.apply(_Z(), g1, pairs, BETA, T, torch.float32, label, weight)[2].backward()
        ops.RouteAggregate.apply(Z12, g2, BETA, T)
        ops.HotPathPairs.apply(_Z(), g1, pairs, BETA, T, torch.float32)[1].sum().backward()
    asked = [(C.addressof(args[0]._obj), args[1], args[2]) for n, args in rec.calls if n == SIZER]
    owners = [C.addressof(o._struct.csr) for o in (g1, g2, pairs)]
    assert sorted(asked) == sorted((o, K, D) for o in owners), asked
    rec.take()
    Zd = torch.randn(N, K, 2 * D)                                       # another shape: asked again, once
    for _ in range(2):
        ops.aggregate_fwd(g1, Zd, BETA, *ops.route_fwd(g1, Zd, T))
    assert [(args[1], args[2]) for n, args in rec.calls if n == SIZER] == [(K, 2 * D)]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_entry(rec):
    g, pairs, Z = _graph(), _pairs(), _Z(False)
    label, weight = _yw()
    H = torch.zeros_like(Z)
    with pytest.raises(ValueError, match="p_out and a_out come together"):
        ops.route_fwd(g, Z, T, p_out=torch.zeros(g.n_edges, dtype=torch.uint8))
    with pytest.raises(ValueError, match="rows, graph has"):
        ops.route_fwd(g, Z[:5], T)
    with pytest.raises(ValueError, match="rows, graph has"):
        ops.HotPathPairs.apply(_Z(True, 12), g, pairs, BETA, T, torch.float32)
    with pytest.raises(ValueError, match="must cover the pair list"):
        ops.score_pairs_train(Z, H, pairs, T, label[:3], weight[:3])
    with pytest.raises(ValueError, match="coef must be"):
        ops.score_pairs_bwd(Z, H, pairs, T, torch.zeros(P), torch.zeros(P), coef=torch.zeros(2, P, K + 1))
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ops.route_fwd(g, Z.double(), T)
    with pytest.raises(ValueError, match="differ in length"):
        ops.PairBCE.apply(torch.zeros(P), label, weight[:3])
    assert rec.entries() == []


# ------------------------------------------------------------------------------------------------ the move
MOVED = ("score_allpairs_fwd", "score_allpairs_bwd", "score_allpairs_bwd_dense", "score_allpairs_bwd_dense_supported",
         "DensePairPlanCache", "LinkPred", "as_link_pred", "ScoreAllPairs", "ScoreAllPairsDense")


def test_ops_reexports_the_moved_names():
    tree = ast.parse(inspect.getsource(ops))
    names = [a.name for node in tree.body if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module == "link_pred"
             for a in node.names]
    for want in MOVED:
        assert want in names, want
    for name in names:
        assert getattr(ops, name) is getattr(link_pred, name), name
