"""The call path of the dense projection wrappers without a GPU: a recording stand-in takes the library's place, and what
project_fwd / project_bwd hand to the C ABI is held against the prototype in _lib.EXPORTS — one entry call per wrapper call
whatever the padding (F % 4 != 0, a factor width below the tile width), the padded sizes as the integer arguments, NULL
exactly where a layer or the kept hidden layer is absent, and results of the caller's own shapes.  (The sparse wrappers
refuse a CPU SparseFeatures before any call: tests/test_gpu_project_paths.py runs them.)"""
import ast
import inspect

import pytest
import torch

from disenlink_amd import _lib, ops, optim, project

N, F, FP, K, NHID, TILE = 9, 37, 40, 4, 8, 32
FWD, BWD = "dl_project_fwd_xp", "dl_project_bwd_xp"


class Recorder:
    """Stands for the loaded library: every symbol is a function that notes (name, args); sizers return 4096, entries 0
    (DL_OK)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 4096 if "_bytes" in name or "_floats" in name else 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(project, "_need_cuda", lambda *tensors: None)
    monkeypatch.setattr(project, "_stream", lambda: 0)
    monkeypatch.setattr(project, "_empty", lambda shape, dtype, device: torch.zeros(shape, dtype=dtype, device=device))
    return r


def _weights(d, two):
    gen = torch.Generator().manual_seed(d + two)
    x = torch.randn(N, F, generator=gen)
    if two:
        return (x, torch.randn(K, NHID, F, generator=gen), torch.randn(K, NHID, generator=gen),
                torch.randn(K, d, NHID, generator=gen), torch.randn(K, d, generator=gen))
    return x, torch.randn(K, d, F, generator=gen), torch.randn(K, d, generator=gen), None, None


def _one_entry(rec, entry):
    """The recorded calls are sizers, then ONE call of `entry` with the prototype's argument count -> its arguments."""
    names = [n for n, _ in rec.calls]
    assert names[-1] == entry and len(names) >= 2, names
    assert all("_bytes" in n or "_floats" in n for n in names[:-1]), names
    args = rec.calls[-1][1]
    assert len(args) == len(_lib.EXPORTS[entry][1])
    return args


@pytest.mark.parametrize("keep", [False, True], ids=["nokeep", "keep"])
@pytest.mark.parametrize("two", [True, False], ids=["two", "single"])
@pytest.mark.parametrize("d", [8, 32])
def test_forward_is_one_entry_call_at_the_padded_sizes(rec, d, two, keep):
    x, W1, b1, W2, b2 = _weights(d, two)
    out = project.project_fwd(x, W1, b1, W2, b2, keep_hid=keep)
    args = _one_entry(rec, FWD)
    assert args[1:6] == (N, FP, K, NHID if two else 1, TILE)
    assert (args[8] is None) == (args[9] is None) == (not two)          # W2, b2
    assert (args[11] is None) == (not (two and keep))                   # hid
    assert args[14] is None                                             # x planes: first sight
    assert ("dl_project_hidden_floats" in [n for n, _ in rec.calls]) == (two and keep)
    if keep and (two or d == TILE):
        Z, hid = out
        assert (hid is None) == (not two)
    else:                                                               # (a padded single layer hands back Z alone, asked or not)
        Z = out
    assert tuple(Z.shape) == (N, K, d) and Z.is_contiguous()


@pytest.mark.parametrize("kept", [False, True], ids=["recompute", "kept"])
@pytest.mark.parametrize("two", [True, False], ids=["two", "single"])
@pytest.mark.parametrize("d", [8, 32])
def test_backward_is_one_entry_call_and_gradients_have_the_weights_shapes(rec, d, two, kept):
    x, W1, b1, W2, _b2 = _weights(d, two)
    dZ = torch.randn(N, K, d)
    hid = torch.zeros(4096) if kept else None
    grads = project.project_bwd(x, W1, b1, W2, dZ, hid=hid)
    args = _one_entry(rec, BWD)
    assert args[1:6] == (N, FP, K, NHID if two else 1, TILE)
    assert (args[8] is None) == (args[13] is None) == (args[14] is None) == (not two)     # W2, dW2, db2
    assert (args[10] is None) == (not (two and kept))                   # hid
    assert args[17] is None                                             # x planes
    dW1, db1, dW2, db2 = grads
    assert dW1.shape == W1.shape and db1.shape == b1.shape
    if two:
        assert dW2.shape == W2.shape and tuple(db2.shape) == (K, d)
    else:
        assert dW2 is None and db2 is None
    live = [g for g in grads if g is not None]
    assert all(g.is_contiguous() for g in live)
    if d == TILE:                                                       # one allocation, back to back ...
        assert optim.flat_view(live) is not None
        rec.calls.clear()
        sep = project.project_bwd(x, W1, b1, W2, dZ, hid=hid, one_allocation=False)
        _one_entry(rec, BWD)
        assert optim.flat_view([g for g in sep if g is not None]) is None              # ... or separate tensors
    elif two:                                                           # trimmed copies of the last layer's gradients
        assert optim.flat_view(live) is None


def test_refusals(rec):
    x, W1, b1, _W2, _b2 = _weights(32, False)
    with pytest.raises(_lib.DisenlinkHipError):
        project.project_fwd(x, torch.randn(K, 130, F), torch.randn(K, 130))
    with pytest.raises(ValueError):
        project.project_fwd(x, torch.randn(K, 32, F + 1), b1)
    with pytest.raises(ValueError):
        project.project_bwd(x, torch.randn(K, 32, F + 1), b1, None, torch.randn(N, K, 32))
    assert rec.calls == []


def test_ops_reexports_the_moved_names():
    tree = ast.parse(inspect.getsource(ops))
    names = [a.name for node in tree.body if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module == "project"
             for a in node.names]
    for want in ("_XPlanes", "_pad_features", "keep_hidden", "project_fwd", "project_bwd", "project_sparse_fwd",
                 "project_sparse_bwd", "project_supported", "project_tile_width", "padded_features", "xplanes_for", "Project"):
        assert want in names, want
    for name in names:
        assert getattr(ops, name) is getattr(project, name), name
