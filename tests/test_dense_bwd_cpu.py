"""CPU-only checks of the dense backward of link_pred (dl_score_allpairs_bwd_dense, Disentangle(link_pred_backward=)):
argument validation happens before the device is touched, the workspace size behaves, and the module's mode switch
raises, copies and pickles as it should."""
import copy
import ctypes as C
import io
import pickle

import pytest
import torch


FAKE = 0x1000          # a non-null "device pointer": validation never dereferences


def _lib():
    from disenlink_amd import _lib, build
    build.build()
    return _lib.load()


def _call(lib, N=5, K=4, d=8, t=1.0, Z=FAKE, H=FAKE, prob=FAKE, g=FAKE, dZ=FAKE, dH=FAKE, ws=None, ws_bytes=0):
    return lib.dl_score_allpairs_bwd_dense(Z, H, N, K, d, t, prob, g, dZ, dH, ws, ws_bytes, None)


def test_dense_backward_rejects_bad_arguments_without_a_gpu():
    lib = _lib()
    assert _call(lib, N=46341) == -1 and b"46340" in lib.dl_last_error()
    assert _call(lib, N=-1) == -1 and b"46340" in lib.dl_last_error()
    assert _call(lib, d=129) == -1 and b"d <= 128" in lib.dl_last_error()
    assert _call(lib, d=4096) == -1 and b"d <= 128" in lib.dl_last_error()
    assert _call(lib, d=0) == -1 and b"d=0" in lib.dl_last_error()
    assert _call(lib, K=0) == -1 and b"K=0" in lib.dl_last_error()
    assert _call(lib, K=65) == -1 and b"K=65" in lib.dl_last_error()
    assert _call(lib, t=0.0) == -1 and b"temperature" in lib.dl_last_error()
    for name in ("Z", "H", "prob", "g", "dZ", "dH"):
        assert _call(lib, **{name: None}) == -1 and b"NULL" in lib.dl_last_error(), name
    need = lib.dl_score_allpairs_bwd_dense_workspace_bytes(5, 4, 8)
    assert need > 0
    assert _call(lib) == -3 and b"workspace" in lib.dl_last_error()                          # no workspace
    assert _call(lib, ws=FAKE, ws_bytes=need - 1) == -3 and b"workspace" in lib.dl_last_error()
    assert str(need).encode() in lib.dl_last_error()
    # N = 0 succeeds, with nothing to write and nothing to read
    assert _call(lib, N=0, Z=None, H=None, prob=None, g=None, dZ=None, dH=None) == 0


def test_dense_backward_workspace_size():
    lib = _lib()
    sup, ws = lib.dl_score_allpairs_bwd_dense_supported, lib.dl_score_allpairs_bwd_dense_workspace_bytes
    assert all(sup(K, d) == 1 for K in (1, 3, 8, 64) for d in (1, 8, 32, 64, 100, 128))
    assert all(sup(K, d) == 0 for K, d in ((0, 8), (65, 8), (4, 0), (4, 129), (4, 256), (-1, -1)))
    for N, K, d in ((100, 0, 8), (100, 65, 8), (100, 4, 0), (100, 4, 129), (0, 4, 8), (-3, 4, 8), (46341, 4, 8)):
        assert ws(N, K, d) == 0, (N, K, d)
    for K, d in ((1, 8), (3, 100), (8, 64), (16, 128), (64, 32)):
        prev = 0
        for N in list(range(1, 1500)) + list(range(1500, 46341, 61)) + [46340]:
            b = ws(N, K, d)
            assert b >= prev and b >= 4 * N * N, (N, K, d, b, prev)                          # G^ alone is N^2 floats
            prev = b


def _model(**kw):
    from disenlink_amd.model import Disentangle
    return Disentangle(12, 6, 8, nfactor=3, beta=0.5, t=1, **kw)


def test_link_pred_backward_keyword():
    with pytest.raises(ValueError, match="link_pred_backward"):
        _model(link_pred_backward="bogus")
    with pytest.raises(ValueError, match="link_pred_backward"):
        _model(link_pred_backward=None)
    assert _model().link_pred_backward == "plan"
    assert _model(link_pred_backward="plan").link_pred_backward == "plan"
    assert _model(link_pred_backward="dense").link_pred_backward == "dense"


def test_dense_mode_survives_deepcopy_and_pickle_and_keeps_the_state_dict_keys():
    torch.manual_seed(0)
    plan, dense = _model(), _model(link_pred_backward="dense")
    assert list(plan.state_dict().keys()) == list(dense.state_dict().keys())
    cp = copy.deepcopy(dense)
    assert cp.link_pred_backward == "dense"
    un = pickle.loads(pickle.dumps(dense))
    assert un.link_pred_backward == "dense"
    buf = io.BytesIO()
    torch.save(dense, buf)
    buf.seek(0)
    ld = torch.load(buf, weights_only=False)
    assert ld.link_pred_backward == "dense"
    for m in (cp, un, ld):
        assert list(m.state_dict().keys()) == list(dense.state_dict().keys())
        for k, v in dense.state_dict().items():
            assert torch.equal(m.state_dict()[k], v)
        with pytest.raises(ValueError, match="needs no"):
            m.set_loss_pairs(torch.ones(4, 4))
    assert copy.deepcopy(plan).link_pred_backward == "plan"


def test_declarations_raise_in_dense_mode_only():
    dense, plan = _model(link_pred_backward="dense"), _model()
    mask = torch.ones(5, 5)
    with pytest.raises(ValueError, match="needs no"):
        dense.set_loss_pairs(mask)
    with pytest.raises(ValueError, match="needs no"):
        dense.set_loss_pairs()
    with pytest.raises(ValueError, match="needs no"):
        dense.assume_static_loss_masks(mask, mask)
    with pytest.raises(ValueError, match="needs no"):
        dense.assume_static_loss_masks(static=False)
    plan.set_loss_pairs()                                     # plan mode: forgetting a declaration still works
    assert dense._dense_plan.rebuilds == 0


def test_operator_refuses_cpu_tensors_and_bad_shapes():
    from disenlink_amd import _lib as L, ops
    Z = torch.zeros(4, 2, 8)
    with pytest.raises(L.DisenlinkHipError, match="GPU"):
        ops.score_allpairs_bwd_dense(Z, Z, 1.0, torch.zeros(4, 4), torch.zeros(4, 4))
    assert ops.score_allpairs_bwd_dense_supported(8, 100) and not ops.score_allpairs_bwd_dense_supported(8, 129)
