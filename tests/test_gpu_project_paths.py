"""The two weight forms of Disentangle.project on the GPU, against each other: a module on its shared [K, ...] buffers (the
per-factor Parameters are the autograd inputs, the gradients are slices of the stacked gradients) and a twin with the same
weights in which one Parameter object was replaced, which stacks its parameters per call.  Same kernels, same inputs: Z and
every parameter's gradient must be the same bits, for dense features and for SparseFeatures, at factor widths that run
padded (d = 8 at the tile width 32, F = 37 at 40) and at the kernels' own."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, K = 301, 3
CASES = [(37, 24, 8), (37, 1, 8), (64, 24, 64), (64, 1, 64)]          # (F, nhid, d): both paddings, then none (compiled node)


def _features(kind, F):
    if kind == "dense":
        return torch.randn(N, F, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    from disenlink_amd.features import SparseFeatures
    rng = np.random.default_rng(5)
    x = (rng.random((N, F)) < 0.1).astype(np.float32)
    x[:, 0] = 1.0                                                        # no constant row under standardisation...
    x[:, 1] = 0.0                                                        # ... and a column without entries
    return SparseFeatures.from_dense(x, standardise=True).to(DEV)


def _modules(F, nhid, d):
    from disenlink_amd.model import Disentangle
    torch.manual_seed(1)
    stacked = Disentangle(F, nhid, d, nfactor=K, beta=0.9).to(DEV)
    twin = Disentangle(F, nhid, d, nfactor=K, beta=0.9).to(DEV)
    twin.load_state_dict(stacked.state_dict())
    lin = twin.factor_1.mlp if nhid == 1 else twin.factor_1.mlp2
    lin.weight = torch.nn.Parameter(lin.weight.detach().clone())
    assert stacked._stacked_params() is not None and twin._stacked_params() is None
    return stacked, twin


@pytest.mark.parametrize("kind", ["dense", "sparse"])
@pytest.mark.parametrize("F,nhid,d", CASES)
def test_stacked_and_unstacked_weights_give_the_same_bits(F, nhid, d, kind):
    from disenlink_amd.optim import flat_view
    x = _features(kind, F)
    G = torch.randn(N, K, d, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    stacked, twin = _modules(F, nhid, d)
    out = {}
    for name, m in (("stacked", stacked), ("twin", twin)):
        Z = m.project(x)
        assert tuple(Z.shape) == (N, K, d)
        (Z * G).sum().backward()
        out[name] = (Z.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()})
    assert torch.equal(out["stacked"][0], out["twin"][0])
    for k, g in out["stacked"][1].items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
        assert torch.equal(g, out["twin"][1][k]), k
    if (nhid, d) == (24, 64):                                            # slices of one allocation: one all-reduce, no stacking in Adam
        assert flat_view([p.grad for p in stacked._stacked_params()]) is not None
    # a second backward accumulates
    for name, m in (("stacked", stacked), ("twin", twin)):
        (m.project(x) * G).sum().backward()
        for k, p in m.named_parameters():
            assert torch.equal(p.grad, 2 * out[name][1][k]), (name, k)
