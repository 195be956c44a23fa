"""The dense matrix-core backward of link_pred (ops.score_allpairs_bwd_dense, Disentangle(link_pred_backward="dense"))
against an fp64 restatement of its formulas, the pair-plan backward, the reference fixtures and CPU autograd."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_case_names, load_golden, load_trajectory, trajectory_names
from oracle import dense_ref, metrics_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from disenlink_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
def bwd64(Z, H, t, prob, g):
    """fp64 restatement of the dense backward on the SAME fp32 prob and g_prob:
         G = g o p o (1 - p),  G^ = G + G^T,  per k: E = exp(Z_k Z_k^T / t), Q = H_k H_k^T,
         dH_k = (G^ o E) H_k,  dZ_k = (G^ o Q o E / t) Z_k,
    and the project's error band as test_gpu_rank.py::logits64 defines it — 1e-5 x the sum of the absolute values of all
    addends of the output element, each dot product's magnitude taken as the sum of its |products| (what fp32 rounding
    scales with): an addend of dH is G^ E H[v,c], whose factor E = exp(z.z / t) moves by E |z|.|z| / t per unit relative
    rounding of the products of z.z; an addend of dZ is G^ Q E Z[v,c] / t with |Q| taken as |h|.|h| and the same term
    for E.  Returns dZ, dH, band_dZ, band_dH (fp64 [N,K,d])."""
    Zd, Hd, p, gd = Z.double(), H.double(), prob.double(), g.double()
    G = gd * p * (1.0 - p)
    Gh, Ga = G + G.t(), G.abs() + G.t().abs()
    zz = torch.einsum("ukd,vkd->kuv", Zd, Zd)
    hh = torch.einsum("ukd,vkd->kuv", Hd, Hd)
    za = torch.einsum("ukd,vkd->kuv", Zd.abs(), Zd.abs())
    ha = torch.einsum("ukd,vkd->kuv", Hd.abs(), Hd.abs())
    E = torch.exp(zz / t)
    dH = torch.einsum("kuv,vkc->ukc", Gh * E, Hd)
    dZ = torch.einsum("kuv,vkc->ukc", Gh * hh * E / t, Zd)
    bH = 1e-5 * torch.einsum("kuv,vkc->ukc", Ga * E * (1.0 + za / t), Hd.abs())
    bZ = 1e-5 * torch.einsum("kuv,vkc->ukc", Ga * E * (ha + hh.abs() * za / t) / t, Zd.abs())
    return dZ, dH, bZ, bH


def tables(N, K, d, seed, scale=0.5):
    gen = torch.Generator().manual_seed(seed)
    Z = (torch.randn(N, K, d, generator=gen) * scale / d ** 0.5).to(DEV)
    H = (torch.randn(N, K, d, generator=gen) * scale / d ** 0.5).to(DEV)
    return Z, H


def gradient(kind, N, seed):
    gen = torch.Generator().manual_seed(seed + 1000)
    g = torch.randn(N, N, generator=gen)
    if kind == "dense":
        pass                                                   # random, not symmetric
    elif kind == "upper":
        g = torch.triu(g, diagonal=1)
    elif kind == "offdiag":
        u, v = (N // 3, (2 * N) // 3 + 1) if N > 1 else (0, 0)  # N = 1 has no off-diagonal entry: the only entry there is
        one = torch.zeros(N, N)
        one[u, min(v, N - 1)] = 1.7
        g = one
    elif kind == "diag":
        one = torch.zeros(N, N)
        one[N // 2, N // 2] = -2.3
        g = one
    return g.to(DEV)


def worst(got, want, band):
    """max over elements of |got - want| / band (0 / 0 = 0: an element without addends must be exactly zero)."""
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / band)
    return float(r.max()) if r.numel() else 0.0


GRID = list(itertools.product((1, 37, 128, 129, 300, 700), (1, 3, 8), (8, 32, 64, 100, 128), (1.0, 2.0)))


@pytest.mark.parametrize("kind", ["dense", "upper", "offdiag", "diag"])
@pytest.mark.parametrize("N,K,d,t", GRID)
def test_operator_matches_fp64(N, K, d, t, kind):
    from disenlink_amd import ops
    Z, H = tables(N, K, d, seed=N * 131 + K * 17 + d)
    prob = ops.score_allpairs_fwd(Z, H, t)
    g = gradient(kind, N, seed=N + K + d)
    dZ, dH = ops.score_allpairs_bwd_dense(Z, H, t, prob, g)
    rZ, rH, bZ, bH = bwd64(Z, H, t, prob, g)
    assert dZ.shape == Z.shape and dH.shape == Z.shape and dZ.dtype == torch.float32
    assert bool(torch.isfinite(dZ).all()) and bool(torch.isfinite(dH).all())
    wZ, wH = worst(dZ, rZ, bZ), worst(dH, rH, bH)
    print(f"dense bwd N={N} K={K} d={d} t={t} {kind}: worst error / band  dZ {wZ:.4f}  dH {wH:.4f}")
    assert wZ <= 1.0 and wH <= 1.0, (wZ, wH)


@pytest.mark.parametrize("N,K,d,t", [(300, 8, 64, 1.0), (129, 3, 100, 2.0), (700, 4, 32, 1.0), (257, 8, 8, 1.0)])
def test_dense_and_plan_backwards_agree_on_a_masked_gradient(N, K, d, t):
    from disenlink_amd import ops
    Z, H = tables(N, K, d, seed=5 * N + d)
    prob = ops.score_allpairs_fwd(Z, H, t)
    gen = torch.Generator().manual_seed(N)
    mask = (torch.rand(N, N, generator=gen) < 0.05).to(DEV)
    g = gradient("dense", N, seed=N) * mask
    cache = ops.DensePairPlanCache()
    cache.set_pairs(N, torch.device(DEV), mask)
    pZ, pH = ops.score_allpairs_bwd(Z, H, cache.pairs, t, prob, g)
    dZ, dH = ops.score_allpairs_bwd_dense(Z, H, t, prob, g)
    _rZ, _rH, bZ, bH = bwd64(Z, H, t, prob, g)
    wZ, wH = worst(dZ, pZ.double(), 2 * bZ), worst(dH, pH.double(), 2 * bH)
    print(f"dense vs plan N={N} K={K} d={d}: worst difference / (sum of the two bands)  dZ {wZ:.4f}  dH {wH:.4f}")
    assert wZ <= 1.0 and wH <= 1.0, (wZ, wH)


# ---------------------------------------------------------------------------------------------------------------------
def _sd(g):
    return {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}


def _module(g, mode):
    from disenlink_amd.model import Disentangle
    m = g["meta"]
    model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"], link_pred_backward=mode)
    model.load_state_dict(_sd(g))
    return model.to(DEV)


@pytest.mark.parametrize("name", golden_case_names())
def test_dense_mode_meets_the_reference_loss_and_gradients(name):
    """The reference's call sequence with NO declaration: what test_dropin_module_loss_and_grads_match_reference asserts."""
    g = load_golden(name)
    m = g["meta"]
    model = _module(g, "dense")
    x, adj, ori, pm, nm = (torch.from_numpy(g[k]).to(DEV) for k in ("x", "adj", "ori_adj", "pos_mask", "neg_mask"))
    emb, a_pred = model(x, adj)
    assert type(a_pred) is torch.Tensor
    loss = (F.binary_cross_entropy(a_pred[pm == 1].unsqueeze(0), ori[pm == 1].unsqueeze(0))
            + F.binary_cross_entropy(a_pred[nm == 1].unsqueeze(0), ori[nm == 1].unsqueeze(0)) / m["m"])
    model.zero_grad()
    loss.backward()
    np.testing.assert_allclose(emb.detach().cpu().numpy(), g["emb"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(a_pred.detach().cpu().numpy(), g["link_pred"], rtol=1e-5, atol=1e-5)
    assert abs(loss.item() - float(g["loss"])) <= 2e-5 * max(1.0, abs(float(g["loss"])))
    for k, prm in model.named_parameters():
        ref = g["grad__" + k]
        scale = max(np.abs(ref).max(), 1e-6)
        err = np.abs(prm.grad.cpu().numpy() - ref).max()
        print(f"{name} {k}: error / scale {err / scale:.2e}")
        assert err <= 1e-4 * scale, (k, err, scale)
    assert model._dense_plan.rebuilds == 0 and model._dense_plan.pairs is None


@pytest.mark.parametrize("name", trajectory_names())
def test_dense_mode_follows_the_reference_training_trajectory(name):
    """test_dropin_module_follows_the_reference_training_trajectory's loop and tolerances, in dense mode."""
    g = load_trajectory(name)
    m = g["meta"]
    model = _module(g, "dense")
    opt = torch.optim.Adam(model.parameters(), lr=m["lr"], weight_decay=5e-4)
    x, adj, ori = (torch.from_numpy(g[k]).to(DEV) for k in ("x", "adj", "ori_adj"))
    mk = {k[6:]: torch.from_numpy(g[k]).to(DEV) for k in g if k.startswith("mask__")}
    best, kept = 0.0, None
    for ep in range(m["epochs"]):
        model.train()
        _emb, a_pred = model(x, adj)
        assert type(a_pred) is torch.Tensor
        loss = (F.binary_cross_entropy(a_pred[mk["pos_train"] == 1].unsqueeze(0), ori[mk["pos_train"] == 1].unsqueeze(0))
                + F.binary_cross_entropy(a_pred[mk["neg_train"] == 1].unsqueeze(0), ori[mk["neg_train"] == 1].unsqueeze(0)) / m["m"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        model.eval()
        auc = metrics_ref.auc_tie_avg(ori[mk["val"] == 1].cpu().numpy(), a_pred[mk["val"] == 1].detach().cpu().numpy())
        assert abs(loss.item() - g["losses"][ep]) <= 2e-4 * abs(g["losses"][ep]), (ep, loss.item(), g["losses"][ep])
        assert abs(auc - g["val_aucs"][ep]) <= 2e-3, (ep, auc, g["val_aucs"][ep])
        if auc > best:
            best, kept = auc, {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.load_state_dict(kept)
    _emb, a_pred = model(x, adj)
    test_auc = metrics_ref.auc_tie_avg(ori[mk["test"] == 1].cpu().numpy(), a_pred[mk["test"] == 1].detach().cpu().numpy())
    assert abs(test_auc - float(g["test_auc"])) <= 5e-3
    assert model._dense_plan.rebuilds == 0


@pytest.mark.parametrize("name", golden_case_names())
def test_whole_matrix_bce_dense_mode_equals_plan_mode_on_an_all_ones_plan(name):
    """A reconstruction BCE over the WHOLE matrix: dense mode against plan mode with every entry declared.  The forward
    bits are the same, so the gradient entering both backwards is identical; tolerance 1e-4 x scale."""
    g = load_golden(name)
    N = g["meta"]["N"]
    x, adj, ori = (torch.from_numpy(g[k]).to(DEV) for k in ("x", "adj", "ori_adj"))
    grads = {}
    for mode in ("plan", "dense"):
        model = _module(g, mode)
        if mode == "plan":
            model.set_loss_pairs(torch.ones(N, N))
        _emb, a_pred = model(x, adj)
        loss = F.binary_cross_entropy(a_pred, ori)
        model.zero_grad()
        loss.backward()
        grads[mode] = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
        grads[mode + "_pred"] = a_pred.detach()
    assert torch.equal(grads["plan_pred"], grads["dense_pred"])
    for k, ref in grads["plan"].items():
        scale = max(np.abs(ref).max(), 1e-6)
        err = np.abs(grads["dense"][k] - ref).max()
        print(f"{name} whole-matrix BCE {k}: |dense - plan| / scale {err / scale:.2e}")
        assert np.isfinite(ref).all() and err <= 1e-4 * scale, (k, err, scale)


WHOLE_CASES = ["k3_d8_hub", "k4_d32", "k4_d8", "k8_d32", "k8_d64", "k8_d8_t2", "tiny_k1", "tiny_k3"]


@pytest.mark.parametrize("loss_kind", ["mean", "weighted", "weighted_t"])
@pytest.mark.parametrize("name", WHOLE_CASES)
def test_whole_matrix_losses_match_cpu_autograd(name, loss_kind):
    """a_pred.mean(), (a_pred * w).sum() / N^2 and (a_pred.t() * w).sum() / N^2 against fp32 CPU autograd of the oracle's
    dense forward; tolerance 1e-4 x scale.  (k5_d64 and k16_d128 are left out: on them the reference's own fp32 gradient
    differs from its fp64 gradient by 1.2e-3 to 2.3e-2 of the scale; on the cases here by at most 3.3e-5.)"""
    g = load_golden(name)
    m = g["meta"]
    N = m["N"]
    w = torch.rand(N, N, generator=torch.Generator().manual_seed(11)) - 0.3

    def the_loss(a_pred, w):
        if loss_kind == "mean":
            return a_pred.mean()
        if loss_kind == "weighted":
            return (a_pred * w).sum() / (N * N)
        return (a_pred.t() * w).sum() / (N * N)

    sd = {k: v.clone().requires_grad_(True) for k, v in _sd(g).items()}
    _e, P = dense_ref.forward(torch.from_numpy(g["x"]), torch.from_numpy(g["adj"]), sd, m["beta"], m["t"])
    the_loss(P, w).backward()
    model = _module(g, "dense")
    _emb, a_pred = model(torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["adj"]).to(DEV))
    model.zero_grad()
    the_loss(a_pred, w.to(DEV)).backward()
    for k, prm in model.named_parameters():
        ref = sd[k].grad.numpy()
        scale = max(np.abs(ref).max(), 1e-6)
        err = np.abs(prm.grad.cpu().numpy() - ref).max()
        print(f"{name} {loss_kind} {k}: error / scale {err / scale:.2e}")
        assert err <= 1e-4 * scale, (k, err, scale)
    assert model._dense_plan.rebuilds == 0


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,d", [(200, 3, 32), (129, 2, 100)])
def test_overflowed_exp_against_a_zero_gradient_gives_nan_like_autograd(N, K, d):
    """One pair whose z.z / t overflows exp (a node with a long z_0: its own diagonal entry — by Cauchy-Schwarz no
    off-diagonal pair can overflow without a diagonal one) and a gradient that is zero there: 0 * inf = NaN in the rows
    torch autograd of the eager formula makes non-finite, every other row within the band."""
    from disenlink_amd import ops
    Z, H = tables(N, K, d, seed=77)
    a = N // 2 + 1
    Z[a, 0, :] = 0.0
    Z[a, 0, 0] = 12.0                                         # z.z = 144 > log(FLT_MAX) = 88.7
    g = gradient("dense", N, seed=3)
    g[a, a] = 0.0
    prob = ops.score_allpairs_fwd(Z, H, 1.0)
    dZ, dH = ops.score_allpairs_bwd_dense(Z, H, 1.0, prob, g)
    Zt, Ht = Z.clone().requires_grad_(True), H.clone().requires_grad_(True)
    logit = (torch.einsum("ukd,vkd->kuv", Ht, Ht) * torch.exp(torch.einsum("ukd,vkd->kuv", Zt, Zt) / 1.0)).sum(0)
    (torch.sigmoid(logit) * g).sum().backward()
    badZ, badH = ~torch.isfinite(Zt.grad), ~torch.isfinite(Ht.grad)
    assert bool(badZ[a, 0].all()) and bool(badH[a, 0].all())                                 # the eager formula does give NaN there
    assert bool((~torch.isfinite(dZ))[badZ].all()) and bool((~torch.isfinite(dH))[badH].all())
    rZ, rH, bZ, bH = bwd64(Z, H, 1.0, prob, g)               # fp64: exp(144) is finite and the zero gradient removes the pair
    rowsZ, rowsH = ~badZ.any(-1), ~badH.any(-1)               # [N, K]: the rows the eager formula leaves finite
    assert int(rowsZ.sum()) == N * K - 1 and int(rowsH.sum()) == N * K - 1
    assert bool(torch.isfinite(dZ[rowsZ]).all()) and bool(torch.isfinite(dH[rowsH]).all())
    wZ, wH = worst(dZ[rowsZ], rZ[rowsZ], bZ[rowsZ]), worst(dH[rowsH], rH[rowsH], bH[rowsH])
    print(f"overflow N={N} K={K} d={d}: worst error / band on the finite rows  dZ {wZ:.4f}  dH {wH:.4f}")
    assert wZ <= 1.0 and wH <= 1.0, (wZ, wH)


# ---------------------------------------------------------------------------------------------------------------------
POISON = 0xFFFFFFFF


@pytest.mark.parametrize("N,K,d", [(129, 3, 100), (700, 8, 64), (300, 1, 8), (2100, 8, 128)])
def test_bitwise_reproducible_and_every_element_written(N, K, d):
    from disenlink_amd import ops
    assert ops._POISON, "the tests run with DL_POISON=1 (conftest.py)"
    Z, H = tables(N, K, d, seed=N)
    prob = ops.score_allpairs_fwd(Z, H, 1.0)
    g = gradient("dense", N, seed=9)
    a = ops.score_allpairs_bwd_dense(Z, H, 1.0, prob, g)
    b = ops.score_allpairs_bwd_dense(Z, H, 1.0, prob, g)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert not bool((x.view(torch.int32) == torch.tensor(POISON - (1 << 32), dtype=torch.int32, device=DEV)).any())
        assert bool(torch.isfinite(x).all())


def test_gradient_layouts_expanded_and_transposed():
    from disenlink_amd import ops
    N, K, d = 150, 3, 32
    Z, H = tables(N, K, d, seed=1)
    prob = ops.score_allpairs_fwd(Z, H, 1.0)
    g = gradient("dense", N, seed=2)
    want = ops.score_allpairs_bwd_dense(Z, H, 1.0, prob, g)
    got = ops.score_allpairs_bwd_dense(Z, H, 1.0, prob, g.t().contiguous().t())             # transposed strides
    assert all(torch.equal(x, y) for x, y in zip(want, got))
    ones = ops.score_allpairs_bwd_dense(Z, H, 1.0, prob, torch.full((N, N), 0.25, device=DEV))
    exp = ops.score_allpairs_bwd_dense(Z, H, 1.0, prob, torch.tensor(0.25, device=DEV).expand(N, N))   # stride 0
    assert all(torch.equal(x, y) for x, y in zip(ones, exp))


def test_launches_follow_the_current_stream():
    from disenlink_amd import ops
    N, K, d = 700, 8, 64
    Z, H = tables(N, K, d, seed=4)
    prob = ops.score_allpairs_fwd(Z, H, 1.0)
    g = gradient("dense", N, seed=5)
    want = ops.score_allpairs_bwd_dense(Z, H, 1.0, prob, g)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device=DEV)
    with torch.cuda.stream(side):
        for _ in range(8):
            big = big @ big * 1e-2                            # work ahead of the inputs on the side stream
        Zs, Hs, gs, ps = Z * 1.0, H * 1.0, g * 1.0, prob * 1.0     # produced on the side stream, consumed by our kernels
        got = ops.score_allpairs_bwd_dense(Zs, Hs, 1.0, ps, gs)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(want, got))


def _sync_debug_mode_is_honoured():
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_dense_mode_step_does_not_synchronise():
    """Forward + backward in dense mode with a whole-matrix loss: no device synchronisation (sync debug mode "error");
    where the build does not honour that mode, the step is captured in ONE graph — a host read cannot be captured — and
    a replay must reproduce the eager gradients bit for bit."""
    g = load_golden("k8_d64")
    model = _module(g, "dense")
    x, adj, ori = (torch.from_numpy(g[k]).to(DEV) for k in ("x", "adj", "ori_adj"))
    params = list(model.parameters())

    def step():
        _emb, a_pred = model(x, adj)
        loss = F.binary_cross_entropy(a_pred, ori) + 0.1 * a_pred.mean()
        return torch.autograd.grad(loss, params)

    eager = [v.clone() for v in step()]                       # builds the graph of adj (host work, once) and the workspace
    torch.cuda.synchronize()
    if _sync_debug_mode_is_honoured():
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            step()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            again = step()
        graph.replay()
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    assert model._dense_plan.rebuilds == 0


def test_unsupported_width_raises_in_forward():
    from disenlink_amd import _lib
    from disenlink_amd.model import Disentangle
    model = Disentangle(16, 1, 160, nfactor=2, beta=0.5, t=1, projection="library", link_pred_backward="dense").to(DEV)
    x = torch.randn(40, 16, device=DEV)
    adj = (torch.rand(40, 40, device=DEV) < 0.2).float()
    adj = ((adj + adj.t()) > 0).float()
    with pytest.raises(_lib.DisenlinkHipError, match="d <= 128"):
        model(x, adj)
