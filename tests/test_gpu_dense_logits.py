"""The dense link_logits (ops.score_allpairs_logits_fwd, ops.score_allpairs_logits_bwd_dense, ops.ScoreAllPairsLogits,
Disentangle.forward_logits) against fp64, against the probability entry, and against the logit-space reconstruction loss on
the same included pairs."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

import recon_logits_ref as rl
import recon_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID_KD = ((1, 8), (3, 100), (8, 64), (4, 128))


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from disenlink_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()


@functools.lru_cache(maxsize=None)
def tables(N, K, d, saturated):
    """recon_ref's tables; ``saturated``: H rescaled (t = 1) so that the largest included |logit| is 60.  Below N = 129 the
    rescaling of N = 129 is taken over the first N rows."""
    if not saturated:
        return recon_ref.tables_cpu(N, K, d, recon_ref.table_seed(N, K, d))
    if N >= 129:
        return rl.saturated_tables(N, K, d, 1.0)[:2]
    Z, H = rl.saturated_tables(129, K, d, 1.0)[:2]
    return Z[:N].clone(), H[:N].clone()


# ---------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("N,Kd,saturated", list(itertools.product((1, 37, 128, 129, 300), GRID_KD, (False, True))))
def test_logits_match_fp64_are_symmetric_and_are_what_the_probability_entry_takes_the_sigmoid_of(N, Kd, saturated):
    """Within band_s (the logits64 convention) of the fp64 logits; symmetric bit for bit; and wherever |L| < 16,
    |sigmoid64(L) - score_allpairs_fwd| <= 3e-7: sigmoid_ref is one expf, one add and one IEEE division, under 3 ulp of 1, of
    the SAME fp32 logit where the probability entry runs the matrix-core kernel (d % 32 == 0).  For the other widths that entry
    runs a vector kernel with a logit of its own; both lie within band_s of fp64 and |d sigmoid / d x| <= 1 / 4, so the bound
    there is 3e-7 + band_s / 2."""
    from disenlink_amd import _lib, ops
    K, d = Kd
    Z, H = tables(N, K, d, saturated)
    want, band = rl.logits64(Z, H, 1.0)[:2]
    L = ops.score_allpairs_logits_fwd(Z.to(DEV), H.to(DEV), 1.0)
    assert L.dtype == torch.float32 and tuple(L.shape) == (N, N) and bool(torch.isfinite(L).all())
    assert torch.equal(L, L.t())
    w = recon_ref.worst(L, want, band)
    prob = ops.score_allpairs_fwd(Z.to(DEV), H.to(DEV), 1.0).double().cpu()
    Ld = L.double().cpu()
    mfma = _lib.score_allpairs_fwd_form(N, K, d, _lib.DL_F32, 1 << 40)["kernel"] >= 2
    assert mfma == (d % 32 == 0)
    bound = torch.full_like(band, 3e-7) if mfma else 3e-7 + band / 2
    inside = Ld.abs() < 16
    gap = (torch.sigmoid(Ld) - prob).abs()
    print(f"dense logits N={N} K={K} d={d} saturated={saturated}: worst error / band {w:.4f}, max |L| {float(Ld.abs().max()):.4g}, "
          f"worst |sigmoid64(L) - prob| where |L| < 16: {float(gap[inside].max()) if bool(inside.any()) else 0.0:.2e}")
    assert w <= 1.0
    assert bool((gap[inside] <= bound[inside]).all())
    if saturated and N >= 129:
        assert float(Ld.abs().max()) > 50 and bool((prob[Ld > 17] == 1.0).all())      # where the probability entry holds no more


# --------------------------------------------------------------------------------------------------------- 2. backward
def logits_bwd64(Z, H, t, g):
    """test_gpu_dense_bwd.bwd64 with G = g as it stands (no p (1 - p) factor): dH_k = ((g + g^T) o E) H_k, dZ_k likewise, and
    its bands -> dZ, dH, band_dZ, band_dH (fp64, CPU)."""
    Zd, Hd, G = Z.double().cpu(), H.double().cpu(), g.double().cpu()
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


@pytest.mark.parametrize("N,Kd,t", list(itertools.product((1, 37, 129, 300), GRID_KD, (1.0, 2.0))))
def test_dense_backward_of_any_gradient_on_the_logits_matches_fp64(N, Kd, t):
    from disenlink_amd import ops
    K, d = Kd
    Z, H = tables(N, K, d, False)
    gen = torch.Generator().manual_seed(N + d)
    g = torch.randn(N, N, generator=gen)                                  # not symmetric
    row = torch.randn(1, N, generator=gen)
    Zg, Hg = Z.to(DEV), H.to(DEV)
    for tag, gg in (("random", g.to(DEV)), ("transposed", g.to(DEV).t()), ("stride 0", row.to(DEV).expand(N, N))):
        assert tag != "transposed" or N == 1 or not gg.is_contiguous()
        dZ, dH = ops.score_allpairs_logits_bwd_dense(Zg, Hg, t, gg)
        rZ, rH, bZ, bH = logits_bwd64(Z, H, t, gg)
        wZ, wH = recon_ref.worst(dZ, rZ, bZ), recon_ref.worst(dH, rH, bH)
        print(f"dense logits backward N={N} K={K} d={d} t={t} {tag}: worst error / band  dZ {wZ:.4f}  dH {wH:.4f}")
        assert dZ.shape == Z.shape and bool(torch.isfinite(dZ).all()) and bool(torch.isfinite(dH).all())
        assert wZ <= 1.0 and wH <= 1.0


def test_autograd_function_and_refusals():
    from disenlink_amd import _lib, ops
    N, K, d = 129, 3, 100
    Z, H = tables(N, K, d, False)
    Zg, Hg = Z.to(DEV).requires_grad_(True), H.to(DEV).requires_grad_(True)
    L = ops.ScoreAllPairsLogits.apply(Zg, Hg, 1.0)
    assert type(L) is torch.Tensor and torch.equal(L.detach(), ops.score_allpairs_logits_fwd(Z.to(DEV), H.to(DEV), 1.0))
    g = torch.randn(N, N, generator=torch.Generator().manual_seed(3)).to(DEV)
    dZ, dH = torch.autograd.grad(L, (Zg, Hg), g)
    wZ, wH = ops.score_allpairs_logits_bwd_dense(Z.to(DEV), H.to(DEV), 1.0, g)
    assert torch.equal(dZ, wZ) and torch.equal(dH, wH)
    wide = torch.randn(8, 2, 160, device=DEV)
    with pytest.raises(_lib.DisenlinkHipError, match="d <= 128"):
        ops.ScoreAllPairsLogits.apply(wide, wide, 1.0)
    with pytest.raises(_lib.DisenlinkHipError, match="d <= 128"):
        ops.score_allpairs_logits_bwd_dense(wide, wide, 1.0, torch.zeros(8, 8, device=DEV))
    assert tuple(ops.score_allpairs_logits_fwd(wide, wide, 1.0).shape) == (8, 8)      # the forward alone serves every d
    with pytest.raises(TypeError, match="fp32"):
        ops.ScoreAllPairsLogits.apply(Zg.detach().bfloat16(), Hg.detach().bfloat16(), 1.0)
    with pytest.raises(ValueError, match=r"\[N, N\]"):
        ops.score_allpairs_logits_bwd_dense(Z.to(DEV), H.to(DEV), 1.0, torch.zeros(N, N + 1, device=DEV))


# -------------------------------------------------------------------------------- 3. the two parts against each other
@pytest.mark.parametrize("N,Kd,saturated", list(itertools.product((129, 300), ((8, 64), (3, 100)), (False, True))))
def test_dense_route_agrees_with_the_reconstruction_loss_on_the_same_included_pairs(N, Kd, saturated):
    """Route A: dense logits + F.binary_cross_entropy_with_logits with the reconstruction weights over the upper triangle +
    the dense backward.  Route B: score_recon_logits_loss.  Within the sum of the two routes' bands: B's are the reference's;
    A's gradient comes from its own fp32 logits (the reference's dG term once more, inside band_dZ / band_dH) through the dense
    backward (logits_bwd64's band on its own g), and its fp32 loss sum carries 1e-5 x the sum of its addends."""
    from disenlink_amd import ops
    K, d = Kd
    Z, H = tables(N, K, d, saturated)
    pos, ign = recon_ref.pair_sets(N, seed=N)
    ref = rl.recon_logits64(Z, H, 1.0, pos, ign)
    Zg, Hg = Z.to(DEV), H.to(DEV)
    loss, dZ, dH, _counts = ops.score_recon_logits_loss(Zg, Hg, 1.0, pos.to(DEV), ign.to(DEV))
    inc = torch.triu(~ign, diagonal=1)
    w_pos, w_neg = ref["w"]
    y = (pos & inc).float().to(DEV)
    weight = (torch.where(pos, w_pos, w_neg) * inc).float().to(DEV)
    L = ops.score_allpairs_logits_fwd(Zg, Hg, 1.0).requires_grad_(True)
    dense_loss = F.binary_cross_entropy_with_logits(L, y, weight=weight, reduction="sum")
    (g,) = torch.autograd.grad(dense_loss, L)
    eZ, eH = ops.score_allpairs_logits_bwd_dense(Zg, Hg, 1.0, g)
    _rZ, _rH, bZ, bH = logits_bwd64(Z, H, 1.0, g)
    zero = torch.zeros_like(ref["dZ"])
    wZ = recon_ref.worst(dZ.double().cpu() - eZ.double().cpu(), zero, 2 * ref["band_dZ"] + bZ)
    wH = recon_ref.worst(dH.double().cpu() - eH.double().cpu(), zero, 2 * ref["band_dH"] + bH)
    wL = abs(float(loss) - float(dense_loss.detach())) / (2 * ref["band_loss"] + 1e-5 * ref["loss"])
    print(f"recon-logit vs dense logits N={N} K={K} d={d} saturated={saturated}: worst difference / (sum of the two bands)  "
          f"loss {wL:.4f}  dZ {wZ:.4f}  dH {wH:.4f}")
    assert wL <= 1.0 and wZ <= 1.0 and wH <= 1.0, (wL, wZ, wH)


# ------------------------------------------------------------------------------------------------------------ 4. module
def _sd(g):
    return {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}


def _module(g, **kw):
    from disenlink_amd.model import Disentangle
    m = g["meta"]
    model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"], **kw)
    model.load_state_dict(_sd(g))
    return model.to(DEV)


@pytest.mark.parametrize("name", ["k8_d64", "k4_d8"])
def test_forward_logits_of_the_module(name):
    """emb has forward's bits; the parameter gradients of a masked BCE-with-logits on link_logits follow the fp64 module
    reference within 1e-4 of each gradient's scale — k4_d8 holds logits up to 1,759, where link_pred is 0 or 1."""
    g = load_golden(name)
    N = g["meta"]["N"]
    want, ref, ign, n, big = rl.module_reference(g, torch.float64)
    model = _module(g)
    x, adj = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["adj"]).to(DEV)
    emb, L = model.forward_logits(x, adj)
    assert type(L) is torch.Tensor and tuple(L.shape) == (N, N) and L.requires_grad
    with torch.no_grad():
        emb0, prob0 = model.forward(x, adj)
    assert torch.equal(emb.detach().view(torch.int32), emb0.view(torch.int32))
    pos = (adj != 0) | (adj.t() != 0)
    mask = torch.triu(~ign, diagonal=1).to(DEV)
    y = (pos & mask).float()
    C = n[0] + n[1]
    weight = torch.where(y > 0, n[1] / n[0] / C, 1.0 / C).float()
    loss = F.binary_cross_entropy_with_logits(L[mask], y[mask], weight=weight[mask], reduction="sum")      # the idiom
    model.zero_grad()
    loss.backward()
    assert abs(loss.item() - want) <= 2e-5 * max(1.0, abs(want))
    worst = 0.0
    for k, p in model.named_parameters():
        scale = max(float(ref[k].abs().max()), 1e-6)
        err = float((p.grad.detach().cpu().double() - ref[k]).abs().max())
        worst = max(worst, err / scale)
        assert err <= recon_ref.MODULE_TOL * scale, (k, err, scale)
    print(f"{name} forward_logits: loss {loss.item():.7g} (fp64 {want:.7g}), largest included |logit| {big:.4g}, worst error / scale {worst:.2e}")


def test_forward_logits_raises_where_the_dense_backward_does_not_serve():
    from disenlink_amd import _lib
    from disenlink_amd.model import Disentangle
    x, adj = torch.zeros(6, 4, device=DEV), torch.zeros(6, 6, device=DEV)
    with pytest.raises(_lib.DisenlinkHipError, match="d <= 128"):
        Disentangle(4, 4, 160, nfactor=2, beta=0.5).to(DEV).forward_logits(x, adj)
    with pytest.raises(_lib.DisenlinkHipError, match="fp32 tables"):
        Disentangle(4, 4, 32, nfactor=4, beta=0.5, table_dtype=torch.bfloat16).to(DEV).forward_logits(x, adj)
