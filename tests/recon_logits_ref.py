"""fp64 CPU restatement of the whole-graph reconstruction loss in LOGIT space (recon.score_recon_logits_loss,
dl_score_recon_logits), with the project's error bands.  Tables, pair sets, ``worst`` and the band convention are
``recon_ref``'s; this file restates only what the logit-space contract changes.

The contract.  The included pairs, the labels y and the weights w of ``recon_ref``; for an included pair with logit s
  loss term = w l(s, y),  l = softplus(s) - s y  (= max(s, 0) - s y + log1p(exp(-|s|)): F.binary_cross_entropy_with_logits),
  d loss / d s = w (sigmoid(s) - y)  — no clamp of the logs, no clamp factor on the gradient,
and from G^ on (G^[u][v] = G^[v][u] = d loss / d s, 0 on the diagonal and for ignored pairs) the products of recon_ref.

Bands, derived exactly as in recon_ref's docstring with p = sigmoid(s) in fp64:
  band_s as there;  the kernel forms G^ from its own fp32 logit, so G^ moves by dG = w p (1 - p) band_s (|d G / d s| = w p (1 - p));
  band_loss = sum_pairs w |p - y| band_s + 1e-5 sum_pairs w l        (|d l / d s| = |p - y|);
  band_dH, band_dZ: recon_ref's expressions with this G^ and this dG.
sigmoid_minus_label's own relative error (4.8e-7, dl_common.h) sits inside the 1e-5 |G^| addend.  Derived, not tuned: nothing
here was set from kernel output.
"""
import torch
import torch.nn.functional as F

import recon_ref

SIGMOID_ONE = 16.64            # an fp32 sigmoid_ref is exactly 1 from this logit on
CLAMP_BELOW = -27.6            # p (1 - p) < 1e-12 below this logit: the probability form's gradient factor acts


def _sets(N, pos, ign, pos_weight):
    eye = torch.eye(N, dtype=torch.bool)
    pos = torch.as_tensor(pos).bool().cpu()
    pos = pos | pos.t()
    ign = torch.zeros(N, N, dtype=torch.bool) if ign is None else torch.as_tensor(ign).bool().cpu()
    inc = ~(ign | ign.t()) & ~eye
    y = pos & inc
    n_pos, n_neg = int(y.sum()) // 2, int((inc & ~pos).sum()) // 2
    C = n_pos + n_neg
    if pos_weight is None:
        pos_weight = n_neg / n_pos if n_pos else 1.0
    w_pos, w_neg = (pos_weight / C, 1.0 / C) if C else (0.0, 0.0)
    W = torch.where(y, torch.full((N, N), w_pos, dtype=torch.float64), torch.full((N, N), w_neg, dtype=torch.float64)) * inc
    return inc, y, W, (n_pos, n_neg), pos_weight, (w_pos, w_neg)


def logits64(Z, H, t):
    """-> (s, band_s, E, hh, |z|.|z|, |h|.|h|): the fp64 logits of all ordered pairs, their band (the logits64 convention) and
    the per-factor pieces the gradient bands need."""
    Zd, Hd = Z.detach().double().cpu(), H.detach().double().cpu()
    zz = torch.einsum("ukd,vkd->kuv", Zd, Zd)
    hh = torch.einsum("ukd,vkd->kuv", Hd, Hd)
    za = torch.einsum("ukd,vkd->kuv", Zd.abs(), Zd.abs())
    ha = torch.einsum("ukd,vkd->kuv", Hd.abs(), Hd.abs())
    E = torch.exp(zz / t)
    s = (hh * E).sum(0)
    band_s = 1e-5 * (E * (ha + hh.abs() * za / t)).sum(0)
    return s, band_s, E, hh, za, ha


def recon_logits64(Z, H, t, pos, ign=None, pos_weight=None):
    """-> dict as recon_ref.recon64: loss, dZ, dH (fp64), counts, band_loss, band_dZ, band_dH, logit, included, w."""
    Zd, Hd = Z.detach().double().cpu(), H.detach().double().cpu()
    N = Zd.shape[0]
    inc, y, W, counts, pos_weight, w = _sets(N, pos, ign, pos_weight)
    s, band_s, E, hh, za, ha = logits64(Z, H, t)
    yf = y.double()
    p = torch.sigmoid(s)
    l = F.softplus(s) - s * yf
    G = W * (p - yf)
    dG = W * p * (1.0 - p) * band_s
    Ga = G.abs()
    out = {"counts": counts, "pos_weight": pos_weight, "w": w, "logit": s, "included": inc, "label": y}
    out["loss"] = 0.5 * float((W * l).sum())
    out["band_loss"] = 0.5 * float((W * (p - yf).abs() * band_s).sum() + 1e-5 * (W * l).sum())
    out["dH"] = torch.einsum("kuv,vkc->ukc", G * E, Hd)
    out["dZ"] = torch.einsum("kuv,vkc->ukc", G * hh * E / t, Zd)
    out["band_dH"] = torch.einsum("kuv,vkc->ukc", 1e-5 * Ga * E * (1.0 + za / t) + dG * E, Hd.abs())
    out["band_dZ"] = torch.einsum("kuv,vkc->ukc", 1e-5 * Ga * E * (ha + hh.abs() * za / t) / t + dG * hh.abs() * E / t, Zd.abs())
    return out


def dense_autograd64(Z, H, t, pos, ign=None, pos_weight=None):
    """The dense formulation under CPU torch autograd in fp64: the masked, weighted F.binary_cross_entropy_with_logits over
    the upper triangle -> (loss, dZ, dH)."""
    Zt = Z.detach().double().cpu().requires_grad_(True)
    Ht = H.detach().double().cpu().requires_grad_(True)
    N = Zt.shape[0]
    inc, y, W, _counts, _pw, _w = _sets(N, pos, ign, pos_weight)
    up = torch.triu(torch.ones(N, N, dtype=torch.bool), 1)
    if not bool((inc & up).any()):
        return 0.0, torch.zeros_like(Zt), torch.zeros_like(Ht)
    logit = (torch.einsum("ukd,vkd->kuv", Ht, Ht) * torch.exp(torch.einsum("ukd,vkd->kuv", Zt, Zt) / t)).sum(0)
    loss = F.binary_cross_entropy_with_logits(logit, (y & up).double(), weight=W * up, reduction="sum")
    loss.backward()
    return float(loss.detach()), Zt.grad, Ht.grad


def saturated_tables(N, K, d, t, target=60.0):
    """recon_ref's tables for (N, K, d) with H multiplied by sqrt(target / max |s|), the maximum over the pairs included under
    pair_sets(N, seed=N): the largest included |logit| in fp64 becomes ``target``.  Z is untouched, so no exp overflows."""
    Z, H = recon_ref.tables_cpu(N, K, d, recon_ref.table_seed(N, K, d))
    pos, ign = recon_ref.pair_sets(N, seed=N)
    inc = ~ign & ~torch.eye(N, dtype=torch.bool)
    s = logits64(Z, H, t)[0]
    return Z, H * float(target / s[inc].abs().max()) ** 0.5, pos, ign


# The conditions the saturated inputs are held to before anything is compared: at least 5 % of the included pairs above 16.64
# and at least 10 included positives below -27.6.  Evaluated in fp64 on the CPU the construction above gives, over the 16
# combinations of the GPU test, a smallest share of 5.4 % (N = 300, (1, 8), t = 1) and at least 10 such positives everywhere
# EXCEPT at N = 129, (K, d) = (1, 8), whose 129 nodes and single factor hold 4 (t = 1) and 2 (t = 2) of them: that shape cannot
# reach 10 at |logit| <= 60 and is held to the count it has (at least one, so the regime is still exercised there); every
# other combination is held to 10.  The band checks are the same on all 16.
MIN_SHARE_ABOVE = 0.05


def min_positives_below(N, K, d):
    return 1 if (N, K, d) == (129, 1, 8) else 10


def saturation(ref):
    """(share of included pairs with logit > 16.64, included positives with logit < -27.6) of a recon_logits64 result."""
    s, inc, y = ref["logit"], ref["included"], ref["label"]
    up = torch.triu(torch.ones_like(inc), 1)
    n = int((inc & up).sum())
    return (int((inc & up & (s > SIGMOID_ONE)).sum()) / n if n else 0.0), int((y & up & (s < CLAMP_BELOW)).sum())


# ---- the module-level check (Disentangle.forward_recon_logits_loss / forward_logits against autograd of the oracle)
def module_reference(g, dtype=torch.float64):
    """CPU autograd of oracle.dense_ref.project -> route_aggregate -> x = sum_k (H_k H_k^T) o e_k under the masked, weighted
    F.binary_cross_entropy_with_logits over the upper triangle, for a golden case ``g``; sets and weights are
    recon_ref.module_reference's -> (loss, {parameter: gradient}, ign, (n_pos, n_neg), largest |logit| among included pairs)."""
    m = g["meta"]
    N = m["N"]
    adj = torch.from_numpy(g["adj"])
    pos = (adj != 0) | (adj.t() != 0)
    _p, ign = recon_ref.pair_sets(N, seed=N)
    inc = torch.triu(~ign, diagonal=1)
    y = (pos & inc).to(dtype)
    n_pos = int(y.sum())
    n_neg = int(inc.sum()) - n_pos
    weight = torch.where(y > 0, torch.tensor(n_neg / n_pos / (n_pos + n_neg), dtype=dtype),
                         torch.tensor(1.0 / (n_pos + n_neg), dtype=dtype)) * inc
    sd = {k[4:]: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in g.items() if k.startswith("sd__")}
    logit = module_logits(g, sd, dtype)
    loss = F.binary_cross_entropy_with_logits(logit, y, weight=weight, reduction="sum")
    loss.backward()
    return (float(loss.detach()), {k: v.grad.double() for k, v in sd.items()}, ign, (n_pos, n_neg),
            float(logit.detach()[inc].abs().max()))


def module_logits(g, sd, dtype):
    """The oracle's dense forward up to the logits: dense_ref.forward without its sigmoid, from the same functions."""
    from oracle import dense_ref
    m = g["meta"]
    x, adj = torch.from_numpy(g["x"]).to(dtype), torch.from_numpy(g["adj"]).to(dtype)
    Z = dense_ref.project(x, sd)                                          # [K,N,d]
    H, e, _att, _p, _s = dense_ref.route_aggregate(Z, adj, m["beta"], m["t"])
    return (torch.bmm(H, H.transpose(1, 2)) * e).sum(dim=0)                # x = sum_k (H_k H_k^T) o e_k
