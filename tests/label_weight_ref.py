"""Labels and weights the pair-list objective is never otherwise run on — soft and smoothed labels, negative weights, weights of
-0.0, weights over thirty binades — and what float64 says of the training step on them, in both score spaces, on the graph and the
pair list of tests/ref64.py.  TEST INFRASTRUCTURE: torch, CPU; on top of ref64 and logit_ref, which take any (y, w) as they are.

Recipes.  Each is a deterministic function of (the binary / positive draw it starts from, a seed) and returns fp32 CPU tensors:

  labels   binary    the existing draw (ref64.reference: rng.random(P) < 0.3; logit_ref.bce_inputs: < 0.4)
           smoothed  the binary draw mapped to {0.05, 0.95}
           soft      uniform fp32 strictly inside (0, 1), with P // 16 pairs set to exactly 0 and P // 16 to exactly 1
           half      0.5 everywhere
  weights  positive  the existing draw ([0.2, 1] / 64, an eighth of them +0.0)
           signed    the existing magnitudes, a third of the live ones negated; the zeros split evenly into +0.0 and -0.0
           negzero   the existing draw with every zero written as -0.0 — nothing else changes
           wide      2^u, u uniform in [-20, 10], positive, no zeros

COMBOS are the four pairings every test runs.

Reference.  Logit space: logit_ref.step64 / step32, unchanged.  Probability space: the rule of ref64.reference's dZ_train —
g = w (p32 - y) / clamp(p32 (1 - p32), 1e-12) at the fp32 probability of the fp64 logit, then ref64.score_bwd64 — and `prob_step32`,
its restatement in fp32 in the form of logit_ref.step32 (the one-pass kernels' coefficient w (p - y) (r >= 1e-12 ? 1 : r 1e12)).

A loss kernel is judged on the scores it is HANDED (`prob_loss_terms64`, `prob_g64`, logit_ref.pair_loss64 / g64 at the fp32 scores
as float64): in probability space log(1 - p) turns one rounding of a probability next to 1 into an error of 0.7 of that pair's term,
which is the forward's error and is held by the forward's band, not the loss kernel's.

Measures.  Per-pair g: logit_ref.g_ratio.  dZ / dH: ref64.row_ratio's formula with the row scales taken from the fp64 gradient of
the same inputs under |w| (`row_ratio`): pairs of opposite sign cancel, and a row that cancels must not be judged against what is
left of it.  With no negative weight that IS ref64.row_ratio.  Loss: |got - ref| / sum |w| |term| (`loss_err`): under `signed` the
loss itself can be near 0.

FP32 holds the largest error the fp32 restatements show against fp64, over `b1_cases` x COMBOS and logit_ref.cases x (soft, signed)
for the step, over logit_ref.BCE_SIZES x COMBOS for the loss kernels — measured again on every run by tests/test_label_weight_cpu.py
within ref64.CPU_SLACK.  BOUND is 4x that (ref64's rule and its reason: another equally valid fp32 summation order and a hardware
exp).  Nothing here was set from what a kernel returns.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import logit_ref
import ref64

F64 = torch.float64
LABELS = ("binary", "smoothed", "soft", "half")
WEIGHTS = ("positive", "signed", "negzero", "wide")
COMBOS = (("smoothed", "positive"), ("soft", "signed"), ("binary", "negzero"), ("half", "wide"))
B1_SHAPES = ((8, 64, "f32"), (4, 64, "f32"),                      # wave per entry
             (16, 128, "f32"), (16, 128, "bf16"),                  # wide rows
             (5, 32, "f32"), (8, 32, "bf16"))                      # group per entry
SPACES = ("prob", "logit")

# Largest error of the fp32 restatements against fp64, as measured (three significant digits).  "prob" / "logit": the step in that
# score space (dZ, dH: row_ratio; loss: loss_err; g: logit_ref.g_ratio, the last two at the restatement's own fp32 scores);
# "prob_kernel" / "logit_kernel": the loss kernels' formulas on the inputs of `bce_case`.
# The two logit-space g figures are large because they are RELATIVE figures of w (sigma(x) - y) under soft labels: where a drawn
# label happens to lie next to sigma(x), s ((1 - y) - y e) cancels and keeps the fma's rounding relative to the larger term, as
# sigmoid_minus_label's comment says (dl_common.h); each is set by the one pair whose label lies closest to its sigma(x).  The
# probability form subtracts two fp32 numbers of which one is the handed score, exactly, and shows none of it.
FP32 = {
    "prob": {"dZ": 4.29e-6, "dH": 5.66e-6, "loss": 9.98e-8, "g": 2.33e-7},       # f32 K16 d128 t1 (half, wide) twice / f32 K4 d64 t2 / bf16 K5 d64 t1
    "logit": {"dZ": 1.12e-6, "dH": 1.18e-6, "loss": 1.01e-7, "g": 2.60e-2},      # f32 K5 d32 t1 / t2 / bf16 K16 d128 t2 / bf16 K4 d32 t2 (soft, signed)
    "prob_kernel": {"loss": 5.80e-8, "g": 1.80e-7},                              # 1 pair / 1,024 pairs
    "logit_kernel": {"loss": 7.88e-8, "g": 4.51e-5},                             # 1,023 pairs / 10,004 pairs (soft, signed)
}
BOUND = {k: {m: 4.0 * v for m, v in d.items()} for k, d in FP32.items()}


def combo_id(combo) -> str:
    return f"{combo[0]}-{combo[1]}"


# -------------------------------------------------------------------------------------------------- the recipes
def _rng(seed: int, what: str):
    return np.random.default_rng([int(seed), LABELS.index(what) if what in LABELS else 16 + WEIGHTS.index(what)])


def make_labels(name: str, binary: torch.Tensor, seed: int) -> torch.Tensor:
    """The label recipe `name` over a binary draw (fp32 0 / 1) -> fp32 labels."""
    b = binary.float()
    n = b.numel()
    if name == "binary":
        return b.clone()
    if name == "smoothed":
        return torch.where(b > 0.5, torch.tensor(0.95), torch.tensor(0.05))
    if name == "half":
        return torch.full((n,), 0.5)
    assert name == "soft", name
    rng = _rng(seed, name)
    y = np.clip(rng.random(n, dtype=np.float32), np.float32(2.0 ** -24), np.float32(1 - 2.0 ** -24))
    ends = rng.permutation(n)[:2 * (n // 16)]
    y[ends[:n // 16]], y[ends[n // 16:]] = 0.0, 1.0
    return torch.from_numpy(y)


def make_weights(name: str, positive: torch.Tensor, seed: int) -> torch.Tensor:
    """The weight recipe `name` over a positive draw (fp32, some of them +0.0) -> fp32 weights."""
    w = positive.float().clone()
    n = w.numel()
    if name == "positive":
        return w
    zeros = torch.nonzero(w == 0)[:, 0]
    if name == "negzero":
        w[zeros] = -0.0
        return w
    rng = _rng(seed, name)
    if name == "wide":
        return torch.from_numpy((2.0 ** rng.uniform(-20.0, 10.0, n)).astype(np.float32))
    assert name == "signed", name
    live = torch.nonzero(w != 0)[:, 0].numpy()
    neg = torch.from_numpy(rng.choice(live, live.size // 3, replace=False)) if live.size >= 3 else torch.zeros(0, dtype=torch.long)
    w[neg] = -w[neg]
    w[zeros[torch.from_numpy(rng.permutation(zeros.numel()))[:zeros.numel() // 2]]] = -0.0
    return w


def base_draw(P: int, seed: int):
    """ref64.reference's own (label, weight) draw, as a function of (P, seed): its generator hands out g_prob first."""
    rng = np.random.default_rng(seed)
    rng.standard_normal(P)
    label = torch.from_numpy((rng.random(P) < 0.3).astype(np.float32))
    weight = torch.from_numpy((rng.uniform(0.2, 1.0, P) / 64).astype(np.float32))
    weight[torch.from_numpy(rng.choice(P, P // 8, replace=False))] = 0.0
    return label, weight


def labels_weights(combo, P: int, seed: int):
    """-> (y, w) fp32 [P] of one combination over the pair list of ref64.structure()."""
    y0, w0 = base_draw(P, seed)
    return make_labels(combo[0], y0, seed), make_weights(combo[1], w0, seed)


def bce_case(n: int, combo):
    """-> (x, y, w) fp32 [n]: the logits of logit_ref.bce_inputs(n), its labels and weights put through the combination."""
    x, y0, w0 = logit_ref.bce_inputs(n)
    return x, make_labels(combo[0], y0, 1000 + n), make_weights(combo[1], w0, 1000 + n)


def sigmoid32(x32: torch.Tensor) -> torch.Tensor:
    """1 / (1 + exp(-x)) in fp32: exactly 1 from 24 ln 2 on, exactly 0 once exp(-x) overflows."""
    x32 = x32.float()
    return 1.0 / (1.0 + torch.exp(-x32))


def loss_kernel_inputs(space, n, combo):
    """What the loss kernel of `space` is handed at size n: bce_case's logits, or their fp32 sigmoids — with the probability of
    the most negative logit written as exactly 0 (what a logit below -88.7 gives; the draw stops at -60), exact 1s being there
    from 24 ln 2 on."""
    x, y, w = bce_case(n, combo)
    if space == "logit":
        return x, y, w
    p = sigmoid32(x)
    if n >= 8:
        p[int(torch.argmin(x))] = 0.0
    return p, y, w


# -------------------------------------------------------------------------------------------------- probability space
def prob_loss_terms64(p, y):
    """[P] -(y clamp(log p, -100) + (1 - y) clamp(log(1 - p), -100)) in fp64 at the probabilities handed in (>= 0 everywhere)."""
    p, y = p.double(), y.double()
    return -(y * torch.log(p).clamp(min=-100.0) + (1 - y) * torch.log(1 - p).clamp(min=-100.0))


def prob_g64(p, y, w):
    """[P] d loss / d prob = w (p - y) / clamp(p (1 - p), 1e-12) in fp64 at the probabilities handed in; weight +-0 = exactly 0."""
    p, y, w = p.double(), y.double(), w.double()
    return torch.where(w == 0, torch.zeros_like(w), w * (p - y) / torch.clamp(p * (1 - p), min=1e-12))


def prob_step64(Z, H, pu, pv, t, y, w):
    """-> x, p32, g, dZ, dH: ref64.reference's dZ_train rule on any (y, w): the coefficient at the fp32 probability of the fp64
    logit (its p (1 - p) formed in fp32, as there), then ref64.score_bwd64."""
    y, w = y.double(), w.double()
    x = ref64.logit64(Z, H, pu, pv, t)
    p32 = ref64.sigmoid32(x)
    r32 = (p32.float() * (1 - p32.float())).double()
    g = torch.where(w == 0, torch.zeros_like(w), w * (p32 - y) / torch.clamp(r32, min=1e-12))
    dZ, dH = ref64.score_bwd64(Z, H, pu, pv, t, g, p32)
    return x, p32, g, dZ, dH


def bce_prob32(p, y, w):
    """-> (loss, g) of dl_pair_bce's formulas in fp32, summed by torch: w -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)) and
    w (p - y) / max(p (1 - p), 1e-12); weight +-0 = exactly nothing."""
    p, y, w = p.float(), y.float(), w.float()
    per = w * -(y * torch.log(p).clamp(min=-100.0) + (1.0 - y) * torch.log(1.0 - p).clamp(min=-100.0))
    g = w * (p - y) / torch.clamp(p * (1.0 - p), min=1e-12)
    dead = w == 0
    return torch.where(dead, torch.zeros_like(per), per).sum(), torch.where(dead, torch.zeros_like(g), g)


def prob_step32(Z, H, pu, pv, t, y, w):
    """prob_step64 restated in fp32 on the CPU in the form of logit_ref.step32: fp32 logits, the fp32 sigmoid, the one-pass
    kernels' coefficient w (p - y) (r >= 1e-12 ? 1 : r 1e12) with r = p (1 - p), gradients by fp32 autograd on ONE thread
    -> x, p, loss, g (bce_prob32 at that p), dZ, dH."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        y, w = y.float(), w.float()
        Zr, Hr = Z.float().requires_grad_(True), H.float().requires_grad_(True)
        x = ref64.logit64(Zr, Hr, pu, pv, float(t))
        p = sigmoid32(x.detach())
        r = p * (1.0 - p)
        gl = w * (p - y) * torch.where(r >= 1e-12, torch.ones_like(r), r * 1e12)
        gl = torch.where(w == 0, torch.zeros_like(gl), gl)
        dZ, dH = torch.autograd.grad(x, (Zr, Hr), gl)
        loss, g = bce_prob32(p, y, w)
    finally:
        torch.set_num_threads(threads)
    return x.detach(), p, loss, g, dZ, dH


# -------------------------------------------------------------------------------------------------- the measures
def row_ratio(got, ref, scale_ref) -> float:
    """ref64.row_ratio with the row scales of another tensor: err_i = max |got_i - ref_i|, scale_i = max(max |scale_ref_i|, the
    median over the non-zero rows of max |scale_ref_j|).  scale_ref = the fp64 gradient under |w|."""
    got, ref, scale_ref = (torch.as_tensor(v).double() for v in (got, ref, scale_ref))
    n = ref.shape[0]
    err = (got - ref).abs().reshape(n, -1).max(1).values
    mag = scale_ref.abs().reshape(n, -1).max(1).values
    nz = mag[mag > 0]
    if nz.numel() == 0:
        return 0.0 if float(err.max()) == 0 else float("inf")
    return float((err / torch.maximum(mag, nz.median())).max())


def loss_err(got, terms64, w) -> float:
    """|got - sum w term| / sum |w| |term|, fp64; terms of weight +-0 are no part of either sum."""
    terms64, w = terms64.double(), torch.as_tensor(w).double()
    live = w != 0
    ref, den = float((w[live] * terms64[live]).sum()), float((w[live].abs() * terms64[live].abs()).sum())
    err = abs(float(got) - ref)
    return err / den if den > 0 else (0.0 if err == 0 else float("inf"))


def loss_kernel_figures(space: str, score32, y, w, loss, g):
    """{"loss", "g"}: a loss kernel's (loss, g) — or a restatement's — against fp64 at the fp32 scores it was handed."""
    s64 = score32.double()
    if space == "prob":
        terms, g_ref = prob_loss_terms64(s64, y), prob_g64(s64, y, w)
    else:
        terms = (1 - y.double()) * logit_ref.softplus64(s64) + y.double() * logit_ref.softplus64(-s64)
        g_ref = logit_ref.g64(s64, y.double(), w.double())
    return {"loss": loss_err(loss, terms, w), "g": logit_ref.g_ratio(g, g_ref, w)}


# -------------------------------------------------------------------------------------------------- cases and references
def b1_cases(lib):
    """The cases of logit_ref.cases(lib) at B1_SHAPES: one shape per kernel family and table type, each at t = 1 and t = 2."""
    out = [c for c in logit_ref.cases(lib) if (c.K, c.d, c.dtype) in B1_SHAPES]
    assert {(c.K, c.d, c.dtype, c.t) for c in out} == {s + (t,) for s in B1_SHAPES for t in logit_ref.STEP_TEMPERATURES}, out
    return out


@functools.lru_cache(maxsize=8)
def reference(K: int, d: int, dtype: str, t: float, beta: float, combo):
    """ref64.reference's tables for the case with the labels and weights of `combo`, and the step in both score spaces:
    r[space] = dict(dZ, dH, dZ_abs, dH_abs (under |w|), and the restatement's score32, loss32, g32, dZ32, dH32); r["x"], r["x_abs"],
    r["p32"] of the fp64 logits; r["y"], r["w"] as fp32."""
    st = ref64.structure()
    base = ref64.reference(K, d, dtype, t, beta)
    Z, H = base["Z"], base["H_in"]
    P = st.pu.numel()
    y, w = labels_weights(combo, P, base["seed"])
    y64, w64 = y.double(), w.double()
    out = dict(Z=Z, H_in=H, y=y, w=w, x=base["logit"], x_abs=base["logit_abs"], seed=base["seed"])
    x, _loss, _g, dZ, dH = logit_ref.step64(Z, H, st.pu, st.pv, t, y64, w64)
    assert torch.equal(x, base["logit"])
    _x, _l, _g, dZa, dHa = logit_ref.step64(Z, H, st.pu, st.pv, t, y64, w64.abs())
    x32, loss32, g32, dZ32, dH32 = logit_ref.step32(Z, H, st.pu, st.pv, t, y64, w64)
    out["logit"] = dict(dZ=dZ, dH=dH, dZ_abs=dZa, dH_abs=dHa, score32=x32, loss32=loss32, g32=g32, dZ32=dZ32, dH32=dH32)
    _x, p32, _g, dZ, dH = prob_step64(Z, H, st.pu, st.pv, t, y64, w64)
    _x, _p, _g, dZa, dHa = prob_step64(Z, H, st.pu, st.pv, t, y64, w64.abs())
    _x32, p, loss32, g32, dZ32, dH32 = prob_step32(Z, H, st.pu, st.pv, t, y64, w64)
    out["prob"] = dict(dZ=dZ, dH=dH, dZ_abs=dZa, dH_abs=dHa, score32=p, loss32=loss32, g32=g32, dZ32=dZ32, dH32=dH32)
    out["p32"] = p32
    return out


def step_figures(r, space: str, dZ, dH, score32=None, loss=None, g=None):
    """{"dZ", "dH"[, "loss", "g"]} of one evaluation of the step (a kernel's, or the restatement's) against r = reference(...)."""
    s = r[space]
    fig = {"dZ": row_ratio(dZ, s["dZ"], s["dZ_abs"]), "dH": row_ratio(dH, s["dH"], s["dH_abs"])}
    if score32 is not None:
        fig.update(loss_kernel_figures(space, score32, r["y"], r["w"], loss, g))
    return fig


def restatement_figures(r, space: str):
    s = r[space]
    return step_figures(r, space, s["dZ32"], s["dH32"], s["score32"], s["loss32"], s["g32"])
