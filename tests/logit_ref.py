"""The pair-list objective in LOGIT space, in plain float64, on the inputs of tests/ref64.py.  TEST INFRASTRUCTURE: torch, CPU.

  logit   x(u, v) = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t)                                  (ref64.logit64)
  loss    sum_q w[q] ((1 - y) softplus(x) + y softplus(-x))  =  sum_q w[q] (max(x, 0) - x y + log1p(exp(-|x|)))
  g       d loss / d x[q] = w[q] (sigma(x) - y)

The loss is written with torch.nn.functional.softplus (fp64; its linear shortcut moved out of reach, see `softplus64`) on BOTH
sides, (1 - y) softplus(x) + y softplus(-x), so that autograd forms sigma(x) - y as (1 - y) sigma(x) - y sigma(-x): each side
to fp64 precision of its own size.  `softplus(x) - x y` would be the same loss, but its autograd gradient is sigma(x) + (-y), and
for y = 1, x = 35 that is 1 - 6e-16 - 1 in fp64: nothing left to hold a kernel against.  There is no hand-derived backward: dZ and dH
are torch.autograd of that loss through ref64.logit64.

`step32` restates the same step in fp32 (torch on the CPU: fp32 tables, fp32 logits, the fp32 form of sigma(x) - y the kernels
use, gradients by fp32 autograd) — another valid fp32 evaluation.  Its error against fp64 on `cases(lib)` is recorded in FP32,
measured again on every run by tests/test_pair_logits_cpu.py within ref64.CPU_SLACK; the GPU bounds are 4x those figures
(ref64's rule and its reason: another equally valid fp32 summation order and a hardware exp).  Nothing here was set from what
the kernels give.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import ref64
from ref64 import band_ratio, hotpath_cases, logit64, row_ratio, structure    # noqa: F401  (the measures and inputs of the GPU test)

F64 = torch.float64
GENERIC_SHAPE = (3, 16)                                           # one shape without a tuned kernel
STEP_TEMPERATURES = (1.0, 2.0)                                    # t == 1 is a code path of its own in the tuned kernels

# Largest error of `step32` against fp64 over `cases(lib)`, as measured (three significant digits): the gradients as
# ref64.row_ratio, the loss and the per-pair loss gradient relative (see `rel_err` / `g_ratio`).  "loss_kernel" and "g" are those
# of `bce32` on the loss-kernel inputs of `bce_inputs`.
FP32 = {
    "dZ": 1.00e-6, "dH": 7.86e-7, "loss": 2.13e-7,               # bf16 K16 d128 t1 / f32 K5 d32 t1 / the generic shape at t1
    "loss_kernel": 7.88e-8, "g": 1.80e-7,                        # 1,023 pairs
}
BOUND = {k: 4.0 * v for k, v in FP32.items()}

Case = namedtuple("Case", "K d dtype t beta generic")


def case_id(c: Case) -> str:
    return f"{c.dtype}-K{c.K}-d{c.d}-t{c.t:g}" + ("-generic" if c.generic else "")


def cases(lib):
    """Every tuned shape of ref64.hotpath_cases in both table types (with the beta that case list gives it) and one generic
    shape (K = 3, d = 16, on the generic kernels), each at t = 1 and t = 2."""
    out, seen = [], set()
    for c in ref64.hotpath_cases(lib):
        if c.generic or (c.K, c.d) in ref64.UNTUNED or (c.K, c.d, c.dtype) in seen:
            continue
        seen.add((c.K, c.d, c.dtype))
        out += [Case(c.K, c.d, c.dtype, t, c.beta, False) for t in STEP_TEMPERATURES]
    out += [Case(*GENERIC_SHAPE, "f32", t, ref64.BETAS[0], True) for t in STEP_TEMPERATURES]
    return out


def softplus64(x):
    """log(1 + exp(x)) by F.softplus in fp64, with its `x > threshold -> x` shortcut raised from 20 (an error of exp(-20) = 2e-9
    there) to 700: below that exp(x) is finite in fp64 and log1p(exp(x)) is exact to rounding, above it the shortcut is (its
    error is exp(-700))."""
    assert x.dtype == F64
    return F.softplus(x, beta=1.0, threshold=700.0)


def pair_loss64(x, y, w):
    """[P] per-pair loss w ((1 - y) softplus(x) + y softplus(-x)); weight 0 = exactly nothing."""
    return w * ((1 - y) * softplus64(x) + y * softplus64(-x))


def g64(x, y, w):
    """w (sigma(x) - y) with both sides of the sigmoid kept: (1 - y) sigma(x) - y sigma(-x)."""
    return w * ((1 - y) * torch.sigmoid(x) - y * torch.sigmoid(-x))


def step64(Z, H, pu, pv, t, y, w):
    """-> x [P], loss, g [P], dZ, dH of the logit-space training step (autograd of the softplus loss through logit64)."""
    Zr, Hr = Z.detach().clone().requires_grad_(True), H.detach().clone().requires_grad_(True)
    x = logit64(Zr, Hr, pu, pv, t)
    xg = x.detach().clone().requires_grad_(True)
    loss = pair_loss64(xg, y, w).sum()
    (g,) = torch.autograd.grad(loss, xg)
    dZ, dH = torch.autograd.grad(x, (Zr, Hr), g)
    return x.detach(), loss.detach(), g, dZ, dH


# ---- the same step in fp32
def sigmoid_minus_label32(x, y):
    """The kernels' form in fp32: e = exp(-|x|), s = 1 / (1 + e), sigma(|x|) = s, sigma(-|x|) = e s, and
    (1 - y) sigma(x) - y sigma(-x) = s ((1 - y) - y e) for x >= 0, s ((1 - y) e - y) for x < 0."""
    e = torch.exp(-x.abs())
    s = 1.0 / (1.0 + e)
    pos = x >= 0
    a, b = 1.0 - y, -y
    return s * (torch.where(pos, b, a) * e + torch.where(pos, a, b))


def bce32(x, y, w):
    """-> (loss, g) of the loss kernel's formulas in fp32: per pair w ((1 - y) max(x, 0) + y max(-x, 0) + log1p(exp(-|x|))), summed
    in fp32 by torch; g = w (sigma(x) - y) by sigmoid_minus_label32."""
    x, y, w = x.float(), y.float(), w.float()
    per = w * ((1.0 - y) * x.clamp(min=0) + y * (-x).clamp(min=0) + torch.log1p(torch.exp(-x.abs())))
    return per.sum(), w * sigmoid_minus_label32(x, y)


def step32(Z, H, pu, pv, t, y, w):
    """step64 restated in fp32 on the CPU: fp32 logits (ref64.logit64 on fp32 tensors), bce32, gradients by fp32 autograd — on
    ONE thread: the backward of a gather adds rows in whatever order the threads arrive, and a recorded figure wants one order."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        Zr, Hr = Z.float().requires_grad_(True), H.float().requires_grad_(True)
        x = logit64(Zr, Hr, pu, pv, float(t))
        loss, g = bce32(x.detach(), y, w)
        dZ, dH = torch.autograd.grad(x, (Zr, Hr), g)
    finally:
        torch.set_num_threads(threads)
    return x.detach(), loss, g, dZ, dH


# ---- the measures
def rel_err(got, ref) -> float:
    return abs(float(got) - float(ref)) / abs(float(ref))


def g_ratio(got, ref, w) -> float:
    """Per-pair loss gradient: max |got - ref| / max(|ref|, 2^-24 w).  w (sigma(x) - y) is held RELATIVE to its own size — that is
    the point of the logit-space form — down to where the logit handed in (an fp32 number) stops mattering: the floor is one fp32
    rounding of the weight."""
    got, ref, w = torch.as_tensor(got).double(), torch.as_tensor(ref).double(), torch.as_tensor(w).double()
    live = w != 0
    if bool(((got != 0) & ~live).any()):
        return math.inf
    den = torch.maximum(ref.abs(), ref64.U * w.abs())[live]
    return float(((got - ref).abs()[live] / den).max()) if den.numel() else 0.0


@functools.lru_cache(maxsize=4)
def reference(K: int, d: int, dtype: str, t: float, beta: float):
    """ref64.reference's tables, H input, labels and weights for the case, and what the logit-space step says of them in fp64
    (keys x, x_abs, loss, g, dZ, dH) and in fp32 (x32, loss32, g32, dZ32, dH32).  The tables are the rounded tables (bf16 cases:
    rounded to bf16), as in ref64.reference."""
    st = ref64.structure()
    r = ref64.reference(K, d, dtype, t, beta)
    Z, H, y, w = r["Z"], r["H_in"], r["label"], r["weight"]
    x, loss, g, dZ, dH = step64(Z, H, st.pu, st.pv, t, y, w)
    assert torch.equal(x, r["logit"])
    x32, loss32, g32, dZ32, dH32 = step32(Z, H, st.pu, st.pv, t, y, w)
    return dict(Z=Z, H_in=H, label=y, weight=w, x=x, x_abs=r["logit_abs"], loss=loss, g=g, dZ=dZ, dH=dH,
                x32=x32, loss32=loss32, g32=g32, dZ32=dZ32, dH32=dH32)


# ---- the loss kernel's inputs
BCE_SIZES = (1, 1023, 1024, 1025, 10004)                          # around the 1,024 partial sums


def bce_inputs(n: int, seed: int = 0):
    """fp32 logits over [-60, 60] (a third of them within [-10, 10]; none at 0), binary labels, weights in [0.2, 1] / 64 with an
    eighth of them 0 — as CPU tensors (x, y, w)."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    x = np.where(rng.random(n) < 1 / 3, rng.uniform(-10, 10, n), rng.uniform(-60, 60, n)).astype(np.float32)
    x[x == 0] = 0.5
    y = (rng.random(n) < 0.4).astype(np.float32)
    w = (rng.uniform(0.2, 1.0, n) / 64).astype(np.float32)
    if n >= 8:
        w[rng.choice(n, n // 8, replace=False)] = 0.0
    return torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(w)


# ---- the saturated list (why the feature exists)
SAT_LO, SAT_HI = 20.0, 200.0
P_ONE_SAFE, P_ZERO_SAFE = 17.5, -90.0     # fp32 sigmoid: exactly 1 from 24 ln 2 = 16.64 on, exactly 0 once exp(-x) overflows (x < -88.73)


@functools.lru_cache(maxsize=1)
def saturated(K: int = 8, d: int = 64, t: float = 1.0, beta: float = 0.6):
    """ref64's tables at (K, d) with H scaled by c (the logit is bilinear in H: x -> c^2 x; Z and with it every exp argument stay
    as they are, below 80), c^2 = 40, 80, 160, ... until the fp64 reference alone puts at least a third of the listed pairs at
    |logit| in [20, 200] AND at least 8 nodes have all their pairs dead in probability space.
    A pair is DEAD in probability space where its fp32 probability is exactly 1 or exactly 0 (x >= 17.5, x <= -90 with a margin
    for the fp32 logit): p (1 - p) = 0 and the one-pass scorer's gradient coefficient is exactly 0.  (A negative logit in
    (-88.7, -20) is saturated — its loss is clamped, its gradient scaled down by p (1 - p) 1e12 below x = -27.6 — but its gradient
    is not exactly 0, so it does not count as dead.)
    Labels: of the pairs with |logit| in [20, 200] every second one (in list order) is WRONG — a negative scored above 20, a positive
    scored below -20 —, every other pair has the label of its sign.  Weights 1 / P, none 0.
    -> dict(Z, H_in, x, x_abs, label, weight, sat, wrong, dead, c2, arg_max): `sat` = the pairs in [20, 200], `dead` = the nodes with
    at least one pair whose pairs are all dead."""
    st = ref64.structure()
    r = ref64.reference(K, d, "f32", t, beta)
    pu, pv = st.pu.long(), st.pv.long()
    P, N = pu.numel(), ref64.N_NODES
    Z = r["Z"]
    arg = float((Z[pu] * Z[pv]).sum(-1).abs().max()) / t
    count = lambda mask: torch.zeros(N, dtype=torch.long).index_add_(0, pu[mask], torch.ones(int(mask.sum()), dtype=torch.long)) \
        .index_add_(0, pv[mask], torch.ones(int(mask.sum()), dtype=torch.long))
    for c2 in (40.0, 80.0, 160.0, 320.0, 640.0):
        H = (r["H_in"] * math.sqrt(c2)).float().double()
        x = logit64(Z, H, pu, pv, t)
        sat = (x.abs() >= SAT_LO) & (x.abs() <= SAT_HI)
        dead_pair = (x >= P_ONE_SAFE) | (x <= P_ZERO_SAFE)
        dead = torch.nonzero((count(torch.ones(P, dtype=torch.bool)) > 0) & (count(~dead_pair) == 0))[:, 0]
        if int(sat.sum()) * 3 >= P and dead.numel() >= 8:
            break
    else:
        raise AssertionError("no scale of H puts a third of the pairs at |logit| in [20, 200] with 8 dead nodes")
    label = (x > 0).double()
    wrong = torch.nonzero(sat)[:, 0][::2]
    label[wrong] = 1.0 - label[wrong]
    weight = torch.full((P,), 1.0 / P, dtype=torch.float32).double()
    return dict(Z=Z, H_in=H, x=x, x_abs=ref64.logit_abs64(Z, H, pu, pv, t), label=label, weight=weight, sat=sat, wrong=wrong,
                dead=dead, c2=c2, arg_max=arg)
