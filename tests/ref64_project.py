"""Plain float64 reference of the factor projection (model.py:13-15, 24-27: Factor / Factor2 fanned out over K factors),
the inputs it is run on and the list of cases that reaches every compiled form of the projection kernels.
TEST INFRASTRUCTURE: torch, float64, CPU.  The sibling of tests/ref64.py (the sparse hot path) for the dense part.

  two-layer    pre[n,k,h] = sum_f x[n,f] W1[k,h,f] + b1[k,h]        hid = relu(pre)
               Z[n,k,c]   = sum_h hid[n,k,h] W2[k,c,h] + b2[k,c]
               dhid = (sum_c dZ[n,k,c] W2[k,c,h]) [pre > 0]
               dW1 = sum_n dhid x,  db1 = sum_n dhid,  dW2 = sum_n dZ hid,  db2 = sum_n dZ
  one layer    Z = x W^T + b (W2 = None),  dW = sum_n dZ x,  db = sum_n dZ

Every output has an "absolute-sum companion" (ref64.py's term): the same sums over magnitudes, the error of a stage
carried into the next —

  pre_abs = sum_f |x| |W1| + |b1|
  Z_abs   = sum_h pre_abs [pre > 0] |W2| + |b2|          (hid <= pre_abs: covers layer 2's own sum and hid's error)
  dhid_abs = (sum_c |dZ| |W2|) [pre > 0]
  dW1_abs = sum_n dhid_abs |x|,  db1_abs = sum_n dhid_abs,  dW2_abs = sum_n |dZ| pre_abs [pre > 0],  db2_abs = sum_n |dZ|

— and is judged per element by ref64.band_ratio: |got - ref| / (2^-24 companion).

ORACLE holds the largest such ratio a plain fp32 evaluation (fp32_evaluation: the same sums on the float32 inputs,
every contraction summed as a tiled kernel sums it, index-ordered within tiles of 128 terms, the tile sums added in order)
shows against this reference over all cases of `cases()`, measured and re-asserted by tests/test_ref64_project_cpu.py.
The gradients of the one long contraction, the node-blocked backward at N = 4229, are recorded under keys of their own
("dW1@N4229", ...), so that they do not set the bound of the small cases.  The bound of a kernel's output is 4x the figure
(another equally valid fp32 summation order, the project's convention) plus, for the forms that form products from three
bf16 planes, the analytic PLANE term below.  The keys live here and not in ref64.ORACLE because tests/test_ref64_cpu.py
holds EVERY key of that table against the sparse oracle.

The three-plane term.  dl_tiles.h: an fp32 operand is split v = hi + mid + lo with hi = bf16(v), mid = bf16(v - hi),
lo = bf16(v - hi - mid), and a product is formed as hi*hi + hi*mid + mid*hi + hi*lo + lo*hi + mid*mid, each exact in the
fp32 accumulator.  bf16 keeps 8 significant bits and rounds to nearest, so |v - hi| <= 2^-8 2^e for 2^e <= |v| < 2^(e+1)
and that remainder is a multiple of 2^(e-23): |mid| <= 2^-8 |v|, and v - hi - mid is at most 2^-8 of the remainder's
binade, i.e. |.| <= 2^-16 |v|, again a multiple of 2^(e-23) — at most 8 significant bits, so lo holds it EXACTLY: three
planes carry every fp32 number in the normal range without truncation (split3_exact below checks this on the inputs of
every case).  What the form loses is the three dropped products: |mid*lo'| + |lo*mid'| + |lo*lo'| <= (2 * 2^-24 + 2^-32)
|v| |v'|.  Per term and product that is PLANE = 2 + 2^-8 units of 2^-24 |v| |v'|, hence of the companion; an output behind
two plane products in a row (Z: layer 1 then layer 2; dW1 of the kept form: dhid then the node contraction) gets two.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import torch

from ref64 import F64, U, band_ratio

# Largest error of the plain fp32 evaluation against this reference over all cases (three significant digits), in units of
# 2^-24 * companion.  tests/test_ref64_project_cpu.py measures them again on every run and holds them within
# ref64.CPU_SLACK on both sides.  Single layer: Z1, dW, db.
ORACLE = {
    "pre": 7.27, "Z": 11.3, "dW1": 18.4, "db1": 9.14, "dW2": 12.4, "db2": 2.43,
    "Z1": 5.54, "dW": 13.3, "db": 1.84,
    "dW1@N4229": 7.84, "db1@N4229": 0.245, "dW2@N4229": 6.50, "db2@N4229": 0.191,     # the node-blocked backward alone
}
PLANE = 2.0 + 2.0 ** -8                 # dropped mid*lo, lo*mid, lo*lo of one three-plane product (derived above)
MASK_MARGIN = 64.0                      # M: every |pre| exceeds M * 2^-24 * pre_abs, well above the bound on pre
MAX_REDRAWS = 4

# plane products between the exactly rounded inputs of a stage and each of its outputs (module docstring; dl_project.hip,
# dl_project_bwd.hip): forward on planes — layer 1, then layer 2 from the split accumulator; backward with a recomputed
# hidden layer — kernel A is fp32 MFMA throughout, only the node contraction of dW1 runs on planes; backward from the
# kept hidden layer — dW2 and dhid (hence db1) on planes, dW1 behind dhid and the node contraction.
PLANE_PRODUCTS = {
    "fwd": {"hid": 1, "Z": 2},
    "recompute": {"dW1": 1, "db1": 0, "dW2": 0, "db2": 0},
    "kept": {"dW1": 2, "db1": 1, "dW2": 1, "db2": 0},
}


LONG_N = 4096                           # from here on the node contraction is "long": ORACLE keys "<gradient>@N4229"
LONG_KEYS = ("dW1", "db1", "dW2", "db2")


def oracle_key(key: str, N: int = 0) -> str:
    key = _JUDGED_BY.get(key, (key,) * 3)[2]
    return key + "@N4229" if (N >= LONG_N and key in LONG_KEYS) else key


def bound(key: str, plane_products: int = 0, N: int = 0) -> float:
    return 4.0 * ORACLE[oracle_key(key, N)] + plane_products * PLANE


# -------------------------------------------------------------------------------------------------- the reference
def forward64(x, W1, b1, W2=None, b2=None):
    """-> dict(pre, hid, Z) in the dtype of the inputs (float64: the reference; float32: the plain fp32 evaluation)."""
    pre = torch.einsum("nf,khf->nkh", x, W1) + b1
    if W2 is None:
        return {"Z": pre}
    hid = pre.clamp_min(0)
    return {"pre": pre, "hid": hid, "Z": torch.einsum("nkh,kdh->nkd", hid, W2) + b2}


def backward64(x, W1, b1, W2, dZ, hid=None):
    """-> dict(dW1, db1, dW2, db2) (one layer: dW, db).  hid given: the kept form (hid > 0 is the mask)."""
    if W2 is None:
        return {"dW": torch.einsum("nkd,nf->kdf", dZ, x), "db": dZ.sum(0)}
    if hid is None:
        hid = (torch.einsum("nf,khf->nkh", x, W1) + b1).clamp_min(0)
    dhid = torch.einsum("nkd,kdh->nkh", dZ, W2) * (hid > 0)
    return {"dW1": torch.einsum("nkh,nf->khf", dhid, x), "db1": dhid.sum(0),
            "dW2": torch.einsum("nkd,nkh->kdh", dZ, hid), "db2": dZ.sum(0)}


def companions64(x, W1, b1, W2, b2, dZ):
    xa, Wa, ga = x.abs(), W1.abs(), dZ.abs()
    pre_abs = torch.einsum("nf,khf->nkh", xa, Wa) + b1.abs()
    if W2 is None:
        return {"Z": pre_abs, "dW": torch.einsum("nkd,nf->kdf", ga, xa), "db": ga.sum(0)}
    on = (torch.einsum("nf,khf->nkh", x, W1) + b1) > 0
    live = pre_abs * on
    dhid_abs = torch.einsum("nkd,kdh->nkh", ga, W2.abs()) * on
    return {"pre": pre_abs, "Z": torch.einsum("nkh,kdh->nkd", live, W2.abs()) + b2.abs(),
            "dW1": torch.einsum("nkh,nf->khf", dhid_abs, xa), "db1": dhid_abs.sum(0),
            "dW2": torch.einsum("nkd,nkh->kdh", ga, live), "db2": ga.sum(0)}


def split3(v32: torch.Tensor):
    """dl_tiles.h:split3 on the CPU: three bf16 planes of an fp32 tensor (as float32 values)."""
    hi = v32.to(torch.bfloat16).float()
    r1 = v32 - hi
    mid = r1.to(torch.bfloat16).float()
    lo = (r1 - mid).to(torch.bfloat16).float()
    return hi, mid, lo


def split3_exact(v32: torch.Tensor) -> bool:
    hi, mid, lo = split3(v32)
    return bool(torch.equal(hi.double() + mid.double() + lo.double(), v32.double()))


# -------------------------------------------------------------------------------------------------- the inputs
POSITIONS = (0, 31, 32, 63, 64, 127, 128)                        # of a tile, plus the last valid index


def marked(n: int):
    """(quiet, loud) row indices among n rows: the tile positions that exist and the last row, alternating."""
    pos = sorted({p for p in POSITIONS if p < n} | {n - 1})
    return pos[0::2], pos[1::2]


def _first_unmarked(n: int):
    used = set(marked(n)[0]) | set(marked(n)[1])
    return next((i for i in range(1, n) if i not in used), None)


def _pow2(gen, n, lo=-2, hi=3):
    return torch.ldexp(torch.ones(n, dtype=F64), torch.randint(lo, hi, (n,), generator=gen))


@functools.lru_cache(maxsize=None)
def reference(N: int, F: int, K: int, nhid: int, d: int):
    """Inputs of one shape (nhid = 0: single layer) and everything the fp64 reference says about them: a dict of CPU
    tensors; x, W1, b1, W2, b2, dZ are float32 (what the kernels are handed, exactly), the rest float64.

    Every value is a normal deviate times a power of two that differs between features (x, W1: per feature; W2: per
    hidden unit; dZ: per output column), rounded to fp32: full 24-bit mantissas, all three bf16 planes populated.
    Rows `marked` quiet / loud are scaled by 2^-12 / 2^+12: node rows of x, hidden units of W1 (and b1), output columns
    of W2 (and b2); one node row of x is all zero and one hidden unit is dead (W1 row 0, b1 < 0: pre < 0 for every node).
    Conditions asserted here (on the reference alone): after at most MAX_REDRAWS passes of redrawing the feature rows of
    the nodes concerned, every |pre| > MASK_MARGIN * 2^-24 * pre_abs — the ReLU mask of ANY fp32 evaluation within the
    bound on pre is the reference's — and everything is finite in fp32."""
    two = nhid > 0
    M = nhid if two else d
    gen = torch.Generator().manual_seed(100003 * N + 1009 * F + 101 * K + 7 * nhid + d)
    sx, sw = _pow2(gen, F), _pow2(gen, F)
    row = torch.ones(N, dtype=F64)
    q, l = marked(N)
    row[q], row[l] = 2.0 ** -12, 2.0 ** 12
    zero_row = _first_unmarked(N)
    if zero_row is not None:
        row[zero_row] = 0.0

    def draw_x(n_rows):
        return torch.randn(n_rows, F, generator=gen, dtype=F64) * sx

    x = (draw_x(N) * row[:, None]).float()
    unit = torch.ones(M, dtype=F64)
    q, l = marked(M)
    unit[q], unit[l] = 2.0 ** -12, 2.0 ** 12
    W1 = torch.randn(K, M, F, generator=gen, dtype=F64) * sw / F ** 0.5 * unit[:, None]
    b1 = torch.randn(K, M, generator=gen, dtype=F64) * 0.5 * unit
    dead = _first_unmarked(M) if two else None
    if dead is not None:
        W1[:, dead] = 0.0
        b1[:, dead] = -b1[:, dead].abs() - 0.125
    W1, b1 = W1.float(), b1.float()
    W2 = b2 = None
    if two:
        col = torch.ones(d, dtype=F64)
        q, l = marked(d)
        col[q], col[l] = 2.0 ** -12, 2.0 ** 12
        W2 = (torch.randn(K, d, nhid, generator=gen, dtype=F64) * _pow2(gen, nhid) / nhid ** 0.5 * col[:, None]).float()
        b2 = (torch.randn(K, d, generator=gen, dtype=F64) * col).float()
    dZ = (torch.randn(N, K, d, generator=gen, dtype=F64) * _pow2(gen, d)).float()

    redraws = 0
    if two:
        while True:
            pre = torch.einsum("nf,khf->nkh", x.double(), W1.double()) + b1.double()
            pre_abs = torch.einsum("nf,khf->nkh", x.double().abs(), W1.double().abs()) + b1.double().abs()
            close = (pre.abs() <= MASK_MARGIN * U * pre_abs).flatten(1).any(1)
            if not bool(close.any()):
                break
            redraws += 1
            assert redraws <= MAX_REDRAWS, f"the ReLU mask of N={N} F={F} K={K} nhid={nhid} stays undecided on {int(close.sum())} nodes"
            x[close] = (draw_x(int(close.sum())) * row[close][:, None]).float()
    X = [None if v is None else v.double() for v in (x, W1, b1, W2, b2)]
    r = dict(x=x, W1=W1, b1=b1, W2=W2, b2=b2, dZ=dZ, redraws=redraws, zero_row=zero_row, dead=dead)
    fwd = forward64(*X)
    bwd = backward64(X[0], X[1], X[2], X[3], dZ.double())
    r.update({k + "64": v for k, v in {**fwd, **bwd}.items()})
    r.update({k + "_abs": v for k, v in companions64(*X, dZ.double()).items()})
    if two:
        assert bool((fwd["pre"].abs() > MASK_MARGIN * U * r["pre_abs"]).all())
        assert dead is None or bool((fwd["pre"][:, :, dead] < 0).all())
        r["hid32"] = fwd["hid"].float()                                   # what the kept backward is handed
        assert torch.equal(r["hid32"] > 0, fwd["pre"] > 0)
        kept = backward64(X[0], X[1], X[2], X[3], dZ.double(), hid=r["hid32"].double())
        r.update({k + "64_kept": v for k, v in kept.items()})
    assert zero_row is None or bool((x[zero_row] == 0).all())
    for k, v in r.items():
        if torch.is_tensor(v) and v.dtype == F64:
            assert bool(torch.isfinite(v.float()).all()), k
    return r


def hidT_layout(hid32: torch.Tensor) -> torch.Tensor:
    """[N, K, nhid] fp32 -> the library's kept hidden layer hidT [K][nhid][ld], ld = N rounded up to 4, NaN in the padding
    columns nobody owns (flat, as dl_project_hidden_floats counts it)."""
    N, K, nhid = hid32.shape
    ld = (N + 3) // 4 * 4
    out = torch.full((K, nhid, ld), float("nan"), dtype=torch.float32)
    out[:, :, :N] = hid32.permute(1, 2, 0)
    return out.reshape(-1)


CHAIN_BLOCK = 128                       # the kernels' tile: 128 nodes (TN), 128 hidden units (TH)


def _chain(n_terms: int, term, like: torch.Tensor) -> torch.Tensor:
    """sum_j term(j) in the dtype of `like`, as a tiled kernel sums: j ascending within tiles of CHAIN_BLOCK terms (one
    rounded multiply and one rounded add per term), then the tile sums added in order, as slabs are.  Elementwise IEEE
    operations only, so the result does not depend on the host's BLAS, vector width or thread count."""
    parts = []
    for j0 in range(0, n_terms, CHAIN_BLOCK):
        acc = torch.zeros_like(like)
        for j in range(j0, min(n_terms, j0 + CHAIN_BLOCK)):
            acc += term(j)
        parts.append(acc)
    total = torch.zeros_like(like)
    for part in parts:
        total += part
    return total


def fp32_evaluation(r):
    """The plain fp32 evaluation the ORACLE figures are measured on: the reference's sums on the float32 inputs, every
    contraction a blocked chain of fp32 multiply-adds (_chain; a library einsum sums in much the same way on one host,
    but its order of summation — hence these figures — changes with the BLAS code path of the CPU it runs on)."""
    x, W1, b1, W2, b2, dZ = (r[k] for k in ("x", "W1", "b1", "W2", "b2", "dZ"))
    N, F = x.shape
    K, M = W1.shape[:2]
    d = dZ.shape[2]
    f32 = torch.float32
    pre = _chain(F, lambda f: x[:, None, None, f] * W1[None, :, :, f], torch.empty(N, K, M, dtype=f32)) + b1
    if W2 is None:
        return {"Z1": pre, "dW": _chain(N, lambda n: dZ[n, :, :, None] * x[n, None, None, :], W1), "db": _chain(N, lambda n: dZ[n], b1)}
    assert torch.equal(pre > 0, r["pre64"] > 0)                        # decisive: the mask is the reference's
    hid = pre.clamp_min(0)
    Z = _chain(M, lambda h: hid[:, :, None, h] * W2[None, :, :, h], torch.empty(N, K, d, dtype=f32)) + b2
    dhid = _chain(d, lambda c: dZ[:, :, c, None] * W2[None, :, c, :], pre) * (pre > 0)
    return {"pre": pre, "Z": Z,
            "dW1": _chain(N, lambda n: dhid[n, :, :, None] * x[n, None, None, :], W1), "db1": _chain(N, lambda n: dhid[n], b1),
            "dW2": _chain(N, lambda n: dZ[n, :, :, None] * hid[n, :, None, :], W2), "db2": _chain(N, lambda n: dZ[n], b2)}


_JUDGED_BY = {"Z1": ("Z", "Z", "Z1"), "hid": ("hid", "pre", "pre")}      # output -> (reference, companion, ORACLE key)


def ratios(got: dict, r, suffix: str = "64") -> dict:
    """band_ratio of every output in `got` against the reference r (suffix "64_kept": the gradients from hid32).  A kept
    hidden layer is judged in the band of pre: the mask is decisive, so |relu(pre') - relu(pre)| <= |pre' - pre|."""
    out = {}
    for k, v in got.items():
        ref, comp, _key = _JUDGED_BY.get(k, (k, k, k))
        out[k] = band_ratio(v, r[ref + suffix] if (ref + suffix) in r else r[ref + "64"], r[comp + "_abs"])
    return out


# -------------------------------------------------------------------------------------------------- the cases
# env: the library's switches of the case; pad=False hands rows of F floats with F % 4 != 0 to the scalar-load kernels.
# expect: the form the case was written for — fwd (with its workspace) = (split, vec, G, chunks per group, launches);
# rec / kept (backward, recomputed / kept hidden layer) = (planes, VEC of kernel A, kernel B family, direct, blocked)
# plus, where the case is about them, (sA, tiles per range, sB, chunks per range).
# also: what the GPU test runs for this case on top (it reads this field, and `reached` counts a mode only where it is set):
# "nows" — the forward once more through dl_project_fwd without a workspace; "xplanes" — forward and both backwards once
# more on persistent x planes, bit for bit the per-call split; "one_alloc" — project_bwd(one_allocation=False), equal values.
# The hidden layer is kept, compared and fed back (the reference's) wherever `kept` is set.
PCase = namedtuple("PCase", "name N F K nhid d env pad fwd rec kept ranges also")
FP32 = (("DL_PROJECT_FP32_MFMA", "1"),)


def _c(name, N, F, K, nhid, d, env=(), pad=True, fwd=None, rec=None, kept=None, ranges=None, also=()):
    return PCase(name, N, F, K, nhid, d, tuple(env), pad, fwd, rec, kept, ranges, tuple(also))


def cases():
    """Smallest shapes that reach every compiled form.  Tails: N in {1, 127, 128, 129, 257, 300}, F in {1, 3, 8, 31, 32,
    33, 63, 64, 65, 129}, nhid in {2, 63, 64, 65, 127, 128, 129, 257}, K in {1, 3}."""
    P, V, S = "planes", "fp32-vector", "fp32-scalar"
    return [
        # ---- per factor width: three-plane products with odd rows / odd hidden width, fp32 MFMA aligned / scalar
        _c("d32-planes-F33-scalarA", 300, 33, 3, 64, 32, pad=False, fwd=(1, 1, 1, 1, 1), rec=(1, 0, P, 0, 0), kept=(1, 1, P, 0, 0), also=("nows",)),
        _c("d32-planes-nhid63", 129, 8, 1, 63, 32, fwd=(1, 0, 1, 1, 1), rec=(1, 1, P, 0, 0), kept=(1, 1, P, 0, 0), also=("nows", "xplanes",)),
        _c("d32-fp32-vector", 257, 64, 3, 128, 32, FP32, fwd=(0, 1, 1, 1, 1), rec=(0, 1, V, 0, 0), kept=(0, 1, V, 0, 0), also=("nows", "one_alloc",)),
        _c("d32-fp32-scalar-F3-nhid2", 127, 3, 1, 2, 32, FP32, pad=False, fwd=(0, 0, 1, 1, 1), rec=(0, 0, S, 0, 0), kept=(0, 1, S, 0, 0), also=("nows",)),
        _c("d64-planes-F31-scalarA", 128, 31, 1, 128, 64, pad=False, fwd=(1, 1, 1, 1, 1), rec=(1, 0, P, 0, 0), kept=(1, 1, P, 0, 0), also=("nows",)),
        _c("d64-planes-nhid129-G2", 300, 32, 3, 129, 64, fwd=(1, 0, 2, 1, 1), rec=(1, 1, P, 0, 0), kept=(1, 1, P, 0, 0), also=("nows", "xplanes",)),
        _c("d64-fp32-vector-F63padded", 129, 63, 1, 64, 64, FP32, fwd=(0, 1, 1, 1, 1), rec=(0, 1, V, 0, 0), kept=(0, 1, V, 0, 0), also=("nows",)),
        _c("d64-fp32-scalar-F65-nhid65", 300, 65, 3, 65, 64, FP32, pad=False, fwd=(0, 0, 1, 1, 1), rec=(0, 0, S, 0, 0), kept=(0, 1, S, 0, 0), also=("nows",)),
        _c("d128-planes-F129-scalarA", 257, 129, 3, 64, 128, pad=False, fwd=(1, 1, 1, 1, 1), rec=(1, 0, P, 0, 0), kept=(1, 1, P, 0, 0), also=("nows",)),
        _c("d128-planes-F65padded-nhid257-G3", 127, 65, 1, 257, 128, fwd=(1, 0, 3, 1, 1), rec=(1, 1, P, 0, 0), kept=(1, 1, P, 0, 0), also=("nows", "xplanes",)),
        _c("d128-fp32-vector-G2", 128, 32, 3, 256, 128, FP32, fwd=(0, 1, 2, 1, 1), rec=(0, 1, V, 0, 0), kept=(0, 1, V, 0, 0), also=("nows",)),
        _c("d128-fp32-scalar-N1-F1-nhid127", 1, 1, 3, 127, 128, FP32, pad=False, fwd=(0, 0, 1, 1, 1), rec=(0, 0, S, 1, 0), kept=(0, 1, S, 1, 0), also=("nows",)),
        # ---- hidden-chunk groups forced: five chunks in groups of 2, 2, 1 and of 2, 2, 1, 0 (an empty group adds zero)
        _c("groups3-nhid600-ragged", 129, 8, 1, 600, 64, (("DL_FWD_GROUPS", "3"),), fwd=(1, 1, 3, 2, 1), rec=(1, 1, P, 0, 0), kept=(1, 1, P, 0, 0)),
        _c("groups4-nhid600-empty", 129, 8, 1, 600, 64, (("DL_FWD_GROUPS", "4"),), fwd=(1, 1, 4, 2, 1), rec=(1, 1, P, 0, 0), kept=(1, 1, P, 0, 0)),
        _c("groups4-nhid600-empty-fp32", 129, 8, 1, 600, 64, FP32 + (("DL_FWD_GROUPS", "4"),), fwd=(0, 1, 4, 2, 1), rec=(0, 1, V, 0, 0), kept=(0, 1, V, 0, 0)),
        # ---- forward in node blocks of 128 rows: 128 + 128 + 44
        _c("fwd-node-blocks", 300, 33, 3, 64, 32, (("DL_FWD_BLOCK_ROWS", "1"),), fwd=(1, 1, 1, 1, 3), rec=(1, 1, P, 0, 0), kept=(1, 1, P, 0, 0)),
        # ---- slab counts of the backward: one range everywhere (kernel B writes dW1 itself), ragged last ranges
        _c("bwd-one-range-direct", 257, 32, 3, 64, 32, (("DL_BWD_TARGET", "1"),), fwd=(1, 1, 1, 1, 1), rec=(1, 1, P, 1, 0), kept=(1, 1, P, 1, 0),
           ranges=(1, 3, 1, 17), also=("one_alloc",)),
        _c("bwd-one-range-direct-fp32", 257, 32, 3, 64, 32, FP32 + (("DL_BWD_TARGET", "1"),), fwd=(0, 1, 1, 1, 1), rec=(0, 1, V, 1, 0), kept=(0, 1, V, 1, 0),
           ranges=(1, 3, 1, 9)),
        _c("bwd-ragged-ranges", 257, 32, 3, 64, 32, (("DL_BWD_TARGET", "6"),), fwd=(1, 1, 1, 1, 1), rec=(1, 1, P, 0, 0), kept=(1, 1, P, 0, 0),
           ranges=(2, 2, 2, 9)),
        _c("bwd-ragged-ranges-fp32", 257, 32, 3, 64, 32, FP32 + (("DL_BWD_TARGET", "6"),), fwd=(0, 1, 1, 1, 1), rec=(0, 1, V, 0, 0), kept=(0, 1, V, 0, 0),
           ranges=(2, 2, 2, 5)),
        # ---- backward in node blocks that accumulate: 4096 + 133 rows
        _c("bwd-node-blocks", 4096 + 133, 48, 2, 64, 32, (("DL_BWD_BLOCK_BYTES", str(1 << 20)),), fwd=(1, 1, 1, 1, 1), rec=(1, 1, P, 0, 1), kept=(1, 1, P, 0, 1)),
        _c("bwd-node-blocks-fp32", 4096 + 133, 48, 2, 64, 32, FP32 + (("DL_BWD_BLOCK_BYTES", str(1 << 20)),), fwd=(0, 1, 1, 1, 1), rec=(0, 1, V, 0, 1), kept=(0, 1, V, 0, 1)),
        # ---- single layer: project1_fwd_kernel<32 / 64 / 128>, kernel B over dZ, column sums
        _c("one-layer-d32-F33-scalarB", 300, 33, 3, 0, 32, pad=False, rec=(0, 0, S, 0, 0)),
        _c("one-layer-d64-F64", 129, 64, 1, 0, 64, rec=(0, 1, V, 0, 0)),
        _c("one-layer-d64-F65-scalarB", 127, 65, 3, 0, 64, pad=False, rec=(0, 0, S, 0, 0)),
        _c("one-layer-d128-F31padded", 257, 31, 3, 0, 128, rec=(0, 1, V, 0, 0)),
        _c("one-layer-d128-F63-N1", 1, 63, 1, 0, 128, pad=False, rec=(0, 0, S, 1, 0)),
    ]


def case_id(c: PCase) -> str:
    return c.name


def lib_F(c: PCase) -> int:
    """The feature count the library sees: ops pads rows to a multiple of 4 floats unless pad=False."""
    return (c.F + 3) // 4 * 4 if c.pad else c.F


def forms(c: PCase, lib_env):
    """The forms the library reports for case c under the case's switches (set here through the lib_env fixture):
    dict(fwd, nows, rec, kept) of _lib.project_*_form dicts (one layer: fwd and rec only)."""
    from disenlink_amd import _lib
    lib = _lib.load()
    for name, value in c.env:
        lib_env(name, value)
    two = c.nhid > 0
    F, nh = lib_F(c), (c.nhid if two else 1)
    ws = int(lib.dl_project_fwd_workspace_bytes(c.N, F, c.K, nh, c.d, int(two)))
    out = {"fwd": _lib.project_fwd_form(c.N, F, c.K, nh, c.d, two, ws), "rec": _lib.project_bwd_form(c.N, F, c.K, nh, c.d, two, False)}
    if two:
        out["nows"] = _lib.project_fwd_form(c.N, F, c.K, nh, c.d, True, 0)
        out["kept"] = _lib.project_bwd_form(c.N, F, c.K, nh, c.d, True, True)
        out["fwd_xp"] = _lib.project_fwd_form(c.N, F, c.K, nh, c.d, True, ws, True)
        out["rec_xp"] = _lib.project_bwd_form(c.N, F, c.K, nh, c.d, True, False, True)
        out["kept_xp"] = _lib.project_bwd_form(c.N, F, c.K, nh, c.d, True, True, True)
    for name, _value in c.env:
        lib_env(name)
    return out


def kernel_b(form: dict) -> str:
    return "planes" if form["planes"] else ("fp32-vector" if form["vecB"] else "fp32-scalar")


def check_expected(c: PCase, f: dict):
    """The case reaches the form it was written for (a changed heuristic must not move it onto another kernel silently)."""
    two = c.nhid > 0
    if two:
        got = tuple(f["fwd"][k] for k in ("split", "vec", "G", "chunks_per_group", "launches"))
        assert got == c.fwd, (c.name, "forward", got, c.fwd)
        assert (f["nows"]["split"], f["nows"]["G"], f["nows"]["launches"]) == (0, 1, 1), (c.name, "no workspace", f["nows"])
    else:
        assert tuple(f["fwd"].values()) == (0, 0, 1, 0, c.N, 1, 0), (c.name, f["fwd"])
    for which, want in (("rec", c.rec), ("kept", c.kept)):
        if want is None:
            continue
        b = f[which]
        got = (b["planes"], b["vecA"], kernel_b(b), b["direct"], b["blocked"])
        assert got == want, (c.name, which, got, want)
        assert b["recompute"] == (1 if (which == "rec" and two) else 0)
        if c.ranges is not None:
            got = (b["sA"], b["tiles_per_range"], b["sB"], b["chunks_per_range"])
            assert got == c.ranges, (c.name, which, "ranges", got, c.ranges)


def reached(all_forms: dict) -> dict:
    """What the case list reaches: sets of template-argument tuples and of launch modes, from {case: forms()}."""
    out = {k: set() for k in ("fwd", "nows", "A", "B", "one_layer", "modes")}
    for c, f in all_forms.items():
        two = c.nhid > 0
        if not two:
            out["one_layer"].add(c.d)
            out["B"].add(kernel_b(f["rec"]))
            out["modes"].add("one layer, kernel B " + kernel_b(f["rec"]))
            continue
        n_tiles, nhc = -(-c.N // 128), -(-c.nhid // 128)
        for which in ("fwd",) + (("nows",) if "nows" in c.also else ()):
            w = f[which]
            out["fwd"].add((c.d, w["vec"], w["split"]))
        w = f["fwd"]
        if "nows" in c.also and (f["nows"]["split"], f["nows"]["G"]) == (0, 1):
            out["modes"].add("no workspace")
            out["nows"].add((c.d, f["nows"]["vec"]))
        if c.kept is not None:
            out["modes"].add("keep hid")
        if "one_alloc" in c.also:
            out["modes"].add("separate gradient allocations")
        out["modes"].add(f"groups G={min(w['G'], 3)}{'+' if w['G'] >= 3 else ''}")
        if w["G"] > 1:
            out["modes"].add("slabs on planes" if w["split"] else "slabs on fp32 MFMA")
            last = nhc - (w["G"] - 1) * w["chunks_per_group"]
            if 0 < last < w["chunks_per_group"]:
                out["modes"].add("ragged last group")
            if last <= 0:
                out["modes"].add("empty group")
        if w["launches"] > 1:
            out["modes"].add("forward node blocks")
            if c.N % w["rows_per_launch"]:
                out["modes"].add("forward node blocks, short last block")
        if "xplanes" in c.also and f["fwd_xp"]["xplanes"]:
            out["modes"].add("persistent x planes")
        if "xplanes" in c.also and f["rec_xp"]["xplanes"] and f["kept_xp"]["xplanes"]:
            out["modes"].add("persistent x^T planes")
        for which in ("rec", "kept"):
            b = f[which]
            out["A"].add((c.d, b["vecA"], b["recompute"], b["planes"]))
            out["B"].add(kernel_b(b))
            fam = "planes" if b["planes"] else "fp32"
            if b["direct"]:
                out["modes"].add(f"kernel B direct, {fam}")
            if b["sA"] > 1 and b["sA"] * b["tiles_per_range"] > n_tiles:
                out["modes"].add(f"ragged last range of kernel A, {which}")
            n_chunks = -(-min(c.N, b["block_rows"]) // (16 if b["planes"] else 32))
            if b["sB"] > 1 and b["sB"] * b["chunks_per_range"] > n_chunks:
                out["modes"].add(f"ragged last range of kernel B, {fam}")
            if b["sA"] > 1:
                out["modes"].add(f"slab sum of dW2 / db1, {which}")
            if b["blocked"]:
                out["modes"].add(f"backward node blocks, {which}, {fam}")
    return out


def required() -> dict:
    """Every reachable combination of template arguments, every kernel-B family, every launch mode of the table."""
    D = (32, 64, 128)
    return {
        # form tuples (d, vec, split): the six with split = 1 reach the three project2_fwd_planes_kernel<D> (vec selects nothing
        # there), the six with split = 0 are project2_fwd_f32_kernel<D, VEC>
        "fwd": {(d, v, s) for d in D for v in (0, 1) for s in (0, 1)},
        # (d, vec, recompute, planes): project2_bwd_hidden_f32_kernel<D, VEC, RECOMPUTE, PLANES_OUT>, but kept + planes is
        # project2_bwd_hidden_planes_kernel<D>; the kept form is only launched with VEC = true
        "A": {(d, v, r, p) for d in D for v in (0, 1) for r in (0, 1) for p in (0, 1) if r or v},
        "B": {"planes", "fp32-vector", "fp32-scalar"},
        "one_layer": set(D),
        "nows": {(d, v) for d in D for v in (0, 1)},                 # dl_project_fwd without a workspace: fp32 MFMA, one group
        "modes": {"no workspace", "keep hid", "separate gradient allocations", "groups G=1", "groups G=2", "groups G=3+", "slabs on planes", "slabs on fp32 MFMA",
                  "ragged last group", "empty group", "forward node blocks", "forward node blocks, short last block",
                  "persistent x planes", "persistent x^T planes", "kernel B direct, planes", "kernel B direct, fp32",
                  "ragged last range of kernel A, rec", "ragged last range of kernel A, kept",
                  "ragged last range of kernel B, planes", "ragged last range of kernel B, fp32",
                  "slab sum of dW2 / db1, rec", "slab sum of dW2 / db1, kept",
                  "backward node blocks, rec, planes", "backward node blocks, kept, planes",
                  "backward node blocks, rec, fp32", "backward node blocks, kept, fp32",
                  "one layer, kernel B fp32-vector", "one layer, kernel B fp32-scalar"},
    }


def check_coverage(lib_env):
    from disenlink_amd import _lib
    # a new entry of either form (a new template argument, a new launch decision) needs a case and a line here first
    assert _lib.PROJECT_FWD_FORM == ("split", "vec", "G", "chunks_per_group", "rows_per_launch", "launches", "xplanes")
    assert _lib.PROJECT_BWD_FORM == ("planes", "vecA", "vecB", "recompute", "sA", "tiles_per_range", "sB", "chunks_per_range", "sC",
                                     "direct", "blocked", "block_rows", "blocks", "xplanes")
    cs = cases()
    assert len({c.name for c in cs}) == len(cs)
    all_forms = {c: forms(c, lib_env) for c in cs}
    for c, f in all_forms.items():
        check_expected(c, f)
    got, want = reached(all_forms), required()
    assert len(want["fwd"]) == 12 and len(want["A"]) == 18
    for k in want:
        assert got[k] >= want[k], (k, "not reached by any case:", sorted(want[k] - got[k], key=str))
    return got
