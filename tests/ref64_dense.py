"""Plain float64 reference of the all-pairs scorer family (model.py:109-113: link_pred, its dense backward, the ranking of
all candidates), the inputs it is run on and the case lists that reach every launch form of those kernels.
TEST INFRASTRUCTURE: torch, float64, CPU.  The sibling of tests/ref64.py (sparse hot path) and tests/ref64_project.py.

  logit     s[u,v] = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t)                       prob = sigmoid(s)
  companion s_abs  = sum_k e_k (|h|.|h| + |h.h| |z|.|z| / t)                            (ref64.logit_abs64's measure)
  backward  G = g p (1 - p),  G^ = G + G^T,  per k: E = exp(Z_k Z_k^T / t), Q = H_k H_k^T
            dH_k = (G^ o E) H_k                   companion (|G| + |G|^T) o E o (1 + Za / t) . |H_k|
            dZ_k = (G^ o Q o E / t) Z_k           companion (|G| + |G|^T) o E o (Ha + |Q| Za / t) / t . |Z_k|
  with Za = |Z_k| |Z_k|^T, Ha = |H_k| |H_k|^T (tests/test_gpu_dense_bwd.py::bwd64's bands without their 1e-5).

Every output is judged per element by ref64.band_ratio: |got - ref| / (2^-24 companion).  ORACLE holds the largest such
ratio a plain fp32 evaluation (fp32_forward / fp32_backward below: elementwise IEEE operations, features summed in index
order within chunks of 32 and the chunk sums added in order, the node contraction of the backward in tiles of 128 whose
sums are added in order within a slice, the slices added in order) shows against this reference over all cases;
tests/test_ref64_dense_cpu.py measures the figures again on every run.  The bound of a kernel's output is 4 x the figure
(another equally valid fp32 summation order and a hardware exp: the project's convention) plus ref64_project.PLANE =
2 + 2^-8 units for every three-plane product between the exactly rounded inputs and the output.

Count of plane products (dl_score_dense.hip, dl_score_dense_bwd.hip, dl_score_rank.hip).
  logit 1.  S = z.z and Q = h.h are each one three-plane product.  S's dropped products move s by at most
            PLANE u e |Q| Za / t and Q's by PLANE u e Ha: the two are SEPARATE addends of the companion, so together
            they are one PLANE x companion, not two.
  dH 1 + 1. The weight G^ o E carries S's term (inside the companion's Za / t addend: one PLANE x companion); the
            weight is then split into three planes EXACTLY (three planes hold any fp32 number: ref64_project's
            docstring) and multiplied against the planes of H_k: a second three-plane product.
  dZ 1 + 1. The weight G^ o Q o E / t carries the logit's single term, the product against Z_k the second.
  The per-shape kernel (dl_score.hip) and the generic kernel (dl_generic.hip) multiply in fp32: no plane term.  bf16
  tables are rounded first and the reference runs on the rounded values; the output is fp32, so the fp32 bound holds.
What the bounds can and cannot see (tests/test_ref64_dense_cpu.py, on a CPU emulation of the scheme: _split6 adds each
plane product of a K = 16 block — one matrix instruction, half a staged chunk of 32 features — to the fp32 accumulator with
one rounding, in mfma_split6's order).  With each of the five removable products dropped in turn the emulation leaves the
bound of the logit and of dZ when the product is dropped from the Gram products, and of dZ and dH when it is dropped from
the second products.  ONE EXCEPTION: a small product (mid*mid, hi*lo, lo*hi) dropped from the backward's Gram products alone
stays inside dH's bound (24 - 50 units against 63.21 on every case tried, also with Z twice as loud).  dH = (G^ o E) H sees
S only through E, a Za / (t + Za) share of its companion, and its bound carries the 14.8 units of a sequential fp32 sum over
128 nodes with loud rows early in the tile.  Such a loss is caught on dZ of the same launch (the same registers feed both
weights), which the test asserts; it is not asserted on dH.
Probabilities: ref64.prob_band over the logit band plus the fp32 sigmoid's own rounding (ORACLE["prob_eps"] units).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import torch

import ref64
import ref64_project as rp
from ref64 import F64, U, band_ratio, prob_band, sigmoid32

# Largest error of the plain fp32 evaluation against this reference over all cases (three significant digits), in units
# of 2^-24 * companion; measured on the CPU by tests/test_ref64_dense_cpu.py and never set from what a kernel gives.
ORACLE = {"logit": 5.80, "prob_eps": 1.48, "dH": 14.8, "dZ": 9.43}
PLANE = rp.PLANE
PLANE_PRODUCTS = {"logit": 1, "dH": 2, "dZ": 2}
F32 = torch.float32


def bound(key: str, planes: bool = True) -> float:
    return 4.0 * ORACLE[key] + (PLANE_PRODUCTS.get(key, 0) * PLANE if planes else 0.0)


# -------------------------------------------------------------------------------------------------- the inputs
Z_QUIET, Z_LOUD, H_QUIET, H_LOUD = 2.0 ** -6, 2.0 ** 1, 2.0 ** -12, 2.0 ** 6
G_QUIET, G_LOUD = 2.0 ** -6, 2.0 ** 6
KINDS = ("dense", "upper", "offdiag", "diag")


def _unmarked(n: int):
    q, l = rp.marked(n)
    used = set(q) | set(l)
    return [i for i in range(n) if i not in used]


def special_rows(N: int):
    """(zero row, (copy a, copy b)) among the rows no mark sits on: the zero row is the first, the copies the second and
    the last of them — in different 32-row blocks from N = 36 on and in different 128-row tiles from N = 131 on."""
    free = _unmarked(N)
    zero = free[0] if N >= 3 else None
    copies = (free[1], free[-1]) if (len(free) >= 3 and free[-1] // 32 != free[1] // 32) else None
    return zero, copies


@functools.lru_cache(maxsize=None)
def tables(N: int, K: int, d: int, dtype: str = "f32"):
    """Z, H [N, K, d] float32 holding values of the table type (bf16 tables: rounded to bf16 first).  Normal deviates times
    a per-feature power of two (2^-2 .. 2^2), normalised so that an ordinary row has |z_k|^2 ~ |h_k|^2 ~ 1, rounded to
    fp32: full 24-bit mantissas, all three bf16 planes populated.  Quiet / loud node rows at the tile positions
    (ref64_project.marked), one all-zero node row, two exact copies of one row (special_rows)."""
    gen = torch.Generator().manual_seed(7 + 1000003 * N + 10007 * K + 101 * d + (5 if dtype == "bf16" else 0))
    out = []
    zero, copies = special_rows(N)
    for quiet, loud in ((Z_QUIET, Z_LOUD), (H_QUIET, H_LOUD)):
        sf = rp._pow2(gen, d)
        row = torch.ones(N, dtype=F64)
        q, l = rp.marked(N)
        row[q], row[l] = quiet, loud
        if N == 1:
            row[0] = 1.0                                                  # the only row: neither quiet nor loud
        if zero is not None:
            row[zero] = 0.0
        x = torch.randn(N, K, d, generator=gen, dtype=F64) * (sf / float((sf * sf).sum()) ** 0.5) * row[:, None, None]
        x = x.float() if dtype == "f32" else x.to(torch.bfloat16).float()
        if copies is not None:
            x[copies[1]] = x[copies[0]]
        assert rp.split3_exact(x)
        out.append(x)
    return out[0], out[1]


def _factor(X, k):
    return X[:, k, :].double()


def forward64(Z, H, t):
    """-> s, s_abs [N, N] float64, looped over the factors (nothing of size K N N is formed)."""
    N, K, _d = Z.shape
    s, s_abs = torch.zeros(N, N, dtype=F64), torch.zeros(N, N, dtype=F64)
    arg = 0.0
    for k in range(K):
        z, h = _factor(Z, k), _factor(H, k)
        S, Q = z @ z.t(), h @ h.t()
        arg = max(arg, float(S.abs().max()) / t)
        E = torch.exp(S / t)
        s += Q * E
        s_abs += E * (h.abs() @ h.abs().t() + Q.abs() * (z.abs() @ z.abs().t()) / t)
    return s, s_abs, arg


@functools.lru_cache(maxsize=6)
def reference(N: int, K: int, d: int, t: float, dtype: str = "f32"):
    """Tables of one case and what the fp64 reference says about them.  Conditions, asserted here on the reference alone:
    everything finite in fp32, max |z.z / t| <= 60 (no exp overflows), at least half of all pairs with |s| < 8."""
    Z, H = tables(N, K, d, dtype)
    s, s_abs, arg = forward64(Z, H, t)
    assert arg <= 60.0, (N, K, d, t, arg)
    assert bool(torch.isfinite(s.float()).all()) and bool(torch.isfinite(s_abs.float()).all())
    assert float((s.abs() < 8).double().mean()) >= 0.5, (N, K, d, t)
    zero, copies = special_rows(N)
    if copies is not None:                                  # equal rows give equal sums; a host's blocked matrix product need not
        a, b = copies
        for x in (s, s_abs):
            x[b, :] = x[a, :]
            x[:, b] = x[:, a]
    return dict(Z=Z, H=H, t=t, s=s, s_abs=s_abs, prob32=sigmoid32(s).float(), zero=zero, copies=copies)


def g_special(N: int):
    """(zero row, zero column) of g_prob: the third and fourth unmarked index (none below N = 37)."""
    free = _unmarked(N)
    return (free[2], free[3]) if N >= 37 else (None, None)


@functools.lru_cache(maxsize=None)
def gradient(N: int, kind: str):
    """g_prob [N, N] float32: full mantissas, mixed signs, a per-column power of two, quiet / loud rows and columns at the
    tile positions, one zero row and one zero column; the rows and the columns of the two copied nodes are alike."""
    gen = torch.Generator().manual_seed(977 * N + 13)
    g = torch.randn(N, N, generator=gen, dtype=F64) * rp._pow2(gen, N)
    scale = torch.ones(N, dtype=F64)
    q, l = rp.marked(N)
    if N > 1:
        scale[q], scale[l] = G_QUIET, G_LOUD
    g = g * scale[:, None] * scale[None, :]
    zr, zc = g_special(N)
    if zr is not None:
        g[zr, :] = 0.0
        g[:, zc] = 0.0
    _zero, copies = special_rows(N)
    if copies is not None:
        a, b = copies
        g[b, :] = g[a, :]
        g[:, b] = g[:, a]
    if kind == "upper":
        g = torch.triu(g, diagonal=1)
    elif kind == "offdiag":
        u, v = (N // 3, min((2 * N) // 3 + 1, N - 1)) if N > 1 else (0, 0)
        one = torch.zeros(N, N, dtype=F64)
        one[u, v] = g[u, v] if float(g[u, v]) != 0 else 1.7
        g = one
    elif kind == "diag":
        one = torch.zeros(N, N, dtype=F64)
        one[N // 2, N // 2] = g[N // 2, N // 2] if float(g[N // 2, N // 2]) != 0 else -2.3
        g = one
    else:
        assert kind == "dense"
    g = g.float()
    assert rp.split3_exact(g)
    return g


@functools.lru_cache(maxsize=4)
def backward_reference(N: int, K: int, d: int, t: float):
    """{kind: dict(g, dZ, dH, dZ_abs, dH_abs)} float64 from the fp32 rounding of the REFERENCE's prob (no forward
    kernel's error leaks into the check of the backward), looped over the factors for all kinds at once."""
    r = reference(N, K, d, t)
    Z, H, p = r["Z"], r["H"], r["prob32"].double()
    out = {}
    for kind in KINDS:
        g = gradient(N, kind)
        G = g.double() * p * (1.0 - p)
        out[kind] = dict(g=g, Gh=G + G.t(), Ga=G.abs() + G.t().abs(), dZ=torch.zeros(N, K, d, dtype=F64), dH=torch.zeros(N, K, d, dtype=F64),
                         dZ_abs=torch.zeros(N, K, d, dtype=F64), dH_abs=torch.zeros(N, K, d, dtype=F64))
    for k in range(K):
        z, h = _factor(Z, k), _factor(H, k)
        Q, za, ha = h @ h.t(), z.abs() @ z.abs().t(), h.abs() @ h.abs().t()
        E = torch.exp(z @ z.t() / t)
        wH_abs, wZ_abs = E * (1.0 + za / t), E * (ha + Q.abs() * za / t) / t
        for o in out.values():
            o["dH"][:, k] = (o["Gh"] * E) @ h
            o["dZ"][:, k] = (o["Gh"] * Q * E / t) @ z
            o["dH_abs"][:, k] = (o["Ga"] * wH_abs) @ h.abs()
            o["dZ_abs"][:, k] = (o["Ga"] * wZ_abs) @ z.abs()
    for o in out.values():
        del o["Gh"], o["Ga"]
        for key in ("dZ", "dH", "dZ_abs", "dH_abs"):
            assert bool(torch.isfinite(o[key].float()).all()), key
    return out


def slice_tiles(N: int, nslice: int):
    """[(first v tile, end)] of every slice of the dense backward: the kernel's split vt_beg = slice * nvt / nslice."""
    nvt = -(-N // 128)
    return [(s * nvt // nslice, (s + 1) * nvt // nslice) for s in range(nslice)]


# -------------------------------------------------------------------------------------------------- plain fp32
def _gram32(X):
    """X X^T of a float32 [N, d] matrix: features in index order within chunks of 32, one rounded multiply and one rounded
    add per term, the chunk sums added in order."""
    N, d = X.shape
    total, tmp = torch.zeros(N, N, dtype=F32), torch.empty(N, N, dtype=F32)
    Xt = X.t().contiguous()
    for c0 in range(0, d, 32):
        acc = torch.zeros(N, N, dtype=F32)
        for j in range(c0, min(d, c0 + 32)):
            torch.mul(Xt[j][:, None], Xt[j][None, :], out=tmp)
            acc += tmp
        total += acc
    return total


def _contract32(W, X, slices):
    """W [N, N] . X [N, d] in float32: v in index order within tiles of 128, the tile sums added in order within a slice, the
    slices added in order."""
    N, d = X.shape
    total, tmp = torch.zeros(N, d, dtype=F32), torch.empty(N, d, dtype=F32)
    Wt = W.t().contiguous()
    for beg, end in slices:
        part = torch.zeros(N, d, dtype=F32)
        for tile in range(beg, end):
            acc = torch.zeros(N, d, dtype=F32)
            for v in range(tile * 128, min(N, tile * 128 + 128)):
                torch.mul(Wt[v][:, None], X[v][None, :], out=tmp)
                acc += tmp
            part += acc
        total += part
    return total


def fp32_forward(Z, H, t):
    """-> logit, prob float32 [N, N]."""
    N, K, _d = Z.shape
    t32 = torch.tensor(t, dtype=F32)
    x = torch.zeros(N, N, dtype=F32)
    for k in range(K):
        e = torch.exp(_gram32(Z[:, k].contiguous()) / t32)
        x += _gram32(H[:, k].contiguous()) * e
    return x, 1.0 / (1.0 + torch.exp(-x))


def fp32_backward(Z, H, t, prob32, g, slices):
    """-> dZ, dH float32 [N, K, d] as the kernel orders its operations: G = (g p)(1 - p), the weights (G^ Q) E / t and G^ E."""
    N, K, d = Z.shape
    t32 = torch.tensor(t, dtype=F32)
    G = g * prob32 * (1.0 - prob32)
    Gh = G + G.t()
    dZ, dH = torch.empty(N, K, d, dtype=F32), torch.empty(N, K, d, dtype=F32)
    for k in range(K):
        z, h = Z[:, k].contiguous(), H[:, k].contiguous()
        e = torch.exp(_gram32(z) / t32)
        dZ[:, k] = _contract32(((Gh * _gram32(h)) * e) / t32, z, slices)
        dH[:, k] = _contract32(Gh * e, h, slices)
    return dZ, dH


# -------------------------------------------------------------------------------------------------- the plane scheme
# dl_tiles.h:mfma_split6 — (plane of A, plane of B) in the order the six products enter the accumulator, smallest first
SIX = ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0))
NAMES = {(1, 1): "mid*mid", (0, 2): "hi*lo", (2, 0): "lo*hi", (0, 1): "hi*mid", (1, 0): "mid*hi", (0, 0): "hi*hi"}
REMOVABLE = SIX[:5]


def _planes(X):
    return [p.double() for p in rp.split3(X)]


def _split6(acc, A, B, lo, hi, drop):
    """acc (float32) += A[:, lo:hi] . B[:, lo:hi]^T from the planes: one K = 16 block = one matrix instruction per plane
    product (a staged chunk of 32 features is two such blocks; the accumulator runs on across chunks, as the kernels' does).
    Every bf16 x bf16 product is exact and an instruction's 16 of them are added to the accumulator with one rounding (the
    instruction taken as ideal)."""
    for pa, pb in SIX:
        if (pa, pb) != drop:
            acc = (acc.double() + A[pa][:, lo:hi] @ B[pb][:, lo:hi].t()).float()
    return acc


def _gram_planes(X, drop):
    N, d = X.shape
    P = _planes(X)
    acc = torch.zeros(N, N, dtype=F32)
    for lo in range(0, d, 16):                                   # zero columns out to a multiple of 32 add nothing
        acc = _split6(acc, P, P, lo, min(d, lo + 16), drop)
    return acc


def _contract_planes(W, X, slices, drop):
    N, d = X.shape
    A, B = _planes(W), [p.t().contiguous() for p in _planes(X)]  # A: weight [u][v]; B^T: [c][v]
    total = None
    for beg, end in slices:
        acc = torch.zeros(N, d, dtype=F32)
        for lo in range(beg * 128, min(N, end * 128), 16):
            acc = _split6(acc, A, B, lo, min(N, lo + 16), drop)
        total = acc if total is None else total + acc
    return total


def planes_forward(Z, H, t, drop=None):
    """The matrix-core scorer on the CPU: three planes per operand, the products of SIX (without `drop`) into an fp32
    accumulator, exp and the sum over k in fp32.  -> logit float32 [N, N]."""
    N, K, _d = Z.shape
    t32 = torch.tensor(t, dtype=F32)
    x = torch.zeros(N, N, dtype=F32)
    for k in range(K):
        e = torch.exp(_gram_planes(Z[:, k].contiguous(), drop) / t32)
        x += _gram_planes(H[:, k].contiguous(), drop) * e
    return x


def planes_backward(Z, H, t, prob32, g, slices, drop_gram=None, drop_second=None):
    N, K, d = Z.shape
    t32 = torch.tensor(t, dtype=F32)
    G = g * prob32 * (1.0 - prob32)
    Gh = G + G.t()
    dZ, dH = torch.empty(N, K, d, dtype=F32), torch.empty(N, K, d, dtype=F32)
    for k in range(K):
        z, h = Z[:, k].contiguous(), H[:, k].contiguous()
        e = torch.exp(_gram_planes(z, drop_gram) / t32)
        dZ[:, k] = _contract_planes(((Gh * _gram_planes(h, drop_gram)) * e) / t32, z, slices, drop_second)
        dH[:, k] = _contract_planes(Gh * e, h, slices, drop_second)
    return dZ, dH


# -------------------------------------------------------------------------------------------------- the cases
KERNELS = ("generic", "per shape", "matrix cores, split on stage", "matrix cores, from planes")
FCase = namedtuple("FCase", "name N K d t dtype kernel force_generic expect")
BCase = namedtuple("BCase", "name N K d t ncb slicing")


def dense_cases(lib):
    """Forward cases; `kernel` names the family, `expect` what the form export must report for the case (a dict)."""
    cs = []
    mf = "matrix cores"
    grid = [(1, 1, 32, 1.0), (37, 3, 64, 2.0), (128, 8, 96, 0.5), (129, 1, 128, 1.0), (260, 3, 32, 0.5), (385, 8, 64, 1.0),
            (129, 64, 32, 2.0), (260, 1, 96, 1.0), (37, 8, 128, 0.5)]
    for N, K, d, t in grid:
        nt = -(-N // 128)
        cs.append(FCase(f"mfma-N{N}-K{K}-d{d}-t{t:g}", N, K, d, t, "f32", mf, False, dict(items=nt * (nt + 1) // 2, grid=256)))
    cs.append(FCase("mfma-N2945-K1-d32-second-round", 2945, 1, 32, 1.0, "f32", mf, False, dict(items=300, grid=512)))
    t_of = ref64.TEMPERATURES
    i = 0
    big = {}
    for dtype in ("f32", "bf16"):
        for K, d in ref64.tuned_shapes(lib, dtype):
            if dtype == "f32" and d % 32 == 0:
                continue
            for N, want in ((63, dict(n_slices=1, slice_w=63, chunks_per_u=1)), (130, dict(n_slices=8, slice_w=17, chunks_per_u=1))):
                cs.append(FCase(f"shape-{dtype}-K{K}-d{d}-N{N}", N, K, d, t_of[i % 3], dtype, "per shape", False, want))
                i += 1
            if dtype not in big or K * d < big[dtype][0] * big[dtype][1]:
                big[dtype] = (K, d)
    for dtype, (K, d) in big.items():
        cs.append(FCase(f"shape-{dtype}-K{K}-d{d}-N2060-two-chunks", 2060, K, d, 1.0, dtype, "per shape", False,
                        dict(n_slices=8, slice_w=258, chunks_per_u=2)))
    for j, (K, d) in enumerate(ref64.UNTUNED):
        cs.append(FCase(f"generic-K{K}-d{d}", 70, K, d, t_of[j % 3], "f32", "generic", False, dict(items=4900)))
    cs.append(FCase("generic-K8-d64-forced", 70, 8, 64, 1.0, "f32", "generic", True, dict(items=4900)))
    return cs


def dense_bwd_cases():
    grid = [(1, 1, 1, 1.0), (37, 3, 8, 2.0), (128, 8, 32, 1.0), (129, 1, 33, 2.0), (300, 3, 64, 1.0), (37, 8, 65, 1.0),
            (129, 3, 96, 2.0), (300, 1, 100, 1.0), (128, 3, 128, 2.0), (300, 8, 32, 2.0), (1, 1, 128, 2.0), (129, 1, 8, 1.0)]
    cs = [BCase(f"N{N}-K{K}-d{d}-t{t:g}", N, K, d, t, -(-d // 32), "one tile per slice") for N, K, d, t in grid]
    for d in (32, 100):
        cs.append(BCase(f"ragged-slices-N600-K32-d{d}", 600, 32, d, 1.0, -(-d // 32), "ragged"))
        cs.append(BCase(f"unsliced-N1000-K64-d{d}", 1000, 64, d, 1.0, -(-d // 32), "unsliced"))
    return cs


def case_id(c):
    return c.name


def forward_form(c: FCase, with_ws: bool):
    """What the library reports for a forward case (host only); force_generic is set and restored here."""
    from disenlink_amd import _lib
    lib = _lib.load()
    code = {"f32": _lib.DL_F32, "bf16": _lib.DL_BF16}[c.dtype]
    old = lib.dl_set_force_generic(1 if c.force_generic else 0)
    try:
        ws = int(lib.dl_score_allpairs_workspace_bytes(c.N, c.K, c.d, code)) if with_ws else 0
        f = _lib.score_allpairs_fwd_form(c.N, c.K, c.d, code, ws)
    finally:
        lib.dl_set_force_generic(old)
    f["kernel"] = KERNELS[f["kernel"]]
    return f


def check_forward_form(c: FCase):
    """The case reaches the form it names, with and without the workspace."""
    for with_ws in (True, False):
        f = forward_form(c, with_ws)
        if c.kernel == "matrix cores":
            assert f["kernel"] == KERNELS[3 if with_ws else 2], (c.name, f)
        else:
            assert f["kernel"] == c.kernel, (c.name, f)
        for k, v in c.expect.items():
            assert f[k] == v, (c.name, k, f)
    return forward_form(c, True)


def backward_form(c: BCase):
    from disenlink_amd import _lib
    f = _lib.score_allpairs_bwd_dense_form(c.N, c.K, c.d)
    nvt = f["Np"] // 128
    f["slicing"] = "unsliced" if f["nslice"] == 1 and nvt > 1 else ("ragged" if f["max_tiles"] > f["min_tiles"] else "one tile per slice")
    return f


def check_backward_form(c: BCase):
    f = backward_form(c)
    assert f["NCB"] == c.ncb and f["slicing"] == c.slicing, (c.name, f)
    assert f["max_tiles"] == 1 or c.slicing != "one tile per slice"
    return f


def ratios_forward(x, r):
    return band_ratio(x, r["s"], r["s_abs"])


def prob_band_of(r, planes: bool, slack: float = 1.0):
    return prob_band(r["s"], slack * bound("logit", planes) * U * r["s_abs"], slack * 4.0 * ORACLE["prob_eps"] * U)


def prob_ratio(prob, r, planes: bool):
    """max over elements of |prob - sigmoid(s)| / its band (<= 1 passes; NaN fails)."""
    err = (torch.as_tensor(prob).double() - torch.sigmoid(r["s"])).abs()
    q = err / prob_band_of(r, planes)
    return float("nan") if bool(torch.isnan(q).any()) else float(q.max())


# -------------------------------------------------------------------------------------------------- ranking
# slices: the DL_RANK_SLICES values the case is run under on top of the library's own choice (1, the tile count, and at
# N = 1000 the 3 that leaves a ragged last slice: 8 tiles in slices of 3, 3, 2).  orders: the permuted orders as well.
RCase = namedtuple("RCase", "name N K d t Q slices orders exclusion")
TOPK = (1, 63, 64, 65, 128)
ORDERS = ("as drawn", "ascending", "descending")
MAX_UNDECIDED = 0.10


def rank_cases():
    return [
        RCase("N1-K1-d1-Q1", 1, 1, 1, 1.0, 1, (1,), False, False),
        RCase("N37-K3-d8-Q16", 37, 3, 8, 2.0, 16, (1,), False, False),
        RCase("N128-K8-d31-Q128", 128, 8, 31, 1.0, 128, (1,), False, False),
        RCase("N129-K1-d32-Q129", 129, 1, 32, 1.0, 129, (1, 2), True, False),
        RCase("N300-K3-d33-Q300", 300, 3, 33, 2.0, 300, (1, 3), False, False),
        RCase("N1000-K8-d48-Q16", 1000, 8, 48, 1.0, 16, (1, 8, 3), False, False),
        RCase("N300-K1-d64-Q128", 300, 1, 64, 1.0, 128, (1, 3), True, False),
        RCase("N1000-K3-d100-Q129", 1000, 3, 100, 2.0, 129, (1, 8, 3), False, False),
        RCase("N300-K8-d128-Q16", 300, 8, 128, 1.0, 16, (1, 3), False, False),
        RCase("N1000-K3-d32-Q300-exclusion", 1000, 3, 32, 1.0, 300, (1, 8, 3), True, True),
    ]


def rank_form(c: RCase, k: int, lib_env, slices=None):
    """The scan's plan for the case under DL_RANK_SLICES = slices (None: the library's own choice), host only."""
    from disenlink_amd import _lib
    lib_env("DL_RANK_SLICES", slices)
    f = _lib.score_topk_form(c.N, c.K, c.d, c.Q, k)
    nt = -(-c.N // 128)
    assert (f["nd"], f["qtiles"], f["cap"]) == (-(-c.d // 32), -(-c.Q // 128), k + 64), (c.name, f)
    assert (f["slices"] - 1) * f["tiles_per_slice"] + f["last_tiles"] == nt and 1 <= f["last_tiles"] <= f["tiles_per_slice"], (c.name, f)
    if slices is not None:
        tps = -(-nt // min(slices, nt))
        assert (f["tiles_per_slice"], f["slices"]) == (tps, -(-nt // tps)), (c.name, slices, f)
    lib_env("DL_RANK_SLICES")
    return f


def _queries(c: RCase):
    """Query nodes (original ids), with duplicates, the first and the last row and — where there are any — the two copies."""
    _zero, copies = special_rows(c.N)
    head = [0, c.N - 1, 0, c.N - 1] + (list(copies) if copies else [])
    gen = torch.Generator().manual_seed(31 * c.N + c.Q)
    q = head[:c.Q] + torch.randint(0, c.N, (max(0, c.Q - len(head)),), generator=gen).tolist()
    return torch.tensor(q, dtype=torch.int64)


def _exclusion(c: RCase):
    """(rows, cols) int64, original ids, or None.  Node 0 loses a whole candidate tile (columns 256 .. 383), node N - 1 the
    first and the last column of a tile and of the table, the first copy keeps 40 candidates (fewer than k from k = 63 on),
    2000 more pairs are scattered."""
    if not c.exclusion:
        return None
    N = c.N
    _zero, copies = special_rows(N)
    gen = torch.Generator().manual_seed(N + 17)
    rows = [torch.zeros(128, dtype=torch.int64), torch.full((4,), N - 1, dtype=torch.int64)]
    cols = [torch.arange(256, 384), torch.tensor([384, 511, 0, N - 2])]
    keep = torch.ones(N, dtype=torch.bool)
    keep[5:45] = False
    rows.append(torch.full((int(keep.sum()),), copies[0], dtype=torch.int64))
    cols.append(torch.nonzero(keep)[:, 0])
    rows.append(torch.randint(0, N, (2000,), generator=gen))
    cols.append(torch.randint(0, N, (2000,), generator=gen))
    return torch.cat(rows), torch.cat(cols)


@functools.lru_cache(maxsize=None)
def _permutation(c: RCase, order: str):
    """perm: new node i is original node perm[i].  Ascending / descending: by the fp64 logit against one ordinary query
    node, so that in ITS row every candidate beats the running threshold / none after the first k does."""
    N = c.N
    if order == "as drawn":
        return torch.arange(N)
    r = reference(c.N, c.K, c.d, c.t)
    pivot = _queries(c)[min(c.Q - 1, 7)]
    return torch.sort(r["s"][pivot], descending=(order == "descending"), stable=True).indices


@functools.lru_cache(maxsize=4)
def rank_view(c: RCase, order: str = "as drawn"):
    """What a ranking call on the case is handed under `order` and what the reference says about it, all in NEW node ids:
    Z, H float32 (rows permuted together), queries int64 [Q], s / band float64 [Q, N] (band = the kernel's bound on the
    logit), cand bool [Q, N] (exclude_self and the exclusion set applied), exclude = (rows, cols) or None, perm, twins."""
    r = reference(c.N, c.K, c.d, c.t)
    perm = _permutation(c, order)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(c.N)
    q_old = _queries(c)
    s = r["s"][q_old][:, perm]
    band = bound("logit") * U * r["s_abs"][q_old][:, perm]
    cand = torch.ones(c.Q, c.N, dtype=torch.bool)
    cand[torch.arange(c.Q), inv[q_old]] = False
    ex = _exclusion(c)
    exclude = None
    if ex is not None:
        mask = torch.zeros(c.N, c.N, dtype=torch.bool)
        mask[ex[0], ex[1]] = True
        cand &= ~mask[q_old][:, perm]
        exclude = (inv[ex[0]], inv[ex[1]])
    twins = tuple(sorted(int(inv[i]) for i in r["copies"])) if r["copies"] else None
    return dict(Z=r["Z"][perm].contiguous(), H=r["H"][perm].contiguous(), queries=inv[q_old], s=s, band=band, cand=cand,
                exclude=exclude, perm=perm, twins=twins, q_old=q_old)


def _without_later_twin(cand, twins):
    """cand with the later twin dropped wherever both twins are candidates (they then stand for one value)."""
    if twins is None:
        return cand, torch.zeros(cand.shape[0], dtype=torch.bool)
    both = cand[:, twins[0]] & cand[:, twins[1]]
    c = cand.clone()
    c[both, twins[1]] = False
    return c, both


def separation(s, band, cand):
    """Candidates of every row by logit descending (equal logits by index): order [Q, N], and for position j whether the
    band of that candidate is disjoint from the bands of ALL others (alone), and whether all bands at positions < j lie
    strictly above all bands at positions >= j (cut [Q, N + 1]; positions past the candidates count as decided)."""
    inf = float("inf")
    sv, order = torch.sort(torch.where(cand, s, torch.full_like(s, -inf)), dim=1, descending=True, stable=True)
    b, c = band.gather(1, order), cand.gather(1, order)
    lower = torch.where(c, sv - b, torch.full_like(sv, inf))
    upper = torch.where(c, sv + b, torch.full_like(sv, -inf))
    Q = s.shape[0]
    above = torch.cat([torch.full((Q, 1), inf, dtype=F64), torch.cummin(lower, 1).values], 1)               # min lower of [0, j)
    below = torch.cat([torch.cummax(upper.flip(1), 1).values.flip(1), torch.full((Q, 1), -inf, dtype=F64)], 1)   # max upper of [j, N)
    cut = above > below
    alone = c & (above[:, :-1] > upper) & (below[:, 1:] < lower)
    return order, alone, cut


def topk_expectation(view, k):
    """-> ref [Q, k] int64 (the reference's top-k by (logit descending, index ascending), -1 where a row has fewer
    candidates), n [Q], decisive [Q] bool: no band of a candidate outside the reference's set reaches a band inside it (the
    twins, equal in every bit, are decided by their index)."""
    s, band, cand, twins = view["s"], view["band"], view["cand"], view["twins"]
    Q, N = s.shape
    order, _alone, _cut = separation(s, band, cand)
    n = torch.clamp(cand.sum(1), max=k)
    ref = order[:, :k].clone()
    if ref.shape[1] < k:
        ref = torch.cat([ref, torch.full((Q, k - ref.shape[1]), -1, dtype=torch.int64)], 1)
    ref[torch.arange(k)[None, :] >= n[:, None]] = -1
    c1, both = _without_later_twin(cand, twins)
    order1, _a, cut1 = separation(s, band, c1)
    kk = torch.full((Q,), k, dtype=torch.int64)
    if twins is not None:                                      # position of the twins' value in the order without the later twin
        pos = (order1 == twins[0]).double().argmax(1)
        kk = torch.where(both & (pos < k - 1), kk - 1, kk)
    kk = torch.clamp(kk, max=N)
    decisive = cut1.gather(1, kk[:, None])[:, 0] | (cand.sum(1) <= k)
    return ref, n, decisive


def rank_targets(c: RCase, per_row: int = 3):
    """Target pairs of dl_score_ranks chosen from the reference (original ids = the ids of the order as drawn): for the
    first 48 distinct query nodes up to `per_row` candidates whose band is disjoint from every other candidate's (first,
    middle, last of them: ties = 0), and for the first 16 of those nodes whose copy of the twins is separated from
    everything else both twins (ties = 1: the other twin).  -> src, dst, greater, ties (int64); none is left out."""
    v = rank_view(c)
    nodes, first = [], []
    for i, u in enumerate(v["queries"].tolist()):
        if u not in nodes:
            nodes.append(u)
            first.append(i)
    first = torch.tensor(first[:48])
    s, band, cand, twins = v["s"][first], v["band"][first], v["cand"][first], v["twins"]
    src, dst, greater, ties = [], [], [], []
    order, alone, _cut = separation(s, band, cand)
    for r, u in enumerate(v["queries"][first].tolist()):
        pos = torch.nonzero(alone[r])[:, 0].tolist()
        for j in sorted({pos[0], pos[len(pos) // 2], pos[-1]} if pos else ())[:per_row]:
            src.append(u); dst.append(int(order[r, j])); greater.append(j); ties.append(0)
    n_twin = 0
    if twins is not None:
        c1, both = _without_later_twin(cand, twins)
        order1, alone1, _c = separation(s, band, c1)
        for r, u in enumerate(v["queries"][first].tolist()):
            if not bool(both[r]) or n_twin >= 16:
                continue
            j = int((order1[r] == twins[0]).double().argmax())
            if bool(alone1[r, j]):
                for w in twins:
                    src.append(u); dst.append(w); greater.append(j); ties.append(1)
                n_twin += 1
    as_t = lambda x: torch.tensor(x, dtype=torch.int64)
    return as_t(src), as_t(dst), as_t(greater), as_t(ties), n_twin
