"""Plain float64 reference of the projection of SPARSE features (disenlink_amd/features.py; model.py:13-15, 24-27 fanned out
over K factors), the inputs it is run on and the list of cases that reaches every compiled form of the sparse kernels
(csrc/dl_project_sparse.hip).  TEST INFRASTRUCTURE: torch, float64, CPU.  The sibling of tests/ref64_project.py.

The features are x~[i,f] = scale[i] X[i,f] + shift[i] with X a CSR; the reference is ref64_project.forward64 / backward64
on x~ formed in float64 from the float32 components.  The companions belong to the formula AS IT IS EVALUATED — the split
form gets no credit for a cancellation between scale * val and shift:

  pre_abs  = |scale_i| sum_nz |val| |W1| + |shift_i| sum_f |W1| + |b1|                      (>= the dense companion)
  dW1_abs  = sum_e |scale_i val_e| dhid_abs + sum_i |shift_i| dhid_abs                      (single layer: dhid_abs = |dZ|)
  Z_abs, dhid_abs, db1_abs, dW2_abs, db2_abs: carried through as in ref64_project.

ORACLE holds the largest band_ratio a plain fp32 evaluation of the same formula (fp32_evaluation: the entries of a row / of
a column in ascending order, chains tiled by 128 terms and the tile sums added in order, csum and g tiled the same way)
shows against this reference over all cases, measured and re-asserted by tests/test_ref64_sparse_project_cpu.py.  The bound
of a kernel's output is 4x that figure plus ref64_project.PLANE per three-plane product on the way to the output
(PLANE_PRODUCTS below, from the forms the library launches).  No bound comes from a kernel.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import torch

import ref64_project as rp
from ref64 import F64, U, band_ratio

# Largest error of the plain fp32 evaluation over all cases, in units of 2^-24 * companion (three significant digits).
# Single layer: Z1, dW, db.
ORACLE = {
    "pre": 3.25, "Z": 8.90, "dW1": 12.4, "db1": 2.27, "dW2": 6.60, "db2": 2.19,
    "Z1": 3.15, "dW": 11.7, "db": 2.08,
}
PLANE = rp.PLANE
MASK_MARGIN = rp.MASK_MARGIN
MAX_REDRAWS = rp.MAX_REDRAWS
POSITIONS = rp.POSITIONS

# Three-plane products between the exactly rounded inputs and each output (csrc/dl_project_sparse.hip): layer 1 is an fp32
# fma chain (sparse_l1_fwd_kernel), layer 2 contracts the kept hidden layer with W2 from three bf16 planes per operand
# (sparse_l2_fwd_kernel: mfma_split6) — one product on the way to Z; the single layer has no layer 2.  The backward runs
# kernel A of dl_project_bwd.hip in its kept fp32-MFMA form (PLANES = false) and fp32 fma chains for dW1 and g: none.
PLANE_PRODUCTS = {
    "fwd": {"hid": 0, "Z": 1, "Z1": 0},
    "bwd": {"dW1": 0, "db1": 0, "dW2": 0, "db2": 0, "dW": 0, "db": 0},
}
_JUDGED_BY = {"Z1": ("Z", "Z", "Z1"), "hid": ("hid", "pre", "pre")}      # output -> (reference, companion, ORACLE key)


def bound(key: str, plane_products: int = 0) -> float:
    return 4.0 * ORACLE[_JUDGED_BY.get(key, (key,) * 3)[2]] + plane_products * PLANE


# -------------------------------------------------------------------------------------------------- the cases
# val / scale / shift: given (True) or None.  full_col: column F-1 holds every node; empty_col: column F // 2 has no entry;
# nnz0: no entry at all; copies: rows (a, b) in different 128-row tiles are exact copies; seg: DL_SPARSE_SEG of the case.
# expect: the form the case was written for = (chunks, last_chunk_cols, affine, max_segments, two_layer, width, vec).
SCase = namedtuple("SCase", "name N F K nhid d val scale shift full_col empty_col nnz0 copies seg expect")


def _c(name, N, F, K, nhid, d, val=False, scale=False, shift=False, full_col=False, empty_col=False, nnz0=False, copies=None,
       seg=None, expect=None):
    return SCase(name, N, F, K, nhid, d, val, scale, shift, full_col, empty_col, nnz0, copies, seg, expect)


def cases():
    """Smallest shapes at which the kernels can go wrong: N in {1, 63, 129, 300}, F in {1, 5, 33, 300}, K in {1, 3}, nhid in
    {0 (single layer), 2, 63, 64, 129, 257}, d in {32, 64, 128}; rows of 0, 1, 7, 8, 9 and F entries (ROW_PATTERN)."""
    return [
        _c("d32-binary-N1-F1-nhid2", 1, 1, 1, 2, 32, expect=(1, 4, 0, 1, 1, 32, 0)),
        _c("d32-val-scale-N63-F5-nhid63", 63, 5, 1, 63, 32, val=True, scale=True, expect=(1, 64, 0, 1, 1, 32, 0)),
        _c("d64-affine-fullcol-seg50-N129-F33-K3-nhid129", 129, 33, 3, 129, 64, scale=True, shift=True, full_col=True, seg=50,
           expect=(2, 132, 1, 3, 1, 64, 0)),
        _c("d128-affine-val-emptycol-copies-N300-F300-K3-nhid257", 300, 300, 3, 257, 128, val=True, scale=True, shift=True,
           empty_col=True, copies=(5, 133), expect=(4, 4, 1, 1, 1, 128, 0)),
        _c("d64-shift-only-vec-N129-F33-nhid64", 129, 33, 1, 64, 64, shift=True, empty_col=True, expect=(1, 64, 1, 1, 1, 64, 1)),
        _c("d128-scale-only-N129-F5-nhid2", 129, 5, 1, 2, 128, scale=True, copies=(1, 128), expect=(1, 4, 0, 1, 1, 128, 0)),
        _c("d32-nnz0-affine-N63-F5-K3-nhid2", 63, 5, 3, 2, 32, scale=True, shift=True, nnz0=True, expect=(1, 8, 1, 0, 1, 32, 0)),
        _c("one-layer-d32-affine-N300-F33-K3", 300, 33, 3, 0, 32, scale=True, shift=True, empty_col=True, copies=(5, 133),
           expect=(1, 96, 1, 1, 0, 0, 1)),
        _c("one-layer-d128-val-fullcol-seg50-N129-F300", 129, 300, 1, 0, 128, val=True, full_col=True, seg=50,
           expect=(1, 128, 0, 3, 0, 0, 1)),
        _c("one-layer-d128-binary-N63-F1-K3", 63, 1, 3, 0, 128, expect=(2, 128, 0, 1, 0, 0, 1)),
        _c("one-layer-d64-binary-N1-F5", 1, 5, 1, 0, 64, expect=(1, 64, 0, 1, 0, 0, 1)),
    ]


def case_id(c: SCase) -> str:
    return c.name


ROW_PATTERN = (1, 0, 7, 8, 9, -1, 2, 3)              # entries of row i: ROW_PATTERN[i % 8], -1 = every column (a full row)


def structure(c: SCase, gen):
    """-> list of N ascending column lists."""
    ec = c.F // 2 if (c.empty_col and c.F >= 2) else None
    allowed = [f for f in range(c.F) if f != ec]
    rows = []
    for i in range(c.N):
        L = ROW_PATTERN[i % len(ROW_PATTERN)]
        L = 0 if c.nnz0 else min(len(allowed), c.F if L < 0 else L)
        cols = sorted(allowed[int(p)] for p in torch.randperm(len(allowed), generator=gen)[:L])
        if c.full_col and not c.nnz0 and (c.F - 1) not in cols:
            cols = sorted(cols + [c.F - 1])
        rows.append(cols)
    if c.copies:
        rows[c.copies[1]] = list(rows[c.copies[0]])
    return rows


def _pow2(gen, n, lo=-2, hi=3):
    return torch.ldexp(torch.ones(n, dtype=F64), torch.randint(lo, hi, (n,), generator=gen))


def dense_X(r, dtype=F64):
    """X [N, F] (the CSR without scale / shift) in `dtype`."""
    N, F = r["shape"]
    X = torch.zeros(N, F, dtype=dtype)
    X[r["row_of"], r["col"].long()] = 1.0 if r["val"] is None else r["val"].to(dtype)
    return X


def dense_x64(r):
    """x~ in float64 from the float32 components: the features the reference is run on."""
    X = dense_X(r)
    if r["scale"] is not None:
        X = r["scale"].double()[:, None] * X
    if r["shift"] is not None:
        X = X + r["shift"].double()[:, None]
    return X


def companions64(r, X64, W1, b1, W2, b2, dZ):
    """The companions of the module docstring (float64)."""
    N, F = r["shape"]
    sa = torch.ones(N, dtype=F64) if r["scale"] is None else r["scale"].double().abs()
    ha = torch.zeros(N, dtype=F64) if r["shift"] is None else r["shift"].double().abs()
    Xa = sa[:, None] * dense_X(r).abs()                                  # |scale_i val_e| on the entries
    Wa, ga = W1.abs(), dZ.abs()
    pre_abs = torch.einsum("nf,khf->nkh", Xa, Wa) + ha[:, None, None] * Wa.sum(2) + b1.abs()
    if W2 is None:
        return {"Z": pre_abs, "dW": torch.einsum("nkd,nf->kdf", ga, Xa) + (ha[:, None, None] * ga).sum(0)[:, :, None],
                "db": ga.sum(0)}
    on = (torch.einsum("nf,khf->nkh", X64, W1) + b1) > 0
    live = pre_abs * on
    dhid_abs = torch.einsum("nkd,kdh->nkh", ga, W2.abs()) * on
    return {"pre": pre_abs, "Z": torch.einsum("nkh,kdh->nkd", live, W2.abs()) + b2.abs(),
            "dW1": torch.einsum("nkh,nf->khf", dhid_abs, Xa) + (ha[:, None, None] * dhid_abs).sum(0)[:, :, None],
            "db1": dhid_abs.sum(0), "dW2": torch.einsum("nkd,nkh->kdh", ga, live), "db2": ga.sum(0)}


@functools.lru_cache(maxsize=None)
def reference(c: SCase):
    """Inputs of one case and everything the fp64 reference says about them: a dict of CPU tensors; rowptr, col (int32), val,
    scale, shift, W1, b1, W2, b2, dZ are what the kernels are handed (float32), the rest float64.

    Values: normal deviates times per-feature powers of two (val, W1: per feature; W2: per hidden unit; dZ: per output
    column), rounded to fp32: full 24-bit mantissas.  Rows `marked` quiet / loud are scaled by 2^-12 / 2^+12: node rows
    (through scale where it is given, else through val where it is given), hidden units of W1 (and b1), output columns of
    W2 (and b2); one hidden unit is dead (W1 row 0, b1 < 0).  Asserted on the reference alone: everything finite in fp32 and,
    after at most MAX_REDRAWS passes of redrawing the rows concerned (their values; their scale and shift; else their
    columns), every |pre| > MASK_MARGIN * 2^-24 * pre_abs."""
    N, F, K, nhid, d = c.N, c.F, c.K, c.nhid, c.d
    two = nhid > 0
    M = nhid if two else d
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) + 100003 * N + 1009 * F
    gen = torch.Generator().manual_seed(seed)
    rows = structure(c, gen)
    sx, sw = _pow2(gen, F), _pow2(gen, F)
    mark = torch.ones(N, dtype=F64)
    q, l = rp.marked(N)
    mark[q], mark[l] = 2.0 ** -12, 2.0 ** 12
    if c.copies:
        mark[c.copies[1]] = mark[c.copies[0]]
    mark_val = c.val and not c.scale                                     # where the node marks go

    def draw_val(i):
        v = torch.randn(len(rows[i]), generator=gen, dtype=F64) * sx[rows[i]]
        return (v * mark[i] if mark_val else v).float()

    def draw_affine(i):
        return (float((0.5 + torch.rand((), generator=gen, dtype=F64)) * mark[i]),
                float(torch.randn((), generator=gen, dtype=F64) * 0.25 * mark[i]))

    vals = [draw_val(i) for i in range(N)] if c.val else None
    aff = [draw_affine(i) for i in range(N)] if (c.scale or c.shift) else None
    unit = torch.ones(M, dtype=F64)
    q, l = rp.marked(M)
    unit[q], unit[l] = 2.0 ** -12, 2.0 ** 12
    fan = max(1.0, min(F, 8) ** 0.5)
    W1 = torch.randn(K, M, F, generator=gen, dtype=F64) * sw / fan * unit[:, None]
    b1 = torch.randn(K, M, generator=gen, dtype=F64) * 0.5 * unit
    dead = rp._first_unmarked(M) if two else None
    if dead is not None:
        W1[:, dead] = 0.0
        b1[:, dead] = -b1[:, dead].abs() - 0.125
    W1, b1 = W1.float(), b1.float()
    W2 = b2 = None
    if two:
        colm = torch.ones(d, dtype=F64)
        q, l = rp.marked(d)
        colm[q], colm[l] = 2.0 ** -12, 2.0 ** 12
        W2 = (torch.randn(K, d, nhid, generator=gen, dtype=F64) * _pow2(gen, nhid) / nhid ** 0.5 * colm[:, None]).float()
        b2 = (torch.randn(K, d, generator=gen, dtype=F64) * colm).float()
    dZ = (torch.randn(N, K, d, generator=gen, dtype=F64) * _pow2(gen, d)).float()

    def assemble():
        if c.copies:
            a, b = c.copies
            rows[b] = list(rows[a])
            if vals is not None:
                vals[b] = vals[a].clone()
            if aff is not None:
                aff[b] = aff[a]
        lens = torch.tensor([len(x) for x in rows], dtype=torch.int64)
        rowptr = torch.zeros(N + 1, dtype=torch.int64)
        rowptr[1:] = lens.cumsum(0)
        col = torch.tensor([f for x in rows for f in x], dtype=torch.int32)
        r = dict(shape=(N, F), rowptr=rowptr.to(torch.int32), col=col, row_of=torch.repeat_interleave(torch.arange(N), lens),
                 val=torch.cat(vals) if vals is not None else None,
                 scale=torch.tensor([a[0] for a in aff], dtype=torch.float32) if c.scale else None,
                 shift=torch.tensor([a[1] for a in aff], dtype=torch.float32) if c.shift else None)
        return r

    redraws = 0
    while True:
        r = assemble()
        X64 = dense_x64(r)
        pre = torch.einsum("nf,khf->nkh", X64, W1.double()) + b1.double()
        comp = companions64(r, X64, W1.double(), b1.double(), W2.double() if two else None, b2.double() if two else None, dZ.double())
        if not two:
            break
        close = (pre.abs() <= MASK_MARGIN * U * comp["pre"]).flatten(1).any(1)
        if not bool(close.any()):
            break
        redraws += 1
        assert redraws <= MAX_REDRAWS, f"the ReLU mask of {c.name} stays undecided on {int(close.sum())} nodes"
        for i in [int(i) for i in close.nonzero().flatten()]:
            if vals is not None and len(rows[i]):
                vals[i] = draw_val(i)
            elif aff is not None:
                aff[i] = draw_affine(i)
            else:
                ec = c.F // 2 if (c.empty_col and c.F >= 2) else None
                allowed = [f for f in range(F) if f != ec]
                assert 0 < len(rows[i]) < len(allowed), f"{c.name}: row {i} cannot be redrawn"
                rows[i] = sorted(allowed[int(p)] for p in torch.randperm(len(allowed), generator=gen)[:len(rows[i])])
    P = [W1.double(), b1.double(), W2.double() if two else None, b2.double() if two else None]
    r.update(W1=W1, b1=b1, W2=W2, b2=b2, dZ=dZ, redraws=redraws, dead=dead, rows=[list(x) for x in rows], x64=X64)
    fwd = rp.forward64(X64, *P)
    bwd = rp.backward64(X64, P[0], P[1], P[2], dZ.double())
    r.update({k + "64": v for k, v in {**fwd, **bwd}.items()})
    r.update({k + "_abs": v for k, v in comp.items()})
    if two:
        assert bool((fwd["pre"].abs() > MASK_MARGIN * U * r["pre_abs"]).all())
        assert dead is None or bool((fwd["pre"][:, :, dead] < 0).all())
        r["hid32"] = fwd["hid"].float()                                   # what the kept backward is handed
        assert torch.equal(r["hid32"] > 0, fwd["pre"] > 0)
        kept = rp.backward64(X64, P[0], P[1], P[2], dZ.double(), hid=r["hid32"].double())
        r.update({k + "64_kept": v for k, v in kept.items()})
    for k, v in r.items():
        if torch.is_tensor(v) and v.dtype == F64:
            assert bool(torch.isfinite(v.float()).all()), k
    return r


def sparse_features(r, device="cpu"):
    """The SparseFeatures the kernels are handed for reference r."""
    from disenlink_amd.features import SparseFeatures
    return SparseFeatures.from_csr(r["rowptr"], r["col"], r["shape"], values=r["val"], scale=r["scale"], shift=r["shift"]).to(device)


# -------------------------------------------------------------------------------------------------- plain fp32
MUTATIONS = ("drop_last_entry", "csum_first_128", "scale_on_shift", "g_only_nonempty", "drop_last_segment")


def _padded(lists, pad_index=0):
    """lists of indices -> (index [n, L] int64 padded with pad_index, mask [n, L] float32 1 / 0)."""
    L = max([len(x) for x in lists] + [1])
    idx = torch.full((len(lists), L), pad_index, dtype=torch.int64)
    msk = torch.zeros(len(lists), L, dtype=torch.float32)
    for i, x in enumerate(lists):
        idx[i, :len(x)] = torch.tensor(x, dtype=torch.int64)
        msk[i, :len(x)] = 1.0
    return idx, msk


def fp32_evaluation(r, mutate: str | None = None, seg: int = 512):
    """The plain fp32 evaluation the ORACLE figures are measured on: the formula of the module docstring on the float32
    inputs, the entries of a row (forward) / of a column (dW1) in ascending order, every chain tiled by 128 terms with the
    tile sums added in order (ref64_project._chain), csum over the features and g over the nodes tiled the same way.
    mutate: one of MUTATIONS — the same evaluation with one thing wrong (tests/test_ref64_sparse_project_cpu.py)."""
    assert mutate is None or mutate in MUTATIONS
    f32 = torch.float32
    N, F = r["shape"]
    W1, b1, W2, b2, dZ = (r[k] for k in ("W1", "b1", "W2", "b2", "dZ"))
    K, M = W1.shape[:2]
    d = dZ.shape[2]
    two = W2 is not None
    rows = [list(x) for x in r["rows"]]
    rowptr = r["rowptr"].long()
    val = r["val"] if r["val"] is not None else torch.ones(r["col"].numel(), dtype=f32)
    row_vals = [val[int(rowptr[i]):int(rowptr[i + 1])] for i in range(N)]
    fwd_rows, fwd_vals = rows, row_vals
    if mutate == "drop_last_entry":
        fwd_rows, fwd_vals = [x[:-1] for x in rows], [v[:-1] for v in row_vals]
    cidx, cmask = _padded(fwd_rows)
    vpad = torch.zeros_like(cmask)
    for i, v in enumerate(fwd_vals):
        vpad[i, :len(v)] = v
    W1T = W1.permute(2, 0, 1).contiguous()                               # [F, K, M]
    acc = rp._chain(cidx.shape[1], lambda j: vpad[:, j, None, None] * W1T[cidx[:, j]], torch.empty(N, K, M, dtype=f32))
    pre = acc if r["scale"] is None else r["scale"][:, None, None] * acc
    if r["shift"] is not None:
        Fc = min(F, 128) if mutate == "csum_first_128" else F
        csum = rp._chain(Fc, lambda f: W1[:, :, f], torch.empty(K, M, dtype=f32))
        term = r["shift"][:, None, None] * csum
        if mutate == "scale_on_shift":
            term = r["scale"][:, None, None] * term
        pre = pre + term
    pre = pre + b1
    out = {}
    if two:
        assert mutate is not None or torch.equal(pre > 0, r["pre64"] > 0)          # decisive: the mask is the reference's
        hid = pre.clamp_min(0)
        out["pre"] = pre
        out["Z"] = rp._chain(M, lambda h: hid[:, :, None, h] * W2[None, :, :, h], torch.empty(N, K, d, dtype=f32)) + b2
        mask = r["pre64"] > 0
        Y = rp._chain(d, lambda cc: dZ[:, :, cc, None] * W2[None, :, cc, :], pre) * mask
        hid_b = r["hid32"]
        out["dW2"] = rp._chain(N, lambda n: dZ[n, :, :, None] * hid_b[n, :, None, :], W2)
        out["db1"] = rp._chain(N, lambda n: Y[n], b1)
        out["db2"] = rp._chain(N, lambda n: dZ[n], b2)
    else:
        out["Z1"] = pre
        Y = dZ
        out["db"] = rp._chain(N, lambda n: dZ[n], b1)
    # dW1[k, m, f] = sum over the entries of column f, rows ascending, of (scale_i val_e) Y[i, k, m]  (+ g[k, m])
    col_rows = [[] for _ in range(F)]
    col_w = [[] for _ in range(F)]
    for i in range(N):
        for j, f in enumerate(rows[i]):
            w = row_vals[i][j]
            if r["scale"] is not None:
                w = r["scale"][i] * w                                     # one fp32 rounding, as the kernel forms it
            col_rows[f].append(i)
            col_w[f].append(float(w))
    if mutate == "drop_last_segment":
        for f in range(F):
            n = len(col_rows[f])
            if n > seg:
                keep = (n - 1) // seg * seg
                col_rows[f], col_w[f] = col_rows[f][:keep], col_w[f][:keep]
    ridx, _m = _padded(col_rows)
    wpad = torch.zeros(F, ridx.shape[1], dtype=f32)
    for f, w in enumerate(col_w):
        wpad[f, :len(w)] = torch.tensor(w, dtype=f32)
    Yt = Y.permute(1, 2, 0).contiguous()                                 # [K, M, N]
    dW = rp._chain(ridx.shape[1], lambda j: wpad[None, None, :, j] * Yt[:, :, ridx[:, j]], torch.empty(K, M, F, dtype=f32))
    if r["shift"] is not None:
        g = rp._chain(N, lambda n: r["shift"][n] * Y[n], torch.empty(K, M, dtype=f32))
        if mutate == "g_only_nonempty":
            nonempty = torch.tensor([len(x) > 0 for x in col_rows])
            dW = dW + g[:, :, None] * nonempty
        else:
            dW = dW + g[:, :, None]
    out["dW1" if two else "dW"] = dW
    return out


def ratios(got: dict, r, suffix: str = "64_kept") -> dict:
    """band_ratio of every output in `got` against the reference r (suffix "64_kept": the gradients from hid32); a kept
    hidden layer is judged in the band of pre (the mask is decisive)."""
    out = {}
    for k, v in got.items():
        ref, comp, _key = _JUDGED_BY.get(k, (k, k, k))
        out[k] = band_ratio(v, r[ref + suffix] if (ref + suffix) in r else r[ref + "64"], r[comp + "_abs"])
    return out


# -------------------------------------------------------------------------------------------------- the census
def max_col_len(r) -> int:
    F = r["shape"][1]
    return int(torch.bincount(r["col"].long(), minlength=F).max()) if r["col"].numel() else 0


def form(c: SCase, lib_env):
    """The launch decisions the library reports for case c under the case's DL_SPARSE_SEG."""
    from disenlink_amd import _lib
    if c.seg is not None:
        lib_env("DL_SPARSE_SEG", c.seg)
    r = reference(c)
    out = _lib.project_sparse_form(c.N, c.F, c.K, max(c.nhid, 1), c.d, c.nhid > 0, c.shift, max_col_len(r))
    if c.seg is not None:
        lib_env("DL_SPARSE_SEG")
    return out


def check_expected(c: SCase, f: dict):
    got = tuple(f[k] for k in ("chunks", "last_chunk_cols", "affine", "max_segments", "two_layer", "width", "vec"))
    assert got == c.expect, (c.name, got, c.expect)
    assert f["seg_len"] == (c.seg or 512)
    assert (f["g_ranges"] > 0) == bool(c.shift)


def reached(all_forms: dict) -> dict:
    out = {k: set() for k in ("l1", "l2", "A", "seg", "modes")}
    for c, f in all_forms.items():
        r = reference(c)
        out["l1"].add(f["two_layer"])                                    # sparse_l1_fwd_kernel<TWO>
        if f["two_layer"]:
            out["l2"].add(f["width"])                                    # sparse_l2_fwd_kernel<D>
            out["A"].add(f["width"])                                     # project2_bwd_hidden_f32_kernel<D, true, false, false>
        if r["col"].numel():
            out["seg"].add(f["vec"])                                     # sparse_dw1_seg_kernel<VEC>
        m = out["modes"]
        m.add("affine" if f["affine"] else "no affine")
        m.add("two layer" if f["two_layer"] else "single layer")
        m.add(f"chunks {f['chunks']}")
        if f["last_chunk_cols"] < 256:
            m.add("ragged last chunk")
        if f["max_segments"] > 1:
            m.add("several segments")
            if max_col_len(r) % f["seg_len"]:
                m.add("ragged last segment")
        if f["max_segments"] == 1:
            m.add("one segment")
        if f["max_segments"] == 0:
            m.add("no entries")
        m.add("val given" if c.val else "val None")
        m.add(f"scale {'given' if c.scale else 'None'}, shift {'given' if c.shift else 'None'}")
        lens = {len(x) for x in r["rows"]}
        m.update(f"row of {n}" for n in (0, 1, 7, 8, 9) if n in lens)
        if c.F in lens and c.F > 1:
            m.add("full row")
        counts = torch.bincount(r["col"].long(), minlength=c.F)
        if r["col"].numel() and int(counts.min()) == 0:
            m.add("column without entries")
        if r["col"].numel() and int(counts.max()) == c.N:
            m.add("column that holds every node")
        if c.copies and c.copies[0] // 128 != c.copies[1] // 128:
            m.add("copied rows in different tiles")
        if f["sA"] > 1:
            m.add("slab sum of dW2 / db1")
    return out


def required() -> dict:
    return {
        "l1": {0, 1}, "l2": {32, 64, 128}, "A": {32, 64, 128}, "seg": {0, 1},
        "modes": {"affine", "no affine", "two layer", "single layer", "chunks 1", "chunks 2", "chunks 4", "ragged last chunk",
                  "several segments", "ragged last segment", "one segment", "no entries", "val given", "val None",
                  "scale None, shift None", "scale given, shift None", "scale None, shift given", "scale given, shift given",
                  "row of 0", "row of 1", "row of 7", "row of 8", "row of 9", "full row", "column without entries",
                  "column that holds every node", "copied rows in different tiles"},
    }


def check_coverage(lib_env):
    from disenlink_amd import _lib
    # a new entry of the form (a new template argument, a new launch decision) needs a case and a line here first
    assert _lib.PROJECT_SPARSE_FORM == ("chunks", "last_chunk_cols", "affine", "max_segments", "seg_len", "two_layer", "width",
                                        "vec", "sA", "g_ranges")
    cs = cases()
    assert len({c.name for c in cs}) == len(cs)
    all_forms = {c: form(c, lib_env) for c in cs}
    for c, f in all_forms.items():
        check_expected(c, f)
    got, want = reached(all_forms), required()
    for k in want:
        assert got[k] >= want[k], (k, "not reached by any case:", sorted(want[k] - got[k], key=str))
    for name, ns in (("N", {1, 63, 129, 300}), ("F", {1, 5, 33, 300}), ("K", {1, 3}), ("nhid", {0, 2, 63, 129, 257}), ("d", {32, 64, 128})):
        assert {getattr(c, name) for c in cs} >= ns, name
    return got
