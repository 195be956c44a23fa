"""fp64 / numpy statements of the two contracts of the scans between two node sets, shared by tests/test_between_cpu.py
and tests/test_gpu_between.py:

* the RECTANGLE (ops.score_mine_between / score_links_between): every pair (a, b) of rows of A against rows of B is a
  candidate — there is no a < b — unless excluded, forbidden by the rule, NaN or below the floor; the order is larger logit
  first, equal logits by a * nB + b; the link graph is the CSR of the A side and of the B side;
* the BLOCKED scans (ops.score_mine_blocks / score_links_blocks / score_link_degrees_blocks): the contract of
  ops.score_mine / score_links on GLOBAL ids, whatever the blocks (mine_ref.select_top, links_ref.select_links).

``FakeScans`` stands in for the C library: it answers the entries the blocked drivers and the rectangular scans make from a
matrix of logits, with these very selections, so that the drivers run without a GPU."""
import ctypes as C

import numpy as np
import torch

import links_ref
import mine_ref


def logits64(ZA, HA, ZB, HB, t):
    """fp64 s(a, b) = sum_k (hA_k[a].hB_k[b]) exp(zA_k[a].zB_k[b] / t) [nA, nB] and mine_ref.logits64's error band."""
    za, ha, zb, hb = ZA.double(), HA.double(), ZB.double(), HB.double()
    zz = torch.einsum("qkd,nkd->qnk", za, zb)
    hh = torch.einsum("qkd,nkd->qnk", ha, hb)
    zabs = torch.einsum("qkd,nkd->qnk", za.abs(), zb.abs())
    habs = torch.einsum("qkd,nkd->qnk", ha.abs(), hb.abs())
    e = torch.exp(zz / t)
    return (hh * e).sum(-1), 1e-5 * (e * (habs + hh.abs() * zabs / t)).sum(-1)


def eligible(S, excluded=None, allowed=None, min_logit=-np.inf):
    """bool [nA, nB]: not excluded, allowed, not NaN, at or above the floor (-0 reaches a floor of 0)."""
    ok = ~torch.isnan(S) & (S >= min_logit)
    if excluded is not None:
        ok &= ~excluded.to(S.device).bool()
    if allowed is not None:
        ok &= allowed.to(S.device).bool()
    return ok


def select_top_between(S, m, excluded=None, allowed=None, min_logit=-np.inf):
    """-> (src, dst, logit): the first m eligible pairs of S [nA, nB], larger logit first (-0 as +0), equal logits by
    a * nB + b, the smaller first."""
    a, b = torch.nonzero(eligible(S, excluded, allowed, min_logit), as_tuple=True)      # ascending a * nB + b
    val = S[a, b]
    val = torch.where(val == 0, torch.zeros_like(val), val)
    order = torch.sort(val, descending=True, stable=True).indices[:m]
    return a[order], b[order], val[order]


def select_links_between(S, excluded=None, allowed=None, min_logit=-np.inf):
    """-> (ab, ba), each (rowptr int64, col int64, logit): every eligible pair in the CSR of the A side (columns b,
    ascending) and of the B side (columns a, ascending), a -0 reported as +0."""
    ok = eligible(S, excluded, allowed, min_logit)
    val = torch.where(S == 0, torch.zeros_like(S), S)
    out = []
    for mask, v in ((ok, val), (ok.T, val.T)):
        rows, cols = torch.nonzero(mask, as_tuple=True)
        rowptr = torch.zeros(mask.shape[0] + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=mask.shape[0]), dim=0)
        out.append((rowptr, cols, v[rows, cols]))
    return tuple(out)


def rule_mask(groups_a, groups_b, allow):
    """bool [nA, nB]: allow[groups_a[a], groups_b[b]]."""
    return torch.as_tensor(allow).bool()[torch.as_tensor(groups_a).long()[:, None], torch.as_tensor(groups_b).long()[None, :]]


# ---------------------------------------------------------------------- the library's stand-in for the blocked drivers
def _view(ptr, n, ctype):
    """n elements of ``ctype`` at the address ``ptr`` as a tensor that shares the memory (nothing for n = 0)"""
    if n == 0 or not ptr:
        return torch.from_numpy(np.zeros(0, dtype=np.ctypeslib.as_array((ctype * 1)()).dtype))
    return torch.from_numpy(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)))


def _i32(ptr, n):
    return _view(ptr, n, C.c_int32)


def _u8(ptr, n):
    return _view(ptr, n, C.c_uint8)


def _i64(ptr, n):
    return _view(ptr, n, C.c_int64)


def _f32(ptr, n):
    return _view(ptr, n, C.c_float)


class FakeScans:
    """Stands for the loaded library over CPU tensors.  ``S`` is the [N, N] matrix of logits of ONE graph whose fp32 table
    Z [N, 1, 1] holds the node's own id: an entry finds the rows it was given by reading its table pointers, takes its
    logits from S (the smaller endpoint's row, as the scans do) and writes what the kernels would — the selections above —
    into the caller's buffers.  Every call is noted in ``calls`` (name, args)."""

    def __init__(self, S):
        self.S, self.calls = S, []

    def ids(self, ptr, n):
        return _f32(ptr, n).long()

    def mask(self, exr, exc, rows, cols):
        if exr is None:
            return None
        rp = _i32(exr, rows + 1).long()
        out = torch.zeros(rows, cols, dtype=torch.bool)
        r = torch.repeat_interleave(torch.arange(rows), rp[1:] - rp[:-1])
        c = _i32(exc, int(rp[-1])).long()
        assert bool(((c >= 0) & (c < cols)).all())
        for i in range(rows):
            seg = c[int(rp[i]):int(rp[i + 1])]
            assert bool((seg[1:] > seg[:-1]).all()), "columns strictly ascending"
        out[r, c] = True
        return out

    def allow(self, nf, nA, nB):
        if nf is None:
            return None
        st = nf._obj
        words = _i64(st.allow, st.n_groups)
        table = torch.tensor([[(int(w) >> h) & 1 for h in range(st.n_groups)] for w in words.tolist()], dtype=torch.bool)
        if hasattr(st, "group_a"):
            return rule_mask(_u8(st.group_a, nA), _u8(st.group_b, nB), table)
        g = _u8(st.group, nA)
        return rule_mask(g, g, table)

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return getattr(self, "_" + name)(*args) if hasattr(type(self), "_" + name) else (1 if name.endswith("_supported") else 0)
        return fn

    # sizers: anything positive
    def _dl_score_mine_workspace_bytes_dtype(self, *a): return 4096
    def _dl_score_links_workspace_bytes_dtype(self, *a): return 4096
    def _dl_score_mine_between_workspace_bytes_dtype(self, *a): return 4096
    def _dl_score_links_between_workspace_bytes_dtype(self, *a): return 4096

    def _write_top(self, a, b, val, m, src, dst, logit, prob, count):
        c = int(a.numel())
        _i64(count, 1)[0] = c
        _i32(src, m)[:c], _i32(dst, m)[:c] = a.int(), b.int()
        _f32(logit, m)[:c], _f32(prob, m)[:c] = val.float(), torch.sigmoid(val.float())

    def _dl_score_mine_dtype(self, Z, H, N, K, d, dt, t, exr, exc, floor, m, src, dst, logit, prob, count, ws, wsb, st, nf):
        ids = self.ids(Z, N)
        ex = self.mask(exr, exc, N, N)
        ok = None if nf is None else self.allow(nf, N, N)
        if ok is not None:
            ex = ~ok if ex is None else (ex | ~ok)
        a, b, val = mine_ref.select_top(self.S[ids][:, ids], m, None if ex is None else (ex | ex.T), floor)
        val = torch.where(val == 0, torch.zeros_like(val), val)
        self._write_top(a, b, val, m, src, dst, logit, prob, count)
        return 0

    def _dl_score_mine_between_dtype(self, ZA, HA, nA, ZB, HB, nB, K, d, dt, t, exr, exc, floor, m, src, dst, logit, prob, count,
                                     ws, wsb, st, nf):
        S = self.S[self.ids(ZA, nA)][:, self.ids(ZB, nB)]
        a, b, val = select_top_between(S, m, self.mask(exr, exc, nA, nB), self.allow(nf, nA, nB), floor)
        self._write_top(a, b, val, m, src, dst, logit, prob, count)
        return 0

    def _dl_score_links_count_dtype(self, Z, H, N, K, d, dt, t, exr, exc, floor, nf, ws, wsb, rowptr, st):
        ids = self.ids(Z, N)
        ex = self.mask(exr, exc, N, N)
        ok = None if nf is None else self.allow(nf, N, N)
        if ok is not None:
            ex = ~ok if ex is None else (ex | ~ok)
        self.diag = links_ref.select_links(self.S[ids][:, ids], ex, floor)
        _i64(rowptr, N + 1)[:] = self.diag[0]
        return 0

    def _dl_score_links_fill_dtype(self, Z, H, N, K, d, dt, t, exr, exc, floor, nf, ws, wsb, rowptr, nnz, col, logit, prob, st):
        _, c, v = self.diag
        assert nnz == c.numel()
        _i32(col, nnz)[:], _f32(logit, nnz)[:], _f32(prob, nnz)[:] = c.int(), v.float(), torch.sigmoid(v.float())
        return 0

    def _dl_score_links_between_count_dtype(self, ZA, HA, nA, ZB, HB, nB, K, d, dt, t, exr, exc, floor, nf, ws, wsb, rpa, rpb, st):
        S = self.S[self.ids(ZA, nA)][:, self.ids(ZB, nB)]
        self.rect = select_links_between(S, self.mask(exr, exc, nA, nB), self.allow(nf, nA, nB), floor)
        _i64(rpa, nA + 1)[:], _i64(rpb, nB + 1)[:] = self.rect[0][0], self.rect[1][0]
        return 0

    def _dl_score_links_between_fill_dtype(self, ZA, HA, nA, ZB, HB, nB, K, d, dt, t, exr, exc, floor, nf, ws, wsb, rpa, rpb,
                                           nnz_a, col_a, logit_a, prob_a, nnz_b, col_b, logit_b, prob_b, st):
        for (_, c, v), nnz, col, logit, prob in ((self.rect[0], nnz_a, col_a, logit_a, prob_a),
                                                 (self.rect[1], nnz_b, col_b, logit_b, prob_b)):
            assert nnz == c.numel()
            _i32(col, nnz)[:], _f32(logit, nnz)[:], _f32(prob, nnz)[:] = c.int(), v.float(), torch.sigmoid(v.float())
        return 0
