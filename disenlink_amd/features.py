"""Sparse feature input of the projection: ``SparseFeatures`` represents

    x~[i, f] = scale[i] * X[i, f] + shift[i]

with X a CSR (``rowptr`` int32 [N+1], ``col`` int32 [nnz] strictly ascending within a row, ``val`` fp32 [nnz] or None = all
ones) and ``scale`` / ``shift`` fp32 [N] or None (1 / 0).  Binary features are X alone; binary features that were row
standardised (main_disentangled.py:99: two values per row) are X with scale = 1/sigma_i and shift = -mu_i/sigma_i.  The
formula above — not any dense matrix the object was made from — defines the features: ``to_dense`` evaluates it.

The object also holds the CSC view of X (``colptr`` [F+1], and per entry its row and its CSR entry index, rows ascending
within a column), built once at construction: x is data and never changes during a run.  ``Disentangle.project`` hands a
CUDA ``SparseFeatures`` to dl_project_sparse_fwd / _bwd (ops.Project); a CPU one goes through ``to_dense``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


class SparseFeatures:
    is_sparse_features = True
    dtype = torch.float32

    def __init__(self, rowptr, col, val, scale, shift, shape, _csc=None):
        N, F = int(shape[0]), int(shape[1])
        self.shape = (N, F)
        self.rowptr = torch.as_tensor(rowptr).to(torch.int32).contiguous()
        self.col = torch.as_tensor(col).to(torch.int32).contiguous()
        self.val = None if val is None else torch.as_tensor(val).to(torch.float32).contiguous()
        self.scale = None if scale is None else torch.as_tensor(scale).to(torch.float32).contiguous()
        self.shift = None if shift is None else torch.as_tensor(shift).to(torch.float32).contiguous()
        if _csc is None:
            self._validate()
            _csc = self._build_csc()
        self.colptr, self.csc_row, self.csc_entry, self.max_col_len = _csc
        self._plans: dict = {}                                  # seg_len -> (colseg, seg_col, struct)

    # ------------------------------------------------------------------ construction
    def _validate(self):
        N, F = self.shape
        rp, col = self.rowptr.cpu().numpy().astype(np.int64), self.col.cpu().numpy().astype(np.int64)
        if N < 0 or F < 1:
            raise ValueError(f"bad shape {self.shape}")
        if rp.shape != (N + 1,) or (N >= 0 and rp[0] != 0) or np.any(np.diff(rp) < 0) or rp[-1] != col.shape[0]:
            raise ValueError("rowptr must start at 0, not decrease and end at nnz")
        if col.size and (col.min() < 0 or col.max() >= F):
            raise ValueError("column index out of range")
        if col.size > 1:
            row_start = np.zeros(col.size, dtype=bool)
            row_start[rp[:-1][rp[:-1] < col.size]] = True
            if np.any((np.diff(col) <= 0) & ~row_start[1:]):
                raise ValueError("columns must be strictly ascending within a row (unsorted or duplicate entries)")
        if self.val is not None and self.val.shape != (col.shape[0],):
            raise ValueError("val must have one value per entry")
        for name in ("scale", "shift"):
            t = getattr(self, name)
            if t is not None and t.shape != (N,):
                raise ValueError(f"{name} must have one value per row")

    def _build_csc(self):
        N, F = self.shape
        rp, col = self.rowptr.cpu().numpy().astype(np.int64), self.col.cpu().numpy().astype(np.int64)
        row_of = np.repeat(np.arange(N, dtype=np.int64), np.diff(rp))
        order = np.argsort(col, kind="stable")                   # entries are row-ascending: stable keeps rows ascending
        counts = np.bincount(col, minlength=F)
        colptr = np.zeros(F + 1, dtype=np.int64)
        np.cumsum(counts, out=colptr[1:])
        dev = self.rowptr.device
        return (torch.from_numpy(colptr.astype(np.int32)).to(dev), torch.from_numpy(row_of[order].astype(np.int32)).to(dev),
                torch.from_numpy(order.astype(np.int32)).to(dev), int(counts.max()) if counts.size else 0)

    @classmethod
    def from_csr(cls, rowptr, col, shape, values=None, scale=None, shift=None) -> "SparseFeatures":
        return cls(rowptr, col, values, scale, shift, shape)

    @classmethod
    def from_coo(cls, rows, cols, shape, values=None, standardise: bool = False) -> "SparseFeatures":
        """Entries (rows[e], cols[e]) (value values[e], or 1) in any order; duplicates are refused.  standardise=True: the
        entries are the raw matrix and scale / shift standardise its rows (from_dense)."""
        N, F = int(shape[0]), int(shape[1])
        rows = np.asarray(torch.as_tensor(rows).cpu().numpy(), dtype=np.int64)
        cols = np.asarray(torch.as_tensor(cols).cpu().numpy(), dtype=np.int64)
        if rows.shape != cols.shape or rows.ndim != 1:
            raise ValueError("rows and cols must be vectors of one length")
        if rows.size and (rows.min() < 0 or rows.max() >= N):
            raise ValueError("row index out of range")
        order = np.lexsort((cols, rows))
        rows, cols = rows[order], cols[order]
        vals = None if values is None else np.asarray(torch.as_tensor(values).cpu().numpy(), dtype=np.float32)[order]
        rowptr = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=N), out=rowptr[1:])
        scale = shift = None
        if standardise:
            scale, shift = _standardising_affine(rowptr, vals, F)
        return cls(rowptr, cols, vals, scale, shift, (N, F))

    @classmethod
    def from_dense(cls, x, standardise: bool = False) -> "SparseFeatures":
        """The non-zero entries of a dense [N, F] matrix.  standardise=True: x is the RAW matrix and the object represents
        datasets.standardise_rows(x): scale = 1/sigma_i, shift = -mu_i/sigma_i with the mean and the unbiased std of row i,
        computed in float64 and rounded once (a constant row gives the NaNs the dense form gives)."""
        x = np.asarray(torch.as_tensor(x).cpu().numpy(), dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("x must be [N, F]")
        rows, cols = np.nonzero(x)                                # row-major order: rows ascending, columns ascending inside
        vals = x[rows, cols]
        return cls.from_coo(rows, cols, x.shape, None if bool(np.all(vals == 1.0)) else vals, standardise=standardise)

    # ------------------------------------------------------------------ what train.py / model.py ask of x
    @property
    def nnz(self) -> int:
        return int(self.col.shape[0])

    @property
    def device(self):
        return self.rowptr.device

    @property
    def is_cuda(self) -> bool:
        return self.rowptr.is_cuda

    def dim(self) -> int:
        return 2

    def _tensors(self):
        return (self.rowptr, self.col, self.val, self.scale, self.shift, self.colptr, self.csc_row, self.csc_entry)

    def to(self, device) -> "SparseFeatures":
        device = torch.device(device)
        if device == self.device:
            return self
        rp, col, val, sc, sh, cp, cr, ce = (None if t is None else t.to(device) for t in self._tensors())
        return SparseFeatures(rp, col, val, sc, sh, self.shape, _csc=(cp, cr, ce, self.max_col_len))

    def cuda(self, device=None) -> "SparseFeatures":
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))

    def cpu(self) -> "SparseFeatures":
        return self.to("cpu")

    def to_dense(self, dtype=torch.float32) -> torch.Tensor:
        """x~ evaluated in `dtype` from the stored fp32 components: scale * X + shift, one rounding per operation."""
        N, F = self.shape
        X = torch.zeros(N, F, dtype=dtype, device=self.device)
        rows = torch.repeat_interleave(torch.arange(N, device=self.device), (self.rowptr[1:] - self.rowptr[:-1]).long())
        X[rows, self.col.long()] = 1.0 if self.val is None else self.val.to(dtype)
        if self.scale is not None:
            X = self.scale.to(dtype)[:, None] * X
        if self.shift is not None:
            X = X + self.shift.to(dtype)[:, None]
        return X

    # ------------------------------------------------------------------ the C struct
    def seg_plan(self, seg_len: int):
        """(colseg [F+1], seg_col [n_seg]) int32 on this object's device: column f is cut into ceil(len_f / seg_len)
        segments of seg_len consecutive entries — a function of that column alone."""
        hit = self._plans.get(seg_len)
        if hit is None:
            cp = self.colptr.cpu().numpy().astype(np.int64)
            nseg = (np.diff(cp) + seg_len - 1) // seg_len
            colseg = np.zeros(cp.shape[0], dtype=np.int64)
            np.cumsum(nseg, out=colseg[1:])
            seg_col = np.repeat(np.arange(nseg.shape[0], dtype=np.int64), nseg)
            hit = (torch.from_numpy(colseg.astype(np.int32)).to(self.device),
                   torch.from_numpy(seg_col.astype(np.int32)).to(self.device), None)
            self._plans[seg_len] = hit
        return hit[0], hit[1]

    def c_struct(self):
        """byref(dl_sparse_features) for the library's current segment length (DL_SPARSE_SEG); the struct and the device
        arrays it points to live as long as this object."""
        seg_len = int(_lib.load().dl_sparse_seg_len())
        colseg, seg_col = self.seg_plan(seg_len)
        st = self._plans[seg_len][2]
        if st is None:
            p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
            st = _lib.DlSparseFeatures(self.shape[0], self.shape[1], self.nnz, p(self.rowptr), p(self.col), p(self.val),
                                       p(self.scale), p(self.shift), p(self.colptr), p(self.csc_row), p(self.csc_entry),
                                       seg_len, int(seg_col.numel()), p(colseg), p(seg_col))
            self._plans[seg_len] = (colseg, seg_col, st)
        return C.byref(st)

    def __repr__(self):
        return (f"SparseFeatures(shape={self.shape}, nnz={self.nnz}, val={'given' if self.val is not None else 'ones'}, "
                f"affine={self.shift is not None or self.scale is not None}, device={self.device})")


def _standardising_affine(rowptr, vals, F: int):
    """scale = 1/sigma, shift = -mu/sigma per row (fp32, rounded once from float64) of the matrix whose row i holds the
    entries vals[rowptr[i]:rowptr[i+1]] (None: ones) and zeros elsewhere: mean and UNBIASED std over the F columns, as
    datasets.standardise_rows takes them."""
    cnt = np.diff(rowptr).astype(np.float64)
    if vals is None:
        s1, s2 = cnt, cnt
    else:
        v = vals.astype(np.float64)
        csum = np.concatenate([[0.0], np.cumsum(v)])
        csum2 = np.concatenate([[0.0], np.cumsum(v * v)])
        s1, s2 = csum[rowptr[1:]] - csum[rowptr[:-1]], csum2[rowptr[1:]] - csum2[rowptr[:-1]]
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = s1 / F
        var = (s2 - F * mu * mu) / (F - 1)
        sigma = np.sqrt(np.maximum(var, 0.0))
        return (1.0 / sigma).astype(np.float32), (-mu / sigma).astype(np.float32)


def is_sparse(x) -> bool:
    return isinstance(x, SparseFeatures)
