"""tests/ref64_sparse_project.py — the fp64 reference of the sparse projection kernels — checked on the CPU: the case list
against the forms the library reports (host only), the input builder against its own conditions, the plain fp32 evaluation
against the reference on every case (ref64_sparse_project.ORACLE records those figures; the kernels' bounds are 4x them plus
the analytic three-plane term), the same evaluation with one thing wrong against those bounds, and features.SparseFeatures."""
import functools

import numpy as np
import pytest
import torch

import ref64
import ref64_sparse_project as sp

SLACK = ref64.CPU_SLACK              # for re-measuring on this host; the GPU bounds do not contain it
CASES = sp.cases()
BY_NAME = {c.name: c for c in CASES}


def test_case_list_reaches_every_sparse_projection_form(lib_env):
    got = sp.check_coverage(lib_env)
    print("\nREACHED", {k: sorted(v, key=str) for k, v in got.items()})


@pytest.mark.parametrize("c", CASES, ids=sp.case_id)
def test_builder_conditions_hold(c):
    """reference() asserts the decisive mask, the dead unit and finiteness itself; here: the structure is what the case
    asks for, mantissas are full, and the dense matrix the companions are taken on is the formula's."""
    r = sp.reference(c)
    print(f"\nBUILDER {c.name} redraws={r['redraws']} nnz={r['col'].numel()} dead={r['dead']}")
    assert r["redraws"] <= sp.MAX_REDRAWS
    sf = sp.sparse_features(r)
    assert torch.equal(sf.to_dense(torch.float64), r["x64"])
    for i, cols in enumerate(r["rows"]):
        assert cols == sorted(set(cols)) and all(0 <= f < c.F for f in cols), i
    if c.copies:
        a, b = c.copies
        assert a // 128 != b // 128 and r["rows"][a] == r["rows"][b] and bool((r["x64"][a] == r["x64"][b]).all())
    if c.nhid > 0:
        assert sp.MASK_MARGIN > sp.bound("hid", sp.PLANE_PRODUCTS["fwd"]["hid"]) * SLACK     # M lies above the bound on pre
    for name in ("val", "scale", "shift", "W1", "W2", "dZ"):
        v = r[name]
        if v is None or v.numel() < 64:
            continue
        assert v.dtype == torch.float32
        low = (v.view(torch.int32) & 0xFF) != 0                           # the low mantissa byte is populated
        assert float(low.double().mean()) > 0.9, name


@functools.lru_cache(maxsize=None)
def _oracle_errors(name):
    c = BY_NAME[name]
    r = sp.reference(c)
    return sp.ratios(sp.fp32_evaluation(r, seg=c.seg or 512), r)


@pytest.mark.parametrize("c", CASES, ids=sp.case_id)
def test_plain_fp32_stays_within_its_recorded_error(c):
    err = _oracle_errors(c.name)
    print("\nCALIBRATION", c.name, {k: f"{v:.3g}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= SLACK * sp.ORACLE[k], (k, v)


def test_recorded_oracle_errors_are_the_measured_maxima():
    worst = {}
    for c in CASES:
        for k, v in _oracle_errors(c.name).items():
            worst[k] = max(v, worst.get(k, 0.0))
    print("\nORACLE measured", {k: f"{v:.3g}" for k, v in worst.items()})
    assert set(worst) == set(sp.ORACLE)
    for k, v in sp.ORACLE.items():
        assert v / SLACK <= worst[k] <= SLACK * v, (k, worst[k], v)


# the fp32 evaluation with one thing wrong -> the cases that catch it (each leaves the bound of at least one output)
MUTATION_CASES = {
    "drop_last_entry": ("d32-val-scale-N63-F5-nhid63", "one-layer-d128-binary-N63-F1-K3"),
    "csum_first_128": ("d128-affine-val-emptycol-copies-N300-F300-K3-nhid257",),
    "scale_on_shift": ("d64-affine-fullcol-seg50-N129-F33-K3-nhid129", "one-layer-d32-affine-N300-F33-K3"),
    "g_only_nonempty": ("d64-shift-only-vec-N129-F33-nhid64", "one-layer-d32-affine-N300-F33-K3"),
    "drop_last_segment": ("d64-affine-fullcol-seg50-N129-F33-K3-nhid129", "one-layer-d128-val-fullcol-seg50-N129-F300"),
}


@pytest.mark.parametrize("mutation", sp.MUTATIONS)
def test_a_wrong_evaluation_leaves_its_bound(mutation):
    assert set(MUTATION_CASES) == set(sp.MUTATIONS)
    for name in MUTATION_CASES[mutation]:
        c = BY_NAME[name]
        r = sp.reference(c)
        err = sp.ratios(sp.fp32_evaluation(r, mutate=mutation, seg=c.seg or 512), r)
        planes = {**sp.PLANE_PRODUCTS["fwd"], **sp.PLANE_PRODUCTS["bwd"], "pre": 0}
        out = {k: v for k, v in err.items() if v > sp.bound(k, planes[k])}
        print(f"\nMUTATION {mutation} on {name}: outside", {k: f"{v:.3g}" for k, v in out.items()})
        assert out, (mutation, name, err)


# ---------------------------------------------------------------------------------------------- features.SparseFeatures
def _binary(N=37, F=23, seed=3):
    rng = np.random.default_rng(seed)
    x = (rng.random((N, F)) < 0.2).astype(np.float32)
    x[4] = 0.0                                                            # an empty row
    x[:, 7] = 0.0                                                         # a column without entries
    return x


def test_from_dense_to_dense_returns_the_input_exactly():
    from disenlink_amd.features import SparseFeatures
    x = _binary()
    sf = SparseFeatures.from_dense(x)
    assert sf.val is None and sf.scale is None and sf.shift is None and sf.shape == x.shape and sf.nnz == int(x.sum())
    assert torch.equal(sf.to_dense(), torch.from_numpy(x))
    y = x * np.random.default_rng(5).standard_normal(x.shape).astype(np.float32)
    sv = SparseFeatures.from_dense(y)
    assert sv.val is not None and torch.equal(sv.to_dense(), torch.from_numpy(y))
    rows, cols = np.nonzero(y)
    perm = np.random.default_rng(6).permutation(rows.size)
    sc = SparseFeatures.from_coo(rows[perm], cols[perm], y.shape, values=y[rows, cols][perm])
    assert torch.equal(sc.to_dense(), torch.from_numpy(y))


def test_standardise_agrees_with_standardise_rows_to_fp32_rounding():
    from disenlink_amd import datasets
    from disenlink_amd.features import SparseFeatures
    x = _binary()
    x[4, 3] = 1.0                                                         # no constant row here
    sf = SparseFeatures.from_dense(x, standardise=True)
    want = datasets.standardise_rows(x)
    got = sf.to_dense().numpy()
    # scale, shift and the dense form are each rounded a few times: a few units of 2^-24 of the row's largest magnitude
    tol = 8 * 2.0 ** -24 * np.abs(want).max(axis=1, keepdims=True)
    assert np.all(np.abs(got - want) <= tol)
    x[9] = 0.0                                                            # a constant row: NaN, as the dense form gives
    assert np.isnan(datasets.standardise_rows(x)[9]).all()
    assert bool(torch.isnan(SparseFeatures.from_dense(x, standardise=True).to_dense()[9]).all())


def test_csc_view_lists_every_entry_once_rows_ascending():
    from disenlink_amd.features import SparseFeatures
    x = _binary()
    sf = SparseFeatures.from_dense(x)
    colptr, crow, centry = sf.colptr.long(), sf.csc_row.long(), sf.csc_entry.long()
    assert sorted(centry.tolist()) == list(range(sf.nnz))
    row_of = torch.repeat_interleave(torch.arange(x.shape[0]), (sf.rowptr[1:] - sf.rowptr[:-1]).long())
    assert torch.equal(row_of[centry], crow)
    for f in range(x.shape[1]):
        seg = crow[colptr[f]:colptr[f + 1]]
        assert bool((sf.col.long()[centry[colptr[f]:colptr[f + 1]]] == f).all())
        assert bool((seg[1:] > seg[:-1]).all())
    assert sf.max_col_len == int(x.sum(0).max())
    colseg, seg_col = sf.seg_plan(3)
    lens = (colptr[1:] - colptr[:-1])
    assert torch.equal((colseg[1:] - colseg[:-1]).long(), (lens + 2) // 3)
    assert torch.equal(seg_col.long(), torch.repeat_interleave(torch.arange(x.shape[1]), (lens + 2) // 3))


def test_builder_refuses_unsorted_or_duplicate_columns():
    from disenlink_amd.features import SparseFeatures
    SparseFeatures.from_csr([0, 2, 2, 3], [1, 4, 0], (3, 5))
    for col in ([4, 1, 0], [1, 1, 0]):
        with pytest.raises(ValueError):
            SparseFeatures.from_csr([0, 2, 2, 3], col, (3, 5))
    with pytest.raises(ValueError):
        SparseFeatures.from_coo([0, 0], [2, 2], (3, 5))
    with pytest.raises(ValueError):
        SparseFeatures.from_csr([0, 1], [5], (1, 5))


@pytest.mark.parametrize("nhid", [1, 6])
def test_cpu_sparse_features_through_the_module_equal_the_dense_cpu_branch(nhid):
    from disenlink_amd.features import SparseFeatures
    from disenlink_amd.model import Disentangle
    x = _binary()
    x[4, 3] = 1.0
    sf = SparseFeatures.from_dense(x, standardise=True)
    torch.manual_seed(0)
    model = Disentangle(x.shape[1], nhid, 8, nfactor=3, beta=0.9)
    assert torch.equal(model.project(sf), model.project(sf.to_dense()))
    from disenlink_amd import ops
    assert ops.padded_features(sf) is sf and ops.xplanes_for(sf) is None
