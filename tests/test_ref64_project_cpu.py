"""tests/ref64_project.py — the fp64 reference of the projection kernels — checked on the CPU: its gradients
against fp64 autograd of the module's own formula, its input builder against its own conditions, the case list against the
forms the library reports (host only), and the plain fp32 evaluation against the reference on every case:
ref64_project.ORACLE records those figures, and the kernels' bounds are 4x them plus the analytic three-plane term."""
import functools

import pytest
import torch

import ref64
import ref64_project as rp

SLACK = ref64.CPU_SLACK              # for re-measuring on this host; the GPU bounds do not contain it


def _shapes():
    seen = []
    for c in rp.cases():
        key = (c.N, c.F, c.K, c.nhid, c.d)
        if key not in seen:
            seen.append(key)
    return seen


def test_reference_gradients_equal_fp64_autograd_of_the_module():
    """Factor2 / Factor as torch modules would compute them (Linear -> ReLU -> Linear per factor), float64 autograd."""
    for key in ((129, 8, 1, 63, 32), (300, 33, 3, 0, 32)):
        r = rp.reference(*key)
        two = r["W2"] is not None
        params = [r[k].double().requires_grad_(True) for k in (("W1", "b1", "W2", "b2") if two else ("W1", "b1"))]
        x = r["x"].double()
        Z = []
        for k in range(key[2]):
            h = torch.nn.functional.linear(x, params[0][k], params[1][k])
            Z.append(torch.nn.functional.linear(torch.relu(h), params[2][k], params[3][k]) if two else h)
        Z = torch.stack(Z, 1)
        assert float((Z.detach() - r["Z64"]).abs().max()) <= 1e-12 * float(r["Z64"].abs().max())
        grads = torch.autograd.grad((Z * r["dZ"].double()).sum(), params)
        for name, g in zip(("dW1", "db1", "dW2", "db2") if two else ("dW", "db"), grads):
            assert float((g - r[name + "64"]).abs().max()) <= 1e-12 * float(r[name + "64"].abs().max()), name


@pytest.mark.parametrize("key", _shapes(), ids=lambda k: "N{}-F{}-K{}-nhid{}-d{}".format(*k))
def test_builder_conditions_hold(key):
    """reference() asserts the decisive mask, the dead unit and finiteness itself; here: the marked rows are where they are
    said to be, mantissas are full, three planes hold every input exactly, and every plane is populated."""
    N, F, K, nhid, d = key
    r = rp.reference(*key)
    two = nhid > 0
    assert r["redraws"] <= rp.MAX_REDRAWS
    print(f"\nBUILDER {key} redraws={r['redraws']} zero_row={r['zero_row']} dead={r['dead']}")
    quiet, loud = rp.marked(N)
    assert 0 in quiet and (N - 1) in quiet + loud
    med = float(r["x"].abs().max(1).values.median()) if N > 8 else None
    if med:
        assert all(float(r["x"][i].abs().max()) < 2.0 ** -8 * med for i in quiet)
        assert all(float(r["x"][i].abs().max()) > 2.0 ** 8 * med for i in loud)
    if N >= 3:
        assert r["zero_row"] is not None and bool((r["x"][r["zero_row"]] == 0).all())
    if two and nhid >= 3:
        assert r["dead"] is not None and bool((r["hid64"][:, :, r["dead"]] == 0).all())
    if two:
        assert rp.MASK_MARGIN > rp.bound("hid", 1) * SLACK               # M lies above the widest bound on pre
        assert bool(((r["pre64"] > 0) == (r["hid32"] > 0)).all())
    for name in ("x", "W1", "b1", "W2", "b2", "dZ") + (("hid32",) if two else ()):
        v = r[name]
        if v is None:
            continue
        assert v.dtype == torch.float32 and rp.split3_exact(v), name
        hi, mid, lo = rp.split3(v)
        if v.numel() >= 64:
            nz = v != 0
            assert float((mid[nz] != 0).double().mean()) > 0.9 and float((lo[nz] != 0).double().mean()) > 0.9, name
    if two:                                                                # dhid, the operand kernel B splits
        dh = (torch.einsum("nkd,kdh->nkh", r["dZ"].double(), r["W2"].double()) * (r["pre64"] > 0)).float()
        assert rp.split3_exact(dh)


def test_three_plane_term_bounds_the_dropped_products():
    """PLANE against a direct evaluation: products of random fp32 pairs from the six kept plane products, in fp64."""
    g = torch.Generator().manual_seed(11)
    a = (torch.randn(1 << 16, generator=g, dtype=torch.float64) * torch.ldexp(torch.ones(1), torch.randint(-20, 20, (1 << 16,), generator=g))).float()
    b = torch.randn(1 << 16, generator=g, dtype=torch.float64).float()
    (ah, am, al), (bh, bm, bl) = [[p.double() for p in rp.split3(v)] for v in (a, b)]
    kept = am * bm + ah * bl + al * bh + ah * bm + am * bh + ah * bh
    worst = float(((kept - a.double() * b.double()).abs() / (ref64.U * (a.double() * b.double()).abs())).max())
    print(f"\nPLANE worst of 65536 random products: {worst:.3f} units (bound {rp.PLANE:.3f})")
    assert 0.1 < worst <= rp.PLANE


@functools.lru_cache(maxsize=None)
def _oracle_errors(key):
    r = rp.reference(*key)
    return rp.ratios(rp.fp32_evaluation(r), r)


@pytest.mark.parametrize("key", _shapes(), ids=lambda k: "N{}-F{}-K{}-nhid{}-d{}".format(*k))
def test_plain_fp32_stays_within_its_recorded_error(key):
    err = _oracle_errors(key)
    print("\nCALIBRATION", key, {k: f"{v:.3g}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= SLACK * rp.ORACLE[rp.oracle_key(k, key[0])], (k, v, rp.oracle_key(k, key[0]))


def test_recorded_oracle_errors_are_the_measured_maxima():
    worst = {}
    for key in _shapes():
        for k, v in _oracle_errors(key).items():
            worst[rp.oracle_key(k, key[0])] = max(v, worst.get(rp.oracle_key(k, key[0]), 0.0))
    print("\nORACLE measured", {k: f"{v:.3g}" for k, v in worst.items()})
    assert set(worst) == set(rp.ORACLE)
    for k, v in rp.ORACLE.items():
        assert v / SLACK <= worst[k] <= SLACK * v, (k, worst[k], v)


def test_case_list_reaches_every_projection_form(lib_env):
    """Every case reaches the form it was written for, and together they reach every reachable instantiation and launch
    mode: the library's own account of its dispatch (dl_project_fwd_form / dl_project_bwd_form) needs no device."""
    got = rp.check_coverage(lib_env)
    print("\nREACHED", {k: sorted(v, key=str) for k, v in got.items()})
