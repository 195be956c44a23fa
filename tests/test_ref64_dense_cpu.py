"""tests/ref64_dense.py — the fp64 reference of the all-pairs scorer family — checked on the CPU: its backward against fp64
autograd of the formula, its input builder against its own conditions, the plain fp32 evaluation against the reference on
every case (ref64_dense.ORACLE records those figures; the kernels' bounds are 4x them plus the analytic three-plane term),
a CPU emulation of the three-plane scheme with all six products and with each removable product dropped, and the case
lists against the forms the library reports (host only)."""
import functools

import pytest
import torch

import ref64
import ref64_dense as rd
import ref64_project as rp

SLACK = ref64.CPU_SLACK              # for re-measuring on this host; the GPU bounds do not contain it


def _lib():
    from disenlink_amd import _lib
    return _lib.load()


def _fwd_shapes():
    seen = []
    for c in rd.dense_cases(_lib()):
        key = (c.N, c.K, c.d, c.t, c.dtype)
        if key not in seen:
            seen.append(key)
    return seen


def _bwd_cases():
    return rd.dense_bwd_cases()


def test_reference_backward_equals_fp64_autograd():
    for N, K, d, t in ((37, 3, 8, 2.0), (129, 1, 33, 2.0)):
        r = rd.reference(N, K, d, t)
        b = rd.backward_reference(N, K, d, t)["dense"]
        Z, H = r["Z"].double().requires_grad_(True), r["H"].double().requires_grad_(True)
        s = (torch.einsum("ukd,vkd->kuv", H, H) * torch.exp(torch.einsum("ukd,vkd->kuv", Z, Z) / t)).sum(0)
        assert float((s.detach() - r["s"]).abs().max()) <= 1e-12 * float(r["s"].abs().max())
        p = r["prob32"].double()
        dZ, dH = torch.autograd.grad((s * (b["g"].double() * p * (1 - p))).sum(), (Z, H))
        assert float((dZ - b["dZ"]).abs().max()) <= 1e-12 * float(b["dZ"].abs().max())
        assert float((dH - b["dH"]).abs().max()) <= 1e-12 * float(b["dH"].abs().max())


@pytest.mark.parametrize("N", [1, 37, 128, 129, 260, 300, 385, 1000])
def test_builder_conditions_hold(N):
    """reference() asserts finiteness, the exponent's range and the share of sensitive pairs itself; here: the marked rows,
    the zero row and the copies are where they are said to be, three planes hold every table exactly and are populated."""
    K, d = 3, 64
    Z, H = rd.tables(N, K, d)
    zero, copies = rd.special_rows(N)
    quiet, loud = rp.marked(N)
    for X, q_, l_ in ((Z, rd.Z_QUIET, rd.Z_LOUD), (H, rd.H_QUIET, rd.H_LOUD)):
        assert X.dtype == torch.float32 and rp.split3_exact(X)
        if N >= 37:
            med = float(X.abs().amax((1, 2)).median())
            assert all(float(X[i].abs().max()) < 4 * q_ * med for i in quiet) and all(float(X[i].abs().max()) > l_ * med / 4 for i in loud)
            assert bool((X[zero] == 0).all()) and torch.equal(X[copies[0]], X[copies[1]]) and copies[0] // 32 != copies[1] // 32
            _hi, mid, lo = rp.split3(X)
            nz = X != 0
            assert float((mid[nz] != 0).double().mean()) > 0.9 and float((lo[nz] != 0).double().mean()) > 0.9
    if N >= 131:
        assert copies[0] // 128 != copies[1] // 128
    g = rd.gradient(N, "dense")
    assert rp.split3_exact(g) and (N == 1 or bool((g < 0).any() and (g > 0).any()))
    zr, zc = rd.g_special(N)
    if zr is not None:
        assert bool((g[zr] == 0).all()) and bool((g[:, zc] == 0).all())
        assert torch.equal(g[copies[0]], g[copies[1]]) and torch.equal(g[:, copies[0]], g[:, copies[1]])


# ---------------------------------------------------------------------------------------------------- the oracle figures
@functools.lru_cache(maxsize=None)
def _forward_errors(key):
    N, K, d, t, dtype = key
    r = rd.reference(N, K, d, t, dtype)
    x, prob = rd.fp32_forward(r["Z"], r["H"], t)
    return {"logit": rd.ratios_forward(x, r), "prob_eps": float((prob.double() - torch.sigmoid(x.double())).abs().max()) / ref64.U}


@functools.lru_cache(maxsize=None)
def _backward_errors(c):
    f = rd.check_backward_form(c)
    r = rd.reference(c.N, c.K, c.d, c.t)
    ref = rd.backward_reference(c.N, c.K, c.d, c.t)
    out = {"dZ": 0.0, "dH": 0.0}
    kinds = rd.KINDS if c.N * c.K <= 2400 else ("dense",)              # the two long cases: the dense gradient only
    for kind in kinds:
        b = ref[kind]
        dZ, dH = rd.fp32_backward(r["Z"], r["H"], c.t, r["prob32"], b["g"], rd.slice_tiles(c.N, f["nslice"]))
        out["dZ"] = max(out["dZ"], ref64.band_ratio(dZ, b["dZ"], b["dZ_abs"]))
        out["dH"] = max(out["dH"], ref64.band_ratio(dH, b["dH"], b["dH_abs"]))
    return out


@pytest.mark.parametrize("key", _fwd_shapes(), ids=lambda k: "N{}-K{}-d{}-t{:g}-{}".format(*k))
def test_plain_fp32_forward_stays_within_its_recorded_error(key):
    err = _forward_errors(key)
    print("\nCALIBRATION forward", key, {k: f"{v:.3g}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= SLACK * rd.ORACLE[k], (k, v)


@pytest.mark.parametrize("case", _bwd_cases(), ids=rd.case_id)
def test_plain_fp32_backward_stays_within_its_recorded_error(case):
    err = _backward_errors(case)
    print("\nCALIBRATION backward", case.name, {k: f"{v:.3g}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= SLACK * rd.ORACLE[k], (k, v)


def test_recorded_oracle_errors_are_the_measured_maxima():
    worst = {}
    for errs in [_forward_errors(k) for k in _fwd_shapes()] + [_backward_errors(c) for c in _bwd_cases()]:
        for k, v in errs.items():
            worst[k] = max(v, worst.get(k, 0.0))
    print("\nORACLE measured", {k: f"{v:.3g}" for k, v in worst.items()})
    assert set(worst) == set(rd.ORACLE)
    for k, v in rd.ORACLE.items():
        assert v / SLACK <= worst[k] <= SLACK * v, (k, worst[k], v)


# ---------------------------------------------------------------------------------------------------- the plane scheme
def _mfma_cases():
    return [c for c in rd.dense_cases(_lib()) if c.kernel == "matrix cores"]


@pytest.mark.parametrize("case", _mfma_cases(), ids=rd.case_id)
def test_plane_scheme_with_all_six_products_stays_inside_the_forward_bounds(case):
    r = rd.reference(case.N, case.K, case.d, case.t)
    x = rd.planes_forward(r["Z"], r["H"], case.t)
    got = rd.ratios_forward(x, r)
    pr = rd.prob_ratio(rd.sigmoid32(x.double()), r, True)
    print(f"\nEMULATION {case.name}: logit {got:.3g} (bound {rd.bound('logit'):.4g}), prob / band {pr:.3g}")
    assert got <= rd.bound("logit") and pr <= 1.0


def _planes_backward(c, kind, **drop):
    f = rd.check_backward_form(c)
    r = rd.reference(c.N, c.K, c.d, c.t)
    b = rd.backward_reference(c.N, c.K, c.d, c.t)[kind]
    dZ, dH = rd.planes_backward(r["Z"], r["H"], c.t, r["prob32"], b["g"], rd.slice_tiles(c.N, f["nslice"]), **drop)
    return ref64.band_ratio(dZ, b["dZ"], b["dZ_abs"]), ref64.band_ratio(dH, b["dH"], b["dH_abs"])


@pytest.mark.parametrize("case", _bwd_cases(), ids=rd.case_id)
def test_plane_scheme_with_all_six_products_stays_inside_the_backward_bounds(case):
    for kind in (rd.KINDS if case.N * case.K <= 2400 else ("dense",)):
        eZ, eH = _planes_backward(case, kind)
        print(f"\nEMULATION {case.name} {kind}: dZ {eZ:.3g} (bound {rd.bound('dZ'):.4g}), dH {eH:.3g} (bound {rd.bound('dH'):.4g})")
        assert eZ <= rd.bound("dZ") and eH <= rd.bound("dH")


# the case that catches each removed product, per output (a removal every listed case lets through fails here: change the
# inputs then, not the bound)
CATCHES_FORWARD = "mfma-N260-K3-d32-t0.5"
CATCHES_GRAM, CATCHES_SECOND = "N129-K1-d8-t1", "N128-K8-d32-t1"


@pytest.mark.parametrize("drop", rd.REMOVABLE, ids=lambda p: rd.NAMES[p])
def test_each_removed_product_exceeds_a_bound(drop):
    c = next(c for c in _mfma_cases() if c.name == CATCHES_FORWARD)
    r = rd.reference(c.N, c.K, c.d, c.t)
    got = rd.ratios_forward(rd.planes_forward(r["Z"], r["H"], c.t, drop=drop), r)
    print(f"\nREMOVED {rd.NAMES[drop]} from the Gram products, {c.name}: logit {got:.3g} (bound {rd.bound('logit'):.4g})")
    assert got > rd.bound("logit")
    # the backward: from its Gram products (S and Q feed dZ's weight whole, dH's only through E: judged on dZ), and from the
    # second products (both outputs)
    b = next(c for c in _bwd_cases() if c.name == CATCHES_GRAM)
    eZ, eH = _planes_backward(b, "dense", drop_gram=drop)
    print(f"REMOVED {rd.NAMES[drop]} from the backward's Gram products, {b.name}: dZ {eZ:.3g} (bound {rd.bound('dZ'):.4g}), dH {eH:.3g}")
    assert eZ > rd.bound("dZ")
    b = next(c for c in _bwd_cases() if c.name == CATCHES_SECOND)
    eZ, eH = _planes_backward(b, "dense", drop_second=drop)
    print(f"REMOVED {rd.NAMES[drop]} from the second products, {b.name}: dZ {eZ:.3g} (bound {rd.bound('dZ'):.4g}), dH {eH:.3g} (bound {rd.bound('dH'):.4g})")
    assert eZ > rd.bound("dZ") and eH > rd.bound("dH")


# ---------------------------------------------------------------------------------------------------- the forms
def test_case_list_reaches_every_allpairs_form(lib_env):
    from disenlink_amd import _lib
    lib = _lib.load()
    assert _lib.SCORE_ALLPAIRS_FWD_FORM == ("kernel", "items", "grid", "n_slices", "slice_w", "chunks_per_u")
    assert _lib.SCORE_ALLPAIRS_KERNELS == rd.KERNELS
    assert _lib.SCORE_ALLPAIRS_BWD_DENSE_FORM == ("Np", "NCB", "nslice", "min_tiles", "max_tiles")
    cs = rd.dense_cases(lib)
    assert len({c.name for c in cs}) == len(cs)
    got = set()
    per_shape = {}
    for c in cs:
        f = rd.check_forward_form(c)
        if c.kernel == "matrix cores":
            nt = -(-c.N // 128)
            got |= {"planes", "split on stage", "diagonal tile"}       # check_forward_form: both PLANES forms of every case
            if nt > 1:
                got.add("off-diagonal tile, vector mirrored store" if c.N % 4 == 0 else "off-diagonal tile, scalar mirrored store")
            if f["items"] > 256:
                got.add("more than 256 items")
        elif c.kernel == "per shape":
            per_shape.setdefault((c.dtype, c.K, c.d), set()).add((f["n_slices"], f["chunks_per_u"]))
        else:
            got.add("generic forced" if c.force_generic else "generic")
    want = {"planes", "split on stage", "diagonal tile", "off-diagonal tile, vector mirrored store",
            "off-diagonal tile, scalar mirrored store", "more than 256 items", "generic", "generic forced"}
    assert got >= want, sorted(want - got)
    tuned = {(dt, K, d) for dt in ("f32", "bf16") for K, d in ref64.tuned_shapes(lib, dt) if dt == "bf16" or d % 32 != 0}
    assert set(per_shape) == tuned and tuned, sorted(tuned - set(per_shape))
    for key, forms in per_shape.items():
        assert forms >= {(1, 1), (8, 1)}, (key, forms)
    for dt in ("f32", "bf16"):
        assert any((8, 2) in forms for key, forms in per_shape.items() if key[0] == dt), dt
    bs = rd.dense_bwd_cases()
    assert len({c.name for c in bs}) == len(bs)
    reached = {(f["NCB"], f["slicing"]) for f in (rd.check_backward_form(c) for c in bs)}
    assert {n for n, _s in reached} == {1, 2, 3, 4}
    assert {s for _n, s in reached} == {"one tile per slice", "ragged", "unsliced"}
    for s in ("ragged", "unsliced"):
        assert {n for n, ss in reached if ss == s} >= {1, 4}
    rs = rd.rank_cases()
    assert len({c.name for c in rs}) == len(rs)
    assert _lib.SCORE_TOPK_FORM == ("nd", "qtiles", "slices", "tiles_per_slice", "last_tiles", "cap")
    scan = set()
    for c in rs:
        for k in rd.TOPK:
            for forced in (None,) + c.slices:
                f = rd.rank_form(c, k, lib_env, forced)
                scan |= {f"{f['qtiles']} query tiles", f"nd {f['nd']}", f"cap {f['cap']}"}
                if forced == 1 and f["tiles_per_slice"] > 1:
                    scan.add("one slice over several tiles")
                if f["slices"] > 1 and f["tiles_per_slice"] == 1:
                    scan.add("one tile per slice")
                if f["slices"] > 1 and f["last_tiles"] < f["tiles_per_slice"]:
                    scan.add("ragged last slice")
        if c.orders:                                        # under its coarsest forced slicing an ordered case compacts a FULL
            for k in rd.TOPK:                               # list (k sorted keys + 64 new ones) at least once: k + 128 columns
                f = rd.rank_form(c, k, lib_env, min(c.slices))
                assert f["tiles_per_slice"] * 128 >= k + 128, (c.name, k, f)
            scan.add("permuted orders under several tiles per slice")
        if c.exclusion:
            scan.add("exclusion")
    want = {"1 query tiles", "2 query tiles", "3 query tiles", "nd 1", "nd 2", "nd 4", "one slice over several tiles",
            "one tile per slice", "ragged last slice", "permuted orders under several tiles per slice", "exclusion"} | {f"cap {k + 64}" for k in rd.TOPK}
    assert scan >= want, sorted(want - scan)
    assert {c.d for c in rs} == {1, 8, 31, 32, 33, 48, 64, 100, 128} and {c.K for c in rs} == {1, 3, 8}
    assert {c.N for c in rs} == {1, 37, 128, 129, 300, 1000} and {c.Q for c in rs} == {1, 16, 128, 129, 300}
    f = rd.rank_form(next(c for c in rs if c.N == 1000), 64, lib_env, 3)
    assert (f["slices"], f["tiles_per_slice"], f["last_tiles"]) == (3, 3, 2)
    print("\nREACHED", sorted(got), sorted(reached), sorted(scan))


# ---------------------------------------------------------------------------------------------------- ranking
@pytest.mark.parametrize("case", rd.rank_cases(), ids=rd.case_id)
def test_ranking_cases_are_decisive(case):
    """From the reference alone: for every order and k at most a tenth of the query rows leave the top-k set to the bands;
    every rank target is separated from every other candidate by more than the sum of their bands, the twins from
    everything but each other; none is left out."""
    c = case
    for order in (rd.ORDERS if c.orders else rd.ORDERS[:1]):
        v = rd.rank_view(c, order)
        assert torch.equal(torch.sort(v["perm"]).values, torch.arange(c.N))
        for k in rd.TOPK:
            ref, n, decisive = rd.topk_expectation(v, k)
            undecided = 1.0 - float(decisive.double().mean())
            print(f"\nDECISIVE {c.name} {order} k={k}: {undecided:.3f} of the rows undecided")
            assert undecided <= rd.MAX_UNDECIDED
            assert bool(((ref >= 0).sum(1) == n).all())
    v = rd.rank_view(c)
    if c.orders:                                            # the pivot query's row is ascending / descending in the node index
        i = min(c.Q - 1, 7)
        for order, sign in (("ascending", 1.0), ("descending", -1.0)):
            w = rd.rank_view(c, order)
            row = w["s"][i]
            assert bool((sign * (row[1:] - row[:-1]) >= 0).all())
    src, dst, greater, ties, n_twin = rd.rank_targets(c)
    print(f"TARGETS {c.name}: {src.numel()} targets, {n_twin} query nodes aimed at the twins")
    if c.N >= 37:
        assert src.numel() >= 16 and n_twin >= 4 and int((ties == 1).sum()) == 2 * n_twin
        row_of = {int(u): i for i, u in reversed(list(enumerate(v["queries"].tolist())))}
        for u, w, g, ti in zip(src.tolist(), dst.tolist(), greater.tolist(), ties.tolist()):
            i = row_of[u]
            others = v["cand"][i].clone()
            others[w] = False
            if ti:
                others[list(v["twins"])] = False
            gap = (v["s"][i] - v["s"][i, w]).abs() - v["band"][i] - v["band"][i, w]
            assert bool((gap[others] > 0).all())
            assert g == int(((v["s"][i] > v["s"][i, w]) & others).sum())
    if c.exclusion:
        k63 = rd.topk_expectation(v, 63)[1]
        assert int(k63.min()) < 63                             # a row left with fewer than k candidates
