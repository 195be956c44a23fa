"""Every compiled form of the projection kernels (project2_fwd_planes_kernel<D> and project2_fwd_f32_kernel<D, VEC> with their
slab sum, project1_fwd_kernel<D>, project2_bwd_hidden_planes_kernel<D> and project2_bwd_hidden_f32_kernel<D, VEC, RECOMPUTE,
PLANES_OUT>, the node contractions on planes / fp32 vector / fp32 scalar, the slab
and column sums) against the plain fp64 reference of tests/ref64_project.py, per element, on the case list of
ref64_project.cases(): the smallest shapes that reach each instantiation and launch mode, which the library itself confirms
for every case before anything runs (dl_project_fwd_form / dl_project_bwd_form; tests/test_ref64_project_cpu.py asserts
that the list reaches all of them).

Each call is handed exactly rounded inputs of the reference: full-mantissa x, W1, b1, W2, b2, dZ with quiet (2^-12) and
loud (2^+12) node rows, hidden units and output columns at tile positions, a zero row, a dead hidden unit and a ReLU mask
that is decisive by construction; the backward from the kept hidden layer gets the REFERENCE's hid cast to fp32, in the
library's hidT [K][nhid][ld] layout with NaN in the padding columns.  No kernel's error leaks into the check of the next.

Per case: Z; the kept hid without its padding; Z once more through dl_project_fwd WITHOUT a workspace (cases marked
"nows"); the four gradients from the recomputed and from the kept hidden layer (one layer: dW, db); every output bit for
bit on a second call; Z the same bits with and without keep_hid; forward node blocks the same bits as one block;
persistent x / x^T planes the same bits as the per-call split (cases marked "xplanes"); one_allocation False / True the
same values (cases marked "one_alloc").  DL_POISON=1 (conftest.py) turns anything read but never written into NaN, and a
NaN fails its assertion.

Bounds.  Per element, c * 2^-24 * (absolute-sum companion), c = 4x the figure the plain fp32 evaluation of
ref64_project.fp32_evaluation shows against the reference over these same cases (ref64_project.ORACLE, re-asserted on
the CPU on every run) plus, where products are formed from three bf16 planes, PLANE = 2 + 2^-8 units per plane product
between the inputs and the output (ref64_project.PLANE_PRODUCTS; derived in ref64_project's docstring from dl_tiles.h).
None was set from what the kernels give.

    output            oracle (worst of 20 shapes)   bound fp32 (4x)   bound on planes      kernels on an MI355X
    hid (band of pre) 7.27                          29.08             + 1 PLANE = 31.09    (still to record, see below)
    Z                 11.3                          45.2              + 2 PLANE = 49.21
    dW1               18.4                          73.6              + 1 / 2 PLANE (recompute / kept)
    db1               9.14                          36.56             + 0 / 1 PLANE
    dW2               12.4                          49.6              + 0 / 1 PLANE
    db2               2.43                          9.72              —
    one layer Z       5.54                          22.16             —
    one layer dW, db  13.3, 1.84                    53.2, 7.36        —
    N = 4229 (node-blocked backward) dW1, db1, dW2, db2:  7.84, 0.245, 6.50, 0.191  ->  31.36, 0.98, 26.0, 0.764 (+ PLANE as above)

Every figure of a run is printed as a FIGURE line before anything is asserted (pytest -s).  Still to record: the kernels'
column (one run, for the record; no bound is to be taken from it), the FIGURE lines under profiles/, and the runs under
three arithmetic-only mutations — a dropped mid*mid product in layer 1, the layer-2 bias added in the slab path as well as
in z_slab_sum_kernel, >= 0 in kernel A's ReLU mask — with the cases that catch each and by what factor.
"""
import pytest
import torch

import ref64_project as rp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _valid_hid(hid, N, K, nhid):
    """hidT [K][nhid][ld] (flat) -> [N, K, nhid] without the padding columns."""
    ld = (N + 3) // 4 * 4
    return hid.view(K, nhid, ld)[:, :, :N].permute(2, 0, 1)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", rp.cases(), ids=rp.case_id)
def test_projection_kernels_match_fp64(case, lib_env, monkeypatch):
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    c = case
    N, K, nhid, d = c.N, c.K, c.nhid, c.d
    two = nhid > 0
    r = rp.reference(N, c.F, K, nhid, d)
    form = rp.forms(c, lib_env)
    rp.check_expected(c, form)                          # the case still reaches the form it was written for
    monkeypatch.setenv("DL_X_PLANES", "0")              # per-call split, except where the case asks for persistent planes
    for name, value in c.env:
        lib_env(name, value)
    figures = []                                        # (what, observed, bound): all printed, then all asserted

    def note(what, got, suffix, plane_products):
        for k, v in rp.ratios({kk: vv.cpu() for kk, vv in got.items()}, r, suffix).items():
            figures.append((f"{what} {k}", float(v), rp.bound(k, plane_products.get(k, 0), N)))

    def exact(what, ok):
        figures.append((what, 0.0 if ok else float("inf"), 0.0))

    x, W1, b1, dZ = (r[k].to(DEV) for k in ("x", "W1", "b1", "dZ"))
    W2, b2 = (r["W2"].to(DEV), r["b2"].to(DEV)) if two else (None, None)
    none = dict.fromkeys(("hid", "Z", "dW1", "db1", "dW2", "db2"), 0)

    # ---- forward
    if two:
        pp = rp.PLANE_PRODUCTS["fwd"] if form["fwd"]["split"] else none
        Z, hid = ops.project_fwd(x, W1, b1, W2, b2, pad=c.pad, keep_hid=True)
        H = _valid_hid(hid, N, K, nhid)
        note("forward", {"Z": Z, "hid": H}, "64", pp)
        exact("forward hid > 0 exactly where pre64 > 0", torch.equal(H.cpu() > 0, r["pre64"] > 0))
        Z2, hid2 = ops.project_fwd(x, W1, b1, W2, b2, pad=c.pad, keep_hid=True)
        exact("forward bitwise repeatable", torch.equal(Z, Z2) and torch.equal(H, _valid_hid(hid2, N, K, nhid)))
        exact("forward Z the same bits without keep_hid", torch.equal(Z, ops.project_fwd(x, W1, b1, W2, b2, pad=c.pad)))
        if form["fwd"]["launches"] > 1:                 # documented: node blocks give the bits of one block
            lib_env("DL_FWD_BLOCK_ROWS")
            Z1, hid1 = ops.project_fwd(x, W1, b1, W2, b2, pad=c.pad, keep_hid=True)
            exact("forward node blocks == one block, Z and hid", torch.equal(Z, Z1) and torch.equal(H, _valid_hid(hid1, N, K, nhid)))
            exact("forward node blocks == one block, no keep_hid", torch.equal(Z, ops.project_fwd(x, W1, b1, W2, b2, pad=c.pad)))
            lib_env("DL_FWD_BLOCK_ROWS", dict(c.env)["DL_FWD_BLOCK_ROWS"])
        if "nows" in c.also:                            # dl_project_fwd with ws = None, ws_bytes = 0: fp32 MFMA, one group
            assert (form["nows"]["split"], form["nows"]["G"]) == (0, 1)
            xk, W1k = ops._pad_features(x, W1) if c.pad else (x, W1)
            Zn = torch.full((N, K, d), float("nan"), device=DEV)
            hidn = torch.full((int(lib.dl_project_hidden_floats(N, K, nhid)),), float("nan"), device=DEV)
            for i in range(2):
                _lib.check(lib.dl_project_fwd(xk.data_ptr(), N, xk.shape[1], K, nhid, d, W1k.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                                              b2.data_ptr(), Zn.data_ptr(), hidn.data_ptr(), None, 0, ops._stream()), "dl_project_fwd")
                if i == 0:
                    first = (Zn.clone(), _valid_hid(hidn, N, K, nhid).clone())
            note("forward, no workspace", {"Z": Zn, "hid": _valid_hid(hidn, N, K, nhid)}, "64", none)
            exact("forward, no workspace bitwise repeatable", torch.equal(first[0], Zn) and torch.equal(first[1], _valid_hid(hidn, N, K, nhid)))
    else:
        Z = ops.project_fwd(x, W1, b1, pad=c.pad)
        note("forward", {"Z1": Z}, "64", none)
        exact("forward bitwise repeatable", torch.equal(Z, ops.project_fwd(x, W1, b1, pad=c.pad)))

    # ---- backward, hidden layer recomputed (one layer: kernel B over dZ, column sums)
    names = ("dW1", "db1", "dW2", "db2") if two else ("dW", "db")
    rec = ops.project_bwd(x, W1, b1, W2, dZ, pad=c.pad)
    note("backward recompute", dict(zip(names, rec)), "64", rp.PLANE_PRODUCTS["recompute"] if form["rec"]["planes"] else none)
    exact("backward recompute bitwise repeatable", _same(rec, ops.project_bwd(x, W1, b1, W2, dZ, pad=c.pad)))
    for g, w in zip(rec, (W1, b1, W2, b2)):
        assert (g is None) == (w is None) and (g is None or g.shape == w.shape)

    # ---- backward from the kept hidden layer: the reference's hid, NaN in the padding columns
    kept = None
    if two and c.kept is not None:
        hidT = rp.hidT_layout(r["hid32"]).to(DEV)
        kept = ops.project_bwd(x, W1, b1, W2, dZ, pad=c.pad, hid=hidT)
        note("backward kept", dict(zip(names, kept)), "64_kept", rp.PLANE_PRODUCTS["kept"] if form["kept"]["planes"] else none)
        exact("backward kept bitwise repeatable", _same(kept, ops.project_bwd(x, W1, b1, W2, dZ, pad=c.pad, hid=hidT)))

    if "one_alloc" in c.also:
        exact("gradients lie in one allocation", rec[0].untyped_storage().data_ptr() == rec[1].untyped_storage().data_ptr())
        sep = ops.project_bwd(x, W1, b1, W2, dZ, pad=c.pad, one_allocation=False)
        exact("separate allocations", sep[0].untyped_storage().data_ptr() != sep[1].untyped_storage().data_ptr())
        exact("one_allocation False == True, recompute", _same(rec, sep))
        exact("one_allocation False == True, kept", _same(kept, ops.project_bwd(x, W1, b1, W2, dZ, pad=c.pad, hid=hidT, one_allocation=False)))

    if "xplanes" in c.also:                             # documented: persistent planes give the bits of the per-call split
        assert form["fwd_xp"]["xplanes"] and form["rec_xp"]["xplanes"] and form["kept_xp"]["xplanes"]
        monkeypatch.delenv("DL_X_PLANES")
        planes = ops.xplanes_for(x, force=True)
        exact("persistent planes built", planes is not None)
        Zx, hidx = ops.project_fwd(x, W1, b1, W2, b2, pad=c.pad, keep_hid=True)
        exact("persistent x planes == per-call split, Z and hid", torch.equal(Z, Zx) and torch.equal(H, _valid_hid(hidx, N, K, nhid)))
        exact("persistent x^T planes == per-call split, recompute", _same(rec, ops.project_bwd(x, W1, b1, W2, dZ, pad=c.pad)))
        exact("persistent x^T planes == per-call split, kept", _same(kept, ops.project_bwd(x, W1, b1, W2, dZ, pad=c.pad, hid=hidT)))
        exact("planes reused", ops.xplanes_for(x) is not None and ops.xplanes_for(x).data_ptr() == planes.data_ptr())

    print()
    for what, got, bnd in figures:
        print(f"FIGURE {c.name}: {what} = {got:.4g} (bound {bnd:.4g})")
    for what, got, bnd in figures:
        assert got <= bnd, (c.name, what, got, bnd)     # a NaN fails
