"""The projection of sparse features on the MI355X (csrc/dl_project_sparse.hip through its C ABI) against the fp64 reference
of tests/ref64_sparse_project.py, element by element inside the bounds derived there (4x the plain fp32 evaluation's error
plus the three-plane term where a product runs on planes); bit-for-bit repeatability and independence of the segment
length; the module and the training loop on a SparseFeatures input against the dense kernels and the real-data fixtures.

Every case prints its FIGURES line (largest band ratio of each output / its bound) before it asserts; one MI355X run is
kept in profiles/sparse_project_figures.txt."""
import json
import os

import numpy as np
import pytest
import torch

import ref64_project as rp
import ref64_sparse_project as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = sp.cases()


def _dev(r, *names):
    return [None if r[n] is None else r[n].to(DEV) for n in names]


def _run_case(c, r, sf):
    """Forward and backward of case c through ops.project_sparse_fwd / _bwd (thin ctypes callers of dl_project_sparse_fwd /
    _bwd); the gradients from the reference's hid32 in the library's layout.  -> dict of CPU tensors."""
    from disenlink_amd import ops
    W1, b1, W2, b2, dZ = _dev(r, "W1", "b1", "W2", "b2", "dZ")
    out = {}
    if c.nhid > 0:
        Z, hid = ops.project_sparse_fwd(sf, W1, b1, W2, b2)
        ld = (c.N + 3) // 4 * 4
        out["hid"] = hid.view(c.K, c.nhid, ld)[:, :, :c.N].permute(2, 0, 1).contiguous().cpu()
        out["Z"] = Z.cpu()
        hidT = rp.hidT_layout(r["hid32"]).to(DEV)                          # NaN in the padding columns nobody owns
        dW1, db1, dW2, db2 = ops.project_sparse_bwd(sf, W1, b1, W2, dZ, hid=hidT)
        out.update(dW1=dW1.cpu(), db1=db1.cpu(), dW2=dW2.cpu(), db2=db2.cpu())
    else:
        out["Z1"] = ops.project_sparse_fwd(sf, W1, b1).cpu()
        dW, db, _a, _b = ops.project_sparse_bwd(sf, W1, b1, None, dZ)
        out.update(dW=dW.cpu(), db=db.cpu())
    return out


@pytest.mark.parametrize("c", CASES, ids=sp.case_id)
def test_sparse_projection_against_fp64(c, lib_env):
    f = sp.form(c, lib_env)
    sp.check_expected(c, f)                                                # the reported form, before the case runs
    r = sp.reference(c)
    sf = sp.sparse_features(r, DEV)
    if c.seg is not None:
        lib_env("DL_SPARSE_SEG", c.seg)
    got = _run_case(c, r, sf)
    planes = {**sp.PLANE_PRODUCTS["fwd"], **sp.PLANE_PRODUCTS["bwd"]}
    err = sp.ratios(got, r)
    print("\nFIGURES", c.name, {k: f"{v:.3g}/{sp.bound(k, planes[k]):.3g}" for k, v in err.items()})
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k                            # nothing read that nobody wrote (DL_POISON)
    for k, v in err.items():
        assert v <= sp.bound(k, planes[k]), (c.name, k, v, sp.bound(k, planes[k]))
    if c.nhid > 0:
        assert torch.equal(got["hid"] > 0, r["pre64"] > 0)
    # the same bits on a second call
    again = _run_case(c, r, sf)
    for k in got:
        assert torch.equal(got[k], again[k]), (c.name, k, "second call")
    # the copied rows: equal bits wherever a row sits
    if c.copies:
        a, b = c.copies
        key = "hid" if c.nhid > 0 else "Z1"
        assert torch.equal(got[key][a], got[key][b])
        if c.nhid > 0:
            assert torch.equal(got["Z"][a], got["Z"][b])
    # forced segment lengths: the forward does not depend on them; dW1 repeats its bits under each
    fwd_key = "hid" if c.nhid > 0 else "Z1"
    dw_key = "dW1" if c.nhid > 0 else "dW"
    for seg in (1, 3, 64):
        lib_env("DL_SPARSE_SEG", seg)
        s1, s2 = _run_case(c, r, sf), _run_case(c, r, sf)
        assert torch.equal(s1[fwd_key], got[fwd_key]), (c.name, "forward under DL_SPARSE_SEG", seg)
        assert torch.equal(s1[dw_key], s2[dw_key]), (c.name, "dW1 repeat under DL_SPARSE_SEG", seg)
        e = sp.ratios({dw_key: s1[dw_key]}, r)[dw_key]
        assert e <= sp.bound(dw_key, 0), (c.name, dw_key, seg, e)


def test_a_plan_of_another_segment_length_is_refused(lib_env):
    from disenlink_amd import _lib
    c = CASES[1]
    r = sp.reference(c)
    sf = sp.sparse_features(r, DEV)
    ref = sf.c_struct()                                                    # cut at the default length
    lib_env("DL_SPARSE_SEG", 7)
    lib = _lib.load()
    rc = lib.dl_project_sparse_bwd(ref, c.K, c.nhid, c.d, None, None, None, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"segment" in lib.dl_last_error()


# ---------------------------------------------------------------------------------------------- module level
def _binary_features(N, F, density, seed, standardise):
    from disenlink_amd.features import SparseFeatures
    rng = np.random.default_rng(seed)
    x = (rng.random((N, F)) < density).astype(np.float32)
    x[:, 0] = 1.0                                                         # no constant row under standardisation...
    x[:, 1] = 0.0                                                         # ... and a column without entries
    return SparseFeatures.from_dense(x, standardise=standardise).to(DEV)


@pytest.mark.parametrize("d,nhid,standardise", [(8, 48, True), (64, 96, False), (64, 1, True)])
def test_module_on_sparse_features_matches_the_dense_kernels(d, nhid, standardise):
    """model.project(sf) against model.project(sf.to_dense()) on the dense kernels: Z within rtol / atol 1e-5 and every
    parameter gradient within 1e-4 of its largest entry (the bands tests/test_gpu_parity.py holds these quantities to)."""
    from disenlink_amd.model import Disentangle
    sf = _binary_features(301, 77, 0.1, 5, standardise)
    xd = sf.to_dense()
    torch.manual_seed(1)
    model = Disentangle(77, nhid, d, nfactor=3, beta=0.9).to(DEV)
    G = torch.randn(301, 3, d, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    grads = {}
    for name, x in (("sparse", sf), ("dense", xd)):
        model.zero_grad()
        Z = model.project(x)
        (Z * G).sum().backward()
        grads[name] = (Z.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()})
    Zs, Zd = grads["sparse"][0], grads["dense"][0]
    np.testing.assert_allclose(Zs.cpu().numpy(), Zd.cpu().numpy(), rtol=1e-5, atol=1e-5)
    for k, gd in grads["dense"][1].items():
        gs = grads["sparse"][1][k]
        scale = max(float(gd.abs().max()), 1e-6)
        assert float((gs - gd).abs().max()) <= 1e-4 * scale, (k, float((gs - gd).abs().max()), scale)


def test_autograd_through_forward_pairs_loss_runs_on_sparse_features():
    from disenlink_amd import train
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    N, F, K, d = 120, 40, 3, 32
    sf = _binary_features(N, F, 0.15, 7, True)
    rng = np.random.default_rng(8)
    src, dst = rng.integers(0, N, 600), rng.integers(0, N, 600)
    keep = src != dst
    split = make_link_split(src[keep], dst[keep], N, m=2, seed=1)
    run = train.prepare_run(split, torch.device(DEV), row_bytes=K * d * 4)
    label, weight = train._loss_vectors(run, torch.device(DEV))
    torch.manual_seed(3)
    model = Disentangle(F, 24, d, nfactor=K, beta=0.9).to(DEV)
    out = {}
    for name, x in (("sparse", sf), ("dense", sf.to_dense())):
        model.zero_grad()
        _emb, prob, loss = model.forward_pairs_loss(x, run.graph, run.train_val_pairs, label, weight)
        loss.backward()
        out[name] = (float(loss), {k: p.grad.clone() for k, p in model.named_parameters()})
        assert all(bool(torch.isfinite(g).all()) for g in out[name][1].values())
    assert abs(out["sparse"][0] - out["dense"][0]) <= 1e-5 * abs(out["dense"][0])
    for k, gd in out["dense"][1].items():
        assert float((out["sparse"][1][k] - gd).abs().max()) <= 1e-4 * max(float(gd.abs().max()), 1e-6), k


# ---------------------------------------------------------------------------------------------- real data, end to end
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["cora", "texas"])
def test_real_data_through_sparse_features_holds_the_dense_tolerances(name, use_graph):
    """real_cora.npz (binary, unstandardised) and real_texas.npz (binary, then row-standardised): the SparseFeatures built
    from feat_row / feat_col through run_link_prediction holds the tolerances test_real_data_auc_parity_with_the_reference_model
    holds for the dense input against the same recorded reference run."""
    from conftest import GOLDEN_DIR
    from disenlink_amd.features import SparseFeatures
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    g = np.load(os.path.join(GOLDEN_DIR, f"real_{name}.npz"))
    m = json.loads(str(g["meta"]))
    edges = g["edges"].astype(np.int64)
    shape = tuple(int(v) for v in g["feat_shape"])
    sf = SparseFeatures.from_coo(g["feat_row"].astype(np.int64), g["feat_col"].astype(np.int64), shape,
                                 standardise="standardise" in g).to(DEV)
    assert sf.val is None and (sf.shift is not None) == ("standardise" in g)
    split = make_link_split(edges[:, 0], edges[:, 1], shape[0], m=m["m"], seed=m["split_seed"])
    torch.manual_seed(m["seed"])
    model = Disentangle(shape[1], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"]).to(DEV)
    res = run_link_prediction(model, sf, prepare_run(split, torch.device(DEV), row_bytes=m["K"] * m["d"] * 4),
                              epochs=m["epochs"], lr=m["lr"], use_graph=use_graph)
    np.testing.assert_allclose(res.losses[:12], g["losses"][:12], rtol=5e-5)
    np.testing.assert_allclose(res.losses, g["losses"], rtol=1e-3)
    assert np.abs(np.array(res.val_aucs) - g["val_aucs"]).max() <= 1e-4, np.abs(np.array(res.val_aucs) - g["val_aucs"]).max()
    assert abs(res.test_auc - float(g["test_auc"])) <= 1e-4, (res.test_auc, float(g["test_auc"]))
