"""tests/ref64.py — the fp64 reference of tests/test_gpu_hotpath_fp64.py — checked on the CPU: against the committed
outputs of the reference model, against fp64 autograd of the dense [K,N,N] formula written out here, and its input
builder against its own conditions.  The last part measures the fp32 numpy oracle (oracle/sparse_ref.py) against the
reference on every case the GPU test runs: ref64.ORACLE records those figures, and the GPU bounds are 4x them."""
import functools

import numpy as np
import pytest
import torch

import ref64
from conftest import golden_case_names, load_golden
from oracle import dense_ref, sparse_ref

F64 = torch.float64
SLACK = ref64.CPU_SLACK              # for re-measuring the oracle on this host; the GPU bounds do not contain it


def _golden_problem(name):
    g = load_golden(name)
    m = g["meta"]
    sd = {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}
    Z = dense_ref.project(torch.from_numpy(g["x"]), sd).permute(1, 0, 2).contiguous().double()        # [N,K,d]
    rowptr, col, _rev = sparse_ref.csr_from_dense(g["adj"])
    return g, m, Z, torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()


@pytest.mark.parametrize("name", golden_case_names())
def test_ref64_reproduces_the_reference_models_outputs(name):
    g, m, Z, rowptr, col = _golden_problem(name)
    N, K, d = Z.shape
    src = ref64.edge_src(rowptr)
    alpha = ref64.alpha64(Z, rowptr, col, m["t"])
    p = torch.argmax(alpha, dim=1)
    assert np.array_equal(p.numpy(), g["p"][src.numpy(), col.numpy()])
    a, s_raw, H = ref64.forward64(Z, rowptr, col, p, m["beta"], m["t"])
    np.testing.assert_allclose(a.numpy(), g["a"][src.numpy(), col.numpy()], rtol=2e-6)
    np.testing.assert_allclose(torch.where(s_raw == 0, torch.ones_like(s_raw), s_raw).numpy(), g["s"], rtol=2e-6)
    np.testing.assert_allclose(H.reshape(N, K * d).numpy(), g["emb"], rtol=1e-5, atol=2e-6)
    idx = torch.arange(N)
    x = ref64.logit64(Z, H, idx.repeat_interleave(N), idx.repeat(N), m["t"]).view(N, N)
    np.testing.assert_allclose(torch.sigmoid(x).numpy(), g["link_pred"], rtol=1e-5, atol=2e-6)


def _dense64(Zk, adj, beta, t):
    """model.py:55-77 and 109-113 as written: dense [K,N,N], float64.  Zk [K,N,d] -> H [K,N,d], P [N,N]."""
    K = Zk.shape[0]
    e = torch.exp(torch.bmm(Zk, Zk.transpose(1, 2)) / t)
    alpha = e / e.sum(dim=0)
    routed = (torch.argmax(alpha, dim=0) + 1) * adj
    H = []
    for k in range(K):
        a_k = (routed == k + 1).double() * alpha[k]
        s_k = a_k.sum(dim=1)
        s_k = torch.where(s_k == 0, torch.ones_like(s_k), s_k)
        H.append(beta * Zk[k] + (1 - beta) * ((a_k / s_k) @ Zk[k]))           # a[i,j] / s[j]: broadcast over columns
    H = torch.stack(H, 0)
    return H, torch.sigmoid((torch.bmm(H, H.transpose(1, 2)) * e).sum(dim=0))


@pytest.mark.parametrize("name", golden_case_names())
def test_ref64_gradients_equal_autograd_of_the_dense_formula(name):
    g, m, Z, rowptr, col = _golden_problem(name)
    N, K, d = Z.shape
    beta, t = m["beta"], m["t"]
    gen = torch.Generator().manual_seed(N * 100 + K)
    pu, pv = torch.randint(0, N, (4 * N,), generator=gen), torch.randint(0, N, (4 * N,), generator=gen)
    pv[:3] = pu[:3]
    g_prob = torch.randn(4 * N, generator=gen, dtype=F64)
    g_emb = torch.randn(N, K, d, generator=gen, dtype=F64)
    # dense
    Zk = Z.permute(1, 0, 2).contiguous().requires_grad_(True)
    Hk, P = _dense64(Zk, torch.from_numpy(g["adj"]).double(), beta, t)
    ((P[pu, pv] * g_prob).sum() + (Hk.permute(1, 0, 2) * g_emb).sum()).backward()
    dZ_dense = Zk.grad.permute(1, 0, 2)
    # ref64
    p = torch.argmax(ref64.alpha64(Z, rowptr, col, t), dim=1)
    _a, _s, H = ref64.forward64(Z, rowptr, col, p, beta, t)
    assert float((H - Hk.detach().permute(1, 0, 2)).abs().max()) <= 1e-12 * float(H.abs().max())
    x = ref64.logit64(Z, H, pu, pv, t)
    assert float((torch.sigmoid(x) - P.detach()[pu, pv]).abs().max()) <= 1e-12
    dZ_s, dH = ref64.score_bwd64(Z, H, pu, pv, t, g_prob)
    dZ_s2, dH2 = ref64.score_bwd64(Z, H, pu, pv, t, g_prob, torch.sigmoid(x))          # sigmoid backward at a given prob
    assert float((dZ_s - dZ_s2).abs().max()) <= 1e-12 * float(dZ_s.abs().max())
    assert float((dH - dH2).abs().max()) <= 1e-12 * float(dH.abs().max())
    dZ = dZ_s + ref64.route_aggregate_bwd64(Z, rowptr, col, p, beta, t, dH + g_emb)
    assert float(dZ_dense.abs().max()) > 0
    assert float((dZ - dZ_dense).abs().max()) <= 1e-11 * float(dZ_dense.abs().max())


def test_input_builder_has_the_ladder_of_degrees_and_pair_counts():
    st = ref64.structure()
    deg = (st.rowptr[1:] - st.rowptr[:-1]).numpy()
    assert tuple(deg[st.ladder]) == ref64.LADDER_DEGREES and deg[st.isolated] == 0
    assert st.graph.n_nodes == ref64.N_NODES and 310 <= ref64.N_NODES <= 330
    pool_edges = int(deg.sum()) - 2 * sum(ref64.LADDER_DEGREES)
    assert 600 <= pool_edges <= 900                                   # a few hundred pool-pool edges, both directions
    assert not np.isin(st.col.numpy()[np.isin(ref64.edge_src(st.rowptr).numpy(), st.ladder)], st.ladder).any()
    pu, pv = st.pu.numpy(), st.pv.numpy()
    first = np.bincount(pu, minlength=ref64.N_NODES)
    second = np.bincount(pv, minlength=ref64.N_NODES)
    assert tuple(first[st.pair_ladder]) == ref64.LADDER_PAIRS and (second[st.pair_ladder] == 0).all()
    inc = (st.pairs.inc.rowptr[1:] - st.pairs.inc.rowptr[:-1]).long().numpy()
    assert np.array_equal(inc, first + second) and tuple(inc[st.pair_ladder]) == ref64.LADDER_PAIRS
    assert st.isolated not in st.pair_ladder
    assert len(st.dup_pairs) == 20 and 2700 <= pu.size <= 2900
    # the production lengths the ladder is built around
    assert st.graph.plan.seg_len == 32 and st.pairs.inc.seg_len == 64 and st.pairs.by_u.seg_len == 64


def _case_keys():
    from disenlink_amd import _lib
    keys = []
    for c in ref64.hotpath_cases(_lib.load()):
        if c[:5] not in keys:
            keys.append(c[:5])
    return keys


def test_cases_cover_every_tuned_shape_of_the_library():
    from disenlink_amd import _lib
    lib = _lib.load()
    cases = ref64.hotpath_cases(lib)
    ids = [ref64.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids)
    for dtype in ("f32", "bf16"):
        shapes = ref64.tuned_shapes(lib, dtype)
        assert (8, 64) in shapes and len(shapes) >= 5
        assert {(c.K, c.d) for c in cases if c.dtype == dtype and not c.generic} >= set(shapes)
        assert {c.t for c in cases if (c.K, c.d, c.dtype, c.generic) == (8, 64, dtype, False)} == set(ref64.TEMPERATURES)
    assert {(c.K, c.d) for c in cases if c.generic} == set(ref64.tuned_shapes(lib, "f32"))
    assert {(c.K, c.d) for c in cases if c.dtype == "f32"} >= set(ref64.UNTUNED)
    assert {c.t for c in cases} == set(ref64.TEMPERATURES) and {c.beta for c in cases} == set(ref64.BETAS)


@functools.lru_cache(maxsize=None)
def _oracle_errors(key):
    """The fp32 numpy oracle against ref64 on one case, each kernel's part handed the inputs the kernel is handed."""
    K, d, dtype, t, beta = key
    st, r = ref64.structure(), ref64.reference(*key)
    rowptr, col, rev = st.graph.rowptr.numpy(), st.graph.col.numpy(), st.graph.rev.numpy()
    pu, pv = st.pu.numpy(), st.pv.numpy()
    f32 = lambda x: x.float().numpy()
    Zh, Hh = f32(r["Z"]), f32(r["H_in"])
    p_o, a_o, _alpha, s_o = sparse_ref.route(Zh, rowptr, col, t)
    assert np.array_equal(p_o, r["p"].numpy())
    out = {"a": ref64.band_ratio(a_o, r["a"], r["a_abs"]), "s": ref64.band_ratio(s_o, r["s"], r["s_abs"])}
    H_o = sparse_ref.aggregate(Zh, rowptr, col, p_o, f32(r["a32"]), f32(r["s32"]), beta)
    out["H"] = ref64.band_ratio(H_o, r["H"], r["H_abs"])
    if dtype == "bf16":     # the oracle's H stored as bf16 (round to nearest even): inside half a unit in the last place + its fp32
        err = (torch.from_numpy(H_o).to(torch.bfloat16).double() - r["H"]).abs()      # band, and far outside a flat 2^-9 |H|
        half = ref64.bf16_half_ulp(r["H"].abs() + SLACK * ref64.ORACLE["H"] * ref64.U * r["H_abs"])
        assert ref64.band_ratio(torch.clamp(err - half, min=0.0), torch.zeros_like(err), r["H_abs"]) <= SLACK * ref64.ORACLE["H"]
        assert ref64.band_ratio(torch.clamp(err - 2.0 ** -9 * r["H"].abs(), min=0.0), torch.zeros_like(err), r["H_abs"]) > 1e3
    prob_o, q_o, e_o = sparse_ref.score_pairs(Zh, Hh, pu, pv, t, return_parts=True)
    x_o = (q_o * e_o).sum(axis=1, dtype=np.float32)
    out["logit"] = ref64.band_ratio(x_o, r["logit"], r["logit_abs"])
    out["prob_eps"] = float((torch.from_numpy(prob_o).double() - torch.sigmoid(torch.from_numpy(x_o).double())).abs().max()) / ref64.U
    band = ref64.prob_band(r["logit"], SLACK * ref64.ORACLE["logit"] * ref64.U * r["logit_abs"], SLACK * ref64.ORACLE["prob_eps"] * ref64.U)
    assert bool(((torch.from_numpy(prob_o).double() - torch.sigmoid(r["logit"])).abs() <= band).all())
    dZs_o, dH_o = sparse_ref.score_pairs_bwd(Zh, Hh, pu, pv, t, f32(r["g_prob"]))
    # the one-pass scorer's part: the clamped BCE gradient from the oracle's OWN fp32 probability, as the kernel forms it
    lab, wgt = f32(r["label"]), f32(r["weight"])
    g_o = (wgt * (prob_o - lab) / np.maximum(prob_o * (1 - prob_o), np.float32(1e-12))).astype(np.float32)
    dZt_o, dHt_o = sparse_ref.score_pairs_bwd(Zh, Hh, pu, pv, t, g_o)
    out["dZ_score"] = max(ref64.row_ratio(dZs_o, r["dZ_score"]), ref64.row_ratio(dZt_o, r["dZ_train"]))
    out["dH"] = max(ref64.row_ratio(dH_o, r["dH"]), ref64.row_ratio(dHt_o, r["dH_train"]))
    dZ_o = sparse_ref.route_aggregate_bwd(Zh, rowptr, col, rev, p_o, f32(r["a32"]), f32(r["s32"]), beta, t, f32(r["dH32"]))
    out["dZ_route"] = ref64.row_ratio(dZ_o, r["dZ_route"])
    out["_info"] = (r["seed"], round(r["scale"], 3), r["margin"], r["n_sat"])
    return out


@pytest.mark.parametrize("key", _case_keys(), ids=lambda k: f"{k[2]}-K{k[0]}-d{k[1]}-t{k[3]:g}")
def test_builder_conditions_hold_and_the_fp32_oracle_stays_within_its_recorded_error(key):
    """ref64.reference asserts the margin / saturation / finiteness conditions itself; here the fp32 oracle's distance to the
    reference is measured in the metrics of the GPU test, printed (pytest -s), and held within CPU_SLACK of ref64.ORACLE."""
    err = _oracle_errors(key)
    print("\nCALIBRATION", key, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in err.items()})
    for k, v in ref64.ORACLE.items():
        assert err[k] <= SLACK * v, (k, err[k], v)


def test_recorded_oracle_errors_are_the_measured_maxima():
    """ORACLE is what the oracle shows, within the slack of another host's summation order, on both sides: the GPU bounds are
    4x ORACLE, so a figure far above the measurement would loosen them unnoticed."""
    errs = [_oracle_errors(k) for k in _case_keys()]
    for k, v in ref64.ORACLE.items():
        worst = max(e[k] for e in errs)
        assert v / SLACK <= worst <= SLACK * v, (k, worst, v)
