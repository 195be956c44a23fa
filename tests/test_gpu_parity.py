"""GPU parity: the HIP path (through the C ABI) against the golden vectors of the reference and
against the CPU oracle on seeded inputs.  Tolerances: fp32, abs/rel 1e-5 on embeddings and
probabilities, 1e-4 relative on parameter gradients, AUC 1e-4."""
import numpy as np
import pytest
import torch

from conftest import golden_case_names, load_golden
from oracle import dense_ref, metrics_ref, sparse_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from disenlink_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()


def _sd(g):
    return {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}


def _Z(g):
    Z = dense_ref.project(torch.from_numpy(g["x"]), _sd(g)).permute(1, 0, 2).contiguous()
    return Z.numpy()


def _decisive(alpha, margin=1e-5):
    """edges whose top-2 routing weights differ by more than `margin` (ties may flip in fp32)."""
    if alpha.shape[1] == 1:
        return np.ones(alpha.shape[0], bool)
    top = np.sort(alpha, axis=1)
    return (top[:, -1] - top[:, -2]) > margin


@pytest.mark.parametrize("force_generic", [0, 1])
@pytest.mark.parametrize("name", golden_case_names())
def test_forward_kernels_match_reference_golden(name, force_generic):
    from disenlink_amd import _lib, ops
    from disenlink_amd.graph import Graph
    g = load_golden(name)
    m = g["meta"]
    N, K, d = m["N"], m["K"], m["d"]
    old = _lib.load().dl_set_force_generic(force_generic)
    try:
        Zh = _Z(g)
        Z = torch.from_numpy(Zh).to(DEV)
        G = Graph.from_dense(torch.from_numpy(g["adj"]).to(DEV), seg_len=8)
        p, a, s = ops.route_fwd(G, Z, m["t"])
        rowptr, col, _rev = sparse_ref.csr_from_dense(g["adj"])
        src = sparse_ref.edge_rows(rowptr)
        _p, _a, alpha, _s = sparse_ref.route(Zh, rowptr, col, m["t"])
        ok = _decisive(alpha)
        # every committed fixture routes every edge decisively (top-2 margin > 1e-5: checked on the CPU when the fixtures were
        # made), so the near-tie masks below select EVERYTHING here — they only say what would have to be left out if a
        # fixture with a near-tie were ever added, and such a fixture must say so explicitly
        assert ok.all(), f"{name}: {int((~ok).sum())} near-tie edges in a golden fixture"
        assert (p.cpu().numpy()[ok] == g["p"][src, col][ok]).all()
        np.testing.assert_allclose(a.cpu().numpy()[ok], g["a"][src, col][ok], rtol=1e-5)
        # A near-tie in the routing of one edge (fp32 may break it either way) changes s of that row, h of that row and of
        # its neighbours: everything is asserted on the nodes no near-tie can reach — all of them in most cases
        row_ok = np.bincount(src[~ok], minlength=N) == 0                       # every edge of the row is decisive
        nb_bad = np.bincount(src, weights=(~row_ok[col]).astype(float), minlength=N) > 0
        node_ok = row_ok & ~nb_bad                                             # ... and of every neighbour's row
        assert node_ok.all(), node_ok.mean()                                   # all nodes, all N^2 scores are compared
        s_h = s.cpu().numpy()
        np.testing.assert_allclose(np.where(s_h == 0, 1, s_h)[row_ok], g["s"][row_ok], rtol=1e-5)
        H = ops.aggregate_fwd(G, Z, m["beta"], p, a, s)
        np.testing.assert_allclose(H.cpu().numpy().reshape(N, K * d)[node_ok], g["emb"][node_ok], rtol=1e-5, atol=1e-5)
        idx = torch.arange(N, dtype=torch.int32, device=DEV)
        prob = ops.score_pairs_fwd(Z, H, idx.repeat_interleave(N), idx.repeat(N), m["t"]).view(N, N)
        both = np.outer(node_ok, node_ok)
        np.testing.assert_allclose(prob.cpu().numpy()[both], g["link_pred"][both], rtol=1e-5, atol=1e-5)
    finally:
        _lib.load().dl_set_force_generic(old)


@pytest.mark.parametrize("force_generic", [0, 1])
@pytest.mark.parametrize("name", golden_case_names())
def test_dropin_module_loss_and_grads_match_reference(name, force_generic):
    """The reference's own call sequence (model(x, adj_sym) -> masked BCE -> backward,
    main_disentangled.py:194-198) on the drop-in module vs. the reference's loss and gradients."""
    from disenlink_amd import _lib
    from disenlink_amd.model import Disentangle
    import torch.nn.functional as F
    g = load_golden(name)
    m = g["meta"]
    old = _lib.load().dl_set_force_generic(force_generic)
    try:
        model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"])
        model.load_state_dict(_sd(g))
        model = model.to(DEV)
        x = torch.from_numpy(g["x"]).to(DEV)
        adj = torch.from_numpy(g["adj"]).to(DEV)
        ori = torch.from_numpy(g["ori_adj"]).to(DEV)
        pm = torch.from_numpy(g["pos_mask"]).to(DEV)
        nm = torch.from_numpy(g["neg_mask"]).to(DEV)
        emb, a_pred = model(x, adj)
        assert emb.shape == (m["N"], m["K"] * m["d"]) and a_pred.shape == (m["N"], m["N"])
        loss = (F.binary_cross_entropy(a_pred[pm == 1].unsqueeze(0), ori[pm == 1].unsqueeze(0))
                + F.binary_cross_entropy(a_pred[nm == 1].unsqueeze(0), ori[nm == 1].unsqueeze(0)) / m["m"])
        model.zero_grad()
        loss.backward()
        np.testing.assert_allclose(emb.detach().cpu().numpy(), g["emb"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(a_pred.detach().cpu().numpy(), g["link_pred"], rtol=1e-5, atol=1e-5)
        assert abs(loss.item() - float(g["loss"])) <= 2e-5 * max(1.0, abs(float(g["loss"])))
        for k, prm in model.named_parameters():
            ref = g["grad__" + k]
            scale = max(np.abs(ref).max(), 1e-6)
            err = np.abs(prm.grad.cpu().numpy() - ref).max()
            assert err <= 1e-4 * scale, (k, err, scale)
        # AUC on fp32 probabilities with tie-averaged ranks (main_disentangled.py:202-204)
        mask = (g["pos_mask"] + g["neg_mask"]) > 0
        y = g["ori_adj"][mask]
        if 0 < y.sum() < y.size:
            auc_gpu = metrics_ref.auc_tie_avg(y, a_pred.detach().cpu().numpy()[mask])
            auc_ref = metrics_ref.auc_tie_avg(y, g["link_pred"][mask])
            assert abs(auc_gpu - auc_ref) <= 1e-4
    finally:
        _lib.load().dl_set_force_generic(old)


def _random_problem(seed, N, K, d, avg_deg, hub=True, scale=0.35):
    rng = np.random.default_rng(seed)
    E = N * avg_deg // 2
    src = rng.integers(0, N, E)
    dst = rng.integers(0, N, E)
    if hub:
        hub_nb = rng.choice(N, size=min(N - 1, 40 * avg_deg), replace=False)
        src = np.r_[src, np.zeros_like(hub_nb)]
        dst = np.r_[dst, hub_nb]
    iso = N - 1
    keep = (src != iso) & (dst != iso)
    src, dst = src[keep], dst[keep]
    Z = (rng.standard_normal((N, K, d)) * scale).astype(np.float32)
    return src, dst, Z, rng


@pytest.mark.parametrize("force_generic", [0, 1])
@pytest.mark.parametrize("K,d,N,deg", [(8, 64, 600, 12), (4, 32, 500, 9), (16, 128, 200, 8), (5, 64, 300, 10),
                                        (3, 5, 97, 6), (1, 16, 64, 5), (8, 64, 2000, 30),
                                        (20, 32, 150, 8), (10, 64, 200, 8), (10, 32, 180, 7),     # recipes of hyperparameters_setting
                                        (64, 8, 90, 6), (2, 1, 70, 5)])                           # K at its maximum; d = 1
def test_forward_and_backward_match_oracle_on_random_graphs(K, d, N, deg, force_generic):
    from disenlink_amd import _lib, ops
    from disenlink_amd.graph import Graph, PairList
    beta, t = 0.6, 1.0
    src, dst, Zh, rng = _random_problem(K * 1000 + d, N, K, d, deg)
    old = _lib.load().dl_set_force_generic(force_generic)
    try:
        G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
        rowptr, col, rev = sparse_ref.csr_from_pairs(src, dst, N, symmetrise=True)
        assert np.array_equal(G.rowptr.cpu().numpy(), rowptr) and np.array_equal(G.rev.cpu().numpy(), rev)
        Z = torch.from_numpy(Zh).to(DEV)
        p, a, s = ops.route_fwd(G, Z, t)
        p_o, a_o, alpha, s_o = sparse_ref.route(Zh, rowptr, col, t)
        ok = _decisive(alpha)
        assert (p.cpu().numpy()[ok] == p_o[ok]).all()
        np.testing.assert_allclose(a.cpu().numpy()[ok], a_o[ok], rtol=1e-5)
        # continue from the GPU's own routing so a flipped near-tie does not poison the rest
        p_h, a_h, s_h = p.cpu().numpy(), a.cpu().numpy(), s.cpu().numpy()
        s_chk = np.zeros_like(s_h)
        np.add.at(s_chk, (sparse_ref.edge_rows(rowptr), p_h.astype(np.int64)), a_h)
        np.testing.assert_allclose(s_h, s_chk, rtol=1e-5, atol=1e-7)
        assert (s_h[N - 1] == 0).all()                                   # isolated node
        H = ops.aggregate_fwd(G, Z, beta, p, a, s)
        H_o = sparse_ref.aggregate(Zh, rowptr, col, p_h, a_h, s_h, beta)
        np.testing.assert_allclose(H.cpu().numpy(), H_o, rtol=1e-5, atol=1e-5)
        P = 4000
        pu, pv = rng.integers(0, N, P), rng.integers(0, N, P)
        pu[:5] = pv[:5]
        pairs = PairList.build(torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV), N)
        prob = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs)            # LDS-staged, XCD-sliced plan
        prob_o = sparse_ref.score_pairs(Zh, H_o, pu, pv, t)
        np.testing.assert_allclose(prob.cpu().numpy(), prob_o, rtol=1e-5, atol=1e-5)
        prob_n = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, None)             # per-pair kernel, no plan
        np.testing.assert_allclose(prob_n.cpu().numpy(), prob_o, rtol=1e-5, atol=1e-5)
        unsliced = PairList.build(pairs.pu, pairs.pv, N, n_slices=1, run_len=16)
        prob_u = ops.score_pairs_fwd(Z, H, unsliced.pu, unsliced.pv, t, unsliced)
        np.testing.assert_allclose(prob_u.cpu().numpy(), prob_o, rtol=1e-5, atol=1e-5)
        # backward
        gp = (rng.standard_normal(P) * 0.1).astype(np.float32)
        dZs, dH = ops.score_pairs_bwd(Z, H, pairs, t, prob, torch.from_numpy(gp).to(DEV))
        dZs_o, dH_o = sparse_ref.score_pairs_bwd(Zh, H_o, pu, pv, t, gp)
        tol = lambda ref: 1e-4 * max(np.abs(ref).max(), 1e-6)
        assert np.abs(dH.cpu().numpy() - dH_o).max() <= tol(dH_o)
        assert np.abs(dZs.cpu().numpy() - dZs_o).max() <= tol(dZs_o)
        # the stored-terms backward (tuned path only): per-factor logit terms from the forward
        prob_c, coef = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs, want_coef=True)
        if K <= 8:
            assert torch.equal(prob_c, prob)
        else:           # factor-blocked kernels: the two instantiations may contract their FMAs differently
            assert torch.allclose(prob_c, prob, rtol=2e-6, atol=1e-7)
        if coef is not None:
            _pr, q_o, e_o = sparse_ref.score_pairs(Zh, H_o, pu, pv, t, return_parts=True)
            np.testing.assert_allclose(coef[0].cpu().numpy(), e_o, rtol=1e-5)
            np.testing.assert_allclose(coef[1].cpu().numpy(), q_o * e_o, rtol=1e-4, atol=1e-5)
            dZc, dHc = ops.score_pairs_bwd(Z, H, pairs, t, prob, torch.from_numpy(gp).to(DEV), coef=coef)
            assert np.abs(dHc.cpu().numpy() - dH_o).max() <= tol(dH_o)
            assert np.abs(dZc.cpu().numpy() - dZs_o).max() <= tol(dZs_o)
        else:
            assert force_generic or not _lib.load().dl_has_fast_path(K, d)
        dZ = ops.route_aggregate_bwd(G, Z, beta, t, p, a, s, dH)
        dZ_o = sparse_ref.route_aggregate_bwd(Zh, rowptr, col, rev, p_h, a_h, s_h, beta, t, dH_o)
        assert np.abs(dZ.cpu().numpy() - dZ_o).max() <= tol(dZ_o)
        # accumulate flag adds onto an existing buffer
        base = torch.full_like(Z, 0.5)
        dZ2 = ops.route_aggregate_bwd(G, Z, beta, t, p, a, s, dH, dZ_accum=base)
        np.testing.assert_allclose(dZ2.cpu().numpy(), dZ.cpu().numpy() + 0.5, rtol=1e-5, atol=1e-5)
        # bitwise reproducible: no float atomics anywhere
        p2, a2, s2 = ops.route_fwd(G, Z, t)
        H2 = ops.aggregate_fwd(G, Z, beta, p2, a2, s2)
        dZ3 = ops.route_aggregate_bwd(G, Z, beta, t, p, a, s, dH)
        assert torch.equal(p, p2) and torch.equal(a, a2) and torch.equal(s, s2)
        assert torch.equal(H, H2) and torch.equal(dZ, dZ3)
    finally:
        _lib.load().dl_set_force_generic(old)


def test_empty_and_degenerate_inputs():
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph, PairList
    z0 = torch.zeros(0, dtype=torch.long)
    N, K, d = 5, 4, 32
    G = Graph.from_edge_rows(z0, z0, N).to(DEV)                          # no edges at all
    Z = torch.randn(N, K, d, device=DEV)
    p, a, s = ops.route_fwd(G, Z, 1.0)
    assert p.numel() == 0 and bool((s == 0).all())
    H = ops.aggregate_fwd(G, Z, 0.7, p, a, s)
    np.testing.assert_allclose(H.cpu().numpy(), 0.7 * Z.cpu().numpy(), rtol=1e-6)   # h = beta z
    pairs = PairList.build(z0.to(DEV), z0.to(DEV), N)
    prob = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, 1.0)
    assert prob.numel() == 0
    dZ, dH = ops.score_pairs_bwd(Z, H, pairs, 1.0, prob, prob)
    assert bool((dZ == 0).all()) and bool((dH == 0).all())
    dZ = ops.route_aggregate_bwd(G, Z, 0.7, 1.0, p, a, s, torch.ones_like(Z))
    np.testing.assert_allclose(dZ.cpu().numpy(), 0.7, rtol=1e-6)


@pytest.mark.parametrize("pad_to_workgroups", [False, True])
def test_plans_of_another_layout_are_still_served_correctly(pad_to_workgroups):
    """A C caller may hand over a segment plan it built itself.  Row-major segments with one partial slot per SEGMENT
    (the round-1 layout) are a valid plan: with whole workgroups of positions the tuned kernels treat every segment as its
    own unit; with a position count that is not a multiple of DL_UNIT_SEGS the API must not let the tuned kernels read
    past the arrays — it takes the generic kernels.  Either way the results are those of the library's own plan."""
    from disenlink_amd import ops
    from disenlink_amd.graph import CsrPlan, Graph
    K, d, N, beta, t, seg_len = 8, 64, 203, 0.6, 1.0, 8
    src, dst, Zh, _rng = _random_problem(7, N, K, d, 11)
    G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N, seg_len=seg_len).to(DEV)
    Z = torch.from_numpy(Zh).to(DEV)
    p0, a0, s0 = ops.route_fwd(G, Z, t)
    H0 = ops.aggregate_fwd(G, Z, beta, p0, a0, s0)
    rowptr = G.rowptr.cpu().numpy()
    rows, begs, ends = [], [], []
    for i in range(N):
        b, e = int(rowptr[i]), int(rowptr[i + 1])
        for sb in (range(b, e, seg_len) if e > b else [b]):
            rows.append(i); begs.append(sb); ends.append(min(sb + seg_len, e) if e > b else b)
    rows, begs, ends = np.array(rows), np.array(begs), np.array(ends)
    nseg_row = np.bincount(rows, minlength=N)
    multi = np.flatnonzero(nseg_row > 1)
    slot0 = np.zeros(multi.size + 1, dtype=np.int64)
    slot0[1:] = np.cumsum(nseg_row[multi])
    row_slot0 = -np.ones(N, dtype=np.int64)
    row_slot0[multi] = slot0[:-1]
    idx_in_row = np.arange(rows.size) - np.repeat(np.cumsum(nseg_row) - nseg_row, nseg_row)
    slots = np.where(row_slot0[rows] >= 0, row_slot0[rows] + idx_in_row, -1)
    if not pad_to_workgroups and rows.size % 4 == 0:               # make the un-padded case really un-aligned: the generic
        rows, begs, ends, slots = rows[:-1], begs[:-1], ends[:-1], slots[:-1]      # kernels walk rowptr, not the segments
    if pad_to_workgroups:
        padn = -rows.size % 4
        rows, begs, ends, slots = (np.r_[rows, -np.ones(padn, int)], np.r_[begs, np.zeros(padn, int)],
                                   np.r_[ends, np.zeros(padn, int)], np.r_[slots, -np.ones(padn, int)])
    i32 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.int32, device=DEV)
    plan = CsrPlan(N, 0, N, G.rowptr, G.col, seg_len, i32(rows), i32(begs), i32(ends), i32(slots), 1, int(rows.size),
                   i32([0, rows.size]), i32(multi), i32(slot0), int(slot0[-1]))
    assert (plan.n_seg % 4 == 0) == pad_to_workgroups
    G1 = Graph(plan, None, None, False)
    p1, a1, s1 = ops.route_fwd(G1, Z, t)
    H1 = ops.aggregate_fwd(G1, Z, beta, p1, a1, s1)
    assert torch.equal(p1, p0)
    np.testing.assert_allclose(a1.cpu().numpy(), a0.cpu().numpy(), rtol=2e-6)
    np.testing.assert_allclose(s1.cpu().numpy(), s0.cpu().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(H1.cpu().numpy(), H0.cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_exp_overflow_propagates_like_the_reference():
    """No max-subtraction in the softmax (model.py:56-60): huge dots give inf/inf = NaN, as on the CPU."""
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph
    N, K, d = 4, 2, 8
    Zh = np.full((N, K, d), 4.0, np.float32)                            # z.z = 128 > 88.7 -> exp = inf
    Zh[3] = 0.1
    src, dst = np.array([0, 1, 2]), np.array([1, 2, 3])
    G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
    rowptr, col, _ = sparse_ref.csr_from_pairs(src, dst, N, symmetrise=True)
    p, a, s = ops.route_fwd(G, torch.from_numpy(Zh).to(DEV), 1.0)
    p_o, a_o, _alpha, _s = sparse_ref.route(Zh, rowptr, col, 1.0)
    assert np.array_equal(np.isnan(a.cpu().numpy()), np.isnan(a_o))
    assert np.array_equal(p.cpu().numpy(), p_o)
    fin = ~np.isnan(a_o)
    np.testing.assert_allclose(a.cpu().numpy()[fin], a_o[fin], rtol=1e-6)


@pytest.mark.parametrize("ways", [0, 2, 4, 8])
@pytest.mark.parametrize("force_generic", [0, 1])
def test_row_sharded_plans_reproduce_the_unsharded_result(force_generic, ways):
    """Row shards on one GPU (three uneven ones, or the 2 / 4 / 8 equal blocks dist.py cuts), sharing the node-indexed
    arrays the way all-gathers would: forward and both backward phases must equal the unsharded run bit for bit."""
    from disenlink_amd import _lib, ops
    from disenlink_amd.graph import Graph, PairList
    K, d, N, beta, t = 8, 64, 700, 0.7, 1.0
    src, dst, Zh, rng = _random_problem(42, N, K, d, 14)
    old = _lib.load().dl_set_force_generic(force_generic)
    try:
        ts, td = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)
        G = Graph.from_edge_rows(ts, td, N)
        Z = torch.from_numpy(Zh).to(DEV)
        p, a, s = ops.route_fwd(G, Z, t)
        H = ops.aggregate_fwd(G, Z, beta, p, a, s)
        P = 5000
        pu, pv = np.sort(rng.integers(0, N, P)), rng.integers(0, N, P)
        tpu, tpv = torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV)
        pairs = PairList.build(tpu, tpv, N)
        prob = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs)
        gp = torch.from_numpy((rng.standard_normal(P) * 0.1).astype(np.float32)).to(DEV)
        dZs, dH = ops.score_pairs_bwd(Z, H, pairs, t, prob, gp)
        dZ = ops.route_aggregate_bwd(G, Z, beta, t, p, a, s, dH, dZ_accum=dZs.clone())

        if ways == 0:
            bounds = [0, 230, 231, N]                  # uneven shards, one of a single row
        else:
            blk = -(-N // ways)                        # dist.block_size: equal blocks, the last one short
            bounds = [min(i * blk, N) for i in range(ways + 1)]
        shards = [Graph.from_edge_rows(ts, td, N, row_range=(lo, hi)) for lo, hi in zip(bounds[:-1], bounds[1:])]
        s2 = torch.full_like(s, float("nan"))
        H2 = torch.full_like(H, float("nan"))
        routed = [ops.route_fwd(g, Z, t, s_out=s2)[:2] for g in shards]          # "all-gather" of s = shared buffer
        for g, (pp, aa) in zip(shards, routed):
            ops.aggregate_fwd(g, Z, beta, pp, aa, s2, H_out=H2)
        assert torch.equal(s, s2) and torch.equal(H, H2)
        assert torch.equal(torch.cat([r[0] for r in routed]), p) and torch.equal(torch.cat([r[1] for r in routed]), a)
        # scorer: each shard scores a slice of the pairs and owns the incidence rows of its nodes
        cut = [0, 1700, 1701, P] if ways == 0 else [int(np.searchsorted(pu, b)) for b in bounds[:-1]] + [P]
        prob2 = torch.cat([ops.score_pairs_fwd(Z, H2, pairs.pu[b:e].contiguous(), pairs.pv[b:e].contiguous(), t, None)
                           for b, e in zip(cut[:-1], cut[1:])])
        np.testing.assert_allclose(prob2.cpu().numpy(), prob.cpu().numpy(), rtol=1e-6, atol=1e-7)
        dZs2 = torch.full_like(Z, float("nan"))
        dH2 = torch.full_like(Z, float("nan"))
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            inc = PairList.build(tpu, tpv, N, row_range=(lo, hi))
            ops.score_pairs_bwd(Z, H, inc, t, prob, gp, dZ_out=dZs2, dH_out=dH2)
        assert torch.equal(dZs, dZs2) and torch.equal(dH, dH2)
        ds = torch.full_like(s, float("nan"))
        ph1 = [ops.route_aggregate_bwd_phase1(g, Z, beta, pp, aa, s, dH, ds) for g, (pp, aa) in zip(shards, routed)]
        dZ2 = dZs.clone()
        for g, (pp, aa), (dw, dwr) in zip(shards, routed, ph1):
            ops.route_aggregate_bwd_phase2(g, Z, beta, t, pp, aa, s, dH, dw, dwr, ds, dZ2, accumulate=True)
        assert torch.equal(dZ, dZ2)
    finally:
        _lib.load().dl_set_force_generic(old)


def test_sharded_training_step_over_rccl_matches_the_unsharded_module():
    """dist.sharded_forward + backward + allreduce_gradients with the HIP backend and RCCL collectives (a
    one-rank group: the only size one GPU can host) against forward_pairs of the same module."""
    import torch.distributed as tdist
    from disenlink_amd import dist as dl_dist
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.graph import Graph, PairList
    from disenlink_amd.metrics import pair_bce_loss
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    sg = synthetic_graph("cora", seed=1)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=1)
    pu = np.concatenate([split.pos_train.u, split.neg_train.u])
    pv = np.concatenate([split.pos_train.v, split.neg_train.v])
    lab = np.concatenate([np.ones(split.pos_train.u.size, np.float32), np.zeros(split.neg_train.u.size, np.float32)])
    order = np.lexsort((pv, pu))
    pu, pv, lab = pu[order], pv[order], torch.from_numpy(lab[order]).to(DEV)
    x = torch.from_numpy(sg.features()).to(DEV)
    torch.manual_seed(0)
    model = Disentangle(sg.n_feat, 64, 32, nfactor=4, beta=0.6, t=1).to(DEV)

    def loss_of(prob):
        w = torch.where(lab > 0, 1.0 / float(lab.sum()), 0.2 / float((1 - lab).sum()))
        return -(w * (lab * prob.clamp_min(1e-12).log() + (1 - lab) * (1 - prob).clamp_min(1e-12).log())).sum()

    graph = Graph.from_edge_rows(torch.from_numpy(split.train_src).to(DEV), torch.from_numpy(split.train_dst).to(DEV), sg.n_nodes)
    pairs = PairList.build(torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV), sg.n_nodes)
    emb, prob = model.forward_pairs(x, graph, pairs)
    model.zero_grad()
    loss_of(prob).backward()
    want = [p.grad.clone() for p in model.parameters()]

    own_group = not tdist.is_initialized()
    if own_group:
        tdist.init_process_group("nccl", init_method="tcp://127.0.0.1:29547", rank=0, world_size=1,
                                 device_id=torch.device(DEV))
    try:
        # One rank owns every row: the shard IS the unsharded graph (mirrored routing plan, one scoring launch) and its
        # step makes no collective and no table copy — the launch sequence of the unsharded module (round-4 verdict: the
        # one-rank sharded squirrel step was 18-22 % slower than the unsharded one, the floor of every weak-scaling curve)
        shard = dl_dist.Shard.build(0, 1, sg.n_nodes, split.train_src, split.train_dst, pu, pv, torch.device(DEV), n_chunks=2)
        assert shard.pair_groups == [] and shard.graph.route_mirror and shard.graph.rev is not None
        dl_dist.reset_message_counts()
        emb_s, prob_s = dl_dist.sharded_forward(model, x, shard)
        counts = dl_dist.reset_message_counts()
        assert counts["collectives"] == 0 and counts["p2p_ops"] == 0 and counts["staging_copies"] == 0, counts
        assert torch.equal(prob_s, prob) and torch.equal(emb_s, emb)              # the same launches: the same bits
        model.zero_grad()
        loss_of(prob_s).backward()
        dl_dist.allreduce_gradients(model)
        got = [p.grad.clone() for p in model.parameters()]
        # the training step with the one-pass scorer over the rank's incidence rows (no (prob, g_prob) all-gather)
        wts = torch.where(lab > 0, 1.0 / float(lab.sum()), 0.2 / float((1 - lab).sum())).contiguous()
        emb_l, prob_l, loss_l = dl_dist.sharded_forward_loss(model, x, shard, lab, wts)
        model.zero_grad()
        loss_l.backward()
        dl_dist.allreduce_gradients(model)
        got_l = [p.grad.clone() for p in model.parameters()]
        # ... and from the pairs that touch the rank's nodes: forward scorer keeping its terms + coefficient-gather backward
        import os
        os.environ["DL_ONE_PASS_SCORER"] = "0"
        try:
            emb_t, prob_t, loss_t = dl_dist.sharded_forward_loss(model, x, shard, lab, wts)
            model.zero_grad()
            loss_t.backward()
            dl_dist.allreduce_gradients(model)
            got_t = [p.grad.clone() for p in model.parameters()]
        finally:
            del os.environ["DL_ONE_PASS_SCORER"]
        torch.cuda.synchronize()
    finally:
        if own_group:
            tdist.destroy_process_group()
    np.testing.assert_allclose(prob_t.detach().cpu().numpy(), prob.detach().cpu().numpy(), rtol=1e-6, atol=1e-7)
    assert abs(float(loss_t.detach()) - float(loss_l.detach())) <= 1e-6 * abs(float(loss_l.detach()))
    for g3, w in zip(got_t, want):
        assert float((g3 - w).abs().max()) <= 2e-5 * max(float(w.abs().max()), 1e-8)
    np.testing.assert_allclose(emb_s.detach().cpu().numpy(), emb.detach().cpu().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(prob_s.detach().cpu().numpy(), prob.detach().cpu().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(prob_l.detach().cpu().numpy(), prob.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    want_loss = torch.nn.functional.binary_cross_entropy(prob.detach(), lab, weight=wts, reduction="sum")   # torch's log clamp at -100
    assert abs(float(loss_l) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    for g1, g2, w in zip(got, got_l, want):
        assert float((g1 - w).abs().max()) <= 1e-5 * max(float(w.abs().max()), 1e-8)
        assert float((g2 - w).abs().max()) <= 2e-5 * max(float(w.abs().max()), 1e-8)


@pytest.mark.parametrize("K,d,N", [(8, 64, 700), (3, 32, 385), (16, 128, 260), (5, 64, 128), (2, 96, 129)])
def test_dense_scorer_on_the_matrix_cores_matches_the_pair_scorer(K, d, N):
    """dl_score_allpairs_fwd (Gram products on MFMA, 128x128 tiles incl. ragged edges) against the pair-list
    scorer evaluated on all N^2 pairs and against the fp64 formula; overflowing factors behave alike."""
    from disenlink_amd import ops
    g = torch.Generator().manual_seed(K * 100 + d)
    amp = 0.3 * (32 / d) ** 0.5 * (4 / K) ** 0.25       # keeps the logits O(1): sigmoid not saturated, exp tame
    Z = (torch.randn(N, K, d, generator=g) * amp).to(DEV)
    H = (torch.randn(N, K, d, generator=g) * amp).to(DEV)
    t = 1.0 if K != 3 else 2.0
    P = ops.score_allpairs_fwd(Z, H, t)
    idx = torch.arange(N, dtype=torch.int32, device=DEV)
    Pp = ops.score_pairs_fwd(Z, H, idx.repeat_interleave(N), idx.repeat(N), t).view(N, N)
    assert P.shape == (N, N)
    np.testing.assert_allclose(P.cpu().numpy(), Pp.cpu().numpy(), rtol=2e-5, atol=1e-6)
    Zd, Hd = Z.double().cpu(), H.double().cpu()
    ref = torch.sigmoid((torch.einsum("ukd,vkd->kuv", Hd, Hd) * torch.exp(torch.einsum("ukd,vkd->kuv", Zd, Zd) / t)).sum(0))
    np.testing.assert_allclose(P.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)
    assert torch.equal(P, ops.score_allpairs_fwd(Z, H, t))                    # reproducible
    assert torch.equal(P, P.t())                                              # mirrored tiles: exactly symmetric
    if d % 32 == 0:                  # without the workspace every tile pair splits what it stages: the same bits
        from disenlink_amd import _lib
        lib = _lib.load()
        assert lib.dl_score_allpairs_workspace_bytes(N, K, d, _lib.DL_F32) > 0
        P0 = torch.full_like(P, float("nan"))
        _lib.check(lib.dl_score_allpairs_fwd(Z.data_ptr(), H.data_ptr(), N, K, d, _lib.DL_F32, float(t), P0.data_ptr(), None, 0,
                                             torch.cuda.current_stream().cuda_stream), "dl_score_allpairs_fwd")
        assert torch.equal(P, P0)
    Zb = Z.clone()
    Zb[1, 0] = 12.0                                                           # exp(z.z) overflows for (1,1)
    Pb = ops.score_allpairs_fwd(Zb, H, t)
    Pbp = ops.score_pairs_fwd(Zb, H, idx.repeat_interleave(N), idx.repeat(N), t).view(N, N)
    assert torch.equal(torch.isnan(Pb), torch.isnan(Pbp))
    ok = ~torch.isnan(Pb)       # large exponents amplify the summation-order difference of the two kernels
    np.testing.assert_allclose(Pb[ok].cpu().numpy(), Pbp[ok].cpu().numpy(), rtol=1e-3, atol=1e-6)


def test_caches_follow_tensor_identity_not_addresses():
    """The per-adjacency graph cache of the drop-in module and the padded-feature cache must not serve a freed
    tensor's entry to a new tensor that happens to reuse its address."""
    from disenlink_amd import ops
    from disenlink_amd.model import Disentangle
    torch.manual_seed(3)
    N, Fdim = 60, 10                                            # F % 4 != 0: the feature-padding cache is in play
    model = Disentangle(Fdim, 16, 32, nfactor=4, beta=0.5, projection="mfma").to(DEV)
    x = torch.randn(N, Fdim, device=DEV)

    def adj_of(seed):
        g = torch.Generator().manual_seed(seed)
        a = (torch.rand(N, N, generator=g) < 0.1).float()
        return ((a + a.t()) > 0).float().to(DEV)

    a1 = adj_of(1)
    addr = a1.data_ptr()
    _e1, p1 = model(x, a1)
    p1 = p1.detach().clone()
    del a1, _e1
    a2 = adj_of(2)                                              # same shape: the allocator usually reuses the block
    _e2, p2 = model(x, a2)
    fresh = Disentangle(Fdim, 16, 32, nfactor=4, beta=0.5, projection="mfma").to(DEV)
    fresh.load_state_dict(model.state_dict())
    _e3, p3 = fresh(x, a2)
    assert torch.equal(p2, p3), ("stale graph served", a2.data_ptr() == addr)
    assert not torch.equal(p1, p2)
    x1 = torch.randn(N, Fdim, device=DEV)
    z1 = model.project(x1).detach().clone()
    xaddr = x1.data_ptr()
    del x1
    x2 = torch.randn(N, Fdim, device=DEV)
    z2 = model.project(x2)
    assert torch.allclose(z2, fresh.project(x2), atol=1e-6), ("stale padded features served", x2.data_ptr() == xaddr)
    assert not torch.equal(z1, z2)


@pytest.mark.parametrize("subclass", ["1", "0"])
def test_dense_backward_plan_is_per_module_grows_with_the_gradients_and_never_goes_wrong_silently(subclass, monkeypatch):
    """(subclass = "1": link_pred is an ops.LinkPred whose indexing reports the entries taken — the plan is learnt from the
    caller's masks; "0": a plain tensor, the plan is learnt from the gradients alone, the safety net behind the former.)
    The backward of the dense [N,N] link_pred runs on a pair plan owned by the MODULE.  Declared masks
    (set_loss_pairs / assume_static_loss_masks(masks)): the plan is their support.  Undeclared: the plan is learnt from
    the gradients and only grows (union), so two models of equal N do not disturb each other and a new mask is noticed.
    In the promised-static mode (no host read) a loss taken OUTSIDE the declared masks gives NaN gradients, and in the
    validated mode it raises — never silently wrong gradients."""
    from disenlink_amd.model import Disentangle
    monkeypatch.setenv("DL_LINK_PRED_SUBCLASS", subclass)
    torch.manual_seed(5)
    N, Fdim = 90, 12
    g = torch.Generator().manual_seed(0)
    a = (torch.rand(N, N, generator=g) < 0.08).float()
    adj = ((a + a.t()) > 0).float().to(DEV)
    x = torch.randn(N, Fdim, device=DEV)
    masks = [(torch.rand(N, N, generator=g) < 0.05).to(DEV) for _ in range(3)]
    lab = adj

    def grads(model, mask):
        model.zero_grad()
        _emb, pred = model(x, adj)
        torch.nn.functional.binary_cross_entropy(pred[mask], lab[mask]).backward()
        return [p.grad.clone() for p in model.parameters()]

    def fresh():
        torch.manual_seed(9)
        return Disentangle(Fdim, 16, 32, nfactor=4, beta=0.6).to(DEV)

    def close(got, ref):
        for x1, x2 in zip(got, ref):
            assert torch.allclose(x1, x2, rtol=2e-5, atol=1e-7), float((x1 - x2).abs().max())

    m1, m2 = fresh(), fresh()
    want = [grads(fresh().set_loss_pairs(mk), mk) for mk in masks]      # the declared plan of each mask
    for rounds in range(2):                                       # interleaved: each module keeps ITS plan
        for model, k in ((m1, 0), (m2, 1), (m1, 0), (m2, 1)):
            close(grads(model, masks[k]), want[k])
    n0 = m1._dense_plan.flat.numel()
    close(grads(m1, masks[2]), want[2])                           # another mask: noticed, the plan GROWS by it ...
    assert m1._dense_plan.flat.numel() > n0
    close(grads(m1, masks[0]), want[0])                           # ... and still serves the first one
    assert m1._dense_plan is not m2._dense_plan
    # declared masks: same bits with and without the host read
    ms, md = fresh().assume_static_loss_masks(masks[0]), fresh().set_loss_pairs(masks[0])
    for _ in range(2):
        for got, ref, dflt in zip(grads(ms, masks[0]), want[0], grads(md, masks[0])):
            assert torch.equal(got, ref) and torch.equal(dflt, ref)
    sub = masks[0] & (torch.rand(N, N, generator=g) < 0.5).to(DEV)       # a loss on PART of the declared support is fine
    close(grads(ms, sub), grads(fresh().set_loss_pairs(sub), sub))
    assert all(bool(torch.isnan(gr).all()) for gr in grads(ms, masks[1]))      # promise broken: NaN, not garbage
    with pytest.raises(RuntimeError, match="outside the declared loss pairs"):
        grads(md, masks[1])
    with pytest.raises(ValueError, match="needs the loss masks"):
        fresh().assume_static_loss_masks()
    # index pairs instead of masks
    r, c = torch.nonzero(masks[0], as_tuple=True)
    for got, ref in zip(grads(fresh().set_loss_pairs((r, c), n_nodes=N), masks[0]), want[0]):
        assert torch.equal(got, ref)


def test_registered_torch_operators_match_the_module_and_compile_without_graph_breaks():
    """torch.ops.disenlink.* (torch.library registrations over the C ABI): the module with use_torch_ops=True gives the
    same probabilities and parameter gradients as the default ctypes path; torch.library.opcheck passes on the scorer
    (schema, fake implementation, autograd registration); and torch.compile(fullgraph=True) traces the whole
    forward_pairs step (the aot_eager backend: tracing and functionalisation, no code generation)."""
    import disenlink_amd.torch_ops as to
    from disenlink_amd.graph import Graph, PairList
    from disenlink_amd.model import Disentangle
    N, F, K, d = 300, 24, 8, 64
    src, dst, _Zh, rng = _random_problem(33, N, K, d, 10)
    G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
    pairs = PairList.build(torch.from_numpy(rng.integers(0, N, 2000)).to(DEV), torch.from_numpy(rng.integers(0, N, 2000)).to(DEV), N)
    x = torch.from_numpy((rng.standard_normal((N, F)) * 0.5).astype(np.float32)).to(DEV)
    lab = (torch.rand(2000, device=DEV) < 0.3).float()

    def make(flag):
        torch.manual_seed(4)
        return Disentangle(F, 32, d, nfactor=K, beta=0.6, use_torch_ops=flag).to(DEV)

    def run(model, fn=None):
        model.zero_grad()
        emb, prob = (fn or model.forward_pairs)(x, G, pairs)
        torch.nn.functional.binary_cross_entropy(prob, lab).backward()
        return emb.detach(), prob.detach(), [p.grad.clone() for p in model.parameters()]

    e0, p0, g0 = run(make(False))
    m1 = make(True)
    e1, p1, g1 = run(m1)
    assert torch.equal(p1, p0) and torch.equal(e1, e0)
    for a_, b_ in zip(g1, g0):
        assert torch.allclose(a_, b_, rtol=1e-5, atol=1e-8)
    hg, hp = to.register_graph(G), to.register_pairs(pairs)
    Z = m1.project(x).detach()
    H = torch.ops.disenlink.route_aggregate(Z, hg, 0.6, 1.0)[0]
    torch.library.opcheck(torch.ops.disenlink.score_pairs_terms.default, (Z.requires_grad_(True), H.requires_grad_(True), hp, 1.0),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    torch._dynamo.reset()
    compiled = torch.compile(m1.forward_pairs, fullgraph=True, backend="aot_eager")
    e2, p2, g2 = run(m1, compiled)
    assert torch.equal(p2, p0) and torch.equal(e2, e0)
    for a_, b_ in zip(g2, g0):
        assert torch.allclose(a_, b_, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("case", ["k4_d8", "k5_d64"])
def test_dense_backward_under_fixed_masks_while_saturation_moves(case):
    """tests/golden/adam_*.npz — 12 Adam steps of the REFERENCE model under fixed masks: the non-zero set of
    d loss / d link_pred grows from step to step (k4_d8: 264 -> 295 of 295 masked entries, k5_d64: 805 -> 1,063) because
    saturated positives carry exactly zero gradient until they de-saturate.  The drop-in module must follow the
    reference's losses and end at its weights in every mode: masks declared + no host read (static), masks declared +
    validated, and nothing declared — the plan learnt from the caller's indexing of link_pred (ops.LinkPred: complete at the
    first backward) and, with that switched off, from the gradients alone (growing).  The two declared modes share one plan
    and must agree bit for bit."""
    import json
    import os
    import torch.nn.functional as F
    from conftest import GOLDEN_DIR
    from disenlink_amd.model import Disentangle
    c = load_golden(case)
    g = dict(np.load(os.path.join(GOLDEN_DIR, f"adam_{case}.npz"), allow_pickle=False))
    am, m = json.loads(str(g["meta"])), c["meta"]
    x, adj, ori = (torch.from_numpy(c[k]).to(DEV) for k in ("x", "adj", "ori_adj"))
    pm, nm = torch.from_numpy(c["pos_mask"]).to(DEV), torch.from_numpy(c["neg_mask"]).to(DEV)

    def run(mode):
        os.environ["DL_LINK_PRED_SUBCLASS"] = "0" if mode == "learnt" else "1"      # "learnt": from the gradients alone; "indexed": from a_pred[mask]
        model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"])
        model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("sd__")})
        model = model.to(DEV)
        if mode == "static":
            model.assume_static_loss_masks(pm, nm)               # the SUMMED masks as the caller holds them (entries 2, 3 too)
        elif mode == "declared":
            model.set_loss_pairs(pm, nm)
        opt = torch.optim.Adam(model.parameters(), lr=am["lr"], weight_decay=am["weight_decay"])
        losses, nnz, plan = [], [], []
        for step in range(am["steps"]):
            _emb, a_pred = model(x, adj)
            a_pred.retain_grad()
            loss = (F.binary_cross_entropy(a_pred[pm == 1].unsqueeze(0), ori[pm == 1].unsqueeze(0))
                    + F.binary_cross_entropy(a_pred[nm == 1].unsqueeze(0), ori[nm == 1].unsqueeze(0)) / m["m"])
            opt.zero_grad()
            loss.backward()
            losses.append(loss.item())
            nnz.append(int(torch.count_nonzero(a_pred.grad)))
            plan.append(model._dense_plan.flat.numel())
            assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters()), (mode, step)
            opt.step()
        return losses, nnz, plan, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}

    try:
        runs = {mode: run(mode) for mode in ("static", "declared", "learnt", "indexed")}
    finally:
        os.environ.pop("DL_LINK_PRED_SUBCLASS", None)
    for mode, (losses, nnz, plan, sd) in runs.items():
        np.testing.assert_allclose(losses, g["losses"], rtol=5e-5, err_msg=mode)
        # the same entries saturate as in the reference (an entry whose logit sits on the fp32 boundary p == 1.0 may differ)
        assert np.abs(np.array(nnz) - g["nnz_grad"]).max() <= 2 and nnz[0] < nnz[-1], (mode, nnz)
        for k, v in sd.items():
            np.testing.assert_allclose(v, g["sd__" + k], rtol=5e-4, atol=5e-6, err_msg=f"{mode} {k}")
    assert runs["static"][0] == runs["declared"][0]                 # bit for bit: losses ...
    for k in runs["static"][3]:
        assert np.array_equal(runs["static"][3][k], runs["declared"][3][k]), k      # ... and weights
    assert runs["learnt"][2][0] < runs["learnt"][2][-1] <= int(g["n_masked"])        # the learnt plan grew towards the masks
    assert runs["learnt"][2][-1] >= int(g["n_masked"]) - 2
    assert set(runs["indexed"][2]) == {int(((pm == 1) | (nm == 1)).sum())}         # from the indexing: the entries the loss takes, at once
    assert set(runs["static"][2]) == {int(((pm != 0) | (nm != 0)).sum())}


@pytest.mark.parametrize("name", __import__("conftest").trajectory_names())
def test_dropin_module_follows_the_reference_training_trajectory(name):
    """The reference's own loop (model(x, adj_sym), dense masks, Adam, main_disentangled.py:150,191-219) around the
    drop-in module, against trajectories recorded from the reference model: losses, validation AUCs, test AUC."""
    import torch.nn.functional as F
    from conftest import load_trajectory
    from disenlink_amd.model import Disentangle
    g = load_trajectory(name)
    m = g["meta"]
    model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"])
    model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")})
    model = model.to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=m["lr"], weight_decay=5e-4)
    x, adj, ori = (torch.from_numpy(g[k]).to(DEV) for k in ("x", "adj", "ori_adj"))
    mk = {k[6:]: torch.from_numpy(g[k]).to(DEV) for k in g if k.startswith("mask__")}
    best, kept = 0.0, None
    for ep in range(m["epochs"]):
        model.train()
        _emb, a_pred = model(x, adj)
        loss = (F.binary_cross_entropy(a_pred[mk["pos_train"] == 1].unsqueeze(0), ori[mk["pos_train"] == 1].unsqueeze(0))
                + F.binary_cross_entropy(a_pred[mk["neg_train"] == 1].unsqueeze(0), ori[mk["neg_train"] == 1].unsqueeze(0)) / m["m"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        model.eval()
        auc = metrics_ref.auc_tie_avg(ori[mk["val"] == 1].cpu().numpy(), a_pred[mk["val"] == 1].detach().cpu().numpy())
        assert abs(loss.item() - g["losses"][ep]) <= 2e-4 * abs(g["losses"][ep]), (ep, loss.item(), g["losses"][ep])
        assert abs(auc - g["val_aucs"][ep]) <= 2e-3, (ep, auc, g["val_aucs"][ep])
        if auc > best:
            best, kept = auc, {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.load_state_dict(kept)
    _emb, a_pred = model(x, adj)
    test_auc = metrics_ref.auc_tie_avg(ori[mk["test"] == 1].cpu().numpy(), a_pred[mk["test"] == 1].detach().cpu().numpy())
    assert abs(test_auc - float(g["test_auc"])) <= 5e-3


@pytest.mark.parametrize("name", ["chameleon", "cora", "squirrel", "texas"])
def test_real_data_auc_parity_with_the_reference_model(name):
    """BASELINE.json: "chameleon, K=8, d=64, fp32" and "Cora, K=4, d=32" ... "AUC parity vs the CPU reference within
    1e-4 on the same edge splits".  tests/golden/real_<name>.npz holds the real dataset arrays and what the reference
    model produced on CPU (30 epochs of the reference schedule, make_real_data.py).  Here: the same data, split and
    seeded initial weights through (a) the drop-in module inside the reference's dense-mask loop and (b) the scalable
    pair-list loop — per-epoch loss, validation AUC and the final test AUC.  (All three run the projection kernels:
    Cora's 1,433 features exercise the padded feature tails of the plane arrays; squirrel = the real 217k-row edge
    list with seeded features, the configuration the benchmark is quoted on; texas = WebKB at hyperparameters_setting:5,
    183 nodes and 1,703 features: a graph far smaller than one launch's grid, K = 5.)"""
    import json
    import os
    import torch.nn.functional as F
    from conftest import GOLDEN_DIR
    from disenlink_amd.datasets import standardise_rows
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    g = np.load(os.path.join(GOLDEN_DIR, f"real_{name}.npz"))
    m = json.loads(str(g["meta"]))
    edges = g["edges"].astype(np.int64)
    if "features" in g:                                             # chameleon: rows standardised (main_disentangled.py:97-101)
        feats = g["features"]
        x = torch.from_numpy(standardise_rows(feats)).to(DEV)
    elif "feat_seed" in g:                                          # squirrel: real edge list, seeded N(0,1) features (blob missing)
        feats = np.random.default_rng(int(g["feat_seed"])).standard_normal(tuple(g["feat_shape"]), dtype=np.float32)
        x = torch.from_numpy(standardise_rows(feats)).to(DEV)
    else:                                                           # Cora: binary features as they are (:117-123);
        feats = np.zeros(tuple(g["feat_shape"]), dtype=np.float32)  # texas (WebKB): binary, then standardised (:91-96)
        feats[g["feat_row"].astype(np.int64), g["feat_col"].astype(np.int64)] = 1.0
        x = torch.from_numpy(standardise_rows(feats) if "standardise" in g else feats).to(DEV)
    n = feats.shape[0]
    split = make_link_split(edges[:, 0], edges[:, 1], n, m=m["m"], seed=m["split_seed"])
    assert (split.pos_train.u.size, split.neg_train.u.size, split.val.u.size, split.test.u.size) == \
        (m["n_pos"], m["n_neg"], m["n_val"], m["n_test"])

    def fresh():
        torch.manual_seed(m["seed"])                                # same creation order as the reference: same weights
        return Disentangle(feats.shape[1], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"]).to(DEV)

    # (b) the scalable loop on pair lists
    res = run_link_prediction(fresh(), x, prepare_run(split, torch.device(DEV), row_bytes=m["K"] * m["d"] * 4),
                              epochs=m["epochs"], lr=m["lr"], use_graph=False)
    np.testing.assert_allclose(res.losses[:12], g["losses"][:12], rtol=5e-5)     # identical start ...
    np.testing.assert_allclose(res.losses, g["losses"], rtol=1e-3)               # ... fp32 noise grows through training
    assert np.abs(np.array(res.val_aucs) - g["val_aucs"]).max() <= 1e-4, np.abs(np.array(res.val_aucs) - g["val_aucs"]).max()
    assert abs(res.test_auc - float(g["test_auc"])) <= 1e-4, (res.test_auc, float(g["test_auc"]))

    # (a) the reference's own loop around the drop-in module
    def dense(u, v):
        a = torch.zeros(n, n, device=DEV)
        a[torch.from_numpy(u).to(DEV), torch.from_numpy(v).to(DEV)] = 1
        return a
    ori = dense(edges[:, 0], edges[:, 1])
    adj = dense(split.train_src, split.train_dst)
    adj_sym = ((adj + adj.t()) != 0).float()
    mk = {"pos": dense(split.pos_train.u, split.pos_train.v) == 1, "neg": dense(split.neg_train.u, split.neg_train.v) == 1,
          "val": dense(split.val.u, split.val.v) == 1, "test": dense(split.test.u, split.test.v) == 1}
    model = fresh()
    if name == "chameleon":                                        # the sync-free mode on the reference's loop: masks declared once
        model.assume_static_loss_masks(mk["pos"], mk["neg"])       # (cora / squirrel: nothing declared, the plan is learnt and grows)
    opt = torch.optim.Adam(model.parameters(), lr=m["lr"], weight_decay=5e-4)
    best, kept = 0.0, None
    for ep in range(m["epochs"]):
        _emb, a_pred = model(x, adj_sym)
        loss = (F.binary_cross_entropy(a_pred[mk["pos"]].unsqueeze(0), ori[mk["pos"]].unsqueeze(0))
                + F.binary_cross_entropy(a_pred[mk["neg"]].unsqueeze(0), ori[mk["neg"]].unsqueeze(0)) / m["m"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        auc = metrics_ref.auc_tie_avg(ori[mk["val"]].cpu().numpy(), a_pred[mk["val"]].detach().cpu().numpy())
        assert abs(loss.item() - g["losses"][ep]) <= (5e-5 if ep < 12 else 1e-3) * g["losses"][ep], (ep, loss.item(), g["losses"][ep])
        assert abs(auc - g["val_aucs"][ep]) <= 1e-4, (ep, auc, g["val_aucs"][ep])
        if auc > best:
            best, kept = auc, {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.load_state_dict(kept)
    _emb, a_pred = model(x, adj_sym)
    test_auc = metrics_ref.auc_tie_avg(ori[mk["test"]].cpu().numpy(), a_pred[mk["test"]].detach().cpu().numpy())
    assert abs(test_auc - float(g["test_auc"])) <= 1e-4, (test_auc, float(g["test_auc"]))


def test_projection_kernels_on_random_shapes():
    """Fuzz: 40 random (N, F, K, nhid, d) incl. N, F, nhid of 1-3 and sizes around the 32 / 64 / 128 tile edges, through
    the forward and both forms of the backward (recompute / kept hidden layer), against fp64."""
    from disenlink_amd import ops
    rng = np.random.default_rng(77)
    for it in range(40):
        d = int(rng.choice([32, 64, 128]))
        N = int(rng.choice([1, 2, 3, 31, 33, 127, 128, 129, 200, 257, 640]))
        F = int(rng.choice([1, 2, 3, 4, 31, 32, 33, 63, 65, 100, 129]))
        K = int(rng.integers(1, 6))
        nhid = int(rng.choice([2, 3, 4, 31, 33, 64, 65, 127, 128, 129, 200]))
        g = torch.Generator().manual_seed(it)
        x = torch.randint(-2, 3, (N, F), generator=g).float()             # exact layer-1 sums: the ReLU mask is unambiguous
        W1 = torch.randint(-8, 9, (K, nhid, F), generator=g).float() / 64
        b1 = torch.randint(-8, 9, (K, nhid), generator=g).float() / 64
        W2 = torch.randn(K, d, nhid, generator=g) / nhid ** 0.5
        b2 = torch.randn(K, d, generator=g) * 0.1
        dZ = torch.randn(N, K, d, generator=g)
        X, G = x.double(), dZ.double()
        pre = torch.einsum("nf,khf->nkh", X, W1.double()) + b1.double()
        hid = pre.clamp_min(0)
        Zref = torch.einsum("nkh,kdh->nkd", hid, W2.double()) + b2.double()
        dh = torch.einsum("nkd,kdh->nkh", G, W2.double()) * (pre > 0)
        ref = (torch.einsum("nkh,nf->khf", dh, X), dh.sum(0), torch.einsum("nkd,nkh->kdh", G, hid), G.sum(0))
        dev = [v.to(DEV) for v in (x, W1, b1, W2, dZ)]
        tag = (it, N, F, K, nhid, d)
        Z, kept = ops.project_fwd(dev[0], dev[1], dev[2], dev[3], b2.to(DEV), keep_hid=True)
        assert float((Z.cpu().double() - Zref).abs().max()) <= 2e-5 * max(float(Zref.abs().max()), 1e-6), tag
        for form, hid_arg in (("recompute", None), ("kept", kept)):
            for name, got, want in zip(("dW1", "db1", "dW2", "db2"), ops.project_bwd(*dev, hid=hid_arg), ref):
                assert torch.isfinite(got).all(), (name, form, tag)
                err = float((got.cpu().double() - want).abs().max())
                assert err <= 2e-5 * max(float(want.abs().max()), 1e-6), (name, form, tag, err)


def test_tuned_and_generic_kernels_agree_on_random_small_problems():
    """Fuzz: 60 random small problems (node counts around the segment / slice / tile edges, random plans) through both
    independent implementations (tuned per-(K,d) kernels and the generic ones): forward and backward must agree."""
    from disenlink_amd import _lib, ops
    from disenlink_amd.graph import Graph, PairList
    lib = _lib.load()
    rng = np.random.default_rng(2024)
    shapes = [(8, 64), (4, 32), (5, 64), (16, 128), (3, 8), (10, 32), (8, 8)]
    for it in range(60):
        K, d = shapes[it % len(shapes)]
        N = int(rng.integers(1, 200))
        E = int(rng.integers(0, 6 * N + 1))
        src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
        P = int(rng.integers(0, 5 * N + 1))
        pu, pv = rng.integers(0, N, P), rng.integers(0, N, P)
        seg_len = int(rng.choice([1, 3, 8, 32]))
        beta, t = float(rng.choice([0.5, 0.7, 0.9])), float(rng.choice([1.0, 2.0]))
        Z = torch.from_numpy((rng.standard_normal((N, K, d)) * 0.3).astype(np.float32)).to(DEV)
        G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N, seg_len=seg_len).to(DEV)
        pairs = PairList.build(torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV), N,
                               seg_len=int(rng.choice([2, 5, 32])), n_slices=int(rng.choice([1, 8, 16])))
        gp = torch.from_numpy(rng.standard_normal(P).astype(np.float32) * 0.1).to(DEV)
        out = {}
        for force in (0, 1):
            old = lib.dl_set_force_generic(force)
            try:
                p, a, s = ops.route_fwd(G, Z, t)
                H = ops.aggregate_fwd(G, Z, beta, p, a, s)
                prob = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs if force == 0 else None)
                dZs, dH = ops.score_pairs_bwd(Z, H, pairs, t, prob, gp)
                dZ = ops.route_aggregate_bwd(G, Z, beta, t, p, a, s, dH.clone(), dZ_accum=dZs.clone())
                out[force] = (p, a, s, H, prob, dZs, dH, dZ)
            finally:
                lib.dl_set_force_generic(old)
        tag = (it, N, E, P, K, d, seg_len)
        same = out[0][0] == out[1][0]                                  # near-ties may route differently: skip those problems
        if not bool(same.all()):
            continue
        for name, x0, x1 in zip(("a", "s", "H", "prob", "dZs", "dH", "dZ"), out[0][1:], out[1][1:]):
            assert torch.isfinite(x0).all(), (name, tag)
            scale = max(float(x1.abs().max()) if x1.numel() else 0.0, 1e-6)
            assert float((x0 - x1).abs().max()) <= 2e-4 * scale if x0.numel() else True, (name, tag)


def test_aggregation_under_skewed_routing():
    """The aggregation kernel owns accumulators per factor CLASS (factor mod 4) and walks max-class-size steps per
    segment: the worst cases are routings that send every edge to one factor or to two factors of the same class.
    Hand-made (p, a, s) on a graph with a hub row (multi-unit partial slots), through the tuned and the generic kernels
    and against an fp64 sum: same H whatever the routing looks like."""
    from disenlink_amd import _lib, ops
    from disenlink_amd.graph import Graph
    lib = _lib.load()
    rng = np.random.default_rng(77)
    for K, d in ((8, 64), (5, 32), (16, 128), (3, 8)):
        N = 700
        src = np.concatenate([rng.integers(0, N, 3000), np.zeros(600, dtype=np.int64)])      # node 0: a hub of ~600 entries
        dst = np.concatenate([rng.integers(0, N, 3000), rng.integers(1, N, 600)])
        G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
        E = G.n_edges
        rowptr = G.plan.rowptr.cpu().numpy().astype(np.int64)
        col = G.plan.col.cpu().numpy().astype(np.int64)
        row = np.repeat(np.arange(N), np.diff(rowptr))
        Zh = (rng.standard_normal((N, K, d)) * 0.5).astype(np.float32)
        ah = rng.uniform(0.1, 1.0, E).astype(np.float32)
        sh = rng.uniform(0.5, 2.0, (N, K)).astype(np.float32)
        patterns = {"all_first": np.zeros(E, np.int64), "all_last": np.full(E, K - 1), "one_class": (np.arange(E) % 2) * (4 if K > 4 else 0),
                    "by_parity": np.arange(E) % K, "random": rng.integers(0, K, E)}
        Z, a, sv = (torch.from_numpy(v).to(DEV) for v in (Zh, ah, sh))
        for name, ph in patterns.items():
            ph = np.minimum(ph, K - 1)
            pt = torch.from_numpy(ph.astype(np.uint8)).to(DEV)
            want = 0.4 * Zh.astype(np.float64)
            w = ah.astype(np.float64) / sh.astype(np.float64)[col, ph]
            np.add.at(want, (row, ph), 0.6 * w[:, None] * Zh.astype(np.float64)[col, ph])
            got = {}
            for force in (0, 1):
                old = lib.dl_set_force_generic(force)
                try:
                    got[force] = ops.aggregate_fwd(G, Z, 0.4, pt, a, sv).cpu().numpy().astype(np.float64)
                finally:
                    lib.dl_set_force_generic(old)
            scale = float(np.abs(want).max())
            for force in (0, 1):
                assert np.abs(got[force] - want).max() <= 2e-5 * scale, (K, d, name, force, float(np.abs(got[force] - want).max()))


def test_scaled_backward_is_the_backward_times_a_device_scalar():
    """dl_route_aggregate_bwd_scaled: dZ = scale * (dZ_in + backward(dH)) with the inputs only read.  scale == 1 gives the
    bits of the accumulating entry point; any other scale agrees to rounding; tuned and generic kernels; a graph with hub
    rows (partial slots + combine).  And through autograd: (c * loss).backward() of the one-pass loss node equals c times
    the gradients of loss.backward()."""
    from disenlink_amd import _lib, ops
    from disenlink_amd.graph import Graph, PairList
    lib = _lib.load()
    rng = np.random.default_rng(5)
    for K, d in ((8, 64), (5, 32), (3, 8)):
        N = 500
        src = np.concatenate([rng.integers(0, N, 2500), np.zeros(400, dtype=np.int64)])
        dst = np.concatenate([rng.integers(0, N, 2500), rng.integers(1, N, 400)])
        G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
        Z = torch.from_numpy((rng.standard_normal((N, K, d)) * 0.3).astype(np.float32)).to(DEV)
        dH = torch.from_numpy(rng.standard_normal((N, K, d)).astype(np.float32)).to(DEV)
        dZ_in = torch.from_numpy(rng.standard_normal((N, K, d)).astype(np.float32)).to(DEV)
        for force in (0, 1):
            old = lib.dl_set_force_generic(force)
            try:
                p, a, sv = ops.route_fwd(G, Z, 1.0)
                want = ops.route_aggregate_bwd(G, Z, 0.6, 1.0, p, a, sv, dH, dZ_accum=dZ_in.clone())
                keep_dH, keep_in = dH.clone(), dZ_in.clone()
                one = ops.route_aggregate_bwd_scaled(G, Z, 0.6, 1.0, p, a, sv, dH, dZ_in, torch.ones((), device=DEV))
                assert torch.equal(one, want), (K, d, force)
                assert torch.equal(dH, keep_dH) and torch.equal(dZ_in, keep_in)            # inputs are only read
                c = torch.tensor(0.37, device=DEV)
                got = ops.route_aggregate_bwd_scaled(G, Z, 0.6, 1.0, p, a, sv, dH, dZ_in, c)
                assert torch.allclose(got, want * 0.37, rtol=1e-6, atol=1e-7 * float(want.abs().max())), (K, d, force)
            finally:
                lib.dl_set_force_generic(old)
    # autograd: a scaled loss
    N, K, d = 400, 8, 64
    src, dst = rng.integers(0, N, 3000), rng.integers(0, N, 3000)
    G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
    pairs = PairList.build(torch.from_numpy(rng.integers(0, N, 5000)).to(DEV), torch.from_numpy(rng.integers(0, N, 5000)).to(DEV), N)
    label = torch.from_numpy((rng.random(5000) < 0.3).astype(np.float32)).to(DEV)
    weight = torch.from_numpy(rng.uniform(0.1, 1.0, 5000).astype(np.float32)).to(DEV)
    grads = {}
    for c in (1.0, 2.5):
        Z = torch.from_numpy((np.random.default_rng(9).standard_normal((N, K, d)) * 0.3).astype(np.float32)).to(DEV).requires_grad_()
        _emb, _prob, loss = ops.HotPathPairsLoss.apply(Z, G, pairs, 0.5, 1.0, torch.float32, label, weight)
        (loss * c).backward()
        grads[c] = Z.grad.clone()
    assert torch.isfinite(grads[1.0]).all() and float(grads[1.0].abs().max()) > 0
    assert torch.allclose(grads[2.5], grads[1.0] * 2.5, rtol=1e-5, atol=1e-7 * float(grads[1.0].abs().max()))


def test_routing_by_peer_block_on_the_gpu_equals_one_routing_pass():
    """dist.Shard.route_by_peer through the kernels: rank 0 .. 3 of a 4-way shard of a squirrel-shaped graph, the Z table
    revealed peer block by peer block (blocks that have not "arrived" are NaN): p, a and the rank's rows of s equal one
    routing pass over the complete table bit for bit, and nothing read a block before its arrival."""
    from disenlink_amd import dist as dd
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.splits import make_link_split
    sg = synthetic_graph("chameleon", seed=4)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=2, seed=4)
    pu = np.concatenate([split.pos_train.u, split.neg_train.u])
    pv = np.concatenate([split.pos_train.v, split.neg_train.v])
    o = np.argsort(pu, kind="stable")
    pu, pv = pu[o], pv[o]
    world, K, d = 4, 8, 64
    be = dd.HipBackend()
    for rank in range(world):
        shard = dd.Shard.build(rank, world, sg.n_nodes, split.train_src, split.train_dst, pu, pv, DEV, row_bytes=K * d * 4,
                               with_backward=False, z_by_peer=True)
        assert len(shard.route_by_peer) == world
        B = shard.part.block
        torch.manual_seed(rank)
        Zfull = torch.randn(shard.n_pad, K, d, device=DEV) * 0.3
        s_ref = torch.zeros((shard.n_pad, K), device=DEV)
        p_ref, a_ref = be.route_fwd(shard.graph, Zfull, 1.0, s_ref)

        class Reveal:
            def __init__(self, Z):
                self.Z, self.seen = Z, []
            def wait(self, q):
                self.Z[q * B:(q + 1) * B] = Zfull[q * B:(q + 1) * B]
                self.seen.append(q)
            def wait_all(self):
                for q in range(world):
                    if q not in self.seen and q != rank:
                        self.wait(q)
        Z = torch.full_like(Zfull, float("nan"))
        Z[shard.lo:shard.hi] = Zfull[shard.lo:shard.hi]
        s = torch.full((shard.n_pad, K), float("nan"), device=DEV)
        p, a = dd.route_in_arrival_order(be, shard, Z, 1.0, s, Reveal(Z))
        assert torch.equal(p, p_ref) and torch.equal(a, a_ref) and not torch.isnan(a).any()
        assert torch.equal(s[shard.lo:shard.hi], s_ref[shard.lo:shard.hi])


def test_launches_follow_the_callers_stream():
    """The library binds to torch's HIP runtime, so a non-default torch stream is honoured."""
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph
    K, d, N = 8, 64, 3000
    src, dst, Zh, _rng = _random_problem(7, N, K, d, 20)
    G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
    Z = torch.from_numpy(Zh).to(DEV)
    p0, a0, s0 = ops.route_fwd(G, Z, 1.0)
    H0 = ops.aggregate_fwd(G, Z, 0.5, p0, a0, s0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Zs = Z * 1.0                                   # produced on the side stream, consumed by our kernels
        for _ in range(5):
            p1, a1, s1 = ops.route_fwd(G, Zs, 1.0)
            H1 = ops.aggregate_fwd(G, Zs, 0.5, p1, a1, s1)
    side.synchronize()
    assert torch.equal(H0, H1) and torch.equal(p0, p1)


def test_training_trajectory_matches_cpu_oracle():
    """Same splits, same init, same schedule (main_disentangled.py:191-224): the HIP module's loss and
    validation-AUC trajectory vs the dense CPU oracle's.  Trajectories drift apart with training
    (hard arg-max routing + fp32 sigmoid saturation), so the gate is tight on
    the first epochs and statistical (1e-3 level) at the end."""
    from test_train_cpu import OraclePairModule
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    sg = synthetic_graph("chameleon", seed=3, scale=0.12)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=1)
    F, nhid, d, K = 32, 24, 32, 4
    x = sg.features()[:, :F].copy()
    torch.manual_seed(1)
    ref_inner = Disentangle(F, nhid, d, nfactor=K, beta=0.7, t=1)
    sd = {k: v.clone() for k, v in ref_inner.state_dict().items()}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                    # a reproducible CPU side: multi-threaded reductions vary run to run
    try:
        res_cpu = run_link_prediction(OraclePairModule(ref_inner), torch.from_numpy(x), prepare_run(split, "cpu"),
                                      epochs=12, lr=1e-3)
    finally:
        torch.set_num_threads(threads)
    gpu = Disentangle(F, nhid, d, nfactor=K, beta=0.7, t=1)
    gpu.load_state_dict(sd)
    gpu = gpu.to(DEV)
    res_gpu = run_link_prediction(gpu, torch.from_numpy(x).to(DEV), prepare_run(split, DEV), epochs=12, lr=1e-3)
    assert abs(res_gpu.losses[0] - res_cpu.losses[0]) <= 1e-5 * abs(res_cpu.losses[0])
    assert abs(res_gpu.val_aucs[0] - res_cpu.val_aucs[0]) <= 1e-4            # fixed weights: the hard gate
    for lg, lc in zip(res_gpu.losses[:4], res_cpu.losses[:4]):
        assert abs(lg - lc) <= 1e-3 * abs(lc)
    # the end of a 12-epoch run on a tiny graph is a statistical statement (hard routing amplifies rounding); the
    # tight end-to-end gates are the real-data trajectories recorded from the reference model (test_real_data_...)
    assert abs(res_gpu.val_aucs[-1] - res_cpu.val_aucs[-1]) <= 1e-2
    assert abs(res_gpu.test_auc - res_cpu.test_auc) <= 1e-2
    assert res_gpu.losses[-1] < res_gpu.losses[0]


def _bf16_round(x):
    return torch.from_numpy(x).to(torch.bfloat16).float().numpy()


@pytest.mark.parametrize("K,d,N,deg", [(8, 64, 600, 12), (16, 128, 300, 10), (4, 32, 400, 8), (8, 32, 300, 8)])
def test_bf16_tables_match_the_oracle_on_bf16_rounded_inputs(K, d, N, deg):
    """bf16 storage of the gathered tables (config 5 of BASELINE.json), fp32 arithmetic.  The reference has
    no bf16 path, so the check is against the fp32 oracle evaluated on the SAME bf16-rounded tables:
    what remains is fp32 summation order (+ one bf16 rounding of H)."""
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph, PairList
    beta, t = 0.6, 1.0
    src, dst, Zh, rng = _random_problem(K * 77 + d, N, K, d, deg, scale=0.3)
    Zr = _bf16_round(Zh)
    G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
    rowptr, col, rev = sparse_ref.csr_from_pairs(src, dst, N, symmetrise=True)
    Zb = torch.from_numpy(Zh).to(DEV).to(torch.bfloat16)
    p, a, s = ops.route_fwd(G, Zb, t)
    p_o, a_o, alpha, _s = sparse_ref.route(Zr, rowptr, col, t)
    ok = _decisive(alpha)
    assert (p.cpu().numpy()[ok] == p_o[ok]).all()
    np.testing.assert_allclose(a.cpu().numpy()[ok], a_o[ok], rtol=1e-5)
    p_h, a_h, s_h = p.cpu().numpy(), a.cpu().numpy(), s.cpu().numpy()
    Hb = ops.aggregate_fwd(G, Zb, beta, p, a, s)
    assert Hb.dtype == torch.bfloat16
    H_o = sparse_ref.aggregate(Zr, rowptr, col, p_h, a_h, s_h, beta)
    np.testing.assert_allclose(Hb.float().cpu().numpy(), H_o, rtol=1e-2, atol=1e-3)      # one bf16 rounding
    Hr = Hb.float().cpu().numpy()
    P = 3000
    pu, pv = rng.integers(0, N, P), rng.integers(0, N, P)
    pairs = PairList.build(torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV), N, row_bytes=K * d * 2)
    prob, coef = ops.score_pairs_fwd(Zb, Hb, pairs.pu, pairs.pv, t, pairs, want_coef=True)
    prob_o = sparse_ref.score_pairs(Zr, Hr, pu, pv, t)
    np.testing.assert_allclose(prob.cpu().numpy(), prob_o, rtol=1e-5, atol=1e-5)
    gp = (rng.standard_normal(P) * 0.1).astype(np.float32)
    tol = lambda ref: 1e-4 * max(np.abs(ref).max(), 1e-6)
    dZs_o, dH_o = sparse_ref.score_pairs_bwd(Zr, Hr, pu, pv, t, gp)
    for cf in (coef, None):
        dZs, dH = ops.score_pairs_bwd(Zb, Hb, pairs, t, prob, torch.from_numpy(gp).to(DEV), coef=cf)
        assert dZs.dtype == torch.float32
        assert np.abs(dH.cpu().numpy() - dH_o).max() <= tol(dH_o)
        assert np.abs(dZs.cpu().numpy() - dZs_o).max() <= tol(dZs_o)
    dZ = ops.route_aggregate_bwd(G, Zb, beta, t, p, a, s, dH)
    dZ_o = sparse_ref.route_aggregate_bwd(Zr, rowptr, col, rev, p_h, a_h, s_h, beta, t, dH_o)
    assert np.abs(dZ.cpu().numpy() - dZ_o).max() <= tol(dZ_o)


def test_bf16_module_auc_close_to_fp32():
    """ΔAUC of bf16 table storage vs fp32 on the same weights and pairs (reported tolerance 2e-3; the
    reference defines none) and fp32 gradients through the fused autograd node."""
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.metrics import auc_tie_avg, pair_bce_loss
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run
    sg = synthetic_graph("chameleon", seed=5, scale=0.3)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=2)
    run = prepare_run(split, DEV)
    x = torch.from_numpy(sg.features()[:, :64].copy()).to(DEV)
    torch.manual_seed(3)
    m32 = Disentangle(64, 128, 64, nfactor=8, beta=0.7, t=1).to(DEV)
    m16 = Disentangle(64, 128, 64, nfactor=8, beta=0.7, t=1, table_dtype=torch.bfloat16).to(DEV)
    m16.load_state_dict(m32.state_dict())
    out = {}
    for name, mdl in (("f32", m32), ("bf16", m16)):
        _emb, prob = mdl.forward_pairs(x, run.graph, run.train_val_pairs)
        a, b = run.n_pos, run.n_pos + run.n_neg
        loss = pair_bce_loss(prob[:a], run.label_pos, prob[a:b], run.label_neg, run.m)
        mdl.zero_grad()
        loss.backward()
        out[name] = (float(auc_tie_avg(run.label_val, prob[b:])), float(loss),
                     torch.cat([p.grad.reshape(-1) for p in mdl.parameters()]))
    assert abs(out["bf16"][0] - out["f32"][0]) <= 2e-3
    assert abs(out["bf16"][1] - out["f32"][1]) <= 2e-2 * abs(out["f32"][1])
    g32, g16 = out["f32"][2], out["bf16"][2]
    assert g16.dtype == torch.float32 and torch.isfinite(g16).all()
    cos = torch.dot(g32, g16) / (g32.norm() * g16.norm())
    assert float(cos) > 0.98


@pytest.mark.parametrize("N,F,K,nhid,d", [(300, 128, 8, 512, 64), (131, 70, 4, 40, 32), (257, 33, 3, 1, 64),
                                           (64, 200, 2, 96, 128), (500, 1433, 4, 1, 32), (129, 64, 16, 33, 128)])
def test_mfma_projection_matches_cpu_mlp(N, F, K, nhid, d):
    """dl_project_fwd (fp32 MFMA, fused two-layer) vs K separate torch MLPs on the CPU, incl. ragged
    N / F / nhid tails; gradients of the autograd wrapper vs CPU autograd."""
    from disenlink_amd.model import Disentangle
    torch.manual_seed(N + F)
    ref = Disentangle(F, nhid, d, nfactor=K, beta=0.5, t=1)
    x = torch.randn(N, F)
    gpu = Disentangle(F, nhid, d, nfactor=K, beta=0.5, t=1, projection="mfma")
    gpu.load_state_dict(ref.state_dict())
    gpu = gpu.to(DEV)
    Z_ref = ref.project(x)                                     # CPU: library GEMM path
    Z = gpu.project(x.to(DEV))                                 # GPU: MFMA kernel
    assert Z.shape == (N, K, d)
    scale = float(Z_ref.abs().max())
    assert float((Z.cpu() - Z_ref).abs().max()) <= 2e-5 * max(scale, 1.0)
    w = torch.randn(N, K, d)
    (Z_ref * w).sum().backward()
    (Z * w.to(DEV)).sum().backward()
    for (name, pr), (_n, pg) in zip(ref.named_parameters(), gpu.named_parameters()):
        s = max(float(pr.grad.abs().max()), 1e-6)
        assert float((pg.grad.cpu() - pr.grad).abs().max()) <= 1e-4 * s, name


@pytest.mark.parametrize("N,F,K,nhid,d", [(5201, 128, 8, 512, 64), (1000, 50, 3, 40, 32), (257, 70, 2, 33, 128),
                                           (700, 128, 4, 1, 64), (4100, 300, 5, 64, 32), (90, 1433, 2, 1, 128),
                                           (2000, 129, 2, 100, 64)])
def test_projection_backward_kernels(N, F, K, nhid, d):
    """dl_project_bwd (recomputed hidden layer, node-range slabs) against an fp64 restatement of the MLP
    gradients (autograd of model.py:13-15 / 24-27): error relative to each gradient's largest entry within
    fp32 summation noise, no worse than the fp32 library form, and bitwise reproducible."""
    from disenlink_amd import ops
    g = torch.Generator().manual_seed(N * 7 + F)
    two = nhid > 1
    dZ = torch.randn(N, K, d, generator=g)
    if two:
        # layer 1 on small dyadic values: its sums are exact in fp32 in any order, so the ReLU mask cannot differ
        # from the fp64 one through rounding of a pre-activation next to zero
        x = torch.randint(-2, 3, (N, F), generator=g).float()
        W1 = torch.randint(-8, 9, (K, nhid, F), generator=g).float() / 64
        b1 = torch.randint(-8, 9, (K, nhid), generator=g).float() / 64
        W2 = torch.randn(K, d, nhid, generator=g) / nhid ** 0.5
    else:
        x = torch.randn(N, F, generator=g)
        W1, b1, W2 = torch.randn(K, d, F, generator=g) / F ** 0.5, torch.randn(K, d, generator=g), None

    def grads64():
        X, G = x.double(), dZ.double()
        if not two:
            return torch.einsum("nkd,nf->kdf", G, X), G.sum(0), None, None
        pre = torch.einsum("nf,khf->nkh", X, W1.double()) + b1.double()
        hid = pre.clamp_min(0)
        dh = torch.einsum("nkd,kdh->nkh", G, W2.double()) * (pre > 0)
        return torch.einsum("nkh,nf->khf", dh, X), dh.sum(0), torch.einsum("nkd,nkh->kdh", G, hid), G.sum(0)

    dev = [None if v is None else v.to(DEV) for v in (x, W1, b1, W2, dZ)]
    ref = grads64()
    for pad in (True, False):                  # False: rows of odd length go through the scalar-load kernels
        out = ops.project_bwd(*dev, pad=pad)
        again = ops.project_bwd(*dev, pad=pad)
        for name, got, rep, want in zip(("dW1", "db1", "dW2", "db2"), out, again, ref):
            if want is None:
                assert got is None
                continue
            assert got.shape == want.shape, name
            assert torch.equal(got, rep), name + " not reproducible"
            scale = float(want.abs().max())
            err = float((got.cpu().double() - want).abs().max())
            assert err <= 2e-5 * scale, (name, pad, err, scale)
    if two:                                    # backward from the KEPT hidden layer: same gradients, no recompute
        Zk, hid = ops.project_fwd(dev[0], dev[1], dev[2], dev[3], torch.zeros(K, d, device=DEV), keep_hid=True)
        ld = (N + 3) // 4 * 4                  # the padding columns of hidT [K][nhid][ld] belong to nobody: poison them
        hid.view(K, nhid, ld)[:, :, N:] = float("nan")
        kept = ops.project_bwd(*dev, hid=hid)
        for name, got, want in zip(("dW1", "db1", "dW2", "db2"), kept, ref):
            err = float((got.cpu().double() - want).abs().max())
            assert err <= 2e-5 * float(want.abs().max()), (name, "kept hidden layer", err)
        assert torch.equal(Zk, ops.project_fwd(dev[0], dev[1], dev[2], dev[3], torch.zeros(K, d, device=DEV)))
    if two:                                    # forward, both load paths, against fp64
        Zref = torch.einsum("nkh,kdh->nkd", (torch.einsum("nf,khf->nkh", x.double(), W1.double()) + b1.double()).clamp_min(0),
                            W2.double())
        for pad in (True, False):
            Z = ops.project_fwd(dev[0], dev[1], dev[2], dev[3], torch.zeros(K, d, device=DEV), pad=pad)
            assert float((Z.cpu().double() - Zref).abs().max()) <= 2e-5 * float(Zref.abs().max())


def test_projection_backward_in_node_blocks(lib_env):
    """Graphs whose masked hidden gradient would exceed the workspace cap are processed in node blocks that
    accumulate into the gradients (cap forced down here): same result as one block, up to summation order."""
    from disenlink_amd import ops
    g = torch.Generator().manual_seed(5)
    N, F, K, nhid, d = 10000, 48, 2, 64, 32
    x = torch.randint(-2, 3, (N, F), generator=g).float()
    W1 = torch.randint(-8, 9, (K, nhid, F), generator=g).float() / 64
    b1 = torch.randint(-8, 9, (K, nhid), generator=g).float() / 64
    W2 = torch.randn(K, d, nhid, generator=g) / 8
    dZ = torch.randn(N, K, d, generator=g)
    dev = [v.to(DEV) for v in (x, W1, b1, W2, dZ)]
    whole = ops.project_bwd(*dev)
    lib_env("DL_BWD_BLOCK_BYTES", 1 << 20)          # 4096-row blocks: 4096 + 4096 + 1808
    blocks = ops.project_bwd(*dev)
    _Z, hid = ops.project_fwd(dev[0], dev[1], dev[2], dev[3], torch.zeros(K, d, device=DEV), keep_hid=True)
    for name, a, b in zip(("dW1", "db1", "dW2", "db2"), whole, ops.project_bwd(*dev, hid=hid)):
        assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()), (name, "kept hidden layer, node blocks")
    for name, a, b in zip(("dW1", "db1", "dW2", "db2"), whole, blocks):
        assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()), name
    # the forward makes its x planes per node block on large graphs (block forced down here): same bits
    lib_env("DL_BWD_BLOCK_BYTES")
    b2 = torch.randn(K, d, generator=g).to(DEV)
    Z1, hid1 = ops.project_fwd(dev[0], dev[1], dev[2], dev[3], b2, keep_hid=True)
    lib_env("DL_FWD_BLOCK_ROWS", 8)                     # 1024-row blocks
    Z2, hid2 = ops.project_fwd(dev[0], dev[1], dev[2], dev[3], b2, keep_hid=True)
    ldh = (N + 3) // 4 * 4
    assert torch.equal(Z1, Z2) and torch.equal(hid1.view(K, nhid, ldh)[:, :, :N], hid2.view(K, nhid, ldh)[:, :, :N])


def test_projection_kernels_at_snap_patents_scale():
    """N = 2.9M nodes, F = 269 (snap-patents), K=8, nhid=512, d=64: the [N,K,nhid] hidden layer
    (48 GB) is never stored — forward fused, backward in 1 GiB node blocks.  Size-independent checks: rows of Z
    equal the same rows projected on their own; the gradients are additive over a split of the nodes."""
    from disenlink_amd import ops
    N, F, K, nhid, d = 2_923_922, 269, 8, 512, 64
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(N, F, device=DEV, generator=g)
    W1 = torch.randn(K, nhid, F, device=DEV, generator=g) / F ** 0.5
    b1 = torch.randn(K, nhid, device=DEV, generator=g) * 0.1
    W2 = torch.randn(K, d, nhid, device=DEV, generator=g) / nhid ** 0.5
    b2 = torch.randn(K, d, device=DEV, generator=g) * 0.1
    Z = ops.project_fwd(x, W1, b1, W2, b2)
    rows = torch.tensor([0, 1, 127, 128, 65_535, 65_536, 1_000_003, N - 129, N - 2, N - 1], device=DEV)
    Zs = ops.project_fwd(x[rows].contiguous(), W1, b1, W2, b2)
    assert float((Z[rows] - Zs).abs().max()) <= 1e-5 * float(Zs.abs().max())
    Zref = torch.einsum("nkh,kdh->nkd", (torch.einsum("nf,khf->nkh", x[rows].double(), W1.double()) + b1.double()).clamp_min(0),
                        W2.double()) + b2.double()
    assert float((Zs.double() - Zref).abs().max()) <= 2e-5 * float(Zref.abs().max())
    dZ = torch.randn(N, K, d, device=DEV, generator=g) * 1e-3
    full = ops.project_bwd(x, W1, b1, W2, dZ)
    cut = 1_234_567
    lo = ops.project_bwd(x[:cut], W1, b1, W2, dZ[:cut])
    hi = ops.project_bwd(x[cut:], W1, b1, W2, dZ[cut:])
    for name, f, a, b in zip(("dW1", "db1", "dW2", "db2"), full, lo, hi):
        assert torch.isfinite(f).all(), name
        assert float((f - (a + b)).abs().max()) <= 5e-5 * float(f.abs().max()), name


@pytest.mark.parametrize("d,nhid", [(3, 1), (8, 24), (16, 1), (48, 40), (100, 16), (5, 7)])
def test_projection_kernels_serve_any_factor_width_up_to_128(d, nhid):
    """Factor / Factor2 (model.py:13-15, 24-27) at widths the kernels are not instantiated for: the module must stay on
    the matrix-core kernels (zero-padded output weights, ops.project_tile_width) — forward against an fp64 MLP, the
    weight gradients against torch autograd of the same MLP — and never reach a library GEMM."""
    from disenlink_amd import ops
    from disenlink_amd.model import Disentangle
    torch.manual_seed(d * 13 + nhid)
    N, Fdim, K = 301, 37, 3
    model = Disentangle(Fdim, nhid, d, nfactor=K, beta=0.5, projection="mfma").to(DEV)
    x = torch.randn(N, Fdim, device=DEV)
    assert ops.project_supported(d) and ops.project_tile_width(d) in (32, 64, 128)
    Z = model.project(x)
    assert Z.shape == (N, K, d) and Z.is_contiguous()
    ref = []
    for f in model.factors:
        xd = x.double()
        if nhid == 1:
            ref.append(xd @ f.mlp.weight.double().t() + f.mlp.bias.double())
        else:
            ref.append(torch.relu(xd @ f.mlp1.weight.double().t() + f.mlp1.bias.double()) @ f.mlp2.weight.double().t()
                       + f.mlp2.bias.double())
    ref = torch.stack(ref, dim=1)
    assert float((Z.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    g = torch.randn_like(Z)
    model.zero_grad()
    (Z * g).sum().backward()
    got = {k: p.grad.clone() for k, p in model.named_parameters()}
    lib = Disentangle(Fdim, nhid, d, nfactor=K, beta=0.5, projection="library").to(DEV)
    lib.load_state_dict(model.state_dict())
    (lib.project(x) * g).sum().backward()
    for k, p in lib.named_parameters():
        assert float((got[k] - p.grad).abs().max()) <= 1e-4 * max(float(p.grad.abs().max()), 1e-6), k
    with pytest.raises(Exception):
        ops.project_fwd(x, torch.randn(K, 130, Fdim, device=DEV), torch.randn(K, 130, device=DEV))    # d > 128: not served


@pytest.mark.parametrize("F", [128, 269])
def test_persistent_x_planes_give_the_same_bits_and_follow_the_tensor(F, monkeypatch):
    """ops._XPlanes: the bf16 planes of x and x^T built once per feature TENSOR (second sight on) and handed to
    dl_project_fwd_xp / dl_project_bwd_xp — the same products, so Z and every gradient are the same bits as with the
    per-call split (DL_X_PLANES=0); an in-place change of x (version counter) or another tensor gets planes of its own."""
    from disenlink_amd import ops
    torch.manual_seed(5)
    N, K, nhid, d = 777, 4, 96, 64
    x = torch.randn(N, F, device=DEV)
    W1, b1 = torch.randn(K, nhid, F, device=DEV) * 0.1, torch.randn(K, nhid, device=DEV) * 0.1
    W2, b2 = torch.randn(K, d, nhid, device=DEV) * 0.1, torch.randn(K, d, device=DEV) * 0.1
    dZ = torch.randn(N, K, d, device=DEV)

    def run():
        Z, hid = ops.project_fwd(x, W1, b1, W2, b2, keep_hid=True)
        return (Z,) + tuple(ops.project_bwd(x, W1, b1, W2, dZ, hid=hid)) + tuple(ops.project_bwd(x, W1, b1, W2, dZ))
    monkeypatch.setenv("DL_X_PLANES", "0")
    want = run()
    monkeypatch.delenv("DL_X_PLANES")
    assert ops.xplanes_for(x) is None                                   # first sight: nothing built
    first = run()                                                       # (project_fwd saw it once more: the bwd calls build / use them)
    planes = ops.xplanes_for(x)
    assert planes is not None and planes.numel() == ops._lib.load().dl_project_xplanes_bytes(N, (F + 3) // 4 * 4)
    second = run()
    for a_, b_, c_ in zip(want, first, second):
        assert torch.equal(a_, b_) and torch.equal(a_, c_)
    assert ops.xplanes_for(x).data_ptr() == planes.data_ptr()          # reused, not rebuilt
    x.mul_(2.0)                                                         # in place: the version counter moves, the planes are stale
    monkeypatch.setenv("DL_X_PLANES", "0")
    want2 = run()
    monkeypatch.delenv("DL_X_PLANES")
    for _ in range(2):
        got2 = run()
    for a_, b_ in zip(want2, got2):
        assert torch.equal(a_, b_)
    assert not torch.equal(want2[0], want[0])


@pytest.mark.parametrize("F", [269, 128])
def test_projection_gradients_lie_back_to_back_at_every_feature_width(F):
    """ops.project_bwd carves its four stacked gradients out of ONE allocation so that the sharded training step all-reduces
    them as one flat tensor (dist.allreduce_gradients: 1 collective, 0 copies) — also when the feature axis is zero-padded
    for the kernels (F % 4 != 0: snap-patents' F = 269 gave four collectives in round 4), with unchanged values."""
    from disenlink_amd import ops
    from disenlink_amd.optim import flat_view
    torch.manual_seed(3)
    N, K, nhid, d = 500, 8, 64, 64
    x = torch.randn(N, F, device=DEV)
    W1, b1 = torch.randn(K, nhid, F, device=DEV) * 0.1, torch.randn(K, nhid, device=DEV) * 0.1
    W2 = torch.randn(K, d, nhid, device=DEV) * 0.1
    dZ = torch.randn(N, K, d, device=DEV)
    got = ops.project_bwd(x, W1, b1, W2, dZ)
    flat = flat_view(list(got))
    assert flat is not None and flat.numel() == sum(g.numel() for g in got)
    assert got[0].shape == W1.shape and got[0].is_contiguous()
    sep = ops.project_bwd(x, W1, b1, W2, dZ, one_allocation=False)
    for a_, b_ in zip(got, sep):
        assert torch.equal(a_, b_)
    # against autograd of the plain formula (fp64)
    xd, W1d, b1d, W2d = (t_.double().requires_grad_(t_ is not x) for t_ in (x, W1, b1, W2))
    hid = torch.relu(torch.einsum("nf,khf->nkh", xd, W1d) + b1d)
    Zd = torch.einsum("nkh,kdh->nkd", hid, W2d)
    Zd.backward(dZ.double())
    for g_, w_ in zip(got[:3], (W1d.grad, b1d.grad, W2d.grad)):
        assert float((g_.double() - w_).abs().max()) <= 2e-5 * float(w_.abs().max())


def test_projection_backward_rejects_bad_arguments():
    from disenlink_amd import _lib, ops
    x, dZ = torch.randn(10, 8, device=DEV), torch.randn(10, 2, 32, device=DEV)
    W1, b1 = torch.randn(2, 32, 8, device=DEV), torch.randn(2, 32, device=DEV)
    with pytest.raises(ValueError):
        ops.project_bwd(x, W1, b1, None, dZ[:, :1])
    lib = _lib.load()
    out = torch.empty_like(W1)
    rc = lib.dl_project_bwd(x.data_ptr(), 10, 8, 2, 1, 32, W1.data_ptr(), b1.data_ptr(), None, dZ.data_ptr(), None,
                            out.data_ptr(), b1.data_ptr(), None, None, None, 0, None)
    assert rc != 0 and b"workspace" in lib.dl_last_error()
    rc = lib.dl_project_bwd(x.data_ptr(), 10, 8, 2, 1, 48, W1.data_ptr(), b1.data_ptr(), None, dZ.data_ptr(), None,
                            out.data_ptr(), b1.data_ptr(), None, None, None, 0, None)
    assert rc != 0 and b"32, 64, 128" in lib.dl_last_error()


@pytest.mark.parametrize("name,K,d,nhid,epochs", [("cora", 4, 32, 64, 10), ("chameleon", 8, 64, 512, 40)])
def test_graph_replayed_epochs_follow_the_eager_trajectory(name, K, d, nhid, epochs):
    """use_graph=True replays the epoch (forward, fused loss, backward, Adam, AUC) from a captured HIP graph: the
    loss / AUC sequence must follow the eager loop's (Adam's moments and step counter live across replays, and
    everything the graph touches outlives it — the chameleon case has a validation set large enough for the radix /
    merge sort paths, the MFMA projection with its kept hidden layer, and 40 epochs of best-weight snapshots
    allocating between replays)."""
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    sg = synthetic_graph(name, seed=3)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=3)
    run = prepare_run(split, torch.device(DEV), row_bytes=K * d * 4)
    x = torch.from_numpy(sg.features()).to(DEV)
    out = {}
    for use_graph in (False, True):
        torch.manual_seed(0)
        model = Disentangle(sg.n_feat, nhid, d, nfactor=K, beta=0.6, t=1).to(DEV)
        out[use_graph] = run_link_prediction(model, x, run, epochs=epochs, lr=1e-3, use_graph=use_graph)
        if use_graph:
            # the loop declares its labels static, so the capture recorded the per-entry stream of the warm-up epochs: a
            # capture without the declaration unbinds (PairList.bind_labels) and would leave _yw None here
            assert run.train_val_pairs.static_labels and run.train_val_pairs._yw is not None
        junk =[torch.randn(1 << 18, device=DEV) for _ in range(8)]      # churn the allocator between the two runs
        del junk
    np.testing.assert_allclose(out[True].losses, out[False].losses, rtol=2e-3)
    np.testing.assert_allclose(out[True].val_aucs, out[False].val_aucs, atol=2e-3)
    assert abs(out[True].test_auc - out[False].test_auc) <= 2e-3


def test_cli_runs_the_reference_flag_set():
    """`python -m disenlink_amd.main` with the flag names of main_disentangled.py:21-50 (incl. a stray token,
    which parse_known_args ignores like the reference's chameleon recipe) on a synthetic stand-in."""
    from disenlink_amd import main as cli
    res = cli.main(["--dataset", "cora", "--synthetic", "--beta", "0.6", "temperature", "1", "--nfactor", "4",
                    "--nhidden", "64", "--nembed", "32", "--layer", "1", "--epochs", "6", "--lr", "0.001", "--m", "5",
                    "--run", "2", "--quiet"])
    assert res.shape == (2,) and np.isfinite(res).all() and (res > 0.4).all() and (res <= 1.0).all()
    with pytest.raises(SystemExit):
        cli.main(["--layer", "2", "--quiet"])


def test_full_size_benchmark_workload_matches_c_oracle():
    """The bench workload at its FULL size (squirrel-synthetic, K=8, d=64: 369k edges, 1.04M pairs) against
    the multi-threaded C restatement, plus size-independent properties: routing symmetry, normaliser =
    per-factor row sums, isolated nodes keep beta*z, scorer symmetric in (u, v), bitwise reproducibility."""
    import bench
    from disenlink_amd import ops
    from oracle import c_ref
    K, d, beta, t = 8, 64, 0.5, 1.0
    sg, split, graph, pairs, _model, _x, Z = bench.build_workload("squirrel", torch.device(DEV), K, d, 512)
    p, a, s = ops.route_fwd(graph, Z, t)
    H = ops.aggregate_fwd(graph, Z, beta, p, a, s)
    prob = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs)
    Zh = Z.cpu().numpy()
    rowptr, col = graph.rowptr.cpu().numpy(), graph.col.cpu().numpy()
    p_o, a_o, s_o = c_ref.route(Zh, rowptr, col, t)
    p_h, a_h, s_h = p.cpu().numpy(), a.cpu().numpy(), s.cpu().numpy()
    same = p_h == p_o
    assert same.mean() > 0.9999                                        # near-ties may flip in fp32
    np.testing.assert_allclose(a_h[same], a_o[same], rtol=1e-5)
    H_o = c_ref.aggregate(Zh, rowptr, col, p_h, a_h, s_h, beta)        # from the GPU's own routing
    np.testing.assert_allclose(H.cpu().numpy(), H_o, rtol=1e-5, atol=1e-5)
    prob_o = c_ref.score_pairs(Zh, H_o, pairs.pu.cpu().numpy(), pairs.pv.cpu().numpy(), t)
    np.testing.assert_allclose(prob.cpu().numpy(), prob_o, rtol=1e-5, atol=1e-5)
    auc_lab = (np.arange(prob_o.size) % 3 == 0).astype(np.float32)      # any fixed labelling: same ranks -> same AUC
    assert abs(metrics_ref.auc_tie_avg(auc_lab, prob.cpu().numpy()) - metrics_ref.auc_tie_avg(auc_lab, prob_o)) <= 1e-4
    # properties
    rev = graph.rev.long()
    assert torch.equal(p, p[rev]) and torch.equal(a, a[rev])            # (i,j) and (j,i) route identically, bitwise
    src = torch.repeat_interleave(torch.arange(graph.n_nodes, device=DEV), (graph.rowptr[1:] - graph.rowptr[:-1]).long())
    s_chk = torch.zeros_like(s).index_put_((src, p.long()), a, accumulate=True)
    np.testing.assert_allclose(s_h, s_chk.cpu().numpy(), rtol=1e-5, atol=1e-6)
    iso = (graph.rowptr[1:] == graph.rowptr[:-1])
    if bool(iso.any()):
        assert torch.equal(H[iso], beta * Z[iso])
    swapped = ops.score_pairs_fwd(Z, H, pairs.pv, pairs.pu, t, None)
    np.testing.assert_allclose(swapped.cpu().numpy(), prob.cpu().numpy(), rtol=1e-6, atol=1e-7)
    p2, a2, s2 = ops.route_fwd(graph, Z, t)
    assert torch.equal(p, p2) and torch.equal(a, a2) and torch.equal(s, s2)
    assert torch.equal(H, ops.aggregate_fwd(graph, Z, beta, p, a, s))
    assert torch.equal(prob, ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs))


def test_fused_pair_bce_matches_torch_bce():
    """dl_pair_bce (loss + gradient in one kernel) vs F.binary_cross_entropy on pos / neg lists incl. saturated
    probabilities (exact 0 and 1: log clamp at -100, gradient clamp 1e-12) and labels that disagree."""
    import torch.nn.functional as F
    from disenlink_amd.metrics import pair_bce_loss, pair_bce_loss_fused, pair_bce_weights
    g = torch.Generator().manual_seed(0)
    n_pos, n_neg, m = 3001, 7003, 5
    prob = torch.rand(n_pos + n_neg, generator=g)
    prob[:50] = 1.0
    prob[50:80] = 0.0
    prob[-40:] = 1.0
    label = torch.cat([torch.ones(n_pos), torch.zeros(n_neg)])
    label[n_pos: n_pos + 7] = 1.0                                        # a sampled "negative" that is an edge
    pr = prob.to(DEV).requires_grad_(True)
    lt = label.to(DEV)
    ref = pair_bce_loss(pr[:n_pos], lt[:n_pos], pr[n_pos:], lt[n_pos:], m)
    (g_ref,) = torch.autograd.grad(ref, pr)
    pf = prob.to(DEV).requires_grad_(True)
    fused = pair_bce_loss_fused(pf, lt, pair_bce_weights(n_pos, n_neg, m, DEV))
    (g_f,) = torch.autograd.grad(fused * 2.0, pf)                       # upstream gradient is applied
    assert abs(float(fused) - float(ref)) <= 1e-5 * abs(float(ref))
    torch.testing.assert_close(g_f, 2.0 * g_ref, rtol=1e-5, atol=0)
    assert torch.equal(fused, pair_bce_loss_fused(pf, lt, pair_bce_weights(n_pos, n_neg, m, DEV)))     # deterministic
    # a NaN probability must surface (torch's BCE refuses it: "all elements of input should be between 0 and 1") — here
    # as a NaN loss, never swallowed into a finite one; a NaN at weight 0 (a pair outside the loss) is ignored
    w = pair_bce_weights(n_pos, n_neg, m, DEV)
    bad = prob.clone()
    bad[5] = float("nan")
    assert torch.isnan(pair_bce_loss_fused(bad.to(DEV), lt, w))
    with pytest.raises(RuntimeError):
        pair_bce_loss(bad[:n_pos], label[:n_pos], bad[n_pos:], label[n_pos:], m)                       # torch, on the CPU
    w0 = w.clone()
    w0[5] = 0.0
    assert torch.isfinite(pair_bce_loss_fused(bad.to(DEV), lt, w0))


@pytest.mark.gpu
def test_auc_counting_kernel_equals_the_sort_form_and_sklearn_vectors():
    """dl_auc_pair_counts (slices of 1,024 scores of the smaller class sorted by a workgroup each, the other class located
    in them by binary searches, integer counts that add up over the slices) behind AucPlan.auc on the GPU: the sklearn
    golden vectors, and the CPU sort form on random scores with heavy ties — either class the smaller one, slice counts
    of 1 .. 69 with ragged last slices — the same integer count."""
    import glob
    import os
    from conftest import GOLDEN_DIR
    from disenlink_amd.metrics import AucPlan
    for path in sorted(glob.glob(os.path.join(GOLDEN_DIR, "auc_*.npz"))):
        g = np.load(path)
        y, sc = torch.from_numpy(g["y"]), torch.from_numpy(g["score"]).float()
        assert abs(float(AucPlan(y.to(DEV)).auc(sc.to(DEV))) - float(g["auc"])) <= 1e-12, path
    rng = np.random.default_rng(11)
    for n, frac, levels in ((2, 0.5, 2), (65, 0.5, 3), (1023, 0.1, 50), (4097, 0.9, 7), (9000, 0.5, 100000), (70000, 0.17, 1000),
                            (140000, 0.03, 1 << 20), (66000, 0.496, 1 << 16), (140000, 0.5, 1 << 12)):
        yb = rng.random(n) < frac
        yb[0], yb[1] = True, False                                                  # both classes present
        y = torch.from_numpy(yb.astype(np.float32))
        sc = torch.from_numpy((rng.integers(0, levels, n) / levels).astype(np.float32))
        sc[rng.random(n) < 0.1] = 1.0
        want = AucPlan(y).auc(sc)                                                   # CPU: sort + binary searches
        plan = AucPlan(y.to(DEV))
        got = plan.auc(sc.to(DEV))
        assert got.is_cuda and float(got) == float(want), (n, frac, levels, float(got), float(want))   # the same integer count
        assert float(plan.auc(sc.to(DEV) * 0 + 0.25)) == 0.5                        # all tied
        big = torch.cat([sc, sc]).to(DEV)[n:]                                       # an offset view, like prob[b:]
        assert float(plan.auc(big)) == float(want)


@pytest.mark.gpu
def test_three_plane_bf16_products_are_fp32_grade(lib_env):
    """Layer 1 and the dW1 contraction run as six exact bf16 products per term from three bf16 planes per operand
    (dl_tiles.h).  Full-mantissa random operands, odd sizes (feature / node / hidden tails of the padded plane arrays):
    the error against fp64 stays within 2x that of the plain fp32 MFMA form (DL_PROJECT_FP32_MFMA=1) and within fp32
    summation noise — and a wide dynamic range inside one row (1e-6 .. 1e+3) loses nothing."""
    from disenlink_amd import ops
    g = torch.Generator().manual_seed(5)
    for (N, F, K, nhid, d) in [(1000, 333, 3, 200, 64), (517, 1436, 2, 96, 32), (300, 100, 2, 130, 128)]:
        x = torch.randn(N, F, generator=g) * torch.logspace(-6, 3, F)[torch.randperm(F, generator=g)]
        W1 = torch.randn(K, nhid, F, generator=g) / F ** 0.5
        b1 = torch.randn(K, nhid, generator=g) * 0.1
        W2 = torch.randn(K, d, nhid, generator=g) / nhid ** 0.5
        b2 = torch.randn(K, d, generator=g) * 0.1
        dZ = torch.randn(N, K, d, generator=g)
        X = x.double()
        pre = torch.einsum("nf,khf->nkh", X, W1.double()) + b1.double()
        hid = pre.clamp_min(0)
        Zref = torch.einsum("nkh,kdh->nkd", hid, W2.double()) + b2.double()
        dev = [v.to(DEV) for v in (x, W1, b1, W2, dZ)]
        errs = {}
        for form in ("planes", "fp32"):
            if form == "fp32":
                lib_env("DL_PROJECT_FP32_MFMA", 1)
            else:
                lib_env("DL_PROJECT_FP32_MFMA")
            Z, kept = ops.project_fwd(dev[0], dev[1], dev[2], dev[3], b2.to(DEV), keep_hid=True)
            dW1 = ops.project_bwd(*dev, hid=kept)[0]
            # reference gradient with the ReLU mask this run actually used (near-zero pre-activations may flip in fp32)
            ldh = (N + 3) // 4 * 4
            mask = (kept.view(K, nhid, ldh)[:, :, :N] > 0).permute(2, 0, 1).cpu()
            dh = torch.einsum("nkd,kdh->nkh", dZ.double(), W2.double()) * mask
            dW1ref = torch.einsum("nkh,nf->khf", dh, X)
            errs[form] = (float((Z.cpu().double() - Zref).abs().max() / Zref.abs().max()),
                          float((dW1.cpu().double() - dW1ref).abs().max() / dW1ref.abs().max()))
        lib_env("DL_PROJECT_FP32_MFMA")
        for i, what in enumerate(("Z", "dW1")):
            assert errs["planes"][i] <= max(2.0 * errs["fp32"][i], 2e-7), (what, errs, (N, F, K, nhid, d))
            assert errs["planes"][i] <= 5e-6, (what, errs)





@pytest.mark.gpu
@pytest.mark.parametrize("K,d,dtype", [(8, 64, torch.float32), (4, 64, torch.float32), (4, 32, torch.float32), (16, 128, torch.float32),
                                       (8, 64, torch.bfloat16)])
def test_one_pass_training_scorer_matches_the_separate_kernels(K, d, dtype):
    """dl_score_pairs_train (scorer forward + weighted-BCE gradient + scorer backward in one pass over the incidence
    plan) against dl_score_pairs_fwd -> dl_pair_bce -> dl_score_pairs_bwd: prob, loss, dZ, dH and the full autograd
    step through ops.HotPathPairsLoss vs ops.HotPathPairs + PairBCE — incl. saturated pairs, weight-0 pairs (validation
    pairs riding along) and a gradient arriving on prob as well."""
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph, PairList
    from disenlink_amd.metrics import pair_bce_weights
    rng = np.random.default_rng(K * 7 + d)
    N, E, P = 700, 5000, 9000
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    pu, pv = rng.integers(0, N, P), rng.integers(0, N, P)
    G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
    pairs = PairList.build(torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV), N, row_bytes=K * d * 4)
    amp = 0.35 * (32 / d) ** 0.5
    Z = (torch.randn(N, K, d, generator=torch.Generator().manual_seed(1)) * amp).to(DEV)
    Z[3] *= 6.0                                                     # a few saturated scores (prob = 1 exactly)
    label = torch.from_numpy((rng.random(P) < 0.3).astype(np.float32)).to(DEV)
    weight = pair_bce_weights(int(P * 0.2), P - int(P * 0.2), 5, DEV)
    weight[-500:] = 0.0                                             # pairs outside the loss
    beta, t = 0.6, 1.0
    # raw entry points on the same tables
    Zt = Z if dtype == torch.float32 else Z.to(dtype)
    H = ops.aggregate_fwd(G, Zt, beta, *ops.route_fwd(G, Zt, t))
    prob1, dZ1, dH1 = ops.score_pairs_train(Zt, H, pairs, t, label, weight)
    prob0 = ops.score_pairs_fwd(Zt, H, pairs.pu, pairs.pv, t, pairs)
    np.testing.assert_allclose(prob1.cpu().numpy(), prob0.cpu().numpy(), rtol=2e-6, atol=1e-7)
    pr = prob1.detach().clone().requires_grad_(True)
    loss_ref = ops.PairBCE.apply(pr, label, weight)
    (g_prob,) = torch.autograd.grad(loss_ref, pr)
    dZ0, dH0 = ops.score_pairs_bwd(Zt, H, pairs, t, prob1, g_prob)          # recompute form on the SAME prob
    for name, got, want in (("dZ", dZ1, dZ0), ("dH", dH1, dH0)):
        assert torch.isfinite(got).all(), name
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-12, name
    assert torch.equal(prob1, ops.score_pairs_train(Zt, H, pairs, t, label, weight)[0])       # reproducible
    # the autograd nodes, with another function of the scores on top of the loss
    outs = {}
    for fused in (True, False):
        Zp = Z.clone().requires_grad_(True)
        if fused:
            emb, prob, loss = ops.HotPathPairsLoss.apply(Zp, G, pairs, beta, t, dtype, label, weight)
        else:
            emb, prob = ops.HotPathPairs.apply(Zp, G, pairs, beta, t, dtype)
            loss = ops.PairBCE.apply(prob, label, weight)
        total = 2.0 * loss + 1e-3 * (prob * prob).sum() + 1e-4 * emb.sum()
        (gZ,) = torch.autograd.grad(total, Zp)
        outs[fused] = (loss.detach(), prob.detach(), gZ)
    assert abs(float(outs[True][0]) - float(outs[False][0])) <= 1e-6 * abs(float(outs[False][0]))
    # the module picks the one-pass form by table size (forced here) and gives the same loss either way
    if dtype == torch.float32 and (K, d) == (8, 64):
        import os
        from disenlink_amd.model import Disentangle
        torch.manual_seed(0)
        m = Disentangle(16, 32, d, nfactor=K, beta=beta, t=t).to(DEV)
        xx = torch.randn(N, 16, device=DEV)
        got = {}
        for mode in ("1", "0"):
            os.environ["DL_ONE_PASS_SCORER"] = mode
            try:
                _e, pr_m, ls_m = m.forward_pairs_loss(xx, G, pairs, label, weight)
                ls_m.backward()
                got[mode] = (float(ls_m), m.factor_0.mlp1.weight.grad.clone())
                m.zero_grad()
            finally:
                os.environ.pop("DL_ONE_PASS_SCORER", None)
        assert abs(got["1"][0] - got["0"][0]) <= 1e-6 * abs(got["0"][0])
        assert float((got["1"][1] - got["0"][1]).abs().max()) <= 2e-5 * float(got["0"][1].abs().max())
    np.testing.assert_allclose(outs[True][1].cpu().numpy(), outs[False][1].cpu().numpy(), rtol=2e-6, atol=1e-7)
    scale = float(outs[False][2].abs().max())
    assert float((outs[True][2] - outs[False][2]).abs().max()) <= (2e-5 if dtype == torch.float32 else 2e-3) * scale


def _one_pass_case(K, d, dtype, seed, overflow=False):
    """A seeded scoring problem for the one-pass training scorer: tables, pair list, labels, loss weights — with a few
    saturated scores (prob == 1 exactly), weight-0 pairs (validation pairs riding along), and optionally one node whose
    exponent overflows (z.z / t > 88.7)."""
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph, PairList
    from disenlink_amd.metrics import pair_bce_weights
    rng = np.random.default_rng(seed)
    N, E, P = 600, 4000, 8000
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    pu, pv = rng.integers(0, N, P), rng.integers(0, N, P)
    pu[:40], pv[:40] = 3, rng.integers(0, N, 40)                     # the saturated node's row gets several segments' worth
    G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N).to(DEV)
    pairs = PairList.build(torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV), N, row_bytes=K * d * (4 if dtype == torch.float32 else 2))
    amp = 0.35 * (32 / d) ** 0.5
    Z = torch.randn(N, K, d, generator=torch.Generator().manual_seed(seed)) * amp
    Z[3] *= 6.0                                                      # saturated scores
    if overflow:
        Z[5] = 2.0 * (128 / d) ** 0.5                                # z5.z5 = 512 per factor: exp(512 / 2) = inf, also at t = 2
        pu[100:104], pv[100:104] = 5, 5
        pairs = PairList.build(torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV), N, row_bytes=K * d * (4 if dtype == torch.float32 else 2))
    Z = Z.to(DEV)
    label = torch.from_numpy((rng.random(P) < 0.3).astype(np.float32)).to(DEV)
    weight = pair_bce_weights(int(P * 0.2), P - int(P * 0.2), 5, DEV)
    weight[-500:] = 0.0
    return G, pairs, Z, label, weight, pu, pv


@pytest.mark.gpu
@pytest.mark.parametrize("K,d,dtype", [(8, 64, torch.float32), (4, 64, torch.float32),         # wave-per-entry kernel, T1 = false
                                       (4, 32, torch.float32), (16, 128, torch.float32),       # the other fp32 shapes
                                       (8, 64, torch.bfloat16), (16, 128, torch.bfloat16)])    # bf16 tables
@pytest.mark.parametrize("t", [2.0, 1.0])
def test_one_pass_training_scorer_matches_the_oracle_directly(K, d, dtype, t):
    """dl_score_pairs_train against oracle/sparse_ref.score_pairs_bwd (NOT against the separate kernels): prob, dZ, dH at
    temperature 2 (the `/ t` of model.py:56,113; main_disentangled.py:40) and 1, incl. saturated pairs (zero gradient),
    weight-0 pairs (nothing at all) and — fp32 (8, 64) — a node whose exponent overflows.  bf16 tables: the oracle is
    evaluated on the same bf16-rounded tables (the reference has no bf16 path)."""
    from disenlink_amd import ops
    overflow = (K, d, dtype) == (8, 64, torch.float32)
    G, pairs, Z, label, weight, pu, pv = _one_pass_case(K, d, dtype, seed=K * 11 + d + int(t), overflow=overflow)
    beta = 0.6
    Zt = Z if dtype == torch.float32 else Z.to(dtype)
    H = ops.aggregate_fwd(G, Zt, beta, *ops.route_fwd(G, Zt, t))
    prob, dZ, dH = ops.score_pairs_train(Zt, H, pairs, t, label, weight)
    Zh, Hh = Zt.float().cpu().numpy(), H.float().cpu().numpy()
    lab, wgt = label.cpu().numpy(), weight.cpu().numpy()
    prob_o, q_o, ex_o = sparse_ref.score_pairs(Zh, Hh, pu, pv, t, return_parts=True)
    pr = prob.cpu().numpy()
    assert np.array_equal(np.isnan(pr), np.isnan(prob_o))
    fin = ~np.isnan(prob_o)
    np.testing.assert_allclose(pr[fin], prob_o[fin], rtol=2e-5, atol=2e-6)
    assert int((prob_o == 1.0).sum()) >= 20                          # the saturated pairs are really there
    # the weighted-BCE gradient of main_disentangled.py:195 in probability space (F.binary_cross_entropy's clamp)
    with np.errstate(invalid="ignore", over="ignore"):
        g_prob = (wgt * (prob_o - lab) / np.maximum(prob_o * (1 - prob_o), np.float32(1e-12))).astype(np.float32)
    g_prob[wgt == 0] = 0.0
    # An overflowed exponent (e_k = inf) saturates the score, so its logit gradient is exactly 0; the reference's autograd
    # then forms 0 * inf = NaN for EVERY parameter (MulBackward of model.py:113 — also for unmasked entries: a run that
    # overflows is dead there).  The one-pass kernel keeps 0 * inf = 0 (documented in DESIGN.md): such pairs contribute
    # nothing, which is what the oracle gives with those pairs left out.
    keep = np.isfinite(ex_o).all(axis=1) & np.isfinite(q_o).all(axis=1)
    assert overflow == bool((~keep).any())
    dZ_o, dH_o = sparse_ref.score_pairs_bwd(Zh, Hh, pu[keep], pv[keep], t, g_prob[keep])
    for name, got, want in (("dZ", dZ, dZ_o), ("dH", dH, dH_o)):
        got = got.cpu().numpy()
        assert np.isfinite(got).all(), name
        assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max() + 1e-12, (name, np.abs(got - want).max(), np.abs(want).max())
    assert float(np.abs(dH_o).max()) > 0 and float(np.abs(dZ_o).max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("K,d,dtype", [(8, 64, torch.float32), (16, 128, torch.bfloat16), (16, 128, torch.float32), (4, 32, torch.float32)])
def test_one_pass_training_scorer_is_independent_of_the_row_sharding(K, d, dtype):
    """dl_score_pairs_train over the incidence rows of a row SHARD (what a rank of the sharded training step runs) gives
    that shard's rows of dZ / dH and the scores of the pairs touching it bit for bit as the unsharded call: every kernel
    family sums a node's entries in an order that depends on the row alone (ascending entries per lane; units summed in
    segment order, or — the wide kernel — as the tree (s0 + s1) + (s2 + s3) of the row's own segments)."""
    from disenlink_amd import ops
    from disenlink_amd.graph import PairList
    G, pairs, Z, label, weight, pu, pv = _one_pass_case(K, d, dtype, seed=31 + K)
    N = Z.shape[0]
    Zt = Z if dtype == torch.float32 else Z.to(dtype)
    H = ops.aggregate_fwd(G, Zt, 0.6, *ops.route_fwd(G, Zt, 1.0))
    prob, dZ, dH = ops.score_pairs_train(Zt, H, pairs, 1.0, label, weight)
    tpu, tpv = torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV)
    wb = 4 if dtype == torch.float32 else 2
    for lo, hi in ((0, 3), (3, 4), (4, 301), (301, N)):                # node 3 (several segments' worth of pairs) alone in a shard
        inc = PairList.build(tpu, tpv, N, row_range=(lo, hi), build_by_u=False, row_bytes=K * d * wb)
        prob_s, dZ_s, dH_s = ops.score_pairs_train(Zt, H, inc, 1.0, label, weight)
        assert torch.equal(dZ_s[lo:hi], dZ[lo:hi]) and torch.equal(dH_s[lo:hi], dH[lo:hi]), (lo, hi)
        touch = torch.from_numpy(((pu >= lo) & (pu < hi)) | ((pv >= lo) & (pv < hi))).to(DEV)
        assert torch.equal(prob_s[touch], prob[touch]), (lo, hi)
    # ... also with XCD-sliced incidence plans (round 6: the slice boundaries come from the WHOLE list, so a shard cuts its
    # rows into the same (row, slice) units as the unsharded plan and adds them in the same slot order)
    whole = PairList.build(tpu, tpv, N, build_by_u=False, row_bytes=K * d * wb, inc_slices=8)
    assert whole.inc.n_slices == 8 and whole.inc.n_slots > N
    prob8, dZ8, dH8 = ops.score_pairs_train(Zt, H, whole, 1.0, label, weight)
    assert torch.equal(prob8, prob)
    for lo, hi in ((0, 4), (4, 301), (301, N)):
        inc = PairList.build(tpu, tpv, N, row_range=(lo, hi), build_by_u=False, row_bytes=K * d * wb, inc_slices=8)
        _p, dZ_s, dH_s = ops.score_pairs_train(Zt, H, inc, 1.0, label, weight)
        assert torch.equal(dZ_s[lo:hi], dZ8[lo:hi]) and torch.equal(dH_s[lo:hi], dH8[lo:hi]), ("sliced", lo, hi)


@pytest.mark.gpu
def test_compiled_projection_adam_auc_and_bf16_hot_path_equal_the_python_operators_bit_for_bit(monkeypatch):
    """Round 5: the rest of the training step behind the compiled binding (csrc/torch/dl_torch.cpp) — the projection over
    the module's shared buffers (forward, the four stacked gradients), the Adam step, the AUC counts, and the hot path with
    bf16 tables — against the Python operators over ctypes: the same kernels, so the same bits; and a whole eager training
    run with DL_NATIVE_OPS=1 against DL_NATIVE_OPS=0."""
    from disenlink_amd import native, ops
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.metrics import AucPlan
    from disenlink_amd.model import Disentangle
    from disenlink_amd.optim import StackedAdam, flat_view
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    native._state["loaded"] = None
    assert native.available()
    # ---- projection node: Z, and every parameter's gradient as a slice of one flat allocation
    torch.manual_seed(0)
    N, F, K, nhid, d = 700, 64, 8, 96, 64
    x = torch.randn(N, F, device=DEV)
    gZ = torch.randn(N, K, d, device=DEV)
    out = {}
    for which in ("python", "native"):
        torch.manual_seed(1)
        m = Disentangle(F, nhid, d, nfactor=K, beta=0.5, t=1).to(DEV)
        flat = m._stacked_params()
        st = m._stacked
        bufs = (st[("mlp1", "weight")], st[("mlp1", "bias")], st[("mlp2", "weight")], st[("mlp2", "bias")])
        assert native.project_ok(x, d, False)
        Z = ops.Project.apply(x, bufs, K, *flat) if which == "python" else native.project_stacked(x, bufs, flat)
        Z.backward(gZ)
        grads = [p.grad for p in flat]
        assert flat_view([g for g in grads]) is not None             # back to back: one all-reduce, no stacking copy in Adam
        out[which] = (Z.detach().clone(), [g.clone() for g in grads], m)
    assert torch.equal(out["python"][0], out["native"][0])
    for a_, b_ in zip(out["python"][1], out["native"][1]):
        assert torch.equal(a_, b_)
    # ---- Adam step on those gradients: native bookkeeping + launch vs the ctypes path
    after = {}
    for which in ("python", "native"):
        m = out[which][2]
        opt = StackedAdam(m, lr=1e-2, weight_decay=5e-4)
        opt._native_ok = which == "native"
        opt._flat_params = [p for k in opt.keys for p in opt.groups[k]]
        for _ in range(3):
            opt.step()
        after[which] = {k: v.clone() for k, v in m.state_dict().items()}
    for k in after["python"]:
        assert torch.equal(after["python"][k], after["native"][k]), k
    # ---- AUC counts
    lab = (torch.rand(5000, device=DEV) < 0.3).float()
    sc = torch.rand(5000, device=DEV)
    sc[::7] = 1.0                                                      # ties
    plan = AucPlan(lab)
    a_native = plan.auc(sc)
    monkeypatch.setenv("DL_NATIVE_OPS", "0")
    native._state["loaded"] = None
    try:
        assert not native.available()
        a_py = plan.auc(sc)
        assert float(a_native) == float(a_py) == pytest.approx(metrics_ref.auc_tie_avg(lab.cpu().numpy(), sc.cpu().numpy()), abs=1e-12)
    finally:
        monkeypatch.delenv("DL_NATIVE_OPS")
        native._state["loaded"] = None
    assert native.available()
    # ---- the hot path with bf16 tables through both bindings
    G, pairs, Z0, label, weight, _pu, _pv = _one_pass_case(8, 64, torch.bfloat16, seed=5)
    res = {}
    for which in ("python", "native"):
        Zr = Z0.clone().requires_grad_(True)
        if which == "python":
            H, prob, loss = ops.HotPathPairsLoss.apply(Zr, G, pairs, 0.6, 1.0, torch.bfloat16, label, weight)
        else:
            H, prob, loss = native.hot_path_pairs_loss(Zr, G, pairs, 0.6, 1.0, label, weight, torch.bfloat16)
        (loss * 2.0 + (H * H).sum() * 1e-3).backward()
        res[which] = (H.detach().clone(), prob.detach().clone(), loss.detach().clone(), Zr.grad.clone())
    for a_, b_, what in zip(res["python"], res["native"], ("H", "prob", "loss", "dZ")):
        assert torch.equal(a_, b_), what
    # ---- a whole eager training run either way: the same trajectory bit for bit
    sg = synthetic_graph("cora", seed=2)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=2)
    run = prepare_run(split, torch.device(DEV), row_bytes=8 * 64 * 4)
    xx = torch.from_numpy(sg.features()[:, :1432].copy()).to(DEV)     # F % 4 == 0: the compiled projection node serves it
    traj = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DL_NATIVE_OPS", mode)
        native._state["loaded"] = None
        torch.manual_seed(0)
        model = Disentangle(xx.shape[1], 64, 64, nfactor=8, beta=0.6, t=1).to(DEV)
        traj[mode] = run_link_prediction(model, xx, run, epochs=6, lr=1e-3, use_graph=False)
    monkeypatch.delenv("DL_NATIVE_OPS")
    native._state["loaded"] = None
    assert traj["1"].losses == traj["0"].losses and traj["1"].val_aucs == traj["0"].val_aucs
    assert traj["1"].test_auc == traj["0"].test_auc


@pytest.mark.gpu
def test_compiled_binding_and_python_operator_agree_at_temperature_2_and_with_a_loss_on_prob():
    """native.hot_path_pairs_loss (C++ autograd node) against ops.HotPathPairsLoss at t = 2 — the wave kernel's T1 = false
    instantiation through both bindings — bit for bit, for loss.backward() and with another loss term on `prob` and on
    the embedding (the advisor's round-4 finding: the compiled node used to drop a gradient arriving on prob); the graph
    and pair list may be dropped by the caller between forward and backward."""
    import gc
    from disenlink_amd import native, ops
    assert native.available()
    for (K, d) in ((8, 64), (4, 64)):
        out = {}
        for name in ("python", "native"):
            for extra in (False, True):
                G, pairs, Z0, label, weight, _pu, _pv = _one_pass_case(K, d, torch.float32, seed=77)
                Z = Z0.clone().requires_grad_(True)
                if name == "python":
                    H, prob, loss = ops.HotPathPairsLoss.apply(Z, G, pairs, 0.6, 2.0, torch.float32, label, weight)
                else:
                    H, prob, loss = native.hot_path_pairs_loss(Z, G, pairs, 0.6, 2.0, label, weight)
                del G, pairs                                           # the node must keep what its backward dereferences
                gc.collect()
                total = loss * 3.0 + ((prob * prob).sum() * 1e-2 + (H * H).sum() * 1e-3 if extra else 0.0)
                total.backward()
                out[(name, extra)] = (H.detach().clone(), prob.detach().clone(), loss.detach().clone(), Z.grad.clone())
        for extra in (False, True):
            for a_, b_, what in zip(out[("python", extra)], out[("native", extra)], ("H", "prob", "loss", "dZ")):
                assert torch.equal(a_, b_), (K, d, what, extra, float((a_ - b_).abs().max()))
        assert not torch.equal(out[("native", False)][3] , out[("native", True)][3])          # the prob / emb terms did arrive


@pytest.mark.gpu
@pytest.mark.parametrize("space", ["prob", "logit"])
def test_compiled_binding_and_python_operator_agree_on_soft_labels_and_signed_weights(space, monkeypatch):
    """Disentangle.forward_pairs_loss / forward_pair_logits_loss on soft labels (exact 0 and 1 among them) and signed weights
    (negative ones, +0.0 and -0.0: tests/label_weight_ref.py) through the compiled node and through the Python operators, three
    steps on the same tensors each (the sights at which a stream would bind): the scores and every parameter gradient bit for
    bit, every score written."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import label_weight_ref as lw
    import ref64
    from disenlink_amd import native
    from disenlink_amd.graph import PairList
    from disenlink_amd.model import Disentangle
    st = ref64.structure()
    G = st.graph.to(DEV)
    P = st.pu.numel()
    y, w = lw.labels_weights(("soft", "signed"), P, 4242)
    label, weight = y.to(DEV), w.to(DEV)
    x = torch.randn(ref64.N_NODES, 24, generator=torch.Generator().manual_seed(3)).to(DEV) * 0.5
    monkeypatch.setenv("DL_ONE_PASS_SCORER", "1")
    res = {}
    try:
        for mode in ("1", "0"):
            monkeypatch.setenv("DL_NATIVE_OPS", mode)
            native._state["loaded"] = None                            # re-read DL_NATIVE_OPS
            assert native.available() == (mode == "1")
            torch.manual_seed(0)
            model = Disentangle(24, 32, 64, nfactor=8, beta=0.6, t=2).to(DEV)
            pairs = PairList.build(st.pu.to(DEV), st.pv.to(DEV), ref64.N_NODES)
            steps = []
            for _sight in range(3):
                model.zero_grad(set_to_none=True)
                fwd = model.forward_pairs_loss if space == "prob" else model.forward_pair_logits_loss
                _emb, score, loss = fwd(x, G, pairs, label, weight)
                loss.backward()
                steps.append([score.detach().clone(), loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
            assert pairs._yw is None                                  # signed weights are never bound
            res[mode] = steps
    finally:
        monkeypatch.delenv("DL_NATIVE_OPS")
        native._state["loaded"] = None
    for a, b in zip(res["1"], res["0"]):
        assert bool(torch.isfinite(a[0]).all()) and len(a) == len(b) > 4
        for i, (u_, v_) in enumerate(zip(a, b)):
            assert torch.equal(u_, v_), (space, i, float((u_ - v_).abs().max()))
    for a in res["1"][1:]:
        assert all(torch.equal(u_, v_) for u_, v_ in zip(a, res["1"][0]))          # ... and the three sights agree


@pytest.mark.gpu
@pytest.mark.parametrize("native_ops", ["1", "0"])
@pytest.mark.parametrize("fixture,shape", [("traj_k8_d64_t2", (8, 64, 2)), ("traj_k16_d128", (16, 128, 1))])
def test_pair_list_training_with_the_one_pass_scorer_follows_the_reference_trajectory_at_t2(fixture, shape, native_ops,
                                                                                            monkeypatch):
    """tests/golden/traj_k8_d64_t2.npz — the REFERENCE model trained 8 epochs at K = 8, d = 64, temperature 2 under the
    reference's schedule — followed by the pair-list training loop (forward_pairs_loss: route, aggregate, the one-pass
    training scorer's wave kernel with T1 = false, Adam, AUC), through the compiled binding and through the Python
    operators: per-epoch loss and validation AUC, test AUC with the best weights.  traj_k16_d128.npz: the same at the
    factor shape of BASELINE configs[4] (K = 16, d = 128: score_train_wide_kernel and the d = 128 projection kernels)."""
    import sys, os
    from conftest import load_trajectory
    from disenlink_amd import native
    from disenlink_amd.model import Disentangle
    from disenlink_amd.train import prepare_run, run_link_prediction
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_dist_cpu import _split_from_trajectory
    monkeypatch.setenv("DL_NATIVE_OPS", native_ops)
    monkeypatch.setenv("DL_ONE_PASS_SCORER", "1")
    native._state["loaded"] = None                                    # re-read DL_NATIVE_OPS
    try:
        g = load_trajectory(fixture)
        m = g["meta"]
        assert (m["K"], m["d"], m["t"]) == shape
        model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"])
        model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")})
        model = model.to(DEV)
        run = prepare_run(_split_from_trajectory(g), torch.device(DEV), row_bytes=m["K"] * m["d"] * 4)
        res = run_link_prediction(model, torch.from_numpy(g["x"]).to(DEV), run, epochs=m["epochs"], lr=m["lr"], patience=200,
                                  use_graph=False)
        for ep in range(m["epochs"]):
            assert abs(res.losses[ep] - g["losses"][ep]) <= 2e-4 * abs(g["losses"][ep]), (ep, res.losses[ep], g["losses"][ep])
            assert abs(res.val_aucs[ep] - g["val_aucs"][ep]) <= 2e-3, (ep, res.val_aucs[ep], g["val_aucs"][ep])
        assert abs(res.test_auc - float(g["test_auc"])) <= 5e-3
    finally:
        native._state["loaded"] = None


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_training_with_the_one_pass_scorer_follows_the_separate_kernels(use_graph, monkeypatch):
    """The training loop with DL_ONE_PASS_SCORER=1 (scorer forward + loss gradient + backward in one pass, the form large
    graphs take by default) against DL_ONE_PASS_SCORER=0 on the same seeded run, eager and replayed from a HIP graph:
    the same loss / validation-AUC trajectory and test AUC."""
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    sg = synthetic_graph("chameleon", seed=5)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=5)
    run = prepare_run(split, torch.device(DEV), row_bytes=8 * 64 * 4)
    x = torch.from_numpy(sg.features()).to(DEV)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DL_ONE_PASS_SCORER", mode)
        torch.manual_seed(0)
        model = Disentangle(sg.n_feat, 64, 64, nfactor=8, beta=0.6, t=1).to(DEV)
        out[mode] = run_link_prediction(model, x, run, epochs=25, lr=1e-3, use_graph=use_graph)
    # two summation orders of the same gradients (agreeing to 1e-6 per step, test above), 25 Adam steps through a hard
    # arg-max: the trajectories stay together to ~1e-3, not to rounding
    np.testing.assert_allclose(out["1"].losses[:5], out["0"].losses[:5], rtol=5e-5)
    np.testing.assert_allclose(out["1"].losses, out["0"].losses, rtol=2e-3)
    np.testing.assert_allclose(out["1"].val_aucs, out["0"].val_aucs, atol=1e-3)
    assert abs(out["1"].test_auc - out["0"].test_auc) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_stacked_adam_is_torch_adam(use_graph, monkeypatch):
    """optim.StackedAdam (the Adam update over the module's 4 shared parameter buffers instead of its 4K views) against
    torch.optim.Adam(fused=True) over the parameters, on the same training run, eager and replayed from a HIP graph:
    with torch's own fused kernel over the buffers — losses, validation AUCs, final weights bit for bit (the stacking
    changes nothing); with dl_adam_step (the default) — the same trajectory to rounding; and the eager loop really takes
    the gradients as the stacked tensors the projection's backward produced (no stacking copy)."""
    from disenlink_amd import optim, train
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    sg = synthetic_graph("chameleon", seed=2)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=2)
    run = train.prepare_run(split, torch.device(DEV), row_bytes=8 * 64 * 4)
    x = torch.from_numpy(sg.features()).to(DEV)
    fast = []
    orig = optim.StackedAdam._stacked_grad
    monkeypatch.setattr(optim.StackedAdam, "_stacked_grad",
                        lambda self, key: (lambda g: (fast.append(g.shape == self.model._stacked[key].shape and
                                                                  g.data_ptr() == self.groups[key][0].grad.data_ptr()), g)[1])(orig(self, key)))
    out = {}
    make = optim.StackedAdam
    for mode in ("stacked_torch_kernel", "torch", "stacked_dl_kernel"):
        monkeypatch.setattr(train, "_STACKED_ADAM", mode != "torch")
        # DL_ADAM_KERNEL=torch: torch._fused_adam_ over the stacked buffers (the switch parity runs use)
        monkeypatch.setattr(train, "_ADAM_KERNEL", "torch" if mode == "stacked_torch_kernel" else "dl")
        torch.manual_seed(0)
        model = Disentangle(sg.n_feat, 64, 64, nfactor=8, beta=0.6, t=1).to(DEV)
        res = train.run_link_prediction(model, x, run, epochs=12, lr=1e-3, use_graph=use_graph)
        out[mode] = (res.losses, res.val_aucs, res.test_auc, [p.detach().clone() for p in model.parameters()])
    a, b, c = out["stacked_torch_kernel"], out["torch"], out["stacked_dl_kernel"]
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]           # the stacking itself: bit for bit
    for a_, b_ in zip(a[3], b[3]):
        assert torch.equal(a_, b_)
    # dl_adam_step (the default): torch.optim.Adam's arithmetic up to the rounding of the bias corrections
    # (12 epochs from a saturated start — loss 19: a pair whose sigmoid sits one ulp from 1.0 carries gradient w or 0,
    # so a last-bit difference in the weights can move one pair's whole contribution: 2.4e-5 was seen with the round-4 scorer)
    np.testing.assert_allclose(c[0], b[0], rtol=6e-5)
    np.testing.assert_allclose(c[1], b[1], atol=2e-4)
    for c_, b_ in zip(c[3], b[3]):                                  # (5.7e-5 seen, for the same reason as the loss above)
        assert torch.allclose(c_, b_, rtol=1e-3, atol=1e-4), float((c_ - b_).abs().max())
    assert fast and all(fast), fast[:8]                             # every gradient arrived stacked: no stacking copy


@pytest.mark.gpu
def test_adam_step_kernel_matches_torch_adam_on_odd_sizes():
    """dl_adam_step against torch.optim.Adam (the reference's optimiser, main_disentangled.py:150) on buffers whose sizes
    are not multiples of 4 (the kernel works in float4 units across buffer boundaries), with and without weight decay,
    over 25 steps: parameters and both moments; the step counter lives on the device."""
    import ctypes as C
    from disenlink_amd import _lib
    lib = _lib.load()
    torch.manual_seed(3)
    sizes = [1, 7, 1030, 4096, 65537, 3]
    for wd in (0.0, 5e-4):
        ps = [torch.randn(n, device=DEV) for n in sizes]
        ref = [p.clone().requires_grad_(True) for p in ps]
        opt = torch.optim.Adam(ref, lr=1e-2, weight_decay=wd)
        m = [torch.zeros_like(p) for p in ps]
        v = [torch.zeros_like(p) for p in ps]
        state = torch.zeros(3, device=DEV)
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        numel = (C.c_size_t * len(ps))(*sizes)
        for step in range(25):
            gs = [torch.randn(n, device=DEV) * (0.1 + step) for n in sizes]
            for r, g in zip(ref, gs):
                r.grad = g.clone()
            opt.step()
            _lib.check(lib.dl_adam_step(len(ps), arr(ps), arr(gs), arr(m), arr(v), numel, state.data_ptr(), 1e-2, 0.9, 0.999,
                                        1e-8, wd, torch.cuda.current_stream().cuda_stream), "dl_adam_step")
        assert float(state[0]) == 25.0
        assert abs(float(state[1]) - 1e-2 / (1 - 0.9 ** 25)) < 1e-8 and abs(float(state[2]) - (1 - 0.999 ** 25) ** 0.5) < 1e-7
        for p, r in zip(ps, ref):
            assert torch.allclose(p, r.detach(), rtol=5e-6, atol=5e-7), (wd, p.numel(), float((p - r.detach()).abs().max()))
        for r, mm, vv in zip(ref, m, v):
            st = opt.state[r]
            assert torch.allclose(mm, st["exp_avg"], rtol=1e-5, atol=1e-7) and torch.allclose(vv, st["exp_avg_sq"], rtol=1e-5, atol=1e-9)
    rc = lib.dl_adam_step(9, None, None, None, None, None, state.data_ptr(), 1e-2, 0.9, 0.999, 1e-8, 0.0, None)
    assert rc == -1 and b"n_bufs" in lib.dl_last_error()


def test_bench_gpus_2_launches_itself_and_reports_a_self_contained_scaling_record():
    """`python bench.py --gpus 2` started plainly (as the driver starts it): the parent launches the two ranks, which on
    this one-GPU box share cuda:0 with gloo carrying the collectives (DL_REHEARSE_ON_ONE_GPU: functional only).  The line
    must carry, per block, the same-problem N=1 time measured in the same run, the sharded-vs-unsharded probability
    difference on rank 0's pair slice (expected exactly 0: the plans are shard-independent), the in-run gather A/B and
    the per-step message counts with zero staging copies."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(DL_REHEARSE_ON_ONE_GPU="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--scale", "0.02"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["launch"]["self_launched"]
    assert set(line["blocks"]) == {"snap_patents_strong", "penn94_bf16_strong", "squirrel_weak"}
    for name, b in line["blocks"].items():
        assert b["n1_same_problem_ms"] > 0 and b["ms_per_step"] > 0 and b["value"] > 0, name
        assert b["messages_per_step"]["staging_copies"] == 0, name
        assert set(b["gather_ab"]["z_gather_ms"]) == {"allgather", "p2p", "broadcast"}, name
        assert len(b["per_rank"]) == 2
        if b["scaling"] == "strong":
            assert b["parity"]["max_abs_dprob_sharded_vs_unsharded_rank0_slice"] == 0.0, (name, b["parity"])
            assert b["parity"]["pairs_compared"] > 0
    assert line["n1_same_problem_ms"] == line["blocks"]["snap_patents_strong"]["n1_same_problem_ms"]


def test_cli_gpus_2_trains_row_sharded_and_matches_the_single_gpu_run():
    """`python -m disenlink_amd.main --gpus 2` (main_disentangled.py's flags; the command launches its two ranks itself;
    on this one-GPU box they share cuda:0 and gloo carries the collectives) against the same command on one GPU: same
    seeded split and initial weights, 6 epochs of the reference schedule — the test AUC with the best weights and the
    per-epoch loss must agree (the sharded step sums the weight gradients in another order: 1e-3 on the AUC)."""
    import os
    import re
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    common = ["--dataset", "chameleon", "--synthetic", "--epochs", "6", "--run", "1", "--nfactor", "8", "--nembed", "64",
              "--nhidden", "64", "--lr", "0.005", "--seed", "3"]

    def run(extra, env_extra):
        r = subprocess.run([sys.executable, "-m", "disenlink_amd.main", *common, *extra], env=dict(env, **env_extra),
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        losses = [float(x) for x in re.findall(r"loss: ([0-9.eE+-]+)", r.stdout)]
        auc = float(re.findall(r"test auc: ([0-9.eE+-]+)", r.stdout)[-1])
        return losses, auc

    l1, a1 = run(["--no-graph"], {})
    l2, a2 = run(["--gpus", "2"], {"DL_REHEARSE_ON_ONE_GPU": "1"})
    assert len(l1) == len(l2) == 6
    np.testing.assert_allclose(l2, l1, rtol=2e-4)
    assert abs(a1 - a2) <= 1e-3, (a1, a2)
    assert 0.5 < a2 <= 1.0


def test_compiled_torch_binding_equals_the_python_operators_bit_for_bit():
    """torch.ops.disenlink_native.hot_path_pairs_loss (C++ autograd node over the C ABI) against ops.HotPathPairsLoss
    (Python autograd.Function over ctypes): H, prob, loss and the gradient on Z — for loss.backward() (the scaled last
    kernel) and with a gradient on the embedding as well — are the same bits; the module takes the compiled path by default
    and trains the same trajectory as with DL_NATIVE_OPS=0."""
    from disenlink_amd import native, ops
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.graph import Graph, PairList
    from disenlink_amd.metrics import pair_bce_weights
    from disenlink_amd.splits import make_link_split
    assert native.available(), "libdisenlink_torch.so must be built on the GPU box (python -m disenlink_amd.build)"
    sg = synthetic_graph("chameleon", seed=4)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=4)
    dev = torch.device(DEV)
    graph = Graph.from_edge_rows(torch.from_numpy(split.train_src).to(dev), torch.from_numpy(split.train_dst).to(dev), sg.n_nodes)
    pu = np.concatenate([split.pos_train.u, split.neg_train.u])
    pv = np.concatenate([split.pos_train.v, split.neg_train.v])
    pairs = PairList.build(torch.from_numpy(pu).to(dev), torch.from_numpy(pv).to(dev), sg.n_nodes)
    label = torch.from_numpy(np.concatenate([split.pos_train.label, split.neg_train.label])).to(dev)
    weight = pair_bce_weights(split.pos_train.u.size, split.neg_train.u.size, 5, dev)
    torch.manual_seed(0)
    K, d = 8, 64
    Z0 = (torch.randn(sg.n_nodes, K, d, device=dev) * 0.2)
    out = {}
    for name in ("python", "native"):
        for with_emb in (False, True):
            Z = Z0.clone().requires_grad_(True)
            if name == "python":
                H, prob, loss = ops.HotPathPairsLoss.apply(Z, graph, pairs, 0.6, 1.0, torch.float32, label, weight)
            else:
                H, prob, loss = native.hot_path_pairs_loss(Z, graph, pairs, 0.6, 1.0, label, weight)
            total = loss * 3.0 + ((H * H).sum() * 1e-3 if with_emb else 0.0)
            total.backward()
            out[(name, with_emb)] = (H.detach().clone(), prob.detach().clone(), loss.detach().clone(), Z.grad.clone())
    for with_emb in (False, True):
        for a_, b_, what in zip(out[("python", with_emb)], out[("native", with_emb)], ("H", "prob", "loss", "dZ")):
            assert torch.equal(a_, b_), (what, with_emb, float((a_ - b_).abs().max()))
    assert float(out[("native", False)][3].abs().max()) > 0


@pytest.mark.gpu
def test_device_early_stop_follows_the_reference_bookkeeping():
    """dl_epoch_finish (early_stop.DeviceEarlyStop) against the loop of main_disentangled.py:199-214 restated on the host:
    a scripted sequence of validation score vectors (improving, equal, worse, NaN-free ties) and loss values — per epoch the
    AUC must equal AucPlan.auc's, the best weights must be the parameter values AFTER the step of the last improving epoch,
    patience must stop the bookkeeping at the same epoch, and launches queued after the stop must change nothing."""
    from disenlink_amd.early_stop import DeviceEarlyStop
    from disenlink_amd.metrics import AucPlan
    from disenlink_amd.model import Disentangle
    torch.manual_seed(3)
    model = Disentangle(7, 5, 8, nfactor=3, beta=0.5, t=1).to(DEV)          # odd sizes: the tail elements of the copy
    rng = np.random.default_rng(11)
    n_val = 3000
    label = torch.from_numpy((rng.random(n_val) < 0.3).astype(np.float32)).to(DEV)
    plan = AucPlan(label)
    patience, epochs = 3, 40
    es = DeviceEarlyStop(model, plan, epochs, patience)
    bufs = list(model._stacked.values())
    # the quality of the scores goes up, stalls (ties with the best: NOT an improvement), goes up, then down for good
    quality = [0.1, 0.3, 0.3, 0.2, 0.5, 0.5, 0.4, 0.45, 0.1, 0.1, 0.1, 0.1, 0.9, 0.95]
    base = torch.from_numpy(rng.standard_normal(n_val).astype(np.float32)).to(DEV)
    noise = {q: torch.from_numpy(np.round(rng.standard_normal(n_val), 1).astype(np.float32)).to(DEV) for q in set(quality)}
    best_auc, stale, want_weights, stop_at, hist = 0.0, 0, [b.clone() for b in bufs], None, []
    for e, q in enumerate(quality):
        score = (q * (label * 2 - 1) + noise[q] + 0 * base).contiguous()     # same q -> the same vector -> the same AUC
        loss = torch.tensor(1.0 / (e + 1), dtype=torch.float32, device=DEV)
        with torch.no_grad():
            for b in bufs:
                b.add_(1.0)                                                # "the step"
        es.finish(loss, score)
        es.post(e) if stop_at is None else None
        if stop_at is None:
            auc = float(plan.auc(score))
            hist.append((float(loss), auc))
            if auc > best_auc:
                best_auc, stale, want_weights = auc, 0, [b.clone() for b in bufs]
            else:
                stale += 1
            if stale > patience:
                stop_at = e
    assert stop_at == 8, stop_at                                        # best at epoch 4; 5 (a tie), 6, 7, 8 are the four stale ones
    for e, (lv, av) in enumerate(hist):
        got = es.read(e) if e >= len(hist) - es.RING else None          # the ring keeps the last RING epochs
        if got is not None:
            assert got == (lv, av), (e, got, lv, av)
    got_hist = es.hist[:len(hist)].cpu().numpy()
    np.testing.assert_array_equal(got_hist, np.array(hist, dtype=np.float64))
    assert torch.count_nonzero(es.hist[len(hist):]) == 0                # nothing recorded after the stop
    st = es.state.cpu()
    assert st[:1].view(torch.float64).item() == best_auc and int(st[3]) == 1 and int(st[2]) == stop_at + 1 and int(st[4]) == 4
    assert int(es.u2.item()) == 0
    for b, w in zip(es.best, want_weights):
        assert torch.equal(b, w)
    es.restore()
    for b, w in zip(bufs, want_weights):
        assert torch.equal(b, w)
    es.reset()
    assert int(es.state.abs().sum()) == 0 and all(torch.equal(b, s) for b, s in zip(es.best, bufs))


@pytest.mark.gpu
@pytest.mark.parametrize("patience", [2, 4])
@pytest.mark.parametrize("use_graph", [False, True])
def test_training_with_device_side_early_stopping_equals_the_host_side_loop(use_graph, patience, monkeypatch):
    """run_link_prediction with the end-of-epoch bookkeeping on the device (history read one epoch behind) against the same
    run with DL_DEVICE_EARLY_STOP=0 (the host reads loss and AUC back every epoch, as the reference does): the same losses,
    validation AUCs, stopping epoch, best AUC and test AUC — bit for bit, with a patience small enough to stop the run."""
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    sg = synthetic_graph("chameleon", seed=7)
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=7)
    run = prepare_run(split, torch.device(DEV), row_bytes=8 * 64 * 4)
    x = torch.from_numpy(sg.features()).to(DEV)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DL_DEVICE_EARLY_STOP", mode)
        torch.manual_seed(0)
        model = Disentangle(sg.n_feat, 64, 64, nfactor=8, beta=0.6, t=1).to(DEV)
        # at this step size the validation AUC peaks at the third epoch, dips and comes back: the run stops on patience
        # after 6 / 8 epochs, the best weights are those of epoch 2
        out[mode] = (run_link_prediction(model, x, run, epochs=60, lr=3e-3, patience=patience, use_graph=use_graph),
                     {k: v.clone() for k, v in model.state_dict().items()})
    r1, r0 = out["1"][0], out["0"][0]
    assert r1.epochs_run == r0.epochs_run and r1.epochs_run == {2: 6, 4: 8}[patience], (r1.epochs_run, r0.epochs_run)
    assert r1.losses == r0.losses and r1.val_aucs == r0.val_aucs
    assert r1.best_val_auc == r0.best_val_auc and r1.test_auc == r0.test_auc
    for k in out["1"][1]:
        assert torch.equal(out["1"][1][k], out["0"][1][k]), k                 # the best weights were loaded back


@pytest.mark.gpu
def test_adam_step_counted_by_the_caller_gives_the_bits_of_the_device_counter():
    """dl_adam_step_at (the eager loop counts the steps: one launch) against dl_adam_step (a one-thread launch advances the
    counter in `state`, for graph replays): the same parameters, moments and state floats after every one of 7 steps over
    buffers of odd sizes."""
    import ctypes as C
    from disenlink_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(5)
    sizes = [1037, 64, 4099, 3]
    mk = lambda: [torch.randn(n, generator=g).to(DEV) for n in sizes]
    p0, grads = mk(), [mk() for _ in range(7)]
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    numel = (C.c_size_t * len(sizes))(*sizes)
    out = {}
    for mode in ("device", "host"):
        p = [t.clone() for t in p0]
        m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
        state = torch.zeros(3, dtype=torch.float32, device=DEV)
        trace = []
        for step, gs in enumerate(grads, start=1):
            if mode == "device":
                _lib.check(lib.dl_adam_step(len(p), ptrs(p), ptrs(gs), ptrs(m), ptrs(v), numel, state.data_ptr(), 1e-3, 0.9, 0.999,
                                            1e-8, 5e-4, torch.cuda.current_stream().cuda_stream), "dl_adam_step")
            else:
                _lib.check(lib.dl_adam_step_at(len(p), ptrs(p), ptrs(gs), ptrs(m), ptrs(v), numel, state.data_ptr(), step, 1e-3, 0.9,
                                               0.999, 1e-8, 5e-4, torch.cuda.current_stream().cuda_stream), "dl_adam_step_at")
            trace.append([t.clone() for t in p + m + v] + [state.clone()])
        out[mode] = trace
    for step, (a, b) in enumerate(zip(out["device"], out["host"]), start=1):
        for i, (x_, y_) in enumerate(zip(a, b)):
            assert torch.equal(x_, y_), (step, i)
    assert float(out["host"][-1][-1][0]) == 7.0
    assert lib.dl_adam_step_at(1, ptrs(p0[:1]), ptrs(p0[:1]), ptrs(p0[:1]), ptrs(p0[:1]), numel, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                               None) != 0                                   # step 0: rejected


@pytest.mark.gpu
@pytest.mark.parametrize("K,d,dtype", [(8, 64, torch.float32), (4, 64, torch.float32),           # wave-per-entry kernel
                                       (16, 128, torch.bfloat16), (16, 128, torch.float32),      # wide rows
                                       (5, 32, torch.float32), (8, 32, torch.bfloat16)])         # group-per-entry kernel
def test_per_entry_labels_give_the_same_bits_and_every_probability(K, d, dtype, monkeypatch):
    """Round 6: dl_pair_incidence.entry_yw (PairList.bind_labels) — the labels / loss weights of the training step as a
    coalesced per-entry stream, the weight's sign picking the ONE entry of a pair that writes prob — against the gathers
    through inc_pair: prob, dZ, dH bit for bit, with self pairs, weight-0 pairs, saturated pairs, over the whole list and
    over row shards (where a pair's first endpoint may live in another shard: its probability is then not this shard's to
    write).  The binding happens the SECOND time the same label / weight tensors are seen."""
    from disenlink_amd import ops
    from disenlink_amd.graph import PairList
    G, pairs, Z, label, weight, pu, pv = _one_pass_case(K, d, dtype, seed=57 + K)
    pu[200:206] = pv[200:206]                                         # self pairs: both entries sit in the same row
    wb = 4 if dtype == torch.float32 else 2
    tpu, tpv = torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV)
    N = Z.shape[0]
    Zt = Z if dtype == torch.float32 else Z.to(dtype)
    H = ops.aggregate_fwd(G, Zt, 0.6, *ops.route_fwd(G, Zt, 1.0))
    for t in (1.0, 2.0):
        for rng_ in (None, (0, 4), (4, 301), (301, N)):
            pl = PairList.build(tpu, tpv, N, row_range=rng_, build_by_u=False, row_bytes=K * d * wb, inc_slices=4 if rng_ is None else None)
            monkeypatch.setenv("DL_ENTRY_LABELS", "0")
            ref = ops.score_pairs_train(Zt, H, pl, t, label, weight)
            assert pl._yw is None
            monkeypatch.setenv("DL_ENTRY_LABELS", "1")
            first = ops.score_pairs_train(Zt, H, pl, t, label, weight)            # first sight of (label, weight): still the gathers
            assert pl._yw is None
            got = ops.score_pairs_train(Zt, H, pl, t, label, weight)              # second sight: bound
            assert pl._yw is not None and tuple(pl._yw.shape) == (pl.inc.n_entries, 2)
            lo, hi = (0, N) if rng_ is None else rng_
            mine = torch.from_numpy((pu >= lo) & (pu < hi)).to(DEV)                # pairs whose FIRST endpoint is a row of this plan
            for a, b, c in zip(ref[1:], first[1:], got[1:]):
                assert torch.equal(a[lo:hi], b[lo:hi]) and torch.equal(a[lo:hi], c[lo:hi]), (K, d, t, rng_)
            assert torch.equal(ref[0][mine], got[0][mine]) and not bool(torch.isnan(got[0][mine]).any())
            # a changed label tensor is a new binding (version counter), not a stale one
            label2 = label.clone()
            label2[:50] = 1.0 - label2[:50]
            monkeypatch.setenv("DL_ENTRY_LABELS", "0")
            ref2 = ops.score_pairs_train(Zt, H, pl, t, label2, weight)
            monkeypatch.setenv("DL_ENTRY_LABELS", "1")
            ops.score_pairs_train(Zt, H, pl, t, label2, weight)
            got2 = ops.score_pairs_train(Zt, H, pl, t, label2, weight)
            assert all(torch.equal(a[lo:hi], b[lo:hi]) for a, b in zip(ref2[1:], got2[1:])) and not torch.equal(ref2[1], ref[1])
            label.add_(0.0)                                                       # an in-place write bumps the version: the old binding must go
            got3 = ops.score_pairs_train(Zt, H, pl, t, label, weight)
            assert all(torch.equal(a[lo:hi], b[lo:hi]) for a, b in zip(ref[1:], got3[1:]))
    # SIGNED weights beside them, over the same row shards: a third of the live weights negated, half of the zeros -0.0.  The
    # weight is any real number (the sign convention belongs to the stream alone), so such a tensor is never bound, every
    # entry writes its pair's probability — each pair whose first endpoint lies in the shard has it written by that shard —
    # and the shard's gradient rows are the unsharded bits.
    srng = np.random.default_rng(991 + K)
    signed = weight.clone()
    live, dead = torch.nonzero(weight != 0)[:, 0].cpu().numpy(), torch.nonzero(weight == 0)[:, 0].cpu().numpy()
    signed[torch.from_numpy(srng.choice(live, live.size // 3, replace=False)).to(DEV)] *= -1.0
    signed[torch.from_numpy(srng.choice(dead, dead.size // 2, replace=False)).to(DEV)] = -0.0
    assert int((signed < 0).sum()) > 2000 and int(torch.signbit(signed[weight == 0]).sum()) == 250
    for t in (1.0, 2.0):
        whole = None
        for rng_ in (None, (0, 4), (4, 301), (301, N)):
            pl = PairList.build(tpu, tpv, N, row_range=rng_, build_by_u=False, row_bytes=K * d * wb)
            monkeypatch.setenv("DL_ENTRY_LABELS", "0")
            ref = ops.score_pairs_train(Zt, H, pl, t, label, signed)
            monkeypatch.setenv("DL_ENTRY_LABELS", "1")
            first = ops.score_pairs_train(Zt, H, pl, t, label, signed)
            got = ops.score_pairs_train(Zt, H, pl, t, label, signed)
            assert pl._yw is None                                                  # a set sign bit: the gathers, at every sight
            whole = ref if rng_ is None else whole
            lo, hi = (0, N) if rng_ is None else rng_
            mine = torch.from_numpy((pu >= lo) & (pu < hi)).to(DEV)
            for a, b, c, w_ in zip(ref[1:], first[1:], got[1:], whole[1:]):
                assert torch.equal(a[lo:hi], b[lo:hi]) and torch.equal(a[lo:hi], c[lo:hi]) and torch.equal(a[lo:hi], w_[lo:hi]), (K, d, t, rng_)
            for out_ in (ref, first, got):
                assert torch.equal(out_[0][mine], whole[0][mine]) and not bool(torch.isnan(out_[0][mine]).any()), (K, d, t, rng_)
        # ... and it is the gradient of sum w BCE, sign and all: linear in w, so w and -w give opposite gradients
        neg = ops.score_pairs_train(Zt, H, PairList.build(tpu, tpv, N, build_by_u=False, row_bytes=K * d * wb), t, label, -signed)
        assert torch.equal(neg[0], whole[0]) and torch.equal(neg[1], -whole[1]) and torch.equal(neg[2], -whole[2]), (K, d, t)
    # Labels made AFRESH for every step (a new tensor object each time, which the allocator places at the address of the one
    # just freed, version 0 again): identity is the object, not the address — no step may see an earlier step's stream.
    pl = PairList.build(tpu, tpv, N, build_by_u=False, row_bytes=K * d * wb)
    pl_ref = PairList.build(tpu, tpv, N, build_by_u=False, row_bytes=K * d * wb)      # sees every label tensor once: always the gathers
    monkeypatch.setenv("DL_ENTRY_LABELS", "1")
    addresses, bound = set(), 0
    for stepno in range(6):
        content = label.clone()
        content[stepno * 40:(stepno + 1) * 40] = 1.0 - content[stepno * 40:(stepno + 1) * 40]
        want = ops.score_pairs_train(Zt, H, pl_ref, 1.0, content, weight)
        assert pl_ref._yw is None
        fresh = content.clone()
        addresses.add(fresh.data_ptr())
        got = ops.score_pairs_train(Zt, H, pl, 1.0, fresh, weight)
        bound += pl._yw is not None
        assert all(torch.equal(a, b) for a, b in zip(want[1:], got[1:])), stepno
        del fresh, got, want, content
    assert bound == 0                                                 # no stream was ever bound to a tensor seen once
    # (whether the allocator really handed out the same address twice depends on its state — it did, 3 to 5 times out of 6,
    # in the runs this test was written against; the by-object rule itself is pinned without an allocator in
    # tests/test_host_cpu.py::test_label_stream_is_keyed_on_tensor_objects)


@pytest.mark.gpu
@pytest.mark.parametrize("K,d,dtype", [(8, 64, torch.float32), (10, 64, torch.float32), (16, 128, torch.bfloat16), (3, 8, torch.float32),
                                       (8, 32, torch.bfloat16)])
def test_rows_of_several_units_summed_inside_the_launch_equal_the_combine_launch(K, d, dtype, lib_env):
    """Round 6: aggregation rows of several units (hub rows) are summed by their LAST unit inside the launch
    (publish_unit_and_sum_row: sc1 stores, an agent-scope counter per row, sc1 loads — the units run on different XCDs)
    instead of a separate combine launch: the same bits as that launch (DL_INKERNEL_COMBINE=0), in every repetition, and the
    plan's counters are all zero again afterwards.  Hubs of 2 to ~40 units, rows of one unit in between."""
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph
    rng = np.random.default_rng(91 + K)
    N = 900
    hubs = [(0, 700), (1, 200), (2, 3000), (5, 140)]
    src = np.concatenate([rng.integers(0, N, 4000)] + [np.full(n, h) for h, n in hubs])
    dst = np.concatenate([rng.integers(0, N, 4000)] + [rng.integers(0, N, n) for _h, n in hubs])
    G = Graph.from_edge_rows(torch.from_numpy(src), torch.from_numpy(dst), N, row_bytes=K * d * (4 if dtype == torch.float32 else 2)).to(DEV)
    assert int(G.plan.multi_row.numel()) >= 4 and G.plan.n_slots >= 12             # (duplicate edge rows are binarised away: the hub of 3000 draws keeps ~870 neighbours)
    Z = (torch.randn(N, K, d, generator=torch.Generator().manual_seed(5)) * 0.4).to(DEV)
    Zt = Z if dtype == torch.float32 else Z.to(dtype)
    p, a, s = ops.route_fwd(G, Zt, 1.0)
    dH = torch.randn(N, K, d, generator=torch.Generator().manual_seed(6)).to(DEV)
    acc0 = torch.randn(N, K, d, generator=torch.Generator().manual_seed(7)).to(DEV)
    lib_env("DL_INKERNEL_COMBINE", 0)
    ref = ops.aggregate_fwd(G, Zt, 0.55, p, a, s)
    ref_b = ops.route_aggregate_bwd(G, Zt, 0.55, 1.0, p, a, s, dH)                          # the backward's phase 2 sums such rows too
    ref_acc = ops.route_aggregate_bwd(G, Zt, 0.55, 1.0, p, a, s, dH, dZ_accum=acc0.clone())   # ... also onto an accumulated input
    for mode in (2, 1):                                               # 2: wherever the kernel can; 1: the default rule (rows of few units)
        lib_env("DL_INKERNEL_COMBINE", mode)
        for rep in range(8):
            got = ops.aggregate_fwd(G, Zt, 0.55, p, a, s)
            assert torch.equal(got, ref), (K, d, mode, rep, float((got.float() - ref.float()).abs().max()))
            assert int(G.plan.unit_count.abs().sum()) == 0
        for rep in range(4):
            assert torch.equal(ops.route_aggregate_bwd(G, Zt, 0.55, 1.0, p, a, s, dH), ref_b), (K, d, mode, rep)
            assert torch.equal(ops.route_aggregate_bwd(G, Zt, 0.55, 1.0, p, a, s, dH, dZ_accum=acc0.clone()), ref_acc), (K, d, mode, rep)
            assert int(G.plan.unit_count.abs().sum()) == 0


def _early_stop_trace(aucs, patience):
    """main_disentangled.py:206-213 applied to a validation-AUC sequence -> (epochs run, best epoch, improved flags)."""
    best, stale, best_ep, flags = 0.0, 0, -1, []
    for ep, a in enumerate(aucs):
        if a > best:
            best, stale, best_ep = a, 0, ep
            flags.append(True)
        else:
            stale += 1
            flags.append(False)
        if stale > patience:
            return ep + 1, best_ep, flags
    return len(aucs), best_ep, flags


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager-device", "eager-host", "replayed-device"])
@pytest.mark.parametrize("tag", ["chameleon", "chameleon_fast", "cora"])
def test_convergence_length_runs_follow_the_reference_protocol(tag, mode, monkeypatch):
    """Round 6: the reference's whole per-run protocol (main_disentangled.py:131-224 — fresh split and
    model per run, validation AUC every epoch from the pre-step forward, best weights after the step, patience, test AUC with
    the best weights, mean / std over the runs) at convergence length.  tests/golden/conv_chameleon*.npz hold what the
    reference's model.py did on CPU (make_convergence.py) for 3 seeds on the real chameleon graph at the recipe of
    hyperparameters_setting:2 (K = 5, d = 32, nhid 512, beta 0.7): 400 epochs at its learning rate 1e-4, where the validation
    AUC still improves at nearly every epoch and the patience of 20 never fires, and ("_fast") at learning rate 1e-3, where it
    peaks and decays and the early stop FIRES; conv_cora.npz: Cora (BASELINE.json configs[0]; binary features, not
    standardised) at ITS recipe, hyperparameters_setting:11 (K = 10, d = 64, nhid 256, beta 0.6, lr 1e-3), where the early stop
    fires after 100-200 epochs.  Here: the pair-list loop on the MI355X with the bookkeeping on the device
    (dl_epoch_finish, history read one epoch behind), on the host (the reference's form), and replayed from a HIP graph.
      * the loop's own decisions are exactly the reference's rule applied to ITS validation AUCs (stop epoch, best epoch);
      * every epoch's validation AUC is within 1e-3 of the reference's (fp32 trajectories separate at
        the 1e-3 level after ~25 epochs of saturation), the first 20 epochs within 1e-4, losses within 2 %;
      * stop epoch and best epoch equal the reference's — or the first epoch where the improved / not-improved decision
        differs is a near tie in the reference itself (its AUC within 2e-3 of its running best): that is then the
        explained divergence point;
      * test AUC within 1e-3 per seed, mean over the seeds within 1e-3 of the reference's mean."""
    import json
    import os
    from conftest import GOLDEN_DIR
    from disenlink_amd.datasets import standardise_rows
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    path = os.path.join(GOLDEN_DIR, f"conv_{tag}.npz")
    if not os.path.exists(path):
        pytest.skip(f"{path} not generated")
    g = np.load(path)
    m = json.loads(str(g["meta"]))
    data = np.load(os.path.join(GOLDEN_DIR, f"real_{m['dataset']}.npz"))
    edges = data["edges"].astype(np.int64)
    if m["dataset"] == "cora":                                       # binary features as they are (main_disentangled.py:117-123)
        feats = np.zeros(tuple(data["feat_shape"]), dtype=np.float32)
        feats[data["feat_row"].astype(np.int64), data["feat_col"].astype(np.int64)] = 1.0
        x = torch.from_numpy(feats).to(DEV)
    else:
        feats = data["features"]
        x = torch.from_numpy(standardise_rows(feats)).to(DEV)
    n = feats.shape[0]
    monkeypatch.setenv("DL_DEVICE_EARLY_STOP", "0" if mode == "eager-host" else "1")
    tests_ref, tests_got = [], []
    for seed in m["seeds"]:
        ref_auc, ref_loss = g[f"s{seed}_val_aucs"], g[f"s{seed}_losses"]
        split = make_link_split(edges[:, 0], edges[:, 1], n, m=m["m"], seed=seed)
        assert (split.pos_train.u.size, split.neg_train.u.size, split.val.u.size, split.test.u.size) == tuple(int(v) for v in g[f"s{seed}_counts"])
        torch.manual_seed(seed)
        model = Disentangle(feats.shape[1], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"]).to(DEV)
        res = run_link_prediction(model, x, prepare_run(split, torch.device(DEV), row_bytes=m["K"] * m["d"] * 4), epochs=m["epochs"],
                                  lr=m["lr"], patience=m["patience"], weight_decay=m["weight_decay"], use_graph=mode.startswith("replayed"))
        aucs = np.array(res.val_aucs)
        # (1) the loop's decisions = the rule on its own AUCs
        run_o, best_o, flags_o = _early_stop_trace(aucs, m["patience"])
        assert res.epochs_run == run_o == len(aucs), (seed, res.epochs_run, run_o)
        assert abs(res.best_val_auc - aucs[best_o]) == 0.0
        # (2) trajectory against the reference's
        run_r, best_r, flags_r = int(g[f"s{seed}_epochs_run"]), int(g[f"s{seed}_best_epoch"]), _early_stop_trace(ref_auc, m["patience"])[2]
        assert _early_stop_trace(ref_auc, m["patience"])[:2] == (run_r, best_r)
        k = min(len(aucs), len(ref_auc))
        assert np.abs(aucs[:20] - ref_auc[:20]).max() <= 1e-4, (seed, np.abs(aucs[:20] - ref_auc[:20]).max())
        assert np.abs(aucs[:k] - ref_auc[:k]).max() <= 1e-3, (seed, np.abs(aucs[:k] - ref_auc[:k]).max())
        np.testing.assert_allclose(np.array(res.losses)[:k], ref_loss[:k], rtol=2e-2)
        # (3) stop / best epoch: equal, or diverging at a near tie of the reference itself
        if (run_o, best_o) != (run_r, best_r):
            first = next(e for e in range(k) if flags_o[e] != flags_r[e])
            margin = abs(ref_auc[first] - ref_auc[:first].max())
            print(f"conv_{tag} seed {seed} {mode}: stop/best ({run_o}, {best_o}) vs reference ({run_r}, {best_r}); decisions first differ at "
                  f"epoch {first}, where the reference's AUC is {margin:.2e} from its running best and ours differs by "
                  f"{abs(aucs[first] - ref_auc[first]):.2e}")
            assert margin <= 2e-3, (seed, first, margin)
        # (4) test AUC with the best weights
        assert abs(res.test_auc - float(g[f"s{seed}_test_auc"])) <= 1e-3, (seed, res.test_auc, float(g[f"s{seed}_test_auc"]))
        tests_ref.append(float(g[f"s{seed}_test_auc"]))
        tests_got.append(res.test_auc)
    assert abs(np.mean(tests_got) - m["test_auc_mean"]) <= 1e-3
    print(f"conv_{tag} {mode}: test AUC {np.mean(tests_got):.6f} +- {np.std(tests_got):.6f} (reference {m['test_auc_mean']:.6f} +- {m['test_auc_std']:.6f})")



@pytest.mark.gpu
def test_link_pred_indexed_with_fresh_index_tensors_every_step_is_learnt_by_object_not_by_address():
    """``a_pred[rows, cols]`` with index tensors made AFRESH for every step (the allocator hands the new ones the address
    of the ones just freed, version 0 again) and OTHER contents each time: ops.LinkPred recognises index tensors by object,
    so every step's entries enter the pair plan of the dense backward — including saturated ones, which carry no gradient
    and which the safety net (learning from the non-zero gradient) would therefore never add."""
    import torch.nn.functional as F
    from disenlink_amd.model import Disentangle
    rng = np.random.default_rng(12)
    N, Fd = 300, 24
    src, dst = rng.integers(0, N, 2500), rng.integers(0, N, 2500)
    adj = torch.zeros(N, N, device=DEV)
    adj[torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)] = 1
    adj_sym = ((adj + adj.t()) != 0).float()
    x = torch.from_numpy(rng.standard_normal((N, Fd)).astype(np.float32) * 1.5).to(DEV)       # large enough for saturated scores
    torch.manual_seed(4)
    model = Disentangle(Fd, 32, 32, nfactor=4, beta=0.6, t=1).to(DEV)
    addresses, taken = set(), []
    for stepno in range(5):
        rows = torch.from_numpy(rng.integers(0, N, 6000)).to(DEV)
        cols = torch.from_numpy(rng.integers(0, N, 6000)).to(DEV)
        addresses.add((rows.data_ptr(), cols.data_ptr()))
        _h, a_pred = model(x, adj_sym)
        vals = a_pred[rows, cols]
        assert int((vals == 1).sum()) > 0                             # saturated entries are really among them
        F.binary_cross_entropy(vals, adj_sym[rows, cols]).backward()
        model.zero_grad()
        taken.append(rows * N + cols)
        plan = model._dense_plan.flat
        assert bool(torch.isin(torch.cat(taken), plan).all()), stepno
        del rows, cols, vals, a_pred, _h
    # (address reuse depends on the allocator's state: typically 2 to 3 of the 5 steps share a rows / cols address)


@pytest.mark.gpu
def test_the_unchanged_reference_loop_teaches_the_dense_backward_its_masks_in_one_epoch():
    """Round 6: the drop-in module inside the reference's loop as it is written
    (main_disentangled.py:192-214: dense masks, ``a_pred[pos_train_adj == 1]``, F.binary_cross_entropy, Adam, the validation
    gather after the step) with NOTHING declared.  link_pred is an ops.LinkPred: its indexing tells the module which entries
    are taken, so the pair plan of dl_score_allpairs_bwd is built from the train masks at the first backward, extended once
    by the validation mask, and never again — learning from the gradients alone rebuilt it in every epoch, because every
    epoch desaturates a few more pairs.  Parameters after 12 epochs equal those of the run that declared its masks
    (assume_static_loss_masks) to rounding, and equal the gradient-learnt run's."""
    import torch.nn.functional as F
    from disenlink_amd.model import Disentangle
    rng = np.random.default_rng(3)
    N, Fd, K, d = 300, 24, 4, 32
    src, dst = rng.integers(0, N, 2500), rng.integers(0, N, 2500)
    ori = torch.zeros(N, N, device=DEV)
    ori[torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)] = 1
    tr = rng.random(2500) < 0.85
    adj = torch.zeros(N, N, device=DEV)
    adj[torch.from_numpy(src[tr]).to(DEV), torch.from_numpy(dst[tr]).to(DEV)] = 1
    adj_sym = ((adj + adj.t()) != 0).float()
    pos_train_adj = torch.zeros(N, N, device=DEV).index_put_((torch.from_numpy(src[tr]).to(DEV), torch.from_numpy(dst[tr]).to(DEV)),
                                                             torch.ones(int(tr.sum()), device=DEV), accumulate=True)
    nu, nv = rng.integers(0, N, 8000), rng.integers(0, N, 8000)
    neg_train_adj = torch.zeros(N, N, device=DEV).index_put_((torch.from_numpy(nu).to(DEV), torch.from_numpy(nv).to(DEV)),
                                                             torch.ones(8000, device=DEV), accumulate=True)
    all_val_adj = torch.zeros(N, N, device=DEV)
    all_val_adj[torch.from_numpy(src[~tr]).to(DEV), torch.from_numpy(dst[~tr]).to(DEV)] = 1
    all_val_adj[torch.from_numpy(rng.integers(0, N, 600)).to(DEV), torch.from_numpy(rng.integers(0, N, 600)).to(DEV)] = 1
    x = torch.from_numpy(rng.standard_normal((N, Fd)).astype(np.float32) * 1.5).to(DEV)      # large enough for saturated scores

    def loop(mode, epochs=12):
        os.environ["DL_LINK_PRED_SUBCLASS"] = "0" if mode == "gradients" else "1"
        try:
            torch.manual_seed(4)
            model = Disentangle(Fd, 32, d, nfactor=K, beta=0.6, t=1).to(DEV)
            if mode == "declared":
                model.assume_static_loss_masks(pos_train_adj, neg_train_adj)
            opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
            builds = []
            for _ in range(epochs):
                _h, a_pred = model(x, adj_sym)
                assert isinstance(a_pred, torch.Tensor)
                loss = F.binary_cross_entropy(a_pred[pos_train_adj == 1].unsqueeze(0), ori[pos_train_adj == 1].unsqueeze(0)) + \
                    F.binary_cross_entropy(a_pred[neg_train_adj == 1].unsqueeze(0), ori[neg_train_adj == 1].unsqueeze(0)) / 5
                opt.zero_grad()
                loss.backward()
                opt.step()
                pred_score = a_pred[all_val_adj == 1]
                assert type(pred_score) is torch.Tensor and pred_score.numel() == int((all_val_adj == 1).sum())
                builds.append(model._dense_plan.rebuilds)
            return [p.detach().clone() for p in model.parameters()], builds, model
        finally:
            os.environ.pop("DL_LINK_PRED_SUBCLASS", None)
    import os
    w_idx, b_idx, m_idx = loop("indexing")
    w_dec, b_dec, _m = loop("declared")
    w_grd, b_grd, _m = loop("gradients")
    assert b_dec[-1] == 1                                             # declared: built once
    assert b_idx[0] == 1 and b_idx[-1] == 2 and b_idx[1] == 2, b_idx   # train masks at the first backward, + the validation mask, then never again
    support = int(((pos_train_adj == 1) | (neg_train_adj == 1) | (all_val_adj == 1)).sum())    # what the loop takes: entries == 1 of the SUMMED masks
    assert m_idx._dense_plan.flat.numel() == support
    for a, b, c in zip(w_idx, w_dec, w_grd):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7) and torch.allclose(a, c, rtol=1e-5, atol=1e-7)
    assert b_grd[-1] >= b_idx[-1]                                     # what the indexing saves (saturated pairs wake up epoch by epoch)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 4])
@pytest.mark.parametrize("t", [1.0, 2.0])
def test_wave_per_entry_forward_scorer_gives_the_training_scorers_bits(K, t, lib_env):
    """Round 6: score_fwd_wave_kernel (d = 64, fp32) — the forward scorer in the geometry of the one-pass training scorer.
    Its probabilities are the training scorer's bit for bit (the same operations up to the sigmoid), the pass that stores the
    per-factor terms for the separate backward gives the same probabilities as the plain pass, and the group-per-entry
    kernel it replaces at this shape (DL_FWD_GROUP_KERNEL=1; still the kernel of every other shape) agrees to rounding in
    probabilities and stored terms — on a problem with saturated scores, self pairs, rows of many segments."""
    from disenlink_amd import ops
    G, pairs, Z, label, weight, pu, pv = _one_pass_case(K, 64, torch.float32, seed=77 + K)
    H = ops.aggregate_fwd(G, Z, 0.6, *ops.route_fwd(G, Z, t))
    lib_env("DL_FWD_GROUP_KERNEL")
    prob_w = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs)
    prob_wc, coef_w = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs, want_coef=True)
    prob_t = ops.score_pairs_train(Z, H, pairs, t, label, weight)[0]
    assert torch.equal(prob_w, prob_t) and torch.equal(prob_wc, prob_w)
    lib_env("DL_FWD_GROUP_KERNEL", 1)
    prob_g, coef_g = ops.score_pairs_fwd(Z, H, pairs.pu, pairs.pv, t, pairs, want_coef=True)
    lib_env("DL_FWD_GROUP_KERNEL")
    assert float((prob_g - prob_w).abs().max()) <= 3e-7
    assert int((prob_w == 1.0).sum()) >= 20                            # the saturated pairs are there
    fin = torch.isfinite(coef_g)
    assert torch.equal(fin, torch.isfinite(coef_w))
    for plane in range(2):                                              # e_k and q_k e_k, each against its own largest finite value
        m = fin[plane]
        err = (coef_w[plane][m] - coef_g[plane][m]).abs().max()
        assert float(err) <= 1e-5 * float(coef_g[plane][m].abs().max()), (plane, float(err))
    # both backward forms from the wave kernel's stored terms agree with the one-pass gradients (through the loss gradient)
    pr = prob_w.detach().clone().requires_grad_(True)
    (g_prob,) = torch.autograd.grad(ops.PairBCE.apply(pr, label, weight), pr)
    dZ0, dH0 = ops.score_pairs_bwd(Z, H, pairs, t, prob_w, g_prob, coef=coef_w)
    _p, dZ1, dH1 = ops.score_pairs_train(Z, H, pairs, t, label, weight)
    for a, b in ((dZ0, dZ1), (dH0, dH1)):
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-12
