"""The autograd Functions of the training step against the same step spelled from the raw wrappers, bit for bit (int32 views
of outputs and gradients): the kernels sum in a fixed order and use no float atomics, so equality is the bar and there is
no tolerance in this file.  Everything runs on the graph and pair list of ref64.structure() — rows on every plan boundary —
at the smallest tuned shape the library reports for each table type, at (4, 32) and at one fp32 shape without a tuned kernel.

Also here: Disentangle._rank_tables against the tables HotPathPairs saves on the same module; two graphs of different sizes
and a pair list taking turns on the device's one workspace; and forward(x, adj) in "plan" and "dense" mode at N = 129,
K = 2, d = 33 (one row past a 128-row tile, one column past a 32-column step) against the raw score_allpairs_* wrappers."""
import numpy as np
import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNTUNED = ref64.UNTUNED[0]                                            # (3, 5): asserted below to have no tuned kernel


def _cases():
    from disenlink_amd import _lib
    lib = _lib.load()
    smallest = lambda dtype: min(ref64.tuned_shapes(lib, dtype), key=lambda s: (s[0] * s[1], s))
    assert not lib.dl_has_fast_path_dtype(*UNTUNED, _lib.DL_F32)
    cases = [("f32", *smallest("f32")), ("bf16", *smallest("bf16")), ("f32", 4, 32), ("f32", *UNTUNED)]
    return sorted(set(cases), key=cases.index)


_device = {}


def _structure():
    if not _device:
        from disenlink_amd.graph import PairList
        st = ref64.structure()
        _device["v"] = (st.graph.to(DEV), PairList.build(st.pu.to(DEV), st.pv.to(DEV), ref64.N_NODES))
    return _device["v"]


def _bits(x):
    x = x.detach().contiguous().reshape(-1)
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _same(what, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert bool(torch.isfinite(want.float()).all()), what
    assert torch.equal(_bits(got), _bits(want)), what


def _randn(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV)


def _tables(K, d, seed=0):
    gen = torch.Generator().manual_seed(1000 * K + d + seed)
    return _randn(gen, ref64.N_NODES, K, d, scale=0.3 * (32 / d) ** 0.5 * (4 / K) ** 0.25), gen


def _raw_pair_bce(prob, label, weight):
    """dl_pair_bce called as the C ABI has it, on 8 KiB of scratch of the test's own -> (loss [1], d loss / d prob)."""
    from disenlink_amd import _lib
    loss, g = torch.full((1,), float("nan"), device=DEV), torch.full_like(prob, float("nan"))
    ws = torch.empty(8192, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().dl_pair_bce(prob.data_ptr(), label.data_ptr(), weight.data_ptr(), prob.numel(), loss.data_ptr(),
                                       g.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
               "dl_pair_bce")
    return loss, g


@pytest.mark.parametrize("dtype,K,d", _cases(), ids=lambda v: str(v))
def test_functions_equal_the_step_spelled_from_the_raw_wrappers(dtype, K, d):
    from disenlink_amd import _lib, ops
    G, pairs = _structure()
    tdt, code = (torch.float32, _lib.DL_F32) if dtype == "f32" else (torch.bfloat16, _lib.DL_BF16)
    beta, t = 0.6, 1.0
    Z0, gen = _tables(K, d)
    P = pairs.n_pairs
    g_emb, g_prob = _randn(gen, *Z0.shape, scale=0.1), _randn(gen, P, scale=0.1)
    label = (torch.rand(P, generator=gen) < 0.3).float().to(DEV)
    weight = (torch.rand(P, generator=gen) * 0.8 + 0.2).div(64).to(DEV)
    weight[::8] = 0.0
    leaf = lambda: Z0.clone().requires_grad_(True)
    # the step's tables, spelled from the raw wrappers
    Zt = Z0 if tdt == torch.float32 else Z0.to(tdt)
    p, a, s = ops.route_fwd(G, Zt, t)
    H = ops.aggregate_fwd(G, Zt, beta, p, a, s)
    assert H.dtype == tdt

    if dtype == "f32":
        # RouteAggregate
        Z = leaf()
        got = ops.RouteAggregate.apply(Z, G, beta, t)
        _same("RouteAggregate H", got, H)
        got.backward(g_emb)
        _same("RouteAggregate dZ", Z.grad, ops.route_aggregate_bwd(G, Z0, beta, t, p, a, s, g_emb))
        # ScorePairs
        Z, Hl = leaf(), H.clone().requires_grad_(True)
        got = ops.ScorePairs.apply(Z, Hl, pairs, t)
        prob, coef = ops.score_pairs_fwd(Z0, H, pairs.pu, pairs.pv, t, pairs, want_coef=True)
        assert (coef is not None) == ((K, d) != UNTUNED)
        _same("ScorePairs prob", got, prob)
        got.backward(g_prob)
        dZ, dH = ops.score_pairs_bwd(Z0, H, pairs, t, prob, g_prob, coef=coef)
        _same("ScorePairs dZ", Z.grad, dZ)
        _same("ScorePairs dH", Hl.grad, dH)

    # HotPathPairs
    Z = leaf()
    emb, got = ops.HotPathPairs.apply(Z, G, pairs, beta, t, tdt)
    prob, coef = ops.score_pairs_fwd(Zt, H, pairs.pu, pairs.pv, t, pairs, want_coef=True)
    _same("HotPathPairs emb", emb, H.float())
    _same("HotPathPairs prob", got, prob)
    torch.autograd.backward([emb, got], [g_emb, g_prob])
    dZ, dH = ops.score_pairs_bwd(Zt, H, pairs, t, prob, g_prob, coef=coef)
    dH += g_emb
    ops.route_aggregate_bwd(G, Zt, beta, t, p, a, s, dH, dZ_accum=dZ)
    _same("HotPathPairs dZ", Z.grad, dZ)

    # PairBCE
    pl = prob.clone().requires_grad_(True)
    loss = ops.PairBCE.apply(pl, label, weight)
    raw_loss, raw_g = _raw_pair_bce(prob, label, weight)
    _same("PairBCE loss", loss.reshape(1), raw_loss)
    g_loss = torch.tensor(0.7, device=DEV)
    loss.backward(g_loss)
    _same("PairBCE d prob", pl.grad, raw_g * g_loss)

    # HotPathPairsLoss (the one-pass scorer: tuned shapes), its three backward cases.  (Fresh label / weight objects per
    # call: PairList.bind_labels then never switches to the per-entry stream, in either spelling.)
    if not ops.score_pairs_train_supported(pairs, K, d, code):
        assert (K, d) == UNTUNED
        return
    prob, dZs, dHs = ops.score_pairs_train(Zt, H, pairs, t, label.clone(), weight.clone())
    raw_loss, _ = _raw_pair_bce(prob, label, weight)

    def step():
        Z = leaf()
        emb, pr, loss = ops.HotPathPairsLoss.apply(Z, G, pairs, beta, t, tdt, label.clone(), weight.clone())
        _same("HotPathPairsLoss emb", emb, H.float())
        _same("HotPathPairsLoss prob", pr, prob)
        _same("HotPathPairsLoss loss", loss.reshape(1), raw_loss)
        return Z, emb, pr, loss

    Z, emb, pr, loss = step()                                            # 1. the loss alone: d/dloss inside the last kernel
    loss.backward(g_loss)
    _same("HotPathPairsLoss dZ, loss only", Z.grad,
          ops.route_aggregate_bwd_scaled(G, Zt, beta, t, p, a, s, dHs, dZs, g_loss))
    Z, emb, pr, loss = step()                                            # 2. gradients on loss, prob and emb
    torch.autograd.backward([emb, pr, loss], [g_emb, g_prob, g_loss])
    dZ, dH = dZs * g_loss, dHs * g_loss
    dZ2, dH2 = ops.score_pairs_bwd(Zt, H, pairs, t, prob, g_prob)
    dZ += dZ2
    dH += dH2
    dH += g_emb
    ops.route_aggregate_bwd(G, Zt, beta, t, p, a, s, dH, dZ_accum=dZ)
    _same("HotPathPairsLoss dZ, loss + prob + emb", Z.grad, dZ)
    Z, emb, pr, loss = step()                                            # 3. no gradient on the loss
    torch.autograd.backward([emb, pr], [g_emb, g_prob])
    dZ, dH = ops.score_pairs_bwd(Zt, H, pairs, t, prob, g_prob)
    dH += g_emb
    ops.route_aggregate_bwd(G, Zt, beta, t, p, a, s, dH, dZ_accum=dZ)
    _same("HotPathPairsLoss dZ, prob + emb", Z.grad, dZ)


def test_rank_tables_are_the_tables_the_training_step_saves():
    from disenlink_amd.model import Disentangle
    G, pairs = _structure()
    K, d = _cases()[1][1:]
    torch.manual_seed(5)
    model = Disentangle(24, 16, d, nfactor=K, beta=0.6, t=1, table_dtype=torch.bfloat16).to(DEV)
    x = _randn(torch.Generator().manual_seed(6), ref64.N_NODES, 24, scale=0.3)
    _emb, prob = model.forward_pairs(x, G, pairs)
    Zt, H = prob.grad_fn.saved_tensors[:2]
    Zr, Hr = model._rank_tables(x, G, torch.bfloat16)
    assert Zr.dtype == Hr.dtype == torch.bfloat16 and not Zr.requires_grad and not Hr.requires_grad
    _same("Z", Zr, Zt)
    _same("H", Hr, H)


def test_two_graphs_and_a_pair_list_take_turns_on_one_workspace():
    from disenlink_amd import _lib, ops
    from disenlink_amd.graph import Graph
    G, pairs = _structure()
    _dtype, K, d = _cases()[0]
    rng = np.random.default_rng(11)
    n2 = 150
    G2 = Graph.from_edge_rows(torch.from_numpy(rng.integers(0, n2, 2000)).to(DEV),
                              torch.from_numpy(rng.integers(0, n2, 2000)).to(DEV), n2)
    Z, gen = _tables(K, d, seed=1)
    Z2 = Z[:n2].contiguous()
    label = (torch.rand(pairs.n_pairs, generator=gen) < 0.3).float().to(DEV)
    weight = torch.full((pairs.n_pairs,), 1 / 64, device=DEV)
    need = lambda owner: int(_lib.load().dl_workspace_bytes(owner.c_plan(), K, d))
    assert len({need(G), need(G2), need(pairs)}) > 1                     # (the turns are between different needs)
    first = {}

    def turn(key, owner, outs):
        assert ops._ws.buf[torch.device(DEV)].numel() >= need(owner), key
        for i, out in enumerate(outs):
            _same(f"{key}[{i}]", out, first.setdefault((key, i), out))

    for _ in range(3):
        p2, a2, s2 = ops.route_fwd(G2, Z2, 1.0)
        turn("route small", G2, (a2, s2))
        p, a, s = ops.route_fwd(G, Z, 1.0)
        turn("route", G, (a, s))
        H2 = ops.aggregate_fwd(G2, Z2, 0.6, p2, a2, s2)
        turn("aggregate small", G2, (H2,))
        H = ops.aggregate_fwd(G, Z, 0.6, p, a, s)
        turn("aggregate", G, (H,))
        turn("train scorer", pairs, ops.score_pairs_train(Z, H, pairs, 1.0, label.clone(), weight.clone()))
        turn("backward small", G2, (ops.route_aggregate_bwd(G2, Z2, 0.6, 1.0, p2, a2, s2, H2),))
        turn("backward", G, (ops.route_aggregate_bwd(G, Z, 0.6, 1.0, p, a, s, H),))


@pytest.mark.parametrize("mode", ["plan", "dense"])
def test_forward_link_pred_equals_the_raw_allpairs_wrappers(mode):
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph, PairList
    from disenlink_amd.model import Disentangle
    N, K, d, F = 129, 2, 33, 12
    rng = np.random.default_rng(3)
    adj = np.zeros((N, N), np.float32)
    adj[rng.integers(0, N, 500), rng.integers(0, N, 500)] = 1
    adj = torch.from_numpy(((adj + adj.T) != 0).astype(np.float32)).to(DEV)
    x = torch.from_numpy((rng.standard_normal((N, F)) * 0.3).astype(np.float32)).to(DEV)
    mask = torch.from_numpy(rng.random((N, N)) < 0.1).to(DEV)
    w = torch.from_numpy(rng.standard_normal((N, N)).astype(np.float32) * 0.1).to(DEV)
    torch.manual_seed(9)
    model = Disentangle(F, 8, d, nfactor=K, beta=0.6, t=1, link_pred_backward=mode).to(DEV)
    graph = Graph.from_dense(adj)

    def loss_of(link_pred):
        if mode == "plan":                                               # the reference's caller: a loss on link_pred[mask]
            return (link_pred[mask] * w[mask]).sum()
        return (link_pred * w).sum() + link_pred.mean()                  # any loss: every entry carries gradient

    emb, link_pred = model(x, graph)
    assert isinstance(link_pred, ops.LinkPred) == (mode == "plan")
    loss_of(link_pred).backward()
    got = [p.grad.clone() for p in model.parameters()]
    model.zero_grad(set_to_none=True)

    # the same step from the raw wrappers: the scorer's gradients are handed to autograd at (Z, H)
    t = float(model.temperature)
    Z = model.project(x)
    H = ops.RouteAggregate.apply(Z, graph, float(model.beta), t)
    prob = ops.score_allpairs_fwd(Z.detach(), H.detach(), t)
    _same("link_pred", link_pred.as_subclass(torch.Tensor), prob)
    _same("emb", emb, H.view(N, -1))
    leaf = prob.clone().requires_grad_(True)
    loss_of(leaf).backward()
    if mode == "plan":
        flat = torch.nonzero(mask.reshape(-1)).reshape(-1)
        plan = PairList.build(torch.div(flat, N, rounding_mode="floor"), flat % N, N, build_by_u=False)
        dZ, dH = ops.score_allpairs_bwd(Z.detach(), H.detach(), plan, t, prob, leaf.grad)
    else:
        dZ, dH = ops.score_allpairs_bwd_dense(Z.detach(), H.detach(), t, prob, leaf.grad)
    torch.autograd.backward([Z, H], [dZ, dH])
    for (name, p), g in zip(model.named_parameters(), got):
        _same(name, g, p.grad)
