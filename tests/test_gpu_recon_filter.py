"""The whole-graph reconstruction loss under a node-group rule (dl_score_recon_filtered, dl_score_recon_logits_filtered;
ops.score_recon_loss(..., node_filter=...), ReconSets.node_filter, Disentangle.forward_recon_loss(..., node_filter=...),
run_link_prediction(recon_node_filter=...)): against the fp64 restatement with every denied pair ignored
(tests/recon_filter_ref.py), bit for bit against the unfiltered call whose ignored set lists every denied pair, and itself
bit for bit across strip heights, slice counts and calls."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import recon_filter_ref as rf
import recon_logits_ref as rl
import recon_ref
from conftest import load_golden
from test_gpu_recon import POISON, _bits, _same, _sync_debug_mode_is_honoured, check
from test_gpu_recon_logits import check as check_logits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from disenlink_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()


def _loss_fn(logits):
    from disenlink_amd import ops
    return ops.score_recon_logits_loss if logits else ops.score_recon_loss


@functools.lru_cache(maxsize=None)
def _inputs(N, K, d):
    """Tables and pair sets of a grid point (CPU; shared, never changed)."""
    Z, H = recon_ref.tables_cpu(N, K, d, recon_ref.table_seed(N, K, d))
    pos, ign = recon_ref.pair_sets(N, seed=N)
    return Z, H, pos, ign


# ------------------------------------------------------------------------------------------------------ 1. the fp64 grid
@pytest.mark.parametrize("N,Kd,rule", list(itertools.product((1, 2, 37, 128, 129, 300), ((1, 8), (3, 100), (8, 64)),
                                                             rf.RULES + rf.PLACED)))
def test_loss_gradients_and_counts_match_fp64(N, Kd, rule):
    K, d = Kd
    Z, H, pos, ign = _inputs(N, K, d)
    nf = rf.make_rule(rule, N, DEV)
    denied = ~rf.allowed_matrix(nf)
    if rule == "tiles" and N == 300:                                   # whole tile pairs are denied, off the diagonal too
        assert bool(denied[:128, 256:].all()) and bool(denied[128:256, 128:256].all()) and not bool(denied[:128, 128:256].any())
    if rule == "alternating" and N >= 37:                              # every 32-bit mask word of every row is mixed
        assert bool((denied[:, :32].sum(1) == 16).all())
    Zg, Hg, pg, ig = Z.to(DEV), H.to(DEV), pos.to(DEV), ign.to(DEV)
    for t in (1.0, 2.0):
        tag = f"N={N} K={K} d={d} t={t} rule={rule}"
        check(tag, _loss_fn(False)(Zg, Hg, t, pg, ig, node_filter=nf), recon_ref.recon64(Z, H, t, pos, ign | denied))
        check_logits(tag, _loss_fn(True)(Zg, Hg, t, pg, ig, node_filter=nf), rl.recon_logits64(Z, H, t, pos, ign | denied))


# ------------------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("N,K,d", [(300, 8, 64), (129, 3, 100), (300, 3, 100), (129, 8, 64)])
def test_bits_of_the_unfiltered_call_that_lists_every_denied_pair(N, K, d, logits):
    from disenlink_amd import ops
    fn = _loss_fn(logits)
    Z, H, pos, ign = _inputs(N, K, d)
    Zg, Hg, pg, ig = Z.to(DEV), H.to(DEV), pos.to(DEV), ign.to(DEV)
    for rule in rf.RULES + rf.PLACED:
        nf = rf.make_rule(rule, N, DEV)
        listed = (ign | ~rf.allowed_matrix(nf)).to(DEV)
        for pw in (None, 3.5):
            got, want = fn(Zg, Hg, 1.0, pg, ig, pos_weight=pw, node_filter=nf), fn(Zg, Hg, 1.0, pg, listed, pos_weight=pw)
            for name, a, b in zip(("loss", "dZ", "dH", "counts"), _bits(got), _bits(want)):
                assert torch.equal(a, b), (rule, pw, name, int((a != b).sum()))
            for x in _bits(got)[1:3]:
                assert not bool((x == POISON).any())
    sets = ops.recon_sets(pg, ig, N, DEV, node_filter=rf.make_rule("all", N, DEV))      # a rule that allows everything
    assert sets.node_filter is not None
    assert _same(fn(Zg, Hg, 1.0, sets), fn(Zg, Hg, 1.0, pg, ig))


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("rule", ["between", "tiles", "only63"])
def test_bits_do_not_depend_on_the_strip_height_the_slice_count_or_the_call(rule, logits, lib_env):
    from disenlink_amd import _lib, ops
    assert ops._POISON, "the tests run with DL_POISON=1 (conftest.py)"
    N, K, d = 300, 8, 64
    fn = _loss_fn(logits)
    Z, H, pos, ign = _inputs(N, K, d)
    Zg, Hg = Z.to(DEV), H.to(DEV)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV, node_filter=rf.make_rule(rule, N, DEV))
    whole = fn(Zg, Hg, 1.0, sets)
    ops.check_recon_counts(whole[3], sets)
    for x in _bits(whole)[1:3]:
        assert not bool((x == POISON).any())
    assert bool(torch.isfinite(whole[1]).all()) and bool(torch.isfinite(whole[2]).all()) and bool(torch.isfinite(whole[0]))
    assert _same(whole, fn(Zg, Hg, 1.0, sets))                                    # two calls
    assert _lib.score_recon_form(N, K, d, 0)["strips"] == 1
    for b in (None, 128, 256):
        assert _same(whole, fn(Zg, Hg, 1.0, sets, block_rows=b)), b
    for forced in (1, 2, 5):                                                      # the scan's slice count
        lib_env("DL_RANK_SLICES", forced)
        nt = -(-N // 128)
        tps = -(-nt // min(forced, nt))
        assert _lib.score_topk_form(N, K, d, 128, 1)["slices"] == -(-nt // tps)
        assert _same(whole, fn(Zg, Hg, 1.0, sets, block_rows=128)), forced
        assert _same(whole, fn(Zg, Hg, 1.0, sets)), forced
        lib_env("DL_RANK_SLICES")


# ------------------------------------------------------------------------------------------------------ 3. bf16 tables
@pytest.mark.parametrize("logits", [False, True])
def test_bf16_tables_give_the_bits_of_the_fp32_call_on_the_rounded_tables(logits):
    from disenlink_amd import ops
    N, K, d = 300, 4, 32
    fn = _loss_fn(logits)
    Z, H, pos, ign = _inputs(N, K, d)
    Zb, Hb = Z.to(BF16).to(DEV), H.to(BF16).to(DEV)
    for rule in ("between", "alternating", "only63"):
        sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV, node_filter=rf.make_rule(rule, N, DEV))
        got, want = fn(Zb, Hb, 1.0, sets, table_dtype=BF16), fn(Zb.float(), Hb.float(), 1.0, sets)
        assert bool(torch.isfinite(want[1]).all()) and bool(torch.isfinite(want[2]).all()) and bool(torch.isfinite(want[0]))
        for name, a, b in zip(("loss", "dZ", "dH", "counts"), _bits(got), _bits(want)):
            assert torch.equal(a, b), (rule, name, int((a != b).sum()))
        ops.check_recon_counts(got[3], sets)
        assert _same(got, fn(Z.to(DEV), H.to(DEV), 1.0, sets, table_dtype=BF16))    # fp32 tensors are rounded inside


# ------------------------------------------------------------------------------------------------------ 4. module and loop
def _sd(g):
    return {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}


def _module(g, table_dtype=torch.float32):
    from disenlink_amd.model import Disentangle
    m = g["meta"]
    model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"], table_dtype=table_dtype)
    model.load_state_dict(_sd(g))
    return model.to(DEV)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("name", recon_ref.MODULE_CASES)
def test_module_parameter_gradients_match_fp64_autograd_of_the_dense_formulation(name, logits):
    """forward_recon[_logits]_loss(..., node_filter=nf).backward() against CPU fp64 autograd of the oracle's dense forward under
    the masked, weighted BCE over the pairs the rule admits; recon_ref.MODULE_TOL x scale, on recon_ref.MODULE_CASES, which
    stay unsaturated under the rule (tests/test_recon_filter_cpu.py), so that the probability and the logit form of the loss
    are one function there and share the reference."""
    from disenlink_amd import ops
    g = load_golden(name)
    N = g["meta"]["N"]
    nf = rf.make_rule(rf.MODULE_RULE, N, DEV)
    want, ref, ign, n, _sat = rf.module_reference(g, rf.allowed_matrix(nf), torch.float64)
    model = _module(g)
    graph = model._graph_of(torch.from_numpy(g["adj"]).to(DEV))
    fwd = model.forward_recon_logits_loss if logits else model.forward_recon_loss
    node = ops.ReconLogitsLoss if logits else ops.ReconLoss
    emb, loss = fwd(torch.from_numpy(g["x"]).to(DEV), graph, ignore=ign.to(DEV), node_filter=nf)
    model.zero_grad()
    loss.backward()
    ops.check_recon_counts(node.last_counts, ops.recon_sets(graph, ign.to(DEV), N, DEV, node_filter=nf))
    assert node.last_counts.tolist() == list(n)
    np.testing.assert_allclose(emb.detach().cpu().numpy(), g["emb"], rtol=1e-5, atol=1e-5)
    assert abs(loss.item() - want) <= 2e-5 * max(1.0, abs(want))
    for k, p in model.named_parameters():
        scale = max(float(ref[k].abs().max()), 1e-6)
        err = float((p.grad.detach().cpu().double() - ref[k]).abs().max())
        print(f"{name} recon{'-logit' if logits else ''} under {rf.MODULE_RULE} {k}: error / scale {err / scale:.2e}")
        assert err <= recon_ref.MODULE_TOL * scale, (k, err, scale)


@pytest.mark.parametrize("logits", [False, True])
def test_hot_path_node_of_a_bf16_module_gives_the_loss_bits_of_the_call_on_the_same_sets(logits):
    from disenlink_amd import ops
    g = load_golden("k8_d64")
    N = g["meta"]["N"]
    _p, ign = recon_ref.pair_sets(N, seed=N)
    model = _module(g, BF16)
    x = torch.from_numpy(g["x"]).to(DEV)
    graph = model._graph_of(torch.from_numpy(g["adj"]).to(DEV))
    sets = ops.recon_sets(graph, ign.to(DEV), N, DEV, node_filter=rf.make_rule(rf.MODULE_RULE, N, DEV))
    plain = ops.recon_sets(graph, ign.to(DEV), N, DEV)
    fwd = model.forward_recon_logits_loss if logits else model.forward_recon_loss
    node = ops.ReconLogitsLoss if logits else ops.ReconLoss
    emb, loss = fwd(x, graph, ignore=sets)
    loss.backward()
    ops.check_recon_counts(node.last_counts, sets)
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters()) and any(bool(p.grad.any()) for p in model.parameters())
    beta, t = float(model.beta), float(model.temperature)
    Zt, _p2, _a, _s, H = ops.step_tables(graph, model.project(x).detach(), beta, t, BF16)
    loss2, _dZ, _dH, counts = _loss_fn(logits)(Zt, H, t, sets, table_dtype=BF16)
    assert torch.equal(loss.detach().reshape(1).view(torch.int32), loss2.to(torch.float32).reshape(1).view(torch.int32))
    ops.check_recon_counts(counts, sets)
    assert fwd(x, graph, ignore=plain)[1].item() != loss.item()          # the tripwire: the rule is read from the sets


@pytest.mark.parametrize("objective,epochs", [("recon", 3), ("recon-logit", 2)])
def test_the_training_loop_under_a_rule(objective, epochs):
    """Three Adam steps under a rule lower the loss; every epoch's check_recon_counts (device counts against the filtered host
    counts) passes, or the loop would raise."""
    from disenlink_amd import ops
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    sg = synthetic_graph("chameleon", seed=3, scale=300 / 2277)
    N = sg.n_nodes
    assert 280 <= N <= 320
    run = prepare_run(make_link_split(sg.src, sg.dst, N, m=2, seed=1), DEV, row_bytes=4 * 16 * 4)
    nf = ops.NodeFilter.between(torch.arange(N) % 2 == 0, torch.arange(N) % 2 == 1, device=DEV)      # users x items
    torch.manual_seed(0)
    model = Disentangle(32, 16, 16, nfactor=4, beta=0.7, t=1).to(DEV)
    x = torch.from_numpy(sg.features()[:, :32].copy()).to(DEV)
    res = run_link_prediction(model, x, run, epochs=epochs, lr=5e-3, objective=objective, recon_block_rows=128, recon_node_filter=nf)
    print(f"{objective} under a rule, N={N}: losses {res.losses} val AUCs {res.val_aucs} test AUC {res.test_auc}")
    assert res.epochs_run == epochs and all(np.isfinite(res.losses))
    if epochs == 3:
        assert res.losses[2] < res.losses[0]
    counts = (ops.ReconLogitsLoss if objective == "recon-logit" else ops.ReconLoss).last_counts.tolist()
    assert 0 < counts[0] and sum(counts) < (N // 2) * (N - N // 2) + 1      # only user-item pairs were charged
    with pytest.raises(ValueError, match="recon_node_filter"):
        run_link_prediction(model, x, run, epochs=1, objective="pairs", recon_node_filter=nf)


def test_launches_follow_the_current_stream():
    from disenlink_amd import ops
    N, K, d = 300, 8, 64
    Z, H, pos, ign = _inputs(N, K, d)
    Z, H = Z.to(DEV), H.to(DEV)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV, node_filter=rf.make_rule("between", N, DEV))
    want = ops.score_recon_loss(Z, H, 1.0, sets, block_rows=256)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device=DEV)
    with torch.cuda.stream(side):
        for _ in range(8):
            big = big @ big * 1e-2                            # work ahead of the inputs on the side stream
        Zs, Hs = Z * 1.0, H * 1.0                             # produced on the side stream, consumed by our kernels
        got = ops.score_recon_loss(Zs, Hs, 1.0, sets, block_rows=256)
    side.synchronize()
    assert _same(want, got)


def test_the_call_does_not_synchronise():
    """test_gpu_recon's check on the filtered entry: with prepared sets that carry a rule, loss and gradients come without a
    device synchronisation (sync debug mode "error"); where the build does not honour that mode the call is captured in ONE
    graph — a host read cannot be captured — and a replay must reproduce the eager bits."""
    from disenlink_amd import ops
    N, K, d = 300, 8, 64
    Z, H, pos, ign = _inputs(N, K, d)
    Z, H = Z.to(DEV), H.to(DEV)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV, node_filter=rf.make_rule("between", N, DEV))
    Zg, Hg = Z.clone().requires_grad_(True), H.clone().requires_grad_(True)

    def step():
        loss = ops.ReconLoss.apply(Zg, Hg, 1.0, sets, None, 128)
        return (loss,) + torch.autograd.grad(2.0 * loss, (Zg, Hg))

    eager = [v.clone() for v in step()]                       # sizes the workspace
    torch.cuda.synchronize()
    if _sync_debug_mode_is_honoured():
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            step()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            again = step()
        graph.replay()
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    ref = ops.score_recon_loss(Z, H, 1.0, sets)
    assert torch.equal(eager[1], 2.0 * ref[1]) and torch.equal(eager[2], 2.0 * ref[2])
    assert not _same(ref, ops.score_recon_loss(Z, H, 1.0, pos.to(DEV), ign.to(DEV)))      # the rule was in force


# ------------------------------------------------------------------------------------------------------ 5. C-level refusals
@pytest.mark.parametrize("entry", ["dl_score_recon_filtered", "dl_score_recon_logits_filtered"])
def test_a_bad_filter_is_refused_and_nothing_is_launched(entry):
    from disenlink_amd import _lib
    lib = _lib.load()
    N, K, d = 37, 2, 8
    Z, H, pos, _ign = _inputs(N, 1, 8)
    Z, H = Z.repeat(1, K, 1).contiguous().to(DEV), H.repeat(1, K, 1).contiguous().to(DEV)
    from disenlink_amd import ops
    sets = ops.recon_sets(pos.to(DEV), None, N, DEV)
    group = torch.zeros(N, dtype=torch.uint8, device=DEV)
    allow = torch.full((64,), -1, dtype=torch.int64, device=DEV)
    loss = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((2,), 7, dtype=torch.int64, device=DEV)
    dZ, dH = torch.full_like(Z, 7.0), torch.full_like(H, 7.0)
    ws = torch.zeros(int(lib.dl_score_recon_workspace_bytes_dtype(N, K, d, _lib.DL_F32, 0)), dtype=torch.uint8, device=DEV)

    def call(nf):
        return getattr(lib, entry)(Z.data_ptr(), H.data_ptr(), N, K, d, _lib.DL_F32, 1.0, sets.pos_rowptr.data_ptr(),
                                   sets.pos_col.data_ptr(), None, None, 0.5, 0.5, 0, loss.data_ptr(), counts.data_ptr(),
                                   dZ.data_ptr(), dH.data_ptr(), ws.data_ptr(), ws.numel(), None, nf)
    for n_groups in (0, 65, -3):
        assert call(C.byref(_lib.DlNodeFilter(group.data_ptr(), n_groups, allow.data_ptr()))) == -1
        assert f"node filter: n_groups={n_groups} outside 1..64".encode() in lib.dl_last_error()
    assert call(C.byref(_lib.DlNodeFilter(None, 1, allow.data_ptr()))) == -1 and b"node filter: NULL" in lib.dl_last_error()
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and counts.tolist() == [7, 7] and bool((dZ == 7.0).all()) and bool((dH == 7.0).all())
    assert call(C.byref(_lib.DlNodeFilter(group.data_ptr(), 64, allow.data_ptr()))) == 0       # 64 groups, every bit set: served
    torch.cuda.synchronize()
    assert counts.tolist() == [sets.n_pos, sets.n_neg] and bool(torch.isfinite(dZ).all()) and float(loss) != 7.0
    assert call(None) == 0                                                                      # NULL: the unfiltered call
    torch.cuda.synchronize()
    assert counts.tolist() == [sets.n_pos, sets.n_neg]
