"""The whole-graph reconstruction loss in LOGIT space (ops.score_recon_logits_loss, ops.ReconLogitsLoss, ops.HotPathReconLogits,
Disentangle.forward_recon_logits_loss, run_link_prediction(objective="recon-logit")) against its fp64 restatement
(tests/recon_logits_ref.py) — on tables that stay inside the fp32 sigmoid's range and on tables that saturate it, where the
probability form clamps —, itself bit for bit across strip heights, slice counts and table types."""
import copy
import functools
import itertools

import numpy as np
import pytest
import torch

import recon_logits_ref as rl
import recon_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
GRID_KD = ((1, 8), (3, 100), (8, 64), (4, 128))


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from disenlink_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()


@functools.lru_cache(maxsize=None)
def case(N, K, d, t, saturated=False):
    """(Z, H, pos, ign, fp64 reference) of one grid point, computed once and shared (read only)."""
    if saturated:
        Z, H, pos, ign = rl.saturated_tables(N, K, d, t)
    else:
        Z, H = recon_ref.tables_cpu(N, K, d, recon_ref.table_seed(N, K, d))
        pos, ign = recon_ref.pair_sets(N, seed=N)
    return Z, H, pos, ign, rl.recon_logits64(Z, H, t, pos, ign)


def check(tag, out, ref):
    """loss, dZ, dH, counts of ``ops.score_recon_logits_loss`` against ``recon_logits64``: worst error / band <= 1."""
    loss, dZ, dH, counts = out
    assert loss.dtype == torch.float64 and dZ.dtype == torch.float32 and dZ.shape == ref["dZ"].shape and dH.shape == ref["dH"].shape
    assert tuple(counts.tolist()) == ref["counts"], (tag, counts.tolist(), ref["counts"])
    assert bool(torch.isfinite(dZ).all()) and bool(torch.isfinite(dH).all()) and bool(torch.isfinite(loss))
    err = abs(float(loss) - ref["loss"])
    wL = 0.0 if err == 0 else err / ref["band_loss"] if ref["band_loss"] > 0 else float("inf")
    wZ, wH = recon_ref.worst(dZ, ref["dZ"], ref["band_dZ"]), recon_ref.worst(dH, ref["dH"], ref["band_dH"])
    print(f"recon-logit {tag}: loss {float(loss):.9g} (fp64 {ref['loss']:.9g})  worst error / band  loss {wL:.4f}  dZ {wZ:.4f}  dH {wH:.4f}")
    assert wL <= 1.0 and wZ <= 1.0 and wH <= 1.0, (tag, wL, wZ, wH)


def run(Z, H, t, pos, ign=None, **kw):
    from disenlink_amd import ops
    return ops.score_recon_logits_loss(Z.to(DEV), H.to(DEV), t, pos.to(DEV), None if ign is None else ign.to(DEV), **kw)


# ------------------------------------------------------------------------------------------------------ 1. the fp64 grid
@pytest.mark.parametrize("N,Kd,t", list(itertools.product((1, 2, 37, 128, 129, 300), GRID_KD, (1.0, 2.0))))
def test_loss_gradients_and_counts_match_fp64(N, Kd, t):
    K, d = Kd
    Z, H, pos, ign, ref = case(N, K, d, t)
    check(f"N={N} K={K} d={d} t={t}", run(Z, H, t, pos, ign), ref)


# -------------------------------------------------------------------------------------------------- 2. the saturated grid
@pytest.mark.parametrize("N,Kd,t", list(itertools.product((129, 300), GRID_KD, (1.0, 2.0))))
def test_saturated_logits_keep_their_loss_and_their_gradient(N, Kd, t):
    """H rescaled so that the largest included |logit| is 60: past 16.64 an fp32 sigmoid is exactly 1 and below -27.6 the
    probability form's clamp factor acts.  The logit entry stays inside the fp64 bands; the probability entry, on the same
    inputs, is more than 100 bands away, so the comparison cannot pass by calling it.  (Measured on the CPU in fp64: the fp64
    logit loss is 10.20 against 17.40 for the fp32-probability form at N = 300, (8, 64), band 2e-3.)"""
    from disenlink_amd import ops
    K, d = Kd
    Z, H, pos, ign, ref = case(N, K, d, t, True)
    share, low = rl.saturation(ref)
    assert share >= rl.MIN_SHARE_ABOVE and low >= rl.min_positives_below(N, K, d), (share, low)
    check(f"saturated N={N} K={K} d={d} t={t} ({100 * share:.1f} % above 16.64, {low} positives below -27.6)", run(Z, H, t, pos, ign), ref)
    prob = ops.score_recon_loss(Z.to(DEV), H.to(DEV), t, pos.to(DEV), ign.to(DEV))
    away = abs(float(prob[0]) - ref["loss"]) / ref["band_loss"]
    print(f"  the probability entry: loss {float(prob[0]):.6g}, {away:.0f} bands away")
    assert away > 100


# ---------------------------------------------------------------------------------------------- 3. one pair in closed form
@pytest.mark.parametrize("positive", [False, True])
def test_one_pair_at_logit_40(positive):
    """N = 2, K = 1, d = 8, Z = 0 (every exp is 1): x = h_0 . h_1 = +40 on a negative, -40 on a positive, w = 1.  The loss is
    40 w and the gradient w sigma(+-40) ~ +-w.  The probability entry: at +40 on a negative p is exactly 1, the loss exactly
    100 w and the gradient exactly 0; at -40 on a positive its clamp factor p (1 - p) 1e12 = 4.25e-6 is left of the gradient."""
    from disenlink_amd import ops
    Z, H = torch.zeros(2, 1, 8), torch.zeros(2, 1, 8)
    H[0, 0, 0], H[1, 0, 0] = 8.0, -5.0 if positive else 5.0
    pos = torch.tensor([[False, positive], [positive, False]])
    ref = rl.recon_logits64(Z, H, 1.0, pos, pos_weight=1.0)
    assert ref["w"] == (1.0, 1.0) and abs(ref["loss"] - 40.0) < 1e-12 and abs(abs(float(ref["dH"][0, 0, 0])) - 5.0) < 1e-12
    out = run(Z, H, 1.0, pos, pos_weight=1.0)
    check(f"one pair, positive={positive}", out, ref)
    assert abs(float(out[0]) - 40.0) <= ref["band_loss"] and abs(float(out[2][0, 0, 0])) > 4.9 and abs(float(out[2][1, 0, 0])) > 7.9
    loss, dZ, dH, counts = ops.score_recon_loss(Z.to(DEV), H.to(DEV), 1.0, pos.to(DEV), pos_weight=1.0)
    assert counts.tolist() == list(ref["counts"])
    if not positive:
        assert float(loss) == 100.0 and not bool(dZ.any()) and not bool(dH.any())
    else:
        assert float(dH.abs().max()) <= 1e-5 * float(out[2].abs().max())


# ------------------------------------------------------------------------------------------------------------- 4. bits
def _bits(out):
    loss, dZ, dH, counts = out
    return [loss.reshape(1).view(torch.int64).cpu(), dZ.view(torch.int32).cpu(), dH.view(torch.int32).cpu(), counts.cpu()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


@pytest.mark.parametrize("K,d", [(8, 64), (3, 100)])
def test_bits_do_not_depend_on_the_strip_height_the_slice_count_or_the_call(K, d, lib_env):
    from disenlink_amd import _lib, ops
    assert ops._POISON, "the tests run with DL_POISON=1 (conftest.py)"
    N = 300
    Z, H, pos, ign, _ref = case(N, K, d, 1.0, True)
    Z, H = Z.to(DEV), H.to(DEV)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV)
    whole = ops.score_recon_logits_loss(Z, H, 1.0, sets)
    assert bool(torch.isfinite(whole[1]).all()) and bool(torch.isfinite(whole[2]).all()) and bool(torch.isfinite(whole[0]))
    assert _same(whole, ops.score_recon_logits_loss(Z, H, 1.0, sets))                    # two calls
    assert _lib.score_recon_form(N, K, d, 0)["strips"] == 1 and _lib.score_recon_form(N, K, d, 128)["strips"] == 3
    assert _same(whole, ops.score_recon_logits_loss(Z, H, 1.0, sets, block_rows=128))
    for forced in (1, 2):                                                                # the scan's slice count
        lib_env("DL_RANK_SLICES", forced)
        assert _same(whole, ops.score_recon_logits_loss(Z, H, 1.0, sets, block_rows=128)), forced
        lib_env("DL_RANK_SLICES")


@pytest.mark.parametrize("N,Kd", list(itertools.product((129, 300), ((8, 64), (3, 100)))))
def test_bf16_tables_give_the_bits_of_the_fp32_entry_on_the_rounded_tables(N, Kd):
    from disenlink_amd import ops
    K, d = Kd
    Z, H, pos, ign, _ref = case(N, K, d, 1.0, True)
    Zb, Hb = Z.to(BF16), H.to(BF16)
    got = ops.score_recon_logits_loss(Zb.to(DEV), Hb.to(DEV), 1.0, pos.to(DEV), ign.to(DEV), table_dtype=BF16)
    want = ops.score_recon_logits_loss(Zb.float().to(DEV), Hb.float().to(DEV), 1.0, pos.to(DEV), ign.to(DEV))
    assert got[1].dtype == torch.float32 and bool(torch.isfinite(got[1]).all()) and bool(got[1].any())
    assert _same(got, want)
    check(f"bf16 tables N={N} K={K} d={d}", got, rl.recon_logits64(Zb.float(), Hb.float(), 1.0, pos, ign))


# --------------------------------------------------------------------------------------------- 5. edges and behaviour
def test_empty_positive_set_everything_ignored_and_explicit_pos_weight():
    N, K, d = 300, 3, 40
    Z, H = recon_ref.tables_cpu(N, K, d, 1)
    pos, ign = recon_ref.pair_sets(N, seed=4)
    none = torch.zeros(N, N, dtype=torch.bool)
    check("no positives", run(Z, H, 1.0, none, ign), rl.recon_logits64(Z, H, 1.0, none, ign))
    check("no positives, nothing ignored", run(Z, H, 1.0, none), rl.recon_logits64(Z, H, 1.0, none))
    for pw in (1.0, 7.25):
        check(f"pos_weight={pw}", run(Z, H, 2.0, pos, ign, pos_weight=pw), rl.recon_logits64(Z, H, 2.0, pos, ign, pw))
    for n in (129, 300):
        loss, dZ, dH, counts = run(Z[:n], H[:n], 1.0, pos[:n, :n], torch.ones(n, n, dtype=torch.bool), block_rows=128)
        assert float(loss) == 0.0 and counts.tolist() == [0, 0]
        assert not bool(dZ.any()) and not bool(dH.any())


def test_a_row_whose_positives_fill_a_whole_tile():
    N, K, d = 300, 3, 40
    Z, H = recon_ref.tables_cpu(N, K, d, 4)
    pos, ign = recon_ref.pair_sets(N, seed=7)
    pos[5, 128:256] = True                                                # the second candidate tile of row 5, all of it
    pos[128:256, 5] = True
    ign[5, :] = ign[:, 5] = False
    check("full tile", run(Z, H, 1.0, pos, ign), rl.recon_logits64(Z, H, 1.0, pos, ign))


def test_launches_follow_the_current_stream():
    from disenlink_amd import ops
    N, K, d = 300, 8, 64
    Z, H, pos, ign, _ref = case(N, K, d, 1.0, True)
    Z, H = Z.to(DEV), H.to(DEV)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV)
    want = ops.score_recon_logits_loss(Z, H, 1.0, sets, block_rows=128)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device=DEV)
    with torch.cuda.stream(side):
        for _ in range(8):
            big = big @ big * 1e-2                            # work ahead of the inputs on the side stream
        Zs, Hs = Z * 1.0, H * 1.0                             # produced on the side stream, consumed by our kernels
        got = ops.score_recon_logits_loss(Zs, Hs, 1.0, sets, block_rows=128)
    side.synchronize()
    assert _same(want, got)


def _sync_debug_mode_is_honoured():
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_the_call_does_not_synchronise():
    """test_gpu_recon's method: sync debug mode "error", or, where the build does not honour it, one captured graph."""
    from disenlink_amd import ops
    N, K, d = 300, 8, 64
    Z, H, pos, ign, _ref = case(N, K, d, 1.0, True)
    Z, H = Z.to(DEV), H.to(DEV)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV)
    Zg, Hg = Z.clone().requires_grad_(True), H.clone().requires_grad_(True)

    def step():
        loss = ops.ReconLogitsLoss.apply(Zg, Hg, 1.0, sets, None, 128)
        return (loss,) + torch.autograd.grad(2.0 * loss, (Zg, Hg))

    before = ops.ReconLoss.last_counts
    eager = [v.clone() for v in step()]                       # sizes the workspace
    assert ops.ReconLogitsLoss.last_counts is not None and ops.ReconLoss.last_counts is before      # counts of its own
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
    ref = ops.score_recon_logits_loss(Z, H, 1.0, sets)
    assert torch.equal(eager[1], 2.0 * ref[1]) and torch.equal(eager[2], 2.0 * ref[2])      # the backward scales by the incoming scalar


def test_unsupported_inputs_raise_before_any_launch():
    from disenlink_amd import _lib, ops
    N = 40
    pos, _ign = recon_ref.pair_sets(N, seed=1)
    sets = ops.recon_sets(pos.to(DEV), None, N, DEV)
    Z = torch.randn(N, 2, 16, device=DEV)
    for f in (lambda a: ops.ReconLogitsLoss.apply(a, a, 1.0, sets), lambda a: ops.score_recon_logits_loss(a, a, 1.0, sets)):
        with pytest.raises(TypeError, match="fp32"):
            f(Z.bfloat16())
        with pytest.raises(_lib.DisenlinkHipError, match="d <= 128"):
            f(torch.randn(N, 2, 129, device=DEV))
        with pytest.raises(_lib.DisenlinkHipError, match="no CPU fallback"):
            f(Z.cpu())
    with pytest.raises(TypeError, match="both bf16 or both fp32"):
        ops.score_recon_logits_loss(Z.bfloat16(), Z, 1.0, sets, table_dtype=BF16)
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.score_recon_logits_loss(Z, Z, 1.0, sets, block_rows=100)


def test_an_overflowed_exp_gives_a_non_finite_loss():
    """Logit space cures the saturation of the sigmoid, not the overflow of exp: z_0 . z_1 / t = 100 > 89 makes the logit of
    the pair (0, 1) infinite in fp32; the loss is then non-finite, never a silent zero, and so are gradients."""
    N, K, d = 37, 3, 8
    Z, H, pos, ign, _ref = case(N, K, d, 1.0)
    Z, H, pos, ign = Z.clone(), H.clone(), pos.clone(), ign.clone()
    Z[0, 1], Z[1, 1], H[0, 1], H[1, 1] = 0.0, 0.0, 0.0, 0.0
    Z[0, 1, 0] = Z[1, 1, 0] = 10.0
    H[0, 1, 0] = H[1, 1, 0] = 1.0
    ign[0, 1] = ign[1, 0] = False
    for positive in (False, True):                            # +inf on a negative: an infinite cost; on a positive: no cost, NaN gradients
        pos[0, 1] = pos[1, 0] = positive
        loss, dZ, dH, counts = run(Z, H, 1.0, pos, ign)
        assert counts.tolist() == list(rl.recon_logits64(Z, H, 1.0, pos, ign)["counts"])
        assert not bool(torch.isfinite(dZ).all()) and not bool(torch.isfinite(dH).all())
        if not positive:
            assert not bool(torch.isfinite(loss))


# ------------------------------------------------------------------------------------------------------------ 6. module
def _sd(g):
    return {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}


def _module(g, table_dtype=torch.float32):
    from disenlink_amd.model import Disentangle
    m = g["meta"]
    model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"], table_dtype=table_dtype)
    model.load_state_dict(_sd(g))
    return model.to(DEV)


@functools.lru_cache(maxsize=None)
def _admitted():
    from test_recon_logits_cpu import module_cases
    return tuple(module_cases())


def test_every_small_golden_case_is_admitted():
    assert _admitted() == recon_ref.SMALL_GOLDEN_CASES


@pytest.mark.parametrize("name", recon_ref.SMALL_GOLDEN_CASES)
def test_module_parameter_gradients_match_fp64_autograd_of_the_dense_formulation(name):
    """forward_recon_logits_loss(...).backward() against CPU fp64 autograd of the oracle's project -> route_aggregate ->
    logits under the masked, weighted BCE-with-logits; tolerance MODULE_TOL = 1e-4 x each gradient's scale, on every case the
    CPU test admits — all eight, k4_d8 (logits up to 1,759) and k8_d8_t2 (up to 1.8e7) included."""
    from disenlink_amd import ops
    assert name in _admitted()
    g = load_golden(name)
    N = g["meta"]["N"]
    want, ref, ign, n, big = rl.module_reference(g, torch.float64)
    model = _module(g)
    graph = model._graph_of(torch.from_numpy(g["adj"]).to(DEV))
    emb, loss = model.forward_recon_logits_loss(torch.from_numpy(g["x"]).to(DEV), graph, ignore=ign.to(DEV))
    model.zero_grad()
    loss.backward()
    ops.check_recon_counts(ops.ReconLogitsLoss.last_counts, ops.recon_sets(graph, ign.to(DEV), N, DEV))
    assert ops.ReconLogitsLoss.last_counts.tolist() == list(n)
    np.testing.assert_allclose(emb.detach().cpu().numpy(), g["emb"], rtol=1e-5, atol=1e-5)
    assert abs(loss.item() - want) <= 2e-5 * max(1.0, abs(want))
    worst = 0.0
    for k, p in model.named_parameters():
        scale = max(float(ref[k].abs().max()), 1e-6)
        err = float((p.grad.detach().cpu().double() - ref[k]).abs().max())
        worst = max(worst, err / scale)
        assert err <= recon_ref.MODULE_TOL * scale, (k, err, scale)
    print(f"{name} recon-logit: loss {loss.item():.7g} (fp64 {want:.7g}), largest included |logit| {big:.4g}, worst error / scale {worst:.2e}")


def test_three_adam_steps_of_the_recon_logit_objective_lower_the_loss_and_the_auc_is_counted_on_logits():
    from disenlink_amd import ops
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.metrics import auc_tie_avg
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    sg = synthetic_graph("chameleon", seed=3, scale=300 / 2277)
    assert 280 <= sg.n_nodes <= 320
    prepared = prepare_run(make_link_split(sg.src, sg.dst, sg.n_nodes, m=2, seed=1), DEV, row_bytes=4 * 16 * 4)
    torch.manual_seed(0)
    model = Disentangle(32, 16, 16, nfactor=4, beta=0.7, t=1).to(DEV)
    first = copy.deepcopy(model)
    x = torch.from_numpy(sg.features()[:, :32].copy()).to(DEV)
    ops.ReconLogitsLoss.last_counts = None
    res = run_link_prediction(model, x, prepared, epochs=3, lr=5e-3, objective="recon-logit", recon_block_rows=128)
    print(f"recon-logit objective, N={sg.n_nodes}: losses {res.losses} val AUCs {res.val_aucs} test AUC {res.test_auc}")
    assert res.epochs_run == 3 and all(np.isfinite(res.losses))
    assert res.losses[2] < res.losses[0]
    assert 0.0 <= res.test_auc <= 1.0 and res.best_val_auc == max(res.val_aucs)
    assert ops.ReconLogitsLoss.last_counts is not None        # the loop compared them with the host's every epoch (check_recon_counts)
    b = prepared.n_pos + prepared.n_neg
    with torch.no_grad():                                     # epoch 0 scores the weights before the first step
        _emb, logit = first.forward_pair_logits(x, prepared.graph, prepared.train_val_pairs)
    assert abs(res.val_aucs[0] - float(auc_tie_avg(prepared.label_val, logit[b:]))) <= 1e-12
    with pytest.raises(ValueError, match="eager loop only"):
        run_link_prediction(model, x, prepared, epochs=1, objective="recon-logit", use_graph=True)


def test_bf16_module_goes_through_the_single_node_on_its_own_rounded_tables():
    from disenlink_amd import ops
    g = load_golden("k8_d64")
    m = g["meta"]
    N, K, d = m["N"], m["K"], m["d"]
    _p, ign = recon_ref.pair_sets(N, seed=N)
    model = _module(g, BF16)
    x = torch.from_numpy(g["x"]).to(DEV)
    graph = model._graph_of(torch.from_numpy(g["adj"]).to(DEV))
    sets = ops.recon_sets(graph, ign.to(DEV), N, DEV)
    emb, loss = model.forward_recon_logits_loss(x, graph, ignore=sets)
    assert "HotPathReconLogits" in type(loss.grad_fn).__name__
    model.zero_grad()
    loss.backward()
    ops.check_recon_counts(ops.ReconLogitsLoss.last_counts, sets)
    grads = [p.grad for p in model.parameters()]
    assert all(bool(torch.isfinite(v).all()) for v in grads) and any(bool(v.any()) for v in grads)
    Zt, _p, _a, _s, H = ops.step_tables(graph, model.project(x).detach(), float(model.beta), float(model.temperature), BF16)
    assert Zt.dtype == BF16 and H.dtype == BF16
    assert torch.equal(emb.detach().view(N, K, d).view(torch.int32), H.float().view(torch.int32))
    loss2, _dZ, _dH, _counts = ops.score_recon_logits_loss(Zt, H, float(model.temperature), sets, table_dtype=BF16)
    assert torch.equal(loss.detach().reshape(1).view(torch.int32), loss2.to(torch.float32).reshape(1).view(torch.int32))
    _emb32, loss32 = _module(g).forward_recon_logits_loss(x, graph, ignore=sets)      # the tripwire: an fp32 module scores other tables
    assert loss32.item() != loss.item()
