"""The whole-graph reconstruction loss (ops.score_recon_loss, ops.ReconLoss, Disentangle.forward_recon_loss,
run_link_prediction(objective="recon")) against its fp64 restatement (tests/recon_ref.py), itself bit for bit across strip
heights and slice counts, and against the dense [N,N] path."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recon_ref
from conftest import ROOT, load_golden
from oracle import dense_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from disenlink_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()


def tables(N, K, d, seed):
    Z, H = recon_ref.tables_cpu(N, K, d, seed)                 # test_gpu_dense_bwd.tables: scale 0.5 / sqrt(d)
    return Z.to(DEV), H.to(DEV)


def check(tag, out, ref):
    """loss, dZ, dH, counts of ``ops.score_recon_loss`` against ``recon_ref.recon64``: worst error / band <= 1."""
    loss, dZ, dH, counts = out
    assert loss.dtype == torch.float64 and dZ.dtype == torch.float32 and dZ.shape == ref["dZ"].shape and dH.shape == ref["dH"].shape
    assert tuple(counts.tolist()) == ref["counts"], (tag, counts.tolist(), ref["counts"])
    assert bool(torch.isfinite(dZ).all()) and bool(torch.isfinite(dH).all()) and bool(torch.isfinite(loss))
    err = abs(float(loss) - ref["loss"])
    wL = 0.0 if err == 0 else err / ref["band_loss"] if ref["band_loss"] > 0 else float("inf")
    wZ, wH = recon_ref.worst(dZ, ref["dZ"], ref["band_dZ"]), recon_ref.worst(dH, ref["dH"], ref["band_dH"])
    print(f"recon {tag}: loss {float(loss):.9g} (fp64 {ref['loss']:.9g})  worst error / band  loss {wL:.4f}  dZ {wZ:.4f}  dH {wH:.4f}")
    assert wL <= 1.0 and wZ <= 1.0 and wH <= 1.0, (tag, wL, wZ, wH)


GRID = list(itertools.product((1, 2, 37, 128, 129, 300, 700), ((1, 8), (3, 100), (8, 64), (4, 128)), (1.0, 2.0)))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Kd,t", GRID)
def test_loss_gradients_and_counts_match_fp64(N, Kd, t):
    from disenlink_amd import ops
    K, d = Kd
    Z, H = tables(N, K, d, recon_ref.table_seed(N, K, d))
    pos, ign = recon_ref.pair_sets(N, seed=N)
    out = ops.score_recon_loss(Z, H, t, pos.to(DEV), ign.to(DEV))
    check(f"N={N} K={K} d={d} t={t}", out, recon_ref.recon64(Z, H, t, pos, ign))


# ---------------------------------------------------------------------------------------------------------------------
POISON = torch.tensor(-1, dtype=torch.int32)


def _bits(out):
    loss, dZ, dH, counts = out
    return [loss.reshape(1).view(torch.int64).cpu(), dZ.view(torch.int32).cpu(), dH.view(torch.int32).cpu(), counts.cpu()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


@pytest.mark.parametrize("N,K,d", [(700, 8, 64), (129, 3, 100)])
def test_bits_do_not_depend_on_the_strip_height_the_slice_count_or_the_call(N, K, d, lib_env):
    from disenlink_amd import _lib, ops
    assert ops._POISON, "the tests run with DL_POISON=1 (conftest.py)"
    Z, H = tables(N, K, d, seed=N)
    pos, ign = recon_ref.pair_sets(N, seed=N + 1)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV)
    whole = ops.score_recon_loss(Z, H, 1.0, sets)
    for x in _bits(whole)[1:3]:
        assert not bool((x == POISON).any())
    assert bool(torch.isfinite(whole[1]).all()) and bool(torch.isfinite(whole[2]).all()) and bool(torch.isfinite(whole[0]))
    assert _same(whole, ops.score_recon_loss(Z, H, 1.0, sets))                    # two calls
    assert _lib.score_recon_form(N, K, d, 0)["strips"] == 1
    for b in (128, 256):
        assert _lib.score_recon_form(N, K, d, b)["strips"] == -(-(-(-N // 128) * 128) // b)
        assert _same(whole, ops.score_recon_loss(Z, H, 1.0, sets, block_rows=b)), b
    for forced in (1, 2, 5):                                                      # the scan's slice count
        lib_env("DL_RANK_SLICES", forced)
        nt = -(-N // 128)
        tps = -(-nt // min(forced, nt))
        assert _lib.score_topk_form(N, K, d, 128, 1)["slices"] == -(-nt // tps)
        assert _same(whole, ops.score_recon_loss(Z, H, 1.0, sets, block_rows=128)), forced
        lib_env("DL_RANK_SLICES")


_CHILD = """
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import recon_ref
from disenlink_amd import _lib, ops
N, K, d = 700, 8, 64
assert _lib.score_topk_form(N, K, d, 768, 1)["slices"] == {slices}
Z, H = recon_ref.tables_cpu(N, K, d, N)
pos, ign = recon_ref.pair_sets(N, seed=N + 1)
out = ops.score_recon_loss(Z.cuda(), H.cuda(), 1.0, pos.cuda(), ign.cuda())
torch.save([x.cpu() for x in out], {path!r})
"""


def test_forced_slice_count_in_a_fresh_process_gives_the_same_bits(tmp_path):
    """DL_RANK_SLICES set before the library is loaded, in a child process of its own."""
    from disenlink_amd import ops
    N, K, d = 700, 8, 64
    Z, H = tables(N, K, d, seed=N)
    pos, ign = recon_ref.pair_sets(N, seed=N + 1)
    want = ops.score_recon_loss(Z, H, 1.0, pos.to(DEV), ign.to(DEV))
    path = str(tmp_path / "child.pt")
    env = dict(os.environ, DL_RANK_SLICES="3")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), slices=3, path=path)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = torch.load(path)
    assert _same(want, got)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,d,t", [(300, 8, 64, 1.0), (700, 8, 64, 1.0), (300, 3, 100, 2.0), (700, 3, 100, 2.0)])
def test_agrees_with_the_dense_path_on_the_same_included_pairs(N, K, d, t):
    """score_allpairs_fwd + torch's weighted BCE over the upper triangle + score_allpairs_bwd_dense: within the sum of the
    two paths' bands (the dense backward's: test_gpu_dense_bwd.bwd64 on its own prob and gradient; torch's fp32 loss sum:
    1e-5 x the sum of its addends)."""
    from disenlink_amd import ops
    from test_gpu_dense_bwd import bwd64
    Z, H = tables(N, K, d, seed=3 * N + d)
    pos, ign = recon_ref.pair_sets(N, seed=N + 2)
    ref = recon_ref.recon64(Z, H, t, pos, ign)
    loss, dZ, dH, _counts = ops.score_recon_loss(Z, H, t, pos.to(DEV), ign.to(DEV))
    inc = torch.triu(~ign, diagonal=1)
    w_pos, w_neg = ref["w"]
    y = (pos & inc).float().to(DEV)
    weight = (torch.where(pos, w_pos, w_neg) * inc).float().to(DEV)
    prob = ops.score_allpairs_fwd(Z, H, t).requires_grad_(True)
    dense_loss = F.binary_cross_entropy(prob, y, weight=weight, reduction="sum")
    (g,) = torch.autograd.grad(dense_loss, prob)
    eZ, eH = ops.score_allpairs_bwd_dense(Z, H, t, prob.detach(), g)
    _rZ, _rH, bZ, bH = bwd64(Z, H, t, prob.detach(), g)
    wZ = recon_ref.worst(dZ.double().cpu() - eZ.double().cpu(), torch.zeros_like(ref["dZ"]), ref["band_dZ"] + bZ.cpu())
    wH = recon_ref.worst(dH.double().cpu() - eH.double().cpu(), torch.zeros_like(ref["dH"]), ref["band_dH"] + bH.cpu())
    wL = abs(float(loss) - float(dense_loss)) / (ref["band_loss"] + 1e-5 * ref["loss"])
    print(f"recon vs dense N={N} K={K} d={d} t={t}: worst difference / (sum of the two bands)  loss {wL:.4f}  dZ {wZ:.4f}  dH {wH:.4f}")
    assert wL <= 1.0 and wZ <= 1.0 and wH <= 1.0, (wL, wZ, wH)


# ---------------------------------------------------------------------------------------------------------------------
def test_empty_positive_set():
    from disenlink_amd import ops
    N, K, d = 300, 3, 40
    Z, H = tables(N, K, d, seed=1)
    _pos, ign = recon_ref.pair_sets(N, seed=4)
    none = torch.zeros(N, N, dtype=torch.bool)
    check("no positives", ops.score_recon_loss(Z, H, 1.0, none.to(DEV), ign.to(DEV)), recon_ref.recon64(Z, H, 1.0, none, ign))
    check("no positives, nothing ignored", ops.score_recon_loss(Z, H, 1.0, none.to(DEV)), recon_ref.recon64(Z, H, 1.0, none))


@pytest.mark.parametrize("N", [129, 300])
def test_everything_ignored(N):
    from disenlink_amd import ops
    Z, H = tables(N, 3, 40, seed=2)
    pos, _ign = recon_ref.pair_sets(N, seed=5)
    loss, dZ, dH, counts = ops.score_recon_loss(Z, H, 1.0, pos.to(DEV), torch.ones(N, N, dtype=torch.bool, device=DEV), block_rows=128)
    assert float(loss) == 0.0 and counts.tolist() == [0, 0]
    assert not bool(dZ.any()) and not bool(dH.any())


def test_explicit_pos_weight():
    from disenlink_amd import ops
    N, K, d = 300, 8, 64
    Z, H = tables(N, K, d, seed=3)
    pos, ign = recon_ref.pair_sets(N, seed=6)
    for pw in (1.0, 7.25):
        check(f"pos_weight={pw}", ops.score_recon_loss(Z, H, 2.0, pos.to(DEV), ign.to(DEV), pos_weight=pw),
              recon_ref.recon64(Z, H, 2.0, pos, ign, pw))


def test_a_row_whose_positives_fill_a_whole_tile_and_a_positive_in_the_last_column():
    from disenlink_amd import ops
    N, K, d = 300, 3, 40
    Z, H = tables(N, K, d, seed=4)
    pos, ign = recon_ref.pair_sets(N, seed=7)
    pos[5, 128:256] = True                                                # the second candidate tile of row 5, all of it
    pos[128:256, 5] = True
    ign[5, :] = ign[:, 5] = False
    check("full tile", ops.score_recon_loss(Z, H, 1.0, pos.to(DEV), ign.to(DEV)), recon_ref.recon64(Z, H, 1.0, pos, ign))
    N = 129                                                              # column N - 1: the only column of the last tile
    Z, H = tables(N, K, d, seed=5)
    pos = torch.zeros(N, N, dtype=torch.bool)
    pos[3, 128] = pos[128, 3] = pos[127, 128] = pos[128, 127] = True
    for b in (None, 128):
        check(f"column N - 1, block_rows={b}", ops.score_recon_loss(Z, H, 1.0, pos.to(DEV), block_rows=b),
              recon_ref.recon64(Z, H, 1.0, pos))


# ---------------------------------------------------------------------------------------------------------------------
def _sd(g):
    return {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}


@pytest.mark.parametrize("name", recon_ref.MODULE_CASES)
def test_module_parameter_gradients_match_fp64_autograd_of_the_dense_formulation(name):
    """forward_recon_loss(...).backward() against CPU fp64 autograd of the oracle's dense forward under the masked, weighted
    BCE over the upper triangle; tolerance 1e-4 x scale, test_gpu_dense_bwd's for its whole-matrix losses.  The cases are the
    small golden cases on which fp32 is faithful to fp64 (recon_ref.MODULE_CASES has the rule and every case's figures);
    the saturated ones are the next test's."""
    loss, grads, counts, g = _module_step(name)
    want, ref, _ign, n, _sat = recon_ref.module_reference(g, torch.float64)
    assert counts == list(n)
    assert abs(loss - want) <= 2e-5 * max(1.0, abs(want))
    for k, got in grads.items():
        scale = max(float(ref[k].abs().max()), 1e-6)
        err = float((got.double() - ref[k]).abs().max())
        print(f"{name} recon {k}: error / scale {err / scale:.2e}")
        assert err <= recon_ref.MODULE_TOL * scale, (k, err, scale)


def _module_step(name):
    from disenlink_amd import ops
    from disenlink_amd.model import Disentangle
    g = load_golden(name)
    m = g["meta"]
    N = m["N"]
    _p, ign = recon_ref.pair_sets(N, seed=N)
    model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"])
    model.load_state_dict(_sd(g))
    model = model.to(DEV)
    graph = model._graph_of(torch.from_numpy(g["adj"]).to(DEV))
    emb, loss = model.forward_recon_loss(torch.from_numpy(g["x"]).to(DEV), graph, ignore=ign.to(DEV))
    model.zero_grad()
    loss.backward()
    ops.check_recon_counts(ops.ReconLoss.last_counts, ops.recon_sets(graph, ign.to(DEV), N, DEV))
    np.testing.assert_allclose(emb.detach().cpu().numpy(), g["emb"], rtol=1e-5, atol=1e-5)
    return loss.item(), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}, ops.ReconLoss.last_counts.tolist(), g


@pytest.mark.parametrize("name", [n for n in recon_ref.SMALL_GOLDEN_CASES if n not in recon_ref.MODULE_CASES])
def test_module_on_saturated_fixtures_runs_counts_and_stays_finite(name):
    """The fixtures whose logits saturate the fp32 sigmoid (no fp32 evaluation follows fp64 there: recon_ref.MODULE_CASES):
    the step runs, sees exactly the host's pairs and gives finite gradients; a loss term is at most 100 w."""
    loss, grads, counts, g = _module_step(name)
    _want, _ref, _ign, n, _sat = recon_ref.module_reference(g, torch.float32)
    assert counts == list(n)
    assert np.isfinite(loss) and 0.0 <= loss <= 100.0 * (2.0 * n[1]) / (n[0] + n[1])      # every term clamped: 100 (pos_weight n_pos + n_neg) / C
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())


def test_saturated_pairs_clamp_the_loss_and_contribute_exactly_zero_gradient():
    """Tables with Z = 0 (every exp is 1) and H along one axis: s(u, v) = K c_u c_v, with c = +-sqrt(25 / 8) on a third of the
    nodes (|s| = 25 among them: the fp32 sigmoid is exactly 1 at +25 where fp64 still holds 1 - 1.4e-11, and 1.4e-11 at -25)
    and |c| <= 0.2 elsewhere (|s| < 3).  Against the fp64 restatement with p rounded to fp32: a saturated negative adds 100 w
    to the loss, not 25 w, and exactly nothing to G^."""
    from disenlink_amd import ops
    N, K, d = 200, 8, 16
    gen = torch.Generator().manual_seed(12)
    c = torch.where(torch.rand(N, generator=gen) < 0.33, torch.tensor((25.0 / 8.0) ** 0.5), 0.2 * torch.rand(N, generator=gen))
    c = c * torch.where(torch.rand(N, generator=gen) < 0.5, -1.0, 1.0)
    H = torch.zeros(N, K, d)
    H[:, :, 0] = c[:, None]
    Z = torch.zeros(N, K, d)
    pos, ign = recon_ref.pair_sets(N, seed=13)
    ref = recon_ref.recon64(Z, H, 1.0, pos, ign, fp32_p=True)
    s, inc = ref["logit"], ref["included"]
    assert int((inc & (s > 20)).sum()) > 1000 and int((inc & (s < -20)).sum()) > 1000 and not bool((inc & (s.abs() > 5) & (s.abs() < 20)).any())
    assert ref["loss"] > recon_ref.recon64(Z, H, 1.0, pos, ign)["loss"] + 1.0      # saturated negatives at 100 w each, not at 25 w
    check("saturated", ops.score_recon_loss(Z.to(DEV), H.to(DEV), 1.0, pos.to(DEV), ign.to(DEV), block_rows=128), ref)


def test_three_adam_steps_of_the_recon_objective_lower_the_loss():
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    sg = synthetic_graph("chameleon", seed=3, scale=300 / 2277)
    assert 280 <= sg.n_nodes <= 320
    run = prepare_run(make_link_split(sg.src, sg.dst, sg.n_nodes, m=2, seed=1), DEV, row_bytes=4 * 16 * 4)
    torch.manual_seed(0)
    model = Disentangle(32, 16, 16, nfactor=4, beta=0.7, t=1).to(DEV)
    x = torch.from_numpy(sg.features()[:, :32].copy()).to(DEV)
    res = run_link_prediction(model, x, run, epochs=3, lr=5e-3, objective="recon", recon_block_rows=128)
    print(f"recon objective, N={sg.n_nodes}: losses {res.losses} val AUCs {res.val_aucs} test AUC {res.test_auc}")
    assert res.epochs_run == 3 and all(np.isfinite(res.losses))
    assert res.losses[2] < res.losses[0]
    assert 0.0 <= res.test_auc <= 1.0 and res.best_val_auc == max(res.val_aucs)
    with pytest.raises(ValueError, match="eager loop only"):
        run_link_prediction(model, x, run, epochs=1, objective="recon", use_graph=True)


# ---------------------------------------------------------------------------------------------------------------------
def test_launches_follow_the_current_stream():
    from disenlink_amd import ops
    N, K, d = 700, 8, 64
    Z, H = tables(N, K, d, seed=4)
    pos, ign = recon_ref.pair_sets(N, seed=8)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV)
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
    """With prepared sets, loss and gradients come without a device synchronisation (sync debug mode "error"); where the
    build does not honour that mode the call is captured in ONE graph — a host read cannot be captured — and a replay must
    reproduce the eager bits."""
    from disenlink_amd import ops
    N, K, d = 300, 8, 64
    Z, H = tables(N, K, d, seed=6)
    pos, ign = recon_ref.pair_sets(N, seed=9)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV)
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
    assert torch.equal(eager[1], 2.0 * ref[1]) and torch.equal(eager[2], 2.0 * ref[2])      # the backward scales by the incoming scalar


def test_unsupported_inputs_raise_in_forward():
    from disenlink_amd import _lib, ops
    N = 40
    pos, _ign = recon_ref.pair_sets(N, seed=1)
    sets = ops.recon_sets(pos.to(DEV), None, N, DEV)
    Z = torch.randn(N, 2, 16, device=DEV)
    with pytest.raises(TypeError, match="fp32"):
        ops.ReconLoss.apply(Z.bfloat16(), Z.bfloat16(), 1.0, sets)
    with pytest.raises(TypeError, match="fp32"):
        ops.score_recon_loss(Z.bfloat16(), Z.bfloat16(), 1.0, sets)
    wide = torch.randn(N, 2, 129, device=DEV)
    with pytest.raises(_lib.DisenlinkHipError, match="d <= 128"):
        ops.ReconLoss.apply(wide, wide, 1.0, sets)
    with pytest.raises(_lib.DisenlinkHipError, match="d <= 128"):
        ops.score_recon_loss(wide, wide, 1.0, sets)
