"""The whole-graph reconstruction loss on bf16 tables (``table_dtype=torch.bfloat16``: dl_score_recon_dtype with DL_BF16, the
one-plane scan and dense backward): bit for bit the fp32 entry on the same tables widened to fp32, within the fp64 bands of
tests/recon_ref.py, the same bits across strip heights, slice counts and calls, and the step of a bf16 module
(ops.HotPathRecon, Disentangle.forward_recon_loss, run_link_prediction(objective="recon"), the CLI)."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recon_ref
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from disenlink_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()


def tables_bf16(N, K, d, seed):
    """recon_ref.tables_cpu rounded to bf16 (nearest-even) -> (Z, H fp32 as drawn, Zb, Hb bf16), on the CPU."""
    Z, H = recon_ref.tables_cpu(N, K, d, seed)
    return Z, H, Z.to(BF16), H.to(BF16)


def _bits(out):
    loss, dZ, dH, counts = out
    return [loss.reshape(1).view(torch.int64).cpu(), dZ.view(torch.int32).cpu(), dH.view(torch.int32).cpu(), counts.cpu()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _cpu(out):
    return tuple(x.cpu() for x in out)


def check(tag, out, ref):
    """test_gpu_recon.check: loss, dZ, dH, counts against ``recon_ref.recon64``, worst error / band <= 1."""
    loss, dZ, dH, counts = out
    assert loss.dtype == torch.float64 and dZ.dtype == torch.float32 and dZ.shape == ref["dZ"].shape and dH.shape == ref["dH"].shape
    assert tuple(counts.tolist()) == ref["counts"], (tag, counts.tolist(), ref["counts"])
    assert bool(torch.isfinite(dZ).all()) and bool(torch.isfinite(dH).all()) and bool(torch.isfinite(loss))
    err = abs(float(loss) - ref["loss"])
    wL = 0.0 if err == 0 else err / ref["band_loss"] if ref["band_loss"] > 0 else float("inf")
    wZ, wH = recon_ref.worst(dZ, ref["dZ"], ref["band_dZ"]), recon_ref.worst(dH, ref["dH"], ref["band_dH"])
    print(f"recon bf16 {tag}: loss {float(loss):.9g} (fp64 {ref['loss']:.9g})  worst error / band  loss {wL:.4f}  dZ {wZ:.4f}  dH {wH:.4f}")
    assert wL <= 1.0 and wZ <= 1.0 and wH <= 1.0, (tag, wL, wZ, wH)


# (K, d): every NCB = 1, 2, 3, 4 and d not a multiple of 32.  (1000, 64, 8): nt K = 512, the unsliced store path of the backward
# (nslice = 1), at the largest K; every other shape takes the sliced path.
GRID = list(itertools.product((1, 129, 300, 700), ((1, 8), (8, 64), (2, 70), (3, 100), (4, 128)), (1.0, 2.0)))
GRID += [(1000, (64, 8), 1.0), (1000, (64, 8), 2.0)]


@functools.lru_cache(maxsize=None)
def _case(N, K, d, t):
    """One grid case, computed once for the tests that share it (results on the CPU, never changed)."""
    from disenlink_amd import ops
    Z, H, Zb, Hb = tables_bf16(N, K, d, recon_ref.table_seed(N, K, d))
    pos, ign = recon_ref.pair_sets(N, seed=N)
    out = _cpu(ops.score_recon_loss(Zb.to(DEV), Hb.to(DEV), t, pos.to(DEV), ign.to(DEV), table_dtype=BF16))
    return Z, H, Zb, Hb, pos, ign, out


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Kd,t", GRID)
def test_bits_of_the_fp32_entry_on_the_rounded_tables(N, Kd, t):
    from disenlink_amd import _lib, ops
    K, d = Kd
    Z, H, Zb, Hb, pos, ign, out = _case(N, K, d, t)
    assert (_lib.score_recon_form(N, K, d, 0, _lib.DL_BF16)["nslice"] == 1) == (N == 1000 or N <= 128)
    want = ops.score_recon_loss(Zb.float().to(DEV), Hb.float().to(DEV), t, pos.to(DEV), ign.to(DEV))
    assert bool(torch.isfinite(want[1]).all()) and bool(torch.isfinite(want[2]).all()) and bool(torch.isfinite(want[0]))
    for name, a, b in zip(("loss", "dZ", "dH", "counts"), _bits(out), _bits(want)):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    # fp32 tensors under the keyword are rounded to nearest-even inside: the bits of the pre-rounded call
    assert _same(out, ops.score_recon_loss(Z.to(DEV), H.to(DEV), t, pos.to(DEV), ign.to(DEV), table_dtype=BF16))


@pytest.mark.parametrize("N,Kd,t", GRID)
def test_loss_gradients_and_counts_match_fp64_on_the_rounded_tables(N, Kd, t):
    K, d = Kd
    _Z, _H, Zb, Hb, pos, ign, out = _case(N, K, d, t)
    check(f"N={N} K={K} d={d} t={t}", out, recon_ref.recon64(Zb.float(), Hb.float(), t, pos, ign))


# ---------------------------------------------------------------------------------------------------------------------
POISON = torch.tensor(-1, dtype=torch.int32)


@pytest.mark.parametrize("N,K,d", [(700, 8, 64), (129, 3, 100)])
def test_bits_do_not_depend_on_the_strip_height_the_slice_count_or_the_call(N, K, d, lib_env):
    from disenlink_amd import _lib, ops
    assert ops._POISON, "the tests run with DL_POISON=1 (conftest.py)"
    _Z, _H, Zb, Hb = tables_bf16(N, K, d, seed=N)
    Zb, Hb = Zb.to(DEV), Hb.to(DEV)
    pos, ign = recon_ref.pair_sets(N, seed=N + 1)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV)

    def run(**kw):
        return ops.score_recon_loss(Zb, Hb, 1.0, sets, table_dtype=BF16, **kw)
    whole = run()
    for x in _bits(whole)[1:3]:
        assert not bool((x == POISON).any())
    assert bool(torch.isfinite(whole[1]).all()) and bool(torch.isfinite(whole[2]).all()) and bool(torch.isfinite(whole[0]))
    assert _same(whole, run())                                                    # two calls
    assert _lib.score_recon_form(N, K, d, 0, _lib.DL_BF16)["strips"] == 1
    for b in (128, 256):
        assert _lib.score_recon_form(N, K, d, b, _lib.DL_BF16)["strips"] == -(-(-(-N // 128) * 128) // b)
        assert _same(whole, run(block_rows=b)), b
    for forced in (1, 2, 5):                                                      # the scan's slice count
        lib_env("DL_RANK_SLICES", forced)
        nt = -(-N // 128)
        tps = -(-nt // min(forced, nt))
        assert _lib.score_topk_form(N, K, d, 128, 1)["slices"] == -(-nt // tps)
        assert _same(whole, run(block_rows=128)), forced
        lib_env("DL_RANK_SLICES")


# ---------------------------------------------------------------------------------------------------------------------
def _checked(tag, Zb, Hb, t, pos, ign=None, **kw):
    from disenlink_amd import ops
    out = ops.score_recon_loss(Zb.to(DEV), Hb.to(DEV), t, pos.to(DEV), None if ign is None else ign.to(DEV), table_dtype=BF16, **kw)
    check(tag, out, recon_ref.recon64(Zb.float(), Hb.float(), t, pos, ign))


def test_empty_positive_set():
    N, K, d = 300, 3, 40
    _Z, _H, Zb, Hb = tables_bf16(N, K, d, seed=1)
    _pos, ign = recon_ref.pair_sets(N, seed=4)
    none = torch.zeros(N, N, dtype=torch.bool)
    _checked("no positives", Zb, Hb, 1.0, none, ign)
    _checked("no positives, nothing ignored", Zb, Hb, 1.0, none)


@pytest.mark.parametrize("N", [129, 300])
def test_everything_ignored(N):
    from disenlink_amd import ops
    _Z, _H, Zb, Hb = tables_bf16(N, 3, 40, seed=2)
    pos, _ign = recon_ref.pair_sets(N, seed=5)
    everything = torch.ones(N, N, dtype=torch.bool)
    loss, dZ, dH, counts = ops.score_recon_loss(Zb.to(DEV), Hb.to(DEV), 1.0, pos.to(DEV), everything.to(DEV), block_rows=128,
                                                table_dtype=BF16)
    assert float(loss) == 0.0 and counts.tolist() == [0, 0]
    assert not bool(dZ.any()) and not bool(dH.any())
    ref = recon_ref.recon64(Zb.float(), Hb.float(), 1.0, pos, everything)
    assert ref["loss"] == 0.0 and ref["counts"] == (0, 0) and not bool(ref["dZ"].any()) and not bool(ref["dH"].any())


def test_a_row_whose_positives_fill_a_whole_tile_and_a_positive_in_the_last_column():
    N, K, d = 300, 3, 40
    _Z, _H, Zb, Hb = tables_bf16(N, K, d, seed=4)
    pos, ign = recon_ref.pair_sets(N, seed=7)
    pos[5, 128:256] = True                                                # the second candidate tile of row 5, all of it
    pos[128:256, 5] = True
    ign[5, :] = ign[:, 5] = False
    _checked("full tile", Zb, Hb, 1.0, pos, ign)
    N = 129                                                              # column N - 1: the only column of the last tile
    _Z, _H, Zb, Hb = tables_bf16(N, K, d, seed=5)
    pos = torch.zeros(N, N, dtype=torch.bool)
    pos[3, 128] = pos[128, 3] = pos[127, 128] = pos[128, 127] = True
    for b in (None, 128):
        _checked(f"column N - 1, block_rows={b}", Zb, Hb, 1.0, pos, block_rows=b)


def saturated_tables(N=200, K=8, d=16):
    """test_gpu_recon's saturated construction on bf16 tables: Z = 0 (every exp is 1), H along one axis, s(u, v) = K c_u c_v.
    sqrt(25 / 8) = 1.76777 rounds to the bf16 value 1.765625, so |s| = 8 x 1.765625^2 = 24.94 in the saturated third (an fp32
    sigmoid is exactly 1 from about 17 on) and, with |c| <= 0.2 elsewhere (0.2 rounds to at most 0.2001953125), |s| <= 2.83."""
    gen = torch.Generator().manual_seed(12)
    c = torch.where(torch.rand(N, generator=gen) < 0.33, torch.tensor((25.0 / 8.0) ** 0.5), 0.2 * torch.rand(N, generator=gen))
    c = c * torch.where(torch.rand(N, generator=gen) < 0.5, -1.0, 1.0)
    H = torch.zeros(N, K, d)
    H[:, :, 0] = c[:, None]
    return torch.zeros(N, K, d).to(BF16), H.to(BF16)


def saturated_reference(Zb, Hb, pos, ign):
    """The fp64 reference (p rounded to fp32) on the ROUNDED tables, and the preconditions it alone must meet."""
    ref = recon_ref.recon64(Zb.float(), Hb.float(), 1.0, pos, ign, fp32_p=True)
    s, inc = ref["logit"], ref["included"]
    assert int((inc & (s > 20)).sum()) > 1000 and int((inc & (s < -20)).sum()) > 1000 and not bool((inc & (s.abs() >= 3) & (s.abs() < 20)).any())
    assert ref["loss"] > recon_ref.recon64(Zb.float(), Hb.float(), 1.0, pos, ign)["loss"] + 1.0      # saturated negatives at 100 w, not 25 w
    return ref


def test_saturated_pairs_clamp_the_loss_and_contribute_exactly_zero_gradient():
    from disenlink_amd import ops
    N = 200
    Zb, Hb = saturated_tables(N)
    pos, ign = recon_ref.pair_sets(N, seed=13)
    ref = saturated_reference(Zb, Hb, pos, ign)
    out = ops.score_recon_loss(Zb.to(DEV), Hb.to(DEV), 1.0, pos.to(DEV), ign.to(DEV), block_rows=128, table_dtype=BF16)
    check("saturated", out, ref)
    assert _same(out, ops.score_recon_loss(Zb.float().to(DEV), Hb.float().to(DEV), 1.0, pos.to(DEV), ign.to(DEV), block_rows=128))


# ---------------------------------------------------------------------------------------------------------------------
def _sd(g):
    return {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}


def _module(g, table_dtype):
    from disenlink_amd.model import Disentangle
    m = g["meta"]
    model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"], table_dtype=table_dtype)
    model.load_state_dict(_sd(g))
    return model.to(DEV)


@pytest.mark.parametrize("name", ["k8_d64", "k4_d32"])
def test_step_of_a_bf16_module_is_the_hand_composition_bit_for_bit(name):
    from disenlink_amd import ops
    g = load_golden(name)
    m = g["meta"]
    N, K, d = m["N"], m["K"], m["d"]
    _p, ign = recon_ref.pair_sets(N, seed=N)
    model = _module(g, BF16)
    x = torch.from_numpy(g["x"]).to(DEV)
    graph = model._graph_of(torch.from_numpy(g["adj"]).to(DEV))
    sets = ops.recon_sets(graph, ign.to(DEV), N, DEV)
    beta, t = float(model.beta), float(model.temperature)

    emb, loss = model.forward_recon_loss(x, graph, ignore=sets)
    model.zero_grad()
    loss.backward()
    ops.check_recon_counts(ops.ReconLoss.last_counts, sets)
    got = {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    model.zero_grad()
    Z = model.project(x)
    Zt, p, a, s, H = ops.step_tables(graph, Z.detach(), beta, t, BF16)
    assert Zt.dtype == BF16 and H.dtype == BF16
    assert torch.equal(emb.detach().view(N, K, d).view(torch.int32), H.float().view(torch.int32))
    loss2, dZ, dH, counts = ops.score_recon_loss(Zt, H, t, sets, table_dtype=BF16)
    assert torch.equal(loss.detach().reshape(1).view(torch.int32), loss2.to(torch.float32).reshape(1).view(torch.int32))
    ops.check_recon_counts(counts, sets)
    Z.backward(ops.route_aggregate_bwd(graph, Zt, beta, t, p, a, s, dH, dZ_accum=dZ))
    for k, prm in model.named_parameters():
        assert torch.equal(got[k].view(torch.int32), prm.grad.view(torch.int32)), k
        assert bool(torch.isfinite(got[k]).all())
    assert any(bool(v.any()) for v in got.values())

    if name == "k8_d64":                                                  # the tripwire: an fp32 module scores other tables
        _emb32, loss32 = _module(g, torch.float32).forward_recon_loss(x, graph, ignore=sets)
        assert loss32.item() != loss.item()


def test_three_adam_steps_of_the_recon_objective_on_bf16_tables_lower_the_loss():
    """test_gpu_recon's loop test for a bf16 module, at K = 4, d = 32: routing and aggregation on bf16 tables exist for the
    tuned shapes only (DL_FAST_SHAPES_BF16: (4, 32), (8, 64), (16, 128), (5, 64), (8, 32)), and the fp32 test's (4, 16) is
    none of them — a bf16 module of that shape is refused by dl_route_fwd, whatever the objective, which is pinned below."""
    from disenlink_amd import _lib
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    sg = synthetic_graph("chameleon", seed=3, scale=300 / 2277)
    assert 280 <= sg.n_nodes <= 320
    run = prepare_run(make_link_split(sg.src, sg.dst, sg.n_nodes, m=2, seed=1), DEV, row_bytes=4 * 32 * 2)
    torch.manual_seed(0)
    model = Disentangle(32, 16, 32, nfactor=4, beta=0.7, t=1, table_dtype=BF16).to(DEV)
    x = torch.from_numpy(sg.features()[:, :32].copy()).to(DEV)
    res = run_link_prediction(model, x, run, epochs=3, lr=5e-3, objective="recon", recon_block_rows=128)
    print(f"recon objective on bf16 tables, N={sg.n_nodes}: losses {res.losses} val AUCs {res.val_aucs} test AUC {res.test_auc}")
    assert res.epochs_run == 3 and all(np.isfinite(res.losses))
    assert res.losses[2] < res.losses[0]
    assert 0.0 <= res.test_auc <= 1.0 and res.best_val_auc == max(res.val_aucs)
    narrow = Disentangle(32, 16, 16, nfactor=4, beta=0.7, t=1, table_dtype=BF16).to(DEV)
    with pytest.raises(_lib.DisenlinkHipError, match="no generic bf16 path"):
        run_link_prediction(narrow, x, run, epochs=1, objective="recon", recon_block_rows=128)


def test_cli_trains_the_recon_objective_on_bf16_tables():
    """`--objective recon --table-dtype bf16` in a process of its own (squirrel's synthetic stand-in: the CLI has no smaller
    graph; K = 4, d = 32: a shape bf16 routing serves, which the CLI's default K = 3 is not); more than one GPU stays refused."""
    from disenlink_amd.main import main
    r = subprocess.run([sys.executable, "-m", "disenlink_amd.main", "--dataset", "squirrel", "--synthetic", "--objective", "recon",
                        "--table-dtype", "bf16", "--nfactor", "4", "--nembed", "32", "--epochs", "2", "--run", "1", "--quiet"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    with pytest.raises(SystemExit, match="one GPU"):
        main(["--synthetic", "--objective", "recon", "--gpus", "2"])
    with pytest.raises(SystemExit, match="one GPU"):
        main(["--synthetic", "--objective", "recon", "--table-dtype", "bf16", "--gpus", "2"])


# ---------------------------------------------------------------------------------------------------------------------
def test_launches_follow_the_current_stream():
    from disenlink_amd import ops
    N, K, d = 700, 8, 64
    _Z, _H, Zb, Hb = tables_bf16(N, K, d, seed=4)
    Zb, Hb = Zb.to(DEV), Hb.to(DEV)
    pos, ign = recon_ref.pair_sets(N, seed=8)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV)
    want = ops.score_recon_loss(Zb, Hb, 1.0, sets, block_rows=256, table_dtype=BF16)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device=DEV)
    with torch.cuda.stream(side):
        for _ in range(8):
            big = big @ big * 1e-2                            # work ahead of the inputs on the side stream
        Zs, Hs = Zb * 1.0, Hb * 1.0                           # produced on the side stream, consumed by our kernels
        got = ops.score_recon_loss(Zs, Hs, 1.0, sets, block_rows=256, table_dtype=BF16)
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
    """test_gpu_recon's check for the bf16 entry: with prepared sets, loss and gradients come without a device
    synchronisation (sync debug mode "error"); where the build does not honour that mode the call is captured in ONE graph
    and a replay must reproduce the eager bits.  The tables are fp32 leaves, rounded inside (straight-through)."""
    from disenlink_amd import ops
    N, K, d = 300, 8, 64
    Z, H, Zb, Hb = tables_bf16(N, K, d, seed=6)
    pos, ign = recon_ref.pair_sets(N, seed=9)
    sets = ops.recon_sets(pos.to(DEV), ign.to(DEV), N, DEV)
    Zg, Hg = Z.to(DEV).requires_grad_(True), H.to(DEV).requires_grad_(True)

    def step():
        loss = ops.ReconLoss.apply(Zg, Hg, 1.0, sets, None, 128, BF16)
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
    ref = ops.score_recon_loss(Zb.to(DEV), Hb.to(DEV), 1.0, sets, table_dtype=BF16)
    assert eager[1].dtype == torch.float32                                                   # fp32 gradients, of the rounded tables
    assert torch.equal(eager[1], 2.0 * ref[1]) and torch.equal(eager[2], 2.0 * ref[2])      # the backward scales by the incoming scalar


def test_unsupported_inputs_raise_in_forward():
    from disenlink_amd import _lib, ops
    N = 40
    pos, _ign = recon_ref.pair_sets(N, seed=1)
    sets = ops.recon_sets(pos.to(DEV), None, N, DEV)
    Z = torch.randn(N, 2, 16, device=DEV)
    for a, b in ((Z.bfloat16(), Z), (Z, Z.bfloat16())):                   # a mix of the two types
        with pytest.raises(TypeError, match="both bf16 or both fp32"):
            ops.score_recon_loss(a, b, 1.0, sets, table_dtype=BF16)
        with pytest.raises(TypeError, match="both bf16 or both fp32"):
            ops.ReconLoss.apply(a, b, 1.0, sets, None, None, BF16)
    with pytest.raises(TypeError, match="table_dtype"):
        ops.score_recon_loss(Z, Z, 1.0, sets, table_dtype=torch.float16)
    with pytest.raises(TypeError):
        ops.score_recon_loss(Z.half(), Z.half(), 1.0, sets, table_dtype=BF16)
    wide = torch.randn(N, 2, 129, device=DEV).bfloat16()
    with pytest.raises(_lib.DisenlinkHipError, match="d <= 128"):
        ops.score_recon_loss(wide, wide, 1.0, sets, table_dtype=BF16)
    with pytest.raises(_lib.DisenlinkHipError, match="d <= 128"):
        ops.ReconLoss.apply(wide, wide, 1.0, sets, None, None, BF16)
    with pytest.raises(TypeError, match="fp32"):                          # without the keyword bf16 tensors stay refused
        ops.score_recon_loss(Z.bfloat16(), Z.bfloat16(), 1.0, sets)
    with pytest.raises(TypeError, match="fp32"):
        ops.ReconLoss.apply(Z.bfloat16(), Z.bfloat16(), 1.0, sets)
