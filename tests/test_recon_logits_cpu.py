"""CPU checks of the logit-space reconstruction loss and the dense link_logits: the fp64 reference against autograd of the
dense formulation with binary_cross_entropy_with_logits, the saturated inputs of the GPU tests, the module cases, the
training loop's objective switch, the CLI option, the header / binding lists and the C-ABI refusals."""
import inspect
import itertools

import pytest
import torch

import recon_logits_ref as rl
import recon_ref

GRID_KD = ((1, 8), (3, 100), (8, 64), (4, 128))


@pytest.mark.parametrize("N,K,d,t,pw", [(1, 2, 8, 1.0, None), (2, 1, 8, 1.0, None), (37, 3, 20, 2.0, None), (60, 2, 8, 1.0, 3.5)])
def test_reference_equals_autograd_of_the_dense_formulation_with_logits(N, K, d, t, pw):
    Z, H = recon_ref.tables_cpu(N, K, d, seed=N + d, scale=1.5)
    pos, ign = recon_ref.pair_sets(N, seed=N)
    r = rl.recon_logits64(Z, H, t, pos, ign, pw)
    loss, dZ, dH = rl.dense_autograd64(Z, H, t, pos, ign, pw)
    assert abs(r["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    for got, want in ((r["dZ"], dZ), (r["dH"], dH)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert r["counts"] == recon_ref.recon64(Z, H, t, pos, ign, pw)["counts"]
    assert r["band_loss"] >= 0 and bool((r["band_dZ"] >= 0).all()) and bool((r["band_dH"] >= 0).all())


def test_logit_and_probability_references_agree_where_nothing_saturates():
    """Away from the clamps the two contracts are one function: the same loss and gradients to fp64 rounding."""
    N, K, d = 37, 3, 20
    Z, H = recon_ref.tables_cpu(N, K, d, seed=5)
    pos, ign = recon_ref.pair_sets(N, seed=N)
    a, b = rl.recon_logits64(Z, H, 1.0, pos, ign), recon_ref.recon64(Z, H, 1.0, pos, ign)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 and float((a["dH"] - b["dH"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("N,Kd,t", list(itertools.product((129, 300), GRID_KD, (1.0, 2.0))))
def test_saturated_inputs_meet_their_conditions(N, Kd, t):
    """The rescaled tables of tests/test_gpu_recon_logits.py: the largest included |logit| is 60, at least 5 % of the included
    pairs lie where an fp32 sigmoid is exactly 1 and at least 10 included positives where p (1 - p) < 1e-12 (N = 129 with
    (K, d) = (1, 8) holds 4 and 2: recon_logits_ref.min_positives_below) — and the probability-space contract, evaluated with an fp32-rounded p, is far from the logit-space loss there."""
    K, d = Kd
    Z, H, pos, ign = rl.saturated_tables(N, K, d, t)
    ref = rl.recon_logits64(Z, H, t, pos, ign)
    inc = ref["included"]
    assert abs(float(ref["logit"][inc].abs().max()) - 60.0) <= 1e-4              # 60 up to the fp32 rounding of the scaled H
    share, low = rl.saturation(ref)
    print(f"N={N} K={K} d={d} t={t}: {100 * share:.1f} % of the included pairs above 16.64, {low} positives below -27.6")
    assert share >= rl.MIN_SHARE_ABOVE and low >= rl.min_positives_below(N, K, d)
    if (N, K, d) == (129, 1, 8):
        assert low == (4 if t == 1.0 else 2)                             # the figures recon_logits_ref records for this shape
    assert bool(torch.isfinite(ref["dZ"]).all()) and bool(torch.isfinite(ref["dH"]).all())
    prob = recon_ref.recon64(Z, H, t, pos, ign, fp32_p=True)
    assert abs(prob["loss"] - ref["loss"]) > 100 * ref["band_loss"]


def test_one_pair_in_closed_form():
    """N = 2, K = 1, d = 8, Z = 0: x = h_0 . h_1.  A negative at x = 40 costs softplus(40) w = 40 w and keeps the gradient
    w sigma(40) ~ w; a positive at x = -40 the same by symmetry."""
    for sign, is_pos in ((1.0, False), (-1.0, True)):
        Z, H = torch.zeros(2, 1, 8), torch.zeros(2, 1, 8)
        H[0, 0, 0], H[1, 0, 0] = 8.0, sign * 5.0
        pos = torch.tensor([[False, is_pos], [is_pos, False]])
        r = rl.recon_logits64(Z, H, 1.0, pos, pos_weight=1.0)
        assert r["counts"] == ((1, 0) if is_pos else (0, 1)) and r["w"] == (1.0, 1.0)
        assert abs(r["loss"] - 40.0) <= 1e-12 and float(r["dH"][0, 0, 0]) == pytest.approx(5.0, abs=1e-12)
        assert float(r["dH"][1, 0, 0]) == pytest.approx(sign * 8.0, abs=1e-12)


def test_module_cases_are_those_on_which_fp32_is_faithful_to_fp64():
    """In logit space a plain fp32 CPU evaluation follows the fp64 parameter gradients to a quarter of the GPU test's tolerance
    on EVERY small golden case — the saturated ones included, which the probability form admits on two of eight."""
    from conftest import golden_case_names, load_golden
    assert set(recon_ref.SMALL_GOLDEN_CASES) <= set(golden_case_names())
    for name in module_cases(verbose=True):
        assert name in recon_ref.SMALL_GOLDEN_CASES
    assert tuple(module_cases()) == recon_ref.SMALL_GOLDEN_CASES


def module_cases(verbose=False):
    """The small golden cases on which fp32 is faithful to fp64 under the MODULE_TOL / 4 rule, recomputed."""
    from conftest import load_golden
    out = []
    for name in recon_ref.SMALL_GOLDEN_CASES:
        g = load_golden(name)
        l64, g64, _ign, _counts, big = rl.module_reference(g, torch.float64)
        l32, g32, _ign, _counts, _big = rl.module_reference(g, torch.float32)
        worst = max(float((g32[k] - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-6) for k in g64)
        if verbose:
            print(f"{name}: fp32 against fp64  loss {abs(l32 - l64) / max(1.0, abs(l64)):.1e}  gradients {worst:.1e}  "
                  f"largest included |logit| {big:.4g}")
        if worst <= recon_ref.MODULE_TOL / 4:
            out.append(name)
    return out


# ---------------------------------------------------------------------------------------------------------------------
class _Recorder(torch.nn.Module):
    """A module that records which of the loop's entry points were called and stops the loop at the first of them."""

    class Stop(Exception):
        pass

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def _stop(self, name):
        self.calls.append(name)
        raise self.Stop

    def forward_pairs(self, *a, **k):
        self._stop("forward_pairs")

    def forward_pair_logits(self, *a, **k):
        self._stop("forward_pair_logits")

    def forward_recon_loss(self, *a, **k):
        self._stop("forward_recon_loss")

    def forward_recon_logits_loss(self, *a, **k):
        self._stop("forward_recon_logits_loss")


class _NoLogits(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward_pairs(self, *a, **k):
        raise AssertionError("refused before the first call")

    forward_recon_loss = forward_pairs


def _tiny_run():
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run
    sg = synthetic_graph("chameleon", seed=2, scale=0.06)
    return sg, prepare_run(make_link_split(sg.src, sg.dst, sg.n_nodes, m=2, seed=0), "cpu")


def test_objective_switch_of_the_training_loop():
    from disenlink_amd import train
    sg, run = _tiny_run()
    x = torch.zeros(sg.n_nodes, 4)
    assert inspect.signature(train.run_link_prediction).parameters["objective"].default == "pairs"
    with pytest.raises(ValueError, match="objective must be"):
        train.run_link_prediction(_Recorder(), x, run, objective="recon-logits")
    with pytest.raises(TypeError, match="forward_recon_logits_loss"):
        train.run_link_prediction(_NoLogits(), x, run, objective="recon-logit")
    m = _Recorder()
    with pytest.raises(ValueError, match="GPU only"):                    # CPU tensors: refused before the first call
        train.run_link_prediction(m, x, run, epochs=1, objective="recon-logit")
    assert m.calls == []
    # the other objectives keep their paths
    for kw, want in (({}, "forward_pairs"), ({"objective": "recon"}, "forward_recon_loss")):
        m = _Recorder()
        with pytest.raises(_Recorder.Stop):
            train.run_link_prediction(m, x, run, epochs=1, **kw)
        assert m.calls == [want]


def test_recon_logit_loop_calls_the_logit_entries_with_recons_sets():
    """_run_recon with its logit flag: forward_recon_logits_loss gets the sets, weight and strip height "recon" gets."""
    from disenlink_amd import ops, train
    sg, run = _tiny_run()
    seen = {}

    class Probe(_Recorder):
        def forward_recon_logits_loss(self, x, graph, ignore=None, pos_weight=None, block_rows=None):
            seen.update(graph=graph, sets=ignore, pos_weight=pos_weight, block_rows=block_rows)
            self._stop("forward_recon_logits_loss")
    m = Probe()
    with pytest.raises(_Recorder.Stop):
        train._run_recon(m, torch.zeros(sg.n_nodes, 4), run, 1, 1e-3, 10, 0.0, None, 2.5, 256, True)
    assert m.calls == ["forward_recon_logits_loss"]
    assert isinstance(seen["sets"], ops.ReconSets) and seen["graph"] is run.graph
    assert seen["pos_weight"] == 2.5 and seen["block_rows"] == 256
    with pytest.raises(ValueError, match="eager loop only"):
        train.run_link_prediction(Probe(), torch.zeros(sg.n_nodes, 4), run, objective="recon-logit", use_graph=True)


def test_cli_has_the_objective_option():
    from disenlink_amd.main import build_parser
    a = build_parser().parse_known_args(["--objective", "recon-logit", "--pos-weight", "3", "--recon-block-rows", "256",
                                         "--table-dtype", "bf16"])[0]
    assert (a.objective, a.pos_weight, a.recon_block_rows, a.table_dtype) == ("recon-logit", 3.0, 256, "bf16")
    assert build_parser().parse_known_args([])[0].objective == "pairs"


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--graph"]])
def test_cli_refuses_what_recon_refuses(extra):
    from disenlink_amd import main
    with pytest.raises(SystemExit, match="one GPU in the eager loop only"):
        main.main(["--dataset", "squirrel", "--synthetic", "--objective", "recon-logit", *extra])


NEW_ENTRIES = ("dl_score_recon_logits", "dl_score_allpairs_logits_fwd", "dl_score_allpairs_logits_workspace_bytes",
               "dl_score_allpairs_logits_bwd_dense")


def test_header_and_binding_list_the_entries():
    import test_host_cpu
    from disenlink_amd import _lib, link_pred, ops, recon
    from disenlink_amd.model import Disentangle
    names = test_host_cpu._declared_symbols()
    for n in NEW_ENTRIES:
        assert n in names and n in _lib.EXPORTS
    assert set(_lib.EXPORTS) == set(names)
    assert _lib.EXPORTS["dl_score_recon_logits"] == _lib.EXPORTS["dl_score_recon_dtype"]          # one argument list
    assert _lib.EXPORTS["dl_score_allpairs_logits_fwd"] == _lib.EXPORTS["dl_score_allpairs_fwd"]
    for n in ("score_recon_logits_loss", "ReconLogitsLoss", "HotPathReconLogits", "score_allpairs_logits_fwd",
              "score_allpairs_logits_bwd_dense", "ScoreAllPairsLogits"):
        assert hasattr(ops, n)
    assert ops.score_recon_logits_loss is recon.score_recon_logits_loss and ops.ScoreAllPairsLogits is link_pred.ScoreAllPairsLogits
    assert inspect.signature(ops.score_recon_logits_loss) == inspect.signature(ops.score_recon_loss)
    assert issubclass(ops.ReconLogitsLoss, ops.ReconLoss) and ops.ReconLogitsLoss.last_counts is None
    assert (inspect.signature(Disentangle.forward_recon_logits_loss) == inspect.signature(Disentangle.forward_recon_loss))
    assert hasattr(Disentangle, "forward_logits")


def test_c_abi_refusals():
    from disenlink_amd import _lib
    lib = _lib.load()
    p = 256

    def call(N=8, K=2, d=8, dt=_lib.DL_F32, t=1.0, Z=p, pr=p, pc=p, ir=None, ic=None, b=0, loss=p, ws=p, ws_bytes=1 << 30):
        return lib.dl_score_recon_logits(Z, p, N, K, d, dt, t, pr, pc, ir, ic, 0.5, 0.5, b, loss, p, p, p, ws, ws_bytes, None)
    for kw, msg in ((dict(d=129), b"1 <= d <= 128"), (dict(K=0), None), (dict(N=0), b"outside 1.."), (dict(t=0.0), b"temperature"),
                    (dict(Z=None), b"NULL argument"), (dict(pr=None), b"NULL argument"), (dict(loss=None), b"NULL argument"),
                    (dict(ir=p), b"both"), (dict(b=100), b"multiple of 128"), (dict(dt=7), b"unknown dtype")):
        assert call(**kw) == -1, kw
        assert msg is None or msg in lib.dl_last_error(), (kw, lib.dl_last_error())
    for dt in (_lib.DL_F32, _lib.DL_BF16):
        need = int(lib.dl_score_recon_workspace_bytes_dtype(8, 2, 8, dt, 0))
        for kw in (dict(ws=None), dict(ws_bytes=need - 1)):
            assert call(dt=dt, **kw) == -3 and b"workspace too small" in lib.dl_last_error(), kw


def test_c_abi_refusals_of_the_dense_logits():
    from disenlink_amd import _lib
    lib = _lib.load()
    p = 256

    def fwd(N=8, K=2, d=8, dt=_lib.DL_F32, t=1.0, Z=p, out=p, ws=p, ws_bytes=1 << 30):
        return lib.dl_score_allpairs_logits_fwd(Z, p, N, K, d, dt, t, out, ws, ws_bytes, None)

    def bwd(N=8, K=2, d=8, t=1.0, g=p, dZ=p, ws=p, ws_bytes=1 << 30):
        return lib.dl_score_allpairs_logits_bwd_dense(p, p, N, K, d, t, g, dZ, p, ws, ws_bytes, None)
    for kw, msg in ((dict(K=0), None), (dict(N=46341), b"46340"), (dict(t=0.0), b"temperature"), (dict(Z=None), b"NULL argument"),
                    (dict(out=None), b"NULL argument"), (dict(dt=_lib.DL_BF16), b"fp32 tables")):
        assert fwd(**kw) == -1, kw
        assert msg is None or msg in lib.dl_last_error(), (kw, lib.dl_last_error())
    for kw, msg in ((dict(d=129), b"1 <= d <= 128"), (dict(K=0), None), (dict(N=46341), b"46340"), (dict(t=0.0), b"temperature"),
                    (dict(g=None), b"NULL argument"), (dict(dZ=None), b"NULL argument")):
        assert bwd(**kw) == -1, kw
        assert msg is None or msg in lib.dl_last_error(), (kw, lib.dl_last_error())
    assert fwd(N=0) == 0 and bwd(N=0) == 0
    # the planes pad d to 32: the forward's workspace for every d, the plain entry's where that one takes the matrix cores
    for N, K, d in ((8, 2, 8), (300, 3, 100), (129, 8, 64)):
        need = int(lib.dl_score_allpairs_logits_workspace_bytes(N, K, d))
        assert need == 2 * 2 * K * 3 * (-(-N // 128) * 128) * (-(-d // 32) * 32)
        if d % 32 == 0:
            assert need == int(lib.dl_score_allpairs_workspace_bytes(N, K, d, _lib.DL_F32))
        for kw in (dict(ws=None), dict(ws_bytes=need - 1)):
            assert fwd(N=N, K=K, d=d, **kw) == -3 and b"workspace too small" in lib.dl_last_error(), kw
        need = int(lib.dl_score_allpairs_bwd_dense_workspace_bytes(N, K, d))
        for kw in (dict(ws=None), dict(ws_bytes=need - 1)):
            assert bwd(N=N, K=K, d=d, **kw) == -3 and b"workspace too small" in lib.dl_last_error(), kw
    for bad in ((0, 2, 8), (46341, 2, 8), (8, 0, 8), (8, 2, 0)):
        assert int(lib.dl_score_allpairs_logits_workspace_bytes(*bad)) == 0


def test_ops_refuse_bad_arguments_before_any_launch():
    from disenlink_amd import ops
    from disenlink_amd.model import Disentangle
    Z = torch.zeros(6, 2, 8)
    pos = (torch.tensor([0, 1]), torch.tensor([1, 2]))
    with pytest.raises(TypeError, match="fp32"):
        ops.score_recon_logits_loss(Z.bfloat16(), Z.bfloat16(), 1.0, pos)
    with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
        ops.score_recon_logits_loss(Z, Z, 1.0, pos)
    with pytest.raises(TypeError, match="fp32"):
        ops.score_allpairs_logits_fwd(Z.bfloat16(), Z.bfloat16(), 1.0)
    with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
        ops.score_allpairs_logits_fwd(Z, Z, 1.0)
    with pytest.raises(ops._lib.DisenlinkHipError, match="d <= 128"):
        Disentangle(4, 4, 160, nfactor=2, beta=0.5).forward_logits(torch.zeros(6, 4), torch.zeros(6, 6))
    with pytest.raises(ops._lib.DisenlinkHipError, match="fp32 tables"):
        Disentangle(4, 4, 8, nfactor=2, beta=0.5, table_dtype=torch.bfloat16).forward_logits(torch.zeros(6, 4), torch.zeros(6, 6))
