"""CPU checks of the whole-graph reconstruction loss: the fp64 reference against autograd of the dense formulation, the
normalisation of the pair sets, the launch form and workspace of dl_score_recon, the training loop's objective switch and
the header / binding lists."""
import inspect
import itertools

import pytest
import torch

import recon_ref

GRID_N = (1, 2, 37, 128, 129, 300, 700)
GRID_KD = ((1, 8), (3, 100), (8, 64), (4, 128))


@pytest.mark.parametrize("N,K,d,t,pw", [(1, 2, 8, 1.0, None), (2, 1, 8, 1.0, None), (37, 3, 20, 2.0, None), (60, 2, 8, 1.0, 3.5)])
def test_reference_equals_autograd_of_the_dense_formulation(N, K, d, t, pw):
    Z, H = recon_ref.tables_cpu(N, K, d, seed=N + d, scale=1.5)
    pos, ign = recon_ref.pair_sets(N, seed=N)
    r = recon_ref.recon64(Z, H, t, pos, ign, pw)
    loss, dZ, dH = recon_ref.dense_autograd64(Z, H, t, pos, ign, pw)
    assert abs(r["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    for got, want in ((r["dZ"], dZ), (r["dH"], dH)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool), 1)
    assert r["counts"] == (int((pos & ~ign & iu).sum()), int((~pos & ~ign & iu).sum()))
    assert sum(r["counts"]) + int((ign & iu).sum()) == N * (N - 1) // 2
    assert r["band_loss"] >= 0 and bool((r["band_dZ"] >= 0).all()) and bool((r["band_dH"] >= 0).all())


def test_the_gpu_grid_keeps_every_probability_strictly_inside_0_1():
    """The tables of tests/test_gpu_recon.py (scale 0.5 / sqrt(d)) never saturate the fp64 sigmoid, and stay far enough from
    0 and 1 that an fp32 log(1 - p) is not dominated by the rounding of 1 - p."""
    for N, (K, d), t in itertools.product(GRID_N, GRID_KD, (1.0, 2.0)):
        if N > 300 and (K, d) != (8, 64):
            continue                                                     # the widest logits are those of (8, 64); keep this quick
        Z, H = recon_ref.tables_cpu(N, K, d, recon_ref.table_seed(N, K, d))
        pos, ign = recon_ref.pair_sets(N, seed=N)
        r = recon_ref.recon64(Z, H, t, pos, ign)
        assert 0.05 < r["p_min"] <= r["p_max"] < 0.95, (N, K, d, t, r["p_min"], r["p_max"])


def _pairs_of(rowptr, col):
    rp = rowptr.tolist()
    return {(u, int(c)) for u in range(len(rp) - 1) for c in col[rp[u]:rp[u + 1]].tolist()}


def test_normalisation_of_the_pair_sets():
    from disenlink_amd import ops
    N = 9
    # self pairs, duplicates, one orientation only, a pair in both sets (3, 4), an ignored pair listed twice in both orientations
    pos = (torch.tensor([0, 0, 2, 2, 4, 5, 5, 7]), torch.tensor([1, 1, 0, 2, 3, 5, 6, 8]))
    ign = (torch.tensor([3, 8, 7, 1, 6, 6]), torch.tensor([4, 7, 8, 1, 2, 2]))
    s = ops.recon_sets(pos, ign, N, "cpu")
    want_pos = {(0, 1), (0, 2), (5, 6)}
    want_ign = {(3, 4), (7, 8), (2, 6)}
    sym = lambda ps: ps | {(b, a) for a, b in ps}
    assert _pairs_of(s.pos_rowptr, s.pos_col) == sym(want_pos)
    assert _pairs_of(s.ign_rowptr, s.ign_col) == sym(want_ign)
    assert (s.n_pos, s.n_ignored, s.n_neg) == (3, 3, N * (N - 1) // 2 - 6)
    assert s.pos_rowptr.dtype == torch.int32 and s.pos_col.dtype == torch.int32
    for rp, c in ((s.pos_rowptr, s.pos_col), (s.ign_rowptr, s.ign_col)):   # ascending, distinct columns per row
        for u in range(N):
            row = c[int(rp[u]):int(rp[u + 1])].tolist()
            assert row == sorted(set(row))
    # a dense mask, a prepared pair_exclusion and the index pairs give the same sets
    m = torch.zeros(N, N)
    m[pos[0], pos[1]] = 1
    for form in (m, ops.pair_exclusion(pos, N, torch.device("cpu"))):
        s2 = ops.recon_sets(form, ign, N, "cpu")
        assert torch.equal(s2.pos_rowptr, s.pos_rowptr) and torch.equal(s2.pos_col, s.pos_col) and s2.n_pos == s.n_pos
    # no ignored set, an empty positive set
    s3 = ops.recon_sets(pos, None, N, "cpu")
    assert s3.ign_rowptr is None and s3.n_pos == 5 and s3.n_neg == 36 - 5
    s4 = ops.recon_sets((torch.zeros(0, dtype=torch.long),) * 2, None, N, "cpu")
    assert s4.n_pos == 0 and s4.pos_col.numel() == 0 and s4.pos_rowptr.tolist() == [0] * (N + 1)
    assert ops.recon_weights(s, None) == (pytest.approx((30 / 3) / 33), pytest.approx(1 / 33))
    assert ops.recon_weights(s, 2.0) == (pytest.approx(2 / 33), pytest.approx(1 / 33))
    assert ops.recon_weights(s4, None) == (pytest.approx(1 / 36), pytest.approx(1 / 36))
    # the reference restates the same normalisation on masks
    mp, mi = torch.zeros(N, N, dtype=torch.bool), torch.zeros(N, N, dtype=torch.bool)
    mp[pos[0], pos[1]] = True
    mi[ign[0], ign[1]] = True
    Z, H = recon_ref.tables_cpu(N, 2, 8, 0)
    assert recon_ref.recon64(Z, H, 1.0, mp, mi)["counts"] == (s.n_pos, s.n_neg)


def _align(x):
    return (x + 255) // 256 * 256


def _formula(N, K, d, block_rows, nslice):
    """include/disenlink_hip.h: four plane arrays, one strip, two cell arrays, the row sums, the slice partials."""
    Np, dp = -(-N // 128) * 128, -(-d // 32) * 32
    return (4 * _align(6 * K * Np * dp) + _align(4 * block_rows * Np) + 2 * _align(block_rows * Np // 32) + _align(8 * N)
            + _align(16 * N) + _align(8 * nslice * N * K * d if nslice > 1 else 0) + 256)


def test_form_and_workspace_have_no_n_squared_term():
    from disenlink_amd import _lib
    lib = _lib.load()
    K, d = 8, 64
    for N, b, strips, rows in ((1, 0, 1, 128), (128, 0, 1, 128), (129, 0, 1, 256), (129, 128, 2, 128), (700, 0, 1, 768),
                               (700, 128, 6, 128), (700, 256, 3, 256), (700, 4096, 1, 768)):
        f = _lib.score_recon_form(N, K, d, b)
        assert (f["Np"], f["strips"], f["block_rows"]) == (-(-N // 128) * 128, strips, rows), (N, b, f)
        assert f["nslice"] == _lib.score_allpairs_bwd_dense_form(N, K, d)["nslice"]         # of the WHOLE N, whatever b
        assert int(lib.dl_score_recon_workspace_bytes(N, K, d, b)) == _formula(N, K, d, rows, f["nslice"])
    for N in (41554, 169343):
        f = _lib.score_recon_form(N, K, d, 0)
        Np = f["Np"]
        assert f["block_rows"] % 128 == 0 and f["block_rows"] * Np * 4 <= 1 << 30 < (f["block_rows"] + 128) * Np * 4
        assert f["strips"] == -(-Np // f["block_rows"]) and f["nslice"] == 1
        need = int(lib.dl_score_recon_workspace_bytes(N, K, d, 0))
        assert need == _formula(N, K, d, f["block_rows"], 1)
        assert need < (1 << 30) + 64 * N * K * d and need < 3 * N * N * 4 // 10                 # a strip and O(N K d), against 3 N^2 floats
        # twice the strip height adds one strip and its cells, nothing else
        more = int(lib.dl_score_recon_workspace_bytes(N, K, d, 2 * f["block_rows"]))
        assert more - need == _formula(N, K, d, 2 * f["block_rows"], 1) - _formula(N, K, d, f["block_rows"], 1)
    assert _lib.score_recon_form(5201, K, d, 0)["strips"] == 1                              # the whole graph where it fits
    assert lib.dl_score_recon_supported(8, 64) == 1 and lib.dl_score_recon_supported(8, 129) == 0
    assert lib.dl_score_recon_supported(65, 8) == 0 and lib.dl_score_recon_supported(1, 1) == 1
    for bad in ((0, 8, 64, 0), (100, 8, 129, 0), (100, 0, 64, 0), (100, 8, 64, 100), (100, 8, 64, -128)):
        assert int(lib.dl_score_recon_workspace_bytes(*bad)) == 0
        with pytest.raises(_lib.DisenlinkHipError):
            _lib.score_recon_form(*bad)


def test_c_abi_refusals():
    from disenlink_amd import _lib
    lib = _lib.load()
    p = 256

    def call(N=8, K=2, d=8, t=1.0, Z=p, pr=p, pc=p, ir=None, ic=None, b=0, loss=p, ws=p, ws_bytes=1 << 30):
        return lib.dl_score_recon(Z, p, N, K, d, t, pr, pc, ir, ic, 0.5, 0.5, b, loss, p, p, p, ws, ws_bytes, None)
    for kw, msg in ((dict(d=129), b"1 <= d <= 128"), (dict(K=0), None), (dict(N=0), b"outside 1.."), (dict(t=0.0), b"temperature"),
                    (dict(Z=None), b"NULL argument"), (dict(pr=None), b"NULL argument"), (dict(loss=None), b"NULL argument"),
                    (dict(ir=p), b"both"), (dict(b=100), b"multiple of 128")):
        assert call(**kw) == -1, kw
        assert msg is None or msg in lib.dl_last_error(), (kw, lib.dl_last_error())
    need = int(lib.dl_score_recon_workspace_bytes(8, 2, 8, 0))
    for kw in (dict(ws=None), dict(ws_bytes=need - 1)):
        assert call(**kw) == -3 and b"workspace too small" in lib.dl_last_error(), kw


def test_ops_refuse_bad_arguments_before_any_launch():
    from disenlink_amd import ops, recon
    Z = torch.zeros(6, 2, 8)
    pos = (torch.tensor([0, 1]), torch.tensor([1, 2]))
    with pytest.raises(TypeError, match="fp32"):
        ops.score_recon_loss(Z.bfloat16(), Z.bfloat16(), 1.0, pos)
    with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
        ops.score_recon_loss(Z, Z, 1.0, pos)
    sets = ops.recon_sets(pos, None, 5, "cpu")
    with pytest.raises(ValueError, match="multiple of 128"):
        recon._block_rows(100)
    with pytest.raises(ValueError, match="5 nodes, tables of 6"):
        recon._sets_arg(sets, None, 6, torch.device("cpu"))
    with pytest.raises(ValueError, match="ignore=None"):
        recon._sets_arg(sets, pos, 5, torch.device("cpu"))


class _Recorder(torch.nn.Module):
    """A module that records which of the loop's entry points were called and stops the loop at the first of them."""

    class Stop(Exception):
        pass

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward_pairs(self, *a, **k):
        self.calls.append("forward_pairs")
        raise self.Stop

    def forward_recon_loss(self, *a, **k):
        self.calls.append("forward_recon_loss")
        raise self.Stop


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
    sig = inspect.signature(train.run_link_prediction)
    assert sig.parameters["objective"].default == "pairs"
    with pytest.raises(ValueError, match="eager loop only"):
        train.run_link_prediction(_Recorder(), x, run, objective="recon", use_graph=True)
    with pytest.raises(ValueError, match="objective must be"):
        train.run_link_prediction(_Recorder(), x, run, objective="dense")
    # the default takes today's path: the pair-list forward, never the reconstruction loss
    for kw in ({}, {"objective": "pairs"}):
        m = _Recorder()
        with pytest.raises(_Recorder.Stop):
            train.run_link_prediction(m, x, run, epochs=1, **kw)
        assert m.calls == ["forward_pairs"]
    m = _Recorder()
    with pytest.raises(_Recorder.Stop):
        train.run_link_prediction(m, x, run, epochs=1, objective="recon")
    assert m.calls == ["forward_recon_loss"]


def test_recon_objective_ignores_every_held_out_pair():
    """The sets the loop hands to forward_recon_loss: positives = the training graph, ignored = validation and test pairs."""
    from disenlink_amd import ops, train
    sg, run = _tiny_run()
    seen = {}

    class Probe(_Recorder):
        def forward_recon_loss(self, x, graph, ignore=None, pos_weight=None, block_rows=None):
            seen.update(graph=graph, sets=ignore, pos_weight=pos_weight, block_rows=block_rows)
            raise self.Stop
    with pytest.raises(_Recorder.Stop):
        train.run_link_prediction(Probe(), torch.zeros(sg.n_nodes, 4), run, epochs=1, objective="recon", pos_weight=2.5,
                                  recon_block_rows=256)
    s, N = seen["sets"], sg.n_nodes
    assert isinstance(s, ops.ReconSets) and seen["graph"] is run.graph and seen["pos_weight"] == 2.5 and seen["block_rows"] == 256
    b = run.n_pos + run.n_neg
    held = {(min(u, v), max(u, v)) for u, v in zip(torch.cat([run.train_val_pairs.pu[b:], run.test_pairs.pu]).tolist(),
                                                   torch.cat([run.train_val_pairs.pv[b:], run.test_pairs.pv]).tolist()) if u != v}
    edges = {(u, v) for u, v in _pairs_of(run.graph.rowptr, run.graph.col) if u < v}
    assert {(u, v) for u, v in _pairs_of(s.ign_rowptr, s.ign_col) if u < v} == held
    assert {(u, v) for u, v in _pairs_of(s.pos_rowptr, s.pos_col) if u < v} == edges - held
    assert s.n_pos == len(edges - held) and s.n_neg == N * (N - 1) // 2 - len(held) - s.n_pos


def test_cli_has_the_objective_options():
    from disenlink_amd.main import build_parser
    a = build_parser().parse_known_args([])[0]
    assert (a.objective, a.pos_weight, a.recon_block_rows) == ("pairs", None, None)
    a = build_parser().parse_known_args(["--objective", "recon", "--pos-weight", "3", "--recon-block-rows", "256"])[0]
    assert (a.objective, a.pos_weight, a.recon_block_rows) == ("recon", 3.0, 256)


def test_header_and_binding_list_the_entries():
    import test_host_cpu
    from disenlink_amd import _lib, ops
    names = test_host_cpu._declared_symbols()
    for n in ("dl_score_recon_supported", "dl_score_recon_form", "dl_score_recon_workspace_bytes", "dl_score_recon"):
        assert n in names and n in _lib.EXPORTS
    assert set(_lib.EXPORTS) == set(names)
    for n in ("score_recon_loss", "ReconLoss", "ReconSets", "recon_sets", "recon_weights", "check_recon_counts"):
        assert hasattr(ops, n)


def test_module_cases_are_those_on_which_fp32_is_faithful_to_fp64():
    """recon_ref.MODULE_CASES: a plain fp32 CPU evaluation of the dense formulation stays within a quarter of the GPU test's
    tolerance of the fp64 one exactly on those cases; on the others the fp32 sigmoid saturates."""
    from conftest import golden_case_names, load_golden
    assert set(recon_ref.SMALL_GOLDEN_CASES) <= set(golden_case_names())
    for name in recon_ref.SMALL_GOLDEN_CASES:
        g = load_golden(name)
        l64, g64, _ign, _counts, s64 = recon_ref.module_reference(g, torch.float64)
        l32, g32, _ign, _counts, s32 = recon_ref.module_reference(g, torch.float32)
        worst = max(float((g32[k] - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-6) for k in g64)
        faithful = worst <= recon_ref.MODULE_TOL / 4 and abs(l32 - l64) <= 5e-6 * max(1.0, abs(l64))
        print(f"{name}: fp32 against fp64  loss {abs(l32 - l64) / max(1.0, abs(l64)):.1e}  gradients {worst:.1e}  saturated {s32}")
        assert faithful == (name in recon_ref.MODULE_CASES), (name, worst, l32, l64)
        assert faithful == (s32 == 0) and s64 <= s32
