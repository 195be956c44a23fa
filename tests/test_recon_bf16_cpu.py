"""CPU checks of the reconstruction loss on bf16 tables: workspace and launch form of the *_dtype entries (host only), the
refusals that come before any launch, the header / binding lists, the CLI's refusals, and the preconditions of the GPU
file's saturation test on the fp64 reference alone."""
import inspect

import pytest
import torch

import recon_ref

BF16 = torch.bfloat16


def test_bf16_workspace_is_smaller_by_the_four_plane_arrays_and_the_form_is_the_same():
    from disenlink_amd import _lib
    lib = _lib.load()
    for N, K, d in ((300, 8, 64), (5201, 8, 64), (41554, 16, 128), (129, 3, 100), (1, 1, 1)):
        Np, dp = -(-N // 128) * 128, -(-d // 32) * 32
        for b in (0, 128, 256):
            f32 = int(lib.dl_score_recon_workspace_bytes(N, K, d, b))
            assert f32 == int(lib.dl_score_recon_workspace_bytes_dtype(N, K, d, _lib.DL_F32, b)) and f32 > 0
            assert f32 - int(lib.dl_score_recon_workspace_bytes_dtype(N, K, d, _lib.DL_BF16, b)) == 16 * K * Np * dp, (N, K, d, b)
            form = _lib.score_recon_form(N, K, d, b)
            assert form == _lib.score_recon_form(N, K, d, b, _lib.DL_F32) == _lib.score_recon_form(N, K, d, b, _lib.DL_BF16)
            assert form["nslice"] == _lib.score_allpairs_bwd_dense_form(N, K, d)["nslice"]
    for bad in ((0, 8, 64, _lib.DL_BF16, 0), (100, 8, 129, _lib.DL_BF16, 0), (100, 8, 64, _lib.DL_BF16, 100), (100, 8, 64, 2, 0),
                (100, 8, 64, -1, 0)):
        assert int(lib.dl_score_recon_workspace_bytes_dtype(*bad)) == 0, bad
        with pytest.raises(_lib.DisenlinkHipError):
            _lib.score_recon_form(bad[0], bad[1], bad[2], bad[4], bad[3])
    assert lib.dl_score_scan_supported(8, 64, _lib.DL_BF16) == 1 and lib.dl_score_scan_supported(8, 129, _lib.DL_BF16) == 0


def test_c_abi_refusals_of_the_dtype_entry():
    from disenlink_amd import _lib
    lib = _lib.load()
    p = 256

    def call(N=8, K=2, d=8, dt=_lib.DL_BF16, t=1.0, Z=p, pr=p, ir=None, b=0, ws=p, ws_bytes=1 << 30):
        return lib.dl_score_recon_dtype(Z, p, N, K, d, dt, t, pr, p, ir, None, 0.5, 0.5, b, p, p, p, p, ws, ws_bytes, None)
    for kw, msg in ((dict(dt=2), b"unknown dtype"), (dict(dt=-1), b"unknown dtype"), (dict(d=129), b"1 <= d <= 128"),
                    (dict(N=0), b"outside 1.."), (dict(t=0.0), b"temperature"), (dict(Z=None), b"NULL argument"),
                    (dict(pr=None), b"NULL argument"), (dict(ir=p), b"both"), (dict(b=100), b"multiple of 128")):
        assert call(**kw) == -1, kw                                       # DL_E_ARG
        assert msg in lib.dl_last_error(), (kw, lib.dl_last_error())
    need = int(lib.dl_score_recon_workspace_bytes_dtype(8, 2, 8, _lib.DL_BF16, 0))
    assert need < int(lib.dl_score_recon_workspace_bytes(8, 2, 8, 0))
    for kw in (dict(ws=None), dict(ws_bytes=need - 1)):
        assert call(**kw) == -3 and b"workspace too small" in lib.dl_last_error(), kw
    # what suffices for bf16 tables is too small for fp32 tables of the same shape
    assert call(dt=_lib.DL_F32, ws_bytes=need) == -3


def test_ops_refuse_bad_tables_before_any_launch():
    from disenlink_amd import ops
    Z = torch.zeros(6, 2, 8)
    pos = (torch.tensor([0, 1]), torch.tensor([1, 2]))
    with pytest.raises(TypeError, match="table_dtype must be"):
        ops.score_recon_loss(Z, Z, 1.0, pos, table_dtype=torch.float16)
    for a, b in ((Z.bfloat16(), Z), (Z, Z.bfloat16()), (Z.half(), Z.half())):
        with pytest.raises(TypeError, match="both bf16 or both fp32"):
            ops.score_recon_loss(a, b, 1.0, pos, table_dtype=BF16)
    with pytest.raises(TypeError, match="fp32"):                          # without the keyword: as before
        ops.score_recon_loss(Z.bfloat16(), Z.bfloat16(), 1.0, pos)
    for a in (Z, Z.bfloat16()):                                           # both forms pass the type check and stop at the device
        with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
            ops.score_recon_loss(a, a, 1.0, pos, table_dtype=BF16)


def test_header_binding_and_python_list_the_entries():
    import test_host_cpu
    from disenlink_amd import _lib, ops, recon
    from disenlink_amd.model import Disentangle
    names = test_host_cpu._declared_symbols()
    for n in ("dl_score_recon_dtype", "dl_score_recon_workspace_bytes_dtype", "dl_score_recon_form_dtype"):
        assert n in names and n in _lib.EXPORTS
    assert set(_lib.EXPORTS) == set(names)
    assert inspect.signature(ops.score_recon_loss).parameters["table_dtype"].default is torch.float32
    assert inspect.signature(recon.ReconLoss.forward).parameters["table_dtype"].default is torch.float32
    assert inspect.signature(_lib.score_recon_form).parameters["dtype"].default == _lib.DL_F32
    assert issubclass(ops.HotPathRecon, torch.autograd.Function)
    assert "fp32 tables" not in Disentangle.forward_recon_loss.__doc__ and "HotPathRecon" in Disentangle.forward_recon_loss.__doc__


def test_cli_takes_bf16_tables_with_the_recon_objective_and_still_refuses_the_rest():
    from disenlink_amd.main import build_parser, main
    a = build_parser().parse_known_args(["--objective", "recon", "--table-dtype", "bf16"])[0]
    assert (a.objective, a.table_dtype) == ("recon", "bf16")
    for dtype in ([], ["--table-dtype", "bf16"]):
        for flag in (["--gpus", "2"], ["--graph"]):
            with pytest.raises(SystemExit, match="one GPU in the eager loop only"):
                main(["--synthetic", "--objective", "recon", *dtype, *flag])
    assert "bf16 tables" in " ".join(build_parser().format_help().split())


def test_saturation_construction_meets_its_preconditions_on_bf16_tables():
    """What test_gpu_recon_bf16's saturation test asserts of the fp64 reference before it looks at the GPU: on the ROUNDED
    tables |s| >= 20 in the saturated group (8 x 1.765625^2 = 24.94), < 3 elsewhere, thousands of each sign."""
    from test_gpu_recon_bf16 import saturated_reference, saturated_tables
    N = 200
    Zb, Hb = saturated_tables(N)
    assert Zb.dtype == BF16 and Hb.dtype == BF16
    c = Hb[:, 0, 0].float().abs()
    assert set(c[c > 1].tolist()) == {1.765625} and float(c[c <= 1].max()) <= 0.2001953125
    pos, ign = recon_ref.pair_sets(N, seed=13)
    ref = saturated_reference(Zb, Hb, pos, ign)
    s = ref["logit"][ref["included"]].abs()
    assert float(s[s >= 20].min()) == pytest.approx(8 * 1.765625 ** 2) and float(s[s < 20].max()) < 3.0
