"""The host side of the all-pairs scans over bf16 tables (dl_score_*_dtype, ``table_dtype=torch.bfloat16``, --scan-dtype): the
workspace sizes against the fp32 ones at the four shapes of test_scan_pins_cpu.py, the launch forms, the refusals that need no
GPU and the command line."""
import pytest
import torch

from disenlink_amd import _lib
from test_scan_pins_cpu import PINNED, T_MAX, _measure

F32, BF16 = _lib.DL_F32, _lib.DL_BF16


def _planes_saved(N, K, d):
    """8 K Np dp: the plane arrays of Z and H (2 bytes an element) shrink from three planes to one"""
    Np, dp = (N + 127) // 128 * 128, (d + 31) // 32 * 32
    return 8 * K * Np * dp


def test_forms_do_not_depend_on_the_table_type(lib_env):
    lib_env("DL_RANK_SLICES", 3)
    lib_env("DL_MINE_TILES", 5)
    lib = _lib.load()
    for shape, want in PINNED.items():
        got = _measure(*shape)
        for name in ("topk_form", "mine_form", "pair_ranks_form", "links_form"):      # one form per family, no type argument
            assert got[name] == want[name]
    for name in ("topk", "mine", "pair_ranks", "links"):
        assert not hasattr(lib, f"dl_score_{name}_form_dtype")


def test_bf16_workspaces_shrink_by_the_two_planes_of_each_table(lib_env):
    lib_env("DL_RANK_SLICES", 3)
    lib_env("DL_MINE_TILES", 5)
    lib = _lib.load()
    for (N, K, d), want in PINNED.items():
        saved = _planes_saved(N, K, d)
        # with DL_F32 the new functions are the old ones
        assert [int(lib.dl_score_mine_workspace_bytes_dtype(N, K, d, F32, m)) for m in (1, 65536)] == want["mine_ws"]
        assert int(lib.dl_score_pair_ranks_workspace_bytes_dtype(N, K, d, F32)) == want["pair_ranks_ws"]
        assert int(lib.dl_score_pair_logits_workspace_bytes_dtype(N, K, d, F32)) == want["pair_logits_ws"]
        assert int(lib.dl_score_links_workspace_bytes_dtype(N, K, d, F32)) == want["links_ws"]
        # mine, pair ranks, pair logits, links: smaller by exactly 8 K Np dp
        assert [int(lib.dl_score_mine_workspace_bytes_dtype(N, K, d, BF16, m)) for m in (1, 65536)] == [w - saved for w in want["mine_ws"]]
        assert int(lib.dl_score_pair_ranks_workspace_bytes_dtype(N, K, d, BF16)) == want["pair_ranks_ws"] - saved
        assert int(lib.dl_score_pair_logits_workspace_bytes_dtype(N, K, d, BF16)) == want["pair_logits_ws"] - saved
        assert int(lib.dl_score_links_workspace_bytes_dtype(N, K, d, BF16)) == want["links_ws"] - saved
        # top-k / ranks: by at least that (the query planes shrink too, and the fp32 copy of the gathered rows goes)
        i = 0
        for Q in (1, N):
            for k, T in ((1, 0), (128, 0), (0, 1), (0, T_MAX)):
                assert int(lib.dl_score_topk_workspace_bytes_dtype(N, K, d, F32, Q, k, T)) == want["topk_ws"][i]
                b = int(lib.dl_score_topk_workspace_bytes_dtype(N, K, d, BF16, Q, k, T))
                assert 0 < b <= want["topk_ws"][i] - saved, (N, K, d, Q, k, T)
                i += 1


def test_unknown_dtype_and_unsupported_shapes():
    lib = _lib.load()
    assert lib.dl_score_scan_supported(8, 64, F32) == 1 and lib.dl_score_scan_supported(8, 64, BF16) == 1
    assert lib.dl_score_scan_supported(8, 64, 2) == 0 and lib.dl_score_scan_supported(8, 129, BF16) == 0
    assert lib.dl_score_scan_supported(65, 64, BF16) == 0
    for dt in (2, -1):
        assert lib.dl_score_mine_workspace_bytes_dtype(300, 3, 128, dt, 10) == 0
        assert lib.dl_score_topk_workspace_bytes_dtype(300, 3, 128, dt, 10, 5, 0) == 0
        assert lib.dl_score_pair_ranks_workspace_bytes_dtype(300, 3, 128, dt) == 0
        assert lib.dl_score_pair_logits_workspace_bytes_dtype(300, 3, 128, dt) == 0
        assert lib.dl_score_links_workspace_bytes_dtype(300, 3, 128, dt) == 0
    # the checks of the C entries that run before anything touches the device
    rc = lib.dl_score_mine_dtype(None, None, 10, 2, 32, 5, 1.0, None, None, 0.0, 3, None, None, None, None, None, None, 0, None, None)
    assert rc == -1 and b"unknown dtype 5" in lib.dl_last_error()
    rc = lib.dl_score_mine_dtype(None, None, 10, 2, 32, BF16, 1.0, None, None, 0.0, 3, None, None, None, None, None, None, 0, None, None)
    assert rc == -1 and b"NULL argument" in lib.dl_last_error()
    rc = lib.dl_score_pair_logits_dtype(None, None, 10, 2, 129, BF16, 1.0, None, None, 4, None, None, 0, None)
    assert rc == -1 and b"1 <= d <= 128" in lib.dl_last_error()
    rc = lib.dl_score_links_count_dtype(None, None, 46341, 2, 32, BF16, 1.0, None, None, 0.0, None, None, 0, None, None)
    assert rc == -1 and b"46340" in lib.dl_last_error()


def _calls(ops):
    q = torch.arange(9)
    return {
        "score_topk": lambda Z, H, **kw: ops.score_topk(Z, H, 1.0, q, 3, **kw),
        "score_ranks": lambda Z, H, **kw: ops.score_ranks(Z, H, 1.0, q[:-1], q[1:], **kw),
        "score_mine": lambda Z, H, **kw: ops.score_mine(Z, H, 1.0, 3, **kw),
        "score_pair_ranks": lambda Z, H, **kw: ops.score_pair_ranks(Z, H, 1.0, q[:-1], q[1:], **kw),
        "score_pair_logits": lambda Z, H, **kw: ops.score_pair_logits(Z, H, 1.0, q[:-1], q[1:], **kw),
        "score_links": lambda Z, H, **kw: ops.score_links(Z, H, 1.0, 0.0, **kw),
        "score_link_degrees": lambda Z, H, **kw: ops.score_link_degrees(Z, H, 1.0, 0.0, **kw),
    }


def test_ops_keyword_refusals_that_need_no_gpu():
    from disenlink_amd import ops
    Z, H = torch.randn(10, 2, 32), torch.randn(10, 2, 32)
    for name, call in _calls(ops).items():
        for tensors in ((Z, H), (Z.bfloat16(), H.bfloat16())):        # CPU tensors: there is no CPU path, with either type
            with pytest.raises(_lib.DisenlinkHipError, match="only on the GPU"):
                call(*tensors, table_dtype=torch.bfloat16)
        for bad in (torch.float16, torch.float64, torch.int32, None, "bf16", _lib.DL_BF16):
            with pytest.raises(TypeError, match="table_dtype"):
                call(Z, H, table_dtype=bad)
        with pytest.raises(TypeError, match="both"):                  # one table of each type
            call(Z.bfloat16(), H, table_dtype=torch.bfloat16)
        with pytest.raises(TypeError, match="both"):
            call(Z.half(), H.half(), table_dtype=torch.bfloat16)
        with pytest.raises(TypeError, match="fp32"):                  # without the keyword nothing changes
            call(Z.bfloat16(), H.bfloat16())
        with pytest.raises(TypeError, match="fp32"):
            call(Z.bfloat16(), H.bfloat16(), table_dtype=torch.float32)
        with pytest.raises(_lib.DisenlinkHipError, match="only on the GPU"):
            call(Z, H)


class _Model:
    """stands where the trained module would: records what the CLI's helpers pass on"""

    def __init__(self):
        self.seen = {}

    def top_missing_links(self, x, graph, m, **kw):
        self.seen["mine"] = kw
        e = torch.zeros(0)
        return e.int(), e.int(), e, e

    def link_ranks(self, x, graph, src, dst, **kw):
        self.seen["rank"] = kw
        return torch.zeros(len(src), dtype=torch.int64), torch.zeros(len(src), dtype=torch.int64)


def test_cli_scan_dtype_parses_and_reaches_the_scan_call():
    from disenlink_amd import main as cli
    p = cli.build_parser()
    assert p.parse_args([]).scan_dtype == "f32" and cli.scan_table_dtype(p.parse_args([])) is None
    args = p.parse_args(["--scan-dtype", "bf16", "--synthetic", "--mine", "5"])
    assert args.scan_dtype == "bf16" and args.mine == 5 and cli.scan_table_dtype(args) is torch.bfloat16
    with pytest.raises(SystemExit):
        p.parse_args(["--scan-dtype", "fp16"])
    model = _Model()
    cli.mine_links(model, None, None, "known", args.mine, log=lambda *_: None, table_dtype=cli.scan_table_dtype(args))
    assert model.seen["mine"] == {"exclude": "known", "node_filter": None, "table_dtype": torch.bfloat16}
    cli.mine_links(model, None, None, "known", 5, log=lambda *_: None)
    assert model.seen["mine"]["table_dtype"] is None                 # the default: fp32 tables
    # every refusal is passed: on a machine without a GPU the run ends where the device is asked for, not before
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="runs on the GPU only"):
            cli.main(["--scan-dtype", "bf16", "--synthetic", "--mine", "5"])
    # the refusals of the scans together with --table-dtype bf16 stay as they are, whatever --scan-dtype says
    for flag, word in ((["--mine", "5"], "bf16 mining"), (["--global-rank-eval"], "bf16 global ranking"),
                       (["--predict-links", "0.9"], "bf16 link graphs")):
        for scan in ([], ["--scan-dtype", "bf16"]):
            with pytest.raises(SystemExit, match=word):
                cli.main(["--synthetic", "--table-dtype", "bf16", *flag, *scan])


def test_module_methods_take_the_keyword():
    import inspect
    from disenlink_amd.model import Disentangle
    for name in ("topk_links", "link_ranks", "top_missing_links", "predicted_links", "missing_link_ranks"):
        par = inspect.signature(getattr(Disentangle, name)).parameters
        assert "table_dtype" in par and par["table_dtype"].default is None
    from disenlink_amd import ops
    for name in ("score_topk", "score_ranks", "score_mine", "score_pair_ranks", "score_pair_logits", "score_links",
                 "score_link_degrees"):
        par = inspect.signature(getattr(ops, name)).parameters
        assert par["table_dtype"].default is torch.float32
