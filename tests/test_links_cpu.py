"""The thresholded link graph without a GPU: the reference selection of tests/links_ref.py on hand-made matrices, the seeds
of the GPU case list against the fp64 reference, the workspace formula, and every refusal of dl_score_links_*,
ops.score_links and --predict-links (none of which gets as far as a launch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import links_ref
import mine_ref
from links_ref import select_links, upper_pairs

INF, NAN = float("inf"), float("nan")


def dense_of(rowptr, col, logit, N):
    """the CSR as a dense matrix, NaN where there is no entry; checks the layout on the way"""
    assert rowptr.dtype == torch.int64 and rowptr.numel() == N + 1 and int(rowptr[0]) == 0 and int(rowptr[-1]) == col.numel()
    out = torch.full((N, N), NAN, dtype=logit.dtype)
    for r in range(N):
        c = col[int(rowptr[r]):int(rowptr[r + 1])]
        assert (c[1:] > c[:-1]).all() and (c != r).all() and ((c >= 0) & (c < N)).all()
        out[r, c] = logit[int(rowptr[r]):int(rowptr[r + 1])]
    return out


def test_select_links_ties_zeros_infinities_nan_and_the_inclusive_floor():
    S = torch.tensor([[9.0, 1.5, -0.0, INF, NAN],
                      [7.0, 9.0, 1.5, -INF, 0.0],
                      [7.0, 7.0, 9.0, 1.5, -2.0],
                      [7.0, 7.0, 7.0, 9.0, NAN],
                      [7.0, 7.0, 7.0, 7.0, 9.0]])                       # the diagonal and the lower triangle do not count
    N = 5
    # no floor: everything but the NaN, -inf included; -0 comes back as +0
    rp, col, lg = select_links(S, None, -INF)
    D = dense_of(rp, col, lg, N)
    assert rp.tolist() == [0, 3, 7, 11, 14, 16]
    assert torch.equal(torch.isnan(D), torch.isnan(D.T)) and torch.equal(D.nan_to_num(5.0), D.T.nan_to_num(5.0))
    assert math.isnan(D[0, 4]) and math.isnan(D[3, 4]) and math.isnan(D[2, 2])
    assert D[0, 3] == INF and D[3, 0] == INF and D[1, 3] == -INF and D[3, 1] == -INF
    assert D[0, 2] == 0 and not torch.signbit(D[0, 2]) and not torch.signbit(D[2, 0])
    # a floor of 0: both zeros pass (-0 >= 0), the tie at 1.5 passes three times, -2 and -inf do not
    rp, col, lg = select_links(S, None, 0.0)
    u, v, x = upper_pairs(rp, col, lg)
    assert list(zip(u.tolist(), v.tolist())) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 4), (2, 3)]
    assert x.tolist() == [1.5, 0.0, INF, 1.5, 0.0, 1.5] and not torch.signbit(x).any()
    # a floor equal to an entry is inclusive; just above it the ties are gone together
    n_pairs = lambda floor: len(upper_pairs(*select_links(S, None, floor))[0])
    assert n_pairs(1.5) == 4 and n_pairs(float(np.nextafter(np.float32(1.5), np.float32(2)))) == 1
    # +inf passes every floor, +inf included; NaN passes none
    rp, col, lg = select_links(S, None, INF)
    assert rp.tolist() == [0, 1, 1, 1, 2, 2] and col.tolist() == [3, 0] and lg.tolist() == [INF, INF]
    # exclusion in either orientation, read as unordered pairs
    ex = torch.zeros(N, N, dtype=torch.bool)
    ex[3, 0] = ex[1, 2] = True
    u, v, x = upper_pairs(*select_links(S, ex, 0.0))
    assert list(zip(u.tolist(), v.tolist())) == [(0, 1), (0, 2), (1, 4), (2, 3)]


def test_select_links_empty_and_all_pairs():
    N = 6
    S = torch.arange(N * N, dtype=torch.float32).reshape(N, N)
    rp, col, lg = select_links(S, None, 1e9)
    assert rp.tolist() == [0] * (N + 1) and col.numel() == 0 and lg.numel() == 0
    rp, col, lg = select_links(S, None, -INF)
    assert (rp[1:] - rp[:-1]).tolist() == [N - 1] * N
    D = dense_of(rp, col, lg, N)
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool), 1)
    assert torch.equal(D[iu], S[iu]) and torch.equal(D.T[iu], S[iu])          # (v, u) carries the logit of (u, v)
    rp, col, lg = select_links(torch.zeros(1, 1), None, -INF)
    assert rp.tolist() == [0, 0] and col.numel() == 0
    # it agrees with mine_ref.select_top as a set
    g = torch.Generator().manual_seed(5)
    S = torch.randn(40, 40, generator=g)
    ex = torch.rand(40, 40, generator=g) < 0.2
    u, v, x = upper_pairs(*select_links(S, ex, 0.1))
    tu, tv, tx = mine_ref.select_top(S, 40 * 40, ex | ex.T, 0.1)
    order = torch.argsort(tu * 40 + tv)
    assert torch.equal(u, tu[order]) and torch.equal(v, tv[order]) and torch.equal(x, tx[order])


def test_the_gpu_cases_keep_within_the_straddle_cap_at_the_fp64_median():
    """test_gpu_links.py::test_against_fp64 asserts this on the device; here the seeds are confirmed on the CPU"""
    for N, (K, d), t in links_ref.GPU_CASES:
        if N < 2:
            continue
        Z, H = links_ref.tables(N, K, d, seed=links_ref.case_seed(N, K, d, t))
        s64, band = mine_ref.logits64(Z, H, t)
        iu = torch.triu(torch.ones(N, N, dtype=torch.bool), 1)
        floor = float(torch.median(s64[iu]))
        straddle = iu & (s64 - band < floor) & (s64 + band >= floor)
        assert int(straddle.sum()) <= max(1, int(0.01 * int(iu.sum()))), (N, K, d, t)


def test_the_golden_thresholds_keep_within_the_doubt_cap():
    """test_gpu_links.py compares predicted_links with the reference link_pred >= p outside the parity tolerance of p: for
    every fixture, with and without its edges as candidates, at most 1 % of the candidates lie inside it"""
    from conftest import golden_case_names, load_golden
    assert set(golden_case_names()) == set(links_ref.GOLDEN_P)
    two_sided = 0
    for name in golden_case_names():
        g = load_golden(name)
        N, p = g["meta"]["N"], links_ref.GOLDEN_P[name]
        lp, adj = g["link_pred"], g["adj"]
        iu = np.triu(np.ones((N, N), bool), 1)
        doubt = links_ref.golden_doubt(lp, p)
        for cand in (iu, iu & ~((adj != 0) | (adj.T != 0))):
            assert int((doubt & cand).sum()) <= 0.01 * int(cand.sum()), name
        n_pass = int((iu & (lp >= p)).sum())
        two_sided += 0 < n_pass < int(iu.sum())
    assert two_sided >= 8                                             # all but the two saturated fixtures


def test_form_and_workspace_formula():
    from disenlink_amd import _lib
    lib = _lib.load()
    for N, K, d in ((1, 1, 8), (2, 3, 40), (129, 2, 96), (300, 8, 64), (5201, 8, 64), (41554, 8, 64), (46340, 1, 1)):
        f = _lib.score_links_form(N, K, d)
        assert f["tiles"] == -(-N // 128) and f["nd"] == -(-d // 32) and f["cells"] == N * f["tiles"]
        assert f["pairs"] == (f["tiles"] * (f["tiles"] + 1) // 2 if N >= 2 else 0) and f["scans"] == (2 if N >= 2 else 0)
        assert f["grid"] == -(-f["pairs"] // f["pairs_per_wg"]) and f["pairs_per_wg"] >= 1
        assert {k: f[k] for k in ("nd", "tiles", "pairs", "pairs_per_wg", "grid")} == \
               {k: v for k, v in _lib.score_mine_form(N, K, d, 1).items() if k in ("nd", "tiles", "pairs", "pairs_per_wg", "grid")}
        assert int(lib.dl_score_links_workspace_bytes(N, K, d)) == links_ref.workspace_bytes(N, K, f)
    # far below an [N,N] fp32 matrix at the Penn94 shape
    assert int(lib.dl_score_links_workspace_bytes(41554, 8, 64)) < 41554 * 41554 * 4 // 20
    assert lib.dl_score_links_supported(8, 64) == 1 and lib.dl_score_links_supported(8, 130) == 0
    for K, d in ((8, 64), (8, 130), (0, 64), (65, 8), (1, 1), (64, 128)):
        assert lib.dl_score_links_supported(K, d) == lib.dl_score_mine_supported(K, d)
    for bad in ((0, 8, 64), (-1, 8, 64), (46341, 8, 64), (100, 8, 130), (100, 0, 64)):
        assert int(lib.dl_score_links_workspace_bytes(*bad)) == 0
        with pytest.raises(_lib.DisenlinkHipError):
            _lib.score_links_form(*bad)


def test_form_follows_the_forced_run_length(lib_env):
    from disenlink_amd import _lib
    lib_env("DL_MINE_TILES", 5)
    f = _lib.score_links_form(1000, 2, 32)
    assert f["pairs"] == 36 and f["pairs_per_wg"] == 5 and f["grid"] == 8
    lib_env("DL_MINE_TILES")
    assert _lib.score_links_form(1000, 2, 32)["pairs_per_wg"] == 1


def _calls(lib, N=8, K=2, d=8, t=1.0, Z=256, H=256, exr=None, exc=None, nf=None, ws=256, ws_bytes=1 << 30, rowptr=256, nnz=0,
           col=256, logit=256):
    """both entries with dummy non-NULL pointers: a refusal returns before the first launch"""
    head = (Z, H, N, K, d, t, exr, exc, 0.0, nf, ws, ws_bytes, rowptr)
    return {"dl_score_links_count": lambda: lib.dl_score_links_count(*head, None),
            "dl_score_links_fill": lambda: lib.dl_score_links_fill(*head, nnz, col, logit, None, None)}


def test_c_abi_refusals():
    from disenlink_amd import _lib
    lib = _lib.load()
    p = 256
    bad_filters = [(_lib.DlNodeFilter(p, 0, p), b"outside 1..64"), (_lib.DlNodeFilter(p, 65, p), b"outside 1..64"),
                   (_lib.DlNodeFilter(None, 2, p), b"NULL group or allow"), (_lib.DlNodeFilter(p, 2, None), b"NULL group or allow")]
    refused = [(dict(d=130), b"1 <= d <= 128"), (dict(d=0), None), (dict(K=0), None), (dict(K=65), None),
               (dict(N=0), b"outside 1..46340"), (dict(N=-3), b"outside 1..46340"), (dict(N=46341), b"outside 1..46340"),
               (dict(t=0.0), b"temperature is 0"), (dict(Z=None), b"NULL argument"), (dict(H=None), b"NULL argument"),
               (dict(rowptr=None), b"NULL argument"), (dict(exr=p), b"go together"), (dict(exc=p), b"go together")]
    refused += [(dict(nf=C.byref(f)), msg) for f, msg in bad_filters]
    for kw, msg in refused:
        for name, call in _calls(lib, **kw).items():
            assert call() == -1, (name, kw)                           # DL_E_ARG
            assert msg is None or msg in lib.dl_last_error(), (name, kw, lib.dl_last_error())
    need = int(lib.dl_score_links_workspace_bytes(8, 2, 8))
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        for name, call in _calls(lib, **kw).items():
            assert call() == -3 and b"workspace too small" in lib.dl_last_error(), (name, kw)      # DL_E_WORKSPACE
    fill = lambda **kw: _calls(lib, ws_bytes=need, **kw)["dl_score_links_fill"]()
    assert fill(nnz=-1) == -1 and b"nnz=-1 is negative" in lib.dl_last_error()
    assert fill(nnz=5, col=None) == -1 and b"NULL output" in lib.dl_last_error()
    assert fill(nnz=5, logit=None) == -1 and b"NULL output" in lib.dl_last_error()
    assert fill(nnz=-1, nf=C.byref(_lib.DlNodeFilter(p, 64, p))) == -1 and b"nnz=-1" in lib.dl_last_error()     # a good filter passes


def test_header_and_binding_list_the_entries():
    import test_host_cpu
    from disenlink_amd import _lib
    names = test_host_cpu._declared_symbols()
    for n in ("dl_score_links_supported", "dl_score_links_form", "dl_score_links_workspace_bytes", "dl_score_links_count",
              "dl_score_links_fill"):
        assert n in names and n in _lib.EXPORTS
    count, fill = _lib.EXPORTS["dl_score_links_count"][1], _lib.EXPORTS["dl_score_links_fill"][1]
    assert fill[:len(count) - 1] == count[:-1] and fill[-1] is count[-1]           # the same arguments, then nnz and the arrays


def test_ops_refuse_bad_arguments_before_any_launch():
    """the tables are on the CPU: a call that got as far as the kernels' own checks fails with DisenlinkHipError"""
    from disenlink_amd import ops
    Z = torch.zeros(6, 2, 8)
    good = ops.NodeFilter.different(torch.tensor([0, 1, 0, 1, 0, 1]))
    asym = ops.NodeFilter(torch.tensor([0, 1, 0, 1, 0, 1]), torch.tensor([[0, 1], [0, 0]]))
    short = ops.NodeFilter.different(torch.tensor([0, 1, 0]))
    for call in (lambda f: ops.score_links(Z, Z, 1.0, 0.0, node_filter=f), lambda f: ops.score_link_degrees(Z, Z, 1.0, 0.0, node_filter=f)):
        with pytest.raises(ValueError, match="node filter of 3 nodes, tables of 6"):
            call(short)
        with pytest.raises(TypeError, match="ops.NodeFilter"):
            call(torch.tensor([0, 1, 0, 1, 0, 1]))
        with pytest.raises(ValueError, match="symmetric"):
            call(asym)
        with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
            call(good)
    with pytest.raises(TypeError, match="fp32"):
        ops.score_links(Z.bfloat16(), Z.bfloat16(), 1.0, 0.0)
    assert ops.LINKS_MAX_N == 46340


def test_cli_flags_parse_and_refuse_what_is_out_of_scope(tmp_path):
    from disenlink_amd.main import build_parser, main
    a = build_parser().parse_args([])
    assert a.predict_links is None and a.links_out is None
    a = build_parser().parse_args(["--predict-links", "0.9", "--links-out", "x.txt"])
    assert a.predict_links == 0.9 and a.links_out == "x.txt"
    base = ["--dataset", "squirrel", "--synthetic", "--epochs", "1", "--run", "1", "--quiet"]
    with pytest.raises(SystemExit, match="--predict-links runs on one GPU with fp32 tables only"):
        main(base + ["--gpus", "2", "--predict-links", "0.5"])
    with pytest.raises(SystemExit, match="--predict-links runs on one GPU with fp32 tables only"):
        main(base + ["--table-dtype", "bf16", "--predict-links", "0.5"])
    for p in ("1.5", "-0.1", "nan"):
        with pytest.raises(SystemExit, match="0 <= P <= 1"):
            main(base + ["--predict-links", p])
    with pytest.raises(SystemExit, match="goes with --predict-links"):
        main(base + ["--links-out", str(tmp_path / "x.txt")])
    groups = tmp_path / "groups.txt"
    groups.write_text("\n".join(str(i % 2) for i in range(10)) + "\n")
    with pytest.raises(SystemExit, match="go together"):
        main(base + ["--predict-links", "0.5", "--node-groups", str(groups)])


def test_predicted_links_views():
    """PredictedLinks.degree / .pairs() on a hand-made CSR (the views are host-side torch)"""
    from disenlink_amd.model import PredictedLinks
    S = torch.tensor([[0.0, 2.0, -1.0, 3.0], [0.0, 0.0, 0.5, -4.0], [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
    rp, col, lg = select_links(S, None, 0.0)
    links = PredictedLinks(rp, col.int(), lg, torch.sigmoid(lg))
    assert links.n_nodes == 4 and links.degree.tolist() == [2, 2, 2, 2]
    src, dst, logit, prob = links.pairs()
    assert list(zip(src.tolist(), dst.tolist())) == [(0, 1), (0, 3), (1, 2), (2, 3)] and logit.tolist() == [2.0, 3.0, 0.5, 1.0]
    assert torch.equal(prob, torch.sigmoid(logit))
