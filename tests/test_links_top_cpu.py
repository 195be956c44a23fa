"""The budgeted link graph without a GPU: the reference selection of tests/links_top_ref.py against brute force, the budgets
chosen for the golden fixtures, the workspace formula and the form, every refusal of dl_score_links_top_* that needs no
device, the flag --predict-top, and the call path of ops.score_top_links through a recording stand-in."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import links_ref
import links_top_ref
from disenlink_amd.scans import score_top_links                      # what this module is about
from links_ref import upper_pairs
from links_top_ref import select_top_links

INF, NAN = float("inf"), float("nan")


def brute_force(S, m, ex, floor):
    """the chosen pairs by sorting Python tuples: larger logit first (-0 as +0), then the smaller u * N + v"""
    N = S.shape[0]
    cand = []
    for u, v in itertools.combinations(range(N), 2):
        x = float(S[u, v])
        if x != x or x < floor or (ex is not None and (bool(ex[u, v]) or bool(ex[v, u]))):
            continue
        cand.append((-(x + 0.0), u * N + v, u, v))
    return sorted((u, v) for _, _, u, v in sorted(cand)[:m])


def test_reference_against_brute_force_on_tiny_matrices():
    g = torch.Generator().manual_seed(11)
    for N in (1, 2, 3, 6, 9):
        S = torch.randn(N, N, generator=g)
        S = (S * 2).round() / 2                                       # halves: many exact ties
        if N >= 6:
            S[0, 3], S[1, 2], S[2, 5], S[0, 1], S[1, 4] = INF, NAN, -INF, -0.0, 0.0
        ex = torch.rand(N, N, generator=g) < 0.15
        total = N * (N - 1) // 2
        for excluded, floor in ((None, -INF), (ex, -INF), (None, 0.0), (ex, -0.5)):
            for m in sorted({1, 2, max(1, total // 2), max(1, total - 1), total + 3}):
                rp, col, lg = select_top_links(S, m, excluded, floor)
                want = brute_force(S, m, excluded, floor)
                u, v, x = upper_pairs(rp, col, lg)
                assert list(zip(u.tolist(), v.tolist())) == want, (N, m, floor)
                assert int(rp[-1]) == 2 * len(want) == col.numel()
                assert all(float(a) == float(S[i, j]) for (i, j), a in zip(want, x)) and not torch.signbit(x[x == 0]).any()
                # symmetric, ascending columns
                rows = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
                key = rows * N + col
                assert (key[1:] > key[:-1]).all()
                D = torch.zeros(N, N, dtype=torch.bool)
                D[rows, col] = True
                assert torch.equal(D, D.T)


def test_reference_cuts_a_tie_class_by_the_pair_index():
    S = torch.full((5, 5), 1.0)
    S[0, 4] = 2.0
    u, v, _ = upper_pairs(*select_top_links(S, 4))
    assert list(zip(u.tolist(), v.tolist())) == [(0, 1), (0, 2), (0, 3), (0, 4)]      # (0, 4) first, then the smallest indices
    assert int(select_top_links(S, 100)[0][-1]) == 20 and int(select_top_links(torch.zeros(1, 1), 3)[0][-1]) == 0
    # m above the candidates: links_ref.select_links itself
    g = torch.Generator().manual_seed(2)
    S = torch.randn(12, 12, generator=g)
    a, b = select_top_links(S, 1000, None, 0.2), links_ref.select_links(S, None, 0.2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_gpu_budgets():
    assert links_top_ref.gpu_m_values(300) == (1, 7, 1000, 44855, 22425) and links_top_ref.gpu_m_values(1) == (1, 7, 1000, 5)
    assert links_top_ref.gpu_m_values(2) == (1, 7, 1000, 6)
    assert links_top_ref.GPU_CASES == links_ref.GPU_CASES
    from disenlink_amd import ops
    assert min(links_top_ref.BIG_M) > ops.MINE_MAX_M and links_top_ref.BIG_N * (links_top_ref.BIG_N - 1) // 2 > max(links_top_ref.BIG_M)


def test_the_golden_budgets_keep_within_the_doubt_cap():
    """test_gpu_links_top.py compares top_predicted_links with the reference's own link_pred around p*, the m-th largest
    reference probability: for every fixture that is not saturated, with and without its edges as candidates, at most 1 % of
    the candidates (or the m-th pair alone) lie within the parity tolerance of p*, and both sides of the cut are populated"""
    from conftest import golden_case_names, load_golden
    assert set(golden_case_names()) == set(links_top_ref.GOLDEN_M) and set(links_top_ref.GOLDEN_SATURATED) < set(links_top_ref.GOLDEN_M)
    for name in golden_case_names():
        g = load_golden(name)
        N, m = g["meta"]["N"], links_top_ref.GOLDEN_M[name]
        lp, adj = g["link_pred"], g["adj"]
        iu = np.triu(np.ones((N, N), bool), 1)
        for cand in (iu, iu & ~((adj != 0) | (adj.T != 0))):
            assert 1 <= m < int(cand.sum()), name
            p, doubt = links_top_ref.golden_cut(lp, cand, m)
            assert int(doubt.sum()) >= 1
            if name in links_top_ref.GOLDEN_SATURATED:
                assert int(doubt.sum()) > 0.9 * int(cand.sum()), name  # nothing to tell apart: the reason they are set aside
            else:
                assert int(doubt.sum()) <= links_top_ref.doubt_cap(int(cand.sum())), (name, int(doubt.sum()), int(cand.sum()))
                assert int((cand & (lp > p) & ~doubt).sum()) > 0 and int((cand & (lp < p) & ~doubt).sum()) > 0, name


def workspace_bytes(N, K, form):
    """dl_score_links_top_workspace_bytes_dtype (fp32 tables) from the plan of dl_score_links_top_form: the workspace of
    dl_score_links (links_ref.workspace_bytes) plus the selection state (32 bytes) and a histogram of 2,048 32-bit counts,
    each rounded up to 256 bytes"""
    return links_ref.workspace_bytes(N, K, form) + 256 + 2048 * 4


def test_form_and_workspace_formula(lib_env):
    from disenlink_amd import _lib
    lib = _lib.load()
    F32, BF16 = _lib.DL_F32, _lib.DL_BF16
    for N, K, d in ((1, 1, 8), (2, 3, 40), (129, 2, 96), (300, 8, 64), (5201, 8, 64), (41554, 8, 64), (46340, 1, 1)):
        f, base = _lib.score_links_top_form(N, K, d), _lib.score_links_form(N, K, d)
        assert list(f) == list(base) + ["scans_offset"]
        assert {k: f[k] for k in base if k != "scans"} == {k: base[k] for k in base if k != "scans"}
        assert f["scans"] == (6 + 2 if N >= 2 else 0) and f["scans_offset"] == _lib.score_mine_form(N, K, d, 1)["scans_offset"] == 24
        got = int(lib.dl_score_links_top_workspace_bytes_dtype(N, K, d, F32))
        assert got == workspace_bytes(N, K, f) == int(lib.dl_score_links_workspace_bytes_dtype(N, K, d, F32)) + 8448
        # bf16 tables: the planes shrink as in dl_score_links, the select's blocks do not
        assert int(lib.dl_score_links_top_workspace_bytes_dtype(N, K, d, BF16)) == \
            int(lib.dl_score_links_workspace_bytes_dtype(N, K, d, BF16)) + 8448
    for bad in ((0, 8, 64), (-1, 8, 64), (46341, 8, 64), (100, 8, 130), (100, 0, 64)):
        assert int(lib.dl_score_links_top_workspace_bytes_dtype(*bad, F32)) == 0
        with pytest.raises(_lib.DisenlinkHipError):
            _lib.score_links_top_form(*bad)
    assert int(lib.dl_score_links_top_workspace_bytes_dtype(100, 8, 64, 7)) == 0
    lib_env("DL_MINE_TILES", 5)
    f = _lib.score_links_top_form(1000, 2, 32)
    assert f["pairs"] == 36 and f["pairs_per_wg"] == 5 and f["grid"] == 8


def _calls(lib, N=8, K=2, d=8, dt=0, t=1.0, Z=256, H=256, exr=None, exc=None, m=5, nf=None, ws=256, ws_bytes=1 << 30, rowptr=256,
           nnz=0, col=256, logit=256):
    """both entries with dummy non-NULL pointers: a refusal returns before the first launch"""
    head = (Z, H, N, K, d, dt, t, exr, exc, 0.0, m, nf, ws, ws_bytes, rowptr)
    return {"count": lambda: lib.dl_score_links_top_count_dtype(*head, None),
            "fill": lambda: lib.dl_score_links_top_fill_dtype(*head, nnz, col, logit, None, None)}


def test_c_abi_refusals_carry_the_links_entries_codes_and_texts():
    from disenlink_amd import _lib
    lib = _lib.load()
    p = 256
    bad_filters = [(_lib.DlNodeFilter(p, 0, p), b"outside 1..64"), (_lib.DlNodeFilter(p, 65, p), b"outside 1..64"),
                   (_lib.DlNodeFilter(None, 2, p), b"NULL group or allow"), (_lib.DlNodeFilter(p, 2, None), b"NULL group or allow")]
    refused = [(dict(d=130), b"1 <= d <= 128"), (dict(d=0), None), (dict(K=0), None), (dict(K=65), None), (dict(dt=7), b"unknown dtype"),
               (dict(N=0), b"outside 1..46340"), (dict(N=-3), b"outside 1..46340"), (dict(N=46341), b"outside 1..46340"),
               (dict(t=0.0), b"temperature is 0"), (dict(m=0), b"m=0 below 1"), (dict(m=-4), b"m=-4 below 1"),
               (dict(Z=None), b"NULL argument"), (dict(H=None), b"NULL argument"),
               (dict(rowptr=None), b"NULL argument"), (dict(exr=p), b"go together"), (dict(exc=p), b"go together")]
    refused += [(dict(nf=C.byref(f)), msg) for f, msg in bad_filters]
    for kw, msg in refused:
        for name, call in _calls(lib, **kw).items():
            assert call() == -1, (name, kw)                           # DL_E_ARG
            assert msg is None or msg in lib.dl_last_error(), (name, kw, lib.dl_last_error())
    # the texts are the links entries' own
    for kw in (dict(N=46341), dict(t=0.0), dict(exr=p), dict(d=130)):
        _calls(lib, **kw)["count"]()
        mine = lib.dl_last_error()
        head = tuple(kw.get(k, v) for k, v in (("Z", p), ("H", p), ("N", 8), ("K", 2), ("d", 8), ("t", 1.0), ("exr", None), ("exc", None)))
        assert lib.dl_score_links_count(*head, 0.0, None, p, 1 << 30, p, None) == -1 and lib.dl_last_error() == mine
    for dt in (_lib.DL_F32, _lib.DL_BF16):
        need = int(lib.dl_score_links_top_workspace_bytes_dtype(8, 2, 8, dt))
        for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
            for name, call in _calls(lib, dt=dt, **kw).items():
                assert call() == -3 and b"workspace too small" in lib.dl_last_error(), (name, kw)      # DL_E_WORKSPACE
                assert b"dl_score_links_top_workspace_bytes_dtype" in lib.dl_last_error()
    # the links workspace alone is too small: the select's blocks come on top
    assert _calls(lib, ws_bytes=int(lib.dl_score_links_workspace_bytes(8, 2, 8)))["count"]() == -3
    need = int(lib.dl_score_links_top_workspace_bytes_dtype(8, 2, 8, 0))
    fill = lambda **kw: _calls(lib, ws_bytes=need, **kw)["fill"]()
    assert fill(nnz=-1) == -1 and b"nnz=-1 is negative" in lib.dl_last_error()
    assert fill(nnz=5, col=None) == -1 and b"NULL output" in lib.dl_last_error()
    assert fill(nnz=5, logit=None) == -1 and b"NULL output" in lib.dl_last_error()
    assert fill(nnz=-1, m=1 << 40, nf=C.byref(_lib.DlNodeFilter(p, 64, p))) == -1 and b"nnz=-1" in lib.dl_last_error()


def test_header_and_binding_list_the_dtype_entries_only():
    import test_host_cpu
    from disenlink_amd import _lib
    names = test_host_cpu._declared_symbols()
    want = ["dl_score_links_top_form", "dl_score_links_top_workspace_bytes_dtype", "dl_score_links_top_count_dtype",
            "dl_score_links_top_fill_dtype"]
    assert sorted(n for n in names if "links_top" in n) == sorted(want) == sorted(n for n in _lib.EXPORTS if "links_top" in n)
    count, fill = _lib.EXPORTS["dl_score_links_top_count_dtype"][1], _lib.EXPORTS["dl_score_links_top_fill_dtype"][1]
    assert fill[:len(count) - 1] == count[:-1] and fill[-1] is count[-1]           # the same arguments, then nnz and the arrays
    links = _lib.EXPORTS["dl_score_links_count_dtype"][1]
    assert count[:10] == links[:10] and count[10] is C.c_int64 and count[11:] == links[10:]      # m behind min_logit


def test_ops_refuse_bad_arguments_before_any_launch():
    from disenlink_amd import ops
    Z = torch.zeros(6, 2, 8)
    good = ops.NodeFilter.different(torch.tensor([0, 1, 0, 1, 0, 1]))
    asym = ops.NodeFilter(torch.tensor([0, 1, 0, 1, 0, 1]), torch.tensor([[0, 1], [0, 0]]))
    short = ops.NodeFilter.different(torch.tensor([0, 1, 0]))
    call = lambda f: ops.score_top_links(Z, Z, 1.0, 5, node_filter=f)
    with pytest.raises(ValueError, match="node filter of 3 nodes, tables of 6"):
        call(short)
    with pytest.raises(TypeError, match="ops.NodeFilter"):
        call(torch.tensor([0, 1, 0, 1, 0, 1]))
    with pytest.raises(ValueError, match="symmetric"):
        call(asym)
    with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
        call(good)
    with pytest.raises(TypeError, match="fp32"):
        ops.score_top_links(Z.bfloat16(), Z.bfloat16(), 1.0, 5)
    assert ops.score_top_links is score_top_links                     # re-exported


def test_cli_flag_parses_and_its_refusals(tmp_path):
    from disenlink_amd.main import build_parser, main
    assert build_parser().parse_args([]).predict_top is None
    a = build_parser().parse_args(["--predict-top", "5000000", "--links-out", "x.txt", "--explain", "--scan-dtype", "bf16"])
    assert a.predict_top == 5000000 and a.links_out == "x.txt" and a.explain and a.scan_dtype == "bf16" and a.predict_links is None
    base = ["--dataset", "squirrel", "--synthetic", "--epochs", "1", "--run", "1", "--quiet"]
    with pytest.raises(SystemExit, match="--predict-top M and --predict-links P each form the predicted graph"):
        main(base + ["--predict-top", "10", "--predict-links", "0.5"])
    with pytest.raises(SystemExit, match="--predict-top runs on one GPU with fp32 tables only"):
        main(base + ["--gpus", "2", "--predict-top", "10"])
    with pytest.raises(SystemExit, match="--predict-top runs on one GPU with fp32 tables only"):
        main(base + ["--table-dtype", "bf16", "--predict-top", "10"])
    for m in ("0", "-3"):
        with pytest.raises(SystemExit, match="--predict-top M: M >= 1"):
            main(base + ["--predict-top", m])
    groups = tmp_path / "groups.txt"
    groups.write_text("\n".join(str(i % 2) for i in range(10)) + "\n")
    with pytest.raises(SystemExit, match="go together"):
        main(base + ["--predict-top", "10", "--node-groups", str(groups)])
    # --links-out, --explain and --link-rule accept the flag in place of --predict-links: the next refusal is the device's
    for extra in (["--links-out", str(tmp_path / "x.txt")], ["--explain"]):
        with pytest.raises(SystemExit, match="GPU only"):
            main(base + ["--no-cuda", "--predict-top", "10"] + extra)


# ---- the call path, as tests/test_scans_call_path_cpu.py holds it for the other scans
N_, K_, D_ = 8, 2, 8


@pytest.fixture
def rec(monkeypatch):
    from test_scans_call_path_cpu import Recorder
    from disenlink_amd import _lib, scans
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(scans, "_need_cuda", lambda *tensors: None)
    monkeypatch.setattr(scans, "_stream", lambda: 0)
    monkeypatch.setattr(scans, "_empty", lambda shape, dtype, device: torch.zeros(shape, dtype=dtype, device=device))
    return r


@pytest.mark.parametrize("table_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("prepared", [False, True])
def test_the_call_is_the_dtype_entries_with_their_own_argument_list(rec, table_dtype, filtered, prepared):
    from test_scans_call_path_cpu import EXCLUDE, QUERY, fits
    from disenlink_amd import _lib, scans
    gen = torch.Generator().manual_seed(3)
    Z, H = torch.randn(N_, K_, D_, generator=gen), torch.randn(N_, K_, D_, generator=gen)
    kw = {"table_dtype": table_dtype}
    if filtered:
        kw["node_filter"] = scans.NodeFilter.same(torch.arange(N_) % 3)
    exclude = scans.pair_exclusion(EXCLUDE, N_, "cpu") if prepared else EXCLUDE
    m = (1 << 40) + 3                                                  # a 64-bit budget
    score_top_links(Z, H, 1.0, m, exclude=exclude, min_logit=0.25, **kw)
    want = _lib.DL_F32 if table_dtype is torch.float32 else _lib.DL_BF16
    calls = [c for c in rec.calls if c[0] != QUERY]
    assert [n for n, _ in calls] == ["dl_score_links_top_workspace_bytes_dtype", "dl_score_links_top_count_dtype",
                                     "dl_score_links_top_fill_dtype"]
    for entry, args in calls:
        codes = _lib.EXPORTS[entry][1]
        assert len(args) == len(codes), entry
        assert all(fits(c, a) for c, a in zip(codes, args)), (entry, args)
        assert args[3 if "_workspace_bytes" in entry else 5] == want, entry
        assert args[:3] == (N_, K_, D_) if "_workspace_bytes" in entry else args[2:5] == (N_, K_, D_), entry
    (_, _), (_, count), (_, fill) = calls
    assert count[6] == 1.0 and count[9] == 0.25 and count[10] == m                 # t, min_logit, then the budget
    assert (count[11] is None) == (not filtered) and count[13] == 4096            # the rule, the workspace as sized
    assert count[7] is not None and count[8] is not None                           # the exclusion CSR
    assert fill[:15] == count[:15] and fill[15] == 0                               # the same head and rowptr, then nnz
    if prepared:
        assert count[7] == exclude.rowptr.data_ptr() and count[8] == exclude.col.data_ptr()      # used as it is


def test_a_prepared_exclusion_of_another_graph_is_refused(rec):
    from disenlink_amd import scans
    Z = torch.zeros(N_, K_, D_)
    with pytest.raises(ValueError, match="exclusion set of 9 nodes, expected 8"):
        score_top_links(Z, Z, 1.0, 5, exclude=scans.pair_exclusion((torch.tensor([0]), torch.tensor([1])), 9, "cpu"))
    assert not [c for c in rec.calls if c[0].endswith("_count_dtype")]
