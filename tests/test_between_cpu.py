"""The scans between two node sets and the blocked scans without a GPU: forms, sizers and every refusal of the new C entries,
the call path of ops.score_*_between / score_*_blocks against a recording stand-in, and the block driver, the merge and the
CSR assembly with tests/between_ref.py standing in for the kernels, against a brute force over all pairs."""
import ctypes as C
import itertools

import pytest
import torch

import between_ref
import links_ref
import mine_ref
from test_scans_call_path_cpu import QUERY, Recorder, fits

INF = float("inf")
SHAPES = ((1, 1, 1, 1), (129, 5, 2, 33), (300, 200, 3, 128), (46340, 46340, 8, 64))


def up(b):
    return (b + 255) // 256 * 256


def planes_bytes(n, K, d, P):
    return up(2 * K * P * (-(-n // 128) * 128) * (-(-d // 32) * 32))


# ---------------------------------------------------------------------- forms, sizers, refusals
@pytest.mark.parametrize("nA,nB,K,d", SHAPES)
def test_forms_and_workspace_formulas(nA, nB, K, d):
    from disenlink_amd import _lib
    lib = _lib.load()
    ta, tb = -(-nA // 128), -(-nB // 128)
    fm, fl = _lib.score_mine_between_form(nA, nB, K, d, 7), _lib.score_links_between_form(nA, nB, K, d)
    for f in (fm, fl):
        assert (f["nd"], f["tiles_a"], f["tiles_b"], f["pairs"]) == (-(-d // 32), ta, tb, ta * tb)
        assert f["pairs_per_wg"] >= 1 and f["grid"] == -(-f["pairs"] // f["pairs_per_wg"])
    assert fm["max_scans"] == 7 and fm["scans_offset"] == 24
    assert fl["scans"] == 2 and fl["cells_a"] == nA * tb and fl["cells_b"] == nB * ta
    for dt, P in ((_lib.DL_F32, 3), (_lib.DL_BF16, 1)):
        tabs = 2 * planes_bytes(nA, K, d, P) + 2 * planes_bytes(nB, K, d, P)
        for m in (1, 65536):
            assert int(lib.dl_score_mine_between_workspace_bytes_dtype(nA, nB, K, d, dt, m)) == 256 + up(2048 * 4) + up(8 * m) + tabs + 256
        assert int(lib.dl_score_links_between_workspace_bytes_dtype(nA, nB, K, d, dt)) == \
            tabs + up(4 * nA * tb) + up(4 * nB * ta) + up(4 * nA) + up(4 * nB) + 256


def test_form_follows_the_forced_run_length(lib_env):
    from disenlink_amd import _lib
    lib_env("DL_MINE_TILES", 4)
    f = _lib.score_links_between_form(300, 200, 2, 32)
    assert f["pairs"] == 6 and f["pairs_per_wg"] == 4 and f["grid"] == 2
    assert _lib.score_mine_between_form(300, 200, 2, 32, 5)["grid"] == 2
    lib_env("DL_MINE_TILES")
    assert _lib.score_links_between_form(300, 200, 2, 32)["pairs_per_wg"] == 1


def test_sizers_and_forms_refuse_what_is_out_of_range():
    from disenlink_amd import _lib
    lib = _lib.load()
    for bad in ((0, 5, 2, 8), (5, 0, 2, 8), (-1, 5, 2, 8), (46341, 5, 2, 8), (5, 46341, 2, 8), (5, 5, 0, 8), (5, 5, 65, 8),
                (5, 5, 2, 0), (5, 5, 2, 129)):
        assert int(lib.dl_score_mine_between_workspace_bytes_dtype(*bad, 0, 5)) == 0
        assert int(lib.dl_score_links_between_workspace_bytes_dtype(*bad, 0)) == 0
        with pytest.raises(_lib.DisenlinkHipError):
            _lib.score_mine_between_form(*bad, 5)
        with pytest.raises(_lib.DisenlinkHipError):
            _lib.score_links_between_form(*bad)
    assert int(lib.dl_score_mine_between_workspace_bytes_dtype(5, 5, 2, 8, 7, 5)) == 0           # unknown dtype
    assert int(lib.dl_score_links_between_workspace_bytes_dtype(5, 5, 2, 8, 7)) == 0
    for m in (0, 65537):
        assert int(lib.dl_score_mine_between_workspace_bytes_dtype(5, 5, 2, 8, 0, m)) == 0
        with pytest.raises(_lib.DisenlinkHipError, match="outside 1..65536"):
            _lib.score_mine_between_form(5, 5, 2, 8, m)


def _calls(lib, nA=8, nB=6, K=2, d=8, dt=0, t=1.0, ZA=256, HA=256, ZB=256, HB=256, exr=None, exc=None, nf=None, ws=256,
           ws_bytes=1 << 30, m=5, out=256, count=256, rpa=256, rpb=256, nnz_a=0, nnz_b=0, col_a=256, logit_a=256, prob_a=None,
           col_b=256, logit_b=256, prob_b=None):
    """the three entries with dummy non-NULL pointers: a refusal returns before the first launch"""
    head = (ZA, HA, nA, ZB, HB, nB, K, d, dt, t, exr, exc, 0.0)
    links = head + (nf, ws, ws_bytes, rpa, rpb)
    return {"mine": lambda: lib.dl_score_mine_between_dtype(*head, m, out, out, out, out, count, ws, ws_bytes, None, nf),
            "count": lambda: lib.dl_score_links_between_count_dtype(*links, None),
            "fill": lambda: lib.dl_score_links_between_fill_dtype(*links, nnz_a, col_a, logit_a, prob_a, nnz_b, col_b, logit_b,
                                                                  prob_b, None)}


def test_c_abi_refusals():
    from disenlink_amd import _lib
    lib = _lib.load()
    p = 256
    NFB = _lib.DlNodeFilterBetween
    refused = [(dict(dt=7), b"unknown dtype"), (dict(d=130), b"1 <= d <= 128"), (dict(d=0), None), (dict(K=0), None),
               (dict(K=65), None), (dict(nA=0), b"nA=0 outside 1..46340"), (dict(nA=46341), b"nA=46341 outside 1..46340"),
               (dict(nB=0), b"nB=0 outside 1..46340"), (dict(nB=-2), b"nB=-2 outside 1..46340"),
               (dict(nB=46341), b"nB=46341 outside 1..46340"), (dict(t=0.0), b"temperature is 0"),
               (dict(ZA=None), b"NULL argument"), (dict(HA=None), b"NULL argument"), (dict(ZB=None), b"NULL argument"),
               (dict(HB=None), b"NULL argument"), (dict(exr=p), b"go together"), (dict(exc=p), b"go together"),
               (dict(nf=C.byref(NFB(p, p, 0, p))), b"n_groups=0 outside 1..64"),
               (dict(nf=C.byref(NFB(p, p, 65, p))), b"n_groups=65 outside 1..64"),
               (dict(nf=C.byref(NFB(None, p, 2, p))), b"NULL group or allow"),
               (dict(nf=C.byref(NFB(p, None, 2, p))), b"NULL group or allow"),
               (dict(nf=C.byref(NFB(p, p, 2, None))), b"NULL group or allow")]
    for kw, msg in refused:
        for name, call in _calls(lib, **kw).items():
            assert call() == -1, (name, kw)                           # DL_E_ARG
            assert msg is None or msg in lib.dl_last_error(), (name, kw, lib.dl_last_error())
    _calls(lib, nA=46341)["count"]()
    assert b"the pair index a nB + b must fit 31 bits" in lib.dl_last_error()
    # what only one of them takes
    for m in (0, 65537):
        assert _calls(lib, m=m)["mine"]() == -1 and b"outside 1..65536" in lib.dl_last_error()
    assert _calls(lib, out=None)["mine"]() == -1 and b"NULL output" in lib.dl_last_error()
    assert _calls(lib, count=None)["mine"]() == -1 and b"NULL output" in lib.dl_last_error()
    for kw in (dict(rpa=None), dict(rpb=None)):
        for name in ("count", "fill"):
            assert _calls(lib, **kw)[name]() == -1 and b"NULL argument" in lib.dl_last_error()
    # the workspace: DL_E_WORKSPACE, with the sizer's name
    need = {"mine": int(lib.dl_score_mine_between_workspace_bytes_dtype(8, 6, 2, 8, 0, 5)),
            "count": int(lib.dl_score_links_between_workspace_bytes_dtype(8, 6, 2, 8, 0))}
    need["fill"] = need["count"]
    for name in need:
        for kw in (dict(ws=None), dict(ws_bytes=need[name] - 1), dict(ws_bytes=0)):
            assert _calls(lib, **kw)[name]() == -3, (name, kw)
            assert b"workspace too small" in lib.dl_last_error() and b"_between_workspace_bytes_dtype" in lib.dl_last_error()
    fill = lambda **kw: _calls(lib, ws_bytes=need["fill"], **kw)["fill"]()
    assert fill(nnz_a=-1) == -1 and b"nnz=-1 is negative" in lib.dl_last_error()
    assert fill(nnz_b=-4) == -1 and b"nnz=-4 is negative" in lib.dl_last_error()
    for kw in (dict(nnz_a=5, col_a=None), dict(nnz_a=5, logit_a=None), dict(nnz_b=5, col_b=None), dict(nnz_b=5, logit_b=None)):
        assert fill(**kw) == -1 and b"NULL output" in lib.dl_last_error()
    assert fill(nnz_a=5, nnz_b=5, prob_a=p) == -1 and b"prob_a and prob_b go together" in lib.dl_last_error()
    assert fill(nnz_a=-1, nf=C.byref(NFB(p, p, 64, p))) == -1 and b"nnz=-1" in lib.dl_last_error()          # a good rule passes


def test_header_and_binding_list_the_entries():
    import test_host_cpu
    from disenlink_amd import _lib
    names = test_host_cpu._declared_symbols()
    want = ["dl_score_mine_between_form", "dl_score_mine_between_workspace_bytes_dtype", "dl_score_mine_between_dtype",
            "dl_score_links_between_form", "dl_score_links_between_workspace_bytes_dtype", "dl_score_links_between_count_dtype",
            "dl_score_links_between_fill_dtype"]
    assert sorted(n for n in names if "_between" in n) == sorted(want) == sorted(n for n in _lib.EXPORTS if "_between" in n)
    count, fill = _lib.EXPORTS["dl_score_links_between_count_dtype"][1], _lib.EXPORTS["dl_score_links_between_fill_dtype"][1]
    assert fill[:len(count) - 1] == count[:-1] and fill[-1] is count[-1]           # the same arguments, then the two sides
    # the unchanged caps of the triangular scans
    from disenlink_amd import ops
    assert ops.LINKS_MAX_N == ops.MINE_MAX_N == ops.BETWEEN_MAX_N == 46340 and ops.BLOCK_NODES == 46208 == 361 * 128


# ---------------------------------------------------------------------- the call path, against a recording stand-in
@pytest.fixture
def rec(monkeypatch):
    from disenlink_amd import _lib, scans
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(scans, "_need_cuda", lambda *tensors: None)
    monkeypatch.setattr(scans, "_stream", lambda: 0)
    monkeypatch.setattr(scans, "_empty", lambda shape, dtype, device: torch.zeros(shape, dtype=dtype, device=device))
    return r


def check_calls(rec, want_entries, want_dt, shapes):
    """every call is a _dtype entry of EXPORTS with a well-typed argument list; the non-sizer calls are ``want_entries``"""
    from disenlink_amd import _lib
    calls = [c for c in rec.calls if c[0] != QUERY]
    assert [n for n, _ in calls if "_workspace_bytes" not in n] == want_entries
    for entry, args in calls:
        assert entry.endswith("_dtype"), entry
        codes = _lib.EXPORTS[entry][1]
        assert len(args) == len(codes), entry
        for c, a in zip(codes, args):
            if c is _lib._NFB:
                assert a is None or type(a).__name__ == "CArgObject", entry
            else:
                assert fits(c, a), (entry, c, a)
        sizer, between = "_workspace_bytes" in entry, "_between" in entry
        assert args[(4 if between else 3) if sizer else (8 if between else 5)] == want_dt, entry
    return [c for c in calls if "_workspace_bytes" not in c[0]]


@pytest.mark.parametrize("table_dtype", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
@pytest.mark.parametrize("ruled", (False, True))
def test_between_calls_are_the_new_dtype_entries(rec, table_dtype, ruled):
    from disenlink_amd import _lib, scans
    g = torch.Generator().manual_seed(2)
    ZA, HA, ZB, HB = (torch.randn(n, 2, 8, generator=g) for n in (9, 9, 5, 5))
    kw = dict(table_dtype=table_dtype, exclude=(torch.tensor([0, 8]), torch.tensor([4, 0])))
    if ruled:
        kw["rule"] = (torch.arange(9) % 3, torch.arange(5) % 2, torch.tensor([[1, 0], [0, 1], [1, 1]]))
    dt = _lib.DL_F32 if table_dtype is torch.float32 else _lib.DL_BF16
    scans.score_mine_between(ZA, HA, ZB, HB, 1.0, 16, **kw)
    (name, args), = check_calls(rec, ["dl_score_mine_between_dtype"], dt, None)
    assert (args[2], args[5], args[6], args[7]) == (9, 5, 2, 8) and (args[-1] is None) == (not ruled)
    rec.calls.clear()
    out = scans.score_links_between(ZA, HA, ZB, HB, 1.0, 0.0, **kw)
    (_, count), (_, fill) = check_calls(rec, ["dl_score_links_between_count_dtype", "dl_score_links_between_fill_dtype"], dt, None)
    assert fill[:18] == count[:18] and fill[18] == 0 and fill[22] == 0 and (count[13] is None) == (not ruled)
    assert out.ab[0].numel() == 10 and out.ba[0].numel() == 6


@pytest.mark.parametrize("table_dtype", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
@pytest.mark.parametrize("filtered", (False, True))
def test_blocks_make_the_old_entries_on_the_diagonal_and_the_new_ones_off_it(rec, table_dtype, filtered):
    from disenlink_amd import _lib, scans
    N = 300                                                           # blocks of 128: 128, 128, 44 rows
    g = torch.Generator().manual_seed(2)
    Z, H = torch.randn(N, 2, 8, generator=g), torch.randn(N, 2, 8, generator=g)
    kw = dict(table_dtype=table_dtype, exclude=(torch.tensor([0, 130, 5]), torch.tensor([129, 299, 7])), block_nodes=128)
    if filtered:
        kw["node_filter"] = scans.NodeFilter.same(torch.arange(N) % 3)
    dt = _lib.DL_F32 if table_dtype is torch.float32 else _lib.DL_BF16
    sizes = [128, 128, 44]
    windows = [(i, j) for i in range(3) for j in range(i, 3)]
    scans.score_mine_blocks(Z, H, 1.0, 16, **kw)
    calls = check_calls(rec, ["dl_score_mine_dtype" if i == j else "dl_score_mine_between_dtype" for i, j in windows], dt, None)
    item = Z.element_size() if table_dtype is torch.float32 else 2
    for (i, j), (name, args) in zip(windows, calls):
        if i == j:
            assert args[2] == sizes[i] and (args[-1] is None) == (not filtered)
            assert (args[7] is None) == (i != 0)                      # (5, 7) lies in block 0; the other two pairs cross a border
        else:
            assert (args[2], args[5]) == (sizes[i], sizes[j]) and (args[-1] is None) == (not filtered)
            assert (args[10] is None) == ((i, j) == (0, 2))
            assert args[3] - args[0] == (j - i) * 128 * 2 * 8 * item  # row slices of ONE table
    rec.calls.clear()
    scans.score_links_blocks(Z, H, 1.0, 0.0, **kw)
    want = []
    for i, j in windows:
        want += ["dl_score_links_count_dtype", "dl_score_links_fill_dtype"] if i == j else \
            ["dl_score_links_between_count_dtype", "dl_score_links_between_fill_dtype"]
    check_calls(rec, want, dt, None)
    rec.calls.clear()
    deg = scans.score_link_degrees_blocks(Z, H, 1.0, 0.0, **kw)
    check_calls(rec, [w for w in want if "count" in w], dt, None)
    assert deg.shape == (N,) and deg.dtype == torch.int64


def test_python_refusals_before_any_launch():
    from disenlink_amd import ops
    Z = torch.zeros(6, 2, 8)
    for bad in (100, 0, 127, 46336, 46208 + 128):
        with pytest.raises(ValueError, match="multiple of 128"):
            ops.score_mine_blocks(Z, Z, 1.0, 5, block_nodes=bad)
    with pytest.raises(ValueError, match="outside 1..65536"):
        ops.score_mine_blocks(Z, Z, 1.0, 0, block_nodes=128)
    asym = ops.NodeFilter(torch.tensor([0, 1, 0, 1, 0, 1]), torch.tensor([[0, 1], [0, 0]]))
    for call in (lambda: ops.score_mine_blocks(Z, Z, 1.0, 5, node_filter=asym),
                 lambda: ops.score_links_blocks(Z, Z, 1.0, 0.0, node_filter=asym),
                 lambda: ops.score_link_degrees_blocks(Z, Z, 1.0, 0.0, node_filter=asym)):
        with pytest.raises(ValueError, match="symmetric"):
            call()
    with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
        ops.score_mine_blocks(Z, Z, 1.0, 5)
    with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
        ops.score_mine_between(Z, Z, Z[:3], Z[:3], 1.0, 5)
    with pytest.raises(ValueError, match="K and d must agree"):
        ops.score_mine_between(Z, Z, torch.zeros(3, 2, 4), torch.zeros(3, 2, 4), 1.0, 5)
    with pytest.raises(ValueError, match=r"outside \[0, 6\) x \[0, 3\)"):
        ops.bipartite_exclusion_csr((torch.tensor([0]), torch.tensor([3])), 6, 3)
    with pytest.raises(ValueError, match=r"\[nA, nB\] = \[6, 3\]"):
        ops.bipartite_exclusion_csr(torch.zeros(3, 6), 6, 3)
    rp, col = ops.bipartite_exclusion_csr((torch.tensor([4, 0, 4, 4]), torch.tensor([2, 1, 0, 2])), 6, 3)
    assert rp.tolist() == [0, 1, 1, 1, 1, 3, 3] and col.tolist() == [1, 0, 2] and rp.dtype == col.dtype == torch.int32
    for rule, msg in (((torch.zeros(6), torch.zeros(3), torch.ones(1, 1)), "groups_a must be"),
                      ((torch.zeros(5, dtype=torch.long), torch.zeros(3, dtype=torch.long), torch.ones(1, 1)), "groups_a must be"),
                      ((torch.zeros(6, dtype=torch.long), torch.ones(3, dtype=torch.long), torch.ones(2, 1)), r"groups_b outside \[0, 1\)"),
                      ((torch.zeros(6, dtype=torch.long), torch.zeros(3, dtype=torch.long), torch.ones(65, 1)), "1 <= g, h <= 64")):
        with pytest.raises(ValueError, match=msg):
            ops.score_mine_between(Z, Z, Z[:3], Z[:3], 1.0, 5, rule=rule)


# ---------------------------------------------------------------------- the driver, with between_ref for the kernels
@pytest.fixture
def fake(monkeypatch):
    from disenlink_amd import _lib, scans

    def install(S):
        f = between_ref.FakeScans(S)
        monkeypatch.setattr(_lib, "load", lambda: f)
        monkeypatch.setattr(scans, "_need_cuda", lambda *tensors: None)
        monkeypatch.setattr(scans, "_stream", lambda: 0)
        return f
    return install


def graph_case(N, seed):
    """small-integer logits, so that ties run across every window; a NaN row, a +inf and a -0; an exclusion set whose pairs
    cross block borders at 128, 256 and 384; the tables carry the node ids (between_ref.FakeScans)"""
    g = torch.Generator().manual_seed(seed)
    S = torch.randint(-3, 4, (N, N), generator=g).float()
    if N > 2:
        S[N // 2, :] = float("nan")
        S[:, N // 2] = float("nan")
        S[0, N - 1] = INF
        S[1, 2] = -0.0
    ids = torch.arange(N, dtype=torch.float32).reshape(N, 1, 1)
    ex = torch.zeros(N, N, dtype=torch.bool)
    if N > 1:
        a, b = torch.randint(0, N, (4 * N,), generator=g), torch.randint(0, N, (4 * N,), generator=g)
        ex[a, b] = True
        for u, v in ((0, 1), (127, 128), (128, 127), (0, 255), (255, 256), (130, 390), (383, 384), (5, 699)):
            if max(u, v) < N:
                ex[u, v] = True
    return S, ids, ex


@pytest.mark.parametrize("N,block", list(itertools.product((1, 2, 129, 300, 700), (128, 256, 384))))
def test_block_driver_merge_and_assembly_against_a_brute_force(fake, N, block):
    from disenlink_amd import ops
    S, ids, ex = graph_case(N, seed=N + block)
    f = fake(S)
    sym = ex | ex.T
    groups = torch.arange(N) % 3
    nf = ops.NodeFilter.different(groups)
    allowed = groups[:, None] != groups[None, :]
    all_pairs = N * (N - 1) // 2
    for floor, m, filt in ((-INF, 50, None), (1.0, 7, None), (-INF, min(all_pairs + 5, 65536), None), (3.5, 20, None), (0.0, 300, nf), (INF, 3, None)):
        f.calls.clear()
        excl = sym if filt is None else (sym | ~allowed)
        src, dst, logit, _ = ops.score_mine_blocks(ids, ids, 1.0, max(m, 1), exclude=ex, min_logit=floor, node_filter=filt,
                                                   block_nodes=block)
        u, v, x = mine_ref.select_top(S, max(m, 1), excl, floor)
        x = torch.where(x == 0, torch.zeros_like(x), x)
        assert src.dtype == dst.dtype == torch.int32
        assert torch.equal(src.long(), u) and torch.equal(dst.long(), v), (floor, m)
        assert torch.equal(logit.view(torch.int32), x.view(torch.int32))
        nb = -(-N // block)
        assert len([c for c in f.calls if c[0] in ("dl_score_mine_dtype", "dl_score_mine_between_dtype")]) == nb * (nb + 1) // 2
    for floor, filt in ((-INF, None), (2.0, None), (0.0, nf), (3.5, None), (INF, None)):
        excl = sym if filt is None else (sym | ~allowed)
        rowptr, col, logit, prob = ops.score_links_blocks(ids, ids, 1.0, floor, exclude=ex, node_filter=filt, block_nodes=block)
        rp, c, x = links_ref.select_links(S, excl, floor)
        assert rowptr.dtype == torch.int64 and col.dtype == torch.int32
        assert torch.equal(rowptr, rp) and torch.equal(col.long(), c)
        assert torch.equal(logit.view(torch.int32), x.view(torch.int32)) and not torch.isnan(prob).any()
        deg = ops.score_link_degrees_blocks(ids, ids, 1.0, floor, exclude=ex, node_filter=filt, block_nodes=block)
        assert torch.equal(deg, rp[1:] - rp[:-1])


def test_the_floor_handed_to_later_windows_is_inclusive(fake):
    """every logit is 1: the list is full after the first window, and the windows after it are asked for logit >= 1 — they
    still return their ties, and the merge cuts by the 64-bit global index, so the result is the first m pairs of the graph"""
    from disenlink_amd import ops
    N = 300
    S = torch.ones(N, N)
    f = fake(S)
    ids = torch.arange(N, dtype=torch.float32).reshape(N, 1, 1)
    src, dst, logit, _ = ops.score_mine_blocks(ids, ids, 1.0, 400, block_nodes=128)
    u, v = torch.triu_indices(N, N, 1)
    assert torch.equal(src.long(), u[:400]) and torch.equal(dst.long(), v[:400])       # (0, 1) .. (0, 299), (1, 2) ...: three windows
    floors = [c[1][9] if c[0] == "dl_score_mine_dtype" else c[1][12] for c in f.calls if c[0].startswith("dl_score_mine") and
              "workspace" not in c[0]]
    assert floors[0] == -INF and floors[1:] == [1.0] * 5


def test_rectangle_reference_on_a_hand_made_matrix():
    NAN = float("nan")
    S = torch.tensor([[1.5, -0.0, INF], [NAN, 1.5, -2.0]])
    a, b, x = between_ref.select_top_between(S, 10)
    assert list(zip(a.tolist(), b.tolist())) == [(0, 2), (0, 0), (1, 1), (0, 1), (1, 2)] and not torch.signbit(x[3])
    a, b, _ = between_ref.select_top_between(S, 10, min_logit=0.0, allowed=between_ref.rule_mask([0, 1], [1, 0, 1], [[0, 1], [1, 0]]))
    assert list(zip(a.tolist(), b.tolist())) == [(0, 2), (0, 0), (1, 1)]
    ab, ba = between_ref.select_links_between(S, torch.tensor([[0, 0, 1], [0, 0, 0]]), None, 0.0)
    assert ab[0].tolist() == [0, 2, 3] and ab[1].tolist() == [0, 1, 1] and ba[0].tolist() == [0, 1, 3, 3] and ba[1].tolist() == [0, 0, 1]
    assert ab[2].tolist() == [1.5, 0.0, 1.5] and ba[2].tolist() == [1.5, 0.0, 1.5]


def test_cli_and_model_take_the_blocked_route():
    import inspect
    from disenlink_amd.main import build_parser
    from disenlink_amd.model import Disentangle
    text = " ".join(build_parser().format_help().split())
    assert "blocks of 46208" in text
    for name in ("top_missing_links", "predicted_links"):
        assert inspect.signature(getattr(Disentangle, name)).parameters["block_nodes"].default is None
        assert "N <= 46,340" not in getattr(Disentangle, name).__doc__
