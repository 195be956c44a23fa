"""The all-pairs scans over bf16 tables (``table_dtype=torch.bfloat16``; dl_score_*_dtype with DL_BF16: one bf16 plane per
operand, one matrix-core product per block) against the fp32 entries on the same tables widened to fp32.

The oracle is a bit contract, not a tolerance.  A bf16 value x splits into hi = x, mid = lo = 0, so five of the six products
of the fp32 scan add exact zeros to an accumulator that starts at +0 and cannot change it; the sixth is the one product of
the bf16 scan, and everything behind the products is the same code.  So indices, logits, probabilities, counts, rowptr / col,
the candidate counter and the padding are compared with torch.equal on bit patterns."""
import itertools

import numpy as np
import pytest
import torch

from mine_ref import logits64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")
BF16 = torch.bfloat16

# the smallest shapes at which tiling, padding and the step count can go wrong: one tile, a tile edge on either side, three
# tiles (diagonal and off-diagonal tile pairs); d padded to 32 and 1..4 column chunks
N_VALUES = (1, 127, 129, 300)
KD_VALUES = ((1, 8), (3, 33), (8, 64), (2, 96), (3, 128))
T_VALUES = (1, 2)
CASES = list(itertools.product(N_VALUES, KD_VALUES, T_VALUES))


def tables(N, K, d, seed=0, scale=1.0):
    """fp32 tables as test_gpu_mine.py draws them (not bf16-exact)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (torch.randn(N, K, d, generator=g) * scale / d ** 0.5).to(DEV)
    H = (torch.randn(N, K, d, generator=g) / d ** 0.5).to(DEV)
    return Z, H


def bf16_tables(N, K, d, seed=0, scale=1.0):
    """drawn in fp32 and rounded once: -> (Zb, Hb) bf16 and their widened fp32 images"""
    Z, H = tables(N, K, d, seed, scale)
    Zb, Hb = Z.bfloat16(), H.bfloat16()
    return Zb, Hb, Zb.float(), Hb.float()


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def filters(N):
    """a symmetric rule for the unordered scans, an asymmetric one for top-k / ranks"""
    from disenlink_amd import ops
    groups = torch.arange(N, device=DEV) % 3
    sym = ops.NodeFilter.different(groups, device=DEV) if N >= 3 else ops.NodeFilter(groups, torch.ones(3, 3), device=DEV)
    asym = ops.NodeFilter(groups, torch.tensor([[1, 1, 0], [0, 1, 1], [1, 0, 1]]), device=DEV)
    assert sym.symmetric and not asym.symmetric
    return sym, asym


def exclusion(N):
    """a few pairs, one listed in both orientations, one a self pair (excludes nothing in the unordered scans)"""
    a = torch.tensor([0, min(3, N - 1), N - 1, 0, N // 2], device=DEV)
    b = torch.tensor([min(2, N - 1), min(1, N - 1), 0, N - 1, N // 2], device=DEV)
    return a, b


def run_family(ops, Z, H, t, N, seed, **kw):
    """Every scan of the family on (Z, H), with and without a node filter -> a flat list of tensors.  ``kw`` is either empty
    (the fp32 entries) or table_dtype=torch.bfloat16; everything else is the same on both sides."""
    sym, asym = filters(N)
    ex = exclusion(N)
    rng = np.random.default_rng(seed)
    q_all = torch.arange(N, device=DEV)
    out = []
    # top-k: several k, exclude_self on and off, an exclusion set, the asymmetric rule
    for k, es in ((1, True), (7, False), (128, True)):
        out += ops.score_topk(Z, H, t, q_all, k, exclude_self=es, **kw)
    out += ops.score_topk(Z, H, t, q_all[::3], 16, exclude=ex, **kw)
    out += ops.score_topk(Z, H, t, q_all, 9, exclude=ex, node_filter=asym, **kw)
    # ranks of target pairs per query (duplicates and an excluded target among them)
    T = min(4 * N, 200)
    src = torch.from_numpy(rng.integers(0, N, T)).to(DEV)
    dst = torch.from_numpy(rng.integers(0, N, T)).to(DEV)
    src[0], dst[0] = ex[0][0], ex[1][0]
    for nf in (None, asym):
        out += ops.score_ranks(Z, H, t, src, dst, exclude=ex, node_filter=nf, **kw)
    # global top-m: m below, at and above the eligible count, and a floor
    for nf in (None, sym):
        full = ops.score_mine(Z.float(), H.float(), t, 65536, exclude=ex, node_filter=nf)      # eligible count of THIS rule (fp32 call)
        elig = len(full[0])
        for m in sorted({max(1, elig - 1), max(1, elig), min(65536, elig + 5)}):
            out += ops.score_mine(Z, H, t, m, exclude=ex, node_filter=nf, **kw)
        out += ops.score_mine(Z, H, t, 50, exclude=ex, min_logit=0.0, node_filter=nf, **kw)
    # global pair ranks: targets including an excluded pair and duplicates; n_others and the candidate counter
    if N >= 2:
        keep = src != dst
        ps, pd = src[keep], dst[keep]
        ps = torch.cat([ps, ps[:3], torch.tensor([0], device=DEV)])
        pd = torch.cat([pd, pd[:3], torch.tensor([min(2, N - 1)], device=DEV)])      # (0, 2): excluded for N >= 3
        for nf in (None, sym):
            out += ops.score_pair_ranks_counted(Z, H, t, ps, pd, exclude=ex, node_filter=nf, **kw)
    # the link graph at two floors, and the degrees alone
    for nf in (None, sym):
        for floor in (NINF, 0.0):
            out += ops.score_links(Z, H, t, floor, exclude=ex, node_filter=nf, **kw)
        out.append(ops.score_link_degrees(Z, H, t, 0.0, exclude=ex, node_filter=nf, **kw))
    return out


@pytest.mark.parametrize("N,KD,t", CASES)
def test_bf16_tables_give_the_bits_of_the_fp32_entries_on_the_widened_tables(N, KD, t):
    from disenlink_amd import ops
    K, d = KD
    seed = N * 131 + K * 7 + d + t
    Zb, Hb, Zw, Hw = bf16_tables(N, K, d, seed)
    want = run_family(ops, Zw, Hw, t, N, seed)
    got = run_family(ops, Zb, Hb, t, N, seed, table_dtype=BF16)
    assert len(want) == len(got) > 40
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b)), (i, a.shape, a.dtype)
    assert any(x.numel() and x.dtype == torch.float32 for x in got)


@pytest.mark.parametrize("N,KD,t", [(129, (3, 33), 2), (300, (8, 64), 1)])
def test_fp32_tables_are_rounded_inside_the_call(N, KD, t):
    from disenlink_amd import ops
    K, d = KD
    Z, H = tables(N, K, d, seed=5 + N)
    assert not torch.equal(Z, Z.bfloat16().float())                  # not bf16-exact
    want = run_family(ops, Z.bfloat16().float(), H.bfloat16().float(), t, N, 5)
    got = run_family(ops, Z, H, t, N, 5, table_dtype=BF16)
    assert same(want, got)
    # the mode is not a no-op: on the same tables the plain fp32 call forms other logits
    a = torch.arange(N - 1, device=DEV)
    plain = ops.score_pair_logits(Z, H, t, a, a + 1)
    rounded = ops.score_pair_logits(Z, H, t, a, a + 1, table_dtype=BF16)
    assert torch.equal(bits(rounded), bits(ops.score_pair_logits(Z.bfloat16().float(), H.bfloat16().float(), t, a, a + 1)))
    assert not torch.equal(bits(plain), bits(rounded))


def test_overflow_inf_first_nan_never_selected_nan_counted():
    from disenlink_amd import ops
    N, d = 90, 32
    Z, H = tables(N, 1, d, seed=7)
    Z[:45] = 4.0                                                      # z.z = 512: exp overflows (all bf16-exact values)
    H[:20] = 0.25                                                     # h.h > 0: +inf
    H[20:30] = 0.25
    H[20:30, :, ::2] = -0.5                                           # against rows 0..19: h.h < 0: -inf
    H[30:45] = 0.0                                                    # h.h = 0 against inf: NaN
    Zb, Hb = Z.bfloat16(), H.bfloat16()
    Zw, Hw = Zb.float(), Hb.float()
    q = torch.arange(N, device=DEV)
    total = N * (N - 1) // 2
    for kw, (Zc, Hc) in (({}, (Zw, Hw)), ({"table_dtype": BF16}, (Zb, Hb))):
        idx, logit, prob = ops.score_topk(Zc, Hc, 1.0, q, 128, **kw)
        assert (logit[0, :19] == float("inf")).all() and torch.isnan(logit[0, -15:]).all()      # +inf first, NaN last
        src, dst, lg, pr = ops.score_mine(Zc, Hc, 1.0, total + 3, **kw)
        assert not torch.isnan(lg).any() and lg[0] == float("inf") and lg[-1] == NINF and len(src) < total
        counted = ops.score_pair_ranks_counted(Zc, Hc, 1.0, q[:-1], q[1:], **kw)[4]
        assert int(counted) == total                                  # NaN logits are counted as candidates
    want = run_family(ops, Zw, Hw, 1.0, N, 7)
    got = run_family(ops, Zb, Hb, 1.0, N, 7, table_dtype=BF16)
    assert same(want, got)
    assert any(x.dtype == torch.float32 and torch.isinf(x).any() for x in got)
    assert any(x.dtype == torch.float32 and torch.isnan(x).any() for x in got)


def test_same_bits_under_any_geometry_and_on_every_call(lib_env):
    from disenlink_amd import ops
    N, K, d, t = 300, 3, 33, 2
    Zb, Hb, Zw, Hw = bf16_tables(N, K, d, seed=13)
    ref = run_family(ops, Zb, Hb, t, N, 13, table_dtype=BF16)
    assert same(ref, run_family(ops, Zb, Hb, t, N, 13, table_dtype=BF16))      # two calls in a row
    for slices, tiles in ((1, 1), (3, 6)):                           # DL_RANK_SLICES, DL_MINE_TILES (6 = all tile pairs)
        lib_env("DL_RANK_SLICES", slices)
        lib_env("DL_MINE_TILES", tiles)
        assert same(ref, run_family(ops, Zb, Hb, t, N, 13, table_dtype=BF16))
    assert same(ref, run_family(ops, Zw, Hw, t, N, 13))               # ... and they are the fp32 bits, under this geometry too


GUARD = 4096


def _guarded_ws(need, poison):
    """a workspace of exactly ``need`` bytes behind a 256-byte aligned start, poisoned, with a guard region behind it"""
    buf = torch.full((need + GUARD + 256,), poison, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 256
    return buf, buf[off:off + need], buf[off + need:off + need + GUARD]


def _raw_mine(lib, Zc, Hc, dt, t, m, need, poison, ws_bytes=None):
    from disenlink_amd import ops
    N, K, d = Zc.shape
    buf, ws, guard = _guarded_ws(need, poison)
    outs = [torch.full((4 * m,), poison, dtype=torch.uint8, device=DEV).view(ty)
            for ty in (torch.int32, torch.int32, torch.float32, torch.float32)]
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    rc = lib.dl_score_mine_dtype(Zc.data_ptr(), Hc.data_ptr(), N, K, d, dt, float(t), None, None, NINF, m,
                                 *[o.data_ptr() for o in outs], count.data_ptr(), ws.data_ptr(),
                                 need if ws_bytes is None else ws_bytes, ops._stream(), None)
    torch.cuda.synchronize()
    return rc, outs + [count], guard


def test_tight_poisoned_workspace_with_a_guard_behind_it():
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    N, K, d, t, m = 129, 3, 33, 1.0, 40
    Zb, Hb, Zw, Hw = bf16_tables(N, K, d, seed=17)
    need = int(lib.dl_score_mine_workspace_bytes_dtype(N, K, d, _lib.DL_BF16, m))
    assert 0 < need < int(lib.dl_score_mine_workspace_bytes(N, K, d, m))
    want = ops.score_mine(Zw, Hw, t, m)
    results = []
    for poison in (0xFF, 0x7F):                                       # NaN patterns of either sign in everything unwritten
        rc, outs, guard = _raw_mine(lib, Zb, Hb, _lib.DL_BF16, t, m, need, poison)
        assert rc == 0 and int(outs[4]) == m and (guard == poison).all()
        assert same(want, outs[:4])
        results.append(outs)
    assert same(results[0], results[1])
    # top-k and the link graph the same way (their workspaces hold the gathered query plane / the cells as well)
    q = torch.arange(N, device=DEV, dtype=torch.int32)
    k = 5
    need = int(lib.dl_score_topk_workspace_bytes_dtype(N, K, d, _lib.DL_BF16, N, k, 0))
    buf, ws, guard = _guarded_ws(need, 0xFF)
    index = torch.full((N, k), -7, dtype=torch.int64, device=DEV)
    logit = torch.full((N * k * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32).view(N, k)
    prob = logit.clone()
    rc = lib.dl_score_topk_dtype(Zb.data_ptr(), Hb.data_ptr(), N, K, d, _lib.DL_BF16, t, q.data_ptr(), N, k, None, None, 1,
                                 index.data_ptr(), logit.data_ptr(), prob.data_ptr(), ws.data_ptr(), need, ops._stream(), None)
    torch.cuda.synchronize()
    assert rc == 0 and (guard == 0xFF).all() and same(ops.score_topk(Zw, Hw, t, q, k), (index, logit, prob))
    need = int(lib.dl_score_links_workspace_bytes_dtype(N, K, d, _lib.DL_BF16))
    buf, ws, guard = _guarded_ws(need, 0xFF)
    rowptr = torch.full((N + 1,), -7, dtype=torch.int64, device=DEV)
    head = (Zb.data_ptr(), Hb.data_ptr(), N, K, d, _lib.DL_BF16, t, None, None, 0.0, None, ws.data_ptr(), need, rowptr.data_ptr())
    assert lib.dl_score_links_count_dtype(*head, ops._stream()) == 0
    nnz = int(rowptr[-1])
    col = torch.full((nnz,), -7, dtype=torch.int32, device=DEV)
    lg = torch.full((nnz * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32)
    pr = lg.clone()
    assert lib.dl_score_links_fill_dtype(*head, nnz, col.data_ptr(), lg.data_ptr(), pr.data_ptr(), ops._stream()) == 0
    torch.cuda.synchronize()
    assert (guard == 0xFF).all() and nnz > 0 and same(ops.score_links(Zw, Hw, t, 0.0), (rowptr, col, lg, pr))


@pytest.mark.parametrize("N,KD,t", [(129, (3, 33), 2), (300, (2, 96), 1), (300, (3, 128), 2)])
def test_logits_against_fp64_within_the_band_of_the_fp32_tests(N, KD, t):
    from disenlink_amd import ops
    K, d = KD
    Zb, Hb, Zw, Hw = bf16_tables(N, K, d, seed=23 + N + d)
    s64, band = logits64(Zw, Hw, t)                                   # 1e-5 * sum |addends| (mine_ref.py), on the widened tables
    u, v = torch.triu_indices(N, N, 1, device=DEV)
    got = ops.score_pair_logits(Zb, Hb, t, u, v, table_dtype=BF16).double()
    err = (got - s64[u, v]).abs()
    print(f"max err / band = {float((err / band[u, v]).max()):.3e}")
    assert (err <= band[u, v] + 1e-30).all()


def _small_graph(N, seed):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, N, 6 * N), rng.integers(0, N, 6 * N)
    adj = np.zeros((N, N), np.float32)
    adj[s, d] = 1
    np.fill_diagonal(adj, 0)
    return ((adj + adj.T) != 0).astype(np.float32)


def test_module_ranks_the_tables_its_bf16_training_step_gathers_from():
    from disenlink_amd.graph import Graph, PairList
    from disenlink_amd.model import Disentangle
    N, F, K, d = 150, 24, 4, 32
    torch.manual_seed(3)
    model = Disentangle(F, 32, d, nfactor=K, beta=0.6, t=1, table_dtype=BF16).to(DEV)
    adj = torch.from_numpy(_small_graph(N, 3)).to(DEV)
    x = (torch.randn(N, F, generator=torch.Generator().manual_seed(3)) * 0.3).to(DEV)
    graph = Graph.from_dense(adj)
    rng = np.random.default_rng(4)
    pu, pv = rng.integers(0, N, 400), rng.integers(0, N, 400)
    keep = pu != pv
    pu, pv = torch.from_numpy(pu[keep]).to(DEV), torch.from_numpy(pv[keep]).to(DEV)
    with torch.no_grad():
        _, prob = model.forward_pairs(x, graph, PairList.build(pu, pv, N))
    r = model.missing_link_ranks(x, graph, pu, pv, table_dtype=model.table_dtype)
    # both sides see identical bf16 tables; the tolerance of test_gpu_mine.py::test_top_missing_links_against_dropin_forward
    np.testing.assert_allclose(torch.sigmoid(r.logit.double()).cpu().numpy(), prob.double().cpu().numpy(), atol=1e-5, rtol=0)
    # table_dtype=None on that module: fp32 tables, as before this keyword existed
    today = model.top_missing_links(x, graph, 60)
    assert same(today, model.top_missing_links(x, graph, 60, table_dtype=None))
    Z, H = model._rank_tables(x, graph)
    assert Z.dtype == torch.float32 and H.dtype == torch.float32
    from disenlink_amd import ops
    assert same(today, ops.score_mine(Z, H, 1.0, 60, exclude=graph))
    Zb, Hb = model._rank_tables(x, graph, BF16)
    assert Zb.dtype == BF16 and Hb.dtype == BF16 and torch.equal(Zb, Z.bfloat16())
    mined = model.top_missing_links(x, graph, 60, table_dtype=BF16)
    assert same(mined, ops.score_mine(Zb.float(), Hb.float(), 1.0, 60, exclude=graph))
    for got in (model.topk_links(x, graph, torch.arange(5, device=DEV), 4, table_dtype=BF16),
                model.predicted_links(x, graph, 0.5, table_dtype=BF16)):
        assert all(torch.is_tensor(v) for v in got)
    g, ti = model.link_ranks(x, graph, pu[:20], pv[:20], table_dtype=BF16)
    assert same((g, ti), ops.score_ranks(Zb.float(), Hb.float(), 1.0, pu[:20], pv[:20]))


def test_argument_errors():
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    Zb, Hb, Zw, Hw = bf16_tables(10, 2, 32)
    q = torch.arange(10, device=DEV)
    for bad in (torch.float16, torch.float64, None, "bf16"):
        with pytest.raises(TypeError, match="table_dtype"):
            ops.score_mine(Zw, Hw, 1.0, 3, table_dtype=bad)
    calls = (lambda Z, H, **kw: ops.score_topk(Z, H, 1.0, q, 3, **kw),
             lambda Z, H, **kw: ops.score_ranks(Z, H, 1.0, q[:-1], q[1:], **kw),
             lambda Z, H, **kw: ops.score_mine(Z, H, 1.0, 3, **kw),
             lambda Z, H, **kw: ops.score_pair_ranks(Z, H, 1.0, q[:-1], q[1:], **kw),
             lambda Z, H, **kw: ops.score_pair_logits(Z, H, 1.0, q[:-1], q[1:], **kw),
             lambda Z, H, **kw: ops.score_links(Z, H, 1.0, 0.0, **kw),
             lambda Z, H, **kw: ops.score_link_degrees(Z, H, 1.0, 0.0, **kw))
    for call in calls:
        with pytest.raises(TypeError, match="fp32"):                  # bf16 tensors without the keyword: as before
            call(Zb, Hb)
        with pytest.raises(TypeError, match="both"):                  # mismatched Z / H types
            call(Zb, Hw, table_dtype=BF16)
        with pytest.raises(TypeError, match="both"):
            call(Zw.half(), Hw.half(), table_dtype=BF16)
    with pytest.raises(_lib.DisenlinkHipError, match="1 <= d <= 128"):
        ops.score_mine(torch.zeros(10, 1, 130, device=DEV, dtype=BF16), torch.zeros(10, 1, 130, device=DEV, dtype=BF16), 1.0, 3,
                       table_dtype=BF16)
    # the C entries: an unknown dtype is DL_E_ARG, a short workspace DL_E_WORKSPACE
    need = int(lib.dl_score_mine_workspace_bytes_dtype(10, 2, 32, _lib.DL_BF16, 3))
    rc, _, _ = _raw_mine(lib, Zb, Hb, 7, 1.0, 3, need, 0xFF)
    assert rc == -1 and b"unknown dtype" in lib.dl_last_error()
    rc, _, guard = _raw_mine(lib, Zb, Hb, _lib.DL_BF16, 1.0, 3, need, 0xFF, ws_bytes=need - 1)
    assert rc == -3 and b"workspace too small" in lib.dl_last_error() and (guard == 0xFF).all()
    assert lib.dl_score_mine_workspace_bytes_dtype(10, 2, 32, 7, 3) == 0
    assert lib.dl_score_scan_supported(2, 32, _lib.DL_BF16) == 1 and lib.dl_score_scan_supported(2, 32, 7) == 0
    assert lib.dl_score_scan_supported(2, 129, _lib.DL_BF16) == 0
