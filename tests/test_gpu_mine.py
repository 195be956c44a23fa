"""The graph's m most likely missing links (ops.score_mine, Disentangle.top_missing_links, --mine) against the fp64
reference of tests/mine_ref.py, the bits of the ranking scan, the drop-in forward and the CLI."""
import contextlib
import io

import numpy as np
import pytest
import torch

import mine_ref
from mine_ref import logits64, mine64, select_top

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")


def tables(N, K, d, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (torch.randn(N, K, d, generator=g) * scale / d ** 0.5).to(DEV)
    H = (torch.randn(N, K, d, generator=g) / d ** 0.5).to(DEV)
    return Z, H


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def assert_sorted_total_order(src, dst, logit, N):
    assert not torch.isnan(logit).any()
    v = logit.double()
    v = torch.where(v == 0, torch.zeros_like(v), v)
    pair = src.long() * N + dst.long()
    if len(v) > 1:
        assert ((v[:-1] > v[1:]) | ((v[:-1] == v[1:]) & (pair[:-1] < pair[1:]))).all()


def assert_valid_mine(out, s64, band, N, m, excluded=None, floor=NINF):
    """a valid global top-m of the fp64 logits within their error bands (assert_valid_topk of test_gpu_rank.py, across rows)"""
    src, dst, logit, prob = out
    assert src.dtype == torch.int32 and dst.dtype == torch.int32 and logit.dtype == torch.float32 and prob.dtype == torch.float32
    c = len(src)
    assert len(dst) == len(logit) == len(prob) == c
    cand = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    if excluded is not None:
        cand &= ~(excluded.bool() | excluded.bool().T)
    sure = cand & (s64 - band >= floor)                              # eligible whatever the rounding
    maybe = cand & (s64 + band >= floor)
    assert min(m, int(sure.sum())) <= c <= min(m, int(maybe.sum()))
    u, v = src.long(), dst.long()
    assert (u < v).all() and (u >= 0).all() and (v < N).all()
    assert maybe[u, v].all() and torch.unique(u * N + v).numel() == c
    assert_sorted_total_order(src, dst, logit, N)
    if c == 0:
        return
    assert (logit.double() - s64[u, v]).abs().le(band[u, v] + 1e-30).all()
    assert (logit >= floor).all()
    got = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    got[u, v] = True
    rest = sure & ~got
    if c < m:
        assert not rest.any()                                        # room left: nothing surely eligible is missing
    else:
        low = torch.argmin(s64[u, v])                                # no omitted candidate is provably above the last one
        assert (s64[rest] - band[rest] <= s64[u[low], v[low]] + band[u[low], v[low]]).all()
    ref = 1.0 / (1.0 + torch.exp(-logit.double()))
    np.testing.assert_allclose(prob.cpu().numpy(), ref.float().cpu().numpy(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("N,KD,t", mine_ref.GPU_CASES)
def test_valid_global_top_m(N, KD, t):
    from disenlink_amd import ops
    K, d = KD
    Z, H = tables(N, K, d, seed=N * 131 + K * 7 + d + t)
    s64, band = logits64(Z, H, t)
    for m in mine_ref.gpu_m_values(N):
        assert_valid_mine(ops.score_mine(Z, H, t, m), s64, band, N, m)
    # a floor at the fp64 median of the candidates: a condition on the seed, judged on the reference alone
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    floor = float(torch.median(s64[iu]))
    straddle = iu & (s64 - band < floor) & (s64 + band >= floor)
    assert int(straddle.sum()) <= max(1, int(0.01 * int(iu.sum())))
    for m in (7, N * (N - 1) // 2 + 5):
        assert_valid_mine(ops.score_mine(Z, H, t, m, min_logit=floor), s64, band, N, m, floor=floor)


@pytest.mark.parametrize("N", [5, 129])
def test_bits_of_the_ranking_scan(N):
    from disenlink_amd import ops
    K, d, t = 3, 40, 2.0
    Z, H = tables(N, K, d, seed=21 + N)
    ex = (torch.tensor([0, 3, N - 1], device=DEV), torch.tensor([2, 1, 0], device=DEV))
    for exclude in (None, ex):
        idx, logit, _ = ops.score_topk(Z, H, t, torch.arange(N, device=DEV), 128)      # every candidate of every query
        S = torch.full((N, N), float("nan"), device=DEV)
        ok = idx >= 0
        S[torch.arange(N, device=DEV)[:, None].expand_as(idx)[ok], idx[ok]] = logit[ok]
        mask = None
        if exclude is not None:
            mask = torch.zeros(N, N, dtype=torch.bool, device=DEV)
            mask[exclude[0], exclude[1]] = True
            mask |= mask.T.clone()
        for m in (1, 50, N * (N - 1) // 2):
            u, v, s = select_top(S, m, mask)                          # S[u, v], u < v: query u, candidate v
            src, dst, lg, _ = ops.score_mine(Z, H, t, m, exclude=exclude)
            assert torch.equal(src.long(), u) and torch.equal(dst.long(), v) and torch.equal(bits(lg), bits(s))


def test_exact_ties_across_the_cut():
    from disenlink_amd import ops
    N, K, d = 200, 2, 32
    Z, H = tables(N, K, d, seed=31)
    zero = torch.from_numpy(np.random.default_rng(31).choice(N, 120, replace=False)).to(DEV)
    H[zero] = 0.0
    H[zero[:40], :, ::2] = -0.0                                       # products of either sign of zero
    live = torch.ones(N, dtype=torch.bool, device=DEV)
    live[zero] = False
    a, b = torch.nonzero(live)[:2, 0].tolist()
    Z[b], H[b] = Z[a], H[a]                                           # a duplicated row: exact ties among the live logits too
    s64, band = logits64(Z, H, 1.0)
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    n_pos, n_zero = int((iu & (s64 > 0)).sum()), int((iu & (s64 == 0)).sum())
    assert n_zero > 5000 and not (iu & (s64 != 0) & (s64.abs() <= band)).any()      # no live logit of doubtful sign
    m = n_pos + n_zero // 3                                           # the cut falls inside the run of zeros
    u, v, s = mine64(Z, H, 1.0, None, NINF, m)
    src, dst, logit, _ = ops.score_mine(Z, H, 1.0, m)
    assert len(src) == m and (logit[n_pos:] == 0).all() and (logit[:n_pos] > 0).all()
    assert torch.equal(src[n_pos:].long(), u[n_pos:]) and torch.equal(dst[n_pos:].long(), v[n_pos:])
    assert_valid_mine((src, dst, logit, _), s64, band, N, m)
    rows_a = ((src == a) & (dst != b)).nonzero()[:, 0]                # (a, w) sits right before (b, w), or after (w, b)
    w = dst[rows_a]
    assert len(rows_a) > 0
    for r, x in zip(rows_a.tolist(), w.tolist()):
        if x > b and float(logit[r]) != 0 and r + 1 < m:
            assert (int(src[r + 1]), int(dst[r + 1])) == (b, x) and bits(logit[r:r + 2])[0] == bits(logit[r:r + 2])[1]


def test_exclusion_forms_agree_and_either_orientation_counts():
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph
    N, K, d, m = 150, 3, 64, 400
    Z, H = tables(N, K, d, seed=3)
    rng = np.random.default_rng(3)
    s, t_ = rng.integers(0, N, 2500), rng.integers(0, N, 2500)
    mask = torch.zeros(N, N, device=DEV)
    mask[torch.from_numpy(s).to(DEV), torch.from_numpy(t_).to(DEV)] = 1          # one orientation only
    G = Graph.from_edge_rows(torch.from_numpy(s).to(DEV), torch.from_numpy(t_).to(DEV), N)
    pairs = (torch.from_numpy(s).to(DEV), torch.from_numpy(t_).to(DEV))
    outs = [ops.score_mine(Z, H, 1.0, m, exclude=e) for e in (G, mask, pairs, (pairs[1], pairs[0]))]
    assert all(same(outs[0], o) for o in outs[1:])
    src, dst = outs[0][0].long(), outs[0][1].long()
    sym = mask.bool() | mask.bool().T
    assert len(src) == m and (src < dst).all() and not sym[src, dst].any()
    s64, band = logits64(Z, H, 1.0)
    assert_valid_mine(outs[0], s64, band, N, m, excluded=mask)
    free = ops.score_mine(Z, H, 1.0, m)
    u, v = int(free[0][0]), int(free[1][0])                          # the best pair, listed only as (v, u)
    only = ops.score_mine(Z, H, 1.0, m, exclude=(torch.tensor([v]), torch.tensor([u])))
    assert (int(only[0][0]), int(only[1][0])) != (u, v) and same([x[1:] for x in free], [x[:m - 1] for x in only])


def test_overflow_inf_first_nan_never():
    from disenlink_amd import ops
    N, d = 90, 32
    Z, H = tables(N, 1, d, seed=7)
    Z[:45] = 4.0                                                      # z.z = 512: exp overflows
    H[:20] = 0.25                                                     # h.h > 0: +inf
    H[20:30] = 0.25
    H[20:30, :, ::2] = -0.5                                           # against rows 0..19: h.h < 0: -inf
    H[30:45] = 0.0                                                    # h.h = 0 against inf: NaN
    idx, logit, _ = ops.score_topk(Z, H, 1.0, torch.arange(N, device=DEV), 128)
    S = torch.full((N, N), float("nan"), device=DEV)
    ok = idx >= 0
    S[torch.arange(N, device=DEV)[:, None].expand_as(idx)[ok], idx[ok]] = logit[ok]
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    n_pinf, n_ninf, n_nan = (int((iu & (S == float("inf"))).sum()), int((iu & (S == NINF)).sum()), int((iu & torch.isnan(S)).sum()))
    assert n_pinf >= 190 and n_ninf >= 200 and n_nan >= 15 * 30
    total = N * (N - 1) // 2
    src, dst, lg, pr = ops.score_mine(Z, H, 1.0, total + 3)           # no floor: everything but the NaN, -inf last
    assert len(src) == total - n_nan and not torch.isnan(lg).any()
    assert torch.isinf(lg[:n_pinf]).all() and (lg[:n_pinf] > 0).all() and (pr[:n_pinf] == 1).all()
    pair = src.long() * N + dst.long()
    assert (pair[:n_pinf][1:] > pair[:n_pinf][:-1]).all()            # +inf in index order
    assert (lg[-n_ninf:] == NINF).all() and torch.isfinite(lg[n_pinf:-n_ninf]).all() and (pr[-n_ninf:] == 0).all()
    u, v, s = select_top(S, total + 3)
    assert torch.equal(src.long(), u) and torch.equal(dst.long(), v) and torch.equal(bits(lg), bits(s))
    fl = ops.score_mine(Z, H, 1.0, total + 3, min_logit=-3.0e38)      # any finite floor: no -inf, no NaN
    assert len(fl[0]) == total - n_nan - n_ninf and same(fl, [x[:len(fl[0])] for x in (src, dst, lg, pr)])
    top = ops.score_mine(Z, H, 1.0, 5, min_logit=float("inf"))
    assert same(top, [x[:5] for x in (src, dst, lg, pr)])


def _raw_call(Z, H, t, m, ws_bytes=None, poison=0xFF):
    """dl_score_mine itself, every buffer pre-filled: -> the full padded outputs and the count"""
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    N, K, d = Z.shape
    need = int(lib.dl_score_mine_workspace_bytes(N, K, d, m))
    ws = torch.full((max(need if ws_bytes is None else ws_bytes, 16),), poison, dtype=torch.uint8, device=DEV)
    outs = [torch.full((4 * m,), poison, dtype=torch.uint8, device=DEV).view(dt)
            for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    rc = lib.dl_score_mine(Z.data_ptr(), H.data_ptr(), N, K, d, float(t), None, None, NINF, m, *[o.data_ptr() for o in outs],
                           count.data_ptr(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, ops._stream())
    return rc, outs, count


def test_padding_and_degenerate_sizes():
    from disenlink_amd import ops
    Z, H = tables(300, 2, 32, seed=9)
    for n, m in ((1, 4), (2, 4), (300, 65536)):
        rc, (src, dst, lg, pr), count = _raw_call(Z[:n].contiguous(), H[:n].contiguous(), 1.0, m)
        c = min(m, n * (n - 1) // 2)
        assert rc == 0 and int(count) == c < m
        assert (src[c:] == -1).all() and (dst[c:] == -1).all() and torch.isnan(lg[c:]).all() and torch.isnan(pr[c:]).all()
        assert (src[:c] >= 0).all() and (src[:c] < dst[:c]).all() and not torch.isnan(lg[:c]).any()
        trimmed = ops.score_mine(Z[:n], H[:n], 1.0, m)
        assert same(trimmed, [x[:c] for x in (src, dst, lg, pr)])
    out = ops.score_mine(Z[:2], H[:2], 1.0, 3, exclude=(torch.tensor([1]), torch.tensor([0])))      # its only pair excluded
    assert all(len(x) == 0 for x in out)
    s64, band = logits64(Z, H, 1.0)
    assert_valid_mine(ops.score_mine(Z, H, 1.0, 65536), s64, band, 300, 65536)


def test_bitwise_reproducible_under_any_geometry(lib_env):
    from disenlink_amd import ops
    N, K, d, m = 700, 3, 64, 5000
    Z, H = tables(N, K, d, seed=13)
    H[100:] = 0.0                                                     # ties across the cut here too: about 2,500 logits > 0
    excl = (torch.arange(N, device=DEV), (torch.arange(N, device=DEV) + 1) % N)
    ref = ops.score_mine(Z, H, 1.0, m, exclude=excl, min_logit=0.0)
    assert len(ref[0]) == m and int((ref[2] == 0).sum()) > 100
    assert same(ref, ops.score_mine(Z, H, 1.0, m, exclude=excl, min_logit=0.0))
    rc, raw, count = _raw_call(Z, H, 1.0, 300, poison=0x7F)           # other garbage in the buffers: the same bits
    rc2, raw2, count2 = _raw_call(Z, H, 1.0, 300)
    assert rc == 0 and rc2 == 0 and int(count) == int(count2) == 300 and same(raw, raw2)
    for tiles in (1, 4, 21):                                          # DL_MINE_TILES: tile pairs per workgroup (21 = all of them)
        lib_env("DL_MINE_TILES", tiles)
        assert same(ref, ops.score_mine(Z, H, 1.0, m, exclude=excl, min_logit=0.0))


def test_argument_errors():
    from disenlink_amd import ops, _lib
    Z, H = tables(10, 2, 32)
    for m in (0, -1, 65537):
        with pytest.raises(_lib.DisenlinkHipError, match="outside 1..65536"):
            ops.score_mine(Z, H, 1.0, m)
    with pytest.raises(_lib.DisenlinkHipError, match="46340"):
        big = torch.zeros(46341, 1, 1, device=DEV)
        ops.score_mine(big, big, 1.0, 3)
    with pytest.raises(_lib.DisenlinkHipError, match="1 <= d <= 128"):
        Zw, Hw = tables(10, 1, 130)
        ops.score_mine(Zw, Hw, 1.0, 3)
    with pytest.raises(TypeError, match="fp32"):
        ops.score_mine(Z.bfloat16(), H.bfloat16(), 1.0, 3)
    with pytest.raises(ValueError):
        ops.score_mine(Z, H, 1.0, 3, exclude=(torch.tensor([10]), torch.tensor([0])))
    lib = _lib.load()
    need = int(lib.dl_score_mine_workspace_bytes(10, 2, 32, 3))
    rc, _, _ = _raw_call(Z, H, 1.0, 3, ws_bytes=need - 1)
    assert rc == -3 and b"workspace too small" in lib.dl_last_error()          # DL_E_WORKSPACE
    with pytest.raises(_lib.DisenlinkHipError, match="workspace too small"):
        _lib.check(rc, "dl_score_mine")


def test_top_missing_links_against_dropin_forward(golden):
    from disenlink_amd.features import SparseFeatures
    from disenlink_amd.model import Disentangle, MinedLinks
    g, meta = golden, golden["meta"]
    model = Disentangle(meta["F"], meta["nhid"], meta["d"], nfactor=meta["K"], beta=meta["beta"], t=meta["t"])
    model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")})
    model = model.to(DEV)
    x, adj = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["adj"]).to(DEV)
    N = meta["N"]
    cand = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1) & ~(adj.bool() | adj.bool().T)
    m = max(1, int(cand.sum()) // 2)
    with torch.no_grad():
        _, lp = model(x, adj)
    lp = lp.double()
    mined = model.top_missing_links(x, adj, m)                       # exclude=None: the edges of adj
    assert isinstance(mined, MinedLinks) and len(mined.src) == min(m, int(cand.sum()))
    u, v = mined.src.long(), mined.dst.long()
    assert cand[u, v].all() and (u < v).all()
    np.testing.assert_allclose(mined.prob.cpu().numpy(), lp[u, v].cpu().numpy(), atol=1e-5, rtol=0)
    got = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    got[u, v] = True
    rest = cand & ~got
    unsat = mined.prob.double().min() < 1 - 1e-4                      # where the probabilities are unsaturated
    if rest.any() and unsat:
        assert float(lp[rest].max()) <= float(lp[u, v].min()) + 1e-5
    if len(u) > 1:
        assert (mined.logit[:-1] >= mined.logit[1:]).all()
    half = model.top_missing_links(x, adj, m, min_prob=0.5)
    assert (half.logit >= 0).all() and len(half.src) == int((mined.logit >= 0).sum()) and same(half, [t[:len(half.src)] for t in mined])
    every = model.top_missing_links(x, adj, m, exclude=(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)))
    assert len(every.src) == m
    sparse = model.top_missing_links(SparseFeatures.from_dense(g["x"]).to(DEV), adj, m)     # the gathers' rounding, not the GEMM's
    us, vs = sparse.src.long(), sparse.dst.long()
    assert len(us) == len(u) and cand[us, vs].all()
    np.testing.assert_allclose(sparse.prob.cpu().numpy(), lp[us, vs].cpu().numpy(), atol=1e-5, rtol=0)


def test_cli_mine_prints_and_writes_its_list(tmp_path):
    from disenlink_amd.main import main
    out = tmp_path / "mined.txt"
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        main(["--dataset", "squirrel", "--synthetic", "--epochs", "3", "--run", "1", "--quiet", "--mine", "50",
              "--mine-out", str(out)])
    lines = buf.getvalue().splitlines()
    head = [i for i, ln in enumerate(lines) if ln.startswith("mined 50 links")]
    assert len(head) == 1
    shown = [ln.split() for ln in lines[head[0] + 1:head[0] + 11]]
    rows = [ln.split() for ln in out.read_text().splitlines()]
    assert len(rows) == 50 and all(len(r) == 4 for r in rows)
    assert [r[:2] for r in shown] == [r[:2] for r in rows[:10]]
    src, dst = np.array([int(r[0]) for r in rows]), np.array([int(r[1]) for r in rows])
    logit, prob = np.array([float(r[2]) for r in rows]), np.array([float(r[3]) for r in rows])
    assert (src < dst).all() and (np.diff(logit) <= 0).all() and ((prob >= 0) & (prob <= 1)).all()
    from disenlink_amd.main import build_parser, load_dataset
    ds = load_dataset(build_parser().parse_args(["--dataset", "squirrel", "--synthetic"]))
    known = set(zip(np.asarray(ds.src).tolist(), np.asarray(ds.dst).tolist()))
    assert not any((a, b) in known or (b, a) in known for a, b in zip(src.tolist(), dst.tolist()))
