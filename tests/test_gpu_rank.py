"""Top-k and filtered ranks of all candidate links (ops.score_topk / score_ranks, Disentangle.topk_links / link_ranks)
against an fp64 restatement of the logit, the drop-in forward, forward_pairs and the CLI."""
import io
import contextlib
import itertools

import numpy as np
import pytest
import torch


pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def logits64(Z, H, t, rows):
    """fp64 s(u, v) for u in rows, all v, and the error band 1e-5 * sum_k exp(z.z / t) (|h|.|h| + |h.h| |z|.|z| / t):
    the dense scorer's measure 1e-5 * sum_k |h.h| exp(z.z / t) with each dot product's magnitude taken as the sum of its
    |products| — what fp32 rounding scales with; under cancellation |h.h| alone is below one rounding step of its terms."""
    Zd, Hd = Z.double(), H.double()
    zz = torch.einsum("qkd,nkd->qnk", Zd[rows], Zd)
    hh = torch.einsum("qkd,nkd->qnk", Hd[rows], Hd)
    za = torch.einsum("qkd,nkd->qnk", Zd[rows].abs(), Zd.abs())
    ha = torch.einsum("qkd,nkd->qnk", Hd[rows].abs(), Hd.abs())
    e = torch.exp(zz / t)
    return (hh * e).sum(-1), 1e-5 * (e * (ha + hh.abs() * za / t)).sum(-1)


def candidates(N, rows, ex_mask=None, exclude_self=True):
    c = torch.ones(len(rows), N, dtype=torch.bool, device=DEV)
    if ex_mask is not None:
        c &= ~ex_mask[rows].bool()
    if exclude_self:
        c[torch.arange(len(rows), device=DEV), rows] = False
    return c


def sigmoid_ref(x):
    return 1.0 / (1.0 + torch.exp(-x))


def assert_sorted_total_order(idx, logit):
    for r in range(idx.shape[0]):
        n = int((idx[r] >= 0).sum())
        assert (idx[r, n:] == -1).all() and torch.isnan(logit[r, n:]).all()
        v, i = logit[r, :n].double(), idx[r, :n]
        key = torch.where(torch.isnan(v), torch.full_like(v, -np.inf), v)
        isnan = torch.isnan(v)
        for j in range(n - 1):
            a, b = key[j], key[j + 1]
            if isnan[j]:
                assert isnan[j + 1] and i[j] < i[j + 1]
            elif not isnan[j + 1]:
                assert a > b or (a == b and i[j] < i[j + 1]), (r, j, float(a), float(b))


def assert_valid_topk(idx, logit, prob, s64, band, cand, k):
    """every row a valid top-k of the fp64 logits within their error band; logits within tolerance; prob = sigmoid."""
    assert_sorted_total_order(idx, logit)
    for r in range(idx.shape[0]):
        c = cand[r]
        n_c = int(c.sum())
        n = min(k, n_c)
        got = idx[r, :n]
        assert int((idx[r] >= 0).sum()) == n
        assert c[got].all() and got.unique().numel() == n
        if n == 0:
            continue
        assert (logit[r, :n].double() - s64[r, got]).abs().le(band[r, got] + 1e-30).all()
        vals = torch.where(c, s64[r], torch.full_like(s64[r], -np.inf))
        order = torch.argsort(vals, descending=True)
        kth = order[n - 1]
        assert (s64[r, got] + band[r, got] >= vals[kth] - band[r, kth]).all()
        low = got[torch.argmin(s64[r, got])]
        rest = c.clone()
        rest[got] = False
        assert (s64[r][rest] - band[r][rest] <= s64[r, low] + band[r, low]).all()
        np.testing.assert_allclose(prob[r, :n].cpu().numpy(), sigmoid_ref(logit[r, :n].double()).float().cpu().numpy(),
                                   rtol=1e-6, atol=1e-7)


def tables(N, K, d, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (torch.randn(N, K, d, generator=g) * scale / d ** 0.5).to(DEV)
    H = (torch.randn(N, K, d, generator=g) / d ** 0.5).to(DEV)
    return Z, H


@pytest.mark.parametrize("N,K,d,t", list(itertools.product([1, 37, 128, 129, 300, 1000], [1, 3, 8], [32, 64, 128], [1, 2])))
def test_topk_against_fp64(N, K, d, t):
    from disenlink_amd import ops
    Z, H = tables(N, K, d, seed=N * 131 + K * 7 + d + t)
    rng = np.random.default_rng(N + K + d)
    q = np.concatenate([[0, N - 1, 0, N - 1], rng.integers(0, N, 12)])
    rows = torch.from_numpy(q).to(DEV)
    k = min(128, N // 3 + 1)
    idx, logit, prob = ops.score_topk(Z, H, t, rows, k)
    assert idx.shape == (len(q), k) and idx.dtype == torch.int64 and logit.dtype == torch.float32
    s64, band = logits64(Z, H, t, rows)
    assert_valid_topk(idx, logit, prob, s64, band, candidates(N, rows), k)
    assert torch.equal(idx[0], idx[2]) and torch.equal(logit[1].view(torch.int32), logit[3].view(torch.int32))   # duplicates


def test_topk_against_dropin_forward(golden):
    from disenlink_amd.model import Disentangle
    g, m = golden, golden["meta"]
    model = Disentangle(m["F"], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"])
    model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")})
    model = model.to(DEV)
    x, adj = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["adj"]).to(DEV)
    N = m["N"]
    k = min(8, N)
    top = model.topk_links(x, adj, torch.arange(N, device=DEV), k, exclude=adj)
    lp = torch.from_numpy(g["link_pred"]).double().to(DEV)
    excl = adj.bool() | torch.eye(N, dtype=torch.bool, device=DEV)
    lp = torch.where(excl, torch.full_like(lp, -np.inf), lp)
    vals, ref = torch.sort(lp, dim=1, descending=True)
    for r in range(N):
        n = min(k, int((~excl[r]).sum()))
        assert int((top.index[r] >= 0).sum()) == n
        np.testing.assert_allclose(top.prob[r, :n].cpu().numpy(), vals[r, :n].cpu().numpy(), atol=1e-6, rtol=0)
        if n and (n == int((~excl[r]).sum()) or float(vals[r, n - 1] - vals[r, n]) > 1e-6):
            assert set(top.index[r, :n].tolist()) == set(ref[r, :n].tolist())


def test_exclusion_forms_and_padding():
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph
    N, K, d, k = 150, 3, 64, 20
    Z, H = tables(N, K, d, seed=3)
    rng = np.random.default_rng(3)
    s, t_ = rng.integers(0, N, 900), rng.integers(0, N, 900)
    s[:140], t_[:140] = 5, np.arange(140)                         # node 5 keeps fewer than k candidates
    s[140:143], t_[140:143] = 7, [0, 1, 2]
    mask = torch.zeros(N, N, device=DEV)
    mask[torch.from_numpy(np.r_[s, t_]).to(DEV), torch.from_numpy(np.r_[t_, s]).to(DEV)] = 1
    G = Graph.from_edge_rows(torch.from_numpy(s).to(DEV), torch.from_numpy(t_).to(DEV), N)
    pairs = (torch.from_numpy(np.r_[s, t_]).to(DEV), torch.from_numpy(np.r_[t_, s]).to(DEV))
    rows = torch.arange(N, device=DEV)
    outs = [ops.score_topk(Z, H, 1.0, rows, k, exclude=e) for e in (G, mask, pairs)]
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1].view(torch.int32), o[1].view(torch.int32))
    idx = outs[0][0]
    ok = idx >= 0
    assert not mask[rows[:, None].expand_as(idx)[ok], idx[ok]].bool().any()
    assert not (idx == rows[:, None]).any()
    n5 = int((~mask[5].bool()).sum()) - (0 if mask[5, 5] else 1)
    assert n5 < k and int((idx[5] >= 0).sum()) == n5 and (idx[5, n5:] == -1).all() and torch.isnan(outs[0][1][5, n5:]).all()
    s64, band = logits64(Z, H, 1.0, rows)
    assert_valid_topk(*outs[0], s64, band, candidates(N, rows, mask), k)
    idx_self, lg, pr = ops.score_topk(Z, H, 1.0, rows, k, exclude=mask, exclude_self=False)
    assert_valid_topk(idx_self, lg, pr, s64, band, candidates(N, rows, mask, exclude_self=False), k)


def test_equal_rows_come_back_in_index_order():
    from disenlink_amd import ops
    N, K, d, k = 200, 2, 32, 50
    Z, H = tables(1, K, d, seed=5)
    Z, H = Z.expand(N, K, d).contiguous(), H.expand(N, K, d).contiguous()
    idx, logit, _ = ops.score_topk(Z, H, 1.0, torch.tensor([0, 3, 199], device=DEV), k)
    assert idx[0].tolist() == list(range(1, k + 1))
    assert idx[1].tolist() == [0, 1, 2] + list(range(4, k + 1))
    assert idx[2].tolist() == list(range(k))
    assert (logit == logit[0, 0]).all()


def test_overflow_puts_inf_first_and_nan_last():
    from disenlink_amd import ops
    N, d = 90, 32
    Z, H = tables(N, 1, d, seed=7)
    Z[:30] = 4.0                                                   # z.z = 512: exp overflows -> +inf (h.h > 0)
    Z[30:45] = 4.0
    H[:30] = 0.25
    H[30:45] = 0.0                                                 # h.h = 0, exp = inf -> NaN
    idx, logit, _ = ops.score_topk(Z, H, 1.0, torch.tensor([2], device=DEV), 128)
    n = N - 1
    assert idx[0, :29].tolist() == [v for v in range(30) if v != 2] and torch.isinf(logit[0, :29]).all()
    assert torch.isfinite(logit[0, 29:n - 15]).all()
    assert idx[0, n - 15:n].tolist() == list(range(30, 45)) and torch.isnan(logit[0, n - 15:n]).all()
    assert (idx[0, n:] == -1).all()
    g, tie = ops.score_ranks(Z, H, 1.0, torch.tensor([2, 2, 2]), torch.tensor([5, 31, 60]))
    assert g.tolist()[:2] == [0, 29 + 45] and tie.tolist()[:2] == [28, 14]


def test_ranks_against_fp64_and_topk():
    from disenlink_amd import ops
    N, K, d = 700, 4, 48
    Z, H = tables(N, K, d, seed=11)
    rng = np.random.default_rng(11)
    src = torch.from_numpy(rng.integers(0, N, 300)).to(DEV)
    dst = torch.from_numpy(rng.integers(0, N, 300)).to(DEV)
    es, ed = rng.integers(0, N, 3000), rng.integers(0, N, 3000)
    es[:300], ed[:300] = src.cpu().numpy(), dst.cpu().numpy()     # every target is in the exclusion set: still ranked
    mask = torch.zeros(N, N, device=DEV)
    mask[torch.from_numpy(es).to(DEV), torch.from_numpy(ed).to(DEV)] = 1
    greater, ties = ops.score_ranks(Z, H, 1.0, src, dst, exclude=mask)
    s64, band = logits64(Z, H, 1.0, src)
    cand = candidates(N, src, mask)
    cand[torch.arange(300, device=DEV), dst] = False
    tgt = s64[torch.arange(300, device=DEV), dst]
    tb = band[torch.arange(300, device=DEV), dst]
    near = ((s64 - tgt[:, None]).abs() <= band + tb[:, None]) & cand
    clean = ~near.any(1)
    assert clean.float().mean() > 0.5
    exp_g = ((s64 > tgt[:, None]) & cand).sum(1)
    assert torch.equal(greater[clean], exp_g[clean]) and (ties[clean] == 0).all()
    # the two epilogues agree: the j-th entry of a top-k row, as a target, has j candidates above it
    rows = torch.arange(0, N, 37, device=DEV)
    idx, logit, _ = ops.score_topk(Z, H, 1.0, rows, 60)
    u = rows[:, None].expand_as(idx).reshape(-1)
    v = idx.reshape(-1)
    g2, t2 = ops.score_ranks(Z, H, 1.0, u, v)
    distinct = (logit[:, 1:] != logit[:, :-1]).all(1)
    j = torch.arange(60, device=DEV).repeat(len(rows))
    sel = distinct[:, None].expand_as(idx).reshape(-1)
    assert sel.any() and torch.equal(g2[sel], j[sel]) and (t2[sel] == 0).all()


def test_deterministic_across_runs_and_slices(lib_env):
    from disenlink_amd import ops
    N, K, d = 1500, 3, 64
    Z, H = tables(N, K, d, seed=13)
    rows = torch.arange(0, N, 3, device=DEV)
    src, dst = rows, (rows * 7 + 1) % N
    excl = (torch.arange(N, device=DEV), (torch.arange(N, device=DEV) + 1) % N)
    ref = ops.score_topk(Z, H, 1.0, rows, 100, exclude=excl)
    rr = ops.score_ranks(Z, H, 1.0, src, dst, exclude=excl)
    again = ops.score_topk(Z, H, 1.0, rows, 100, exclude=excl)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(ref, again))
    for s in (1, 2, 5, 12):
        lib_env("DL_RANK_SLICES", s)
        out = ops.score_topk(Z, H, 1.0, rows, 100, exclude=excl)
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1].view(torch.int32), ref[1].view(torch.int32))
        g, t = ops.score_ranks(Z, H, 1.0, src, dst, exclude=excl)
        assert torch.equal(g, rr[0]) and torch.equal(t, rr[1])


def test_argument_errors():
    from disenlink_amd import ops, _lib
    Z, H = tables(10, 2, 32)
    with pytest.raises(ValueError):
        ops.score_topk(Z, H, 1.0, torch.tensor([0]), 0)
    with pytest.raises(ValueError):
        ops.score_topk(Z, H, 1.0, torch.tensor([0]), 129)
    with pytest.raises(ValueError):
        ops.score_topk(Z, H, 1.0, torch.tensor([10]), 3)
    with pytest.raises(TypeError):
        ops.score_topk(Z.bfloat16(), H.bfloat16(), 1.0, torch.tensor([0]), 3)
    with pytest.raises(_lib.DisenlinkHipError):
        Zw, Hw = tables(10, 1, 160)
        ops.score_topk(Zw, Hw, 1.0, torch.tensor([0]), 3)
    with pytest.raises(ValueError):
        ops.score_ranks(Z, H, 1.0, torch.tensor([0, 1]), torch.tensor([2]))


def test_scale_without_n_squared():
    from disenlink_amd import ops
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.graph import Graph, PairList
    from disenlink_amd.model import Disentangle
    sg = synthetic_graph("snap_patents", seed=0, scale=0.25)
    N = int(sg.n_nodes) if hasattr(sg, "n_nodes") else int(max(sg.src.max(), sg.dst.max()) + 1)
    assert N > 700_000
    torch.manual_seed(0)
    F, K, d = 16, 2, 32
    model = Disentangle(F, 32, d, nfactor=K, beta=0.7, t=1).to(DEV)
    x = torch.randn(N, F, device=DEV) * 0.3
    src, dst = torch.from_numpy(np.asarray(sg.src)).to(DEV), torch.from_numpy(np.asarray(sg.dst)).to(DEV)
    G = Graph.from_edge_rows(src, dst, N)
    Z, H = model._rank_tables(x, G)
    queries = torch.from_numpy(np.random.default_rng(0).choice(N, 256, replace=False)).to(DEV)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    idx, logit, prob = ops.score_topk(Z, H, 1.0, queries, 100, exclude=G)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < (1 << 30)
    with torch.no_grad():
        for r in range(8):
            u = queries[r]
            v = torch.arange(N, device=DEV)
            _, p = model.forward_pairs(x, G, PairList.build(u.repeat(N), v, N))
            cand = torch.ones(N, dtype=torch.bool, device=DEV)
            lo, hi = int(G.rowptr[u]), int(G.rowptr[u + 1])
            cand[G.col[lo:hi].long()] = False
            cand[u] = False
            got = idx[r]
            assert (got >= 0).all() and cand[got].all()
            np.testing.assert_allclose(prob[r].cpu().numpy(), p[got].cpu().numpy(), atol=1e-6, rtol=0)
            kth = torch.sort(torch.where(cand, p.double(), torch.full_like(p.double(), -1.0)), descending=True).values[99]
            assert (p[got].double() >= kth - 1e-6).all()
            rest = cand.clone()
            rest[got] = False
            assert (p[rest].double() <= p[got].double().min() + 1e-6).all()


def test_cli_rank_eval_prints_metrics():
    from disenlink_amd.main import main
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        main(["--dataset", "chameleon", "--synthetic", "--epochs", "3", "--run", "1", "--rank-eval", "--quiet"])
    final = [ln for ln in buf.getvalue().splitlines() if ln.startswith("final")]
    assert len(final) == 1
    toks = final[0].split()
    vals = {toks[i]: float(toks[i + 1]) for i in range(3, len(toks) - 1, 2)}
    assert set(vals) == {"mrr", "hits@1", "hits@10", "hits@50", "hits@100"}
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in vals.values())
    assert vals["hits@1"] <= vals["hits@10"] <= vals["hits@50"] <= vals["hits@100"]
