"""Global rank counts of target pairs among all unordered pairs (ops.score_pair_ranks, Disentangle.missing_link_ranks,
--global-rank-eval): exact against the enumerated graph (ops.score_mine with m = every pair lists every non-NaN candidate
with the scan's own bits), bracketed by fp64 independently of the mining, under every launch geometry, on ties and special
values, under heavy clustering, and through the module and the CLI.

Order of a NaN target: the contract (NaN below everything, equal only to NaN) makes every non-NaN candidate rank strictly
above it, so its ``greater`` is the number of non-NaN candidates and its ties are the other NaN candidates; that is what
dl_score_ranks counts for a NaN target too, and what is asserted here."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import mine_ref
import pair_rank_ref
from pair_rank_ref import candidates, counts_from_list, targets_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def tables(N, K, d, seed=0, scale=1.0):
    """the tables of test_gpu_mine.py::tables"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (torch.randn(N, K, d, generator=g) * scale / d ** 0.5).to(DEV)
    H = (torch.randn(N, K, d, generator=g) / d ** 0.5).to(DEV)
    return Z, H


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def mined_matrix(N, src, dst, logit):
    S = torch.full((N, N), float("nan"), device=DEV)
    listed = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    S[src.long(), dst.long()] = logit
    listed[src.long(), dst.long()] = True
    return S, listed


def check_against_enumeration(Z, H, t, src, dst, mask):
    """Every output of score_pair_ranks against the list of EVERY candidate (N (N - 1) / 2 <= 65,536); mask: bool [N,N],
    symmetric, or None.  -> (outputs, mined list, |C|, NaN candidates)."""
    from disenlink_amd import ops
    N = Z.shape[0]
    src, dst = src.to(DEV), dst.to(DEV)
    lo, hi = torch.minimum(src, dst), torch.maximum(src, dst)
    n_c = int(candidates(N, mask, DEV).sum())
    ms, md, ml, _ = ops.score_mine(Z, H, t, N * (N - 1) // 2, exclude=mask)
    n_nan = n_c - len(ms)
    greater, ties, logit, n_others, counted = ops.score_pair_ranks_counted(Z, H, t, src, dst, exclude=mask)
    assert greater.dtype == ties.dtype == n_others.dtype == torch.int64 and logit.dtype == torch.float32
    assert greater.shape == ties.shape == logit.shape == n_others.shape == (len(src),)
    in_c = torch.ones(len(src), dtype=torch.bool, device=DEV) if mask is None else ~mask[lo, hi]
    assert int(counted) == n_c and torch.equal(n_others, n_c - in_c.long())
    S, listed = mined_matrix(N, ms, md, ml)
    in_list = in_c & listed[lo, hi]                                   # a NaN target is a candidate the list leaves out
    assert torch.equal(bits(logit[in_list]), bits(S[lo, hi][in_list])) and torch.isnan(logit[in_c & ~in_list]).all()
    exp_g, exp_t = counts_from_list(ml, n_nan, logit, in_c)
    assert torch.equal(greater, exp_g) and torch.equal(ties, exp_t)
    assert (greater >= 0).all() and (ties >= 0).all() and (greater + ties <= n_others).all()
    return (greater, ties, logit, n_others), (ms, md, ml), n_c, n_nan


def topk_logits(Z, H, t, lo, hi):
    """score_topk's logit for query lo[i], candidate hi[i]: every other candidate of the query excluded, so the row's list
    holds the wanted ones whatever N is"""
    from disenlink_amd import ops
    N = Z.shape[0]
    block = torch.ones(N, N, dtype=torch.bool, device=DEV)
    block[lo, hi] = False
    q = torch.unique(lo)
    idx, lg, _ = ops.score_topk(Z, H, t, q, 128, exclude=block)
    assert int((idx >= 0).sum(1).max()) < 128                        # nothing cut off
    S = torch.full((N, N), float("nan"), device=DEV)
    ok = idx >= 0
    S[q[:, None].expand_as(idx)[ok], idx[ok]] = lg[ok]
    return S[lo, hi]


@pytest.mark.parametrize("N,KD,t", pair_rank_ref.GPU_CASES)
def test_exact_against_the_enumerated_graph(N, KD, t):
    K, d = KD
    seed = N * 131 + K * 7 + d + t
    Z, H = tables(N, K, d, seed=seed)
    src, dst = targets_for(N, seed)
    src, dst = src.to(DEV), dst.to(DEV)
    lo, hi = torch.minimum(src, dst), torch.maximum(src, dst)
    g = torch.Generator().manual_seed(seed + 1)
    mask = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    half = torch.arange(len(src), device=DEV) % 2 == 0                # half of the targets are members of E, listed as (max, min)
    mask[hi[half], lo[half]] = True
    extra = torch.randint(0, N, (2, N), generator=g).to(DEV)      # and other pairs, self pairs among them
    mask[extra[0], extra[1]] = True
    mask |= mask.T.clone()
    (greater, ties, logit, n_others), _, n_c, n_nan = check_against_enumeration(Z, H, t, src, dst, mask)
    assert n_nan == 0
    ex = mask[lo, hi]
    assert ex.any() and (N <= 5 or (~ex).any())
    got = topk_logits(Z, H, t, lo[ex], hi[ex])                        # excluded targets: the bits of the ranking scan
    assert torch.equal(bits(logit[ex]), bits(got))
    if N == 300 and KD == (3, 40):                                    # no exclusion at all; the other exclusion forms
        from disenlink_amd import ops
        check_against_enumeration(Z, H, t, src, dst, None)
        r, c = torch.nonzero(torch.triu(mask), as_tuple=True)         # includes (u, u) entries
        ref = ops.score_pair_ranks(Z, H, t, src, dst, exclude=mask)
        assert same(ref, ops.score_pair_ranks(Z, H, t, src, dst, exclude=(c, r)))
        assert same(ref, ops.score_pair_ranks(Z, H, t, dst.int(), src.int(), exclude=(r.tolist(), c.tolist())))


@pytest.mark.parametrize("N,KD,t", pair_rank_ref.GPU_CASES)
def test_bracketed_by_fp64_independently_of_the_mining(N, KD, t):
    """For every target: candidates surely above it <= greater, and greater + ties <= candidates possibly at or above it,
    with mine_ref.logits64 and its band.  Width of the brackets, a condition on the reference alone: at most
    max(10, 0.1 % of |C|); the widest over the 60 cases is 23 of 44,850 (N = 300, K = 8, d = 64)."""
    from disenlink_amd import ops
    K, d = KD
    Z, H = tables(N, K, d, seed=N * 131 + K * 7 + d + t)
    g = torch.Generator().manual_seed(N + K + d)
    src = torch.randint(0, N, (200,), generator=g)
    dst = (src + 1 + torch.randint(0, N - 1, (200,), generator=g)) % N
    src, dst = src.to(DEV), dst.to(DEV)
    lo, hi = torch.minimum(src, dst), torch.maximum(src, dst)
    s64, band = mine_ref.logits64(Z, H, t)
    cu, cv = torch.nonzero(candidates(N, None, DEV), as_tuple=True)
    sc, bc = s64[cu, cv][None, :], band[cu, cv][None, :]
    si, bi = s64[lo, hi][:, None], band[lo, hi][:, None]
    other = ~((cu[None, :] == lo[:, None]) & (cv[None, :] == hi[:, None]))
    sure = ((sc - bc > si + bi) & other).sum(1)
    maybe = ((sc + bc >= si - bi) & other).sum(1)
    assert int((maybe - sure).max()) <= max(10, len(cu) // 1000)      # the brackets say something
    greater, ties, logit, n_others = ops.score_pair_ranks(Z, H, t, src, dst)
    assert (logit.double() - s64[lo, hi]).abs().le(band[lo, hi] + 1e-30).all()
    assert (sure <= greater).all() and (greater + ties <= maybe).all()
    assert (n_others == len(cu) - 1).all()


def expected_from_top_list(ml, sel):
    """(greater, ties) of the entries ``sel`` of a mined list, all strictly above its last entry: everything above them is
    in the list"""
    k = pair_rank_ref.order_key(ml)
    asc = torch.sort(k).values
    gt = len(k) - torch.searchsorted(asc, k[sel], right=True)
    ge = len(k) - torch.searchsorted(asc, k[sel], right=False)
    return gt, ge - gt - 1


def test_beyond_one_list_and_under_every_geometry(lib_env):
    from disenlink_amd import ops
    geo = pair_rank_ref.GEOMETRY
    N, K, d = geo["N"], geo["K"], geo["d"]
    Z, H = tables(N, K, d, seed=17)
    excl = (torch.arange(N, device=DEV), (torch.arange(N, device=DEV) + 1) % N)
    ms, md, ml, _ = ops.score_mine(Z, H, 1.0, 10000, exclude=excl)
    assert len(ms) == 10000 and N * (N - 1) // 2 > 65536
    sel = ml > ml[-1]
    assert int(sel.sum()) > 9000
    src, dst = md[sel], ms[sel]                                       # given as (max, min)
    exp_g, exp_t = expected_from_top_list(ml, sel)
    ref = ops.score_pair_ranks_counted(Z, H, 1.0, src, dst, exclude=excl)
    assert torch.equal(ref[0], exp_g) and torch.equal(ref[1], exp_t) and torch.equal(bits(ref[2]), bits(ml[sel]))
    assert int(ref[4]) == N * (N - 1) // 2 - N and (ref[3] == int(ref[4]) - 1).all()
    assert same(ref, ops.score_pair_ranks_counted(Z, H, 1.0, src, dst, exclude=excl))
    for tiles in geo["tiles"]:
        lib_env("DL_MINE_TILES", tiles)
        for _ in range(2):
            assert same(ref, ops.score_pair_ranks_counted(Z, H, 1.0, src, dst, exclude=excl))


def all_pairs(N):
    u, v = torch.triu_indices(N, N, 1)
    return u.to(DEV), v.to(DEV)


def test_exact_copies_of_a_row_tie():
    N, K, d = 200, 2, 32
    Z, H = tables(N, K, d, seed=31)
    a, b = 70, 150
    Z[b], H[b] = Z[a], H[a]
    w = torch.tensor([w for w in range(N) if w < a or w > b], device=DEV)
    src = torch.cat([torch.full_like(w, a), torch.full_like(w, b)])   # (a, w) and (b, w): the copy has the same operand role
    dst = torch.cat([w, w])
    (greater, ties, logit, _), _, _, n_nan = check_against_enumeration(Z, H, 1.0, src, dst, None)
    assert n_nan == 0 and (ties >= 1).all()
    assert torch.equal(bits(logit[:len(w)]), bits(logit[len(w):])) and torch.equal(greater[:len(w)], greater[len(w):])


def test_overflowed_exp_inf_groups_and_nan():
    N, d = 90, 32
    Z, H = tables(N, 1, d, seed=7)
    Z[:45] = 4.0                                                      # z.z = 512: exp overflows
    H[:20] = 0.25                                                     # h.h > 0: +inf
    H[20:30] = 0.25
    H[20:30, :, ::2] = -0.5                                           # against rows 0..19: h.h < 0: -inf
    H[30:45] = 0.0                                                    # h.h = 0 against inf: NaN
    src, dst = all_pairs(N)
    mask = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    mask[31, 40] = mask[0, 1] = mask[50, 60] = True                   # a NaN, a +inf and a finite target outside C
    mask |= mask.T.clone()
    (greater, ties, logit, n_others), (ms, md, ml), n_c, n_nan = check_against_enumeration(Z, H, 1.0, src, dst, mask)
    n_pinf, n_ninf = int((ml == float("inf")).sum()), int((ml == float("-inf")).sum())
    assert n_pinf >= 190 and n_ninf >= 200 and n_nan >= 15 * 30 and not torch.isnan(ml).any()
    isn = torch.isnan(logit)
    in_c = ~mask[src, dst]
    assert int((isn & in_c).sum()) == n_nan and int((isn & ~in_c).sum()) == 1
    assert (greater[isn] == len(ms)).all()                            # every non-NaN candidate is above a NaN
    assert torch.equal(ties[isn], n_nan - in_c[isn].long())
    pinf = logit == float("inf")
    assert (greater[pinf] == 0).all() and torch.equal(ties[pinf], n_pinf - in_c[pinf].long())
    ninf = logit == float("-inf")
    assert (greater[ninf] == len(ms) - n_ninf).all() and (ties[ninf] == n_ninf - 1).all()


def test_signed_zeros_are_one_value():
    N, K, d = 64, 1, 8
    g = torch.Generator().manual_seed(3)
    Z = torch.full((N, K, d), math.sqrt(69.0 / d))
    Z[32:] = -Z[32:]                                                  # across the groups exp(-69) = 1e-30
    H = torch.randn(N, K, d, generator=g) * 1e-10                     # h.h of either sign, about 1e-20: the product underflows
    Z, H = Z.to(DEV), H.to(DEV)
    src, dst = all_pairs(N)
    (greater, ties, logit, _), _, n_c, _ = check_against_enumeration(Z, H, 1.0, src, dst, None)
    zero = logit == 0
    assert int(zero.sum()) == 32 * 32
    from disenlink_amd import _lib, ops                              # the library's own output keeps the sign: both occur
    lib = _lib.load()
    raw = torch.empty(len(src), dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib.dl_score_pair_logits_workspace_bytes(N, K, d)), dtype=torch.uint8, device=DEV)
    a32, b32 = src.int(), dst.int()
    _lib.check(lib.dl_score_pair_logits(Z.data_ptr(), H.data_ptr(), N, K, d, 1.0, a32.data_ptr(), b32.data_ptr(),
                                        len(src), raw.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "dl_score_pair_logits")
    assert torch.equal(raw == 0, zero) and (raw[zero].signbit()).any() and (~raw[zero].signbit()).any()
    assert not logit[zero].signbit().any() and torch.equal(bits(raw[~zero]), bits(logit[~zero]))
    assert (ties[zero] == 32 * 32 - 1).all() and torch.unique(greater[zero]).numel() == 1      # one value, whatever the sign
    assert int(greater[zero][0]) == int((logit > 0).sum())


def test_heavy_clustering_with_many_workgroups():
    from disenlink_amd import _lib, ops
    N, K, d = 2000, 1, 8
    g = torch.Generator().manual_seed(11)
    Hi = torch.randint(-2, 3, (N, K, d), generator=g)
    Z, H = torch.zeros(N, K, d, device=DEV), Hi.float().to(DEV)
    S = (Hi[:, 0].long() @ Hi[:, 0].long().T).to(DEV)                 # every logit is this integer, in any arithmetic
    assert int(S.abs().max()) <= 32
    T = 600
    src = torch.randint(0, N, (T,), generator=g)
    dst = (src + 1 + torch.randint(0, N - 1, (T,), generator=g)) % N
    src, dst = src.to(DEV), dst.to(DEV)
    lo, hi = torch.minimum(src, dst), torch.maximum(src, dst)
    er, ec = torch.randint(0, N, (2, 40000), generator=g).to(DEV)
    er, ec = torch.cat([er, hi[::2]]), torch.cat([ec, lo[::2]])       # a random exclusion set and half of the targets
    mask = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    mask[er, ec] = True
    mask |= mask.T.clone()
    cand = candidates(N, mask, DEV)
    n_c = int(cand.sum())
    hist = torch.bincount(S[cand] + 32, minlength=65)                 # candidates per value
    above = torch.flip(torch.cumsum(torch.flip(hist, [0]), 0), [0]) - hist
    in_c = ~mask[lo, hi]
    x = S[lo, hi] + 32
    assert _lib.score_pair_ranks_form(N, K, d, T)["grid"] > 100
    greater, ties, logit, n_others, counted = ops.score_pair_ranks_counted(Z, H, 1.0, src, dst, exclude=(er, ec))
    assert torch.equal(logit, S[lo, hi].float())
    assert torch.equal(greater, above[x]) and torch.equal(ties, hist[x] - in_c.long())
    assert int(counted) == n_c and torch.equal(n_others, n_c - in_c.long())


def test_pair_logits_alone_have_the_bits_of_the_ranking_scan():
    from disenlink_amd import ops
    N, K, d = 129, 3, 40
    Z, H = tables(N, K, d, seed=5)
    q = torch.arange(N, device=DEV)
    idx, lg, _ = ops.score_topk(Z, H, 2.0, q, 128, exclude_self=True)
    ok = idx[:, :100] >= 0
    a = q[:, None].expand(N, 100)[ok]
    b = idx[:, :100][ok]
    out = ops.score_pair_logits(Z, H, 2.0, a, b)                      # either orientation: a[i] is the A operand
    assert torch.equal(bits(out), bits(lg[:, :100][ok]))
    none = torch.zeros(0, dtype=torch.int64)
    assert ops.score_pair_logits(Z, H, 2.0, none, none).shape == (0,)


def test_argument_errors_and_empty_inputs():
    from disenlink_amd import ops, _lib
    Z, H = tables(10, 2, 32)
    with pytest.raises(TypeError, match="fp32"):
        ops.score_pair_ranks(Z.bfloat16(), H.bfloat16(), 1.0, [0], [1])
    with pytest.raises(ValueError, match="self pair"):
        ops.score_pair_ranks(Z, H, 1.0, [0, 3], [1, 3])
    for s, v in (([0, 10], [1, 2]), ([0, 1], [-1, 2])):
        with pytest.raises(ValueError, match="outside"):
            ops.score_pair_ranks(Z, H, 1.0, s, v)
    with pytest.raises(ValueError, match="differ in length"):
        ops.score_pair_ranks(Z, H, 1.0, [0, 1], [2])
    with pytest.raises(_lib.DisenlinkHipError, match="temperature"):
        ops.score_pair_ranks(Z, H, 0.0, [0], [1])
    with pytest.raises(_lib.DisenlinkHipError, match="1 <= d <= 128"):
        Zw, Hw = tables(10, 1, 130)
        ops.score_pair_ranks(Zw, Hw, 1.0, [0], [1])
    with pytest.raises(ValueError):
        ops.score_pair_ranks(Z, H, 1.0, [0], [1], exclude=(torch.tensor([10]), torch.tensor([0])))
    none = torch.zeros(0, dtype=torch.int64)
    out = ops.score_pair_ranks_counted(Z, H, 1.0, none, none, exclude=(torch.tensor([1, 2]), torch.tensor([0, 2])))
    assert [o.dtype for o in out[:4]] == [torch.int64, torch.int64, torch.float32, torch.int64]
    assert all(o.shape == (0,) for o in out[:4]) and int(out[4]) == 44                 # T = 0; (2, 2) excludes nothing
    g, t_, lg, n = ops.score_pair_ranks(Z[:2], H[:2], 1.0, [1], [0])                    # the graph's only pair
    assert (g.tolist(), t_.tolist(), n.tolist()) == ([0], [0], [0])
    lib = _lib.load()
    need = int(lib.dl_score_pair_ranks_workspace_bytes(10, 2, 32))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int64, device=DEV)
    key = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = lib.dl_score_pair_ranks(Z.data_ptr(), H.data_ptr(), 10, 2, 32, 1.0, None, None, key.data_ptr(), 1, cnt.data_ptr(),
                                 cnt[2:].data_ptr(), cnt[1:].data_ptr(), ws.data_ptr(), need - 1, ops._stream())
    assert rc == -3 and b"workspace too small" in lib.dl_last_error()


def test_missing_link_ranks_consistent_with_top_missing_links(golden):
    from disenlink_amd.features import SparseFeatures
    from disenlink_amd.model import Disentangle, PairRanks
    g, meta = golden, golden["meta"]
    model = Disentangle(meta["F"], meta["nhid"], meta["d"], nfactor=meta["K"], beta=meta["beta"], t=meta["t"])
    model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")})
    model = model.to(DEV)
    x, adj = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["adj"]).to(DEV)
    N = meta["N"]
    n_c = int(candidates(N, adj.bool(), DEV).sum())
    mined = model.top_missing_links(x, adj, max(1, n_c // 2))
    sel = pair_rank_ref.order_key(mined.logit) > pair_rank_ref.order_key(mined.logit[-1:])
    exp_g, exp_t = expected_from_top_list(mined.logit, sel)
    r = model.missing_link_ranks(x, adj, mined.dst[sel], mined.src[sel])          # exclude=None: the edges of adj
    assert isinstance(r, PairRanks) and not r.logit.requires_grad
    assert torch.equal(r.greater, exp_g) and torch.equal(r.ties, exp_t) and torch.equal(bits(r.logit), bits(mined.logit[sel]))
    assert (r.n_others == n_c - 1).all()
    e, f = torch.nonzero(torch.triu(adj.bool() | adj.bool().T, 1), as_tuple=True)  # the known edges: ranked although excluded
    if len(e):
        k = model.missing_link_ranks(x, adj, e, f)
        assert (k.n_others == n_c).all() and (k.greater + k.ties <= n_c).all() and (k.greater >= 0).all()
        s = model.missing_link_ranks(SparseFeatures.from_dense(g["x"]).to(DEV), adj, e, f)
        assert (s.n_others == n_c).all() and s.greater.shape == k.greater.shape


def test_cli_global_rank_eval_prints_finite_metrics():
    from disenlink_amd.main import main
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        main(["--dataset", "squirrel", "--synthetic", "--epochs", "3", "--run", "1", "--global-rank-eval"])
    lines = buf.getvalue().splitlines()
    shown = [ln for ln in lines if ln.startswith("test global ranking:")]
    final = [ln for ln in lines if ln.startswith("final")]
    assert len(shown) == 1 and len(final) == 1
    for text in (shown[0][len("test global ranking:"):], final[0]):
        tok = text.split()
        vals = {tok[i]: float(tok[i + 1]) for i in range(len(tok) - 1) if tok[i].startswith(("auc_all", "mean_rank", "mrr", "recall@"))}
        assert set(vals) == {"auc_all", "mean_rank", "mrr", "recall@100", "recall@1000", "recall@10000"}
        assert all(np.isfinite(v) for v in vals.values()) and 0.0 <= vals["auc_all"] <= 1.0 and vals["mean_rank"] >= 1.0
