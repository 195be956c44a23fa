"""Link scans between two node sets (ops.score_mine_between / score_links_between) and by blocks on graphs of any size
(ops.score_mine_blocks / score_links_blocks / score_link_degrees_blocks): the rectangles bit for bit against the triangular
scans of the concatenated table under NodeFilter.between (unchanged code that test_gpu_mine.py / test_gpu_links.py hold
against fp64), one rectangle directly against fp64, the blocks bit for bit against the unblocked calls, a graph past the
cap with an exact oracle, and determinism."""
import itertools

import numpy as np
import pytest
import torch

import between_ref
from test_gpu_mine import bits, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF, NINF = float("inf"), float("-inf")


def tables(n, K, d, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (torch.randn(n, K, d, generator=g) / d ** 0.5).to(DEV)
    H = (torch.randn(n, K, d, generator=g) / d ** 0.5).to(DEV)
    return Z, H


# ---------------------------------------------------------------------- rectangles against the parent, bit for bit
RECTS = ((1, 1), (5, 129), (129, 5), (128, 256), (300, 200))
KDT = ((1, 8, 1.0), (3, 40, 2.0), (2, 96, 1.0), (8, 64, 1.0))


def rect_case(nA, nB, K, d, t):
    """two tables with what the issue lists: duplicated rows in B (equal logits, cut by a * nB + b), a NaN row of A (never
    eligible), one +inf logit, an exclusion set that reaches into the ragged last tiles of both sides, and a rule on groups
    >= 32 that is not symmetric"""
    ZA, HA = tables(nA, K, d, seed=nA * 131 + nB * 17 + K * 7 + d)
    ZB, HB = tables(nB, K, d, seed=nA * 31 + nB * 171 + K * 5 + d + 1)
    if nB >= 3:
        ZB[1], HB[1] = ZB[0], HB[0]
    if nA >= 3:
        HA[1] = float("nan")
    if nA >= 3 and nB >= 3:                                           # z.z / t = 200: exp overflows; h.h > 0: +inf
        ZA[0] = ZB[nB - 1] = (200.0 * t / d) ** 0.5
        HA[0] = HB[nB - 1] = 0.25
    rng = np.random.default_rng(nA + nB)
    ra = np.concatenate([rng.integers(0, nA, 3 * max(nA, nB)), [nA - 1, nA - 1, 0, nA // 2, nA - 1]])
    cb = np.concatenate([rng.integers(0, nB, 3 * max(nA, nB)), [nB - 1, 0, nB - 1, nB // 2, max(nB - 2, 0)]])
    excl = (torch.from_numpy(ra).to(DEV), torch.from_numpy(cb).to(DEV))
    ga, gb = 32 + torch.arange(nA) % 3, 40 + torch.arange(nB) % 4
    allow = torch.zeros(44, 44, dtype=torch.bool)
    for g in range(32, 35):
        for h in range(40, 44):
            allow[g, h] = (g + 2 * h) % 3 != 0
            allow[h, g] = not allow[g, h]                             # the other direction says the opposite: A's row decides
    return ZA, HA, ZB, HB, excl, (ga.to(DEV), gb.to(DEV), allow)


def parent_filters(nA, nB, rule):
    """NodeFilter.between on cat(A, B), and the symmetrised rule restricted to A x B"""
    from disenlink_amd import ops
    in_a = torch.cat([torch.ones(nA, dtype=torch.bool), torch.zeros(nB, dtype=torch.bool)])
    ga, gb, allow = rule
    sym = torch.zeros_like(allow)
    sym[32:35, 40:44] = allow[32:35, 40:44]
    sym |= sym.T.clone()
    return ops.NodeFilter.between(in_a, ~in_a, device=DEV), ops.NodeFilter(torch.cat([ga, gb]), sym, device=DEV)


def split_parent_links(links, nA):
    """the A rows and the B rows of the parent's symmetric CSR as the two sides of the rectangle"""
    rowptr, col, logit, prob = links
    cut = int(rowptr[nA])
    return ((rowptr[:nA + 1], col[:cut] - nA, logit[:cut], prob[:cut]),
            (rowptr[nA:] - cut, col[cut:], logit[cut:], prob[cut:]))


@pytest.mark.parametrize("table_dtype", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
@pytest.mark.parametrize("K,d,t", KDT)
@pytest.mark.parametrize("nA,nB", RECTS)
def test_rectangles_have_the_bits_of_the_triangular_scans(lib_env, nA, nB, K, d, t, table_dtype):
    from disenlink_amd import ops
    ZA, HA, ZB, HB, excl, rule = rect_case(nA, nB, K, d, t)
    Zc, Hc = torch.cat([ZA, ZB]), torch.cat([HA, HB])
    plain, ruled = parent_filters(nA, nB, rule)
    excl_parent = (excl[0], excl[1] + nA)
    big = min(nA * nB + 5, 65536)
    configs = [dict(exclude=None, rule=None, floor=NINF, ms=(1, big)), dict(exclude=excl, rule=rule, floor=0.0, ms=(7, big)),
               dict(exclude=excl, rule=None, floor=NINF, ms=(big,))]
    want = []
    for c in configs:                                                 # the reference, once
        kw = dict(exclude=None if c["exclude"] is None else excl_parent, node_filter=plain if c["rule"] is None else ruled,
                  table_dtype=table_dtype)
        mined = []
        for m in c["ms"]:
            src, dst, logit, prob = ops.score_mine(Zc, Hc, t, m, min_logit=c["floor"], **kw)
            assert (src < nA).all() and (dst >= nA).all()
            mined.append((src, dst - nA, logit, prob))
        want.append((mined, split_parent_links(ops.score_links(Zc, Hc, t, c["floor"], **kw), nA)))
    n_inf = int((want[0][0][1][2] == INF).sum())
    assert n_inf == (1 if nA >= 3 and nB >= 3 else 0)                 # the +inf pair leads the list
    if nA >= 3:
        assert not (want[0][0][1][0] == 1).any() and len(want[0][0][1][0]) == min(big, (nA - 1) * nB)      # the NaN row
    if nB >= 3 and nA >= 5:                                           # the duplicated rows of B: equal bits, (a, 0) before (a, 1)
        src, dst, logit, _ = want[0][0][1]
        i0, i1 = ((src == 2) & (dst == 0)).nonzero()[0, 0], ((src == 2) & (dst == 1)).nonzero()[0, 0]
        assert int(i1) == int(i0) + 1 and bits(logit)[i0] == bits(logit)[i1]
    pairs = -(-nA // 128) * -(-nB // 128)
    for tiles in (1, 4, pairs):
        lib_env("DL_MINE_TILES", tiles)
        for c, (mined, links) in zip(configs, want):
            kw = dict(exclude=c["exclude"], rule=c["rule"], table_dtype=table_dtype)
            for m, ref in zip(c["ms"], mined):
                got = ops.score_mine_between(ZA, HA, ZB, HB, t, m, min_logit=c["floor"], **kw)
                assert got[0].dtype == got[1].dtype == torch.int32 and same(got, ref), (tiles, m)
            got = ops.score_links_between(ZA, HA, ZB, HB, t, c["floor"], **kw)
            assert same(got.ab, links[0]) and same(got.ba, links[1]), tiles
            assert got.ab[0].dtype == got.ba[0].dtype == torch.int64 and got.ab[1].dtype == torch.int32


def test_dense_mask_and_pair_list_exclusions_agree():
    from disenlink_amd import ops
    nA, nB, K, d = 140, 70, 2, 32
    ZA, HA, ZB, HB, excl, _ = rect_case(nA, nB, K, d, 1.0)
    mask = torch.zeros(nA, nB, device=DEV)
    mask[excl[0], excl[1]] = 1
    a = ops.score_mine_between(ZA, HA, ZB, HB, 1.0, 500, exclude=excl)
    b = ops.score_mine_between(ZA, HA, ZB, HB, 1.0, 500, exclude=mask)
    assert same(a, b) and not mask.bool()[a[0].long(), a[1].long()].any() and len(a[0]) == 500


# ---------------------------------------------------------------------- one rectangle directly against fp64
def test_a_rectangle_against_fp64():
    from disenlink_amd import ops
    nA, nB, K, d, t = 129, 200, 3, 40, 1.0
    ZA, HA = tables(nA, K, d, seed=5)
    ZB, HB = tables(nB, K, d, seed=6)
    s64, band = between_ref.logits64(ZA, HA, ZB, HB, t)
    floor = float(torch.median(s64))
    straddle = (s64 - band < floor) & (s64 + band >= floor)           # judged on the reference alone
    assert int(straddle.sum()) <= 0.01 * nA * nB
    for fl, m in ((NINF, 1), (NINF, 1000), (floor, 7), (floor, 65536), (NINF, nA * nB + 5)):
        src, dst, logit, prob = ops.score_mine_between(ZA, HA, ZB, HB, t, m, min_logit=fl)
        sure, maybe = s64 - band >= fl, s64 + band >= fl
        c = len(src)
        assert min(m, int(sure.sum())) <= c <= min(m, int(maybe.sum()))
        a, b = src.long(), dst.long()
        assert (a >= 0).all() and (a < nA).all() and (b >= 0).all() and (b < nB).all()
        assert maybe[a, b].all() and torch.unique(a * nB + b).numel() == c
        v = torch.where(logit == 0, torch.zeros_like(logit), logit).double()
        pair = a * nB + b
        assert ((v[:-1] > v[1:]) | ((v[:-1] == v[1:]) & (pair[:-1] < pair[1:]))).all()
        assert (logit.double() - s64[a, b]).abs().le(band[a, b] + 1e-30).all() and (logit >= fl).all()
        got = torch.zeros(nA, nB, dtype=torch.bool, device=DEV)
        got[a, b] = True
        rest = sure & ~got
        if c < m:
            assert not rest.any()
        else:
            low = torch.argmin(s64[a, b])
            assert (s64[rest] - band[rest] <= s64[a[low], b[low]] + band[a[low], b[low]]).all()
        np.testing.assert_allclose(prob.cpu().numpy(), (1.0 / (1.0 + torch.exp(-logit.double()))).float().cpu().numpy(),
                                   rtol=1e-6, atol=1e-7)
    # the link graph at the same floor: everything surely above it, nothing surely below, both sides the same pairs
    links = ops.score_links_between(ZA, HA, ZB, HB, t, floor)
    for (rowptr, col, logit, prob), S, B, n in ((links.ab, s64, band, nA), (links.ba, s64.T, band.T, nB)):
        rows = torch.repeat_interleave(torch.arange(n, device=DEV), rowptr[1:] - rowptr[:-1])
        got = torch.zeros(S.shape, dtype=torch.bool, device=DEV)
        got[rows, col.long()] = True
        assert int(got.sum()) == col.numel() == int(rowptr[-1])       # no pair twice
        assert not ((S - B >= floor) & ~got).any() and not (got & ~(S + B >= floor)).any()
        assert (logit.double() - S[rows, col.long()]).abs().le(B[rows, col.long()] + 1e-30).all()
        key = rows * S.shape[1] + col.long()
        assert (key[1:] > key[:-1]).all()                             # columns ascending within a row
    ab = torch.zeros(nA, nB, device=DEV)
    ab[torch.repeat_interleave(torch.arange(nA, device=DEV), links.ab[0][1:] - links.ab[0][:-1]), links.ab[1].long()] = links.ab[2]
    ba = torch.zeros(nB, nA, device=DEV)
    ba[torch.repeat_interleave(torch.arange(nB, device=DEV), links.ba[0][1:] - links.ba[0][:-1]), links.ba[1].long()] = links.ba[2]
    assert torch.equal(bits(ab), bits(ba.T.contiguous()))


# ---------------------------------------------------------------------- blocks at small N against the unblocked calls
@pytest.mark.parametrize("table_dtype", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
@pytest.mark.parametrize("N,block", list(itertools.product((129, 300, 700), (128, 256))))
def test_blocks_have_the_bits_of_the_unblocked_scans(N, block, table_dtype):
    from disenlink_amd import ops
    K, d, t = 3, 40, 2.0
    Z, H = tables(N, K, d, seed=N + block)
    H[N // 3:N // 3 + 40] = 0.0                                        # a run of exactly equal logits across the windows
    Z[5], H[5] = Z[N - 2], H[N - 2]
    rng = np.random.default_rng(N)
    ex = (torch.from_numpy(np.concatenate([rng.integers(0, N, 4 * N), [0, 127, 128, N - 1, 127]])).to(DEV),
          torch.from_numpy(np.concatenate([rng.integers(0, N, 4 * N), [N - 1, 128, 127, 0, N - 1]])).to(DEV))
    nf = ops.NodeFilter.different(torch.arange(N) % 5, device=DEV)
    for kw in (dict(), dict(exclude=ex), dict(exclude=ex, node_filter=nf)):
        kw["table_dtype"] = table_dtype
        for floor, m in ((NINF, 1), (NINF, 5000), (0.0, 777), (0.0, 65536)):
            ref = ops.score_mine(Z, H, t, m, min_logit=floor, **kw)
            got = ops.score_mine_blocks(Z, H, t, m, min_logit=floor, block_nodes=block, **kw)
            assert got[0].dtype == got[1].dtype == torch.int32 and same(got, ref), (floor, m)
        for floor in (NINF, 0.0, 0.05):
            ref = ops.score_links(Z, H, t, floor, **kw)
            got = ops.score_links_blocks(Z, H, t, floor, block_nodes=block, **kw)
            assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and same(got, ref), floor
            assert torch.equal(ops.score_link_degrees_blocks(Z, H, t, floor, block_nodes=block, **kw),
                               ops.score_link_degrees(Z, H, t, floor, **kw))


def test_model_methods_take_the_blocked_route():
    from disenlink_amd.model import Disentangle, MinedLinks, PredictedLinks
    N, F = 300, 24
    g = torch.Generator().manual_seed(4)
    model = Disentangle(F, 16, 8, nfactor=3, beta=0.9, t=1.0).to(DEV)
    x = torch.randn(N, F, generator=g).to(DEV)
    a = torch.rand(N, N, generator=g) < 0.03
    adj = (a | a.T).float().to(DEV)
    adj.fill_diagonal_(0)
    ref = model.top_missing_links(x, adj, 2000)
    got = model.top_missing_links(x, adj, 2000, block_nodes=128)
    assert isinstance(got, MinedLinks) and len(got.src) == 2000 and same(got, ref)
    assert not adj.bool()[got.src.long(), got.dst.long()].any()
    ref = model.predicted_links(x, adj, 0.5)
    got = model.predicted_links(x, adj, 0.5, block_nodes=128)
    assert isinstance(got, PredictedLinks) and int(ref.rowptr[-1]) > 0 and same(got, ref)


# ---------------------------------------------------------------------- past the cap, with an exact oracle
BIG_N = 66000
PLANTED = [0, 127, 128, 46207, 46208, 46209, 65535, 65536, 65999, 1, 2, 300, 1000, 5000, 12345, 20000, 30000, 40000, 46000, 46100,
           46300, 47000, 50000, 55000, 60000, 64000, 65000, 65998, 129, 255, 256, 257, 46336, 46335, 23104, 23103, 9999, 33333, 44444,
           61234]


@pytest.fixture(scope="module")
def big_graph():
    """Z = 0 and H[u] = a_u e_0: every logit is the exact integer a_u a_v, 0 outside the planted nodes"""
    a = torch.zeros(BIG_N)
    ids = torch.tensor(PLANTED)
    a[ids] = torch.arange(2, 2 + len(PLANTED)).float()                # distinct small integers: 6 * 4 = 8 * 3 and the like tie
    Z = torch.zeros(BIG_N, 1, 8, device=DEV)
    H = torch.zeros(BIG_N, 1, 8, device=DEV)
    H[:, 0, 0] = a.to(DEV)
    order = torch.argsort(ids)
    P, A = ids[order].tolist(), a[ids[order]].tolist()
    pairs = [(P[i], P[j], A[i] * A[j]) for i in range(len(P)) for j in range(i + 1, len(P))]
    return Z, H, pairs


def planted_order(pairs, excluded=()):
    """the planted pairs in the scans' order: larger logit first, equal logits by the 64-bit u * N + v"""
    keep = [p for p in pairs if (p[0], p[1]) not in excluded]
    return sorted(keep, key=lambda p: (-p[2], p[0] * BIG_N + p[1]))


def test_mining_past_the_cap(big_graph):
    from disenlink_amd import ops
    Z, H, pairs = big_graph
    assert BIG_N > ops.MINE_MAX_N and len(pairs) == 780
    with pytest.raises(ops._lib.DisenlinkHipError, match="46340"):
        ops.score_mine(Z, H, 1.0, 5)                                   # the unblocked entry keeps its cap
    src, dst, logit, prob = ops.score_mine_blocks(Z, H, 1.0, 1000, min_logit=0.5)
    want = planted_order(pairs)
    assert list(zip(src.tolist(), dst.tolist())) == [(u, v) for u, v, _ in want]
    assert logit.tolist() == [x for _, _, x in want] and (prob > 0.98).all()
    assert len({x for _, _, x in want}) < len(want)                   # there are ties, cut by the global index
    # no floor: the planted pairs, then the zero logits by ascending global index (row 0, across the block border at 46,208)
    excluded = {(0, 127), (128, 65999), (46207, 46208), (0, 5), (0, 46208 + 3), (0, 46300 + 1)}
    ex = (torch.tensor([e[1] for e in excluded], device=DEV), torch.tensor([e[0] for e in excluded], device=DEV))      # as (v, u)
    tail = 50000
    src, dst, logit, _ = ops.score_mine_blocks(Z, H, 1.0, len(pairs) + tail, exclude=ex)
    want = planted_order(pairs, excluded)
    k = len(want)
    assert k == len(pairs) - 3 and len(src) == len(pairs) + tail
    assert list(zip(src[:k].tolist(), dst[:k].tolist())) == [(u, v) for u, v, _ in want] and logit[:k].tolist() == [x for _, _, x in want]
    planted = set(PLANTED)
    zeros = [v for v in range(1, BIG_N) if v not in planted and (0, v) not in excluded][:len(src) - k]
    assert len(zeros) == len(src) - k and zeros[-1] > 46208             # the tail lies in row 0 and crosses the border
    assert (src[k:] == 0).all() and dst[k:].tolist() == zeros and (logit[k:] == 0).all() and not torch.signbit(logit[k:]).any()


def test_link_graph_past_the_cap(big_graph):
    from disenlink_amd import ops
    Z, H, pairs = big_graph
    excluded = {(0, 127), (128, 65999), (46207, 46208), (46209, 65536)}
    ex = (torch.tensor([e[0] for e in excluded], device=DEV), torch.tensor([e[1] for e in excluded], device=DEV))
    rowptr, col, logit, prob = ops.score_links_blocks(Z, H, 1.0, 0.5, exclude=ex)
    keep = [p for p in pairs if (p[0], p[1]) not in excluded]
    entries = sorted([(u, v, x) for u, v, x in keep] + [(v, u, x) for u, v, x in keep])
    assert rowptr.shape == (BIG_N + 1,) and int(rowptr[-1]) == len(entries) == 2 * (780 - 4)
    rows = torch.repeat_interleave(torch.arange(BIG_N, device=DEV), rowptr[1:] - rowptr[:-1])
    assert rows.tolist() == [e[0] for e in entries] and col.tolist() == [e[1] for e in entries]
    assert logit.tolist() == [e[2] for e in entries] and (prob > 0.98).all()
    deg = ops.score_link_degrees_blocks(Z, H, 1.0, 0.5, exclude=ex)
    assert torch.equal(deg, rowptr[1:] - rowptr[:-1]) and int(deg.sum()) == len(entries)


# ---------------------------------------------------------------------- determinism
def raw_between(ZA, HA, ZB, HB, t, m, floor, poison):
    """the three entries themselves, every buffer pre-filled with ``poison`` -> all their outputs"""
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    (nA, K, d), nB = ZA.shape, ZB.shape[0]
    fill = lambda n, dt: torch.full((max(n, 1) * dt.itemsize,), poison, dtype=torch.uint8, device=DEV).view(dt)
    ws = fill(int(lib.dl_score_mine_between_workspace_bytes_dtype(nA, nB, K, d, 0, m)), torch.uint8)
    mined = [fill(m, dt) for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
    count = fill(1, torch.int64)
    head = (ZA.data_ptr(), HA.data_ptr(), nA, ZB.data_ptr(), HB.data_ptr(), nB, K, d, 0, float(t), None, None, float(floor))
    assert lib.dl_score_mine_between_dtype(*head, m, *(o.data_ptr() for o in mined), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                           ops._stream(), None) == 0
    ws = fill(int(lib.dl_score_links_between_workspace_bytes_dtype(nA, nB, K, d, 0)), torch.uint8)
    rpa, rpb = fill(nA + 1, torch.int64), fill(nB + 1, torch.int64)
    links = head + (None, ws.data_ptr(), ws.numel(), rpa.data_ptr(), rpb.data_ptr())
    assert lib.dl_score_links_between_count_dtype(*links, ops._stream()) == 0
    nnz = int(rpa[-1])
    assert nnz == int(rpb[-1])
    sides = [[fill(nnz, dt) for dt in (torch.int32, torch.float32, torch.float32)] for _ in range(2)]
    assert lib.dl_score_links_between_fill_dtype(*links, nnz, *(o.data_ptr() for o in sides[0]), nnz,
                                                 *(o.data_ptr() for o in sides[1]), ops._stream()) == 0
    return mined + [count, rpa, rpb] + sides[0] + sides[1]


def test_same_bits_on_every_call_and_over_other_garbage():
    from disenlink_amd import ops
    nA, nB, K, d, m = 300, 200, 3, 64, 300
    ZA, HA, ZB, HB, excl, rule = rect_case(nA, nB, K, d, 1.0)
    for kw in (dict(), dict(exclude=excl, rule=rule)):
        assert same(ops.score_mine_between(ZA, HA, ZB, HB, 1.0, 5000, min_logit=0.0, **kw),
                    ops.score_mine_between(ZA, HA, ZB, HB, 1.0, 5000, min_logit=0.0, **kw))
        one, two = (ops.score_links_between(ZA, HA, ZB, HB, 1.0, 0.0, **kw) for _ in range(2))
        assert same(one.ab, two.ab) and same(one.ba, two.ba)
    a, b = raw_between(ZA, HA, ZB, HB, 1.0, m, 0.0, 0x7F), raw_between(ZA, HA, ZB, HB, 1.0, m, 0.0, 0xFF)
    assert int(a[4]) == m and same(a, b)
    few = raw_between(ZA[:2].contiguous(), HA[:2].contiguous(), ZB[:3].contiguous(), HB[:3].contiguous(), 1.0, 16, NINF, 0x7F)
    c = int(few[4])                                                   # fewer candidates than m: the padding
    assert c == 3 and (few[0][c:] == -1).all() and (few[1][c:] == -1).all() and torch.isnan(few[2][c:]).all() and torch.isnan(few[3][c:]).all()
    Z, H = tables(300, 3, 40, seed=8)
    assert same(ops.score_mine_blocks(Z, H, 2.0, 4000, block_nodes=128), ops.score_mine_blocks(Z, H, 2.0, 4000, block_nodes=128))
    assert same(ops.score_links_blocks(Z, H, 2.0, 0.0, block_nodes=128), ops.score_links_blocks(Z, H, 2.0, 0.0, block_nodes=128))
