"""The thresholded link graph (ops.score_links, ops.score_link_degrees, Disentangle.predicted_links, --predict-links):
exact against the enumerated pairs (ops.score_pair_logits + links_ref.select_links), against the fp64 reference of
tests/mine_ref.py, the set ops.score_mine lists, the node-group rules of test_gpu_node_filter.py, the reference model's own
link_pred (tests/golden) and the CLI."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

import links_ref
import mine_ref
from conftest import golden_case_names, load_golden
from links_ref import select_links, upper_pairs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF, NINF = float("inf"), float("-inf")
POISON_BITS = -1                                                      # DL_POISON fills with 0xFF bytes


def tables(N, K, d, seed=0, scale=1.0):
    return links_ref.tables(N, K, d, seed, scale, DEV)


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def enumerate_logits(Z, H, t):
    """S [N,N]: S[u,v] for u < v from ops.score_pair_logits (the smaller endpoint as the A operand), NaN elsewhere"""
    from disenlink_amd import ops
    N = Z.shape[0]
    u, v = torch.triu_indices(N, N, 1, device=DEV)
    S = torch.full((N, N), float("nan"), device=DEV)
    if u.numel():
        S[u, v] = ops.score_pair_logits(Z, H, t, u, v)
    return S


def assert_layout(out, N):
    rowptr, col, logit, prob = out
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and logit.dtype == torch.float32 and prob.dtype == torch.float32
    assert rowptr.shape == (N + 1,) and int(rowptr[0]) == 0 and int(rowptr[-1]) == len(col) == len(logit) == len(prob)
    assert (rowptr[1:] >= rowptr[:-1]).all()


def assert_equals_reference(out, S, N, excluded=None, floor=NINF):
    """bit for bit the selection of links_ref.select_links, in both orientations, and prob = sigmoid(logit)"""
    assert_layout(out, N)
    rowptr, col, logit, prob = out
    rp, rc, rl = select_links(S, excluded, floor)
    assert torch.equal(rowptr, rp) and torch.equal(col.long(), rc) and torch.equal(bits(logit), bits(rl))
    ref = 1.0 / (1.0 + torch.exp(-logit.double()))
    np.testing.assert_allclose(prob.cpu().numpy(), ref.float().cpu().numpy(), rtol=1e-6, atol=1e-7)


def floors_of(S):
    """-inf, the fp32 median, a floor equal to one actual logit, a floor above the maximum, +inf"""
    N = S.shape[0]
    x = S[torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)]
    x = x[~torch.isnan(x)]
    if x.numel() == 0:
        return [NINF, 0.0, INF]
    srt = torch.sort(x).values
    above = float(np.nextafter(np.float32(float(srt[-1])), np.float32(INF)))
    return [NINF, float(torch.median(x)), float(srt[(3 * len(srt)) // 4]), above, INF]


@pytest.mark.parametrize("N,KD,t", links_ref.GPU_CASES)
def test_exact_against_the_enumerated_pairs(N, KD, t):
    from disenlink_amd import ops
    K, d = KD
    Z, H = tables(N, K, d, seed=links_ref.case_seed(N, K, d, t))
    S = enumerate_logits(Z, H, t)
    floors = floors_of(S)
    for i, floor in enumerate(floors):
        out = ops.score_links(Z, H, t, floor)
        assert_equals_reference(out, S, N, None, floor)
        deg = out[0][1:] - out[0][:-1]
        if floor == NINF:
            assert (deg == N - 1).all()
        if N >= 2 and i >= len(floors) - 2:                           # above the maximum, and +inf: nothing
            assert not out[0].any() and len(out[1]) == 0
    if N >= 2:                                                        # the floor that equals a logit keeps that logit
        out = ops.score_links(Z, H, t, floors[2])
        assert len(out[2]) and float(out[2].min()) == floors[2]


@pytest.mark.parametrize("N,KD,t", links_ref.GPU_CASES)
def test_against_fp64(N, KD, t):
    from disenlink_amd import ops
    K, d = KD
    Z, H = tables(N, K, d, seed=links_ref.case_seed(N, K, d, t))
    s64, band = mine_ref.logits64(Z, H, t)
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    # a floor at the fp64 median of the candidates: a condition on the seed, judged on the reference alone
    floor = float(torch.median(s64[iu])) if N >= 2 else 0.0
    straddle = iu & (s64 - band < floor) & (s64 + band >= floor)
    assert int(straddle.sum()) <= max(1, int(0.01 * int(iu.sum())))
    out = ops.score_links(Z, H, t, floor)
    assert_layout(out, N)
    u, v, logit = upper_pairs(out[0], out[1], out[2])
    got = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    got[u, v] = True
    assert int(got.sum()) == len(u) and 2 * len(u) == len(out[1])
    sure, never = iu & (s64 - band >= floor), iu & (s64 + band < floor)
    assert got[sure].all() and not got[never].any()
    assert (logit.double() - s64[u, v]).abs().le(band[u, v] + 1e-30).all()
    # the mirrored entries carry the same bits
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), out[0][1:] - out[0][:-1])
    D = torch.zeros(N, N, dtype=torch.int32, device=DEV)
    D[rows, out[1].long()] = bits(out[2])
    assert torch.equal(D, D.T)


@pytest.mark.parametrize("N", [129, 300])
def test_the_same_set_as_score_mine(N):
    from disenlink_amd import ops
    K, d, t = 3, 40, 2.0
    Z, H = tables(N, K, d, seed=21 + N)
    ex = (torch.tensor([0, 3, N - 1, 128], device=DEV), torch.tensor([2, 1, 0, 5], device=DEV))
    total = N * (N - 1) // 2
    assert total <= 65536
    for exclude in (None, ex):
        for floor in (NINF, 0.0, 0.05):
            out = ops.score_links(Z, H, t, floor, exclude=exclude)
            u, v, logit, prob = upper_pairs(*out)
            src, dst, lg, pr = ops.score_mine(Z, H, t, total, exclude=exclude, min_logit=floor)
            assert len(src) == len(u) > 0
            order = torch.argsort(src.long() * N + dst.long())
            assert torch.equal(u, src.long()[order]) and torch.equal(v, dst.long()[order])
            assert torch.equal(bits(logit), bits(lg[order])) and torch.equal(bits(prob), bits(pr[order]))


def test_exclusion_forms_agree_and_either_orientation_counts():
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph
    N, K, d = 150, 3, 64
    Z, H = tables(N, K, d, seed=3)
    rng = np.random.default_rng(3)
    s, t_ = torch.from_numpy(rng.integers(0, N, 2500)).to(DEV), torch.from_numpy(rng.integers(0, N, 2500)).to(DEV)
    mask = torch.zeros(N, N, device=DEV)
    mask[s, t_] = 1                                                   # one orientation only
    G = Graph.from_edge_rows(s, t_, N)
    S = enumerate_logits(Z, H, 1.0)
    for floor in (NINF, 0.0):
        outs = [ops.score_links(Z, H, 1.0, floor, exclude=e) for e in (G, mask, (s, t_), (t_, s))]
        assert all(same(outs[0], o) for o in outs[1:])
        assert_equals_reference(outs[0], S, N, mask.bool(), floor)
    free = ops.score_links(Z, H, 1.0, 0.0)
    u, v = (int(x[0]) for x in upper_pairs(free[0], free[1]))         # its first pair, listed only as (v, u)
    only = ops.score_links(Z, H, 1.0, 0.0, exclude=(torch.tensor([v]), torch.tensor([u])))
    one = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    one[u, v] = True
    assert len(only[1]) == len(free[1]) - 2
    assert_equals_reference(only, S, N, one, 0.0)


@pytest.mark.parametrize("N,K,d,t", [(N, K, d, t) for N in (1, 130, 300) for K, d, t in ((1, 8, 1.0), (3, 64, 2.0))])
def test_node_filter_equals_the_rule_as_exclusion(N, K, d, t, lib_env):
    """every NodeFilter rule of test_gpu_node_filter.py: the bits of the unfiltered call with the disallowed pairs excluded"""
    from disenlink_amd import ops
    from test_gpu_node_filter import unordered_cases
    Z, H = tables(N, K, d, seed=N + 7 * K + d + 2)
    cases = unordered_cases(N, seed=N + 2)
    assert {c[0] for c in cases} == {"one", "random", "per_tile", "alternating", "wide", "pool"}
    first = {}
    for name, f, allowed, ex, n_cand in cases:
        for floor in (NINF, 0.0):
            got = ops.score_links(Z, H, t, floor, exclude=ex, node_filter=f)
            want = ops.score_links(Z, H, t, floor, exclude=ex | ~allowed)
            assert same(got, want), (name, floor)
            if name == "one":
                assert same(got, ops.score_links(Z, H, t, floor, exclude=ex))
            u, v = upper_pairs(got[0], got[1])
            assert bool(allowed[u, v].all()), name
            if floor == NINF:
                assert len(u) == n_cand, name
            assert torch.equal(ops.score_link_degrees(Z, H, t, floor, exclude=ex, node_filter=f), got[0][1:] - got[0][:-1])
            first[(name, floor)] = got
    lib_env("DL_MINE_TILES", 4)                                       # runs of tile pairs in one workgroup
    for name, f, allowed, ex, n_cand in cases:
        for floor in (NINF, 0.0):
            assert same(first[(name, floor)], ops.score_links(Z, H, t, floor, exclude=ex, node_filter=f)), name


def test_a_filter_on_the_wrong_device_is_refused():
    from disenlink_amd import ops
    Z, H = tables(6, 1, 8, seed=1)
    f = ops.NodeFilter.different(torch.tensor([0, 1, 0, 1, 0, 1]))
    with pytest.raises(ValueError, match="use NodeFilter.to"):
        ops.score_links(Z, H, 1.0, 0.0, node_filter=f)
    asym = ops.NodeFilter(torch.tensor([0, 1, 0, 1, 0, 1]), torch.tensor([[0, 1], [0, 0]])).to(DEV)
    with pytest.raises(ValueError, match="symmetric"):
        ops.score_link_degrees(Z, H, 1.0, 0.0, node_filter=asym)


def test_zeros_of_either_sign_and_exact_ties():
    from disenlink_amd import ops
    N, K, d = 200, 2, 32
    Z, H = tables(N, K, d, seed=31)
    zero = torch.from_numpy(np.random.default_rng(31).choice(N, 120, replace=False)).to(DEV)
    H[zero] = 0.0
    H[zero[:40], :, ::2] = -0.0                                       # products of either sign of zero
    live = torch.ones(N, dtype=torch.bool, device=DEV)
    live[zero] = False
    a, b = torch.nonzero(live)[:2, 0].tolist()
    Z[b], H[b] = Z[a], H[a]                                           # a duplicated row: exact ties among the live logits
    S = enumerate_logits(Z, H, 1.0)
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    n_zero = int((iu & (S == 0)).sum())
    assert n_zero > 5000
    out = ops.score_links(Z, H, 1.0, 0.0)                             # every zero reaches the floor of 0, as +0
    assert_equals_reference(out, S, N, None, 0.0)
    assert int((out[2] == 0).sum()) == 2 * n_zero and not torch.signbit(out[2]).any()
    tie = float(S[a, b + 1]) if b + 1 < N and bool(live[b + 1]) else float(S[a, torch.nonzero(live)[2, 0]])
    out = ops.score_links(Z, H, 1.0, tie)                             # a floor inside a tie: both of its pairs stay
    assert_equals_reference(out, S, N, None, tie)
    assert int((out[2] == tie).sum()) >= 4


def test_overflow_inf_always_nan_never():
    from disenlink_amd import ops
    N, d = 90, 32
    Z, H = tables(N, 1, d, seed=7)
    Z[:45] = 4.0                                                      # z.z = 512: exp overflows
    H[:20] = 0.25                                                     # h.h > 0: +inf
    H[20:30] = 0.25
    H[20:30, :, ::2] = -0.5                                           # against rows 0..19: h.h < 0: -inf
    H[30:45] = 0.0                                                    # h.h = 0 against inf: NaN
    S = enumerate_logits(Z, H, 1.0)
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    n_pinf, n_ninf, n_nan = int((iu & (S == INF)).sum()), int((iu & (S == NINF)).sum()), int((iu & torch.isnan(S)).sum())
    assert n_pinf >= 190 and n_ninf >= 200 and n_nan >= 15 * 30
    total = N * (N - 1) // 2
    for floor, want in ((NINF, total - n_nan), (-3.0e38, total - n_nan - n_ninf), (3.0e38, n_pinf), (INF, n_pinf)):
        out = ops.score_links(Z, H, 1.0, floor)
        assert_equals_reference(out, S, N, None, floor)
        assert len(out[1]) == 2 * want and not torch.isnan(out[2]).any() and not torch.isnan(out[3]).any()
        assert int((out[2] == INF).sum()) == 2 * n_pinf and (out[3][out[2] == INF] == 1).all()


def test_bitwise_reproducible_under_any_geometry(lib_env):
    from disenlink_amd import ops
    N, K, d = 700, 3, 64                                              # 6 tiles, 21 tile pairs
    Z, H = tables(N, K, d, seed=13)
    H[100:400] = 0.0
    excl = (torch.arange(N, device=DEV), (torch.arange(N, device=DEV) + 1) % N)
    ref = ops.score_links(Z, H, 1.0, 0.0, exclude=excl)
    assert_layout(ref, N)
    assert int((ref[2] == 0).sum()) > 1000 and int((ref[2] > 0).sum()) > 1000
    assert int(ref[1].min()) >= 0 and int(ref[1].max()) < N
    assert not (bits(ref[2]) == POISON_BITS).any() and not (bits(ref[3]) == POISON_BITS).any()      # every slot was written
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), ref[0][1:] - ref[0][:-1])
    key = rows * N + ref[1].long()
    assert (key[1:] > key[:-1]).all() and (rows != ref[1]).all()      # strictly ascending columns within every row
    assert same(ref, ops.score_links(Z, H, 1.0, 0.0, exclude=excl))
    for tiles in (1, 4, 21):                                          # DL_MINE_TILES: tile pairs per workgroup (21 = all of them)
        lib_env("DL_MINE_TILES", tiles)
        assert same(ref, ops.score_links(Z, H, 1.0, 0.0, exclude=excl))
        assert torch.equal(ops.score_link_degrees(Z, H, 1.0, 0.0, exclude=excl), ref[0][1:] - ref[0][:-1])
    # the same pairs as score_mine lists at a floor that keeps them below its cap
    lib_env("DL_MINE_TILES")
    floor = float(torch.sort(ref[2]).values[-20001])
    out = ops.score_links(Z, H, 1.0, floor, exclude=excl)
    u, v, logit = upper_pairs(out[0], out[1], out[2])
    src, dst, lg, _ = ops.score_mine(Z, H, 1.0, 65536, exclude=excl, min_logit=floor)
    order = torch.argsort(src.long() * N + dst.long())
    assert 0 < len(u) == len(src) < 65536
    assert torch.equal(u, src.long()[order]) and torch.equal(v, dst.long()[order]) and torch.equal(bits(logit), bits(lg[order]))


def test_a_short_fill_writes_nothing_out_of_bounds():
    """dl_score_links_fill with an nnz below the count's: slots >= nnz are skipped, the slots below it are the same bits"""
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    N, K, d = 300, 2, 32
    Z, H = tables(N, K, d, seed=17)
    full = ops.score_links(Z, H, 1.0, 0.0)
    nnz = len(full[1])
    ws = torch.full((int(lib.dl_score_links_workspace_bytes(N, K, d)),), 0x7F, dtype=torch.uint8, device=DEV)
    rowptr = torch.full((N + 1,), -7, dtype=torch.int64, device=DEV)
    head = (Z.data_ptr(), H.data_ptr(), N, K, d, 1.0, None, None, 0.0, None, ws.data_ptr(), ws.numel(), rowptr.data_ptr())
    assert lib.dl_score_links_count(*head, ops._stream()) == 0
    assert torch.equal(rowptr, full[0])
    short = nnz // 2
    col = torch.full((nnz,), -5, dtype=torch.int32, device=DEV)
    logit = torch.full((nnz,), -5.0, device=DEV)
    assert lib.dl_score_links_fill(*head, short, col.data_ptr(), logit.data_ptr(), None, ops._stream()) == 0      # prob not wanted
    assert torch.equal(col[:short], full[1][:short]) and torch.equal(bits(logit[:short]), bits(full[2][:short]))
    assert (col[short:] == -5).all() and (logit[short:] == -5.0).all()
    assert lib.dl_score_links_fill(*head, 0, None, None, None, ops._stream()) == 0


def test_argument_errors():
    from disenlink_amd import ops, _lib
    Z, H = tables(10, 2, 32)
    with pytest.raises(ValueError, match="46340"):
        big = torch.zeros(46341, 1, 1, device=DEV)
        ops.score_links(big, big, 1.0, 0.0)
    with pytest.raises(_lib.DisenlinkHipError):
        Zw, Hw = tables(10, 1, 130)
        ops.score_links(Zw, Hw, 1.0, 0.0)
    with pytest.raises(TypeError, match="fp32"):
        ops.score_links(Z.bfloat16(), H.bfloat16(), 1.0, 0.0)
    with pytest.raises(ValueError):
        ops.score_links(Z, H, 1.0, 0.0, exclude=(torch.tensor([10]), torch.tensor([0])))
    with pytest.raises(_lib.DisenlinkHipError, match="temperature is 0"):
        ops.score_link_degrees(Z, H, 0.0, 0.0)


GOLDEN_P = links_ref.GOLDEN_P


def assert_links_of(links, lp, p, cand):
    """links == cand & (lp >= p), leaving out only the pairs whose lp lies within test_gpu_parity.py's tolerance for
    link_pred of p, at most 1 % of the candidates (judged on lp alone); prob = lp within that tolerance"""
    N = lp.shape[0]
    doubt = (lp - p).abs() <= 1e-5 + 1e-5 * lp.abs()
    assert int((doubt & cand).sum()) <= 0.01 * int(cand.sum())
    u, v, logit, prob = links.pairs()
    got = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    got[u, v] = True
    assert int(got.sum()) == len(u) and not (got & ~cand).any()
    assert torch.equal(got & ~doubt, cand & (lp >= p) & ~doubt)
    np.testing.assert_allclose(prob.cpu().numpy(), lp[u, v].cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(links.degree, (got | got.T).sum(1))
    return got, doubt


@pytest.mark.parametrize("name", golden_case_names())
def test_predicted_links_against_the_reference_link_pred(name):
    from disenlink_amd.model import Disentangle, PredictedLinks
    g = load_golden(name)
    meta = g["meta"]
    model = Disentangle(meta["F"], meta["nhid"], meta["d"], nfactor=meta["K"], beta=meta["beta"], t=meta["t"])
    model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")})
    model = model.to(DEV)
    x, adj = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["adj"]).to(DEV)
    N, p = meta["N"], GOLDEN_P[name]
    ref = torch.from_numpy(g["link_pred"]).double().to(DEV)           # the reference model's own link_pred
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    edges = adj.bool() | adj.bool().T
    none = (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    for exclude, cand in ((none, iu), (None, iu & ~edges)):
        links = model.predicted_links(x, adj, p, exclude=exclude)
        assert isinstance(links, PredictedLinks) and links.n_nodes == N
        assert_layout(links, N)
        got, _ = assert_links_of(links, ref, p, cand)
    given = model.predicted_links(x, adj, p, exclude=torch.nonzero(edges, as_tuple=True))
    assert same(links, given)                                         # exclude=None: the edges of adj
    G = links.to_graph()
    assert G.n_nodes == N and G.n_edges == 2 * int(got.sum())
    if G.n_edges:
        with torch.no_grad():
            emb, lp = model(x, G)                                     # the predicted graph runs through forward
        assert emb.shape[0] == N and lp.shape == (N, N) and torch.isfinite(emb).all()


def test_sparse_features_give_the_dense_result_on_cora():
    """tests/golden/real_cora.npz: SparseFeatures and dense features give the links of the module's own dense link_pred (the
    gathers' rounding against the GEMM's: the same links away from the threshold, the same probabilities in tolerance)"""
    import os
    from conftest import GOLDEN_DIR
    from disenlink_amd.features import SparseFeatures
    from disenlink_amd.graph import Graph
    from disenlink_amd.model import Disentangle
    g = np.load(os.path.join(GOLDEN_DIR, "real_cora.npz"))
    m = json.loads(str(g["meta"]))
    edges = torch.from_numpy(g["edges"].astype(np.int64)).to(DEV)
    N, F = (int(v) for v in g["feat_shape"])
    row, col = g["feat_row"].astype(np.int64), g["feat_col"].astype(np.int64)
    sf = SparseFeatures.from_coo(row, col, (N, F)).to(DEV)
    xd = torch.zeros(N, F, device=DEV)
    xd[torch.from_numpy(row).to(DEV), torch.from_numpy(col).to(DEV)] = 1.0
    G = Graph.from_edge_rows(edges[:, 0], edges[:, 1], N)
    torch.manual_seed(m["seed"])
    model = Disentangle(F, m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"]).to(DEV)
    with torch.no_grad():
        lp = model(xd, G)[1].double()
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), (G.rowptr[1:] - G.rowptr[:-1]).long())
    known = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    known[rows, G.col.long()] = True
    cand = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1) & ~known
    p = float(torch.quantile(lp[cand][::97].float(), 0.9))            # about a tenth of the candidates pass
    dense, doubt = assert_links_of(model.predicted_links(xd, G, p), lp, p, cand)
    sparse, _ = assert_links_of(model.predicted_links(sf, G, p), lp, p, cand)
    assert int(dense.sum()) > 1000 and not ((dense ^ sparse) & ~doubt).any()      # they differ only inside the tolerance of p


def test_cli_predict_links_prints_and_writes_what_the_module_gives(tmp_path):
    from disenlink_amd import main as cli
    groups = tmp_path / "groups.txt"
    ds = cli.load_dataset(cli.build_parser().parse_args(["--dataset", "squirrel", "--synthetic"]))
    groups.write_text("\n".join(str(i % 3) for i in range(ds.n_nodes)) + "\n")
    out = tmp_path / "links.txt"
    seen = {}
    real = cli.predict_links

    def spy(*args, **kwargs):
        seen["links"] = real(*args, **kwargs)
        return seen["links"]
    cli.predict_links = spy
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            cli.main(["--dataset", "squirrel", "--synthetic", "--epochs", "1", "--run", "1", "--quiet", "--predict-links", "0.7",
                      "--links-out", str(out), "--node-groups", str(groups), "--link-rule", "different"])
    finally:
        cli.predict_links = real
    links = seen["links"]
    src, dst, _, prob = (t.cpu().numpy() for t in links.pairs())
    line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("predicted ")]
    assert len(line) == 1
    words = line[0].split()
    n = ds.n_nodes
    deg = links.degree.cpu().numpy()
    assert int(words[1]) == len(src) > 0 and words[2] == "links"
    assert float(words[words.index("density") + 1]) == pytest.approx(len(src) / (n * (n - 1) / 2), rel=1e-5)
    assert float(words[words.index("mean") + 2]) == pytest.approx(deg.mean(), rel=1e-5) and int(words[-1]) == deg.max()
    rows = [ln.split() for ln in out.read_text().splitlines()]
    assert len(rows) == len(src) and all(len(r) == 3 for r in rows)
    assert [int(r[0]) for r in rows] == src.tolist() and [int(r[1]) for r in rows] == dst.tolist()
    np.testing.assert_allclose([float(r[2]) for r in rows], prob, rtol=1e-8)
    assert (src < dst).all() and (prob >= np.float32(0.7) - 1e-6).all() and (src % 3 != dst % 3).all()
    known = set(zip(np.asarray(ds.src).tolist(), np.asarray(ds.dst).tolist()))
    assert not any((a, b) in known or (b, a) in known for a, b in zip(src.tolist(), dst.tolist()))
