"""The node-group rule of the candidate scans (ops.NodeFilter; dl_score_*_filtered) against the UNFILTERED scans: for N
small enough to list them, a filtered call must return, bit for bit, what the unfiltered call returns when the pairs the rule
does not allow are added to its exclusion set.  (The unfiltered scans are pinned against fp64 in test_gpu_dense_fp64.py,
test_gpu_rank.py, test_gpu_mine.py and test_gpu_pair_ranks.py.)  Shapes: one tile, a second tile of two rows, three tiles
with a ragged last one; forced geometries put several tiles / tile pairs into one workgroup."""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(N, K, d, t) for N in (1, 130, 300) for K, d in ((1, 8), (3, 64)) for t in (1.0, 2.0)]
TOPK = 8


def tables(N, K, d, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (torch.randn(N, K, d, generator=g) / d ** 0.5).to(DEV)
    H = (torch.randn(N, K, d, generator=g) / d ** 0.5).to(DEV)
    return Z, H


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def rules(N, seed):
    """name -> NodeFilter (on the CPU): the smallest set at which the mask code can go wrong"""
    from disenlink_amd.ops import NodeFilter
    gen = torch.Generator().manual_seed(seed)
    idx = torch.arange(N)
    out = {"one": NodeFilter(torch.zeros(N, dtype=torch.int64), torch.ones(1, 1)),
           "random": NodeFilter.different(torch.randperm(N, generator=gen) % 2),
           "per_tile": NodeFilter(idx // 128 % 2, ~torch.eye(2, dtype=torch.bool)),
           "alternating": NodeFilter(idx % 2, ~torch.eye(2, dtype=torch.bool))}
    allow = torch.zeros(64, 64, dtype=torch.bool)                      # nodes in groups 0, 31, 32, 63; bit 63 in use
    for a, b in ((0, 0), (0, 31), (31, 63), (32, 32), (63, 63)):
        allow[a, b] = allow[b, a] = True
    out["wide"] = NodeFilter(torch.tensor([31, 32, 63, 0])[torch.randint(0, 4, (N,), generator=gen)] if N > 1
                             else torch.tensor([63]), allow)
    assert N == 1 or set(out["wide"].groups.tolist()) == {0, 31, 32, 63}
    out["asymmetric"] = NodeFilter(torch.randint(0, 2, (N,), generator=gen), torch.tensor([[False, True], [False, False]]))
    pool = torch.zeros(N, dtype=torch.bool)
    pool[torch.randperm(N, generator=gen)[:5]] = True
    out["pool"] = NodeFilter.candidates(pool)
    return out


MIXED = ("random", "alternating", "wide", "asymmetric")


def exclusion(N, seed, pool=None):
    """a dense [N, N] exclusion mask: a ring, random pairs and, with ``pool``, every pool member in row 0 and one pair
    inside the pool"""
    gen = torch.Generator().manual_seed(seed)
    ex = torch.zeros(N, N, dtype=torch.bool)
    ex[torch.arange(N), (torch.arange(N) + 1) % N] = True
    ex[torch.randint(0, N, (3 * N,), generator=gen), torch.randint(0, N, (3 * N,), generator=gen)] = True
    if pool is not None:
        ex[0, pool] = True
        members = torch.nonzero(pool).reshape(-1)
        if len(members) > 1:
            ex[members[0], members[1]] = True
    return ex


def check_inputs(name, f, N, allowed, ex, unordered):
    """on the CPU, before any launch: the case is not trivial"""
    if N == 1:
        return
    off = ~torch.eye(N, dtype=torch.bool)
    frac = float(allowed[off].float().mean())
    if name in MIXED:
        assert 0.1 <= frac <= 0.9, (name, frac)
    if name == "per_tile":
        nt = (N + 127) // 128
        blocks = [allowed[a * 128:(a + 1) * 128, b * 128:(b + 1) * 128] for a in range(nt) for b in range(a, nt)]
        assert any(bool(b.all()) for b in blocks) and any(not bool(b.any()) for b in blocks)
    if name != "one":                                                  # ("one" disallows nothing)
        e = (ex | ex.T) if unordered else ex
        assert (e & allowed & off).any() and (e & ~allowed & off).any() and (~e & ~allowed & off).any()


def target_pairs(N, allowed, seed, one_per_node):
    """(src, dst) on the CPU, src != dst: random targets and three pairs the rule allows and three it does not (where
    there are any); ``one_per_node``: a target for every node as well."""
    gen = torch.Generator().manual_seed(seed)
    if N == 1:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    src = torch.randint(0, N, (40,), generator=gen)
    if one_per_node:
        src = torch.cat([torch.arange(N), src])
    else:
        src = torch.cat([src, src[:5]])                                # repeated query nodes
    dst = (src + 1 + torch.randint(0, N - 1, (len(src),), generator=gen)) % N
    off = ~torch.eye(N, dtype=torch.bool)
    yes, no = torch.nonzero(allowed & off)[:3], torch.nonzero(~allowed & off)[-3:]
    extra = torch.cat([yes, no])
    return torch.cat([src, extra[:, 0]]), torch.cat([dst, extra[:, 1]])


@pytest.mark.parametrize("N,K,d,t", SHAPES)
def test_topk_equals_the_unfiltered_scan_with_the_rule_as_exclusion(N, K, d, t, lib_env):
    from disenlink_amd import ops
    Z, H = tables(N, K, d, seed=N + 7 * K + d)
    uu, vv = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    query_sets = [torch.arange(N), torch.tensor([N - 1, 0, N // 2, 0, N // 3, N - 1])]
    cases = []
    for name, f in rules(N, seed=N).items():
        allowed = f.allowed(uu.reshape(-1), vv.reshape(-1)).reshape(N, N)
        ex = exclusion(N, seed=3 * N + 1, pool=f.groups.bool() if name == "pool" else None)
        check_inputs(name, f, N, allowed, ex, unordered=False)
        if name == "pool" and N > 1:                                   # rows with fewer than k candidates, and one with none
            left = (allowed & ~ex & ~torch.eye(N, dtype=torch.bool)).sum(1)
            assert int(left[0]) == 0 and bool(((left > 0) & (left < TOPK)).any())
        cases.append((name, f.to(DEV), allowed.to(DEV), ex.to(DEV)))
    first = {}
    for name, f, allowed, ex in cases:
        for q in query_sets:
            for exclude_self in (True, False):
                got = ops.score_topk(Z, H, t, q, TOPK, exclude=ex, exclude_self=exclude_self, node_filter=f)
                want = ops.score_topk(Z, H, t, q, TOPK, exclude=ex | ~allowed, exclude_self=exclude_self)
                assert same(got, want), (name, exclude_self)
                if name == "one":
                    assert same(got, ops.score_topk(Z, H, t, q, TOPK, exclude=ex, exclude_self=exclude_self))
                index = got[0]
                rows = q.to(DEV)[:, None].expand_as(index)[index >= 0]
                assert bool(allowed[rows, index[index >= 0]].all()), name
                assert same(got, ops.score_topk(Z, H, t, q, TOPK, exclude=ex, exclude_self=exclude_self, node_filter=f))
                if q is query_sets[0] and exclude_self:
                    first[name] = got
    lib_env("DL_RANK_SLICES", 1)                                       # every candidate tile in one workgroup
    for name, f, allowed, ex in cases:
        assert same(first[name], ops.score_topk(Z, H, t, query_sets[0], TOPK, exclude=ex, node_filter=f)), name


@pytest.mark.parametrize("N,K,d,t", SHAPES)
def test_ranks_equal_the_unfiltered_scan_with_the_rule_as_exclusion(N, K, d, t, lib_env):
    from disenlink_amd import ops
    Z, H = tables(N, K, d, seed=N + 7 * K + d + 1)
    uu, vv = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    cases = []
    for name, f in rules(N, seed=N + 1).items():
        allowed = f.allowed(uu.reshape(-1), vv.reshape(-1)).reshape(N, N)
        ex = exclusion(N, seed=3 * N + 2)
        check_inputs(name, f, N, allowed, ex, unordered=False)
        for one_per_node in (True, False):
            src, dst = target_pairs(N, allowed, seed=N + 5, one_per_node=one_per_node)
            if N == 1:
                src, dst = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)      # the one pair there is
            elif name != "one":                                        # allowed and disallowed targets
                assert bool(allowed[src, dst].any()) and not bool(allowed[src, dst].all()), name
            cases.append((name, f.to(DEV), allowed.to(DEV), ex.to(DEV), src.to(DEV), dst.to(DEV)))
    first = {}
    for name, f, allowed, ex, src, dst in cases:
        got = ops.score_ranks(Z, H, t, src, dst, exclude=ex, node_filter=f)
        want = ops.score_ranks(Z, H, t, src, dst, exclude=ex | ~allowed)
        assert same(got, want), name
        if name == "one":
            assert same(got, ops.score_ranks(Z, H, t, src, dst, exclude=ex))
        assert same(got, ops.score_ranks(Z, H, t, src, dst, exclude=ex, node_filter=f))
        first[(name, len(src))] = got
    lib_env("DL_RANK_SLICES", 1)
    for name, f, allowed, ex, src, dst in cases:
        assert same(first[(name, len(src))], ops.score_ranks(Z, H, t, src, dst, exclude=ex, node_filter=f)), name


def unordered_cases(N, seed):
    uu, vv = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    cases = []
    for name, f in rules(N, seed=seed).items():
        if name == "asymmetric":                                       # refused by the unordered scans (test_node_filter_cpu.py)
            continue
        allowed = f.allowed(uu.reshape(-1), vv.reshape(-1), unordered=True).reshape(N, N)
        assert torch.equal(allowed, allowed.T)
        ex = exclusion(N, seed=3 * N + 3, pool=f.groups.bool() if name == "pool" else None)
        check_inputs(name, f, N, allowed, ex, unordered=True)
        n_cand = int((torch.triu(allowed, 1) & ~(ex | ex.T)).sum())    # counted on the CPU
        cases.append((name, f.to(DEV), allowed.to(DEV), ex.to(DEV), n_cand))
    return cases


@pytest.mark.parametrize("N,K,d,t", SHAPES)
def test_mine_equals_the_unfiltered_scan_with_the_rule_as_exclusion(N, K, d, t, lib_env):
    from disenlink_amd import ops
    Z, H = tables(N, K, d, seed=N + 7 * K + d + 2)
    cases = unordered_cases(N, seed=N + 2)
    first = {}
    for name, f, allowed, ex, n_cand in cases:
        for m, floor in ((50, float("-inf")), (1000, 0.0)):            # min_prob = 0.5 as its logit floor
            got = ops.score_mine(Z, H, t, m, exclude=ex, min_logit=floor, node_filter=f)
            want = ops.score_mine(Z, H, t, m, exclude=ex | ~allowed, min_logit=floor)
            assert same(got, want), (name, m)
            if name == "one":
                assert same(got, ops.score_mine(Z, H, t, m, exclude=ex, min_logit=floor))
            assert bool(allowed[got[0].long(), got[1].long()].all()) and bool((got[0] < got[1]).all()), name
            if floor == float("-inf"):
                assert len(got[0]) == min(m, n_cand), name
            assert same(got, ops.score_mine(Z, H, t, m, exclude=ex, min_logit=floor, node_filter=f))
            first[(name, m)] = got
    lib_env("DL_MINE_TILES", 4)                                        # runs of tile pairs in one workgroup
    for name, f, allowed, ex, n_cand in cases:
        for m, floor in ((50, float("-inf")), (1000, 0.0)):
            assert same(first[(name, m)], ops.score_mine(Z, H, t, m, exclude=ex, min_logit=floor, node_filter=f)), name


@pytest.mark.parametrize("N,K,d,t", SHAPES)
def test_pair_ranks_equal_the_unfiltered_scan_with_the_rule_as_exclusion(N, K, d, t, lib_env):
    from disenlink_amd import ops
    Z, H = tables(N, K, d, seed=N + 7 * K + d + 3)
    cases = unordered_cases(N, seed=N + 3)
    first = {}
    for name, f, allowed, ex, n_cand in cases:
        src, dst = target_pairs(N, allowed.cpu(), seed=N + 6, one_per_node=False)
        if N > 1 and name != "one":                                    # allowed and disallowed targets
            hit = allowed.cpu()[src, dst]
            assert bool(hit.any()) and not bool(hit.all()), name
        got = ops.score_pair_ranks_counted(Z, H, t, src, dst, exclude=ex, node_filter=f)
        want = ops.score_pair_ranks_counted(Z, H, t, src, dst, exclude=ex | ~allowed)
        assert same(got, want), name
        assert int(got[4]) == n_cand, (name, int(got[4]), n_cand)      # the DEVICE count (at N = 1: the host's, no scan runs)
        if len(src):
            assert bool((got[0] + got[1] <= got[3]).all())
        if name == "one":
            assert same(got, ops.score_pair_ranks_counted(Z, H, t, src, dst, exclude=ex))
        assert same(got, ops.score_pair_ranks_counted(Z, H, t, src, dst, exclude=ex, node_filter=f))
        assert same(got[:4], ops.score_pair_ranks(Z, H, t, src, dst, exclude=ex, node_filter=f))
        first[name] = (got, src, dst)
    lib_env("DL_MINE_TILES", 4)
    for name, f, allowed, ex, n_cand in cases:
        got, src, dst = first[name]
        assert same(got, ops.score_pair_ranks_counted(Z, H, t, src, dst, exclude=ex, node_filter=f)), name


def test_a_filter_on_the_wrong_device_or_of_the_wrong_kind_is_refused():
    from disenlink_amd import ops
    Z, H = tables(6, 1, 8, seed=1)
    f = ops.NodeFilter.different(torch.tensor([0, 1, 0, 1, 0, 1]))
    with pytest.raises(ValueError, match="use NodeFilter.to"):
        ops.score_mine(Z, H, 1.0, 3, node_filter=f)
    asym = ops.NodeFilter(torch.tensor([0, 1, 0, 1, 0, 1]), torch.tensor([[0, 1], [0, 0]])).to(DEV)
    with pytest.raises(ValueError, match="symmetric"):
        ops.score_pair_ranks(Z, H, 1.0, torch.tensor([0]), torch.tensor([1]), node_filter=asym)
    assert len(ops.score_topk(Z, H, 1.0, torch.arange(6), 2, node_filter=asym)[0]) == 6


def test_top_missing_links_of_different_groups_on_a_golden_model():
    from conftest import golden_case_names, load_golden
    from disenlink_amd.model import Disentangle
    from disenlink_amd.ops import NodeFilter
    g = load_golden(golden_case_names()[0])
    meta = g["meta"]
    model = Disentangle(meta["F"], meta["nhid"], meta["d"], nfactor=meta["K"], beta=meta["beta"], t=meta["t"])
    model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")})
    model = model.to(DEV)
    x, adj = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["adj"]).to(DEV)
    N = meta["N"]
    groups = (torch.arange(N) * 7 % 3).to(DEV)
    same_group = groups[:, None] == groups[None, :]
    known = adj.bool() | adj.bool().T
    m = max(1, int((torch.triu(~same_group, 1) & ~known).sum()) // 2)
    mined = model.top_missing_links(x, adj, m, node_filter=NodeFilter.different(groups))
    assert len(mined.src) == m
    assert bool((groups[mined.src.long()] != groups[mined.dst.long()]).all())
    assert not bool(known[mined.src.long(), mined.dst.long()].any())
    assert same(mined, model.top_missing_links(x, adj, m, exclude=known | same_group))
    n = min(5, m)                                                      # the i-th mined link has i candidates above it
    ranks = model.missing_link_ranks(x, adj, mined.src[:n], mined.dst[:n], node_filter=NodeFilter.different(groups))
    place = torch.arange(n, device=DEV)
    assert bool(((ranks.greater <= place) & (place <= ranks.greater + ranks.ties)).all())
    assert same([ranks.logit], [mined.logit[:n]])


def test_cli_mines_only_links_that_obey_the_rule(tmp_path):
    from disenlink_amd.main import build_parser, load_dataset, main
    ds = load_dataset(build_parser().parse_args(["--dataset", "squirrel", "--synthetic"]))
    groups = np.random.default_rng(3).integers(0, 3, ds.n_nodes)
    gfile, out = tmp_path / "groups.txt", tmp_path / "mined.txt"
    np.savetxt(gfile, groups, fmt="%d")
    with contextlib.redirect_stdout(io.StringIO()):
        main(["--dataset", "squirrel", "--synthetic", "--epochs", "3", "--run", "1", "--quiet", "--mine", "20",
              "--mine-out", str(out), "--node-groups", str(gfile), "--link-rule", "different"])
    rows = [ln.split() for ln in out.read_text().splitlines()]
    assert len(rows) == 20
    src, dst = np.array([int(r[0]) for r in rows]), np.array([int(r[1]) for r in rows])
    assert (src < dst).all() and (groups[src] != groups[dst]).all()
    known = set(zip(np.asarray(ds.src).tolist(), np.asarray(ds.dst).tolist()))
    assert not any((a, b) in known or (b, a) in known for a, b in zip(src.tolist(), dst.tolist()))
