"""The reference of the global pair ranks on hand-made matrices, metrics.global_ranking_metrics, the host-only plan of
dl_score_pair_ranks, what the GPU test's case lists reach, and the CLI flag (no GPU needed)."""
import math

import numpy as np
import pytest
import torch

import pair_rank_ref
from pair_rank_ref import counts_from_list, order_key, pair_ranks, targets_for

INF, NAN = float("inf"), float("nan")


def _upper(rows):
    return torch.triu(torch.tensor(rows, dtype=torch.float64), 1)


def test_ties_and_duplicates_of_a_target():
    #            (0,1) (0,2) (0,3)       (1,2) (1,3)        (2,3)
    S = _upper([[0, 5.0, 3.0, 5.0], [0, 0, 1.0, 3.0], [0, 0, 0, 7.0], [0, 0, 0, 0]])
    g, t, n = pair_ranks(S, [0, 3, 0, 2, 0], [1, 0, 1, 0, 2])         # (0,1), (3,0) = {0,3}, (0,1) again, {0,2}, {0,2}
    assert g.tolist() == [1, 1, 1, 3, 3]                               # above 5: 7;  above 3: 7, 5, 5
    assert t.tolist() == [1, 1, 1, 1, 1]                               # the other 5; the other 3 — a duplicate is not counted
    assert n.tolist() == [5] * 5
    g, t, n = pair_ranks(S, [2], [3])
    assert (g.tolist(), t.tolist(), n.tolist()) == ([0], [0], [5])
    S[3, 0] = 100.0                                                    # the lower triangle is never read
    assert pair_ranks(S, [2], [3])[0].tolist() == [0]


def test_target_inside_and_outside_the_exclusion_set_either_orientation():
    S = _upper([[0, 5.0, 3.0, 5.0], [0, 0, 1.0, 3.0], [0, 0, 0, 7.0], [0, 0, 0, 0]])
    ex = torch.zeros(4, 4, dtype=torch.bool)
    ex[3, 0] = True                                                    # the pair {0, 3}, listed as (3, 0)
    ex[2, 3] = True
    ex[1, 1] = True                                                    # a self pair excludes nothing
    g, t, n = pair_ranks(S, [0, 1, 0, 3], [3, 0, 2, 1], ex)           # candidates: (0,1) 5, (0,2) 3, (1,2) 1, (1,3) 3
    assert n.tolist() == [4, 3, 3, 3]                                  # {0,3} is excluded: all 4 are others
    assert g.tolist() == [0, 0, 1, 1] and t.tolist() == [1, 0, 1, 1]   # {0,3} = 5 is ranked although excluded: ties (0,1)
    assert ((g + t) <= n).all()
    sym = ex | ex.T
    assert all(torch.equal(a, b) for a, b in zip(pair_ranks(S, [0, 1], [3, 0], ex), pair_ranks(S, [3, 0], [0, 1], sym)))


def test_signed_zeros_infinities_and_nan():
    #            (0,1)  (0,2)  (0,3) (0,4)       (1,2) (1,3) (1,4)      (2,3) (2,4)       (3,4)
    S = _upper([[0, 0.0, -0.0, INF, NAN], [0, 0, -INF, INF, NAN], [0, 0, 0, 2.0, -1.0], [0, 0, 0, 0, NAN], [0] * 5])
    src, dst = torch.triu_indices(5, 5, 1)
    g, t, n = pair_ranks(S, src, dst)
    val = S[src, dst].tolist()
    exp_g = {0.0: 3, INF: 0, -INF: 6, 2.0: 2, -1.0: 5}
    for i, x in enumerate(val):
        if math.isnan(x):
            assert (int(g[i]), int(t[i])) == (7, 2)                    # NaN: below every value, equal to the other two NaN
        else:
            assert int(g[i]) == exp_g[x] and int(t[i]) == (1 if x in (0.0, INF) else 0)      # -0 == +0, inf == inf
    assert n.tolist() == [9] * 10
    # the enumeration route of the GPU test gives the same counts
    lg = S[src, dst].float()
    g2, t2 = counts_from_list(lg[~torch.isnan(lg)], 3, lg, torch.ones(10, dtype=torch.bool))
    assert torch.equal(g2, g) and torch.equal(t2, t)
    k = order_key(torch.tensor([NAN, -INF, -1.0, -0.0, 0.0, 1e-45, 2.0, INF]))
    assert k[0] == 0 and k[3] == k[4] and (k[1:3] < k[3]).all() and (k[:-1] <= k[1:]).all() and int(k[-1]) == 0xFF800000


def test_no_targets_and_a_single_node():
    S = _upper([[0, 1.0], [0, 0]])
    assert all(x.numel() == 0 and x.dtype == torch.int64 for x in pair_ranks(S, [], []))
    assert all(x.numel() == 0 for x in pair_ranks(torch.zeros(1, 1, dtype=torch.float64), [], []))
    g, t, n = pair_ranks(S, [1], [0])
    assert (g.tolist(), t.tolist(), n.tolist()) == ([0], [0], [0])     # the only pair: nothing else to rank against


def test_reference_matches_a_plain_loop():
    g = torch.Generator().manual_seed(5)
    N = 9
    S = torch.randint(-3, 4, (N, N), generator=g).double()             # many ties
    ex = torch.rand(N, N, generator=g) < 0.15
    src, dst = targets_for(N, 3, n=20)
    G, T_, Nn = pair_ranks(S, src, dst, ex)
    for i, (a, b) in enumerate(zip(src.tolist(), dst.tolist())):
        lo, hi = min(a, b), max(a, b)
        gr = ti = no = 0
        for u in range(N):
            for v in range(u + 1, N):
                if ex[u, v] or ex[v, u] or (u, v) == (lo, hi):
                    continue
                no += 1
                gr += S[u, v] > S[lo, hi]
                ti += S[u, v] == S[lo, hi]
        assert (int(G[i]), int(T_[i]), int(Nn[i])) == (int(gr), int(ti), no)


def test_global_ranking_metrics_hand_computed():
    from disenlink_amd.metrics import global_ranking_metrics
    greater = torch.tensor([0, 0, 3, 99, 5000])
    ties = torch.tensor([0, 2, 0, 1, 0])
    n = torch.tensor([10000, 10000, 9999, 10000, 9999])
    r = global_ranking_metrics(greater, ties, n, ms=(100, 1000))
    ranks = np.array([1.0, 2.0, 4.0, 100.5, 5001.0])
    below = ranks - 1.0
    assert list(r) == ["auc_all", "mean_rank", "mrr", "recall@100", "recall@1000"]
    assert r["auc_all"] == pytest.approx(1.0 - float(np.mean(below / n.numpy())), rel=1e-12)
    assert r["mean_rank"] == pytest.approx(float(ranks.mean()), rel=1e-12)
    assert r["mrr"] == pytest.approx(float(np.mean(1.0 / ranks)), rel=1e-12)
    assert r["recall@100"] == pytest.approx(3 / 5)                      # 100.5 is not <= 100
    assert r["recall@1000"] == pytest.approx(4 / 5)
    assert list(global_ranking_metrics(greater, ties, n)) == ["auc_all", "mean_rank", "mrr", "recall@100", "recall@1000",
                                                              "recall@10000"]
    best = global_ranking_metrics([0, 0], [0, 0], [7, 7])
    worst = global_ranking_metrics([7, 7], [0, 0], [7, 7])
    tied = global_ranking_metrics([0], [7], [7])
    assert best["auc_all"] == 1.0 and worst["auc_all"] == 0.0 and tied["auc_all"] == 0.5
    assert global_ranking_metrics([0], [0], [0])["auc_all"] == 1.0      # the graph's only pair
    e = global_ranking_metrics(torch.zeros(0), torch.zeros(0), torch.zeros(0))
    assert all(math.isnan(v) for v in e.values()) and "recall@10000" in e
    with pytest.raises(ValueError):
        global_ranking_metrics(torch.zeros(2), torch.zeros(2), torch.zeros(3))


def test_form_and_workspace_are_host_only():
    from disenlink_amd import _lib
    lib = _lib.load()
    assert lib.dl_score_pair_ranks_supported(8, 64) == 1 and lib.dl_score_pair_ranks_supported(8, 130) == 0
    f = _lib.score_pair_ranks_form(5201, 8, 64, 1000)
    assert f["nd"] == 2 and f["tiles"] == 41 and f["pairs"] == 41 * 42 // 2
    assert f["grid"] == -(-f["pairs"] // f["pairs_per_wg"]) and f["pairs_per_wg"] >= 1
    assert f["separators"] == 1000 and f["targets_per_separator"] == 1 and f["lds_levels"] == 10 and f["global_levels"] == 0
    f = _lib.score_pair_ranks_form(41554, 8, 64, 100000)                # beyond the table: a second level in global memory
    assert f["targets_per_separator"] == 25 and f["separators"] == 4000 and f["lds_levels"] == 12 and f["global_levels"] == 5
    assert f["separators"] <= 4096 and (f["separators"] - 1) * f["targets_per_separator"] < 100000
    assert _lib.score_pair_ranks_form(300, 2, 32, 0)["separators"] == 0
    big = _lib.score_pair_ranks_form(2_900_000, 1, 8, 5)                # no cap at 46,340: the tile-pair count bounds N
    assert big["tiles"] == 22657 and big["pairs"] == 22657 * 22658 // 2
    assert int(lib.dl_score_pair_ranks_workspace_bytes(41554, 8, 64)) > int(lib.dl_score_pair_ranks_workspace_bytes(5201, 8, 64)) > 0
    assert int(lib.dl_score_pair_logits_workspace_bytes(5201, 8, 64)) > 0
    for bad in ((0, 8, 64), (8388481, 1, 8), (100, 8, 130), (100, 0, 64), (-5, 8, 64)):
        assert int(lib.dl_score_pair_ranks_workspace_bytes(*bad)) == 0 and int(lib.dl_score_pair_logits_workspace_bytes(*bad)) == 0
        with pytest.raises(_lib.DisenlinkHipError):
            _lib.score_pair_ranks_form(*bad, 10)
    assert _lib.score_pair_ranks_form(1, 2, 32, 3)["pairs"] == 0


def test_form_at_the_largest_accepted_n_and_the_refusal_beyond_it(lib_env, monkeypatch):
    """N = 8,388,480 = 65,535 tiles: 2,147,450,880 tile pairs, the most an int32 holds; the intermediates of the pair count
    and of the grid do not fit 32 bits there."""
    from disenlink_amd import _lib
    lib = _lib.load()
    top = 65535 * 128
    for N in (46341 * 128, top - 127, top):                             # 46,341 tiles: where nt (nt + 1) first passes 2^31
        nt = -(-N // 128)
        for tiles in (None, 1, 1 << 20):
            lib_env("DL_MINE_TILES", tiles)
            f = _lib.score_pair_ranks_form(N, 1, 8, 1000)
            assert f["tiles"] == nt and f["pairs"] == nt * (nt + 1) // 2 > 0
            assert f["pairs_per_wg"] >= 1 and f["grid"] >= 1
            assert f["grid"] * f["pairs_per_wg"] >= f["pairs"] > (f["grid"] - 1) * f["pairs_per_wg"]
            if tiles is not None:
                assert f["pairs_per_wg"] == tiles
    lib_env("DL_MINE_TILES")
    assert _lib.score_pair_ranks_form(top, 1, 8, 1000)["pairs"] == 2147450880
    assert int(lib.dl_score_pair_ranks_workspace_bytes(top, 1, 8)) > 0 and int(lib.dl_score_pair_logits_workspace_bytes(top, 1, 8)) > 0
    assert int(lib.dl_score_pair_ranks_workspace_bytes(top + 1, 1, 8)) == 0
    assert int(lib.dl_score_pair_logits_workspace_bytes(top + 1, 1, 8)) == 0
    with pytest.raises(_lib.DisenlinkHipError, match="8388480"):
        _lib.score_pair_ranks_form(top + 1, 1, 8, 1000)
    one = (lib.dl_score_pair_ranks(1, 1, top + 1, 1, 8, 1.0, None, None, None, 0, 1, 1, 1, None, 0, None),
           lib.dl_score_pair_logits(1, 1, top + 1, 1, 8, 1.0, 1, 1, 1, 1, None, 0, None))
    assert all(rc < 0 for rc in one) and b"8388480" in lib.dl_last_error()      # refused on the shape, before anything is read
    # ... and, in Python, a prepared exclusion set on another device than the tables: refused before any call is made
    from disenlink_amd import scans
    monkeypatch.setattr(scans, "_need_cuda", lambda *tensors: None)
    monkeypatch.setattr(scans, "_scan_call", lambda name, *args: pytest.fail(f"dl_score_{name} was called"))
    Z = torch.zeros(8, 1, 8)
    ex = scans.pair_exclusion((torch.tensor([0]), torch.tensor([1])), 8, "cpu")
    with pytest.raises(ValueError, match="exclusion set on meta, tables on cpu"):
        scans.score_pair_ranks(Z, Z, 1.0, [0, 2], [1, 3], exclude=ex._replace(rowptr=ex.rowptr.to("meta")))


def test_gpu_cases_reach_every_chunk_count_and_run_length(lib_env):
    from disenlink_amd import _lib
    forms = [_lib.score_pair_ranks_form(N, K, d, 200) for N, (K, d), _ in pair_rank_ref.GPU_CASES]
    assert {f["nd"] for f in forms} == {1, 2, 3, 4}
    assert {f["tiles"] for f in forms} == {1, 2, 3}
    assert all(N * (N - 1) // 2 <= 65536 for N, _, _ in pair_rank_ref.GPU_CASES)      # ops.score_mine can list every pair
    geo = pair_rank_ref.GEOMETRY
    seen = []
    for tiles in geo["tiles"]:
        lib_env("DL_MINE_TILES", tiles)
        f = _lib.score_pair_ranks_form(geo["N"], geo["K"], geo["d"], 5000)
        assert f["pairs"] == 21 and f["pairs_per_wg"] == tiles
        seen.append(f["grid"])
    assert seen == [21, 6, 1]                                           # one, a few and all tile pairs per workgroup
    lib_env("DL_MINE_TILES")
    assert _lib.score_pair_ranks_form(2000, 1, 8, 300)["grid"] > 100    # the clustering case: many workgroups
    for N in (2, 5, 127, 300):
        src, dst = targets_for(N, 1)
        assert (src != dst).all() and src.min() >= 0 and max(int(src.max()), int(dst.max())) < N
        assert (src > dst).any() or N == 2
        lo, hi = torch.minimum(src, dst), torch.maximum(src, dst)
        assert torch.unique(lo * N + hi).numel() < src.numel() or N == 2      # repeated targets
    s300, d300 = targets_for(300, 1)
    have = set(zip(torch.minimum(s300, d300).tolist(), torch.maximum(s300, d300).tolist()))
    assert {(0, 1), (0, 299), (126, 127), (127, 128), (128, 129), (298, 299)} <= have


def test_global_rank_eval_flag_parses_and_refuses_what_is_out_of_scope():
    from disenlink_amd.main import build_parser, main
    assert build_parser().parse_args([]).global_rank_eval is False
    assert build_parser().parse_args(["--global-rank-eval"]).global_rank_eval is True
    with pytest.raises(SystemExit, match="one GPU"):
        main(["--synthetic", "--gpus", "2", "--global-rank-eval"])
    with pytest.raises(SystemExit, match="one GPU"):
        main(["--synthetic", "--table-dtype", "bf16", "--global-rank-eval"])
