"""The fp64 reference of the global top-m link mining on hand-made cases, the host-only plan and workspace size of
dl_score_mine, and what the GPU test's case list reaches (no GPU needed)."""
import math

import numpy as np
import pytest
import torch

import mine_ref
from mine_ref import mine64, select_top

INF, NAN = float("inf"), float("nan")


def _sym(rows):
    S = torch.tensor(rows, dtype=torch.float64)
    return torch.triu(S, 1) + torch.triu(S, 1).T


def test_select_ties_by_pair_index():
    S = torch.zeros(4, 4, dtype=torch.float64)
    S[0, 3] = S[1, 2] = 5.0
    S[0, 1] = 5.0
    S[2, 3] = 7.0
    u, v, s = select_top(S, 4)
    assert list(zip(u.tolist(), v.tolist())) == [(2, 3), (0, 1), (0, 3), (1, 2)] and s.tolist() == [7.0, 5.0, 5.0, 5.0]
    u, v, _ = select_top(S, 6)                                    # the zeros follow, in index order
    assert list(zip(u.tolist(), v.tolist()))[4:] == [(0, 2), (1, 3)]
    S[3, 2] = 100.0                                               # the lower triangle is never read
    assert select_top(S, 1)[2].tolist() == [7.0]


def test_select_signed_zeros_are_equal():
    S = torch.zeros(3, 3, dtype=torch.float64)
    S[0, 1], S[0, 2], S[1, 2] = 0.0, -0.0, 0.0
    u, v, s = select_top(S, 3)
    assert list(zip(u.tolist(), v.tolist())) == [(0, 1), (0, 2), (1, 2)]
    assert math.copysign(1.0, float(s[1])) == -1.0                # the value comes back as it was
    assert [len(select_top(S, 3, min_logit=f)[0]) for f in (0.0, -0.0, 1e-300)] == [3, 3, 0]


def test_select_inf_nan_and_floor():
    S = _sym([[0, INF, -INF, NAN], [0, 0, 2.0, INF], [0, 0, 0, -1.0], [0, 0, 0, 0]])
    u, v, s = select_top(S, 10)
    assert list(zip(u.tolist(), v.tolist())) == [(0, 1), (1, 3), (1, 2), (2, 3), (0, 2)]      # NaN never, -inf last
    assert s.tolist() == [INF, INF, 2.0, -1.0, -INF]
    assert select_top(S, 10, min_logit=-1e300)[2].tolist() == [INF, INF, 2.0, -1.0]
    assert select_top(S, 10, min_logit=-1.0)[2].tolist() == [INF, INF, 2.0, -1.0]
    assert select_top(S, 10, min_logit=INF)[2].tolist() == [INF, INF]
    assert len(select_top(S, 10, min_logit=NAN)[0]) == 0
    assert select_top(S, 1)[2].tolist() == [INF] and len(select_top(torch.zeros(1, 1), 3)[0]) == 0


def test_select_exclusion_and_m_beyond_eligible():
    S = _sym([[0, 3.0, 2.0], [0, 0, 1.0], [0, 0, 0]])
    ex = torch.zeros(3, 3, dtype=torch.bool)
    ex[0, 1] = True
    u, v, s = select_top(S, 100, ex)
    assert list(zip(u.tolist(), v.tolist())) == [(0, 2), (1, 2)] and s.tolist() == [2.0, 1.0]


def test_mine64_matches_a_plain_loop():
    g = torch.Generator().manual_seed(4)
    N, K, d, t = 9, 2, 5, 2.0
    Z, H = torch.randn(N, K, d, generator=g) * 0.5, torch.randn(N, K, d, generator=g)
    ex = torch.zeros(N, N, dtype=torch.bool)
    ex[7, 2] = ex[0, 1] = True                                    # (7, 2) is honoured as the pair {2, 7}
    ref = []
    for u in range(N):
        for v in range(u + 1, N):
            if (u, v) in ((2, 7), (0, 1)):
                continue
            s = sum(float(H[u, k].double() @ H[v, k].double()) * math.exp(float(Z[u, k].double() @ Z[v, k].double()) / t)
                    for k in range(K))
            if s >= -0.25:
                ref.append((-s, u * N + v, u, v))
    ref.sort()
    u, v, s = mine64(Z, H, t, ex, -0.25, 12)
    assert list(zip(u.tolist(), v.tolist())) == [(a, b) for _, _, a, b in ref[:12]]
    np.testing.assert_allclose(s.numpy(), [-r[0] for r in ref[:12]], rtol=1e-12)


def test_form_and_workspace_are_host_only_and_monotone_in_m():
    from disenlink_amd import _lib
    lib = _lib.load()
    prev = 0
    for m in (1, 2, 100, 4096, 65536):
        b = int(lib.dl_score_mine_workspace_bytes(5201, 8, 64, m))
        assert b >= prev and b >= 8 * m
        prev = b
    assert int(lib.dl_score_mine_workspace_bytes(5201, 8, 64, 65536)) > int(lib.dl_score_mine_workspace_bytes(5201, 8, 64, 1))
    assert int(lib.dl_score_mine_workspace_bytes(41554, 8, 64, 100)) > int(lib.dl_score_mine_workspace_bytes(5201, 8, 64, 100))
    for bad in ((5201, 8, 64, 0), (5201, 8, 64, 65537), (46341, 8, 64, 10), (-1, 8, 64, 10), (100, 8, 130, 10), (100, 0, 64, 10)):
        assert int(lib.dl_score_mine_workspace_bytes(*bad)) == 0
        with pytest.raises(_lib.DisenlinkHipError):
            _lib.score_mine_form(*bad)
    assert lib.dl_score_mine_supported(8, 64) == 1 and lib.dl_score_mine_supported(8, 130) == 0
    f = _lib.score_mine_form(5201, 8, 64, 100)
    assert f["nd"] == 2 and f["tiles"] == 41 and f["pairs"] == 41 * 42 // 2 and f["max_scans"] == 7
    assert f["grid"] == -(-f["pairs"] // f["pairs_per_wg"]) and f["pairs_per_wg"] >= 1
    assert _lib.score_mine_form(5201, 8, 64, 65536) == f          # the plan does not depend on m
    one = _lib.score_mine_form(1, 8, 64, 5)
    assert one["pairs"] == 0 and one["max_scans"] == 0
    assert _lib.score_mine_form(46340, 1, 1, 1)["tiles"] == 363


def test_form_follows_the_forced_run_length(lib_env):
    from disenlink_amd import _lib
    lib_env("DL_MINE_TILES", 5)
    f = _lib.score_mine_form(1000, 2, 32, 10)
    assert f["pairs"] == 36 and f["pairs_per_wg"] == 5 and f["grid"] == 8
    lib_env("DL_MINE_TILES", 1000)
    assert _lib.score_mine_form(1000, 2, 32, 10)["grid"] == 1
    lib_env("DL_MINE_TILES")
    assert _lib.score_mine_form(1000, 2, 32, 10)["pairs_per_wg"] == 1


def test_gpu_cases_reach_every_chunk_count_and_tile_layout():
    from disenlink_amd import _lib
    forms = [_lib.score_mine_form(N, K, d, 7) for N, (K, d), _ in mine_ref.GPU_CASES]
    assert {f["nd"] for f in forms} == {1, 2, 3, 4}               # every 32-column chunk count of 1 <= d <= 128
    assert {f["tiles"] for f in forms} == {1, 2, 3}               # one tile, a partial second tile, several tile pairs
    for N in mine_ref.GPU_N:
        ms = mine_ref.gpu_m_values(N)
        assert ms[0] == 1 and ms[-1] > N * (N - 1) // 2 and all(1 <= m <= 65536 for m in ms)


def test_mine_flags_parse_and_refuse_what_is_out_of_scope():
    from disenlink_amd.main import build_parser, main
    a = build_parser().parse_args([])
    assert a.mine == 0 and a.mine_out is None
    a = build_parser().parse_args(["--mine", "50", "--mine-out", "x.txt"])
    assert a.mine == 50 and a.mine_out == "x.txt"
    with pytest.raises(SystemExit, match="one GPU"):
        main(["--synthetic", "--gpus", "2", "--mine", "5"])
    with pytest.raises(SystemExit, match="one GPU"):
        main(["--synthetic", "--table-dtype", "bf16", "--mine", "5"])
    with pytest.raises(SystemExit, match="65536"):
        main(["--synthetic", "--mine", "70000"])
