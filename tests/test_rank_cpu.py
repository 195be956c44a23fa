"""Ranking metrics and the exclusion normaliser of the ranking ops, on the CPU (no GPU needed)."""
import math

import numpy as np
import pytest
import torch

from disenlink_amd.metrics import ranking_metrics


def test_ranking_metrics_hand_computed_with_ties():
    greater = torch.tensor([0, 0, 3, 9, 120])
    ties = torch.tensor([0, 2, 0, 1, 0])
    # ranks 1, 2, 4, 10.5, 121
    r = ranking_metrics(greater, ties, ks=(1, 10, 50, 100))
    ranks = np.array([1.0, 2.0, 4.0, 10.5, 121.0])
    assert r["mrr"] == pytest.approx(float(np.mean(1.0 / ranks)), rel=1e-12)
    assert r["hits@1"] == pytest.approx(1 / 5)
    assert r["hits@10"] == pytest.approx(3 / 5)          # 10.5 is not <= 10
    assert r["hits@50"] == pytest.approx(4 / 5)
    assert r["hits@100"] == pytest.approx(4 / 5)
    assert list(r) == ["mrr", "hits@1", "hits@10", "hits@50", "hits@100"]


def test_ranking_metrics_all_tied_and_empty():
    r = ranking_metrics(np.zeros(4, np.int64), np.full(4, 3, np.int64), ks=(1, 3))
    assert r["mrr"] == pytest.approx(1 / 2.5) and r["hits@1"] == 0.0 and r["hits@3"] == 1.0
    e = ranking_metrics(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    assert all(math.isnan(v) for v in e.values())
    with pytest.raises(ValueError):
        ranking_metrics(torch.zeros(2), torch.zeros(3))


def _edges(N, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, N, n), rng.integers(0, N, n)


def test_exclusion_csr_forms_agree():
    from disenlink_amd.graph import Graph
    from disenlink_amd.ops import exclusion_csr
    N = 23
    s, d = _edges(N, 60, 1)
    s = np.concatenate([s, s[:5]])                        # duplicates collapse
    d = np.concatenate([d, d[:5]])
    rows, cols = np.concatenate([s, d]), np.concatenate([d, s])
    mask = np.zeros((N, N), np.float32)
    mask[rows, cols] = 1
    g = Graph.from_edge_rows(torch.from_numpy(s), torch.from_numpy(d), N)
    ref_ptr = np.zeros(N + 1, np.int64)
    ref_ptr[1:] = np.cumsum(mask.sum(1))
    ref_col = np.nonzero(mask)[1]
    for form in (torch.from_numpy(mask), (torch.from_numpy(rows), torch.from_numpy(cols)), (rows.tolist(), cols.tolist()), g):
        ptr, col = exclusion_csr(form, N)
        assert ptr.dtype == torch.int32 and col.dtype == torch.int32 and ptr.device.type == "cpu"
        np.testing.assert_array_equal(ptr.numpy(), ref_ptr)
        np.testing.assert_array_equal(col.numpy(), ref_col)


def test_exclusion_csr_empty_and_errors():
    from disenlink_amd.ops import exclusion_csr
    assert exclusion_csr(None, 5) == (None, None)
    ptr, col = exclusion_csr((torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)), 5)
    assert ptr.tolist() == [0] * 6 and col.numel() == 0
    with pytest.raises(ValueError):
        exclusion_csr((torch.tensor([0, 5]), torch.tensor([1, 1])), 5)
    with pytest.raises(ValueError):
        exclusion_csr(torch.zeros(4, 5), 5)
    with pytest.raises(ValueError):
        exclusion_csr((torch.tensor([0]), torch.tensor([1, 2])), 5)


def test_rank_eval_flag_parses_and_refuses_several_gpus():
    from disenlink_amd.main import build_parser, main
    assert build_parser().parse_args([]).rank_eval is False
    assert build_parser().parse_args(["--rank-eval"]).rank_eval is True
    with pytest.raises(SystemExit, match="one GPU"):
        main(["--synthetic", "--gpus", "2", "--rank-eval"])
