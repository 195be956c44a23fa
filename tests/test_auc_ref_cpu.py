"""The CPU forms of the tie-averaged AUC (metrics.AucPlan's sort + search path, metrics.auc_tie_avg, metrics.ShardedAucPlan
on gloo) against the brute-force pair count of tests/auc_ref.py, on the cases the GPU test gives the kernel; and the NaN
contract: a NaN among the scores makes every form of the AUC NaN, so that no host loop can take a diverged epoch for an
improvement."""
import glob
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import auc_ref
from conftest import GOLDEN_DIR


def test_the_brute_force_count_reproduces_the_sklearn_vectors():
    paths = sorted(glob.glob(os.path.join(GOLDEN_DIR, "auc_*.npz")))
    assert len(paths) == 3, paths
    for path in paths:
        g = np.load(path)
        y, sc = g["y"], g["score"].astype(np.float32)
        pos_idx, neg_idx = np.nonzero(y > 0.5)[0], np.nonzero(~(y > 0.5))[0]
        assert abs(auc_ref.auc(sc, pos_idx, neg_idx) - float(g["auc"])) <= 1e-12, path


def test_the_brute_force_count_on_cases_small_enough_to_count_by_hand():
    f = lambda *v: np.array(v, np.float32)
    # positives {3, 1}, negatives {2, 1, 0}: 3 beats all three (6), 1 beats 0 (2) and ties with 1 (1)
    assert auc_ref.u2(f(3, 2, 1, 1, 0), [0, 2], [1, 3, 4]) == 9
    assert auc_ref.u2(f(0.0, -0.0), [0], [1]) == 1 and auc_ref.u2(f(-0.0, 0.0), [0], [1]) == 1      # equal
    assert auc_ref.u2(f(1e-45, 0.0), [0], [1]) == 2 and auc_ref.u2(f(0.0, 1e-45), [0], [1]) == 0     # a denormal is not 0
    assert auc_ref.u2(f(np.inf, np.inf, -np.inf, 3e38), [0, 2], [1, 3]) == 1 + 2 + 0 + 0
    assert auc_ref.has_nan(f(0, np.nan, 1), [0], [1]) and not auc_ref.has_nan(f(0, np.nan, 1), [0], [2])
    sizes = auc_ref.ladder_sizes()
    assert len(sizes) == len(set(sizes)) == 60 and max(a * b for a, b in sizes) <= auc_ref.PAIR_LIMIT
    for a, b in ((1, 1), (1024, 1024), (1025, 3001), (3001, 2049), (2048, 2048)):
        assert (a, b) in sizes


@pytest.mark.parametrize("key", auc_ref.all_case_keys(), ids=lambda k: "-".join(str(v) for v in k[1:]))
def test_cpu_sort_form_and_rank_form_equal_the_brute_force_count(key):
    """AucPlan.auc on the CPU (negatives sorted, positives searched) and auc_tie_avg (ranks of the whole vector): the
    integer count 2U of the first is the reference's, exactly; both quotients are the reference's double — AucPlan's by
    the same correctly rounded division, the rank form within the rounding of its sums of half-integers (exact below
    2^53) and one division."""
    from disenlink_amd.metrics import AucPlan, auc_tie_avg
    c = auc_ref.case(*key)
    assert not auc_ref.has_nan(c.score, c.pos_idx, c.neg_idx)
    label, score = torch.from_numpy(c.label), torch.from_numpy(c.score)
    plan = AucPlan(label)
    assert (plan.n_pos, plan.n_neg) == (c.n_pos, c.n_neg)
    got = float(plan.auc(score))
    denom2 = 2.0 * c.n_pos * c.n_neg
    print(c.name, "u2", c.u2, "plan", got * denom2, "ref auc", c.auc)
    assert got == c.auc, (c.name, got, c.auc)
    assert round(got * denom2) == c.u2                                      # the integer count itself
    rank = float(auc_tie_avg(label, score))
    assert rank == c.auc, (c.name, rank, c.auc)
    if key[0] == "family" and key[1] in auc_ref.EXACT_AUC:
        assert c.auc == auc_ref.EXACT_AUC[key[1]]
    if key[0] == "family" and key[1] == "only_inf":
        assert np.isinf(c.score).all() and math.isfinite(got) and math.isfinite(rank)


@pytest.mark.parametrize("n_pos,n_neg", [(65, 1025), (1025, 65), (40, 40)])
def test_a_nan_score_makes_both_cpu_forms_nan(n_pos, n_neg):
    """One NaN positive, one NaN negative, all NaN, NaN in one class only (either class), with either class the smaller
    one: NaN from AucPlan.auc's sort path and from auc_tie_avg, as 0-dim float64 tensors.  (Before the contract the sort
    path gave exactly 1.0 for all-NaN scores: torch sorts NaN last and finds it above everything.)"""
    from disenlink_amd.metrics import AucPlan, auc_tie_avg
    for name, (score, pos_idx, neg_idx) in auc_ref.nan_inputs(n_pos, n_neg).items():
        assert auc_ref.has_nan(score, pos_idx, neg_idx)
        label = torch.from_numpy(auc_ref.labels(score.size, pos_idx))
        a = AucPlan(label).auc(torch.from_numpy(score))
        b = auc_tie_avg(label, torch.from_numpy(score), check=False)
        c = auc_tie_avg(label, torch.from_numpy(score))
        print(name, float(a), float(b), float(c))
        for v in (a, b, c):
            assert v.dtype == torch.float64 and v.dim() == 0 and math.isnan(float(v)), (name, float(v))
    # a NaN-free vector afterwards: nothing sticks
    c0 = auc_ref.case("ladder", 65, 1025)
    assert float(AucPlan(torch.from_numpy(c0.label)).auc(torch.from_numpy(c0.score))) == c0.auc


def test_sharded_auc_on_two_ranks_is_nan_everywhere_when_one_rank_holds_a_nan():
    """ShardedAucPlan, world = 2 on gloo: NaN-free input gives the reference's AUC on both ranks; a NaN among rank 1's
    scores only — a positive, or a negative — makes the all-reduced sum, hence the AUC, NaN on BOTH ranks; so does a NaN on
    a rank that holds negatives only (its share of the count is empty, its scores still speak)."""
    from test_dist_cpu import _auc_worker, _free_port
    c = auc_ref.case("ladder", 65, 1025)
    n = c.score.size
    label = c.label

    def run(label, score, cuts):
        out = mp.Manager().dict()
        mp.spawn(_auc_worker, args=(2, _free_port(), label, score, cuts, out), nprocs=2, join=True)
        return out[0], out[1]
    cuts = [0, n // 3, n]
    clean = run(label, c.score, cuts)
    assert clean[0] == clean[1] and abs(clean[0] - c.auc) <= 1e-15, (clean, c.auc)
    rank1 = np.arange(n // 3, n)
    for where in (rank1[label[rank1] > 0.5][0], rank1[label[rank1] < 0.5][-1]):
        score = c.score.copy()
        score[where] = np.nan
        got = run(label, score, cuts)
        assert math.isnan(got[0]) and math.isnan(got[1]), (int(where), got)
    order = np.argsort(-label, kind="stable")                              # positives first: rank 1 holds negatives only
    y, sc = label[order], c.score[order].copy()
    sc[-1] = np.nan
    got = run(y, sc, [0, n - 200, n])
    assert math.isnan(got[0]) and math.isnan(got[1]), got


class _ScriptedStop:
    """What early_stop.drive needs of a DeviceEarlyStop, answering from a script of (loss, auc)."""
    LAG, per = 1, 1

    def __init__(self, script):
        self.script, self.launches = script, 0

    def post(self, launch):
        self.launches += 1

    def read(self, epoch):
        return self.script[epoch]


def test_host_loops_take_a_nan_epoch_for_a_stale_one():
    """`nan > best` is false: early_stop.drive and the eager loop of train.run_link_prediction count a NaN validation AUC as
    an epoch without improvement — the best AUC and the kept weights are those of the last FINITE improvement, patience
    runs over the NaN epochs, and the history shows the NaN.  (The loops are unchanged; with an AUC of 1.0 for NaN scores
    they kept the diverged weights.)"""
    from disenlink_amd.early_stop import drive
    from disenlink_amd.train import RunResult
    nan = float("nan")
    script = [(1.0, 0.6), (0.9, 0.7), (nan, nan), (nan, nan), (0.8, 0.65), (0.7, 0.8), (nan, nan), (nan, nan), (nan, nan)]
    res = RunResult(nan, 0.0, 0)
    es = _ScriptedStop(script)
    assert drive(es, len(script), 3, lambda: None, res) == 0.8
    assert res.epochs_run == 9 and np.array_equal(np.isnan(res.val_aucs), [a != a for _l, a in script])
    res = RunResult(nan, 0.0, 0)
    assert drive(_ScriptedStop(script), 50, 1, lambda: None, res) == 0.7 and res.epochs_run == 4   # stops on the second NaN

    # the eager host loop on the CPU, the oracle standing in for the kernels: the validation scores turn NaN from epoch 3 on
    from disenlink_amd.data import synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    from test_train_cpu import OraclePairModule

    class DivergingValidation(OraclePairModule):
        calls = 0

        def forward_pairs(self, x, graph, pairs):
            emb, prob = super().forward_pairs(x, graph, pairs)
            if self.training:
                self.calls += 1
                if self.calls > 3:
                    prob = prob.clone()
                    prob[run.n_pos + run.n_neg:] = nan
            return emb, prob

    sg = synthetic_graph("chameleon", seed=2, scale=0.06)
    run = prepare_run(make_link_split(sg.src, sg.dst, sg.n_nodes, m=2, seed=0), "cpu")
    torch.manual_seed(0)
    model = DivergingValidation(Disentangle(16, 8, 8, nfactor=3, beta=0.7, t=1))
    x = torch.from_numpy(sg.features()[:, :16].copy())
    snap = model.state_dict
    res = run_link_prediction(model, x, run, epochs=25, lr=5e-3, patience=3)
    assert res.epochs_run == int(np.nanargmax(res.val_aucs[:3])) + 1 + 3 + 1 and res.epochs_run <= 7
    assert not np.isnan(res.val_aucs[:3]).any() and np.isnan(res.val_aucs[3:]).all()
    assert res.best_val_auc == max(res.val_aucs[:3]) and 0.0 < res.best_val_auc < 1.0
    assert math.isfinite(res.test_auc) and all(bool(torch.isfinite(v).all()) for v in snap().values())
