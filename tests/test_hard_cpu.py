"""Hard negatives without a device: the reference of tests/hard_ref.py against the plain sampler's (sample_ref), the near-tie
condition of tests/test_gpu_hard.py on the reference itself, and the refusals that need no GPU.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import hard_ref as hr
import sample_ref as sr
import test_gpu_sample as tgs                                   # its lists and tables (nothing of it touches a device here)

N = tgs.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _cand(m, c, exclude_self=False, seed=hr.SEED, epoch=hr.EPOCH):
    _n, rowptr, col, _rows = sr.exclusion_graph()
    return hr.candidates(tgs.sources(), m, N, rowptr, col, seed, epoch, c, exclude_self)


# ------------------------------------------------------------------------------------------------ 1. candidate 0 is the plain draw
@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("m", [1, 3, 5])
def test_one_candidate_is_the_plain_sampler(m, exclude_self):
    ref, ref_failed = tgs.ref_draw(m, hr.SEED, hr.EPOCH, exclude_self)
    cand = _cand(m, 1, exclude_self)
    k, which, failed = hr.select(cand, np.zeros(cand.shape))
    assert np.array_equal(cand[:, 0], ref) and np.array_equal(k, ref) and failed == ref_failed == 6 * m
    assert ((which == 0) == (ref >= 0)).all()


@pytest.mark.parametrize("m,c", hr.MC)
def test_candidate_zero_is_the_plain_draw(m, c):
    ref, ref_failed = tgs.ref_draw(m, hr.SEED, hr.EPOCH, False)
    cand = _cand(m, c)
    assert cand.shape == (300 * m, c) and np.array_equal(cand[:, 0], ref)
    u = np.repeat(tgs.sources(), m)
    assert (cand[u == 2] == -1).all()                              # node 2 excludes everything: every candidate dead
    assert (cand[u == 0] >= 0).all()                               # node 0 excludes nothing: the first attempt succeeds
    _n, _rowptr, _col, rows = sr.exclusion_graph()
    for e in np.flatnonzero(u != 2)[::7]:
        assert all(int(v) not in rows[u[e]] for v in cand[e] if v >= 0)
    # the candidates are separate draws (another counter each), and an entry fails only where ALL of them do
    live = cand >= 0
    assert c == 1 or (cand[:, 0] != cand[:, 1])[live[:, 0] & live[:, 1]].any()
    _k, _which, failed = hr.select(cand, np.zeros(cand.shape))
    assert failed == int((~live.any(axis=1)).sum()) <= ref_failed
    # a source outside the table: dead, whatever the exclusion set
    out = hr.candidates([0, N, -1], m, N, None, None, hr.SEED, hr.EPOCH, c)
    assert (out[:m] >= 0).all() and (out[m:] == -1).all()


def test_the_rule_on_hand_made_logits():
    cand = np.array([[4, 5, 6], [4, 5, 6], [-1, 5, 6], [4, -1, 6], [-1, -1, -1], [4, 5, 4], [4, 5, 6]], dtype=np.int32)
    nan, inf = float("nan"), float("inf")
    x = np.array([[1.0, 2.0, 2.0],        # a tie: the lowest index
                  [nan, -inf, nan],       # a NaN ranks below -inf
                  [9.0, nan, nan],        # every live logit NaN: the first live candidate (the dead one's value is not looked at)
                  [nan, 9.0, 0.5],        # a dead candidate between
                  [1.0, 1.0, 1.0],        # no live candidate
                  [3.0, 1.0, 3.0],        # a duplicated node: itself
                  [1.0, inf, 2.0]])       # +inf wins
    k, which, failed = hr.select(cand, x)
    assert k.tolist() == [5, 5, 5, 6, -1, 4, 5] and which.tolist() == [1, 1, 1, 2, -1, 0, 1] and failed == 1
    dec, node = hr.decisive(cand, x, 1e-6)
    assert node.tolist() == k.tolist()
    assert dec.tolist() == [False, True, False, True, False, True, True]


# ------------------------------------------------------------------------------------------------ 2. the near-tie condition
@pytest.mark.parametrize("m,c", hr.MC)
@pytest.mark.parametrize("K,d", hr.SHAPES)
def test_reference_is_decisive_on_the_gpu_inputs(K, d, m, c):
    """The GPU test requires at most 1 % non-decisive entries; here the reference shows that the inputs allow it."""
    Z, H = tgs.tables(K, d)
    cand = _cand(m, c)
    for t in hr.TEMPS:
        x64, tol, fig = hr.tolerance(Z, H, tgs.sources(), m, cand, t)
        share = hr.non_decisive_share(cand, x64, tol)
        print("FIGURE hard reference", f"K{K} d{d} t{t:g} m{m} c{c}", f"fp32 restatement {fig:.3g} tol {tol:.3g} non-decisive {share:.4f}")
        assert 0 < tol < 1e-4                                      # fp32 rounding of sums of K d products, nothing else
        assert share <= hr.MAX_NON_DECISIVE
        # the fp32 restatement itself keeps the fp64 node on every decisive entry
        dec, node = hr.decisive(cand, x64, tol)
        k32, _which, _failed = hr.select(cand, hr.logits(Z, H, tgs.sources(), m, cand, t, torch.float32).numpy())
        assert np.array_equal(k32[dec], node[dec])


# ------------------------------------------------------------------------------------------------ 3. refusals without a device
def test_argument_refusals():
    from disenlink_amd import ops
    from disenlink_amd.train import run_link_prediction
    Z = torch.zeros(N, 8, 64)
    src = torch.zeros(4, dtype=torch.int32)
    for c in (0, 65, -1):
        with pytest.raises(ValueError, match="candidates"):
            ops.sample_hard_negatives(Z, Z, 1.0, src, c, 3, N)
        with pytest.raises(ValueError, match="candidates"):
            ops.HardDraw(c, 0, 0)
    with pytest.raises(TypeError, match="fp32"):
        ops.sample_hard_negatives(Z.bfloat16(), Z.bfloat16(), 1.0, src, 4, 3, N)
    draw = ops.HardDraw(4, seed=3, epoch=0)
    assert draw.candidates == 4 and draw.k is None and draw.logit is None
    order, k_rowptr = torch.zeros(12, dtype=torch.int32), torch.zeros(N + 1, dtype=torch.int32)
    for fn in (ops.score_sampled_train, ops.score_sampled_bpr_train):
        with pytest.raises(ValueError, match="HardDraw"):
            fn(Z, Z, 1.0, None, draw, 1.0, order=order, k_rowptr=k_rowptr)
    with pytest.raises(ValueError, match="HardDraw"):
        ops.HotPathBprLoss.apply(Z, None, 0.6, 1.0, None, draw, 1.0, None, order, k_rowptr)
    from disenlink_amd.model import Disentangle
    model = Disentangle(24, 16, 64, nfactor=8, beta=0.6, t=1)
    x = torch.zeros(N, 24)
    with pytest.raises(ValueError, match="HardDraw"):
        model.forward_bpr_loss(x, None, None, draw, 1.0, None, order, k_rowptr)
    for step in (model.forward_pairs_resampled_loss, model.forward_pair_logits_resampled_loss):
        with pytest.raises(ValueError, match="HardDraw"):
            step(x, None, None, None, None, None, draw, 1.0, order, k_rowptr)
    # the loop: a value outside [0, 64], and an objective that does not resample — before anything is looked at
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="hard_negatives"):
            run_link_prediction(None, None, None, objective="bpr", hard_negatives=bad)
    for objective in ("pairs", "pairs-logit", "recon", "recon-logit"):
        with pytest.raises(ValueError, match="hard_negatives"):
            run_link_prediction(None, None, None, objective=objective, hard_negatives=4)
    with pytest.raises(ValueError, match="objective"):             # resampling itself still refuses the reconstruction loss
        run_link_prediction(None, torch.zeros(1), None, objective="recon", resample_negatives=True, hard_negatives=4)


# ------------------------------------------------------------------------------------------------ 4. the command line
@pytest.mark.parametrize("extra,match", [
    (["--hard-negatives", "65", "--objective", "bpr"], "0 .. 64"),
    (["--hard-negatives", "-1", "--objective", "bpr"], "0 .. 64"),
    (["--hard-negatives", "4"], "--resample-negatives"),
    (["--hard-negatives", "4", "--objective", "pairs-logit"], "--resample-negatives"),
    (["--hard-negatives", "4", "--objective", "recon"], "--resample-negatives"),
    (["--hard-negatives", "4", "--objective", "bpr", "--gpus", "2"], "one GPU"),
    (["--hard-negatives", "4", "--objective", "bpr", "--graph"], "one GPU"),
    (["--hard-negatives", "4", "--objective", "bpr", "--table-dtype", "bf16"], "one GPU"),
    (["--hard-negatives", "4", "--resample-negatives", "--gpus", "2"], "one GPU"),
    (["--hard-negatives", "4", "--resample-negatives", "--table-dtype", "bf16"], "one GPU"),
])
def test_cli_refusals(extra, match):
    from disenlink_amd import main
    with pytest.raises(SystemExit, match=match):                   # refused before anything is launched
        main.main(["--dataset", "squirrel", "--synthetic", *extra])


# ------------------------------------------------------------------------------------------------ 5. the C interface
def test_entries_in_header_and_exports():
    from disenlink_amd import _lib
    header = open(os.path.join(ROOT, "include", "disenlink_hip.h")).read()
    for name, n_args in (("dl_sample_negatives_hard", 20), ("dl_sample_negatives_hard_supported", 3)):
        assert name in _lib.EXPORTS and len(_lib.EXPORTS[name][1]) == n_args
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl is not None and decl.group(1).count(",") + 1 == n_args
    lib = _lib.load()
    assert lib.dl_sample_negatives_hard_supported(8, 64, _lib.DL_F32) == 1
    assert lib.dl_sample_negatives_hard_supported(3, 20, _lib.DL_F32) == 1
    assert lib.dl_sample_negatives_hard_supported(8, 64, _lib.DL_BF16) == 0
    assert lib.dl_sample_negatives_hard_supported(64, 64, _lib.DL_F32) == 0          # K d = 4096 > 2048
    assert lib.dl_sample_negatives_hard_supported(65, 1, _lib.DL_F32) == 0
