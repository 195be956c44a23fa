"""dl_auc_pair_counts / dl_auc_pair_counts_add (auc_slice_search_kernel: slices of 1,024 scores of the smaller class sorted
by a workgroup each, chunks of the other class located in them by binary searches) against the brute-force pair count of
tests/auc_ref.py — the SAME INTEGER — on a ladder of class sizes around the slice length, on every chunk geometry
DL_AUC_TARGET can give, and on score families made of the values a sort network or a search can get wrong (ties, signed
zeros, denormals, infinities beside the kernel's own +inf padding); and the NaN contract: a NaN among the listed scores
sets DL_AUC_NAN_MARK in the count and makes AucPlan.auc NaN, through the ctypes path and the compiled binding alike."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import auc_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GARBAGE = 0x5A5A5A5A5A5A5A5A                                            # what u2 holds before an overwriting call
NAN_MARK = -(1 << 63)                                                  # DL_AUC_NAN_MARK read as int64


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from disenlink_amd import _lib
    _lib.load()


def _dev(c):
    return (torch.from_numpy(np.array(c.score)).to(DEV), torch.from_numpy(np.array(c.pos_idx)).to(DEV),
            torch.from_numpy(np.array(c.neg_idx)).to(DEV))


def _counts(score, pos_idx, neg_idx, u2=None, add=False) -> int:
    """One call of dl_auc_pair_counts (u2 pre-filled with garbage: the call overwrites) or of dl_auc_pair_counts_add."""
    from disenlink_amd import _lib
    lib = _lib.load()
    assert score.dtype == torch.float32 and score.is_contiguous() and pos_idx.dtype == neg_idx.dtype == torch.int64
    if u2 is None:
        u2 = torch.full((1,), GARBAGE, dtype=torch.int64, device=DEV)
    fn = lib.dl_auc_pair_counts_add if add else lib.dl_auc_pair_counts
    _lib.check(fn(score.data_ptr(), pos_idx.data_ptr(), pos_idx.numel(), neg_idx.data_ptr(), neg_idx.numel(), u2.data_ptr(),
                  torch.cuda.current_stream().cuda_stream), "dl_auc_pair_counts")
    return int(u2.item())


def _plan(score_len, pos_idx, neg_idx):
    """An AucPlan over the given index lists IN THE GIVEN (shuffled) ORDER: built from the label vector, then handed the
    lists as they are — the same two sets, so the same count, gathered in a scattered order."""
    from disenlink_amd.metrics import AucPlan
    label = torch.zeros(score_len, device=DEV)
    label[pos_idx] = 1.0
    plan = AucPlan(label)
    assert torch.equal(plan.pos_idx, pos_idx.sort().values) and torch.equal(plan.neg_idx, neg_idx.sort().values)
    plan.pos_idx, plan.neg_idx = pos_idx, neg_idx
    return plan


def _grid_of_the_library(n_pos, n_neg):
    from disenlink_amd import _lib
    g = (C.c_int * 4)()
    _lib.check(_lib.load().dl_auc_pair_counts_grid(n_pos, n_neg, g), "dl_auc_pair_counts_grid")
    return list(g)


def _grid_restated(n_pos, n_neg, target=0):
    """[positives sliced, slices, chunks, scores per chunk] — the host arithmetic of auc_pair_counts, written out again."""
    small_is_pos = n_pos <= n_neg
    n_small, n_large = (n_pos, n_neg) if small_is_pos else (n_neg, n_pos)
    slices = -(-n_small // 1024)
    target = target if target > 0 else 1024
    chunks = min(max(1, min(-(-n_large // 1024), -(-target // slices))), 65535)
    per = -(-n_large // chunks)
    return [int(small_is_pos), slices, -(-n_large // per), per]


@pytest.fixture(params=["1", "0"], ids=["compiled-binding", "ctypes"])
def auc_path(request, monkeypatch):
    """AucPlan.auc through native.auc_pair_counts (dl_torch.cpp) or through the ctypes call of the same entry."""
    from disenlink_amd import native
    monkeypatch.setenv("DL_NATIVE_OPS", request.param)
    native._state["loaded"] = None                                     # re-read DL_NATIVE_OPS
    assert native.available() == (request.param == "1")                # a missing binding is an error, not a ctypes run
    yield request.param
    monkeypatch.undo()
    native._state["loaded"] = None


@pytest.mark.parametrize("n_pos,n_neg", auc_ref.ladder_sizes())
def test_counts_on_the_class_size_ladder_are_the_brute_force_integer(n_pos, n_neg):
    """n_small in {1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049} x n_large in {n_small, 1023, 1024, 1025, 3001}, either
    class the smaller one, index lists interleaved and shuffled: one slice, a full slice, a slice of one score, two and
    three slices, a searched class that ends on a chunk boundary and one past it."""
    c = auc_ref.case("ladder", n_pos, n_neg)
    score, pos_idx, neg_idx = _dev(c)
    got = _counts(score, pos_idx, neg_idx)
    print(c.name, "kernel", got, "reference", c.u2)
    assert got == c.u2
    auc = _plan(score.numel(), pos_idx, neg_idx).auc(score)
    assert auc.is_cuda and auc.dtype == torch.float64 and float(auc) == c.auc
    grid = _grid_of_the_library(n_pos, n_neg)
    assert grid == _grid_restated(n_pos, n_neg), (grid, _grid_restated(n_pos, n_neg))
    assert grid[0] == int(n_pos <= n_neg)                               # equal sizes: the positives are the sorted class
    assert grid[1] == -(-min(n_pos, n_neg) // 1024) and grid[2] * grid[3] >= max(n_pos, n_neg) > (grid[2] - 1) * grid[3]


@pytest.mark.parametrize("n_pos,n_neg", [(2049, 3001), (3001, 2049), (1025, 3001), (3001, 1025)])
def test_every_chunk_geometry_gives_the_same_integer(n_pos, n_neg, lib_env):
    """DL_AUC_TARGET = 1 (one chunk per slice), 3 (with the two slices of 1,025 scores: two chunks of 1,501 scores — ragged,
    no multiple of 1,024; with the three slices of 2,049 scores still one chunk, where 5 gives the two ragged chunks),
    100000 (capped by ceil(n_large / 1024) = 3 chunks of 1,001, the default's grid): the grids differ — the library's own
    arithmetic, compared with its restatement here — and the count does not."""
    c = auc_ref.case("ladder", n_pos, n_neg)
    score, pos_idx, neg_idx = _dev(c)
    default = _counts(score, pos_idx, neg_idx)
    assert default == c.u2
    grids = {}
    try:
        for target in (1, 3, 5, 100000):
            lib_env("DL_AUC_TARGET", target)
            grids[target] = _grid_of_the_library(n_pos, n_neg)
            assert grids[target] == _grid_restated(n_pos, n_neg, target), (target, grids[target])
            got = _counts(score, pos_idx, neg_idx)
            print(c.name, "target", target, "grid", grids[target], "kernel", got, "reference", c.u2)
            assert got == default == c.u2, (target, grids[target])
    finally:
        lib_env("DL_AUC_TARGET")
    slices = -(-min(n_pos, n_neg) // 1024)
    assert grids[1][1:] == [slices, 1, 3001] and grids[100000][1:] == [slices, 3, 1001]
    assert (grids[3][1:], grids[5][1:]) == (([2, 2, 1501], [2, 3, 1001]) if slices == 2 else ([3, 1, 3001], [3, 2, 1501]))
    assert _grid_of_the_library(n_pos, n_neg) == grids[100000]          # the default aims at 1,024 workgroups: capped too


@pytest.mark.parametrize("n_pos,n_neg", auc_ref.family_sizes())
@pytest.mark.parametrize("family", sorted(auc_ref.FAMILIES))
def test_counts_on_score_families_are_the_brute_force_integer(family, n_pos, n_neg):
    """Three levels (heavy ties), all equal (exactly 0.5), logits up to +-3e38, -0.0 with +0.0 (equal), denormals with 0 and
    the smallest normal (all distinct: no flush to zero in one half of the kernel and not in the other), real +inf in the
    sliced class beside the +inf padding, -inf in both classes, nothing but +-inf, and separated classes (exactly 1 and
    exactly 0) — at (65, 1025) and (1025, 2049), either class the smaller one."""
    c = auc_ref.case("family", family, n_pos, n_neg)
    score, pos_idx, neg_idx = _dev(c)
    assert torch.equal(score.cpu().view(torch.int32), torch.from_numpy(np.array(c.score)).view(torch.int32))   # bits arrive
    got = _counts(score, pos_idx, neg_idx)
    print(c.name, "kernel", got, "reference", c.u2)
    assert got == c.u2
    auc = float(_plan(score.numel(), pos_idx, neg_idx).auc(score))
    assert auc == c.auc
    if family in auc_ref.EXACT_AUC:
        assert auc == auc_ref.EXACT_AUC[family]
    if family == "only_inf":
        assert math.isfinite(auc) and bool(torch.isinf(score).all())


@pytest.mark.parametrize("n_pos,n_neg", [(1025, 2049), (2049, 1025)])
def test_the_overwriting_and_the_adding_entry_and_an_unaligned_score_view(n_pos, n_neg):
    c = auc_ref.case("ladder", n_pos, n_neg)
    score, pos_idx, neg_idx = _dev(c)
    assert _counts(score, pos_idx, neg_idx) == c.u2                     # over 0x5A5A...: overwritten
    u2 = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert _counts(score, pos_idx, neg_idx, u2, add=True) == c.u2
    assert _counts(score, pos_idx, neg_idx, u2, add=True) == 2 * c.u2   # added, not overwritten
    assert _counts(score, pos_idx, neg_idx, u2) == c.u2                 # ... and overwritten again
    for lead in (1, 2, 3):                                              # a view that starts 4, 8, 12 bytes past an aligned address
        view = torch.cat([torch.full((lead,), float("nan"), device=DEV), score])[lead:]
        assert view.data_ptr() % 16 == 4 * lead and view.is_contiguous()
        assert _counts(view, pos_idx, neg_idx) == c.u2
    # scores that no list names are never looked at: NaN in them changes nothing
    wide = torch.cat([score, torch.full((77,), float("nan"), device=DEV)])
    assert _counts(wide, pos_idx, neg_idx) == c.u2
    # an empty class: the count is 0 (over garbage), no launch
    none = pos_idx[:0]
    assert _counts(score, none, neg_idx) == 0 and _counts(score, pos_idx, none) == 0


@pytest.mark.parametrize("n_pos,n_neg", [(65, 1025), (1025, 65), (1025, 2049), (2049, 1025), (1024, 1024)])
def test_a_nan_score_gives_a_nan_auc_on_both_call_paths(n_pos, n_neg, auc_path):
    """One NaN positive, one NaN negative, all NaN, every positive NaN, every negative NaN: AucPlan.auc is NaN — a 0-dim
    float64 tensor on the device, selected there — whichever class is sliced.  (Without the mark the kernel's fminf /
    fmaxf network dropped the NaNs and its searches found a NaN below everything: all-NaN scores gave exactly 1.0 with
    n_pos <= n_neg and exactly 0.0 otherwise.)  A NaN-free vector through the same plan afterwards: the exact AUC."""
    clean = None
    for name, (score, pos_idx, neg_idx) in auc_ref.nan_inputs(n_pos, n_neg).items():
        s, p, n = (torch.from_numpy(a).to(DEV) for a in (score, pos_idx, neg_idx))
        plan = _plan(s.numel(), p, n)
        auc = plan.auc(s)
        print(name, n_pos, n_neg, auc_path, float(auc))
        assert auc.is_cuda and auc.dtype == torch.float64 and auc.dim() == 0 and math.isnan(float(auc)), (name, float(auc))
        if clean is None:
            c = auc_ref.Case("clean", auc_ref.ladder_scores(n_pos + n_neg, 99), pos_idx.copy(), neg_idx.copy())
            clean = (torch.from_numpy(np.array(c.score)).to(DEV), c.auc)
        assert float(plan.auc(clean[0])) == clean[1]                    # nothing sticks


def test_a_nan_anywhere_in_the_grid_marks_the_count():
    """The raw count carries DL_AUC_NAN_MARK (bit 63: negative as int64) wherever the NaN is loaded: in the last, ragged
    slice (one real score beside 1,023 slots of padding), in slot cnt - 1 of a slice (next to the padding), in the second
    chunk of the searched class only, and the adding entry keeps the mark over a count that is already there.  A NaN-free
    call on the same buffers afterwards gives the exact count again."""
    for n_pos, n_neg in ((2049, 3001), (3001, 2049), (1500, 3001), (3001, 1500)):
        c = auc_ref.case("ladder", n_pos, n_neg) if (n_pos, n_neg) in auc_ref.ladder_sizes() else auc_ref.ladder_case(n_pos, n_neg)
        score, pos_idx, neg_idx = _dev(c)
        small, large = (c.pos_idx, c.neg_idx) if n_pos <= n_neg else (c.neg_idx, c.pos_idx)
        grid = _grid_of_the_library(n_pos, n_neg)
        assert grid[2] == 3 and grid[3] == 1001                          # three chunks of the searched class
        places = {"last slot of the sliced class (the padding follows)": small[len(small) - 1],
                  "last slot of a full slice": small[1023],
                  "second chunk of the searched class": large[grid[3] + 7],
                  "first searched score": large[0], "last searched score": large[len(large) - 1]}
        for what, at in places.items():
            bad = score.clone()
            bad[int(at)] = float("nan")
            got = _counts(bad, pos_idx, neg_idx)
            print(c.name, what, hex(got & (2 ** 64 - 1)))
            assert got < 0 and got & NAN_MARK == NAN_MARK, (what, got)
            u2 = torch.full((1,), 12345, dtype=torch.int64, device=DEV)
            assert _counts(bad, pos_idx, neg_idx, u2, add=True) < 0, what
            assert _counts(bad, pos_idx, neg_idx, u2, add=True) < 0, what   # OR, not ADD: a second NaN call keeps the mark
            assert _counts(score, pos_idx, neg_idx) == c.u2, what          # NaN-free again: the exact count
