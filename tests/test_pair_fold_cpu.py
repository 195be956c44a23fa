"""The forward plan that folds mirrored pairs (graph.PairList.build(fold_mirrors=True): ``fwd``, ``fwd_pair``, ``fwd_pair2``),
the plan builder alone: every listed pair is scored exactly once, as the first or the second id of an entry; two ids share
an entry only where their endpoints are mirrors; the matching is one to one; ``by_u`` and the incidence plan are what they
are without folding."""
import numpy as np
import pytest
import torch

from test_host_cpu import _check_plan


def _lists():
    rng = np.random.default_rng(11)
    n = 160
    pu, pv = rng.integers(0, n, 900), rng.integers(0, n, 900)
    m = rng.choice(900, 250, replace=False)                         # mirrors of a quarter of the list, some of them twice
    pu, pv = np.concatenate([pu, pv[m], pv[m[:40]]]), np.concatenate([pv, pu[m], pu[m[:40]]])
    pu, pv = np.concatenate([pu, pu[:30], np.arange(20)]), np.concatenate([pv, pv[:30], np.arange(20)])   # repeats, self pairs
    perm = rng.permutation(pu.size)
    yield "random", n, pu[perm], pv[perm]
    # by hand: a mirror; a mirror whose reverse is listed twice; an ordered pair twice, its reverse once; self pairs, twice
    yield "hand", 8, np.array([1, 2, 3, 4, 4, 5, 5, 6, 7, 7, 0]), np.array([2, 1, 4, 3, 3, 6, 6, 5, 7, 7, 3])
    yield "no mirrors", 8, np.array([0, 0, 1, 5, 5]), np.array([1, 2, 2, 5, 5])


@pytest.mark.parametrize("case", list(_lists()), ids=lambda c: c[0])
def test_folded_forward_plan_lists_every_pair_once(case):
    from disenlink_amd.graph import PairList
    _, n, pu, pv = case
    P = pu.size
    tu, tv = torch.from_numpy(pu), torch.from_numpy(pv)
    kw = dict(seg_len=5, run_len=8, n_slices=4)
    pl, plain = PairList.build(tu, tv, n, **kw), PairList.build(tu, tv, n, fold_mirrors=False, **kw)
    assert plain.fwd is None and plain.fwd_pair is None and plain.fwd_pair2 is None
    # by_u and the incidence plan do not know about folding: byte for byte what they are without it
    for a, b in ((pl.by_u, plain.by_u), (pl.inc, plain.inc)):
        for name in ("rowptr", "col", "seg_row", "seg_beg", "seg_end", "seg_slot", "slice_seg0", "multi_row", "multi_slot0"):
            assert getattr(a, name).numpy().tobytes() == getattr(b, name).numpy().tobytes(), name
        assert (a.n_seg, a.seg_len, a.n_slices, a.slice_max_seg, a.n_slots) == (b.n_seg, b.seg_len, b.n_slices, b.slice_max_seg, b.n_slots)
    assert pl.by_u_pair.numpy().tobytes() == plain.by_u_pair.numpy().tobytes()
    assert pl.inc_pair.numpy().tobytes() == plain.inc_pair.numpy().tobytes()

    # the number of one-to-one mirror matches, counted independently: per unordered pair min(#(u,v), #(v,u))
    fwdc, revc = {}, {}
    for u, v in zip(pu.tolist(), pv.tolist()):
        if u < v:
            fwdc[(u, v)] = fwdc.get((u, v), 0) + 1
        elif u > v:
            revc[(v, u)] = revc.get((v, u), 0) + 1
    n_fold = sum(min(c, revc.get(k, 0)) for k, c in fwdc.items())
    if n_fold == 0:
        assert pl.fwd is None
        return
    q1, q2 = pl.fwd_pair.numpy().astype(np.int64), pl.fwd_pair2.numpy().astype(np.int64)
    assert pl.fwd.n_entries == q1.size == q2.size == P - n_fold and int((q2 >= 0).sum()) == n_fold
    # every pair id exactly once, as a first or a second id
    assert sorted(np.concatenate([q1, q2[q2 >= 0]]).tolist()) == list(range(P))
    # an entry sits in the row of its first id's u and names its v; its second id is the reverse, and never a self pair
    _check_plan(pl.fwd, pl.fwd.rowptr.numpy(), 8, unit_segs=1)
    row_of = np.repeat(np.arange(n), np.diff(pl.fwd.rowptr.numpy()))
    assert np.array_equal(pu[q1], row_of) and np.array_equal(pv[q1], pl.fwd.col.numpy())
    has = q2 >= 0
    assert np.array_equal(pu[q2[has]], pv[q1[has]]) and np.array_equal(pv[q2[has]], pu[q1[has]])
    assert np.all(pu[q1[has]] < pv[q1[has]])                       # kept in the row of min(u, v)
    assert pl.fwd.n_slices == pl.by_u.n_slices and pl.fwd.seg_len == pl.by_u.seg_len


def test_mirror_partners_by_hand():
    from disenlink_amd.graph import mirror_partners
    pu = torch.tensor([1, 2, 3, 4, 4, 5, 5, 6, 7, 7, 0])
    pv = torch.tensor([2, 1, 4, 3, 3, 6, 6, 5, 7, 7, 3])
    # (1,2)+(2,1); (3,4) with the FIRST of the two (4,3); the first of the two (5,6) with (6,5); self pairs and (0,3) alone
    assert mirror_partners(pu, pv, 8).tolist() == [1, -1, 3, -1, -1, 7, -1, -1, -1, -1, -1]
    assert mirror_partners(pu[:0], pv[:0], 8).numel() == 0
