"""The forward scorer over a MIXED hub plan (graph.HubPlan.build_mixed, dl_pair_hub_mixed; the MIXED forms of
hub::score_fwd_wave_kernel) against the same call on the plan without hub rows (hub_rows=0: the wave-per-entry kernel alone)
and on the three-list plan of the same list (DL_SCORE_HUB_MIXED=0): probabilities, logits and both arrays of stored terms
must be the same BITS — a slot runs the arithmetic of an entry whichever endpoint is its hub row and whatever else shares
its step.  Compared as int32, so that inf and NaN count too.

One list of N = 260 nodes and about 3.6 k pairs (d = 64, fp32), built block by block so that its plan, asserted before any
launch, holds: work items of 288, 264, 129 and 120 steps (waves of 36, 33, 17 / 16 and 15 steps), the 129 over all five
lists; with the item length cut to 8 gathered rows, items of 1 to 16 steps (waves of 0, 1 and 2 steps); over both plans every
shape as a full step (A211 stands alone in its list, so it always runs as a last step — full or short) and as a last step
with every number of dead slots its shape allows — A: 1, 2, 3; A211: 1 (dead third row); B: 2 (dead second row); B31: 1 (dead
second row) — and C steps with a dead fourth slot; a short last block and a residual plan; entries whose hub row is their
SECOND listed endpoint, with and without a mirrored pair.  K in {4, 8}, t in {1, 2}, mirrors folded and not, with stored terms
and without, the logit entry; tables: random, all zero, one factor duplicated, one row at 1e20.  Every call runs twice."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D = 260, 64
HUB_ROWS = 69                      # four blocks of 16 and a last block of 5
A, A211, B, B31, C = range(5)


def _pair_list():
    """Blocks of 16 hub rows (ids below 64), each a list of groups (c slots on one partner row) over its rows, least loaded
    row first; five rows of a short block, residual rows, then the partners (ids from 90): every hub row has more entries
    than any partner, so the owner rule makes exactly these rows the hub rows."""
    rng = np.random.default_rng(17)
    pu, pv = [], []

    def block(first_row, partners, n3, n2, n1, n_c, c_group):
        load = np.zeros(16, np.int64)
        groups = [3] * n3 + [2] * n2 + [1] * n1
        for at, extra in ((0, 4), (n3, 4), (n3 + n2, 12), (n3 + n2 + 1, 8)):       # some remainders share their row with C steps
            groups[at] += extra
            n_c -= extra // 4
        groups += [c_group] * (n_c // (c_group // 4))
        if n_c % (c_group // 4):
            groups.append(4 * (n_c % (c_group // 4)))
        assert len(groups) <= len(partners)
        for c, v in zip(groups, partners):
            rows = np.argsort(load, kind="stable")[:c]
            load[rows] += 1
            pu.extend((first_row + rows).tolist())
            pv.extend([v] * c)
        return load

    big, mid = list(range(90, 190)), list(range(190, 260))
    loads = [block(0, big, 6, 5, 15, 277, 16),         # 288 steps: A 2 (3 live), A211 1, B 2, B31 6, C 277
             block(16, big[::-1], 3, 3, 10, 257, 16),  # 264 steps: A 2 (1 live), A211 1, B 1, B31 3, C 257
             block(32, mid, 4, 3, 8, 122, 12),         # 129 steps: A 1 (2 live), A211 1, B 1, B31 4, C 122
             block(48, mid[::-1], 2, 1, 3, 117, 12)]   # 120 steps: A 0, A211 1 (dead third row), B 0, B31 2, C 117
    assert all(x.min() > y.max() for x, y in zip(loads, loads[1:])) and loads[-1].min() >= 29
    for u in range(64, 69):                            # the short last block
        v = rng.choice(np.arange(90, N), size=9, replace=False)
        pu.extend([u] * 9 + [u]); pv.extend(v.tolist() + [u])        # ... and a self pair
    for u in range(69, 90):                            # residual rows
        k = int(rng.integers(0, 5))
        pu.extend([u] * k); pv.extend(rng.choice(np.arange(90, N), size=k, replace=False).tolist())
    pu.append(75); pv.append(75)
    # the second block's rows trade ids with the last 16 partners: a mirrored pair is folded into the entry of its smaller
    # endpoint, so those rows are the SECOND endpoint of their folded entries
    relabel = np.arange(N)
    relabel[16:32], relabel[244:260] = np.arange(244, 260), np.arange(16, 32)
    pu, pv = relabel[np.array(pu)], relabel[np.array(pv)]
    flip = rng.random(pu.size) < 0.35                  # listed from the partner's side: the owner is the second endpoint
    pu, pv = np.where(flip, pv, pu), np.where(flip, pu, pv)
    both = rng.choice(pu.size, size=400, replace=False)               # mirrored pairs, of flipped entries and of others
    both = both[pu[both] != pv[both]]
    pu, pv = np.concatenate([pu, pv[both]]), np.concatenate([pv, pu[both]])
    perm = rng.permutation(pu.size)
    return pu[perm], pv[perm], int(flip.sum())


def _waves(n_steps):
    return {len(range(w, n_steps, 8)) for w in range(8)}


def _check_features(pl, cut):
    from disenlink_amd import graph
    h = pl.hub_mixed
    assert h is not None and h.mixed and h.n_rows == HUB_ROWS and h.n_blocks == 5 and h.n_slices == 1
    block_row = h.block_row.cpu().reshape(-1, 16)
    assert [sorted(r.tolist()) for r in block_row[:4]] == [list(range(lo, lo + 16)) for lo in (0, 244, 32, 48)]
    assert sorted(block_row[4].tolist()) == [-1] * 11 + list(range(64, 69))
    assert h.rest is not None and h.rest.n_entries > 20
    lens = (h.item_step[:, 1:] - h.item_step[:, :-1]).cpu()
    steps = dict(zip(h.item_block.cpu().tolist(), lens.sum(1).tolist()))
    assert [steps[b] for b in range(4)] == [288, 264, 129, 120], steps
    assert lens[h.item_block.cpu() == 2].reshape(-1).tolist() == [1, 1, 1, 4, 122]      # 129 steps over all five lists
    waves = set().union(*(_waves(n) for n in lens.sum(1).tolist()), *(_waves(n) for n in (cut.hub_mixed.item_step[:, 5] - cut.hub_mixed.item_step[:, 0]).tolist()))
    assert {0, 1, 2, 15, 16, 17, 33, 36} <= waves, waves
    # step forms over both plans: (list, ran as the list's last step, dead slots)
    forms, dead_rows = set(), set()
    for x in (h, cut.hub_mixed):
        x.check()
        live, rows = (x.step_q >= 0).cpu(), (x.step_v >= 0).cpu()
        for b in x.item_step.cpu().tolist():
            for l in range(5):
                for s in range(b[l], b[l + 1]):
                    is_last = l != C and s == b[l + 1] - 1
                    forms.add((l, is_last, 4 - int(live[s].sum())))
                    nv = graph.HUB_MIXED_SHAPES[l][3] + 1
                    if int(rows[s].sum()) < nv:
                        assert is_last                                # dead rows: only where the kernel looks for them
                        dead_rows.add((l, int(rows[s].sum())))
    want = {(A, False, 0), (A, True, 0), (A, True, 1), (A, True, 2), (A, True, 3), (A211, True, 0), (A211, True, 1),
            (B, False, 0), (B, True, 0), (B, True, 2), (B31, False, 0), (B31, True, 0), (B31, True, 1), (C, False, 0), (C, False, 1)}
    assert want <= forms, sorted(want - forms)
    assert {(A, 1), (A, 2), (A, 3), (A211, 2), (B, 1), (B31, 1)} <= dead_rows, dead_rows
    # hub rows that are the second listed endpoint of their pair, with and without a second (mirrored) pair id
    pu = pl.pu.cpu().long()
    st, sl = torch.nonzero(h.step_q.cpu() >= 0, as_tuple=True)
    item_of = torch.repeat_interleave(torch.arange(h.n_items), (h.item_step[:, 5] - h.item_step[:, 0]).cpu().long())     # items are stored in step order
    u = h.block_row.cpu()[h.item_block.cpu()[item_of[st]].long() * 16 + h.step_u.cpu()[st, sl].long()].long()
    second = u != pu[h.step_q.cpu()[st, sl].long()]
    two = h.step_q2.cpu()[st, sl] >= 0
    counts = int((second & two).sum()), int((second & ~two).sum()), int((~second & two).sum())
    assert counts[0] > 20 and counts[1] > 200 and counts[2] > 20, counts


_shared = {}


def _lists(fold):
    """(mixed plan, the same with short work items in four slices, no hub rows) — built once"""
    if fold not in _shared:
        from disenlink_amd import graph
        pu, pv, n_flip = _pair_list()
        assert 3000 <= pu.size <= 4200 and n_flip > 1000
        tu, tv = torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV)
        mixed = graph.PairList.build(tu, tv, N, n_slices=1, hub_rows=HUB_ROWS, fold_mirrors=fold)
        plain = graph.PairList.build(tu, tv, N, n_slices=1, hub_rows=0, fold_mirrors=fold)
        old = graph.HUB_MIXED_ITEM_ROWS
        try:
            graph.HUB_MIXED_ITEM_ROWS = 8
            cut = graph.PairList.build(tu, tv, N, n_slices=4, hub_rows=HUB_ROWS, fold_mirrors=fold)
        finally:
            graph.HUB_MIXED_ITEM_ROWS = old
        assert plain.hub is None and plain.hub_mixed is None and (mixed.fwd is not None) == fold
        assert cut.hub_mixed.n_items > 10 * mixed.hub_mixed.n_items
        if fold:
            _check_features(mixed, cut)
        else:
            mixed.hub_mixed.check(), cut.hub_mixed.check()
            assert mixed.hub_mixed.step_q2 is None
        assert bool(mixed.c_struct_by_u()._obj.hub_mixed) and bool(mixed.c_struct_by_u()._obj.hub)
        _shared[fold] = (mixed, cut, plain)
    return _shared[fold]


_tabs = {}


def _tables(K, kind):
    if (K, kind) not in _tabs:
        g = torch.Generator().manual_seed(31 * K + len(kind))
        Z, H = torch.randn(N, K, D, generator=g) * 0.35, torch.randn(N, K, D, generator=g) * 0.35
        if kind == "zero":
            Z, H = torch.zeros_like(Z), torch.zeros_like(H)
        elif kind == "duplicated factor":
            Z[:, 1], H[:, 1] = Z[:, 0], H[:, 0]
        elif kind == "row at 1e20":
            Z[3], H[100] = 1e20, 1e20                  # a hub row and a partner row: inf and NaN
        _tabs[(K, kind)] = (Z.to(DEV).contiguous(), H.to(DEV).contiguous())
    return _tabs[(K, kind)]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _score(pl, K, kind, t, what):
    """prob (what == 'prob'), (prob, coef_e, coef_q) ('coef') or logits ('logit') — run twice, the same bits"""
    from disenlink_amd import ops
    Z, H = _tables(K, kind)
    outs = []
    for _ in range(2):
        if what == "logit":
            out = (ops.score_pairs_logits_fwd(Z, H, pl.pu, pl.pv, t, pl),)
        elif what == "coef":
            p, c = ops.score_pairs_fwd(Z, H, pl.pu, pl.pv, t, pl, want_coef=True)
            out = (p, c[0], c[1])
        else:
            out = (ops.score_pairs_fwd(Z, H, pl.pu, pl.pv, t, pl),)
        torch.cuda.synchronize()
        outs.append([_bits(x).clone() for x in out])
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    return outs[0]


def _mixed_off(fn):
    from disenlink_amd import _lib
    os.environ["DL_SCORE_HUB_MIXED"] = "0"
    _lib.config_reload()
    try:
        return fn()
    finally:
        del os.environ["DL_SCORE_HUB_MIXED"]
        _lib.config_reload()


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("t", [1.0, 2.0])
@pytest.mark.parametrize("K", [4, 8])
def test_mixed_plan_gives_the_bits_of_the_plain_plan_and_of_the_three_lists(K, t, fold):
    mixed, cut, plain = _lists(fold)
    for kind in ("random", "zero", "duplicated factor", "row at 1e20"):
        for what in ("prob", "coef", "logit"):
            ref = _score(plain, K, kind, t, what)
            if kind == "random" and what == "prob":
                p = ref[0].view(torch.float32)
                assert bool(torch.isfinite(p).all()) and float(p.std()) > 0.05
            if kind == "row at 1e20" and what == "prob":
                assert not bool(torch.isfinite(ref[0].view(torch.float32)).all()) or bool((ref[0].view(torch.float32) == 1.0).any())
            three = _mixed_off(lambda: _score(mixed, K, kind, t, what))
            for name, got in (("three lists", three), ("mixed", _score(mixed, K, kind, t, what)), ("mixed, short items", _score(cut, K, kind, t, what))):
                for x, y in zip(got, ref):
                    assert torch.equal(x, y), f"{name}, {kind}, {what}: {int((x != y).sum())} of {y.numel()} words differ"


@pytest.mark.parametrize("want_coef", [False, True])
def test_writes_every_listed_id_and_nothing_else(want_coef):
    """Straight into the library with sentinel-filled buffers of P + 7 slots."""
    from disenlink_amd import _lib, ops
    mixed, cut, plain = _lists(True)
    K, P, SENTINEL = 8, mixed.n_pairs, -7.0
    Z, H = _tables(K, "random")
    lib = _lib.load()
    outs = []
    for pl in (mixed, cut, plain):
        prob = torch.full((P + 7,), SENTINEL, device=DEV)
        cf = torch.full((2, P, K), SENTINEL, device=DEV) if want_coef else None
        _lib.check(lib.dl_score_pairs_fwd(Z.data_ptr(), H.data_ptr(), N, K, D, _lib.DL_F32, 1.0, pl.pu.data_ptr(),
                                          pl.pv.data_ptr(), P, pl.c_struct_by_u(), prob.data_ptr(),
                                          cf.data_ptr() if cf is not None else None, ops._stream()), "dl_score_pairs_fwd")
        torch.cuda.synchronize()
        assert bool((prob[P:] == SENTINEL).all()) and bool((prob[:P] != SENTINEL).all())
        if cf is not None:
            assert bool((cf != SENTINEL).all())
        outs.append((prob, cf))
    for prob, cf in outs[:2]:
        assert torch.equal(prob, outs[2][0])
        if want_coef:
            assert torch.equal(cf, outs[2][1])


def test_the_library_refuses_a_plan_of_another_layout():
    from disenlink_amd import _lib, ops
    mixed, _, _ = _lists(True)
    K = 8
    Z, H = _tables(K, "random")
    s = mixed.c_struct_by_u()._obj
    m = s.hub_mixed.contents
    prob = torch.empty(mixed.n_pairs, device=DEV)
    m.n_lists = 3
    try:
        rc = _lib.load().dl_score_pairs_fwd(Z.data_ptr(), H.data_ptr(), N, K, D, _lib.DL_F32, 1.0, mixed.pu.data_ptr(),
                                            mixed.pv.data_ptr(), mixed.n_pairs, mixed.c_struct_by_u(), prob.data_ptr(), None, ops._stream())
    finally:
        m.n_lists = 5
    assert rc == -1 and b"n_lists" in _lib.load().dl_last_error()
