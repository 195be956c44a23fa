"""The forward scorer on a plan that folds mirrored pairs (graph.PairList.build(fold_mirrors=True); dl_pair_incidence.inc_pair2):
one entry scores (u, v) and its listed reverse (v, u), and a segment's last step gathers no rows for entries past its end.

N = 96, d = 64, K in {4, 8}, t in {1, 2}, fp32 — the wave-per-entry kernel — on ONE pair list that holds mirrored pairs, a
mirror whose reverse is listed twice, an ordered pair listed twice, self pairs, rows whose segments are 1, 2, 3, 4, 5 and 64
entries long, and one saturated row (Z[3] scaled as test_gpu_parity._one_pass_case scales it).  Asserted: the folded
plan's probabilities and stored terms are the unfolded plan's and the training scorer's bit for bit; they lie within the
band tests/test_gpu_hotpath_fp64.py allows the scorer around an fp64 restatement written here; and a call into sentinel-filled
buffers with P + 7 slots writes every listed id and nothing else.  One bf16 case at (16, 128) — the group-per-entry
kernel, which carries the same second store — agrees with the unfolded plan bit for bit as well.
"""
import numpy as np
import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D = 96, 64
SENTINEL = -7.0


def _pair_list():
    rng = np.random.default_rng(5)
    pu, pv = [], []

    def add(u, v):
        pu.extend(np.atleast_1d(u).tolist())
        pv.extend(np.atleast_1d(v).tolist())

    hub_v = rng.integers(24, N, 150)
    add(np.full(150, 10), hub_v)                                   # segments of 64, 64 and the rest
    add(hub_v[:12], np.full(12, 10))                               # ... a dozen of them mirrored
    add(np.full(40, 3), rng.integers(24, N, 40))                   # the saturated row
    for k, u in enumerate((11, 12, 13, 14, 15)):                   # rows of 1 .. 5 entries, no mirrors among them
        add(np.full(k + 1, u), 40 + 7 * k + np.arange(k + 1))
    add([16, 17], [17, 16])                                        # a mirror
    add([18, 19, 19], [19, 18, 18])                                # a mirror whose reverse is listed twice
    add([20, 20], [21, 21])                                        # an ordered pair listed twice
    add([22, 22, 10, 23], [22, 22, 10, 23])                        # self pairs (one of them twice, one in the hub row)
    bu, bv = rng.integers(24, N, 300), rng.integers(24, N, 300)    # the bulk; mirrors of a fifth of it
    add(bu, bv)
    add(bv[:60], bu[:60])
    perm = rng.permutation(len(pu))
    return np.array(pu)[perm], np.array(pv)[perm]


def _seg_lengths(plan):
    live = plan.seg_row.cpu() >= 0
    return set((plan.seg_end.cpu() - plan.seg_beg.cpu())[live].tolist())


_shared = {}


def _lists():
    """The pair list, with and without folding (built once)."""
    if not _shared:
        from disenlink_amd.graph import PairList
        pu, pv = _pair_list()
        tu, tv = torch.from_numpy(pu).to(DEV), torch.from_numpy(pv).to(DEV)
        folded, plain = PairList.build(tu, tv, N), PairList.build(tu, tv, N, fold_mirrors=False)
        assert plain.fwd is None and folded.fwd is not None
        q2 = folded.fwd_pair2.cpu().long()
        n_fold = int((q2 >= 0).sum())
        assert n_fold >= 60 and folded.fwd.n_entries == pu.size - n_fold
        for plan in (folded.fwd, plain.by_u):                      # the segment lengths the kernel branches on are all there
            assert {1, 2, 3, 4, 5, 64} <= _seg_lengths(plan), _seg_lengths(plan)
        _shared["v"] = (pu, pv, folded, plain)
    return _shared["v"]


def _tables(K, t, dtype=torch.float32, d=D):
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph
    rng = np.random.default_rng(100 + K)
    G = Graph.from_edge_rows(torch.from_numpy(rng.integers(0, N, 700)), torch.from_numpy(rng.integers(0, N, 700)), N).to(DEV)
    Z = torch.randn(N, K, d, generator=torch.Generator().manual_seed(31 + K)) * 0.35 * (32 / d) ** 0.5
    Z[3] *= 6.0                                                    # saturated scores
    Z = Z.to(dtype).to(DEV)
    H = ops.aggregate_fwd(G, Z, 0.6, *ops.route_fwd(G, Z, t))
    return Z, H


def _logit64(Z, H, pu, pv, t):
    """model.py:109-113 in fp64: sum_k (h_u^k . h_v^k) exp(z_u^k . z_v^k / t)."""
    Z, H = Z.double().cpu(), H.double().cpu()
    pu, pv = torch.from_numpy(pu), torch.from_numpy(pv)
    return ((H[pu] * H[pv]).sum(-1) * torch.exp((Z[pu] * Z[pv]).sum(-1) / t)).sum(-1)


@pytest.mark.parametrize("t", [1.0, 2.0])
@pytest.mark.parametrize("K", [4, 8])
def test_folded_forward_plan_gives_the_unfolded_bits(K, t):
    from disenlink_amd import _lib, ops
    pu, pv, folded, plain = _lists()
    P = pu.size
    Z, H = _tables(K, t)
    prob = ops.score_pairs_fwd(Z, H, folded.pu, folded.pv, t, folded)
    prob_c, coef = ops.score_pairs_fwd(Z, H, folded.pu, folded.pv, t, folded, want_coef=True)
    prob_u, coef_u = ops.score_pairs_fwd(Z, H, plain.pu, plain.pv, t, plain, want_coef=True)
    label = torch.from_numpy((np.random.default_rng(1).random(P) < 0.3).astype(np.float32)).to(DEV)
    prob_t = ops.score_pairs_train(Z, H, folded, t, label, torch.ones(P, device=DEV))[0]
    x64 = _logit64(Z, H, pu, pv, t)
    band = ref64.prob_band(x64, ref64.BOUND["logit"] * ref64.U * ref64.logit_abs64(Z.double().cpu(), H.double().cpu(),
                                                                                   torch.from_numpy(pu), torch.from_numpy(pv), t),
                           ref64.BOUND["prob_eps"] * ref64.U)
    ratio = float(((prob.double().cpu() - torch.sigmoid(x64)).abs() / band).max())
    print(f"FIGURE K={K} t={t}: prob / band {ratio:.3f}; prob == 1 at {int((prob == 1.0).sum())} pairs; "
          f"max |logit| {float(x64.abs().max()):.1f}")
    assert prob.numel() == P and coef.shape == (2, P, K)
    assert torch.equal(prob, prob_u)
    assert torch.equal(prob, prob_t)
    assert torch.equal(prob_c, prob)
    assert torch.equal(coef.view(torch.int32), coef_u.view(torch.int32))
    assert ratio <= 1.0
    assert bool(torch.isfinite(x64).all()) and int((prob == 1.0).sum()) >= 1          # the saturated row is there

    # into sentinel-filled buffers with P + 7 slots: every listed id written, nothing else
    lib = _lib.load()
    for pl in (folded, plain):
        out = torch.full((P + 7,), SENTINEL, device=DEV)
        terms = torch.full((2 * P * K + 7,), SENTINEL, device=DEV)
        for cf in (None, terms):
            out.fill_(SENTINEL)
            _lib.check(lib.dl_score_pairs_fwd(Z.data_ptr(), H.data_ptr(), N, K, D, _lib.DL_F32, float(t), pl.pu.data_ptr(),
                                              pl.pv.data_ptr(), P, pl.c_struct_by_u(), out.data_ptr(),
                                              cf.data_ptr() if cf is not None else None, ops._stream()), "dl_score_pairs_fwd")
            assert torch.equal(out[:P], prob) and bool((out[P:] == SENTINEL).all())
        assert torch.equal(terms[:2 * P * K].view(2, P, K).view(torch.int32), coef.view(torch.int32))
        assert bool((terms[2 * P * K:] == SENTINEL).all())


def test_group_per_entry_kernel_stores_the_mirror_too():
    """bf16 tables at (16, 128): score_fwd_seg_kernel on the folded plan against the unfolded one."""
    from disenlink_amd import ops
    pu, pv, folded, plain = _lists()
    K, d, t = 16, 128, 2.0
    Z, H = _tables(K, t, torch.bfloat16, d)
    prob, coef = ops.score_pairs_fwd(Z, H, folded.pu, folded.pv, t, folded, want_coef=True)
    prob_u, coef_u = ops.score_pairs_fwd(Z, H, plain.pu, plain.pv, t, plain, want_coef=True)
    assert coef is not None and coef_u is not None
    assert torch.equal(prob, prob_u) and torch.equal(coef.view(torch.int32), coef_u.view(torch.int32))
    assert torch.equal(ops.score_pairs_fwd(Z, H, folded.pu, folded.pv, t, folded), prob)
    x64 = _logit64(Z, H, pu, pv, t)
    band = ref64.prob_band(x64, ref64.BOUND["logit"] * ref64.U * ref64.logit_abs64(Z.double().cpu(), H.double().cpu(),
                                                                                   torch.from_numpy(pu), torch.from_numpy(pv), t),
                           ref64.BOUND["prob_eps"] * ref64.U)
    ratio = float(((prob.double().cpu() - torch.sigmoid(x64)).abs() / band).max())
    print(f"FIGURE bf16 K={K} d={d}: prob / band {ratio:.3f}")
    assert ratio <= 1.0
