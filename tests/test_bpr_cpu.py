"""The pairwise ranking objective without a GPU: the fp64 reference's hand-written coefficients against torch autograd of the
written-out loss, and the fixed lists of ``SampledNegatives(dst=...)`` (torch on the CPU: no kernel is involved)."""
import numpy as np
import torch

import bpr_ref
import ref64


def _case(seed=0, N=23, K=3, d=5, n_rows=40, m=4):
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    Z = (0.4 * torch.randn(N, K, d, generator=g)).double()
    H = (0.4 * torch.randn(N, K, d, generator=g)).double()
    src = np.sort(rng.integers(0, N, n_rows))
    dst = rng.integers(0, N, n_rows)
    dst[3] = src[3]                                               # v == u
    k = rng.integers(0, N, n_rows * m)
    k[::7] = -1                                                   # failed draws
    k[4 * m:5 * m] = -1                                           # a row whose draws all failed
    k[9] = dst[9 // m]                                            # k == v
    k[10] = src[10 // m]                                          # k == u
    k[12] = k[13] = 5                                             # a duplicated draw
    return Z, H, src, dst, m, k


def test_step64_is_autograd_of_the_written_out_loss():
    for t, w in ((1.0, 1.0 / 160), (2.0, 0.37)):
        Z, H, src, dst, m, k = _case()
        xp, xn, loss, dZ, dH = bpr_ref.step64(Z, H, src, dst, m, k, t, w)
        s, v, pu, pk, row, live = bpr_ref.triples(src, dst, m, k)
        assert int(live.sum()) == xn.numel() and xp.numel() == len(src)
        Zr, Hr = Z.clone().requires_grad_(True), H.clone().requires_grad_(True)
        total = bpr_ref.loss64(ref64.logit64(Zr, Hr, s, v, t), ref64.logit64(Zr, Hr, pu, pk, t), row, w)
        aZ, aH = torch.autograd.grad(total, (Zr, Hr))
        assert abs(float(total.detach()) - loss) <= 1e-12 * abs(loss)
        for got, ref in ((dZ, aZ), (dH, aH)):
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        # the row without a live draw has a logit and no part in anything: dropping it changes nothing
        keep = np.ones(len(src), bool)
        keep[4] = False
        _xp, _xn, loss2, dZ2, dH2 = bpr_ref.step64(Z, H, src[keep], dst[keep], m, k.reshape(-1, m)[keep].reshape(-1), t, w)
        assert abs(loss2 - loss) <= 1e-12 * abs(loss)
        for got, ref in ((dZ2, dZ), (dH2, dH)):
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_step32_restates_step64():
    Z, H, src, dst, m, k = _case(1)
    ref, fp32 = bpr_ref.bound(Z.float().double(), H.float().double(), src, dst, m, k, 1.0, 1.0 / 160)
    print("FIGURE fp32 restatement (cpu case)", {n: f"{v:.3g}" for n, v in fp32.items()})
    assert all(0 <= v < 1e-4 for v in fp32.values())             # fp32 against fp64: a restatement, not another formula


def test_sampled_negatives_with_dst():
    from disenlink_amd.sampled import SampledNegatives
    rng = np.random.default_rng(3)
    N, n_rows, m = 31, 200, 3
    src, dst = rng.integers(0, N, n_rows), rng.integers(0, N, n_rows)
    ex = (torch.from_numpy(src), torch.from_numpy(dst))
    sp = SampledNegatives(torch.from_numpy(src), m, N, ex, "cpu", dst=torch.from_numpy(dst))
    s, v = sp.src.numpy(), sp.dst.numpy()
    assert sp.src.dtype == sp.dst.dtype == sp.dst_order.dtype == sp.dst_rowptr.dtype == torch.int32
    assert (np.diff(s) >= 0).all()
    assert np.array_equal(np.sort(s.astype(np.int64) * N + v), np.sort(src * N + dst))          # the rows as a multiset
    perm = np.argsort(src, kind="stable")
    assert np.array_equal(s, src[perm]) and np.array_equal(v, dst[perm])                       # ... through the STABLE sort
    assert np.array_equal(sp.dst_order.numpy(), np.argsort(v, kind="stable"))
    assert np.array_equal(sp.dst_rowptr.numpy(), np.searchsorted(np.sort(v), np.arange(N + 1)))
    # without dst: every attribute is what it is with it, and the three lists are absent
    plain = SampledNegatives(torch.from_numpy(src), m, N, ex, "cpu")
    assert plain.dst is None and plain.dst_order is None and plain.dst_rowptr is None
    for name in ("src", "u_rowptr", "ex_rowptr", "ex_col"):
        assert torch.equal(getattr(plain, name), getattr(sp, name)), name
    assert (plain.m, plain.n_rows, plain.n_nodes, plain.n_entries) == (sp.m, sp.n_rows, sp.n_nodes, sp.n_entries)
    assert np.array_equal(plain.u_rowptr.numpy(), m * np.searchsorted(np.sort(src), np.arange(N + 1)))
    for bad in (torch.from_numpy(dst[:-1]), torch.from_numpy(dst).float(), torch.full((n_rows,), N)):
        try:
            SampledNegatives(torch.from_numpy(src), m, N, None, "cpu", dst=bad)
        except ValueError:
            continue
        raise AssertionError("a malformed dst must be refused")
