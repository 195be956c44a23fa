"""The CPU restatements the device sampler and the sampled trainer are judged by (tests/sample_ref.py), checked themselves:
the Philox round function against numpy's own generator and the published known-answer counters, the sampler's rule, and the
fp64 loss against torch's BCE.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sample_ref as sr

# Random123's known-answer vectors of philox4x32-10 (kat_vectors): counter, key -> output
KAT32 = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


@pytest.mark.parametrize("ctr,key,out", KAT32)
def test_philox4x32_known_answers(ctr, key, out):
    assert tuple(int(v) for v in sr.philox(ctr, key, 32)) == out


@pytest.mark.parametrize("ctr,key", [((0, 0, 0, 0), (0, 0)), ((5, 7, 11, 13), (17, 19)),
                                     ((2 ** 64 - 1, 0, 3, 2 ** 63), (2 ** 64 - 1, 12345))])
def test_round_function_is_numpy_philox(ctr, key):
    """numpy.random.Philox is Philox4x64-10 — the same round structure at W = 64 with its own constants.  Its counter layout:
    counter[0] is the least significant word, and the generator INCREMENTS the 256-bit counter before it produces its first
    block, so random_raw(4) of Philox(counter=c, key=k) is the block of c + 1."""
    got = np.random.Philox(counter=np.array(ctr, dtype=np.uint64), key=np.array(key, dtype=np.uint64)).random_raw(4)
    big = sum(v << (64 * i) for i, v in enumerate(ctr)) + 1
    inc = tuple((big >> (64 * i)) & (2 ** 64 - 1) for i in range(4))
    assert [int(v) for v in got] == [int(v) for v in sr.philox(inc, key, 64)]


_graph = sr.exclusion_graph


def test_sampler_never_returns_an_excluded_pair():
    N, rowptr, col, rows = _graph()
    src = np.sort(np.random.default_rng(0).integers(0, N, 200))
    for exclude_self in (False, True):
        k, _failed = sr.sample(src, 3, N, rowptr, col, seed=11, epoch=4, exclude_self=exclude_self)
        u = np.repeat(src, 3)
        for a, b in zip(u.tolist(), k.tolist()):
            assert b == -1 or (0 <= b < N and b not in rows[a] and not (exclude_self and a == b))


def test_sampler_is_a_pure_function_of_seed_epoch_entry():
    N, rowptr, col, _rows = _graph()
    src = np.sort(np.random.default_rng(1).integers(3, N, 120))
    k, _ = sr.sample(src, 2, N, rowptr, col, seed=5, epoch=9)
    again, _ = sr.sample(src, 2, N, rowptr, col, seed=5, epoch=9)
    assert np.array_equal(k, again)
    # entry e alone decides: the first 40 rows drawn on their own give the first 80 entries
    head, _ = sr.sample(src[:40], 2, N, rowptr, col, seed=5, epoch=9)
    assert np.array_equal(head, k[:80])
    assert not np.array_equal(k, sr.sample(src, 2, N, rowptr, col, seed=5, epoch=10)[0])
    assert not np.array_equal(k, sr.sample(src, 2, N, rowptr, col, seed=6, epoch=9)[0])
    # the epoch's high word is part of the counter
    assert not np.array_equal(k, sr.sample(src, 2, N, rowptr, col, seed=5, epoch=9 + 2 ** 32)[0])


def test_sampler_flags_a_saturated_row():
    N, rowptr, col, _rows = _graph()
    src = np.array([0, 2, 2, 5])
    k, failed = sr.sample(src, 3, N, rowptr, col, seed=0, epoch=0)
    assert failed == 6 and (k[3:9] == -1).all() and (k[:3] >= 0).all() and (k[9:] >= 0).all()


@pytest.mark.parametrize("space", ["prob", "logit"])
def test_fp64_loss_is_torch_bce_on_the_listed_pairs(space):
    g = torch.Generator().manual_seed(0)
    N, K, d, t, w = 30, 3, 8, 2.0, 1.0 / 7
    Z = 0.25 * torch.randn(N, K, d, generator=g, dtype=torch.float64)
    H = 0.25 * torch.randn(N, K, d, generator=g, dtype=torch.float64)
    src = np.sort(np.random.default_rng(2).integers(0, N, 25))
    k = np.random.default_rng(3).integers(-1, N, 50).astype(np.int32)
    pu, pv, live = sr.listed(src, 2, k)
    assert int(live.sum()) == int((k >= 0).sum()) < 50
    score, loss, dZ, dH = sr.step64(Z, H, pu, pv, t, w, space)
    Zr, Hr = Z.clone().requires_grad_(True), H.clone().requires_grad_(True)
    x = ((Hr[pu] * Hr[pv]).sum(-1) * torch.exp((Zr[pu] * Zr[pv]).sum(-1) / t)).sum(-1)
    zero = torch.zeros_like(x)
    ref = w * (F.binary_cross_entropy_with_logits(x, zero, reduction="sum") if space == "logit"
               else F.binary_cross_entropy(torch.sigmoid(x), zero, reduction="sum"))
    rz, rh = torch.autograd.grad(ref, (Zr, Hr))
    # probability space forms the loss and the coefficient at the fp32 probability: 2^-24 of a probability apart, which
    # log(1 - p) divides by 1 - p (the scores here stay below 0.97: 6e-8 / 0.03 = 2e-6)
    assert float(torch.sigmoid(x).max()) < 0.97
    tol = 1e-12 if space == "logit" else 2e-6
    assert abs(loss - float(ref.detach())) <= tol * abs(float(ref.detach()))
    assert float((dZ - rz).abs().max()) <= tol * float(rz.abs().max())
    assert float((dH - rh).abs().max()) <= tol * float(rh.abs().max())
    assert score.numel() == pu.numel()
