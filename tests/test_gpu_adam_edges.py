"""adam_update_kernel (dl_adam_step: the step counter on the device; dl_adam_step_at: counted by the caller) at the edges
test_adam_step_kernel_matches_torch_adam_on_odd_sizes does not visit: DL_ADAM_MAX_BUFS buffers with empty ones between
them, every buffer between guard elements; the all-zero point, where the denominator is eps alone; and a NaN gradient
element, which must poison its own element of p, m and v and nothing else.  Both entries must leave the same bits."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
SENTINEL = -12345.5
SIZES = [5, 0, 1030, 3, 0, 4099, 1, 70001]                              # DL_ADAM_MAX_BUFS = 8 buffers, two of them empty
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
TORCH_HYPER = dict(lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"])


def _guarded(values):
    """values[i] inside an allocation of its own, SENTINEL on GUARD floats before and after it -> (allocations, views)."""
    allocs, views = [], []
    for val in values:
        alloc = torch.full((2 * GUARD + val.numel(),), SENTINEL, dtype=torch.float32, device=DEV)
        view = alloc[GUARD: GUARD + val.numel()]
        view.copy_(val)
        allocs.append(alloc)
        views.append(view)
    return allocs, views


def _guards_intact(allocs, views):
    return all(bool((a[:GUARD] == SENTINEL).all()) and bool((a[GUARD + v.numel():] == SENTINEL).all()) for a, v in zip(allocs, views))


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _run(entry, p0, grads_per_step, wd):
    """`entry` over the steps -> (p, m, v views, state, all allocations intact?) after the last one."""
    from disenlink_amd import _lib
    lib = _lib.load()
    pa, p = _guarded(p0)
    ma, m = _guarded([torch.zeros_like(t) for t in p0])
    va, v = _guarded([torch.zeros_like(t) for t in p0])
    state = torch.zeros(3, dtype=torch.float32, device=DEV)
    numel = (C.c_size_t * len(p0))(*[t.numel() for t in p0])
    st = torch.cuda.current_stream().cuda_stream
    h = HYPER
    for step, gs in enumerate(grads_per_step, start=1):
        ga, g = _guarded(gs)
        g_before = [a.clone() for a in ga]
        if entry == "device-counter":
            _lib.check(lib.dl_adam_step(len(p), _ptrs(p), _ptrs(g), _ptrs(m), _ptrs(v), numel, state.data_ptr(), h["lr"], h["beta1"],
                                        h["beta2"], h["eps"], wd, st), "dl_adam_step")
        else:
            _lib.check(lib.dl_adam_step_at(len(p), _ptrs(p), _ptrs(g), _ptrs(m), _ptrs(v), numel, state.data_ptr(), step, h["lr"],
                                           h["beta1"], h["beta2"], h["eps"], wd, st), "dl_adam_step_at")
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ga, g_before))   # gradients are only read
    intact = _guards_intact(pa, p) and _guards_intact(ma, m) and _guards_intact(va, v)
    return p, m, v, state, intact


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _both_entries(p0, grads_per_step, wd):
    """The two entries on the same input: the same bits in p, m, v and the state, nothing outside the buffers written."""
    dev = _run("device-counter", p0, grads_per_step, wd)
    host = _run("host-counter", p0, grads_per_step, wd)
    assert dev[4] and host[4]
    for a, b in zip(dev[:3], host[:3]):
        assert _same_bits(a, b)
    assert torch.equal(dev[3], host[3]) and float(dev[3][0]) == len(grads_per_step)
    return dev[:3]


def _randn(seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.randn(n, generator=g) * scale).to(DEV) for n in SIZES]


@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_eight_buffers_with_empty_ones_between_them_follow_torch_adam_inside_their_guards(wd):
    """Three steps against torch.optim.Adam in fp32 (the reference's optimiser), at the tolerances of the 25-step test."""
    p0 = _randn(1)
    grads = [_randn(10 + s, 0.1 + s) for s in range(3)]
    p, m, v = _both_entries(p0, grads, wd)
    ref = [t.clone().requires_grad_(True) for t in p0 if t.numel()]
    opt = torch.optim.Adam(ref, weight_decay=wd, **TORCH_HYPER)
    for gs in grads:
        for r, g in zip(ref, [g for g in gs if g.numel()]):
            r.grad = g.clone()
        opt.step()
    live = [i for i, n in enumerate(SIZES) if n]
    for r, i in zip(ref, live):
        st = opt.state[r]
        assert torch.allclose(p[i], r.detach(), rtol=5e-6, atol=5e-7), (wd, SIZES[i], float((p[i] - r.detach()).abs().max()))
        assert torch.allclose(m[i], st["exp_avg"], rtol=1e-5, atol=1e-7) and torch.allclose(v[i], st["exp_avg_sq"], rtol=1e-5, atol=1e-9)


def test_at_the_all_zero_point_the_denominator_is_eps_alone():
    """g = m = v = 0.  Without weight decay the update is step_size * 0 / eps = 0: p keeps its bits (also a -0.0 and a
    denormal), m and v stay +0.  With weight decay the gradient is wd * p: compared with torch's Adam."""
    p0 = _randn(2)
    p0[2][:4] = torch.tensor([-0.0, 0.0, 1e-40, -3e3], device=DEV)
    zeros = [[torch.zeros_like(t) for t in p0] for _ in range(2)]
    p, m, v = _both_entries(p0, zeros, 0.0)
    assert _same_bits(p, p0)
    assert all(torch.equal(t.view(torch.int32), torch.zeros_like(t).view(torch.int32)) for t in m + v)
    p, m, v = _both_entries(p0, zeros, 5e-4)
    ref = [t.clone().requires_grad_(True) for t in p0 if t.numel()]
    opt = torch.optim.Adam(ref, weight_decay=5e-4, **TORCH_HYPER)
    for _ in range(2):
        for r in ref:
            r.grad = torch.zeros_like(r)
        opt.step()
    for r, i in zip(ref, [i for i, n in enumerate(SIZES) if n]):
        assert torch.allclose(p[i], r.detach(), rtol=5e-6, atol=5e-7), (SIZES[i], float((p[i] - r.detach()).abs().max()))
        assert not torch.equal(p[i], p0[i])                            # the decay moved it


def test_a_nan_gradient_element_poisons_its_own_element_only():
    p0 = _randn(3)
    clean = [_randn(20), _randn(21)]
    where = {0: [0, 4], 2: [3, 4, 1029], 3: [1], 5: [4098], 6: [0], 7: [0, 35000, 70000]}   # first / last elements, float4 edges
    bad = [[g.clone() for g in clean[0]], clean[1]]                     # NaN in the first step: it stays in m and v
    for i, at in where.items():
        bad[0][i][at] = float("nan")
    pc, mc, vc = _both_entries(p0, clean, 5e-4)
    pb, mb, vb = _both_entries(p0, bad, 5e-4)
    for i, n in enumerate(SIZES):
        mask = torch.zeros(n, dtype=torch.bool, device=DEV)
        if i in where:
            mask[where[i]] = True
        for name, got, ref in (("p", pb[i], pc[i]), ("m", mb[i], mc[i]), ("v", vb[i], vc[i])):
            assert torch.equal(torch.isnan(got), mask), (name, i)
            assert torch.equal(got[~mask], ref[~mask]), (name, i)      # every other element: the bits of the clean run
