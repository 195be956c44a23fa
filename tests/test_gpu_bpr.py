"""The pairwise ranking objective (BPR) on the resampled negatives: dl_score_sampled_bpr_train, its Python entry points, the step
and the loop, against tests/bpr_ref.py, on N = 70 nodes with the lists of tests/test_gpu_sample.py.

Bounds.  The project's rule (ref64, sample_ref): 4 x the error the fp32 restatement of the same sums (bpr_ref.step32: delta and
G_r taken in fp32) shows against fp64 — measured in this run as the largest figure over the (K, d, t, m) cases of test 1
(`_bounds`), never taken from what the kernels return.  Every figure is printed as a FIGURE line before anything is asserted
(pytest -s).
"""
import contextlib
import functools
import io
import warnings

import numpy as np
import pytest
import torch

import bpr_ref
import ref64
import sample_ref as sr
import test_gpu_sample as tgs                                   # its lists, tables, dataset and model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = tgs.N
SHAPES = ((8, 64), (4, 64), (3, 20), (4, 32))   # both register forms, the generic form at an odd width and at a geo-kernel shape
TEMPS = (1.0, 2.0)
MS = (1, 3)
CASES = [(K, d, t, m) for K, d in SHAPES for t in TEMPS for m in MS] + [(8, 64, t, 63) for t in TEMPS]
UNUSED = 7                                                       # the node no list names
HUB = 9                                                          # the dst of every fourth row: 75 rows, two chunks of 64
SEED, EPOCH = 1, 7


def _ops():
    from disenlink_amd import ops
    return ops


@functools.lru_cache(maxsize=1)
def exclusion():
    """sample_ref.exclusion_graph (node 0 excludes nothing, node 1 all but two, node 2 everything) with node 7 added to every
    row: no draw names it.  -> (rowptr int32, col int32)."""
    _n, _rowptr, _col, rows = sr.exclusion_graph()
    rows = [sorted(set(r) | {UNUSED}) for r in rows]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, np.array([c for r in rows for c in r], dtype=np.int32)


@functools.lru_cache(maxsize=1)
def positives():
    """dst of the 300 source rows: a hub named by 75 rows (it spans chunks on the positives' partner side), one row with
    dst == src, never node 7."""
    rng = np.random.default_rng(13)
    src = tgs.sources()
    dst = rng.integers(0, N, src.size)
    dst[dst == UNUSED] = 8
    dst[::4] = HUB
    dst[50] = src[50]
    assert (dst == HUB).sum() > 64 and dst[50] == src[50] and not (dst == UNUSED).any() and not (src == UNUSED).any()
    return dst


@functools.lru_cache(maxsize=None)
def draws(m):
    """The CPU sampler's k under `exclusion`, with one live entry patched to k == dst."""
    rowptr, col = exclusion()
    src, dst = tgs.sources(), positives()
    k, _failed = sr.sample(src, m, N, rowptr, col, SEED, EPOCH)
    u = np.repeat(src, m)
    assert (k[u == 2] == -1).all() and (u == 2).sum() == 6 * m    # rows whose negatives all failed
    assert not (k == UNUSED).any()
    e = int(np.flatnonzero((k >= 0) & (u == 3))[0])
    k[e] = dst[e // m]
    assert (k == np.repeat(dst, m)).any() and (k[u != 2] >= 0).mean() > 0.9
    return k.astype(np.int32)


def _sampled(m, keep=None):
    src, dst = tgs.sources(), positives()
    if keep is not None:
        src, dst = src[keep], dst[keep]
    return _ops().SampledNegatives(torch.from_numpy(src), m, N, None, DEV, dst=torch.from_numpy(dst))


def _weight(m):
    return 1.0 / (m * tgs.sources().size)


@functools.lru_cache(maxsize=None)
def reference(K, d, t, m):
    Z, H = tgs.tables(K, d)
    ref, fp32 = bpr_ref.bound(Z, H, tgs.sources(), positives(), m, draws(m), t, _weight(m))
    return ref, fp32


@functools.lru_cache(maxsize=1)
def _bounds():
    """4 x the largest error of the fp32 restatement against fp64 over the cases of test 1."""
    out = {}
    for K, d, t, m in CASES:
        for name, v in reference(K, d, t, m)[1].items():
            out[name] = max(out.get(name, 0.0), v)
    print("FIGURE fp32 restatement", {n: f"{v:.3g}" for n, v in out.items()})
    return {name: 4.0 * v for name, v in out.items()}


def _run(K, d, t, m, weight=None, keep=None, **kw):
    Z, H = tgs.tables(K, d)
    k = draws(m)
    if keep is not None:
        k = k.reshape(-1, m)[keep].reshape(-1)
    return _ops().score_sampled_bpr_train(Z.float().to(DEV), H.float().to(DEV), t, _sampled(m, keep), torch.from_numpy(k).to(DEV),
                                          _weight(m) if weight is None else weight, **kw)


# ------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("K,d,t,m", CASES)
def test_against_fp64(K, d, t, m):
    ref, _fp32 = reference(K, d, t, m)
    bound = _bounds()
    live = torch.from_numpy(draws(m) >= 0)
    loss, pos, neg, dZ, dH = _run(K, d, t, m)
    neg = neg.cpu()
    assert (neg[~live] == 0).all()                                 # a failed draw: logit 0
    fig = bpr_ref.figures(ref, (pos.cpu(), neg[live], float(loss), dZ.cpu(), dH.cpu()))
    print("FIGURE bpr trainer", f"K{K} d{d} t{t:g} m{m}", {n: f"{v:.3g}" for n, v in fig.items()},
          "bound", {n: f"{v:.3g}" for n, v in bound.items()})
    for name in ("pos", "neg", "loss", "dZ", "dH"):
        assert fig[name] <= bound[name], (name, fig[name], bound[name])
    assert float(dZ[UNUSED].abs().max()) == 0 and float(dH[UNUSED].abs().max()) == 0      # nobody names node 7: exactly 0
    # the rows whose draws all failed contribute nothing: the same answer without them (their pos_logit is still written)
    keep = tgs.sources() != 2
    loss2, pos2, _neg2, dZ2, dH2 = _run(K, d, t, m, keep=keep)
    assert torch.equal(pos2, pos[torch.from_numpy(keep).to(DEV)]) and bool(torch.isfinite(pos).all())
    f2 = {"loss": abs(float(loss2) - float(loss)) / abs(float(loss)), "dZ": ref64.row_ratio(dZ2.cpu(), dZ.cpu().double()),
          "dH": ref64.row_ratio(dH2.cpu(), dH.cpu().double())}
    print("FIGURE without the dead rows", f"K{K} d{d} t{t:g} m{m}", {n: f"{v:.3g}" for n, v in f2.items()})
    for name, v in f2.items():
        assert v <= bound[name], (name, v, bound[name])


# ------------------------------------------------------------------------------------------------ 2. the existing kernels' bits
@pytest.mark.parametrize("t", TEMPS)
@pytest.mark.parametrize("K,d", SHAPES)
def test_logits_of_the_existing_kernels(K, d, t):
    ops = _ops()
    from disenlink_amd.graph import PairList
    m = 3
    Z, H = tgs.tables(K, d)
    Zg, Hg = Z.float().to(DEV), H.float().to(DEV)
    _loss, pos, neg, _dZ, _dH = _run(K, d, t, m)
    k = torch.from_numpy(draws(m)).to(DEV)
    _l, old_neg, _z, _h = ops.score_sampled_train(Zg, Hg, t, _sampled(m), k, _weight(m), logits=True)
    if (K, d) != (4, 32):
        assert torch.equal(neg, old_neg)                           # the register forms and the generic order: the same bits
    else:                                                          # the sampled trainer runs its geo kernel there
        live = k >= 0
        ref = reference(K, d, t, m)[0][1]
        for name, got in (("bpr", neg), ("sampled", old_neg)):
            fig = bpr_ref._score_fig(got[live].cpu(), ref)
            print("FIGURE neg_logit at the geo shape", name, f"t{t:g} {fig:.3g} bound {_bounds()['neg']:.3g}")
            assert fig <= _bounds()["neg"]
    if d == 64:
        src, dst = torch.from_numpy(tgs.sources()).to(DEV), torch.from_numpy(positives()).to(DEV)
        pairs = PairList.build(src, dst, N, row_bytes=K * d * 4)
        assert ops.score_pairs_train_logits_supported(pairs, K, d, 0)
        label = torch.ones(src.numel(), dtype=torch.float32, device=DEV)
        weight = torch.full((src.numel(),), 1.0 / src.numel(), dtype=torch.float32, device=DEV)
        old_pos, _z, _h = ops.score_pairs_train_logits(Zg, Hg, pairs, t, label, weight)
        assert torch.equal(pos, old_pos)


# ------------------------------------------------------------------------------------------------ 3. determinism, poison, accumulate
@pytest.mark.parametrize("K,d,m", [(K, d, 3) for K, d in SHAPES] + [(8, 64, 63)])
def test_determinism_poison_accumulate(K, d, m):
    from disenlink_amd import _dev
    assert _dev._POISON, "the suite runs with DL_POISON=1: outputs and workspace start as NaN bit patterns"
    out = _run(K, d, 2.0, m)
    for name, v in zip(("loss", "pos", "neg", "dZ", "dH"), out):
        assert bool(torch.isfinite(v).all()), name
    again = _run(K, d, 2.0, m)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    loss, pos, neg, dZ, dH = out
    base_z, base_h = torch.full_like(dZ, 0.5), torch.full_like(dH, -0.25)
    _l, _p, _n, accZ, accH = _run(K, d, 2.0, m, dZ_accum=base_z.clone(), dH_accum=base_h.clone())
    assert torch.equal(accZ, base_z + dZ) and torch.equal(accH, base_h + dH)
    l0, p0, n0, z0, h0 = _run(K, d, 2.0, m, weight=0.0)            # weight 0: no loss, no gradient, the logits as ever
    assert float(l0) == 0 and float(z0.abs().max()) == 0 and float(h0.abs().max()) == 0
    assert torch.equal(p0, pos) and torch.equal(n0, neg)
    none = np.zeros(tgs.sources().size, bool)                      # n_rows = 0
    le, pe, ne, ze, he = _run(K, d, 2.0, m, keep=none)
    assert float(le) == 0 and pe.numel() == 0 and ne.numel() == 0 and float(ze.abs().max()) == 0 and float(he.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals():
    ops = _ops()
    from disenlink_amd._lib import DisenlinkHipError
    from disenlink_amd.train import run_link_prediction
    m = 3
    sp = _sampled(m)
    k = torch.from_numpy(draws(m)).to(DEV)
    Z = torch.zeros(N, 8, 64, device=DEV)
    with pytest.raises(TypeError):
        ops.score_sampled_bpr_train(Z.bfloat16(), Z.bfloat16(), 1.0, sp, k, 1.0)
    assert not ops.score_sampled_bpr_supported(8, 64, torch.bfloat16) and ops.score_sampled_bpr_supported(8, 64)
    big = torch.zeros(N, 64, 64, device=DEV)                       # K d = 4096 > 2048
    with pytest.raises(DisenlinkHipError):
        ops.score_sampled_bpr_train(big, big, 1.0, sp, k, 1.0)
    src, dst = torch.from_numpy(tgs.sources()), torch.from_numpy(positives())
    sp64 = ops.SampledNegatives(src, 64, N, None, DEV, dst=dst)    # m = 64: a row no longer fits a chunk
    with pytest.raises(ValueError, match="m <= 63"):
        ops.score_sampled_bpr_train(Z, Z, 1.0, sp64, torch.zeros(sp64.n_entries, dtype=torch.int32, device=DEV), 1.0)
    with pytest.raises(ValueError, match="dst"):
        ops.score_sampled_bpr_train(Z, Z, 1.0, ops.SampledNegatives(src, m, N, None, DEV), k, 1.0)
    with pytest.raises(ValueError):
        ops.score_sampled_bpr_train(Z, Z, 1.0, sp, k[:-1].contiguous(), 1.0)
    _split, plain_run, x = tgs._prepared(False)
    _split, run, _x = tgs._prepared(True)
    model = tgs._model()
    with pytest.raises(ValueError, match="use_graph"):
        run_link_prediction(model, x, run, epochs=1, objective="bpr", use_graph=True)
    with pytest.raises(ValueError, match="GPU"):
        run_link_prediction(model, x.cpu(), run, epochs=1, objective="bpr")
    with pytest.raises(ValueError, match="prepare_run"):
        run_link_prediction(model, x, plain_run, epochs=1, objective="bpr")
    from disenlink_amd import main
    for extra in (["--gpus", "2"], ["--graph"], ["--table-dtype", "bf16"]):
        with pytest.raises(SystemExit, match="one GPU"):           # refused before anything is launched
            main.main(["--dataset", "squirrel", "--synthetic", "--objective", "bpr", *extra])


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_end_to_end():
    import torch.nn.functional as F
    ops = _ops()
    from disenlink_amd.graph import PairList
    from disenlink_amd.train import _make_adam, run_link_prediction
    split, run, x = tgs._prepared(True)
    sp, m = run.sampled, tgs.M_TRAIN
    seed, lr = 9, 1e-3
    order = np.argsort(split.train_src, kind="stable")
    assert np.array_equal(sp.src.cpu().numpy(), split.train_src[order]) and np.array_equal(sp.dst.cpu().numpy(), split.train_dst[order])
    assert run.val_pairs.n_pairs == run.label_val.numel()
    w = 1.0 / sp.n_entries
    k0, failed = ops.sample_negatives(sp, seed=seed, epoch=0)
    assert int(failed) == 0

    # (i) the parameter gradients of one step against a hand-rolled one on a second identical model: forward_pair_logits on
    # ONE PairList [edge rows | live entries], softplus of the differences by torch, autograd
    model = tgs._model()
    _emb, pos, neg, val, loss = model.forward_bpr_loss(x, run.graph, sp, k0, w, run.val_pairs)
    loss.backward()
    g_new = tgs._grads(model)
    hand = tgs._model()
    live = k0 >= 0
    row = (torch.arange(sp.n_entries, device=DEV) // m)[live]
    pu = torch.cat([sp.src.long(), sp.src.long()[row]])
    pv = torch.cat([sp.dst.long(), k0.long()[live]])
    both = PairList.build(pu, pv, N, row_bytes=8 * 64 * 4)
    _emb, logit = hand.forward_pair_logits(x, run.graph, both)
    pos_h, neg_h = logit[:sp.n_rows], logit[sp.n_rows:]
    loss_h = (w * F.softplus(neg_h - pos_h[row])).sum()
    loss_h.backward()
    g_hand = tgs._grads(hand)
    # Tolerance: each step's scorer gradient lies within the fp64 bound B of case 1 (row ratio), so the two differ by at most
    # 2 B of a row's scale; everything behind the scorer is one linear chain of the same kernels (test_gpu_sample.py::
    # test_end_to_end), hence the comparison per parameter tensor, in units of its largest entry.
    B = max(_bounds()[n] for n in ("dZ", "dH"))
    lo, lh = float(loss.detach()), float(loss_h.detach())
    print("FIGURE end to end loss", lo, lh, "bound", 2 * _bounds()["loss"])
    assert abs(lo - lh) <= 2 * _bounds()["loss"] * abs(lh)
    for i, (gn, gh) in enumerate(zip(g_new, g_hand)):
        if float(gh.abs().max()) == 0:                             # a parameter the loss does not reach
            assert float(gn.abs().max()) == 0
            continue
        err = float((gn - gh).abs().max()) / float(gh.abs().max())
        print("FIGURE end to end gradient", i, tuple(gn.shape), f"{err:.3g} bound {2 * B:.3g}")
        assert err <= 2 * B
    with torch.no_grad():                                          # the validation logits: the forward scorer's bits
        _emb, val_ref = tgs._model().forward_pair_logits(x, run.graph, run.val_pairs)
    assert torch.equal(val, val_ref) and not val.requires_grad and not pos.requires_grad and not neg.requires_grad

    # (ii) the loop: 3 epochs; its losses are the bits of a hand loop over the same calls with the epoch counter 0, 1, 2
    model = tgs._model()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                             # no failed draw on this graph: no warning
        res = run_link_prediction(model, x, run, epochs=3, lr=lr, objective="bpr", resample_seed=seed)
    assert res.epochs_run == 3 and res.failed_draws == 0 and all(np.isfinite(res.losses))
    assert len(res.val_aucs) == 3 and all(np.isfinite(res.val_aucs)) and np.isfinite(res.test_auc)
    hand = tgs._model()
    opt = _make_adam(hand, True, lr, 5e-4)
    losses = []
    for e in range(3):
        hand.train()
        k, _f = ops.sample_negatives(sp, seed=seed, epoch=e)
        _emb, _p, _n, _v, loss = hand.forward_bpr_loss(x, run.graph, sp, k, w, run.val_pairs)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach().double()))
    assert losses == [float(v) for v in res.losses], (losses, res.losses)


def test_cli_objective_bpr_prints_metrics():
    from disenlink_amd.main import main
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        main(["--dataset", "chameleon", "--synthetic", "--epochs", "3", "--run", "1", "--objective", "bpr", "--rank-eval", "--quiet"])
    final = [ln for ln in buf.getvalue().splitlines() if ln.startswith("final")]
    assert len(final) == 1
    toks = final[0].split()
    vals = {toks[i]: float(toks[i + 1]) for i in range(3, len(toks) - 1, 2)}
    assert set(vals) == {"mrr", "hits@1", "hits@10", "hits@50", "hits@100"}
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in vals.values())
