"""Hard negatives on the device: dl_sample_negatives_hard, its Python entry points, the steps that draw inside their forward
and the loop, against tests/hard_ref.py, on N = 70 nodes with the lists of tests/test_gpu_sample.py.

Bounds.  The draws are exact: every candidate is the CPU restatement's.  The selection is held to fp64 where fp64 decides: an
entry is decisive when the fp64 logits of its best node and of its best other node differ by more than `tol` = 4 x the error
of the fp32 restatement of the same logits against fp64 (the project's rule; measured in the run, never taken from the
kernel), relative to max(|best|, median |x|); there the kept node must be the fp64 one, and at most 1 % of the live entries may
be non-decisive (tests/test_hard_cpu.py shows that the reference itself meets this on every input used here).  Everything else
is bit equality.  Every figure is printed as a FIGURE line before anything is asserted (pytest -s).
"""
import contextlib
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import hard_ref as hr
import sample_ref as sr
import test_gpu_bpr as tgb                                      # its positives and its SampledNegatives with dst
import test_gpu_sample as tgs                                   # its lists, tables, dataset and model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = tgs.N
SEED, EPOCH = hr.SEED, hr.EPOCH


def _ops():
    from disenlink_amd import ops
    return ops


def _tables(K, d):
    Z, H = tgs.tables(K, d)
    return Z.float().to(DEV), H.float().to(DEV)


@functools.lru_cache(maxsize=None)
def _cand(m, c):
    _n, rowptr, col, _rows = sr.exclusion_graph()
    return hr.candidates(tgs.sources(), m, N, rowptr, col, SEED, EPOCH, c)


def _draw(Zg, Hg, t, m, c, **kw):
    k, x, failed = _ops().sample_hard_negatives(Zg, Hg, t, tgs._sampled(m), c, seed=SEED, epoch=EPOCH, **kw)
    return k.cpu().numpy(), x.cpu().numpy(), int(failed)


def _check_selection(tag, k, failed, cand, x64, tol):
    """Every k one of its entry's live candidates (-1 exactly where there is none), the failed count, the fp64 node on every
    decisive entry, and the cap on the non-decisive share."""
    live = cand >= 0
    none = ~live.any(axis=1)
    assert np.array_equal(k < 0, none) and failed == int(none.sum())
    assert ((cand == k[:, None]) & live).any(axis=1)[~none].all()
    dec, node = hr.decisive(cand, x64, tol)
    share = hr.non_decisive_share(cand, x64, tol)
    wrong = int((k[dec] != node[dec]).sum())
    print("FIGURE hard selection", tag, f"tol {tol:.3g} non-decisive {share:.4f} decisive {int(dec.sum())} wrong {wrong}")
    assert wrong == 0
    return share


# ------------------------------------------------------------------------------------------------ 1. c = 1 is the existing sampler
@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("m", [1, 3, 5])
def test_one_candidate_is_the_existing_sampler(m, exclude_self):
    ops = _ops()
    sp = tgs._sampled(m)
    for (K, d), (seed, epochs) in zip(((8, 64), (3, 20)), tgs.SEED_EPOCHS.items()):
        Zg, Hg = _tables(K, d)
        for epoch in epochs[:2]:
            k0, f0 = ops.sample_negatives(sp, seed=seed, epoch=epoch, exclude_self=exclude_self)
            k1, _x, f1 = ops.sample_hard_negatives(Zg, Hg, 1.0, sp, 1, seed=seed, epoch=epoch, exclude_self=exclude_self)
            assert torch.equal(k0, k1) and int(f0) == int(f1) == 6 * m
            assert np.array_equal(k1.cpu().numpy(), tgs.ref_draw(m, seed, epoch, exclude_self)[0])
    ep = torch.tensor([EPOCH], dtype=torch.int64, device=DEV)       # the epoch is read from device memory
    ka, _x, _f = ops.sample_hard_negatives(Zg, Hg, 1.0, sp, 1, seed=SEED, epoch=ep, exclude_self=exclude_self)
    ep.add_(1)
    kb, _x, _f = ops.sample_hard_negatives(Zg, Hg, 1.0, sp, 1, seed=SEED, epoch=ep, exclude_self=exclude_self)
    assert np.array_equal(ka.cpu().numpy(), tgs.ref_draw(m, SEED, EPOCH, exclude_self)[0])
    assert np.array_equal(kb.cpu().numpy(), tgs.ref_draw(m, SEED, EPOCH + 1, exclude_self)[0])


# ------------------------------------------------------------------------------------------------ 2. selection against fp64
@pytest.mark.parametrize("m,c", hr.MC)
@pytest.mark.parametrize("t", hr.TEMPS)
@pytest.mark.parametrize("K,d", hr.SHAPES)
def test_selection_against_fp64(K, d, t, m, c):
    Z, H = tgs.tables(K, d)
    cand = _cand(m, c)
    x64, tol, fig = hr.tolerance(Z, H, tgs.sources(), m, cand, t)
    print("FIGURE fp32 restatement of the candidates' logits", f"K{K} d{d} t{t:g} m{m} c{c}", f"{fig:.3g}")
    k, x, failed = _draw(*_tables(K, d), t, m, c)
    share = _check_selection(f"K{K} d{d} t{t:g} m{m} c{c}", k, failed, cand, x64.numpy(), tol)
    assert share <= hr.MAX_NON_DECISIVE
    u = np.repeat(tgs.sources(), m)
    assert (k[u == 2] == -1).all() and failed == 6 * m             # node 2 excludes everything; nobody else fails with c >= 3


# ------------------------------------------------------------------------------------------------ 3. the trainer's bits
@pytest.mark.parametrize("t", hr.TEMPS)
@pytest.mark.parametrize("K,d", hr.SHAPES)
def test_logit_is_the_trainers(K, d, t):
    ops = _ops()
    m, c = 3, 4
    Z, H = tgs.tables(K, d)
    Zg, Hg = _tables(K, d)
    sp = tgs._sampled(m)
    k, x, _failed = ops.sample_hard_negatives(Zg, Hg, t, sp, c, seed=SEED, epoch=EPOCH)
    w = 1.0 / sp.n_entries
    _loss, _pos, neg, _dZ, _dH = ops.score_sampled_bpr_train(Zg, Hg, t, tgb._sampled(m), k, w)
    assert torch.equal(x, neg)                                     # bit for bit, dead entries (0) included
    assert bool((x[k < 0] == 0).all()) and bool((k < 0).any())
    # within tol of fp64 at the kept candidate
    cand = _cand(m, c)
    x64, tol, _fig = hr.tolerance(Z, H, tgs.sources(), m, cand, t)
    kn = k.cpu().numpy()
    live = kn >= 0
    which = np.argmax((cand == kn[:, None]) & (cand >= 0), axis=1)
    ref = x64.numpy()[np.arange(kn.size), which][live]
    floor = np.median(np.abs(x64.numpy()[cand >= 0]))
    err = float(np.max(np.abs(x.cpu().numpy()[live] - ref) / np.maximum(np.abs(ref), floor)))
    print("FIGURE hard logit against fp64", f"K{K} d{d} t{t:g}", f"{err:.3g} tol {tol:.3g}")
    assert err <= tol
    # candidate 0 is the plain draw: the kept logit is never below the plain draw's, exactly
    k0, _f = ops.sample_negatives(sp, seed=SEED, epoch=EPOCH)
    _l, _p, plain, _z, _h = ops.score_sampled_bpr_train(Zg, Hg, t, tgb._sampled(m), k0, w)
    alive = k0 >= 0
    assert bool(alive.any()) and bool((x[alive] >= plain[alive]).all())
    assert bool((x[alive] > plain[alive]).any())                   # and the selection does select


# ------------------------------------------------------------------------------------------------ 4. ties and NaN
@pytest.mark.parametrize("K,d", [(8, 64), (3, 20)])
def test_ties_nan_and_inf(K, d):
    m, c, t = 1, 16, 1.0
    Z, H = tgs.tables(K, d)
    cand = _cand(m, c)
    live = cand >= 0
    first = np.where(live.any(axis=1), cand[np.arange(cand.shape[0]), np.argmax(live, axis=1)], -1)
    src = tgs.sources()

    # (i) every node with the rows of node 5: every candidate of an entry ties, the first live one is kept
    Zt, Ht = Z[5:6].expand_as(Z).contiguous(), H[5:6].expand_as(H).contiguous()
    k, x, _failed = _draw(Zt.float().to(DEV), Ht.float().to(DEV), t, m, c)
    assert np.array_equal(k, first) and (k >= 0).sum() > 250

    # (ii) two nodes with identical rows, four times the usual scale: where the pair beats every other node decisively, the
    # one that comes first among the candidates is kept
    a, b = 20, 41
    Z2, H2 = Z.clone(), H.clone()
    H2[a] = 4.0 * H[a]
    Z2[b], H2[b] = Z2[a], H2[a]
    merged = np.where(cand == b, a, cand)
    x64, tol, _fig = hr.tolerance(Z2, H2, src, m, cand, t)
    dec, node = hr.decisive(merged, x64.numpy(), tol)
    k, x, _failed = _draw(Z2.float().to(DEV), H2.float().to(DEV), t, m, c)
    isab = (cand == a) | (cand == b)
    both = dec & (node == a) & (cand == a).any(axis=1) & (cand == b).any(axis=1)
    expect = cand[np.arange(cand.shape[0]), np.argmax(isab, axis=1)]
    print("FIGURE hard ties", f"K{K} d{d}", "entries won by the twin nodes with both among the candidates:", int(both.sum()),
          "b first:", int((expect[both] == b).sum()))
    assert both.sum() >= 2 and (expect[both] == b).any() and (expect[both] == a).any()
    assert np.array_equal(k[both], expect[both])

    # (iii) a node whose H row is NaN: never kept while another live candidate exists, kept when it is the only one
    bad = 55                                                       # (no source: as a source it would score NaN against everybody)
    Z3, H3 = Z.clone(), H.clone()
    H3[bad] = float("nan")
    k, x, failed = _draw(Z3.float().to(DEV), H3.float().to(DEV), t, m, c)
    others = (live & (cand != bad)).any(axis=1)
    assert (cand == bad).any(axis=1).sum() > 20 and not (k[others] == bad).any()
    x64, tol, _fig = hr.tolerance(Z3, H3, src, m, np.where(cand == bad, -1, cand), t)     # (the tolerance of the finite logits)
    x64 = hr.logits(Z3, H3, src, m, cand, t)
    _check_selection(f"K{K} d{d} NaN row", k, failed, cand, x64.numpy(), tol)
    k1, x1, _f = _draw(Z3.float().to(DEV), H3.float().to(DEV), t, m, 1)
    only = cand[:, 0] == bad
    assert only.sum() >= 1 and (k1[only] == bad).all() and np.isnan(x1[only]).all() and not np.isnan(x1[~only]).any()

    # (iv) a +inf logit wins: for the 30 rows of source 3, a node whose H row is 3e38 sign(H[3]) under z = 0
    rows3 = np.flatnonzero(src == 3)
    vals, counts = np.unique(cand[rows3][(cand[rows3] >= 0) & (cand[rows3] != 3)], return_counts=True)
    p = int(vals[np.argmax(counts)])
    Z4, H4 = Z.clone(), H.clone()
    Z4[p] = 0.0
    H4[p] = 3e38 * torch.sign(H[3])
    k, x, _failed = _draw(Z4.float().to(DEV), H4.float().to(DEV), t, m, c)
    has = rows3[(cand[rows3] == p).any(axis=1)]
    assert has.size >= 3 and (k[has] == p).all() and np.isposinf(x[has]).all()


# ------------------------------------------------------------------------------------------------ 5. edges
@pytest.mark.parametrize("K,d", [(8, 64), (4, 64), (3, 20)])
def test_edges(K, d):
    from disenlink_amd import _dev, _lib
    ops = _ops()
    assert _dev._POISON, "the suite runs with DL_POISON=1: outputs start as NaN bit patterns"
    Z, H = tgs.tables(K, d)
    Zg, Hg = _tables(K, d)
    t = 2.0
    _n, rowptr, col, _rows = sr.exclusion_graph()
    ex = (torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV))
    # c = 3 does not divide 64 (21 entries per chunk, one idle lane) and leaves the last chunk partial (900 = 42 x 21 + 18), as
    # does c = 4 (900 = 56 x 16 + 4); c = 64: one entry per chunk; twice the same bits, every output written
    for m, c in ((3, 3), (3, 4), (1, 64)):
        sp = tgs._sampled(m)
        out = ops.sample_hard_negatives(Zg, Hg, t, sp, c, seed=SEED, epoch=EPOCH)
        again = ops.sample_hard_negatives(Zg, Hg, t, sp, c, seed=SEED, epoch=EPOCH)
        assert all(torch.equal(p, q) for p, q in zip(out, again))
        k, x, failed = out
        assert sp.n_entries % (64 // c) != 0 or c == 64
        assert sp.n_entries > 4 * (64 // c)                         # more than one workgroup
        assert bool(torch.isfinite(x).all()) and int(k.min()) == -1 and int(k.max()) < N and int(failed) == 6 * m
        # n_failed given: added onto it
        acc = torch.full((1,), 100, dtype=torch.int32, device=DEV)
        _k, _x, f2 = ops.sample_hard_negatives(Zg, Hg, t, sp, c, seed=SEED, epoch=EPOCH, n_failed=acc)
        assert f2 is acc and int(acc) == 100 + 6 * m
    # n_rows = 0
    empty = torch.zeros(0, dtype=torch.int32, device=DEV)
    k, x, failed = ops.sample_hard_negatives(Zg, Hg, t, empty, 4, 3, N, ex, seed=SEED, epoch=EPOCH)
    assert k.numel() == 0 and x.numel() == 0 and int(failed) == 0
    # one entry
    one = np.array([5])
    cand = hr.candidates(one, 1, N, rowptr, col, SEED, EPOCH, 4)
    x64, tol, _fig = hr.tolerance(Z, H, one, 1, cand, t)
    k, x, failed = ops.sample_hard_negatives(Zg, Hg, t, torch.from_numpy(one).int().to(DEV), 4, 1, N, ex, seed=SEED, epoch=EPOCH)
    assert k.numel() == 1
    _check_selection(f"K{K} d{d} one entry", k.cpu().numpy(), int(failed), cand, x64.numpy(), tol)
    # sources outside the table: -1, counted once each, logit 0; the entries between them as ever
    raw = np.array([0, N, 5, -3, 2 ** 31 - 1, 9])
    cand = hr.candidates(raw, 2, N, rowptr, col, SEED, EPOCH, 3)
    x64, tol, _fig = hr.tolerance(Z, H, np.where((raw >= 0) & (raw < N), raw, 0), 2, cand, t)
    k, x, failed = ops.sample_hard_negatives(Zg, Hg, t, torch.from_numpy(raw).int().to(DEV), 3, 2, N, ex, seed=SEED, epoch=EPOCH)
    k, x = k.cpu().numpy(), x.cpu().numpy()
    outside = np.repeat((raw < 0) | (raw >= N), 2)
    assert (k[outside] == -1).all() and (x[outside] == 0).all() and int(failed) == 6 and (k[~outside] >= 0).all()
    _check_selection(f"K{K} d{d} sources outside", k, int(failed), cand, x64.numpy(), tol)
    # x_out = NULL: the same k
    sp = tgs._sampled(3)
    k_ref, _x, _f = ops.sample_hard_negatives(Zg, Hg, t, sp, 4, seed=SEED, epoch=EPOCH)
    k2 = torch.full((sp.n_entries,), -7, dtype=torch.int32, device=DEV)
    nf = torch.zeros(1, dtype=torch.int32, device=DEV)
    ep = torch.tensor([EPOCH], dtype=torch.int64, device=DEV)
    rc = _lib.load().dl_sample_negatives_hard(Zg.data_ptr(), Hg.data_ptr(), N, K, d, _lib.DL_F32, ctypes.c_float(t), sp.src.data_ptr(),
                                              sp.n_rows, 3, 4, sp.ex_rowptr.data_ptr(), sp.ex_col.data_ptr(), SEED, ep.data_ptr(), 0,
                                              k2.data_ptr(), None, nf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(k2, k_ref) and int(nf) == 18
    # the device-side refusals of the entry
    big = torch.zeros(N, 64, 64, device=DEV)
    with pytest.raises(_lib.DisenlinkHipError):
        ops.sample_hard_negatives(big, big, t, sp, 4)
    with pytest.raises(ValueError, match="nodes"):
        ops.sample_hard_negatives(Zg[:N - 1], Hg[:N - 1], t, sp, 4)


# ------------------------------------------------------------------------------------------------ 6. the step
def _step_inputs():
    _split, run, x = tgs._prepared(True)
    a, n_val = run.n_pos, run.label_val.numel()
    label = torch.cat([run.label_pos, run.label_val])
    weight = torch.cat([torch.full((a,), 1.0 / a, device=DEV), torch.zeros(n_val, device=DEV)])
    return run, x, label, weight


def _forward_tables(model, run, x):
    ops = _ops()
    with torch.no_grad():
        Z = model.project(x)
        Zt, _p, _a, _s, H = ops.step_tables(run.graph, Z, float(model.beta), float(model.temperature), torch.float32)
    return Zt, H


@pytest.mark.parametrize("step", ["bpr", "pairs", "pairs-logit"])
def test_step_draws_from_its_own_tables(step):
    ops = _ops()
    run, x, label, weight = _step_inputs()
    sp = run.sampled
    seed, c = 9, 4
    w = 1.0 / sp.n_entries

    def call(model, k, **kw):
        if step == "bpr":
            _emb, pos, neg, val, loss = model.forward_bpr_loss(x, run.graph, sp, k, w, run.val_pairs, **kw)
            outs = (pos, neg, val)
        else:
            fn = model.forward_pair_logits_resampled_loss if step == "pairs-logit" else model.forward_pairs_resampled_loss
            _emb, score, neg, loss = fn(x, run.graph, run.pos_val_pairs, label, weight, sp, k, w / tgs.M_TRAIN, **kw)
            outs = (score, neg)
        loss.backward()
        return loss.detach(), outs, tgs._grads(model)

    model = tgs._model()
    draw = ops.HardDraw(c, seed, 0)
    assert draw.k is None
    loss, outs, grads = call(model, draw)
    Zt, H = _forward_tables(model, run, x)
    k_ref, x_ref, f_ref = ops.sample_hard_negatives(Zt, H, float(model.temperature), sp, c, seed=seed, epoch=0)
    assert torch.equal(draw.k, k_ref) and torch.equal(draw.logit, x_ref) and int(draw.n_failed) == int(f_ref)
    assert not draw.k.requires_grad and not draw.logit.requires_grad
    k_plain, _f = ops.sample_negatives(sp, seed=seed, epoch=0)
    assert not torch.equal(draw.k, k_plain)
    if step != "pairs":
        assert torch.equal(outs[1], draw.logit)                    # the step's negative logits are the draw's
    # the same call with the tensor draw.k: the same bits everywhere
    hand = tgs._model()
    loss_h, outs_h, grads_h = call(hand, draw.k)
    assert torch.equal(loss, loss_h) and all(torch.equal(p, q) for p, q in zip(outs, outs_h))
    assert all(torch.equal(p, q) for p, q in zip(grads, grads_h))
    if step != "pairs":                                            # (probability space: the hardest negatives sit at p = 1, where
        assert any(float(g.abs().max()) > 0 for g in grads)        # the clamped BCE has no gradient — what logit space is for)
    order, k_rowptr = ops.sampled_order(draw.k, N)
    with pytest.raises(ValueError, match="HardDraw"):
        call(tgs._model(), ops.HardDraw(c, seed, 0), order=order, k_rowptr=k_rowptr)


# ------------------------------------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("objective,resample", [("bpr", False), ("pairs-logit", True)])
def test_end_to_end(objective, resample):
    from disenlink_amd.train import run_link_prediction
    _split, run, x = tgs._prepared(True)

    def go(**kw):
        model = tgs._model()
        res = run_link_prediction(model, x, run, epochs=3, lr=1e-3, objective=objective, resample_negatives=resample,
                                  resample_seed=9, **kw)
        return res, [p.detach().clone() for p in model.parameters()]

    hard, _p = go(hard_negatives=4)
    assert hard.epochs_run == 3 and all(np.isfinite(hard.losses)) and len(set(hard.losses)) == 3
    assert isinstance(hard.failed_draws, int) and hard.failed_draws == 0 and np.isfinite(hard.test_auc)
    assert len(hard.val_aucs) == 3 and all(np.isfinite(hard.val_aucs))
    plain, p0 = go()
    one, p1 = go(hard_negatives=1)
    zero, pz = go(hard_negatives=0)
    assert plain.losses == one.losses == zero.losses and plain.val_aucs == one.val_aucs and plain.test_auc == one.test_auc
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(p0, p1, pz))
    assert hard.losses[0] > plain.losses[0]                        # harder negatives: a larger loss on the same first forward


def test_cli_hard_negatives_prints_metrics():
    from disenlink_amd.main import main
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        main(["--dataset", "chameleon", "--synthetic", "--epochs", "3", "--run", "1", "--objective", "bpr", "--hard-negatives", "4",
              "--rank-eval", "--quiet"])
    final = [ln for ln in buf.getvalue().splitlines() if ln.startswith("final")]
    assert len(final) == 1
    toks = final[0].split()
    vals = {toks[i]: float(toks[i + 1]) for i in range(3, len(toks) - 1, 2)}
    assert set(vals) == {"mrr", "hits@1", "hits@10", "hits@50", "hits@100"}
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in vals.values())


def test_gpu_side_refusals():
    from disenlink_amd.model import Disentangle
    from disenlink_amd.train import run_link_prediction
    _split, plain_run, x = tgs._prepared(False)
    _split, run, _x = tgs._prepared(True)
    model = tgs._model()
    for kw in ({"objective": "bpr"}, {"resample_negatives": True}):
        with pytest.raises(ValueError, match="use_graph"):
            run_link_prediction(model, x, run, epochs=1, use_graph=True, hard_negatives=4, **kw)
        with pytest.raises(ValueError, match="GPU"):
            run_link_prediction(model, x.cpu(), run, epochs=1, hard_negatives=4, **kw)
        with pytest.raises(ValueError, match="prepare_run"):
            run_link_prediction(model, x, plain_run, epochs=1, hard_negatives=4, **kw)
        with pytest.raises(ValueError, match="hard_negatives"):
            run_link_prediction(model, x, run, epochs=1, hard_negatives=65, **kw)
    torch.manual_seed(0)
    bf16 = Disentangle(24, 16, 64, nfactor=8, beta=0.6, t=1, table_dtype=torch.bfloat16).to(DEV)
    with pytest.raises(TypeError, match="fp32"):
        run_link_prediction(bf16, x, run, epochs=1, objective="bpr", hard_negatives=4)
    with pytest.raises(TypeError, match="fp32"):
        run_link_prediction(bf16, x, run, epochs=1, resample_negatives=True, hard_negatives=4)
