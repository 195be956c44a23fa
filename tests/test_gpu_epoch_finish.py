"""dl_epoch_finish (epoch_finish_kernel: the AUC from the integer counts, `auc > best`, the conditional copy of the parameter
buffers into the best-weights buffers, patience, history) called directly: every bit it leaves is a copy or the outcome
of a comparison, so everything is checked with torch.equal — the copy over more float4 slots than one trip of its
grid-stride loop, from and to views that are NOT 16-byte aligned (the scalar path), with DL_ADAM_MAX_BUFS buffers and an
empty one, between guard elements; the max_epochs boundary; patience 0, a first AUC of exactly 0, denom2 = 0; and epochs
whose validation scores are NaN (DL_AUC_NAN_MARK in the counts): stale epochs that must never reach the best weights."""
import ctypes as C
import math
import struct

import numpy as np
import pytest
import torch

import auc_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_BUFS = 8                                                            # DL_ADAM_MAX_BUFS
GUARD = 8                                                               # floats on either side of a view (32 bytes)
SENTINEL = -12345.5
NAN_MARK = -(1 << 63)                                                  # DL_AUC_NAN_MARK read as int64


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from disenlink_amd import _lib
    _lib.load()


class Guarded:
    """Views of `sizes` floats, each inside an allocation of its own filled with SENTINEL, GUARD floats before and after it,
    starting `lead` floats past a 16-byte boundary."""

    def __init__(self, sizes, lead, fill):
        self.allocs, self.views = [], []
        for i, n in enumerate(sizes):
            alloc = torch.full((GUARD + lead + n + GUARD + 4,), SENTINEL, dtype=torch.float32, device=DEV)
            assert alloc.data_ptr() % 16 == 0
            view = alloc[GUARD + lead: GUARD + lead + n]
            assert view.numel() == n and view.is_contiguous() and (n == 0 or view.data_ptr() % 16 == 4 * lead)
            view.copy_(fill(i, n))
            self.allocs.append(alloc)
            self.views.append(view)
        self.lead = lead

    def guards_intact(self) -> bool:
        ok = True
        for alloc, view in zip(self.allocs, self.views):
            a = GUARD + self.lead
            ok = ok and bool((alloc[:a] == SENTINEL).all()) and bool((alloc[a + view.numel():] == SENTINEL).all())
        return ok

    def snapshot(self):
        return [a.clone() for a in self.allocs]


class Finisher:
    """The caller's side of dl_epoch_finish: state, a history between guard rows, u2, a pinned ring."""

    def __init__(self, params, best, max_epochs, patience, denom2=1000.0, ring=4):
        from disenlink_amd import _lib
        self.lib, self.check = _lib.load(), _lib.check
        self.params, self.best = params, best
        n = len(params)
        self.n = n
        self._p = (C.c_void_p * n)(*[t.data_ptr() for t in params])
        self._b = (C.c_void_p * n)(*[t.data_ptr() for t in best])
        self._numel = (C.c_size_t * n)(*[t.numel() for t in params])
        assert self.lib.dl_epoch_state_bytes() == 48
        self.state = torch.zeros(6, dtype=torch.int64, device=DEV)
        self.hist_alloc = torch.full((max(max_epochs, 1) + 4, 2), SENTINEL, dtype=torch.float64, device=DEV)
        self.hist = self.hist_alloc[2: 2 + max(max_epochs, 1)]
        self.u2 = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.loss = torch.zeros(1, dtype=torch.float32, device=DEV)
        self.ring = torch.zeros(ring, 4, dtype=torch.float64).pin_memory()
        self.max_epochs, self.patience, self.denom2, self.n_ring = max_epochs, patience, denom2, ring

    def __call__(self, loss, counts):
        """One end of an epoch with *u2 = counts (what dl_auc_pair_counts_add would have left there)."""
        self.loss.fill_(loss)
        self.u2.fill_(counts)
        self.check(self.lib.dl_epoch_finish(self.n, self._p, self._b, self._numel, self.loss.data_ptr(), self.u2.data_ptr(),
                                            self.denom2, self.state.data_ptr(), self.hist.data_ptr(), self.max_epochs,
                                            self.patience, self.ring.data_ptr(), self.n_ring,
                                            torch.cuda.current_stream().cuda_stream), "dl_epoch_finish")
        torch.cuda.synchronize()
        assert int(self.u2.item()) == 0                                 # cleared by every call, stopped or not

    def fields(self):
        """(best_auc, stale, epoch, stopped, best_epoch) and the internal counter, which must be back at 0."""
        s = self.state.cpu()
        assert int(s[5]) & 0xFFFFFFFF == 0
        return (struct.unpack("d", struct.pack("q", int(s[0])))[0], int(s[1]), int(s[2]), int(s[3]), int(s[4]))

    def hist_rows_written(self):
        h = self.hist_alloc.cpu()
        return [i - 2 for i in range(h.shape[0]) if not bool((h[i] == SENTINEL).all())]


def _fill(seed):
    def fill(i, n):
        return torch.from_numpy(np.random.default_rng(1000 * seed + i).standard_normal(n).astype(np.float32)).to(DEV)
    return fill


SIZE_SETS = {"odd-and-long": [1, 7, 0, 300003, 3],                     # 75,005 float4 slots > 64 x 256: several trips
             "max-bufs": [5, 0, 1024, 3, 4099, 1, 16, 70001]}           # DL_ADAM_MAX_BUFS buffers, 18,789 slots


@pytest.mark.parametrize("src_lead,dst_lead", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["aligned", "src+4B", "dst+4B", "both+4B"])
@pytest.mark.parametrize("sizes", sorted(SIZE_SETS))
def test_best_weights_copy_is_exact_inside_its_buffers_on_the_vector_and_the_scalar_path(sizes, src_lead, dst_lead):
    sizes = SIZE_SETS[sizes]
    assert len(sizes) <= MAX_BUFS and sum((n + 3) // 4 for n in sizes) > 64 * 256
    params, best = Guarded(sizes, src_lead, _fill(1)), Guarded(sizes, dst_lead, _fill(2))
    fin = Finisher(params.views, best.views, max_epochs=10, patience=5)
    before = best.snapshot()
    fin(0.5, 0)                                                         # AUC exactly 0.0 in the first epoch: NOT above best = 0
    assert all(torch.equal(a, b) for a, b in zip(best.allocs, before))
    assert fin.fields() == (0.0, 1, 1, 0, 0)
    fin(0.4, 600)                                                       # 0.6: improved
    assert all(torch.equal(b, p) for b, p in zip(best.views, params.views)) and best.guards_intact() and params.guards_intact()
    assert fin.fields() == (0.6, 0, 2, 0, 1)
    kept = best.snapshot()
    for p in params.views:
        p.add_(1.0)                                                     # "the step"
    params_now = params.snapshot()
    for counts in (500, 600):                                           # worse, then a tie: not improved
        fin(0.3, counts)
        assert all(torch.equal(a, b) for a, b in zip(best.allocs, kept))
    assert fin.fields() == (0.6, 2, 4, 0, 1)
    fin(0.2, 601)
    assert all(torch.equal(b, p) for b, p in zip(best.views, params.views)) and best.guards_intact()
    assert all(torch.equal(a, b) for a, b in zip(params.allocs, params_now))     # the source is only read
    assert fin.fields() == (0.601, 0, 5, 0, 4)
    want = np.array([[0.5, 0.0], [0.4, 0.6], [0.3, 0.5], [0.3, 0.6], [0.2, 0.601]])
    want[:, 0] = want[:, 0].astype(np.float32)                          # the loss is a float32
    np.testing.assert_array_equal(fin.hist[:5].cpu().numpy(), want)
    assert fin.hist_rows_written() == [0, 1, 2, 3, 4]


def test_epochs_past_max_epochs_change_nothing_but_the_counts():
    sizes = [7, 1030]
    params, best = Guarded(sizes, 0, _fill(3)), Guarded(sizes, 0, _fill(4))
    fin = Finisher(params.views, best.views, max_epochs=3, patience=100, ring=2)
    after_third = None
    for call in range(5):
        for p in params.views:
            p.add_(1.0)
        fin(1.0 / (call + 1), 100 * (call + 1))                         # AUC 0.1, 0.2, ... rising: every epoch would improve
        if call == 2:
            after_third = ([p.clone() for p in params.views], fin.ring.clone(), fin.state.clone())
        if call >= 2:
            assert fin.hist_rows_written() == [0, 1, 2]                 # exactly three rows, the guard rows untouched
            assert fin.fields() == (0.3, 0, 3, 0, 2)
            assert all(torch.equal(b, w) for b, w in zip(best.views, after_third[0]))
            assert torch.equal(fin.ring, after_third[1]) and torch.equal(fin.state, after_third[2])
    assert best.guards_intact()
    # ring of 2: slot 0 holds epoch 2 (tag 3), slot 1 epoch 1 (tag 2) — calls 4 and 5 would have landed on slots 1 and 0
    assert fin.ring[:, :3].tolist() == [[float(np.float32(1.0 / 3)), 0.3, 3.0], [0.5, 0.2, 2.0]]
    np.testing.assert_array_equal(fin.hist.cpu().numpy()[:, 1], [0.1, 0.2, 0.3])


def test_patience_zero_a_zero_denominator_and_a_marked_count():
    sizes = [9, 260]
    # patience = 0: the first epoch without improvement stops the bookkeeping; a better epoch afterwards changes nothing
    params, best = Guarded(sizes, 0, _fill(5)), Guarded(sizes, 0, _fill(6))
    fin = Finisher(params.views, best.views, max_epochs=10, patience=0)
    fin(1.0, 500)
    assert fin.fields() == (0.5, 0, 1, 0, 0)
    kept = best.snapshot()
    for p in params.views:
        p.add_(1.0)
    fin(1.0, 400)
    assert fin.fields() == (0.5, 1, 2, 1, 0)                            # stale 1 > 0: stopped
    fin(1.0, 900)
    assert fin.fields() == (0.5, 1, 2, 1, 0) and fin.hist_rows_written() == [0, 1]
    assert all(torch.equal(a, b) for a, b in zip(best.allocs, kept))
    # denom2 = 0 (a class is absent): the AUC is NaN, no epoch is ever an improvement
    params, best = Guarded(sizes, 0, _fill(7)), Guarded(sizes, 0, _fill(8))
    fin = Finisher(params.views, best.views, max_epochs=10, patience=2, denom2=0.0)
    kept = best.snapshot()
    for call, counts in enumerate((0, 5, 1 << 40)):
        fin(0.25, counts)
        assert fin.fields() == (0.0, call + 1, call + 1, int(call + 1 > 2), 0)
    h = fin.hist[:3].cpu().numpy()
    assert (h[:, 0] == 0.25).all() and np.isnan(h[:, 1]).all() and all(torch.equal(a, b) for a, b in zip(best.allocs, kept))
    # DL_AUC_NAN_MARK in the counts, with or without other bits: a NaN AUC in the history and the ring, a stale epoch
    params, best = Guarded(sizes, 1, _fill(9)), Guarded(sizes, 1, _fill(10))
    fin = Finisher(params.views, best.views, max_epochs=10, patience=1)
    fin(1.0, 300)
    kept = best.snapshot()
    for p in params.views:
        p.fill_(float("nan"))                                           # the run has diverged
    fin(float("nan"), NAN_MARK | 777)
    assert fin.fields() == (0.3, 1, 2, 0, 0) and all(torch.equal(a, b) for a, b in zip(best.allocs, kept))
    assert math.isnan(float(fin.hist[1, 0])) and math.isnan(float(fin.hist[1, 1]))
    assert math.isnan(fin.ring[1, 1].item()) and fin.ring[1, 2].item() == 2.0
    fin(float("nan"), NAN_MARK)
    assert fin.fields() == (0.3, 2, 3, 1, 0)                            # the second NaN epoch: patience 1 is over
    for p in params.views:
        p.fill_(1.0)
    fin(0.1, 999)
    assert fin.fields() == (0.3, 2, 3, 1, 0) and all(torch.equal(a, b) for a, b in zip(best.allocs, kept))


@pytest.fixture(params=["1", "0"], ids=["compiled-binding", "ctypes"])
def finish_path(request, monkeypatch):
    """DeviceEarlyStop.finish through native.epoch_finish (dl_torch.cpp) or through the two ctypes calls."""
    from disenlink_amd import native
    monkeypatch.setenv("DL_NATIVE_OPS", request.param)
    native._state["loaded"] = None                                     # re-read DL_NATIVE_OPS
    assert native.available() == (request.param == "1")
    yield request.param
    monkeypatch.undo()
    native._state["loaded"] = None


@pytest.fixture(scope="module")
def scripted_epochs():
    """Validation labels and the score vectors of six epochs — finite and rising, all NaN, one NaN, finite but worse,
    finite and better — with the AUC each epoch must record: the brute-force count's, or NaN.  Formed once."""
    rng = np.random.default_rng(23)
    n_val = 3000
    label = (rng.random(n_val) < 0.3).astype(np.float32)
    pos_idx, neg_idx = np.nonzero(label > 0.5)[0], np.nonzero(label < 0.5)[0]
    assert len(pos_idx) <= len(neg_idx)                                 # an unmarked all-NaN epoch would read as AUC 1.0
    noise = np.round(rng.standard_normal(n_val), 1).astype(np.float32)
    finite = lambda q: (np.float32(q) * (label * 2 - 1) + noise).astype(np.float32)
    one_nan = finite(0.9)
    one_nan[pos_idx[5]] = np.nan
    scores = [finite(0.1), finite(0.3), np.full(n_val, np.nan, np.float32), one_nan, finite(0.2), finite(0.5)]
    aucs = [float("nan") if np.isnan(s).any() else auc_ref.auc(s, pos_idx, neg_idx) for s in scores]
    assert aucs[0] < aucs[4] < aucs[1] < aucs[5] < 1.0 and math.isnan(aucs[2]) and math.isnan(aucs[3])
    return label, scores, aucs


@pytest.mark.parametrize("patience", [5, 1])
def test_epochs_with_nan_validation_scores_are_stale_epochs(patience, finish_path, scripted_epochs):
    """DeviceEarlyStop over a run that diverges for two epochs and comes back: the loop of main_disentangled.py:199-214
    restated on the host with `nan > best` false.  The history and read() show NaN for the two NaN epochs, the best AUC is
    never NaN, the best weights are those after the last FINITE improvement (the NaN epochs' weights are NaN: they must not
    be kept), and with patience 1 the second NaN epoch stops the run.  An AUC of 1.0 for the all-NaN epoch — what the
    counts gave before they carried DL_AUC_NAN_MARK — fails every one of these."""
    from disenlink_amd.early_stop import DeviceEarlyStop
    from disenlink_amd.metrics import AucPlan
    from disenlink_amd.model import Disentangle
    label, scores, aucs = scripted_epochs
    torch.manual_seed(3)
    model = Disentangle(7, 5, 8, nfactor=3, beta=0.5, t=1).to(DEV)
    plan = AucPlan(torch.from_numpy(label).to(DEV))
    es = DeviceEarlyStop(model, plan, len(scores), patience)
    assert es._native == (finish_path == "1")
    bufs = list(model._stacked.values())
    best_auc, stale, best_epoch, stopped_at = 0.0, 0, 0, None
    want_weights = [b.clone() for b in bufs]
    for e, (score, auc) in enumerate(zip(scores, aucs)):
        bad = math.isnan(auc)
        with torch.no_grad():
            for b in bufs:                                              # "the step": a diverged epoch leaves NaN weights
                b.fill_(float("nan") if bad else float(e + 1))
        loss = torch.tensor(float("nan") if bad else 1.0 / (e + 1), dtype=torch.float32, device=DEV)
        es.finish(loss, torch.from_numpy(score).to(DEV))
        es.post(e)
        torch.cuda.synchronize()
        assert int(es.u2.item()) == 0                                   # the mark does not leak into the next epoch
        if stopped_at is not None:
            continue
        got_loss, got_auc = es.read(e)
        print(e, "device", got_auc, "reference", auc)
        assert (math.isnan(got_auc) and math.isnan(got_loss)) if bad else (got_auc == auc and got_loss == float(loss)), (e, got_auc, auc)
        if auc > best_auc:                                              # false for NaN
            best_auc, stale, best_epoch, want_weights = auc, 0, e, [b.clone() for b in bufs]
        else:
            stale += 1
        if stale > patience:
            stopped_at = e
    assert stopped_at == {5: None, 1: 3}[patience] and best_epoch == {5: 5, 1: 1}[patience]
    recorded = len(scores) if stopped_at is None else stopped_at + 1
    hist = es.hist.cpu().numpy()
    np.testing.assert_array_equal(hist[:recorded, 1], np.array(aucs[:recorded]))       # NaN == NaN here
    assert np.isnan(hist[2:4]).all() and np.count_nonzero(hist[recorded:]) == 0
    st = es.state.cpu()
    got_best = st[:1].view(torch.float64).item()
    assert got_best == best_auc and not math.isnan(got_best)
    assert (int(st[1]), int(st[2]), int(st[3]), int(st[4])) == (stale, recorded, int(stopped_at is not None), best_epoch)
    for b, w in zip(es.best, want_weights):
        assert torch.equal(b, w) and bool(torch.isfinite(b).all())
    es.restore()
    for b, w in zip(bufs, want_weights):
        assert torch.equal(b, w) and bool(torch.isfinite(b).all())


@pytest.fixture(scope="module")
def texas_run():
    import json
    import os
    from conftest import GOLDEN_DIR
    from disenlink_amd.datasets import standardise_rows
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run
    g = np.load(os.path.join(GOLDEN_DIR, "real_texas.npz"))
    m = json.loads(str(g["meta"]))
    edges = g["edges"].astype(np.int64)
    feats = np.zeros(tuple(g["feat_shape"]), dtype=np.float32)
    feats[g["feat_row"].astype(np.int64), g["feat_col"].astype(np.int64)] = 1.0
    x = torch.from_numpy(standardise_rows(feats) if "standardise" in g else feats).to(DEV)
    split = make_link_split(edges[:, 0], edges[:, 1], feats.shape[0], m=m["m"], seed=m["split_seed"])
    return m, x, prepare_run(split, torch.device(DEV), row_bytes=m["K"] * m["d"] * 4)


@pytest.mark.parametrize("device_early_stop", ["1", "0"], ids=["device-early-stop", "eager-host"])
def test_a_run_that_diverges_keeps_its_last_finite_best(device_early_stop, texas_run, monkeypatch):
    """run_link_prediction on texas (183 nodes, K = 5) at ten times the reference's step size: on the CPU oracle path
    (OraclePairModule, torch Adam) lr = 1e-3 saturates every probability after one step (loss 20, zero gradients) and
    Adam's momentum carries the weights to an overflow — every probability NaN from epoch 4 on.  The run must report a
    finite best validation AUC below 1, the largest finite entry of its history, NaN validation AUCs from the diverged
    epoch on, and give back finite weights; with an AUC of 1.0 for NaN scores it reported 1.0 and kept NaN weights."""
    from disenlink_amd.model import Disentangle
    from disenlink_amd.train import run_link_prediction
    m, x, run = texas_run
    monkeypatch.setenv("DL_DEVICE_EARLY_STOP", device_early_stop)
    torch.manual_seed(m["seed"])
    model = Disentangle(x.shape[1], m["nhid"], m["d"], nfactor=m["K"], beta=m["beta"], t=m["t"]).to(DEV)
    res = run_link_prediction(model, x, run, epochs=12, lr=1e-3, patience=200, use_graph=False)
    aucs = np.array(res.val_aucs)
    print(device_early_stop, "val_aucs", res.val_aucs, "losses", res.losses, "best", res.best_val_auc, "test", res.test_auc)
    assert res.epochs_run == 12 and np.isnan(aucs).any() and not np.isnan(aucs[0])
    first = int(np.argmax(np.isnan(aucs)))
    assert np.isnan(aucs[first:]).all() and not np.isnan(aucs[:first]).any()        # NaN from the diverged epoch on
    assert math.isfinite(res.best_val_auc) and res.best_val_auc < 1.0 and res.best_val_auc == np.nanmax(aucs)
    assert all(bool(torch.isfinite(v).all()) for v in model.state_dict().values())  # the restored weights
    assert math.isfinite(res.test_auc) and 0.0 <= res.test_auc <= 1.0
