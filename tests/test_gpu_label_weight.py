"""The training scorers and the loss kernels on soft labels and on signed, zero and wide weights (dl_score_pairs_train,
dl_score_pairs_train_logits, dl_pair_bce, dl_pair_bce_logits, the per-entry stream of PairList.bind_labels) against the fp64
reference of tests/label_weight_ref.py, on the graph and the pair list of ref64.structure(): 322 nodes, adjacency rows of 0 .. 290
entries, incidence rows of 0 .. 300 pairs.

What the library promises and these tests hold it to (include/disenlink_hip.h, dl_score_pairs_train): w is any real weight and
the gradient is that of sum w BCE; every pair of the plan has its score written, whatever its weight; weights of +-0.0 contribute
exactly nothing; a captured step reads the labels of replay time.

Bounds: label_weight_ref.BOUND = 4 x the error of the fp32 restatements against fp64, measured on these cases and measured again
on every run by tests/test_label_weight_cpu.py; scores in the bands of tests/test_gpu_hotpath_fp64.py.  None was set from what the
kernels give; every figure is printed as a FIGURE line before anything is asserted (pytest -s).

For the record, the largest figure of each kind in one run on an MI355X (no bound was taken from it):

    figure                                  probability space: kernels / bound     logit space: kernels / bound
    score (prob: of its band; logit: 2^-24 companion)   0.244 / 1   K3 d8 t1       1.57 / 10.16      K3 d8 t1
    one-pass dZ   [row ratio, |w| scales]   4.74e-06 / 1.72e-05  K5 d32 t1 (half, wide)   3.49e-06 / 4.48e-06  K5 d32 t1 (half, wide)
    one-pass dH                             4.72e-06 / 2.26e-05  the same case            3.55e-06 / 4.72e-06  the same case
    separate path dZ  (soft, signed)        1.57e-06 / 1.72e-05  K16 d128 t2              9.50e-07 / 4.48e-06  K5 d32 t2
    separate path dH                        6.82e-07 / 2.26e-05  K5 d32 t2                1.07e-06 / 4.72e-06  K5 d32 t2
    loss  [of sum |w| |term|]               1.05e-07 / 3.99e-07  K8 d64 t1 (half, wide)   1.12e-07 / 4.04e-07  K8 d64 t2
    g     [g_ratio]                         2.33e-07 / 9.32e-07  bf16 K5 d64 t1           9.59e-03 / 1.04e-01  bf16 K4 d32 t2 (soft, signed)
    loss kernel alone: loss                 8.55e-08 / 2.32e-07  1 pair                   8.49e-08 / 3.15e-07  1,025 pairs
    loss kernel alone: g                    1.80e-07 / 7.20e-07  1,024 pairs              1.66e-05 / 1.80e-04  10,004 pairs

Before the fixes that came with this file (the sign of a caller's weight read as the stream's writer flag; a captured step
replaying the per-entry copy of its warm-up labels) the first, second and fifth test below and the two cases added to
tests/test_gpu_parity.py failed: unwritten scores under `signed` and `negzero`, dZ / dH row ratios of 2.2 under `signed` (the
gradient of sum |w| BCE), stale labels in the replay.  The loss kernels alone and the non-finite weight test passed before, too.
"""
import pytest
import torch

import label_weight_ref as lw
import logit_ref
import ref64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = ref64.U
SOFT_SIGNED = ("soft", "signed")


def _lib():
    from disenlink_amd import _lib
    return _lib.load()


def _b1_cases():
    return lw.b1_cases(_lib())


def _b2_cases():
    return [c for c in logit_ref.cases(_lib()) if not c.generic]          # the generic shape has no one-pass scorer


_device = {}


def _device_structure():
    if not _device:
        from disenlink_amd.graph import PairList
        st = ref64.structure()
        G = st.graph.to(DEV)
        pairs = PairList.build(st.pu.to(DEV), st.pv.to(DEV), ref64.N_NODES)
        for mine, theirs in ((pairs.by_u, st.pairs.by_u), (pairs.inc, st.pairs.inc)):
            assert torch.equal(mine.rowptr.cpu(), theirs.rowptr) and torch.equal(mine.col.cpu(), theirs.col)
        _device["v"] = (st, G, pairs)
    return _device["v"]


def _fresh_pairs():
    from disenlink_amd.graph import PairList
    st = ref64.structure()
    return PairList.build(st.pu.to(DEV), st.pv.to(DEV), ref64.N_NODES)


class _Figures:
    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def note(self, what, observed, bound):
        self.rows.append((what, float(observed), float(bound)))

    def exact(self, what, ok):
        self.rows.append((what, 0.0 if ok else float("inf"), 0.0))

    def check(self):
        for what, observed, bound in self.rows:
            print(f"FIGURE {self.tag} | {what} | {observed:.4g} | {bound:.4g}")
        bad = [f for f in self.rows if not f[1] <= f[2]]                      # (a NaN is not <= anything)
        assert not bad, bad


def _tables(r, dtype):
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    Zt, H = r["Z"].to(tdt).to(DEV), r["H_in"].to(tdt).to(DEV)
    assert torch.equal(Zt.double().cpu(), r["Z"]) and torch.equal(H.double().cpu(), r["H_in"])
    return Zt, H


def _train(space, Zt, H, pairs, t, label, weight):
    """One call of the one-pass scorer of `space` -> (score, dZ, dH)."""
    from disenlink_amd import ops
    fn = ops.score_pairs_train if space == "prob" else ops.score_pairs_train_logits
    return fn(Zt, H, pairs, t, label, weight)


def _loss(space, score, label, weight):
    from disenlink_amd import ops
    return (ops.pair_bce if space == "prob" else ops.pair_bce_logits)(score, label, weight)


def _separate(space, Zt, H, pairs, t, label, weight):
    """The separate-kernel path: forward, loss kernel, backward -> (score, dZ, dH)."""
    from disenlink_amd import ops
    if space == "prob":
        prob = ops.score_pairs_fwd(Zt, H, pairs.pu, pairs.pv, t, pairs)
        _l, g = ops.pair_bce(prob, label, weight)
        return (prob,) + tuple(ops.score_pairs_bwd(Zt, H, pairs, t, prob, g))
    x = ops.score_pairs_logits_fwd(Zt, H, pairs.pu, pairs.pv, t, pairs)
    _l, g = ops.pair_bce_logits(x, label, weight)
    return (x,) + tuple(ops.score_pairs_logits_bwd(Zt, H, pairs, t, g))


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _score_figures(fig, tag, space, r, score):
    """(a): every score of the list is written (DL_POISON=1: an unwritten one is a NaN) and lies in its band."""
    fig.exact(f"{tag} every score written", bool(torch.isfinite(score).all()))
    if space == "prob":
        band = ref64.prob_band(r["x"], ref64.BOUND["logit"] * U * r["x_abs"], ref64.BOUND["prob_eps"] * U)
        fig.note(f"{tag} prob / band", float(((score.double().cpu() - torch.sigmoid(r["x"])).abs() / band).max()), 1.0)
    else:
        fig.note(f"{tag} logit", ref64.band_ratio(score.cpu(), r["x"], r["x_abs"]), ref64.BOUND["logit"])


def _step_figures(fig, tag, space, r, score, dZ, dH, loss=None, g=None):
    """(b): dZ, dH (and the loss kernel's loss and g on the scores it was handed) within label_weight_ref.BOUND."""
    have = loss is not None
    got = lw.step_figures(r, space, dZ.cpu(), dH.cpu(), score.cpu() if have else None, loss.cpu() if have else None,
                          g.cpu() if have else None)
    for k, v in got.items():
        fig.note(f"{tag} {k}", v, lw.BOUND[space][k])


def _id(v):
    return logit_ref.case_id(v) if isinstance(v, logit_ref.Case) else str(v)


# ------------------------------------------------------------------------------------------------------------------ B1
@pytest.mark.parametrize("space", lw.SPACES)
@pytest.mark.parametrize("case", _b1_cases(), ids=_id)
def test_every_combination_against_fp64_on_one_shape_per_kernel_family(case, space, monkeypatch):
    """One shape per kernel family and table type, t = 1 and 2, the four combinations, three calls each — the gathers
    (DL_ENTRY_LABELS=0), the first sight of the tensors, the second sight (the stream is bound there unless the weights hold a sign
    bit, which keep the gathers: PairList.bind_labels) — (a) every score written and in its band, (b) dZ, dH, loss and g within
    bounds, (c) the three calls give the same bits, (d) weights of -0.0 give the bits of +0.0, (e) under signed weights the
    separate-kernel path lies within the bounds of the same fp64 reference."""
    from disenlink_amd import ops
    assert ops._POISON, "the tests run with DL_POISON=1 (conftest.py)"
    K, d, dtype, t, beta, _generic = case
    st, G, pairs = _device_structure()
    fig = _Figures(f"{logit_ref.case_id(case)} {space}")
    runs = {}
    try:
        for combo in lw.COMBOS + (("binary", "positive"),):
            r = lw.reference(K, d, dtype, t, beta, combo)
            Zt, H = _tables(r, dtype)
            label, weight = r["y"].to(DEV), r["w"].to(DEV)
            tag = lw.combo_id(combo)
            monkeypatch.setenv("DL_ENTRY_LABELS", "0")
            off = _train(space, Zt, H, pairs, t, label, weight)
            monkeypatch.setenv("DL_ENTRY_LABELS", "1")
            first = _train(space, Zt, H, pairs, t, label, weight)
            unbound_at_first = pairs._yw is None
            second = _train(space, Zt, H, pairs, t, label, weight)
            fig.exact(f"{tag} stream bound at the second sight exactly where no weight holds a sign bit",
                      unbound_at_first and (pairs._yw is not None) == (not bool(torch.signbit(r["w"]).any())))
            for name, out in (("gathers", off), ("first sight", first), ("second sight", second)):
                _score_figures(fig, f"{tag} ({name})", space, r, out[0])
            fig.exact(f"{tag} the three calls give the same bits", _same_bits(off, first) and _same_bits(off, second))
            loss, g = _loss(space, second[0], label, weight)
            _step_figures(fig, tag, space, r, second[0], second[1], second[2], loss, g)
            runs[combo] = second
            if combo == SOFT_SIGNED:
                sep = _separate(space, Zt, H, pairs, t, label, weight)
                _score_figures(fig, f"{tag} (separate path)", space, r, sep[0])
                _step_figures(fig, f"{tag} (separate path)", space, r, sep[0], sep[1], sep[2])
            pairs.unbind_labels()
        fig.exact("negzero == positive, bit for bit (score, dZ, dH)", _same_bits(runs[("binary", "negzero")], runs[("binary", "positive")]))
    finally:
        pairs.unbind_labels()
    fig.check()


# ------------------------------------------------------------------------------------------------------------------ B2
@pytest.mark.parametrize("space", lw.SPACES)
@pytest.mark.parametrize("case", _b2_cases(), ids=_id)
def test_soft_labels_and_signed_weights_on_every_tuned_shape(case, space):
    """(soft, signed) on every shape the library reports a tuned kernel for, both table types, t = 1 and 2: (a) and (b)."""
    from disenlink_amd import _lib
    K, d, dtype, t, beta, _generic = case
    st, G, pairs = _device_structure()
    code = _lib.DL_F32 if dtype == "f32" else _lib.DL_BF16
    assert _lib.load().dl_has_fast_path_dtype(K, d, code)
    r = lw.reference(K, d, dtype, t, beta, SOFT_SIGNED)
    Zt, H = _tables(r, dtype)
    label, weight = r["y"].to(DEV), r["w"].to(DEV)
    fig = _Figures(f"{logit_ref.case_id(case)} {space}")
    try:
        score, dZ, dH = _train(space, Zt, H, pairs, t, label, weight)
        loss, g = _loss(space, score, label, weight)
    finally:
        pairs.unbind_labels()
    _score_figures(fig, "soft-signed", space, r, score)
    _step_figures(fig, "soft-signed", space, r, score, dZ, dH, loss, g)
    fig.check()


# ------------------------------------------------------------------------------------------------------------------ B3
@pytest.mark.parametrize("space", lw.SPACES)
@pytest.mark.parametrize("n", logit_ref.BCE_SIZES)
def test_loss_kernels_alone(n, space):
    """dl_pair_bce / dl_pair_bce_logits around their 1,024 partial sums, on the four combinations (probability space: the fp32
    sigmoids of the logits, exact 0 and exact 1 among them): loss and g against fp64 at the scores handed in; g is exactly 0
    wherever the weight is +-0.0; y = 0.5 at x = 0 gives g == 0 exactly in logit space."""
    fig = _Figures(f"n={n} {space}")
    for combo in lw.COMBOS:
        s, y, w = lw.loss_kernel_inputs(space, n, combo)
        loss, g = _loss(space, s.to(DEV), y.to(DEV), w.to(DEV))
        got = lw.loss_kernel_figures(space, s, y, w, loss.cpu(), g.cpu())
        for k, v in got.items():
            fig.note(f"{lw.combo_id(combo)} {k}", v, lw.BOUND[space + "_kernel"][k])
        dead = (w == 0).to(DEV)
        fig.exact(f"{lw.combo_id(combo)} g is +0.0 wherever w is +-0.0, finite everywhere",
                  bool((g.view(torch.int32)[dead] == 0).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(loss)))
    if space == "logit":
        _x, y, w = lw.loss_kernel_inputs(space, n, ("half", "wide"))
        _loss0, g = _loss(space, torch.zeros(n, device=DEV), y.to(DEV), w.to(DEV))
        fig.exact("y = 0.5 at x = 0: g == 0 exactly", bool((g == 0).all()))
    fig.check()


# ------------------------------------------------------------------------------------------------------------------ B4
def _quiet_pair(st):
    """The first pair of the list that is no self pair, whose endpoints both have at least 2 pairs, neither of them among the
    three nodes with the most pairs — judged on the list alone."""
    cnt = torch.bincount(torch.cat([st.pu, st.pv]).long(), minlength=ref64.N_NODES)
    top3 = torch.topk(cnt, 3).indices
    ok = (st.pu != st.pv) & (cnt[st.pu.long()] >= 2) & (cnt[st.pv.long()] >= 2) & ~torch.isin(st.pu, top3) & ~torch.isin(st.pv, top3)
    return int(torch.nonzero(ok)[0])


@pytest.mark.parametrize("space", lw.SPACES)
@pytest.mark.parametrize("shape", [(8, 64), (5, 32)], ids=lambda s: f"K{s[0]}-d{s[1]}")
def test_a_non_finite_weight_stays_visible_and_local(shape, space):
    """One pair's weight is NaN, then +inf (fp32 tables; the wave-per-entry and the group-per-entry kernel): its score is written
    and finite, the loss is NaN / not finite, every element of the two endpoints' rows of dZ and dH is not finite, and every other
    row has the bits of the run with that weight 0."""
    K, d = shape
    case = next(c for c in _b1_cases() if (c.K, c.d, c.dtype, c.t) == (K, d, "f32", 1.0))
    st, G, pairs = _device_structure()
    r = lw.reference(K, d, "f32", case.t, case.beta, ("smoothed", "positive"))
    Zt, H = _tables(r, "f32")
    q0 = _quiet_pair(st)
    u, v = int(st.pu[q0]), int(st.pv[q0])
    others = torch.ones(ref64.N_NODES, dtype=torch.bool)
    others[[u, v]] = False
    others = others.to(DEV)
    label = r["y"].to(DEV)
    out = {}
    try:
        for name, value in (("zero", 0.0), ("nan", float("nan")), ("inf", float("inf"))):
            w = r["w"].clone()
            w[q0] = value
            weight = w.to(DEV)
            score, dZ, dH = _train(space, Zt, H, pairs, case.t, label, weight)
            score2, dZ2, dH2 = _train(space, Zt, H, pairs, case.t, label, weight)      # the second sight: the stream, where it binds
            assert _same_bits((score, dZ, dH), (score2, dZ2, dH2)), name
            loss, _g = _loss(space, score, label, weight)
            out[name] = (score, dZ, dH, loss)
            pairs.unbind_labels()
    finally:
        pairs.unbind_labels()
    zs, zdZ, zdH, zloss = out["zero"]
    assert bool(torch.isfinite(zs).all()) and bool(torch.isfinite(zdZ).all()) and bool(torch.isfinite(zdH).all()) and bool(torch.isfinite(zloss))
    for name in ("nan", "inf"):
        score, dZ, dH, loss = out[name]
        assert bool(torch.isfinite(score).all()) and torch.equal(score, zs), name          # written, finite, the same scores
        assert bool(torch.isnan(loss)) if name == "nan" else not bool(torch.isfinite(loss)), (name, float(loss))
        for node in (u, v):
            assert not bool(torch.isfinite(dZ[node]).any()) and not bool(torch.isfinite(dH[node]).any()), (name, node)
        assert torch.equal(dZ[others], zdZ[others]) and torch.equal(dH[others], zdH[others]), name


# ------------------------------------------------------------------------------------------------------------------ B5
@pytest.mark.parametrize("space", lw.SPACES)
def test_a_replayed_step_reads_the_labels_of_replay_time(space):
    """(8, 64) fp32: two eager warm-up calls on a side stream (which would bind the per-entry stream), one captured call, a replay;
    then label.copy_() / weight.copy_() with another combination and another replay: both replays give the bits of an eager call
    on a fresh PairList with the values the tensors held at replay time.  One stream, no parallel branches."""
    case = next(c for c in _b1_cases() if (c.K, c.d, c.dtype, c.t) == (8, 64, "f32", 1.0))
    K, d, dtype, t, beta, _generic = case
    r1 = lw.reference(K, d, dtype, t, beta, ("smoothed", "positive"))
    r2 = lw.reference(K, d, dtype, t, beta, SOFT_SIGNED)
    Zt, H = _tables(r1, dtype)
    pairs = _fresh_pairs()
    label, weight = r1["y"].to(DEV), r1["w"].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _train(space, Zt, H, pairs, t, label, weight)
    torch.cuda.current_stream().wait_stream(side)
    assert pairs._yw is not None and not getattr(pairs, "static_labels", False)     # the warm-up did bind; nothing was declared static
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _train(space, Zt, H, pairs, t, label, weight)
    for y, w in ((r1["y"], r1["w"]), (r2["y"], r2["w"])):
        label.copy_(y.to(DEV))
        weight.copy_(w.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = tuple(x.clone() for x in out)
        want = _train(space, Zt, H, _fresh_pairs(), t, y.to(DEV), w.to(DEV))
        for a, b, what in zip(got, want, ("score", "dZ", "dH")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, int((a != b).sum()))
    del graph
