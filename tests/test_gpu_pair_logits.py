"""The pair-list objective in LOGIT space on the GPU (include/disenlink_hip.h: dl_score_pairs_logits_fwd / _bwd,
dl_score_pairs_train_logits, dl_pair_bce_logits; ops.HotPathPairLogits / HotPathPairLogitsLoss / PairBCELogits; the compiled
operator; run_link_prediction(objective="pairs-logit")) against the fp64 reference of tests/logit_ref.py on the graph and the pair
list of ref64.structure(): 322 nodes, adjacency rows of 0 .. 290 entries, incidence rows of 0 .. 300 pairs.

Bounds.  Forward logits: ref64.BOUND["logit"] * 2^-24 * the absolute-sum companion, per pair (the existing band).  Gradients:
ref64.row_ratio within logit_ref.BOUND = 4 x the error of the fp32 restatement `logit_ref.step32` against fp64, measured on
these cases and measured again on every run by tests/test_pair_logits_cpu.py.  Loss values and the loss kernel's gradient:
relative, 4 x the restatement's.  None was set from what the kernels give; every figure is printed as a FIGURE line before
anything is asserted (pytest -s).

test_saturated_pairs_keep_their_gradient_and_their_order fails without the feature, and is why it exists.
"""
import numpy as np
import pytest
import torch

import logit_ref
import ref64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = ref64.U
B = logit_ref.BOUND


def _cases():
    from disenlink_amd import _lib
    return logit_ref.cases(_lib.load())


_device = {}


def _device_structure():
    """ref64.structure() on the device (built once), and the same pair list with a forced hub plan / without hub rows."""
    if not _device:
        from disenlink_amd.graph import PairList
        st = ref64.structure()
        G = st.graph.to(DEV)
        tu, tv = st.pu.to(DEV), st.pv.to(DEV)
        pairs = PairList.build(tu, tv, ref64.N_NODES)
        for mine, theirs in ((pairs.by_u, st.pairs.by_u), (pairs.inc, st.pairs.inc)):
            assert torch.equal(mine.rowptr.cpu(), theirs.rowptr) and torch.equal(mine.col.cpu(), theirs.col)
        _device["v"] = (st, G, pairs)
    return _device["v"]


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


dev32 = lambda x: x.float().to(DEV)


def _quiet_nodes(st):
    """Three ladder nodes (first endpoint of 1, 64 and 300 pairs) and the mask of the pairs that touch them."""
    nodes = torch.tensor([int(st.pair_ladder[i]) for i in (1, 3, 8)])
    assert [int(((st.pu == n) | (st.pv == n)).sum()) for n in nodes] == [1, 64, 300]
    return nodes, torch.isin(st.pu, nodes) | torch.isin(st.pv, nodes)


@pytest.mark.parametrize("case", _cases(), ids=logit_ref.case_id)
def test_logit_kernels_match_fp64(case):
    """1. forward logits in the band, 2. the bit contracts of the raw entries, 3. one-pass gradients and the separate backward
    against fp64 — for every tuned shape in both table types and the generic shape, at t = 1 and t = 2."""
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    K, d, dtype, t, beta, generic = case
    st, G, pairs = _device_structure()
    r = logit_ref.reference(K, d, dtype, t, beta)
    tdt, code = (torch.float32, _lib.DL_F32) if dtype == "f32" else (torch.bfloat16, _lib.DL_BF16)
    fig = _Figures(logit_ref.case_id(case))
    Zt, H_in = r["Z"].to(tdt).to(DEV), r["H_in"].to(tdt).to(DEV)
    assert torch.equal(Zt.double().cpu(), r["Z"]) and torch.equal(H_in.double().cpu(), r["H_in"])   # bf16: the rounded tables
    label, weight = dev32(r["label"]), dev32(r["weight"])
    dup = torch.from_numpy(st.dup_pairs).to(DEV)
    old = lib.dl_set_force_generic(1 if generic else 0)
    try:
        assert bool(lib.dl_has_fast_path_dtype(K, d, code)) != ((K, d) == logit_ref.GENERIC_SHAPE)
        # 1. forward logits: with the plan, without it
        fwd = None
        for form in ("plan", "no plan"):
            if form == "no plan" and dtype == "bf16":              # no per-pair bf16 kernel: refused, as for probabilities
                with pytest.raises(_lib.DisenlinkHipError, match="no generic bf16 path"):
                    ops.score_pairs_logits_fwd(Zt, H_in, pairs.pu, pairs.pv, t, None)
                continue
            x = ops.score_pairs_logits_fwd(Zt, H_in, pairs.pu, pairs.pv, t, pairs if form == "plan" else None)
            fig.note(f"logits fwd ({form})", ref64.band_ratio(x.cpu(), r["x"], r["x_abs"]), ref64.BOUND["logit"])
            fig.exact(f"logits fwd ({form}) duplicate pairs give identical bits", torch.equal(x[dup[:, 0]], x[dup[:, 1]]))
            fig.exact(f"logits fwd ({form}) bitwise repeatable",
                      torch.equal(x, ops.score_pairs_logits_fwd(Zt, H_in, pairs.pu, pairs.pv, t, pairs if form == "plan" else None)))
            fwd = x if form == "plan" else fwd
        # 3. one-pass gradients
        supported = ops.score_pairs_train_logits_supported(pairs, K, d, code)
        fig.exact("one-pass logit scorer is there exactly where the probability one is",
                  supported == ops.score_pairs_train_supported(pairs, K, d, code) == (not generic))
        if supported:
            x, dZ, dH = ops.score_pairs_train_logits(Zt, H_in, pairs, t, label, weight)
            fig.note("train logits", ref64.band_ratio(x.cpu(), r["x"], r["x_abs"]), ref64.BOUND["logit"])
            fig.note("train dZ", ref64.row_ratio(dZ.cpu(), r["dZ"]), B["dZ"])
            fig.note("train dH", ref64.row_ratio(dH.cpu(), r["dH"]), B["dH"])
            if dtype == "f32" and (K, d) in ((4, 64), (8, 64)):
                fig.exact("train logits == forward logits, bit for bit", torch.equal(x, fwd))
            quiet, theirs = _quiet_nodes(st)              # weight 0 on every pair of three nodes: their rows are exactly 0
            w0 = weight.clone()
            w0[theirs.to(DEV)] = 0.0
            _xq, dZq, dHq = ops.score_pairs_train_logits(Zt, H_in, pairs, t, label, w0)
            fig.exact("rows touched only by weight-0 pairs are exactly 0",
                      bool((dZq[quiet.to(DEV)] == 0).all()) and bool((dHq[quiet.to(DEV)] == 0).all()) and float(dZq.abs().max()) > 0)
            for _again in range(2):                     # the second sight of the same tensors binds per-entry labels (graph.py)
                x2, dZ2, dH2 = ops.score_pairs_train_logits(Zt, H_in, pairs, t, label, weight)
                fig.exact("train bitwise repeatable", torch.equal(x, x2) and torch.equal(dZ, dZ2) and torch.equal(dH, dH2))
            pairs.unbind_labels()
        # the separate backward from the reference's d loss / d logit (fp32)
        g = dev32(r["g"])
        dZ, dH = ops.score_pairs_logits_bwd(Zt, H_in, pairs, t, g)
        g64 = g.double().cpu()
        Zr, Hr = r["Z"].clone().requires_grad_(True), r["H_in"].clone().requires_grad_(True)
        dZ_ref, dH_ref = torch.autograd.grad(ref64.logit64(Zr, Hr, st.pu, st.pv, t), (Zr, Hr), g64)
        fig.note("logits bwd dZ", ref64.row_ratio(dZ.cpu(), dZ_ref), B["dZ"])
        fig.note("logits bwd dH", ref64.row_ratio(dH.cpu(), dH_ref), B["dH"])
        dZ2, dH2 = ops.score_pairs_logits_bwd(Zt, H_in, pairs, t, g)
        fig.exact("logits bwd bitwise repeatable", torch.equal(dZ, dZ2) and torch.equal(dH, dH2))
    finally:
        lib.dl_set_force_generic(old)
    fig.check()


@pytest.mark.parametrize("case", _cases(), ids=logit_ref.case_id)
def test_separate_path_agrees_with_the_one_pass_node(case):
    """4. HotPathPairLogits + PairBCELogits against HotPathPairLogitsLoss from the same Z (both route and aggregate with the same
    kernels: the same H bits): the loss within the loss bound, the parameter-side dZ within the row-ratio bound — the summation
    orders differ, so not bits.  The generic shape has the separate path only: there it is held against fp64 through the
    reference's own H instead (test_logit_kernels_match_fp64), and here only runs end to end."""
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    K, d, dtype, t, beta, generic = case
    st, G, pairs = _device_structure()
    r = logit_ref.reference(K, d, dtype, t, beta)
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    label, weight = dev32(r["label"]), dev32(r["weight"])
    fig = _Figures(logit_ref.case_id(case))
    old = lib.dl_set_force_generic(1 if generic else 0)
    try:
        out = {}
        for path in ("separate",) if generic else ("separate", "one pass"):
            Z = dev32(r["Z"]).requires_grad_(True)
            if path == "separate":
                emb, x = ops.HotPathPairLogits.apply(Z, G, pairs, beta, t, tdt)
                loss = ops.PairBCELogits.apply(x, label, weight)
            else:
                emb, x, loss = ops.HotPathPairLogitsLoss.apply(Z, G, pairs, beta, t, tdt, label, weight)
            loss.backward()
            out[path] = (emb.detach(), x.detach(), loss.detach(), Z.grad.clone())
        pairs.unbind_labels()
        emb, x, loss, dZ = out["separate"]
        fig.exact("finite", all(bool(torch.isfinite(v).all()) for v in out["separate"]))
        if not generic:
            emb1, x1, loss1, dZ1 = out["one pass"]
            fig.exact("emb bits", torch.equal(emb, emb1))
            fig.note("loss, separate against one pass", logit_ref.rel_err(loss, loss1), B["loss"])
            fig.note("dZ, separate against one pass", ref64.row_ratio(dZ.cpu(), dZ1.double().cpu()), B["dZ"])
            if dtype == "f32" and (K, d) in ((4, 64), (8, 64)):
                fig.exact("logit and loss bits where forward and training logits are the same bits",
                          torch.equal(x, x1) and torch.equal(loss, loss1))
    finally:
        lib.dl_set_force_generic(old)
    fig.check()


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("t", [1.0, 2.0])
def test_forward_logit_bit_contracts(K, t):
    """2. fp32 tables, d = 64: the hub plan, its residual plan and the plain plan give the same bits; a folded mirrored pair stores
    the same bits under both ids; the training logits are the forward logits; two calls give the same bits."""
    from disenlink_amd import ops
    from disenlink_amd.graph import PairList
    st, G, _pairs = _device_structure()
    r = logit_ref.reference(K, 64, "f32", t, ref64.BETAS[0])
    Z, H = dev32(r["Z"]), dev32(r["H_in"])
    # the structure's list plus the mirror of every third pair: (v, u) listed as well as (u, v)
    pu = torch.cat([st.pu, st.pv[::3]]).to(DEV)
    pv = torch.cat([st.pv, st.pu[::3]]).to(DEV)
    n0 = st.pu.numel()
    plain = PairList.build(pu, pv, ref64.N_NODES, hub_rows=0, fold_mirrors=False)
    folded = PairList.build(pu, pv, ref64.N_NODES, hub_rows=0)
    hub = PairList.build(pu, pv, ref64.N_NODES, hub_rows=32)
    assert plain.fwd is None and plain.hub is None and folded.fwd is not None and folded.hub is None
    assert hub.hub is not None and hub.hub.n_items > 0 and hub.hub.rest is not None and hub.hub.rest.n_entries > 0
    assert int((hub.hub.step_q2 >= 0).sum()) > 0 and int((hub.hub.rest_pair2 >= 0).sum()) > 0         # folded mirrors in both parts
    score = lambda pl: ops.score_pairs_logits_fwd(Z, H, pl.pu, pl.pv, t, pl)
    ref = score(plain)
    for name, pl in (("folded", folded), ("hub", hub)):
        got = score(pl)
        assert torch.equal(got, ref), f"{name}: {int((got != ref).sum())} of {ref.numel()} logits differ"
        assert torch.equal(got, score(pl)), name
    mirror = torch.arange(n0, pu.numel(), device=DEV)
    first = torch.arange(0, n0, 3, device=DEV)
    got = score(hub)
    assert torch.equal(got[mirror], got[first])                                         # both ids of a mirrored pair
    assert float(ref.std()) > 0.05 and bool(torch.isfinite(ref).all())
    label = (torch.arange(pu.numel(), device=DEV) % 3 == 0).float()
    weight = torch.full((pu.numel(),), 1.0 / pu.numel(), device=DEV)
    x, _dZ, _dH = ops.score_pairs_train_logits(Z, H, plain, t, label, weight)
    assert torch.equal(x, ref), f"{int((x != ref).sum())} training logits differ from the forward logits"


def test_one_pass_logit_scorer_is_independent_of_the_row_sharding():
    """dl_score_pairs_train_logits over the incidence rows of a row shard gives that shard's rows of dZ / dH and the logits of the
    pairs touching it bit for bit as the unsharded call (the form of
    test_one_pass_training_scorer_is_independent_of_the_row_sharding, at (8, 64) fp32)."""
    from disenlink_amd import ops
    from disenlink_amd.graph import PairList
    K, d, t = 8, 64, 1.0
    st, G, _pairs = _device_structure()
    r = logit_ref.reference(K, d, "f32", t, ref64.BETAS[0])
    Z, H = dev32(r["Z"]), dev32(r["H_in"])
    label, weight = dev32(r["label"]), dev32(r["weight"])
    N = ref64.N_NODES
    tpu, tpv = st.pu.to(DEV), st.pv.to(DEV)
    big = int(st.pair_ladder[-1])                                     # the row with 300 pairs (several segments) alone in a shard
    whole = PairList.build(tpu, tpv, N, build_by_u=False, row_bytes=K * d * 4)
    x, dZ, dH = ops.score_pairs_train_logits(Z, H, whole, t, label, weight)
    cuts = sorted({0, big, big + 1, N})
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        inc = PairList.build(tpu, tpv, N, row_range=(lo, hi), build_by_u=False, row_bytes=K * d * 4)
        x_s, dZ_s, dH_s = ops.score_pairs_train_logits(Z, H, inc, t, label, weight)
        assert torch.equal(dZ_s[lo:hi], dZ[lo:hi]) and torch.equal(dH_s[lo:hi], dH[lo:hi]), (lo, hi)
        touch = (((tpu >= lo) & (tpu < hi)) | ((tpv >= lo) & (tpv < hi)))
        assert torch.equal(x_s[touch], x[touch]), (lo, hi)
    sliced = PairList.build(tpu, tpv, N, build_by_u=False, row_bytes=K * d * 4, inc_slices=8)
    assert sliced.inc.n_slices == 8 and sliced.inc.n_slots > 0
    x8, dZ8, dH8 = ops.score_pairs_train_logits(Z, H, sliced, t, label, weight)
    assert torch.equal(x8, x)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        inc = PairList.build(tpu, tpv, N, row_range=(lo, hi), build_by_u=False, row_bytes=K * d * 4, inc_slices=8)
        _x, dZ_s, dH_s = ops.score_pairs_train_logits(Z, H, inc, t, label, weight)
        assert torch.equal(dZ_s[lo:hi], dZ8[lo:hi]) and torch.equal(dH_s[lo:hi], dH8[lo:hi]), ("sliced", lo, hi)


@pytest.mark.parametrize("shape", [(8, 64, "f32"), (16, 128, "bf16"), (4, 32, "f32")], ids=lambda s: f"{s[2]}-K{s[0]}-d{s[1]}")
def test_nan_logit_at_weight_zero_leaves_every_gradient_finite(shape):
    """One listed pair (u, v) gets tables whose exponents overflow in two factors with h.h of opposite signs: its logit is
    inf - inf = NaN.  With weight 0 on every pair that touches u or v, the one-pass gradients stay finite everywhere (the factor
    clamps keep 0 * inf at 0), the rows of u and v are exactly 0, every other row is what fp64 says without those pairs, and the
    loss kernel ignores the NaN.  (One wave-per-entry kernel, the wide kernel on bf16 tables, the group-per-entry kernel.)"""
    from disenlink_amd import ops
    K, d, dtype = shape
    st, G, pairs = _device_structure()
    r = logit_ref.reference(K, d, dtype, 1.0, ref64.BETAS[0])
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    q0 = int(torch.nonzero((st.pu != st.pv) & (st.pu != st.isolated) & (st.pv != st.isolated))[0])
    u, v = int(st.pu[q0]), int(st.pv[q0])
    Z, H = r["Z"].clone(), r["H_in"].clone()
    Z[u, :2] = Z[v, :2] = (100.0 / d) ** 0.5                          # z_k[u].z_k[v] = 100 for k = 0, 1: expf overflows
    H[u, :2] = 1.0
    H[v, 0], H[v, 1] = 1.0, -1.0                                      # (+d) inf + (-d) inf
    Zt, Ht = Z.to(tdt).to(DEV), H.to(tdt).to(DEV)
    touched = ((st.pu == u) | (st.pv == u) | (st.pu == v) | (st.pv == v))
    w64 = r["weight"].clone()
    w64[touched] = 0.0
    label, weight = dev32(r["label"]), dev32(w64)
    x, dZ, dH = ops.score_pairs_train_logits(Zt, Ht, pairs, 1.0, label, weight)
    pairs.unbind_labels()
    touched = touched.to(DEV)
    assert bool(torch.isnan(x[q0])) and bool(torch.isfinite(x[~touched]).all())
    assert bool(torch.isfinite(dZ).all()) and bool(torch.isfinite(dH).all())
    for node in (u, v):
        assert bool((dZ[node] == 0).all()) and bool((dH[node] == 0).all())
    loss, g = ops.pair_bce_logits(x, label, weight)
    assert bool(torch.isfinite(loss)) and bool((g[touched] == 0).all()) and bool(torch.isfinite(g).all())
    # no other pair reads the rows of u or v: the fp64 step on the untouched tables with those weights is the reference
    _x, loss_ref, _g, dZ_ref, dH_ref = logit_ref.step64(r["Z"], r["H_in"], st.pu, st.pv, 1.0, r["label"], w64)
    assert ref64.row_ratio(dZ.cpu(), dZ_ref) <= B["dZ"] and ref64.row_ratio(dH.cpu(), dH_ref) <= B["dH"]
    assert logit_ref.rel_err(loss, loss_ref) <= B["loss"]


def _auc_counts(score: np.ndarray, label: np.ndarray) -> float:
    """Tie-averaged AUC of fp32 scores from integer counts on the CPU: sum over positives of 2 #{negatives below} +
    #{negatives equal}, over 2 n_pos n_neg."""
    pos, neg = score[label > 0.5], np.sort(score[label <= 0.5])
    u2 = int(np.searchsorted(neg, pos, side="left").sum()) + int(np.searchsorted(neg, pos, side="right").sum())
    return float(np.float64(u2) / np.float64(2.0 * pos.size * neg.size))


def test_saturated_pairs_keep_their_gradient_and_their_order():
    """5. Why the feature exists (fails without it).  H scaled until the fp64 reference alone puts at least a third of the pairs at
    |logit| in [20, 200], every second one of them with the WRONG label (logit_ref.saturated).  In probability space a pair
    whose fp32 probability is exactly 0 or 1 has gradient exactly 0 — pinned here as the contrast — and its score ties in the
    AUC; in logit space the same rows are within the fp64 bound and the AUC is that of the logits, exactly."""
    from disenlink_amd import ops
    from disenlink_amd.metrics import AucPlan
    K, d, t = 8, 64, 1.0
    st, G, pairs = _device_structure()
    s = logit_ref.saturated(K, d, t, ref64.BETAS[0])
    P = s["x"].numel()
    fig = _Figures("saturated")
    share = float(s["sat"].double().mean())
    fig.note("1/3 <= share of pairs with |logit| in [20, 200]", 1.0 / 3.0, share)
    fig.note("largest exp argument", s["arg_max"], 80.0)
    n_wrong_sat = int(s["wrong"].numel())
    fig.exact("half of the saturated pairs are wrong", abs(2 * n_wrong_sat - int(s["sat"].sum())) <= 1)
    dead = s["dead"].to(DEV)
    Z, H = dev32(s["Z"]), dev32(s["H_in"])
    assert torch.equal(H.double().cpu(), s["H_in"])
    label, weight = dev32(s["label"]), dev32(s["weight"])
    # fp64: the step, and which dead nodes carry a wrongly labelled pair (their reference rows are large)
    _x, loss64, _g, dZ_ref, dH_ref = logit_ref.step64(s["Z"], s["H_in"], st.pu, st.pv, t, s["label"], s["weight"])
    wrong_nodes = set(st.pu[s["wrong"]].tolist()) | set(st.pv[s["wrong"]].tolist())
    loud = [n for n in s["dead"].tolist() if n in wrong_nodes]
    fig.exact("some node has only dead pairs, one of them wrongly labelled", len(loud) >= 1)
    scale = float(dH_ref.abs().flatten(1).max(1).values[dH_ref.abs().flatten(1).max(1).values > 0].median())
    fig.exact("their fp64 gradient rows are of the size of the others (at least a tenth of the median row)",
              all(float(dH_ref[n].abs().max()) >= 0.1 * scale for n in loud))
    # probability space: today's behaviour, the contrast
    prob, dZp, dHp = ops.score_pairs_train(Z, H, pairs, t, label, weight)
    pairs.unbind_labels()
    fig.exact("prob: rows of nodes with only dead pairs are exactly 0", bool((dZp[dead] == 0).all()) and bool((dHp[dead] == 0).all()))
    # logit space
    x, dZ, dH = ops.score_pairs_train_logits(Z, H, pairs, t, label, weight)
    pairs.unbind_labels()
    fig.note("logits", ref64.band_ratio(x.cpu(), s["x"], s["x_abs"]), ref64.BOUND["logit"])
    fig.note("logit: dZ, all rows", ref64.row_ratio(dZ.cpu(), dZ_ref), B["dZ"])
    fig.note("logit: dH, all rows", ref64.row_ratio(dH.cpu(), dH_ref), B["dH"])
    dd = s["dead"]
    fig.note("logit: dH, the dead rows against their own size",
             float(((dH.cpu().double()[dd] - dH_ref[dd]).abs().flatten(1).max(1).values
                    / dH_ref[dd].abs().flatten(1).max(1).values.clamp_min(scale)).max()), B["dH"])
    fig.exact("logit: the dead rows with a wrong pair are not 0", all(float(dH[n].abs().max()) > 0 for n in loud))
    loss, _gk = ops.pair_bce_logits(x, label, weight)
    fig.note("loss", logit_ref.rel_err(loss, loss64), B["loss"])
    # AUC: labels as listed.  On probabilities every pair scored exactly 1 ties; on logits nothing is lost
    plan = AucPlan(label)
    one = prob == 1.0
    fig.exact("at least a quarter of the probabilities are exactly 1 (one tie block)", float(one.float().mean()) >= 0.25)
    x_np, p_np, y_np = x.cpu().numpy(), prob.cpu().numpy(), label.cpu().numpy()
    auc_x, auc_p = float(plan.auc(x)), float(plan.auc(prob))
    fig.exact("AUC on logits == CPU tie-averaged AUC of the same fp32 logits", auc_x == _auc_counts(x_np, y_np))
    fig.exact("AUC on probabilities == that of the same fp32 probabilities", auc_p == _auc_counts(p_np, y_np))
    fig.exact("the tie block costs the probabilities' AUC its order", auc_p != auc_x and np.unique(x_np[one.cpu().numpy()]).size > 0.9 * int(one.sum()))
    fig.check()


@pytest.mark.parametrize("n", logit_ref.BCE_SIZES)
def test_loss_kernel_matches_fp64(n):
    """6. dl_pair_bce_logits against the fp64 formula on the fp32 logits it is handed, around the 1,024 partial sums; and, on the
    pairs with |x| < 10 of every LIST, against dl_pair_bce on sigmoid(x) to 1e-5 relative (the tolerance and the kind of input —
    a list of pairs — of test_fused_pair_bce_matches_torch_bce).  Not at n = 1: a single pair whose label agrees costs
    -log(p) = delta with p = 1 - delta, and the fp32 probability carries delta to 2^-24 / delta only — 1.3e-3 at |x| = 10, 1.3e-5
    measured on this input — which is probability space's error, the one this kernel exists to avoid, not a tolerance to meet."""
    from disenlink_amd import ops
    x, y, w = logit_ref.bce_inputs(n)
    loss, g = ops.pair_bce_logits(x.to(DEV), y.to(DEV), w.to(DEV))
    fig = _Figures(f"bce n={n}")
    want = logit_ref.pair_loss64(x.double(), y.double(), w.double()).sum()
    fig.note("loss", logit_ref.rel_err(loss, want), B["loss_kernel"])
    fig.note("g", logit_ref.g_ratio(g.cpu(), logit_ref.g64(x.double(), y.double(), w.double()), w), B["g"])
    loss2, g2 = ops.pair_bce_logits(x.to(DEV), y.to(DEV), w.to(DEV))
    fig.exact("deterministic", torch.equal(loss, loss2) and torch.equal(g, g2))
    # |x| < 10: the value dl_pair_bce gives on sigmoid(x), to the tolerance of test_fused_pair_bce_matches_torch_bce
    near = x.abs() < 10
    if n > 1:
        assert int(near.sum()) >= 100
        xs, ys, ws = x[near].to(DEV), y[near].to(DEV), w[near].to(DEV)
        a, _ga = ops.pair_bce_logits(xs, ys, ws)
        b, _gb = ops.pair_bce(torch.sigmoid(xs), ys, ws)
        fig.note("|x| < 10: against dl_pair_bce on sigmoid(x)", abs(float(a) - float(b)) / max(abs(float(b)), 1e-30), 1e-5)
    fig.check()


def test_loss_kernel_at_infinite_and_nan_logits():
    from disenlink_amd import ops
    inf, nan = float("inf"), float("nan")
    f = lambda *v: torch.tensor(v, dtype=torch.float32, device=DEV)
    w = f(0.5, 0.5, 0.25, 0.25)
    loss, g = ops.pair_bce_logits(f(inf, -inf, 3.0, -2.0), f(1.0, 0.0, 1.0, 0.0), w)          # the agreeing label costs 0
    fin, _ = ops.pair_bce_logits(f(3.0, -2.0), f(1.0, 0.0), w[2:])
    assert torch.equal(loss, fin) and g[:2].tolist() == [0.0, 0.0] and bool(torch.isfinite(g).all())
    for x, y in ((inf, 0.0), (-inf, 1.0)):                                                  # the other label costs inf
        loss, g = ops.pair_bce_logits(f(x, 3.0), f(y, 1.0), w[:2])
        assert float(loss) == inf and float(g[0]) == (0.5 if y == 0.0 else -0.5)
    loss, g = ops.pair_bce_logits(f(nan, 3.0, -2.0), f(1.0, 1.0, 0.0), f(0.0, 0.25, 0.25))    # NaN at w = 0: ignored
    assert torch.equal(loss, fin) and float(g[0]) == 0.0
    loss, g = ops.pair_bce_logits(f(nan, 3.0, -2.0), f(1.0, 1.0, 0.0), f(0.5, 0.25, 0.25))    # NaN at w != 0: a NaN loss
    assert bool(torch.isnan(loss)) and bool(torch.isnan(g[0])) and bool(torch.isfinite(g[1:]).all())
    # the small side is kept where fp32 probabilities have long rounded: sigma(30) - 1 = -9.36e-14
    _l, g = ops.pair_bce_logits(f(30.0, -30.0, 90.0), f(1.0, 0.0, 1.0), f(1.0, 1.0, 1.0))
    want = torch.tensor([-9.357622968839299e-14, 9.357622968839299e-14, -8.194012623990515e-40], dtype=torch.float64)
    assert torch.allclose(g.double().cpu()[:2], want[:2], rtol=B["g"], atol=0) and float(g[2]) <= 0.0


def _model_and_inputs(table_dtype, seed=3):
    from disenlink_amd.model import Disentangle
    st, G, pairs = _device_structure()
    torch.manual_seed(seed)
    model = Disentangle(32, 48, 64, nfactor=8, beta=0.6, t=1, table_dtype=table_dtype).to(DEV)
    x = torch.randn(ref64.N_NODES, 32, generator=torch.Generator().manual_seed(seed)).to(DEV)
    rng = np.random.default_rng(seed)
    P = st.pu.numel()
    label = torch.from_numpy((rng.random(P) < 0.3).astype(np.float32)).to(DEV)
    weight = torch.from_numpy((rng.uniform(0.2, 1.0, P) / 64).astype(np.float32)).to(DEV)
    weight[::9] = 0.0
    return model, x, G, pairs, label, weight


@pytest.mark.parametrize("table_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("extra", [False, True], ids=["loss", "loss+logits+emb"])
def test_compiled_operator_equals_the_python_functions_bit_for_bit(table_dtype, extra, monkeypatch):
    """7. Disentangle.forward_pair_logits_loss through the compiled node (DL_NATIVE_OPS=1) and through ops.HotPathPairLogitsLoss
    (DL_NATIVE_OPS=0): emb, logits, loss and every parameter gradient — for loss.backward() (d/dloss applied inside the last
    kernel) and with further gradients arriving on the logits and on the embedding (the logit backward)."""
    from disenlink_amd import native
    out = {}
    try:
        for mode in ("1", "0"):
            monkeypatch.setenv("DL_NATIVE_OPS", mode)
            native._state["loaded"] = None
            assert native.available() == (mode == "1")
            model, x, G, pairs, label, weight = _model_and_inputs(table_dtype)
            emb, logit, loss = model.forward_pair_logits_loss(x, G, pairs, label, weight)
            assert (type(loss.grad_fn).__name__ == "HotPathPairLogitsLossBackward") == (mode == "0"), type(loss.grad_fn).__name__
            total = loss * 1.5
            if extra:
                total = total + torch.nn.functional.softplus(-logit[::5]).mean() + (emb * emb).sum() * 1e-3
            total.backward()
            pairs.unbind_labels()
            out[mode] = (emb.detach().clone(), logit.detach().clone(), loss.detach().clone(),
                         {k: p.grad.clone() for k, p in model.named_parameters()})
    finally:
        monkeypatch.delenv("DL_NATIVE_OPS", raising=False)
        native._state["loaded"] = None
    for a, b, what in zip(out["1"][:3], out["0"][:3], ("emb", "logit", "loss")):
        assert torch.equal(a, b), what
    assert out["1"][3].keys() == out["0"][3].keys() and len(out["1"][3]) == 4 * 8
    for k in out["1"][3]:
        assert torch.equal(out["1"][3][k], out["0"][3][k]), k
        assert bool(torch.isfinite(out["1"][3][k]).all()) and float(out["1"][3][k].abs().max()) > 0, k


def test_training_loop_in_logit_space_runs_the_same_eager_early_stopped_and_replayed(monkeypatch):
    """8. 30 epochs of run_link_prediction(objective="pairs-logit") on a 300-node synthetic graph at (8, 64): the eager loop with the
    bookkeeping on the host, the device early stop and HIP-graph replay give the same loss and AUC histories bit for bit; the
    loss is finite throughout and lower at the end than at the start."""
    from disenlink_amd.data import SPECS, synthetic_graph
    from disenlink_amd.model import Disentangle
    from disenlink_amd.splits import make_link_split
    from disenlink_amd.train import prepare_run, run_link_prediction
    sg = synthetic_graph("cora", seed=4, scale=300.0 / SPECS["cora"]["N"])
    assert sg.n_nodes == 300
    split = make_link_split(sg.src, sg.dst, sg.n_nodes, m=5, seed=4)
    run = prepare_run(split, torch.device(DEV), row_bytes=8 * 64 * 4)
    x = torch.from_numpy(sg.features()[:, :64].copy()).to(DEV)
    out = {}
    for name, early, use_graph in (("eager", "0", False), ("device early stop", "1", False), ("graph replay", "1", True)):
        monkeypatch.setenv("DL_DEVICE_EARLY_STOP", early)
        torch.manual_seed(0)
        model = Disentangle(64, 64, 64, nfactor=8, beta=0.6, t=1).to(DEV)
        out[name] = run_link_prediction(model, x, run, epochs=30, lr=2e-3, patience=200, use_graph=use_graph,
                                        objective="pairs-logit")
    ref = out["eager"]
    assert ref.epochs_run == 30 and len(ref.losses) == 30
    assert all(np.isfinite(ref.losses)) and ref.losses[-1] < ref.losses[0], (ref.losses[0], ref.losses[-1])
    assert all(0.0 <= a <= 1.0 for a in ref.val_aucs) and 0.0 <= ref.test_auc <= 1.0
    for name in ("device early stop", "graph replay"):
        got = out[name]
        assert got.losses == ref.losses and got.val_aucs == ref.val_aucs, name
        assert got.best_val_auc == ref.best_val_auc and got.test_auc == ref.test_auc, name
