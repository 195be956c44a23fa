"""Every compiled instantiation of the hot-path kernels (routing, aggregation, pair scorer, scorer backward, one-pass
training scorer, routing/aggregation backward) against the plain fp64 reference of tests/ref64.py, on ONE graph and ONE
pair list whose rows sit on the production plans' boundaries: adjacency rows of 0, 1, 2, 7..9, 15..17, 31..33, 63..65,
127..129, 255..257 and 290 entries (segments of 32 in units of 4; routing segments of 8 / 16), incidence rows and forward
runs of 0, 1, 63..65, 255..257 and 300 (segments and runs of 64, units of 256), duplicated edges, self-loops, an isolated
node, duplicate pairs and u == v pairs — with the default plan parameters throughout.

The shapes are asked of the library (dl_has_fast_path_dtype over K = 1..64, d in {4, 8, 16, 32, 64, 128}, both table
types), not copied: a new X(K, D) in dl_fast.h is tested the day it is compiled.  Every tuned fp32 shape runs once more
on the generic kernels, three shapes have no tuned kernel at all, (8, 64) runs at t = 1, 2 and 0.5.

Each kernel is handed exactly rounded inputs of the reference (ref64.reference): tables Z, the reference's (a, s) cast
to fp32, its H rounded to the table type, the fp32 sigmoid of its logit, its dH cast to fp32 — no kernel's error leaks into
the check of the next, and routing is decisive on every edge (margin > 1e-5 in fp64), so p must be exact everywhere.

Bounds.  Forward outputs: per element, c * 2^-24 * (absolute-sum companion of ref64).  Gradients: per node,
max |got_i - ref_i| / max(max |ref_i|, median_j max |ref_j|)  (ref64.row_ratio).  Every constant is 4x the largest value the
fp32 numpy oracle (oracle/sparse_ref.py) itself shows against ref64 on these same cases — measured and re-asserted by
tests/test_ref64_cpu.py, recorded in ref64.ORACLE; the 4 covers another equally valid fp32 summation order and a
hardware exp.  None was set from what the kernels give.  Probabilities: max sigma' over the logit band times the band,
plus eps 2^-24.

bf16 H: half a bf16 unit in the last place on top of the fp32 band of the element, per element.  bf16 keeps 8 significant
bits, so half a unit in the last place of x is 2^(floor(log2 |x|) - 8): between 2^-9 |x| (x just below a power of two) and
2^-8 |x| (x a power of two), and it is taken exactly, from the binade of |H64| + band (ref64.bf16_half_ulp).  The binade
is that of |H64| + band and not of |H64| on purpose: the kernel rounds ITS fp32 value, which may lie anywhere within the
band of H64, so an element less than one band below a power of two may be rounded in the next binade, whose half unit is
twice as large; only those elements get the larger allowance, every other element the half unit of its own binade.  The flat 2^-9 |H64| is NOT that bound and no bf16 store can
meet it: -0.2509822 lies in [2^-2, 2^-1), where bf16 numbers are 2^-9 apart, its nearest neighbour -0.251953 is 9.7e-4 =
0.99 half-units away, but 2^-9 |x| is only 4.9e-4.  The fp32 numpy oracle's own H, rounded to nearest even on the CPU,
exceeds 2^-9 |H64| by 3.2e4 band units at (4, 32) and (5, 64) alike and stays inside the exact half-unit bound with
the oracle's fp32 figure (tests/test_ref64_cpu.py asserts both).  The excess over 2^-9 |H64| is still printed.

    output                           oracle (worst of 25 inputs)  bound (4x)   kernels on an MI355X (worst of the 38 cases)
    a        [2^-24 companion]       3.17                         12.68        2.17   K2 d1 t2
    s        [2^-24 companion]       4.41                         17.64        4.41   K2 d1 t2
    H        [2^-24 companion]       5.07                         20.28        6.81   K20 d32 t0.5, generic
    H bf16, beyond half a unit in the last place   as H          20.28        2.94   K16 d128 t1 (beyond 2^-9 |H64|: 3.25e4)
    logit    [2^-24 companion]       2.54                         10.16        prob: 0.24 of its band (K3 d8 t1), every form
    prob eps [2^-24]                 1.51                         6.04         and the one-pass scorer alike
    dZ score [row ratio]             6.43e-06                     2.57e-05     9.6e-07 (stored terms 3.4e-07, one pass 1.2e-06)
    dH       [row ratio]             2.61e-06                     1.04e-05     1.1e-06 (stored terms 3.2e-07, one pass 8.5e-07)
    dZ route+aggregate [row ratio]   1.12e-06                     4.48e-06     1.1e-06 (onto dZ_accum 7.3e-07, scaled 7.1e-07)

The kernels' column is for the record (one run); no bound was taken from it.  Every figure of a run is
printed as a FIGURE line before anything is asserted (pytest -s).  bf16 tables have no per-pair scorer: the call without
a plan must be refused by the library, and is asserted to be.
(The oracle's dZ-score figure contains its own fp32 probability in the sigmoid backward; the scorer backward is handed
the reference's, which is why it lands well below it.)
"""
import numpy as np
import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = ref64.U


def _cases():
    from disenlink_amd import _lib
    return ref64.hotpath_cases(_lib.load())


_device = {}


def _device_structure():
    """The builder's graph and pair list on the device (built once; the same rows as the CPU plans the builder checked)."""
    if not _device:
        from disenlink_amd.graph import PairList
        st = ref64.structure()
        G = st.graph.to(DEV)
        pairs = PairList.build(st.pu.to(DEV), st.pv.to(DEV), ref64.N_NODES)
        for mine, theirs in ((pairs.by_u, st.pairs.by_u), (pairs.inc, st.pairs.inc)):
            assert torch.equal(mine.rowptr.cpu(), theirs.rowptr) and torch.equal(mine.col.cpu(), theirs.col)
            assert mine.seg_len == theirs.seg_len and mine.n_seg == theirs.n_seg
        _device["v"] = (st, G, pairs)
    return _device["v"]


def test_case_ids_show_every_tuned_shape_of_the_library():
    from disenlink_amd import _lib
    lib = _lib.load()
    cases = _cases()
    for dtype in ("f32", "bf16"):
        shapes = ref64.tuned_shapes(lib, dtype)
        assert (8, 64) in shapes                                                   # the benchmark's shape
        assert {(c.K, c.d) for c in cases if c.dtype == dtype and not c.generic} >= set(shapes)
    assert {(c.K, c.d) for c in cases if c.generic} == set(ref64.tuned_shapes(lib, "f32"))
    assert not any(lib.dl_has_fast_path_dtype(K, d, _lib.DL_F32) for K, d in ref64.UNTUNED)


@pytest.mark.parametrize("case", _cases(), ids=ref64.case_id)
def test_hot_path_kernels_match_fp64(case):
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    K, d, dtype, t, beta, generic = case
    st, G, pairs = _device_structure()
    r = ref64.reference(K, d, dtype, t, beta)
    tdt, code = (torch.float32, _lib.DL_F32) if dtype == "f32" else (torch.bfloat16, _lib.DL_BF16)
    B = ref64.BOUND
    figures = []                                        # (what, observed, bound): all printed, then all asserted

    def note(what, observed, bound):
        figures.append((what, float(observed), float(bound)))

    def exact(what, ok):
        figures.append((what, 0.0 if ok else float("inf"), 0.0))

    dev32 = lambda x: x.float().to(DEV)
    Zt, H_in = r["Z"].to(tdt).to(DEV), r["H_in"].to(tdt).to(DEV)
    assert torch.equal(Zt.double().cpu(), r["Z"]) and torch.equal(H_in.double().cpu(), r["H_in"])     # the kernels see the reference's values
    old = lib.dl_set_force_generic(1 if generic else 0)
    try:
        assert bool(lib.dl_has_fast_path_dtype(K, d, code)) == ((K, d) not in ref64.UNTUNED)
        # 1. routing
        p, a, s = ops.route_fwd(G, Zt, t)
        exact("route p exact on every edge", torch.equal(p.cpu().long(), r["p"]))
        note("route a", ref64.band_ratio(a.cpu(), r["a"], r["a_abs"]), B["a"])
        note("route s", ref64.band_ratio(s.cpu(), r["s"], r["s_abs"]), B["s"])
        exact("route s == 0 at the isolated node", bool((s[st.isolated] == 0).all()))
        p2, a2, s2 = ops.route_fwd(G, Zt, t)
        exact("route bitwise repeatable", torch.equal(p, p2) and torch.equal(a, a2) and torch.equal(s, s2))

        # 2. aggregation, from the reference's (p, a, s)
        p_in, a_in, s_in = r["p"].to(torch.uint8).to(DEV), dev32(r["a32"]), dev32(r["s32"])
        H = ops.aggregate_fwd(G, Zt, beta, p_in, a_in, s_in)
        assert H.dtype == tdt
        err = (H.double().cpu() - r["H"]).abs()
        if dtype == "bf16":
            note("aggregate H beyond 2^-9 |H64| (recorded, unattainable: see the docstring)",
                 ref64.band_ratio(torch.clamp(err - 2.0 ** -9 * r["H"].abs(), min=0.0), torch.zeros_like(err), r["H_abs"]), float("inf"))
            err = torch.clamp(err - ref64.bf16_half_ulp(r["H"].abs() + B["H"] * U * r["H_abs"]), min=0.0)
        note("aggregate H" + (" beyond half a bf16 ulp" if dtype == "bf16" else ""),
             ref64.band_ratio(err, torch.zeros_like(err), r["H_abs"]), B["H"])
        exact("aggregate bitwise repeatable", torch.equal(H, ops.aggregate_fwd(G, Zt, beta, p_in, a_in, s_in)))

        # 3. pair scorer, from the reference's H: with the plan, without it, with the stored terms
        p64 = torch.sigmoid(r["logit"])
        band = ref64.prob_band(r["logit"], B["logit"] * U * r["logit_abs"], B["prob_eps"] * U)
        dup = torch.from_numpy(st.dup_pairs).to(DEV)
        coef = None
        for form in ("plan", "no plan", "plan + coef"):
            if form == "plan + coef":
                prob, coef = ops.score_pairs_fwd(Zt, H_in, pairs.pu, pairs.pv, t, pairs, want_coef=True)
                prob_again, coef_again = ops.score_pairs_fwd(Zt, H_in, pairs.pu, pairs.pv, t, pairs, want_coef=True)
                if coef is not None:
                    exact("score fwd stored terms bitwise repeatable", torch.equal(coef.view(torch.int32), coef_again.view(torch.int32)))
                exact("stored terms exist exactly where a tuned kernel runs",
                      (coef is not None) == ((K, d) not in ref64.UNTUNED and not generic))
            elif form == "no plan" and dtype == "bf16":          # no per-pair bf16 kernel: refused, not served some other way
                with pytest.raises(_lib.DisenlinkHipError, match="no generic bf16 path"):
                    ops.score_pairs_fwd(Zt, H_in, pairs.pu, pairs.pv, t, None)
                continue
            else:
                prob = ops.score_pairs_fwd(Zt, H_in, pairs.pu, pairs.pv, t, pairs if form == "plan" else None)
                prob_again = ops.score_pairs_fwd(Zt, H_in, pairs.pu, pairs.pv, t, pairs if form == "plan" else None)
            note(f"score fwd ({form}) prob / band", float(((prob.double().cpu() - p64).abs() / band).max()), 1.0)
            exact(f"score fwd ({form}) duplicate pairs give identical bits",
                  torch.equal(prob[dup[:, 0]].view(torch.int32), prob[dup[:, 1]].view(torch.int32)))
            exact(f"score fwd ({form}) bitwise repeatable", torch.equal(prob, prob_again))

        # 4. scorer backward from a random g_prob, at the fp32 probabilities of the reference's logits
        prob_in, g_prob = dev32(r["prob32"]), dev32(r["g_prob"])
        for cf in ((None, coef) if coef is not None else (None,)):
            tag = "score bwd" + (" (coef)" if cf is not None else "")
            dZ, dH = ops.score_pairs_bwd(Zt, H_in, pairs, t, prob_in, g_prob, coef=cf)
            note(tag + " dZ", ref64.row_ratio(dZ.cpu(), r["dZ_score"]), B["dZ_score"])
            note(tag + " dH", ref64.row_ratio(dH.cpu(), r["dH"]), B["dH"])
            dZ2, dH2 = ops.score_pairs_bwd(Zt, H_in, pairs, t, prob_in, g_prob, coef=cf)
            exact(tag + " bitwise repeatable", torch.equal(dZ, dZ2) and torch.equal(dH, dH2))

        # 5. one-pass training scorer: weighted BCE of (label, weight), weight-0 pairs included
        if ops.score_pairs_train_supported(pairs, K, d, code):
            label, weight = dev32(r["label"]), dev32(r["weight"])
            prob, dZ, dH = ops.score_pairs_train(Zt, H_in, pairs, t, label, weight)
            note("score train prob / band", float(((prob.double().cpu() - p64).abs() / band).max()), 1.0)
            note("score train dZ", ref64.row_ratio(dZ.cpu(), r["dZ_train"]), B["dZ_score"])
            note("score train dH", ref64.row_ratio(dH.cpu(), r["dH_train"]), B["dH"])
            for _again in range(2):                     # the second sight of the same tensors binds per-entry labels (graph.py)
                prob2, dZ2, dH2 = ops.score_pairs_train(Zt, H_in, pairs, t, label, weight)
                exact("score train bitwise repeatable", torch.equal(prob, prob2) and torch.equal(dZ, dZ2) and torch.equal(dH, dH2))
            pairs.unbind_labels()
        else:
            exact("one-pass scorer is there for every tuned shape", (K, d) in ref64.UNTUNED or generic)

        # 6. routing / aggregation backward from the reference's dH (fp32): plain, accumulating, scaled
        dH_in = dev32(r["dH32"])
        dZ = ops.route_aggregate_bwd(G, Zt, beta, t, p_in, a_in, s_in, dH_in)
        note("route+aggregate bwd dZ", ref64.row_ratio(dZ.cpu(), r["dZ_route"]), B["dZ_route"])
        exact("route+aggregate bwd bitwise repeatable", torch.equal(dZ, ops.route_aggregate_bwd(G, Zt, beta, t, p_in, a_in, s_in, dH_in)))
        gen = torch.Generator().manual_seed(r["seed"])
        base64 = torch.randn(r["dZ_route"].shape, generator=gen, dtype=torch.float64).float().double() \
            * float(r["dZ_route"].abs().flatten(1).max(1).values.median())
        base = dev32(base64)
        got = ops.route_aggregate_bwd(G, Zt, beta, t, p_in, a_in, s_in, dH_in, dZ_accum=base.clone())
        note("route+aggregate bwd onto dZ_accum", ref64.row_ratio(got.cpu(), r["dZ_route"] + base.double().cpu()), B["dZ_route"])
        exact("dZ_accum bitwise repeatable",
              torch.equal(got, ops.route_aggregate_bwd(G, Zt, beta, t, p_in, a_in, s_in, dH_in, dZ_accum=base.clone())))
        scale = torch.tensor([0.37], device=DEV)
        got = ops.route_aggregate_bwd_scaled(G, Zt, beta, t, p_in, a_in, s_in, dH_in, base, scale)
        want = float(scale.double().cpu()) * (r["dZ_route"] + base.double().cpu())
        note("route+aggregate bwd scaled", ref64.row_ratio(got.cpu(), want), B["dZ_route"])
        exact("scaled bwd bitwise repeatable",
              torch.equal(got, ops.route_aggregate_bwd_scaled(G, Zt, beta, t, p_in, a_in, s_in, dH_in, base, scale)))
    finally:
        lib.dl_set_force_generic(old)

    for what, observed, bound in figures:
        print(f"FIGURE {ref64.case_id(case)} | {what} | {observed:.4g} | {bound:.4g}")
    bad = [f for f in figures if not f[1] <= f[2]]                        # (a NaN is not <= anything)
    assert not bad, bad
