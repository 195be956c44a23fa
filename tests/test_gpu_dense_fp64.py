"""Every kernel of the all-pairs scorer family against the plain fp64 reference of tests/ref64_dense.py, per element:
  * the dense scorer dl_score_allpairs_fwd — score_allpairs_split_kernel<PLANES> (dl_score_dense.hip) with and without
    its workspace, the per-shape score_allpairs_kernel<K, D, T> of every tuned shape in both table types (dl_score.hip),
    score_allpairs_fwd_kernel (dl_generic.hip);
  * the ranking scan dl_score_topk / dl_score_ranks — rank_scan_kernel<TOPK | RANKS | DIAG>, topk_merge_kernel and the
    target kernels (dl_score_rank.hip);
  * the dense backward dl_score_allpairs_bwd_dense — ghat_kernel, split_cols_kernel, score_dense_bwd_kernel<1..4>,
    combine_kernel (dl_score_dense_bwd.hip),
on the case lists of ref64_dense (dense_cases, rank_cases, dense_bwd_cases): the smallest shapes that reach each launch
form, which the library itself confirms for every case before anything runs (dl_score_allpairs_fwd_form,
dl_score_allpairs_bwd_dense_form, dl_score_topk_form; tests/test_ref64_dense_cpu.py asserts that the lists reach all forms).

Each call is handed exactly rounded inputs of the reference: full-mantissa tables with quiet and loud node rows at tile
positions, a zero row and two exact copies of one row; the backward gets the fp32 rounding of the REFERENCE's prob.  No
kernel's error leaks into the check of the next.  DL_POISON=1 (conftest.py) turns anything read but never written into
NaN, and a NaN fails its assertion.

Bounds.  Per element, c * 2^-24 * (absolute-sum companion), c = 4 x the figure the plain fp32 evaluation shows against the
reference over these same cases (ref64_dense.ORACLE, measured again on the CPU on every run) plus PLANE = 2 + 2^-8 per
three-plane product between the inputs and the output (ref64_dense's docstring derives the counts).  None was set from
what the kernels give; tests/test_ref64_dense_cpu.py shows on a CPU emulation of the plane scheme that all six products
stay inside them and that each single removed product leaves them.

    output   oracle   bound fp32 (4x)   bound on planes          kernels on an MI355X (profiles/dense_fp64_figures.txt)
    logit    5.80     23.2              + 1 PLANE = 25.20        scan 5.10
    prob     band of the logit through the sigmoid + 4 x 1.48 units of 2^-24: figure = error / band, bound 1
                                                                 matrix cores 0.231, per shape 0.239, generic 0.218, scan 0.201
    dH       14.8     59.2              + 2 PLANE = 63.21        32.4
    dZ       9.43     37.72             + 2 PLANE = 41.73        19.4
(the last column is the record of one run, for the reader; no bound is taken from it)

What the hardware run settled.  Both claims of the code hold: for d % 32 == 0 and query < candidate sigmoid(scan logit) has
the bits of the dense scorer's P[query, candidate], and the scan's logit of a pair does not depend on where in a tile its
rows sit (the copies tie exactly, the permuted orders and every slicing return the same bits).  One expectation did not:
the two copied rows of the DENSE scorer are not equal in every bit.  Every entry of P is formed once, with the smaller index
as the A operand; against a partner between the copies the operand order differs for the two copies, which swaps hi*lo and
lo*hi in the accumulation and moved the last bit of 20 entries over the ten matrix-core cases (at most 0.052 of two bands).
The kernel's store comment says as much, so the test was corrected, not the code: equal bits against every partner outside
[a, b] (same operand order, different tile positions), within two bands between them; dl_tiles.h now says "ordered pair".

Every figure of a run is printed as a FIGURE line before anything is asserted (pytest -s).  The looser tests of
test_gpu_rank.py, test_gpu_dense_bwd.py and test_gpu_parity.py stay as the wide net; this file is the tight one.
"""
import pytest
import torch

import ref64_dense as rd
from ref64 import U, band_ratio, prob_band

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _load():
    from disenlink_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _forward_without_workspace(lib, Z, H, c):
    """dl_score_allpairs_fwd with ws == NULL (the matrix-core kernel then splits what it stages: PLANES = false)."""
    from disenlink_amd import _lib, ops
    P = torch.full((c.N, c.N), float("nan"), device=Z.device)
    code = {"f32": _lib.DL_F32, "bf16": _lib.DL_BF16}[c.dtype]
    _lib.check(lib.dl_score_allpairs_fwd(Z.data_ptr(), H.data_ptr(), c.N, c.K, c.d, code, float(c.t), P.data_ptr(), None, 0,
                                         ops._stream()), "dl_score_allpairs_fwd")
    return P


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


class Figures:
    """(what, observed, bound): all printed as FIGURE lines, then all asserted; a NaN fails."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def note(self, what, got, bnd):
        self.rows.append((what, float(got), float(bnd)))

    def exact(self, what, ok):
        self.rows.append((what, 0.0 if bool(ok) else float("inf"), 0.0))

    def close(self):
        print()
        for what, got, bnd in self.rows:
            print(f"FIGURE {self.name}: {what} = {got:.4g} (bound {bnd:.4g})")
        for what, got, bnd in self.rows:
            assert got <= bnd, (self.name, what, got, bnd)


# ---------------------------------------------------------------------------------------------------------------- forward
def _forward_cases():
    from disenlink_amd import _lib
    return rd.dense_cases(_lib.load())


@pytest.mark.parametrize("case", _forward_cases(), ids=rd.case_id)
def test_dense_scorer_matches_fp64(case):
    from disenlink_amd import ops
    lib = _load()
    c = case
    rd.check_forward_form(c)                              # the case still reaches the kernel and geometry it was written for
    r = rd.reference(c.N, c.K, c.d, c.t, c.dtype)
    planes = c.kernel == "matrix cores"
    fig = Figures(c.name)
    dt = torch.float32 if c.dtype == "f32" else torch.bfloat16
    Z, H = r["Z"].to(DEV).to(dt), r["H"].to(DEV).to(dt)
    old = lib.dl_set_force_generic(1 if c.force_generic else 0)
    try:
        P = ops.score_allpairs_fwd(Z, H, c.t)
        P2 = ops.score_allpairs_fwd(Z, H, c.t)
        Pn = _forward_without_workspace(lib, Z, H, c)
        Pc = P.cpu()                                        # (synchronises: the switch below is read at launch time only)
    finally:
        lib.dl_set_force_generic(old)
    fig.note("prob error / band", rd.prob_ratio(Pc, r, planes), 1.0)
    fig.note("prob error / band, no workspace", rd.prob_ratio(Pn.cpu(), r, planes), 1.0)
    fig.exact("bitwise repeatable", _same(P, P2))
    fig.exact("P == P^T bit for bit", _same(P, P.t().contiguous()))
    fig.exact("the same bits with and without the workspace", _same(P, Pn))
    if r["zero"] is not None:
        z = r["zero"]
        fig.exact("prob == 0.5 exactly on the zero row and column", bool((Pc[z] == 0.5).all() and (Pc[:, z] == 0.5).all()))
    if r["copies"] is not None:
        # Every entry is formed once, from the (min, max) ordering of its pair (dl_score_dense.hip), and the two orderings of
        # a pair may differ in the last bit: against a partner OUTSIDE [a, b] both copies stand on the same side of the pair,
        # so the bits must be equal although the copies sit at different tile positions; against a partner between them the
        # sides are swapped, and both values lie in the band of the one reference value.
        a, b = r["copies"]
        out = torch.ones(c.N, dtype=torch.bool)
        out[a:b + 1] = False
        fig.exact("the copied rows have equal bits against every partner outside them", _same(Pc[a][out], Pc[b][out])
                  and _same(Pc[a, a], Pc[b, b]) and _same(Pc[a, a], Pc[a, b]))
        two = 2.0 * rd.prob_band_of(r, planes)[a]
        gap = ((Pc[a].double() - Pc[b].double()).abs() / two)[~out]
        fig.note(f"the copied rows against the {int((~out).sum())} partners between them ({int((Pc[a] != Pc[b])[~out].sum())} differ in bits), "
                 "difference / two bands", float(gap.max()), 1.0)
    fig.close()


# --------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("case", rd.dense_bwd_cases(), ids=rd.case_id)
def test_dense_backward_matches_fp64(case):
    from disenlink_amd import ops
    _load()
    c = case
    rd.check_backward_form(c)
    r = rd.reference(c.N, c.K, c.d, c.t)
    ref = rd.backward_reference(c.N, c.K, c.d, c.t)
    fig = Figures(c.name)
    Z, H, prob = r["Z"].to(DEV), r["H"].to(DEV), r["prob32"].to(DEV)
    for kind in rd.KINDS:
        b = ref[kind]
        g = b["g"].to(DEV)
        dZ, dH = ops.score_allpairs_bwd_dense(Z, H, c.t, prob, g)
        dZ2, dH2 = ops.score_allpairs_bwd_dense(Z, H, c.t, prob, g)
        # band_ratio: an element whose companion is 0 must be exactly 0 (else the ratio is inf)
        fig.note(f"{kind} dZ", band_ratio(dZ.cpu(), b["dZ"], b["dZ_abs"]), rd.bound("dZ"))
        fig.note(f"{kind} dH", band_ratio(dH.cpu(), b["dH"], b["dH_abs"]), rd.bound("dH"))
        fig.exact(f"{kind} finite", bool(torch.isfinite(dZ).all() and torch.isfinite(dH).all()))
        fig.exact(f"{kind} bitwise repeatable", _same(dZ, dZ2) and _same(dH, dH2))
        if kind == "dense" and r["copies"] is not None:      # g_prob treats the two copies alike
            a, bb = r["copies"]
            fig.exact("dense: the copied rows have equal bits", _same(dZ[a], dZ[bb]) and _same(dH[a], dH[bb]))
    fig.close()


# ---------------------------------------------------------------------------------------------------------------- ranking
def _check_topk(fig, tag, view, k, idx, logit, prob):
    """One top-k result (CPU tensors, ids of the view) against the reference: every returned logit inside the band of the
    returned index, the reference's set wherever the bands decide it and a valid top-k under the band rule elsewhere, the
    reference's candidate at every position whose band stands alone, the output sorted, rows short of k padded."""
    s, band, cand, twins = view["s"], view["band"], view["cand"], view["twins"]
    Q, N = s.shape
    ref, n, decisive = rd.topk_expectation(view, k)
    valid = idx >= 0
    pos = torch.arange(k)[None, :]
    fig.exact(f"{tag} rows hold min(k, candidates) entries, then -1 / NaN / NaN",
              torch.equal(valid, pos < n[:, None]) and bool((idx[~valid] == -1).all()) and bool(torch.isnan(logit[~valid]).all())
              and bool(torch.isnan(prob[~valid]).all()))
    safe = idx.clamp(min=0)
    s_g, b_g = s.gather(1, safe), band.gather(1, safe)
    err = (logit.double() - s_g).abs()
    q = torch.where(valid & (err > 0), err / b_g.clamp_min(1e-300), torch.zeros_like(err))
    fig.note(f"{tag} logit of the returned index", float("nan") if bool(torch.isnan(logit[valid]).any()) else float(q.max()) * rd.bound("logit"),
             rd.bound("logit"))
    pb = prob_band(s_g, b_g, 4.0 * rd.ORACLE["prob_eps"] * U)
    pe = torch.where(valid, (prob.double() - torch.sigmoid(s_g)).abs() / pb, torch.zeros_like(err))
    fig.note(f"{tag} prob error / band", float(pe.max()), 1.0)
    fig.exact(f"{tag} only candidates, each once", bool(cand.gather(1, safe)[valid].all())
              and bool(((torch.sort(torch.where(valid, idx, -1 - pos), 1).values.diff(dim=1)) != 0).all()))
    both = valid[:, 1:] & valid[:, :-1]
    down = (logit[:, :-1] > logit[:, 1:]) | ((logit[:, :-1] == logit[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))
    fig.exact(f"{tag} sorted: larger logit first, equal logits by index", bool(down[both].all()))
    same_set = (torch.sort(idx, 1).values == torch.sort(ref, 1).values).all(1)
    fig.exact(f"{tag} the reference's set in the {int(decisive.sum())} of {Q} rows the bands decide", bool(same_set[decisive].all()))
    for row in torch.nonzero(decisive & ~same_set)[:, 0].tolist()[:4]:       # what differs, for the record
        got, want = set(idx[row].tolist()), set(ref[row].tolist())
        for what, vs in (("missing", sorted(want - got)), ("extra", sorted(got - want))):
            for w in vs[:4]:
                where = (idx[row] == w).nonzero()
                lg = float(logit[row, int(where[0])]) if where.numel() else float("nan")
                print(f"DETAIL {tag} row {row} query {int(view['queries'][row])} twins {twins}: {what} {w}, s = {float(s[row, w])!r}, "
                      f"band = {float(band[row, w]):.3g}, returned logit = {lg!r}, candidate = {bool(cand[row, w])}")
    order, alone, _cut = rd.separation(s, band, cand)
    kk = min(k, N)
    at = alone[:, :kk] & valid[:, :kk]
    fig.exact(f"{tag} the reference's candidate at the {int(at.sum())} positions whose band stands alone", bool((idx[:, :kk] == order[:, :kk])[at].all()))
    inf = float("inf")
    for row in torch.nonzero(~decisive)[:, 0].tolist():                       # the band rule of test_gpu_rank.assert_valid_topk
        m = int(n[row])
        if m == 0:
            continue
        got = idx[row, :m]
        vals = torch.where(cand[row], s[row], torch.full_like(s[row], -inf))
        kth = torch.argsort(vals, descending=True)[m - 1]
        ok = bool((s[row, got] + band[row, got] >= vals[kth] - band[row, kth]).all())
        low = got[torch.argmin(s[row, got])]
        rest = cand[row].clone()
        rest[got] = False
        ok = ok and bool((s[row][rest] - band[row][rest] <= s[row, low] + band[row, low]).all())
        fig.exact(f"{tag} row {row}: a valid top-k under the band rule", ok)
    if twins is not None:                                                     # exact copies: adjacent, equal bits, index order
        ia, ib = (idx == twins[0]), (idx == twins[1])
        rows = ia.any(1) & ib.any(1)
        pa, pb_ = ia.double().argmax(1)[rows], ib.double().argmax(1)[rows]
        la, lb = logit[rows].gather(1, pa[:, None]), logit[rows].gather(1, pb_[:, None])
        between = all(bool((logit[r, a:b + 1] == logit[r, a]).all())             # apart only where others tie with them
                      for r, a, b in zip(torch.nonzero(rows)[:, 0].tolist(), pa.tolist(), pb_.tolist()) if b != a + 1)
        fig.exact(f"{tag} the copies come in index order with equal bits ({int(rows.sum())} rows)", bool((pb_ > pa).all()) and _same(la, lb) and between)
    return decisive


@pytest.mark.parametrize("case", rd.rank_cases(), ids=rd.case_id)
def test_ranking_matches_fp64(case, lib_env):
    from disenlink_amd import ops
    _load()
    c = case
    fig = Figures(c.name)
    for k in rd.TOPK:
        rd.rank_form(c, k, lib_env)
    base, decided = {}, {}
    zero_row = rd.special_rows(c.N)[0]
    for order in (rd.ORDERS if c.orders else rd.ORDERS[:1]):
        v = rd.rank_view(c, order)
        Z, H, queries = v["Z"].to(DEV), v["H"].to(DEV), v["queries"].to(DEV)
        exclude = None if v["exclude"] is None else tuple(x.to(DEV) for x in v["exclude"])
        for k in rd.TOPK:
            tag = f"{order} k={k}"
            if order != "as drawn":
                # The same (index, logit bits) after undoing the permutation, under the library's own slicing and under
                # every forced one: with several tiles per slice the pivot query's list is compacted every round, 64 new
                # keys merged into a full sorted prefix (ascending) or none of them kept (descending).
                bi, bl, _bp = base[k]
                distinct = torch.ones_like(bi, dtype=torch.bool)
                distinct[:, 1:] &= bl[:, 1:] != bl[:, :-1]
                distinct[:, :-1] &= bl[:, 1:] != bl[:, :-1]
                last = (bi >= 0).sum(1) - 1                                   # the last entry may tie with what lies beyond
                rows = torch.nonzero((last >= 0) & ~decided[k])[:, 0]
                distinct[rows, last[rows]] = False
                for forced in (None,) + c.slices:
                    f = rd.rank_form(c, k, lib_env, forced)
                    lib_env("DL_RANK_SLICES", forced)
                    idx, logit, _prob = (x.cpu() for x in ops.score_topk(Z, H, c.t, queries, k, exclude=exclude))
                    lib_env("DL_RANK_SLICES")
                    how = f"{tag} DL_RANK_SLICES={forced} ({f['slices']} x {f['tiles_per_slice']}, last {f['last_tiles']})"
                    orig = torch.where(idx >= 0, v["perm"][idx.clamp(min=0)], idx)
                    fig.exact(f"{how} the logit bits of the order as drawn", _same(logit, bl))
                    fig.exact(f"{how} the indices of the order as drawn wherever the logit is distinct", bool((orig == bi)[distinct & (bi >= 0)].all()))
                continue
            idx, logit, prob = (x.cpu() for x in ops.score_topk(Z, H, c.t, queries, k, exclude=exclude))
            base[k] = (idx, logit, prob)
            decided[k] = _check_topk(fig, tag, v, k, idx, logit, prob)
            again = ops.score_topk(Z, H, c.t, queries, k, exclude=exclude)
            fig.exact(f"{tag} bitwise repeatable", _same(again[0].cpu(), idx) and _same(again[1].cpu(), logit))
            for forced in c.slices:                     # every forced slice count gives the bits of the library's own choice
                f = rd.rank_form(c, k, lib_env, forced)
                lib_env("DL_RANK_SLICES", forced)
                out = ops.score_topk(Z, H, c.t, queries, k, exclude=exclude)
                lib_env("DL_RANK_SLICES")
                fig.exact(f"{tag} DL_RANK_SLICES={forced} ({f['slices']} x {f['tiles_per_slice']}, last {f['last_tiles']}) the same bits",
                          _same(out[0].cpu(), idx) and _same(out[1].cpu(), logit))
        if order != "as drawn":
            continue
        # ---- the claims of dl_tiles.h / dl_score_rank.hip: the scan forms the dense scorer's bits (query as the A operand)
        if c.d % 32 == 0:
            P = ops.score_allpairs_fwd(Z, H, c.t).cpu()
            idx, logit, prob = base[rd.TOPK[-1]]
            qn = v["queries"][:, None].expand_as(idx)
            ok = idx >= 0
            Pq = P[qn[ok], idx[ok]]
            up = (qn < idx)[ok]
            fig.exact(f"sigmoid(scan logit) == P[query, candidate] bit for bit, query < candidate ({int(up.sum())} pairs)",
                      _same(prob[ok][up], Pq[up]))
            s_g, b_g = v["s"].gather(1, idx.clamp(min=0))[ok], v["band"].gather(1, idx.clamp(min=0))[ok]
            pb = prob_band(s_g, b_g, 4.0 * rd.ORACLE["prob_eps"] * U)
            diff = ((prob[ok].double() - Pq.double()).abs() / (2.0 * pb))[~up]
            fig.note(f"|sigmoid(scan logit) - P| / (two bands), query > candidate ({int((~up).sum())} pairs)", float(diff.max()) if diff.numel() else 0.0, 1.0)
        # ---- ranks of the targets the builder chose from the reference
        src, dst, greater, ties, n_twin = rd.rank_targets(c)
        if src.numel():
            for forced in (None,) + c.slices:
                lib_env("DL_RANK_SLICES", forced)
                g, ti = ops.score_ranks(Z, H, c.t, src.to(DEV), dst.to(DEV), exclude=exclude)
                lib_env("DL_RANK_SLICES")
                fig.exact(f"ranks DL_RANK_SLICES={forced}: greater of {src.numel()} targets exactly the reference's", torch.equal(g.cpu(), greater))
                fig.exact(f"ranks DL_RANK_SLICES={forced}: ties exactly the reference's ({n_twin} query nodes aimed at the copies)", torch.equal(ti.cpu(), ties))
    fig.close()
