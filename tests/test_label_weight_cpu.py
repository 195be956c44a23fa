"""tests/label_weight_ref.py without a GPU: the recipes meet the conditions they are built for, and the fp32 restatements of the
training step and of the loss kernels are measured against fp64 again — the figures the GPU bounds of
tests/test_gpu_label_weight.py are 4x of."""
import numpy as np
import pytest
import torch

import label_weight_ref as lw
import logit_ref
import ref64

SLACK = ref64.CPU_SLACK              # for re-measuring on this host; the GPU bounds do not contain it
SOFT_SIGNED = ("soft", "signed")


def _lib():
    from disenlink_amd import _lib
    return _lib.load()


def _step_cases():
    """(case, combo): the B1 shapes with every combination, every other tuned shape (and the generic one) with (soft, signed)."""
    lib = _lib()
    b1 = lw.b1_cases(lib)
    out = [(c, combo) for c in b1 for combo in lw.COMBOS]
    return out + [(c, SOFT_SIGNED) for c in logit_ref.cases(lib) if c not in b1]


def _id(v):
    return logit_ref.case_id(v) if isinstance(v, logit_ref.Case) else lw.combo_id(v)


def _bits(x):
    return x.contiguous().view(torch.int32)


def test_recipes_are_fp32_exact_deterministic_and_hold_what_they_promise():
    st = ref64.structure()
    P = st.pu.numel()
    base = ref64.reference(8, 64, "f32", 1.0, ref64.BETAS[0])
    seed = base["seed"]
    y0, w0 = lw.base_draw(P, seed)
    assert torch.equal(y0.double(), base["label"]) and torch.equal(w0.double(), base["weight"])     # "the existing draw"
    for combo in [(a, b) for a in lw.LABELS for b in lw.WEIGHTS]:
        y, w = lw.labels_weights(combo, P, seed)
        y2, w2 = lw.labels_weights(combo, P, seed)
        assert y.dtype == w.dtype == torch.float32 and y.numel() == w.numel() == P      # fp32 tensors: fp32-exact as they stand
        assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(w), _bits(w2))
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(w).all())
        assert float(y.min()) >= 0 and float(y.max()) <= 1
    sign = lambda w: torch.signbit(w)
    # signed: the magnitudes of the existing draw; P // 16 each of negative, +0.0 and -0.0 at the least
    w = lw.make_weights("signed", w0, seed)
    assert torch.equal(w.abs(), w0)
    assert int((w < 0).sum()) >= P // 16 and int(((w == 0) & ~sign(w)).sum()) >= P // 16 and int(((w == 0) & sign(w)).sum()) >= P // 16
    assert int((w < 0).sum()) == int((w0 != 0).sum()) // 3 and int((w > 0).sum()) > P // 2
    # negzero: the zeros carry the sign bit, every other bit of the draw is untouched
    w = lw.make_weights("negzero", w0, seed)
    assert torch.equal(w, w0) and bool((sign(w) == (w0 == 0)).all()) and int((w0 == 0).sum()) == P // 8
    # wide: positive over thirty binades
    w = lw.make_weights("wide", w0, seed)
    assert float(w.min()) >= 2.0 ** -20 and float(w.max()) <= 2.0 ** 10 and float(w.max() / w.min()) > 2.0 ** 25
    # soft: exact ends and a strict inside; smoothed: the binary draw at 0.05 / 0.95; half
    y = lw.make_labels("soft", y0, seed)
    assert int((y == 0).sum()) == P // 16 and int((y == 1).sum()) == P // 16 and int(((y > 0) & (y < 1)).sum()) == P - 2 * (P // 16)
    y = lw.make_labels("smoothed", y0, seed)
    assert bool(((y == np.float32(0.95)) == (y0 == 1)).all()) and bool(((y == np.float32(0.05)) == (y0 == 0)).all())
    assert bool((lw.make_labels("half", y0, seed) == 0.5).all())
    # the loss-kernel inputs: the same recipes over bce_inputs' own draw
    for n in logit_ref.BCE_SIZES:
        x, y, w = lw.bce_case(n, SOFT_SIGNED)
        x0, _y0, w0n = logit_ref.bce_inputs(n)
        assert torch.equal(x, x0) and torch.equal(w.abs(), w0n) and y.numel() == w.numel() == n
    assert int((lw.bce_case(10004, SOFT_SIGNED)[2] < 0).sum()) > 2000


def test_row_ratio_with_its_own_scales_is_ref64s_and_negzero_changes_nothing_in_fp64():
    case = lw.b1_cases(_lib())[0]
    r = lw.reference(*case[:5], ("binary", "negzero"))
    base = ref64.reference(*case[:5])
    for space in lw.SPACES:
        s = r[space]
        assert lw.row_ratio(s["dZ32"], s["dZ"], s["dZ"]) == ref64.row_ratio(s["dZ32"], s["dZ"])
        assert torch.equal(s["dZ"], s["dZ_abs"]) and torch.equal(s["dH"], s["dH_abs"])
    # (binary, negzero) is ref64.reference's own training step: the same fp64 gradients, bit for bit
    assert torch.equal(r["prob"]["dZ"], base["dZ_train"]) and torch.equal(r["prob"]["dH"], base["dH_train"])
    lr = logit_ref.reference(*case[:5])
    assert torch.equal(r["logit"]["dZ"], lr["dZ"]) and torch.equal(r["logit"]["dH"], lr["dH"])
    # under `signed` the |w| scales differ from the gradient's own and are what the measure uses
    r = lw.reference(*case[:5], SOFT_SIGNED)
    assert not torch.equal(r["prob"]["dZ"], r["prob"]["dZ_abs"])
    assert bool(torch.isfinite(r["prob"]["dZ"]).all()) and bool(torch.isfinite(r["logit"]["dZ"]).all())


@pytest.mark.parametrize("case,combo", _step_cases(), ids=_id)
def test_fp32_restatement_of_the_step_stays_within_its_recorded_error(case, combo):
    r = lw.reference(*case[:5], combo)
    for space in lw.SPACES:
        err = lw.restatement_figures(r, space)
        print("\nCALIBRATION", space, logit_ref.case_id(case), lw.combo_id(combo), {k: f"{v:.3g}" for k, v in err.items()})
        for k, v in err.items():
            assert v <= SLACK * lw.FP32[space][k], (space, k, v, lw.FP32[space][k])
    # the restatement's scores lie in the bands the GPU test holds the kernels' scores to
    assert ref64.band_ratio(r["logit"]["score32"], r["x"], r["x_abs"]) <= ref64.BOUND["logit"]
    band = ref64.prob_band(r["x"], ref64.BOUND["logit"] * ref64.U * r["x_abs"], ref64.BOUND["prob_eps"] * ref64.U)
    assert float(((r["prob"]["score32"].double() - torch.sigmoid(r["x"])).abs() / band).max()) <= 1.0
    # weights of +-0.0 are no part of any reference gradient coefficient
    dead = r["w"] == 0
    assert bool((r["prob"]["g32"][dead] == 0).all()) and bool((r["logit"]["g32"][dead] == 0).all())


def test_fp32_restatement_of_the_loss_kernels_stays_within_its_recorded_error():
    worst = {space: {"loss": 0.0, "g": 0.0} for space in lw.SPACES}
    for n in logit_ref.BCE_SIZES:
        for combo in lw.COMBOS:
            for space in lw.SPACES:
                s, y, w = lw.loss_kernel_inputs(space, n, combo)
                loss, g = lw.bce_prob32(s, y, w) if space == "prob" else logit_ref.bce32(s, y, w)
                fig = lw.loss_kernel_figures(space, s, y, w, loss, g)
                worst[space] = {k: max(worst[space][k], fig[k]) for k in fig}
                if space == "prob" and n >= 1023:
                    assert int((s == 0).sum()) >= 1 and int((s == 1).sum()) >= 1
    print("\nCALIBRATION loss kernels", worst)
    for space in lw.SPACES:
        for k, v in worst[space].items():
            assert v <= SLACK * lw.FP32[space + "_kernel"][k], (space, k, v)


def test_a_weight_tensor_with_a_set_sign_bit_is_never_bound():
    """PairList.bind_labels: the stream's weight sign is its writer flag, so it is built for weights >= +0.0 only — `signed` and
    `negzero` keep the gathers at every sight, `positive` and `wide` are bound at the second, and the bound stream reproduces the
    caller's weights with one writing entry (clear sign bit) per pair."""
    st = ref64.structure()
    P = st.pu.numel()
    from disenlink_amd.graph import PairList
    for name in lw.WEIGHTS:
        pl = PairList.build(st.pu, st.pv, ref64.N_NODES, build_by_u=False)
        y, w = lw.labels_weights(("soft", name), P, 11)
        for sight in range(3):
            pl.bind_labels(y, w, P)
            assert (pl._yw is not None) == (sight >= 1 and name in ("positive", "wide")), (name, sight)
        if pl._yw is not None:
            q = pl.inc_pair.long()
            assert torch.equal(pl._yw[:, 0], y[q]) and torch.equal(pl._yw[:, 1].abs(), w[q])
            writers = torch.zeros(P, dtype=torch.long).index_add_(0, q, (~torch.signbit(pl._yw[:, 1])).long())
            self_pair = st.pu == st.pv                                # both entries of a self pair sit in the writing row
            assert bool((writers[~self_pair] == 1).all()) and bool((writers[self_pair] == 2).all())
        w.neg_()                                                      # a new version of the same tensor is judged afresh
        for sight in range(2):
            pl.bind_labels(y, w, P)
        assert pl._yw is None                                         # every recipe negated holds a set sign bit
    assert not pl.static_labels


def test_bounds_are_four_times_the_recorded_figures():
    for k, d in lw.FP32.items():
        assert all(v > 0 for v in d.values()), k
        assert lw.BOUND[k] == {m: 4.0 * v for m, v in d.items()}
