"""The pair-list objective in logit space, without a GPU: the fp32 restatement of tests/logit_ref.py is measured against fp64 again
(the figures the GPU bounds are 4x of), the new C entries stand in the header and in _lib.EXPORTS with matching argument
counts, and the training loop / command line refuse what the objective cannot run."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import logit_ref
import ref64
from conftest import ROOT

SLACK = ref64.CPU_SLACK              # for re-measuring on this host; the GPU bounds do not contain it
NEW_ENTRIES = ("dl_score_pairs_logits_fwd", "dl_score_pairs_logits_bwd", "dl_score_pairs_train_logits_supported",
               "dl_score_pairs_train_logits", "dl_pair_bce_logits")


def _cases():
    from disenlink_amd import _lib
    return logit_ref.cases(_lib.load())


def test_cases_cover_every_tuned_shape_at_both_temperatures_and_one_generic_shape():
    from disenlink_amd import _lib
    lib = _lib.load()
    cases = _cases()
    for dtype in ("f32", "bf16"):
        for K, d in ref64.tuned_shapes(lib, dtype):
            assert {c.t for c in cases if (c.K, c.d, c.dtype) == (K, d, dtype) and not c.generic} == {1.0, 2.0}
    assert {(c.K, c.d, c.t) for c in cases if c.generic} == {(3, 16, 1.0), (3, 16, 2.0)}
    assert not lib.dl_has_fast_path_dtype(3, 16, _lib.DL_F32)


@pytest.mark.parametrize("case", _cases(), ids=logit_ref.case_id)
def test_fp32_restatement_of_the_step_stays_within_its_recorded_error(case):
    r = logit_ref.reference(case.K, case.d, case.dtype, case.t, case.beta)
    err = {"dZ": ref64.row_ratio(r["dZ32"], r["dZ"]), "dH": ref64.row_ratio(r["dH32"], r["dH"]),
           "loss": logit_ref.rel_err(r["loss32"], r["loss"])}
    print("\nCALIBRATION", logit_ref.case_id(case), {k: f"{v:.3g}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= SLACK * logit_ref.FP32[k], (k, v, logit_ref.FP32[k])
    # the fp64 step is what it says it is: g = w (sigma(x) - y), written with both sides of the sigmoid; weight 0 = nothing
    assert torch.allclose(r["g"], logit_ref.g64(r["x"], r["label"], r["weight"]), rtol=1e-12, atol=1e-300)
    assert bool((r["g"][r["weight"] == 0] == 0).all()) and int((r["weight"] == 0).sum()) > 0
    # the fp32 logits lie in the band the forward test holds the kernels to
    assert ref64.band_ratio(r["x32"], r["x"], r["x_abs"]) <= ref64.BOUND["logit"]


def test_fp32_restatement_of_the_loss_kernel_stays_within_its_recorded_error():
    worst = {"loss_kernel": 0.0, "g": 0.0}
    for n in logit_ref.BCE_SIZES:
        x, y, w = logit_ref.bce_inputs(n)
        loss, g = logit_ref.bce32(x, y, w)
        ref = logit_ref.pair_loss64(x.double(), y.double(), w.double()).sum()
        worst["loss_kernel"] = max(worst["loss_kernel"], logit_ref.rel_err(loss, ref))
        worst["g"] = max(worst["g"], logit_ref.g_ratio(g, logit_ref.g64(x.double(), y.double(), w.double()), w))
    print("\nCALIBRATION loss kernel", worst)
    for k, v in worst.items():
        assert v <= SLACK * logit_ref.FP32[k], (k, v, logit_ref.FP32[k])


def test_fp64_loss_is_the_issues_formula_and_keeps_the_small_side():
    x = torch.tensor([-150.0, -35.0, -3.0, 0.25, 3.0, 35.0, 150.0], dtype=torch.float64)
    for y in (0.0, 1.0):
        yy, w = torch.full_like(x, y), torch.ones_like(x)
        want = x.clamp(min=0) - x * yy + torch.log1p(torch.exp(-x.abs()))
        assert torch.allclose(logit_ref.pair_loss64(x, yy, w), want, rtol=1e-13, atol=0)
        g = logit_ref.g64(x, yy, w)
        assert bool((g != 0).all())                              # sigma(35) - 1 = -6.3e-16 is kept, not rounded to 0
        small = -torch.exp(-x) / (1 + torch.exp(-x)) if y == 1.0 else torch.exp(x) / (1 + torch.exp(x))
        assert torch.allclose(g, small, rtol=1e-12, atol=0)
    # and the fp32 form the kernels use keeps it too
    g32 = logit_ref.sigmoid_minus_label32(torch.tensor([35.0, -35.0]), torch.tensor([1.0, 0.0]))
    assert torch.allclose(g32.double(), torch.tensor([-6.305116760146989e-16, 6.305116760146989e-16], dtype=torch.float64), rtol=1e-6, atol=0)


def test_saturated_list_meets_the_conditions_it_is_built_for():
    s = logit_ref.saturated()
    P = s["x"].numel()
    assert int(s["sat"].sum()) * 3 >= P and s["arg_max"] < 80
    assert s["wrong"].numel() * 2 in (int(s["sat"].sum()), int(s["sat"].sum()) + 1)
    x, y = s["x"], s["label"]
    assert bool(((x[s["wrong"]] > 0) == (y[s["wrong"]] == 0)).all())        # wrong = label against the sign
    assert s["dead"].numel() >= 8
    p32 = ref64.sigmoid32(x)
    st = ref64.structure()
    for node in s["dead"].tolist():
        mine = (st.pu == node) | (st.pv == node)
        assert bool(((p32[mine] == 0) | (p32[mine] == 1)).all())


# ---------------------------------------------------------------------------------------------- header and EXPORTS
def _prototypes():
    text = open(os.path.join(ROOT, "include", "disenlink_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(dl_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def test_new_entries_stand_in_the_header_and_in_exports_with_matching_argument_counts():
    from disenlink_amd import _lib
    protos = _prototypes()
    for name in NEW_ENTRIES:
        assert name in protos, f"{name} is not declared in include/disenlink_hip.h"
        assert name in _lib.EXPORTS, f"{name} has no ctypes signature in _lib.EXPORTS"
        n_args = len([a for a in protos[name].split(",") if a.strip() and a.strip() != "void"])
        assert n_args == len(_lib.EXPORTS[name][1]), (name, n_args, len(_lib.EXPORTS[name][1]))
        assert hasattr(_lib.load(), name)
    # each logit entry takes what its probability twin takes, minus what logit space has no use for
    n = lambda e: len(_lib.EXPORTS[e][1])
    assert n("dl_score_pairs_logits_fwd") == n("dl_score_pairs_fwd") - 1            # no coef
    assert n("dl_score_pairs_logits_bwd") == n("dl_score_pairs_bwd") - 2            # no prob, no coef
    assert _lib.EXPORTS["dl_score_pairs_train_logits"] == _lib.EXPORTS["dl_score_pairs_train"]
    assert _lib.EXPORTS["dl_score_pairs_train_logits_supported"] == _lib.EXPORTS["dl_score_pairs_train_supported"]
    assert _lib.EXPORTS["dl_pair_bce_logits"] == _lib.EXPORTS["dl_pair_bce"]


def test_new_entries_report_argument_errors_without_a_gpu():
    import ctypes as C
    from disenlink_amd import _lib
    lib = _lib.load()
    inc = _lib.DlPairIncidence()
    assert lib.dl_score_pairs_train_logits_supported(None, 8, 64, _lib.DL_F32) == 0
    rc = lib.dl_score_pairs_train_logits(None, None, 8, 64, _lib.DL_F32, 1.0, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"incidence is NULL" in lib.dl_last_error()
    rc = lib.dl_score_pairs_train_logits(None, None, 3, 16, _lib.DL_F32, 1.0, C.byref(inc), None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"dl_score_pairs_train_logits needs a tuned kernel" in lib.dl_last_error()
    rc = lib.dl_score_pairs_logits_bwd(None, None, 8, 64, _lib.DL_F32, 0.0, C.byref(inc), None, None, None, None, 0, None)
    assert rc == -1 and b"temperature" in lib.dl_last_error()
    rc = lib.dl_score_pairs_logits_fwd(None, None, 4, 8, 64, _lib.DL_F32, 1.0, None, None, 3, None, None, None)
    assert rc == -1 and b"NULL" in lib.dl_last_error()
    rc = lib.dl_pair_bce_logits(None, None, None, 4, None, None, None, 0, None)
    assert rc == -1 and b"loss is NULL" in lib.dl_last_error()
    one = (C.c_float * 1)()
    rc = lib.dl_pair_bce_logits(None, None, None, 4, one, None, None, 0, None)
    assert rc == -1 and b"dl_pair_bce_logits needs >= 4352 bytes" in lib.dl_last_error()


def test_binding_abi_moved_on_both_sides_together():
    from disenlink_amd import native
    src = open(os.path.join(ROOT, "disenlink_amd", "csrc", "torch", "dl_torch.cpp")).read()
    assert int(re.search(r"#define DL_TORCH_BINDING_ABI (\d+)", src).group(1)) == native.BINDING_ABI >= 7
    assert "hot_path_pair_logits_loss" in native._OPS and "hot_path_pair_logits_loss(Tensor Z" in src


# ---------------------------------------------------------------------------------------------- the loop and the command line
def _run(n_pos=3, n_neg=3, n_val=2, n_test=2, labels=None):
    lab = labels or (n_pos, n_neg, n_val, n_test)
    pairs = lambda n: SimpleNamespace(n_pairs=n)
    return SimpleNamespace(graph=None, train_val_pairs=pairs(n_pos + n_neg + n_val), n_pos=n_pos, n_neg=n_neg,
                           label_pos=torch.ones(lab[0]), label_neg=torch.zeros(lab[1]),
                           label_val=torch.tensor([1.0, 0.0] * n_val)[:lab[2]], test_pairs=pairs(n_test),
                           label_test=torch.tensor([1.0, 0.0] * n_test)[:lab[3]], m=1)


class _LogitModel(torch.nn.Module):
    def forward_pair_logits(self, x, graph, pairs):
        raise AssertionError("refused before the first forward")

    forward_pair_logits_loss = forward_pairs = forward_pair_logits


def test_run_link_prediction_refuses_what_the_objective_cannot_run():
    from disenlink_amd import train
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="objective must be"):
        train.run_link_prediction(_LogitModel(), x, _run(), objective="logits")
    with pytest.raises(ValueError, match="label / weight must cover the pair list"):
        train.run_link_prediction(_LogitModel(), x, _run(labels=(3, 2, 2, 2)), objective="pairs-logit")
    with pytest.raises(ValueError, match="label / weight must cover the pair list"):
        train.run_link_prediction(_LogitModel(), x, _run(labels=(3, 3, 2, 1)), objective="pairs-logit")
    with pytest.raises(TypeError, match="forward_pair_logits"):
        train.run_link_prediction(torch.nn.Linear(1, 1), x, _run(), objective="pairs-logit")
    with pytest.raises(ValueError, match="GPU only"):
        train.run_link_prediction(_LogitModel(), x, _run(), objective="pairs-logit")
    with pytest.raises(NotImplementedError, match="one GPU only"):
        train.run_link_prediction_sharded(_LogitModel(), x, None, objective="pairs-logit")
    with pytest.raises(ValueError, match="objective=\"pairs\" only"):
        train.run_link_prediction_sharded(_LogitModel(), x, None, objective="recon")


def test_model_refuses_labels_that_do_not_cover_the_pair_list():
    from disenlink_amd.model import Disentangle
    model = Disentangle(6, 8, 4, nfactor=2, beta=0.5)
    with pytest.raises(ValueError, match="label / weight must cover the pair list"):
        model.forward_pair_logits_loss(torch.zeros(5, 6), None, SimpleNamespace(n_pairs=4), torch.zeros(3), torch.zeros(4))
    with pytest.raises(ValueError, match="label / weight must cover the pair list"):
        model.forward_pair_logits_loss(torch.zeros(5, 6), None, SimpleNamespace(n_pairs=4), torch.zeros(4), torch.zeros(5))


def test_command_line_takes_the_objective_and_refuses_it_sharded():
    from disenlink_amd import main as cli
    args = cli.build_parser().parse_args(["--synthetic", "--objective", "pairs-logit"]) if hasattr(cli, "build_parser") else None
    assert args is None or args.objective == "pairs-logit"
    with pytest.raises(SystemExit, match="pairs-logit runs on one GPU only"):
        cli.main(["--synthetic", "--gpus", "2", "--objective", "pairs-logit"])
    with pytest.raises(SystemExit):                               # argparse: not a choice
        cli.main(["--synthetic", "--objective", "logits"])
