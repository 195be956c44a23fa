"""The host side of the reconstruction loss under a node-group rule (recon.recon_sets(..., node_filter=...), the refusals,
the training loop's and the CLI's switches), against the fp64 restatement with every denied pair ignored
(tests/recon_filter_ref.py).  No GPU."""
import inspect

import pytest
import torch

import recon_filter_ref as rf
import recon_ref


@pytest.mark.parametrize("rule", rf.RULES)
@pytest.mark.parametrize("N", [2, 37, 129, 300])
def test_counts_and_normalised_sets_under_a_rule(N, rule):
    from disenlink_amd import ops
    pos, ign = recon_ref.pair_sets(N, seed=N)
    nf = rf.make_rule(rule, N)
    A = rf.allowed_matrix(nf)
    assert torch.equal(A, A.t())
    if rule == "only63":
        assert nf.n_groups == 64 and int(nf._pair_words[63]) < 0 and not bool(nf._pair_words[:63].any())     # bit 63 alone
    Z = torch.zeros(N, 1, 1)
    want = recon_ref.recon64(Z, Z, 1.0, pos, ign | ~A)["counts"]
    sets = ops.recon_sets(pos, ign, N, "cpu", node_filter=nf)
    assert (sets.n_pos, sets.n_neg) == want, (sets.n_pos, sets.n_neg, want)
    assert sets.node_filter is nf and sets.n_nodes == N
    if rule == "deny":
        assert want == (0, 0) and ops.recon_weights(sets) == (0.0, 0.0)
    elif N >= 37:
        assert want[0] > 0 and want[1] > 0                              # the rule leaves something of both kinds
    eye = torch.eye(N, dtype=torch.bool)
    got_pos, got_ign = rf.pairs_of(sets.pos_rowptr, sets.pos_col), rf.pairs_of(sets.ign_rowptr, sets.ign_col)
    assert got_pos == {(u, v) for u, v in (pos & ~ign & A & ~eye).nonzero().tolist()}
    assert got_ign == {(u, v) for u, v in (ign & A & ~eye).nonzero().tolist()}
    assert sets.n_ignored == len(got_ign) // 2
    assert not any(not A[u, v] for u, v in got_pos | got_ign)          # no denied pair in either CSR
    for rp, c in ((sets.pos_rowptr, sets.pos_col), (sets.ign_rowptr, sets.ign_col)):      # the kernels' form
        if rp is not None:
            assert rp.dtype == torch.int32 and c.dtype == torch.int32 and rp.numel() == N + 1
            r = rp.tolist()
            assert all(c[r[u]:r[u + 1]].tolist() == sorted(set(c[r[u]:r[u + 1]].tolist())) for u in range(N))
    w_pos, w_neg = ops.recon_weights(sets)
    if want[0] and want[1]:                                             # the default pos_weight is that of the filtered counts
        assert w_neg == 1.0 / sum(want) and w_pos == (want[1] / want[0]) / sum(want)


def test_without_a_rule_the_sets_are_what_they_were():
    from disenlink_amd import ops
    N = 129
    pos, ign = recon_ref.pair_sets(N, seed=N)
    a, b = ops.recon_sets(pos, ign, N, "cpu"), ops.recon_sets(pos, ign, N, "cpu", node_filter=rf.make_rule("all", N))
    assert a.node_filter is None and ops.ReconSets(*a[:8]).node_filter is None    # positional construction as before the field
    for x, y in zip(a[:8], b[:8]):
        assert torch.equal(x, y) if torch.is_tensor(x) else x == y
    assert a.n_neg == N * (N - 1) // 2 - a.n_ignored - a.n_pos
    assert ops.ReconSets._fields[-1] == "node_filter" and len(ops.ReconSets._fields) == 9


def test_refusals():
    from disenlink_amd import ops, recon
    from disenlink_amd.model import Disentangle
    N = 37
    pos, ign = recon_ref.pair_sets(N, seed=N)
    asym = ops.NodeFilter(torch.arange(N) % 2, torch.tensor([[False, True], [False, False]]))
    with pytest.raises(ValueError, match="symmetric"):
        ops.recon_sets(pos, ign, N, "cpu", node_filter=asym)
    with pytest.raises(ValueError, match=f"node filter of {N + 1} nodes"):
        ops.recon_sets(pos, ign, N, "cpu", node_filter=rf.make_rule("same3", N + 1))
    with pytest.raises(TypeError, match="NodeFilter"):
        ops.recon_sets(pos, ign, N, "cpu", node_filter=torch.arange(N) % 2)
    with pytest.raises(ValueError, match="use NodeFilter.to"):                   # the filter's device against the sets'
        ops.recon_sets(pos, ign, N, "cpu", node_filter=rf.make_rule("same3", N).to("meta"))
    nf, other = rf.make_rule("same3", N), rf.make_rule("same3", N)
    sets = ops.recon_sets(pos, ign, N, "cpu", node_filter=nf)
    Z = torch.zeros(N, 2, 8)
    for call in (ops.score_recon_loss, ops.score_recon_logits_loss):
        with pytest.raises(ValueError, match="carry their node filter"):          # a second filter beside prepared sets
            call(Z, Z, 1.0, sets, node_filter=other)
        with pytest.raises(ValueError, match="symmetric"):                       # ahead of the tables' own refusals
            call(Z, Z, 1.0, pos, ign, node_filter=asym)
        with pytest.raises(ValueError, match=f"node filter of {N + 1} nodes"):
            call(Z, Z, 1.0, pos, ign, node_filter=rf.make_rule("same3", N + 1))
        with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):  # the sets' own filter passes this check
            call(Z, Z, 1.0, sets, node_filter=nf)
    with pytest.raises(ValueError, match="carry their node filter"):
        recon._sets_arg(ops.recon_sets(pos, ign, N, "cpu"), None, N, torch.device("cpu"), other)
    assert recon._sets_arg(sets, None, N, torch.device("cpu"), nf) is sets and recon._sets_arg(sets, None, N, torch.device("cpu")) is sets
    model = Disentangle(4, 4, 8, nfactor=2, beta=0.5, t=1)
    for fwd in (model.forward_recon_loss, model.forward_recon_logits_loss):
        assert inspect.signature(fwd).parameters["node_filter"].default is None
        with pytest.raises(ValueError, match="carry their node filter"):
            fwd(torch.zeros(N, 4), None, sets, node_filter=other)


def test_training_loop_and_cli_switches(tmp_path):
    from test_recon_cpu import _Recorder, _tiny_run
    from disenlink_amd import ops, train
    from disenlink_amd.main import build_parser, main
    sg, run = _tiny_run()
    N = sg.n_nodes
    nf = ops.NodeFilter.different(torch.arange(N) % 2)
    x = torch.zeros(N, 4)
    assert inspect.signature(train.run_link_prediction).parameters["recon_node_filter"].default is None
    for objective in ("pairs", "pairs-logit"):
        with pytest.raises(ValueError, match="recon_node_filter"):
            train.run_link_prediction(_Recorder(), x, run, objective=objective, recon_node_filter=nf)
    seen = {}

    class Probe(_Recorder):
        def forward_recon_loss(self, x, graph, ignore=None, pos_weight=None, block_rows=None):
            seen.update(sets=ignore)
            raise self.Stop
    with pytest.raises(_Recorder.Stop):
        train.run_link_prediction(Probe(), x, run, epochs=1, objective="recon", recon_node_filter=nf)
    s = seen["sets"]
    assert isinstance(s, ops.ReconSets) and s.node_filter is nf
    A = rf.allowed_matrix(nf)
    assert all(A[u, v] for u, v in rf.pairs_of(s.pos_rowptr, s.pos_col) | rf.pairs_of(s.ign_rowptr, s.ign_col))
    assert s.n_pos + s.n_neg + s.n_ignored == int(torch.triu(A, 1).sum())
    with pytest.raises(_Recorder.Stop):                               # without it: the loop's sets as they were
        train.run_link_prediction(Probe(), x, run, epochs=1, objective="recon")
    assert seen["sets"].node_filter is None

    assert build_parser().parse_known_args([])[0].recon_link_rule is False
    groups = tmp_path / "groups.txt"
    groups.write_text("\n".join(str(i % 2) for i in range(N)))
    base = ["--synthetic", "--no-cuda"]
    rule = ["--node-groups", str(groups), "--link-rule", "different"]
    with pytest.raises(SystemExit, match="--recon-link-rule puts the rule"):      # without --link-rule
        main(base + ["--objective", "recon", "--recon-link-rule"])
    with pytest.raises(SystemExit, match="--objective recon or recon-logit"):     # with another objective
        main(base + rule + ["--objective", "pairs", "--recon-link-rule"])
    with pytest.raises(SystemExit, match="--objective recon or recon-logit"):
        main(base + rule + ["--recon-link-rule"])
    with pytest.raises(SystemExit, match="give one of them"):                     # the rule still needs something to restrict
        main(base + rule + ["--objective", "recon"])
    with pytest.raises(SystemExit, match="GPU only"):                             # accepted: the run itself needs the GPU
        main(base + rule + ["--objective", "recon", "--recon-link-rule"])


def test_header_and_binding_list_the_filtered_entries():
    import test_host_cpu
    from disenlink_amd import _lib
    names = test_host_cpu._declared_symbols()
    for n in ("dl_score_recon_filtered", "dl_score_recon_logits_filtered"):
        assert n in names and n in _lib.EXPORTS and hasattr(_lib.load(), n)
        assert _lib.EXPORTS[n][1] == _lib.EXPORTS["dl_score_recon_dtype"][1] + [_lib._NF]
    assert set(_lib.EXPORTS) == set(names)


def test_c_abi_refuses_a_bad_filter_before_any_launch():
    """n_groups outside 1..64 and a NULL member: the code and the words of the other _filtered entries; arguments that the
    unfiltered entry refuses are still refused first (host checks only: no GPU is needed to be refused)."""
    import ctypes as C
    from disenlink_amd import _lib
    lib = _lib.load()
    p = 256

    def call(entry, nf, **kw):
        a = dict(N=8, K=2, d=8, t=1.0)
        a.update(kw)
        return getattr(lib, entry)(p, p, a["N"], a["K"], a["d"], _lib.DL_F32, a["t"], p, p, None, None, 0.5, 0.5, 0, p, p, p, p, p,
                                   1 << 30, None, nf)
    for entry in ("dl_score_recon_filtered", "dl_score_recon_logits_filtered"):
        for n_groups in (0, 65, -1):
            assert call(entry, C.byref(_lib.DlNodeFilter(p, n_groups, p))) == -1
            assert f"node filter: n_groups={n_groups} outside 1..64".encode() in lib.dl_last_error()
        for f in (_lib.DlNodeFilter(None, 2, p), _lib.DlNodeFilter(p, 2, None)):
            assert call(entry, C.byref(f)) == -1 and b"node filter: NULL group or allow array" in lib.dl_last_error()
        assert call(entry, C.byref(_lib.DlNodeFilter(p, 0, p)), t=0.0) == -1 and b"temperature" in lib.dl_last_error()


def test_module_fixtures_stay_unsaturated_under_the_rule():
    """The rule of the GPU module test (recon_filter_ref.MODULE_RULE) on recon_ref.MODULE_CASES: a plain fp32 CPU evaluation of
    the dense formulation stays within a quarter of the GPU test's tolerance of the fp64 one, test_recon_cpu's rule for
    choosing the cases, and the rule leaves pairs of both kinds."""
    from conftest import load_golden
    for name in recon_ref.MODULE_CASES:
        g = load_golden(name)
        A = rf.allowed_matrix(rf.make_rule(rf.MODULE_RULE, g["meta"]["N"]))
        l64, g64, _ign, n, s64 = rf.module_reference(g, A, torch.float64)
        l32, g32, _ign, n32, s32 = rf.module_reference(g, A, torch.float32)
        _l, _g, _i, n_all, _s = recon_ref.module_reference(g, torch.float64)
        worst = max(float((g32[k] - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-6) for k in g64)
        print(f"{name} under {rf.MODULE_RULE}: counts {n} of {n_all}  fp32 against fp64  loss {abs(l32 - l64) / max(1.0, abs(l64)):.1e}  "
              f"gradients {worst:.1e}  saturated {s32}")
        assert n == n32 and 0 < n[0] < n_all[0] and 0 < n[1] < n_all[1]
        assert worst <= recon_ref.MODULE_TOL / 4 and abs(l32 - l64) <= 5e-6 * max(1.0, abs(l64)) and s32 == 0 and s64 == 0
