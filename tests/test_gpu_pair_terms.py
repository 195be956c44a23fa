"""The per-factor terms of given pairs (dl_score_pair_terms, ops.score_pair_terms, Disentangle.explain_links, --explain):
every cell against ``ops.score_pair_logits`` on derived tables (tests/terms_ref.py), bit for bit; the consumers' logits; bf16
tables; NULL outputs; repeat calls; overflow; the module and the CLI."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import terms_ref
from terms_ref import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16


def tables(N, K, d, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Z = (torch.randn(N, K, d, generator=g) / d ** 0.5).to(DEV)
    H = (torch.randn(N, K, d, generator=g) / d ** 0.5).to(DEV)
    return Z, H


@functools.lru_cache(maxsize=None)
def run_case(case):
    """the tables, the pairs and the terms of one case: computed once, shared by the three oracle tests, never modified"""
    from disenlink_amd import ops
    N, K, d, t, n_pairs = case
    Z, H = tables(N, K, d, seed=N * 131 + K * 7 + d)
    a, b = (v.to(DEV) for v in terms_ref.case_pairs(N, n_pairs, seed=n_pairs + N))
    terms = ops.score_pair_terms(Z, H, t, a, b)
    assert isinstance(terms, ops.PairTerms)
    for x in terms:
        assert x.shape == (n_pairs, K) and x.dtype == torch.float32 and x.is_contiguous()
    return Z, H, a, b, terms


@pytest.mark.parametrize("case", terms_ref.GPU_CASES)
def test_cum_is_the_logit_of_the_prefix_tables(case):
    from disenlink_amd import ops
    Z, H, a, b, terms = run_case(case)
    t, K = case[3], case[1]
    for k in range(K):
        assert same_bits(terms.cum[:, k], ops.score_pair_logits(*terms_ref.prefix_tables(Z, H, k), t, a, b)), k
    assert same_bits(terms.logit, ops.score_pair_logits(Z, H, t, a, b))
    assert not (terms.logit.view(torch.int32) == -2 ** 31).any()      # -0 is reported as +0


@pytest.mark.parametrize("case", terms_ref.GPU_CASES)
def test_q_is_the_logit_with_z_zeroed(case):
    from disenlink_amd import ops
    Z, H, a, b, terms = run_case(case)
    t, K = case[3], case[1]
    for k in range(K):
        assert same_bits(terms.q[:, k], ops.score_pair_logits(*terms_ref.gram_tables(Z, H, k), t, a, b)), k


@pytest.mark.parametrize("case", terms_ref.GPU_CASES)
def test_e_is_the_logit_with_a_unit_h(case):
    from disenlink_amd import ops
    Z, H, a, b, terms = run_case(case)
    t, K = case[3], case[1]
    for k in range(K):
        assert same_bits(terms.e[:, k], ops.score_pair_logits(*terms_ref.weight_tables(Z, H, k), t, a, b)), k


def test_logit_is_what_the_consumers_report():
    from disenlink_amd import ops
    N, K, d, t = 300, 5, 64, 0.5
    Z, H = tables(N, K, d, seed=5)
    q = torch.arange(N, device=DEV)
    index, logit, _ = ops.score_topk(Z, H, t, q, 10)
    assert (index >= 0).all()
    top = ops.score_pair_terms(Z, H, t, q.repeat_interleave(10), index.reshape(-1))
    assert same_bits(top.logit, logit.reshape(-1))
    src, dst, logit, _ = ops.score_mine(Z, H, t, 50)
    assert len(src) == 50 and same_bits(ops.score_pair_terms(Z, H, t, src, dst).logit, logit)
    rowptr, col, logit, _ = ops.score_links(Z, H, t, float(torch.quantile(top.logit, 0.5)))
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), rowptr[1:] - rowptr[:-1])
    assert 100 < len(col) < N * N
    links = ops.score_pair_terms(Z, H, t, torch.minimum(rows, col.long()), torch.maximum(rows, col.long()))
    assert same_bits(links.logit, logit)


def test_bf16_tables_give_the_bits_of_the_widened_tables():
    from disenlink_amd import ops
    for N, K, d, t, n_pairs in ((129, 2, 33, 1.0, 129), (300, 5, 64, 0.5, 300), (300, 2, 128, 1.0, 127)):
        Z, H = tables(N, K, d, seed=d)
        a, b = (v.to(DEV) for v in terms_ref.case_pairs(N, n_pairs, seed=3))
        wide = ops.score_pair_terms(Z.bfloat16().float(), H.bfloat16().float(), t, a, b)
        for got in (ops.score_pair_terms(Z, H, t, a, b, table_dtype=BF16),
                    ops.score_pair_terms(Z.bfloat16(), H.bfloat16(), t, a, b, table_dtype=BF16)):
            assert all(same_bits(x, y) for x, y in zip(got, wide))
        assert same_bits(wide.logit, ops.score_pair_logits(Z, H, t, a, b, table_dtype=BF16))


def _raw_call(Z, H, t, a, b, want, dtype=None):
    """dl_score_pair_terms[_dtype] itself, every buffer pre-filled: -> rc and the three arrays (None where not asked for)"""
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    N, K, d = Z.shape
    P = len(a)
    a32, b32 = a.to(torch.int32).contiguous(), b.to(torch.int32).contiguous()
    outs = [torch.full((P, K), -7.25, device=DEV) if w else None for w in want]
    ws = torch.full((int(lib.dl_score_pair_terms_workspace_bytes(N, K, d)),), 0x7F, dtype=torch.uint8, device=DEV)
    ptrs = [o.data_ptr() if o is not None else None for o in outs]
    tail = (float(t), a32.data_ptr(), b32.data_ptr(), P, *ptrs, ws.data_ptr(), ws.numel(), ops._stream())
    if dtype is None:
        rc = lib.dl_score_pair_terms(Z.data_ptr(), H.data_ptr(), N, K, d, *tail)
    else:
        rc = lib.dl_score_pair_terms_dtype(Z.data_ptr(), H.data_ptr(), N, K, d, dtype, *tail)
    torch.cuda.synchronize()
    return rc, outs


def test_null_outputs_leave_the_other_arrays_as_they_are():
    from disenlink_amd import _lib
    N, K, d, t = 300, 3, 65, 0.5
    Z, H = tables(N, K, d, seed=2)
    a, b = (v.to(DEV) for v in terms_ref.case_pairs(N, 200, seed=9))
    rc, full = _raw_call(Z, H, t, a, b, (True, True, True))
    assert rc == 0 and not any((o == -7.25).any() for o in full)      # every cell written
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, True)):
        rc, part = _raw_call(Z, H, t, a, b, want)
        assert rc == 0
        for o, ref in zip(part, full):
            assert o is None or same_bits(o, ref)
    rc, _ = _raw_call(Z, H, t, a, b, (False, False, False))
    assert rc == -1 and b"all NULL" in _lib.load().dl_last_error()
    rc, none = _raw_call(Z, H, t, a[:0], b[:0], (True, True, True))    # nothing to do: success, nothing launched
    assert rc == 0


def test_two_calls_give_the_same_bits():
    import os
    from disenlink_amd import ops
    assert os.environ.get("DL_POISON") == "1"                         # outputs and workspace start as NaN patterns
    N, K, d, t = 300, 5, 64, 0.5
    Z, H = tables(N, K, d, seed=4)
    a, b = (v.to(DEV) for v in terms_ref.case_pairs(N, 300, seed=1))
    first = ops.score_pair_terms(Z, H, t, a, b)
    second = ops.score_pair_terms(Z, H, t, a, b)
    for x, y in zip(first, second):
        assert not torch.isnan(x).any() and torch.equal(x.view(torch.int32), y.view(torch.int32))
    empty = ops.score_pair_terms(Z, H, t, a[:0], b[:0])
    assert all(x.shape == (0, K) and x.dtype == torch.float32 for x in empty)
    assert empty.logit.shape == (0,) and empty.contrib.shape == (0, K) and empty.factor.shape == (0,)


def test_overflow_shows_from_its_factor_on_and_nowhere_else():
    from disenlink_amd import ops
    N, K, d, t, k0 = 129, 3, 32, 1.0, 1
    Z, H = tables(N, K, d, seed=8)
    u, v = 5, 77
    Zo, Ho = Z.clone(), H.clone()
    Zo[u, k0] = 10.0                                                  # z.z = 3200: e = +inf
    Zo[v, k0] = 10.0
    Ho[u, k0] = 0.0                                                   # q = 0: the term is inf * 0 = NaN
    a, b = (x.to(DEV) for x in terms_ref.case_pairs(N, 128, seed=6))
    a[10], b[10] = u, v
    plain, over = ops.score_pair_terms(Z, H, t, a, b), ops.score_pair_terms(Zo, Ho, t, a, b)
    assert over.e[10, k0] == float("inf") and over.q[10, k0] == 0
    assert torch.isfinite(over.cum[10, :k0]).all() and torch.isnan(over.cum[10, k0:]).all()
    for k in range(K):
        assert same_bits(over.cum[:, k], ops.score_pair_logits(*terms_ref.prefix_tables(Zo, Ho, k), t, a, b))
    assert int(over.factor[10]) == -1 and torch.isnan(over.logit[10])
    clean = ~((a == u) | (a == v) | (b == u) | (b == v))              # pairs that touch neither row: the same bits as before
    assert int(clean.sum()) > 100
    for x, y in zip(over, plain):
        assert same_bits(x[clean], y[clean])
    assert (over.factor[clean] >= 0).all()


def _golden_model(name):
    from conftest import load_golden
    from disenlink_amd.model import Disentangle
    g = load_golden(name)
    meta = g["meta"]
    model = Disentangle(meta["F"], meta["nhid"], meta["d"], nfactor=meta["K"], beta=meta["beta"], t=meta["t"])
    model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")})
    return model.to(DEV), torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["adj"]).to(DEV), meta


def test_explain_links_contrib_and_factor_are_the_numpy_restatement():
    from conftest import golden_case_names
    from disenlink_amd import ops
    model, x, adj, meta = _golden_model(golden_case_names()[0])
    N, K = meta["N"], meta["K"]
    iu = torch.triu_indices(N, N, 1)[:, :300].to(DEV)
    terms = model.explain_links(x, adj, iu[0], iu[1])
    assert isinstance(terms, ops.PairTerms) and terms.cum.shape == (iu.shape[1], K)
    cum = terms.cum.cpu().numpy()
    assert same_bits(terms.contrib, terms_ref.contrib(cum))
    assert np.array_equal(terms.factor.cpu().numpy(), terms_ref.factor(cum)) and terms.factor.dtype == torch.int64
    m = min(50, iu.shape[1])
    mined = model.top_missing_links(x, adj, m)                       # the list a user would explain
    why = model.explain_links(x, adj, mined.src, mined.dst)
    assert same_bits(why.logit, mined.logit)
    bf = model.explain_links(x, adj, mined.src, mined.dst, table_dtype=BF16)
    assert bf.cum.shape == why.cum.shape and not any(t.requires_grad for t in bf)


def test_cli_mine_explain_adds_the_factor_columns(tmp_path):
    from disenlink_amd import main as cli
    out, plain = tmp_path / "explained.txt", tmp_path / "plain.txt"
    seen = {}
    real = cli.mine_links

    def spy(*args, **kwargs):
        seen["args"], seen["kwargs"] = args, kwargs
        return real(*args, **kwargs)
    cli.mine_links = spy
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            cli.main(["--dataset", "squirrel", "--synthetic", "--epochs", "3", "--run", "1", "--quiet", "--mine", "20", "--explain",
                      "--mine-out", str(out)])
    finally:
        cli.mine_links = real
    assert seen["kwargs"]["explained"] is True
    model, x, graph, known, m, _ = seen["args"]
    kw = dict(seen["kwargs"], explained=False)
    mined = real(model, x, graph, known, m, str(plain), log=lambda *_: None, **kw)      # the same model without --explain
    rows = [ln.split() for ln in out.read_text().splitlines()]
    assert len(rows) == 20 and all(len(r) == 6 for r in rows)
    assert [" ".join(r[:4]) for r in rows] == plain.read_text().splitlines()
    terms = model.explain_links(x, graph, mined.src, mined.dst)
    factor = terms.factor.cpu().numpy()
    assert [int(r[4]) for r in rows] == factor.tolist()
    top = terms.contrib.cpu().numpy()[np.arange(20), factor]
    assert [np.float32(r[5]) for r in rows] == top.tolist()
    line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("mined links by dominant factor:")]
    assert len(line) == 1
    counts = dict(tok.split(":") for tok in line[0].split(":", 1)[1].split())
    K = terms.cum.shape[1]
    assert [int(counts[str(k)]) for k in range(K)] == np.bincount(factor, minlength=K).tolist()


def test_argument_errors():
    from disenlink_amd import _lib, ops
    Z, H = tables(10, 2, 32)
    ids = torch.arange(4, device=DEV)
    with pytest.raises(ValueError, match="differ in length"):
        ops.score_pair_terms(Z, H, 1.0, ids, ids[:3])
    with pytest.raises(ValueError, match="outside"):
        ops.score_pair_terms(Z, H, 1.0, ids, ids + 7)
    with pytest.raises(TypeError, match="fp32"):
        ops.score_pair_terms(Z.bfloat16(), H.bfloat16(), 1.0, ids, ids)
    with pytest.raises(_lib.DisenlinkHipError, match="temperature is 0"):
        ops.score_pair_terms(Z, H, 0.0, ids, ids)
    with pytest.raises(_lib.DisenlinkHipError, match="1 <= d <= 128"):
        Zw = torch.zeros(10, 1, 130, device=DEV)
        ops.score_pair_terms(Zw, Zw, 1.0, ids, ids)
