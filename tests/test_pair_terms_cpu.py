"""The per-factor terms of given pairs without a GPU: the workspace entry, every refusal of dl_score_pair_terms[_dtype] (they
all come before anything touches the device), the argument checks of ops.score_pair_terms, ``PairTerms.contrib`` / ``.factor``
on hand-made running sums, and --explain in the CLI."""
import numpy as np
import pytest
import torch

import terms_ref
from disenlink_amd import _lib
from test_scan_pins_cpu import PINNED

F32, BF16 = _lib.DL_F32, _lib.DL_BF16
NAN, INF = float("nan"), float("inf")
TOP_N = 65535 * 128


def test_workspace_is_that_of_the_pair_logits():
    lib = _lib.load()
    for N, K, d in PINNED:
        assert int(lib.dl_score_pair_terms_workspace_bytes(N, K, d)) == int(lib.dl_score_pair_logits_workspace_bytes(N, K, d)) \
            == PINNED[(N, K, d)]["pair_logits_ws"]
        for dt in (F32, BF16):
            want = int(lib.dl_score_pair_logits_workspace_bytes_dtype(N, K, d, dt))
            assert int(lib.dl_score_pair_terms_workspace_bytes_dtype(N, K, d, dt)) == want > 0
    for bad in ((0, 8, 64), (TOP_N + 1, 1, 8), (100, 8, 130), (100, 0, 64), (-5, 8, 64)):
        assert int(lib.dl_score_pair_terms_workspace_bytes(*bad)) == 0
        assert int(lib.dl_score_pair_terms_workspace_bytes_dtype(*bad, BF16)) == 0
    assert int(lib.dl_score_pair_terms_workspace_bytes(TOP_N, 1, 8)) > 0
    for dt in (2, -1):
        assert int(lib.dl_score_pair_terms_workspace_bytes_dtype(300, 3, 128, dt)) == 0


def _terms(lib, Z=1, H=1, N=10, K=2, d=32, dtype=F32, t=1.0, a=1, b=1, n_pairs=4, e=1, q=1, cum=1, ws=None, ws_bytes=0):
    """dl_score_pair_terms_dtype with made-up addresses: every call here is refused before an address is used"""
    return lib.dl_score_pair_terms_dtype(Z, H, N, K, d, dtype, t, a, b, n_pairs, e, q, cum, ws, ws_bytes, None)


def _logits(lib, Z=1, H=1, N=10, K=2, d=32, dtype=F32, t=1.0, a=1, b=1, n_pairs=4, ws=None, ws_bytes=0):
    return lib.dl_score_pair_logits_dtype(Z, H, N, K, d, dtype, t, a, b, n_pairs, 1, ws, ws_bytes, None)


def test_refusals_of_the_c_entry_are_those_of_the_pair_logits():
    lib = _lib.load()
    shared = [                                                        # (arguments, a word of the message), in the order of the checks
        (dict(dtype=5), b"unknown dtype 5"),
        (dict(K=0), b""),
        (dict(d=0), b""),
        (dict(d=129), b"1 <= d <= 128"),
        (dict(K=65), b""),
        (dict(N=0), b"8388480"),
        (dict(N=TOP_N + 1, K=1, d=8), b"8388480"),
        (dict(t=0.0), b"temperature is 0"),
        (dict(n_pairs=-1), b"n_pairs=-1"),
        (dict(n_pairs=(1 << 30) + 1), b"n_pairs="),
        (dict(Z=None), b"NULL argument"),
        (dict(H=None), b"NULL argument"),
        (dict(a=None), b"NULL argument"),
        (dict(b=None), b"NULL argument"),
        # an earlier check wins over a later one
        (dict(dtype=7, d=129, t=0.0, Z=None), b"unknown dtype 7"),
        (dict(d=129, t=0.0, Z=None), b"1 <= d <= 128"),
        (dict(t=0.0, n_pairs=-1, Z=None), b"temperature is 0"),
        (dict(n_pairs=-1, Z=None), b"n_pairs=-1"),
    ]
    for kw, word in shared:
        rc = _terms(lib, **kw)
        msg = lib.dl_last_error()
        assert rc == -1 and word in msg, (kw, rc, msg)
        assert _logits(lib, **kw) == rc and lib.dl_last_error() == msg, kw      # the same code and the same words
    assert _terms(lib, e=None, q=None, cum=None) == -1 and b"all NULL" in lib.dl_last_error()
    assert _terms(lib, Z=None, e=None, q=None, cum=None) == -1 and b"NULL argument" in lib.dl_last_error()      # the tables first
    need = int(lib.dl_score_pair_terms_workspace_bytes_dtype(10, 2, 32, F32))
    for kw in (dict(ws=None, ws_bytes=need), dict(ws=1, ws_bytes=need - 1), dict(ws=1, ws_bytes=0),
               dict(ws=1, ws_bytes=need - 1, e=None), dict(ws=1, ws_bytes=need - 1, q=None, cum=None)):
        assert _terms(lib, **kw) == -3, kw                              # DL_E_WORKSPACE
        assert b"workspace too small" in lib.dl_last_error() and b"dl_score_pair_terms_workspace_bytes" in lib.dl_last_error()
    assert _terms(lib, e=None, q=None, cum=None, ws=1, ws_bytes=0) == -1          # the outputs before the workspace
    # nothing to do: success whatever the pointers, nothing launched
    assert _terms(lib, n_pairs=0, Z=None, H=None, a=None, b=None, e=None, q=None, cum=None) == 0
    assert _terms(lib, n_pairs=0, t=0.0) == -1                          # ... but only behind the checks of the values
    # the fp32 entry is a call of the _dtype one
    assert lib.dl_score_pair_terms(1, 1, 10, 2, 129, 1.0, 1, 1, 4, 1, 1, 1, None, 0, None) == -1
    assert b"1 <= d <= 128" in lib.dl_last_error()
    assert lib.dl_score_pair_terms(1, 1, 10, 2, 32, 1.0, 1, 1, 4, None, None, None, None, 0, None) == -1
    assert b"all NULL" in lib.dl_last_error()
    assert lib.dl_score_pair_terms(1, 1, 10, 2, 32, 1.0, 1, 1, 4, 1, 1, 1, 1, need - 1, None) == -3
    assert lib.dl_score_pair_terms(None, None, 10, 2, 32, 1.0, None, None, 0, None, None, None, None, 0, None) == 0


def test_ops_refusals(monkeypatch):
    from disenlink_amd import ops, scans
    Z, H = torch.randn(10, 2, 32), torch.randn(10, 2, 32)
    ids = torch.arange(4)
    with pytest.raises(_lib.DisenlinkHipError, match="only on the GPU"):        # there is no CPU path
        ops.score_pair_terms(Z, H, 1.0, ids, ids)
    with pytest.raises(TypeError, match="fp32"):                      # bf16 tensors without the keyword
        ops.score_pair_terms(Z.bfloat16(), H.bfloat16(), 1.0, ids, ids)
    with pytest.raises(TypeError, match="fp32"):
        ops.score_pair_terms(Z.bfloat16(), H.bfloat16(), 1.0, ids, ids, table_dtype=torch.float32)
    with pytest.raises(TypeError, match="both"):
        ops.score_pair_terms(Z.bfloat16(), H, 1.0, ids, ids, table_dtype=torch.bfloat16)
    for bad in (torch.float16, None, "bf16"):
        with pytest.raises(TypeError, match="table_dtype"):
            ops.score_pair_terms(Z, H, 1.0, ids, ids, table_dtype=bad)
    # the checks behind the device check, which come before anything is launched: reached here with the device check lifted
    monkeypatch.setattr(scans, "_need_cuda", lambda *tensors: None)
    for call in (ops.score_pair_terms, ops.score_pair_logits):        # the same checks in both
        with pytest.raises(ValueError, match="differ in length"):
            call(Z, H, 1.0, ids, ids[:3])
        with pytest.raises(ValueError, match=r"a outside \[0, 10\)"):
            call(Z, H, 1.0, ids + 7, ids)
        with pytest.raises(ValueError, match=r"b outside \[0, 10\)"):
            call(Z, H, 1.0, ids, -ids - 1)
        with pytest.raises(TypeError, match="integer node ids"):
            call(Z, H, 1.0, ids.float(), ids)
        with pytest.raises(ValueError, match="differ in shape"):
            call(Z, H[:, :1], 1.0, ids, ids)
        with pytest.raises(_lib.DisenlinkHipError, match="1 <= d <= 128"):
            call(torch.zeros(10, 1, 130), torch.zeros(10, 1, 130), 1.0, ids, ids)
    empty = ops.score_pair_terms(Z, H, 1.0, ids[:0], ids[:0])         # P = 0: empty [0, K] tensors, nothing launched
    assert isinstance(empty, ops.PairTerms) and all(x.shape == (0, 2) and x.dtype == torch.float32 for x in empty)
    assert empty.logit.shape == (0,) and empty.contrib.shape == (0, 2)
    assert empty.factor.shape == (0,) and empty.factor.dtype == torch.int64


HAND = np.array([
    [1.0, 3.0, 3.5],            # contributions 1, 2, 0.5
    [2.0, 4.0, 6.0],            # 2, 2, 2: a tie resolves to the first index
    [0.5, 1.0, 1.5],            # 0.5 three times
    [-1.0, -3.0, -3.5],         # all negative: the least negative wins
    [-2.0, -1.0, -4.0],         # -2, 1, -3
    [0.0, -0.0, 0.0],           # zeros of either sign are equal
    [1.0, NAN, NAN],            # a NaN from factor 1 on
    [NAN, NAN, NAN],
    [1.0, INF, INF],            # +inf, then inf - inf = NaN
    [1.0, 2.0, INF],            # +inf in the last factor only: it dominates
    [-INF, -INF, -INF],         # -inf, then NaN
], dtype=np.float32)
HAND_FACTOR = [1, 0, 0, 2, 1, 0, -1, -1, -1, 2, -1]


def test_contrib_and_factor_on_hand_made_running_sums():
    from disenlink_amd import ops
    cum = torch.from_numpy(HAND)
    terms = ops.PairTerms(torch.zeros_like(cum), torch.zeros_like(cum), cum)
    assert terms.e.shape == terms.q.shape == terms.cum.shape and tuple(terms._fields) == ("e", "q", "cum")
    c = terms.contrib
    assert c.dtype == torch.float32 and c.shape == cum.shape
    assert c[0].tolist() == [1.0, 2.0, 0.5] and c[4].tolist() == [-2.0, 1.0, -3.0] and c[3].tolist() == [-1.0, -2.0, -0.5]
    assert c[9].tolist() == [1.0, 1.0, INF] and c[8, 1] == INF and torch.isnan(c[8, 2]) and torch.isnan(c[10, 1:]).all()
    assert terms_ref.same_bits(c, terms_ref.contrib(HAND))
    f = terms.factor
    assert f.dtype == torch.int64 and f.tolist() == HAND_FACTOR
    assert terms_ref.factor(HAND).tolist() == HAND_FACTOR
    assert terms_ref.same_bits(terms.cum, HAND)                             # the properties leave the arrays alone
    lg = terms.logit
    assert lg.shape == (len(HAND),) and lg[0] == 3.5 and torch.isnan(lg[6]) and lg[9] == INF
    neg = ops.PairTerms(cum[:1], cum[:1], torch.tensor([[1.0, -0.0]]))
    assert neg.logit.view(torch.int32).tolist() == [0]                # -0 is reported as +0
    one = ops.PairTerms(cum[:, :1], cum[:, :1], cum[:, :1])           # K = 1: the one factor, or -1
    assert one.factor.tolist() == [0, 0, 0, 0, 0, 0, 0, -1, 0, 0, 0] and terms_ref.factor(HAND[:, :1]).tolist() == one.factor.tolist()
    rng = np.random.default_rng(0)
    r = rng.standard_normal((200, 8)).astype(np.float32).round(1)     # coarse values: many exact ties
    rt = ops.PairTerms(None, None, torch.from_numpy(r))
    assert terms_ref.same_bits(rt.contrib, terms_ref.contrib(r)) and rt.factor.tolist() == terms_ref.factor(r).tolist()


def test_bit_comparison_helper():
    a = np.array([0.0, -0.0, NAN, 1.0], np.float32)
    b = np.array([-0.0, 0.0, np.float32(np.uint32(0xFFC00001).view(np.float32)), 1.0], np.float32)
    assert terms_ref.same_bits(a, b) and terms_ref.same_bits(torch.from_numpy(a), b)
    assert not terms_ref.same_bits(a, np.array([0.0, 0.0, NAN, np.nextafter(np.float32(1), np.float32(2))], np.float32))
    assert not terms_ref.same_bits(a, a[:3])


class _Model:
    """stands where the trained module would: three mined links and hand-made terms for them"""

    def __init__(self):
        self.seen = {}

    def top_missing_links(self, x, graph, m, **kw):
        from disenlink_amd.model import MinedLinks
        return MinedLinks(torch.tensor([0, 2, 4], dtype=torch.int32), torch.tensor([1, 3, 5], dtype=torch.int32),
                          torch.tensor([3.5, 1.0, NAN]), torch.tensor([0.9, 0.7, NAN]))

    def explain_links(self, x, graph, src, dst, **kw):
        from disenlink_amd import ops
        self.seen["explain"] = (src.tolist(), dst.tolist(), kw)
        cum = torch.from_numpy(HAND[[0, 4, 6]])
        return ops.PairTerms(cum, cum, cum)


def test_cli_explain_columns_and_refusal(tmp_path):
    from disenlink_amd import main as cli
    p = cli.build_parser()
    assert p.parse_args([]).explain is False and p.parse_args(["--explain"]).explain is True
    for argv in (["--synthetic", "--explain"], ["--synthetic", "--explain", "--rank-eval"],
                 ["--synthetic", "--explain", "--mine-out", "x"]):
        with pytest.raises(SystemExit, match="--explain names the factor"):
            cli.main(argv)
    if not torch.cuda.is_available():                                 # with --mine the run goes on to where the device is asked for
        for flag in (["--mine", "5"], ["--predict-links", "0.9"]):
            with pytest.raises(SystemExit, match="runs on the GPU only"):
                cli.main(["--synthetic", "--explain", *flag])
    model, out, plain, said = _Model(), tmp_path / "e.txt", tmp_path / "p.txt", []
    cli.mine_links(model, None, None, "known", 3, str(out), log=said.append, table_dtype=torch.bfloat16, explained=True)
    assert model.seen["explain"] == ([0, 2, 4], [1, 3, 5], {"table_dtype": torch.bfloat16})
    cli.mine_links(model, None, None, "known", 3, str(plain), log=lambda *_: None)
    rows = [ln.split() for ln in out.read_text().splitlines()]
    assert [" ".join(r[:4]) for r in rows] == plain.read_text().splitlines()
    assert [r[4:] for r in rows] == [["1", "2"], ["1", "1"], ["-1", "nan"]]
    assert said[0] == "mined links by dominant factor: 0:0 1:2 2:0 nan:1"
    assert said[1].endswith("src dst logit prob factor contrib") and said[2].split()[4:] == ["1", "2"]
