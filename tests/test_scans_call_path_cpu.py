"""The call path of disenlink_amd.scans without a GPU: a recording stand-in takes the library's place, and every C call a
public scan makes is held against the prototype in _lib.EXPORTS — the entry is the _dtype one, the argument count and the
kind of every argument fit, the table type sits where the entry has it, and the node filter is NULL exactly when none was
given.  An argument list spliced wrongly fails here instead of on a device."""
import ctypes as C

import pytest
import torch

from disenlink_amd import _lib, scans

N, K, D = 8, 2, 8
QUERY = "dl_score_topk_supported"                 # the capability question of the table check: the one call that is no entry


class Recorder:
    """Stands for the loaded library: every symbol is a function that notes (name, args); entries return 0 (DL_OK),
    sizers 4096 bytes, the capability question 1."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 1 if name == QUERY else 4096 if "_workspace_bytes" in name else 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(scans, "_need_cuda", lambda *tensors: None)
    monkeypatch.setattr(scans, "_stream", lambda: 0)
    # outputs nobody fills: zeros, so that the counts read back from them (mine's count, the links' rowptr[N]) are 0
    monkeypatch.setattr(scans, "_empty", lambda shape, dtype, device: torch.zeros(shape, dtype=dtype, device=device))
    return r


def fits(code, value) -> bool:
    """Whether ``value`` is what the scans pass for an argument of ctypes type ``code``."""
    if code is _lib._NF:
        return value is None or type(value).__name__ == "CArgObject"          # byref(dl_node_filter)
    if code is _lib._P:
        return value is None or type(value) is int
    if code is _lib._f:
        return type(value) is float
    assert code in (_lib._i, _lib._z, C.c_int64), code
    return type(value) is int


IDS = torch.tensor([0, 3, 5, 6, 7])
OTHER = torch.tensor([1, 2, 4, 0, 3])
EXCLUDE = (torch.tensor([0, 1, 2]), torch.tensor([4, 5, 6]))
SCANS = {                                         # name: (call(Z, H, **kw), takes a node filter)
    "score_topk": (lambda Z, H, **kw: scans.score_topk(Z, H, 1.0, IDS, 4, exclude=EXCLUDE, **kw), True),
    "score_ranks": (lambda Z, H, **kw: scans.score_ranks(Z, H, 1.0, IDS, OTHER, exclude=EXCLUDE, **kw), True),
    "score_mine": (lambda Z, H, **kw: scans.score_mine(Z, H, 1.0, 16, exclude=EXCLUDE, **kw), True),
    "score_links": (lambda Z, H, **kw: scans.score_links(Z, H, 1.0, 0.0, exclude=EXCLUDE, **kw), True),
    "score_link_degrees": (lambda Z, H, **kw: scans.score_link_degrees(Z, H, 1.0, 0.0, exclude=EXCLUDE, **kw), True),
    "score_top_links": (lambda Z, H, **kw: scans.score_top_links(Z, H, 1.0, 5, exclude=EXCLUDE, **kw), True),
    "score_pair_ranks": (lambda Z, H, **kw: scans.score_pair_ranks(Z, H, 1.0, IDS, OTHER, exclude=EXCLUDE, **kw), True),
    "score_pair_logits": (lambda Z, H, **kw: scans.score_pair_logits(Z, H, 1.0, IDS, OTHER, **kw), False),
    "score_pair_terms": (lambda Z, H, **kw: scans.score_pair_terms(Z, H, 1.0, IDS, OTHER, **kw), False),
}
ENTRIES = {                                       # the C entries each scan is made of (its sizers come on top)
    "score_topk": ["dl_score_topk_dtype"],
    "score_ranks": ["dl_score_ranks_dtype"],
    "score_mine": ["dl_score_mine_dtype"],
    "score_links": ["dl_score_links_count_dtype", "dl_score_links_fill_dtype"],
    "score_link_degrees": ["dl_score_links_count_dtype"],
    "score_top_links": ["dl_score_links_top_count_dtype", "dl_score_links_top_fill_dtype"],
    "score_pair_ranks": ["dl_score_pair_logits_dtype", "dl_score_pair_ranks_dtype"],
    "score_pair_logits": ["dl_score_pair_logits_dtype"],
    "score_pair_terms": ["dl_score_pair_terms_dtype"],
}
CASES = [(name, dtype, filtered) for name, (_call, takes) in SCANS.items() for dtype in (torch.float32, torch.bfloat16)
         for filtered in ((False, True) if takes else (False,))]


@pytest.mark.parametrize("name,table_dtype,filtered", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_every_call_is_the_dtype_entry_with_its_own_argument_list(rec, name, table_dtype, filtered):
    gen = torch.Generator().manual_seed(3)
    Z, H = torch.randn(N, K, D, generator=gen), torch.randn(N, K, D, generator=gen)
    kw = {"table_dtype": table_dtype}
    if filtered:
        kw["node_filter"] = scans.NodeFilter.same(torch.arange(N) % 3)
    SCANS[name][0](Z, H, **kw)
    want = _lib.DL_F32 if table_dtype is torch.float32 else _lib.DL_BF16
    calls = [c for c in rec.calls if c[0] != QUERY]
    assert [n for n, _ in calls if "_workspace_bytes" not in n] == ENTRIES[name]
    assert len(calls) > len(ENTRIES[name])                                     # ... and at least one sizer was asked
    for entry, args in calls:
        assert entry.endswith("_dtype"), entry
        codes = _lib.EXPORTS[entry][1]
        assert len(args) == len(codes), entry
        assert all(fits(c, a) for c, a in zip(codes, args)), (entry, args)
        assert args[3 if "_workspace_bytes" in entry else 5] == want, entry   # sizers: (N, K, d, dt, ...)
        assert args[:3] == (N, K, D) if "_workspace_bytes" in entry else args[2:5] == (N, K, D), entry
        if _lib._NF in codes:
            assert (args[codes.index(_lib._NF)] is None) == (not filtered), entry
    if name in ("score_links", "score_top_links"):
        (_, count), (_, fill) = [c for c in calls if "_workspace_bytes" not in c[0]]
        n = 13 if name == "score_links" else 14                                # the budgeted graph's m sits ahead of the rule
        assert fill[:n] == count[:n]
        assert fill[n] == count[n] and fill[n + 1] == 0                        # the same rowptr, then nnz
