"""The plain and the _filtered entries of the all-pairs scans on the device.  disenlink_amd.scans calls the _dtype entries
only, so every fp32 entry that forwards to one gets a direct call here, with hand-laid arguments: the plain entry, the
_filtered one with a NULL rule and with a rule, each compared bit for bit with the public function on the same inputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, K, D, T_ = 129, 2, 33, 1.0                    # one row past a 128-row tile, one column past a 32-column step
TOPK, M = 4, 16


def same(a, b) -> bool:
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


@pytest.fixture(scope="module")
def env():
    from disenlink_amd import _lib, scans
    gen = torch.Generator().manual_seed(29)
    e = type("Env", (), {})()
    e.lib, e.scans = _lib.load(), scans
    e.Z = (torch.randn(N, K, D, generator=gen) * 0.4).to(DEV)
    e.H = (torch.randn(N, K, D, generator=gen) * 0.4).to(DEV)
    e.src = torch.tensor([128, 3, 77, 3, 0], dtype=torch.int32, device=DEV)          # 5 queries / targets, one node twice
    e.dst = torch.tensor([5, 128, 12, 64, 127], dtype=torch.int32, device=DEV)
    rows, cols = torch.randint(0, N, (20,), generator=gen), torch.randint(0, N, (20,), generator=gen)
    rows[0], cols[0] = 3, 128                                                          # a target that is excluded
    e.exclude = (rows.to(DEV), cols.to(DEV))
    e.ordered = scans.exclusion_csr(e.exclude, N, DEV)
    e.unordered = scans._unordered_exclusion_csr(e.exclude, N, DEV)
    e.rule = scans.NodeFilter.same(torch.arange(N) % 3, device=DEV)
    return e


def ws_for(nbytes) -> torch.Tensor:
    assert nbytes > 0
    return torch.full((max(256, int(nbytes)),), 0xFF, dtype=torch.uint8, device=DEV)


def out(shape, dtype) -> torch.Tensor:
    return torch.full(shape if isinstance(shape, tuple) else (shape,), -3, dtype=dtype, device=DEV)


def variants(e, base: str, unordered: bool):
    """(entry, trailing arguments, node_filter of the public call): plain, _filtered with NULL, _filtered with the rule."""
    rule, keep = e.rule._c_arg(N, torch.device(DEV), unordered)
    return [(base, (), None, keep), (base + "_filtered", (None,), None, keep), (base + "_filtered", (rule,), e.rule, keep)]


def call(e, entry: str, *args) -> None:
    assert getattr(e.lib, entry)(*args) == 0, (entry, e.lib.dl_last_error())


def stream() -> int:
    from disenlink_amd import _dev
    return _dev._stream()


def test_topk(env):
    e = env
    rp, cp = (x.data_ptr() for x in e.ordered)
    Q = e.src.numel()
    for entry, tail, nf, _keep in variants(e, "dl_score_topk", False):
        ws = ws_for(e.lib.dl_score_topk_workspace_bytes(N, K, D, Q, TOPK, 0))
        index, logit, prob = out((Q, TOPK), torch.int64), out((Q, TOPK), torch.float32), out((Q, TOPK), torch.float32)
        call(e, entry, e.Z.data_ptr(), e.H.data_ptr(), N, K, D, T_, e.src.data_ptr(), Q, TOPK, rp, cp, 1, index.data_ptr(),
             logit.data_ptr(), prob.data_ptr(), ws.data_ptr(), ws.numel(), stream(), *tail)
        ref = e.scans.score_topk(e.Z, e.H, T_, e.src, TOPK, exclude=e.exclude, node_filter=nf)
        assert all(same(a, b) for a, b in zip((index, logit, prob), ref)), entry


def test_ranks(env):
    e = env
    rp, cp = (x.data_ptr() for x in e.ordered)
    order = torch.argsort(e.src, stable=True)                                          # targets grouped by query node
    queries, counts = torch.unique_consecutive(e.src[order], return_counts=True)
    Q, T = queries.numel(), e.src.numel()
    tptr = torch.zeros(Q + 1, dtype=torch.int32, device=DEV)
    tptr[1:] = torch.cumsum(counts, dim=0).to(torch.int32)
    tdst, queries = e.dst[order].contiguous(), queries.to(torch.int32).contiguous()
    for entry, tail, nf, _keep in variants(e, "dl_score_ranks", False):
        ws = ws_for(e.lib.dl_score_topk_workspace_bytes(N, K, D, Q, 0, T))
        greater, ties = out(T, torch.int64), out(T, torch.int64)
        call(e, entry, e.Z.data_ptr(), e.H.data_ptr(), N, K, D, T_, queries.data_ptr(), Q, tptr.data_ptr(), tdst.data_ptr(), T,
             rp, cp, greater.data_ptr(), ties.data_ptr(), ws.data_ptr(), ws.numel(), stream(), *tail)
        ref = e.scans.score_ranks(e.Z, e.H, T_, e.src, e.dst, exclude=e.exclude, node_filter=nf)
        assert same(greater, ref[0][order]) and same(ties, ref[1][order]), entry


def test_mine(env):
    e = env
    rp, cp = (x.data_ptr() for x in e.unordered)
    for entry, tail, nf, _keep in variants(e, "dl_score_mine", True):
        ws = ws_for(e.lib.dl_score_mine_workspace_bytes(N, K, D, M))
        src, dst, logit, prob = out(M, torch.int32), out(M, torch.int32), out(M, torch.float32), out(M, torch.float32)
        count = out(1, torch.int64)
        call(e, entry, e.Z.data_ptr(), e.H.data_ptr(), N, K, D, T_, rp, cp, float("-inf"), M, src.data_ptr(), dst.data_ptr(),
             logit.data_ptr(), prob.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), stream(), *tail)
        ref = e.scans.score_mine(e.Z, e.H, T_, M, exclude=e.exclude, node_filter=nf)
        c = int(count.item())
        assert c == M == len(ref[0]), entry
        assert all(same(a[:c], b) for a, b in zip((src, dst, logit, prob), ref)), entry


def test_pair_logits_and_terms(env):
    e = env
    P = e.src.numel()
    head = (e.Z.data_ptr(), e.H.data_ptr(), N, K, D, T_, e.src.data_ptr(), e.dst.data_ptr(), P)
    ws = ws_for(e.lib.dl_score_pair_logits_workspace_bytes(N, K, D))
    logit = out(P, torch.float32)
    call(e, "dl_score_pair_logits", *head, logit.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    logit = torch.where(logit == 0, torch.zeros_like(logit), logit)                    # the public function reports -0 as +0
    assert same(logit, e.scans.score_pair_logits(e.Z, e.H, T_, e.src, e.dst))
    ws = ws_for(e.lib.dl_score_pair_terms_workspace_bytes(N, K, D))
    terms = [out((P, K), torch.float32) for _ in range(3)]
    call(e, "dl_score_pair_terms", *head, *(x.data_ptr() for x in terms), ws.data_ptr(), ws.numel(), stream())
    ref = e.scans.score_pair_terms(e.Z, e.H, T_, e.src, e.dst)
    assert all(same(a, b) for a, b in zip(terms, ref))


def test_pair_ranks(env):
    e = env
    rp, cp = (x.data_ptr() for x in e.unordered)
    T = e.src.numel()
    lo, hi = torch.minimum(e.src, e.dst).contiguous(), torch.maximum(e.src, e.dst).contiguous()
    key = e.scans._order_keys(e.scans.score_pair_logits(e.Z, e.H, T_, lo, hi))
    ksorted, order = torch.sort(key, stable=True)
    first = torch.searchsorted(ksorted, ksorted)
    tord = torch.where(ksorted >= 0x80000000, ksorted - 0x100000000, ksorted).to(torch.int32).contiguous()
    excluded = {(min(a, b), max(a, b)) for a, b in zip(e.exclude[0].tolist(), e.exclude[1].tolist())}
    is_cand = torch.tensor([(a, b) not in excluded for a, b in zip(lo.tolist(), hi.tolist())], device=DEV).to(torch.int64)
    assert 0 < int(is_cand.sum()) < T                                                  # both kinds of target are here
    for entry, tail, nf, _keep in variants(e, "dl_score_pair_ranks", True):
        ws = ws_for(e.lib.dl_score_pair_ranks_workspace_bytes(N, K, D))
        above, equal, counted = out(T + 1, torch.int64), out(T + 1, torch.int64), out(1, torch.int64)
        call(e, entry, e.Z.data_ptr(), e.H.data_ptr(), N, K, D, T_, rp, cp, tord.data_ptr(), T, above.data_ptr(),
             equal.data_ptr(), counted.data_ptr(), ws.data_ptr(), ws.numel(), stream(), *tail)
        ref = e.scans.score_pair_ranks_counted(e.Z, e.H, T_, e.src, e.dst, exclude=e.exclude, node_filter=nf)
        cs = torch.cumsum(above, dim=0)
        greater, ties = torch.empty_like(ref[0]), torch.empty_like(ref[1])
        greater[order] = cs[T] - cs[:T]
        ties[order] = equal[first]
        in_c = is_cand if nf is None else is_cand * nf.allowed(lo, hi, unordered=True).to(torch.int64)
        assert same(counted, ref[4]) and same(greater, ref[0]) and same(ties - in_c, ref[1]), entry


def test_links_count_and_fill(env):
    e = env
    rp, cp = (x.data_ptr() for x in e.unordered)
    rule, _keep = e.rule._c_arg(N, torch.device(DEV), True)
    for filt, nf in ((None, None), (rule, e.rule)):                                    # these entries take the rule themselves
        ref = e.scans.score_links(e.Z, e.H, T_, 0.0, exclude=e.exclude, node_filter=nf)
        ws = ws_for(e.lib.dl_score_links_workspace_bytes(N, K, D))
        rowptr = out(N + 1, torch.int64)
        head = (e.Z.data_ptr(), e.H.data_ptr(), N, K, D, T_, rp, cp, 0.0, filt, ws.data_ptr(), ws.numel(), rowptr.data_ptr())
        call(e, "dl_score_links_count", *head, stream())
        assert same(rowptr, ref[0])
        nnz = int(rowptr[-1].item())
        assert nnz == len(ref[1]) > 0
        col, logit, prob = out(nnz, torch.int32), out(nnz, torch.float32), out(nnz, torch.float32)
        call(e, "dl_score_links_fill", *head, nnz, col.data_ptr(), logit.data_ptr(), prob.data_ptr(), stream())
        assert all(same(a, b) for a, b in zip((col, logit, prob), ref[1:]))
