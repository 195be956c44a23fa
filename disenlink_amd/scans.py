"""The all-pairs inference scans over libdisenlink_hip.so: top-k and ranks of a node's candidates, mining, the
thresholded and the budgeted link graph, pair ranks, and the logits and per-factor terms of given pairs — with the exclusion sets and
node-group rules they take — and, at the end, mining and the link graph between two node sets and by blocks on graphs of
any size.  Nothing here is differentiable.

Every scan goes through ONE C entry, ``dl_score_<name>_dtype`` (the implementation; the plain and ``_filtered`` entries
of the C ABI forward to it), sized by ``dl_score_<name>_workspace_bytes_dtype``; each writes its argument list once,
in that entry's order.  ``ops`` re-exports the public names.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from ._dev import _empty, _need_cuda, _nkd, _stream, _ws
from .graph import Graph


# ---------------------------------------------------------------------- ranking of all candidates (dl_score_rank.hip)
RANK_MAX_K = 128


def exclusion_csr(exclude, n_nodes: int, device=None):
    """Normalise an exclusion set to the CSR the ranking kernels take: (rowptr int32 [N+1], col int32) with ascending,
    distinct columns per row, on ``device`` (default: where the set lives), or (None, None) for ``exclude=None``.
    ``exclude``: a ``Graph`` (its stored entries), a dense [N,N] mask (entries != 0) or a ``(rows, cols)`` pair of index
    sequences.  Duplicates collapse (``torch.unique`` on row * N + col)."""
    if exclude is None:
        return None, None
    N = int(n_nodes)
    if isinstance(exclude, Graph):
        if exclude.n_nodes != N:
            raise ValueError(f"exclusion graph has {exclude.n_nodes} nodes, expected {N}")
        rows = _csr_rows(exclude.rowptr, exclude.row_offset)
        key = _sorted_keys(rows, exclude.col[:rows.numel()].to(torch.int64), N, device)
    else:
        key = _pair_keys(exclude, N, N, device, ("(rows, cols)", "[0, N)", "[N, N]"))
    return _local_csr(*_split_keys(key, N), N)


def _csr_rows(rowptr: torch.Tensor, first_row: int = 0) -> torch.Tensor:
    """int64 [nnz]: the row of every entry of a CSR whose rows start at ``first_row``."""
    ptr = rowptr.to(torch.int64)
    return torch.repeat_interleave(torch.arange(first_row, first_row + ptr.numel() - 1, device=ptr.device), ptr[1:] - ptr[:-1])


def _sorted_keys(rows: torch.Tensor, cols: torch.Tensor, n_cols: int, device) -> torch.Tensor:
    """The distinct keys row * n_cols + col of int64 pairs, ascending (rows ascending, columns ascending in a row), on
    ``device`` (default: where the pairs live)."""
    dev = rows.device if device is None else torch.device(device)
    return torch.unique(rows.to(dev) * n_cols + cols.to(dev))


def _pair_keys(exclude, n_rows: int, n_cols: int, device, names) -> torch.Tensor:
    """``_sorted_keys`` of an exclusion set given as a pair of index sequences or as a dense [n_rows, n_cols] mask
    (entries != 0); ``names`` = how the refusals call the pair list, its range and the mask's shape."""
    if isinstance(exclude, (tuple, list)):
        if len(exclude) != 2:
            raise ValueError(f"an exclusion pair list is {names[0]}")
        rows, cols = (torch.as_tensor(v, device=device).reshape(-1).to(torch.int64) for v in exclude)
        if rows.numel() != cols.numel():
            raise ValueError("exclusion rows and cols differ in length")
        if rows.numel() and (int(rows.min()) < 0 or int(cols.min()) < 0 or int(rows.max()) >= n_rows
                             or int(cols.max()) >= n_cols):
            raise ValueError(f"exclusion pair outside {names[1]}")
    else:
        m = torch.as_tensor(exclude, device=device)
        if m.dim() != 2 or tuple(m.shape) != (n_rows, n_cols):
            raise ValueError(f"an exclusion mask must be {names[2]} = [{n_rows}, {n_cols}], got {tuple(m.shape)}")
        rows, cols = torch.nonzero(m, as_tuple=True)
    return _sorted_keys(rows, cols, n_cols, device)


def _split_keys(key: torch.Tensor, n_cols: int):
    r = torch.div(key, n_cols, rounding_mode="floor")
    return r, key - r * n_cols


def _local_csr(rows: torch.Tensor, cols: torch.Tensor, n_rows: int):
    """(rowptr int32 [n_rows+1], col int32) of int64 pairs already sorted by row, then column."""
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), dim=0)
    return rowptr.to(torch.int32), cols.to(torch.int32)


def _scan_dtype(table_dtype) -> int:
    """The dl_dtype of a scan's ``table_dtype`` keyword: fp32 (the default) or bf16."""
    if table_dtype is torch.float32:
        return _lib.DL_F32
    if table_dtype is torch.bfloat16:
        return _lib.DL_BF16
    raise TypeError(f"table_dtype must be torch.float32 or torch.bfloat16, got {table_dtype!r}")


def _rank_tables(Z, H, table_dtype=torch.float32):
    """[N,K,d] tables on the device, 1 <= d <= 128 (dl_score_topk_supported).  ``table_dtype=torch.float32`` (the default):
    fp32 tensors, nothing else.  ``torch.bfloat16``: Z and H are both bf16 tensors, used as they are, or both fp32 tensors,
    rounded to nearest-even here exactly as the training step rounds its tables (``HotPathPairs``); the scans then run their
    one-plane kernels (dl_score_*_dtype with DL_BF16)."""
    if _scan_dtype(table_dtype) == _lib.DL_F32:
        if Z.dtype != torch.float32 or H.dtype != torch.float32:
            raise TypeError(f"the ranking kernels take fp32 tables, got {Z.dtype} / {H.dtype}")
    else:
        if Z.dtype != H.dtype or Z.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"table_dtype=torch.bfloat16 takes Z and H both bf16 or both fp32, got {Z.dtype} / {H.dtype}")
        _need_cuda(Z, H)
        Z, H = Z.to(torch.bfloat16), H.to(torch.bfloat16)
    _need_cuda(Z, H)
    N, K, d = _nkd(Z)
    if tuple(H.shape) != tuple(Z.shape):
        raise ValueError("Z and H differ in shape")
    if N < 1 or not _lib.load().dl_score_topk_supported(K, d):
        raise _lib.DisenlinkHipError(f"the ranking kernels serve N >= 1, K <= 64 and 1 <= d <= 128 (got N={N}, K={K}, d={d})")
    return Z.contiguous(), H.contiguous(), N, K, d


def _node_ids(ids, N: int, device, what: str) -> torch.Tensor:
    ids = torch.as_tensor(ids, device=device).reshape(-1)
    if ids.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what} must be integer node ids, got {ids.dtype}")
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= N):
        raise ValueError(f"{what} outside [0, {N})")
    return ids.to(torch.int32).contiguous()


def _id_pairs(a, b, N: int, device, what_a: str, what_b: str):
    """The two ends of listed pairs as ``_node_ids``, of one length."""
    a, b = _node_ids(a, N, device, what_a), _node_ids(b, N, device, what_b)
    if a.numel() != b.numel():
        raise ValueError(f"{what_a} and {what_b} differ in length")
    return a, b


def _csr_args(rowptr, col, device):
    if rowptr is None:
        return None, None, ()
    if col.numel() == 0:                                             # a valid address for an empty column array
        col = torch.zeros(1, dtype=torch.int32, device=device)
    return rowptr.data_ptr(), col.data_ptr(), (rowptr, col)


def _group_array(groups, what: str = "groups", n=None) -> torch.Tensor:
    """The one check of a group array's form: 1-D, of an integer type and, where ``n`` is given, of n entries."""
    g = torch.as_tensor(groups)
    if g.dim() != 1 or g.dtype.is_floating_point or g.dtype.is_complex or (n is not None and g.numel() != n):
        of = "" if n is None else f" of {n} entries"
        raise ValueError(f"{what} must be a 1-D integer array{of}, got {tuple(g.shape)} {g.dtype}")
    return g


def _group_range(g: torch.Tensor, n: int, what: str = "groups") -> None:
    """... and of its values, all in [0, n): ONE host read."""
    lo, hi = (int(v) for v in torch.stack(torch.aminmax(g.to(torch.int64))).tolist())
    if lo < 0 or hi >= n:
        raise ValueError(f"{what} outside [0, {n}): min {lo}, max {hi}")


class NodeFilter:
    """A rule on node GROUPS for the candidate scans (dl_node_filter): ``groups`` [N] gives every node a group below
    ``n_groups`` <= 64, and the boolean matrix ``allow`` [n_groups, n_groups] says whether a row of group g may take a
    partner of group h — what an exclusion set could only say by listing O(N^2) pairs.  Prepared once, like
    ``pair_exclusion``: the arrays are converted and moved, and ONE host read checks groups.max() < n_groups.
    Ordered scans (``score_topk``, ``score_ranks``): the row is the query, the partner the candidate, ``allow`` may be
    asymmetric.  Unordered scans (``score_mine``, ``score_pair_ranks``) need a symmetric rule (``symmetric``) and raise
    ValueError otherwise; ``candidates`` carries a rule of its own for them (both endpoints in the pool)."""

    def __init__(self, groups, allow, device=None, _pair_allow=None):
        g = _group_array(groups)
        a = torch.as_tensor(allow).detach().to("cpu")
        if a.dim() != 2 or a.shape[0] != a.shape[1] or not 1 <= a.shape[0] <= 64:
            raise ValueError(f"allow must be [n_groups, n_groups] with 1 <= n_groups <= 64, got {tuple(a.shape)}")
        a = a != 0
        n = int(a.shape[0])
        if g.numel():
            _group_range(g, n)                                         # the one host read
        self.symmetric = bool(torch.equal(a, a.t()))
        pair = _pair_allow if _pair_allow is not None else a if self.symmetric else None      # the unordered scans' rule
        dev = g.device if device is None else torch.device(device)
        self.n_nodes, self.n_groups = int(g.numel()), n
        self.groups = g.to(device=dev, dtype=torch.uint8).contiguous()
        self.allow = a.to(dev)
        self.pair_allow = None if pair is None else pair.to(dev)
        self._words = self._pack(a).to(dev)
        self._pair_words = None if pair is None else self._pack(pair).to(dev)

    @staticmethod
    def _pack(a: torch.Tensor) -> torch.Tensor:
        """allow [n, n] bool -> the uint64 words of dl_node_filter (bit h of word g), as int64 bits."""
        words = [sum(1 << h for h in range(a.shape[1]) if bool(a[g, h])) for g in range(a.shape[0])]
        return torch.tensor([w - (1 << 64) if w >= (1 << 63) else w for w in words], dtype=torch.int64)

    @staticmethod
    def _dense_groups(groups):
        g = _group_array(groups)
        n = int(g.max()) + 1 if g.numel() else 1
        if n > 64 or (g.numel() and int(g.min()) < 0):
            raise ValueError(f"a node filter takes groups 0..63, got {int(g.min())}..{n - 1}")
        return g, max(n, 1)

    @classmethod
    def same(cls, groups, device=None) -> "NodeFilter":
        """Only links between nodes of the same group."""
        g, n = cls._dense_groups(groups)
        return cls(g, torch.eye(n, dtype=torch.bool), device)

    @classmethod
    def different(cls, groups, device=None) -> "NodeFilter":
        """Only links between nodes of different groups."""
        g, n = cls._dense_groups(groups)
        return cls(g, ~torch.eye(n, dtype=torch.bool), device)

    @classmethod
    def between(cls, mask_a, mask_b, both_ways: bool = True, device=None) -> "NodeFilter":
        """Rows in ``mask_a`` take partners in ``mask_b`` (users -> items); with ``both_ways`` also the reverse, which
        makes the rule symmetric.  The masks are boolean [N] and may overlap."""
        ma, mb = torch.as_tensor(mask_a) != 0, torch.as_tensor(mask_b) != 0
        if ma.dim() != 1 or ma.shape != mb.shape:
            raise ValueError(f"the masks must be 1-D and of one length, got {tuple(ma.shape)} and {tuple(mb.shape)}")
        g = ma.to(torch.uint8) + 2 * mb.to(ma.device).to(torch.uint8)      # 0 neither, 1 a, 2 b, 3 both
        allow = torch.zeros(4, 4, dtype=torch.bool)
        for r in range(4):
            for c in range(4):
                allow[r, c] = bool(r & 1 and c & 2) or bool(both_ways and r & 2 and c & 1)
        return cls(g, allow, device)

    @classmethod
    def candidates(cls, mask, device=None) -> "NodeFilter":
        """A fixed candidate pool (boolean [N]).  Ordered scans: any query takes only pool members.  Unordered scans: both
        endpoints are in the pool."""
        m = torch.as_tensor(mask) != 0
        if m.dim() != 1:
            raise ValueError(f"the mask must be 1-D, got {tuple(m.shape)}")
        return cls(m.to(torch.uint8), torch.tensor([[False, True], [False, True]]), device,
                   _pair_allow=torch.tensor([[False, False], [False, True]]))

    def to(self, device) -> "NodeFilter":
        """The same filter with its arrays on ``device`` (no check is repeated)."""
        f = object.__new__(NodeFilter)
        f.n_nodes, f.n_groups, f.symmetric = self.n_nodes, self.n_groups, self.symmetric
        for name in ("groups", "allow", "pair_allow", "_words", "_pair_words"):
            v = getattr(self, name)
            setattr(f, name, None if v is None else v.to(device))
        return f

    def allowed(self, u, v, unordered: bool = False) -> torch.Tensor:
        """bool per pair: may row u[i] take partner v[i]?  The kernels' rule in torch on index tensors (for tests and
        callers that post-process; no hot path uses it).  ``unordered``: the rule of the unordered scans."""
        a = self._pair_rule() if unordered else self.allow
        u = torch.as_tensor(u, device=self.groups.device).long()
        v = torch.as_tensor(v, device=self.groups.device).long()
        return a[self.groups[u].long(), self.groups[v].long()]

    def _pair_rule(self) -> torch.Tensor:
        if self.pair_allow is None:
            raise ValueError("an unordered scan needs a symmetric node filter (allow[g][h] == allow[h][g]); "
                             "this one is asymmetric")
        return self.pair_allow

    def _n_pairs_allowed(self) -> torch.Tensor:
        """int64 [1] on the filter's device: unordered pairs u < v the rule admits, from the group sizes."""
        a = self._pair_rule().to(torch.int64)
        c = torch.bincount(self.groups.long(), minlength=self.n_groups).to(torch.int64)
        cross = (a * c[:, None] * c[None, :]).sum() - (a.diagonal() * c * c).sum()
        return (cross // 2 + (a.diagonal() * (c * (c - 1) // 2)).sum()).reshape(1)

    def _c_arg(self, N: int, device, unordered: bool):
        """(byref(dl_node_filter), keep-alive) for a scan over N nodes on ``device``; raises before anything launches."""
        words = self._words
        if unordered:
            self._pair_rule()
            words = self._pair_words
        if self.groups.device != torch.device(device):
            raise ValueError(f"node filter on {self.groups.device}, tables on {device}: use NodeFilter.to(device)")
        st = _lib.DlNodeFilter(self.groups.data_ptr(), self.n_groups, words.data_ptr())
        return C.byref(st), (st, self.groups, words)


def _filter_check(node_filter, Z, unordered: bool) -> None:
    """The host-side refusals of a node filter, ahead of every other check and of any launch."""
    if node_filter is None:
        return
    if not isinstance(node_filter, NodeFilter):
        raise TypeError(f"node_filter must be an ops.NodeFilter, got {type(node_filter).__name__}")
    if node_filter.n_nodes != int(Z.shape[0]):
        raise ValueError(f"node filter of {node_filter.n_nodes} nodes, tables of {int(Z.shape[0])}")
    if unordered:
        node_filter._pair_rule()


def _scan_tables(Z, H, node_filter, unordered: bool, table_dtype=torch.float32):
    """How every scan starts: the refusals of the node filter, then of the tables -> (Z, H, N, K, d)."""
    _filter_check(node_filter, Z, unordered)
    return _rank_tables(Z, H, table_dtype)


def _scan_buffers(excl, ws_bytes: int, device):
    """-> (ex_rowptr, ex_col, workspace, keep-alive): the exclusion CSR ``excl`` = (rowptr, col) as C arguments and the
    shared workspace of ``ws_bytes``."""
    rp, cp, keep = _csr_args(*excl, device)
    return rp, cp, _ws.get(max(256, int(ws_bytes)), device), keep


def _filter_arg(node_filter, N: int, device, unordered: bool):
    """(dl_node_filter* or None, keep-alive) for ``_scan_call``."""
    return (None, ()) if node_filter is None else node_filter._c_arg(N, device, unordered)


def _scan_call(name: str, *args) -> None:
    """The one call path of the scans: the C entry dl_score_``name``_dtype with ``args`` in that entry's own order —
    (Z, H, N, K, d, dt, t, ...), the rule of ``_filter_arg`` or None where the entry has it."""
    entry = f"dl_score_{name}_dtype"
    _lib.check(getattr(_lib.load(), entry)(*args), entry)


def _scan_ws_bytes(name: str, N: int, K: int, d: int, dt: int, *rest) -> int:
    """dl_score_``name``_workspace_bytes_dtype: the workspace of the scan on tables of type ``dt``."""
    return int(getattr(_lib.load(), f"dl_score_{name}_workspace_bytes_dtype")(N, K, d, dt, *rest))


def score_topk(Z, H, t: float, queries, k: int, exclude=None, exclude_self: bool = True, node_filter=None,
               table_dtype=torch.float32):
    """-> (index int64 [Q,k], logit f32 [Q,k], prob f32 [Q,k]): the k best candidates of every query node by the logit
    s(u,v) = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t) (pre-sigmoid link_pred, model.py:109-113), sorted (larger
    first, +inf first, NaN last, equal logits by index), prob = sigmoid(logit).  Candidates: every node outside the
    query's exclusion set (``exclusion_csr``) and, with ``exclude_self``, other than the query itself; rows with fewer than
    k are padded with index -1 / NaN.  ``node_filter`` (a ``NodeFilter``): only candidates whose group the query's group
    allows, on top of the exclusion.  Inference only (dl_score_topk: nothing of size Q x N is formed).
    ``table_dtype=torch.bfloat16`` (here and in every scan below): the scan runs on bf16 tables — bf16 tensors as they are,
    fp32 tensors rounded to nearest-even — with one matrix-core product per block instead of six and a third of the plane
    workspace; it returns bit for bit what the fp32 scan returns on the rounded tables (``Z.bfloat16().float()``)."""
    dt = _scan_dtype(table_dtype)
    Z, H, N, K, d = _scan_tables(Z, H, node_filter, False, table_dtype)
    k = int(k)
    if not 1 <= k <= RANK_MAX_K:
        raise ValueError(f"k={k} outside 1..{RANK_MAX_K}")
    q = _node_ids(queries, N, Z.device, "queries")
    Q = int(q.numel())
    index = _empty((Q, k), torch.int64, Z.device)
    logit = _empty((Q, k), torch.float32, Z.device)
    prob = _empty((Q, k), torch.float32, Z.device)
    if Q == 0:
        return index, logit, prob
    rp, cp, ws, _keep = _scan_buffers(exclusion_csr(exclude, N, Z.device), _scan_ws_bytes("topk", N, K, d, dt, Q, k, 0), Z.device)
    nf, _keep_nf = _filter_arg(node_filter, N, Z.device, False)
    _scan_call("topk", Z.data_ptr(), H.data_ptr(), N, K, d, dt, float(t), q.data_ptr(), Q, k, rp, cp,
               1 if exclude_self else 0, index.data_ptr(), logit.data_ptr(), prob.data_ptr(), ws.data_ptr(), ws.numel(),
               _stream(), nf)
    return index, logit, prob


def score_ranks(Z, H, t: float, src, dst, exclude=None, node_filter=None, table_dtype=torch.float32):
    """-> (greater, ties) int64 [P] for the target pairs (src[i], dst[i]): how many candidates of src[i] (every node other
    than src[i] and outside its exclusion set; dst[i] itself is never counted, and is ranked even when it is in the
    exclusion set — the filtered protocol) have a logit strictly above / equal to the target's, by value.  The target's
    logit is the one the scan computes.  rank = 1 + greater + ties / 2 (metrics.ranking_metrics).  ``node_filter``: only
    candidates the rule allows for src[i] are counted; a target is ranked whether or not it is allowed.  dl_score_ranks."""
    dt = _scan_dtype(table_dtype)
    Z, H, N, K, d = _scan_tables(Z, H, node_filter, False, table_dtype)
    s, v = _id_pairs(src, dst, N, Z.device, "src", "dst")
    T = int(s.numel())
    greater = _empty(T, torch.int64, Z.device)
    ties = _empty(T, torch.int64, Z.device)
    if T == 0:
        return greater, ties
    order = torch.argsort(s, stable=True)                              # targets grouped by query node
    queries, counts = torch.unique_consecutive(s[order], return_counts=True)
    Q = int(queries.numel())
    tptr = torch.zeros(Q + 1, dtype=torch.int32, device=Z.device)
    tptr[1:] = torch.cumsum(counts, dim=0).to(torch.int32)
    tdst = v[order].contiguous()
    queries = queries.to(torch.int32).contiguous()
    g_sorted = _empty(T, torch.int64, Z.device)
    t_sorted = _empty(T, torch.int64, Z.device)
    rp, cp, ws, _keep = _scan_buffers(exclusion_csr(exclude, N, Z.device), _scan_ws_bytes("topk", N, K, d, dt, Q, 0, T), Z.device)
    nf, _keep_nf = _filter_arg(node_filter, N, Z.device, False)
    _scan_call("ranks", Z.data_ptr(), H.data_ptr(), N, K, d, dt, float(t), queries.data_ptr(), Q, tptr.data_ptr(),
               tdst.data_ptr(), T, rp, cp, g_sorted.data_ptr(), t_sorted.data_ptr(), ws.data_ptr(), ws.numel(), _stream(), nf)
    greater[order] = g_sorted
    ties[order] = t_sorted
    return greater, ties


# ---------------------------------------------------------------------- the graph's most likely missing links (dl_score_mine.hip)
MINE_MAX_M = 65536
MINE_MAX_N = 46340


def _unordered_exclusion_csr(exclude, N: int, device):
    """``exclusion_csr`` of an UNORDERED pair set: every listed pair (a, b), in either order, as column max(a, b) of row
    min(a, b) — the only row dl_score_mine looks in."""
    rowptr, col = exclusion_csr(exclude, N, device)
    if rowptr is None:
        return None, None
    rows, cols = _csr_rows(rowptr), col.to(torch.int64)
    return exclusion_csr((torch.minimum(rows, cols), torch.maximum(rows, cols)), N, device)


def _operands(tables, K: int, d: int, dt: int):
    """The tables of a scan of the mining family — ``[(Z, H)]``: the unordered pairs of one node set, a triangle;
    ``[(ZA, HA), (ZB, HB)]``: rows of A against rows of B, a rectangle — as their C entries take them -> (the suffix of
    the entries' names, the leading arguments of the entry, the arguments of its sizer, the rows per side)."""
    (ZA, HA), nA = tables[0], int(tables[0][0].shape[0])
    if len(tables) == 1:
        return "", (ZA.data_ptr(), HA.data_ptr(), nA, K, d, dt), (nA, K, d, dt), (nA,)
    (ZB, HB), nB = tables[1], int(tables[1][0].shape[0])
    return ("_between", (ZA.data_ptr(), HA.data_ptr(), nA, ZB.data_ptr(), HB.data_ptr(), nB, K, d, dt), (nA, nB, K, d, dt),
            (nA, nB))


def _mine(tables, K: int, d: int, dt: int, t, m: int, excl, min_logit, nf):
    """One mining call on prepared ``tables`` (``_operands``), exclusion CSR ``excl`` = (rowptr, col) and rule argument
    ``nf`` -> (src, dst, logit, prob), local to the tables, cut to the count (the one host read)."""
    between, lead, shape, _rows = _operands(tables, K, d, dt)
    dev = tables[0][0].device
    rp, cp, ws, _keep = _scan_buffers(excl, _scan_ws_bytes("mine" + between, *shape, m), dev)
    src, dst = _empty(max(m, 0), torch.int32, dev), _empty(max(m, 0), torch.int32, dev)
    logit, prob = _empty(max(m, 0), torch.float32, dev), _empty(max(m, 0), torch.float32, dev)
    count = _empty(1, torch.int64, dev)
    _scan_call("mine" + between, *lead, float(t), rp, cp, float(min_logit), m, src.data_ptr(), dst.data_ptr(), logit.data_ptr(),
               prob.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), _stream(), nf)
    c = int(count.item())
    return src[:c], dst[:c], logit[:c], prob[:c]


def score_mine(Z, H, t: float, m: int, exclude=None, min_logit: float = float("-inf"), node_filter=None,
               table_dtype=torch.float32):
    """-> (src int32 [c], dst int32 [c], logit f32 [c], prob f32 [c]), c = min(m, eligible): the m best unordered pairs
    src < dst of the WHOLE graph by the logit s(u,v) = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t) (pre-sigmoid
    link_pred), sorted in ``score_topk``'s order (larger first, +inf first, equal logits by src * N + dst), with the bits
    ``score_topk`` returns for query src, candidate dst.  ``exclude`` (a ``Graph``, a dense [N,N] mask or ``(rows, cols)``)
    is taken as a set of unordered pairs; a pair is eligible iff its logit is >= ``min_logit`` (NaN never is).
    1 <= m <= 65,536, N <= 46,340.  Inference only; nothing of size N x N is formed (dl_score_mine), and the one host read
    is that of the count, at the very end.  ``node_filter`` (a symmetric ``NodeFilter``): only pairs whose groups the rule
    allows, on top of the exclusion and the floor."""
    dt = _scan_dtype(table_dtype)
    Z, H, N, K, d = _scan_tables(Z, H, node_filter, True, table_dtype)
    m = int(m)
    excl = _unordered_exclusion_csr(exclude, N, Z.device)
    nf, _keep_nf = _filter_arg(node_filter, N, Z.device, True)
    return _mine([(Z, H)], K, d, dt, t, m, excl, min_logit, nf)


# ---------------------------------------------------------------------- every pair above a floor, as a CSR (DEG / FILL scans)
LINKS_MAX_N = MINE_MAX_N
_INT64_MAX = (1 << 63) - 1


def _links_count(tables, K: int, d: int, dt: int, t, excl, min_logit, nf, budget=None):
    """The count pass of a link graph on prepared ``tables`` (``_operands``), exclusion CSR ``excl`` and rule argument
    ``nf``; ``budget``: the m of the budgeted graph (one node set only) -> (the int64 rowptr of every side, on the device;
    the name of the graph's entries; the arguments the fill pass shares with the count; keep-alive)."""
    between, lead, shape, rows = _operands(tables, K, d, dt)
    name = "links" + (between if budget is None else "_top")
    dev = tables[0][0].device
    ex = _csr_args(*excl, dev)
    # a workspace of its own, held across the two calls: the shared grow-only buffer may be handed out (and, under DL_POISON,
    # refilled) in between, and the fill pass reads the planes, the cell offsets and (budgeted) the threshold the count left
    ws = _empty(max(256, _scan_ws_bytes(name, *shape)), torch.uint8, dev)
    rowptrs = [_empty(n + 1, torch.int64, dev) for n in rows]
    head = (*lead, float(t), ex[0], ex[1], float(min_logit), *(() if budget is None else (budget,)), nf, ws.data_ptr(),
            ws.numel(), *map(torch.Tensor.data_ptr, rowptrs))
    _scan_call(name + "_count", *head, _stream())
    return rowptrs, name, head, (tables, ex, ws)


def _links_fill(rowptrs, name: str, head):
    """The fill pass of a link graph: the one host read, of the number of entries (every side holds every pair once, a
    symmetric CSR twice), three arrays of that length per side, and the fill entry with the count's arguments ``head`` ->
    a (rowptr, col, logit, prob) per side."""
    nnz = int(rowptrs[0][-1].item())                                  # the one host read
    dev = rowptrs[0].device
    sides, args = [], []
    for rowptr in rowptrs:
        col, logit, prob = _empty(nnz, torch.int32, dev), _empty(nnz, torch.float32, dev), _empty(nnz, torch.float32, dev)
        sides.append((rowptr, col, logit, prob))
        args += (nnz, col.data_ptr(), logit.data_ptr(), prob.data_ptr())
    _scan_call(name + "_fill", *head, *args, _stream())
    return sides


def _links(tables, K: int, d: int, dt: int, t, excl, min_logit, nf, fill: bool = True):
    """Both passes -> a (rowptr, col, logit, prob) per side; ``fill=False``: the count alone, col / logit / prob None."""
    rowptrs, name, head, _keep = _links_count(tables, K, d, dt, t, excl, min_logit, nf)
    return _links_fill(rowptrs, name, head) if fill else [(rowptr, None, None, None) for rowptr in rowptrs]


def _graph_count(Z, H, t, min_logit, exclude, node_filter, table_dtype, budget=None):
    """How ``score_links``, ``score_link_degrees`` and (with the ``budget`` m) ``score_top_links`` start: the refusals, the
    exclusion CSR, the rule, then ``_links_count`` on the one table pair."""
    dt = _scan_dtype(table_dtype)
    Z, H, N, K, d = _scan_tables(Z, H, node_filter, True, table_dtype)
    if N > LINKS_MAX_N:
        raise ValueError(f"N={N} above {LINKS_MAX_N} (the tile-pair walk of dl_score_mine)")
    if budget is None:
        excl = _unordered_exclusion_csr(exclude, N, Z.device)
    else:
        budget = min(int(budget), _INT64_MAX)
        ex = _exclusion_arg(exclude, N, Z.device, keyed=False)
        excl = (ex.rowptr, ex.col)
    nf, keep_nf = _filter_arg(node_filter, N, Z.device, True)
    rowptrs, name, head, keep = _links_count([(Z, H)], K, d, dt, t, excl, min_logit, nf, budget)
    return rowptrs, name, head, (keep, keep_nf)


def score_links(Z, H, t: float, min_logit: float, exclude=None, node_filter=None, table_dtype=torch.float32):
    """-> (rowptr int64 [N+1], col int32 [nnz], logit f32 [nnz], prob f32 [nnz]): the predicted graph, EVERY unordered pair
    whose logit s(u,v) = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t) (pre-sigmoid link_pred) reaches ``min_logit``, as a
    symmetric CSR over all N nodes — each pair as (u, v) and as (v, u) with the same bits, columns ascending within a row,
    prob = sigmoid(logit).  Eligibility is ``score_mine``'s without m: u != v, outside ``exclude`` (a ``Graph``, a dense
    [N,N] mask or ``(rows, cols)``, taken as unordered pairs), allowed by ``node_filter`` (a symmetric ``NodeFilter``), NaN
    never; the bits are those of ``score_pair_logits(min(u, v), max(u, v))``.  N <= 46,340, fp32 or bf16 tables.  Inference only;
    nothing of size N x N is formed (dl_score_links_count / dl_score_links_fill: two scans), there is no cap on nnz, and the
    one host read is that of rowptr[N], between the scans, to allocate the outputs.  Same bits on every call."""
    rowptrs, name, head, _keep = _graph_count(Z, H, t, min_logit, exclude, node_filter, table_dtype)
    return _links_fill(rowptrs, name, head)[0]


def score_link_degrees(Z, H, t: float, min_logit: float, exclude=None, node_filter=None, table_dtype=torch.float32):
    """-> int64 [N]: the predicted degree of every node, i.e. how many partners ``score_links`` would list for it — the
    count pass alone (dl_score_links_count): one scan, no host read, no fill."""
    (rowptr,), _name, _head, _keep = _graph_count(Z, H, t, min_logit, exclude, node_filter, table_dtype)
    return rowptr[1:] - rowptr[:-1]


# ---------------------------------------------------------------------- the m best pairs, any m, as a CSR (select, then DEG / FILL)
def score_top_links(Z, H, t: float, m: int, exclude=None, min_logit: float = float("-inf"), node_filter=None,
                    table_dtype=torch.float32):
    """-> (rowptr int64 [N+1], col int32 [nnz], logit f32 [nnz], prob f32 [nnz]), nnz = 2 min(m, eligible): the m most
    likely unordered pairs of the WHOLE graph, for any m >= 1, in ``score_links``' layout — the set ``score_mine`` would list
    if it had no cap (its eligibility: ``exclude``, ``node_filter``, logit >= ``min_logit``, NaN never; its order: larger
    logit first, equal logits by src * N + dst, so a cut through tied logits keeps the smaller), each pair as (u, v) and as
    (v, u) with the bits of ``score_pair_logits(min(u, v), max(u, v))``, columns ascending within a row, not sorted by
    logit.  An m above N (N - 1) / 2 means every eligible pair.  ``exclude``: as in ``score_links``, or a prepared
    ``pair_exclusion(...)``, which skips the normalisation per call.  N <= 46,340, fp32 or bf16 tables.  Inference only;
    nothing of size N x N is formed (dl_score_links_top_count / _fill: the select of ``score_mine``, at most six histogram
    scans, then the two scans of ``score_links`` under the threshold key it left on the device), and the one host read is
    that of rowptr[N], to allocate the outputs.  Same bits on every call."""
    rowptrs, name, head, _keep = _graph_count(Z, H, t, min_logit, exclude, node_filter, table_dtype, budget=m)
    return _links_fill(rowptrs, name, head)[0]


# ---------------------------------------------------------------------- where given pairs stand among ALL pairs (COUNT scan)
def _order_keys(logit: torch.Tensor) -> torch.Tensor:
    """The scans' total order of fp32 values as int64 keys in [0, 2^32): NaN -> 0, -0 as +0, larger value = larger key."""
    x = torch.where(logit == 0, torch.zeros_like(logit), logit)
    b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b + 0x80000000)
    return torch.where(torch.isnan(logit), torch.zeros_like(key), key)


PairExclusion = namedtuple("PairExclusion", ["n_nodes", "rowptr", "col", "key", "n_pairs"])


def pair_exclusion(exclude, N: int, device) -> PairExclusion:
    """An exclusion set normalised once for ``score_pair_ranks`` (a caller with a fixed graph passes the result as
    ``exclude`` and skips the normalisation per call): the CSR of ``_unordered_exclusion_csr``, its sorted pair keys
    u * N + v and the int64 [1] number of pairs u < v among them ((u, u) entries exclude nothing)."""
    rowptr, col = _unordered_exclusion_csr(exclude, N, device)
    if rowptr is None:
        return PairExclusion(N, None, None, None, torch.zeros(1, dtype=torch.int64, device=device))
    rows, cols = _csr_rows(rowptr), col.to(torch.int64)
    return PairExclusion(N, rowptr, col, rows * N + cols, (cols > rows).sum().reshape(1))


def _exclusion_arg(exclude, N: int, device, keyed: bool) -> PairExclusion:
    """``exclude`` as a scan takes it: a prepared ``PairExclusion``, accepted if it is of N nodes and on ``device``, or a raw
    set of unordered pairs, normalised here — with its keys and pair count (``pair_exclusion``) if ``keyed``, else the CSR
    alone."""
    if not isinstance(exclude, PairExclusion):
        if keyed:
            return pair_exclusion(exclude, N, device)
        return PairExclusion(N, *_unordered_exclusion_csr(exclude, N, device), None, None)
    if exclude.n_nodes != N:
        raise ValueError(f"exclusion set of {exclude.n_nodes} nodes, expected {N}")
    if exclude.rowptr is not None and exclude.rowptr.device != device:
        raise ValueError(f"exclusion set on {exclude.rowptr.device}, tables on {device}")
    return exclude


def _score_pairs(name: str, Z, H, t: float, a, b, table_dtype, per_factor: bool):
    """What ``score_pair_logits`` and ``score_pair_terms`` share: tables, the two id arrays of one length, the fp32 outputs
    (three [P, K] arrays if ``per_factor``, else one [P]), the workspace and the call of dl_score_``name``_dtype (none for
    P = 0) -> the list of outputs."""
    dt = _scan_dtype(table_dtype)
    Z, H, N, K, d = _rank_tables(Z, H, table_dtype)
    a, b = _id_pairs(a, b, N, Z.device, "a", "b")
    P = int(a.numel())
    out = [_empty((P, K) if per_factor else (P,), torch.float32, Z.device) for _ in range(3 if per_factor else 1)]
    if P:
        ws = _ws.get(max(256, _scan_ws_bytes(name, N, K, d, dt)), Z.device)
        _scan_call(name, Z.data_ptr(), H.data_ptr(), N, K, d, dt, float(t), a.data_ptr(), b.data_ptr(), P,
                   *(o.data_ptr() for o in out), ws.data_ptr(), ws.numel(), _stream())
    return out


def score_pair_logits(Z, H, t: float, a, b, table_dtype=torch.float32):
    """-> logit f32 [P]: s(a[i], b[i]) with row a[i] as the A operand, from the products of the scans — the bits
    ``score_topk`` returns for query a[i], candidate b[i] (dl_score_pair_logits; a -0 comes back as +0, as the keyed
    outputs of ``score_topk`` and ``score_mine`` report it)."""
    (logit,) = _score_pairs("pair_logits", Z, H, t, a, b, table_dtype, per_factor=False)
    return torch.where(logit == 0, torch.zeros_like(logit), logit)


class PairTerms(namedtuple("PairTerms", ["e", "q", "cum"])):
    """The per-factor terms of scored pairs (``score_pair_terms``), fp32 [P, K] each: ``e`` = exp(z_k[a].z_k[b] / t),
    ``q`` = h_k[a].h_k[b], ``cum`` = the scan's running sum after factor k (its last column is the logit)."""
    __slots__ = ()

    @property
    def logit(self) -> torch.Tensor:
        """f32 [P]: ``cum[:, -1]`` with a -0 reported as +0 — the bits the scans report for the pair."""
        x = self.cum[:, -1]
        return torch.where(x == 0, torch.zeros_like(x), x)

    @property
    def contrib(self) -> torch.Tensor:
        """f32 [P, K]: what factor k added to the sum: cum[:, 0], then cum[:, k] - cum[:, k-1]."""
        out = self.cum.clone()
        out[:, 1:] -= self.cum[:, :-1]
        return out

    @property
    def factor(self) -> torch.Tensor:
        """int64 [P]: the factor with the largest contribution (the first of equals), -1 where the row holds a NaN."""
        c = self.contrib
        top = c.max(dim=1, keepdim=True).values
        first = (c == top).to(torch.int64).argmax(dim=1)          # argmax of 0/1 values: the first 1
        return torch.where(torch.isnan(c).any(dim=1), torch.full_like(first, -1), first)


def score_pair_terms(Z, H, t: float, a, b, table_dtype=torch.float32) -> PairTerms:
    """-> PairTerms(e, q, cum), fp32 [P, K] each: WHY the pair (a[i], b[i]) scores as it does — per factor k the routing
    weight e = exp(z_k[a].z_k[b] / t), the Gram product q = h_k[a].h_k[b] and the running sum cum of the very pass
    ``score_pair_logits`` runs (dl_score_pair_terms: same gathers and products, row a[i] as the A operand).
    ``cum[:, -1]`` has the bits ``score_pair_logits`` returns, hence those ``score_topk``, ``score_mine`` and
    ``score_links`` list (``.logit``: with their -0 -> +0); ``cum[:, k]`` is the logit of the tables cut to factors 0..k.
    ``.contrib`` and ``.factor`` name the factor that makes the link.  Inference only."""
    return PairTerms(*_score_pairs("pair_terms", Z, H, t, a, b, table_dtype, per_factor=True))


def score_pair_ranks_counted(Z, H, t: float, src, dst, exclude=None, node_filter=None, table_dtype=torch.float32):
    """The hook of the tests and of tools/pair_rank_time.py, not part of the interface: ``score_pair_ranks`` and, as a fifth
    value, the int64 [1] DEVICE count of the candidates the scan counted, which equals N (N - 1) / 2 - |excluded pairs| (the
    one exact check that works where nothing can be enumerated; under a ``node_filter``: the pairs the rule allows, less
    the excluded ones among them)."""
    dt = _scan_dtype(table_dtype)
    Z, H, N, K, d = _scan_tables(Z, H, node_filter, True, table_dtype)
    dev = Z.device
    s, v = _id_pairs(src, dst, N, dev, "src", "dst")
    if bool((s == v).any()):
        raise ValueError("a target is a self pair (src[i] == dst[i])")
    T = int(s.numel())
    ex = _exclusion_arg(exclude, N, dev, keyed=True)
    rowptr, col, ex_key = ex.rowptr, ex.col, ex.key
    total = N * (N - 1) // 2 - ex.n_pairs
    nf, _keep_nf = _filter_arg(node_filter, N, dev, True)
    if node_filter is not None:                                       # allowed pairs, less the excluded ones among them
        total = node_filter._n_pairs_allowed()
        if ex_key is not None and ex_key.numel():
            er, ec = torch.div(ex_key, N, rounding_mode="floor"), ex_key % N
            total = total - ((ec > er) & node_filter.allowed(er, ec, unordered=True)).sum().reshape(1)
    if T == 0:
        e = torch.zeros(0, dtype=torch.int64, device=dev)
        return e, e.clone(), torch.zeros(0, dtype=torch.float32, device=dev), e.clone(), total
    lo, hi = torch.minimum(s, v).contiguous(), torch.maximum(s, v).contiguous()
    logit = score_pair_logits(Z, H, t, lo, hi, table_dtype)           # the smaller endpoint as the A operand
    key = _order_keys(logit)
    ksorted, order = torch.sort(key, stable=True)
    first = torch.searchsorted(ksorted, ksorted)                      # first place of each target's value
    tord = torch.where(ksorted >= 0x80000000, ksorted - 0x100000000, ksorted).to(torch.int32).contiguous()      # uint32 bits
    above = _empty(T + 1, torch.int64, dev)
    equal = _empty(T + 1, torch.int64, dev)
    counted = _empty(1, torch.int64, dev)
    rp, cp, ws, _keep = _scan_buffers((rowptr, col), _scan_ws_bytes("pair_ranks", N, K, d, dt), dev)
    _scan_call("pair_ranks", Z.data_ptr(), H.data_ptr(), N, K, d, dt, float(t), rp, cp, tord.data_ptr(), T, above.data_ptr(),
               equal.data_ptr(), counted.data_ptr(), ws.data_ptr(), ws.numel(), _stream(), nf)
    cs = torch.cumsum(above, dim=0)
    g_sorted = cs[T] - cs[:T]                                         # candidates that found more than p targets below them
    t_sorted = equal[first]
    in_c = torch.ones(T, dtype=torch.int64, device=dev)               # the target itself is a candidate unless excluded
    if rowptr is not None and ex_key.numel():
        tkey = lo.to(torch.int64) * N + hi.to(torch.int64)
        pos = torch.searchsorted(ex_key, tkey).clamp_(max=ex_key.numel() - 1)
        in_c = (ex_key[pos] != tkey).to(torch.int64)
    if node_filter is not None:                                       # ... and only where the rule allows it
        in_c = in_c * node_filter.allowed(lo, hi, unordered=True).to(torch.int64)
    greater = torch.empty(T, dtype=torch.int64, device=dev)
    ties = torch.empty(T, dtype=torch.int64, device=dev)
    greater[order] = g_sorted
    ties[order] = t_sorted
    return greater, ties - in_c, logit, total - in_c, counted


def score_pair_ranks(Z, H, t: float, src, dst, exclude=None, node_filter=None, table_dtype=torch.float32):
    """-> (greater int64, ties int64, logit f32, n_others int64), each [T]: where the unordered target pairs
    {src[i], dst[i]} (either orientation; duplicates allowed; no self pairs) stand among ALL unordered pairs u < v < N of
    the graph outside ``exclude`` (a set of unordered pairs, as in ``score_mine``, or a prepared ``pair_exclusion``).  logit[i] is formed with the smaller
    endpoint as the A operand (the bits ``score_mine`` lists); greater / ties count the candidates other than the target
    itself whose logit is strictly above / equal by value (+inf above everything finite, -0 equal to +0, NaN below
    everything and equal only to NaN).  The filtered protocol of ``score_ranks``: a target is ranked whether or not it is
    excluded, other targets count as candidates unless excluded.  n_others[i] = candidates - [target i is one], so
    greater + ties <= n_others; rank = 1 + greater + ties / 2 (metrics.global_ranking_metrics).  Inference only; one
    target pass and ONE scan (dl_score_pair_logits, dl_score_pair_ranks), nothing of size N x N, no cap at N = 46,340.
    ``node_filter`` (a symmetric ``NodeFilter``): the candidates are the pairs the rule allows outside ``exclude``; a target
    is ranked whether or not it is allowed."""
    return score_pair_ranks_counted(Z, H, t, src, dst, exclude, node_filter, table_dtype)[:4]


# ---------------------------------------------------------------------- two node sets: rows of A against rows of B (RECT scans)
BETWEEN_MAX_N = MINE_MAX_N
BLOCK_NODES = 46208                                                    # the default block of the *_blocks scans: 361 tiles
BLOCKS_MAX_N = 8388480                                                 # DL_SCORE_PAIR_RANKS_MAX_N


def bipartite_exclusion_csr(exclude, nA: int, nB: int, device=None):
    """An exclusion set between two node sets as the CSR the rectangular scans take: (rowptr int32 [nA+1], col int32) with
    B-local, strictly ascending columns per row of A, or (None, None) for ``exclude=None``.  ``exclude``: ``(rows_a,
    cols_b)`` index sequences or a dense [nA, nB] mask (entries != 0).  Duplicates collapse."""
    if exclude is None:
        return None, None
    nA, nB = int(nA), int(nB)
    key = _pair_keys(exclude, nA, nB, device, ("(rows_a, cols_b)", f"[0, {nA}) x [0, {nB})", "[nA, nB]"))
    return _local_csr(*_split_keys(key, nB), nA)


def _between_rule(rule, nA: int, nB: int, device):
    """``rule`` = (groups_a [nA], groups_b [nB], allow [g, h]) -> (groups_a uint8, groups_b uint8, allow words int64 [n],
    n): pair (a, b) is allowed iff allow[groups_a[a], groups_b[b]]; the row of A decides, so allow need not be symmetric."""
    if not isinstance(rule, (tuple, list)) or len(rule) != 3:
        raise TypeError("rule is (groups_a, groups_b, allow[g, h])")
    ga, gb = (torch.as_tensor(v) for v in rule[:2])
    allow = torch.as_tensor(rule[2]).detach().to("cpu") != 0
    _group_array(ga, "groups_a", nA)
    _group_array(gb, "groups_b", nB)
    if allow.dim() != 2 or not (1 <= allow.shape[0] <= 64 and 1 <= allow.shape[1] <= 64):
        raise ValueError(f"allow must be [g, h] with 1 <= g, h <= 64, got {tuple(allow.shape)}")
    _group_range(ga, int(allow.shape[0]), "groups_a")
    _group_range(gb, int(allow.shape[1]), "groups_b")
    n = int(max(allow.shape))
    square = torch.zeros(n, n, dtype=torch.bool)
    square[:allow.shape[0], :allow.shape[1]] = allow
    return (ga.to(device=device, dtype=torch.uint8).contiguous(), gb.to(device=device, dtype=torch.uint8).contiguous(),
            NodeFilter._pack(square).to(device), n)


def _between_filter_arg(groups_a, groups_b, words, n_groups: int):
    """(byref(dl_node_filter_between), keep-alive) of prepared device arrays."""
    st = _lib.DlNodeFilterBetween(groups_a.data_ptr(), groups_b.data_ptr(), n_groups, words.data_ptr())
    return C.byref(st), (st, groups_a, groups_b, words)


def _between_tables(ZA, HA, ZB, HB, table_dtype):
    if ZA.dim() == 3 and ZB.dim() == 3 and tuple(ZA.shape[1:]) != tuple(ZB.shape[1:]):
        raise ValueError(f"tables A are {list(ZA.shape)}, tables B {list(ZB.shape)}: K and d must agree")
    ZA, HA, nA, K, d = _rank_tables(ZA, HA, table_dtype)
    ZB, HB, nB, _, _ = _rank_tables(ZB, HB, table_dtype)
    if ZA.device != ZB.device:
        raise ValueError(f"tables A on {ZA.device}, tables B on {ZB.device}")
    for n, what in ((nA, "nA"), (nB, "nB")):
        if n > BETWEEN_MAX_N:
            raise ValueError(f"{what}={n} above {BETWEEN_MAX_N} (the pair index a nB + b of the rectangular scans)")
    return ZA, HA, ZB, HB, nA, nB, K, d


def _between_start(ZA, HA, ZB, HB, rule, table_dtype):
    """How the scans between two node sets start: the refusals of the rule, then of the tables -> (tables as ``_operands``
    takes them, nA, nB, K, d, dt, rule argument, its keep-alive)."""
    dt = _scan_dtype(table_dtype)
    ruled = None if rule is None else _between_rule(rule, int(ZA.shape[0]), int(ZB.shape[0]), ZA.device)      # its refusals first
    ZA, HA, ZB, HB, nA, nB, K, d = _between_tables(ZA, HA, ZB, HB, table_dtype)
    nf, keep_nf = (None, ()) if ruled is None else _between_filter_arg(*ruled)
    return [(ZA, HA), (ZB, HB)], nA, nB, K, d, dt, nf, keep_nf


def score_mine_between(ZA, HA, ZB, HB, t: float, m: int, exclude=None, min_logit: float = float("-inf"), rule=None,
                       table_dtype=torch.float32):
    """-> (src int32 [c], dst int32 [c], logit f32 [c], prob f32 [c]), c = min(m, eligible): the m best pairs (a, b) of rows
    of tables A [nA,K,d] against rows of tables B [nB,K,d] — users x items, new nodes x old nodes — by the logit of
    ``score_mine``, rows of A as the A operand: the bits ``score_pair_logits`` gives for (a, nA + b) on ``cat(A, B)``.  src
    is A-local, dst B-local; the order is ``score_mine``'s (larger logit first, equal logits by src * nB + dst).  Every one of
    the nA nB pairs is a candidate (there is no src < dst) unless it is in ``exclude`` (``(rows_a, cols_b)`` or a dense
    [nA, nB] mask), forbidden by ``rule`` = (groups_a, groups_b, allow[g, h]) (allowed iff allow[groups_a[a], groups_b[b]];
    it need not be symmetric) or below ``min_logit`` (NaN never is eligible).  1 <= m <= 65,536, nA, nB <= 46,340.  Only the
    ceil(nA/128) x ceil(nB/128) tile pairs of the rectangle are formed (dl_score_mine_between_dtype), where
    ``NodeFilter.between`` on the concatenated table walks (nA + nB)^2 / 2 products for the same result."""
    tables, nA, nB, K, d, dt, nf, _keep_nf = _between_start(ZA, HA, ZB, HB, rule, table_dtype)
    return _mine(tables, K, d, dt, t, int(m), bipartite_exclusion_csr(exclude, nA, nB, tables[0][0].device), min_logit, nf)


LinksBetween = namedtuple("LinksBetween", ["ab", "ba"])


def score_links_between(ZA, HA, ZB, HB, t: float, min_logit: float, exclude=None, rule=None,
                        table_dtype=torch.float32) -> LinksBetween:
    """-> LinksBetween(ab, ba), two (rowptr int64, col int32, logit f32, prob f32) tuples: EVERY pair (a, b) of rows of A
    against rows of B whose logit reaches ``min_logit``, as the CSR of the A side (``ab``: rowptr [nA+1], columns = rows of
    B) and of the B side (``ba``: rowptr [nB+1], columns = rows of A).  Every pair appears in both with the same bits,
    columns ascending within a row, a -0 as +0.  Logit, eligibility, ``exclude`` and ``rule`` as in ``score_mine_between``;
    two scans and the one host read of the number of pairs, as in ``score_links`` (dl_score_links_between_count_dtype /
    _fill_dtype).  nA, nB <= 46,340."""
    tables, nA, nB, K, d, dt, nf, _keep_nf = _between_start(ZA, HA, ZB, HB, rule, table_dtype)
    return LinksBetween(*_links(tables, K, d, dt, t, bipartite_exclusion_csr(exclude, nA, nB, tables[0][0].device), min_logit, nf))


# ---------------------------------------------------------------------- any N: diagonal blocks and rectangles, merged on the host
def _block_bounds(N: int, block_nodes):
    bn = BLOCK_NODES if block_nodes is None else int(block_nodes)
    if bn < 128 or bn % 128 or bn > BLOCK_NODES:
        raise ValueError(f"block_nodes={bn}: a multiple of 128 in 128..{BLOCK_NODES}")
    if N > BLOCKS_MAX_N:
        raise ValueError(f"N={N} above {BLOCKS_MAX_N}")
    return bn, [(lo, min(lo + bn, N)) for lo in range(0, N, bn)]


class _BlockWindows:
    """What the windows of a blocked scan share: the tables, the blocks, the exclusion set cut by window (ONE pass over the
    pairs u < v: a stable sort by (block of u, block of v), then a slice per window, shifted to local ids) and the rule."""

    def __init__(self, Z, H, t, exclude, node_filter, table_dtype, block_nodes):
        self.dt = _scan_dtype(table_dtype)
        _filter_check(node_filter, Z, True)                            # the host-side refusals, ahead of the tables' own
        self.bn, self.blocks = _block_bounds(int(Z.shape[0]), block_nodes)
        self.Z, self.H, self.N, self.K, self.d = _rank_tables(Z, H, table_dtype)
        self.t, self.dev = float(t), self.Z.device
        nb = len(self.blocks)
        self.filter = node_filter
        if node_filter is not None:
            node_filter._c_arg(self.N, self.dev, True)                 # its refusals (device, symmetry), ahead of any launch
        rowptr, col = _unordered_exclusion_csr(exclude, self.N, self.dev)
        self.ex = None
        if rowptr is not None and col.numel():
            r, c = _csr_rows(rowptr), col.to(torch.int64)
            keep = c > r                                              # (u, u) entries exclude nothing
            r, c = r[keep], c[keep]
            w = torch.div(r, self.bn, rounding_mode="floor") * nb + torch.div(c, self.bn, rounding_mode="floor")
            order = torch.argsort(w, stable=True)                     # within a window: rows ascending, columns ascending
            start = torch.zeros(nb * nb + 1, dtype=torch.int64)
            start[1:] = torch.cumsum(torch.bincount(w, minlength=nb * nb), dim=0).cpu()      # one host read, nb^2 numbers
            self.ex = (r[order], c[order], start.tolist())

    def windows(self):
        """(i, j) with i <= j, row-major: the pieces of every row block then arrive in ascending column blocks."""
        nb = len(self.blocks)
        return [(i, j) for i in range(nb) for j in range(i, nb)]

    def tables(self, i, j):
        """The tables of window (i, j) as ``_operands`` takes them: the row slice of block i and, off the diagonal, of j."""
        return [(self.Z[lo:hi], self.H[lo:hi]) for lo, hi in ([self.blocks[i]] if i == j else [self.blocks[i], self.blocks[j]])]

    def exclusion(self, i, j):
        """The sub-CSR of window (i, j): rows local to block i, columns local to block j (None, None: nothing excluded)."""
        if self.ex is None:
            return None, None
        r, c, start = self.ex
        w = i * len(self.blocks) + j
        s, e = start[w], start[w + 1]
        if s == e:
            return None, None
        (lo_i, hi_i), (lo_j, _) = self.blocks[i], self.blocks[j]
        return _local_csr(r[s:e] - lo_i, c[s:e] - lo_j, hi_i - lo_i)

    def rule(self, i, j):
        """The rule of window (i, j) as its entry takes it: a dl_node_filter on the group bytes of block i (diagonal), or a
        dl_node_filter_between on those of blocks i and j; the unordered scans' symmetric allow words either way."""
        f = self.filter
        if f is None:
            return None, ()
        ga = f.groups[self.blocks[i][0]:self.blocks[i][1]]
        if i == j:
            st = _lib.DlNodeFilter(ga.data_ptr(), f.n_groups, f._pair_words.data_ptr())
            return C.byref(st), (st, ga, f._pair_words)
        return _between_filter_arg(ga, f.groups[self.blocks[j][0]:self.blocks[j][1]], f._pair_words, f.n_groups)


def _merge_top(best, new, N: int, m: int):
    """The m best of two lists of (src int64, dst int64, logit, prob) in the scans' total order: larger order key first,
    equal keys by the 64-bit global pair index src * N + dst."""
    if best is None:
        cat = new
    else:
        cat = tuple(torch.cat((a, b)) for a, b in zip(best, new))
    src, dst, logit, prob = cat
    by_index = torch.argsort(src * N + dst, stable=True)
    by_key = torch.argsort(_order_keys(logit[by_index]), stable=True, descending=True)
    take = by_index[by_key][:m]
    return src[take], dst[take], logit[take], prob[take]


def score_mine_blocks(Z, H, t: float, m: int, exclude=None, min_logit: float = float("-inf"), node_filter=None,
                      table_dtype=torch.float32, block_nodes=None):
    """``score_mine`` for ANY N up to 8,388,480: -> (src int32 [c], dst int32 [c], logit f32 [c], prob f32 [c]) with
    src < dst in GLOBAL ids, c = min(m, eligible), larger logit first, equal logits by the 64-bit src * N + dst.  The nodes
    are cut into contiguous blocks of ``block_nodes`` rows (a multiple of 128, default 46,208); every diagonal block goes
    through dl_score_mine_dtype on its row slice, every pair of blocks i < j through dl_score_mine_between_dtype with block i
    as A — the bits the triangular scan forms for u < v — and the windows' lists are merged with torch.  Once m pairs are
    held, their last logit is the (inclusive) floor of the windows after, so ties survive.  For N <= 46,340 the result is bit
    for bit ``score_mine``'s, for every block size.  Peak memory: the workspace of ONE window and O(N + m) arrays; one host
    read per window (its count)."""
    m = int(m)
    if not 1 <= m <= MINE_MAX_M:
        raise ValueError(f"m={m} outside 1..{MINE_MAX_M}")
    W = _BlockWindows(Z, H, t, exclude, node_filter, table_dtype, block_nodes)
    floor, best = float(min_logit), None
    n0 = W.blocks[0][1] - W.blocks[0][0]                               # the shared workspace once, at the largest window's size
    need = _scan_ws_bytes("mine", n0, W.K, W.d, W.dt, m)
    if len(W.blocks) > 1:
        need = max(need, _scan_ws_bytes("mine_between", n0, W.blocks[1][1] - W.blocks[1][0], W.K, W.d, W.dt, m))
    _ws.get(max(256, need), W.dev)
    for i, j in W.windows():
        nf, _keep_nf = W.rule(i, j)
        src, dst, logit, prob = _mine(W.tables(i, j), W.K, W.d, W.dt, W.t, m, W.exclusion(i, j), floor, nf)
        if src.numel() == 0:
            continue
        best = _merge_top(best, (src.to(torch.int64) + W.blocks[i][0], dst.to(torch.int64) + W.blocks[j][0], logit, prob), W.N, m)
        if best[0].numel() == m:                                      # full: nothing below the m-th can enter any more
            last = float(best[2][-1].item())
            floor = max(floor, last) if last == last else floor
    if best is None:
        e = torch.zeros(0, dtype=torch.int32, device=W.dev)
        return e, e.clone(), torch.zeros(0, dtype=torch.float32, device=W.dev), torch.zeros(0, dtype=torch.float32, device=W.dev)
    return best[0].to(torch.int32), best[1].to(torch.int32), best[2], best[3]


def _links_windows(W: _BlockWindows, min_logit: float, fill: bool):
    """Runs every window of a blocked link graph; yields, per window side, (row block, column offset, piece) where piece is
    (rowptr int64 [rows+1], col, logit, prob) — col / logit / prob are None for ``fill=False`` (the count pass alone)."""
    for i, j in W.windows():
        nf, _keep_nf = W.rule(i, j)
        sides = _links(W.tables(i, j), W.K, W.d, W.dt, W.t, W.exclusion(i, j), min_logit, nf, fill)
        yield i, W.blocks[j][0], sides[0]                              # rows of block i, columns local to block j
        if i != j:
            yield j, W.blocks[i][0], sides[1]


def score_link_degrees_blocks(Z, H, t: float, min_logit: float, exclude=None, node_filter=None, table_dtype=torch.float32,
                              block_nodes=None):
    """``score_link_degrees`` for any N up to 8,388,480 -> int64 [N]: the count passes of the windows of
    ``score_links_blocks`` alone, added up per node."""
    W = _BlockWindows(Z, H, t, exclude, node_filter, table_dtype, block_nodes)
    deg = torch.zeros(W.N, dtype=torch.int64, device=W.dev)
    for b, _off, (rowptr, _c, _l, _p) in _links_windows(W, min_logit, fill=False):
        lo, hi = W.blocks[b]
        deg[lo:hi] += rowptr[1:] - rowptr[:-1]
    return deg


def score_links_blocks(Z, H, t: float, min_logit: float, exclude=None, node_filter=None, table_dtype=torch.float32,
                       block_nodes=None):
    """``score_links`` for ANY N up to 8,388,480 -> (rowptr int64 [N+1], col int32 [nnz], logit f32 [nnz], prob f32 [nnz]): the
    symmetric CSR over all N nodes in GLOBAL ids, columns strictly ascending, each pair twice with the same bits.  Blocks as
    in ``score_mine_blocks``: diagonal blocks through dl_score_links_count_dtype / _fill_dtype on row slices, block pairs
    i < j through the _between entries, whose A side is a piece of the rows of block i and whose B side one of block j.  The
    windows run in row-major order, so the pieces of a row arrive in ascending column blocks and are copied to their place
    behind one another: no sort of the result.  For N <= 46,340 the result is bit for bit ``score_links``'s, for every block
    size.  Peak memory: the pieces and the result (2 x the result arrays), the workspace of ONE window, O(N) arrays and one
    int32 degree per row and piece (N x blocks); one host read per window."""
    W = _BlockWindows(Z, H, t, exclude, node_filter, table_dtype, block_nodes)
    deg = torch.zeros(W.N, dtype=torch.int64, device=W.dev)
    pieces = []
    for b, off, (rowptr, col, logit, prob) in _links_windows(W, min_logit, fill=True):
        lo, hi = W.blocks[b]
        d32 = (rowptr[1:] - rowptr[:-1]).to(torch.int32)
        deg[lo:hi] += d32
        if col.numel():
            pieces.append((b, off, d32, col, logit, prob))
    out_rowptr = torch.zeros(W.N + 1, dtype=torch.int64, device=W.dev)
    out_rowptr[1:] = torch.cumsum(deg, dim=0)
    nnz = int(out_rowptr[-1].item())
    out_col = _empty(nnz, torch.int32, W.dev)
    out_logit, out_prob = _empty(nnz, torch.float32, W.dev), _empty(nnz, torch.float32, W.dev)
    cursor = out_rowptr[:-1].clone()                                   # where the next piece of every row starts
    pieces.reverse()
    while pieces:                                                      # in arrival order; a piece is freed once it is placed
        b, off, d32, col, logit, prob = pieces.pop()
        lo, hi = W.blocks[b]
        d64 = d32.to(torch.int64)
        first = torch.cumsum(d64, dim=0) - d64                         # the piece's own exclusive prefix
        dest = torch.repeat_interleave(cursor[lo:hi] - first, d64) + torch.arange(col.numel(), device=W.dev)
        out_col[dest] = col + off
        out_logit[dest] = logit
        out_prob[dest] = prob
        cursor[lo:hi] += d64
    return out_rowptr, out_col, out_logit, out_prob
