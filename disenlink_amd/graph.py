"""Graph and pair-list containers handed to libdisenlink_hip.so.

The reference keeps the training adjacency as a dense ``[N,N]`` fp32 matrix
(``main_disentangled.py:137-142``).  Here it is a CSR of the binarised, symmetrised adjacency
plus a row-segment plan that cuts skewed rows into pieces of at most ``seg_len`` entries (one
wavefront per piece).  A plan may cover only a contiguous block of rows (one shard per GPU);
column ids stay global.

All tensors are int32 and live on the device of the input.  Building is plain torch index
plumbing, done once per adjacency / pair list — it is not on the per-epoch path.
"""
from __future__ import annotations

import os
import ctypes as C
import itertools
import weakref
from dataclasses import dataclass, field

import torch

from . import _lib

DEFAULT_SEG_LEN = int(os.environ.get("DL_SEG_LEN", "32"))        # adjacency rows (DL_SEG_LEN: experiments only)
# routing plan (no per-row reduction, hence no partials: shorter segments only add waves in flight — squirrel route
# phase 46.6 -> 42.9 us, real chameleon 33.4 -> 25.2, Penn94-sized unchanged); 0 = the adjacency plan's
DEFAULT_ROUTE_SEG_LEN = int(os.environ.get("DL_ROUTE_SEG_LEN", "0"))      # 0 = route_seg_len() decides (16, or 8 on small graphs)


def route_seg_len(n_entries: int) -> int:
    """Entries per wavefront of the routing plan (its kernel sums nothing across a row, so this is a pure grain choice;
    the per-entry results do not depend on it).  16 on graphs that fill the chip; 8 where 16 would leave fewer segments
    than the 4,096 wavefront slots of the 256 CUs (chameleon: routing phase 15.5 -> 13.6 us, Cora 14.3 -> 11.5)."""
    if DEFAULT_ROUTE_SEG_LEN:
        return DEFAULT_ROUTE_SEG_LEN
    return 16 if n_entries >= 16 * 4096 else 8
DEFAULT_INC_SEG_LEN = 64    # pair-incidence rows (backward of the scorer)
DEFAULT_RUN_LEN = 64        # pairs-by-first-endpoint rows (forward scorer)
DEFAULT_SLICES = 8          # XCDs of an MI355X
UNIT_SEGS = 4               # wavefronts per workgroup = segment positions per workgroup (DL_UNIT_SEGS)
L2_BYTES_PER_XCD = 4 << 20


CACHE_BYTES = 256 << 20     # Infinity Cache of an MI355X


def length_order(n_nodes: int, row_bytes: int, n_tables: int = 2) -> bool:
    """Whether a plan over these tables should place its units by LENGTH (longest first) inside a slice instead of
    in entry order.  A workgroup's four wavefronts end together (its LDS and its barrier), so four segments of 3, 60, 7
    and 31 entries leave most of the group idle; side by side by length they finish together, and longest-first is the
    better schedule for the tail.  The price is that consecutive workgroups no longer walk consecutive rows: where the
    row streams come from HBM that costs more than it gains (snap-patents-shaped, 3 GB: route / aggregate +11 %), where
    the gathered tables (Z and H: n_tables * n_nodes * row_bytes) fit the Infinity Cache it is free — real squirrel
    step 220 -> 208 us, chameleon 72 -> 62; squirrel-shaped graphs up to 170 MB of tables -5 %, 340 MB and up: even.
    Results do not depend on it (a unit's segments and its slot stay what they are).  DL_PLAN_SORT=0/1 forces it."""
    forced = os.environ.get("DL_PLAN_SORT")
    if forced is not None and forced != "":
        return forced != "0"
    return float(n_nodes) * row_bytes * n_tables <= CACHE_BYTES


def auto_slices(n_nodes: int, row_bytes: int, entries_per_row: float = 1e9, n_tables: int = 2) -> int:
    """Number of column slices of an XCD-aware plan (a multiple of 8: slice q belongs to XCD stream q % 8,
    the slices of a stream follow each other in time).  Aim: one slice of the gathered tables (Z and H rows
    of n_nodes / n_slices nodes) near an XCD's 4 MiB L2, while a (row, slice) group keeps >= ~4 entries so
    that the per-segment staging of the row stays amortised.  Measured (tools/): squirrel
    483 -> 196 us with 8 slices; a 41.6k-node table (170 MB) 600 -> 357 us with 32."""
    forced = os.environ.get("DL_FORCE_SLICES")              # experiments only
    if forced:
        return int(forced)
    table = float(n_nodes) * row_bytes * n_tables
    # small tables: the FEWEST slices that put a slice inside an L2 (round 6, wave-per-entry scorer: chameleon — 9.3 MB —
    # 34.0 / 32.4 / 34.3 / 40.9 us at 2 / 4 / 8 / 16 slices, profiles/r7q_fwd_slices.txt; squirrel — 21.3 MB — needs the 8)
    for few in (1, 2, 4):
        if table / few <= 0.7 * L2_BYTES_PER_XCD:
            return few if entries_per_row >= 4 * few else 1
    if entries_per_row < 2 * DEFAULT_SLICES:                     # rows too short to be cut 8 ways
        return 1
    t_cap = 1
    while 2 * t_cap * DEFAULT_SLICES * 4 <= entries_per_row:       # keep >= 4 entries per (row, slice)
        t_cap *= 2
    t = 1
    while t < t_cap and table / (DEFAULT_SLICES * t) > 1.5 * L2_BYTES_PER_XCD:
        t *= 2
    if table / (DEFAULT_SLICES * t) > 2 * L2_BYTES_PER_XCD:       # a slice that does not fit an L2 buys nothing and
        return 1                                                  # costs the per-(row, slice) staging (Penn94-sized,
                                                                  # bf16 tables: scorer 7.3 ms unsliced, 11.7 ms at 32)
    return DEFAULT_SLICES * t


def auto_inc_slices(n_nodes: int, row_bytes: int, entries_per_row: float, n_tables: int = 2) -> int:
    """Column slices of the INCIDENCE plan (one-pass training scorer, scorer backward).  Every (row, slice) group there
    is a unit with a partial slot — 2 K d 4 bytes written, then read by the combine launch, through memory — so slices
    cost per group what they buy per gathered row.  Measured (profiles/r7a_inc_slices_sweep.txt, r7b_train_scorer_ab.txt,
    interleaved same-process runs): squirrel (21 MB of Z + H, 388 entries per row) 379 us at 4, 363 at 8, 454 at 16;
    chameleon (9 MB, 148) 73 / 70 / 89 at 2 / 4 / 8; Penn94-sized K = 8 fp32 (170 MB, 331) 6.79 ms at 8, 5.78 at 16, 5.95
    at 32; K = 16 bf16 (340 MB) 15.4 ms unsliced, 14.5 at 16, 16.3 at 32.  The rule that picks the best of each: the
    fewest slices that put a slice of the tables inside an XCD's L2 (0.7 x 4 MiB), but never groups shorter than ~20
    entries; nothing where even that leaves slices 8x beyond the L2 (the hit rate it buys is then below ~1/8)."""
    forced = os.environ.get("DL_FORCE_INC_SLICES")                 # experiments only
    if forced:
        return int(forced)
    table = float(n_nodes) * row_bytes * n_tables
    s_len = 1
    while 2 * s_len * 20 <= entries_per_row:                        # groups of >= ~20 entries
        s_len *= 2
    s_fit = 1
    while table / s_fit > 0.7 * L2_BYTES_PER_XCD and s_fit < 256:
        s_fit *= 2
    s = max(1, min(s_fit, s_len))
    return s if table / s <= 8 * L2_BYTES_PER_XCD else 1


def slice_bounds(col: torch.Tensor, n_slices: int) -> torch.Tensor:
    """The n_slices - 1 boundaries of column_slices (quantiles of `col`): slice q = [bounds[q-1], bounds[q])."""
    E = int(col.numel())
    sorted_col = torch.sort(col).values
    cut = (torch.arange(1, n_slices, device=col.device, dtype=torch.int64) * E) // n_slices
    return sorted_col[cut]


def column_slices(col: torch.Tensor, n_slices: int) -> torch.Tensor:
    """Slice id of every entry: the column (node id) space is cut into n_slices contiguous ranges holding EQUAL
    NUMBERS OF ENTRIES (boundaries at the quantiles of `col`), not equal numbers of nodes — each XCD stream then gets
    the same amount of work whatever the degree distribution over node ids is (real squirrel: the heaviest of 8
    equal-width slices held 31 % more pairs than the average; scorer 226 -> see DESIGN.md).  Entries with the same
    column always share a slice.  dl_host_plan_build (dl_host.hip) computes the same boundaries."""
    if int(col.numel()) == 0 or n_slices <= 1:
        return torch.zeros_like(col)
    return torch.bucketize(col, slice_bounds(col, n_slices), right=True)


def _i32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.int32).contiguous()


# Integer handles of live Graph / PairList objects (the registered operators of torch_ops.py take handles, not Python
# objects).  Held WEAKLY and assigned at construction: reading a handle is then a plain attribute access — traceable by
# torch.compile — and a caller that builds a new pair list per epoch does not accumulate GPU plans in a registry.
_HANDLES: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()
_next_handle = itertools.count(1)


def _assign_handle(obj) -> None:
    obj._dl_handle = next(_next_handle)
    _HANDLES[obj._dl_handle] = obj


def by_handle(handle: int, kind):
    obj = _HANDLES.get(int(handle))
    return obj if isinstance(obj, kind) else None


class _PlanOwner:
    """What Graph and PairList share as owners of a plan the kernels walk (``c_plan()``): the scratch that plan needs."""

    def workspace_bytes(self, K: int, d: int) -> int:
        """Bytes of workspace the kernels over this object's plan need at (K, d): dl_workspace_bytes, asked once per
        (K, d) and remembered here — the plan of an object never changes."""
        need = self._ws_need.get((K, d))
        if need is None:
            need = self._ws_need[(K, d)] = int(_lib.load().dl_workspace_bytes(self.c_plan(), K, d))
        return need


@dataclass
class CsrPlan:
    """Rows [row_offset, row_offset + n_rows) of a CSR over n_total nodes + its segment plan.

    ``n_slices > 1`` makes the plan XCD-aware: the column space is cut into ``n_slices`` node ranges of equal entry
    count, no segment spans two ranges (needs ``col`` ascending inside each row) and segments are stored slice-major
    (``slice_seg0``).

    The ``seg_*`` arrays are indexed by POSITION: a workgroup of ``UNIT_SEGS`` wavefronts serves ``UNIT_SEGS``
    consecutive positions, and the segments of a row are placed in aligned runs (units) of at most ``UNIT_SEGS`` that
    the workgroup sums on chip; ``seg_row == -1`` marks a padding position, ``seg_slot`` is the partial slot of the
    segment's unit (-1: the row is a single unit and needs no partials).  See include/disenlink_hip.h."""
    n_rows: int
    row_offset: int
    n_total: int
    rowptr: torch.Tensor
    col: torch.Tensor
    seg_len: int
    seg_row: torch.Tensor
    seg_beg: torch.Tensor
    seg_end: torch.Tensor
    seg_slot: torch.Tensor
    n_slices: int
    slice_max_seg: int
    slice_seg0: torch.Tensor
    multi_row: torch.Tensor
    multi_slot0: torch.Tensor
    n_slots: int
    slot_multi: torch.Tensor | None = None      # [n_slots] index (into multi_row) of the row a partial slot belongs to
    unit_count: torch.Tensor | None = None      # [n_multi] zeroed int32, owned by the plan: the in-launch row sums count
                                                # the units of a row here and leave it all zero again (disenlink_hip.h)

    def __post_init__(self):
        dev = self.multi_slot0.device
        if self.slot_multi is None:
            n = self.multi_slot0[1:] - self.multi_slot0[:-1]
            self.slot_multi = torch.repeat_interleave(torch.arange(n.numel(), device=dev, dtype=torch.int32), n.long())
        if self.unit_count is None:
            self.unit_count = torch.zeros(int(self.multi_row.numel()), dtype=torch.int32, device=dev)

    @property
    def n_entries(self) -> int:
        return int(self.col.numel())

    @property
    def n_seg(self) -> int:
        return int(self.seg_row.numel())

    @property
    def device(self) -> torch.device:
        return self.rowptr.device

    @staticmethod
    def build(rowptr: torch.Tensor, col: torch.Tensor, n_total: int, row_offset: int = 0,
              seg_len: int = DEFAULT_SEG_LEN, n_slices: int = 1, keep: torch.Tensor | None = None,
              unit_segs: int = UNIT_SEGS, by_length: bool = False, bounds: torch.Tensor | None = None) -> "CsrPlan":
        """``keep`` (bool per entry, optional): segments cover only the kept entries, which must form one
        contiguous run inside every row (e.g. the upper triangle ``col >= row`` of a sorted row).
        ``unit_segs = 1``: every segment is its own unit — for plans whose kernels reduce nothing across segments
        (routing, the forward scorer): positions then simply follow the entry order.
        ``bounds`` (optional, n_slices - 1 ascending node ids): the column slices' boundaries given from outside instead of
        the quantiles of THIS plan's columns — a row shard passes the whole list's boundaries, so that its rows are cut
        into exactly the units the unsharded plan cuts them into (the units of a row are summed in slot order: same bits)."""
        if unit_segs not in (1, UNIT_SEGS):
            raise ValueError(f"unit_segs must be 1 or {UNIT_SEGS}")
        if seg_len < 1 or n_slices < 1:
            raise ValueError("seg_len and n_slices must be >= 1")
        rowptr = rowptr.to(torch.int64)
        col = col.to(torch.int64)
        n_rows = int(rowptr.numel()) - 1
        if row_offset < 0 or row_offset + n_rows > n_total:
            raise ValueError("row block outside [0, n_total)")
        dev = rowptr.device
        E_all = int(col.numel())
        deg_all = rowptr[1:] - rowptr[:-1]
        ar = lambda n: torch.arange(n, device=dev)
        # groups = maximal entry ranges with equal (row, column slice); entries are sorted by (row, col)
        row_all = torch.repeat_interleave(ar(n_rows), deg_all)
        if keep is None:
            orig, row_of, kcol = ar(E_all), row_all, col
        else:
            orig = torch.nonzero(keep.to(dev)).reshape(-1)          # original entry index of every kept entry
            row_of, kcol = row_all[orig], col[orig]
        E = int(orig.numel())
        deg = torch.bincount(row_of, minlength=n_rows) if E else torch.zeros(n_rows, dtype=torch.int64, device=dev)
        if n_slices > 1 and bounds is not None:
            if int(bounds.numel()) != n_slices - 1:
                raise ValueError("bounds must hold n_slices - 1 boundaries")
            sl_of = torch.bucketize(kcol, bounds.to(kcol.device), right=True)
        else:
            sl_of = column_slices(kcol, n_slices) if n_slices > 1 else 0
        gid = row_of * n_slices + sl_of
        if E and n_slices > 1 and bool((gid[1:] < gid[:-1]).any()):
            raise ValueError("sliced plans need col ascending inside every row")
        new = torch.ones(E, dtype=torch.bool, device=dev)
        if E:
            new[1:] = gid[1:] != gid[:-1]
            if keep is not None and bool(((orig[1:] != orig[:-1] + 1) & ~new[1:]).any()):
                raise ValueError("kept entries must be contiguous inside every row")
        gpos = torch.nonzero(new).reshape(-1)                       # positions in the kept list
        gpos_end = torch.cat([gpos[1:], torch.tensor([E], device=dev)]) if E else gpos
        gstart = orig[gpos] if E else gpos                          # ... and as original entry indices
        gend = (orig[gpos_end - 1] + 1) if E else gpos
        g_id = gid[gpos] if E else gpos
        nch = (gend - gstart + seg_len - 1) // seg_len
        ch0 = torch.cumsum(nch, 0) - nch
        seg_g = torch.repeat_interleave(ar(gstart.numel()), nch)
        seg_beg = gstart[seg_g] + (ar(seg_g.numel()) - ch0[seg_g]) * seg_len
        seg_end = torch.minimum(seg_beg + seg_len, gend[seg_g])
        seg_row = torch.div(g_id[seg_g], n_slices, rounding_mode="floor")
        seg_slice = g_id[seg_g] - seg_row * n_slices
        # empty rows still own one (empty) segment: their outputs must be written
        empty = torch.nonzero(deg == 0).reshape(-1)
        seg_row = torch.cat([seg_row, empty])
        seg_beg = torch.cat([seg_beg, rowptr[empty]])
        seg_end = torch.cat([seg_end, rowptr[empty]])
        seg_slice = torch.cat([seg_slice, torch.zeros_like(empty)])
        # entry order: (row, first entry); a (row, slice) group is a run of this order
        order = torch.argsort(seg_row * (E_all + 1) + seg_beg, stable=True)
        seg_row, seg_beg, seg_end, seg_slice = seg_row[order], seg_beg[order], seg_end[order], seg_slice[order]
        S = int(seg_row.numel())
        # UNITS: up to UNIT_SEGS consecutive segments of one (row, slice) group, counted from the group's first
        # segment — so the chunking of a row depends on that row alone (a shard cuts its rows exactly like the whole
        # graph does: results stay bitwise independent of the sharding).  A workgroup (UNIT_SEGS wavefronts) serves
        # UNIT_SEGS consecutive POSITIONS of a slice stream and sums each unit on chip; only rows with more than one
        # unit go through partial slots (one per UNIT, not per segment).
        grp_key = seg_row * n_slices + seg_slice
        gnew = torch.ones(S, dtype=torch.bool, device=dev)
        gnew[1:] = grp_key[1:] != grp_key[:-1]
        gstart_pos = torch.nonzero(gnew).reshape(-1)
        g_of = torch.cumsum(gnew, 0) - 1
        idx_in_grp = ar(S) - gstart_pos[g_of]
        unew = gnew | (idx_in_grp % unit_segs == 0)
        u_of = torch.cumsum(unew, 0) - 1                          # unit of every segment, units in entry order
        ufirst = torch.nonzero(unew).reshape(-1)
        n_units = int(ufirst.numel())
        u_size = torch.bincount(u_of, minlength=n_units)
        u_pad = torch.where(u_size == 3, torch.full_like(u_size, 4), u_size)   # 1, 2, 4: aligned when placed largest first
        u_row, u_slice = seg_row[ufirst], seg_slice[ufirst]
        # partial slots: one per unit of a multi-unit row, consecutive per row in entry order
        nunit_row = torch.bincount(u_row, minlength=n_rows)
        multi_row = torch.nonzero(nunit_row > 1).reshape(-1)
        multi_slot0 = torch.zeros(multi_row.numel() + 1, dtype=torch.int64, device=dev)
        multi_slot0[1:] = torch.cumsum(nunit_row[multi_row], dim=0)
        row_slot0 = torch.full((n_rows,), -1, dtype=torch.int64, device=dev)
        row_slot0[multi_row] = multi_slot0[:-1]
        row_unit0 = torch.cumsum(nunit_row, 0) - nunit_row
        u_idx_in_row = ar(n_units) - row_unit0[u_row]
        u_slot = torch.where(row_slot0[u_row] >= 0, row_slot0[u_row] + u_idx_in_row, row_slot0[u_row])
        # storage: one STREAM of positions per XCD.  Column slice q belongs to stream q % 8 and the slices of a stream
        # follow each other in time (q // 8), so an XCD works on one slice at a time.  Inside a slice the units are placed
        # by padded size, largest first (stable: entry order among equals — or, with by_length, most entries first: see
        # length_order), so no unit straddles a group of UNIT_SEGS positions; every slice region is padded to a multiple
        # of UNIT_SEGS.  Pad positions have seg_row = -1.
        n_streams = min(n_slices, DEFAULT_SLICES)
        u_stream = u_slice % n_streams
        key = (u_stream * (n_slices + 1) + u_slice) * 8 + (UNIT_SEGS - u_pad)
        if by_length and n_units:                                  # ... and by entries inside a size class, longest first
            u_entries = torch.zeros(n_units, dtype=torch.int64, device=dev).index_add_(0, u_of, seg_end - seg_beg)
            span = int(seg_len) * UNIT_SEGS
            key = key * (span + 1) + (span - u_entries)
        uperm = torch.argsort(key, stable=True)
        sl_size = torch.zeros(n_slices, dtype=torch.int64, device=dev).index_add_(0, u_slice, u_pad)
        sl_size = (sl_size + UNIT_SEGS - 1) // UNIT_SEGS * UNIT_SEGS
        sl_order = torch.argsort((ar(n_slices) % n_streams) * (n_slices + 1) + ar(n_slices), stable=True)   # (stream, slice)
        sl_base = torch.zeros(n_slices, dtype=torch.int64, device=dev)
        sl_base[sl_order] = torch.cumsum(sl_size[sl_order], 0) - sl_size[sl_order]
        pad_sorted = u_pad[uperm]
        run = torch.cumsum(pad_sorted, 0) - pad_sorted             # exclusive cumsum over all units in storage order ...
        sl_sorted = u_slice[uperm]
        first_of_slice = torch.ones(n_units, dtype=torch.bool, device=dev)
        first_of_slice[1:] = sl_sorted[1:] != sl_sorted[:-1]
        run0 = run[torch.nonzero(first_of_slice).reshape(-1)]      # ... minus its value at the slice's first unit
        slice_rank = torch.cumsum(first_of_slice, 0) - 1
        u_pos = torch.empty(n_units, dtype=torch.int64, device=dev)
        u_pos[uperm] = sl_base[sl_sorted] + run - run0[slice_rank]
        n_pos = int(sl_size.sum())
        pos = u_pos[u_of] + (ar(S) - ufirst[u_of])
        p_row = torch.full((n_pos,), -1, dtype=torch.int64, device=dev)
        p_beg = torch.zeros(n_pos, dtype=torch.int64, device=dev)
        p_end = torch.zeros(n_pos, dtype=torch.int64, device=dev)
        p_slot = torch.full((n_pos,), -1, dtype=torch.int64, device=dev)
        p_row[pos], p_beg[pos], p_end[pos], p_slot[pos] = seg_row, seg_beg, seg_end, u_slot[u_of]
        stream_size = torch.zeros(n_streams, dtype=torch.int64, device=dev).index_add_(0, ar(n_slices) % n_streams, sl_size)
        slice_seg0 = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
        slice_seg0[1:] = torch.cumsum(stream_size, 0)
        return CsrPlan(n_rows, row_offset, n_total, _i32(rowptr), _i32(col), seg_len, _i32(p_row),
                       _i32(p_beg), _i32(p_end), _i32(p_slot), n_streams,
                       int(stream_size.max()), _i32(slice_seg0),
                       _i32(multi_row), _i32(multi_slot0), int(multi_slot0[-1]))

    def to(self, device) -> "CsrPlan":
        mv = lambda t: t.to(device)
        return CsrPlan(self.n_rows, self.row_offset, self.n_total, mv(self.rowptr), mv(self.col), self.seg_len,
                       mv(self.seg_row), mv(self.seg_beg), mv(self.seg_end), mv(self.seg_slot), self.n_slices,
                       self.slice_max_seg, mv(self.slice_seg0), mv(self.multi_row), mv(self.multi_slot0), self.n_slots)

    def c_value(self) -> _lib.DlCsrPlan:
        return _lib.DlCsrPlan(
            self.n_rows, self.row_offset, self.n_total, self.n_entries, self.rowptr.data_ptr(), self.col.data_ptr(),
            self.seg_len, self.n_seg, self.seg_row.data_ptr(), self.seg_beg.data_ptr(), self.seg_end.data_ptr(),
            self.seg_slot.data_ptr(), self.n_slices, self.slice_max_seg, self.slice_seg0.data_ptr(),
            int(self.multi_row.numel()), self.n_slots, self.multi_row.data_ptr(), self.multi_slot0.data_ptr(),
            self.slot_multi.data_ptr(), self.unit_count.data_ptr())


@dataclass
class Graph(_PlanOwner):
    plan: CsrPlan
    rev: torch.Tensor | None = None      # reverse-edge permutation (unsharded builds only)
    route: CsrPlan | None = None         # plan walked by the routing kernel: XCD-sliced, and (unsharded builds)
    route_mirror: bool = False           # covering col >= row only — routing is symmetric, so each undirected
                                         # edge is computed once and written to both entries through rev
    route_hub: HubPlan | None = None     # the entries with col >= row as hub blocks (route_hub_plan; None: walk `route`)
    _struct: _lib.DlGraph | None = field(default=None, repr=False)
    _ws_need: dict = field(default_factory=dict, repr=False)          # (K, d) -> bytes: workspace_bytes

    def __post_init__(self):
        _assign_handle(self)

    # convenience views
    n_nodes = property(lambda self: self.plan.n_total)
    n_rows = property(lambda self: self.plan.n_rows)
    row_offset = property(lambda self: self.plan.row_offset)
    n_edges = property(lambda self: self.plan.n_entries)
    n_seg = property(lambda self: self.plan.n_seg)
    rowptr = property(lambda self: self.plan.rowptr)
    col = property(lambda self: self.plan.col)
    device = property(lambda self: self.plan.device)

    # ------------------------------------------------------------------ builders
    @staticmethod
    def from_edge_rows(src: torch.Tensor, dst: torch.Tensor, n_nodes: int, symmetrise: bool = True,
                       seg_len: int = DEFAULT_SEG_LEN, row_range: tuple[int, int] | None = None,
                       row_bytes: int = 2048, route_hub: bool | None = None) -> "Graph":
        """Directed edge rows (duplicates allowed) -> CSR of the binarised adjacency.

        ``symmetrise=True`` reproduces ``adj_sym = (adj + adj.T) != 0`` (main_disentangled.py:141-142).
        ``row_range=(lo, hi)`` keeps only rows lo..hi-1 (one shard); column ids stay global.
        ``route_hub``: whether the routing kernel gets a hub plan (route_hub_plan) — None = where the graph's first block
        of 16 owner rows shares gathered rows (auto_hub_rows; a uniform sparse graph or a row shard gets none and nothing
        changes), True = always (unsharded builds only), False = never.  The results do not depend on it.
        """
        if n_nodes < 0 or n_nodes >= 2 ** 31:
            raise ValueError(f"n_nodes={n_nodes} out of int32 range")
        src = src.reshape(-1).to(torch.int64)
        dst = dst.reshape(-1).to(torch.int64)
        if src.numel() != dst.numel():
            raise ValueError("src and dst differ in length")
        if src.numel() and (int(src.min()) < 0 or int(dst.min()) < 0 or
                            int(src.max()) >= n_nodes or int(dst.max()) >= n_nodes):
            raise ValueError("edge endpoint outside [0, n_nodes)")
        if symmetrise:
            src, dst = torch.cat([src, dst]), torch.cat([dst, src])
        key = torch.unique(src * n_nodes + dst)            # sorted, duplicates collapsed
        if key.numel() >= 2 ** 31:
            raise ValueError("more than 2^31-1 edges")
        r = torch.div(key, n_nodes, rounding_mode="floor")
        c = key - r * n_nodes
        tkey = c * n_nodes + r
        rev = torch.searchsorted(key, tkey)
        if key.numel():
            ok = (rev < key.numel()) & (key[rev.clamp(max=key.numel() - 1)] == tkey)
            if not bool(ok.all()):
                raise ValueError("adjacency is not symmetric (reverse edge missing); pass symmetrise=True")
        lo, hi = (0, n_nodes) if row_range is None else row_range
        if not (0 <= lo <= hi <= n_nodes):
            raise ValueError("row_range outside [0, n_nodes]")
        counts = torch.bincount(r, minlength=n_nodes) if key.numel() else torch.zeros(n_nodes, dtype=torch.int64,
                                                                                      device=key.device)
        full_ptr = torch.zeros(n_nodes + 1, dtype=torch.int64, device=key.device)
        full_ptr[1:] = torch.cumsum(counts, dim=0)
        e0, e1 = int(full_ptr[lo]), int(full_ptr[hi])
        by_len = length_order(n_nodes, row_bytes)
        plan = CsrPlan.build(full_ptr[lo:hi + 1] - e0, c[e0:e1], n_nodes, row_offset=lo, seg_len=seg_len, by_length=by_len)
        mirror = row_range is None
        lc, lr = c[e0:e1], r[e0:e1] - lo
        # XCD slicing of the routing plan was measured and rejected: hub rows already give the Z gathers a high
        # L2 hit rate, and the extra segments cost more than they save (squirrel 50 -> 72 us; 41.6k-node shard
        # 115 -> 107 us; re-measured in round 6 on the mirrored 22 us kernel: 31.5 / 31.1 / 32.5 / 35.0 us by events at
        # 1 / 2 / 4 / 8 slices).  `row_bytes` is kept for callers that pass the model shape.
        route = CsrPlan.build(full_ptr[lo:hi + 1] - e0, lc, n_nodes, row_offset=lo,
                              seg_len=min(seg_len, route_seg_len((e1 - e0 + 1) // 2 if mirror else e1 - e0)), n_slices=1,
                              keep=(lc >= lr + lo) if mirror else None, unit_segs=1, by_length=by_len)
        route.rowptr, route.col = plan.rowptr, plan.col        # the SAME arrays: only the segments differ
        if route_hub and not mirror:
            raise ValueError("a routing hub plan needs the unsharded graph (row_range=None)")
        hub = route_hub_plan(lr, lc, rev, n_nodes, force=bool(route_hub)) if mirror and route_hub is not False else None
        return Graph(plan, _i32(rev) if mirror else None, route, mirror, hub)

    @staticmethod
    def from_dense(adj: torch.Tensor, seg_len: int = DEFAULT_SEG_LEN, row_bytes: int = 2048,
                   route_hub: bool | None = None) -> "Graph":
        """Dense ``adj_sym`` as the reference passes it to ``model(x, adj_sym)`` (main_disentangled.py:194).
        ``route_hub``: as in from_edge_rows."""
        if adj.dim() != 2 or adj.shape[0] != adj.shape[1]:
            raise ValueError("adj must be square")
        # The reference multiplies by adj (model.py:62: p * adj, compared with the factor numbers): its layer is only
        # meaningful for entries that are 0 or 1.  Anything else would be an edge here and garbage there: refuse it.
        if adj.layout != torch.strided:                            # sparse COO / CSR: the stored entries (an extension)
            coo = adj.to_sparse_coo().coalesce()
            val, idx = coo.values(), coo.indices()
            if bool(((val != 0) & (val != 1)).any()):
                raise ValueError("adj must hold 0 / 1 entries (the reference's layer multiplies by it, model.py:62)")
            keep = val != 0
            return Graph.from_edge_rows(idx[0][keep], idx[1][keep], adj.shape[0], symmetrise=False, seg_len=seg_len,
                                        row_bytes=row_bytes, route_hub=route_hub)
        nz = torch.nonzero(adj)
        if nz.shape[0] and bool((adj[nz[:, 0], nz[:, 1]] != 1).any()):
            raise ValueError("adj must hold 0 / 1 entries (the reference's layer multiplies by it, model.py:62)")
        return Graph.from_edge_rows(nz[:, 0], nz[:, 1], adj.shape[0], symmetrise=False, seg_len=seg_len,
                                    row_bytes=row_bytes, route_hub=route_hub)

    def to(self, device) -> "Graph":
        plan = self.plan.to(device)
        route = None if self.route is None else self.route.to(device)
        if route is not None:
            route.rowptr, route.col = plan.rowptr, plan.col
        return Graph(plan, None if self.rev is None else self.rev.to(device), route, self.route_mirror,
                     None if self.route_hub is None else self.route_hub.to(device))

    def c_struct(self):
        if self._struct is None:
            rp = self.route.c_value() if self.route is not None else _lib.DlCsrPlan()
            self._struct = _lib.DlGraph(self.plan.c_value(), rp, self.rev.data_ptr() if self.rev is not None else None,
                                        1 if self.route_mirror else 0)
            h = self.route_hub
            if h is not None and h.n_items > 0:
                # the kernel walks the hub plan INSTEAD of the routing plan: it must hold every entry with col >= row
                row = torch.repeat_interleave(torch.arange(self.n_rows, device=self.device), (self.rowptr[1:] - self.rowptr[:-1]).long())
                n_upper = int((self.col.long() >= row).sum())
                if not self.route_mirror or h.rest is not None or h.step_q2 is None or h.n_entries != n_upper:
                    raise ValueError(f"routing hub plan: needs a mirrored graph, no residual plan and each of the {n_upper} "
                                     f"entries with col >= row as a slot (it holds {h.n_entries})")
                self._struct.route_hub = C.pointer(h.c_value())
        return C.byref(self._struct)

    def c_plan(self):
        self.c_struct()
        return C.byref(self._struct.csr)


def mirror_partners(pu: torch.Tensor, pv: torch.Tensor, n_nodes: int) -> torch.Tensor:
    """-> second int64[P]: ``second[q] = q'`` where pair q = (u, v), u < v, is matched with a listed reverse q' = (v, u),
    else -1.  The matching is one to one: the j-th copy of an ordered pair is matched with the j-th copy of its reverse
    (in list order), surplus copies on either side stay unmatched, and so do self pairs.  The matched entry stays in the
    row of min(u, v): which of the two segments would end up with the shorter tail depends on the slicing that follows,
    and the tail steps it could save are the ones the scorer no longer gathers for anyway."""
    P, dev = pu.numel(), pu.device
    second = torch.full((P,), -1, dtype=torch.int64, device=dev)
    if P == 0:
        return second
    lo_, hi_ = torch.minimum(pu, pv), torch.maximum(pu, pv)
    # occurrence number of every pair among the copies of the same ORDERED pair, in list order
    okey = pu * n_nodes + pv
    order = torch.argsort(okey, stable=True)
    sk = okey[order]
    first = torch.ones(P, dtype=torch.bool, device=dev)
    first[1:] = sk[1:] != sk[:-1]
    pos = torch.arange(P, device=dev)
    occ = torch.empty(P, dtype=torch.int64, device=dev)
    occ[order] = pos - torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), 0).values
    # lexicographic order by (unordered pair, occurrence, direction): partners become neighbours, u < v first
    perm = torch.argsort((pu > pv).to(torch.int64), stable=True)
    perm = perm[torch.argsort(occ[perm], stable=True)]
    perm = perm[torch.argsort((lo_ * n_nodes + hi_)[perm], stable=True)]
    a, b = perm[:-1], perm[1:]
    match = (lo_[a] == lo_[b]) & (hi_[a] == hi_[b]) & (occ[a] == occ[b]) & (pu[a] < pv[a]) & (pu[b] > pv[b])
    second[a[match]] = b[match]
    return second


# ---------------------------------------------------------------------------------------------- hub plan (forward scorer)
HUB_W = 16                  # rows of a hub block (DL_HUB_W: 16 [Z | H] rows of K = 8, d = 64, fp32 are 64 KB of LDS)
# Automatic choice of the hub rows: a list whose FIRST block of HUB_W ranked rows scores at least HUB_MIN_SHARE entries per
# gathered row pair gets a hub plan over EVERY row with entries; any other list gets none (1.0 = nothing shared: uniform
# sparse lists stay exactly as they were).  Taking blocks only while they reach the threshold was measured and lost: on
# squirrel_real the scorer alone takes (us per call, median of 12 interleaved rounds, profiles/r10_fwd_hub.txt) 146.3
# without hub rows, 148.1 / 139.1 / 136.7 / 137.2 with the top 512 / 1,024 / 1,376 (= every block at >= 1.25) / 2,048
# rows and 132.9 with all 5,144 — the residual launch behind the hub launch, with its own tail, costs more than the
# blocks near 1.0 do, and a block at 1.0 is still a step of four gathers like the wave-per-entry kernel's.
HUB_MIN_SHARE = 1.25
# A (block, slice) whose steps gather more partner rows than this is cut into several work items, each staging the
# block's rows again: the longest (block, slice) of squirrel_real has ~1,300 steps, five times what a workgroup gets on
# average, and uncut it would be the tail of the launch.  256 is what every figure above was measured with.  The sweep on
# the benchmark's own plan (profiles/r12_fwd_hub_pipeline.txt, section 3; us per call): 128 / 256 / 384 / 512 / 768 / 1,024
# = 129.3 / 118.7 / 116.4 / 116.3 / 117.7 / 116.1 — 512 and 1,024 pass the keep rule against 256 and tie; 512 is the shorter.
HUB_ITEM_ROWS = 512
# Slot -> gathered partner row of a step, list by list (dl_hub.h: SHAPE_*): the three lists [A | B | C] of HubPlan.build and the
# five [A | A211 | B | B31 | C] of HubPlan.build_mixed.  A shape gathers (its last slot's row + 1) rows.
HUB_SHAPES = ((0, 1, 2, 3), (0, 0, 1, 1), (0, 0, 0, 0))
HUB_MIXED_SHAPES = ((0, 1, 2, 3), (0, 0, 1, 2), (0, 0, 1, 1), (0, 0, 0, 1), (0, 0, 0, 0))
# The two parts of the mixed plan, for A/B runs (tools/fwd_hub_ab.py; both on is what ships): the heavier endpoint of a pair is
# its hub row (hub_owner); a group's remainder stays one piece (HubPlan.build_mixed(mixed=True)).
HUB_MIXED_OWNER = True
HUB_MIXED_SHAPES_ON = True
# Gathered partner rows per work item of the mixed plan.  A step of the mixed plan gathers fewer rows, so at HUB_ITEM_ROWS = 512
# its longest item is 407 steps on squirrel_real (324 on the three lists) and 434 on chameleon_real (356) — and the longest
# chain of steps is the launch's tail.  The scorer alone, us per call at 192 / 256 / 320 / 384 / 448 / 512 rows
# (profiles/r17_fwd_hub_mixed.txt): squirrel_real 99.1 / 98.0 / 96.6 / 96.4 / 96.4 / 96.7 (three lists 110.1 in that run),
# chameleon_real 32.5 / 29.9 / 32.8 / 36.8 / 41.4 / 46.7 (three lists 41.3: at 512 the mixed plan LOSES there).  320 ties the
# best on squirrel_real and keeps most of chameleon_real's gain.  (None = HUB_ITEM_ROWS)
HUB_MIXED_ITEM_ROWS = 320


def hub_gathers(c: torch.Tensor) -> torch.Tensor:
    """Partner rows gathered for c slots on one partner row: c // 4 steps of shape C, a remainder of 2 or 3 a half of a
    shape B step, a remainder of 1 or 3 a slot of a shape A step."""
    return c // 4 + torch.tensor([0, 1, 1, 2], device=c.device)[c % 4]


def hub_owner(row: torch.Tensor, col: torch.Tensor, n_nodes: int):
    """(hub row, partner row) of every forward entry under the owner rule of the mixed plan: the endpoint with more
    forward entries, counted over both endpoints of all entries; ties go to the smaller id.  The score is symmetric bit
    for bit (fold_mirrors relies on it), so which endpoint is staged in LDS and which is gathered changes no result —
    but the heavy rows then share more partner rows, as in route_hub_plan."""
    deg = torch.bincount(torch.cat([row, col]), minlength=n_nodes)
    swap = (deg[col] > deg[row]) | ((deg[col] == deg[row]) & (col < row))
    return torch.where(swap, col, row), torch.where(swap, row, col)


def hub_rank(row: torch.Tensor, n_nodes: int):
    """Rows ranked by entry count, most first, ties by row index -> (rank of every row, rows with entries)."""
    cnt = torch.bincount(row, minlength=n_nodes)
    order = torch.argsort(-cnt, stable=True)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(n_nodes, device=row.device)
    return rank, order, int((cnt > 0).sum())


def hub_block_counts(row: torch.Tensor, col: torch.Tensor, n_nodes: int):
    """(entries, gathered row pairs) of every block of HUB_W consecutive ranked rows under the packing of
    HubPlan.build — what a (block, partner row) combination gathers does not depend on slices or work items."""
    rank, _, n_live = hub_rank(row, n_nodes)
    nb = (n_live + HUB_W - 1) // HUB_W
    blk = torch.div(rank[row], HUB_W, rounding_mode="floor")
    key, c = torch.unique(blk * n_nodes + col, return_counts=True)
    gathers = torch.zeros(nb, dtype=torch.int64, device=row.device).index_add_(0, torch.div(key, n_nodes, rounding_mode="floor"),
                                                                             hub_gathers(c))
    return torch.bincount(blk, minlength=nb), gathers


def auto_hub_rows(row: torch.Tensor, col: torch.Tensor, n_nodes: int, min_share: float | None = None) -> int:
    """Hub rows of a list: every row with entries if the first block shares at least min_share entries per gathered row
    pair, else none."""
    if row.numel() == 0:
        return 0
    entries, gathers = hub_block_counts(row, col, n_nodes)
    if float(entries[0]) < (HUB_MIN_SHARE if min_share is None else min_share) * float(gathers[0]):
        return 0
    return int((torch.bincount(row, minlength=n_nodes) > 0).sum())


@dataclass
class HubPlan:
    """The forward entries of the T rows with the most entries as blocks of HUB_W rows, work items and steps of four
    slots (dl_pair_hub, include/disenlink_hip.h), and the residual plan over every other row."""
    n_rows: int                     # T
    n_blocks: int
    block_row: torch.Tensor         # [n_blocks * HUB_W]
    n_items: int
    n_slices: int                   # slice streams
    slice_max_item: int
    slice_item0: torch.Tensor       # [n_slices + 1]
    item_block: torch.Tensor        # [n_items]
    item_slice: torch.Tensor        # [n_items] column slice (not passed to the library)
    item_step: torch.Tensor         # [n_items, 4]
    step_v: torch.Tensor            # [n_steps, 4]
    step_u: torch.Tensor
    step_q: torch.Tensor
    step_q2: torch.Tensor | None
    n_entries: int
    rest: CsrPlan | None
    rest_pair: torch.Tensor | None
    rest_pair2: torch.Tensor | None
    _struct: _lib.DlPairHub | None = field(default=None, repr=False)
    _struct_mixed: _lib.DlPairHubMixed | None = field(default=None, repr=False)

    @property
    def n_steps(self) -> int:
        return int(self.step_v.shape[0])

    @property
    def mixed(self) -> bool:
        """A plan of build_mixed: five lists per item (dl_pair_hub_mixed), not three."""
        return int(self.item_step.shape[1]) == len(HUB_MIXED_SHAPES) + 1

    @property
    def shapes(self):
        """Slot -> gathered row of the step shapes, list by list."""
        return HUB_MIXED_SHAPES if self.mixed else HUB_SHAPES

    @property
    def n_gathered(self) -> int:
        """Partner row pairs the hub steps gather."""
        return int((self.step_v >= 0).sum())

    @staticmethod
    def build(row, col, pair, pair2, n_nodes: int, n_rows: int, n_slices: int, bounds, rest_csr,
              item_rows: int | None = None) -> "HubPlan":
        """``row, col, pair, pair2`` (int64; pair2 may be None): the forward entries; ``n_rows`` = T; ``bounds`` the
        list's column slice boundaries; ``rest_csr(keep)`` builds the residual plan from the entries ``keep`` selects;
        ``item_rows``: gathered partner rows per work item (None = HUB_ITEM_ROWS, the scorer's)."""
        item_rows = HUB_ITEM_ROWS if item_rows is None else int(item_rows)
        dev = row.device
        ar = lambda n: torch.arange(n, device=dev)
        excl = lambda x: torch.cumsum(x, 0) - x
        rank, order, n_live = hub_rank(row, n_nodes)
        T = max(0, min(int(n_rows), n_live))
        nb = (T + HUB_W - 1) // HUB_W
        block_row = torch.full((nb * HUB_W,), -1, dtype=torch.int64, device=dev)
        block_row[:T] = order[:T]
        in_hub = rank[row] < T
        hrow, v, q = row[in_hub], col[in_hub], pair[in_hub]
        q2 = None if pair2 is None else pair2[in_hub]
        E = int(v.numel())
        blk = torch.div(rank[hrow], HUB_W, rounding_mode="floor")
        ul = rank[hrow] - blk * HUB_W
        sl = torch.bucketize(v, bounds.to(dev), right=True) if n_slices > 1 else torch.zeros_like(v)
        n_streams = min(n_slices, DEFAULT_SLICES)
        # groups = the entries of one (block, slice) on one partner row; a partner row lies in one slice
        key = (blk * n_slices + sl) * n_nodes + v
        perm = torch.argsort(key, stable=True)
        key, blk, sl, v, ul, q = key[perm], blk[perm], sl[perm], v[perm], ul[perm], q[perm]
        q2 = None if q2 is None else q2[perm]
        gnew = torch.ones(E, dtype=torch.bool, device=dev)
        gnew[1:] = key[1:] != key[:-1]
        gfirst = torch.nonzero(gnew).reshape(-1)
        g_of = torch.cumsum(gnew, 0) - 1
        G = int(gfirst.numel())
        c = torch.bincount(g_of, minlength=G)
        g_bs = torch.div(key[gfirst], n_nodes, rounding_mode="floor")          # block * n_slices + slice
        nC, rem = torch.div(c, 4, rounding_mode="floor"), c % 4
        hasB, hasA = (rem >= 2).long(), ((rem == 1) | (rem == 3)).long()
        gath = nC + hasB + hasA
        # work items: a (block, slice), cut where its groups have gathered HUB_ITEM_ROWS partner rows
        bs_new = torch.ones(G, dtype=torch.bool, device=dev)
        bs_new[1:] = g_bs[1:] != g_bs[:-1]
        bs_first = torch.nonzero(bs_new).reshape(-1)
        bs_of = torch.cumsum(bs_new, 0) - 1
        cum = excl(gath)
        part = torch.div(cum - cum[bs_first][bs_of], item_rows, rounding_mode="floor")
        inew = bs_new.clone()
        inew[1:] |= part[1:] != part[:-1]
        ifirst = torch.nonzero(inew).reshape(-1)
        i_of = torch.cumsum(inew, 0) - 1                                        # item of every group
        I = int(ifirst.numel())
        within = lambda x: excl(x) - excl(x)[ifirst][i_of]                      # exclusive count inside the item
        cC, cB, cA = within(nC), within(hasB), within(hasA)
        tot = lambda x: torch.zeros(I, dtype=torch.int64, device=dev).index_add_(0, i_of, x)
        nC_i, nB_i, nA_i = tot(nC), (tot(hasB) + 1) // 2, (tot(hasA) + 3) // 4
        n_i = nA_i + nB_i + nC_i
        i_blk = torch.div(g_bs[ifirst], n_slices, rounding_mode="floor")
        i_sl = g_bs[ifirst] - i_blk * n_slices
        # storage: one stream of items per XCD, the slices of a stream one after the other, largest item first inside
        big = int(n_i.max()) + 1 if I else 1
        iperm = torch.argsort(((i_sl % n_streams) * (n_slices + 1) + i_sl) * big + (big - 1 - n_i), stable=True)
        ipos = torch.empty_like(iperm)
        ipos[iperm] = ar(I)
        base = torch.empty(I, dtype=torch.int64, device=dev)
        base[iperm] = excl(n_i[iperm])
        item_step = torch.stack([base, base + nA_i, base + nA_i + nB_i, base + n_i], dim=1)
        per_stream = torch.bincount(i_sl % n_streams, minlength=n_streams)
        slice_item0 = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
        slice_item0[1:] = torch.cumsum(per_stream, 0)
        S = int(n_i.sum())
        # slots
        p = ar(E) - gfirst[g_of]
        e_c, e_nC, e_item = c[g_of], nC[g_of], i_of[g_of]
        r = p - 4 * e_nC
        isC = r < 0
        isB = ~isC & (e_c % 4 >= 2) & (r < 2)
        isA = ~isC & ~isB
        eA, eB, eC = item_step[e_item, 0], item_step[e_item, 1], item_step[e_item, 2]
        half, aslot = cB[g_of], cA[g_of]
        step = torch.where(isC, eC + cC[g_of] + torch.div(p, 4, rounding_mode="floor"),
                           torch.where(isB, eB + torch.div(half, 2, rounding_mode="floor"),
                                       eA + torch.div(aslot, 4, rounding_mode="floor")))
        slot = torch.where(isC, p % 4, torch.where(isB, (half % 2) * 2 + r, aslot % 4))
        vset = torch.where(isC, torch.zeros_like(p), torch.where(isB, half % 2, aslot % 4))
        mk = lambda fill: torch.full((S, 4), fill, dtype=torch.int64, device=dev)
        step_v, step_u, step_q = mk(-1), mk(0), mk(-1)
        step_v[step, vset] = v
        step_u[step, slot] = ul
        step_q[step, slot] = q
        step_q2 = None
        if q2 is not None:
            step_q2 = mk(-1)
            step_q2[step, slot] = q2
        rest = rest_pair = rest_pair2 = None
        if int((~in_hub).sum()):
            got = rest_csr(~in_hub)
            rest, rest_pair = got[0], got[1]
            rest_pair2 = got[2] if len(got) > 2 else None
        item_block = torch.empty(I, dtype=torch.int64, device=dev)
        item_block[ipos] = i_blk
        item_slice = torch.empty(I, dtype=torch.int64, device=dev)
        item_slice[ipos] = i_sl
        item_step_s = torch.empty_like(item_step)
        item_step_s[ipos] = item_step
        return HubPlan(T, nb, _i32(block_row), I, n_streams, int(per_stream.max()) if I else 0, _i32(slice_item0),
                       _i32(item_block), _i32(item_slice), _i32(item_step_s), _i32(step_v), _i32(step_u), _i32(step_q),
                       None if step_q2 is None else _i32(step_q2), E, rest, rest_pair, rest_pair2)

    @staticmethod
    def build_mixed(row, col, pair, pair2, n_nodes: int, n_rows: int, n_slices: int, bounds, rest_csr,
                    item_rows: int | None = None, mixed: bool = True) -> "HubPlan":
        """The MIXED plan (dl_pair_hub_mixed): arguments, ranks, blocks, column slices and work items as in ``build`` —
        ``row`` is the hub row of an entry, which PairList.build chooses by ``hub_owner`` — but an item holds FIVE lists
        [A | A211 | B | B31 | C] and ``item_step`` is [n_items, 6].  The c slots of a group give c // 4 C steps and, for a
        remainder of 1, 2 or 3, ONE piece that gathers its partner row once.  Per item: 3-pieces pair with 1-pieces (B31),
        2-pieces with each other (B), an odd 2-piece takes up to two 1-pieces (A211; none left: it closes list B), the
        1-pieces left go in fours (A).  A list's leftover closes its last step with dead slots and dead rows; a 3-piece that
        finds no 1-piece closes list B31, and any further one is a C step whose fourth slot is dead — a dead slot, never a
        dead row, so the kernel's contract holds (check).  ``mixed=False`` cuts a remainder of 3 into 2 + 1 and fills A
        and B only: the packing of ``build`` in this layout, for A/B runs."""
        item_rows = HUB_ITEM_ROWS if item_rows is None else int(item_rows)
        dev = row.device
        ar = lambda n: torch.arange(n, device=dev)
        excl = lambda x: torch.cumsum(x, 0) - x
        # ranks, blocks, groups and work items: build's, with one gather per remainder
        rank, order, n_live = hub_rank(row, n_nodes)
        T = max(0, min(int(n_rows), n_live))
        nb = (T + HUB_W - 1) // HUB_W
        block_row = torch.full((nb * HUB_W,), -1, dtype=torch.int64, device=dev)
        block_row[:T] = order[:T]
        in_hub = rank[row] < T
        hrow, v, q = row[in_hub], col[in_hub], pair[in_hub]
        q2 = None if pair2 is None else pair2[in_hub]
        E = int(v.numel())
        blk = torch.div(rank[hrow], HUB_W, rounding_mode="floor")
        ul = rank[hrow] - blk * HUB_W
        sl = torch.bucketize(v, bounds.to(dev), right=True) if n_slices > 1 else torch.zeros_like(v)
        n_streams = min(n_slices, DEFAULT_SLICES)
        key = (blk * n_slices + sl) * n_nodes + v
        perm = torch.argsort(key, stable=True)
        key, v, ul, q = key[perm], v[perm], ul[perm], q[perm]
        q2 = None if q2 is None else q2[perm]
        gnew = torch.ones(E, dtype=torch.bool, device=dev)
        gnew[1:] = key[1:] != key[:-1]
        gfirst = torch.nonzero(gnew).reshape(-1)
        g_of = torch.cumsum(gnew, 0) - 1
        G = int(gfirst.numel())
        c = torch.bincount(g_of, minlength=G)
        g_bs = torch.div(key[gfirst], n_nodes, rounding_mode="floor")
        nC, rem = torch.div(c, 4, rounding_mode="floor"), c % 4
        gath = nC + (rem > 0).long() if mixed else hub_gathers(c)
        bs_new = torch.ones(G, dtype=torch.bool, device=dev)
        bs_new[1:] = g_bs[1:] != g_bs[:-1]
        bs_first = torch.nonzero(bs_new).reshape(-1)
        bs_of = torch.cumsum(bs_new, 0) - 1
        cum = excl(gath)
        part = torch.div(cum - cum[bs_first][bs_of], item_rows, rounding_mode="floor")
        inew = bs_new.clone()
        inew[1:] |= part[1:] != part[:-1]
        ifirst = torch.nonzero(inew).reshape(-1)
        i_of = torch.cumsum(inew, 0) - 1
        I = int(ifirst.numel())
        tot = lambda at, x: torch.zeros(I, dtype=torch.int64, device=dev).index_add_(0, at, x)
        cC, nC_i = excl(nC) - excl(nC)[ifirst][i_of], tot(i_of, nC)
        # pieces, in group order: (group, slots, first slot inside the group)
        if mixed:
            pg = torch.nonzero(rem > 0).reshape(-1)
            psz, poff = rem[pg], 4 * nC[pg]
        else:
            g2, g1 = torch.nonzero(rem >= 2).reshape(-1), torch.nonzero((rem == 1) | (rem == 3)).reshape(-1)
            pg = torch.cat([g2, g1])
            psz = torch.cat([torch.full_like(g2, 2), torch.ones_like(g1)])
            poff = torch.cat([4 * nC[g2], 4 * nC[g1] + 2 * (rem[g1] == 3).long()])
            o = torch.argsort(pg * 2 + (psz == 1).long(), stable=True)
            pg, psz, poff = pg[o], psz[o], poff[o]
        Pn = int(pg.numel())
        pit = i_of[pg]

        def ranked(size):                                           # (pieces of this size per item, a piece's number among them)
            m = (psz == size).long()
            n = tot(pit, m)
            return n, excl(m) - excl(n)[pit]
        (n1, k1), (n2, k2), (n3, k3) = ranked(1), ranked(2), ranked(3)
        m31 = torch.minimum(n3, n1)                                  # full B31 steps
        x3, r1 = n3 - m31, n1 - m31                                  # 3-pieces / 1-pieces without a partner
        nB, odd2 = torch.div(n2, 2, rounding_mode="floor"), n2 % 2
        s211 = odd2 * torch.clamp(r1, max=2) if mixed else torch.zeros_like(r1)      # 1-pieces beside the odd 2-piece
        lens = torch.stack([(r1 - s211 + 3) // 4, (s211 > 0).long(), nB + odd2 * (s211 == 0).long(), m31 + (x3 > 0).long(),
                            nC_i + torch.clamp(x3 - 1, min=0)], dim=1)
        n_i = lens.sum(1)
        i_blk = torch.div(g_bs[ifirst], n_slices, rounding_mode="floor")
        i_sl = g_bs[ifirst] - i_blk * n_slices
        big = int(n_i.max()) + 1 if I else 1
        iperm = torch.argsort(((i_sl % n_streams) * (n_slices + 1) + i_sl) * big + (big - 1 - n_i), stable=True)
        ipos = torch.empty_like(iperm)
        ipos[iperm] = ar(I)
        base = torch.empty(I, dtype=torch.int64, device=dev)
        base[iperm] = excl(n_i[iperm])
        item_step = torch.cat([base[:, None], base[:, None] + torch.cumsum(lens, 1)], dim=1)      # [I, 6]
        per_stream = torch.bincount(i_sl % n_streams, minlength=n_streams)
        slice_item0 = torch.zeros(n_streams + 1, dtype=torch.int64, device=dev)
        slice_item0[1:] = torch.cumsum(per_stream, 0)
        S = int(n_i.sum())
        # where a piece goes: (list, step inside the list, its first slot, its row of the step)
        LA, LA211, LB, LB31, LC = range(5)
        m31p, s211p, nBp = m31[pit], s211[pit], nB[pit]
        j1 = k1 - m31p                                               # a 1-piece's number among those without a 3-piece
        in31, in211, jA = k1 < m31p, (k1 >= m31p) & (j1 < s211p), j1 - s211p
        last2 = k2 == 2 * nBp                                        # the odd 2-piece
        w = torch.where
        is1, is2 = psz == 1, psz == 2
        p_list = w(is1, w(in31, LB31, w(in211, LA211, LA)), w(is2, w(last2 & (s211p > 0), LA211, LB), w(k3 <= m31p, LB31, LC)))
        p_step = w(is1, w(in31, k1, w(in211, 0, torch.div(jA, 4, rounding_mode="floor"))),
                   w(is2, w(last2, w(s211p > 0, 0, nBp), torch.div(k2, 2, rounding_mode="floor")),
                     w(k3 <= m31p, k3, nC_i[pit] + k3 - m31p - 1)))
        p_slot = w(is1, w(in31, 3, w(in211, 2 + j1, jA % 4)), w(is2 & ~last2, 2 * (k2 % 2), 0))
        p_row = w(is1, w(in31, 1, w(in211, 1 + j1, jA % 4)), w(is2 & ~last2, k2 % 2, 0))
        p_at = item_step[pit, p_list] + p_step
        # slots: the first 4 * (c // 4) entries of a group fill its C steps, the others are its piece(s)
        p = ar(E) - gfirst[g_of]
        isC = p < 4 * nC[g_of]
        g_piece = torch.full((G,), Pn, dtype=torch.int64, device=dev)
        if Pn:
            g_piece.scatter_reduce_(0, pg, ar(Pn), reduce="amin")
        pe = torch.clamp(g_piece[g_of], max=max(Pn - 1, 0))
        if not mixed and Pn:
            pe = pe + (~isC & (p >= poff[pe] + psz[pe])).long()      # the 1 of a 2 + 1
        if Pn == 0:
            p_at = p_slot = p_row = poff = torch.zeros(1, dtype=torch.int64, device=dev)
        step = w(isC, item_step[i_of[g_of], LC] + cC[g_of] + torch.div(p, 4, rounding_mode="floor"), p_at[pe])
        slot = w(isC, p % 4, p_slot[pe] + p - poff[pe])
        vset = w(isC, torch.zeros_like(p), p_row[pe])
        mk = lambda fill: torch.full((S, 4), fill, dtype=torch.int64, device=dev)
        step_v, step_u, step_q = mk(-1), mk(0), mk(-1)
        step_v[step, vset] = v
        step_u[step, slot] = ul
        step_q[step, slot] = q
        step_q2 = None
        if q2 is not None:
            step_q2 = mk(-1)
            step_q2[step, slot] = q2
        rest = rest_pair = rest_pair2 = None
        if int((~in_hub).sum()):
            got = rest_csr(~in_hub)
            rest, rest_pair = got[0], got[1]
            rest_pair2 = got[2] if len(got) > 2 else None
        item_block = torch.empty(I, dtype=torch.int64, device=dev)
        item_block[ipos] = i_blk
        item_slice = torch.empty(I, dtype=torch.int64, device=dev)
        item_slice[ipos] = i_sl
        item_step_s = torch.empty_like(item_step)
        item_step_s[ipos] = item_step
        return HubPlan(T, nb, _i32(block_row), I, n_streams, int(per_stream.max()) if I else 0, _i32(slice_item0),
                       _i32(item_block), _i32(item_slice), _i32(item_step_s), _i32(step_v), _i32(step_u), _i32(step_q),
                       None if step_q2 is None else _i32(step_q2), E, rest, rest_pair, rest_pair2)

    def to(self, device) -> "HubPlan":
        mv = lambda t: None if t is None else t.to(device)
        return HubPlan(self.n_rows, self.n_blocks, mv(self.block_row), self.n_items, self.n_slices, self.slice_max_item,
                       mv(self.slice_item0), mv(self.item_block), mv(self.item_slice), mv(self.item_step), mv(self.step_v),
                       mv(self.step_u), mv(self.step_q), mv(self.step_q2), self.n_entries, mv(self.rest),
                       mv(self.rest_pair), mv(self.rest_pair2))

    def check(self) -> None:
        """Refuse a plan the kernel would fault on.  hub::score_fwd_wave_kernel gathers the partner rows of every step but
        the last of an item's A list and B list without looking at them: a dead partner row (-1) anywhere else, or in
        front of a live one, is a read outside the tables.  Run once, when the plan is bound (c_value)."""
        if self.n_items == 0:
            return
        dev = self.step_v.device
        st = self.item_step.long()
        shapes = self.shapes                                                    # slot -> row of every list; the last list is C
        lens = (st[:, 1:] - st[:, :-1]).reshape(-1)
        ends = torch.cumsum(lens, 0)
        ok = bool((lens >= 0).all()) and int(ends[-1]) == self.n_steps and bool((st[1:, 0] == st[:-1, -1]).all()) \
            and int(st[0, 0]) == 0
        if ok:
            smap = torch.repeat_interleave(torch.tensor(shapes, device=dev).repeat(self.n_items, 1), lens, dim=0)    # [n_steps, 4]
            nv = smap[:, 3] + 1
            is_c = torch.repeat_interleave(torch.arange(len(shapes), device=dev).repeat(self.n_items), lens) == len(shapes) - 1
            last = torch.zeros(self.n_steps, dtype=torch.bool, device=dev)
            last[(ends - 1)[lens > 0]] = True
            used = torch.arange(4, device=dev)[None, :] < nv[:, None]            # the partner rows a step of this shape gathers
            live = (self.step_v >= 0) & used
            full = ~last | is_c                                                 # a C step is never short
            ok = not bool(((used & ~live)[full]).any()) and bool(live[:, 0].all()) \
                and not bool((live[:, 1:] & ~live[:, :-1]).any())
            if ok and self.mixed:                                               # a live slot scores against a live row
                ok = not bool(((self.step_q >= 0) & ~torch.gather(live, 1, smap)).any())
        if not ok:
            raise ValueError("hub plan: dead partner rows may only close the last step of an item's A list and B list "
                             "(dl_pair_hub, disenlink_hip.h)" if not self.mixed else
                             "mixed hub plan: dead partner rows may only close the last step of an item's A, A211, B and B31 "
                             "lists, and no live slot scores against one (dl_pair_hub_mixed, disenlink_hip.h)")

    def c_value(self) -> _lib.DlPairHub:
        if self._struct is None:
            self.check()
            ptr = lambda t: None if t is None else t.data_ptr()
            self._struct = _lib.DlPairHub(
                self.n_blocks, ptr(self.block_row), self.n_items, self.n_slices, self.slice_max_item, ptr(self.slice_item0),
                ptr(self.item_block), ptr(self.item_step), self.n_steps, ptr(self.step_v), ptr(self.step_u),
                ptr(self.step_q), ptr(self.step_q2), self.n_entries,
                self.rest.c_value() if self.rest is not None else _lib.DlCsrPlan(), ptr(self.rest_pair), ptr(self.rest_pair2))
        return self._struct

    def c_value_mixed(self) -> _lib.DlPairHubMixed:
        if self._struct_mixed is None:
            if not self.mixed:
                raise ValueError("not a mixed hub plan (HubPlan.build_mixed)")
            self._struct_mixed = _lib.DlPairHubMixed(self.c_value(), len(HUB_MIXED_SHAPES))
        return self._struct_mixed


# Work item length of the ROUTING hub plan, in gathered partner rows, and its column slices (the partner rows of a slice are
# gathered by the XCDs that serve its stream, like a pair list's).  The scorer's HUB_ITEM_ROWS = 512 would leave 299 items
# for the 256 CUs of squirrel_real's 78,062 gathered rows, and a wave is a chain of dependent steps: the longest item is the
# kernel's tail.  route_fwd alone on squirrel_real, us per call with the row sums, median of 12 interleaved rounds
# (profiles/r14_route_hub.txt): 28.5 on the routing plan; 4 slices at 32 / 64 / 96 / 128 / 160 / 256 rows 26.6 / 24.3 / 24.0 /
# 22.8 / 24.2 / 30.5; 128 rows in 1 / 2 / 8 slices 25.5 / 23.0 / 25.8 (a stream per XCD leaves items of a few steps).
# The routing PLAN stays unsliced (from_edge_rows).
ROUTE_HUB_ITEM_ROWS = 128
ROUTE_HUB_SLICES = 4


def route_hub_plan(row: torch.Tensor, col: torch.Tensor, rev: torch.Tensor, n_nodes: int, force: bool = False) -> HubPlan | None:
    """The hub plan the routing kernel walks instead of the mirrored routing plan (dl_graph.route_hub), or None.
    ``row, col`` (int64): every directed entry of the symmetric CSR, ``rev`` its reverse-edge permutation.  Each entry e
    with col >= row — one per undirected edge — becomes a slot of the block row of its OWNER, the endpoint of larger
    degree (ties: the smaller node id), scored against the other endpoint as the partner row: on a skewed graph the
    hubs then own most edges and a block of 16 of them gathers a partner row once for several.  The slot carries e
    and rev[e] (-1 for a self-loop): routing is symmetric, both entries get the result.  ROUTE_HUB_SLICES column slices of
    the partner rows, no residual plan.
    Built where the first block of 16 owners shares gathered rows (auto_hub_rows — the scorer's rule), always with
    ``force``; a graph without entries has none."""
    e = torch.nonzero(col >= row).reshape(-1)
    if e.numel() == 0:
        return None
    r, c = row[e], col[e]
    deg = torch.bincount(row, minlength=n_nodes)
    swap = deg[c] > deg[r]                                         # c >= r: a tie stays with the smaller id
    owner, partner = torch.where(swap, c, r), torch.where(swap, r, c)
    e2 = rev[e]
    e2 = torch.where(e2 == e, torch.full_like(e2, -1), e2)
    T = int((torch.bincount(owner, minlength=n_nodes) > 0).sum()) if force else auto_hub_rows(owner, partner, n_nodes)
    if T == 0:
        return None
    S = ROUTE_HUB_SLICES
    bnd = slice_bounds(partner, S) if S > 1 else None
    return HubPlan.build(owner, partner, e, e2, n_nodes, T, S, bnd, None, item_rows=ROUTE_HUB_ITEM_ROWS)


@dataclass
class PairList(_PlanOwner):
    """Scored pairs ``(pu[q], pv[q])`` with the two CSR views the kernels walk:
    ``by_u`` — every pair once, in the row of its first endpoint (forward scorer), and
    ``inc``  — every pair twice, once per endpoint (backward; rows = nodes ``[row_offset, +n_rows)``).
    Both are XCD-sliced by the second endpoint by default.

    ``fwd`` is the plan the forward scorer walks: ``by_u`` itself, or (``fold_mirrors``, the default, where the list holds
    mirrors) a by-u plan in which a listed ``(u, v)`` whose reverse ``(v, u)`` is listed too occupies ONE entry that carries
    both pair ids (``fwd_pair`` and ``fwd_pair2``, -1 = none) — the score is symmetric, the second gather of the two rows
    is work the result does not need."""
    n_nodes: int
    pu: torch.Tensor
    pv: torch.Tensor
    by_u: CsrPlan
    by_u_pair: torch.Tensor
    inc: CsrPlan
    inc_pair: torch.Tensor
    fwd: CsrPlan | None = None                       # None = by_u (nothing folded)
    fwd_pair: torch.Tensor | None = None
    fwd_pair2: torch.Tensor | None = None
    hub: HubPlan | None = None                       # the forward entries as hub blocks + a residual plan (None: no hub rows)
    hub_mixed: HubPlan | None = None                 # the same entries as a mixed plan (HubPlan.build_mixed), walked instead of `hub`
    _struct: _lib.DlPairIncidence | None = field(default=None, repr=False)
    _struct_u: _lib.DlPairIncidence | None = field(default=None, repr=False)
    _yw: torch.Tensor | None = field(default=None, repr=False)      # per-entry (label, signed weight): bind_labels
    _yw_key: tuple | None = field(default=None, repr=False)
    _yw_seen: tuple | None = field(default=None, repr=False)
    _yw_signed: tuple | None = field(default=None, repr=False)     # the (label, weight) found to hold a sign bit: not bound
    static_labels: bool = False                                   # the caller's word that label / weight never change: bind_labels
    _ws_need: dict = field(default_factory=dict, repr=False)          # (K, d) -> bytes: workspace_bytes

    def __post_init__(self):
        _assign_handle(self)

    def bind_labels(self, label: torch.Tensor, weight: torch.Tensor, n_pairs_total: int | None = None) -> None:
        """Lay the labels / loss weights of a training step out per incidence entry (dl_pair_incidence.entry_yw: a
        coalesced stream instead of two random reads per entry; the weight's sign picks the one entry of a pair that
        writes prob) — for the label and weight tensors the loop passes EVERY epoch (main_disentangled.py:195: the masks
        are fixed for a run).  Keyed on the tensors' identity and version counter; built the second time the same pair
        of tensor OBJECTS is seen, so a caller that draws new labels for every step never pays for it — and never gets the
        stream of an earlier tensor that lived at the same address.  Writes that bypass the
        version counter (``.data``, raw kernels) are not seen: call ``unbind_labels()`` after such a write.

        Signed weights.  The weight is any real number, and the kernels read a caller's array signed; the stream has no
        room for that, because the sign of ITS weight is the writer flag.  Of the two ways out — carrying the flag elsewhere
        (a third stream column, or the sign of the label, which soft labels leave free but which a -0.0 label would not)
        or not binding such a tensor — the second is taken: a weight tensor that holds a set sign bit anywhere (negative,
        -0.0, a NaN with the bit set) is never bound and keeps the gathers, where every entry writes prob and the weight
        keeps its sign.  That costs one host read of one flag at bind time (the second sight only, never per step) and
        leaves the stream, its 8 bytes per entry and the kernels' fast path for the weights training loops have: w >= 0.

        Captured steps.  While the current stream is capturing, nothing is bound and the gathers are recorded: a replay
        then reads what ``label`` and ``weight`` hold at replay time, which is how a captured graph is fed.  A caller
        whose labels never change during the run says so with ``static_labels = True`` (train._graphed_epoch does): the
        stream its warm-up calls bound is then recorded instead, and a later in-place write is the caller's breach.  No
        stream is ever BUILT during a capture (that takes a host read)."""
        capturing = label.is_cuda and torch.cuda.is_current_stream_capturing()
        if os.environ.get("DL_ENTRY_LABELS", "1") == "0" or label.is_inference() or weight.is_inference() \
                or (capturing and not self.static_labels):          # (A/B runs; no version counter; a replay reads live labels)
            self.unbind_labels()
            return
        # identity = the tensor OBJECTS (weak references) and their version counters: an address can be handed to a new
        # tensor with other contents — a caller that makes its labels afresh every step gets the same data_ptr and version 0
        # again and again — an object cannot
        def same(key):
            return key is not None and key[0]() is label and key[1]() is weight and key[2:] == (label._version, weight._version)
        if not same(self._yw_key):
            key = (weakref.ref(label), weakref.ref(weight), label._version, weight._version)
            if not same(self._yw_seen):                             # first sight: keep the gathers, remember the pair
                self._yw_seen = key
                self.unbind_labels()
                return
            # a capture in progress (no host read allowed), or a set sign bit anywhere (one host read per tensor version,
            # remembered in _yw_signed): the gathers
            if capturing or same(self._yw_signed) or bool(torch.signbit(weight).any()):
                if not capturing:
                    self._yw_signed = key
                self.unbind_labels()
                return
            q = self.inc_pair.long()
            deg = (self.inc.rowptr[1:] - self.inc.rowptr[:-1]).long()
            rows = torch.repeat_interleave(torch.arange(self.inc.n_rows, device=q.device), deg) + self.inc.row_offset
            first = rows == self.pu.long()[q]                        # the entry in the row of the pair's first endpoint
            w = weight.reshape(-1).float()[q]
            self._yw = torch.stack([label.reshape(-1).float()[q], torch.where(first, w, -w)], dim=1).contiguous()
            self._yw_key = key
        self.c_struct(n_pairs_total)
        self._struct.entry_yw = self._yw.data_ptr()

    def unbind_labels(self) -> None:
        self._yw = self._yw_key = None
        if self._struct is not None:
            self._struct.entry_yw = None

    @property
    def n_pairs(self) -> int:
        return int(self.pu.numel())

    @staticmethod
    def build(pu: torch.Tensor, pv: torch.Tensor, n_nodes: int, seg_len: int = DEFAULT_INC_SEG_LEN,
              run_len: int = DEFAULT_RUN_LEN, row_range: tuple[int, int] | None = None,
              n_slices: int | None = None, by_u_range: tuple[int, int] | None = None,
              build_by_u: bool = True, row_bytes: int = 2048, inc_slices: int | None = None,
              fold_mirrors: bool = True, hub_rows: int | None = None, hub_mixed: bool | None = None) -> "PairList":
        """``row_range`` restricts the incidence rows to one shard's nodes (the pair ids in ``inc_pair``
        then index prob / g_prob arrays covering the whole pair list); ``by_u_range`` restricts the rows
        of the forward plan (every pu must lie inside it).  ``n_slices`` / ``inc_slices``: column slices of the forward
        plan / of the incidence plan (defaults: auto_slices / auto_inc_slices — the incidence plan pays a partial slot
        per (row, slice) group, the forward plan sums nothing across segments).  ``fold_mirrors=False`` keeps the forward
        scorer on ``by_u`` (one entry per listed pair), which is built the same either way.  ``hub_rows``: how many of the
        rows with the most forward entries are scored by blocks of HUB_W rows (HubPlan) — None = auto_hub_rows (a list
        without hub rows, or a row shard, gets none and nothing changes), 0 = none.  ``hub_mixed``: whether the list also
        gets the mixed plan (HubPlan.build_mixed over the hub_owner orientation, the same number of hub rows), which the
        scorer then walks instead of ``hub`` — None = wherever it gets a hub plan, False = never, True = it must."""
        pu = pu.reshape(-1).to(torch.int64)
        pv = pv.reshape(-1).to(torch.int64)
        if pu.numel() != pv.numel():
            raise ValueError("pu and pv differ in length")
        P = pu.numel()
        if n_slices is None:
            n_slices = auto_slices(n_nodes, row_bytes, entries_per_row=P / max(1, len(torch.unique(pu))))
        if inc_slices is None:
            # (from the WHOLE list, whatever row_range says: a shard must cut its rows exactly as the unsharded plan does)
            inc_slices = auto_inc_slices(n_nodes, row_bytes, entries_per_row=2.0 * P / max(1, n_nodes))
        if 2 * P >= 2 ** 31:
            raise ValueError("too many pairs for int32 incidence")
        if P and (int(torch.minimum(pu.min(), pv.min())) < 0 or int(torch.maximum(pu.max(), pv.max())) >= n_nodes):
            raise ValueError("pair endpoint outside [0, n_nodes)")
        dev = pu.device
        ids = torch.arange(P, device=dev)

        def csr(node, other, pair, lo, hi, seg, unit_segs=UNIT_SEGS, slices=None, pair2=None, bnd=None):
            slices = n_slices if slices is None else slices
            # slice boundaries from ALL entries of the list (before the row range cuts it): the same for every shard
            if bnd is None:
                bnd = slice_bounds(other, slices) if slices > 1 and other.numel() else None
            keep = (node >= lo) & (node < hi)
            node, other, pair = node[keep], other[keep], pair[keep]
            pair2 = None if pair2 is None else pair2[keep]
            order = torch.argsort((node - lo) * n_nodes + other, stable=True)   # fixed order -> reproducible sums
            rowptr = torch.zeros(hi - lo + 1, dtype=torch.int64, device=dev)
            if node.numel():
                rowptr[1:] = torch.cumsum(torch.bincount(node - lo, minlength=hi - lo), dim=0)
            plan = CsrPlan.build(rowptr, other[order], n_nodes, row_offset=lo, seg_len=seg, n_slices=slices,
                                 unit_segs=unit_segs, by_length=length_order(n_nodes, row_bytes), bounds=bnd)
            return (plan, _i32(pair[order])) if pair2 is None else (plan, _i32(pair[order]), _i32(pair2[order]))

        ulo, uhi = (0, n_nodes) if by_u_range is None else by_u_range
        if P and build_by_u and (int(pu.min()) < ulo or int(pu.max()) >= uhi):
            raise ValueError("a first endpoint lies outside by_u_range")
        if build_by_u:
            by_u, by_u_pair = csr(pu, pv, ids, ulo, uhi, run_len, unit_segs=1)     # the forward scorer sums nothing across segments
        else:                                              # backward-only list (sharded runs): empty forward plan
            by_u, by_u_pair = csr(pu[:0], pv[:0], ids[:0], 0, 0, run_len, unit_segs=1)
        lo, hi = (0, n_nodes) if row_range is None else row_range
        inc, inc_pair = csr(torch.cat([pu, pv]), torch.cat([pv, pu]), ids.repeat(2), lo, hi, seg_len, slices=inc_slices)
        fwd = fwd_pair = fwd_pair2 = None
        f_u, f_v, f_q, f_q2 = pu, pv, ids, None                    # the forward entries
        if build_by_u and fold_mirrors:
            second = mirror_partners(pu, pv, n_nodes)
            if bool((second >= 0).any()):
                kept = torch.ones(P, dtype=torch.bool, device=dev)
                kept[second[second >= 0]] = False                  # the partner is scored by the entry that names it
                f_u, f_v, f_q, f_q2 = pu[kept], pv[kept], ids[kept], second[kept]
                fwd, fwd_pair, fwd_pair2 = csr(f_u, f_v, f_q, ulo, uhi, run_len, unit_segs=1, pair2=f_q2)
        hub = None
        if hub_rows is not None and hub_rows > 0 and (by_u_range is not None or not build_by_u):
            raise ValueError("hub rows need the full-range forward plan")
        if build_by_u and by_u_range is None and P and hub_rows != 0:
            T = auto_hub_rows(f_u, f_v, n_nodes) if hub_rows is None else int(hub_rows)
            if T > 0:
                bnd = slice_bounds(f_v, n_slices) if n_slices > 1 else None     # the forward plan's own boundaries
                rest_csr = lambda keep: csr(f_u[keep], f_v[keep], f_q[keep], 0, n_nodes, run_len, unit_segs=1,
                                            pair2=None if f_q2 is None else f_q2[keep], bnd=bnd)
                hub = HubPlan.build(f_u, f_v, f_q, f_q2, n_nodes, T, n_slices, bnd, rest_csr)
        mixed = None
        if hub_mixed and hub is None:
            raise ValueError("a mixed hub plan needs a list that gets a hub plan (hub_rows)")
        if hub is not None and hub_mixed is not False:
            # the decision and the number of hub rows are the listed orientation's (no list changes category); every row
            # with entries there = every owner row with entries here
            o_u, o_v = hub_owner(f_u, f_v, n_nodes) if HUB_MIXED_OWNER else (f_u, f_v)
            o_bnd = slice_bounds(o_v, n_slices) if n_slices > 1 else None
            o_rest = lambda keep: csr(o_u[keep], o_v[keep], f_q[keep], 0, n_nodes, run_len, unit_segs=1,
                                      pair2=None if f_q2 is None else f_q2[keep], bnd=o_bnd)
            mixed = HubPlan.build_mixed(o_u, o_v, f_q, f_q2, n_nodes, n_nodes if hub_rows is None else T, n_slices, o_bnd,
                                        o_rest, item_rows=HUB_MIXED_ITEM_ROWS, mixed=HUB_MIXED_SHAPES_ON)
        return PairList(n_nodes, _i32(pu), _i32(pv), by_u, by_u_pair, inc, inc_pair, fwd, fwd_pair, fwd_pair2, hub, mixed)

    def c_struct(self, n_pairs_total: int | None = None):
        if self._struct is None:
            self._struct = _lib.DlPairIncidence(self.inc.c_value(), self.inc_pair.data_ptr(),
                                                self.n_pairs if n_pairs_total is None else n_pairs_total)
        return C.byref(self._struct)

    def c_struct_by_u(self):
        """The forward scorer's plan: ``fwd`` (mirrors folded) where there is one, else ``by_u``."""
        if self._struct_u is None:
            if self.fwd is None:
                self._struct_u = _lib.DlPairIncidence(self.by_u.c_value(), self.by_u_pair.data_ptr(), self.n_pairs)
            else:
                self._struct_u = _lib.DlPairIncidence(self.fwd.c_value(), self.fwd_pair.data_ptr(), self.n_pairs, None,
                                                      self.fwd_pair2.data_ptr(), self.n_pairs - self.fwd.n_entries)
            if self.hub is not None and self.hub.n_items > 0:
                if self.hub.mixed:
                    raise ValueError("PairList.hub holds a mixed plan: that is PairList.hub_mixed")
                self._struct_u.hub = C.pointer(self.hub.c_value())
            if self.hub_mixed is not None and self.hub_mixed.n_items > 0:
                self._struct_u.hub_mixed = C.pointer(self.hub_mixed.c_value_mixed())
        return C.byref(self._struct_u)

    def c_plan(self):
        self.c_struct()
        return C.byref(self._struct.csr)
