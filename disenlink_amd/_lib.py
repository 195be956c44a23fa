"""ctypes binding of libdisenlink_hip.so (include/disenlink_hip.h).

There is no CPU or eager fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libdisenlink_hip.so")


class DlCsrPlan(C.Structure):
    _fields_ = [
        ("n_rows", C.c_int32), ("row_offset", C.c_int32), ("n_total", C.c_int32), ("n_entries", C.c_int32),
        ("rowptr", C.c_void_p), ("col", C.c_void_p),
        ("seg_len", C.c_int32), ("n_seg", C.c_int32),
        ("seg_row", C.c_void_p), ("seg_beg", C.c_void_p), ("seg_end", C.c_void_p), ("seg_slot", C.c_void_p),
        ("n_slices", C.c_int32), ("slice_max_seg", C.c_int32), ("slice_seg0", C.c_void_p),
        ("n_multi", C.c_int32), ("n_slots", C.c_int32), ("multi_row", C.c_void_p), ("multi_slot0", C.c_void_p),
        ("slot_multi", C.c_void_p), ("unit_count", C.c_void_p),
    ]


class DlPairHub(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("block_row", C.c_void_p),
                ("n_items", C.c_int32), ("n_slices", C.c_int32), ("slice_max_item", C.c_int32),
                ("slice_item0", C.c_void_p), ("item_block", C.c_void_p), ("item_step", C.c_void_p),
                ("n_steps", C.c_int32), ("step_v", C.c_void_p), ("step_u", C.c_void_p), ("step_q", C.c_void_p),
                ("step_q2", C.c_void_p), ("n_entries", C.c_int32),
                ("rest", DlCsrPlan), ("rest_pair", C.c_void_p), ("rest_pair2", C.c_void_p)]


class DlPairHubMixed(C.Structure):
    _fields_ = [("hub", DlPairHub), ("n_lists", C.c_int32)]


class DlGraph(C.Structure):
    _fields_ = [("csr", DlCsrPlan), ("route", DlCsrPlan), ("rev", C.c_void_p), ("route_mirror", C.c_int32),
                ("route_hub", C.POINTER(DlPairHub))]


class DlPairIncidence(C.Structure):
    _fields_ = [("csr", DlCsrPlan), ("inc_pair", C.c_void_p), ("n_pairs", C.c_int32), ("entry_yw", C.c_void_p),
                ("inc_pair2", C.c_void_p), ("n_second", C.c_int32), ("hub", C.POINTER(DlPairHub)),
                ("hub_mixed", C.POINTER(DlPairHubMixed))]


class DlHostCsr(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_entries", C.c_int32), ("rowptr", C.POINTER(C.c_int32)),
                ("col", C.POINTER(C.c_int32)), ("rev", C.POINTER(C.c_int32))]


class DlHostPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("seg_len", "n_seg", "n_slices", "slice_max_seg", "n_multi", "n_slots")] + \
               [(n, C.POINTER(C.c_int32)) for n in ("seg_row", "seg_beg", "seg_end", "seg_slot", "slice_seg0",
                                                    "multi_row", "multi_slot0", "slot_multi")]


class DlSparseFeatures(C.Structure):
    _fields_ = [("N", C.c_int32), ("F", C.c_int32), ("nnz", C.c_int32),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
                ("colptr", C.c_void_p), ("csc_row", C.c_void_p), ("csc_entry", C.c_void_p),
                ("seg_len", C.c_int32), ("n_seg", C.c_int32), ("colseg", C.c_void_p), ("seg_col", C.c_void_p)]


class DlNodeFilter(C.Structure):
    _fields_ = [("group", C.c_void_p), ("n_groups", C.c_int32), ("allow", C.c_void_p)]


class DlNodeFilterBetween(C.Structure):
    _fields_ = [("group_a", C.c_void_p), ("group_b", C.c_void_p), ("n_groups", C.c_int32), ("allow", C.c_void_p)]


_P = C.c_void_p          # device pointers travel as integers
_G, _I = C.POINTER(DlGraph), C.POINTER(DlPairIncidence)
_i, _f, _z = C.c_int, C.c_float, C.c_size_t
_S = C.POINTER(DlSparseFeatures)
_NF = C.POINTER(DlNodeFilter)
_NFB = C.POINTER(DlNodeFilterBetween)
EXPORTS = {
    # name: (restype, argtypes) -- one entry per symbol declared in include/disenlink_hip.h
    "dl_host_csr_from_edges": (_i, [_P, _P, C.c_int64, C.c_int32, _i, C.POINTER(DlHostCsr)]),
    "dl_host_csr_free": (None, [C.POINTER(DlHostCsr)]),
    "dl_host_plan_build": (_i, [C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32,
                                C.POINTER(DlHostPlan)]),
    "dl_host_plan_free": (None, [C.POINTER(DlHostPlan)]),
    "dl_version": (C.c_char_p, []),
    "dl_last_error": (C.c_char_p, []),
    "dl_config_reload": (None, []),
    "dl_has_fast_path": (_i, [_i, _i]),
    "dl_has_fast_path_dtype": (_i, [_i, _i, _i]),
    "dl_set_force_generic": (_i, [_i]),
    "dl_workspace_bytes": (_z, [C.POINTER(DlCsrPlan), _i, _i]),
    "dl_project_supported": (_i, [_i]),
    "dl_project_fwd_workspace_bytes": (_z, [_i, _i, _i, _i, _i, _i]),
    "dl_project_hidden_floats": (_z, [_i, _i, _i]),
    "dl_project_fwd_form": (_i, [_i, _i, _i, _i, _i, _i, _z, _i, C.POINTER(C.c_int)]),
    "dl_project_bwd_form": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int)]),
    "dl_project_fwd": (_i, [_P, _i, _i, _i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _z, _P]),
    "dl_project_xplanes_bytes": (_z, [_i, _i]),
    "dl_project_xplanes_build": (_i, [_P, _i, _i, _P, _z, _P]),
    "dl_project_fwd_xp": (_i, [_P, _i, _i, _i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _z, _P, _P]),
    "dl_project_bwd_xp": (_i, [_P, _i, _i, _i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _z, _P, _P]),
    "dl_project_bwd_workspace_bytes": (_z, [_i, _i, _i, _i, _i, _i]),
    "dl_project_bwd": (_i, [_P, _i, _i, _i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _z, _P]),
    "dl_sparse_seg_len": (_i, []),
    "dl_project_sparse_fwd_workspace_bytes": (_z, [_S, _i, _i, _i, _i]),
    "dl_project_sparse_bwd_workspace_bytes": (_z, [_S, _i, _i, _i, _i]),
    "dl_project_sparse_form": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int)]),
    "dl_project_sparse_fwd": (_i, [_S, _i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _z, _P]),
    "dl_project_sparse_bwd": (_i, [_S, _i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _z, _P]),
    "dl_route_fwd": (_i, [_G, _P, _i, _i, _i, _f, _P, _P, _P, _P, _z, _P]),
    "dl_aggregate_fwd": (_i, [_G, _P, _i, _i, _i, _f, _P, _P, _P, _P, _P, _z, _P]),
    "dl_score_pairs_fwd": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _P, _i, _I, _P, _P, _P]),
    "dl_score_allpairs_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "dl_score_allpairs_fwd_form": (_i, [_i, _i, _i, _i, _z, C.POINTER(C.c_int)]),
    "dl_score_allpairs_bwd_dense_form": (_i, [_i, _i, _i, C.POINTER(C.c_int)]),
    "dl_score_topk_form": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_int)]),
    "dl_score_allpairs_fwd": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _P, _z, _P]),
    "dl_score_allpairs_bwd": (_i, [_P, _P, _i, _i, _i, _i, _f, _I, _P, _P, _i, _P, _P, _P, _P, _P, _z, _P]),
    "dl_score_allpairs_bwd_dense_supported": (_i, [_i, _i]),
    "dl_score_allpairs_bwd_dense_workspace_bytes": (_z, [_i, _i, _i]),
    "dl_score_allpairs_bwd_dense": (_i, [_P, _P, _i, _i, _i, _f, _P, _P, _P, _P, _P, _z, _P]),
    "dl_score_allpairs_logits_workspace_bytes": (_z, [_i, _i, _i]),
    "dl_score_allpairs_logits_fwd": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _P, _z, _P]),
    "dl_score_allpairs_logits_bwd_dense": (_i, [_P, _P, _i, _i, _i, _f, _P, _P, _P, _P, _z, _P]),
    "dl_score_recon_supported": (_i, [_i, _i]),
    "dl_score_recon_form": (_i, [_i, _i, _i, _i, C.POINTER(C.c_int)]),
    "dl_score_recon_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "dl_score_recon": (_i, [_P, _P, _i, _i, _i, _f, _P, _P, _P, _P, _f, _f, _i, _P, _P, _P, _P, _P, _z, _P]),
    "dl_score_recon_form_dtype": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_int)]),
    "dl_score_recon_workspace_bytes_dtype": (_z, [_i, _i, _i, _i, _i]),
    "dl_score_recon_dtype": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _P, _P, _P, _f, _f, _i, _P, _P, _P, _P, _P, _z, _P]),
    "dl_score_recon_logits": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _P, _P, _P, _f, _f, _i, _P, _P, _P, _P, _P, _z, _P]),
    "dl_score_recon_filtered": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _P, _P, _P, _f, _f, _i, _P, _P, _P, _P, _P, _z, _P, _NF]),
    "dl_score_recon_logits_filtered": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _P, _P, _P, _f, _f, _i, _P, _P, _P, _P, _P, _z, _P, _NF]),
    "dl_score_topk_supported": (_i, [_i, _i]),
    "dl_score_mine_supported": (_i, [_i, _i]),
    "dl_score_mine_form": (_i, [_i, _i, _i, _i, C.POINTER(C.c_int)]),
    "dl_score_pair_ranks_supported": (_i, [_i, _i]),
    "dl_score_pair_ranks_form": (_i, [_i, _i, _i, _i, C.POINTER(C.c_int)]),
    "dl_score_links_supported": (_i, [_i, _i]),
    "dl_score_links_form": (_i, [_i, _i, _i, C.POINTER(C.c_int)]),
    "dl_score_scan_supported": (_i, [_i, _i, _i]),
    "dl_auc_pair_counts_supported": (_i, [_i, _i]),
    "dl_auc_pair_counts": (_i, [_P, _P, _i, _P, _i, _P, _P]),
    "dl_auc_pair_counts_add": (_i, [_P, _P, _i, _P, _i, _P, _P]),
    "dl_auc_pair_counts_grid": (_i, [_i, _i, C.POINTER(C.c_int)]),
    "dl_epoch_state_bytes": (C.c_size_t, []),
    "dl_epoch_finish": (_i, [_i, _P, _P, _P, _P, _P, C.c_double, _P, _P, C.c_longlong, C.c_longlong, _P, _i, _P]),
    "dl_score_pairs_train_supported": (_i, [_P, _i, _i, _i]),
    "dl_score_pairs_train": (_i, [_P, _P, _i, _i, _i, _f, _P, _P, _P, _P, _P, _P, _P, _z, _P]),
    "dl_adam_step": (_i, [_i, _P, _P, _P, _P, _P, _P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P]),
    "dl_adam_step_at": (_i, [_i, _P, _P, _P, _P, _P, _P, C.c_longlong, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P]),
    "dl_pair_bce": (_i, [_P, _P, _P, _i, _P, _P, _P, _z, _P]),
    "dl_score_pairs_bwd": (_i, [_P, _P, _i, _i, _i, _f, _I, _P, _P, _P, _P, _P, _P, _z, _P]),
    # the pair-list objective in logit space
    "dl_score_pairs_logits_fwd": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _P, _i, _I, _P, _P]),
    "dl_score_pairs_logits_bwd": (_i, [_P, _P, _i, _i, _i, _f, _I, _P, _P, _P, _P, _z, _P]),
    "dl_score_pairs_train_logits_supported": (_i, [_P, _i, _i, _i]),
    "dl_score_pairs_train_logits": (_i, [_P, _P, _i, _i, _i, _f, _P, _P, _P, _P, _P, _P, _P, _z, _P]),
    "dl_pair_bce_logits": (_i, [_P, _P, _P, _i, _P, _P, _P, _z, _P]),
    "dl_route_aggregate_bwd_phase1": (_i, [_G, _P, _i, _i, _i, _f, _P, _P, _P, _P, _P, _P, _P, _P, _z, _P]),
    "dl_route_aggregate_bwd_phase2": (_i, [_G, _P, _i, _i, _i, _f, _f, _P, _P, _P, _P, _P, _P, _P, _P, _i, _P, _z, _P]),
    "dl_route_aggregate_bwd": (_i, [_G, _P, _i, _i, _i, _f, _f, _P, _P, _P, _P, _P, _i, _P, _z, _P]),
    "dl_route_aggregate_bwd_scaled": (_i, [_G, _P, _i, _i, _i, _f, _f, _P, _P, _P, _P, _P, _P, _P, _P, _z, _P]),
    # fresh training negatives every epoch: the sampler and the trainer over sampled partners
    "dl_sample_negatives": (_i, [_P, _i, _i, _i, _P, _P, C.c_uint64, _P, _i, _P, _P, _P]),
    # hard negatives: Z, H, N, K, d, dtype, t, src, n_rows, m, c, exclusion, seed, epoch, exclude_self, k, logit, n_failed, stream
    "dl_sample_negatives_hard_supported": (_i, [_i, _i, _i]),
    "dl_sample_negatives_hard": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _i, _i, _i, _P, _P, C.c_uint64, _P, _i, _P, _P, _P, _P]),
}
_SAMPLED = [_P, _P, _i, _i, _i, _i, _f, _P, _i, _i, _P, _P, _P, _P, _f, _P, _P, _P, _P, _i, _P, _z, _P]
for _name in ("dl_score_sampled_train", "dl_score_sampled_train_logits"):
    EXPORTS.update({_name + "_supported": (_i, [_i, _i, _i]), _name + "_workspace_bytes": (_z, [_i] * 4),
                    _name: (_i, _SAMPLED)})
# the pairwise ranking trainer on the same draws: ... t, src, dst, n_rows, m, six lists, w, five outputs, accumulate, workspace
EXPORTS.update({
    "dl_score_sampled_bpr_train_supported": (_i, [_i, _i, _i]),
    "dl_score_sampled_bpr_train_workspace_bytes": (_z, [_i] * 5),
    "dl_score_sampled_bpr_train": (_i, [_P, _P, _i, _i, _i, _i, _f, _P, _P, _i, _i] + [_P] * 6 + [_f] + [_P] * 5 + [_i, _P, _z, _P]),
})


def _scan_rows(name: str, res, codes: list, at: int, filtered: bool = False) -> dict:
    """The EXPORTS rows of one scan entry (or sizer) from the argument codes of its plain form, written once: ``name``;
    ``name``_dtype, the same list with the dl_dtype behind its first ``at`` codes; and, where ``filtered``, ``name``_filtered,
    the list plus the node filter — which the _dtype entry then takes last as well."""
    rows = {name: (res, codes), name + "_dtype": (res, codes[:at] + [_i] + codes[at:] + [_NF] * filtered)}
    if filtered:
        rows[name + "_filtered"] = (res, codes + [_NF])
    return rows


_TAB = [_P, _P, _i, _i, _i, _f]                       # Z, H, N, K, d, t: how every scan entry starts
_EX = [_P, _P]                                        # exclusion rowptr, col
_WS = [_P, _z, _P]                                    # workspace, its size, stream
_LINKS = _TAB + _EX + [_f, _NF, _P, _z, _P]           # ... min_logit, filter, workspace, its size, rowptr
for _name, _codes, _filtered in (
        ("topk", _TAB + [_P, _i, _i] + _EX + [_i, _P, _P, _P] + _WS, True),
        ("ranks", _TAB + [_P, _i, _P, _P, _i] + _EX + [_P, _P] + _WS, True),
        ("mine", _TAB + _EX + [_f, _i, _P, _P, _P, _P, _P] + _WS, True),
        ("pair_ranks", _TAB + _EX + [_P, _i, _P, _P, _P] + _WS, True),
        ("pair_logits", _TAB + [_P, _P, _i, _P] + _WS, False),
        ("pair_terms", _TAB + [_P, _P, _i, _P, _P, _P] + _WS, False),
        ("links_count", _LINKS + [_P], False),
        ("links_fill", _LINKS + [C.c_int64, _P, _P, _P, _P], False)):
    EXPORTS.update(_scan_rows("dl_score_" + _name, _i, _codes, 5, _filtered))
for _name, _n in (("topk", 6), ("mine", 4), ("pair_logits", 3), ("pair_ranks", 3), ("pair_terms", 3), ("links", 3)):
    EXPORTS.update(_scan_rows(f"dl_score_{_name}_workspace_bytes", _z, [_i] * _n, 3))
# the budgeted link graph has the _dtype entries only: ... N, K, d, dtype, t, exclusion, min_logit, m (64-bit), filter, ...
_LINKS_TOP = _TAB[:5] + [_i, _f] + _EX + [_f, C.c_int64, _NF, _P, _z, _P]
EXPORTS.update({
    "dl_score_links_top_form": (_i, [_i, _i, _i, C.POINTER(C.c_int)]),
    "dl_score_links_top_workspace_bytes_dtype": (_z, [_i] * 4),
    "dl_score_links_top_count_dtype": (_i, _LINKS_TOP + [_P]),
    "dl_score_links_top_fill_dtype": (_i, _LINKS_TOP + [C.c_int64, _P, _P, _P, _P]),
})
# the scans between two node sets have the _dtype entries only: ZA, HA, nA, ZB, HB, nB, K, d, dtype, t, exclusion, min_logit, ...
_BETWEEN = [_P, _P, _i, _P, _P, _i, _i, _i, _i, _f] + _EX + [_f]
_LINKS_BETWEEN = _BETWEEN + [_NFB, _P, _z, _P, _P]   # ... the two-sided rule, workspace, its size, rowptr_a, rowptr_b
EXPORTS.update({
    "dl_score_mine_between_form": (_i, [_i] * 5 + [C.POINTER(C.c_int)]),
    "dl_score_mine_between_workspace_bytes_dtype": (_z, [_i] * 6),
    "dl_score_mine_between_dtype": (_i, _BETWEEN + [_i, _P, _P, _P, _P, _P] + _WS + [_NFB]),
    "dl_score_links_between_form": (_i, [_i] * 4 + [C.POINTER(C.c_int)]),
    "dl_score_links_between_workspace_bytes_dtype": (_z, [_i] * 5),
    "dl_score_links_between_count_dtype": (_i, _LINKS_BETWEEN + [_P]),
    "dl_score_links_between_fill_dtype": (_i, _LINKS_BETWEEN + [C.c_int64, _P, _P, _P, C.c_int64, _P, _P, _P, _P]),
})

DL_F32, DL_BF16 = 0, 1

_lib = None


class DisenlinkHipError(RuntimeError):
    pass


def _hip_runtime_global() -> None:
    """libdisenlink_hip.so is linked without a HIP runtime (-no-hip-rt) and binds to the one the host
    process uses.  Under PyTorch that is torch's bundled libamdhip64.so, so that torch's streams and
    allocations are valid in our launches; promote it to the global symbol scope before loading."""
    import torch  # noqa: F401  (loads torch's HIP runtime first)
    cand = [os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"),
            "/opt/rocm/lib/libamdhip64.so"]
    for path in cand:
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
            return
    raise DisenlinkHipError("no libamdhip64.so found (looked in torch/lib and /opt/rocm/lib)")


def load() -> C.CDLL:
    """Load the library once.  Raises if it was not built (python -m disenlink_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("DL_LIB_PATH", LIB_PATH)      # override: kernel experiments with alternative builds
    if not os.path.exists(path):
        raise DisenlinkHipError(
            f"{path} not found: the HIP library is required (there is no CPU fallback). "
            "Build it with `python -m disenlink_amd.build` or __graft_entry__.build().")
    _hip_runtime_global()
    lib = C.CDLL(path)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)      # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().dl_last_error().decode(errors="replace")
        raise DisenlinkHipError(f"{what} failed (code {rc}): {msg}")


PROJECT_FWD_FORM = ("split", "vec", "G", "chunks_per_group", "rows_per_launch", "launches", "xplanes")
PROJECT_BWD_FORM = ("planes", "vecA", "vecB", "recompute", "sA", "tiles_per_range", "sB", "chunks_per_range", "sC", "direct",
                    "blocked", "block_rows", "blocks", "xplanes")


def project_fwd_form(N: int, F: int, K: int, nhid: int, d: int, two_layer: bool, ws_bytes: int, have_xplanes: bool = False) -> dict:
    """Which kernel instantiation and launch mode dl_project_fwd takes for this problem (dl_project_fwd_form)."""
    out = (C.c_int * len(PROJECT_FWD_FORM))()
    check(load().dl_project_fwd_form(N, F, K, nhid, d, int(two_layer), ws_bytes, int(have_xplanes), out), "dl_project_fwd_form")
    return dict(zip(PROJECT_FWD_FORM, out))


def project_bwd_form(N: int, F: int, K: int, nhid: int, d: int, two_layer: bool, have_hid: bool, have_xplanes: bool = False) -> dict:
    """Which kernels the first node block of dl_project_bwd runs for this problem (dl_project_bwd_form)."""
    out = (C.c_int * len(PROJECT_BWD_FORM))()
    check(load().dl_project_bwd_form(N, F, K, nhid, d, int(two_layer), int(have_hid), int(have_xplanes), out), "dl_project_bwd_form")
    return dict(zip(PROJECT_BWD_FORM, out))


PROJECT_SPARSE_FORM = ("chunks", "last_chunk_cols", "affine", "max_segments", "seg_len", "two_layer", "width", "vec",
                       "sA", "g_ranges")


def project_sparse_form(N: int, F: int, K: int, nhid: int, d: int, two_layer: bool, affine: bool, max_col_len: int) -> dict:
    """The launch decisions of dl_project_sparse_fwd / _bwd for this problem (dl_project_sparse_form)."""
    out = (C.c_int * len(PROJECT_SPARSE_FORM))()
    check(load().dl_project_sparse_form(N, F, K, nhid, d, int(two_layer), int(affine), max_col_len, out), "dl_project_sparse_form")
    return dict(zip(PROJECT_SPARSE_FORM, out))


SCORE_ALLPAIRS_FWD_FORM = ("kernel", "items", "grid", "n_slices", "slice_w", "chunks_per_u")
SCORE_ALLPAIRS_KERNELS = ("generic", "per shape", "matrix cores, split on stage", "matrix cores, from planes")
SCORE_ALLPAIRS_BWD_DENSE_FORM = ("Np", "NCB", "nslice", "min_tiles", "max_tiles")
SCORE_TOPK_FORM = ("nd", "qtiles", "slices", "tiles_per_slice", "last_tiles", "cap")
SCORE_MINE_FORM = ("nd", "tiles", "pairs", "pairs_per_wg", "grid", "max_scans", "scans_offset")


def score_allpairs_fwd_form(N: int, K: int, d: int, dtype: int, ws_bytes: int) -> dict:
    """Which kernel and launch geometry dl_score_allpairs_fwd takes for this problem (dl_score_allpairs_fwd_form)."""
    out = (C.c_int * len(SCORE_ALLPAIRS_FWD_FORM))()
    check(load().dl_score_allpairs_fwd_form(N, K, d, dtype, ws_bytes, out), "dl_score_allpairs_fwd_form")
    return dict(zip(SCORE_ALLPAIRS_FWD_FORM, out))


def score_allpairs_bwd_dense_form(N: int, K: int, d: int) -> dict:
    """The launch form of dl_score_allpairs_bwd_dense for this problem (dl_score_allpairs_bwd_dense_form)."""
    out = (C.c_int * len(SCORE_ALLPAIRS_BWD_DENSE_FORM))()
    check(load().dl_score_allpairs_bwd_dense_form(N, K, d, out), "dl_score_allpairs_bwd_dense_form")
    return dict(zip(SCORE_ALLPAIRS_BWD_DENSE_FORM, out))


SCORE_RECON_FORM = ("Np", "strips", "block_rows", "nslice")


def score_recon_form(N: int, K: int, d: int, block_rows: int = 0, dtype: int = DL_F32) -> dict:
    """The strips of dl_score_recon for this problem (``block_rows`` = 0: the default height) and the slice count of its
    backward, which is the dense backward's for the whole N (dl_score_recon_form_dtype; the form is the same for both table
    types)."""
    out = (C.c_int * len(SCORE_RECON_FORM))()
    check(load().dl_score_recon_form_dtype(N, K, d, dtype, block_rows, out), "dl_score_recon_form_dtype")
    return dict(zip(SCORE_RECON_FORM, out))


def score_topk_form(N: int, K: int, d: int, Q: int, k: int) -> dict:
    """The ranking scan's plan for this problem under the current DL_RANK_SLICES (dl_score_topk_form)."""
    out = (C.c_int * len(SCORE_TOPK_FORM))()
    check(load().dl_score_topk_form(N, K, d, Q, k, out), "dl_score_topk_form")
    return dict(zip(SCORE_TOPK_FORM, out))


def score_mine_form(N: int, K: int, d: int, m: int) -> dict:
    """The link-mining scan's plan for this problem under the current DL_MINE_TILES (dl_score_mine_form)."""
    out = (C.c_int * len(SCORE_MINE_FORM))()
    check(load().dl_score_mine_form(N, K, d, m, out), "dl_score_mine_form")
    return dict(zip(SCORE_MINE_FORM, out))


SCORE_PAIR_RANKS_FORM = ("nd", "tiles", "pairs", "pairs_per_wg", "grid", "separators", "targets_per_separator", "lds_levels",
                         "global_levels")


def score_pair_ranks_form(N: int, K: int, d: int, T: int) -> dict:
    """The counting scan's plan for this problem under the current DL_MINE_TILES (dl_score_pair_ranks_form)."""
    out = (C.c_int * len(SCORE_PAIR_RANKS_FORM))()
    check(load().dl_score_pair_ranks_form(N, K, d, T, out), "dl_score_pair_ranks_form")
    return dict(zip(SCORE_PAIR_RANKS_FORM, out))


SCORE_LINKS_FORM = ("nd", "tiles", "pairs", "pairs_per_wg", "grid", "scans", "cells")


def score_links_form(N: int, K: int, d: int) -> dict:
    """The link-graph scans' plan for this problem under the current DL_MINE_TILES (dl_score_links_form)."""
    out = (C.c_int * len(SCORE_LINKS_FORM))()
    check(load().dl_score_links_form(N, K, d, out), "dl_score_links_form")
    return dict(zip(SCORE_LINKS_FORM, out))


SCORE_LINKS_TOP_FORM = SCORE_LINKS_FORM + ("scans_offset",)


def score_links_top_form(N: int, K: int, d: int) -> dict:
    """The budgeted link graph's plan for this problem under the current DL_MINE_TILES (dl_score_links_top_form): the
    fields of ``score_links_form`` with ``scans`` = histogram scans at most + count + fill, and where in the aligned
    workspace the number of histogram scans that ran stands."""
    out = (C.c_int * len(SCORE_LINKS_TOP_FORM))()
    check(load().dl_score_links_top_form(N, K, d, out), "dl_score_links_top_form")
    return dict(zip(SCORE_LINKS_TOP_FORM, out))


SCORE_MINE_BETWEEN_FORM = ("nd", "tiles_a", "tiles_b", "pairs", "pairs_per_wg", "grid", "max_scans", "scans_offset")
SCORE_LINKS_BETWEEN_FORM = SCORE_MINE_BETWEEN_FORM[:6] + ("scans", "cells_a", "cells_b")


def score_mine_between_form(nA: int, nB: int, K: int, d: int, m: int) -> dict:
    """The plan of the rectangular mining scan under the current DL_MINE_TILES (dl_score_mine_between_form)."""
    out = (C.c_int * len(SCORE_MINE_BETWEEN_FORM))()
    check(load().dl_score_mine_between_form(nA, nB, K, d, m, out), "dl_score_mine_between_form")
    return dict(zip(SCORE_MINE_BETWEEN_FORM, out))


def score_links_between_form(nA: int, nB: int, K: int, d: int) -> dict:
    """The plan of the rectangular link-graph scans under the current DL_MINE_TILES (dl_score_links_between_form)."""
    out = (C.c_int * len(SCORE_LINKS_BETWEEN_FORM))()
    check(load().dl_score_links_between_form(nA, nB, K, d, out), "dl_score_links_between_form")
    return dict(zip(SCORE_LINKS_BETWEEN_FORM, out))


def config_reload() -> None:
    """Have the library read its environment switches again (it reads them once, at first use: csrc/dl_config.h).
    For tests and A/B scripts that change a DL_* variable inside a running process."""
    load().dl_config_reload()
