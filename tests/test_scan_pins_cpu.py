"""The host numbers of the all-pairs scans, pinned: the workspace sizes and the launch forms of dl_score_topk / dl_score_ranks,
dl_score_mine, dl_score_pair_ranks, dl_score_pair_logits and dl_score_links at four shapes, with Q, k, T and m at their smallest
and largest legal values.  The literals were recorded from the library as it stood BEFORE the scans' host scaffolding was
moved onto csrc/dl_scan.h (one workspace carver, one launch helper), under DL_RANK_SLICES=3 and DL_MINE_TILES=5 so that
nothing depends on a CU count: callers size their buffers by these entries, so a change of the block order, of the 256-byte
rounding or of the trailing slack shows here as a number, not as an overrun on the device."""
from disenlink_amd import _lib

# (N, K, d) -> what the entries returned; the order of the lists is that of the loops in _measure
PINNED = {(1, 1, 1): {'topk_ws': [100096, 100864, 100864, 38654804992, 100096, 100864, 100864, 38654804992],
                 'mine_ws': [58112, 582144],
                 'pair_ranks_ws': 49664,
                 'pair_logits_ws': 49408,
                 'links_ws': 49920,
                 'topk_form': [(1, 1, 1, 1, 1, 65), (1, 1, 1, 1, 1, 192), (1, 1, 1, 1, 1, 65), (1, 1, 1, 1, 1, 192)],
                 'mine_form': [(1, 1, 0, 1, 0, 0, 24), (1, 1, 0, 1, 0, 0, 24)],
                 'pair_ranks_form': [(1, 1, 0, 1, 0, 0, 1, 0, 0), (1, 1, 0, 1, 0, 4096, 262144, 13, 18)],
                 'links_form': (1, 1, 0, 1, 0, 0, 1)},
     (129, 2, 33): {'topk_ws': [592640, 594432, 592896, 38655297024, 990976, 1252864, 858112, 38655562240],
                    'mine_ws': [402176, 926208],
                    'pair_ranks_ws': 393728,
                    'pair_logits_ws': 393472,
                    'links_ws': 395520,
                    'topk_form': [(2, 1, 2, 1, 1, 65), (2, 1, 2, 1, 1, 192), (2, 2, 2, 1, 1, 65), (2, 2, 2, 1, 1, 192)],
                    'mine_form': [(2, 2, 3, 3, 1, 7, 24), (2, 2, 3, 3, 1, 7, 24)],
                    'pair_ranks_form': [(2, 2, 3, 3, 1, 0, 1, 0, 0), (2, 2, 3, 3, 1, 4096, 262144, 13, 18)],
                    'links_form': (2, 2, 3, 3, 1, 2, 258)},
     (300, 3, 128): {'topk_ws': [2364672, 2367488, 2364416, 38657068544, 4932864, 5847040, 4464896, 38659169024],
                     'mine_ws': [1778432, 2302464],
                     'pair_ranks_ws': 1769984,
                     'pair_logits_ws': 1769728,
                     'links_ws': 1774848,
                     'topk_form': [(4, 1, 3, 1, 1, 65), (4, 1, 3, 1, 1, 192), (4, 3, 3, 1, 1, 65), (4, 3, 3, 1, 1, 192)],
                     'mine_form': [(4, 3, 6, 5, 2, 7, 24), (4, 3, 6, 5, 2, 7, 24)],
                     'pair_ranks_form': [(4, 3, 6, 5, 2, 0, 1, 0, 0), (4, 3, 6, 5, 2, 4096, 262144, 13, 18)],
                     'links_form': (4, 3, 6, 5, 2, 2, 900)},
     (46340, 8, 64): {'topk_ws': [286267648, 286270464, 286267392, 38940971520, 833605376, 974849536, 761131008, 39415835136],
                      'mine_ws': [285483776, 286007808],
                      'pair_ranks_ws': 285475328,
                      'pair_logits_ws': 285475072,
                      'links_ws': 352946432,
                      'topk_form': [(2, 1, 3, 121, 121, 65), (2, 1, 3, 121, 121, 192), (2, 363, 3, 121, 121, 65),
                                    (2, 363, 3, 121, 121, 192)],
                      'mine_form': [(2, 363, 66066, 5, 13214, 7, 24), (2, 363, 66066, 5, 13214, 7, 24)],
                      'pair_ranks_form': [(2, 363, 66066, 5, 13214, 0, 1, 0, 0), (2, 363, 66066, 5, 13214, 4096, 262144, 13, 18)],
                      'links_form': (2, 363, 66066, 5, 13214, 2, 16821420)}}

T_MAX = 1 << 30


def _measure(N, K, d):
    lib = _lib.load()
    return {
        "topk_ws": [int(lib.dl_score_topk_workspace_bytes(N, K, d, Q, k, T)) for Q in (1, N)
                    for k, T in ((1, 0), (128, 0), (0, 1), (0, T_MAX))],
        "mine_ws": [int(lib.dl_score_mine_workspace_bytes(N, K, d, m)) for m in (1, 65536)],
        "pair_ranks_ws": int(lib.dl_score_pair_ranks_workspace_bytes(N, K, d)),
        "pair_logits_ws": int(lib.dl_score_pair_logits_workspace_bytes(N, K, d)),
        "links_ws": int(lib.dl_score_links_workspace_bytes(N, K, d)),
        "topk_form": [tuple(_lib.score_topk_form(N, K, d, Q, k).values()) for Q in (1, N) for k in (1, 128)],
        "mine_form": [tuple(_lib.score_mine_form(N, K, d, m).values()) for m in (1, 65536)],
        "pair_ranks_form": [tuple(_lib.score_pair_ranks_form(N, K, d, T).values()) for T in (0, T_MAX)],
        "links_form": tuple(_lib.score_links_form(N, K, d).values()),
    }


def test_workspace_sizes_and_forms_are_the_recorded_ones(lib_env):
    lib_env("DL_RANK_SLICES", 3)
    lib_env("DL_MINE_TILES", 5)
    for shape, want in PINNED.items():
        got = _measure(*shape)
        for name in want:
            assert got[name] == want[name], (shape, name, got[name], want[name])
