// Environment switches of the library, read ONCE (at the first call that needs one) into a static structure: no launch
// path calls getenv.  dl_config_reload() (C ABI) reads the environment again — tests and A/B scripts that flip a switch
// inside one process call it after changing the variable.  Every switch is a measurement / test knob: defaults are what
// ships (README.md lists the few a maintainer would set, tools/README.md the rest).
#pragma once

namespace dl {

struct Config {
    int stream_rows;            // DL_STREAM_ROWS: -1 = by table size (default), 0 / 1 = never / always stream the H rows
    bool fwd_group_kernel;      // DL_FWD_GROUP_KERNEL: group-per-entry forward scorer instead of the wave-per-entry one
    bool fwd_hub;               // DL_FWD_HUB: 0 = ignore a pair list's hub plan (dl_pair_hub) and walk the whole forward plan (default 1)
    bool route_hub;             // DL_ROUTE_HUB: 0 = ignore a graph's routing hub plan (dl_graph.route_hub) and walk the routing plan (default 1)
    bool score_hub_mixed;       // DL_SCORE_HUB_MIXED: 0 = ignore a pair list's mixed hub plan (dl_pair_incidence.hub_mixed) and walk `hub` (default 1)
    int auc_target;             // DL_AUC_TARGET: workgroups of the AUC count kernel (0 = default)
    bool project_fp32_mfma;     // DL_PROJECT_FP32_MFMA: plain fp32 MFMA projection instead of the three-plane products
    int fwd_groups;             // DL_FWD_GROUPS: hidden-chunk groups of the projection forward (0 = default)
    long long fwd_block_rows;   // DL_FWD_BLOCK_ROWS: x-plane node block, in tiles of 128 rows (0 = default; tests force blocking)
    long long bwd_block_bytes;  // DL_BWD_BLOCK_BYTES: cap of the per-block hidden gradient (0 = default; tests force blocking)
    int bwd_target;             // DL_BWD_TARGET: workgroups per launch of the projection backward (0 = default)
    int inkernel_combine;       // DL_INKERNEL_COMBINE: 0 = rows of several units always through the separate combine launch,
                                // 1 (default) = inside the launch where the plan's rows are few units long, 2 = wherever a kernel can
    int rank_slices;            // DL_RANK_SLICES: candidate slices of the ranking scan (0 = by the CU count; results do not depend on it)
    int mine_tiles;             // DL_MINE_TILES: tile pairs per workgroup of the link-mining scans (0 = by the CU count; results do not depend on it)
    int sparse_seg;             // DL_SPARSE_SEG: entries per column segment of the sparse projection's dW1 gather (0 = default; tests)
};

const Config& config();
void config_reload();

}  // namespace dl
