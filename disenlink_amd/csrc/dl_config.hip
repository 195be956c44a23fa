// The one place that reads the environment (dl_config.h).
#include <stdlib.h>
#include <algorithm>
#include <mutex>
#include "dl_config.h"
#include "disenlink_hip.h"

namespace dl {
namespace {

Config g_config;
std::once_flag g_once;

bool flag(const char* name) {                 // set and not "0" / "" ; the historical switches were "set = on"
    const char* e = getenv(name);
    return e != nullptr && e[0] != '\0' && !(e[0] == '0' && e[1] == '\0');
}
long long number(const char* name) {
    const char* e = getenv(name);
    return e != nullptr && e[0] != '\0' ? atoll(e) : 0;
}

void read_environment() {
    Config c;
    const char* sr = getenv("DL_STREAM_ROWS");
    c.stream_rows = (sr == nullptr || sr[0] == '\0') ? -1 : (sr[0] == '1' ? 1 : 0);
    c.fwd_group_kernel = flag("DL_FWD_GROUP_KERNEL");
    const char* fh = getenv("DL_FWD_HUB");
    c.fwd_hub = !(fh != nullptr && fh[0] == '0' && fh[1] == '\0');
    const char* rh = getenv("DL_ROUTE_HUB");
    c.route_hub = !(rh != nullptr && rh[0] == '0' && rh[1] == '\0');
    const char* hm = getenv("DL_SCORE_HUB_MIXED");
    c.score_hub_mixed = !(hm != nullptr && hm[0] == '0' && hm[1] == '\0');
    c.auc_target = (int)std::max(0LL, number("DL_AUC_TARGET"));
    c.project_fp32_mfma = getenv("DL_PROJECT_FP32_MFMA") != nullptr;
    c.fwd_groups = (int)std::max(0LL, number("DL_FWD_GROUPS"));
    c.fwd_block_rows = std::max(0LL, number("DL_FWD_BLOCK_ROWS"));
    c.bwd_block_bytes = std::max(0LL, number("DL_BWD_BLOCK_BYTES"));
    c.bwd_target = (int)std::max(0LL, number("DL_BWD_TARGET"));
    const char* ic = getenv("DL_INKERNEL_COMBINE");
    c.inkernel_combine = (ic == nullptr || ic[0] == '\0') ? 1 : std::max(0, std::min(2, atoi(ic)));
    c.rank_slices = (int)std::max(0LL, number("DL_RANK_SLICES"));
    c.mine_tiles = (int)std::max(0LL, std::min(1LL << 20, number("DL_MINE_TILES")));
    c.sparse_seg = (int)std::max(0LL, std::min(1LL << 20, number("DL_SPARSE_SEG")));
    g_config = c;
}

}  // namespace

const Config& config() {
    std::call_once(g_once, read_environment);
    return g_config;
}

void config_reload() {
    std::call_once(g_once, read_environment);
    read_environment();
}

}  // namespace dl

extern "C" void dl_config_reload(void) { dl::config_reload(); }
