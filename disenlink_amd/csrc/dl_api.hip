// C ABI of libdisenlink_hip.so: argument validation, workspace carving and dispatch.
#include <stdarg.h>
#include <string.h>
#include "dl_common.h"
#include "dl_kernels.h"

namespace dl {

static thread_local char g_err[512] = "";
static int g_force_generic = 0;

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return DL_E_LAUNCH;
    }
    return DL_OK;
}

static int check_shape(int K, int d) {
    DL_REQUIRE(K >= 1 && K <= DL_MAX_FACTORS, "K=%d outside 1..%d", K, DL_MAX_FACTORS);
    DL_REQUIRE(d >= 1 && d <= 4096, "d=%d outside 1..4096", d);
    return DL_OK;
}

static int check_plan(const dl_csr_plan* c, const char* what) {
    DL_REQUIRE(c != nullptr, "%s is NULL", what);
    DL_REQUIRE(c->n_rows >= 0 && c->n_entries >= 0 && c->row_offset >= 0, "%s: negative size", what);
    DL_REQUIRE((long long)c->row_offset + c->n_rows <= c->n_total, "%s: rows [%d, %d) exceed n_total=%d", what,
               c->row_offset, c->row_offset + c->n_rows, c->n_total);
    if (c->n_rows > 0) DL_REQUIRE(c->rowptr != nullptr, "%s.rowptr is NULL", what);
    if (c->n_entries > 0) DL_REQUIRE(c->col != nullptr, "%s.col is NULL", what);
    return DL_OK;
}

// What every kernel over a dl_pair_hub needs of it (dl_hub.h: 16-byte scalar loads); which entries it holds is the caller's to check.
static int check_hub(const dl_pair_hub* hp, const char* what, bool need_q2) {
    DL_REQUIRE(hp->n_slices >= 1 && hp->slice_max_item >= 1 && hp->n_blocks >= 1 && hp->n_steps >= 1, "%s: empty grid", what);
    DL_REQUIRE(hp->block_row && hp->slice_item0 && hp->item_block && hp->item_step && hp->step_v && hp->step_u && hp->step_q &&
               (hp->step_q2 || !need_q2), "%s: NULL array", what);
    DL_REQUIRE((((uintptr_t)hp->step_v | (uintptr_t)hp->step_u | (uintptr_t)hp->step_q | (uintptr_t)hp->step_q2) & 15) == 0,
               "%s: step_v, step_u, step_q and step_q2 must be 16-byte aligned", what);
    return DL_OK;
}


// Workspace layout (256-byte aligned blocks):
//   dw[E] | dwr[E] | ds[n_total*K] | vec_part[n_slots*K] | row_part[n_slots*2*K*d]
struct Workspace {
    float *dw, *dwr, *ds, *vec_part, *row_part;
    size_t bytes;
};

static Workspace carve(const dl_csr_plan* c, int K, int d, void* ws) {
    Workspace w;
    const size_t e = align256((size_t)c->n_entries * sizeof(float));
    const size_t nk = align256((size_t)c->n_total * K * sizeof(float));
    const size_t vp = align256((size_t)c->n_slots * K * sizeof(float));
    const size_t rp = align256((size_t)c->n_slots * 2 * K * d * sizeof(float));
    char* base = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    w.dw = (float*)base;
    w.dwr = (float*)(base + e);
    w.ds = (float*)(base + 2 * e);
    w.vec_part = (float*)(base + 2 * e + nk);
    w.row_part = (float*)(base + 2 * e + nk + vp);
    w.bytes = 2 * e + nk + vp + rp + 256;
    return w;
}

static int check_workspace(const dl_csr_plan* c, int K, int d, void* ws, size_t ws_bytes, Workspace* out) {
    *out = carve(c, K, d, ws);
    if (!ws || ws_bytes < out->bytes) {
        set_error("workspace too small: have %zu, need %zu (dl_workspace_bytes)", ws ? ws_bytes : (size_t)0, out->bytes);
        return DL_E_WORKSPACE;
    }
    return DL_OK;
}

// A usable segment plan: the arrays are there and the position counts are whole workgroups (a workgroup reads the
// DL_UNIT_SEGS descriptors of its group unconditionally; plans of another layout take the generic kernels instead).
static bool has_seg_plan(const dl_csr_plan* c) {
    return c->seg_len > 0 && c->seg_len <= DL_WAVE && c->n_seg > 0 && c->seg_row && c->seg_beg && c->seg_end && c->seg_slot &&
           c->n_slices >= 1 && c->slice_seg0 && c->slice_max_seg > 0 &&
           c->n_seg % DL_UNIT_SEGS == 0 && c->slice_max_seg % DL_UNIT_SEGS == 0 &&
           (c->n_multi == 0 || (c->multi_row && c->multi_slot0));
}

static bool use_fast(const dl_csr_plan* c, int K, int d, int dtype) {
    return !g_force_generic && fast_supported(K, d, dtype) && has_seg_plan(c);
}

// which dense scorer serves (K, d, dtype): the one decision of dl_score_allpairs_fwd and dl_score_allpairs_fwd_form
enum AllpairsKernel { ALLPAIRS_GENERIC = 0, ALLPAIRS_PER_SHAPE = 1, ALLPAIRS_MFMA = 2 };
static AllpairsKernel allpairs_kernel(int K, int d, int dtype) {
    if (!g_force_generic && dtype == DL_F32 && dense_mfma_supported(d)) return ALLPAIRS_MFMA;      // Gram products on the matrix cores
    if (!g_force_generic && fast_supported(K, d, dtype)) return ALLPAIRS_PER_SHAPE;
    return ALLPAIRS_GENERIC;
}

// bf16 tables exist only on the tuned path
static int check_dtype(const dl_csr_plan* c, int K, int d, int dtype) {
    DL_REQUIRE(dtype == DL_F32 || dtype == DL_BF16, "unknown dtype %d", dtype);
    if (dtype == DL_BF16)
        DL_REQUIRE(c && use_fast(c, K, d, dtype),
                   "bf16 tables need a tuned kernel for K=%d d=%d and a segment plan (no generic bf16 path)", K, d);
    return DL_OK;
}

}  // namespace dl

using namespace dl;

extern "C" {

const char* dl_version(void) { return "disenlink_hip 0.8 (gfx950)"; }
const char* dl_last_error(void) { return g_err; }
int dl_has_fast_path(int K, int d) { return fast_supported(K, d, DL_F32) ? 1 : 0; }
int dl_has_fast_path_dtype(int K, int d, dl_dtype dtype) { return fast_supported(K, d, (int)dtype) ? 1 : 0; }

int dl_set_force_generic(int on) {
    int old = g_force_generic;
    if (on >= 0) g_force_generic = on ? 1 : 0;
    return old;
}

size_t dl_workspace_bytes(const dl_csr_plan* plan, int K, int d) {
    if (!plan || K < 1 || d < 1) return 0;
    return carve(plan, K, d, nullptr).bytes;
}

int dl_project_supported(int d) { return project_supported(d) ? 1 : 0; }

size_t dl_project_fwd_workspace_bytes(int N, int F, int K, int nhid, int d, int two_layer) {
    (void)F;
    if (N <= 0 || K < 1 || nhid < 1 || d < 1) return 0;
    return project_fwd_workspace_bytes(N, F, K, nhid, d, two_layer != 0);
}

int dl_project_fwd_form(int N, int F, int K, int nhid, int d, int two_layer, size_t ws_bytes, int have_xplanes, int* out) {
    DL_REQUIRE(out != nullptr && project_supported(d) && N >= 1 && F >= 1 && K >= 1 && nhid >= 1, "bad argument");
    project_fwd_form(N, F, K, two_layer ? nhid : 1, d, two_layer != 0, ws_bytes, have_xplanes != 0, out);
    return DL_OK;
}

int dl_project_bwd_form(int N, int F, int K, int nhid, int d, int two_layer, int have_hid, int have_xplanes, int* out) {
    DL_REQUIRE(out != nullptr && project_supported(d) && N >= 1 && F >= 1 && K >= 1 && nhid >= 1, "bad argument");
    project_bwd_form(N, F, K, two_layer ? nhid : 1, d, two_layer != 0, have_hid != 0, have_xplanes != 0, out);
    return DL_OK;
}

size_t dl_project_hidden_floats(int N, int K, int nhid) {
    if (N <= 0 || K < 1 || nhid < 1) return 0;
    return (size_t)K * nhid * (size_t)((N + 3) & ~3);
}

size_t dl_project_xplanes_bytes(int N, int F) { return (N > 0 && F > 0) ? project_xplanes_bytes(N, F) : 0; }

int dl_project_xplanes_build(const float* x, int N, int F, void* xplanes, size_t xplanes_bytes, void* stream) {
    DL_REQUIRE(N >= 0 && F >= 1, "bad size N=%d F=%d", N, F);
    if (N == 0) return DL_OK;
    DL_REQUIRE(x && xplanes && xplanes_bytes >= project_xplanes_bytes(N, F) && ((uintptr_t)xplanes & 15) == 0,
               "x planes buffer: %zu bytes given, %zu needed (dl_project_xplanes_bytes), 16-byte aligned", xplanes_bytes,
               project_xplanes_bytes(N, F));
    return project_xplanes_build(x, N, F, xplanes, (hipStream_t)stream);
}

int dl_project_fwd(const float* x, int N, int F, int K, int nhid, int d, const float* W1, const float* b1,
                   const float* W2, const float* b2, float* Z, float* hid_out, void* ws, size_t ws_bytes,
                   void* stream) {
    return dl_project_fwd_xp(x, N, F, K, nhid, d, W1, b1, W2, b2, Z, hid_out, ws, ws_bytes, nullptr, stream);
}

int dl_project_fwd_xp(const float* x, int N, int F, int K, int nhid, int d, const float* W1, const float* b1,
                      const float* W2, const float* b2, float* Z, float* hid_out, void* ws, size_t ws_bytes,
                      const void* xplanes, void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(project_supported(d), "projection kernel supports d in {32, 64, 128}, got %d", d);
    DL_REQUIRE(N >= 0 && F >= 1 && nhid >= 1, "bad size N=%d F=%d nhid=%d", N, F, nhid);
    DL_REQUIRE(K <= 65535, "K too large for the launch grid");
    DL_REQUIRE((W2 == nullptr) == (b2 == nullptr), "W2 and b2 must both be given (two-layer) or both NULL");
    if (N == 0) return DL_OK;
    DL_REQUIRE(x && W1 && b1 && Z, "NULL argument");
    DL_REQUIRE((long long)N * K * d < (1LL << 40) && (long long)128 * F < (1LL << 31), "projection sizes out of range");
    DL_REQUIRE(hid_out == nullptr || W2 != nullptr, "hid_out is for the two-layer form only");
    DL_REQUIRE(xplanes == nullptr || ((uintptr_t)xplanes & 15) == 0, "x planes must be 16-byte aligned");
    return project_fwd(x, N, F, K, nhid, d, W1, b1, W2, b2, Z, ws, ws_bytes, hid_out, (hipStream_t)stream,
                       W2 != nullptr ? xplanes : nullptr);
}

size_t dl_project_bwd_workspace_bytes(int N, int F, int K, int nhid, int d, int two_layer) {
    if (N <= 0 || F < 1 || K < 1 || nhid < 1 || d < 1) return 0;
    return project_bwd_workspace_bytes(N, F, K, two_layer ? nhid : 1, d, two_layer != 0);
}

int dl_project_bwd(const float* x, int N, int F, int K, int nhid, int d, const float* W1, const float* b1,
                   const float* W2, const float* dZ, const float* hid, float* dW1, float* db1, float* dW2, float* db2,
                   void* ws, size_t ws_bytes, void* stream) {
    return dl_project_bwd_xp(x, N, F, K, nhid, d, W1, b1, W2, dZ, hid, dW1, db1, dW2, db2, ws, ws_bytes, nullptr, stream);
}

int dl_project_bwd_xp(const float* x, int N, int F, int K, int nhid, int d, const float* W1, const float* b1,
                      const float* W2, const float* dZ, const float* hid, float* dW1, float* db1, float* dW2, float* db2,
                      void* ws, size_t ws_bytes, const void* xplanes, void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(project_supported(d), "projection kernel supports d in {32, 64, 128}, got %d", d);
    DL_REQUIRE(N >= 0 && F >= 1 && nhid >= 1, "bad size N=%d F=%d nhid=%d", N, F, nhid);
    DL_REQUIRE(K <= 4096, "K too large for the launch grid");
    const bool two = W2 != nullptr;
    DL_REQUIRE(dW1 && db1 && (!two || (dW2 && db2)), "NULL gradient output");
    if (N == 0) {                                              // no nodes: every gradient is zero
        hipStream_t st = (hipStream_t)stream;
        const size_t m = two ? (size_t)nhid : (size_t)d;
        hipError_t e = hipMemsetAsync(dW1, 0, sizeof(float) * K * m * F, st);
        if (e == hipSuccess) e = hipMemsetAsync(db1, 0, sizeof(float) * K * m, st);
        if (two && e == hipSuccess) e = hipMemsetAsync(dW2, 0, sizeof(float) * (size_t)K * d * nhid, st);
        if (two && e == hipSuccess) e = hipMemsetAsync(db2, 0, sizeof(float) * (size_t)K * d, st);
        DL_REQUIRE(e == hipSuccess, "hipMemsetAsync: %s", hipGetErrorString(e));
        return DL_OK;
    }
    DL_REQUIRE(x && W1 && b1 && dZ, "NULL argument");
    const size_t need = project_bwd_workspace_bytes(N, F, K, two ? nhid : 1, d, two);
    DL_REQUIRE(ws != nullptr && ws_bytes >= need, "workspace too small: %zu < %zu bytes (dl_project_bwd_workspace_bytes)",
               ws_bytes, need);
    DL_REQUIRE(hid == nullptr || two, "hid is for the two-layer form only");
    DL_REQUIRE(xplanes == nullptr || ((uintptr_t)xplanes & 15) == 0, "x planes must be 16-byte aligned");
    return project_bwd(x, N, F, K, two ? nhid : 1, d, W1, b1, W2, dZ, hid, dW1, db1, dW2, db2, ws, (hipStream_t)stream,
                       xplanes);
}

int dl_route_fwd(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float t, uint8_t* p, float* a,
                 float* s, void* ws, size_t ws_bytes, void* stream) {
    DL_REQUIRE(g != nullptr, "graph is NULL");
    const dl_csr_plan* c = &g->csr;
    if (int rc = check_plan(c, "graph")) return rc;
    if (int rc = check_shape(K, d)) return rc;
    if (int rc = check_dtype(c, K, d, dtype)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (c->n_rows == 0) return DL_OK;
    DL_REQUIRE(Z && s, "Z or s is NULL");
    if (c->n_entries > 0) DL_REQUIRE(p && a, "p or a is NULL");
    if (use_fast(c, K, d, dtype)) {
        Workspace w;
        if (int rc = check_workspace(c, K, d, ws, ws_bytes, &w)) return rc;
        // optional routing plan (XCD-sliced and / or upper-triangle with mirrored writes)
        const dl_csr_plan* rp = &g->route;
        const bool have = has_seg_plan(rp) && rp->n_rows == c->n_rows && rp->n_total == c->n_total &&
                          rp->row_offset == c->row_offset && rp->rowptr == c->rowptr && rp->col == c->col;
        const bool mirror = have && g->route_mirror != 0;
        if (mirror)
            DL_REQUIRE((g->rev != nullptr || c->n_entries == 0) && c->row_offset == 0 && c->n_rows == c->n_total,
                       "route_mirror needs rev and an unsharded plan");
        // optional hub plan over the mirrored entries (dl_graph.route_hub): the shapes with a hub form only, same bits
        const dl_pair_hub* hp = nullptr;
        if (g->route_hub != nullptr && mirror && config().route_hub && fast_route_hub_supported(K, d, dtype) &&
            g->route_hub->n_items > 0) {
            hp = g->route_hub;
            // the plan must stand for the whole routing plan: no residual, and one live slot per entry with col >= row —
            // (n_entries + self-loops) / 2 of them; the exact count is checked where the plan is bound (graph.py), here its range
            DL_REQUIRE(hp->rest.n_entries == 0 && 2LL * hp->n_entries >= c->n_entries && hp->n_entries <= c->n_entries,
                       "route_hub must hold each of the graph's entries with col >= row (%d entries in all) and no residual plan: "
                       "it holds %d + %d", c->n_entries, hp->n_entries, hp->rest.n_entries);
            if (int rc = check_hub(hp, "route_hub", true)) return rc;
        }
        return fast_route_fwd(c, have ? rp : nullptr, mirror, g->rev, hp, Z, K, d, dtype, t, p, a, s, w.vec_part,
                              (hipStream_t)stream);
    }
    return generic_route_fwd(c, (const float*)Z, K, d, t, p, a, s, (hipStream_t)stream);
}

int dl_aggregate_fwd(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta, const uint8_t* p,
                     const float* a, const float* s, void* H, void* ws, size_t ws_bytes, void* stream) {
    DL_REQUIRE(g != nullptr, "graph is NULL");
    const dl_csr_plan* c = &g->csr;
    if (int rc = check_plan(c, "graph")) return rc;
    if (int rc = check_shape(K, d)) return rc;
    if (int rc = check_dtype(c, K, d, dtype)) return rc;
    if (c->n_rows == 0) return DL_OK;
    DL_REQUIRE(Z && s && H, "Z, s or H is NULL");
    if (c->n_entries > 0) DL_REQUIRE(p && a, "p or a is NULL");
    if (use_fast(c, K, d, dtype)) {
        Workspace w;
        if (int rc = check_workspace(c, K, d, ws, ws_bytes, &w)) return rc;
        return fast_aggregate_fwd(c, Z, K, d, dtype, beta, p, a, s, H, w.row_part, (hipStream_t)stream);
    }
    return generic_aggregate_fwd(c, (const float*)Z, K, d, beta, p, a, s, (float*)H, (hipStream_t)stream);
}

// dl_score_pairs_fwd and dl_score_pairs_logits_fwd: one set of checks, one dispatch (logit: logits out, no stored terms)
static int score_pairs_fwd_space(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                                 const int32_t* pu, const int32_t* pv, int n_pairs, const dl_pair_incidence* by_u,
                                 float* prob, float* coef, bool logit, void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    if (int rc = check_dtype(by_u ? &by_u->csr : nullptr, K, d, dtype)) return rc;
    DL_REQUIRE(N >= 0 && n_pairs >= 0, "negative size");
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (n_pairs == 0) return DL_OK;
    DL_REQUIRE(Z && H && pu && pv && prob, "NULL argument");
    if (by_u) {
        if (int rc = check_plan(&by_u->csr, "by_u")) return rc;
        const int n_second = by_u->inc_pair2 ? by_u->n_second : 0;      // mirrored pairs folded into one entry
        DL_REQUIRE(n_second >= 0 && by_u->csr.n_entries + n_second == n_pairs && by_u->n_pairs == n_pairs && by_u->inc_pair,
                   "by_u must list each of the %d pairs exactly once", n_pairs);
        DL_REQUIRE(by_u->csr.n_total == N, "by_u.n_total=%d != N=%d", by_u->csr.n_total, N);
        if (by_u->hub_mixed != nullptr)
            DL_REQUIRE(by_u->hub_mixed->n_lists == DL_HUB_MIXED_LISTS, "by_u.hub_mixed: n_lists=%d, the kernels walk %d",
                       by_u->hub_mixed->n_lists, DL_HUB_MIXED_LISTS);
        // hub blocks + residual plan: the same entries, cut in two — as three lists per item (hub), as five (hub_mixed), or both
        const dl_pair_hub* const hubs[2] = {by_u->hub, by_u->hub_mixed ? &by_u->hub_mixed->hub : nullptr};
        const char* const names[2][2] = {{"by_u.hub", "by_u.hub.rest"}, {"by_u.hub_mixed", "by_u.hub_mixed.rest"}};
        for (int x = 0; x < 2; ++x) {
            const dl_pair_hub* hp = hubs[x];
            if (hp == nullptr) continue;
            DL_REQUIRE(hp->n_items >= 0 && hp->n_entries >= 0 && hp->rest.n_entries >= 0 &&
                       hp->n_entries + hp->rest.n_entries == by_u->csr.n_entries,
                       "%s must hold each of the plan's %d entries exactly once", names[x][0], by_u->csr.n_entries);
            if (int rc = hp->n_items > 0 ? check_hub(hp, names[x][0], by_u->inc_pair2 != nullptr) : DL_OK) return rc;
            if (hp->rest.n_entries > 0) {
                if (int rc = check_plan(&hp->rest, names[x][1])) return rc;
                DL_REQUIRE(hp->rest.n_total == N && hp->rest.seg_len == by_u->csr.seg_len && hp->rest_pair &&
                           (hp->rest_pair2 || !by_u->inc_pair2), "%s does not match by_u", names[x][1]);
            }
        }
        if (use_fast(&by_u->csr, K, d, dtype))
            return logit ? fast_score_pairs_logits_fwd(by_u, Z, H, K, d, dtype, t, prob, (hipStream_t)stream)
                         : fast_score_pairs_fwd(by_u, Z, H, K, d, dtype, t, prob, coef, (hipStream_t)stream);
    }
    DL_REQUIRE(coef == nullptr, "coef output needs the tuned scorer (a (K,d) with a fast path and a by_u plan)");
    if (logit)
        return generic_score_pairs_logits_fwd((const float*)Z, (const float*)H, K, d, t, pu, pv, n_pairs, prob,
                                              (hipStream_t)stream);
    return generic_score_pairs_fwd((const float*)Z, (const float*)H, K, d, t, pu, pv, n_pairs, prob,
                                   (hipStream_t)stream);
}

int dl_score_pairs_fwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                       const int32_t* pu, const int32_t* pv, int n_pairs, const dl_pair_incidence* by_u,
                       float* prob, float* coef, void* stream) {
    return score_pairs_fwd_space(Z, H, N, K, d, dtype, t, pu, pv, n_pairs, by_u, prob, coef, false, stream);
}

int dl_score_pairs_logits_fwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                              const int32_t* pu, const int32_t* pv, int n_pairs, const dl_pair_incidence* by_u,
                              float* logit, void* stream) {
    return score_pairs_fwd_space(Z, H, N, K, d, dtype, t, pu, pv, n_pairs, by_u, logit, nullptr, true, stream);
}

size_t dl_score_allpairs_workspace_bytes(int N, int K, int d, dl_dtype dtype) {
    if (N <= 0 || K < 1 || d < 1 || dtype != DL_F32 || g_force_generic) return 0;
    return dense_score_workspace_bytes(N, K, d);
}

int dl_score_allpairs_fwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, float* prob,
                          void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(dtype == DL_F32 || dtype == DL_BF16, "unknown dtype %d", dtype);
    DL_REQUIRE(N >= 0 && N <= 46340, "dense [N,N] scoring needs 0 <= N <= 46340, got %d", N);
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (N == 0) return DL_OK;
    DL_REQUIRE(Z && H && prob, "NULL argument");
    const AllpairsKernel which = allpairs_kernel(K, d, dtype);
    if (which == ALLPAIRS_MFMA)
        return dense_mfma_score_allpairs_fwd((const float*)Z, (const float*)H, N, K, d, t, prob, ws, ws_bytes,
                                             (hipStream_t)stream);
    if (which == ALLPAIRS_PER_SHAPE)
        return fast_score_allpairs_fwd(Z, H, N, K, d, dtype, t, prob, (hipStream_t)stream);
    DL_REQUIRE(dtype == DL_F32, "bf16 tables need a tuned kernel for K=%d d=%d", K, d);
    return generic_score_allpairs_fwd((const float*)Z, (const float*)H, N, K, d, t, prob, (hipStream_t)stream);
}

size_t dl_score_allpairs_logits_workspace_bytes(int N, int K, int d) {
    if (N <= 0 || N > 46340 || K < 1 || K > DL_MAX_FACTORS || d < 1) return 0;
    return dense_logits_workspace_bytes(N, K, d);
}

int dl_score_allpairs_logits_fwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, float* logit,
                                 void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(dtype == DL_F32, "the dense logits serve fp32 tables, got dtype %d", (int)dtype);
    DL_REQUIRE(N >= 0 && N <= 46340, "dense [N,N] scoring needs 0 <= N <= 46340, got %d", N);
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (N == 0) return DL_OK;
    DL_REQUIRE(Z && H && logit, "NULL argument");
    const size_t need = dense_logits_workspace_bytes(N, K, d);
    if (!ws || ws_bytes < need) {
        set_error("workspace too small: have %zu, need %zu (dl_score_allpairs_logits_workspace_bytes)", ws ? ws_bytes : (size_t)0,
                  need);
        return DL_E_WORKSPACE;
    }
    return dense_mfma_score_allpairs_logits_fwd((const float*)Z, (const float*)H, N, K, d, t, logit, ws, (hipStream_t)stream);
}

int dl_score_allpairs_fwd_form(int N, int K, int d, dl_dtype dtype, size_t ws_bytes, int* out) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(out != nullptr && (dtype == DL_F32 || dtype == DL_BF16) && N >= 1 && N <= 46340, "bad argument");
    for (int i = 0; i < DL_SCORE_ALLPAIRS_FWD_FORM_LEN; ++i) out[i] = 0;
    const AllpairsKernel which = allpairs_kernel(K, d, dtype);
    DL_REQUIRE(which != ALLPAIRS_GENERIC || dtype == DL_F32, "bf16 tables need a tuned kernel for K=%d d=%d", K, d);
    out[0] = (int)which;
    if (which == ALLPAIRS_MFMA) dense_mfma_form(N, K, d, ws_bytes, out);
    else if (which == ALLPAIRS_PER_SHAPE) fast_score_allpairs_form(N, K, d, dtype, out);
    else generic_score_allpairs_form(N, out);
    return DL_OK;
}

int dl_score_topk_supported(int K, int d) { return score_rank_supported(K, d) ? 1 : 0; }

int dl_score_topk_form(int N, int K, int d, int n_queries, int k, int* out) {
    DL_REQUIRE(out != nullptr && N >= 1 && n_queries >= 1 && k >= 0 && k <= 128 && score_rank_supported(K, d), "bad argument");
    score_topk_form(N, d, n_queries, k, out);
    return DL_OK;
}

static bool known_dtype(dl_dtype dtype) { return dtype == DL_F32 || dtype == DL_BF16; }

// every scan of the family serves the same (K, d), with fp32 tables (three planes, six products) and with bf16 tables (one)
int dl_score_scan_supported(int K, int d, dl_dtype dtype) { return known_dtype(dtype) && score_rank_supported(K, d) ? 1 : 0; }

size_t dl_score_topk_workspace_bytes(int N, int K, int d, int n_queries, int k, int n_targets) {
    return dl_score_topk_workspace_bytes_dtype(N, K, d, DL_F32, n_queries, k, n_targets);
}

size_t dl_score_topk_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype, int n_queries, int k, int n_targets) {
    if (N <= 0 || n_queries <= 0 || k < 0 || n_targets < 0 || !score_rank_supported(K, d) || !known_dtype(dtype)) return 0;
    return score_rank_workspace_bytes(N, K, d, n_queries, k, n_targets, dtype);
}

// a node-group rule (NULL = none): host-side checks only, the arrays are device memory
static int check_filter(const dl_node_filter* f) {
    if (f == nullptr) return DL_OK;
    DL_REQUIRE(f->n_groups >= 1 && f->n_groups <= 64, "node filter: n_groups=%d outside 1..64", f->n_groups);
    DL_REQUIRE(f->group != nullptr && f->allow != nullptr, "node filter: NULL group or allow array");
    return DL_OK;
}

// ---- the all-pairs scans (dl_score_rank.hip, dl_score_mine.hip): one checklist, and what differs between the families
enum ScanFlags : unsigned {
    OWN_N = 1,          // the entry reports the range of N itself, with its own text
    CAP_ELEMS = 2,      // N K d < 2^40
    EX_TOGETHER = 4,    // exclusion rowptr and col go together (else: col follows rowptr)
    WS_CODE = 8,        // a small workspace is DL_E_WORKSPACE (else DL_E_ARG, in the ranking entries' words)
};
struct ScanSpec {
    const char* serves;                        // who refuses an unsupported (K, d)
    int n_min, n_max;  const char* n_why;      // range of N and its reason
    unsigned flags;
};
static const ScanSpec RANK_SCAN = {"the ranking scan serves", 1, 2147483647, "", OWN_N};
static const ScanSpec MINE_SCAN = {"the link-mining scan serves", 0, 46340, "the pair index u N + v must fit 31 bits",
                                   EX_TOGETHER | WS_CODE};
static const ScanSpec LINKS_SCAN = {"the link-graph scan serves", 1, DL_SCORE_LINKS_MAX_N, "the tile-pair walk of dl_score_mine",
                                    EX_TOGETHER | WS_CODE};
// 128-row tiles whose pair count fits an int32: N <= 65,535 * 128
static const ScanSpec PAIR_SCAN = {"the pair scans serve", 1, DL_SCORE_PAIR_RANKS_MAX_N, "the tile-pair count must fit 31 bits",
                                   CAP_ELEMS | EX_TOGETHER | WS_CODE};
static_assert((DL_SCORE_PAIR_RANKS_MAX_N / 128LL) * (DL_SCORE_PAIR_RANKS_MAX_N / 128LL + 1) / 2 <= 2147483647LL &&
              DL_SCORE_PAIR_RANKS_MAX_N % 128 == 0, "65,535 tiles of 128 rows: 2,147,450,880 tile pairs");

static bool scan_shape_ok(const ScanSpec& s, int N, int K, int d) {      // the *_workspace_bytes entries: 0 where a call is refused
    return N >= s.n_min && N <= s.n_max && score_rank_supported(K, d) &&
           (!(s.flags & CAP_ELEMS) || (long long)N * K * d < (1LL << 40));
}
static int check_scan_shape(const ScanSpec& s, int N, int K, int d, dl_dtype dtype = DL_F32) {
    DL_REQUIRE(known_dtype(dtype), "unknown dtype %d", (int)dtype);
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(score_rank_supported(K, d), "%s fp32 tables with 1 <= d <= 128, got d=%d", s.serves, d);
    if (!(s.flags & OWN_N)) DL_REQUIRE(N >= s.n_min && N <= s.n_max, "N=%d outside %d..%d (%s)", N, s.n_min, s.n_max, s.n_why);
    if (s.flags & CAP_ELEMS) DL_REQUIRE((long long)N * K * d < (1LL << 40), "tables too large");
    return DL_OK;
}
// have_args: the entry's pointers are there.  Filter, t and ranges stay with the entry: their order decides what is reported.
static int check_scan_ptrs(const ScanSpec& s, bool have_args, const int32_t* ex_rowptr, const int32_t* ex_col) {
    DL_REQUIRE(have_args, "NULL argument");
    if (s.flags & EX_TOGETHER) DL_REQUIRE((ex_rowptr == nullptr) == (ex_col == nullptr), "exclusion rowptr and col go together");
    else DL_REQUIRE(ex_rowptr == nullptr || ex_col != nullptr, "exclusion rowptr without col");
    return DL_OK;
}
static int check_scan_ws(const ScanSpec& s, const void* ws, size_t ws_bytes, size_t need, const char* sizer) {
    if (ws != nullptr && ws_bytes >= need) return DL_OK;
    const size_t have = ws ? ws_bytes : (size_t)0;
    if (s.flags & WS_CODE) set_error("workspace too small: have %zu, need %zu (%s)", have, need, sizer);
    else set_error("workspace too small: %zu < %zu bytes (%s)", have, need, sizer);
    return (s.flags & WS_CODE) ? DL_E_WORKSPACE : DL_E_ARG;
}

static int check_rank_args(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* queries,
                           int n_queries, const int32_t* ex_rowptr, const int32_t* ex_col) {
    if (int rc = check_scan_shape(RANK_SCAN, N, K, d, dtype)) return rc;
    DL_REQUIRE(N >= 1 && n_queries >= 0, "bad size N=%d n_queries=%d", N, n_queries);
    DL_REQUIRE((long long)N * K * d < (1LL << 40), "tables too large");
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    return check_scan_ptrs(RANK_SCAN, n_queries == 0 || (Z && H && queries), ex_rowptr, ex_col);
}

int dl_score_topk(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* queries, int n_queries, int k,
                  const int32_t* ex_rowptr, const int32_t* ex_col, int exclude_self, int64_t* index, float* logit, float* prob,
                  void* ws, size_t ws_bytes, void* stream) {
    return dl_score_topk_filtered(Z, H, N, K, d, t, queries, n_queries, k, ex_rowptr, ex_col, exclude_self, index, logit, prob, ws,
                                  ws_bytes, stream, nullptr);
}

int dl_score_topk_filtered(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* queries, int n_queries,
                           int k, const int32_t* ex_rowptr, const int32_t* ex_col, int exclude_self, int64_t* index, float* logit,
                           float* prob, void* ws, size_t ws_bytes, void* stream, const dl_node_filter* filter) {
    return dl_score_topk_dtype(Z, H, N, K, d, DL_F32, t, queries, n_queries, k, ex_rowptr, ex_col, exclude_self, index, logit, prob,
                               ws, ws_bytes, stream, filter);
}

// The *_dtype entries are the implementations; the fp32 entries above and below call them with DL_F32.
int dl_score_topk_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* queries,
                        int n_queries, int k, const int32_t* ex_rowptr, const int32_t* ex_col, int exclude_self, int64_t* index,
                        float* logit, float* prob, void* ws, size_t ws_bytes, void* stream, const dl_node_filter* filter) {
    if (int rc = check_rank_args(Z, H, N, K, d, dtype, t, queries, n_queries, ex_rowptr, ex_col)) return rc;
    if (int rc = check_filter(filter)) return rc;
    DL_REQUIRE(k >= 1 && k <= 128, "k=%d outside 1..128", k);
    if (n_queries == 0) return DL_OK;
    DL_REQUIRE(index && logit && prob, "NULL output");
    const size_t need = score_rank_workspace_bytes(N, K, d, n_queries, k, 0, dtype);
    if (int rc = check_scan_ws(RANK_SCAN, ws, ws_bytes, need, "dl_score_topk_workspace_bytes")) return rc;
    return score_topk(Z, H, dtype, N, K, d, t, queries, n_queries, k, ex_rowptr, ex_col, exclude_self, index, logit, prob, ws,
                      (hipStream_t)stream, filter);
}

int dl_score_ranks(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* queries, int n_queries,
                   const int32_t* tptr, const int32_t* tdst, int n_targets, const int32_t* ex_rowptr, const int32_t* ex_col,
                   int64_t* greater, int64_t* ties, void* ws, size_t ws_bytes, void* stream) {
    return dl_score_ranks_filtered(Z, H, N, K, d, t, queries, n_queries, tptr, tdst, n_targets, ex_rowptr, ex_col, greater, ties,
                                   ws, ws_bytes, stream, nullptr);
}

int dl_score_ranks_filtered(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* queries, int n_queries,
                            const int32_t* tptr, const int32_t* tdst, int n_targets, const int32_t* ex_rowptr,
                            const int32_t* ex_col, int64_t* greater, int64_t* ties, void* ws, size_t ws_bytes, void* stream,
                            const dl_node_filter* filter) {
    return dl_score_ranks_dtype(Z, H, N, K, d, DL_F32, t, queries, n_queries, tptr, tdst, n_targets, ex_rowptr, ex_col, greater, ties,
                                ws, ws_bytes, stream, filter);
}

int dl_score_ranks_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* queries,
                         int n_queries, const int32_t* tptr, const int32_t* tdst, int n_targets, const int32_t* ex_rowptr,
                         const int32_t* ex_col, int64_t* greater, int64_t* ties, void* ws, size_t ws_bytes, void* stream,
                         const dl_node_filter* filter) {
    if (int rc = check_rank_args(Z, H, N, K, d, dtype, t, queries, n_queries, ex_rowptr, ex_col)) return rc;
    if (int rc = check_filter(filter)) return rc;
    DL_REQUIRE(n_targets >= 0, "negative size");
    if (n_queries == 0 || n_targets == 0) return DL_OK;
    DL_REQUIRE(tptr && tdst && greater && ties, "NULL argument");
    DL_REQUIRE((long long)n_targets + n_queries < (1LL << 31), "too many targets");
    const size_t need = score_rank_workspace_bytes(N, K, d, n_queries, 0, n_targets, dtype);
    if (int rc = check_scan_ws(RANK_SCAN, ws, ws_bytes, need, "dl_score_topk_workspace_bytes")) return rc;
    return score_ranks(Z, H, dtype, N, K, d, t, queries, n_queries, tptr, tdst, n_targets, ex_rowptr, ex_col, greater, ties, ws,
                       (hipStream_t)stream, filter);
}

int dl_score_mine_supported(int K, int d) { return score_mine_supported(K, d) ? 1 : 0; }

static int check_mine_shape(int N, int K, int d, int m, dl_dtype dtype = DL_F32) {
    if (int rc = check_scan_shape(MINE_SCAN, N, K, d, dtype)) return rc;
    DL_REQUIRE(m >= 1 && m <= 65536, "m=%d outside 1..65536", m);
    return DL_OK;
}

int dl_score_mine_form(int N, int K, int d, int m, int* out) {
    if (int rc = check_mine_shape(N, K, d, m)) return rc;
    DL_REQUIRE(out != nullptr, "out is NULL");
    score_mine_form(N, d, m, out);
    return DL_OK;
}

size_t dl_score_mine_workspace_bytes(int N, int K, int d, int m) { return dl_score_mine_workspace_bytes_dtype(N, K, d, DL_F32, m); }

size_t dl_score_mine_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype, int m) {
    if (!scan_shape_ok(MINE_SCAN, N, K, d) || !known_dtype(dtype) || m < 1 || m > 65536) return 0;
    return score_mine_workspace_bytes(N, K, d, m, dtype);
}

int dl_score_mine(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* ex_rowptr, const int32_t* ex_col,
                  float min_logit, int m, int32_t* src, int32_t* dst, float* logit, float* prob, int64_t* count, void* ws,
                  size_t ws_bytes, void* stream) {
    return dl_score_mine_filtered(Z, H, N, K, d, t, ex_rowptr, ex_col, min_logit, m, src, dst, logit, prob, count, ws, ws_bytes,
                                  stream, nullptr);
}

int dl_score_mine_filtered(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* ex_rowptr,
                           const int32_t* ex_col, float min_logit, int m, int32_t* src, int32_t* dst, float* logit, float* prob,
                           int64_t* count, void* ws, size_t ws_bytes, void* stream, const dl_node_filter* filter) {
    return dl_score_mine_dtype(Z, H, N, K, d, DL_F32, t, ex_rowptr, ex_col, min_logit, m, src, dst, logit, prob, count, ws, ws_bytes,
                               stream, filter);
}

int dl_score_mine_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                        const int32_t* ex_col, float min_logit, int m, int32_t* src, int32_t* dst, float* logit, float* prob,
                        int64_t* count, void* ws, size_t ws_bytes, void* stream, const dl_node_filter* filter) {
    if (int rc = check_mine_shape(N, K, d, m, dtype)) return rc;
    if (int rc = check_filter(filter)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (int rc = check_scan_ptrs(MINE_SCAN, N == 0 || (Z && H), ex_rowptr, ex_col)) return rc;
    DL_REQUIRE(src && dst && logit && prob && count, "NULL output");
    if (int rc = check_scan_ws(MINE_SCAN, ws, ws_bytes, score_mine_workspace_bytes(N, K, d, m, dtype), "dl_score_mine_workspace_bytes"))
        return rc;
    return score_mine(Z, H, dtype, N, K, d, t, ex_rowptr, ex_col, min_logit, m, src, dst, logit, prob, count, ws, (hipStream_t)stream,
                      filter);
}

int dl_score_links_supported(int K, int d) { return score_links_supported(K, d) ? 1 : 0; }

int dl_score_links_form(int N, int K, int d, int* out) {
    if (int rc = check_scan_shape(LINKS_SCAN, N, K, d)) return rc;
    DL_REQUIRE(out != nullptr, "out is NULL");
    score_links_form(N, d, out);
    return DL_OK;
}

size_t dl_score_links_workspace_bytes(int N, int K, int d) { return dl_score_links_workspace_bytes_dtype(N, K, d, DL_F32); }

size_t dl_score_links_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype) {
    return scan_shape_ok(LINKS_SCAN, N, K, d) && known_dtype(dtype) ? score_links_workspace_bytes(N, K, d, dtype) : 0;
}

// what the count and the fill call check alike
static int check_links_args(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                            const int32_t* ex_col, const dl_node_filter* filter, const void* ws, size_t ws_bytes,
                            const int64_t* rowptr) {
    if (int rc = check_scan_shape(LINKS_SCAN, N, K, d, dtype)) return rc;
    if (int rc = check_filter(filter)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (int rc = check_scan_ptrs(LINKS_SCAN, Z && H && rowptr, ex_rowptr, ex_col)) return rc;
    return check_scan_ws(LINKS_SCAN, ws, ws_bytes, score_links_workspace_bytes(N, K, d, dtype), "dl_score_links_workspace_bytes");
}

int dl_score_links_count(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* ex_rowptr,
                         const int32_t* ex_col, float min_logit, const dl_node_filter* filter, void* ws, size_t ws_bytes,
                         int64_t* rowptr, void* stream) {
    return dl_score_links_count_dtype(Z, H, N, K, d, DL_F32, t, ex_rowptr, ex_col, min_logit, filter, ws, ws_bytes, rowptr, stream);
}

int dl_score_links_count_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                               const int32_t* ex_col, float min_logit, const dl_node_filter* filter, void* ws, size_t ws_bytes,
                               int64_t* rowptr, void* stream) {
    if (int rc = check_links_args(Z, H, N, K, d, dtype, t, ex_rowptr, ex_col, filter, ws, ws_bytes, rowptr)) return rc;
    return score_links_count(Z, H, dtype, N, K, d, t, ex_rowptr, ex_col, min_logit, filter, ws, rowptr, (hipStream_t)stream);
}

int dl_score_links_fill(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* ex_rowptr,
                        const int32_t* ex_col, float min_logit, const dl_node_filter* filter, void* ws, size_t ws_bytes,
                        const int64_t* rowptr, int64_t nnz, int32_t* col, float* logit, float* prob, void* stream) {
    return dl_score_links_fill_dtype(Z, H, N, K, d, DL_F32, t, ex_rowptr, ex_col, min_logit, filter, ws, ws_bytes, rowptr, nnz, col,
                                     logit, prob, stream);
}

int dl_score_links_fill_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                              const int32_t* ex_col, float min_logit, const dl_node_filter* filter, void* ws, size_t ws_bytes,
                              const int64_t* rowptr, int64_t nnz, int32_t* col, float* logit, float* prob, void* stream) {
    if (int rc = check_links_args(Z, H, N, K, d, dtype, t, ex_rowptr, ex_col, filter, ws, ws_bytes, rowptr)) return rc;
    DL_REQUIRE(nnz >= 0, "nnz=%lld is negative", (long long)nnz);
    DL_REQUIRE(nnz == 0 || (col && logit), "NULL output");
    return score_links_fill(dtype, N, K, d, t, ex_rowptr, ex_col, min_logit, filter, ws, rowptr, (long long)nnz, col, logit, prob,
                            (hipStream_t)stream);
}

// ---- the budgeted link graph: the links entries' checklist, and m
int dl_score_links_top_form(int N, int K, int d, int* out) {
    if (int rc = check_scan_shape(LINKS_SCAN, N, K, d)) return rc;
    DL_REQUIRE(out != nullptr, "out is NULL");
    score_links_top_form(N, d, out);
    return DL_OK;
}

size_t dl_score_links_top_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype) {
    return scan_shape_ok(LINKS_SCAN, N, K, d) && known_dtype(dtype) ? score_links_top_workspace_bytes(N, K, d, dtype) : 0;
}

static int check_links_top_args(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                                const int32_t* ex_col, int64_t m, const dl_node_filter* filter, const void* ws, size_t ws_bytes,
                                const int64_t* rowptr) {
    if (int rc = check_scan_shape(LINKS_SCAN, N, K, d, dtype)) return rc;
    if (int rc = check_filter(filter)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    DL_REQUIRE(m >= 1, "m=%lld below 1", (long long)m);
    if (int rc = check_scan_ptrs(LINKS_SCAN, Z && H && rowptr, ex_rowptr, ex_col)) return rc;
    return check_scan_ws(LINKS_SCAN, ws, ws_bytes, score_links_top_workspace_bytes(N, K, d, dtype),
                         "dl_score_links_top_workspace_bytes_dtype");
}

int dl_score_links_top_count_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                                   const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit, int64_t m,
                                   const dl_node_filter* filter, void* ws, size_t ws_bytes, int64_t* rowptr, void* stream) {
    if (int rc = check_links_top_args(Z, H, N, K, d, dtype, t, ex_rowptr, ex_col, m, filter, ws, ws_bytes, rowptr)) return rc;
    return score_links_top_count(Z, H, dtype, N, K, d, t, ex_rowptr, ex_col, min_logit, (long long)m, filter, ws, rowptr,
                                 (hipStream_t)stream);
}

int dl_score_links_top_fill_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                                  const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit, int64_t m,
                                  const dl_node_filter* filter, void* ws, size_t ws_bytes, const int64_t* rowptr, int64_t nnz,
                                  int32_t* col, float* logit, float* prob, void* stream) {
    if (int rc = check_links_top_args(Z, H, N, K, d, dtype, t, ex_rowptr, ex_col, m, filter, ws, ws_bytes, rowptr)) return rc;
    DL_REQUIRE(nnz >= 0, "nnz=%lld is negative", (long long)nnz);
    DL_REQUIRE(nnz == 0 || (col && logit), "NULL output");
    return score_links_top_fill(dtype, N, K, d, t, ex_rowptr, ex_col, min_logit, filter, ws, rowptr, (long long)nnz, col, logit, prob,
                                (hipStream_t)stream);
}

// ---- the scans between two node sets: the checklist of the mining / links entries on (nA, nB), and the two-sided rule
static const ScanSpec BETWEEN_SCAN = {"the scans between two node sets serve", 1, DL_SCORE_BETWEEN_MAX_N,
                                      "the pair index a nB + b must fit 31 bits", OWN_N | EX_TOGETHER | WS_CODE};
static_assert((long long)DL_SCORE_BETWEEN_MAX_N * DL_SCORE_BETWEEN_MAX_N <= 2147483647LL, "the pair index and the candidate count");

static bool between_shape_ok(int nA, int nB, int K, int d, dl_dtype dtype) {
    return scan_shape_ok(BETWEEN_SCAN, nA, K, d) && scan_shape_ok(BETWEEN_SCAN, nB, K, d) && known_dtype(dtype);
}
static int check_between_shape(int nA, int nB, int K, int d, dl_dtype dtype) {
    if (int rc = check_scan_shape(BETWEEN_SCAN, nA, K, d, dtype)) return rc;
    DL_REQUIRE(nA >= 1 && nA <= DL_SCORE_BETWEEN_MAX_N, "nA=%d outside 1..%d (%s)", nA, DL_SCORE_BETWEEN_MAX_N, BETWEEN_SCAN.n_why);
    DL_REQUIRE(nB >= 1 && nB <= DL_SCORE_BETWEEN_MAX_N, "nB=%d outside 1..%d (%s)", nB, DL_SCORE_BETWEEN_MAX_N, BETWEEN_SCAN.n_why);
    return DL_OK;
}
static int check_filter_between(const dl_node_filter_between* f) {
    if (f == nullptr) return DL_OK;
    DL_REQUIRE(f->n_groups >= 1 && f->n_groups <= 64, "node filter: n_groups=%d outside 1..64", f->n_groups);
    DL_REQUIRE(f->group_a != nullptr && f->group_b != nullptr && f->allow != nullptr, "node filter: NULL group or allow array");
    return DL_OK;
}

int dl_score_mine_between_form(int nA, int nB, int K, int d, int m, int* out) {
    if (int rc = check_between_shape(nA, nB, K, d, DL_F32)) return rc;
    DL_REQUIRE(m >= 1 && m <= 65536, "m=%d outside 1..65536", m);
    DL_REQUIRE(out != nullptr, "out is NULL");
    score_mine_between_form(nA, nB, d, out);
    return DL_OK;
}

size_t dl_score_mine_between_workspace_bytes_dtype(int nA, int nB, int K, int d, dl_dtype dtype, int m) {
    if (!between_shape_ok(nA, nB, K, d, dtype) || m < 1 || m > 65536) return 0;
    return score_mine_between_workspace_bytes(nA, nB, K, d, m, dtype);
}

int dl_score_mine_between_dtype(const void* ZA, const void* HA, int nA, const void* ZB, const void* HB, int nB, int K, int d,
                                dl_dtype dtype, float t, const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit, int m,
                                int32_t* src, int32_t* dst, float* logit, float* prob, int64_t* count, void* ws, size_t ws_bytes,
                                void* stream, const dl_node_filter_between* filter) {
    if (int rc = check_between_shape(nA, nB, K, d, dtype)) return rc;
    DL_REQUIRE(m >= 1 && m <= 65536, "m=%d outside 1..65536", m);
    if (int rc = check_filter_between(filter)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (int rc = check_scan_ptrs(BETWEEN_SCAN, ZA && HA && ZB && HB, ex_rowptr, ex_col)) return rc;
    DL_REQUIRE(src && dst && logit && prob && count, "NULL output");
    if (int rc = check_scan_ws(BETWEEN_SCAN, ws, ws_bytes, score_mine_between_workspace_bytes(nA, nB, K, d, m, dtype),
                               "dl_score_mine_between_workspace_bytes_dtype"))
        return rc;
    return score_mine_between(ZA, HA, ZB, HB, dtype, nA, nB, K, d, t, ex_rowptr, ex_col, min_logit, m, src, dst, logit, prob, count, ws,
                              (hipStream_t)stream, filter);
}

int dl_score_links_between_form(int nA, int nB, int K, int d, int* out) {
    if (int rc = check_between_shape(nA, nB, K, d, DL_F32)) return rc;
    DL_REQUIRE(out != nullptr, "out is NULL");
    score_links_between_form(nA, nB, d, out);
    return DL_OK;
}

size_t dl_score_links_between_workspace_bytes_dtype(int nA, int nB, int K, int d, dl_dtype dtype) {
    return between_shape_ok(nA, nB, K, d, dtype) ? score_links_between_workspace_bytes(nA, nB, K, d, dtype) : 0;
}

// what the count and the fill call check alike
static int check_links_between_args(const void* ZA, const void* HA, int nA, const void* ZB, const void* HB, int nB, int K, int d,
                                    dl_dtype dtype, float t, const int32_t* ex_rowptr, const int32_t* ex_col,
                                    const dl_node_filter_between* filter, const void* ws, size_t ws_bytes, const int64_t* rowptr_a,
                                    const int64_t* rowptr_b) {
    if (int rc = check_between_shape(nA, nB, K, d, dtype)) return rc;
    if (int rc = check_filter_between(filter)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (int rc = check_scan_ptrs(BETWEEN_SCAN, ZA && HA && ZB && HB && rowptr_a && rowptr_b, ex_rowptr, ex_col)) return rc;
    return check_scan_ws(BETWEEN_SCAN, ws, ws_bytes, score_links_between_workspace_bytes(nA, nB, K, d, dtype),
                         "dl_score_links_between_workspace_bytes_dtype");
}

int dl_score_links_between_count_dtype(const void* ZA, const void* HA, int nA, const void* ZB, const void* HB, int nB, int K, int d,
                                       dl_dtype dtype, float t, const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit,
                                       const dl_node_filter_between* filter, void* ws, size_t ws_bytes, int64_t* rowptr_a,
                                       int64_t* rowptr_b, void* stream) {
    if (int rc = check_links_between_args(ZA, HA, nA, ZB, HB, nB, K, d, dtype, t, ex_rowptr, ex_col, filter, ws, ws_bytes, rowptr_a,
                                          rowptr_b))
        return rc;
    return score_links_between_count(ZA, HA, ZB, HB, dtype, nA, nB, K, d, t, ex_rowptr, ex_col, min_logit, filter, ws, rowptr_a,
                                     rowptr_b, (hipStream_t)stream);
}

int dl_score_links_between_fill_dtype(const void* ZA, const void* HA, int nA, const void* ZB, const void* HB, int nB, int K, int d,
                                      dl_dtype dtype, float t, const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit,
                                      const dl_node_filter_between* filter, void* ws, size_t ws_bytes, const int64_t* rowptr_a,
                                      const int64_t* rowptr_b, int64_t nnz_a, int32_t* col_a, float* logit_a, float* prob_a,
                                      int64_t nnz_b, int32_t* col_b, float* logit_b, float* prob_b, void* stream) {
    if (int rc = check_links_between_args(ZA, HA, nA, ZB, HB, nB, K, d, dtype, t, ex_rowptr, ex_col, filter, ws, ws_bytes, rowptr_a,
                                          rowptr_b))
        return rc;
    DL_REQUIRE(nnz_a >= 0 && nnz_b >= 0, "nnz=%lld is negative", (long long)(nnz_a < 0 ? nnz_a : nnz_b));
    DL_REQUIRE((nnz_a == 0 || (col_a && logit_a)) && (nnz_b == 0 || (col_b && logit_b)), "NULL output");
    DL_REQUIRE((prob_a == nullptr) == (prob_b == nullptr), "prob_a and prob_b go together");
    return score_links_between_fill(dtype, nA, nB, K, d, t, ex_rowptr, ex_col, min_logit, filter, ws, rowptr_a, rowptr_b,
                                    (long long)nnz_a, col_a, logit_a, prob_a, (long long)nnz_b, col_b, logit_b, prob_b,
                                    (hipStream_t)stream);
}

int dl_score_pair_ranks_supported(int K, int d) { return score_rank_supported(K, d) ? 1 : 0; }

int dl_score_pair_ranks_form(int N, int K, int d, int n_targets, int* out) {
    if (int rc = check_scan_shape(PAIR_SCAN, N, K, d)) return rc;
    DL_REQUIRE(out != nullptr && n_targets >= 0, "bad argument");
    score_pair_ranks_form(N, d, n_targets, out);
    return DL_OK;
}

size_t dl_score_pair_logits_workspace_bytes(int N, int K, int d) { return dl_score_pair_logits_workspace_bytes_dtype(N, K, d, DL_F32); }

size_t dl_score_pair_logits_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype) {
    return scan_shape_ok(PAIR_SCAN, N, K, d) && known_dtype(dtype) ? score_pair_logits_workspace_bytes(N, K, d, dtype) : 0;
}

size_t dl_score_pair_ranks_workspace_bytes(int N, int K, int d) { return dl_score_pair_ranks_workspace_bytes_dtype(N, K, d, DL_F32); }

size_t dl_score_pair_ranks_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype) {
    return scan_shape_ok(PAIR_SCAN, N, K, d) && known_dtype(dtype) ? score_pair_ranks_workspace_bytes(N, K, d, dtype) : 0;
}

int dl_score_pair_logits(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* a, const int32_t* b,
                         int n_pairs, float* logit, void* ws, size_t ws_bytes, void* stream) {
    return dl_score_pair_logits_dtype(Z, H, N, K, d, DL_F32, t, a, b, n_pairs, logit, ws, ws_bytes, stream);
}

// what the two scorers of given pairs check alike, up to their pointers (have_args; not looked at for n_pairs == 0, where
// the entry returns DL_OK after this).  What follows stays with the entry: the workspace, under its own sizer's name.
static int check_pair_args(int N, int K, int d, dl_dtype dtype, float t, int n_pairs, bool have_args) {
    if (int rc = check_scan_shape(PAIR_SCAN, N, K, d, dtype)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    DL_REQUIRE(n_pairs >= 0 && n_pairs <= (1 << 30), "n_pairs=%d outside 0..2^30", n_pairs);
    return n_pairs == 0 ? DL_OK : check_scan_ptrs(PAIR_SCAN, have_args, nullptr, nullptr);
}

int dl_score_pair_logits_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* a,
                               const int32_t* b, int n_pairs, float* logit, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_pair_args(N, K, d, dtype, t, n_pairs, Z && H && a && b && logit)) return rc;
    if (n_pairs == 0) return DL_OK;
    if (int rc = check_scan_ws(PAIR_SCAN, ws, ws_bytes, score_pair_logits_workspace_bytes(N, K, d, dtype),
                               "dl_score_pair_logits_workspace_bytes"))
        return rc;
    return score_pair_logits(Z, H, dtype, N, K, d, t, a, b, n_pairs, logit, ws, (hipStream_t)stream);
}

size_t dl_score_pair_terms_workspace_bytes(int N, int K, int d) { return dl_score_pair_terms_workspace_bytes_dtype(N, K, d, DL_F32); }

size_t dl_score_pair_terms_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype) {
    return dl_score_pair_logits_workspace_bytes_dtype(N, K, d, dtype);
}

int dl_score_pair_terms(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* a, const int32_t* b,
                        int n_pairs, float* e, float* q, float* cum, void* ws, size_t ws_bytes, void* stream) {
    return dl_score_pair_terms_dtype(Z, H, N, K, d, DL_F32, t, a, b, n_pairs, e, q, cum, ws, ws_bytes, stream);
}

// any of e, q, cum may be NULL, so none of them counts among the arguments; all three NULL is refused on its own
int dl_score_pair_terms_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* a,
                              const int32_t* b, int n_pairs, float* e, float* q, float* cum, void* ws, size_t ws_bytes,
                              void* stream) {
    if (int rc = check_pair_args(N, K, d, dtype, t, n_pairs, Z && H && a && b)) return rc;
    if (n_pairs == 0) return DL_OK;
    DL_REQUIRE(e || q || cum, "NULL output: e, q and cum are all NULL");
    if (int rc = check_scan_ws(PAIR_SCAN, ws, ws_bytes, score_pair_logits_workspace_bytes(N, K, d, dtype),
                               "dl_score_pair_terms_workspace_bytes"))
        return rc;
    return score_pair_terms(Z, H, dtype, N, K, d, t, a, b, n_pairs, e, q, cum, ws, (hipStream_t)stream);
}

int dl_score_pair_ranks(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* ex_rowptr,
                        const int32_t* ex_col, const uint32_t* target_order, int n_targets, unsigned long long* above,
                        unsigned long long* equal, unsigned long long* n_candidates, void* ws, size_t ws_bytes, void* stream) {
    return dl_score_pair_ranks_filtered(Z, H, N, K, d, t, ex_rowptr, ex_col, target_order, n_targets, above, equal, n_candidates,
                                        ws, ws_bytes, stream, nullptr);
}

int dl_score_pair_ranks_filtered(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* ex_rowptr,
                                 const int32_t* ex_col, const uint32_t* target_order, int n_targets, unsigned long long* above,
                                 unsigned long long* equal, unsigned long long* n_candidates, void* ws, size_t ws_bytes,
                                 void* stream, const dl_node_filter* filter) {
    return dl_score_pair_ranks_dtype(Z, H, N, K, d, DL_F32, t, ex_rowptr, ex_col, target_order, n_targets, above, equal, n_candidates,
                                     ws, ws_bytes, stream, filter);
}

int dl_score_pair_ranks_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                              const int32_t* ex_col, const uint32_t* target_order, int n_targets, unsigned long long* above,
                              unsigned long long* equal, unsigned long long* n_candidates, void* ws, size_t ws_bytes, void* stream,
                              const dl_node_filter* filter) {
    if (int rc = check_scan_shape(PAIR_SCAN, N, K, d, dtype)) return rc;
    if (int rc = check_filter(filter)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    DL_REQUIRE(n_targets >= 0 && n_targets <= (1 << 30), "n_targets=%d outside 0..2^30", n_targets);
    const bool have = Z && H && above && equal && n_candidates && (n_targets == 0 || target_order);
    if (int rc = check_scan_ptrs(PAIR_SCAN, have, ex_rowptr, ex_col)) return rc;
    const size_t need = score_pair_ranks_workspace_bytes(N, K, d, dtype);
    if (int rc = check_scan_ws(PAIR_SCAN, ws, ws_bytes, need, "dl_score_pair_ranks_workspace_bytes")) return rc;
    return score_pair_ranks(Z, H, dtype, N, K, d, t, ex_rowptr, ex_col, target_order, n_targets, above, equal, n_candidates, ws,
                            (hipStream_t)stream, filter);
}

int dl_auc_pair_counts_supported(int n_pos, int n_neg) {
    return n_pos >= 0 && n_neg >= 0 && auc_counts_supported(n_pos, n_neg) ? 1 : 0;
}

int dl_auc_pair_counts(const float* score, const int64_t* pos_idx, int n_pos, const int64_t* neg_idx, int n_neg,
                       unsigned long long* u2, void* stream) {
    DL_REQUIRE(n_pos >= 0 && n_neg >= 0, "negative size");
    DL_REQUIRE(u2 != nullptr, "u2 is NULL");
    DL_REQUIRE(auc_counts_supported(n_pos, n_neg), "n_pos * n_neg too large for the slice-and-search form (%d x %d)",
               n_pos, n_neg);
    if (n_pos > 0 && n_neg > 0) DL_REQUIRE(score && pos_idx && neg_idx, "NULL argument");
    return auc_pair_counts(score, pos_idx, n_pos, neg_idx, n_neg, u2, (hipStream_t)stream);
}

int dl_auc_pair_counts_add(const float* score, const int64_t* pos_idx, int n_pos, const int64_t* neg_idx, int n_neg,
                           unsigned long long* u2, void* stream) {
    DL_REQUIRE(n_pos >= 0 && n_neg >= 0, "negative size");
    DL_REQUIRE(u2 != nullptr, "u2 is NULL");
    DL_REQUIRE(auc_counts_supported(n_pos, n_neg), "n_pos * n_neg too large for the slice-and-search form (%d x %d)",
               n_pos, n_neg);
    if (n_pos > 0 && n_neg > 0) DL_REQUIRE(score && pos_idx && neg_idx, "NULL argument");
    return auc_pair_counts(score, pos_idx, n_pos, neg_idx, n_neg, u2, (hipStream_t)stream, /*clear=*/false);
}

int dl_auc_pair_counts_grid(int n_pos, int n_neg, int* grid) {
    DL_REQUIRE(n_pos >= 1 && n_neg >= 1, "both classes must be present (%d x %d)", n_pos, n_neg);
    DL_REQUIRE(grid != nullptr, "grid is NULL");
    DL_REQUIRE(auc_counts_supported(n_pos, n_neg), "n_pos * n_neg too large for the slice-and-search form (%d x %d)",
               n_pos, n_neg);
    const AucGrid g = auc_grid(n_pos, n_neg);
    grid[0] = g.small_is_pos; grid[1] = g.slices; grid[2] = g.chunks; grid[3] = g.per;
    return DL_OK;
}

size_t dl_epoch_state_bytes(void) { return epoch_state_bytes(); }

int dl_epoch_finish(int n_bufs, const float* const* params, float* const* best, const size_t* numel, const float* loss,
                    unsigned long long* u2, double denom2, void* state, double* hist, long long max_epochs,
                    long long patience, double* host_ring, int ring, void* stream) {
    DL_REQUIRE(n_bufs >= 0 && n_bufs <= DL_ADAM_MAX_BUFS, "n_bufs=%d outside 0..%d", n_bufs, DL_ADAM_MAX_BUFS);
    DL_REQUIRE(loss && u2 && state, "loss / u2 / state is NULL");
    DL_REQUIRE(max_epochs >= 0 && (max_epochs == 0 || hist != nullptr), "hist is NULL");
    DL_REQUIRE(patience >= 0, "negative patience");
    if (n_bufs > 0) DL_REQUIRE(params && best && numel, "NULL argument");
    for (int i = 0; i < n_bufs; ++i) DL_REQUIRE(numel[i] == 0 || (params[i] && best[i]), "buffer %d: NULL pointer", i);
    DL_REQUIRE(host_ring == nullptr || ring >= 1, "ring=%d", ring);
    return epoch_finish(n_bufs, params, best, numel, loss, u2, denom2, state, hist, max_epochs, patience, host_ring, ring,
                        (hipStream_t)stream);
}

int dl_pair_bce(const float* prob, const float* y, const float* w, int n_pairs, float* loss, float* g, void* ws,
                size_t ws_bytes, void* stream) {
    DL_REQUIRE(n_pairs >= 0, "negative size");
    DL_REQUIRE(loss != nullptr, "loss is NULL");
    DL_REQUIRE(ws != nullptr && ws_bytes >= 4096 + 256, "dl_pair_bce needs >= 4352 bytes of workspace");
    if (n_pairs > 0) DL_REQUIRE(prob && y && w && g, "NULL argument");
    float* partial = (float*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    return pair_bce(prob, y, w, n_pairs, loss, g, partial, (hipStream_t)stream);
}

int dl_pair_bce_logits(const float* logit, const float* y, const float* w, int n_pairs, float* loss, float* g, void* ws,
                       size_t ws_bytes, void* stream) {
    DL_REQUIRE(n_pairs >= 0, "negative size");
    DL_REQUIRE(loss != nullptr, "loss is NULL");
    DL_REQUIRE(ws != nullptr && ws_bytes >= 4096 + 256, "dl_pair_bce_logits needs >= 4352 bytes of workspace");
    if (n_pairs > 0) DL_REQUIRE(logit && y && w && g, "NULL argument");
    float* partial = (float*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    return pair_bce_logits(logit, y, w, n_pairs, loss, g, partial, (hipStream_t)stream);
}

int dl_adam_step(int n_bufs, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, const size_t* numel, float* state, double lr, double beta1, double beta2,
                 double eps, double weight_decay, void* stream) {
    DL_REQUIRE(n_bufs >= 0 && n_bufs <= DL_ADAM_MAX_BUFS, "n_bufs=%d outside 0..%d", n_bufs, DL_ADAM_MAX_BUFS);
    DL_REQUIRE(state != nullptr, "state is NULL");
    DL_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "bad Adam hyper-parameters");
    if (n_bufs > 0) DL_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel, "NULL argument");
    for (int i = 0; i < n_bufs; ++i)
        DL_REQUIRE(numel[i] == 0 || (params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i]), "buffer %d: NULL pointer", i);
    return adam_step(n_bufs, params, grads, exp_avg, exp_avg_sq, numel, state, lr, beta1, beta2, eps, weight_decay,
                     (hipStream_t)stream);
}

int dl_adam_step_at(int n_bufs, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const size_t* numel, float* state, long long step, double lr, double beta1,
                    double beta2, double eps, double weight_decay, void* stream) {
    DL_REQUIRE(n_bufs >= 0 && n_bufs <= DL_ADAM_MAX_BUFS, "n_bufs=%d outside 0..%d", n_bufs, DL_ADAM_MAX_BUFS);
    DL_REQUIRE(step >= 1 && step < (1ll << 24), "step=%lld outside 1..2^24-1", step);
    DL_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "bad Adam hyper-parameters");
    if (n_bufs > 0) DL_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel, "NULL argument");
    for (int i = 0; i < n_bufs; ++i)
        DL_REQUIRE(numel[i] == 0 || (params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i]), "buffer %d: NULL pointer", i);
    return adam_step(n_bufs, params, grads, exp_avg, exp_avg_sq, numel, state, lr, beta1, beta2, eps, weight_decay,
                     (hipStream_t)stream, step);
}

int dl_score_pairs_bwd(const void* Z, const void* H, int K, int d, dl_dtype dtype, float t,
                       const dl_pair_incidence* inc, const float* prob, const float* g_prob, const float* coef,
                       float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(inc != nullptr, "incidence is NULL");
    const dl_csr_plan* c = &inc->csr;
    if (int rc = check_plan(c, "incidence")) return rc;
    if (int rc = check_dtype(c, K, d, dtype)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (c->n_rows == 0) return DL_OK;
    DL_REQUIRE(Z && H && dZ && dH, "NULL argument");
    if (c->n_entries > 0) DL_REQUIRE(inc->inc_pair && prob && g_prob, "NULL pair argument");
    if (use_fast(c, K, d, dtype)) {
        Workspace w;
        if (int rc = check_workspace(c, K, d, ws, ws_bytes, &w)) return rc;
        return fast_score_pairs_bwd(inc, Z, H, K, d, dtype, t, prob, g_prob, coef, dZ, dH, w.row_part,
                                    (hipStream_t)stream);
    }
    return generic_score_pairs_bwd(inc, (const float*)Z, (const float*)H, K, d, t, prob, g_prob, dZ, dH,
                                   (hipStream_t)stream);
}

int dl_score_pairs_logits_bwd(const void* Z, const void* H, int K, int d, dl_dtype dtype, float t,
                              const dl_pair_incidence* inc, const float* g_logit, float* dZ, float* dH, void* ws,
                              size_t ws_bytes, void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(inc != nullptr, "incidence is NULL");
    const dl_csr_plan* c = &inc->csr;
    if (int rc = check_plan(c, "incidence")) return rc;
    if (int rc = check_dtype(c, K, d, dtype)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (c->n_rows == 0) return DL_OK;
    DL_REQUIRE(Z && H && dZ && dH, "NULL argument");
    if (c->n_entries > 0) DL_REQUIRE(inc->inc_pair && g_logit, "NULL pair argument");
    if (use_fast(c, K, d, dtype)) {
        Workspace w;
        if (int rc = check_workspace(c, K, d, ws, ws_bytes, &w)) return rc;
        return fast_score_pairs_logits_bwd(inc, Z, H, K, d, dtype, t, g_logit, dZ, dH, w.row_part, (hipStream_t)stream);
    }
    return generic_score_pairs_logits_bwd(inc, (const float*)Z, (const float*)H, K, d, t, g_logit, dZ, dH,
                                          (hipStream_t)stream);
}

int dl_score_allpairs_bwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                          const dl_pair_incidence* inc, const int32_t* pu, const int32_t* pv, int n_pairs,
                          const float* prob, const float* g_prob, float* dZ, float* dH, void* ws, size_t ws_bytes,
                          void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(inc != nullptr, "incidence is NULL");
    const dl_csr_plan* c = &inc->csr;
    if (int rc = check_plan(c, "incidence")) return rc;
    DL_REQUIRE(N >= 0 && N <= 46340, "dense [N,N] scoring needs 0 <= N <= 46340, got %d", N);
    DL_REQUIRE(c->n_total == N, "incidence.n_total=%d != N=%d", c->n_total, N);
    DL_REQUIRE(n_pairs >= 0 && inc->n_pairs == n_pairs && c->n_entries == 2 * (long long)n_pairs,
               "the incidence plan must list each of the %d pairs once per endpoint", n_pairs);
    if (n_pairs > 0) DL_REQUIRE(pu && pv && prob && g_prob, "NULL pair argument");
    // the gathered vectors use the per-entry scratch of the plan's workspace (2 x n_entries floats >= 2 x n_pairs)
    Workspace w;
    if (int rc = check_workspace(c, K, d, ws, ws_bytes, &w)) return rc;
    if (int rc = gather_dense_pairs(pu, pv, N, n_pairs, prob, g_prob, w.dw, w.dwr, (hipStream_t)stream)) return rc;
    return dl_score_pairs_bwd(Z, H, K, d, dtype, t, inc, w.dw, w.dwr, nullptr, dZ, dH, ws, ws_bytes, stream);
}

int dl_score_allpairs_bwd_dense_supported(int K, int d) {
    return K >= 1 && K <= DL_MAX_FACTORS && dense_bwd_supported(d) ? 1 : 0;
}

size_t dl_score_allpairs_bwd_dense_workspace_bytes(int N, int K, int d) {
    if (N <= 0 || N > 46340 || !dl_score_allpairs_bwd_dense_supported(K, d)) return 0;
    return dense_bwd_workspace_bytes(N, K, d);
}

int dl_score_allpairs_bwd_dense_form(int N, int K, int d, int* out) {
    DL_REQUIRE(out != nullptr && N >= 1 && N <= 46340 && dl_score_allpairs_bwd_dense_supported(K, d), "bad argument");
    dense_bwd_form(N, K, d, out);
    return DL_OK;
}

int dl_score_allpairs_bwd_dense(const float* Z, const float* H, int N, int K, int d, float t, const float* prob,
                                const float* g_prob, float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(dense_bwd_supported(d), "the dense backward serves fp32 tables with 1 <= d <= 128, got d=%d", d);
    DL_REQUIRE(N >= 0 && N <= 46340, "dense [N,N] scoring needs 0 <= N <= 46340, got %d", N);
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (N == 0) return DL_OK;
    DL_REQUIRE(Z && H && prob && g_prob && dZ && dH, "NULL argument");
    const size_t need = dense_bwd_workspace_bytes(N, K, d);
    if (!ws || ws_bytes < need) {
        set_error("workspace too small: have %zu, need %zu (dl_score_allpairs_bwd_dense_workspace_bytes)", ws ? ws_bytes : (size_t)0,
                  need);
        return DL_E_WORKSPACE;
    }
    return dense_bwd_score_allpairs(Z, H, N, K, d, t, prob, g_prob, dZ, dH, ws, (hipStream_t)stream);
}

int dl_score_allpairs_logits_bwd_dense(const float* Z, const float* H, int N, int K, int d, float t, const float* g_logit,
                                       float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(dense_bwd_supported(d), "the dense backward serves fp32 tables with 1 <= d <= 128, got d=%d", d);
    DL_REQUIRE(N >= 0 && N <= 46340, "dense [N,N] scoring needs 0 <= N <= 46340, got %d", N);
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (N == 0) return DL_OK;
    DL_REQUIRE(Z && H && g_logit && dZ && dH, "NULL argument");
    const size_t need = dense_bwd_workspace_bytes(N, K, d);
    if (!ws || ws_bytes < need) {
        set_error("workspace too small: have %zu, need %zu (dl_score_allpairs_bwd_dense_workspace_bytes)", ws ? ws_bytes : (size_t)0,
                  need);
        return DL_E_WORKSPACE;
    }
    return dense_bwd_score_allpairs(Z, H, N, K, d, t, nullptr, g_logit, dZ, dH, ws, (hipStream_t)stream);
}

int dl_score_recon_supported(int K, int d) { return K >= 1 && K <= DL_MAX_FACTORS && score_recon_supported(K, d) ? 1 : 0; }

// block_rows: 0 (the default) or a positive multiple of 128
static bool recon_shape_ok(int N, int K, int d, dl_dtype dtype, int block_rows) {
    return N >= 1 && N <= DL_SCORE_RECON_MAX_N && known_dtype(dtype) && dl_score_recon_supported(K, d) && block_rows >= 0 &&
           block_rows % 128 == 0;
}

int dl_score_recon_form(int N, int K, int d, int block_rows, int* out) { return dl_score_recon_form_dtype(N, K, d, DL_F32, block_rows, out); }

int dl_score_recon_form_dtype(int N, int K, int d, dl_dtype dtype, int block_rows, int* out) {
    DL_REQUIRE(out != nullptr && recon_shape_ok(N, K, d, dtype, block_rows), "bad argument");
    score_recon_form(N, K, d, dtype, block_rows, out);
    return DL_OK;
}

size_t dl_score_recon_workspace_bytes(int N, int K, int d, int block_rows) {
    return dl_score_recon_workspace_bytes_dtype(N, K, d, DL_F32, block_rows);
}

size_t dl_score_recon_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype, int block_rows) {
    return recon_shape_ok(N, K, d, dtype, block_rows) ? score_recon_workspace_bytes(N, K, d, dtype, block_rows) : 0;
}

int dl_score_recon(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* pos_rowptr, const int32_t* pos_col,
                   const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg, int block_rows, double* loss_out,
                   int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream) {
    return dl_score_recon_dtype(Z, H, N, K, d, DL_F32, t, pos_rowptr, pos_col, ign_rowptr, ign_col, w_pos, w_neg, block_rows, loss_out,
                                counts_out, dZ, dH, ws, ws_bytes, stream);
}

// dl_score_recon_dtype, dl_score_recon_logits and their _filtered forms: one set of checks, one driver
static int score_recon_space(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* pos_rowptr,
                             const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg,
                             int block_rows, bool logit, double* loss_out, int64_t* counts_out, float* dZ, float* dH, void* ws,
                             size_t ws_bytes, void* stream, const dl_node_filter* filter) {
    DL_REQUIRE(known_dtype(dtype), "unknown dtype %d", (int)dtype);
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(dl_score_recon_supported(K, d), "the reconstruction loss serves fp32 and bf16 tables with 1 <= d <= 128, got d=%d", d);
    DL_REQUIRE(N >= 1 && N <= DL_SCORE_RECON_MAX_N, "N=%d outside 1..%d", N, DL_SCORE_RECON_MAX_N);
    DL_REQUIRE(block_rows >= 0 && block_rows % 128 == 0, "block_rows=%d is neither 0 nor a positive multiple of 128", block_rows);
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    DL_REQUIRE(Z && H && pos_rowptr && pos_col && loss_out && counts_out && dZ && dH, "NULL argument");
    DL_REQUIRE((ign_rowptr == nullptr) == (ign_col == nullptr), "ign_rowptr and ign_col must both be given or both be NULL");
    if (int rc = check_filter(filter)) return rc;
    const size_t need = score_recon_workspace_bytes(N, K, d, dtype, block_rows);
    if (!ws || ws_bytes < need) {
        set_error("workspace too small: have %zu, need %zu (dl_score_recon_workspace_bytes%s)", ws ? ws_bytes : (size_t)0, need,
                  dtype == DL_F32 ? "" : "_dtype");
        return DL_E_WORKSPACE;
    }
    return score_recon(Z, H, N, K, d, dtype, t, pos_rowptr, pos_col, ign_rowptr, ign_col, w_pos, w_neg, block_rows, logit, loss_out,
                       counts_out, dZ, dH, ws, (hipStream_t)stream, filter);
}

int dl_score_recon_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* pos_rowptr,
                         const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg,
                         int block_rows, double* loss_out, int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes,
                         void* stream) {
    return dl_score_recon_filtered(Z, H, N, K, d, dtype, t, pos_rowptr, pos_col, ign_rowptr, ign_col, w_pos, w_neg, block_rows,
                                   loss_out, counts_out, dZ, dH, ws, ws_bytes, stream, nullptr);
}

int dl_score_recon_filtered(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* pos_rowptr,
                            const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg,
                            int block_rows, double* loss_out, int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes,
                            void* stream, const dl_node_filter* filter) {
    return score_recon_space(Z, H, N, K, d, dtype, t, pos_rowptr, pos_col, ign_rowptr, ign_col, w_pos, w_neg, block_rows, false,
                             loss_out, counts_out, dZ, dH, ws, ws_bytes, stream, filter);
}

int dl_score_recon_logits(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* pos_rowptr,
                          const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg,
                          int block_rows, double* loss_out, int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes,
                          void* stream) {
    return dl_score_recon_logits_filtered(Z, H, N, K, d, dtype, t, pos_rowptr, pos_col, ign_rowptr, ign_col, w_pos, w_neg, block_rows,
                                          loss_out, counts_out, dZ, dH, ws, ws_bytes, stream, nullptr);
}

int dl_score_recon_logits_filtered(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                                   const int32_t* pos_rowptr, const int32_t* pos_col, const int32_t* ign_rowptr,
                                   const int32_t* ign_col, float w_pos, float w_neg, int block_rows, double* loss_out,
                                   int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream,
                                   const dl_node_filter* filter) {
    return score_recon_space(Z, H, N, K, d, dtype, t, pos_rowptr, pos_col, ign_rowptr, ign_col, w_pos, w_neg, block_rows, true,
                             loss_out, counts_out, dZ, dH, ws, ws_bytes, stream, filter);
}

int dl_score_pairs_train_supported(const dl_pair_incidence* inc, int K, int d, dl_dtype dtype) {
    return inc != nullptr && use_fast(&inc->csr, K, d, dtype) ? 1 : 0;
}

// dl_score_pairs_train and dl_score_pairs_train_logits: one set of checks, one dispatch
static int score_pairs_train_space(const void* Z, const void* H, int K, int d, dl_dtype dtype, float t,
                                   const dl_pair_incidence* inc, const float* y, const float* w, float* prob, float* dZ,
                                   float* dH, void* ws, size_t ws_bytes, bool logit, void* stream) {
    const char* const entry = logit ? "dl_score_pairs_train_logits" : "dl_score_pairs_train";
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(inc != nullptr, "incidence is NULL");
    const dl_csr_plan* c = &inc->csr;
    if (int rc = check_plan(c, "incidence")) return rc;
    if (int rc = check_dtype(c, K, d, dtype)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    DL_REQUIRE(use_fast(c, K, d, dtype), "%s needs a tuned kernel for K=%d d=%d (%s_supported)", entry, K, d, entry);
    if (c->n_rows == 0) return DL_OK;
    DL_REQUIRE(Z && H && dZ && dH, "NULL argument");
    if (c->n_entries > 0) DL_REQUIRE(inc->inc_pair && y && w && prob, "NULL pair argument");
    Workspace wsp;
    if (int rc = check_workspace(c, K, d, ws, ws_bytes, &wsp)) return rc;
    if (logit) return fast_score_pairs_train_logits(inc, Z, H, K, d, dtype, t, y, w, prob, dZ, dH, wsp.row_part, (hipStream_t)stream);
    return fast_score_pairs_train(inc, Z, H, K, d, dtype, t, y, w, prob, dZ, dH, wsp.row_part, (hipStream_t)stream);
}

int dl_score_pairs_train(const void* Z, const void* H, int K, int d, dl_dtype dtype, float t,
                         const dl_pair_incidence* inc, const float* y, const float* w, float* prob, float* dZ,
                         float* dH, void* ws, size_t ws_bytes, void* stream) {
    return score_pairs_train_space(Z, H, K, d, dtype, t, inc, y, w, prob, dZ, dH, ws, ws_bytes, false, stream);
}

int dl_score_pairs_train_logits_supported(const dl_pair_incidence* inc, int K, int d, dl_dtype dtype) {
    return dl_score_pairs_train_supported(inc, K, d, dtype);
}

int dl_score_pairs_train_logits(const void* Z, const void* H, int K, int d, dl_dtype dtype, float t,
                                const dl_pair_incidence* inc, const float* y, const float* w, float* logit, float* dZ,
                                float* dH, void* ws, size_t ws_bytes, void* stream) {
    return score_pairs_train_space(Z, H, K, d, dtype, t, inc, y, w, logit, dZ, dH, ws, ws_bytes, true, stream);
}

int dl_route_aggregate_bwd_phase1(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta,
                                  const uint8_t* p, const float* a, const float* s, const float* dH, float* dw,
                                  float* dwr, float* ds, void* ws, size_t ws_bytes, void* stream) {
    DL_REQUIRE(g != nullptr, "graph is NULL");
    const dl_csr_plan* c = &g->csr;
    if (int rc = check_plan(c, "graph")) return rc;
    if (int rc = check_shape(K, d)) return rc;
    if (int rc = check_dtype(c, K, d, dtype)) return rc;
    if (c->n_rows == 0) return DL_OK;
    DL_REQUIRE(Z && s && dH && ds, "NULL argument");
    if (c->n_entries > 0) DL_REQUIRE(p && a && dw && dwr, "NULL per-edge argument");
    if (use_fast(c, K, d, dtype)) {
        Workspace w;
        if (int rc = check_workspace(c, K, d, ws, ws_bytes, &w)) return rc;
        return fast_bwd_phase1(c, Z, K, d, dtype, beta, p, a, s, dH, dw, dwr, ds, w.vec_part, (hipStream_t)stream);
    }
    return generic_bwd_phase1(c, (const float*)Z, K, d, beta, p, a, s, dH, dw, dwr, ds, (hipStream_t)stream);
}

static int bwd_phase2_impl(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta, float t,
                           const uint8_t* p, const float* a, const float* s, const float* dH, const float* dw,
                           const float* dwr, const float* ds, const float* dz_in, const float* scale, float* dZ, void* ws,
                           size_t ws_bytes, void* stream) {
    DL_REQUIRE(g != nullptr, "graph is NULL");
    const dl_csr_plan* c = &g->csr;
    if (int rc = check_plan(c, "graph")) return rc;
    if (int rc = check_shape(K, d)) return rc;
    if (int rc = check_dtype(c, K, d, dtype)) return rc;
    DL_REQUIRE(t != 0.0f, "temperature is 0");
    if (c->n_rows == 0) return DL_OK;
    DL_REQUIRE(Z && s && dH && ds && dZ, "NULL argument");
    if (c->n_entries > 0) DL_REQUIRE(p && a && dw && dwr, "NULL per-edge argument");
    if (use_fast(c, K, d, dtype)) {
        Workspace w;
        if (int rc = check_workspace(c, K, d, ws, ws_bytes, &w)) return rc;
        return fast_bwd_phase2(c, Z, K, d, dtype, beta, t, p, a, s, dH, dw, dwr, ds, dz_in, scale, dZ, w.row_part,
                               (hipStream_t)stream);
    }
    return generic_bwd_phase2(c, (const float*)Z, K, d, beta, t, p, a, s, dH, dw, dwr, ds, dz_in, scale, dZ,
                              (hipStream_t)stream);
}

int dl_route_aggregate_bwd_phase2(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta,
                                  float t, const uint8_t* p, const float* a, const float* s, const float* dH,
                                  const float* dw, const float* dwr, const float* ds, float* dZ, int accumulate,
                                  void* ws, size_t ws_bytes, void* stream) {
    return bwd_phase2_impl(g, Z, K, d, dtype, beta, t, p, a, s, dH, dw, dwr, ds, accumulate ? dZ : nullptr, nullptr, dZ,
                           ws, ws_bytes, stream);
}

static int bwd_both_impl(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta, float t,
                         const uint8_t* p, const float* a, const float* s, const float* dH, const float* dz_in,
                         const float* scale, float* dZ, void* ws, size_t ws_bytes, void* stream) {
    DL_REQUIRE(g != nullptr, "graph is NULL");
    const dl_csr_plan* c = &g->csr;
    if (int rc = check_plan(c, "graph")) return rc;
    if (int rc = check_shape(K, d)) return rc;
    DL_REQUIRE(c->row_offset == 0 && c->n_rows == c->n_total,
               "dl_route_aggregate_bwd needs an unsharded plan; call the two phases with an all-gather of ds between");
    Workspace w;
    if (int rc = check_workspace(c, K, d, ws, ws_bytes, &w)) return rc;
    if (int rc = dl_route_aggregate_bwd_phase1(g, Z, K, d, dtype, beta, p, a, s, dH, w.dw, w.dwr, w.ds, ws, ws_bytes,
                                               stream))
        return rc;
    return bwd_phase2_impl(g, Z, K, d, dtype, beta, t, p, a, s, dH, w.dw, w.dwr, w.ds, dz_in, scale, dZ, ws, ws_bytes,
                           stream);
}

int dl_route_aggregate_bwd(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta, float t,
                           const uint8_t* p, const float* a, const float* s, const float* dH, float* dZ,
                           int accumulate, void* ws, size_t ws_bytes, void* stream) {
    return bwd_both_impl(g, Z, K, d, dtype, beta, t, p, a, s, dH, accumulate ? dZ : nullptr, nullptr, dZ, ws, ws_bytes,
                         stream);
}

int dl_route_aggregate_bwd_scaled(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta, float t,
                                  const uint8_t* p, const float* a, const float* s, const float* dH, const float* dZ_in,
                                  const float* scale, float* dZ, void* ws, size_t ws_bytes, void* stream) {
    return bwd_both_impl(g, Z, K, d, dtype, beta, t, p, a, s, dH, dZ_in, scale, dZ, ws, ws_bytes, stream);
}

}  // extern "C"
