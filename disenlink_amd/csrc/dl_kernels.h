// Internal launch functions behind the C ABI (dl_api.hip dispatches between them).
#pragma once
#include <hip/hip_runtime.h>
#include "disenlink_hip.h"

namespace dl {

// generic: any K <= 64, any d (dl_generic.hip)
int generic_route_fwd(const dl_csr_plan* c, const float* Z, int K, int d, float t, uint8_t* p, float* a, float* s,
                      hipStream_t st);
int generic_aggregate_fwd(const dl_csr_plan* c, const float* Z, int K, int d, float beta, const uint8_t* p,
                          const float* a, const float* s, float* H, hipStream_t st);
int generic_score_pairs_fwd(const float* Z, const float* H, int K, int d, float t, const int32_t* pu,
                            const int32_t* pv, int P, float* prob, hipStream_t st);
int generic_score_pairs_bwd(const dl_pair_incidence* inc, const float* Z, const float* H, int K, int d, float t,
                            const float* prob, const float* g_prob, float* dZ, float* dH, hipStream_t st);
// ... in logit space: logits out; the backward from d loss / d logit
int generic_score_pairs_logits_fwd(const float* Z, const float* H, int K, int d, float t, const int32_t* pu,
                                   const int32_t* pv, int P, float* logit, hipStream_t st);
int generic_score_pairs_logits_bwd(const dl_pair_incidence* inc, const float* Z, const float* H, int K, int d, float t,
                                   const float* g_logit, float* dZ, float* dH, hipStream_t st);
int generic_bwd_phase1(const dl_csr_plan* c, const float* Z, int K, int d, float beta, const uint8_t* p,
                       const float* a, const float* s, const float* dH, float* dw, float* dwr, float* ds,
                       hipStream_t st);
int generic_bwd_phase2(const dl_csr_plan* c, const float* Z, int K, int d, float beta, float t, const uint8_t* p,
                       const float* a, const float* s, const float* dH, const float* dw, const float* dwr,
                       const float* ds, const float* dz_in, const float* scale, float* dZ, hipStream_t st);

// tuned, per-(K, D, table type) instantiations (dl_fast.hip)
bool fast_supported(int K, int d, int dtype);
// hub: the routing hub plan to walk instead of `route` (NULL = none; the caller has checked that the shape has a hub form)
int fast_route_fwd(const dl_csr_plan* g, const dl_csr_plan* route, bool mirror, const int32_t* rev, const dl_pair_hub* hub,
                   const void* Z, int K, int d, int dtype, float t, uint8_t* p, float* a, float* s, float* s_part,
                   hipStream_t st);
bool fast_route_hub_supported(int K, int d, int dtype);
int fast_aggregate_fwd(const dl_csr_plan* g, const void* Z, int K, int d, int dtype, float beta, const uint8_t* p,
                       const float* a, const float* s, void* H, float* h_part, hipStream_t st);
int fast_bwd_phase1(const dl_csr_plan* g, const void* Z, int K, int d, int dtype, float beta, const uint8_t* p,
                    const float* a, const float* s, const float* dH, float* dw, float* dwr, float* ds,
                    float* ds_part, hipStream_t st);
int fast_bwd_phase2(const dl_csr_plan* g, const void* Z, int K, int d, int dtype, float beta, float t,
                    const uint8_t* p, const float* a, const float* s, const float* dH, const float* dw,
                    const float* dwr, const float* ds, const float* dz_in, const float* scale, float* dZ, float* dz_part, hipStream_t st);
int fast_score_pairs_fwd(const dl_pair_incidence* by_u, const void* Z, const void* H, int K, int d, int dtype,
                         float t, float* prob, float* coef, hipStream_t st);
int fast_score_pairs_train(const dl_pair_incidence* inc, const void* Z, const void* H, int K, int d, int dtype, float t,
                           const float* y, const float* w, float* prob, float* dZ, float* dH, float* part, hipStream_t st);
int fast_score_pairs_bwd(const dl_pair_incidence* inc, const void* Z, const void* H, int K, int d, int dtype,
                         float t, const float* prob, const float* g_prob, const float* coef, float* dZ, float* dH,
                         float* part, hipStream_t st);
// the same three in logit space (the forward without stored terms, the one-pass step with gl = w (sigma(x) - y), the recompute backward)
int fast_score_pairs_logits_fwd(const dl_pair_incidence* by_u, const void* Z, const void* H, int K, int d, int dtype,
                                float t, float* logit, hipStream_t st);
int fast_score_pairs_train_logits(const dl_pair_incidence* inc, const void* Z, const void* H, int K, int d, int dtype, float t,
                                  const float* y, const float* w, float* logit, float* dZ, float* dH, float* part, hipStream_t st);
int fast_score_pairs_logits_bwd(const dl_pair_incidence* inc, const void* Z, const void* H, int K, int d, int dtype,
                                float t, const float* g_logit, float* dZ, float* dH, float* part, hipStream_t st);

// prob / g_prob of the dense [N][N] scorer at the listed pairs (dl_generic.hip)
int gather_dense_pairs(const int32_t* pu, const int32_t* pv, int N, int P, const float* prob, const float* g_prob,
                       float* prob_q, float* g_q, hipStream_t st);

int fast_score_allpairs_fwd(const void* Z, const void* H, int N, int K, int d, int dtype, float t, float* prob,
                            hipStream_t st);
int generic_score_allpairs_fwd(const float* Z, const float* H, int N, int K, int d, float t, float* prob,
                               hipStream_t st);

// the launch decisions of the three dense scorers, the dense backward and the ranking scan for a problem (host only;
// include/disenlink_hip.h lists the entries): each fills its part of the form from the code its launch calls
void generic_score_allpairs_form(int N, int* out);
void fast_score_allpairs_form(int N, int K, int d, int dtype, int* out);
void dense_mfma_form(int N, int K, int d, size_t ws_bytes, int* out);
void dense_bwd_form(int N, int K, int d, int* out);
void score_topk_form(int N, int d, int Q, int k, int* out);
void score_mine_form(int N, int d, int m, int* out);
void score_pair_ranks_form(int N, int d, int T, int* out);
void score_links_form(int N, int d, int* out);

// dense scorer on the matrix cores (dl_score_dense.hip): fp32 tables, d % 32 == 0
bool dense_mfma_supported(int d);
size_t dense_score_workspace_bytes(int N, int K, int d);
int dense_mfma_score_allpairs_fwd(const float* Z, const float* H, int N, int K, int d, float t, float* prob, void* ws, size_t ws_bytes,
                                  hipStream_t st);

// ... and the logits of the same pairs: the kernel from planes without its sigmoid, every d (the planes pad it), ws required
size_t dense_logits_workspace_bytes(int N, int K, int d);
int dense_mfma_score_allpairs_logits_fwd(const float* Z, const float* H, int N, int K, int d, float t, float* logit, void* ws,
                                         hipStream_t st);

// dense backward of the dense scorer on the matrix cores (dl_score_dense_bwd.hip): fp32 tables, 1 <= d <= 128
bool dense_bwd_supported(int d);
size_t dense_bwd_workspace_bytes(int N, int K, int d);
// (prob == NULL: g_prob is the gradient with respect to the logits)
int dense_bwd_score_allpairs(const float* Z, const float* H, int N, int K, int d, float t, const float* prob, const float* g_prob,
                             float* dZ, float* dH, void* ws, hipStream_t st);

// ... its stages on their own, for a G^ that arrives in strips of rows (dl_score_recon.hip): the transposed planes, the main
// kernel over the u tiles [ut0, ut0 + n_ut) with ghat = the Np-wide rows of G^ from row 128 ut0 on, and the sum of the v
// slices.  The v range is cut into dense_bwd_nslice(N, K) slices whatever the u range.
int dense_bwd_nslice(int N, int K);
size_t dense_bwd_part_floats(int N, int K, int d);
// dt = DL_BF16 (the reconstruction loss on bf16 tables): copy_cols for the transposed planes, one plane per array, and the
// one-plane form of the main kernel.
void dense_bwd_cols(const float* Z, const float* H, int N, int K, int d, __bf16* zT, __bf16* hT, hipStream_t st);
void copy_cols(const __bf16* Z, const __bf16* H, int N, int K, int d, __bf16* zT, __bf16* hT, hipStream_t st);
void dense_bwd_tiles(const __bf16* zp, const __bf16* hp, const __bf16* zT, const __bf16* hT, dl_dtype dt, const float* ghat, int N,
                     int K, int d, float t, int ut0, int n_ut, bool strip, float* part, float* dZ, float* dH, hipStream_t st);
void dense_bwd_combine(const float* part, int N, int K, int d, float* dZ, float* dH, hipStream_t st);

// whole-graph reconstruction loss and gradient by strips of rows (dl_score_recon.hip; its scan is the RECON mode of
// dl_score_rank.hip): fp32 or bf16 tables (dt), 1 <= d <= 128; the form does not depend on dt, the workspace does
bool score_recon_supported(int K, int d);
void score_recon_form(int N, int K, int d, dl_dtype dt, int block_rows, int* out);
size_t score_recon_workspace_bytes(int N, int K, int d, dl_dtype dt, int block_rows);
void score_recon_strip(const __bf16* cz, const __bf16* ch, dl_dtype dt, int N, int K, int d, float t, int q0, int rows,
                       const int32_t* pos_rowptr, const int32_t* pos_col, const int32_t* ig_rowptr, const int32_t* ig_col, float w_pos,
                       float w_neg, bool logit, const dl_node_filter* filter, float* ghat, float* lcell, unsigned* ccell, hipStream_t st);
// logit: loss term and gradient per pair in logit space (dl_score_recon_logits); everything but the scan's epilogue is shared
// filter (NULL: none; checked by the caller): a symmetric node-group rule, a pair it denies is ignored (dl_score_recon_filtered)
int score_recon(const void* Z, const void* H, int N, int K, int d, dl_dtype dt, float t, const int32_t* pos_rowptr,
                const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg, int block_rows,
                bool logit, double* loss, int64_t* counts, float* dZ, float* dH, void* ws, hipStream_t st,
                const dl_node_filter* filter = nullptr);

// ranking of all candidates of query rows on the matrix cores (dl_score_rank.hip): fp32 tables, 1 <= d <= 128
bool score_rank_supported(int K, int d);
// dt: the type of the tables Z and H, DL_F32 (three bf16 planes per operand, six products) or DL_BF16 (the table is its own
// plane, one product); the launch forms do not depend on it, the workspace does
size_t score_rank_workspace_bytes(int N, int K, int d, int Q, int k, int T, dl_dtype dt = DL_F32);
int score_topk(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* queries, int Q, int k,
               const int32_t* ex_rowptr, const int32_t* ex_col, int exclude_self, int64_t* index, float* logit, float* prob,
               void* ws, hipStream_t st, const dl_node_filter* filter = nullptr);       // filter: checked by the caller
int score_ranks(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* queries, int Q, const int32_t* tptr,
                const int32_t* tdst, int T, const int32_t* ex_rowptr, const int32_t* ex_col, int64_t* greater, int64_t* ties,
                void* ws, hipStream_t st, const dl_node_filter* filter = nullptr);

// global top-m of the logits of all unordered pairs on the matrix cores (dl_score_mine.hip): fp32 tables, 1 <= d <= 128
bool score_mine_supported(int K, int d);
size_t score_mine_workspace_bytes(int N, int K, int d, int m, dl_dtype dt = DL_F32);
int score_mine(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* ex_rowptr, const int32_t* ex_col,
               float min_logit, int m, int32_t* src, int32_t* dst, float* logit, float* prob, int64_t* count, void* ws,
               hipStream_t st, const dl_node_filter* filter = nullptr);

// logits of given (A row, B row) pairs with the bits of the scans (dl_score_rank.hip), and the global rank counts of sorted
// target keys among all unordered pairs (dl_score_mine.hip, one counting scan): fp32 tables, 1 <= d <= 128
size_t score_pair_logits_workspace_bytes(int N, int K, int d, dl_dtype dt = DL_F32);
int score_pair_logits(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* a, const int32_t* b, int T,
                      float* logit, void* ws, hipStream_t st);
// the per-factor terms of given pairs from the same pass (e, q, cum: [T][K] each, NULL = not wanted; not all NULL); the
// workspace is score_pair_logits_workspace_bytes
int score_pair_terms(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* a, const int32_t* b, int T,
                     float* e, float* q, float* cum, void* ws, hipStream_t st);
size_t score_pair_ranks_workspace_bytes(int N, int K, int d, dl_dtype dt = DL_F32);
int score_pair_ranks(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* ex_rowptr, const int32_t* ex_col,
                     const unsigned* tord, int T, unsigned long long* gcnt, unsigned long long* tcnt, unsigned long long* ncand,
                     void* ws, hipStream_t st, const dl_node_filter* filter = nullptr);

// every unordered pair whose logit reaches a floor, as a symmetric CSR (dl_score_mine.hip: a counting scan, the offsets, a
// filling scan over the workspace the count left): fp32 tables, 1 <= d <= 128, N <= 46,340
bool score_links_supported(int K, int d);
size_t score_links_workspace_bytes(int N, int K, int d, dl_dtype dt = DL_F32);
int score_links_count(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* ex_rowptr, const int32_t* ex_col,
                      float min_logit, const dl_node_filter* filter, void* ws, int64_t* rowptr, hipStream_t st);
int score_links_fill(dl_dtype dt, int N, int K, int d, float t, const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit,
                     const dl_node_filter* filter, void* ws, const int64_t* rowptr, long long nnz, int32_t* col, float* logit,
                     float* prob, hipStream_t st);

// rows of a table A against rows of a table B (dl_score_mine.hip, the RECT instantiations): the top m and the thresholded
// link graph of the nA x nB rectangle, 1 <= nA, nB <= 46,340; the rule has a group array per side (checked by the caller)
void score_mine_between_form(int nA, int nB, int d, int* out);
size_t score_mine_between_workspace_bytes(int nA, int nB, int K, int d, int m, dl_dtype dt);
int score_mine_between(const void* ZA, const void* HA, const void* ZB, const void* HB, dl_dtype dt, int nA, int nB, int K, int d, float t,
                       const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit, int m, int32_t* src, int32_t* dst, float* logit,
                       float* prob, int64_t* count, void* ws, hipStream_t st, const dl_node_filter_between* filter);
void score_links_between_form(int nA, int nB, int d, int* out);
size_t score_links_between_workspace_bytes(int nA, int nB, int K, int d, dl_dtype dt);
int score_links_between_count(const void* ZA, const void* HA, const void* ZB, const void* HB, dl_dtype dt, int nA, int nB, int K, int d,
                              float t, const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit,
                              const dl_node_filter_between* filter, void* ws, int64_t* rowptr_a, int64_t* rowptr_b, hipStream_t st);
int score_links_between_fill(dl_dtype dt, int nA, int nB, int K, int d, float t, const int32_t* ex_rowptr, const int32_t* ex_col,
                             float min_logit, const dl_node_filter_between* filter, void* ws, const int64_t* rowptr_a,
                             const int64_t* rowptr_b, long long nnz_a, int32_t* col_a, float* logit_a, float* prob_a, long long nnz_b,
                             int32_t* col_b, float* logit_b, float* prob_b, hipStream_t st);

// the m best unordered pairs, any m, as that CSR (dl_score_mine.hip: the select of score_mine, then the link scans under the
// threshold key it left in the workspace): the limits of score_links
void score_links_top_form(int N, int d, int* out);
size_t score_links_top_workspace_bytes(int N, int K, int d, dl_dtype dt = DL_F32);
int score_links_top_count(const void* Z, const void* H, dl_dtype dt, int N, int K, int d, float t, const int32_t* ex_rowptr,
                          const int32_t* ex_col, float min_logit, long long m, const dl_node_filter* filter, void* ws, int64_t* rowptr,
                          hipStream_t st);
int score_links_top_fill(dl_dtype dt, int N, int K, int d, float t, const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit,
                         const dl_node_filter* filter, void* ws, const int64_t* rowptr, long long nnz, int32_t* col, float* logit,
                         float* prob, hipStream_t st);

// tie-averaged AUC counts (dl_metrics.hip)
bool auc_counts_supported(int n_pos, int n_neg);           // the smaller class fits the LDS
int auc_pair_counts(const float* score, const int64_t* pos_idx, int n_pos, const int64_t* neg_idx, int n_neg,
                    unsigned long long* u2, hipStream_t st, bool clear = true);
struct AucGrid { int small_is_pos, slices, chunks, per; };  // grid = slices x chunks, `per` searched scores per chunk
AucGrid auc_grid(int n_pos, int n_neg);                     // both sizes >= 1

size_t epoch_state_bytes();
int epoch_finish(int n_bufs, const float* const* params, float* const* best, const size_t* numel, const float* loss,
                 unsigned long long* u2, double denom2, void* state, double* hist, long long max_epochs, long long patience,
                 double* host_ring, int ring, hipStream_t st);
int adam_step(int n_bufs, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
              const size_t* numel, float* state, double lr, double beta1, double beta2, double eps, double weight_decay,
              hipStream_t st, long long host_step = 0);

int pair_bce_logits(const float* logit, const float* y, const float* w, int n, float* loss, float* g, float* partial,
                    hipStream_t st);
int pair_bce(const float* prob, const float* y, const float* w, int n, float* loss, float* g, float* partial,
             hipStream_t st);

// factor projection on the matrix cores (dl_project.hip)
bool project_supported(int d);
size_t project_fwd_workspace_bytes(int N, int F, int K, int nhid, int d, bool two_layer);
bool split_products();   // layer-1 / dW1 products from three bf16 planes per operand (off: DL_PROJECT_FP32_MFMA=1)
int project_fwd(const float* x, int N, int F, int K, int nhid, int d, const float* W1, const float* b1,
                const float* W2, const float* b2, float* Z, void* ws, size_t ws_bytes, float* hid_out, hipStream_t st,
                const void* xplanes = nullptr);
// persistent bf16 planes of x and x^T (x is constant for a run): built once, handed to project_fwd / project_bwd
size_t project_xplanes_bytes(int N, int F);
const void* project_xplanes_xT(const void* xplanes, int N, int F);
int project_xplanes_build(const float* x, int N, int F, void* xplanes, hipStream_t st);
// its backward (dl_project_bwd.hip): weight / bias gradients, W2 == nullptr for the single layer
size_t project_bwd_workspace_bytes(int N, int F, int K, int nhid, int d, bool two_layer);
// the dispatch decisions of project_fwd / project_bwd for a problem (host only; include/disenlink_hip.h lists the entries)
void project_fwd_form(int N, int F, int K, int nhid, int d, bool two_layer, size_t ws_bytes, bool have_xplanes, int* out);
void project_bwd_form(int N, int F, int K, int nhid, int d, bool two_layer, bool have_hid, bool have_xplanes, int* out);
int project_bwd(const float* x, int N, int F, int K, int nhid, int d, const float* W1, const float* b1,
                const float* W2, const float* dZ, const float* hid, float* dW1, float* db1, float* dW2, float* db2,
                void* ws, hipStream_t st, const void* xplanes = nullptr);

// the kept-hidden-layer half of the backward without the dW1 contraction (dl_project_bwd.hip), for dl_project_sparse.hip
size_t project_bwd_kept_workspace_bytes(int N, int K, int nhid, int d, bool two_layer);
void project_bwd_kept_form(int N, int K, int nhid, int d, bool two_layer, int* out3);   // sA, tiles per range, sC
void project_bwd_kept(int N, int K, int nhid, int d, const float* b1, const float* W2, const float* dZ, const float* hidT,
                      float* dhid, float* db1, float* dW2, float* db2, void* ws, hipStream_t st);

// projection of sparse features (dl_project_sparse.hip): layer 1 and dW1 as gathers over the CSR / CSC of x
int sparse_seg_len();
size_t project_sparse_fwd_workspace_bytes(const dl_sparse_features* x, int K, int nhid, int d, bool two_layer);
size_t project_sparse_bwd_workspace_bytes(const dl_sparse_features* x, int K, int nhid, int d, bool two_layer);
void project_sparse_form(int N, int F, int K, int nhid, int d, bool two_layer, bool affine, int max_col_len, int* out);
int project_sparse_fwd(const dl_sparse_features* x, int K, int nhid, int d, const float* W1, const float* b1, const float* W2,
                       const float* b2, float* Z, float* hid_out, void* ws, hipStream_t st);
int project_sparse_bwd(const dl_sparse_features* x, int K, int nhid, int d, const float* b1, const float* W2, const float* dZ,
                       const float* hid, float* dW1, float* db1, float* dW2, float* db2, void* ws, hipStream_t st);

}  // namespace dl
