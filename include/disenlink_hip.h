/*
 * disenlink_hip.h — C ABI of libdisenlink_hip.so (MI355X / gfx950).
 *
 * The reference (sjz5202/DisenLink) has no FFI / plugin interface: its hot path is the ATen op
 * sequence inside model.py.  This header is the boundary a maintainer would bind instead of
 * those op sequences; each entry point cites the reference lines it replaces.  INTEGRATION.md
 * shows the ctypes stub.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every pointer is a DEVICE pointer.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Nothing here
 *     allocates, frees or synchronises; scratch comes from the caller (`ws`, sized by
 *     dl_workspace_bytes).  Launches are asynchronous on `stream`.
 *   - the library is linked WITHOUT a HIP runtime and binds to the one the host process uses,
 *     so the caller's streams and allocations are valid here.
 *   - return 0 on success, a negative DL_E_* code on error; dl_last_error() returns the
 *     message of the calling thread's last failing call.
 *   - layouts: Z, H are [n_total][K][d] row-major (== torch.cat(h_k, dim=1) of model.py:114) in the
 *     storage type named by the `dtype` argument (fp32 or bf16); dZ, dH are always fp32 of the same
 *     shape; indices int32; factor ids uint8; s is fp32 [n_total][K] RAW row sums (the zero -> 1
 *     substitution of model.py:72 is applied where s is read).
 *   - sharding: a plan may cover only rows [row_offset, row_offset + n_rows) of the n_total
 *     nodes (one shard per GPU).  Node-indexed arrays are always indexed by GLOBAL node id and
 *     only the plan's rows are written; per-entry arrays (p, a, ...) are local to the plan.
 *   - results do not depend on launch order / placement; no float atomics are used, so every
 *     entry point is bitwise reproducible run to run.
 */
#ifndef DISENLINK_HIP_H
#define DISENLINK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DL_OK            0
#define DL_E_ARG        -1   /* null pointer / bad size / unsupported K or d */
#define DL_E_LAUNCH     -2   /* hipLaunch / hipGetLastError failure */
#define DL_E_WORKSPACE  -3   /* workspace missing or too small */

#define DL_MAX_FACTORS  64   /* K <= 64 */

/* Storage type of the node tables Z and H.  Arithmetic, per-edge values, probabilities and every
 * gradient are fp32 in both cases; bf16 only halves the bytes of the gathered rows (tuned kernels
 * only; the reference has no bf16 path — parity is defined against the fp32 restatement). */
typedef enum dl_dtype { DL_F32 = 0, DL_BF16 = 1 } dl_dtype;

/* A CSR over (a shard of) the nodes plus the segment plan that balances skewed rows: every row is
 * cut into >= 1 segments of <= seg_len consecutive entries; one wavefront owns one segment and one
 * workgroup (DL_UNIT_SEGS = 4 wavefronts) serves DL_UNIT_SEGS consecutive POSITIONS of the seg_* arrays.
 *
 * Units.  The segments of a row (of one column slice of a row, see below) are grouped, counting from the
 * row's first segment, into UNITS of at most DL_UNIT_SEGS consecutive segments (the kernels recognise a unit
 * as a run of positions with the same row AND the same slot inside one group of DL_UNIT_SEGS positions).  A unit never straddles a
 * group of DL_UNIT_SEGS positions (units of 3 are padded to 4, units are stored largest first inside a
 * slice, every slice region is padded to a multiple of DL_UNIT_SEGS; seg_row = -1 marks a padding
 * position), so the workgroup that holds it sums it on chip, in segment order.  Only rows with more than
 * one unit reduce through partial slots in the workspace — one slot per unit, summed in slot (= entry)
 * order by a combine kernel.  How a row is cut depends on that row alone, so a row shard gives the same
 * bits as the whole graph.
 *
 * XCD-aware slicing (optional, n_slices = 8 on MI355X): the column space is cut into n_slices
 * node ranges of equal entry count and no segment spans two of them; positions are stored slice-major and
 * workgroup b serves slice b % n_slices.  Workgroups b and b+8 are observed to share an XCD, so
 * each XCD's 4 MiB L2 only ever gathers rows of "its" 1/8 of the node table.  Placement is a
 * speed matter only: results do not depend on it. */
#define DL_UNIT_SEGS 4
typedef struct dl_csr_plan {
    int32_t n_rows;             /* rows of this plan */
    int32_t row_offset;         /* global node id of row 0 */
    int32_t n_total;            /* global node count (extent of node-indexed arrays) */
    int32_t n_entries;
    const int32_t* rowptr;      /* [n_rows+1] */
    const int32_t* col;         /* [n_entries] global node ids */
    int32_t seg_len;
    int32_t n_seg;              /* segment POSITIONS, padding included (a multiple of DL_UNIT_SEGS per slice) */
    const int32_t* seg_row;     /* [n_seg] local row of the segment, -1 = padding position */
    const int32_t* seg_beg;     /* [n_seg] first entry of the segment */
    const int32_t* seg_end;     /* [n_seg] one past its last entry */
    const int32_t* seg_slot;    /* [n_seg] partial slot of the segment's UNIT, -1 if the row is a single unit */
    int32_t n_slices;           /* >= 1 */
    int32_t slice_max_seg;      /* largest number of positions in one slice stream (sizes the launch grid) */
    const int32_t* slice_seg0;  /* [n_slices+1] first position of each slice stream (multiples of DL_UNIT_SEGS) */
    int32_t n_multi;            /* rows with more than one unit */
    int32_t n_slots;            /* units belonging to such rows */
    const int32_t* multi_row;   /* [n_multi] local row */
    const int32_t* multi_slot0; /* [n_multi+1] first slot of each such row (slots are consecutive) */
    /* Optional pair (both NULL = rows of several units are always summed by a separate combine launch): with them the
     * kernels that know how sum such a row INSIDE the launch — every unit stores its partial slot, adds 1 to the row's
     * counter, and the unit whose add comes last adds the slots in the combine kernel's own order and writes the row
     * (same bits as the separate launch; no float atomics).  unit_count belongs to the plan: n_multi zero-initialised
     * int32 in device memory that only the library writes — the last unit of a row puts its counter back to 0, so the
     * array is all zero again when a launch has completed; one launch at a time per plan. */
    const int32_t* slot_multi;  /* [n_slots] index (into multi_row / multi_slot0) of the row a slot belongs to */
    int32_t* unit_count;        /* [n_multi] */
} dl_csr_plan;

/* The binarised, symmetrised training adjacency (main_disentangled.py:137-142): entries are the
 * directed non-zeros of adj_sym, col ascending inside a row, both directions present. */
typedef struct dl_graph {
    dl_csr_plan csr;
    /* Optional second segment plan over the SAME rowptr/col arrays, used by dl_route_fwd only (route.n_seg == 0
     * disables it).  It may be XCD-sliced (routing gathers whole Z rows, K*d*4 bytes per edge), and with
     * route_mirror != 0 it covers only the entries with col >= row: routing is symmetric — (i,j) and (j,i)
     * evaluate the same fma chain — so each undirected edge is computed once and written to both entries
     * through rev[e] = index of (col[e], row(e)).  Mirroring needs an unsharded plan. */
    dl_csr_plan route;
    const int32_t* rev;         /* [n_entries], needed when route_mirror != 0 */
    int32_t route_mirror;
    /* Optional (NULL = none), read by dl_route_fwd only: the entries with col >= row of an unsharded, mirrored graph as
     * a hub plan (dl_pair_hub below) — every undirected edge is a slot in a block row of its endpoint of LARGER degree,
     * scored against the other endpoint as the partner row.  step_q holds the entry's index into p / a, step_q2 the index
     * of the reverse entry (-1 for a self-loop); there is no residual plan (rest.n_entries == 0) and n_entries equals the
     * number of entries with col >= row.  Used for fp32 tables with d = 64 and K in {4, 8} unless DL_ROUTE_HUB=0; every
     * other call walks `route` as before.  Same bits either way. */
    const struct dl_pair_hub* route_hub;
} dl_graph;

/* A CSR over pair slots: row u lists other endpoints (csr.col) and pair ids (inc_pair).
 *   - as the backward's node-incidence list, every pair occupies two slots (one per endpoint;
 *     a pair (u,u) appears twice in row u);
 *   - as the forward's "pairs by first endpoint" list, every pair occupies one slot in row pu. */
typedef struct dl_pair_incidence {
    dl_csr_plan csr;
    const int32_t* inc_pair;    /* [csr.n_entries] */
    int32_t n_pairs;            /* extent of the prob / g_prob arrays */
    /* Optional (NULL = not given), read by dl_score_pairs_train only: the labels and loss weights of its `y` / `w`
     * arguments laid out PER ENTRY, [csr.n_entries][2] = (y[inc_pair[e]], +-w[inc_pair[e]]) — a coalesced stream instead of
     * two random 4-byte reads per entry.  The sign of the weight marks the entry that writes prob[]: + in the row of the
     * pair's FIRST endpoint (csr row == pu), - (also -0.0) in the other one, so every probability is written once.
     * Whoever sets it keeps it consistent with the y / w passed alongside (disenlink_amd/graph.py caches it per label /
     * weight tensor). */
    const float* entry_yw;
    /* Optional (NULL = not given), read by dl_score_pairs_fwd only: a forward plan with mirrored pairs folded.  The
     * score is symmetric in its endpoints, so where the list holds both (u,v) and (v,u) one entry can stand for the
     * two: inc_pair2[e] is the id of the second pair entry e scores (-1 = none), its probability and per-factor terms
     * are written next to those of inc_pair[e].  n_second counts the entries with inc_pair2[e] >= 0: such a plan lists
     * every pair exactly once as a first or a second id, csr.n_entries + n_second == n_pairs. */
    const int32_t* inc_pair2;   /* [csr.n_entries] */
    int32_t n_second;
    /* Optional (NULL = not given), read by dl_score_pairs_fwd only: the same entries cut into a hub plan and a residual
     * plan (dl_pair_hub below).  csr / inc_pair / inc_pair2 still describe the whole list. */
    const struct dl_pair_hub* hub;
    /* Optional (NULL = not given), read by dl_score_pairs_fwd only: the same entries once more as a hub plan of five step
     * shapes (dl_pair_hub_mixed below), which gathers fewer partner rows for the same scores.  Where it is given it is
     * walked INSTEAD of `hub` (fp32 tables, d = 64, K in {4, 8}) unless DL_SCORE_HUB_MIXED=0; same bits either way. */
    const struct dl_pair_hub_mixed* hub_mixed;
} dl_pair_incidence;

/* Hub plan of the forward scorer.  The rows with the most entries ("hub rows", ranked by entry count) are cut into
 * blocks of DL_HUB_W consecutive ranked rows; the 16 rows of a block score against many of the same partner rows, and a
 * workgroup that holds the block's [Z | H] rows in LDS gathers such a partner row ONCE for up to four of them.
 * A work item is one (block, column slice) — long ones are cut into several items — and holds three lists of STEPS of
 * four SLOTS; a slot is one entry (u_local = its row's place in the block, its pair id, its second pair id or -1):
 *   shape A: four gathered partner rows, slot e scores against row e;
 *   shape B: two gathered rows, slots 0,1 against the first and 2,3 against the second;
 *   shape C: one gathered row, all four slots against it.
 * A dead slot has pair id -1, a dead partner row -1; only the last step of a list holds any, behind its live ones — the
 * kernel relies on it: it gathers the partner rows of every other step without looking at them.  Steps are stored item by
 * item as [A steps | B steps | C steps], item_step = the four boundaries.  Items are stored slice-major like the
 * positions of a dl_csr_plan: workgroup b serves slice stream b % n_slices.  Every entry of the list is a live slot of
 * exactly one step or an entry of `rest`, a plan of the usual form over the rows that are no hub rows.
 * The four step_* arrays must be 16-byte aligned: a step's four words are read as one vector. */
#define DL_HUB_W 16
typedef struct dl_pair_hub {
    int32_t n_blocks;
    const int32_t* block_row;   /* [n_blocks * DL_HUB_W] global node id of the block's rows, -1 = none */
    int32_t n_items;
    int32_t n_slices;           /* slice streams (the grid's stride) */
    int32_t slice_max_item;     /* most items in one stream (sizes the grid) */
    const int32_t* slice_item0; /* [n_slices + 1] first item of each stream */
    const int32_t* item_block;  /* [n_items] */
    const int32_t* item_step;   /* [n_items][4]: A steps [0],[1)  B steps [1],[2)  C steps [2],[3) */
    int32_t n_steps;
    const int32_t* step_v;      /* [n_steps][4] partner rows (A: 4, B: the first 2, C: the first), -1 = dead */
    const int32_t* step_u;      /* [n_steps][4] u_local of each slot, 0 .. DL_HUB_W - 1 */
    const int32_t* step_q;      /* [n_steps][4] pair id of each slot, -1 = dead */
    const int32_t* step_q2;     /* [n_steps][4] second pair id (-1 = none); NULL when inc_pair2 is NULL */
    int32_t n_entries;          /* live slots */
    dl_csr_plan rest;           /* residual plan (rest.n_entries + n_entries == csr.n_entries) */
    const int32_t* rest_pair;   /* [rest.n_entries] */
    const int32_t* rest_pair2;  /* [rest.n_entries], NULL when inc_pair2 is NULL */
} dl_pair_hub;

/* Hub plan of the forward scorer with MIXED step shapes.  The c slots of one block on one partner row give c / 4 steps of
 * shape C as above, but the remainder of 1, 2 or 3 slots stays ONE piece that gathers its partner row once, and pieces of
 * different partner rows share a step.  An item holds five lists of steps, stored [A | A211 | B | B31 | C]:
 *   A    1+1+1+1  four gathered rows,  slot e against row e;
 *   A211 2+1+1    three gathered rows, slots 0,1 against the first, 2 against the second, 3 against the third;
 *   B    2+2      two gathered rows,   slots 0,1 against the first and 2,3 against the second;
 *   B31  3+1      two gathered rows,   slots 0,1,2 against the first and 3 against the second;
 *   C    4        one gathered row,    all four slots against it.
 * `hub` is a dl_pair_hub whose item_step is [n_items][6] — the six boundaries of the five lists — and whose step_v holds
 * the gathered rows of a step in its first 4 / 3 / 2 / 2 / 1 words.  A slot's hub row may be EITHER endpoint of its pair
 * (the score is symmetric).  Dead partner rows stand only in the last step of each of the first four lists, behind the
 * live ones; a dead slot (pair id -1) scores nothing wherever it stands.  Everything else is as in dl_pair_hub. */
#define DL_HUB_MIXED_LISTS 5
typedef struct dl_pair_hub_mixed {
    dl_pair_hub hub;
    int32_t n_lists;            /* DL_HUB_MIXED_LISTS */
} dl_pair_hub_mixed;

/* ---- host-side graph preparation (no GPU; the only entry points that allocate: malloc'd outputs are
 * released by the matching *_free).  Counterpart of the dense adjacency construction of
 * main_disentangled.py:137-142 for hosts without Python; disenlink_amd/graph.py builds identical arrays
 * with torch index ops on the device.  Upload the arrays and point a dl_csr_plan at them. */
typedef struct dl_host_csr {
    int32_t n_nodes;
    int32_t n_entries;
    int32_t* rowptr;            /* [n_nodes+1] */
    int32_t* col;               /* [n_entries], ascending inside a row */
    int32_t* rev;               /* [n_entries] */
} dl_host_csr;

typedef struct dl_host_plan {   /* the segment-plan fields of dl_csr_plan, in host memory */
    int32_t seg_len, n_seg, n_slices, slice_max_seg, n_multi, n_slots;
    int32_t *seg_row, *seg_beg, *seg_end, *seg_slot, *slice_seg0, *multi_row, *multi_slot0;
    int32_t* slot_multi;        /* [n_slots]; unit_count is not built here: n_multi zeroed int32 on the device */
} dl_host_plan;

/* Directed edge rows (duplicates allowed) -> CSR of the binarised adjacency; symmetrise != 0 reproduces
 * adj_sym = (adj + adj.T) != 0.  Fails if the result is not symmetric. */
int dl_host_csr_from_edges(const int64_t* src, const int64_t* dst, int64_t n_edge_rows, int32_t n_nodes,
                           int symmetrise, dl_host_csr* out);
void dl_host_csr_free(dl_host_csr* csr);

/* Segment plan of a CSR (see dl_csr_plan): segments of <= seg_len entries, never spanning two of the
 * n_col_slices column slices (1 = unsliced; a multiple of 8 = XCD streams x time), optionally only over
 * the entries with keep[e] != 0 (one contiguous run per row, e.g. col >= row for symmetric routing).
 * unit_segs = DL_UNIT_SEGS groups the segments of a row into units (plans whose kernels sum over a row);
 * unit_segs = 1 makes every segment its own unit, positions in entry order (routing plan, forward scorer).
 * by_length != 0 places the units of one size class by their number of entries, most first, instead of in entry order:
 * the wavefronts of a workgroup then finish together.  Use it when the gathered tables (2 * n_total * K * d * element
 * size) fit the 256 MiB Infinity Cache; where the row streams come from HBM, entry order is faster.  Results do not
 * depend on it. */
int dl_host_plan_build(int32_t n_rows, int32_t n_total, const int32_t* rowptr, const int32_t* col, int32_t seg_len,
                       int32_t n_col_slices, const uint8_t* keep, int32_t unit_segs, int32_t by_length,
                       dl_host_plan* out);
void dl_host_plan_free(dl_host_plan* plan);

const char* dl_version(void);
const char* dl_last_error(void);
/* The library's environment switches (measurement / test knobs, csrc/dl_config.h) are read once, at the first call that
 * needs one: no launch path touches the environment.  This reads them again (for a process that changes one). */
void dl_config_reload(void);

/* 1 if (K,d) runs on the tuned wavefront-tiled kernels, 0 if it falls back to the generic ones. */
int dl_has_fast_path(int K, int d);
int dl_has_fast_path_dtype(int K, int d, dl_dtype dtype);
/* Force the generic kernels (parity cross-check of the two implementations): 1 = on, 0 = off,
 * negative = query only.  Returns the previous value. */
int dl_set_force_generic(int on);

/* Scratch needed by the calls below for this plan and shape. */
size_t dl_workspace_bytes(const dl_csr_plan* plan, int K, int d);

/* Factor projection on the matrix cores: replaces model.py:13-15 / 24-27 fanned out at model.py:106.
 *   two-layer (Factor2):   Z[n][k][:] = W2[k] . relu(W1[k] . x[n] + b1[k]) + b2[k]
 *                          W1 [K][nhid][F], b1 [K][nhid], W2 [K][d][nhid], b2 [K][d]
 *   single layer (Factor): pass W2 = b2 = NULL, nhid = 1:  Z[n][k][:] = W1[k] . x[n] + b1[k],  W1 [K][d][F], b1 [K][d]
 * x is fp32 [N][F] row-major, Z fp32 [N][K][d].  d must be 32, 64 or 128 (dl_project_supported).
 * fp32 in, fp32 results.  With the workspace, both layers run on the bf16 matrix path at fp32-grade accuracy: x, W1,
 * W2 (once per call) and the hidden activations (in registers) are split into three bf16 planes each
 * (v = hi + mid + lo) and every term is the sum of six exact bf16 products in an fp32 accumulator; when ws is
 * NULL / too small or DL_PROJECT_FP32_MFMA=1 is set, everything is plain fp32 MFMA (v_mfma_f32_32x32x2_f32: an
 * exact k-ordered fmaf chain).
 * ws (optional, dl_project_fwd_workspace_bytes): the plane arrays, and on small graphs the partial sums of the
 * several workgroups per node tile that share the hidden layer (added in a fixed order); without it one workgroup
 * walks the whole hidden layer with fp32 MFMA — same result up to rounding / summation order, slower.
 * ws == NULL is equivalent to a workspace of 0 bytes: where the layout needs none (DL_PROJECT_FP32_MFMA=1 with one
 * hidden-chunk group) both run the same form, node blocks of DL_FWD_BLOCK_ROWS included. */
int dl_project_supported(int d);
size_t dl_project_fwd_workspace_bytes(int N, int F, int K, int nhid, int d, int two_layer);
/* hid_out (optional, two-layer form, dl_project_hidden_floats(N, K, nhid) floats): keep the hidden layer
 * relu(W1 x + b1), laid out hidT [K][nhid][(N+3)&~3], for dl_project_bwd — worth its 8 bytes of traffic per
 * hidden unit from F of about 150 up; NULL = the backward recomputes it (no [N,K,nhid] memory at all). */
size_t dl_project_hidden_floats(int N, int K, int nhid);
int dl_project_fwd(const float* x, int N, int F, int K, int nhid, int d,
                   const float* W1, const float* b1, const float* W2, const float* b2,
                   float* Z, float* hid_out, void* ws, size_t ws_bytes, void* stream);

/* Persistent operand planes of the feature matrix (round 5).  model.py:106 evaluates the K MLPs on the SAME x every epoch
 * (main_disentangled.py:194): dl_project_fwd / dl_project_bwd split x (and x^T) into the three bf16 planes of the matrix
 * path inside ws on every call.  A caller that keeps x for a run builds them ONCE into a buffer of its own
 * (dl_project_xplanes_bytes; 16-byte aligned; tile-major planes of x, then of x^T) and passes it to the _xp forms, which
 * then skip those splits — same products, same bits.  The buffer is valid for exactly the (x contents, N, F) it was built
 * from; xplanes == NULL behaves like the plain entry points.  Two-layer form on the bf16 matrix path only (the single
 * layer and DL_PROJECT_FP32_MFMA=1 ignore it); graphs processed in node blocks re-split per block and ignore it too. */
size_t dl_project_xplanes_bytes(int N, int F);
int dl_project_xplanes_build(const float* x, int N, int F, void* xplanes, size_t xplanes_bytes, void* stream);
int dl_project_fwd_xp(const float* x, int N, int F, int K, int nhid, int d,
                      const float* W1, const float* b1, const float* W2, const float* b2,
                      float* Z, float* hid_out, void* ws, size_t ws_bytes, const void* xplanes, void* stream);
int dl_project_bwd_xp(const float* x, int N, int F, int K, int nhid, int d,
                      const float* W1, const float* b1, const float* W2, const float* dZ, const float* hid,
                      float* dW1, float* db1, float* dW2, float* db2,
                      void* ws, size_t ws_bytes, const void* xplanes, void* stream);

/* Backward of the projection: replaces autograd of model.py:13-15 / 24-27 under loss.backward()
 * (main_disentangled.py:198).  dZ fp32 [N][K][d] in; weight and bias gradients out, shaped like the weights
 * (dW1 like W1, db1 like b1, dW2 like W2, db2 like b2; single layer: W2 = dW2 = db2 = NULL, nhid = 1).
 * x is data and gets no gradient.  The hidden layer is recomputed on the matrix cores (never read from HBM);
 * ws needs dl_project_bwd_workspace_bytes(...) bytes (the masked hidden gradient of one node block — kept as the
 * three bf16 planes of its transpose, the operand of the dW1 contraction on the bf16 matrix path, fp32-grade like
 * the forward's layer 1 — the planes of x^T for that block, and the per-node-range partial slabs).  Sums over nodes are taken range by range in a fixed order (no float
 * atomics): the gradients are bitwise reproducible. */
size_t dl_project_bwd_workspace_bytes(int N, int F, int K, int nhid, int d, int two_layer);
int dl_project_bwd(const float* x, int N, int F, int K, int nhid, int d,
                   const float* W1, const float* b1, const float* W2, const float* dZ,
                   const float* hid /* hid_out of the forward, or NULL = recompute */,
                   float* dW1, float* db1, float* dW2, float* db2,
                   void* ws, size_t ws_bytes, void* stream);

/* Which form of the projection a problem runs (host only, nothing is launched): the decisions dl_project_fwd /
 * dl_project_bwd take, computed by the code that takes them, under the current DL_* switches.  For tests that must
 * know which kernel instantiation and launch mode a shape reaches.
 *   dl_project_fwd_form   ws_bytes = 0: no workspace.  out[DL_PROJECT_FWD_FORM_LEN] =
 *       [0] three-plane products (else fp32 MFMA)  [1] VEC  [2] hidden-chunk groups G  [3] chunks per group
 *       [4] rows per launch  [5] launches  [6] the persistent x planes are used
 *       (single layer: 0, 0, 1, 0, N, 1, 0)
 *   dl_project_bwd_form   of the first node block (a last block may be shorter).  out[DL_PROJECT_BWD_FORM_LEN] =
 *       [0] plane dhid + plane kernel B  [1] VEC of kernel A  [2] VEC of the fp32 kernel B  [3] hidden layer recomputed
 *       [4] node ranges of kernel A  [5] node tiles per range  [6] node ranges of kernel B  [7] node chunks per range
 *       [8] ranges of the column sums  [9] kernel B writes dW1 directly  [10] node blocks accumulate  [11] rows per block
 *       [12] blocks  [13] the persistent x^T planes are used */
#define DL_PROJECT_FWD_FORM_LEN 7
#define DL_PROJECT_BWD_FORM_LEN 14
int dl_project_fwd_form(int N, int F, int K, int nhid, int d, int two_layer, size_t ws_bytes, int have_xplanes, int* out);
int dl_project_bwd_form(int N, int F, int K, int nhid, int d, int two_layer, int have_hid, int have_xplanes, int* out);

/* Sparse feature input of the projection (replaces model.py:13-15 / 24-27 fanned out at model.py:106 for features that
 * are sparse, or two-valued per row after row standardisation):
 *     x~[i][f] = scale[i] * X[i][f] + shift[i]
 * X is a CSR (columns strictly ascending within a row; val == NULL: all ones), scale / shift are per node (NULL: 1 / 0).
 * The struct also carries the CSC view of X (rows ascending within a column; csc_entry = index of the entry in col / val)
 * and the segment plan of the dW1 gather: column f is cut into ceil(len / seg_len) segments of seg_len consecutive entries
 * (the last may be shorter), numbered colseg[f] .. colseg[f+1]-1; seg_col[s] is the column of segment s.  How a column is
 * cut depends on that column alone.  seg_len must be dl_sparse_seg_len() (512 entries unless DL_SPARSE_SEG is set).
 * Every pointer is a device pointer; N, F, nnz, seg_len, n_seg are host values. */
typedef struct dl_sparse_features {
    int32_t N, F, nnz;
    const int32_t* rowptr;      /* [N+1] */
    const int32_t* col;         /* [nnz] */
    const float* val;           /* [nnz] or NULL = ones */
    const float* scale;         /* [N] or NULL = 1 */
    const float* shift;         /* [N] or NULL = 0 */
    const int32_t* colptr;      /* [F+1] */
    const int32_t* csc_row;     /* [nnz] */
    const int32_t* csc_entry;   /* [nnz] */
    int32_t seg_len, n_seg;
    const int32_t* colseg;      /* [F+1] */
    const int32_t* seg_col;     /* [n_seg] */
} dl_sparse_features;
int dl_sparse_seg_len(void);

/* Projection of sparse features: model.py:13-15 / 24-27 at model.py:106 with layer 1 as a gather.  The arguments are those
 * of dl_project_fwd with the struct in place of x (N and F are the struct's).  Per node i and output column c of layer 1
 * (c = k * nhid + h; single layer: c = k * d + dd):
 *     acc = sum over the entries e of row i, ascending, of val[e] * W1[c][col[e]]          (one fp32 fma chain)
 *     pre = scale[i] * acc + shift[i] * csum[c] + b1[c],   csum[c] = sum_f W1[c][f]  (formed only when shift is given)
 * two-layer: hid = relu(pre) goes to hid_out (REQUIRED, dl_project_hidden_floats(N, K, nhid) floats, the layout of
 * dl_project_fwd's hid_out) and Z = W2 . hid + b2 is formed from it on the matrix cores (three bf16 planes per operand,
 * six exact products per term); single layer (W2 = b2 = NULL, nhid = 1): Z = pre.  d in {32, 64, 128}.
 * A row's result depends on that row alone.  No float atomics: bitwise reproducible.
 * ws (required): dl_project_sparse_fwd_workspace_bytes — W1 transposed to [F][K*nhid] (per call: the weights move every
 * step) and csum. */
size_t dl_project_sparse_fwd_workspace_bytes(const dl_sparse_features* x, int K, int nhid, int d, int two_layer);
int dl_project_sparse_fwd(const dl_sparse_features* x, int K, int nhid, int d,
                          const float* W1, const float* b1, const float* W2, const float* b2,
                          float* Z, float* hid_out, void* ws, size_t ws_bytes, void* stream);

/* Its backward (autograd of model.py:13-15 / 24-27 under loss.backward(), main_disentangled.py:198): the gradients of
 * dl_project_bwd.  hid (two-layer) is REQUIRED: there is no recompute form.  dW2, db2, db1 and the masked hidden
 * gradient dhid come from the kept form of dl_project_bwd's first kernel; dW1 is a gather over the CSC view:
 *     dW1[c][f] = sum over the entries e of column f, rows ascending, of (scale[i] * val[e]) * dhid[i][c]  +  g[c],
 *     g[c] = sum_i shift[i] * dhid[i][c]   (only with shift; node ranges summed in a fixed order),
 * column segments summed by separate waves and added in segment order.  Every element of every gradient is written
 * (empty columns included).  No float atomics.  ws (required): dl_project_sparse_bwd_workspace_bytes. */
size_t dl_project_sparse_bwd_workspace_bytes(const dl_sparse_features* x, int K, int nhid, int d, int two_layer);
int dl_project_sparse_bwd(const dl_sparse_features* x, int K, int nhid, int d,
                          const float* W1, const float* b1, const float* W2, const float* dZ, const float* hid,
                          float* dW1, float* db1, float* dW2, float* db2, void* ws, size_t ws_bytes, void* stream);

/* The launch decisions of the two entries above for a shape (host only, nothing is launched; model.py:13-15, 24-27, 106),
 * under the current DL_SPARSE_SEG / DL_BWD_TARGET.  affine: shift is given; max_col_len: entries of the longest column.
 * out[DL_PROJECT_SPARSE_FORM_LEN] =
 *   [0] 256-column chunks of the layer-1 output  [1] columns of the last chunk (256 = not ragged)  [2] the affine term
 *   (csum, g) is formed  [3] segments of the longest column  [4] entries per segment  [5] two-layer  [6] width of the
 *   layer-2 kernel and of kernel A (0: single layer, neither runs)  [7] the dW1 gather reads dhid rows as aligned quads
 *   [8] node ranges of kernel A  [9] node ranges of g */
#define DL_PROJECT_SPARSE_FORM_LEN 10
int dl_project_sparse_form(int N, int F, int K, int nhid, int d, int two_layer, int affine, int max_col_len, int* out);

/* Routing: replaces model.py:56-72 restricted to adj==1 entries.
 *   per edge e=(i,j):  sigma_k = z_k[i].z_k[j] / t ; e_k = exp(sigma_k) ; alpha_k = e_k / sum_k e_k
 *                      p[e] = argmax_k alpha_k (first max; NaN counts as max) ; a[e] = alpha_p
 *   per node:          s[i][k] = sum_{e in row i, p[e]=k} a[e]          (raw; model.py:70-71) */
int dl_route_fwd(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float t,
                 uint8_t* p, float* a, float* s, void* ws, size_t ws_bytes, void* stream);

/* Aggregation ("K-factor edge scatter"): replaces model.py:73-75.
 *   H[i][k] = beta*Z[i][k] + (1-beta) * sum_{e=(i,j), p[e]=k} a[e] / s~[j][k] * Z[j][k]
 *   with s~ = (s==0 ? 1 : s) and the normaliser taken at the NEIGHBOUR j (model.py:73 broadcast);
 *   s must hold the rows of every neighbour (all-gathered when sharded). */
int dl_aggregate_fwd(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta,
                     const uint8_t* p, const float* a, const float* s,
                     void* H, void* ws, size_t ws_bytes, void* stream);

/* Pair-list link scorer: replaces model.py:109-113 evaluated at the listed (u,v) only.
 *   prob[q] = sigmoid( sum_k (h_k[u].h_k[v]) * exp(z_k[u].z_k[v] / t) )    (raw exp, not softmax)
 * by_u (optional, may be NULL): the same pairs as a CSR by first endpoint (each pair once, inc_pair =
 * position in pu/pv/prob — or, with inc_pair2, a listed (u,v) and its listed reverse (v,u) as ONE entry
 * that names both positions); lets a wavefront keep the u rows in LDS for a whole segment and, when
 * sliced, keeps the gathered v rows inside one XCD's L2.
 * coef (optional, may be NULL; training only): [2][n_pairs][K] — coef[0][q][k] = e_k = exp(z_k[u].z_k[v]/t)
 * and coef[1][q][k] = (h_k[u].h_k[v]) * e_k, the per-factor terms of the logit.  Handing them to
 * dl_score_pairs_bwd turns the backward into two plain weighted row gathers (no dot products). */
int dl_score_pairs_fwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                       const int32_t* pu, const int32_t* pv, int n_pairs,
                       const dl_pair_incidence* by_u,
                       float* prob, float* coef, void* stream);

/* Dense scorer: replaces model.py:109-113 as written — prob[u][v] for ALL N*N ordered pairs (row-major
 * fp32 [N][N]), the link_pred the reference's caller indexes with dense masks (main_disentangled.py:195).
 * No pair list is materialised.  fp32 tables with d % 32 == 0 go to the matrix cores (two Gram products per
 * factor, six exact bf16 products per term from three bf16 planes per operand; only the tile pairs u <= v are computed and mirrored: prob is symmetric bit for bit);
 * other shapes use the vector kernels.  Its backward is dl_score_allpairs_bwd over the support of the caller's
 * loss masks.  N*N must stay below 2^31: N <= 46340.
 * ws (optional, dl_score_allpairs_workspace_bytes): the bf16 planes of Z and H, split once per call; without it
 * (NULL / too small) every tile pair splits the rows it stages — same result bit for bit, slower. */
size_t dl_score_allpairs_workspace_bytes(int N, int K, int d, dl_dtype dtype);
/* Which kernel and launch geometry dl_score_allpairs_fwd takes (host only, nothing is launched; honours
 * dl_set_force_generic), computed by the code that takes the decision.  ws_bytes = 0: no workspace.
 * out[DL_SCORE_ALLPAIRS_FWD_FORM_LEN] =
 *   [0] kernel: 0 generic, 1 per shape, 2 matrix cores splitting what they stage, 3 matrix cores from planes
 *   [1] work items (generic: ordered pairs; per shape: rows x chunks; matrix cores: tile pairs u tile <= v tile)
 *   [2] workgroups  [3] column slices  [4] slice width  [5] 256-column chunks per row and slice ([3..5]: per shape only) */
#define DL_SCORE_ALLPAIRS_FWD_FORM_LEN 6
int dl_score_allpairs_fwd_form(int N, int K, int d, dl_dtype dtype, size_t ws_bytes, int* out);
int dl_score_allpairs_fwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                          float* prob, void* ws, size_t ws_bytes, void* stream);

/* The LOGITS of the dense scorer: logit[u][v] = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t) for all N*N ordered pairs
 * (row-major fp32 [N][N]) — model.py:109-113 without its sigmoid, the tensor F.binary_cross_entropy_with_logits is written on
 * (replaces link_pred of main_disentangled.py:195 for a caller that wants a loss without the saturation of the fp32 sigmoid:
 * sigmoid_ref is exactly 1 from logit 16.64 on).  The argument list is dl_score_allpairs_fwd's with `logit` in place of
 * `prob`.  It is that entry's matrix-core kernel from planes with the sigmoid left out: the same products in the same order,
 * so wherever dl_score_allpairs_fwd takes that kernel (fp32 tables, d % 32 == 0) prob = sigmoid(logit) element by element, and
 * logit is symmetric bit for bit (only the tile pairs u <= v are computed, and mirrored).  The planes pad every factor to a
 * multiple of 32 columns with zeros, so every d of the library is served by this one kernel; fp32 tables only (DL_BF16 is
 * DL_E_ARG), N <= 46340, t != 0, N = 0 succeeds.  Logit space does not cure an overflowed exp: such an entry is inf or NaN.
 * ws: dl_score_allpairs_logits_workspace_bytes(N, K, d) bytes (0 for arguments out of range), the planes of Z and H — NOT
 * optional here: a missing or short workspace fails with DL_E_WORKSPACE.  For d % 32 == 0 it is
 * dl_score_allpairs_workspace_bytes(N, K, d, DL_F32).  No atomics, no host read, the caller's stream. */
size_t dl_score_allpairs_logits_workspace_bytes(int N, int K, int d);
int dl_score_allpairs_logits_fwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                                 float* logit, void* ws, size_t ws_bytes, void* stream);

/* Backward of dl_score_allpairs_fwd (autograd of model.py:109-113 + sigmoid under main_disentangled.py:195-198) on a
 * FIXED pair plan: the reference's caller takes its loss on link_pred[mask == 1] with masks built once per run
 * (main_disentangled.py:167-190), so d loss / d link_pred can be non-zero only on the masks' support.  The caller
 * hands that support over ONCE as a pair list (pu, pv) with its incidence plan `inc` (the one dl_score_pairs_bwd
 * takes; inc->n_pairs = n_pairs) and every step the dense prob [N][N] of the forward and the dense gradient
 * g_prob [N][N] autograd produced; the call reads both at the listed entries and writes
 *   dZ, dH = sum over the listed (u,v) of the scorer's backward terms (see dl_score_pairs_bwd),
 * for the plan's rows.  Entries of g_prob OUTSIDE the list are not read: the plan must cover every entry that can
 * carry gradient (keying the plan on the gradient's non-zero entries instead is wrong — a saturated positive,
 * p == 1.0 with y == 1, has exactly zero BCE gradient one epoch and a non-zero one the next).  Listed entries whose
 * gradient happens to be zero add exactly zero.  ws: dl_workspace_bytes(&inc->csr, K, d) — the gathered
 * prob / g_prob vectors live in it. */
int dl_score_allpairs_bwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                          const dl_pair_incidence* inc, const int32_t* pu, const int32_t* pv, int n_pairs,
                          const float* prob, const float* g_prob, float* dZ, float* dH,
                          void* ws, size_t ws_bytes, void* stream);

/* Dense backward of dl_score_allpairs_fwd: the gradient of ANY loss on link_pred — what the reference's autograd gives
 * for whatever its caller does with the dense output (model.py:109-113 under loss.backward(), main_disentangled.py:198)
 * — without a pair plan, a declaration or a host read.  prob is the forward's saved output, g_prob the dense gradient
 * d loss / d link_pred, both [N][N] row-major; g_prob need not be symmetric.  With G = g_prob o prob o (1 - prob),
 * G^ = G + G^T and per factor k  S = Z_k Z_k^T, E = exp(S / t), Q = H_k H_k^T:
 *   dH_k = (G^ o E) . H_k          dZ_k = (G^ o Q o E / t) . Z_k          (the diagonal included as written),
 * on the matrix cores: the forward's Gram products (three bf16 planes per operand, six exact products per term), the
 * two weight tiles split into three bf16 planes as well and multiplied against the rows of H_k / Z_k the same way.
 * Every tile is formed: a zero of G^ against an overflowed E = inf gives NaN, as autograd does.  fp32 tables with
 * 1 <= d <= 128 (dl_score_allpairs_bwd_dense_supported; d is padded to a multiple of 32 with zero columns), N <= 46340.
 * Every element of dZ, dH [N][K][d] is written.  No float atomics; the v range is sliced for occupancy as a function
 * of (N, K, d) only and the slices are summed in order, so results are bitwise reproducible.  N = 0 succeeds.
 * ws: dl_score_allpairs_bwd_dense_workspace_bytes(N, K, d) bytes (0 for unsupported shapes): G^, the planes of Z, H and
 * of their transposes, and the slices' partial sums; a missing or short workspace fails with DL_E_WORKSPACE. */
int dl_score_allpairs_bwd_dense_supported(int K, int d);              /* fp32 tables, 1 <= d <= 128 */
/* The launch form of dl_score_allpairs_bwd_dense (host only).  out[DL_SCORE_ALLPAIRS_BWD_DENSE_FORM_LEN] =
 *   [0] Np  [1] 32-column chunks of the padded factor width (the kernel's NCB)  [2] slices of the v range (1: no combine
 *   launch)  [3] v tiles of the shortest slice  [4] v tiles of the longest slice
 * [0..2] come from the layout code the launch calls; [3] and [4] restate on the host the split the kernel itself takes
 * (slice s walks the tiles [s nvt / nslice, (s + 1) nvt / nslice)), which lives in device code. */
#define DL_SCORE_ALLPAIRS_BWD_DENSE_FORM_LEN 5
int dl_score_allpairs_bwd_dense_form(int N, int K, int d, int* out);
size_t dl_score_allpairs_bwd_dense_workspace_bytes(int N, int K, int d);
int dl_score_allpairs_bwd_dense(const float* Z, const float* H, int N, int K, int d, float t,
                                const float* prob, const float* g_prob,   /* dense [N][N], row-major */
                                float* dZ, float* dH,                     /* [N][K][d], every element written */
                                void* ws, size_t ws_bytes, void* stream);

/* Dense backward of dl_score_allpairs_logits_fwd: the gradient of ANY loss on the logits (what autograd gives for model.py:109-113
 * without the sigmoid).  g_logit = d loss / d logit, dense [N][N] row-major, not necessarily symmetric; G^ = g_logit + g_logit^T
 * with no p (1 - p) factor and no saved forward output, and everything behind G^ is dl_score_allpairs_bwd_dense: the same
 * kernels, limits (fp32 tables, 1 <= d <= 128, N <= 46340, t != 0), determinism and "every tile is formed" NaN, and the same
 * workspace (dl_score_allpairs_bwd_dense_workspace_bytes; form: dl_score_allpairs_bwd_dense_form). */
int dl_score_allpairs_logits_bwd_dense(const float* Z, const float* H, int N, int K, int d, float t,
                                       const float* g_logit,                /* dense [N][N], row-major */
                                       float* dZ, float* dH,                /* [N][K][d], every element written */
                                       void* ws, size_t ws_bytes, void* stream);

/* Whole-graph reconstruction loss and its gradient with nothing of size N x N in memory: every non-edge is a negative, the
 * positives are up-weighted (the objective of the GAE family), and the gradient of the tables comes from the same call.
 * Included pairs: all unordered {u, v}, u != v, that are not in the ignored set; a pair in both sets is ignored.  For an
 * included pair, with s = sum_k (h_k[u].h_k[v]) exp(z_k[u].z_k[v] / t) and p = sigmoid(s):
 *   y = 1 if the pair is a positive, else 0;   w = w_pos for y = 1, else w_neg   (the caller's pos_weight / C and 1 / C,
 *   C = the number of included pairs, known on the host before the launch);
 *   loss = sum w BCE(p, y), the logs clamped at -100 as F.binary_cross_entropy and dl_pair_bce clamp them;
 *   d loss / d s = w (p - y), in the one-pass scorer's form with its max(p (1 - p), 1e-12) clamp (dl_score_pairs_train):
 *   a saturated pair contributes exactly 0.
 * pos_rowptr / pos_col and ign_rowptr / ign_col: SYMMETRIC CSRs over the N nodes (int32, rowptr [N + 1], columns ascending
 * and distinct within a row, every pair listed in both of its rows); the ignored set may be NULL / NULL.  Self entries of
 * either set mean nothing: the diagonal never carries loss.
 * Outputs: loss_out [1] double, counts_out [2] int64 = included positives and negatives as the scan saw them (DEVICE
 * values: the caller compares them with its own n_pos and N (N - 1) / 2 - |ignored| - n_pos), dZ, dH fp32 [N][K][d], every
 * element written.
 * Method: block_rows rows at a time (0 = the default: the largest multiple of 128 whose strip of block_rows x Np floats
 * stays at or under 1 GiB, the whole graph where that fits; otherwise a positive multiple of 128), the ranking scan in a
 * mode of its own forms the logits of the strip's rows against all nodes, and per value the loss term and
 * G^[u][v] = d loss / d s_uv (0 for ignored pairs, the diagonal and outside N); dl_score_allpairs_bwd_dense's kernel then
 * runs over the strip's rows with the strip as its G^.  Every unordered pair is visited from both of its rows: loss and
 * counts are the row sums halved (exactly).  No tile is skipped, so a zero of G^ against an overflowed exp gives NaN in the
 * gradients exactly as dl_score_allpairs_bwd_dense documents.  No float atomics, no host read, no allocation, the caller's
 * stream; the same bits on every call, for every block_rows and for every DL_RANK_SLICES.
 * Limits: fp32 tables, 1 <= d <= 128 (dl_score_recon_supported), 1 <= N <= DL_SCORE_RECON_MAX_N, t != 0.
 * ws: dl_score_recon_workspace_bytes(N, K, d, block_rows) bytes (0 for arguments out of range): with Np = N rounded up to 128
 * and dp = d to 32, four plane arrays of 6 K Np dp bytes, one strip of 4 block_rows Np, two cell arrays of block_rows Np / 32,
 * 24 N of row sums and the dense backward's slice partials (8 nslice N K d, none for nslice = 1), each rounded up to 256;
 * a missing or short workspace fails with DL_E_WORKSPACE. */
#define DL_SCORE_RECON_MAX_N 4194304
int dl_score_recon_supported(int K, int d);                          /* fp32 tables, 1 <= d <= 128 */
/* The launch form (host only).  out[DL_SCORE_RECON_FORM_LEN] = [0] Np  [1] strips  [2] rows per strip  [3] slices of the
 * v range of the backward: dl_score_allpairs_bwd_dense_form's for the whole N, whatever block_rows is. */
#define DL_SCORE_RECON_FORM_LEN 4
int dl_score_recon_form(int N, int K, int d, int block_rows, int* out);
size_t dl_score_recon_workspace_bytes(int N, int K, int d, int block_rows);
int dl_score_recon(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* pos_rowptr,
                   const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg,
                   int block_rows, double* loss_out, int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes,
                   void* stream);
/* The same on tables of either type: each entry has the argument list of the one above with `dtype` behind d, and the entries
 * above are these with DL_F32.  DL_BF16: Z and H are bf16 [N][K][d]; each table is its own single plane, so the scan and the
 * Gram products of the backward issue one matrix-core product per K = 16 block instead of six, and the backward's second
 * products (fp32 weights, three planes, against a one-plane table) three instead of six.  loss, counts, dZ and dH keep their
 * types (dZ, dH fp32: the gradient with respect to the bf16 values).
 * Bits: for every output element (loss, counts, dZ, dH) that is finite in the DL_F32 call on the same tables widened to fp32,
 * the DL_BF16 call returns the same bits — the products left out multiply planes that are identically zero and add exact
 * zeros.  An element that is non-finite in one call is non-finite in the other (which NaN or infinity is not promised); the
 * "no tile is skipped" NaN of an overflowed exp is kept.
 * Workspace: smaller than the DL_F32 one by exactly 16 K Np dp bytes (four plane arrays, each 6 K Np dp -> 2 K Np dp).
 * Unchanged: the limits (dl_score_scan_supported(K, d, dtype) states those of the shape), the strip rule and the form, the
 * determinism, the stream behaviour and the absence of atomics, host reads and synchronisation.  An unknown dtype is DL_E_ARG
 * and 0 from dl_score_recon_workspace_bytes_dtype. */
int dl_score_recon_form_dtype(int N, int K, int d, dl_dtype dtype, int block_rows, int* out);
size_t dl_score_recon_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype, int block_rows);
int dl_score_recon_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* pos_rowptr,
                         const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg,
                         int block_rows, double* loss_out, int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes,
                         void* stream);

/* The same objective in LOGIT space (replaces dl_score_recon_dtype where the fp32 sigmoid saturates — from logit 16.64 on it is
 * exactly 1, p (1 - p) falls under the 1e-12 clamp below -27.6, and a saturated pair then costs 100 w with gradient exactly 0,
 * so a confident false positive among the N^2 / 2 negatives is never pushed back; with the raw exp in the score such logits
 * are the ordinary regime).  The argument list, the sets, the weights, the outputs, the limits and refusals, the strips, the
 * form (dl_score_recon_form_dtype) and the workspace (dl_score_recon_workspace_bytes_dtype) are dl_score_recon_dtype's; there
 * are no twins of those.  What differs is the scan's epilogue, per included pair with logit s, label y and weight w:
 *   loss term = w l(s, y),   l = (1 - y) max(s, 0) + y max(-s, 0) + log1p(exp(-|s|))   (F.binary_cross_entropy_with_logits;
 *                            a zero factor drops its term; the body of dl_pair_bce_logits),
 *   d loss / d s = w (sigmoid(s) - y), formed without cancellation as dl_score_pairs_train_logits forms it: no clamp factor,
 *                            a gradient for every finite s.
 * Logit space cures the saturation of the sigmoid, not the overflow of exp: a non-finite logit (an overflowed exp, a NaN
 * table entry) gives a non-finite loss and non-finite gradients, never a silent zero; the "no tile is skipped" NaN of a zero
 * of G^ against E = inf is kept.  Launches, determinism (the same bits on every call, for every block_rows and DL_RANK_SLICES),
 * the DL_BF16 bits rule and the absence of atomics, host reads and synchronisation are dl_score_recon_dtype's. */
int dl_score_recon_logits(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* pos_rowptr,
                          const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg,
                          int block_rows, double* loss_out, int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes,
                          void* stream);

/* Ranking of ALL candidate links of query nodes (an extension; the reference has no counterpart): the logit of the dense
 * scorer, s(u,v) = sum_k (h_k[u].h_k[v]) * exp(z_k[u].z_k[v] / t) (pre-sigmoid link_pred, model.py:109-113), for every
 * (query, candidate) pair on the matrix cores (the dense scorer's three-plane products, the query as the A operand;
 * d padded to a multiple of 32 with zero columns), and nothing of size n_queries x N in memory.
 * Total order: a larger logit ranks first; +inf above every finite value, -inf below every finite value, NaN below
 * everything (-0 equals +0); equal logits by candidate index, the smaller first.
 * Candidates of query row q (node u = queries[q], int32 in [0, N)): every v in [0, N) except the columns of row u of the
 * exclusion CSR (ex_rowptr [N+1], ex_col: int32, ascending columns per row; both NULL = nothing excluded) and, when
 * exclude_self != 0, u itself.  fp32 tables Z, H [N][K][d] with 1 <= d <= 128 (dl_score_topk_supported); anything else
 * fails.  Inference only.
 * ws: dl_score_topk_workspace_bytes(N, K, d, n_queries, k, 0) bytes for dl_score_topk and (.., n_queries, 0, n_targets)
 * for dl_score_ranks: the gathered query rows and their planes, the planes of Z and H, and for top-k n_queries x slices
 * lists of k + 64 8-byte keys.  Results are bitwise reproducible and do not depend on the slicing (DL_RANK_SLICES). */
int dl_score_topk_supported(int K, int d);
/* The scan's plan for a problem under the current DL_RANK_SLICES (host only; without the switch the slice count follows
 * the device's CU count, 256 where no device answers).  out[DL_SCORE_TOPK_FORM_LEN] =
 *   [0] 32-column chunks of the padded factor width  [1] query tiles  [2] candidate slices  [3] candidate tiles per slice
 *   [4] tiles of the last slice  [5] keys per (row, slice) list */
#define DL_SCORE_TOPK_FORM_LEN 6
int dl_score_topk_form(int N, int K, int d, int n_queries, int k, int* out);
size_t dl_score_topk_workspace_bytes(int N, int K, int d, int n_queries, int k, int n_targets);
/* Top-k (1 <= k <= 128) per query row: index int64 [n_queries][k], logit and prob = sigmoid(logit) fp32 [n_queries][k],
 * sorted by the total order; a row with fewer than k candidates is padded at the end with index -1 and NaN.  Duplicate
 * query ids are allowed. */
int dl_score_topk(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* queries, int n_queries, int k,
                  const int32_t* ex_rowptr, const int32_t* ex_col, int exclude_self, int64_t* index, float* logit, float* prob,
                  void* ws, size_t ws_bytes, void* stream);
/* Filtered rank counts of target pairs, grouped by query: the targets of query row q are tdst[tptr[q] .. tptr[q+1])
 * (tptr [n_queries+1] int32).  For target i = (u, v), with s_i = s(u, v) as the scan computes it (bit for bit):
 *   greater[i] = #{candidates w != v of row q: s(u, w) ranks strictly above s_i by value}
 *   ties[i]    = #{candidates w != v of row q: s(u, w) has the value of s_i}   (NaN equals NaN, inf equals inf)
 * (int64).  The query node u itself is never a candidate; the target v is never excluded from being ranked even when it is
 * in the exclusion set (the "filtered" protocol).  rank = 1 + greater + ties / 2. */
int dl_score_ranks(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* queries, int n_queries,
                   const int32_t* tptr, const int32_t* tdst, int n_targets, const int32_t* ex_rowptr, const int32_t* ex_col,
                   int64_t* greater, int64_t* ties, void* ws, size_t ws_bytes, void* stream);

/* The graph's m most likely missing links (an extension; the reference has no counterpart): the global top-m of the logit
 * s(u,v) = sum_k (h_k[u].h_k[v]) * exp(z_k[u].z_k[v] / t) over ALL unordered pairs, with nothing of size N x N in memory.
 * Candidates: the unordered pairs {u, v}, 0 <= u < v < N, each considered once; self pairs never.  Pair (u, v) is
 * excluded iff v is among the columns of row u of the exclusion CSR (ex_rowptr [N+1], ex_col: int32, ascending columns
 * per row, the layout dl_score_topk takes; both NULL = nothing excluded).  Only the row of the SMALLER endpoint is looked
 * at: a caller with an unordered set lists every pair in that row (or symmetrises the set).
 * Score: on the matrix cores with the three-plane, six-product scheme of the dense scorer, the rows of the smaller
 * endpoint as the A operand, d padded to a multiple of 32 with zero columns: for every returned pair the logit has the
 * bits dl_score_topk returns for query u, candidate v.
 * Eligible: s >= min_logit.  A NaN logit is never eligible, whatever the floor; min_logit = -inf admits everything else,
 * -inf included.
 * Result: the first min(m, eligible) eligible candidates in dl_score_topk's total order (a larger logit first, +inf
 * above every finite value, -0 equal to +0), equal logits by u N + v, the smaller first: src[i] < dst[i] (int32 [m]),
 * logit[i], prob[i] = sigmoid(logit[i]) (fp32 [m]), sorted; entries i >= count are padded with index -1 and NaN;
 * count[0] = min(m, eligible) (int64, a DEVICE value: the call reads nothing back, never synchronises and never
 * allocates).  Every element of every output array is written on every call.
 * Limits: 1 <= m <= 65536; N <= 46340 (the pair index fits 31 bits, the dense scorer's limit); fp32 tables with
 * 1 <= d <= 128 (dl_score_mine_supported, as dl_score_topk_supported); anything else fails.  N < 2 succeeds with count = 0.
 * Method: a radix select over the 64-bit key (order of the logit, then ~(u N + v)): up to six histogram scans of the
 * tile pairs (u tile <= v tile), one per 10/11-bit digit, each followed by a one-workgroup kernel that picks the digit;
 * a device flag ends the search as soon as the chosen prefix holds exactly the keys still needed, and the remaining
 * histogram scans return at once; one emit scan and a sort of the <= m emitted keys.  Every scan recomputes the logits
 * with the same instruction stream.  Integer atomics only: the outputs are the same bits on every call and do not depend
 * on how the tile pairs are spread over workgroups (DL_MINE_TILES).
 * ws: dl_score_mine_workspace_bytes(N, K, d, m) bytes (0 for arguments out of range): the selection state, a histogram,
 * m 8-byte keys and the planes of Z and H; a missing or short workspace fails with DL_E_WORKSPACE. */
int dl_score_mine_supported(int K, int d);                 /* fp32 tables, 1 <= d <= 128, as dl_score_topk_supported */
/* The launch plan for a problem under the current DL_MINE_TILES (host only; without the switch the run length follows
 * the device's CU count, 256 where no device answers).  out[DL_SCORE_MINE_FORM_LEN] =
 *   [0] 32-column chunks of the padded factor width  [1] 128-row tiles  [2] tile pairs (u tile <= v tile)
 *   [3] tile pairs per workgroup  [4] workgroups of a scan  [5] scans at most (six digits and the emit; 0 for N < 2)
 *   [6] byte offset, from the workspace rounded up to 256 bytes, of the 32-bit count of scans that ran in the last call */
#define DL_SCORE_MINE_FORM_LEN 7
int dl_score_mine_form(int N, int K, int d, int m, int* out);
size_t dl_score_mine_workspace_bytes(int N, int K, int d, int m);
int dl_score_mine(const float* Z, const float* H, int N, int K, int d, float t,
                  const int32_t* ex_rowptr, const int32_t* ex_col,      /* known pairs, both NULL = none */
                  float min_logit, int m,
                  int32_t* src, int32_t* dst, float* logit, float* prob, int64_t* count,
                  void* ws, size_t ws_bytes, void* stream);

/* Global rank counts of target pairs among ALL unordered pairs of the graph (an extension; the reference has no
 * counterpart): where T given pairs stand in the order dl_score_mine lists from the top, with nothing of size N x N in
 * memory and no cap on N other than the tile-pair count (N <= 8,388,480) and N K d < 2^40.  Two calls:
 *
 * dl_score_pair_logits (an extension; the reference has no counterpart): logit[i] = s(a[i], b[i]) for n_pairs given pairs
 * (int32 node ids in [0, N), not checked), row a[i] as the A operand, from the products of the scans: the bits
 * dl_score_topk returns for query a[i], candidate b[i], and dl_score_mine lists for a[i] < b[i] (except that a -0 is
 * written as it is, where those two report +0: their outputs are rebuilt from order keys).  Useful alone: "score these
 * pairs with the bits of the scans".  ws: dl_score_pair_logits_workspace_bytes(N, K, d): the planes of Z and H.
 *
 * dl_score_pair_ranks (an extension; the reference has no counterpart): ONE scan of the tile pairs of dl_score_mine (the
 * same walk, staging, products and exclusion mask: pair (u, v), u < v, is a candidate iff v is not among the columns of
 * row u of the exclusion CSR; NaN logits ARE candidates here).  target_order [n_targets]: the order keys of the target
 * logits, ASCENDING, where the key of x is 0 for NaN and otherwise b ^ 0x80000000 for b >= 0, ~b for b < 0 (b = the bits
 * of x, -0 taken as +0): larger value = larger key, NaN below everything and equal only to NaN.  Every candidate finds
 * lo = the number of target keys strictly below its own (a separator table of <= 4,096 keys in LDS, then a binary search
 * in target_order) and adds 1 to above[lo] (lo > 0) and, if target_order[lo] equals its key, to equal[lo]:
 *   above [n_targets + 1]: candidates strictly above sorted target p = sum of above[p + 1 .. n_targets]
 *   equal [n_targets + 1]: candidates with the key of sorted target p = equal[first place of that key]
 *   n_candidates [1]     : candidates counted = N (N - 1) / 2 - entries (u, v > u) of the exclusion CSR
 * (64-bit DEVICE values; the call zeroes them itself).  A target that is a candidate counts itself once in its equal
 * range: the caller subtracts it.  Integer atomics only: the same bits on every call and under every DL_MINE_TILES.
 * ws: dl_score_pair_ranks_workspace_bytes(N, K, d) (0 for arguments out of range); a short workspace fails with
 * DL_E_WORKSPACE.  No allocation, no synchronisation, no host read; the caller's stream. */
int dl_score_pair_ranks_supported(int K, int d);           /* fp32 tables, 1 <= d <= 128, as dl_score_topk_supported */
/* The launch plan under the current DL_MINE_TILES (host only; an extension, the reference has no counterpart).
 * out[DL_SCORE_PAIR_RANKS_FORM_LEN] =
 *   [0] 32-column chunks of the padded factor width  [1] 128-row tiles  [2] tile pairs  [3] tile pairs per workgroup
 *   [4] workgroups  [5] separators in LDS  [6] targets per separator  [7] search levels in LDS, at most
 *   [8] search levels in global memory, at most */
#define DL_SCORE_PAIR_RANKS_FORM_LEN 9
#define DL_SCORE_PAIR_RANKS_MAX_N 8388480     /* 65,535 tiles of 128 rows: 2,147,450,880 tile pairs, the most an int32 holds */
int dl_score_pair_ranks_form(int N, int K, int d, int n_targets, int* out);
size_t dl_score_pair_logits_workspace_bytes(int N, int K, int d);
size_t dl_score_pair_ranks_workspace_bytes(int N, int K, int d);
int dl_score_pair_logits(const float* Z, const float* H, int N, int K, int d, float t,
                         const int32_t* a, const int32_t* b, int n_pairs, float* logit,
                         void* ws, size_t ws_bytes, void* stream);
int dl_score_pair_ranks(const float* Z, const float* H, int N, int K, int d, float t,
                        const int32_t* ex_rowptr, const int32_t* ex_col,      /* excluded pairs, both NULL = none */
                        const uint32_t* target_order, int n_targets,
                        unsigned long long* above, unsigned long long* equal, unsigned long long* n_candidates,
                        void* ws, size_t ws_bytes, void* stream);

/* dl_score_pair_terms (an extension; the reference has no counterpart): WHY a pair scores as it does — the per-factor terms
 * of s(a[i], b[i]) = sum_k q_k e_k for n_pairs given pairs, from the very pass dl_score_pair_logits runs (same gathers, same
 * products, row a[i] as the A operand), which writes what it holds per factor instead of the final sum alone.  Three fp32
 * arrays [n_pairs][K], row-major; each may be NULL (not wanted), not all three:
 *   e  [i][k] = exp(z_k[a].z_k[b] / t)   the routing weight of factor k
 *   q  [i][k] = h_k[a].h_k[b]            the Gram product of factor k
 *   cum[i][k] = the running sum after factor k has been added: the logit of the tables cut to factors 0..k
 * Bit contract: cum[i][K-1] has the bits dl_score_pair_logits returns for the pair, hence the bits dl_score_topk,
 * dl_score_mine and dl_score_links_fill report for it (with their rule that a -0 is reported as +0: here, as in
 * dl_score_pair_logits, a -0 is written as it is).  The contribution of factor k is cum[i][k] - cum[i][k-1] (cum[i][0] for
 * k = 0); q[i][k] * e[i][k] is the same term before it is rounded into the sum.  A NaN or +-inf in factor k shows in
 * cum[i][k..] exactly as it does in the logit.  Every cell of a non-NULL array is written once, without atomics: the same
 * bits on every call.
 * Limits, supported shapes, codes and the order of the checks are those of dl_score_pair_logits_dtype (node ids in [0, N),
 * not checked; N <= DL_SCORE_PAIR_RANKS_MAX_N; N K d < 2^40; n_pairs <= 2^30; t != 0; a missing or short workspace is
 * DL_E_WORKSPACE); e, q and cum all NULL is DL_E_ARG.  n_pairs = 0 succeeds and launches nothing.
 * ws: dl_score_pair_terms_workspace_bytes(N, K, d) = dl_score_pair_logits_workspace_bytes(N, K, d).  No allocation, no
 * synchronisation, no host read; the caller's stream.  The _dtype forms (DL_BF16: bf16 tables, one plane, one product; the
 * bits of the DL_F32 call on the widened tables) follow the rules of the *_dtype family below. */
size_t dl_score_pair_terms_workspace_bytes(int N, int K, int d);
size_t dl_score_pair_terms_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype);
int dl_score_pair_terms(const float* Z, const float* H, int N, int K, int d, float t,
                        const int32_t* a, const int32_t* b, int n_pairs,
                        float* e, float* q, float* cum,                        /* [n_pairs][K] each; NULL = not wanted */
                        void* ws, size_t ws_bytes, void* stream);
int dl_score_pair_terms_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                              const int32_t* a, const int32_t* b, int n_pairs, float* e, float* q, float* cum,
                              void* ws, size_t ws_bytes, void* stream);

/* A rule on node groups for the four candidate scans above (an extension; the reference has no counterpart): which KINDS of
 * node may be linked, where an exclusion CSR could only list the O(N^2) pairs one by one.
 *   group    [N] uint8, DEVICE: the group of every node, each < n_groups (a precondition: device data is not read back)
 *   n_groups 1..64
 *   allow    [n_groups] uint64, DEVICE: bit h of allow[g] set = a row of group g may take a partner of group h
 * Ordered scans (dl_score_topk_filtered, dl_score_ranks_filtered): the row is the query node, the partner the candidate;
 * allow may be asymmetric.  Unordered scans (dl_score_mine_filtered, dl_score_pair_ranks_filtered): the pair u < v is a
 * candidate iff bit group[v] of allow[group[u]] is set; allow MUST be symmetric (bit h of allow[g] == bit g of allow[h]:
 * a precondition, the rule of a pair would otherwise depend on the numbering of its nodes).
 * The rule combines with the exclusion CSR, exclude_self and min_logit by AND: a candidate passes all of them.  Targets keep
 * their contract: a target is ranked whether or not the rule allows it, and counts as a candidate of the other targets
 * only if allowed and not excluded; n_candidates of dl_score_pair_ranks_filtered counts allowed, non-excluded pairs.
 * The rule enters the scans' 128-bit row masks (group bytes of the candidate tile and the allow table in 768 bytes of
 * LDS); products, logits, order, limits, supported shapes, workspace sizes and the _form functions are those of the
 * unfiltered entries, and results stay independent of DL_RANK_SLICES / DL_MINE_TILES.  Every tile pair is still formed.
 * Each entry takes the arguments of its unfiltered counterpart followed by the filter; NULL = no rule = the unfiltered
 * call.  n_groups outside 1..64 or a NULL member fails with DL_E_ARG.  No allocation, no synchronisation, no host read. */
typedef struct dl_node_filter {
    const uint8_t* group;
    int32_t n_groups;
    const uint64_t* allow;
} dl_node_filter;
int dl_score_topk_filtered(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* queries, int n_queries,
                           int k, const int32_t* ex_rowptr, const int32_t* ex_col, int exclude_self, int64_t* index, float* logit,
                           float* prob, void* ws, size_t ws_bytes, void* stream, const dl_node_filter* filter);
int dl_score_ranks_filtered(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* queries, int n_queries,
                            const int32_t* tptr, const int32_t* tdst, int n_targets, const int32_t* ex_rowptr,
                            const int32_t* ex_col, int64_t* greater, int64_t* ties, void* ws, size_t ws_bytes, void* stream,
                            const dl_node_filter* filter);
int dl_score_mine_filtered(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* ex_rowptr,
                           const int32_t* ex_col, float min_logit, int m, int32_t* src, int32_t* dst, float* logit, float* prob,
                           int64_t* count, void* ws, size_t ws_bytes, void* stream, const dl_node_filter* filter);
int dl_score_pair_ranks_filtered(const float* Z, const float* H, int N, int K, int d, float t, const int32_t* ex_rowptr,
                                 const int32_t* ex_col, const uint32_t* target_order, int n_targets, unsigned long long* above,
                                 unsigned long long* equal, unsigned long long* n_candidates, void* ws, size_t ws_bytes,
                                 void* stream, const dl_node_filter* filter);

/* The rule on the one all-pairs pass that trains, the whole-graph reconstruction loss: the arguments of dl_score_recon_dtype
 * and dl_score_recon_logits followed by the filter.  It is an unordered scan: allow MUST be symmetric.  Included pairs are then
 * the unordered {u, v} with u != v, outside the ignored set, whose bit group[v] of allow[group[u]] is set.  A pair the rule
 * denies behaves exactly like an ignored one, whether it is a positive or not: no loss term, G^ = 0, not counted in
 * counts_out.  The caller takes w_pos = pos_weight / C and w_neg = 1 / C over the pairs that remain (C = positives the rule
 * admits + allowed pairs - ignored allowed pairs - those positives); with nothing included the loss is 0, the gradients are
 * zero and counts_out is (0, 0).  The rule's deny words of a candidate tile go into the scan's ignored mask (768 more bytes of
 * LDS); form and workspace are the unfiltered entries', no tile is skipped (a tile pair the rule denies whole still writes its
 * zeros of G^ and keeps the "zero against E = inf" NaN), and the bits are those of the unfiltered entry given an ignored set
 * that also lists every denied pair: the same on every call, for every block_rows and every DL_RANK_SLICES, and under the
 * DL_BF16 bits rule.  filter == NULL: the launches and bits of the unfiltered entry.  n_groups outside 1..64 or a NULL member
 * fails with DL_E_ARG before any launch.  No float atomics, no allocation, no synchronisation, no host read. */
int dl_score_recon_filtered(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* pos_rowptr,
                            const int32_t* pos_col, const int32_t* ign_rowptr, const int32_t* ign_col, float w_pos, float w_neg,
                            int block_rows, double* loss_out, int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes,
                            void* stream, const dl_node_filter* filter);
int dl_score_recon_logits_filtered(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                                   const int32_t* pos_rowptr, const int32_t* pos_col, const int32_t* ign_rowptr,
                                   const int32_t* ign_col, float w_pos, float w_neg, int block_rows, double* loss_out,
                                   int64_t* counts_out, float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream,
                                   const dl_node_filter* filter);

/* The thresholded link graph (an extension; the reference has no counterpart): EVERY unordered pair whose logit reaches a
 * floor, as a symmetric CSR over all N nodes, with nothing of size N x N in memory and no cap on the number of pairs.
 * Eligible: exactly dl_score_mine's rule without m — u < v < N, v not among the columns of row u of the exclusion CSR
 * (the row of the SMALLER endpoint, as there), allowed by the node filter if one is given (symmetric, NULL = none), and
 * s >= min_logit (a NaN logit is never eligible; -0 reaches a floor of 0).  The logit has the bits dl_score_pair_logits
 * returns for (u, v), the smaller endpoint as the A operand; a -0 is reported as +0.
 * Result: rowptr int64 [N+1], col int32 [nnz], logit / prob fp32 [nnz] (prob = sigmoid(logit)); every eligible pair {u, v}
 * appears as (u, v) and as (v, u) with the same bits, columns within a row strictly ascending; nnz = rowptr[N] = twice the
 * number of eligible pairs, rowptr[r + 1] - rowptr[r] the predicted degree of node r.
 * Two calls with the same arguments, because the caller allocates col / logit / prob between them:
 *   dl_score_links_count: splits the planes of Z and H into the workspace, runs one scan of dl_score_mine's tile pairs that
 *     writes, per node and 128-node tile, the number of eligible partners in that tile (cnt [N][tiles] in the workspace: each
 *     cell is written exactly once, so nothing is zeroed first and nothing is added atomically), turns every row of cnt into
 *     its exclusive prefix and writes rowptr (a DEVICE array; the call reads nothing back).
 *   dl_score_links_fill: one more scan over the workspace the count left (Z and H are not read again: the workspace must be
 *     the same memory, untouched in between), which recomputes the logits with the same instruction stream and writes every
 *     eligible pair at rowptr[u] + cnt[u][tile of v] + its rank in the tile's pass mask, and likewise for (v, u).  nnz is the
 *     length of col / logit / prob (the caller's read of rowptr[N]); a slot >= nnz is not written, so a call that does not
 *     match its count cannot write out of bounds.  prob may be NULL (not wanted); nnz = 0 launches nothing.
 * No atomics on the output path and no dependence on arrival order: the same bits on every call and under every
 * DL_MINE_TILES.
 * Limits: 1 <= N <= 46340 (DL_SCORE_LINKS_MAX_N: the tile-pair walk of dl_score_mine); fp32 tables with 1 <= d <= 128
 * (dl_score_links_supported, as dl_score_mine_supported); anything else fails, as do nnz < 0, NULL tables, a bad filter and
 * a missing or short workspace (DL_E_WORKSPACE).  No allocation, no synchronisation, no host read; the caller's stream.
 * ws: dl_score_links_workspace_bytes(N, K, d) (0 for arguments out of range): the planes of Z and H, cnt (4 N tiles bytes:
 * 60 MB at N = 41,554 against 6.9 GB for an [N,N] fp32 matrix) and the degrees. */
#define DL_SCORE_LINKS_MAX_N 46340
int dl_score_links_supported(int K, int d);                /* fp32 tables, 1 <= d <= 128, as dl_score_mine_supported */
/* The launch plan under the current DL_MINE_TILES (host only).  out[DL_SCORE_LINKS_FORM_LEN] =
 *   [0] 32-column chunks of the padded factor width  [1] 128-row tiles  [2] tile pairs (u tile <= v tile)
 *   [3] tile pairs per workgroup  [4] workgroups of a scan  [5] scans of count + fill (0 for N < 2)  [6] cells of cnt */
#define DL_SCORE_LINKS_FORM_LEN 7
int dl_score_links_form(int N, int K, int d, int* out);
size_t dl_score_links_workspace_bytes(int N, int K, int d);
int dl_score_links_count(const float* Z, const float* H, int N, int K, int d, float t,
                         const int32_t* ex_rowptr, const int32_t* ex_col,      /* known pairs, both NULL = none */
                         float min_logit, const dl_node_filter* filter,        /* NULL = no rule */
                         void* ws, size_t ws_bytes, int64_t* rowptr, void* stream);
int dl_score_links_fill(const float* Z, const float* H, int N, int K, int d, float t,
                        const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit, const dl_node_filter* filter,
                        void* ws, size_t ws_bytes, const int64_t* rowptr, int64_t nnz,
                        int32_t* col, float* logit, float* prob, void* stream);

/* ---- The all-pairs scans over tables of either type.  One entry per launch entry of the family above, with the argument
 * list of its *_filtered form (filter NULL = no rule) and `dtype`, the element type of Z and H, behind d.  DL_F32: exactly
 * the entry above, which is a call of this one.  DL_BF16: Z and H are bf16 [N][K][d].  A bf16 value is its own hi plane
 * (mid = lo = 0), so the scan stages ONE bf16 plane per operand instead of three and issues ONE matrix-core product per
 * K = 16 block instead of six; the plane arrays of the workspace shrink to a third (for mine, pair logits / ranks and links:
 * by exactly 8 K Np dp bytes, Np = N rounded up to 128, dp = d to 32; top-k / ranks also lose the fp32 copy of the gathered
 * query rows).  Nothing else differs: limits, outputs, order, padding, determinism and the launch forms (*_form) are those
 * of the fp32 entries.
 * Bit contract: for finite tables, a DL_BF16 call returns bit for bit what the DL_F32 call returns on the same tables
 * widened to fp32 -- the five products it leaves out add exact zeros to an accumulator that starts at +0.
 * An unknown dtype is DL_E_ARG (the *_workspace_bytes_dtype functions return 0 for it).  dl_score_links_fill_dtype reads the
 * workspace dl_score_links_count_dtype left with the SAME dtype. */
int dl_score_scan_supported(int K, int d, dl_dtype dtype);  /* every scan of the family: 1 <= K <= 64, 1 <= d <= 128 */
size_t dl_score_topk_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype, int n_queries, int k, int n_targets);
size_t dl_score_mine_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype, int m);
size_t dl_score_pair_logits_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype);
size_t dl_score_pair_ranks_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype);
size_t dl_score_links_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype);
int dl_score_topk_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* queries,
                        int n_queries, int k, const int32_t* ex_rowptr, const int32_t* ex_col, int exclude_self, int64_t* index,
                        float* logit, float* prob, void* ws, size_t ws_bytes, void* stream, const dl_node_filter* filter);
int dl_score_ranks_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* queries,
                         int n_queries, const int32_t* tptr, const int32_t* tdst, int n_targets, const int32_t* ex_rowptr,
                         const int32_t* ex_col, int64_t* greater, int64_t* ties, void* ws, size_t ws_bytes, void* stream,
                         const dl_node_filter* filter);
int dl_score_mine_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                        const int32_t* ex_col, float min_logit, int m, int32_t* src, int32_t* dst, float* logit, float* prob,
                        int64_t* count, void* ws, size_t ws_bytes, void* stream, const dl_node_filter* filter);
int dl_score_pair_logits_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* a,
                               const int32_t* b, int n_pairs, float* logit, void* ws, size_t ws_bytes, void* stream);
int dl_score_pair_ranks_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                              const int32_t* ex_col, const uint32_t* target_order, int n_targets, unsigned long long* above,
                              unsigned long long* equal, unsigned long long* n_candidates, void* ws, size_t ws_bytes, void* stream,
                              const dl_node_filter* filter);
int dl_score_links_count_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                               const int32_t* ex_col, float min_logit, const dl_node_filter* filter, void* ws, size_t ws_bytes,
                               int64_t* rowptr, void* stream);
int dl_score_links_fill_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* ex_rowptr,
                              const int32_t* ex_col, float min_logit, const dl_node_filter* filter, void* ws, size_t ws_bytes,
                              const int64_t* rowptr, int64_t nnz, int32_t* col, float* logit, float* prob, void* stream);

/* The budgeted link graph (an extension; the reference has no counterpart): the m most likely unordered pairs of the whole
 * graph, for ANY m, as the symmetric CSR of dl_score_links -- what a caller wants who knows how many links to take ("the
 * 1 % most likely pairs") and not the probability that yields them.  Provided in the _dtype argument convention only.
 * Eligible: dl_score_mine's rule -- u < v < N, v not among the columns of row u of the exclusion CSR (the row of the SMALLER
 * endpoint), allowed by the node filter if one is given (symmetric, NULL = none), s >= min_logit, NaN never.  min_logit and
 * the budget combine by AND: the result holds the min(m, eligible) best eligible pairs.
 * Order: dl_score_mine's -- larger logit first (+inf above everything finite, -0 equal to +0), equal logits by u N + v, the
 * smaller first.  The result is exactly the set dl_score_mine would list if it had no cap on m; a cut through a class of
 * tied logits falls where it puts it.
 * Output: dl_score_links_fill's -- rowptr int64 [N+1], col int32 [nnz], logit / prob fp32 [nnz], every chosen pair as (u, v)
 * and as (v, u) with the same bits, columns within a row strictly ascending, a -0 reported as +0, prob = sigmoid(logit) formed
 * where the logit is in a register, prob NULL allowed.  rowptr[N] = nnz = 2 min(m, eligible).  The CSR is not sorted by
 * logit; it carries the logits, and a caller who wants a list sorts it.
 * Two calls with the same arguments, as for dl_score_links:
 *   dl_score_links_top_count_dtype: splits the planes once, runs dl_score_mine's radix select on the 64-bit key (up to six
 *     histogram scans and one-workgroup picks; once the threshold key is final the remaining histogram scans return at
 *     workgroup start), which leaves the key of the m-th best pair in the workspace, then dl_score_links_count's scan with
 *     one more condition (the pair's key reaches that threshold), the offsets and rowptr.  Neither the emit scan nor the
 *     ordering of dl_score_mine runs, which is why m has no cap.  Nothing is read back between the select and the count.
 *   dl_score_links_top_fill_dtype: dl_score_links_fill's scan under the same condition over the workspace the count left
 *     (the same memory, untouched in between: it holds the threshold, the planes and cnt); a slot >= nnz is not written.
 * m is 64-bit, m >= 1; a value above N (N - 1) / 2 means every eligible pair.
 * Integer atomics appear in the histograms only (counts: their order does not matter); nothing on the output path is atomic
 * or depends on an arrival order, so a call gives the same bits every time and under every DL_MINE_TILES.
 * Limits: 1 <= N <= DL_SCORE_LINKS_MAX_N, d <= 128, fp32 and bf16 tables (dl_score_scan_supported).  Codes, texts and the
 * order of the checks are the links entries': dtype, K and d, N, filter, t, then m >= 1, NULL tables or rowptr, the exclusion
 * pair, the workspace (DL_E_WORKSPACE); the fill then nnz >= 0 and its outputs.  No allocation, no synchronisation, no host
 * read; the caller's stream.
 * ws: dl_score_links_top_workspace_bytes_dtype(N, K, d, dtype) (0 for arguments out of range): dl_score_links' workspace plus
 * the selection state and one histogram of 2,048 counts (8,448 bytes more).
 * The launch plan (host only): out[DL_SCORE_LINKS_TOP_FORM_LEN] = the fields [0..6] of dl_score_links_form with
 *   [5] scans at most: six histogram scans + count + fill (0 for N < 2)
 *   [7] byte offset, inside the 256-byte aligned workspace, of the 32-bit number of histogram scans that ran */
#define DL_SCORE_LINKS_TOP_FORM_LEN 8
int dl_score_links_top_form(int N, int K, int d, int* out);
size_t dl_score_links_top_workspace_bytes_dtype(int N, int K, int d, dl_dtype dtype);
int dl_score_links_top_count_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                                   const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit, int64_t m,
                                   const dl_node_filter* filter, void* ws, size_t ws_bytes, int64_t* rowptr, void* stream);
int dl_score_links_top_fill_dtype(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                                  const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit, int64_t m,
                                  const dl_node_filter* filter, void* ws, size_t ws_bytes, const int64_t* rowptr, int64_t nnz,
                                  int32_t* col, float* logit, float* prob, void* stream);

/* Link scans BETWEEN TWO NODE SETS (an extension; the reference has no counterpart): rows of a table A [nA][K][d] against
 * rows of a table B [nB][K][d] -- users x items, new nodes x old nodes, or block i x block j of one graph past the cap of
 * the triangular walk.  Every tile pair of the ceil(nA/128) x ceil(nB/128) grid is formed, in row-major order, by the
 * kernels of dl_score_mine / dl_score_links in their rectangular form: nA nB candidates cost nA nB products, where the
 * triangular scan of the concatenated table under a node filter costs (nA + nB)^2 / 2.  Provided in the _dtype argument
 * convention only (tables of either type; both tables have the one dtype).
 * Logit: rows of A are the A operand.  The logit of (a, b) has the bits dl_score_pair_logits returns for (a, nA + b) on the
 * table cat(A, B); for blocks i < j of one graph these are the bits the triangular scans form for u < v.
 * Eligible: a < nA, b < nB (no a < b test, no diagonal: the two sets are distinct tables), b not among the columns of row a
 * of the exclusion CSR (BIPARTITE: ex_rowptr int32 [nA+1], columns B-local and strictly ascending; both NULL = none),
 * allowed by the rule if one is given, and s >= min_logit (NaN never; -0 reaches a floor of 0).
 * Rule (dl_node_filter_between, NULL = none): group_a [nA] and group_b [nB] give every row a group below n_groups <= 64;
 * (a, b) is allowed iff bit group_b[b] of allow[group_a[a]] is set.  The row of A decides: the rule need not be symmetric.
 * Nothing past group_a[nA-1] or group_b[nB-1] is read.
 * dl_score_mine_between_dtype: the m best pairs, 1 <= m <= 65536, with dl_score_mine's select (up to six histogram scans,
 *   one emit scan, the ordering) on the key (order of the logit, then a nB + b, the smaller first).  Outputs as dl_score_mine:
 *   src (A-local) / dst (B-local) int32 [m], logit / prob fp32 [m], padded with -1 / NaN, count[0] = min(m, eligible).
 * dl_score_links_between_count_dtype / _fill_dtype: every eligible pair, as TWO CSRs: the A side (rowptr_a int64 [nA+1],
 *   columns = rows of B) and the B side (rowptr_b int64 [nB+1], columns = rows of A).  Every pair appears once in each, with
 *   the same bits, columns strictly ascending, a -0 reported as +0; rowptr_a[nA] = rowptr_b[nB] = the number of pairs.  Two
 *   calls with the same arguments over the same untouched workspace, as for dl_score_links: the count writes, per row and
 *   128-row tile of the other side, the number of eligible partners (cnt_a [nA][tiles of B], cnt_b [nB][tiles of A]; every
 *   cell is written exactly once, zeros included: no memset, no atomics), their prefixes and the two rowptr arrays; the fill
 *   recomputes the logits with the same instruction stream and writes each pair to its slot in both sides.  A slot >= nnz_a
 *   (>= nnz_b) is not written.  prob_a and prob_b may be NULL together (not wanted).
 * Same bits on every call and under every DL_MINE_TILES.  Limits: 1 <= nA, nB <= DL_SCORE_BETWEEN_MAX_N (the pair index
 * a nB + b must fit 31 bits); K, d, t, dtype as for the other scans.  Order of the checks: dtype, K and d, nA, nB, (m,) the
 * rule, t, NULL arguments, the exclusion pair, the workspace (DL_E_WORKSPACE); the fill then nnz >= 0 and its outputs.  No
 * allocation, no synchronisation, no host read, the environment is not read; the caller's stream.
 * ws: the *_workspace_bytes_dtype functions (0 for arguments out of range): the planes of the four tables, and the selection
 * state, one histogram and m keys (mine) or the two cell arrays and the degrees (links).
 * The launch plans under the current DL_MINE_TILES (host only):
 *   out[DL_SCORE_MINE_BETWEEN_FORM_LEN] = [0] 32-column chunks of the padded factor width  [1] tiles of A  [2] tiles of B
 *     [3] tile pairs  [4] tile pairs per workgroup  [5] workgroups of a scan  [6] scans at most (six digits + emit)
 *     [7] byte offset, inside the 256-byte aligned workspace, of the 32-bit number of scans that ran
 *   out[DL_SCORE_LINKS_BETWEEN_FORM_LEN] = [0..5] the same  [6] scans of count + fill  [7] cells of cnt_a  [8] cells of cnt_b */
typedef struct dl_node_filter_between {
    const uint8_t* group_a;
    const uint8_t* group_b;
    int32_t n_groups;
    const uint64_t* allow;
} dl_node_filter_between;
#define DL_SCORE_BETWEEN_MAX_N 46340
#define DL_SCORE_MINE_BETWEEN_FORM_LEN 8
#define DL_SCORE_LINKS_BETWEEN_FORM_LEN 9
int dl_score_mine_between_form(int nA, int nB, int K, int d, int m, int* out);
size_t dl_score_mine_between_workspace_bytes_dtype(int nA, int nB, int K, int d, dl_dtype dtype, int m);
int dl_score_mine_between_dtype(const void* ZA, const void* HA, int nA, const void* ZB, const void* HB, int nB, int K, int d,
                                dl_dtype dtype, float t, const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit, int m,
                                int32_t* src, int32_t* dst, float* logit, float* prob, int64_t* count, void* ws, size_t ws_bytes,
                                void* stream, const dl_node_filter_between* filter);
int dl_score_links_between_form(int nA, int nB, int K, int d, int* out);
size_t dl_score_links_between_workspace_bytes_dtype(int nA, int nB, int K, int d, dl_dtype dtype);
int dl_score_links_between_count_dtype(const void* ZA, const void* HA, int nA, const void* ZB, const void* HB, int nB, int K, int d,
                                       dl_dtype dtype, float t, const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit,
                                       const dl_node_filter_between* filter, void* ws, size_t ws_bytes, int64_t* rowptr_a,
                                       int64_t* rowptr_b, void* stream);
int dl_score_links_between_fill_dtype(const void* ZA, const void* HA, int nA, const void* ZB, const void* HB, int nB, int K, int d,
                                      dl_dtype dtype, float t, const int32_t* ex_rowptr, const int32_t* ex_col, float min_logit,
                                      const dl_node_filter_between* filter, void* ws, size_t ws_bytes, const int64_t* rowptr_a,
                                      const int64_t* rowptr_b, int64_t nnz_a, int32_t* col_a, float* logit_a, float* prob_a,
                                      int64_t nnz_b, int32_t* col_b, float* logit_b, float* prob_b, void* stream);

/* Tie-averaged AUC of a score vector against FIXED labels: replaces sklearn.metrics.roc_auc_score at
 * main_disentangled.py:202-204 / 217-219 (validation AUC every epoch, test AUC at the end).  pos_idx / neg_idx
 * (int64, device) are the positions of the positive and negative labels in score, found once per run; the call
 * writes u2[0] = sum over positives p of ( 2 * #{negatives n: s_n < s_p} + #{n: s_n == s_p} ) as an exact 64-bit
 * integer, so AUC = u2 / (2 * n_pos * n_neg) — the Mann-Whitney statistic with tie-averaged ranks.  One launch:
 * the smaller class is cut into slices of 1,024 scores, a workgroup sorts its slice (bitonic network, shuffles +
 * LDS) and binary-searches its chunk of the other class in it; the counts of the slices add up.  Work grows as
 * ceil(min/1024) * max: dl_auc_pair_counts_supported says whether the sizes are in range (n_pos * n_neg <= 4e11;
 * beyond that a device sort on the caller's side is the better tool).
 * NaN: a NaN score has no rank, so the AUC of a list that holds one is NaN (sklearn raises).  Any NaN among the scores
 * that pos_idx / neg_idx list sets DL_AUC_NAN_MARK (bit 63) in u2[0] — an integer OR from a wavefront that loaded it, in
 * the same launch; counts stay below 2^40, so neither they nor the sums of dl_auc_pair_counts_add carry into it, and the
 * other bits of a marked value mean nothing.  A reader tests the mark (u2 < 0 as int64) before it divides:
 * dl_epoch_finish, metrics.AucPlan and metrics.ShardedAucPlan do.  Without a NaN the count is exact and the mark is
 * clear.  +inf and -inf are ordinary scores (equal to themselves, above / below every finite one). */
#define DL_AUC_NAN_MARK (1ull << 63)
int dl_auc_pair_counts_supported(int n_pos, int n_neg);
int dl_auc_pair_counts(const float* score, const int64_t* pos_idx, int n_pos, const int64_t* neg_idx, int n_neg,
                       unsigned long long* u2, void* stream);
/* The same, ADDING the counts to *u2 instead of overwriting it (no memset in front of the launch): for a caller that keeps
 * *u2 at zero between evaluations — dl_epoch_finish reads and clears it. */
int dl_auc_pair_counts_add(const float* score, const int64_t* pos_idx, int n_pos, const int64_t* neg_idx, int n_neg,
                           unsigned long long* u2, void* stream);
/* The launch geometry of the two calls above for these sizes (both >= 1), host arithmetic only, no GPU work:
 * grid[0] = 1 if the positives are the sliced (sorted) class — they are when n_pos <= n_neg — else 0, grid[1] = slices of
 * 1,024 scores, grid[2] = chunks of the searched class, grid[3] = scores per chunk; slices x chunks workgroups
 * (DL_AUC_TARGET: the number of workgroups aimed at, default 1,024). */
int dl_auc_pair_counts_grid(int n_pos, int n_neg, int* grid);

/* End-of-epoch bookkeeping of the training loop ON THE DEVICE (main_disentangled.py:199-214: loss and validation AUC of
 * the epoch, `if auc > best_auc: best_auc = auc; weights = deepcopy(state_dict); stale = 0 else stale += 1`, patience), in
 * one launch, so that the host need not read anything back before it launches the next epoch:
 *   auc = *u2 / denom2 in double (u2 = the counts of dl_auc_pair_counts[_add], denom2 = 2 n_pos n_neg; NaN if denom2 <= 0
 *   or if *u2 carries DL_AUC_NAN_MARK: `auc > best_auc` is then false, i.e. a stale epoch whose hist / ring entry is NaN);
 *   if !stopped && auc > best_auc: best[i][:] = params[i][:] for the n_bufs <= DL_ADAM_MAX_BUFS buffers (numel[i] floats
 *   each: the weights AFTER the step, like :209), best_auc = auc, stale = 0, best_epoch = epoch;  else stale += 1;
 *   hist[2 epoch] = loss[0], hist[2 epoch + 1] = auc;  epoch += 1;  stale > patience: stopped = 1;  *u2 = 0.
 * Once stopped, or once max_epochs epochs are recorded, the call changes nothing but *u2 = 0 (epochs the host queued
 * before it saw the stop; the tail of a replayed graph that holds several epochs).
 * host_ring (or NULL): PINNED, device-accessible host memory of ring x 4 doubles — slot (epoch mod ring) receives
 *   { loss, auc, epoch + 1, unused } as well, for a host that reads the history behind an event without a copy.
 * state: dl_epoch_state_bytes() bytes owned by the caller, zero-initialised once (best_auc = 0 as at :189):
 *   { double best_auc; int64 stale, epoch, stopped, best_epoch; uint32 internal[2]; }
 * params / best / numel: HOST arrays like dl_adam_step's; loss, u2, hist, state: device memory. */
size_t dl_epoch_state_bytes(void);
int dl_epoch_finish(int n_bufs, const float* const* params, float* const* best, const size_t* numel, const float* loss,
                    unsigned long long* u2, double denom2, void* state, double* hist, long long max_epochs,
                    long long patience, double* host_ring, int ring, void* stream);

/* Pair-list loss of main_disentangled.py:195 and its gradient in one pass:
 *   loss[0] = sum_q w[q] * BCE(prob[q], y[q])       (log clamped at -100, like F.binary_cross_entropy)
 *   g[q]    = w[q] * (prob[q] - y[q]) / max(prob[q] (1 - prob[q]), 1e-12)       = dloss / dprob[q]
 * With w = 1/n_pos on the positive pairs and 1/(m n_neg) on the negative ones this is the reference's
 * BCE(pos) + BCE(neg)/m.  ws: at least 4352 bytes of scratch (1,024 partial sums, added in a fixed order). */
int dl_pair_bce(const float* prob, const float* y, const float* w, int n_pairs, float* loss, float* g,
                void* ws, size_t ws_bytes, void* stream);

/* The optimiser step of the training loop: torch.optim.Adam's update (main_disentangled.py:150 — weight decay added to
 * the gradient, bias-corrected first and second moments) over n_bufs <= DL_ADAM_MAX_BUFS contiguous fp32 buffers in one
 * launch:
 *   g' = g + weight_decay p;  m = m + (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= (lr / (1 - beta1^step)) * m / ( sqrt(v) / sqrt(1 - beta2^step) + eps )
 * params / grads / exp_avg / exp_avg_sq: HOST arrays of n_bufs device pointers, numel: host array of element counts.
 * state: 3 device floats owned by the caller, zero-initialised once: the step counter, the step size lr / (1 - beta1^step)
 * and sqrt(1 - beta2^step) — the call increments the counter ON THE DEVICE first (no host sync; a captured graph replays
 * it).  Hyper-parameters are doubles like torch's (the bias corrections are formed in double).  Same arithmetic as
 * torch's fused Adam up to rounding. */
#define DL_ADAM_MAX_BUFS 8
int dl_adam_step(int n_bufs, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, const size_t* numel, float* state,
                 double lr, double beta1, double beta2, double eps, double weight_decay, void* stream);
/* The same update with the step number counted by the CALLER (step = 1 for the first update): no counter launch in front
 * of the update — for loops that are not replayed from a graph.  The bias corrections are formed on the device with the
 * expressions dl_adam_step uses (the same bits for the same step); state (or NULL) receives {step, step size, sqrt(1 - beta2^step)}. */
int dl_adam_step_at(int n_bufs, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const size_t* numel, float* state, long long step,
                    double lr, double beta1, double beta2, double eps, double weight_decay, void* stream);

/* Backward of dl_score_pairs_fwd (autograd of model.py:109-113 + sigmoid, as triggered at
 * main_disentangled.py:198).  g_prob = dLoss/dprob per pair.  Writes dZ and dH for the plan's rows:
 *   gl = g_prob * prob * (1 - prob);  dH[u] += gl e_k H[v][k];  dZ[u] += gl (q_k e_k)/t Z[v][k]
 * coef: the array dl_score_pairs_fwd filled (n_pairs = inc->n_pairs), or NULL to recompute e and q. */
int dl_score_pairs_bwd(const void* Z, const void* H, int K, int d, dl_dtype dtype, float t,
                       const dl_pair_incidence* inc, const float* prob, const float* g_prob,
                       const float* coef, float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream);

/* Training step of the scorer in ONE pass over the incidence plan: scorer forward (model.py:109-113), the weighted
 * BCE gradient of main_disentangled.py:195 (g = w (p - y) / max(p (1 - p), 1e-12), as dl_pair_bce computes it) and
 * the scorer backward (main_disentangled.py:198) together.  The wave that owns a node's pair slots has the
 * per-factor dot products of every entry, so it forms prob itself and accumulates dZ / dH from the partner rows it
 * just gathered: the partner rows are gathered once per direction (2 x n_pairs x 2 rows) instead of once for the
 * forward plus twice for the backward.  Writes prob[q] for every pair of the plan (for the loss VALUE — call
 * dl_pair_bce on it — and for the validation AUC) and dZ, dH for the plan's rows = d(sum_q w BCE(prob, y)) / d(Z, H).
 * y is any label in [0, 1] and w ANY real weight, negative ones included: the gradients are those of sum_q w BCE with the
 * weight's sign, as dl_score_pairs_fwd / dl_pair_bce / dl_score_pairs_bwd give them, and prob[q] is written whatever w[q]
 * is (every entry of a pair writes it: both form the same bits).  Pairs with w = +-0.0 (validation pairs riding along)
 * contribute exactly nothing to the gradients and are still scored.  A NaN or infinite w[q] reaches the rows of that pair's
 * two endpoints and no other row.  The sign convention of dl_pair_incidence.entry_yw (a negative sign = "the pair's
 * other entry writes prob", the weight is the magnitude) belongs to that stream ALONE: it is read when inc->entry_yw is
 * set, in which case y / w are not read, and it cannot carry a weight with a set sign bit — whoever builds the stream
 * builds it for weights >= +0.0 only and leaves entry_yw NULL otherwise (PairList.bind_labels does).
 * Tuned (K, d) only: dl_score_pairs_train_supported; otherwise use dl_score_pairs_fwd / dl_pair_bce / _bwd. */
int dl_score_pairs_train_supported(const dl_pair_incidence* inc, int K, int d, dl_dtype dtype);
int dl_score_pairs_train(const void* Z, const void* H, int K, int d, dl_dtype dtype, float t,
                         const dl_pair_incidence* inc, const float* y, const float* w,
                         float* prob, float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream);

/* ---- The pair-list objective in LOGIT space (opt-in; the entries above keep the reference's probability space and their
 * bits).  x[q] = sum_k (h_k[u].h_k[v]) * exp(z_k[u].z_k[v] / t) is the value the entries above feed their sigmoid; here it
 * is the score itself, and the loss is the binary cross entropy WITH LOGITS:
 *   loss = sum_q w[q] (max(x, 0) - x y + log1p(exp(-|x|))),      d loss / d x[q] = w[q] (sigma(x[q]) - y[q]).
 * A fp32 probability is exactly 1 from x = 16.64 on and p (1 - p) passes under the 1e-12 clamp below x = -27.6: in
 * probability space such a pair has a zero gradient, a loss pinned at 100 w and a score that ties in the AUC.  In logit space
 * it keeps all three.  sigma(x) - y is formed as (1 - y) sigma(x) - y sigma(-x) from e = exp(-|x|), sigma(|x|) = 1 / (1 + e),
 * sigma(-|x|) = e / (1 + e): either side to < 4 ulp of its own size, so y = 1 gives -sigma(-x), never 1.0 - 1.0.
 * Logit space cures the saturation of the sigmoid, not the overflow of exp: where an exponent e_k overflows, the logit is
 * +-inf (or NaN) and the gradients of that pair are huge, infinite or NaN — in probability space such a pair had gradient 0.
 *
 * dl_score_pairs_logits_fwd: dl_score_pairs_fwd with logit[q] = x[q] out and no stored terms (same arguments otherwise, same
 * checks, same kernels up to the sigmoid).  Bit contracts, where the probability entries have them (fp32 tables, d = 64,
 * K in {4, 8}): the logits are those of dl_score_pairs_train_logits; a hub plan, its residual plan and the plain plan give
 * the same bits; a folded mirrored pair (inc_pair2) stores the same bits under both ids. */
int dl_score_pairs_logits_fwd(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                              const int32_t* pu, const int32_t* pv, int n_pairs,
                              const dl_pair_incidence* by_u, float* logit, void* stream);

/* Backward of dl_score_pairs_logits_fwd, recomputing e and q (dl_score_pairs_bwd with coef = NULL): g_logit = dLoss/dlogit
 * per pair IS the per-entry coefficient,
 *   gl = g_logit;  dH[u] += gl e_k H[v][k];  dZ[u] += gl (q_k e_k)/t Z[v][k].  */
int dl_score_pairs_logits_bwd(const void* Z, const void* H, int K, int d, dl_dtype dtype, float t,
                              const dl_pair_incidence* inc, const float* g_logit,
                              float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream);

/* dl_score_pairs_train in logit space: one pass that writes logit[q] (for every pair of the plan, under the same rules: any
 * real w, signed; the sign-bit writer flag on the entry_yw stream only) and dZ, dH = d(sum_q w BCE-with-logits(x, y)) / d(Z, H) with gl = w (sigma(x) - y), gl = 0 for w == 0, and NO
 * p (1 - p) clamp factor; from gl on it is dl_score_pairs_train (coefficient clamps, accumulation order, partial slots;
 * entry_yw works unchanged).  Same shape rule as dl_score_pairs_train_supported. */
int dl_score_pairs_train_logits_supported(const dl_pair_incidence* inc, int K, int d, dl_dtype dtype);
int dl_score_pairs_train_logits(const void* Z, const void* H, int K, int d, dl_dtype dtype, float t,
                                const dl_pair_incidence* inc, const float* y, const float* w,
                                float* logit, float* dZ, float* dH, void* ws, size_t ws_bytes, void* stream);

/* The loss above and its gradient in one pass, beside dl_pair_bce:
 *   loss[0] = sum_q w[q] (max(x, 0) - x y + log1p(exp(-|x|)))          g[q] = w[q] (sigma(x[q]) - y[q])
 * max(x, 0) - x y is formed as (1 - y) max(x, 0) + y max(-x, 0), a zero factor dropping its term: x = +-inf costs 0 under the
 * agreeing label and inf under the other.  A NaN logit at w = 0 is ignored; at w != 0 it gives a NaN loss.
 * ws: at least 4352 bytes of scratch (the same 1,024 partial sums, added in the same fixed order as dl_pair_bce's). */
int dl_pair_bce_logits(const float* logit, const float* y, const float* w, int n_pairs, float* loss, float* g,
                       void* ws, size_t ws_bytes, void* stream);

/* Backward of aggregate + normaliser + routing softmax (autograd of model.py:56-75; argmax and
 * masks carry no gradient), SURVEY.md Appendix A.3, split at its one global dependency:
 *   phase 1:  dw[e] = (1-beta) dH[i][p].Z[j][p],  dwr[e] = (1-beta) dH[j][p].Z[i][p]  (reverse edge)
 *             ds[i][k] = -(sum_{e in row i, p=k} dwr[e] a[e]) / s~[i][k]^2          (0 where s == 0)
 *   phase 2:  da = dw/s~[j][p] + ds[i][p],  dar = dwr/s~[i][p] + ds[j][p]
 *             dZ[i] (+)= beta dH[i] + sum_e (1-beta) a/s~[i][p] dH[j][p]
 *                                   + sum_e sum_k (da+dar) a ([k==p]-alpha_k)/t Z[j][k]
 * dH and (for phase 2) ds must hold the rows of every neighbour (all-gathered when sharded).
 * dw, dwr are per-entry scratch of the caller ([n_entries] each).
 * dl_route_aggregate_bwd runs both phases back to back (single GPU). */
int dl_route_aggregate_bwd_phase1(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta,
                                  const uint8_t* p, const float* a, const float* s, const float* dH,
                                  float* dw, float* dwr, float* ds, void* ws, size_t ws_bytes, void* stream);
int dl_route_aggregate_bwd_phase2(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta, float t,
                                  const uint8_t* p, const float* a, const float* s, const float* dH,
                                  const float* dw, const float* dwr, const float* ds,
                                  float* dZ, int accumulate, void* ws, size_t ws_bytes, void* stream);
int dl_route_aggregate_bwd(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta, float t,
                           const uint8_t* p, const float* a, const float* s,
                           const float* dH, float* dZ, int accumulate,
                           void* ws, size_t ws_bytes, void* stream);

/* dZ = scale[0] * (dZ_in + the backward above applied to dH): dl_route_aggregate_bwd with the accumulated input read
 * from its own array (dZ_in: NULL = 0, may be dZ itself) and the result multiplied by a DEVICE scalar (scale: NULL = 1).
 * For a caller whose incoming gradients are g * dH and g * dZ_in with g = d(total)/d(loss) known only on the device
 * (autograd of main_disentangled.py:198 through a fused loss): the backward is linear, so the two scaling passes over
 * [N,K,d] arrays and their copies disappear.  scale[0] == 1 gives the bits of dl_route_aggregate_bwd. */
int dl_route_aggregate_bwd_scaled(const dl_graph* g, const void* Z, int K, int d, dl_dtype dtype, float beta, float t,
                                  const uint8_t* p, const float* a, const float* s,
                                  const float* dH, const float* dZ_in, const float* scale, float* dZ,
                                  void* ws, size_t ws_bytes, void* stream);

/* ---- Fresh training negatives every epoch, drawn and trained on the device (opt-in; nothing above changes).
 *
 * dl_sample_negatives: for entry e = r m + j (r < n_rows, j < m) draw a partner k uniformly over [0, N) such that
 * (src[r], k) is not in the exclusion CSR (ex_rowptr [N+1], ex_col ascending per row: the normal form the scans read;
 * both NULL = nothing excluded) and, with exclude_self != 0, k != src[r] — the rule of the fixed split's structured
 * negatives: an edge row of the whole dataset is never a negative.
 * Randomness is counter-based: Philox4x32-10 with key = (seed low, seed high) and counter = (e, attempt, epoch low, epoch
 * high); k = (uint64(word 0) * N) >> 32.  The draw is a pure function of (seed, epoch, e): no dependence on the grid, the wave
 * order or the call.  Bias of the map: a value receives floor or ceil of 2^32 / N of the 2^32 words, i.e. at most N / 2^32
 * relative to uniform.  epoch_dev: ONE uint64 in device memory, read by the kernel (a loop advances it with a device add; no
 * host value changes between epochs).
 * At most 64 attempts per entry: an entry that exhausts them writes k = -1 and adds 1 to *n_failed (device uint32, an integer
 * atomic; the caller zeroes it); the trainers below give such an entry weight 0.  A src[r] outside [0, N) fails likewise.
 * Duplicated draws inside an epoch are KEPT as separate entries: nothing is de-duplicated (the fixed split does).
 * One thread per entry, no LDS, no workspace, no host read, no synchronisation; the caller's stream. */
int dl_sample_negatives(const int32_t* src, int n_rows, int m, int N, const int32_t* ex_rowptr, const int32_t* ex_col,
                        uint64_t seed, const uint64_t* epoch_dev, int exclude_self, int32_t* k_out, uint32_t* n_failed,
                        void* stream);

/* dl_sample_negatives_hard: hard negatives (dynamic negative sampling) — c candidates per entry instead of one, the one
 * the caller's CURRENT tables score highest is kept.  Entry e = r m + j has 1 <= c <= 64 candidates; candidate i is drawn by the
 * rule of dl_sample_negatives (at most 64 attempts, rejection against the exclusion row of src[r], and of k == src[r] with
 * exclude_self) with the Philox counter (e, i 64 + attempt, epoch low, epoch high), key = seed: candidate 0 is, bit for bit,
 * the draw dl_sample_negatives makes for e, and c = 1 is that sampler.  A candidate that spends its attempts is dead.
 * k_out[e] = the live candidate with the largest logit x(u, k) = sum_f (h_f[u].h_f[k]) exp(z_f[u].z_f[k] / t), taken in fp32
 * from Z, H [N][K][d]; ties go to the lowest i; a NaN logit ranks below every number, -inf included, and if every live
 * candidate's logit is NaN the first live one is kept.  All c dead, or src[r] outside [0, N) (never read): k_out[e] = -1 and
 * ONE count in *n_failed (entries, not candidates; device uint32, the caller zeroes it).  Duplicated candidates are legal.
 * x_out (may be NULL): the kept candidate's logit, 0 where k_out[e] = -1 — the bits dl_score_sampled_bpr_train writes to
 * neg_logit for the same (u, k) at the same shape (d = 64 with K in {4, 8}: its register form; otherwise its generic order).
 * The result is a pure function of (seed, epoch, e, Z, H, t): the same bits on every call, whatever the grid.  One wave per
 * floor(64 / c) consecutive entries, one lane per candidate for the draw, then a serial walk that gathers the rows of each live
 * candidate (c E 2 K d 4 bytes gathered in all); no LDS, no workspace, no float atomics, no host read, no synchronisation; the
 * one atomic is the integer n_failed.  fp32 tables with 1 <= K <= 64 and K d <= 2048 (dl_sample_negatives_hard_supported);
 * bf16 tables are refused.  src ascending is not required for the result, only for the reuse of the loaded u rows. */
int dl_sample_negatives_hard_supported(int K, int d, dl_dtype dtype);
int dl_sample_negatives_hard(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t, const int32_t* src,
                             int n_rows, int m, int c, const int32_t* ex_rowptr, const int32_t* ex_col, uint64_t seed,
                             const uint64_t* epoch_dev, int exclude_self, int32_t* k_out, float* x_out, uint32_t* n_failed,
                             void* stream);

/* dl_score_sampled_train: the outputs of dl_score_pairs_train for the n_rows m entries (u_e, k_e), u_e = src[e / m], label 0
 * and ONE weight w, without a plan:
 *   score[e] = sigmoid(x_e) (_logits: x_e),  x_e = sum_f (h_f[u].h_f[k]) exp(z_f[u].z_f[k] / t);   0 for an entry with k = -1;
 *   loss[0]  = sum_e -w max(log(1 - score), -100)          (_logits: sum_e w (max(x, 0) + log1p(exp(-|x|))));
 *   dZ, dH [N][K][d] = d loss / d (Z, H) with g = w (p - 0) under dl_pair_bce's max(p (1 - p), 1e-12) clamp (_logits:
 *   g = w sigma(x), no clamp), every pair in both endpoints' rows; accumulate != 0 adds onto dZ / dH instead (another list's
 *   gradients and these then sum without a launch of their own).  EVERY row of dZ / dH is written: a node no entry names reads
 *   exactly 0.  w = 0 and k = -1 contribute exactly nothing.  k == u is legal.
 * src ascending; u_rowptr [N+1]: the CSR of the u side in ENTRIES (u_rowptr[n] = m x the number of src values < n);
 * order [E]: the STABLE ascending sort of k over the entries (the -1 entries first); k_rowptr [N+1]: k_rowptr[n] = the number
 * of entries with k < n (so k_rowptr[0] = the failed draws, k_rowptr[N] = E).  Both are the caller's to compute on the device.
 * Two passes over chunks of 64 list positions (row side, then partner side through 2K stored coefficients per entry), partial
 * slots where a row spans chunks, one finishing launch that adds partner side first, then row side: fixed orders throughout,
 * no float atomics, no host read, no synchronisation; the same bits on every call.  fp32 tables with 1 <= K <= 64 and
 * K d <= 2048 (dl_score_sampled_train_supported; d = 64 with K in {4, 8} has its own kernels, whose scores are the bits of
 * dl_score_pairs_train's); bf16 tables are refused.  ws: dl_score_sampled_train_workspace_bytes(n_rows m, N, K, d). */
int dl_score_sampled_train_supported(int K, int d, dl_dtype dtype);
size_t dl_score_sampled_train_workspace_bytes(int n_entries, int N, int K, int d);
int dl_score_sampled_train(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                           const int32_t* src, int n_rows, int m, const int32_t* u_rowptr, const int32_t* k,
                           const int32_t* order, const int32_t* k_rowptr, float w, float* score, float* loss,
                           float* dZ, float* dH, int accumulate, void* ws, size_t ws_bytes, void* stream);
int dl_score_sampled_train_logits_supported(int K, int d, dl_dtype dtype);
size_t dl_score_sampled_train_logits_workspace_bytes(int n_entries, int N, int K, int d);
int dl_score_sampled_train_logits(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                                  const int32_t* src, int n_rows, int m, const int32_t* u_rowptr, const int32_t* k,
                                  const int32_t* order, const int32_t* k_rowptr, float w, float* score, float* loss,
                                  float* dZ, float* dH, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* dl_score_sampled_bpr_train: the pairwise ranking loss (BPR) on the sampled negatives, in logit space, without a plan.  Edge
 * row r < n_rows has the positive (u_r, v_r) = (src[r], dst[r]) and the m entries e = r m + j with partners k[e] (-1 = a failed
 * draw: no term).  With x(a, b) the logit of dl_score_sampled_train_logits and delta_rj = x(u_r, k_rj) - x(u_r, v_r) (in fp32):
 *   pos_logit[r] = x(u_r, v_r) (written for EVERY row, also one whose draws all failed);   neg_logit[e] = x(u_r, k_e), 0 for k = -1;
 *   loss[0] = sum_{r, j live} w (max(delta, 0) + log1p(exp(-|delta|)));
 *   dZ, dH [N][K][d] = d loss / d (Z, H) with g_rj = w sigma(delta_rj) on the negative's logit and -G_r = -sum_j g_rj (ascending
 *   j) on the positive's, per-factor coefficients and finite clamps as in dl_score_sampled_train_logits, every pair in both
 *   endpoints' rows; accumulate != 0 adds onto dZ / dH.  EVERY row of dZ / dH is written: a node no list names reads exactly
 *   0.  w = 0, k = -1 and a row without a live draw contribute exactly nothing.  k == v, k == u and v == u are legal;
 *   duplicated draws are separate terms.  An overflowed exp is not cured: inf - inf is NaN and stays NaN.
 * Preconditions: src ascending; u_rowptr [N+1] the CSR of the u side in ENTRIES (u_rowptr[n] = m x the number of src values
 * < n); dst_order [n_rows] the STABLE ascending sort of dst over the rows and dst_rowptr [N+1], dst_rowptr[n] = the number of
 * rows with dst < n (fixed for the run); order [n_rows m] / k_rowptr [N+1] the epoch's, as for dl_score_sampled_train.  An
 * endpoint outside [0, N) makes its row no term (logits 0).  1 <= m <= 63 (a chunk of the row pass is floor(64 / (m + 1))
 * whole rows; larger m is refused), n_rows m <= (2^31 - 1) / (2 K), and n_rows m, N K d each below 2^31.
 * Row pass over chunks of whole rows, two partner passes over chunks of 64 list positions (k side, positives' partner side)
 * through 2K stored coefficients per pair, partial slots where a node spans chunks, one finishing launch that adds k side,
 * then positives' partner side, then row side; the loss through 1,024 partial sums: fixed orders throughout, no float
 * atomics, no host read, no synchronisation; the same bits on every call.  fp32 tables with 1 <= K <= 64 and K d <= 2048
 * (dl_score_sampled_bpr_train_supported; d = 64 with K in {4, 8} has its own kernels, whose logits are the bits of
 * dl_score_sampled_train_logits'); bf16 tables are refused.  ws: dl_score_sampled_bpr_train_workspace_bytes(n_rows, m, N, K, d)
 * (0 for arguments the entry refuses). */
int dl_score_sampled_bpr_train_supported(int K, int d, dl_dtype dtype);
size_t dl_score_sampled_bpr_train_workspace_bytes(int n_rows, int m, int N, int K, int d);
int dl_score_sampled_bpr_train(const void* Z, const void* H, int N, int K, int d, dl_dtype dtype, float t,
                               const int32_t* src, const int32_t* dst, int n_rows, int m, const int32_t* u_rowptr,
                               const int32_t* dst_order, const int32_t* dst_rowptr, const int32_t* k, const int32_t* order,
                               const int32_t* k_rowptr, float w, float* pos_logit, float* neg_logit, float* loss,
                               float* dZ, float* dH, int accumulate, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISENLINK_HIP_H */
