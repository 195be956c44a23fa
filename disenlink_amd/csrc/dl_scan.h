// What the all-pairs scans share (dl_score_dense.hip, dl_score_rank.hip, dl_score_mine.hip): the arithmetic of a pipeline
// step, the order keys of the logits, the walk of a row's excluded columns, and the host scaffolding of a scan (workspace
// carving, the launch of a kernel with more than 64 KiB of dynamic LDS, with or without a node-group rule).  Internal:
// only things that more than one scan uses live here; what belongs to one mode stays in its unit.
#pragma once
#include "dl_common.h"
#include "dl_tiles.h"

namespace dl {
namespace scan {

using namespace project;

typedef unsigned long long u64;

// ---- a pipeline step (after the products of gram_block<P>, dl_tiles.h) ---------------------------------------------
// P = planes per operand: 3 for fp32 tables, 1 for bf16 tables (the instantiations the *_dtype entries launch with DL_BF16).
// Everything after the products (factor_update, the masks, every epilogue) does not know P.
// The operand of a wave in step s: row `row` of the LDS plane image [2][P][128][SPLIT_PITCH] the step reads (A: row =
// 32 wu + lane % 32 of the u image, B: 64 wv + lane % 32 of the v image), lane half h at k = 8h .. 8h + 7 of a block.
template <int P = 3>
__device__ __forceinline__ const __bf16* gram_operand(const __bf16* image, int s, int row, int half) {
    return image + (s & 1) * P * PLANE_ROWS * SPLIT_PITCH + row * SPLIT_PITCH + half * 8;
}

// Step r of a factor's 2 nd steps is over: S = z.z complete (r = nd - 1) gives e = exp(S / t), Q = h.h complete
// (r = 2 nd - 1) gives term += Q * e; either way the accumulators start the next product from zero.
__device__ __forceinline__ void factor_update(f32x16 (&acc)[2], float (&e)[2][16], f32x16 (&term)[2], int r, int nd, float t) {
    if (r == nd - 1) {
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
            for (int q = 0; q < 16; ++q) e[bb][q] = expf(div_t(acc[bb][q], t));
            zero_acc(acc[bb]);
        }
    } else if (r == 2 * nd - 1) {
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
            for (int q = 0; q < 16; ++q) term[bb][q] += acc[bb][q] * e[bb][q];
            zero_acc(acc[bb]);
        }
    }
}

// ---- keys ----------------------------------------------------------------------------------------------------------
// Total order of the logits as an unsigned key: NaN -> 0, every other value (-0 taken as +0) to its order-preserving
// image, which is >= 0x007FFFFF (-inf) and <= 0xFF800000 (+inf).
__device__ __forceinline__ unsigned ord_key(float x) {
    if (x != x) return 0u;
    const unsigned b = __float_as_uint(x == 0.0f ? 0.0f : x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_value(unsigned o) {
    if (o == 0u) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
// 64-bit selection key: the value's order, then an index (candidate v, or pair u N + v; smaller index = larger key).  Never 0.
__device__ __forceinline__ u64 make_key(float x, unsigned index) { return ((u64)ord_key(x) << 32) | (u64)(0xFFFFFFFFu - index); }

// ---- exclusion CSR (ascending columns per row) ---------------------------------------------------------------------
// first entry of ex_col[lo, hi) whose column is >= v (hi if none)
__device__ __forceinline__ int first_col_at_least(const int32_t* __restrict__ ex_col, int lo, int hi, int v) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ex_col[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// ORs the columns [v0, v0 + 128) of ex_col[c, end) into the 4-word mask m; returns the cursor: the first entry past them
__device__ __forceinline__ int exclusion_mask(const int32_t* __restrict__ ex_col, int c, int end, int v0, unsigned* m) {
    for (; c < end; ++c) {
        const int col = ex_col[c] - v0;
        if (col >= PLANE_ROWS) break;
        m[col >> 5] |= 1u << (col & 31);
    }
    return c;
}

// ---- host ----------------------------------------------------------------------------------------------------------
inline int device_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, c = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
            n = c;
        if (n <= 0) n = 256;
    }
    return n;
}

// A workspace as consecutive blocks, each rounded up to 256 bytes, behind the 256-byte aligned start of ws; bytes() is what
// the blocks taken so far need, the slack for aligning ws included.  ws = NULL: sizes only.
struct Carver {
    char* base;
    size_t o = 0;
    explicit Carver(void* ws) : base((char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255)) {}
    template <class T>
    T* take(size_t count) {
        T* r = (T*)(base + o);
        o += (sizeof(T) * count + 255) & ~(size_t)255;
        return r;
    }
    size_t bytes() const { return o + 256; }
};

// The node-group rule as the kernels take it (NULL: none)
inline FilterArgs filter_args(const dl_node_filter* nf) {
    return nf != nullptr ? FilterArgs{nf->group, (const u64*)nf->allow, nf->n_groups} : FilterArgs{nullptr, nullptr, 0};
}

// Launch of a kernel with more than 64 KiB of dynamic LDS; the devices whose limit is raised are kept per instantiation.
template <auto KERNEL, class... Args>
inline void launch_lds(unsigned grid, int threads, size_t lds, hipStream_t st, const Args&... args) {
    static unsigned long long done = 0;
    ensure_dynamic_lds(reinterpret_cast<const void*>(KERNEL), lds, done);
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(threads), lds, st, args...);
}
// The tables of a scan as its one-plane or three-plane arrays: dst = K matrices of plane_array_elems<P>(N, d, 32) elements.
// DL_BF16 tables are copied (rows != NULL: gathered), DL_F32 tables split; a gather of fp32 rows is the caller's.
inline void table_planes(const void* T, dl_dtype dt, const int32_t* rows, int R, int K, int d, __bf16* dst, hipStream_t st) {
    if (dt == DL_BF16) copy_rows((const __bf16*)T, rows, K, R, d, K * d, (size_t)d, dst, st);
    else split_rows((const float*)T, K, R, d, K * d, (size_t)d, dst, st);
}
inline size_t table_plane_elems(dl_dtype dt, size_t rows, size_t cols) {
    return dt == DL_BF16 ? plane_array_elems<1>(rows, cols, SPLIT_COLS) : plane_array_elems<3>(rows, cols, SPLIT_COLS);
}

// ... of a scan in its plain or, under a node-group rule, its FILT instantiation (which keeps FILTER_LDS_BYTES behind `lds`)
template <auto PLAIN, auto FILTERED, class Args>
inline void launch_scan(const dl_node_filter* nf, unsigned grid, int threads, size_t lds, hipStream_t st, const Args& a) {
    if (nf != nullptr) launch_lds<FILTERED>(grid, threads, lds + FILTER_LDS_BYTES, st, a);
    else launch_lds<PLAIN>(grid, threads, lds, st, a);
}

}  // namespace scan
}  // namespace dl
