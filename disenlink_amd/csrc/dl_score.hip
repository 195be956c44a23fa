// Pair scorer, dense gather-form scorer and separate scorer backward in probability space (the kernels: dl_score.h).
// (one of the tuned-kernel translation units; the shared pieces and the design notes are in dl_fast.h)
#include "dl_score.h"

namespace dl {

int fast_score_pairs_fwd(const dl_pair_incidence* by_u, const void* Z, const void* H, int K, int d, int dtype,
                         float t, float* prob, float* coef, hipStream_t st) {
#define X_F32(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, float>::score_fwd(by_u, Z, H, t, prob, coef, st);
#define X_BF16(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, fast::bf16_t>::score_fwd(by_u, Z, H, t, prob, coef, st);
    DL_DISPATCH(X)
#undef X_F32
#undef X_BF16
}

int fast_score_pairs_bwd(const dl_pair_incidence* inc, const void* Z, const void* H, int K, int d, int dtype,
                         float t, const float* prob, const float* g_prob, const float* coef, float* dZ, float* dH,
                         float* part, hipStream_t st) {
#define X_F32(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, float>::score_bwd(inc, Z, H, t, prob, g_prob, coef, dZ, dH, part, st);
#define X_BF16(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, fast::bf16_t>::score_bwd(inc, Z, H, t, prob, g_prob, coef, dZ, dH, part, st);
    DL_DISPATCH(X)
#undef X_F32
#undef X_BF16
}

int fast_score_allpairs_fwd(const void* Z, const void* H, int N, int K, int d, int dtype, float t, float* prob,
                            hipStream_t st) {
#define X_F32(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, float>::score_allpairs(Z, H, N, t, prob, st);
#define X_BF16(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, fast::bf16_t>::score_allpairs(Z, H, N, t, prob, st);
    DL_DISPATCH(X)
#undef X_F32
#undef X_BF16
}

void fast_score_allpairs_form(int N, int K, int d, int dtype, int* out) {
    const fast::AllpairsGeo g = fast::allpairs_geo(N, (size_t)K * d * (dtype == DL_BF16 ? sizeof(fast::bf16_t) : sizeof(float)));
    out[1] = (int)g.items;
    out[2] = (int)g.blocks;
    out[3] = g.n_slices;
    out[4] = g.slice_w;
    out[5] = g.chunks_per_u;
}

}  // namespace dl
