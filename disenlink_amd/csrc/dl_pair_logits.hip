// The pair-list objective in LOGIT space (include/disenlink_hip.h): the logit forms of the forward scorer, of the one-pass training
// scorer and of the recompute backward — the LOGIT instantiations of the kernels of dl_score.h, dl_train.h and dl_score_bwd.h, in
// a translation unit of their own (the probability forms keep their instruction streams).  The loss kernel is dl_train.hip's.
#include "dl_score.h"
#include "dl_train.h"

namespace dl {

// the logit-space objective: `logit` receives the logits, dZ / dH are the gradients of sum_q w BCE-with-logits(logit, y)
int fast_score_pairs_train_logits(const dl_pair_incidence* inc, const void* Z, const void* H, int K, int d, int dtype, float t,
                                  const float* y, const float* w, float* logit, float* dZ, float* dH, float* part, hipStream_t st) {
    return score_pairs_train_space<true>(inc, Z, H, K, d, dtype, t, y, w, logit, dZ, dH, part, st);
}


// the logit-space entries: the forward without stored terms with logits out, the recompute backward from d loss / d logit
int fast_score_pairs_logits_fwd(const dl_pair_incidence* by_u, const void* Z, const void* H, int K, int d, int dtype,
                                float t, float* logit, hipStream_t st) {
#define X_F32(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, float>::template score_fwd<true>(by_u, Z, H, t, logit, nullptr, st);
#define X_BF16(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, fast::bf16_t>::template score_fwd<true>(by_u, Z, H, t, logit, nullptr, st);
    DL_DISPATCH(X)
#undef X_F32
#undef X_BF16
}

int fast_score_pairs_logits_bwd(const dl_pair_incidence* inc, const void* Z, const void* H, int K, int d, int dtype,
                                float t, const float* g_logit, float* dZ, float* dH, float* part, hipStream_t st) {
#define X_F32(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, float>::template score_bwd<true>(inc, Z, H, t, nullptr, g_logit, nullptr, dZ, dH, part, st);
#define X_BF16(KK, DD) if (K == KK && d == DD) return fast::ScoreOps<KK, DD, fast::bf16_t>::template score_bwd<true>(inc, Z, H, t, nullptr, g_logit, nullptr, dZ, dH, part, st);
    DL_DISPATCH(X)
#undef X_F32
#undef X_BF16
}

}  // namespace dl
