// The likelihood of one observed count under one draw, shared by the kernels that score observed counts: the pointwise predictive
// density (vc_pointwise.hip) and the predictive PIT (vc_pit.hip).  The log2 bracket of the log-probability and the lookup of its lgamma
// constant in the engine's per-gene count histogram.  Like vc_draw_model.h they rely on the including translation unit's `#pragma clang fp contract(off)`.
#pragma once
#include "vc_common.h"

// log-probability / ln 2 without its lgamma constant.  eta2 = eta log2 e;  NB: r log2 r + k eta2 - (r + k) log2(r + mu)
template <int NOISE>
__device__ __forceinline__ float pw_lik(float k, float eta2, float r, float rl2) {
  const float mu = __builtin_amdgcn_exp2f(eta2);
  if (NOISE == VC_NOISE_NB) {
    const float L = __builtin_amdgcn_logf(r + mu);
    return __builtin_fmaf(-(r + k), L, __builtin_fmaf(k, eta2, rl2));
  }
  return __builtin_fmaf(k, eta2, -(mu * VC_LOG2E));
}

// the lgamma constant of (matrix, gene, count): the histogram entry of that count.  `a`: the launch's arguments with h_ptr (CSR
// [2 Ng + 1]), h_val (ascending within a gene), h_lgc (lgamma(r + k) - lgamma(r) - lgamma(k + 1), or -lgamma(k + 1), per entry) and Ng
template <class Args>
__device__ __forceinline__ double pw_const(const Args& a, int mat, int g, float k) {
  if (k == 0.f) return 0.0;
  int lo = a.h_ptr[(size_t)mat * a.Ng + g], hi = a.h_ptr[(size_t)mat * a.Ng + g + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float v = a.h_val[mid];
    if (v == k) return a.h_lgc[mid];
    if (v < k) lo = mid + 1; else hi = mid;
  }
  return __builtin_nan("");                  // a count the histogram does not list: cannot happen on a finalized engine
}
