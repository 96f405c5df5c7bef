// What vc_gene_glm.hip and vc_gene_glm_batch.hip share, statement for statement, beyond what every per-gene solver shares
// (vc_gene_math.h: the count load, mu = 2^n 2^f, the likelihood element, the fold): the sums of the harmonic regression per element
// (eta in float64 from the float32 tables, float64 per-lane sums of the float32 residual and weight against the float64 basis row),
// the prior of a coefficient and the packed float64 Cholesky algebra.  The contract of every piece is the one written at the head
// of vc_gene_glm.hip.
#pragma once

#include "vc_gene_math.h"

// every product-sum is written as the fma it is meant to be; nothing else may be contracted (the same operations in every instantiation)
#pragma clang fp contract(off)

namespace {

constexpr int GLM_MAX_HALVINGS = 30;
constexpr double GLM_BOUND = 50.0;

// index of (i, j), j <= i, in the packed lower triangle
__device__ __host__ constexpr int glm_tri(int i, int j) { return i * (i + 1) / 2 + j; }

template <int H>
struct GlmSums {
  static constexpr int K = 2 * H + 1;
  static constexpr int NH = K * (K + 1) / 2;
  static constexpr int OFF_H = K, OFF_L = K + NH, OFF_A = OFF_L + 1, OFF_N = OFF_A + 1, N = OFF_N + K;
};

// The cells c0 + threadIdx.x, c0 + threadIdx.x + 256, ... < c1 of the gene's row at nu, added to this lane's
// acc = [g (K) | H packed (NH) | L | A | N (K)]; nu[0] is whatever constant the cells of [c0, c1) share
template <int H, int NOISE, bool U16>
__device__ __forceinline__ void glm_sweep(const void* __restrict__ row, long long c0, long long c1, long long Nc,
                                          const float* __restrict__ B, const float* __restrict__ logm, float r, double lnr,
                                          const double (&nu)[2 * H + 1], double (&acc)[GlmSums<H>::N]) {
  typedef GlmSums<H> S;
  constexpr int K = S::K;
  for (long long c = c0 + threadIdx.x; c < c1; c += GENE_NT) {
    const float k = gene_count<U16>(row, c);
    double b[K];
    b[0] = 1.0;
#pragma unroll
    for (int i = 1; i < K; ++i) b[i] = (double)B[(long long)i * Nc + c];
    double eta = (double)logm[c] + nu[0];
#pragma unroll
    for (int i = 1; i < K; ++i) eta = __builtin_fma(nu[i], b[i], eta);
    const float mu = gene_exp_f32(eta);
    float res, wf, w;                                               // the Hessian is the observed one: the Fisher weight wf is not used
    double term, mag;
    gene_lik<NOISE>(k, mu, eta, r, lnr, res, wf, w, term, mag);
    const double rd = (double)res, wd = (double)w;
    const double n2 = __builtin_fma(wd, wd, rd * rd);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      acc[i] = __builtin_fma(rd, b[i], acc[i]);
      const double wb = wd * b[i];
#pragma unroll
      for (int j = 0; j <= i; ++j) acc[S::OFF_H + glm_tri(i, j)] = __builtin_fma(wb, b[j], acc[S::OFF_H + glm_tri(i, j)]);
      acc[S::OFF_N + i] = __builtin_fma(n2, b[i] * b[i], acc[S::OFF_N + i]);
    }
    acc[S::OFF_L] += term;
    acc[S::OFF_A] += mag;
  }
}

// In-place Cholesky of the packed lower triangle (float64); false if a pivot is not a positive finite number
template <int K>
__device__ __forceinline__ bool glm_chol(double (&a)[K * (K + 1) / 2]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    double d = a[glm_tri(j, j)];
#pragma unroll
    for (int q = 0; q < j; ++q) d = __builtin_fma(-a[glm_tri(j, q)], a[glm_tri(j, q)], d);
    ok = ok && d > 0.0 && d < 1.0e300;
    const double l = __builtin_sqrt(ok ? d : 1.0);
    a[glm_tri(j, j)] = l;
    const double il = 1.0 / l;
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      double s = a[glm_tri(i, j)];
#pragma unroll
      for (int q = 0; q < j; ++q) s = __builtin_fma(-a[glm_tri(i, q)], a[glm_tri(j, q)], s);
      a[glm_tri(i, j)] = s * il;
    }
  }
  return ok;
}

// x := (L L')^-1 x
template <int K>
__device__ __forceinline__ void glm_solve(const double (&l)[K * (K + 1) / 2], double (&x)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double s = x[i];
#pragma unroll
    for (int q = 0; q < i; ++q) s = __builtin_fma(-l[glm_tri(i, q)], x[q], s);
    x[i] = s / l[glm_tri(i, i)];
  }
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
    double s = x[i];
#pragma unroll
    for (int q = i + 1; q < K; ++q) s = __builtin_fma(-l[glm_tri(q, i)], x[q], s);
    x[i] = s / l[glm_tri(i, i)];
  }
}

// The prior of one coefficient (at = g K + i): it has one where its mean is finite and its precision a positive finite number
__device__ __forceinline__ void glm_prior(const double* prior_mean, const double* prior_prec, long long at, double& pm, double& pp) {
  pm = 0.0;
  pp = 0.0;
  if (prior_mean) {
    const double m = prior_mean[at], p = prior_prec[at];
    if (__builtin_fabs(m) < 1.0e300 && p > 0.0 && p < 1.0e300) { pm = m; pp = p; }
  }
}

}  // namespace
