// What vc_gene_glm.hip and vc_gene_glm_batch.hip share, statement for statement: the per-element arithmetic of the harmonic regression
// (eta in float64 from the float32 tables, mu = 2^n 2^f with one v_exp_f32, residual, weight and NB logarithm in float32, float64
// per-lane sums), the fold of the workgroup (shuffle tree, waves in wave order through the LDS) and the packed float64 Cholesky algebra.
// The contract of every piece is the one written at the head of vc_gene_glm.hip.
#pragma once

#include "vc_common.h"

// every product-sum is written as the fma it is meant to be; nothing else may be contracted (the same operations in every instantiation)
#pragma clang fp contract(off)

namespace {

constexpr int GLM_NW = 4;                 // waves per workgroup
constexpr int GLM_NT = GLM_NW * 64;
constexpr int GLM_MAX_HALVINGS = 30;
constexpr double GLM_EPS32 = 1.1920928955078125e-07;
constexpr double GLM_LOG2E = 1.4426950408889634;
constexpr double GLM_BOUND = 50.0;

template <bool U16>
__device__ __forceinline__ float glm_count(const void* row, long long c) {
  if (U16) return (float)((const unsigned short*)row)[c];
  return ((const float*)row)[c];
}

// acc[i] := the sum of acc[i] over the workgroup, in every lane: shuffle tree over the wave, then the waves in wave order
template <int N>
__device__ __forceinline__ void glm_fold(double (&acc)[N], double (*part)[N], double* tot, int lane, int wave) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = acc[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double s = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < GLM_NW; ++w) s += part[w][threadIdx.x];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = tot[i];
}

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
  for (long long c = c0 + threadIdx.x; c < c1; c += GLM_NT) {
    const float k = glm_count<U16>(row, c);
    double b[K];
    b[0] = 1.0;
#pragma unroll
    for (int i = 1; i < K; ++i) b[i] = (double)B[(long long)i * Nc + c];
    double eta = (double)logm[c] + nu[0];
#pragma unroll
    for (int i = 1; i < K; ++i) eta = __builtin_fma(nu[i], b[i], eta);
    // mu = 2^n 2^f: the fraction is exact in float64 and rounds once to float32; beyond 2^120 the step is refused by its objective
    double t = eta * GLM_LOG2E;
    t = t > 120.0 ? 120.0 : (t < -140.0 ? -140.0 : t);
    const double tn = __builtin_rint(t);
    const float mu = __builtin_ldexpf(__builtin_amdgcn_exp2f((float)(t - tn)), (int)tn);
    const double kd = (double)k;
    float res, w;
    double term, mag;
    if (NOISE == VC_NOISE_NB) {
      const float s = r + mu;
      const float rs = __builtin_amdgcn_rcpf(s);
      const float p = r * rs;                                       // r / (r + mu)
      res = (k - mu) * p;
      w = (mu * rs) * p * (k + r);
      // ln(r + mu) = max(eta, ln r) + ln(1 + x), x = min(mu, r) / max(mu, r): the large part is exact in float64, the float32
      // logarithm is taken of a number in [1, 2], so d and w lose nothing to the size of eta (counts of 10^4: (k + r) ln(r + mu) ~ 10^5)
      const bool big = mu >= r;
      const float x = (big ? r : mu) * __builtin_amdgcn_rcpf(big ? mu : r);
      const double lg = (double)(VC_LN2 * __builtin_amdgcn_logf(1.f + x));
      const double e = eta - lnr;
      const double d = big ? -lg : e - lg;                          // eta - ln(r + mu)
      const double wl = big ? e + lg : lg;                          // ln(r + mu) - ln r
      const double ls = (big ? eta : lnr) + lg;
      const double kr = (double)(k + r);
      term = __builtin_fma(kd, d, -(double)r * wl);
      mag = __builtin_fma(kr, __builtin_fabs(ls), __builtin_fabs(kd * eta));
    } else {
      res = k - mu;
      w = mu;
      term = __builtin_fma(kd, eta, -(double)mu);
      mag = __builtin_fabs(kd * eta) + (double)mu;
    }
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

}  // namespace
