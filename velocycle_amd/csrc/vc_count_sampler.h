// Exact count samplers on the device: k ~ Poisson(mu) and k ~ GammaPoisson(r, r / mu), the reference's negative binomial
// (velocity_inference_model.py:385-386, phase_inference_model.py).  Used by vc_sample_counts and vc_predictive_check (vc_ppc.hip).
//
// A sample is a pure function of (seed, draw, matrix, element index, eta, r): every random word comes from the Philox4x32-10 block
//   counter = (index low, index high, draw, matrix << 16 | stage << 8 | attempt),   key = (seed low, seed high)
// stage 0: the gamma variate, stage 1: the Poisson variate; attempt a of a rejection loop takes block a.  Nothing depends on the
// launch shape, on chunking or sharding, on the order of the cells in storage or on the storage type of the counts.
// A word w becomes the uniform u = ((w >> 9) + 0.5) 2^-23 in [2^-24, 1 - 2^-24]: the top 23 bits, so that n + 0.5 fits float32's 24-bit
// significand and u is exact in float32 (never 0, never 1) and equal to the checker's float64 value.
//
// Algorithms (DESIGN.md section 5 has the same text with its reasons):
//   gamma(r)     Marsaglia-Tsang (2000), d = r' - 1/3, c = 1 / sqrt(9 d), r' = r + 1 for r < 1 and the result times u^(1/r) then.
//                Per attempt one block: words 0, 1 -> a normal by Marsaglia's polar method (rejected outside the unit disc),
//                word 2 -> the acceptance uniform, word 3 -> the boost uniform.  lambda = gamma mu / r.
//   lambda < 10  inversion by sequential search from k = 0 (p_0 = e^-lambda, p_k = p_(k-1) lambda / k), at most 96 terms; a uniform
//                above the float32 sum of those terms (a rounding event of probability ~1e-7) is redrawn from the next block.
//   lambda >= 10 Hoermann's PTRS (1993), transformed rejection with squeeze; words 0, 1 of the attempt's block.  log k! by the
//                Stirling series to 1 / (1260 x^5) on x >= 8 (smaller arguments shifted up by the recurrence).  The full acceptance
//                test (only the attempts that pass neither the squeeze nor the quick reject reach it) is evaluated in float64.
// Every loop is bounded by VC_CS_ATTEMPTS; running out of attempts, a lambda that is not finite or lies above VC_CS_MU_MAX returns
// VC_CS_FAIL (-1) and the caller latches a status: a made-up value is never returned.
//
// The arithmetic is float32 with one rounding per written operation (no contraction), IEEE division and square root; the only
// hardware approximations are v_exp_f32 and v_log_f32.  The exception is PTRS's full test ln(V invalpha / (al / us^2 + b)) <=
// k ln lam - lam - ln k!: float64 (the library's log) from the float32 V, us, k, lam and constants, because its right-hand side is
// the difference of two terms of ~1.4e7 at lam = 1e6 where a float32 ulp is 1.  tests/ppc_checker.py restates the same operations
// in numpy.
#pragma once
#include "vc_common.h"

#define VC_CS_MU_MAX 1048576.f      // 2^20: supported range of the Poisson rate (after the gamma mixing)
#define VC_CS_SMALL 10.f            // inversion below, PTRS from here on
#define VC_CS_KCAP 96               // terms of the sequential search
#define VC_CS_ATTEMPTS 64           // blocks per rejection loop
#define VC_CS_FAIL (-1)

#pragma clang fp contract(off)

__device__ __forceinline__ float vc_cs_uniform(uint32_t w) { return ((float)(w >> 9) + 0.5f) * (1.0f / 8388608.0f); }
__device__ __forceinline__ float vc_cs_ln(float x) { return VC_LN2 * __builtin_amdgcn_logf(x); }

__device__ __forceinline__ void vc_cs_block(uint64_t seed, uint64_t idx, uint32_t draw, uint32_t mat, uint32_t stage, uint32_t attempt,
                                            uint32_t w[4]) {
  vc_philox((uint32_t)idx, (uint32_t)(idx >> 32), draw, (mat << 16) | (stage << 8) | attempt, (uint32_t)seed, (uint32_t)(seed >> 32), w);
}

// log(k!) = lgamma(k + 1), k >= 0 an integer, in float64 (PTRS's full test: see vc_cs_poisson)
__device__ __forceinline__ double vc_cs_lfact(double k) {
  double x = k + 1.0, corr = 0.0;
  if (x < 8.0) {
    double pr = x;
#pragma unroll
    for (int j = 1; j < 8; ++j) pr = pr * (x + (double)j);
    corr = log(pr);
    x = x + 8.0;
  }
  const double inv = 1.0 / x, inv2 = inv * inv;
  const double ser = inv * (0.083333333333333333 - inv2 * (0.0027777777777777778 - inv2 * 0.00079365079365079365));
  return (((x - 0.5) * log(x) - x) + 0.91893853320467274) + (ser - corr);
}

// gamma(r, 1) variate, r > 0; < 0: out of attempts
__device__ __forceinline__ float vc_cs_gamma(uint64_t seed, uint64_t idx, uint32_t draw, uint32_t mat, float r) {
  const bool boost = r < 1.f;
  const float rr = boost ? r + 1.f : r;
  const float d = rr - 0.33333333333333333f;
  const float c = 1.f / __builtin_sqrtf(9.f * d);
#pragma unroll 1
  for (uint32_t a = 0; a < VC_CS_ATTEMPTS; ++a) {
    uint32_t w[4];
    vc_cs_block(seed, idx, draw, mat, 0u, a, w);
    const float v1 = 2.f * vc_cs_uniform(w[0]) - 1.f, v2 = 2.f * vc_cs_uniform(w[1]) - 1.f;
    const float s = v1 * v1 + v2 * v2;
    if (!(s < 1.f)) continue;
    const float x = v1 * __builtin_sqrtf((-2.f * vc_cs_ln(s)) / s);
    const float v = 1.f + c * x;
    if (!(v > 0.f)) continue;
    const float v3 = (v * v) * v;
    const float lhs = vc_cs_ln(vc_cs_uniform(w[2]));
    const float rhs = ((0.5f * (x * x) + d) - d * v3) + d * vc_cs_ln(v3);
    if (lhs < rhs) {
      float g = d * v3;
      if (boost) g = g * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(vc_cs_uniform(w[3])) / r);
      return g;
    }
  }
  return -1.f;
}

// Poisson(lam) variate, 0 <= lam <= VC_CS_MU_MAX; VC_CS_FAIL otherwise or out of attempts
__device__ __forceinline__ int vc_cs_poisson(uint64_t seed, uint64_t idx, uint32_t draw, uint32_t mat, float lam) {
  if (!(lam >= 0.f && lam <= VC_CS_MU_MAX)) return VC_CS_FAIL;
  if (lam < VC_CS_SMALL) {
    const float p0 = __builtin_amdgcn_exp2f(-(lam * VC_LOG2E));
#pragma unroll 1
    for (uint32_t a = 0; a < VC_CS_ATTEMPTS; ++a) {
      uint32_t w[4];
      vc_cs_block(seed, idx, draw, mat, 1u, a, w);
      const float u = vc_cs_uniform(w[0]);
      float p = p0, s = p0;
      int k = 0;
#pragma unroll 1
      while (u > s && k < VC_CS_KCAP) {
        ++k;
        p = (p * lam) / (float)k;
        s = s + p;
      }
      if (u <= s) return k;
    }
    return VC_CS_FAIL;
  }
  const float slam = __builtin_sqrtf(lam);
  const double loglam = log((double)lam);
  const float b = 0.931f + 2.53f * slam;
  const float al = -0.059f + 0.02483f * b;
  const float invalpha = 1.1239f + 1.1328f / (b - 3.4f);
  const float vr = 0.9277f - 3.6224f / (b - 2.f);
#pragma unroll 1
  for (uint32_t a = 0; a < VC_CS_ATTEMPTS; ++a) {
    uint32_t w[4];
    vc_cs_block(seed, idx, draw, mat, 1u, a, w);
    const float U = vc_cs_uniform(w[0]) - 0.5f, V = vc_cs_uniform(w[1]);
    const float us = 0.5f - __builtin_fabsf(U);
    const float kf = __builtin_floorf((((2.f * al) / us + b) * U + lam) + 0.43f);
    if (us >= 0.07f && V <= vr) return (int)kf;
    if (kf < 0.f || (us < 0.013f && V > us)) continue;
    // the full test, in float64 from the float32 V, us, kf, lam and constants: k ln lam - lam and ln k! are ~1.4e7 at lam = 1e6 and
    // their difference is a log-probability of order -1 .. -10, lost entirely to float32's ulp of 1 there
    const double usd = (double)us;
    const double lhs = log(((double)V * (double)invalpha) / ((double)al / (usd * usd) + (double)b));
    const double rhs = ((double)kf * loglam - (double)lam) - vc_cs_lfact((double)kf);
    if (lhs <= rhs) return (int)kf;
  }
  return VC_CS_FAIL;
}

// one count from eta2 = eta log2 e (the units vc_pointwise.hip evaluates eta in); nb: r = 1 / shape_inv > 0, else Poisson
__device__ __forceinline__ int vc_cs_count(uint64_t seed, uint64_t idx, uint32_t draw, uint32_t mat, float eta2, float r, bool nb) {
  const float mu = __builtin_amdgcn_exp2f(eta2);
  float lam = mu;
  if (nb) {
    if (!(r > 0.f)) return VC_CS_FAIL;
    const float g = vc_cs_gamma(seed, idx, draw, mat, r);
    if (g < 0.f) return VC_CS_FAIL;
    lam = (g * mu) / r;
  }
  return vc_cs_poisson(seed, idx, draw, mat, lam);
}
