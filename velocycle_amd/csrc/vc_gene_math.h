// What the four stand-alone per-gene solvers (vc_gene_glm, vc_gene_glm_batch, vc_gene_dispersion, vc_gene_kinetics) share, statement
// for statement.  Device: the count load, mu = 2^n 2^f with one v_exp_f32, the Poisson / negative-binomial element in float32 with
// float64 terms, and the fold of the workgroup (shuffle tree, waves in wave order through the LDS).  Host: the refusals the entry
// points make with the same words, the error message and the check after the launch.  The bit-for-bit contracts between the solvers
// (two kernels on one problem, glm and dispersion alternating on the same mu) hold because each of these is written here once.
// The basis row and eta (b[0] = 1, b[i] = B[i][c]; eta = logm_c + nu[0], then one fma per harmonic) are NOT here: glm_sweep, dsp_mu
// and kin_cell write the same statements, and moving them into a function changes the instructions emitted for vc_gene_glm
// (every instantiation) and vc_gene_kinetics (NW = 3), though not the operations.
#pragma once

#include <string>

#include "vc_common.h"

void vc_set_global_error(const char* msg);      // vc_engine.hip: the message vc_last_error(NULL) returns

// every product-sum is written as the fma it is meant to be; nothing else may be contracted (the same operations in every instantiation)
#pragma clang fp contract(off)

namespace {

constexpr int GENE_NW = 4;                // waves per workgroup
constexpr int GENE_NT = GENE_NW * 64;
constexpr double GENE_EPS32 = 1.1920928955078125e-07;
constexpr double GENE_LOG2E = 1.4426950408889634;

template <bool U16>
__device__ __forceinline__ float gene_count(const void* row, long long c) {
  if (U16) return (float)((const unsigned short*)row)[c];
  return ((const float*)row)[c];
}

// acc[i] := the sum of acc[i] over the workgroup, in every lane: shuffle tree over the wave, then the waves in wave order.  part has
// GENE_NW rows of STRIDE numbers.  No barrier follows the last read of tot: whoever writes part / tot again places one
template <int N, int STRIDE = N>
__device__ __forceinline__ void gene_fold(double (&acc)[N], double (*part)[STRIDE], double* tot, int lane, int wave) {
  static_assert(N <= STRIDE, "the LDS rows are too short");
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
    for (int w = 1; w < GENE_NW; ++w) s += part[w][threadIdx.x];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = tot[i];
}

// e^eta = 2^n 2^f: the fraction is exact in float64 and rounds once to float32, so the result carries one rounding whatever |eta|;
// beyond 2^120 a step is refused by its objective
__device__ __forceinline__ float gene_exp_f32(double eta) {
  double t = eta * GENE_LOG2E;
  t = t > 120.0 ? 120.0 : (t < -140.0 ? -140.0 : t);
  const double tn = __builtin_rint(t);
  return __builtin_ldexpf(__builtin_amdgcn_exp2f((float)(t - tn)), (int)tn);
}

// One count k against the mean mu = e^eta: the residual res, the Fisher weight w, the observed weight wo, the term of the objective
// and its magnitude.    res = k - mu | (k - mu) r / (r + mu)     w = mu | mu r / (r + mu)     wo = mu | mu r (k + r) / (r + mu)^2
template <int NOISE>
__device__ __forceinline__ void gene_lik(float k, float mu, double eta, float r, double lnr, float& res, float& w, float& wo, double& term,
                                         double& mag) {
  const double kd = (double)k;
  if (NOISE == VC_NOISE_NB) {
    const float s = r + mu;
    const float rs = __builtin_amdgcn_rcpf(s);
    const float p = r * rs;                                         // r / (r + mu)
    res = (k - mu) * p;
    w = mu * p;
    wo = (mu * rs) * p * (k + r);
    // ln(r + mu) = max(eta, ln r) + ln(1 + x), x = min(mu, r) / max(mu, r): the large part is exact in float64, the float32
    // logarithm is taken of a number in [1, 2], so d and wl lose nothing to the size of eta (counts of 10^4: (k + r) ln(r + mu) ~ 10^5)
    const bool big = mu >= r;
    const float x = (big ? r : mu) * __builtin_amdgcn_rcpf(big ? mu : r);
    const double lg = (double)(VC_LN2 * __builtin_amdgcn_logf(1.f + x));
    const double e = eta - lnr;
    const double d = big ? -lg : e - lg;                            // eta - ln(r + mu)
    const double wl = big ? e + lg : lg;                            // ln(r + mu) - ln r
    const double ls = (big ? eta : lnr) + lg;
    const double kr = (double)(k + r);
    term = __builtin_fma(kd, d, -(double)r * wl);
    mag = __builtin_fma(kr, __builtin_fabs(ls), __builtin_fabs(kd * eta));
  } else {
    res = k - mu;
    w = mu;
    wo = mu;
    term = __builtin_fma(kd, eta, -(double)mu);
    mag = __builtin_fabs(kd * eta) + (double)mu;
  }
}

// ---- host: what the four extern "C" entry points share ----

// sets "<fn>: <text>" as the message of vc_last_error(NULL)
inline int gene_fail(const char* fn, int code, const char* text) {
  try { vc_set_global_error((std::string(fn) + ": " + text).c_str()); } catch (...) {}
  return code;
}

constexpr int GENE_NO_NOISE = -1;         // vc_gene_dispersion: the noise is not an argument

// The refusals every entry point makes with the same words, in the order they have always been made.  What only the entry point
// knows travels in: own = its verdict on K (and NW), null where they pass; nc_limited = Nc is held to 2^31 - 1 like Ng;
// min_iter = the least max_iter (0: a call may only evaluate).  VC_OK: nothing is refused so far
inline int gene_refuse(const char* fn, int noise, int count_kind, const char* own, int64_t Ng, int64_t Nc, bool nc_limited,
                       int64_t gene_stride, int min_iter, int max_iter, double tol) {
  if (noise != GENE_NO_NOISE) {
    if (noise == VC_NOISE_LOGNORMAL) return gene_fail(fn, VC_ERR_UNSUPPORTED, "Lognormal noise is not implemented (Poisson or NegativeBinomial)");
    if (noise != VC_NOISE_NB && noise != VC_NOISE_POISSON) return gene_fail(fn, VC_ERR_ARG, "noise must be VC_NOISE_POISSON or VC_NOISE_NB");
  }
  if (count_kind != VC_COUNTS_F32 && count_kind != VC_COUNTS_U16) return gene_fail(fn, VC_ERR_ARG, "count_kind must be VC_COUNTS_F32 or VC_COUNTS_U16");
  if (own) return gene_fail(fn, VC_ERR_ARG, own);
  if (Ng < 1 || Nc < 1) return gene_fail(fn, VC_ERR_ARG, "Ng and Nc must be >= 1");
  if (Ng > 0x7fffffffLL || (nc_limited && Nc > 0x7fffffffLL))
    return gene_fail(fn, VC_ERR_ARG, nc_limited ? "more than 2^31 - 1 genes or cells in one call" : "more than 2^31 - 1 genes in one call");
  if (gene_stride < Nc) return gene_fail(fn, VC_ERR_ARG, "gene_stride < Nc");
  if (max_iter < min_iter) return gene_fail(fn, VC_ERR_ARG, min_iter > 0 ? "max_iter must be >= 1" : "max_iter must be >= 0");
  if (!(tol >= 0.0)) return gene_fail(fn, VC_ERR_ARG, "tol must be >= 0");
  return VC_OK;
}

// after the launch: VC_OK, or VC_ERR_HIP with the runtime's words
inline int gene_launched(const char* fn) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return VC_OK;
  try { gene_fail(fn, VC_ERR_HIP, (std::string("launch failed: ") + hipGetErrorString(err)).c_str()); } catch (...) {}
  return VC_ERR_HIP;
}

}  // namespace
