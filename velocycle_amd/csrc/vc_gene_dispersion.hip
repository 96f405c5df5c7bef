// Per-gene negative-binomial dispersion with the means known: vc_gene_dispersion of include/velocycle_hip.h, the third factor of the
// model of Phases.from_cycle_mle / vc_gene_glm (the reference fits it only inside the SVI, as shape_inv).  Stand-alone like vc_gene_glm:
// no engine, no workspace, one launch; the whole one-parameter iteration of a gene runs inside its workgroup.
//
// Per gene g, eta_c = nu . B[:, c] + logm_c, mu = exp(eta), r = e^rho = 1 / dispersion:
//   L(rho)  = sum_c lgamma(k + r) - lgamma(r) + k (eta - ln(r + mu)) - r (ln(r + mu) - ln r)       (+ sum_c -lgamma(k + 1): the log-likelihood)
//   f(rho)  = L(rho) - (alpha - 1) rho - beta e^-rho                                               (optional prior shape_inv ~ Gamma(alpha, beta))
//   s = dL/dr    = sum_c psi(k + r) - psi(r) - log1p(mu / r) + (mu - k) / (r + mu)
//   h = d2L/dr2  = sum_c psi'(k + r) - psi'(r) + 1 / r - 1 / (r + mu) - (mu - k) / (r + mu)^2
//   f' = r s - (alpha - 1) + beta / r,   f'' = r^2 h + r s - beta / r
//
// Mapping: one workgroup of GENE_NW waves per gene, lanes walk the row with stride 256 (gene_count, as in vc_gene_glm).  mu is formed
// as glm_sweep forms it (eta float64 by the same statements, mu = gene_exp_f32(eta): 2^n 2^f with one float32 exp2), so both kernels
// see the same mu; it is the only float32 number here.  Everything that depends on r is float64.  Sums: per-lane float64 accumulators,
// the shuffle tree, the waves in wave order through the LDS (gene_fold) -- no float atomics, identical bits on repetition.
//
// Gamma terms: counts are integers, so  sum_c psi(k + r) - psi(r) = sum_{j >= 0} N_{>j} / (r + j),  N_{>j} = #{c: k_c > j}  (lgamma: the
// same with ln(r + j), psi': with -1 / (r + j)^2).  The first walk over the row builds the counts' histogram below DSP_T in the LDS with
// integer atomics (order-independent), a workgroup scan turns it into N_{>j}; a pass then spends at most DSP_T float64 terms over 256
// lanes on the gamma part (N_{>j} is non-increasing: a lane stops at its first 0) and the cell loop keeps log1p and two divisions per
// element.  A cell with k >= DSP_T adds psi(k + r) - psi(r + DSP_T) and its siblings from Stirling's series at arguments >= DSP_T,
// the leading differences written so that they do not cancel (log1p((k - T) / (r + T)), (k - T) / ((r + T)(r + k))).
//
// Iteration over rho in [VC_DISP_RHO_MIN, VC_DISP_RHO_MAX] (status codes: velocycle_hip.h); after the fold every lane holds the same
// totals, so the control flow is uniform:
//   noise    4 eps32 sqrt(sum_c [r mu (k - mu) / (r + mu)^2]^2)  +  64 eps64 r sum_c |parts of s|
//   bounds   f'(hi) > -noise -> AT_UPPER;  else f'(lo) < noise -> AT_LOWER
//   start    r_start, or sum mu^2 / sum((k - mu)^2 - mu) (hi if the denominator is <= 0), clipped; a start that is not strictly inside
//            the bracket (lo, hi) is replaced by its midpoint (both ends have just been evaluated)
//   at rho   f'' < 0 and f'^2 / -f'' <= tol -> CONVERGED;  |f'| <= noise -> ROUNDING;  steps == max_iter -> MAX_ITER
//   step     the sign of f' shrinks the bracket; rho' = rho - f' / f'' if f'' < 0 and rho' lies strictly inside, else the midpoint
//   max_iter == 0: one pass at r_start -> EVALUATED.  A nu that is not finite -> NO_DATA, NaN outputs.
#include "vc_gene_math.h"                         // gene_count, gene_exp_f32, gene_fold and the entry point's refusals: shared by the per-gene solvers

// every product-sum is written as the fma it is meant to be; nothing else may be contracted (the same operations in every instantiation)
#pragma clang fp contract(off)

namespace {

constexpr int DSP_T = 1024;               // counts below it go through the histogram (why 1024)
constexpr int DSP_PER = DSP_T / GENE_NT;  // histogram entries per lane in the scan
constexpr double DSP_EPS64 = 2.220446049250313e-16;
constexpr int DSP_L = 0, DSP_S = 1, DSP_H = 2, DSP_N = 3, DSP_P = 4, DSP_NACC = 5;

// eta (float64) and mu (one float32 rounding) of cell c: glm_sweep's statements and its gene_exp_f32, so that both kernels see the same mu
template <int K>
__device__ __forceinline__ float dsp_mu(const float* __restrict__ B, const float* __restrict__ logm, long long Nc, long long c,
                                        const double (&nu)[K], double& eta_out) {
  double b[K];
  b[0] = 1.0;
#pragma unroll
  for (int i = 1; i < K; ++i) b[i] = (double)B[(long long)i * Nc + c];
  double eta = (double)logm[c] + nu[0];
#pragma unroll
  for (int i = 1; i < K; ++i) eta = __builtin_fma(nu[i], b[i], eta);
  eta_out = eta;
  return gene_exp_f32(eta);
}

struct DspPoint {
  double L, fp, fpp, noise;
};

// One pass over the gene at r (lnr = ln r): L, f', f'' and the noise of f', the same in every lane
template <int H, bool U16>
__device__ __forceinline__ DspPoint dsp_pass(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                             const float* __restrict__ logm, const double (&nu)[2 * H + 1], double r, double lnr,
                                             double pa, double pb, const unsigned* ngt, double (*part)[DSP_NACC], double* tot, int lane,
                                             int wave) {
  double acc[DSP_NACC];
#pragma unroll
  for (int i = 0; i < DSP_NACC; ++i) acc[i] = 0.0;
  const double ir = 1.0 / r;
  // the gamma terms of every count below DSP_T (and of the first DSP_T factors of the larger ones)
  for (int j = threadIdx.x; j < DSP_T; j += GENE_NT) {
    const unsigned n = ngt[j];
    if (n == 0) break;
    const double x = r + (double)j, ix = 1.0 / x, nd = (double)n;
    const double p = nd * ix;
    acc[DSP_L] = __builtin_fma(nd, log(x), acc[DSP_L]);
    acc[DSP_S] += p;
    acc[DSP_H] = __builtin_fma(-p, ix, acc[DSP_H]);
    acc[DSP_P] += p;
  }
  const double x0 = r + (double)DSP_T, i0 = 1.0 / x0, lnx0 = log(x0);
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float k = gene_count<U16>(row, c);
    double eta;
    const double md = (double)dsp_mu<2 * H + 1>(B, logm, Nc, c, nu, eta);
    const double kd = (double)k;
    const double rs = 1.0 / (r + md);
    // ln(r + mu) = max(eta, ln r) + log1p(x), x = min(mu, r) / max(mu, r), as in vc_gene_glm: eta stands for ln mu, so that the rounding
    // of mu reaches d = eta - ln(r + mu) and w = ln(r + mu) - ln r only through x
    const bool big = md >= r;
    const double lg = log1p((big ? r : md) / (big ? md : r));
    const double e = eta - lnr;
    const double d = big ? -lg : e - lg;
    const double wl = big ? e + lg : lg;
    const double q = (md - kd) * rs;
    double term = __builtin_fma(kd, d, -r * wl);
    double sc = q - wl;
    double hc = md * rs * ir - q * rs;                               // 1 / r - 1 / (r + mu) = mu / (r (r + mu))
    double mag = __builtin_fabs(wl) + __builtin_fabs(q);
    if (k >= (float)DSP_T) {
      // lgamma, psi, psi' at x1 = r + k minus the same at x0 = r + T (both >= T: Stirling's series, its next term < 1e-24)
      const double dk = kd - (double)DSP_T, x1 = x0 + dk, i1 = 1.0 / x1;
      const double lp = log1p(dk * i0);
      const double a2 = i0 * i0, b2 = i1 * i1;
      const double a3 = a2 * i0, b3 = b2 * i1, a4 = a2 * a2, b4 = b2 * b2;
      const double dlg = __builtin_fma(dk, lnx0, __builtin_fma(x1 - 0.5, lp, -dk)) + (i1 - i0) * (1.0 / 12.0) -
                         (b3 - a3) * (1.0 / 360.0) + (b4 * i1 - a4 * i0) * (1.0 / 1260.0);
      const double cross = dk * (x0 + x1) * a2 * b2;                 // 1 / x0^2 - 1 / x1^2
      const double dps = lp + 0.5 * dk * i0 * i1 + cross * (1.0 / 12.0) + (b4 - a4) * (1.0 / 120.0) - (b4 * b2 - a4 * a2) * (1.0 / 252.0);
      const double dtg = -dk * i0 * i1 - 0.5 * cross + (b3 - a3) * (1.0 / 6.0) - (b4 * i1 - a4 * i0) * (1.0 / 30.0) +
                         (b4 * b3 - a4 * a3) * (1.0 / 42.0);
      term += dlg;
      sc += dps;
      hc += dtg;
      mag += dps;
    }
    const double nz = r * md * q * rs;
    acc[DSP_L] += term;
    acc[DSP_S] += sc;
    acc[DSP_H] += hc;
    acc[DSP_N] = __builtin_fma(nz, nz, acc[DSP_N]);
    acc[DSP_P] += mag;
  }
  gene_fold<DSP_NACC>(acc, part, tot, lane, wave);
  __syncthreads();                                                   // part / tot are written again by the next fold
  DspPoint pt;
  const double rs_ = r * acc[DSP_S];
  pt.L = acc[DSP_L];
  pt.fp = rs_ - pa + pb * ir;
  pt.fpp = __builtin_fma(r * r, acc[DSP_H], rs_) - pb * ir;
  pt.noise = 4.0 * GENE_EPS32 * __builtin_sqrt(acc[DSP_N]) + 64.0 * DSP_EPS64 * r * acc[DSP_P];
  return pt;
}

template <int H, bool U16>
__global__ __launch_bounds__(GENE_NT) void vc_gene_dispersion_kernel(const void* __restrict__ counts, long long Nc, long long gene_stride,
                                                                    const float* __restrict__ B, const float* __restrict__ logm,
                                                                    const double* __restrict__ nu_in, const float* __restrict__ r_start,
                                                                    const double* __restrict__ prior_alpha,
                                                                    const double* __restrict__ prior_beta, double tol, int max_iter,
                                                                    double* __restrict__ rho_out, float* __restrict__ r_out,
                                                                    double* __restrict__ info_out, double* __restrict__ loglik_out,
                                                                    double* __restrict__ score_out, int* __restrict__ iter_out,
                                                                    int* __restrict__ status_out) {
  constexpr int K = 2 * H + 1;
  __shared__ double part[GENE_NW][DSP_NACC];
  __shared__ double tot[DSP_NACC];
  __shared__ unsigned ngt[DSP_T];
  __shared__ unsigned wtot[GENE_NW];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long g = blockIdx.x;
  const void* row = U16 ? (const void*)((const unsigned short*)counts + g * gene_stride) : (const void*)((const float*)counts + g * gene_stride);
  const double nan = __builtin_nan("");

  double nu[K];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    nu[i] = nu_in[g * K + i];
    finite = finite && __builtin_fabs(nu[i]) < 1.0e300;
  }
  if (!finite) {
    if (threadIdx.x == 0) {
      rho_out[g] = nan;
      r_out[g] = __builtin_nanf("");
      info_out[g] = nan;
      loglik_out[g] = nan;
      score_out[g] = nan;
      iter_out[g] = 0;
      status_out[g] = VC_DISP_NO_DATA;
    }
    return;
  }
  double pa = 0.0, pb = 0.0;
  if (prior_alpha) {
    const double al = prior_alpha[g], be = prior_beta[g];
    if (al > 0.0 && al < 1.0e300 && be > 0.0 && be < 1.0e300) { pa = al - 1.0; pb = be; }
  }

  // first walk: the histogram of the counts below DSP_T (larger ones in no bin) and the moment sums of the start
  for (int j = threadIdx.x; j < DSP_T; j += GENE_NT) ngt[j] = 0u;
  __syncthreads();
  double mom[2] = {0.0, 0.0};
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float k = gene_count<U16>(row, c);
    if (k >= 0.f && k < (float)DSP_T) atomicAdd(&ngt[(int)k], 1u);       // the index is inside whatever the count
    double eta;
    const double md = (double)dsp_mu<K>(B, logm, Nc, c, nu, eta);
    const double dv = (double)k - md;
    mom[0] = __builtin_fma(md, md, mom[0]);
    mom[1] += __builtin_fma(dv, dv, -md);
  }
  gene_fold<2>(mom, (double(*)[2])(void*)&part[0][0], tot, lane, wave);
  __syncthreads();                                                   // part / tot are written again by the next fold
  // N_{>j} = Nc - #{k <= j}: every lane scans its DSP_PER consecutive bins, the lanes by a shuffle scan, the waves through the LDS
  {
    unsigned a[DSP_PER], s = 0u;
#pragma unroll
    for (int i = 0; i < DSP_PER; ++i) {
      a[i] = ngt[DSP_PER * threadIdx.x + i];
      s += a[i];
    }
    unsigned inc = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned v = __shfl_up(inc, off, 64);
      if (lane >= off) inc += v;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    unsigned run = inc - s;
    for (int w = 0; w < wave; ++w) run += wtot[w];
#pragma unroll
    for (int i = 0; i < DSP_PER; ++i) {
      run += a[i];
      ngt[DSP_PER * threadIdx.x + i] = (unsigned)Nc - run;
    }
    __syncthreads();
  }

  const double lo = VC_DISP_RHO_MIN, hi = VC_DISP_RHO_MAX;
  int status = VC_DISP_MAX_ITER, steps = 0;
  double rho, info = nan;
  DspPoint pt;
#define DSP_AT(R, LNR) dsp_pass<H, U16>(row, Nc, B, logm, nu, (R), (LNR), pa, pb, ngt, part, tot, lane, wave)
  if (max_iter == 0) {
    const double r = (double)r_start[g];
    rho = log(r);
    pt = DSP_AT(r, rho);
    info = -pt.fpp;
    status = VC_DISP_EVALUATED;
  } else {
    rho = hi;
    pt = DSP_AT(exp(hi), hi);
    if (pt.fp > -pt.noise) {
      status = VC_DISP_AT_UPPER;
    } else {
      rho = lo;
      pt = DSP_AT(exp(lo), lo);
      if (pt.fp < pt.noise) {
        status = VC_DISP_AT_LOWER;
      } else {
        double a = lo, b = hi;                                       // f'(a) > 0 > f'(b)
        double r0 = r_start ? (double)r_start[g] : (mom[1] > 0.0 ? mom[0] / mom[1] : exp(hi));
        rho = log(r0);
        rho = rho > hi ? hi : (rho < lo ? lo : rho);
        if (!(rho > a && rho < b)) rho = 0.5 * (a + b);
        for (;;) {
          pt = DSP_AT(exp(rho), rho);
          info = -pt.fpp;
          if (pt.fpp < 0.0 && pt.fp * pt.fp / -pt.fpp <= tol) { status = VC_DISP_CONVERGED; break; }
          if (__builtin_fabs(pt.fp) <= pt.noise) { status = VC_DISP_ROUNDING; break; }
          if (steps >= max_iter) { status = VC_DISP_MAX_ITER; break; }
          if (pt.fp > 0.0) a = rho; else b = rho;
          const double nt = rho - pt.fp / pt.fpp;
          rho = (pt.fpp < 0.0 && nt > a && nt < b) ? nt : 0.5 * (a + b);
          ++steps;
        }
      }
    }
  }
#undef DSP_AT
  if (threadIdx.x == 0) {
    rho_out[g] = rho;
    r_out[g] = max_iter == 0 ? r_start[g] : (float)exp(rho);
    info_out[g] = info;
    loglik_out[g] = pt.L;
    score_out[g] = pt.fp;
    iter_out[g] = steps;
    status_out[g] = status;
  }
}

constexpr char DSP_FN[] = "vc_gene_dispersion";

}  // namespace

extern "C" int vc_gene_dispersion(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride,
                                  const float* basis_dev, int K, const float* logm_dev, const double* nu_dev, const float* r_start_dev,
                                  const double* prior_alpha_dev, const double* prior_beta_dev, double tol, int max_iter, double* rho_dev,
                                  float* r_dev, double* info_dev, double* loglik_dev, double* score_dev, int32_t* iterations_dev,
                                  int32_t* status_dev, void* hip_stream) {
  const int refused = gene_refuse(DSP_FN, GENE_NO_NOISE, count_kind, K != 1 && K != 3 && K != 5 && K != 7 ? "K must be 1, 3, 5 or 7 (2 H + 1, H in 0..3)" : nullptr,
                                  Ng, Nc, true, gene_stride, 0, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (!counts_dev || !basis_dev || !logm_dev || !nu_dev) return gene_fail(DSP_FN, VC_ERR_ARG, "null input pointer");
  if (!rho_dev || !r_dev || !info_dev || !loglik_dev || !score_dev || !iterations_dev || !status_dev) return gene_fail(DSP_FN, VC_ERR_ARG, "null output pointer");
  if ((prior_alpha_dev == nullptr) != (prior_beta_dev == nullptr)) return gene_fail(DSP_FN, VC_ERR_ARG, "the prior needs both its alpha and its beta");
  if (max_iter == 0 && !r_start_dev) return gene_fail(DSP_FN, VC_ERR_ARG, "max_iter == 0 (evaluate only) needs r_start_dev");
  const dim3 grid((unsigned)Ng), block(GENE_NT);
  hipStream_t st = (hipStream_t)hip_stream;
#define DSP_LAUNCH(H, U16)                                                                                                             \
  hipLaunchKernelGGL((vc_gene_dispersion_kernel<H, U16>), grid, block, 0, st, counts_dev, (long long)Nc, (long long)gene_stride,       \
                     basis_dev, logm_dev, nu_dev, r_start_dev, prior_alpha_dev, prior_beta_dev, tol, max_iter, rho_dev, r_dev,         \
                     info_dev, loglik_dev, score_dev, (int*)iterations_dev, (int*)status_dev)
#define DSP_LAUNCH_H(H)                                                                                                               \
  do {                                                                                                                                \
    if (u16) DSP_LAUNCH(H, true); else DSP_LAUNCH(H, false);                                                                           \
  } while (0)
  const bool u16 = count_kind == VC_COUNTS_U16;
  switch (K) {
    case 1: DSP_LAUNCH_H(0); break;
    case 3: DSP_LAUNCH_H(1); break;
    case 5: DSP_LAUNCH_H(2); break;
    default: DSP_LAUNCH_H(3); break;
  }
#undef DSP_LAUNCH_H
#undef DSP_LAUNCH
  return gene_launched(DSP_FN);
}
