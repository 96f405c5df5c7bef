// Per-gene harmonic regression given the cells' phases: vc_gene_glm of include/velocycle_hip.h, the model of Phases.from_cycle_mle
// (reference velocycle/phases.py:487-507, utils.torch_fourier_basis) solved for the other factor.  Stand-alone: no engine, no
// workspace, one launch; the whole damped Newton iteration of a gene runs inside its workgroup.
//
// Per gene g:  maximise over nu (K = 2H+1 coefficients)
//   Poisson            sum_c k eta - mu                                eta_c = nu . B[:, c] + logm_c,   mu = exp(eta)
//   negative binomial  sum_c k eta - (k + r) ln(r + mu)  (+ Nc r ln r: formed as k d - r w, d = eta - ln(r + mu), w = ln(r + mu) - ln r)
//   minus              sum_i prec_i (nu_i - m_i)^2 / 2                 (optional Gaussian prior)
// Gradient  sum_c res B_i,  res = k - mu | (k - mu) r / (r + mu);  observed Hessian  sum_c w B_i B_j,  w = mu | mu r (k + r) / (r + mu)^2,
// prior precisions on its diagonal.  Both objectives are concave.
//
// Mapping: one workgroup of GENE_NW waves per gene, its lanes walk the gene's row of the [genes][cells] block with stride 256 (every wave
// instruction reads 64 consecutive cells: coalesced).  Per element: eta in float64 from the float32 tables and the float64 nu (K fmas),
// mu = 2^n 2^f with one v_exp_f32 on the fraction (mu carries one rounding whatever |eta|), the residual, the weight and the logarithm
// in float32.  Sums: every lane accumulates in float64 (products with B are exact there), the lanes of a wave are folded by a fixed
// shuffle tree, the waves added in wave order through the LDS -- no atomics, identical bits on repetition.  After the fold every lane
// holds the same totals and runs the same float64 K x K algebra (Cholesky, step, tests), so the control flow is uniform by construction
// and nothing has to be broadcast.
//
// Iteration (status codes: velocycle_hip.h):
//   start    nu0 = ln(sum k / sum e^logm), harmonics 0 (prior means where finite, except nu0)
//   at nu    g, H, objective L, A = sum |terms of L|, N_i = sum (w^2 + res^2) B_i^2
//            Cholesky of H fails (pivot <= 0 or not finite)          -> SINGULAR
//            dec = g' H^-1 g <= tol                                    -> CONVERGED
//            every |g_i| <= 4 eps32 sqrt(N_i)                          -> ROUNDING   (the gradient is its own float32 rounding:
//                                                                         a relative error e of mu moves res by w e, res rounds by |res| e)
//            steps taken == max_iter                                   -> MAX_ITER
//   step     nu' = nu + t H^-1 g, t = 1; a harmonic of nu' outside [-50, 50] -> UNBOUNDED (nu stays the last point inside)
//            accepted unless L' < L - 8 eps32 max(A, A') (a drop beyond the objective's own rounding), else t /= 2; a gene has
//            GLM_MAX_HALVINGS halvings in all (then MAX_ITER): no path spins.
// Outputs are those of the last accepted point: nu, packed H^-1, L without the prior term, dec, steps taken, status.
// vc_gene_glm_weighted.hip repeats glm_factor, the start, this iteration and the covariance block statement for statement (with case
// weights in its sweep): a change to the step or stopping rules has to be made in both files.
#include "vc_gene_glm_math.h"                     // glm_sweep, glm_prior and the packed algebra, shared with vc_gene_glm_batch.hip; through it vc_gene_math.h

#pragma clang fp contract(off)

namespace {

// One pass over the gene's cells at nu: acc = [g (K) | H packed (NH) | L | A | N (K)], folded over the workgroup
template <int H, int NOISE, bool U16>
__device__ __forceinline__ void glm_pass(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                         const float* __restrict__ logm, float r, double lnr, const double (&nu)[2 * H + 1],
                                         double (&acc)[GlmSums<H>::N], double (*part)[GlmSums<H>::N], double* tot, int lane, int wave) {
  typedef GlmSums<H> S;
#pragma unroll
  for (int i = 0; i < S::N; ++i) acc[i] = 0.0;
  glm_sweep<H, NOISE, U16>(row, 0, Nc, Nc, B, logm, r, lnr, nu, acc);
  gene_fold<S::N>(acc, part, tot, lane, wave);
}

// Gradient gr, Cholesky factor of the Hessian and penalty of the penalised objective at nu, from the sums of a pass
template <int H>
__device__ __forceinline__ bool glm_factor(const double (&acc)[GlmSums<H>::N], const double (&nu)[2 * H + 1], const double (&pm)[2 * H + 1],
                                           const double (&pp)[2 * H + 1], double (&gr)[2 * H + 1],
                                           double (&chol)[GlmSums<H>::NH], double& pen) {
  typedef GlmSums<H> S;
  pen = 0.0;
#pragma unroll
  for (int i = 0; i < S::NH; ++i) chol[i] = acc[S::OFF_H + i];
#pragma unroll
  for (int i = 0; i < S::K; ++i) {
    const double d = nu[i] - pm[i];
    gr[i] = __builtin_fma(-pp[i], d, acc[i]);
    chol[glm_tri(i, i)] += pp[i];
    pen = __builtin_fma(0.5 * pp[i] * d, d, pen);
  }
  return glm_chol<S::K>(chol);
}

template <int H, int NOISE, bool U16>
__global__ __launch_bounds__(GENE_NT) void vc_gene_glm_kernel(const void* __restrict__ counts, long long Nc, long long gene_stride,
                                                             const float* __restrict__ B, const float* __restrict__ logm,
                                                             const float* __restrict__ rg, const double* __restrict__ prior_mean,
                                                             const double* __restrict__ prior_prec, double tol, int max_iter,
                                                             double* __restrict__ nu_out, double* __restrict__ cov_out,
                                                             double* __restrict__ loglik_out, double* __restrict__ dec_out,
                                                             int* __restrict__ iter_out, int* __restrict__ status_out) {
  typedef GlmSums<H> S;
  constexpr int K = S::K, NH = S::NH;
  __shared__ double part[GENE_NW][S::N];
  __shared__ double tot[S::N];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long g = blockIdx.x;
  const void* row = U16 ? (const void*)((const unsigned short*)counts + g * gene_stride) : (const void*)((const float*)counts + g * gene_stride);
  const float r = NOISE == VC_NOISE_NB ? rg[g] : 0.f;
  const double lnr = NOISE == VC_NOISE_NB ? log((double)r) : 0.0;

  double pm[K], pp[K];                                              // the prior of this gene
#pragma unroll
  for (int i = 0; i < K; ++i) glm_prior(prior_mean, prior_prec, g * K + i, pm[i], pp[i]);

  // start: sum k and sum e^logm
  double nu[K];
  {
    double s2[2] = {0.0, 0.0};
    for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
      s2[0] += (double)gene_count<U16>(row, c);
      s2[1] += (double)__builtin_amdgcn_exp2f(VC_LOG2E * logm[c]);
    }
    gene_fold<2>(s2, (double(*)[2])(void*)&part[0][0], tot, lane, wave);
    __syncthreads();                                               // part / tot are used with another row length below
    nu[0] = log(s2[0] / s2[1]);
#pragma unroll
    for (int i = 1; i < K; ++i) nu[i] = pp[i] > 0.0 ? pm[i] : 0.0;
    if (!(s2[0] > 0.0) || !(__builtin_fabs(nu[0]) < 1.0e300)) {    // no count at all (or no finite scale): no maximum
      if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        for (int i = 0; i < K; ++i) nu_out[g * K + i] = i == 0 ? nu[0] : 0.0;
        for (int i = 0; i < NH; ++i) cov_out[g * NH + i] = nan;
        loglik_out[g] = nan;
        dec_out[g] = nan;
        iter_out[g] = 0;
        status_out[g] = VC_GLM_UNBOUNDED;
      }
      return;
    }
  }

  double acc[S::N];
  glm_pass<H, NOISE, U16>(row, Nc, B, logm, r, lnr, nu, acc, part, tot, lane, wave);
  int status = VC_GLM_MAX_ITER, steps = 0, halvings = GLM_MAX_HALVINGS;
  double dec = __builtin_nan(""), Lcur = 0.0;
  double chol[NH];
  bool have_chol = false;
  for (;;) {
    // acc holds the sums at nu; only L and A of them outlive the next pass (the step is retried from nu, gr and dx)
    Lcur = acc[S::OFF_L];
    const double Acur = acc[S::OFF_A];
    double gr[K], pen;
    have_chol = glm_factor<H>(acc, nu, pm, pp, gr, chol, pen);
    if (!have_chol) { status = VC_GLM_SINGULAR; break; }
    double dx[K];
#pragma unroll
    for (int i = 0; i < K; ++i) dx[i] = gr[i];
    glm_solve<K>(chol, dx);
    dec = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) dec = __builtin_fma(gr[i], dx[i], dec);
    if (!(__builtin_fabs(dec) < 1.0e300)) { status = VC_GLM_SINGULAR; have_chol = false; break; }
    if (dec <= tol) { status = VC_GLM_CONVERGED; break; }
    bool noise = true;
#pragma unroll
    for (int i = 0; i < K; ++i) noise = noise && __builtin_fabs(gr[i]) <= 4.0 * GENE_EPS32 * __builtin_sqrt(acc[S::OFF_N + i]);
    if (noise) { status = VC_GLM_ROUNDING; break; }
    if (steps >= max_iter) { status = VC_GLM_MAX_ITER; break; }
    const double Lpen = Lcur - pen;
    double t = 1.0;
    bool moved = false, overwritten = false;
    for (;;) {
      double trial[K];
      bool inside = true;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        trial[i] = __builtin_fma(t, dx[i], nu[i]);
        if (i > 0) inside = inside && __builtin_fabs(trial[i]) <= GLM_BOUND;
      }
      if (!inside) { status = VC_GLM_UNBOUNDED; break; }
      glm_pass<H, NOISE, U16>(row, Nc, B, logm, r, lnr, trial, acc, part, tot, lane, wave);
      overwritten = true;
      double pen2 = 0.0;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const double d = trial[i] - pm[i];
        pen2 = __builtin_fma(0.5 * pp[i] * d, d, pen2);
      }
      const double A = acc[S::OFF_A] > Acur ? acc[S::OFF_A] : Acur;
      if (acc[S::OFF_L] - pen2 >= Lpen - 8.0 * GENE_EPS32 * A) {      // false for a NaN: such a step is halved
#pragma unroll
        for (int i = 0; i < K; ++i) nu[i] = trial[i];
        moved = true;
        break;
      }
      if (halvings == 0) { status = VC_GLM_MAX_ITER; break; }
      --halvings;
      t *= 0.5;
    }
    if (!moved) {
      if (overwritten) {                                             // a refused trial's sums are in acc: form those of nu again
        glm_pass<H, NOISE, U16>(row, Nc, B, logm, r, lnr, nu, acc, part, tot, lane, wave);
        Lcur = acc[S::OFF_L];
        have_chol = glm_factor<H>(acc, nu, pm, pp, gr, chol, pen);
      }
      break;
    }
    ++steps;
  }

  // the covariance H^-1 of the last accepted point, column by column from the factor
  double cov[NH];
  if (have_chol) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      double e[K];
#pragma unroll
      for (int i = 0; i < K; ++i) e[i] = i == j ? 1.0 : 0.0;
      glm_solve<K>(chol, e);
#pragma unroll
      for (int i = j; i < K; ++i) cov[glm_tri(i, j)] = e[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < NH; ++i) cov[i] = __builtin_nan("");
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < K; ++i) nu_out[g * K + i] = nu[i];
#pragma unroll
    for (int i = 0; i < NH; ++i) cov_out[g * NH + i] = cov[i];
    loglik_out[g] = Lcur;
    dec_out[g] = dec;
    iter_out[g] = steps;
    status_out[g] = status;
  }
}

constexpr char GLM_FN[] = "vc_gene_glm";

}  // namespace

extern "C" int vc_gene_glm(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev,
                           int K, const float* logm_dev, int noise, const float* r_dev, const double* prior_mean_dev,
                           const double* prior_prec_dev, double tol, int max_iter, double* nu_dev, double* cov_dev, double* loglik_dev,
                           double* dec_dev, int32_t* iterations_dev, int32_t* status_dev, void* hip_stream) {
  const int refused = gene_refuse(GLM_FN, noise, count_kind, K != 1 && K != 3 && K != 5 && K != 7 ? "K must be 1, 3, 5 or 7 (2 H + 1, H in 0..3)" : nullptr,
                                  Ng, Nc, false, gene_stride, 1, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (!counts_dev || !basis_dev || !logm_dev) return gene_fail(GLM_FN, VC_ERR_ARG, "null input pointer");
  if (!nu_dev || !cov_dev || !loglik_dev || !dec_dev || !iterations_dev || !status_dev) return gene_fail(GLM_FN, VC_ERR_ARG, "null output pointer");
  if (noise == VC_NOISE_NB && !r_dev) return gene_fail(GLM_FN, VC_ERR_ARG, "the negative binomial needs r_dev (1 / dispersion per gene)");
  if ((prior_mean_dev == nullptr) != (prior_prec_dev == nullptr)) return gene_fail(GLM_FN, VC_ERR_ARG, "the prior needs both its means and its precisions");
  const dim3 grid((unsigned)Ng), block(GENE_NT);
  hipStream_t st = (hipStream_t)hip_stream;
#define GLM_LAUNCH(H, NOISE, U16)                                                                                                      \
  hipLaunchKernelGGL((vc_gene_glm_kernel<H, NOISE, U16>), grid, block, 0, st, counts_dev, (long long)Nc, (long long)gene_stride,       \
                     basis_dev, logm_dev, r_dev, prior_mean_dev, prior_prec_dev, tol, max_iter, nu_dev, cov_dev, loglik_dev, dec_dev,  \
                     (int*)iterations_dev, (int*)status_dev)
#define GLM_LAUNCH_H(H)                                                                                                               \
  do {                                                                                                                                \
    if (noise == VC_NOISE_NB) { if (u16) GLM_LAUNCH(H, VC_NOISE_NB, true); else GLM_LAUNCH(H, VC_NOISE_NB, false); }                     \
    else { if (u16) GLM_LAUNCH(H, VC_NOISE_POISSON, true); else GLM_LAUNCH(H, VC_NOISE_POISSON, false); }                                \
  } while (0)
  const bool u16 = count_kind == VC_COUNTS_U16;
  switch (K) {
    case 1: GLM_LAUNCH_H(0); break;
    case 3: GLM_LAUNCH_H(1); break;
    case 5: GLM_LAUNCH_H(2); break;
    default: GLM_LAUNCH_H(3); break;
  }
#undef GLM_LAUNCH_H
#undef GLM_LAUNCH
  return gene_launched(GLM_FN);
}
