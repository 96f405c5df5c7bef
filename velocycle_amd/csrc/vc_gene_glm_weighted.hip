// Per-gene harmonic regression with case weights: vc_gene_glm_weighted of include/velocycle_hip.h.  The model, the mapping of a gene's
// row onto a workgroup, the iteration and its status codes are those written at the head of vc_gene_glm.hip; every cell's contribution
// is multiplied by a weight w_bc >= 0 read from row b of a float32 table, and one call solves R rows of weights for every gene (a cell
// bootstrap: Poisson(1) integer weights per row; a held-out fit: 0 / 1; the ordinary weighted regression: the caller's weights).
//
// Sums, wt = (double)w_bc:  gradient sum (wt res) B_i,  Hessian sum (wt wo) B_i B_j,  objective sum wt term (the negative binomial's
// r ln r is inside term: weighted with it),  magnitude A = sum wt mag,  rounding scale N_i = sum ((wt wo)^2 + (wt res)^2) B_i^2,
// start nu_0 = ln(sum wt k / sum wt e^logm).  The prior is not weighted.  Each product is formed first (wt x, exact at wt == 1) and the
// float64 operations that follow are those of glm_sweep in the same order, so a table of ones gives vc_gene_glm's bits.
//
// Mapping: one workgroup of GENE_NW waves per (gene, row), grid = (R, genes) with the row in x, the fast index: the workgroups in
// flight share a gene's count row and stream the weight table.  That order was 9 % faster at 50 000 x 2 000, R = 200 than the gene in x
// (one 4 Nc-byte weight row hot, the counts streamed); DESIGN.md has both times.  gridDim.y holds at most 65535 genes, so the entry
// point launches slabs of GLMW_SLAB genes one after the other on the stream (g_base: the slab's first gene); R <= 65535 keeps
// gridDim.x * blockDim.x below 2^32.  Float64 per-lane sums, shuffle tree, waves in wave order through the LDS: no atomics, identical
// bits on repetition and under any cutting of genes or rows into calls.
//
// glmw_factor, the start, the iteration and the covariance block below are vc_gene_glm.hip's, statement for statement, with glm_pass
// replaced by glmw_pass: that file's gfx950 assembly may not move, so nothing of it could be factored out.  A change to the step or
// stopping rules has to be made in both files.
#include "vc_gene_glm_math.h"                     // the packed algebra, glm_prior, GlmSums; through it vc_gene_math.h

#pragma clang fp contract(off)

namespace {

// glm_sweep of vc_gene_glm_math.h over the whole row with every contribution multiplied by the cell's weight
template <int H, int NOISE, bool U16>
__device__ __forceinline__ void glmw_sweep(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                           const float* __restrict__ logm, const float* __restrict__ wrow, float r, double lnr,
                                           const double (&nu)[2 * H + 1], double (&acc)[GlmSums<H>::N]) {
  typedef GlmSums<H> S;
  constexpr int K = S::K;
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float k = gene_count<U16>(row, c);
    const double wt = (double)wrow[c];
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
    const double rd = wt * (double)res, wd = wt * (double)w;
    const double n2 = __builtin_fma(wd, wd, rd * rd);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      acc[i] = __builtin_fma(rd, b[i], acc[i]);
      const double wb = wd * b[i];
#pragma unroll
      for (int j = 0; j <= i; ++j) acc[S::OFF_H + glm_tri(i, j)] = __builtin_fma(wb, b[j], acc[S::OFF_H + glm_tri(i, j)]);
      acc[S::OFF_N + i] = __builtin_fma(n2, b[i] * b[i], acc[S::OFF_N + i]);
    }
    acc[S::OFF_L] += wt * term;
    acc[S::OFF_A] += wt * mag;
  }
}

// One pass over the gene's cells at nu under the row's weights: acc = [g (K) | H packed (NH) | L | A | N (K)], folded over the workgroup
template <int H, int NOISE, bool U16>
__device__ __forceinline__ void glmw_pass(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                          const float* __restrict__ logm, const float* __restrict__ wrow, float r, double lnr,
                                          const double (&nu)[2 * H + 1], double (&acc)[GlmSums<H>::N], double (*part)[GlmSums<H>::N],
                                          double* tot, int lane, int wave) {
  typedef GlmSums<H> S;
#pragma unroll
  for (int i = 0; i < S::N; ++i) acc[i] = 0.0;
  glmw_sweep<H, NOISE, U16>(row, Nc, B, logm, wrow, r, lnr, nu, acc);
  gene_fold<S::N>(acc, part, tot, lane, wave);
}

// Gradient gr, Cholesky factor of the Hessian and penalty of the penalised objective at nu, from the sums of a pass (vc_gene_glm's)
template <int H>
__device__ __forceinline__ bool glmw_factor(const double (&acc)[GlmSums<H>::N], const double (&nu)[2 * H + 1], const double (&pm)[2 * H + 1],
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
__global__ __launch_bounds__(GENE_NT) void vc_gene_glm_weighted_kernel(const void* __restrict__ counts, long long g_base, long long Ng, long long Nc,
                                                                      long long gene_stride, const float* __restrict__ B,
                                                                      const float* __restrict__ logm, const float* __restrict__ rg,
                                                                      const double* __restrict__ prior_mean,
                                                                      const double* __restrict__ prior_prec,
                                                                      const float* __restrict__ weights, long long R,
                                                                      long long weight_stride, const double* __restrict__ start,
                                                                      double tol, int max_iter, double* __restrict__ nu_out,
                                                                      double* __restrict__ cov_out, double* __restrict__ loglik_out,
                                                                      double* __restrict__ dec_out, int* __restrict__ iter_out,
                                                                      int* __restrict__ status_out) {
  typedef GlmSums<H> S;
  constexpr int K = S::K, NH = S::NH;
  __shared__ double part[GENE_NW][S::N];
  __shared__ double tot[S::N];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long g = g_base + blockIdx.y, b = blockIdx.x;         // the row is the fast index
  const long long at = b * Ng + g;                                  // the (row, gene) pair's place in every output
  const void* row = U16 ? (const void*)((const unsigned short*)counts + g * gene_stride) : (const void*)((const float*)counts + g * gene_stride);
  const float* wrow = weights + b * weight_stride;
  const float r = NOISE == VC_NOISE_NB ? rg[g] : 0.f;
  const double lnr = NOISE == VC_NOISE_NB ? log((double)r) : 0.0;

  double pm[K], pp[K];                                              // the prior of this gene
#pragma unroll
  for (int i = 0; i < K; ++i) glm_prior(prior_mean, prior_prec, g * K + i, pm[i], pp[i]);

  // start: sum wt k and sum wt e^logm (formed whatever the start: a row without a weighted count has no maximum)
  double nu[K];
  {
    double s2[2] = {0.0, 0.0};
    for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
      const double wt = (double)wrow[c];
      s2[0] += wt * (double)gene_count<U16>(row, c);
      s2[1] += wt * (double)__builtin_amdgcn_exp2f(VC_LOG2E * logm[c]);
    }
    gene_fold<2>(s2, (double(*)[2])(void*)&part[0][0], tot, lane, wave);
    __syncthreads();                                               // part / tot are used with another row length below
    nu[0] = log(s2[0] / s2[1]);
#pragma unroll
    for (int i = 1; i < K; ++i) nu[i] = pp[i] > 0.0 ? pm[i] : 0.0;
    if (!(s2[0] > 0.0) || !(__builtin_fabs(nu[0]) < 1.0e300)) {    // no weighted count at all (or no finite scale): no maximum
      if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        for (int i = 0; i < K; ++i) nu_out[at * K + i] = i == 0 ? nu[0] : 0.0;
        if (cov_out) for (int i = 0; i < NH; ++i) cov_out[at * NH + i] = nan;
        loglik_out[at] = nan;
        dec_out[at] = nan;
        iter_out[at] = 0;
        status_out[at] = VC_GLM_UNBOUNDED;
      }
      return;
    }
    if (start) {                                                    // the gene's warm start, if it is a point the iteration may visit
      double sv[K];
      bool usable = true;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        sv[i] = start[g * K + i];
        usable = usable && __builtin_fabs(sv[i]) < 1.0e300 && (i == 0 || __builtin_fabs(sv[i]) <= GLM_BOUND);
      }
      if (usable) {
#pragma unroll
        for (int i = 0; i < K; ++i) nu[i] = sv[i];
      }
    }
  }

  double acc[S::N];
  glmw_pass<H, NOISE, U16>(row, Nc, B, logm, wrow, r, lnr, nu, acc, part, tot, lane, wave);
  int status = VC_GLM_MAX_ITER, steps = 0, halvings = GLM_MAX_HALVINGS;
  double dec = __builtin_nan(""), Lcur = 0.0;
  double chol[NH];
  bool have_chol = false;
  for (;;) {
    // acc holds the sums at nu; only L and A of them outlive the next pass (the step is retried from nu, gr and dx)
    Lcur = acc[S::OFF_L];
    const double Acur = acc[S::OFF_A];
    double gr[K], pen;
    have_chol = glmw_factor<H>(acc, nu, pm, pp, gr, chol, pen);
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
      glmw_pass<H, NOISE, U16>(row, Nc, B, logm, wrow, r, lnr, trial, acc, part, tot, lane, wave);
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
        glmw_pass<H, NOISE, U16>(row, Nc, B, logm, wrow, r, lnr, nu, acc, part, tot, lane, wave);
        Lcur = acc[S::OFF_L];
        have_chol = glmw_factor<H>(acc, nu, pm, pp, gr, chol, pen);
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
    for (int i = 0; i < K; ++i) nu_out[at * K + i] = nu[i];
    if (cov_out) {
#pragma unroll
      for (int i = 0; i < NH; ++i) cov_out[at * NH + i] = cov[i];
    }
    loglik_out[at] = Lcur;
    dec_out[at] = dec;
    iter_out[at] = steps;
    status_out[at] = status;
  }
}

constexpr char GLMW_FN[] = "vc_gene_glm_weighted";
constexpr int64_t GLMW_MAX_ROWS = 65535;          // gridDim.x, and 65535 * GENE_NT < 2^32
constexpr int64_t GLMW_SLAB = 65535;              // genes per launch: gridDim.y

}  // namespace

extern "C" int vc_gene_glm_weighted(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride,
                                    const float* basis_dev, int K, const float* logm_dev, int noise, const float* r_dev,
                                    const double* prior_mean_dev, const double* prior_prec_dev, const float* weights_dev, int64_t R,
                                    int64_t weight_stride, const double* start_dev, double tol, int max_iter, double* nu_dev,
                                    double* cov_dev, double* loglik_dev, double* dec_dev, int32_t* iterations_dev, int32_t* status_dev,
                                    void* hip_stream) {
  const int refused = gene_refuse(GLMW_FN, noise, count_kind, K != 1 && K != 3 && K != 5 && K != 7 ? "K must be 1, 3, 5 or 7 (2 H + 1, H in 0..3)" : nullptr,
                                  Ng, Nc, false, gene_stride, 1, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (!counts_dev || !basis_dev || !logm_dev) return gene_fail(GLMW_FN, VC_ERR_ARG, "null input pointer");
  if (!nu_dev || !loglik_dev || !dec_dev || !iterations_dev || !status_dev) return gene_fail(GLMW_FN, VC_ERR_ARG, "null output pointer (only cov_dev may be NULL)");
  if (noise == VC_NOISE_NB && !r_dev) return gene_fail(GLMW_FN, VC_ERR_ARG, "the negative binomial needs r_dev (1 / dispersion per gene)");
  if ((prior_mean_dev == nullptr) != (prior_prec_dev == nullptr)) return gene_fail(GLMW_FN, VC_ERR_ARG, "the prior needs both its means and its precisions");
  if (!weights_dev) return gene_fail(GLMW_FN, VC_ERR_ARG, "null weights_dev");
  if (R < 1 || R > GLMW_MAX_ROWS) return gene_fail(GLMW_FN, VC_ERR_ARG, "R must be in 1..65535 rows of weights per call");
  if (weight_stride < Nc) return gene_fail(GLMW_FN, VC_ERR_ARG, "weight_stride < Nc");
  const dim3 block(GENE_NT);
  hipStream_t st = (hipStream_t)hip_stream;
#define GLMW_LAUNCH(H, NOISE, U16)                                                                                                       \
  hipLaunchKernelGGL((vc_gene_glm_weighted_kernel<H, NOISE, U16>), grid, block, 0, st, counts_dev, (long long)g0, (long long)Ng,         \
                     (long long)Nc,                                                                                                      \
                     (long long)gene_stride, basis_dev, logm_dev, r_dev, prior_mean_dev, prior_prec_dev, weights_dev, (long long)R,      \
                     (long long)weight_stride, start_dev, tol, max_iter, nu_dev, cov_dev, loglik_dev, dec_dev, (int*)iterations_dev,     \
                     (int*)status_dev)
#define GLMW_LAUNCH_H(H)                                                                                                                 \
  do {                                                                                                                                  \
    if (noise == VC_NOISE_NB) { if (u16) GLMW_LAUNCH(H, VC_NOISE_NB, true); else GLMW_LAUNCH(H, VC_NOISE_NB, false); }                     \
    else { if (u16) GLMW_LAUNCH(H, VC_NOISE_POISSON, true); else GLMW_LAUNCH(H, VC_NOISE_POISSON, false); }                                \
  } while (0)
  const bool u16 = count_kind == VC_COUNTS_U16;
  for (int64_t g0 = 0; g0 < Ng; g0 += GLMW_SLAB) {                 // every slab reads and writes at its genes' own places
    const int64_t n = Ng - g0 < GLMW_SLAB ? Ng - g0 : GLMW_SLAB;
    const dim3 grid((unsigned)R, (unsigned)n);
    switch (K) {
      case 1: GLMW_LAUNCH_H(0); break;
      case 3: GLMW_LAUNCH_H(1); break;
      case 5: GLMW_LAUNCH_H(2); break;
      default: GLMW_LAUNCH_H(3); break;
    }
  }
#undef GLMW_LAUNCH_H
#undef GLMW_LAUNCH
  return gene_launched(GLMW_FN);
}
