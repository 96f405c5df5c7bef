// Batch-aware per-gene harmonic regression with case weights: vc_gene_glm_batch_weighted of include/velocycle_hip.h.  The model, the
// segment walk, the Schur-complement algebra, the iteration and its status codes are those written at the head of vc_gene_glm_batch.hip;
// every cell's contribution is multiplied by a weight w_bc >= 0 read from row b of a float32 table, and one call solves R rows of weights
// for every gene (the cell bootstrap of the batch-aware fit; a held-out fit: 0 / 1; the ordinary weighted regression).
//
// Sums of a segment, wt = (double)w_bc:  sum (wt res) = dL/d delta_b,  h_b = sum (wt wo) B_i (W_b = h_b0),  N with (wt wo)^2 + (wt res)^2,
// L = sum wt term,  A = sum wt mag,  start nu_0 = ln(sum wt k / sum wt e^logm).  The priors of nu and delta are not weighted.  Each
// product is formed first (wt x, exact at wt == 1) and the float64 operations that follow are glm_sweep's in the same order, so a table
// of ones with R = 1 and no start gives vc_gene_glm_batch's bits.  A batch whose cells all weigh 0 in a row has W_b = 0, D_b = q_b: its
// offset goes to its prior mean and nothing is singular.
//
// Mapping: vc_gene_glm_weighted's.  One workgroup of GENE_NW waves per (gene, row), grid = (R, genes) with the row in x, the fast index;
// slabs of GLMBW_SLAB genes launched one after the other on the stream (g_base: the slab's first gene); R <= 65535.  The segment table
// travels in the kernel's arguments.  No atomics: identical bits on repetition and under any cutting of genes or rows into calls.
//
// glmbw_block, glmbw_factor, the iteration and the covariance block below are vc_gene_glm_batch.hip's, statement for statement, with
// glmb_pass replaced by glmbw_pass: that file's gfx950 assembly may not move, so nothing of it could be factored out.  A change to the
// step or stopping rules has to be made in both files.
#include "vc_gene_glm_math.h"                     // the packed algebra, glm_prior, GlmSums; through it vc_gene_math.h

#pragma clang fp contract(off)

namespace {

struct GlmbwSeg {                                  // the segment offsets travel in the kernel's arguments: no device array, no copy
  long long s[VC_GLM_MAX_BATCHES + 1];
};

template <int K>
struct GlmbwLds {
  double delta[VC_GLM_MAX_BATCHES];             // the offsets of the last accepted point
  double trial[VC_GLM_MAX_BATCHES];             // those of the point a pass is made at
  double step[VC_GLM_MAX_BATCHES];
  double m[VC_GLM_MAX_BATCHES], q[VC_GLM_MAX_BATCHES];
  double res[VC_GLM_MAX_BATCHES];               // sum res of the segment
  double n0[VC_GLM_MAX_BATCHES];                // sum w^2 + res^2
  double h[VC_GLM_MAX_BATCHES][K];              // sum w B_i; h[b][0] = W_b
};

// The penalised gradient entry, 1 / D_b and the validity of batch b at the offset d_b
template <int K>
__device__ __forceinline__ bool glmbw_block(const GlmbwLds<K>& s, int b, double db, double& dm, double& gb, double& iD) {
  const double q = s.q[b], m = s.m[b];
  dm = db - m;
  gb = __builtin_fma(-q, dm, s.res[b]);
  const double D = s.h[b][0] + q;
  const bool ok = D > 0.0 && D < 1.0e300 && q > 0.0 && q < 1.0e300 && __builtin_fabs(m) < 1.0e300;
  iD = 1.0 / (ok ? D : 1.0);
  return ok;
}

// glm_sweep of vc_gene_glm_math.h over the cells [c0, c1) with every contribution multiplied by the cell's weight
template <int H, int NOISE, bool U16>
__device__ __forceinline__ void glmbw_sweep(const void* __restrict__ row, long long c0, long long c1, long long Nc,
                                            const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ wrow,
                                            float r, double lnr, const double (&nu)[2 * H + 1], double (&acc)[GlmSums<H>::N]) {
  typedef GlmSums<H> S;
  constexpr int K = S::K;
  for (long long c = c0 + threadIdx.x; c < c1; c += GENE_NT) {
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

// One pass at (nu, s.trial) under the row's weights: acc = the pair's totals [g (K) | H packed (NH) | L | A | N (K)] in every lane,
// the delta block in s
template <int H, int NOISE, bool U16>
__device__ __forceinline__ void glmbw_pass(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                          const float* __restrict__ logm, const float* __restrict__ wrow, float r, double lnr,
                                          const double (&nu)[2 * H + 1], int Nb,
                                          const GlmbwSeg& seg, GlmbwLds<2 * H + 1>& s, double* gsum, double (&acc)[GlmSums<H>::N],
                                          double (*part)[GlmSums<H>::N], double* tot, int lane, int wave) {
  typedef GlmSums<H> S;
  constexpr int K = S::K;
  for (int b = 0; b < Nb; ++b) {
    double nub[K];
    nub[0] = nu[0] + s.trial[b];
#pragma unroll
    for (int i = 1; i < K; ++i) nub[i] = nu[i];
#pragma unroll
    for (int i = 0; i < S::N; ++i) acc[i] = 0.0;
    glmbw_sweep<H, NOISE, U16>(row, seg.s[b], seg.s[b + 1], Nc, B, logm, wrow, r, lnr, nub, acc);
    gene_fold<S::N>(acc, part, tot, lane, wave);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < S::N; ++i) gsum[i] = b == 0 ? acc[i] : gsum[i] + acc[i];
      s.res[b] = acc[0];
      s.n0[b] = acc[S::OFF_N];
#pragma unroll
      for (int i = 0; i < K; ++i) s.h[b][i] = acc[S::OFF_H + glm_tri(i, 0)];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < S::N; ++i) acc[i] = gsum[i];
}

// From the sums of a pass at (nu, dl): the nu gradient gr, the Schur right-hand side, the Cholesky factor of S, the penalty,
// sum_b g_b^2 / D_b and whether every delta gradient entry is within its rounding.  false: SINGULAR
template <int H>
__device__ __forceinline__ bool glmbw_factor(const double (&acc)[GlmSums<H>::N], const double (&nu)[2 * H + 1], const double (&pm)[2 * H + 1],
                                            const double (&pp)[2 * H + 1], int Nb, const GlmbwLds<2 * H + 1>& s, const double* dl,
                                            double (&gr)[2 * H + 1], double (&rhs)[2 * H + 1], double (&chol)[GlmSums<H>::NH], double& pen,
                                            double& gd2, bool& delta_noise) {
  typedef GlmSums<H> S;
  constexpr int K = S::K;
  pen = 0.0;
  gd2 = 0.0;
  delta_noise = true;
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) chol[glm_tri(i, j)] = j == 0 ? 0.0 : acc[S::OFF_H + glm_tri(i, j)];
  }
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double d = nu[i] - pm[i];
    gr[i] = __builtin_fma(-pp[i], d, acc[i]);
    rhs[i] = i == 0 ? -pp[0] * d : gr[i];
    chol[glm_tri(i, i)] += pp[i];
    pen = __builtin_fma(0.5 * pp[i] * d, d, pen);
  }
  bool ok = true;
  for (int b = 0; b < Nb; ++b) {
    double dm, gb, iD;
    ok = glmbw_block<K>(s, b, dl[b], dm, gb, iD) && ok;
    const double q = s.q[b];
    const double qD = q * iD;
    pen = __builtin_fma(0.5 * q * dm, dm, pen);
    rhs[0] = __builtin_fma(q, __builtin_fma(gb, iD, dm), rhs[0]);
    gd2 = __builtin_fma(gb * iD, gb, gd2);
    delta_noise = delta_noise && __builtin_fabs(gb) <= 4.0 * GENE_EPS32 * __builtin_sqrt(s.n0[b]);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double hi = s.h[b][i];
      chol[glm_tri(i, 0)] = __builtin_fma(hi, qD, chol[glm_tri(i, 0)]);
      if (i > 0) {
        const double hD = hi * iD;
        rhs[i] = __builtin_fma(-hD, gb, rhs[i]);
#pragma unroll
        for (int j = 1; j <= i; ++j) chol[glm_tri(i, j)] = __builtin_fma(-hD, s.h[b][j], chol[glm_tri(i, j)]);
      }
    }
  }
  return glm_chol<K>(chol) && ok;
}

template <int H, int NOISE, bool U16>
__global__ __launch_bounds__(GENE_NT) void vc_gene_glm_batch_weighted_kernel(
    const void* __restrict__ counts, long long g_base, long long Ng, long long Nc, long long gene_stride, const float* __restrict__ B,
    const float* __restrict__ logm, const float* __restrict__ rg, int Nb, const GlmbwSeg seg, const double* __restrict__ delta_mean,
    const double* __restrict__ delta_prec, const double* __restrict__ prior_mean, const double* __restrict__ prior_prec,
    const float* __restrict__ weights, long long weight_stride, const double* __restrict__ start_nu,
    const double* __restrict__ start_delta, double tol, int max_iter, double* __restrict__ nu_out, double* __restrict__ delta_out,
    double* __restrict__ cov_out, double* __restrict__ dvar_out, double* __restrict__ loglik_out, double* __restrict__ dec_out,
    int* __restrict__ iter_out, int* __restrict__ status_out) {
  typedef GlmSums<H> S;
  constexpr int K = S::K, NH = S::NH;
  __shared__ double part[GENE_NW][S::N];
  __shared__ double tot[S::N];
  __shared__ double gsum[S::N];
  __shared__ GlmbwLds<K> s;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tb = threadIdx.x;                                        // the batch this thread looks after (tb < Nb)
  const long long g = g_base + blockIdx.y, rb = blockIdx.x;         // the row is the fast index
  const long long at = rb * Ng + g;                                  // the (row, gene) pair's place in every output
  const void* row = U16 ? (const void*)((const unsigned short*)counts + g * gene_stride) : (const void*)((const float*)counts + g * gene_stride);
  const float* wrow = weights + rb * weight_stride;
  const float r = NOISE == VC_NOISE_NB ? rg[g] : 0.f;
  const double lnr = NOISE == VC_NOISE_NB ? log((double)r) : 0.0;
  const double nan = __builtin_nan("");

  double pm[K], pp[K];                                              // the prior of nu
#pragma unroll
  for (int i = 0; i < K; ++i) glm_prior(prior_mean, prior_prec, g * K + i, pm[i], pp[i]);
  // the gene's warm start, if it is a point the iteration may visit; every lane reads all of it: one decision for all
  bool warm = start_nu != nullptr;
  if (warm) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double v = start_nu[g * K + i];
      warm = warm && __builtin_fabs(v) < 1.0e300 && (i == 0 || __builtin_fabs(v) <= GLM_BOUND);
    }
    for (int b = 0; b < Nb; ++b) warm = warm && __builtin_fabs(start_delta[g * Nb + b]) <= GLM_BOUND;   // false for a NaN
  }
  if (tb < Nb) {
    const double m = delta_mean[g * Nb + tb];
    const double d0 = warm ? start_delta[g * Nb + tb] : m;
    s.m[tb] = m;
    s.q[tb] = delta_prec[g * Nb + tb];
    s.delta[tb] = d0;
    s.trial[tb] = d0;
    s.step[tb] = 0.0;
  }

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
    if (!(s2[0] > 0.0 && s2[0] < 1.0e300) || !(__builtin_fabs(nu[0]) < 1.0e300)) {   // no weighted count (or no finite scale): no maximum
      if (threadIdx.x == 0) {
        for (int i = 0; i < K; ++i) nu_out[at * K + i] = i == 0 ? nu[0] : 0.0;
        if (cov_out) for (int i = 0; i < NH; ++i) cov_out[at * NH + i] = nan;
        loglik_out[at] = nan;
        dec_out[at] = nan;
        iter_out[at] = 0;
        status_out[at] = VC_GLM_UNBOUNDED;
      }
      if (tb < Nb) {
        delta_out[at * Nb + tb] = s.m[tb];
        if (dvar_out) dvar_out[at * Nb + tb] = nan;
      }
      return;
    }
    if (warm) {
#pragma unroll
      for (int i = 0; i < K; ++i) nu[i] = start_nu[g * K + i];
    }
  }

  double acc[S::N];
  glmbw_pass<H, NOISE, U16>(row, Nc, B, logm, wrow, r, lnr, nu, Nb, seg, s, gsum, acc, part, tot, lane, wave);
  int status = VC_GLM_MAX_ITER, steps = 0, halvings = GLM_MAX_HALVINGS;
  double dec = nan, Lcur = 0.0;
  double chol[NH];
  bool have_chol = false;
  for (;;) {
    // acc and the delta block hold the sums at (nu, s.delta); only L and A outlive the next pass
    Lcur = acc[S::OFF_L];
    const double Acur = acc[S::OFF_A];
    double gr[K], rhs[K], pen, gd2;
    bool delta_noise;
    have_chol = glmbw_factor<H>(acc, nu, pm, pp, Nb, s, s.delta, gr, rhs, chol, pen, gd2, delta_noise);
    if (!have_chol) { status = VC_GLM_SINGULAR; break; }
    double dx[K];
#pragma unroll
    for (int i = 0; i < K; ++i) dx[i] = rhs[i];
    glm_solve<K>(chol, dx);
    dec = gd2;
#pragma unroll
    for (int i = 0; i < K; ++i) dec = __builtin_fma(rhs[i], dx[i], dec);
    if (!(__builtin_fabs(dec) < 1.0e300)) { status = VC_GLM_SINGULAR; have_chol = false; break; }
    if (dec <= tol) { status = VC_GLM_CONVERGED; break; }
    bool noise = delta_noise;
#pragma unroll
    for (int i = 0; i < K; ++i) noise = noise && __builtin_fabs(gr[i]) <= 4.0 * GENE_EPS32 * __builtin_sqrt(acc[S::OFF_N + i]);
    if (noise) { status = VC_GLM_ROUNDING; break; }
    if (steps >= max_iter) { status = VC_GLM_MAX_ITER; break; }
    if (tb < Nb) {
      double dm, gb, iD;
      glmbw_block<K>(s, tb, s.delta[tb], dm, gb, iD);
      double hd = 0.0;
#pragma unroll
      for (int i = 0; i < K; ++i) hd = __builtin_fma(s.h[tb][i], dx[i], hd);
      s.step[tb] = (gb - hd) * iD;
    }
    __syncthreads();
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
      double pen2 = 0.0;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const double d = trial[i] - pm[i];
        pen2 = __builtin_fma(0.5 * pp[i] * d, d, pen2);
      }
      for (int b = 0; b < Nb; ++b) {                                  // every lane forms every trial offset: one decision for all
        const double db = __builtin_fma(t, s.step[b], s.delta[b]);
        inside = inside && __builtin_fabs(db) <= GLM_BOUND;
        const double d = db - s.m[b];
        pen2 = __builtin_fma(0.5 * s.q[b] * d, d, pen2);
      }
      if (!inside) { status = VC_GLM_UNBOUNDED; break; }
      __syncthreads();                                                // s.trial may still be read as the last pass's offsets
      if (tb < Nb) s.trial[tb] = __builtin_fma(t, s.step[tb], s.delta[tb]);
      __syncthreads();
      glmbw_pass<H, NOISE, U16>(row, Nc, B, logm, wrow, r, lnr, trial, Nb, seg, s, gsum, acc, part, tot, lane, wave);
      overwritten = true;
      const double A = acc[S::OFF_A] > Acur ? acc[S::OFF_A] : Acur;
      if (acc[S::OFF_L] - pen2 >= Lpen - 8.0 * GENE_EPS32 * A) {      // false for a NaN: such a step is halved
#pragma unroll
        for (int i = 0; i < K; ++i) nu[i] = trial[i];
        if (tb < Nb) s.delta[tb] = s.trial[tb];
        __syncthreads();
        moved = true;
        break;
      }
      if (halvings == 0) { status = VC_GLM_MAX_ITER; break; }
      --halvings;
      t *= 0.5;
    }
    if (!moved) {
      if (overwritten) {                                             // a refused trial's sums are in acc and s: form those of the point again
        __syncthreads();
        if (tb < Nb) s.trial[tb] = s.delta[tb];
        __syncthreads();
        glmbw_pass<H, NOISE, U16>(row, Nc, B, logm, wrow, r, lnr, nu, Nb, seg, s, gsum, acc, part, tot, lane, wave);
        Lcur = acc[S::OFF_L];
        have_chol = glmbw_factor<H>(acc, nu, pm, pp, Nb, s, s.delta, gr, rhs, chol, pen, gd2, delta_noise);
      }
      break;
    }
    ++steps;
  }

  // S^-1 of the last accepted point, column by column from the factor; the delta variances from the same factor
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
    for (int i = 0; i < NH; ++i) cov[i] = nan;
  }
  if (tb < Nb) {
    double var = nan;
    if (have_chol) {
      double dm, gb, iD, x[K];
      glmbw_block<K>(s, tb, s.delta[tb], dm, gb, iD);
#pragma unroll
      for (int i = 0; i < K; ++i) x[i] = s.h[tb][i];
      glm_solve<K>(chol, x);
      double hSh = 0.0;
#pragma unroll
      for (int i = 0; i < K; ++i) hSh = __builtin_fma(s.h[tb][i], x[i], hSh);
      var = __builtin_fma(hSh * iD, iD, iD);
    }
    delta_out[at * Nb + tb] = s.delta[tb];
    if (dvar_out) dvar_out[at * Nb + tb] = var;
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

constexpr char GLMBW_FN[] = "vc_gene_glm_batch_weighted";
constexpr int64_t GLMBW_MAX_ROWS = 65535;         // gridDim.x, and 65535 * GENE_NT < 2^32
constexpr int64_t GLMBW_SLAB = 65535;             // genes per launch: gridDim.y

}  // namespace

extern "C" int vc_gene_glm_batch_weighted(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride,
                                          const float* basis_dev, int K, const float* logm_dev, int noise, const float* r_dev, int Nb,
                                          const int64_t* seg_host, const double* delta_prior_mean_dev, const double* delta_prior_prec_dev,
                                          const double* prior_mean_dev, const double* prior_prec_dev, const float* weights_dev, int64_t R,
                                          int64_t weight_stride, const double* start_nu_dev, const double* start_delta_dev, double tol,
                                          int max_iter, double* nu_dev, double* delta_dev, double* cov_nu_dev, double* delta_var_dev,
                                          double* loglik_dev, double* dec_dev, int32_t* iterations_dev, int32_t* status_dev,
                                          void* hip_stream) {
  const int refused = gene_refuse(GLMBW_FN, noise, count_kind, K != 1 && K != 3 && K != 5 && K != 7 ? "K must be 1, 3, 5 or 7 (2 H + 1, H in 0..3)" : nullptr,
                                  Ng, Nc, false, gene_stride, 1, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (Nb < 1 || Nb > VC_GLM_MAX_BATCHES) return gene_fail(GLMBW_FN, VC_ERR_ARG, "Nb must be in 1..VC_GLM_MAX_BATCHES");
  if (!counts_dev || !basis_dev || !logm_dev || !seg_host) return gene_fail(GLMBW_FN, VC_ERR_ARG, "null input pointer");
  if (!delta_prior_mean_dev || !delta_prior_prec_dev)
    return gene_fail(GLMBW_FN, VC_ERR_ARG, "every batch offset needs its prior (delta_prior_mean_dev, delta_prior_prec_dev)");
  if (!nu_dev || !delta_dev || !loglik_dev || !dec_dev || !iterations_dev || !status_dev)
    return gene_fail(GLMBW_FN, VC_ERR_ARG, "null output pointer (only cov_nu_dev and delta_var_dev may be NULL, together)");
  if (noise == VC_NOISE_NB && !r_dev) return gene_fail(GLMBW_FN, VC_ERR_ARG, "the negative binomial needs r_dev (1 / dispersion per gene)");
  if ((prior_mean_dev == nullptr) != (prior_prec_dev == nullptr)) return gene_fail(GLMBW_FN, VC_ERR_ARG, "the prior of nu needs both its means and its precisions");
  GlmbwSeg seg;
  for (int b = 0; b <= VC_GLM_MAX_BATCHES; ++b) seg.s[b] = b <= Nb ? (long long)seg_host[b] : (long long)Nc;
  if (seg.s[0] != 0 || seg.s[Nb] != (long long)Nc) return gene_fail(GLMBW_FN, VC_ERR_ARG, "seg must start at 0 and end at Nc");
  for (int b = 0; b < Nb; ++b) {
    if (seg.s[b + 1] < seg.s[b]) return gene_fail(GLMBW_FN, VC_ERR_ARG, "seg must be non-decreasing");
    if (seg.s[b + 1] == seg.s[b]) return gene_fail(GLMBW_FN, VC_ERR_ARG, "empty segment (a batch without a cell)");
  }
  if (!weights_dev) return gene_fail(GLMBW_FN, VC_ERR_ARG, "null weights_dev");
  if (R < 1 || R > GLMBW_MAX_ROWS) return gene_fail(GLMBW_FN, VC_ERR_ARG, "R must be in 1..65535 rows of weights per call");
  if (weight_stride < Nc) return gene_fail(GLMBW_FN, VC_ERR_ARG, "weight_stride < Nc");
  if ((start_nu_dev == nullptr) != (start_delta_dev == nullptr))
    return gene_fail(GLMBW_FN, VC_ERR_ARG, "a start needs both start_nu_dev and start_delta_dev");
  if ((cov_nu_dev == nullptr) != (delta_var_dev == nullptr))
    return gene_fail(GLMBW_FN, VC_ERR_ARG, "cov_nu_dev and delta_var_dev are stored together: both NULL or both given");
  const dim3 block(GENE_NT);
  hipStream_t st = (hipStream_t)hip_stream;
#define GLMBW_LAUNCH(H, NOISE, U16)                                                                                                      \
  hipLaunchKernelGGL((vc_gene_glm_batch_weighted_kernel<H, NOISE, U16>), grid, block, 0, st, counts_dev, (long long)g0, (long long)Ng,   \
                     (long long)Nc, (long long)gene_stride, basis_dev, logm_dev, r_dev, Nb, seg, delta_prior_mean_dev,                   \
                     delta_prior_prec_dev, prior_mean_dev, prior_prec_dev, weights_dev, (long long)weight_stride, start_nu_dev,          \
                     start_delta_dev, tol, max_iter, nu_dev, delta_dev, cov_nu_dev, delta_var_dev, loglik_dev, dec_dev,                  \
                     (int*)iterations_dev, (int*)status_dev)
#define GLMBW_LAUNCH_H(H)                                                                                                                \
  do {                                                                                                                                  \
    if (noise == VC_NOISE_NB) { if (u16) GLMBW_LAUNCH(H, VC_NOISE_NB, true); else GLMBW_LAUNCH(H, VC_NOISE_NB, false); }                   \
    else { if (u16) GLMBW_LAUNCH(H, VC_NOISE_POISSON, true); else GLMBW_LAUNCH(H, VC_NOISE_POISSON, false); }                              \
  } while (0)
  const bool u16 = count_kind == VC_COUNTS_U16;
  for (int64_t g0 = 0; g0 < Ng; g0 += GLMBW_SLAB) {                // every slab reads and writes at its genes' own places
    const int64_t n = Ng - g0 < GLMBW_SLAB ? Ng - g0 : GLMBW_SLAB;
    const dim3 grid((unsigned)R, (unsigned)n);
    switch (K) {
      case 1: GLMBW_LAUNCH_H(0); break;
      case 3: GLMBW_LAUNCH_H(1); break;
      case 5: GLMBW_LAUNCH_H(2); break;
      default: GLMBW_LAUNCH_H(3); break;
    }
  }
#undef GLMBW_LAUNCH_H
#undef GLMBW_LAUNCH
  return gene_launched(GLMBW_FN);
}
