// Batch-aware per-gene harmonic regression: vc_gene_glm_batch of include/velocycle_hip.h.  The model of vc_gene_glm with the phase
// model's per-batch offsets (ElogS = nu . zeta(phi) + Db . dnu + count_factor), nu and the offsets estimated jointly per gene.
// Stand-alone: no engine, no workspace, one launch; the whole damped Newton iteration of a gene runs inside its workgroup.
//
// Per gene g, cells sorted by batch (batch b owns the cells [seg[b], seg[b + 1])):  maximise over nu (K = 2H+1) and delta (Nb)
//   L(nu, delta)       vc_gene_glm's Poisson / negative-binomial objective at  eta_c = nu . B[:, c] + delta_b(c) + logm_c
//   minus              sum_b q_b (delta_b - m_b)^2 / 2                 (always: it is what tells nu_0 from the mean of delta)
//   minus              sum_i prec_i (nu_i - m_i)^2 / 2                 (optional, as in vc_gene_glm)
// The objective stays concave: the offsets enter eta linearly.
//
// Mapping: vc_gene_glm's (glm_sweep of vc_gene_glm_math.h per element, gene_fold of vc_gene_math.h).  A pass walks the segments one after the
// other with nu_0 + delta_b for nu_0 and folds after each; the sums of a segment are those of a whole pass of vc_gene_glm, and because
// b_0 = 1 their column 0 is the delta block:  sum res = dL/d delta_b,  sum w B_i = h_b (the cross column; h_b0 = W_b = sum w),
// N[0] the rounding scale of dL/d delta_b.  Thread 0 adds the segment to the gene's totals in the LDS (segments in order: fixed bits) and
// files the K + 2 numbers of the block there; after the last segment every lane reads the totals back and runs the same float64 algebra.
//
// Algebra: the delta block of the Hessian is diagonal, D_b = W_b + q_b, so the step is a Schur complement,
//   S = H_nunu - sum_b h_b h_b' / D_b,   rhs = g_nu - sum_b h_b g_b / D_b,   dnu = S^-1 rhs,   ddelta_b = (g_b - h_b . dnu) / D_b
// with row and column 0 formed without cancellation (W_b is 10^4..10^6 against q_b ~ 4):
//   S_0j = sum_b h_bj q_b / D_b (+ prec_0 at j = 0),   rhs_0 = sum_b q_b ((delta_b - m_b) + g_b / D_b) - prec_0 (nu_0 - m_0)
// dec = g' H^-1 g = rhs . dnu + sum_b g_b^2 / D_b.  cov_nu = S^-1; delta_var_b = 1 / D_b + h_b' S^-1 h_b / D_b^2.
//
// Rules: vc_gene_glm's, over the K + Nb coefficients.  start nu_0 = ln(sum k / sum e^logm), harmonics 0 (prior means), delta = m;
// SINGULAR when a D_b or a pivot of S is not a positive finite number (a q_b or m_b that is not: the same); CONVERGED on dec <= tol;
// ROUNDING when every one of the K + Nb gradient entries is within 4 eps32 sqrt(N_i); MAX_ITER; the full step halved on the penalised
// objective (30 halvings per gene); UNBOUNDED when a harmonic or a delta_b of a trial leaves [-50, 50], or the gene has no count.
#include "vc_gene_glm_math.h"                     // glm_sweep, glm_prior and the packed algebra, shared with vc_gene_glm.hip; through it vc_gene_math.h

#pragma clang fp contract(off)

namespace {

struct GlmSeg {                                  // the segment offsets travel in the kernel's arguments: no device array, no copy
  long long s[VC_GLM_MAX_BATCHES + 1];
};

template <int K>
struct GlmbLds {
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
__device__ __forceinline__ bool glmb_block(const GlmbLds<K>& s, int b, double db, double& dm, double& gb, double& iD) {
  const double q = s.q[b], m = s.m[b];
  dm = db - m;
  gb = __builtin_fma(-q, dm, s.res[b]);
  const double D = s.h[b][0] + q;
  const bool ok = D > 0.0 && D < 1.0e300 && q > 0.0 && q < 1.0e300 && __builtin_fabs(m) < 1.0e300;
  iD = 1.0 / (ok ? D : 1.0);
  return ok;
}

// One pass at (nu, s.trial): acc = the gene's totals [g (K) | H packed (NH) | L | A | N (K)] in every lane, the delta block in s
template <int H, int NOISE, bool U16>
__device__ __forceinline__ void glmb_pass(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                          const float* __restrict__ logm, float r, double lnr, const double (&nu)[2 * H + 1], int Nb,
                                          const GlmSeg& seg, GlmbLds<2 * H + 1>& s, double* gsum, double (&acc)[GlmSums<H>::N],
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
    glm_sweep<H, NOISE, U16>(row, seg.s[b], seg.s[b + 1], Nc, B, logm, r, lnr, nub, acc);
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
__device__ __forceinline__ bool glmb_factor(const double (&acc)[GlmSums<H>::N], const double (&nu)[2 * H + 1], const double (&pm)[2 * H + 1],
                                            const double (&pp)[2 * H + 1], int Nb, const GlmbLds<2 * H + 1>& s, const double* dl,
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
    ok = glmb_block<K>(s, b, dl[b], dm, gb, iD) && ok;
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
__global__ __launch_bounds__(GENE_NT) void vc_gene_glm_batch_kernel(
    const void* __restrict__ counts, long long Nc, long long gene_stride, const float* __restrict__ B, const float* __restrict__ logm,
    const float* __restrict__ rg, int Nb, const GlmSeg seg, const double* __restrict__ delta_mean, const double* __restrict__ delta_prec,
    const double* __restrict__ prior_mean, const double* __restrict__ prior_prec, double tol, int max_iter, double* __restrict__ nu_out,
    double* __restrict__ delta_out, double* __restrict__ cov_out, double* __restrict__ dvar_out, double* __restrict__ loglik_out,
    double* __restrict__ dec_out, int* __restrict__ iter_out, int* __restrict__ status_out) {
  typedef GlmSums<H> S;
  constexpr int K = S::K, NH = S::NH;
  __shared__ double part[GENE_NW][S::N];
  __shared__ double tot[S::N];
  __shared__ double gsum[S::N];
  __shared__ GlmbLds<K> s;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tb = threadIdx.x;                                        // the batch this thread looks after (tb < Nb)
  const long long g = blockIdx.x;
  const void* row = U16 ? (const void*)((const unsigned short*)counts + g * gene_stride) : (const void*)((const float*)counts + g * gene_stride);
  const float r = NOISE == VC_NOISE_NB ? rg[g] : 0.f;
  const double lnr = NOISE == VC_NOISE_NB ? log((double)r) : 0.0;
  const double nan = __builtin_nan("");

  double pm[K], pp[K];                                              // the prior of nu
#pragma unroll
  for (int i = 0; i < K; ++i) glm_prior(prior_mean, prior_prec, g * K + i, pm[i], pp[i]);
  if (tb < Nb) {
    const double m = delta_mean[g * Nb + tb];
    s.m[tb] = m;
    s.q[tb] = delta_prec[g * Nb + tb];
    s.delta[tb] = m;
    s.trial[tb] = m;
    s.step[tb] = 0.0;
  }

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
        for (int i = 0; i < K; ++i) nu_out[g * K + i] = i == 0 ? nu[0] : 0.0;
        for (int i = 0; i < NH; ++i) cov_out[g * NH + i] = nan;
        loglik_out[g] = nan;
        dec_out[g] = nan;
        iter_out[g] = 0;
        status_out[g] = VC_GLM_UNBOUNDED;
      }
      if (tb < Nb) {
        delta_out[g * Nb + tb] = s.m[tb];
        dvar_out[g * Nb + tb] = nan;
      }
      return;
    }
  }

  double acc[S::N];
  glmb_pass<H, NOISE, U16>(row, Nc, B, logm, r, lnr, nu, Nb, seg, s, gsum, acc, part, tot, lane, wave);
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
    have_chol = glmb_factor<H>(acc, nu, pm, pp, Nb, s, s.delta, gr, rhs, chol, pen, gd2, delta_noise);
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
      glmb_block<K>(s, tb, s.delta[tb], dm, gb, iD);
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
      glmb_pass<H, NOISE, U16>(row, Nc, B, logm, r, lnr, trial, Nb, seg, s, gsum, acc, part, tot, lane, wave);
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
        glmb_pass<H, NOISE, U16>(row, Nc, B, logm, r, lnr, nu, Nb, seg, s, gsum, acc, part, tot, lane, wave);
        Lcur = acc[S::OFF_L];
        have_chol = glmb_factor<H>(acc, nu, pm, pp, Nb, s, s.delta, gr, rhs, chol, pen, gd2, delta_noise);
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
      glmb_block<K>(s, tb, s.delta[tb], dm, gb, iD);
#pragma unroll
      for (int i = 0; i < K; ++i) x[i] = s.h[tb][i];
      glm_solve<K>(chol, x);
      double hSh = 0.0;
#pragma unroll
      for (int i = 0; i < K; ++i) hSh = __builtin_fma(s.h[tb][i], x[i], hSh);
      var = __builtin_fma(hSh * iD, iD, iD);
    }
    delta_out[g * Nb + tb] = s.delta[tb];
    dvar_out[g * Nb + tb] = var;
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

constexpr char GLMB_FN[] = "vc_gene_glm_batch";

}  // namespace

extern "C" int vc_gene_glm_batch(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev,
                                 int K, const float* logm_dev, int noise, const float* r_dev, int Nb, const int64_t* seg_host,
                                 const double* delta_prior_mean_dev, const double* delta_prior_prec_dev, const double* prior_mean_dev,
                                 const double* prior_prec_dev, double tol, int max_iter, double* nu_dev, double* delta_dev, double* cov_nu_dev,
                                 double* delta_var_dev, double* loglik_dev, double* dec_dev, int32_t* iterations_dev, int32_t* status_dev,
                                 void* hip_stream) {
  const int refused = gene_refuse(GLMB_FN, noise, count_kind, K != 1 && K != 3 && K != 5 && K != 7 ? "K must be 1, 3, 5 or 7 (2 H + 1, H in 0..3)" : nullptr,
                                  Ng, Nc, false, gene_stride, 1, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (Nb < 1 || Nb > VC_GLM_MAX_BATCHES) return gene_fail(GLMB_FN, VC_ERR_ARG, "Nb must be in 1..VC_GLM_MAX_BATCHES");
  if (!counts_dev || !basis_dev || !logm_dev || !seg_host) return gene_fail(GLMB_FN, VC_ERR_ARG, "null input pointer");
  if (!delta_prior_mean_dev || !delta_prior_prec_dev)
    return gene_fail(GLMB_FN, VC_ERR_ARG, "every batch offset needs its prior (delta_prior_mean_dev, delta_prior_prec_dev)");
  if (!nu_dev || !delta_dev || !cov_nu_dev || !delta_var_dev || !loglik_dev || !dec_dev || !iterations_dev || !status_dev)
    return gene_fail(GLMB_FN, VC_ERR_ARG, "null output pointer");
  if (noise == VC_NOISE_NB && !r_dev) return gene_fail(GLMB_FN, VC_ERR_ARG, "the negative binomial needs r_dev (1 / dispersion per gene)");
  if ((prior_mean_dev == nullptr) != (prior_prec_dev == nullptr)) return gene_fail(GLMB_FN, VC_ERR_ARG, "the prior of nu needs both its means and its precisions");
  GlmSeg seg;
  for (int b = 0; b <= VC_GLM_MAX_BATCHES; ++b) seg.s[b] = b <= Nb ? (long long)seg_host[b] : (long long)Nc;
  if (seg.s[0] != 0 || seg.s[Nb] != (long long)Nc) return gene_fail(GLMB_FN, VC_ERR_ARG, "seg must start at 0 and end at Nc");
  for (int b = 0; b < Nb; ++b) {
    if (seg.s[b + 1] < seg.s[b]) return gene_fail(GLMB_FN, VC_ERR_ARG, "seg must be non-decreasing");
    if (seg.s[b + 1] == seg.s[b]) return gene_fail(GLMB_FN, VC_ERR_ARG, "empty segment (a batch without a cell)");
  }
  const dim3 grid((unsigned)Ng), block(GENE_NT);
  hipStream_t st = (hipStream_t)hip_stream;
#define GLMB_LAUNCH(H, NOISE, U16)                                                                                                     \
  hipLaunchKernelGGL((vc_gene_glm_batch_kernel<H, NOISE, U16>), grid, block, 0, st, counts_dev, (long long)Nc, (long long)gene_stride, \
                     basis_dev, logm_dev, r_dev, Nb, seg, delta_prior_mean_dev, delta_prior_prec_dev, prior_mean_dev, prior_prec_dev,  \
                     tol, max_iter, nu_dev, delta_dev, cov_nu_dev, delta_var_dev, loglik_dev, dec_dev, (int*)iterations_dev,            \
                     (int*)status_dev)
#define GLMB_LAUNCH_H(H)                                                                                                              \
  do {                                                                                                                                \
    if (noise == VC_NOISE_NB) { if (u16) GLMB_LAUNCH(H, VC_NOISE_NB, true); else GLMB_LAUNCH(H, VC_NOISE_NB, false); }                   \
    else { if (u16) GLMB_LAUNCH(H, VC_NOISE_POISSON, true); else GLMB_LAUNCH(H, VC_NOISE_POISSON, false); }                              \
  } while (0)
  const bool u16 = count_kind == VC_COUNTS_U16;
  switch (K) {
    case 1: GLMB_LAUNCH_H(0); break;
    case 3: GLMB_LAUNCH_H(1); break;
    case 5: GLMB_LAUNCH_H(2); break;
    default: GLMB_LAUNCH_H(3); break;
  }
#undef GLMB_LAUNCH_H
#undef GLMB_LAUNCH
  return gene_launched(GLMB_FN);
}
