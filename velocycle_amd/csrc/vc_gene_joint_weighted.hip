// Joint per-gene fit of the harmonics and the kinetics with case weights: vc_gene_joint_weighted of include/velocycle_hip.h.  The model,
// the mapping of a gene's two rows onto a workgroup, the iteration over theta = (nu [K], x = log gamma, y = log beta) and its status
// codes are those written at the head of vc_gene_joint.hip; every cell's contribution is multiplied by a weight w_bc >= 0 read from row
// b of a float32 table, and one call solves R rows of weights for every gene (the cell bootstrap of the joint fit and of its MAP angular
// speed: Poisson(1) integer weights per row; a held-out fit: 0 / 1; the caller's weights).  It takes from vc_gene_joint the step
// vc_gene_kinetics_weighted takes from vc_gene_kinetics.
//
// Sums, wt = (double)w_bc: every sum of a regular pass, of the Fisher pass, of the start's walk and of the profile pass takes its element
// times wt --
//   res -> wt res,  w -> wt w,  wo -> wt wo  of both layers (so G, O, F, the score and the information of nuw),
//   L_S, L_U = sum wt term (the negative binomial's r ln r is inside term: weighted with it),  A = sum wt |terms|,
//   rounding scales  N_i = sum ((wt woS)^2 + (wt resS)^2) gS_i^2 + ((wt woU)^2 + (wt resU)^2) gU_i^2,
//   n_clamped = the cells with w > 0 and z <= 0,
//   default start nu_0 = ln(sum wt k_S / sum wt e^logm),  y = ln(sum wt e^etaS zp / sum wt k_U).
// The priors are not weighted.  Each product with wt is formed first (exact at wt == 1) and the float64 operations that follow are those
// of jnt_pass / jnt_fisher in the same order, so a table of ones gives vc_gene_joint's bits.  The weight is one float32 load per cell,
// multiplied into the six float32 factors as they are widened: no accumulator is added to a pass.
//
// Per-row inputs: the angular speed's coefficients and the start may each differ from row to row (a stride in numbers from one row's
// table to the next; 0: shared) -- every replicate of an outer iteration at its own nuw and its own previous theta.  There is no nu
// table: nu is an unknown here.  The priors are shared by the rows.
//
// Mapping: one workgroup of GENE_NW waves per (gene, row), grid = (R, genes) with the row in x, the fast index (the workgroups in
// flight share a gene's two count rows and stream the weight table, as in vc_gene_kinetics_weighted).  gridDim.y holds at most 65535
// genes, so the entry point launches slabs of JNTW_SLAB genes one after the other on the stream (g_base: the slab's first gene);
// R <= 65535 keeps gridDim.x * blockDim.x below 2^32.  Float64 per-lane sums, shuffle tree, waves in wave order through the LDS: no
// atomics, identical bits on repetition and under any cutting of genes or rows into calls.
//
// JntwDims, jntw_cell, jntw_dc, jntw_rows and the iteration below are vc_gene_joint.hip's, statement for statement, with jnt_pass and
// jnt_fisher replaced by their weighted forms: that file's gfx950 assembly may not move, so nothing of it was factored out.  A change to
// the step or stopping rules has to be made in both files.
#include "vc_gene_glm_math.h"                     // vc_gene_math.h (gene_count, gene_exp_f32, gene_lik, gene_fold, the refusals) and glm_tri, glm_chol, glm_solve

// every product-sum is written as the fma it is meant to be; nothing else may be contracted (the same operations in every instantiation)
#pragma clang fp contract(off)

namespace {

constexpr int JNTW_MAX_HALVINGS = 30;
constexpr double JNTW_BOUND = 30.0;       // x, y; nu is held to GLM_BOUND
constexpr double JNTW_FLOOR = 1.0e-5;     // the model's relu(z) + 1e-5

template <int H, int NW>
struct JntwDims {
  static constexpr int K = 2 * H + 1;
  static constexpr int D = K + 2;                     // theta = (nu, x, y): x at K, y at K + 1
  static constexpr int NHD = D * (D + 1) / 2;
  static constexpr int NWA = NW > 0 ? NW : 1;
  static constexpr int NWH = NWA * (NWA + 1) / 2;
  // sums of the regular pass: gradient, observed matrix (packed), rounding scales, the two objectives, sum |terms|, clamped cells
  static constexpr int OFF_G = 0, OFF_O = D, OFF_N = OFF_O + NHD, OFF_LS = OFF_N + D, OFF_LU = OFF_LS + 1, OFF_A = OFF_LU + 1,
                       OFF_C = OFF_A + 1, NACC = OFF_C + 1;
  // sums of the Fisher pass: F (packed); the profile pass adds the score, I_ww (packed) and I_wt (row i: the K + 2 of nuw_i)
  static constexpr int P_F = 0, P_S = NHD, P_I = P_S + NWA, P_X = P_I + NWH, NPRO = P_X + NWA * D;
  static constexpr int NLDS = NACC > NPRO ? NACC : NPRO;
};

// What a cell contributes through the link, float64 except m0
struct JntwCell {
  double etaS;
  double e0;           // etaS - y
  double d, om, zp;
  bool a;
  float m0;            // e^(etaS - y), one float32 rounding
};

template <int H, int NW>
__device__ __forceinline__ JntwCell jntw_cell(const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ W,
                                              long long Nc, long long c, const double (&nu)[2 * H + 1], const double (&dc)[2 * H + 1],
                                              const double (&nuw)[JntwDims<H, NW>::NWA], double ex, double y, double (&b)[2 * H + 1],
                                              double (&wr)[JntwDims<H, NW>::NWA]) {
  constexpr int K = 2 * H + 1;
  b[0] = 1.0;
#pragma unroll
  for (int i = 1; i < K; ++i) b[i] = (double)B[(long long)i * Nc + c];
  double eta = (double)logm[c] + nu[0];
  double d = 0.0;
#pragma unroll
  for (int i = 1; i < K; ++i) {
    eta = __builtin_fma(nu[i], b[i], eta);
    d = __builtin_fma(dc[i], b[i], d);
  }
  double om = 0.0;
  wr[0] = 0.0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    wr[i] = (double)W[(long long)i * Nc + c];
    om = __builtin_fma(nuw[i], wr[i], om);
  }
  JntwCell o;
  const double z = __builtin_fma(om, d, ex);
  o.a = z > 0.0;
  o.zp = o.a ? z + JNTW_FLOOR : JNTW_FLOOR;
  o.d = d;
  o.om = om;
  o.etaS = eta;
  o.e0 = eta - y;
  o.m0 = gene_exp_f32(o.e0);
  return o;
}

// d = sum_{i >= 1} dc[i] b[i]: dc[2h] = h nu[2h - 1] (cos row), dc[2h - 1] = -h nu[2h] (sin row)
template <int H>
__device__ __forceinline__ void jntw_dc(const double (&nu)[2 * H + 1], double (&dc)[2 * H + 1]) {
  dc[0] = 0.0;
#pragma unroll
  for (int h = 1; h <= H; ++h) {
    dc[2 * h] = (double)h * nu[2 * h - 1];
    dc[2 * h - 1] = -(double)h * nu[2 * h];
  }
}

// gU = (b + s db, p, -1) and u = (s db, p) of a cell (u_0 = 0, u_y = 0 are not stored)
template <int H>
__device__ __forceinline__ void jntw_rows(const double (&b)[2 * H + 1], double s, double p, double (&gU)[2 * H + 3], double (&u)[2 * H + 2]) {
  constexpr int K = 2 * H + 1;
  u[0] = 0.0;
#pragma unroll
  for (int h = 1; h <= H; ++h) {
    u[2 * h - 1] = s * ((double)h * b[2 * h]);
    u[2 * h] = s * (-(double)h * b[2 * h - 1]);
  }
  u[K] = p;
  gU[0] = 1.0;
#pragma unroll
  for (int i = 1; i < K; ++i) gU[i] = b[i] + u[i];
  gU[K] = p;
  gU[K + 1] = -1.0;
}

// One regular pass over both rows of the gene at th under the row's weights: the NACC sums, folded over the workgroup
template <int H, int NW, int NOISE, bool U16>
__device__ __forceinline__ void jntw_pass(const void* __restrict__ rowS, const void* __restrict__ rowU, long long Nc,
                                          const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ W,
                                          const float* __restrict__ wrow, const double (&th)[2 * H + 3],
                                          const double (&nuw)[JntwDims<H, NW>::NWA], float r, double lnr,
                                          double (&acc)[JntwDims<H, NW>::NACC], double (*part)[JntwDims<H, NW>::NLDS], double* tot,
                                          int lane, int wave) {
  typedef JntwDims<H, NW> S;
  constexpr int K = S::K, D = S::D;
#pragma unroll
  for (int i = 0; i < S::NACC; ++i) acc[i] = 0.0;
  double nu[K], dc[K];
#pragma unroll
  for (int i = 0; i < K; ++i) nu[i] = th[i];
  jntw_dc<H>(nu, dc);
  const double x = th[K], y = th[K + 1];
  const double ex = exp(x);
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float kS = gene_count<U16>(rowS, c);
    const float k = gene_count<U16>(rowU, c);
    const double wt = (double)wrow[c];
    double b[K], wr[S::NWA];
    const JntwCell cl = jntw_cell<H, NW>(B, logm, W, Nc, c, nu, dc, nuw, ex, y, b, wr);
    // the spliced element: glm_sweep's
    const float muS = gene_exp_f32(cl.etaS);
    float resS, wS, woS;
    double termS, magS;
    gene_lik<NOISE>(kS, muS, cl.etaS, r, lnr, resS, wS, woS, termS, magS);
    // the unspliced element: kin_pass's
    const float zpf = (float)cl.zp;
    const float mu = cl.m0 * zpf;
    const double etaU = cl.e0 + (double)(VC_LN2 * __builtin_amdgcn_logf(zpf));
    float res, w, wo;
    double term, mag;
    gene_lik<NOISE>(k, mu, etaU, r, lnr, res, w, wo, term, mag);
    const double p = cl.a ? ex / cl.zp : 0.0;
    const double s = cl.a ? cl.om / cl.zp : 0.0;
    double gU[D], u[K + 1];
    jntw_rows<H>(b, s, p, gU, u);
    const double rS = wt * (double)resS, oS = wt * (double)woS, rd = wt * (double)res, od = wt * (double)wo;
    const double n2S = __builtin_fma(oS, oS, rS * rS), n2 = __builtin_fma(od, od, rd * rd);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      // gradient and rounding scale
      if (i < K) {
        acc[S::OFF_G + i] = __builtin_fma(rS, b[i], acc[S::OFF_G + i]);
        acc[S::OFF_N + i] = __builtin_fma(n2S, b[i] * b[i], acc[S::OFF_N + i]);
      }
      acc[S::OFF_G + i] = __builtin_fma(rd, gU[i], acc[S::OFF_G + i]);
      acc[S::OFF_N + i] = __builtin_fma(n2, gU[i] * gU[i], acc[S::OFF_N + i]);
      // observed matrix, row i of the packed lower triangle
      const double og = od * gU[i];
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double v = acc[S::OFF_O + glm_tri(i, j)];
        if (i < K) v = __builtin_fma(oS * b[i], b[j], v);
        v = __builtin_fma(og, gU[j], v);
        if (i <= K && i > 0 && j > 0) v = __builtin_fma(rd * u[i], u[j], v);
        acc[S::OFF_O + glm_tri(i, j)] = v;
      }
    }
    acc[S::OFF_O + glm_tri(K, K)] = __builtin_fma(-rd, p, acc[S::OFF_O + glm_tri(K, K)]);
    acc[S::OFF_LS] += wt * termS;
    acc[S::OFF_LU] += wt * term;
    acc[S::OFF_A] += wt * magS + wt * mag;
    acc[S::OFF_C] += cl.a || !(wt > 0.0) ? 0.0 : 1.0;
  }
  gene_fold<S::NACC, S::NLDS>(acc, part, tot, lane, wave);
  __syncthreads();                                                   // part / tot are written again by the next fold
}

// The Fisher pass at th under the row's weights: F = sum (wt wS) gS gS' + (wt wU) gU gU' (packed, without Lambda).  PROFILE: also
// score_i = sum (wt resU) q W_i, I_ww = sum (wt wU) q^2 W_i W_j (packed) and I_wt[i] = sum (wt wU) q W_i gU, q = a d / zp
template <int H, int NW, int NOISE, bool U16, bool PROFILE>
__device__ __forceinline__ void jntw_fisher(const void* __restrict__ rowS, const void* __restrict__ rowU, long long Nc,
                                            const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ W,
                                            const float* __restrict__ wrow, const double (&th)[2 * H + 3],
                                            const double (&nuw)[JntwDims<H, NW>::NWA], float r, double lnr,
                                            double (&fa)[PROFILE ? JntwDims<H, NW>::NPRO : JntwDims<H, NW>::NHD],
                                            double (*part)[JntwDims<H, NW>::NLDS], double* tot, int lane, int wave) {
  typedef JntwDims<H, NW> S;
  constexpr int K = S::K, D = S::D, N = PROFILE ? S::NPRO : S::NHD;
#pragma unroll
  for (int i = 0; i < N; ++i) fa[i] = 0.0;
  double nu[K], dc[K];
#pragma unroll
  for (int i = 0; i < K; ++i) nu[i] = th[i];
  jntw_dc<H>(nu, dc);
  const double x = th[K], y = th[K + 1];
  const double ex = exp(x);
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float kS = gene_count<U16>(rowS, c);
    const float k = gene_count<U16>(rowU, c);
    const double wt = (double)wrow[c];
    double b[K], wr[S::NWA];
    const JntwCell cl = jntw_cell<H, NW>(B, logm, W, Nc, c, nu, dc, nuw, ex, y, b, wr);
    const float muS = gene_exp_f32(cl.etaS);
    float resS, wS, woS;
    double termS, magS;
    gene_lik<NOISE>(kS, muS, cl.etaS, r, lnr, resS, wS, woS, termS, magS);
    const float zpf = (float)cl.zp;
    const float mu = cl.m0 * zpf;
    const double etaU = cl.e0 + (double)(VC_LN2 * __builtin_amdgcn_logf(zpf));
    float res, w, wo;
    double term, mag;
    gene_lik<NOISE>(k, mu, etaU, r, lnr, res, w, wo, term, mag);
    const double izp = 1.0 / cl.zp;
    const double p = cl.a ? ex * izp : 0.0, s = cl.a ? cl.om * izp : 0.0;
    double gU[D], u[K + 1];
    jntw_rows<H>(b, s, p, gU, u);
    const double fS = wt * (double)wS, wd = wt * (double)w;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double wg = wd * gU[i];
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double v = fa[S::P_F + glm_tri(i, j)];
        if (i < K) v = __builtin_fma(fS * b[i], b[j], v);
        fa[S::P_F + glm_tri(i, j)] = __builtin_fma(wg, gU[j], v);
      }
    }
    if (PROFILE) {
      const double q = cl.a ? cl.d * izp : 0.0;
      const double rq = (wt * (double)res) * q, wq = wd * q;
#pragma unroll
      for (int i = 0; i < S::NWA; ++i) {
        fa[S::P_S + i] = __builtin_fma(rq, wr[i], fa[S::P_S + i]);
        const double wqi = wq * wr[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) fa[S::P_I + glm_tri(i, j)] = __builtin_fma(wqi * q, wr[j], fa[S::P_I + glm_tri(i, j)]);
#pragma unroll
        for (int j = 0; j < D; ++j) fa[S::P_X + i * D + j] = __builtin_fma(wqi, gU[j], fa[S::P_X + i * D + j]);
      }
    }
  }
  gene_fold<N, S::NLDS>(fa, part, tot, lane, wave);
  __syncthreads();                                                   // part / tot are written again by the next fold
}

template <int H, int NW, int NOISE, bool U16>
__global__ __launch_bounds__(GENE_NT) void vc_gene_joint_weighted_kernel(
    const void* __restrict__ counts_s, const void* __restrict__ counts_u, long long g_base, long long Ng, long long Nc,
    long long gene_stride, const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ W,
    const double* __restrict__ nuw_in, long long nuw_row_stride, const float* __restrict__ rg, const double* __restrict__ prior_mean,
    const double* __restrict__ prior_prec, const double* __restrict__ prior, const float* __restrict__ weights, long long weight_stride,
    const double* __restrict__ start, long long start_row_stride, double tol, int max_iter, double* __restrict__ theta_out,
    double* __restrict__ cov_out, double* __restrict__ lls_out, double* __restrict__ llu_out, double* __restrict__ dec_out,
    int* __restrict__ iter_out, int* __restrict__ status_out, int* __restrict__ clamped_out, double* __restrict__ score_out,
    double* __restrict__ info_out) {
  typedef JntwDims<H, NW> S;
  constexpr int K = S::K, D = S::D, NHD = S::NHD, NWA = S::NWA, NWH = S::NWH;
  __shared__ double part[GENE_NW][S::NLDS];
  __shared__ double tot[S::NLDS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long g = g_base + blockIdx.y, bw = blockIdx.x;          // the row is the fast index
  const long long at = bw * Ng + g;                                  // the (row, gene) pair's place in every output
  const void* rowS = U16 ? (const void*)((const unsigned short*)counts_s + g * gene_stride) : (const void*)((const float*)counts_s + g * gene_stride);
  const void* rowU = U16 ? (const void*)((const unsigned short*)counts_u + g * gene_stride) : (const void*)((const float*)counts_u + g * gene_stride);
  const float* wrow = weights + bw * weight_stride;
  const double nan = __builtin_nan("");

  // the priors: means pm and precisions pp of theta (shared by the rows, not weighted)
  double pm[D], pp[D];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    pm[i] = prior_mean[g * K + i];
    pp[i] = prior_prec[g * K + i];
    finite = finite && __builtin_fabs(pm[i]) < 1.0e300 && pp[i] > 0.0 && pp[i] < 1.0e300;
  }
  {
    const double mx = prior[g * 4 + 0], sx = prior[g * 4 + 1], my = prior[g * 4 + 2], sy = prior[g * 4 + 3];
    finite = finite && __builtin_fabs(mx) < 1.0e300 && __builtin_fabs(my) < 1.0e300 && sx > 0.0 && sx < 1.0e300 && sy > 0.0 && sy < 1.0e300;
    pm[K] = mx;
    pm[K + 1] = my;
    pp[K] = 1.0 / (sx * sx);
    pp[K + 1] = 1.0 / (sy * sy);
    finite = finite && pp[K] < 1.0e300 && pp[K + 1] < 1.0e300;
  }
  double nuw[NWA];
  nuw[0] = 0.0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    nuw[i] = nuw_in[bw * nuw_row_stride + i];                        // a stride of 0: the table all rows share
    finite = finite && __builtin_fabs(nuw[i]) < 1.0e300;
  }
  const float r = NOISE == VC_NOISE_NB ? rg[g] : 1.f;
  const double lnr = NOISE == VC_NOISE_NB ? log((double)r) : 0.0;
  finite = finite && r > 0.f && r < 3.0e38f;

  // the start: the row's start_dev where every entry of the gene is finite and inside the box, else the default
  // nu_0 = ln(sum wt k_S / sum wt e^logm), harmonics at their prior means, x = mu_gamma, y = ln(sum wt e^etaS zp / sum wt k_U), clipped
  // to the box; a pair without a weighted count in a layer has no fit, whatever the start
  double th[D];
  bool given = start != nullptr;
  if (start) {
    const double* sr = start + bw * start_row_stride;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      th[i] = sr[g * D + i];
      given = given && __builtin_fabs(th[i]) <= (i < K ? GLM_BOUND : JNTW_BOUND);     // false for a NaN
    }
  }
  if (finite) {
    double s3[3] = {0.0, 0.0, 0.0};
    for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
      const double wt = (double)wrow[c];
      s3[0] += wt * (double)gene_count<U16>(rowS, c);
      s3[1] += wt * (double)__builtin_amdgcn_exp2f(VC_LOG2E * logm[c]);
      s3[2] += wt * (double)gene_count<U16>(rowU, c);
    }
    gene_fold<3, S::NLDS>(s3, part, tot, lane, wave);
    __syncthreads();                                                 // part / tot are written again by the next fold
    finite = s3[0] > 0.0 && s3[0] < 1.0e300 && s3[2] > 0.0 && s3[2] < 1.0e300;        // false for a NaN weight
    if (finite && !given) {                                          // the same decision in every lane
#pragma unroll
      for (int i = 0; i < D; ++i) th[i] = pm[i];
      th[0] = log(s3[0] / s3[1]);
      finite = __builtin_fabs(th[0]) < 1.0e300;
#pragma unroll
      for (int i = 0; i <= K; ++i) {
        const double bound = i < K ? GLM_BOUND : JNTW_BOUND;
        th[i] = th[i] > bound ? bound : (th[i] < -bound ? -bound : th[i]);
      }
      double nu[K], dc[K];
#pragma unroll
      for (int i = 0; i < K; ++i) nu[i] = finite ? th[i] : 0.0;
      jntw_dc<H>(nu, dc);
      const double ex = exp(th[K]);
      double s1[1] = {0.0};
      for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
        const double wt = (double)wrow[c];
        double b[K], wr[NWA];
        const JntwCell cl = jntw_cell<H, NW>(B, logm, W, Nc, c, nu, dc, nuw, ex, 0.0, b, wr);
        s1[0] = __builtin_fma(wt * (double)cl.m0, cl.zp, s1[0]);
      }
      gene_fold<1, S::NLDS>(s1, part, tot, lane, wave);
      __syncthreads();                                               // part / tot are written again by the next fold
      const double y = log(s1[0] / s3[2]);
      finite = finite && __builtin_fabs(y) < 1.0e300;
      th[K + 1] = y > JNTW_BOUND ? JNTW_BOUND : (y < -JNTW_BOUND ? -JNTW_BOUND : y);
    }
  }
  if (!finite) {                                                     // the same decision in every lane
    if (threadIdx.x == 0) {
      for (int i = 0; i < D; ++i) theta_out[at * D + i] = nan;
      if (cov_out) for (int i = 0; i < NHD; ++i) cov_out[at * NHD + i] = nan;
      lls_out[at] = nan;
      llu_out[at] = nan;
      dec_out[at] = nan;
      iter_out[at] = 0;
      status_out[at] = VC_JNT_NO_DATA;
      clamped_out[at] = 0;
      for (int i = 0; i < NW; ++i) score_out[at * NW + i] = nan;
      for (int i = 0; i < NW * (NW + 1) / 2; ++i) info_out[at * (NW * (NW + 1) / 2) + i] = nan;
    }
    return;
  }

  // F + Lambda at th, factored into chol (the sums of the regular pass are dead by then: only what was taken from them is kept)
#define JNTW_FISHER()                                                                                                                  \
  do {                                                                                                                                 \
    double fa[NHD];                                                                                                                    \
    jntw_fisher<H, NW, NOISE, U16, false>(rowS, rowU, Nc, B, logm, W, wrow, th, nuw, r, lnr, fa, part, tot, lane, wave);               \
    _Pragma("unroll") for (int i = 0; i < NHD; ++i) chol[i] = fa[i];                                                                   \
    _Pragma("unroll") for (int i = 0; i < D; ++i) chol[glm_tri(i, i)] += pp[i];                                                        \
    have = glm_chol<D>(chol);                                                                                                          \
  } while (0)
#define JNTW_STEP()                                                                                                                    \
  do {                                                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < D; ++i) dx[i] = gr[i];                                                                       \
    glm_solve<D>(chol, dx);                                                                                                            \
    dec = 0.0;                                                                                                                         \
    inside = true;                                                                                                                     \
    _Pragma("unroll") for (int i = 0; i < D; ++i) {                                                                                    \
      dec = __builtin_fma(gr[i], dx[i], dec);                                                                                          \
      inside = inside && __builtin_fabs(th[i] + dx[i]) <= (i < K ? GLM_BOUND : JNTW_BOUND);                                            \
    }                                                                                                                                  \
  } while (0)

  enum { AT_POINT = 0, AT_TRIAL = 1, AT_LAST = 2 };                  // what the pass of this turn is for
  double acc[S::NACC], tr[D], dx[D], chol[NHD];
#pragma unroll
  for (int i = 0; i < D; ++i) tr[i] = th[i];
  int status = VC_JNT_MAX_ITER, steps = 0, halvings = JNTW_MAX_HALVINGS, mode = AT_POINT;
  double LS = 0.0, LU = 0.0, Acur = 0.0, clamped = 0.0, fcur = 0.0, dec = nan, t = 1.0;
  bool have = false, inside = true;
  for (;;) {
    jntw_pass<H, NW, NOISE, U16>(rowS, rowU, Nc, B, logm, W, wrow, tr, nuw, r, lnr, acc, part, tot, lane, wave);
    if (mode == AT_TRIAL) {
      double pen2 = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const double d = tr[i] - pm[i];
        pen2 = __builtin_fma(0.5 * pp[i] * d, d, pen2);
      }
      const double A = acc[S::OFF_A] > Acur ? acc[S::OFF_A] : Acur;
      if ((acc[S::OFF_LS] + acc[S::OFF_LU]) - pen2 >= fcur - 8.0 * GENE_EPS32 * A) {      // false for a NaN: such a step is halved
#pragma unroll
        for (int i = 0; i < D; ++i) th[i] = tr[i];
        ++steps;
      } else {
        if (halvings == 0) {                                         // a refused trial's sums are in acc: form those of th again, then stop
          status = VC_JNT_MAX_ITER;
          mode = AT_LAST;
#pragma unroll
          for (int i = 0; i < D; ++i) tr[i] = th[i];
          continue;
        }
        --halvings;
        t *= 0.5;
#pragma unroll
        for (int i = 0; i < D; ++i) tr[i] = __builtin_fma(t, dx[i], th[i]);               // between th and a point inside the box: inside
        continue;
      }
    }
    // acc holds the sums at th; only L_S, L_U, A and the count of clamped cells outlive the next pass
    LS = acc[S::OFF_LS];
    LU = acc[S::OFF_LU];
    Acur = acc[S::OFF_A];
    clamped = acc[S::OFF_C];
    double gr[D], pen = 0.0;
    bool noise = true;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double d = th[i] - pm[i];
      gr[i] = __builtin_fma(-pp[i], d, acc[S::OFF_G + i]);
      pen = __builtin_fma(0.5 * pp[i] * d, d, pen);
      noise = noise && __builtin_fabs(gr[i]) <= 4.0 * GENE_EPS32 * __builtin_sqrt(acc[S::OFF_N + i]);
    }
    fcur = (LS + LU) - pen;
#pragma unroll
    for (int i = 0; i < NHD; ++i) chol[i] = acc[S::OFF_O + i];
#pragma unroll
    for (int i = 0; i < D; ++i) chol[glm_tri(i, i)] += pp[i];
    const bool observed = glm_chol<D>(chol);
    have = observed;
    if (!observed) JNTW_FISHER();
    JNTW_STEP();
    if (mode == AT_LAST) break;
    if (max_iter == 0) { status = VC_JNT_EVALUATED; break; }
    if (!have || !(__builtin_fabs(dec) < 1.0e300)) { status = VC_JNT_MAX_ITER; break; }
    if (dec <= tol) { status = VC_JNT_CONVERGED; break; }
    if (noise) { status = VC_JNT_ROUNDING; break; }
    if (steps >= max_iter) { status = VC_JNT_MAX_ITER; break; }
    // a barely positive definite observed matrix throws the step out of the box: the Fisher step, which the priors bound, before giving up
    if (observed && !inside) {
      JNTW_FISHER();
      JNTW_STEP();
      if (!have || !(__builtin_fabs(dec) < 1.0e300)) { status = VC_JNT_MAX_ITER; break; }
    }
    if (!inside) { status = VC_JNT_UNBOUNDED; break; }
    t = 1.0;
#pragma unroll
    for (int i = 0; i < D; ++i) tr[i] = th[i] + dx[i];
    mode = AT_TRIAL;
  }
#undef JNTW_STEP

  // A^-1 of the last accepted point, column by column from the factor
  double cov[NHD];
  if (have) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double e[D];
#pragma unroll
      for (int i = 0; i < D; ++i) e[i] = i == j ? 1.0 : 0.0;
      glm_solve<D>(chol, e);
#pragma unroll
      for (int i = j; i < D; ++i) cov[glm_tri(i, j)] = e[i];
    }
  } else {
    dec = nan;
#pragma unroll
    for (int i = 0; i < NHD; ++i) cov[i] = nan;
  }

  // the pass at the returned point for nuw: score_i = sum (wt resU) q W_i and the profile information I_ww - I_wt (I_tt + Lambda)^-1 I_tw
  double score[NWA], info[NWH];
  if (NW > 0) {
    double fa[S::NPRO];
    jntw_fisher<H, NW, NOISE, U16, true>(rowS, rowU, Nc, B, logm, W, wrow, th, nuw, r, lnr, fa, part, tot, lane, wave);
    double fc[NHD];
#pragma unroll
    for (int i = 0; i < NHD; ++i) fc[i] = fa[S::P_F + i];
#pragma unroll
    for (int i = 0; i < D; ++i) fc[glm_tri(i, i)] += pp[i];
    const bool ok = glm_chol<D>(fc);
#pragma unroll
    for (int i = 0; i < NWA; ++i) {
      score[i] = fa[S::P_S + i];
      double v[D];                                                   // (I_tt + Lambda)^-1 I_tw, column i
#pragma unroll
      for (int j = 0; j < D; ++j) v[j] = fa[S::P_X + i * D + j];
      glm_solve<D>(fc, v);
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double sub = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) sub = __builtin_fma(fa[S::P_X + j * D + q], v[q], sub);
        info[glm_tri(i, j)] = ok ? fa[S::P_I + glm_tri(i, j)] - sub : nan;
      }
    }
  }
#undef JNTW_FISHER

  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < D; ++i) theta_out[at * D + i] = th[i];
    if (cov_out) {
#pragma unroll
      for (int i = 0; i < NHD; ++i) cov_out[at * NHD + i] = cov[i];
    }
    lls_out[at] = LS;
    llu_out[at] = LU;
    dec_out[at] = dec;
    iter_out[at] = steps;
    status_out[at] = status;
    clamped_out[at] = (int)clamped;
    if (NW > 0) {
#pragma unroll
      for (int i = 0; i < NWA; ++i) score_out[at * NWA + i] = score[i];
#pragma unroll
      for (int i = 0; i < NWH; ++i) info_out[at * NWH + i] = info[i];
    }
  }
}

constexpr char JNTW_FN[] = "vc_gene_joint_weighted";
constexpr int64_t JNTW_MAX_ROWS = 65535;          // gridDim.x, and 65535 * GENE_NT < 2^32
constexpr int64_t JNTW_SLAB = 65535;              // genes per launch: gridDim.y

}  // namespace

extern "C" int vc_gene_joint_weighted(const void* counts_s_dev, const void* counts_u_dev, int count_kind, int64_t Ng, int64_t Nc,
                                      int64_t gene_stride, const float* basis_dev, int K, const float* logm_dev, const float* w_dev, int NW,
                                      const double* nuw_dev, int64_t nuw_row_stride, int noise, const float* r_dev,
                                      const double* prior_mean_dev, const double* prior_prec_dev, const double* prior_dev,
                                      const float* weights_dev, int64_t R, int64_t weight_stride, const double* start_dev,
                                      int64_t start_row_stride, double tol, int max_iter, double* theta_dev, double* cov_dev,
                                      double* loglik_s_dev, double* loglik_u_dev, double* dec_dev, int32_t* iterations_dev,
                                      int32_t* status_dev, int32_t* n_clamped_dev, double* score_w_dev, double* info_w_dev,
                                      void* hip_stream) {
  const char* own = nullptr;                                         // what only this entry point says, reported in its place among the shared refusals
  if (K == 7) own = "K must be 3 or 5: H = 3 is not instantiated";
  else if (K != 3 && K != 5) own = "K must be 3 or 5 (2 H + 1, H in {1, 2}; H = 0 has no velocity)";
  else if (NW < 0 || NW > 3) own = "NW must be in 0..3 (rows of the angular speed's design)";
  const int refused = gene_refuse(JNTW_FN, noise, count_kind, own, Ng, Nc, true, gene_stride, 0, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (!counts_s_dev || !counts_u_dev || !basis_dev || !logm_dev || !prior_dev) return gene_fail(JNTW_FN, VC_ERR_ARG, "null input pointer");
  if (!prior_mean_dev || !prior_prec_dev)
    return gene_fail(JNTW_FN, VC_ERR_ARG, "null input pointer: prior_mean_dev and prior_prec_dev are required (without a prior on nu a gene with few cells has no maximum)");
  if (!theta_dev || !loglik_s_dev || !loglik_u_dev || !dec_dev || !iterations_dev || !status_dev || !n_clamped_dev)
    return gene_fail(JNTW_FN, VC_ERR_ARG, "null output pointer (only cov_dev may be NULL)");
  if (NW > 0 && (!w_dev || !nuw_dev)) return gene_fail(JNTW_FN, VC_ERR_ARG, "NW > 0 needs w_dev and nuw_dev");
  if (NW > 0 && (!score_w_dev || !info_w_dev)) return gene_fail(JNTW_FN, VC_ERR_ARG, "NW > 0 needs score_w_dev and info_w_dev (the NW outputs)");
  if (NW == 0 && (score_w_dev || info_w_dev)) return gene_fail(JNTW_FN, VC_ERR_ARG, "score_w_dev and info_w_dev need NW > 0 (the NW outputs)");
  if (noise == VC_NOISE_NB && !r_dev) return gene_fail(JNTW_FN, VC_ERR_ARG, "the negative binomial needs r_dev (1 / dispersion per gene)");
  if (max_iter == 0 && !start_dev) return gene_fail(JNTW_FN, VC_ERR_ARG, "max_iter == 0 (evaluate only) needs start_dev");
  if (!weights_dev) return gene_fail(JNTW_FN, VC_ERR_ARG, "null weights_dev");
  if (R < 1 || R > JNTW_MAX_ROWS) return gene_fail(JNTW_FN, VC_ERR_ARG, "R must be in 1..65535 rows of weights per call");
  if (weight_stride < Nc) return gene_fail(JNTW_FN, VC_ERR_ARG, "weight_stride < Nc");
  if (NW > 0 && nuw_row_stride != 0 && nuw_row_stride < NW) return gene_fail(JNTW_FN, VC_ERR_ARG, "nuw_row_stride must be 0 (shared) or >= NW");
  if (start_dev && start_row_stride != 0 && start_row_stride < Ng * (K + 2))
    return gene_fail(JNTW_FN, VC_ERR_ARG, "start_row_stride must be 0 (shared) or >= Ng * (K + 2)");
  const dim3 block(GENE_NT);
  hipStream_t st = (hipStream_t)hip_stream;
  const long long nuw_stride = NW > 0 ? (long long)nuw_row_stride : 0, start_stride = start_dev ? (long long)start_row_stride : 0;
#define JNTW_LAUNCH(H, NW_, NOISE, U16)                                                                                                \
  hipLaunchKernelGGL((vc_gene_joint_weighted_kernel<H, NW_, NOISE, U16>), grid, block, 0, st, counts_s_dev, counts_u_dev, (long long)g0, \
                     (long long)Ng, (long long)Nc, (long long)gene_stride, basis_dev, logm_dev, w_dev, nuw_dev, nuw_stride, r_dev,     \
                     prior_mean_dev, prior_prec_dev, prior_dev, weights_dev, (long long)weight_stride, start_dev, start_stride, tol,   \
                     max_iter, theta_dev, cov_dev, loglik_s_dev, loglik_u_dev, dec_dev, (int*)iterations_dev, (int*)status_dev,        \
                     (int*)n_clamped_dev, score_w_dev, info_w_dev)
#define JNTW_LAUNCH_S(H, NW_)                                                                                                         \
  do {                                                                                                                                \
    if (noise == VC_NOISE_NB) { if (u16) JNTW_LAUNCH(H, NW_, VC_NOISE_NB, true); else JNTW_LAUNCH(H, NW_, VC_NOISE_NB, false); }         \
    else { if (u16) JNTW_LAUNCH(H, NW_, VC_NOISE_POISSON, true); else JNTW_LAUNCH(H, NW_, VC_NOISE_POISSON, false); }                    \
  } while (0)
#define JNTW_LAUNCH_H(H)                                                                                                              \
  switch (NW) {                                                                                                                       \
    case 0: JNTW_LAUNCH_S(H, 0); break;                                                                                               \
    case 1: JNTW_LAUNCH_S(H, 1); break;                                                                                               \
    case 2: JNTW_LAUNCH_S(H, 2); break;                                                                                               \
    default: JNTW_LAUNCH_S(H, 3); break;                                                                                              \
  }
  const bool u16 = count_kind == VC_COUNTS_U16;
  for (int64_t g0 = 0; g0 < Ng; g0 += JNTW_SLAB) {                 // every slab reads and writes at its genes' own places
    const int64_t n = Ng - g0 < JNTW_SLAB ? Ng - g0 : JNTW_SLAB;
    const dim3 grid((unsigned)R, (unsigned)n);
    if (K == 3) { JNTW_LAUNCH_H(1) } else { JNTW_LAUNCH_H(2) }
  }
#undef JNTW_LAUNCH_H
#undef JNTW_LAUNCH_S
#undef JNTW_LAUNCH
  return gene_launched(JNTW_FN);
}
