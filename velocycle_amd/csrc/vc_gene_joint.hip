// Joint per-gene fit of the harmonics and the kinetics over both layers, with the phases and the angular speed known: vc_gene_joint of
// include/velocycle_hip.h, the reference's velocity model (velocity_inference_model.py:360-386, with_delta_nu=False) solved per gene
// for theta = (nu [K], x = log gamma, y = log beta) from one row of spliced and one row of unspliced counts.  nu enters the unspliced
// mean twice: through etaS and through d = nu . d zeta / d phi inside relu(om d + gamma).  Stand-alone like vc_gene_glm and
// vc_gene_kinetics: no engine, no workspace, one launch; the whole (K + 2)-parameter iteration of a gene runs inside its workgroup.
//
// Per gene g and cell c, with b the column [1, sin phi, cos phi, sin 2 phi, ...], db its phi-derivative from the same rows
// (db_0 = 0, db_{2h-1} = h b_{2h}, db_{2h} = -h b_{2h-1}) and W the rows of the angular speed's design:
//   etaS = nu . b + logm_c,   d = nu . db,   om = sum_i nuw_i W_i(c),   z = om d + e^x,   a = [z > 0],   zp = a z + 1e-5
//   etaU = etaS - y + ln zp,  muS = e^etaS,  muU = e^(etaS - y) zp
//   L_S, L_U = Poisson  sum k eta - mu     NB  sum k eta - (k + r) ln(r + mu)  (+ Nc r ln r: formed as k dd - r wl like vc_gene_glm)
//   f    = L_S + L_U - (theta - m)' Lambda (theta - m) / 2        (Lambda: diagonal; nu's from two tables, x's and y's the model's)
// With s = a om / zp, p = a e^x / zp and u = (s db, p, 0) (= a grad z / zp):  gS = (b, 0, 0),  gU = (b + s db, p, -1), and with
// res, w (Fisher), wo (observed) of each layer from gene_lik:
//   G = sum resS gS + resU gU - Lambda (theta - m)
//   O = sum woS gS gS' + woU gU gU' + resU u u' - [sum resU p]_xx + Lambda       (observed: d2 etaU = -u u' + p e_x e_x')
//   F = sum wS gS gS' + wU gU gU' + Lambda                                       (Fisher, always positive definite)
//   N_i = sum (woS^2 + resS^2) gS_i^2 + (woU^2 + resU^2) gU_i^2                  (rounding scale of G_i)
//
// Mapping and arithmetic are vc_gene_kinetics': one workgroup of GENE_NW waves per gene, lanes walk both rows with stride 256
// (gene_count); etaS, d, om, z and etaS - y float64 from the float32 tables and the float64 parameters; e^etaS and e^(etaS - y) from
// gene_exp_f32; gene_lik per layer; ln zp one float32 logarithm; the unspliced element (mu, etaU, gene_lik, p) is kin_pass's
// statements (at max_iter == 0 loglik_u and n_clamped are vc_gene_kinetics' evaluate-only outputs at the same point, bit for bit).  Sums: per-lane
// float64 accumulators folded by gene_fold in wave order through the LDS -- no atomics, identical bits on repetition.  After the fold
// every lane holds the same totals and runs the same packed (K + 2)-dimensional float64 algebra (glm_chol, glm_solve): uniform control.
//
// Registers: the regular pass forms G, O, N, L_S, L_U, sum |terms| and the clamped count (2 (K + 2) + (K + 2)(K + 3) / 2 + 4 sums, 46 at
// H = 2).  F is formed in a pass of its own and only when it is needed: where O fails glm_chol, for the out-of-box retry and in the
// profile pass.  A gene's bits do not depend on that choice.
//
// Iteration over theta, nu in [-50, 50]^K (GLM_BOUND), x and y in [-30, 30] (status codes: velocycle_hip.h):
//   start    start_dev where every entry of the gene is finite and inside the box, else the default: nu_0 = ln(sum k_S / sum e^logm),
//            harmonics at their prior means, x = mu_gamma, y = ln(sum e^etaS zp / sum k_U), clipped to the box (the walk for y is
//            made only where the default is needed; its outcome cannot end a gene that has a usable start)
//   at theta A = O where glm_chol succeeds on it, else F;  dec = G' A^-1 G <= tol                     -> CONVERGED
//            every |G_i| <= 4 eps32 sqrt(N_i)                                                        -> ROUNDING
//            steps taken == max_iter, or dec not finite                                              -> MAX_ITER
//   step     theta + t A^-1 G, t = 1; a full step out of the box is taken with F instead if A was O, else -> UNBOUNDED (the last point
//            inside is kept); accepted unless f' < f - 8 eps32 max(sum |terms|, sum |terms|'), else t /= 2; JNT_MAX_HALVINGS halvings per
//            gene in all (then MAX_ITER): no path spins.
//   max_iter == 0: one pass at the start -> EVALUATED.  A layer without a count, or a coefficient, a prior or r that is not finite
//   -> NO_DATA, NaN.
// With NW > 0 one more pass at the returned point forms the score of nuw and its profile information (the Fisher information of nuw
// with all K + 2 parameters profiled out under their priors).
#include "vc_gene_glm_math.h"                     // vc_gene_math.h (gene_count, gene_exp_f32, gene_lik, gene_fold, the refusals) and glm_tri, glm_chol, glm_solve

// every product-sum is written as the fma it is meant to be; nothing else may be contracted (the same operations in every instantiation)
#pragma clang fp contract(off)

namespace {

constexpr int JNT_MAX_HALVINGS = 30;
constexpr double JNT_BOUND = 30.0;        // x, y; nu is held to GLM_BOUND
constexpr double JNT_FLOOR = 1.0e-5;      // the model's relu(z) + 1e-5

template <int H, int NW>
struct JntDims {
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

// What a cell contributes through the link, float64 except m0 (kin_cell's statements, with etaS and om kept)
struct JntCell {
  double etaS;
  double e0;           // etaS - y
  double d, om, zp;
  bool a;
  float m0;            // e^(etaS - y), one float32 rounding
};

template <int H, int NW>
__device__ __forceinline__ JntCell jnt_cell(const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ W,
                                            long long Nc, long long c, const double (&nu)[2 * H + 1], const double (&dc)[2 * H + 1],
                                            const double (&nuw)[JntDims<H, NW>::NWA], double ex, double y, double (&b)[2 * H + 1],
                                            double (&wr)[JntDims<H, NW>::NWA]) {
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
  JntCell o;
  const double z = __builtin_fma(om, d, ex);
  o.a = z > 0.0;
  o.zp = o.a ? z + JNT_FLOOR : JNT_FLOOR;
  o.d = d;
  o.om = om;
  o.etaS = eta;
  o.e0 = eta - y;
  o.m0 = gene_exp_f32(o.e0);
  return o;
}

// d = sum_{i >= 1} dc[i] b[i]: dc[2h] = h nu[2h - 1] (cos row), dc[2h - 1] = -h nu[2h] (sin row)
template <int H>
__device__ __forceinline__ void jnt_dc(const double (&nu)[2 * H + 1], double (&dc)[2 * H + 1]) {
  dc[0] = 0.0;
#pragma unroll
  for (int h = 1; h <= H; ++h) {
    dc[2 * h] = (double)h * nu[2 * h - 1];
    dc[2 * h - 1] = -(double)h * nu[2 * h];
  }
}

// gU = (b + s db, p, -1) and u = (s db, p) of a cell (u_0 = 0, u_y = 0 are not stored)
template <int H>
__device__ __forceinline__ void jnt_rows(const double (&b)[2 * H + 1], double s, double p, double (&gU)[2 * H + 3], double (&u)[2 * H + 2]) {
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

// One regular pass over both rows of the gene at th: the NACC sums, folded over the workgroup
template <int H, int NW, int NOISE, bool U16>
__device__ __forceinline__ void jnt_pass(const void* __restrict__ rowS, const void* __restrict__ rowU, long long Nc,
                                         const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ W,
                                         const double (&th)[2 * H + 3], const double (&nuw)[JntDims<H, NW>::NWA], float r, double lnr,
                                         double (&acc)[JntDims<H, NW>::NACC], double (*part)[JntDims<H, NW>::NLDS], double* tot, int lane,
                                         int wave) {
  typedef JntDims<H, NW> S;
  constexpr int K = S::K, D = S::D;
#pragma unroll
  for (int i = 0; i < S::NACC; ++i) acc[i] = 0.0;
  double nu[K], dc[K];
#pragma unroll
  for (int i = 0; i < K; ++i) nu[i] = th[i];
  jnt_dc<H>(nu, dc);
  const double x = th[K], y = th[K + 1];
  const double ex = exp(x);
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float kS = gene_count<U16>(rowS, c);
    const float k = gene_count<U16>(rowU, c);
    double b[K], wr[S::NWA];
    const JntCell cl = jnt_cell<H, NW>(B, logm, W, Nc, c, nu, dc, nuw, ex, y, b, wr);
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
    const double p = cl.a ? ex / cl.zp : 0.0;                       // kin_pass's statement
    const double s = cl.a ? cl.om / cl.zp : 0.0;
    double gU[D], u[K + 1];
    jnt_rows<H>(b, s, p, gU, u);
    const double rS = (double)resS, oS = (double)woS, rd = (double)res, od = (double)wo;
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
    acc[S::OFF_LS] += termS;
    acc[S::OFF_LU] += term;
    acc[S::OFF_A] += magS + mag;
    acc[S::OFF_C] += cl.a ? 0.0 : 1.0;
  }
  gene_fold<S::NACC, S::NLDS>(acc, part, tot, lane, wave);
  __syncthreads();                                                   // part / tot are written again by the next fold
}

// The Fisher pass at th: F = sum wS gS gS' + wU gU gU' (packed, without Lambda).  PROFILE: also score_i = sum resU q W_i,
// I_ww = sum wU q^2 W_i W_j (packed) and I_wt[i] = sum wU q W_i gU, q = a d / zp
template <int H, int NW, int NOISE, bool U16, bool PROFILE>
__device__ __forceinline__ void jnt_fisher(const void* __restrict__ rowS, const void* __restrict__ rowU, long long Nc,
                                           const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ W,
                                           const double (&th)[2 * H + 3], const double (&nuw)[JntDims<H, NW>::NWA], float r, double lnr,
                                           double (&fa)[PROFILE ? JntDims<H, NW>::NPRO : JntDims<H, NW>::NHD],
                                           double (*part)[JntDims<H, NW>::NLDS], double* tot, int lane, int wave) {
  typedef JntDims<H, NW> S;
  constexpr int K = S::K, D = S::D, N = PROFILE ? S::NPRO : S::NHD;
#pragma unroll
  for (int i = 0; i < N; ++i) fa[i] = 0.0;
  double nu[K], dc[K];
#pragma unroll
  for (int i = 0; i < K; ++i) nu[i] = th[i];
  jnt_dc<H>(nu, dc);
  const double x = th[K], y = th[K + 1];
  const double ex = exp(x);
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float kS = gene_count<U16>(rowS, c);
    const float k = gene_count<U16>(rowU, c);
    double b[K], wr[S::NWA];
    const JntCell cl = jnt_cell<H, NW>(B, logm, W, Nc, c, nu, dc, nuw, ex, y, b, wr);
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
    jnt_rows<H>(b, s, p, gU, u);
    const double fS = (double)wS, wd = (double)w;
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
      const double rq = (double)res * q, wq = wd * q;
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
__global__ __launch_bounds__(GENE_NT) void vc_gene_joint_kernel(const void* __restrict__ counts_s, const void* __restrict__ counts_u,
                                                               long long Nc, long long gene_stride, const float* __restrict__ B,
                                                               const float* __restrict__ logm, const float* __restrict__ W,
                                                               const double* __restrict__ nuw_in, const float* __restrict__ rg,
                                                               const double* __restrict__ prior_mean, const double* __restrict__ prior_prec,
                                                               const double* __restrict__ prior, const double* __restrict__ start,
                                                               double tol, int max_iter, double* __restrict__ theta_out,
                                                               double* __restrict__ cov_out, double* __restrict__ lls_out,
                                                               double* __restrict__ llu_out, double* __restrict__ dec_out,
                                                               int* __restrict__ iter_out, int* __restrict__ status_out,
                                                               int* __restrict__ clamped_out, double* __restrict__ score_out,
                                                               double* __restrict__ info_out) {
  typedef JntDims<H, NW> S;
  constexpr int K = S::K, D = S::D, NHD = S::NHD, NWA = S::NWA, NWH = S::NWH;
  __shared__ double part[GENE_NW][S::NLDS];
  __shared__ double tot[S::NLDS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long g = blockIdx.x;
  const void* rowS = U16 ? (const void*)((const unsigned short*)counts_s + g * gene_stride) : (const void*)((const float*)counts_s + g * gene_stride);
  const void* rowU = U16 ? (const void*)((const unsigned short*)counts_u + g * gene_stride) : (const void*)((const float*)counts_u + g * gene_stride);
  const double nan = __builtin_nan("");

  // the priors: means pm and precisions pp of theta
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
    nuw[i] = nuw_in[i];
    finite = finite && __builtin_fabs(nuw[i]) < 1.0e300;
  }
  const float r = NOISE == VC_NOISE_NB ? rg[g] : 1.f;
  const double lnr = NOISE == VC_NOISE_NB ? log((double)r) : 0.0;
  finite = finite && r > 0.f && r < 3.0e38f;

  // the start: start_dev where all of the gene's entries are finite and inside the box, else the default nu_0 = ln(sum k_S / sum e^logm),
  // harmonics at their prior means, x = mu_gamma, y = ln(sum e^etaS zp / sum k_U), clipped to the box
  double th[D];
  bool given = start != nullptr;
  if (start) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      th[i] = start[g * D + i];
      given = given && __builtin_fabs(th[i]) <= (i < K ? GLM_BOUND : JNT_BOUND);      // false for a NaN
    }
  }
  if (finite) {
    double s3[3] = {0.0, 0.0, 0.0};
    for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
      s3[0] += (double)gene_count<U16>(rowS, c);
      s3[1] += (double)__builtin_amdgcn_exp2f(VC_LOG2E * logm[c]);
      s3[2] += (double)gene_count<U16>(rowU, c);
    }
    gene_fold<3, S::NLDS>(s3, part, tot, lane, wave);
    __syncthreads();                                                 // part / tot are written again by the next fold
    finite = s3[0] > 0.0 && s3[2] > 0.0;                             // a layer without a count has no fit
    if (finite && !given) {                                          // the same decision in every lane
#pragma unroll
      for (int i = 0; i < D; ++i) th[i] = pm[i];
      th[0] = log(s3[0] / s3[1]);
      finite = __builtin_fabs(th[0]) < 1.0e300;
#pragma unroll
      for (int i = 0; i <= K; ++i) {
        const double bound = i < K ? GLM_BOUND : JNT_BOUND;
        th[i] = th[i] > bound ? bound : (th[i] < -bound ? -bound : th[i]);
      }
      double nu[K], dc[K];
#pragma unroll
      for (int i = 0; i < K; ++i) nu[i] = finite ? th[i] : 0.0;
      jnt_dc<H>(nu, dc);
      const double ex = exp(th[K]);
      double s1[1] = {0.0};
      for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
        double b[K], wr[NWA];
        const JntCell cl = jnt_cell<H, NW>(B, logm, W, Nc, c, nu, dc, nuw, ex, 0.0, b, wr);
        s1[0] = __builtin_fma((double)cl.m0, cl.zp, s1[0]);
      }
      gene_fold<1, S::NLDS>(s1, part, tot, lane, wave);
      __syncthreads();                                               // part / tot are written again by the next fold
      const double y = log(s1[0] / s3[2]);
      finite = finite && __builtin_fabs(y) < 1.0e300;
      th[K + 1] = y > JNT_BOUND ? JNT_BOUND : (y < -JNT_BOUND ? -JNT_BOUND : y);
    }
  }
  if (!finite) {                                                     // the same decision in every lane
    if (threadIdx.x == 0) {
      for (int i = 0; i < D; ++i) theta_out[g * D + i] = nan;
      for (int i = 0; i < NHD; ++i) cov_out[g * NHD + i] = nan;
      lls_out[g] = nan;
      llu_out[g] = nan;
      dec_out[g] = nan;
      iter_out[g] = 0;
      status_out[g] = VC_JNT_NO_DATA;
      clamped_out[g] = 0;
      for (int i = 0; i < NW; ++i) score_out[g * NW + i] = nan;
      for (int i = 0; i < NW * (NW + 1) / 2; ++i) info_out[g * (NW * (NW + 1) / 2) + i] = nan;
    }
    return;
  }

  // F + Lambda at th, factored into chol (the sums of the regular pass are dead by then: only what was taken from them is kept)
#define JNT_FISHER()                                                                                                                   \
  do {                                                                                                                                 \
    double fa[NHD];                                                                                                                    \
    jnt_fisher<H, NW, NOISE, U16, false>(rowS, rowU, Nc, B, logm, W, th, nuw, r, lnr, fa, part, tot, lane, wave);                      \
    _Pragma("unroll") for (int i = 0; i < NHD; ++i) chol[i] = fa[i];                                                                   \
    _Pragma("unroll") for (int i = 0; i < D; ++i) chol[glm_tri(i, i)] += pp[i];                                                        \
    have = glm_chol<D>(chol);                                                                                                          \
  } while (0)
#define JNT_STEP()                                                                                                                     \
  do {                                                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < D; ++i) dx[i] = gr[i];                                                                       \
    glm_solve<D>(chol, dx);                                                                                                            \
    dec = 0.0;                                                                                                                         \
    inside = true;                                                                                                                     \
    _Pragma("unroll") for (int i = 0; i < D; ++i) {                                                                                    \
      dec = __builtin_fma(gr[i], dx[i], dec);                                                                                          \
      inside = inside && __builtin_fabs(th[i] + dx[i]) <= (i < K ? GLM_BOUND : JNT_BOUND);                                             \
    }                                                                                                                                  \
  } while (0)

  enum { AT_POINT = 0, AT_TRIAL = 1, AT_LAST = 2 };                  // what the pass of this turn is for
  double acc[S::NACC], tr[D], dx[D], chol[NHD];
#pragma unroll
  for (int i = 0; i < D; ++i) tr[i] = th[i];
  int status = VC_JNT_MAX_ITER, steps = 0, halvings = JNT_MAX_HALVINGS, mode = AT_POINT;
  double LS = 0.0, LU = 0.0, Acur = 0.0, clamped = 0.0, fcur = 0.0, dec = nan, t = 1.0;
  bool have = false, inside = true;
  for (;;) {
    jnt_pass<H, NW, NOISE, U16>(rowS, rowU, Nc, B, logm, W, tr, nuw, r, lnr, acc, part, tot, lane, wave);
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
    if (!observed) JNT_FISHER();
    JNT_STEP();
    if (mode == AT_LAST) break;
    if (max_iter == 0) { status = VC_JNT_EVALUATED; break; }
    if (!have || !(__builtin_fabs(dec) < 1.0e300)) { status = VC_JNT_MAX_ITER; break; }
    if (dec <= tol) { status = VC_JNT_CONVERGED; break; }
    if (noise) { status = VC_JNT_ROUNDING; break; }
    if (steps >= max_iter) { status = VC_JNT_MAX_ITER; break; }
    // a barely positive definite observed matrix throws the step out of the box: the Fisher step, which the priors bound, before giving up
    if (observed && !inside) {
      JNT_FISHER();
      JNT_STEP();
      if (!have || !(__builtin_fabs(dec) < 1.0e300)) { status = VC_JNT_MAX_ITER; break; }
    }
    if (!inside) { status = VC_JNT_UNBOUNDED; break; }
    t = 1.0;
#pragma unroll
    for (int i = 0; i < D; ++i) tr[i] = th[i] + dx[i];
    mode = AT_TRIAL;
  }
#undef JNT_STEP

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

  // the pass at the returned point for nuw: score_i = sum resU q W_i and the profile information I_ww - I_wt (I_tt + Lambda)^-1 I_tw
  double score[NWA], info[NWH];
  if (NW > 0) {
    double fa[S::NPRO];
    jnt_fisher<H, NW, NOISE, U16, true>(rowS, rowU, Nc, B, logm, W, th, nuw, r, lnr, fa, part, tot, lane, wave);
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
#undef JNT_FISHER

  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < D; ++i) theta_out[g * D + i] = th[i];
#pragma unroll
    for (int i = 0; i < NHD; ++i) cov_out[g * NHD + i] = cov[i];
    lls_out[g] = LS;
    llu_out[g] = LU;
    dec_out[g] = dec;
    iter_out[g] = steps;
    status_out[g] = status;
    clamped_out[g] = (int)clamped;
    if (NW > 0) {
#pragma unroll
      for (int i = 0; i < NWA; ++i) score_out[g * NWA + i] = score[i];
#pragma unroll
      for (int i = 0; i < NWH; ++i) info_out[g * NWH + i] = info[i];
    }
  }
}

constexpr char JNT_FN[] = "vc_gene_joint";

}  // namespace

extern "C" int vc_gene_joint(const void* counts_s_dev, const void* counts_u_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride,
                             const float* basis_dev, int K, const float* logm_dev, const float* w_dev, int NW, const double* nuw_dev,
                             int noise, const float* r_dev, const double* prior_mean_dev, const double* prior_prec_dev,
                             const double* prior_dev, const double* start_dev, double tol, int max_iter, double* theta_dev, double* cov_dev,
                             double* loglik_s_dev, double* loglik_u_dev, double* dec_dev, int32_t* iterations_dev, int32_t* status_dev,
                             int32_t* n_clamped_dev, double* score_w_dev, double* info_w_dev, void* hip_stream) {
  const char* own = nullptr;                                         // what only this entry point says, reported in its place among the shared refusals
  if (K == 7) own = "K must be 3 or 5: H = 3 is not instantiated";
  else if (K != 3 && K != 5) own = "K must be 3 or 5 (2 H + 1, H in {1, 2}; H = 0 has no velocity)";
  else if (NW < 0 || NW > 3) own = "NW must be in 0..3 (rows of the angular speed's design)";
  const int refused = gene_refuse(JNT_FN, noise, count_kind, own, Ng, Nc, true, gene_stride, 0, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (!counts_s_dev || !counts_u_dev || !basis_dev || !logm_dev || !prior_dev) return gene_fail(JNT_FN, VC_ERR_ARG, "null input pointer");
  if (!prior_mean_dev || !prior_prec_dev)
    return gene_fail(JNT_FN, VC_ERR_ARG, "null input pointer: prior_mean_dev and prior_prec_dev are required (without a prior on nu a gene with few cells has no maximum)");
  if (!theta_dev || !cov_dev || !loglik_s_dev || !loglik_u_dev || !dec_dev || !iterations_dev || !status_dev || !n_clamped_dev)
    return gene_fail(JNT_FN, VC_ERR_ARG, "null output pointer");
  if (NW > 0 && (!w_dev || !nuw_dev)) return gene_fail(JNT_FN, VC_ERR_ARG, "NW > 0 needs w_dev and nuw_dev");
  if (NW > 0 && (!score_w_dev || !info_w_dev)) return gene_fail(JNT_FN, VC_ERR_ARG, "NW > 0 needs score_w_dev and info_w_dev (the NW outputs)");
  if (NW == 0 && (score_w_dev || info_w_dev)) return gene_fail(JNT_FN, VC_ERR_ARG, "score_w_dev and info_w_dev need NW > 0 (the NW outputs)");
  if (noise == VC_NOISE_NB && !r_dev) return gene_fail(JNT_FN, VC_ERR_ARG, "the negative binomial needs r_dev (1 / dispersion per gene)");
  if (max_iter == 0 && !start_dev) return gene_fail(JNT_FN, VC_ERR_ARG, "max_iter == 0 (evaluate only) needs start_dev");
  const dim3 grid((unsigned)Ng), block(GENE_NT);
  hipStream_t st = (hipStream_t)hip_stream;
#define JNT_LAUNCH(H, NW_, NOISE, U16)                                                                                                 \
  hipLaunchKernelGGL((vc_gene_joint_kernel<H, NW_, NOISE, U16>), grid, block, 0, st, counts_s_dev, counts_u_dev, (long long)Nc,         \
                     (long long)gene_stride, basis_dev, logm_dev, w_dev, nuw_dev, r_dev, prior_mean_dev, prior_prec_dev, prior_dev,    \
                     start_dev, tol, max_iter, theta_dev, cov_dev, loglik_s_dev, loglik_u_dev, dec_dev, (int*)iterations_dev,          \
                     (int*)status_dev, (int*)n_clamped_dev, score_w_dev, info_w_dev)
#define JNT_LAUNCH_S(H, NW_)                                                                                                          \
  do {                                                                                                                                \
    if (noise == VC_NOISE_NB) { if (u16) JNT_LAUNCH(H, NW_, VC_NOISE_NB, true); else JNT_LAUNCH(H, NW_, VC_NOISE_NB, false); }           \
    else { if (u16) JNT_LAUNCH(H, NW_, VC_NOISE_POISSON, true); else JNT_LAUNCH(H, NW_, VC_NOISE_POISSON, false); }                      \
  } while (0)
#define JNT_LAUNCH_H(H)                                                                                                               \
  switch (NW) {                                                                                                                       \
    case 0: JNT_LAUNCH_S(H, 0); break;                                                                                                \
    case 1: JNT_LAUNCH_S(H, 1); break;                                                                                                \
    case 2: JNT_LAUNCH_S(H, 2); break;                                                                                                \
    default: JNT_LAUNCH_S(H, 3); break;                                                                                               \
  }
  const bool u16 = count_kind == VC_COUNTS_U16;
  if (K == 3) { JNT_LAUNCH_H(1) } else { JNT_LAUNCH_H(2) }
#undef JNT_LAUNCH_H
#undef JNT_LAUNCH_S
#undef JNT_LAUNCH
  return gene_launched(JNT_FN);
}
