// Per-gene kinetics of the velocity model with the cycle, the phases and the angular speed known: vc_gene_kinetics of
// include/velocycle_hip.h, the unspliced half of the reference's model (velocity_inference_model.py:360-386, with_delta_nu=False) solved
// for (log gamma, log beta) of every gene.  Stand-alone like vc_gene_glm and vc_gene_dispersion: no engine, no workspace, one launch; the
// whole two-parameter iteration of a gene runs inside its workgroup.
//
// Per gene g and cell c, with x = log gamma, y = log beta, B the rows [1, sin phi, cos phi, sin 2 phi, ...] and W the rows of the
// angular speed's design:
//   etaS = nu . B[:, c] + logm_c
//   d    = sum_h h (nu_sin_h cos h phi - nu_cos_h sin h phi)                  (d etaS / d phi, from the same basis rows)
//   om   = sum_i nuw_i W_i(c),   z = om d + e^x,   a = [z > 0],   zp = a z + 1e-5
//   etaU = etaS - y + ln zp,     mu = e^(etaS - y) zp
//   L    = Poisson  sum_c k etaU - mu     NB  sum_c k etaU - (k + r) ln(r + mu)  (+ Nc r ln r: formed as k dd - r wl like vc_gene_glm)
//   f    = L - px (x - mx)^2 / 2 - py (y - my)^2 / 2                           (the model's Normal priors; px = 1 / sd^2)
// Derivatives of etaU: p = a e^x / zp (x), -1 (y), q W_i with q = a d / zp (nuw_i); d2 etaU / dx2 = p (1 - p).  Residual and weights:
//   res = k - mu | (k - mu) r / (r + mu)     w (Fisher) = mu | mu r / (r + mu)     wo (observed) = mu | mu r (k + r) / (r + mu)^2
//
// Mapping: one workgroup of GENE_NW waves per gene, lanes walk the row with stride 256 (gene_count, as in vc_gene_glm).  etaS, d, om, z
// and etaS - y are float64 from the float32 tables and the float64 parameters (the set of clamped cells is that of a float64 evaluation
// of the tables); e^(etaS - y) = 2^n 2^f with one float32 exp2 (gene_exp_f32), mu is its float32 product with zp; res, w, wo and the
// NB logarithm are float32 (gene_lik, the element of glm_sweep, with etaU for eta), ln zp is a float32 logarithm.  Sums: per-lane
// float64 accumulators, the shuffle tree, the waves in wave order through the LDS (gene_fold) -- no atomics, identical bits on
// repetition.  After the fold every lane holds the same totals and runs the same 2 x 2 float64 algebra: the control flow is uniform.
//
// Iteration over (x, y) in [-30, 30]^2 (status codes: velocycle_hip.h):
//   start    start_dev, or x = mx, y = ln(sum_c e^etaS zp / sum_c k) (clipped to the box)
//   at (x,y) G = (sum res p, -sum res) - prior terms;  A = the observed matrix  sum wo g g' - [sum res p (1 - p)]_xx + diag(px, py)
//            where it is positive definite, else the Fisher matrix  sum w g g' + diag(px, py)  (always positive definite)
//            dec = G' A^-1 G <= tol                                               -> CONVERGED
//            |G_x| <= 4 eps32 sqrt(sum (wo^2 + res^2) p^2) and |G_y| <= 4 eps32 sqrt(sum wo^2 + res^2)  -> ROUNDING
//            steps taken == max_iter, or dec not finite                           -> MAX_ITER
//   step     (x, y) + t A^-1 G, t = 1; a full step out of the box is taken with the Fisher matrix instead if A was the observed one
//            (a barely positive definite observed matrix), else -> UNBOUNDED; accepted unless f' < f - 8 eps32 max(sum |terms|,
//            sum |terms|'), else t /= 2; KIN_MAX_HALVINGS halvings per gene in all (then MAX_ITER): no path spins.
//   max_iter == 0: one pass at start_dev -> EVALUATED.  A coefficient, a prior or r that is not finite, or no count -> NO_DATA, NaN.
// With NW > 0 one more pass at the returned point forms the score of nuw and its profile information (the Fisher information of nuw
// with (x, y) profiled out under their priors).
#include "vc_gene_math.h"                         // gene_count, gene_exp_f32, gene_lik, gene_fold and the entry point's refusals: shared by the per-gene solvers

// every product-sum is written as the fma it is meant to be; nothing else may be contracted (the same operations in every instantiation)
#pragma clang fp contract(off)

namespace {

constexpr int KIN_MAX_HALVINGS = 30;
constexpr double KIN_BOUND = 30.0;
constexpr double KIN_FLOOR = 1.0e-5;      // the model's relu(z) + 1e-5
// sums of a pass: gradient, Fisher matrix, observed matrix, rounding scales of the gradient, objective, sum |terms|, clamped cells
constexpr int KIN_GX = 0, KIN_GY = 1, KIN_FXX = 2, KIN_FXY = 3, KIN_FYY = 4, KIN_OXX = 5, KIN_OXY = 6, KIN_OYY = 7, KIN_NX = 8,
              KIN_NY = 9, KIN_L = 10, KIN_A = 11, KIN_C = 12, KIN_NACC = 13;
constexpr int KIN_NLDS = 18;              // the longest row folded: the profile pass at NW = 3

// The parameters of a gene that every pass reads
template <int H, int NW>
struct KinGene {
  static constexpr int K = 2 * H + 1;
  static constexpr int NWA = NW > 0 ? NW : 1;
  double nu[K];        // the cycle's coefficients
  double dc[K];        // d = sum_{i >= 1} dc[i] B[i]: dc[2h] = h nu[2h - 1] (cos row), dc[2h - 1] = -h nu[2h] (sin row)
  double nuw[NWA];
  float r;
  double lnr;
};

// What a cell contributes through the link, float64 except mu
struct KinCell {
  double e0;           // etaS - y
  double d, zp;
  bool a;
  float m0;            // e^(etaS - y), one float32 rounding
};

template <int H, int NW>
__device__ __forceinline__ KinCell kin_cell(const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ W,
                                            long long Nc, long long c, const KinGene<H, NW>& G, double ex, double y,
                                            double (&wr)[KinGene<H, NW>::NWA]) {
  constexpr int K = 2 * H + 1;
  double b[K];
  b[0] = 1.0;
#pragma unroll
  for (int i = 1; i < K; ++i) b[i] = (double)B[(long long)i * Nc + c];
  double eta = (double)logm[c] + G.nu[0];
  double d = 0.0;
#pragma unroll
  for (int i = 1; i < K; ++i) {
    eta = __builtin_fma(G.nu[i], b[i], eta);
    d = __builtin_fma(G.dc[i], b[i], d);
  }
  double om = 0.0;
  wr[0] = 0.0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    wr[i] = (double)W[(long long)i * Nc + c];
    om = __builtin_fma(G.nuw[i], wr[i], om);
  }
  KinCell o;
  const double z = __builtin_fma(om, d, ex);
  o.a = z > 0.0;
  o.zp = o.a ? z + KIN_FLOOR : KIN_FLOOR;
  o.d = d;
  o.e0 = eta - y;
  o.m0 = gene_exp_f32(o.e0);
  return o;
}

// One pass over the gene's cells at (x, y): the KIN_NACC sums, folded over the workgroup
template <int H, int NW, int NOISE, bool U16>
__device__ __forceinline__ void kin_pass(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                         const float* __restrict__ logm, const float* __restrict__ W, const KinGene<H, NW>& G, double x,
                                         double y, double (&acc)[KIN_NACC], double (*part)[KIN_NLDS], double* tot, int lane, int wave) {
#pragma unroll
  for (int i = 0; i < KIN_NACC; ++i) acc[i] = 0.0;
  const double ex = exp(x);
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float k = gene_count<U16>(row, c);
    double wr[KinGene<H, NW>::NWA];
    const KinCell cl = kin_cell<H, NW>(B, logm, W, Nc, c, G, ex, y, wr);
    const float zpf = (float)cl.zp;
    const float mu = cl.m0 * zpf;
    const double etaU = cl.e0 + (double)(VC_LN2 * __builtin_amdgcn_logf(zpf));
    float res, w, wo;
    double term, mag;
    gene_lik<NOISE>(k, mu, etaU, G.r, G.lnr, res, w, wo, term, mag);
    const double p = cl.a ? ex / cl.zp : 0.0;
    const double rd = (double)res, wd = (double)w, od = (double)wo;
    const double n2 = __builtin_fma(od, od, rd * rd);
    const double wp = wd * p, op = od * p;
    acc[KIN_GX] = __builtin_fma(rd, p, acc[KIN_GX]);
    acc[KIN_GY] -= rd;
    acc[KIN_FXX] = __builtin_fma(wp, p, acc[KIN_FXX]);
    acc[KIN_FXY] -= wp;
    acc[KIN_FYY] += wd;
    acc[KIN_OXX] = __builtin_fma(op, p, acc[KIN_OXX]);
    acc[KIN_OXX] = __builtin_fma(-rd * p, 1.0 - p, acc[KIN_OXX]);
    acc[KIN_OXY] -= op;
    acc[KIN_OYY] += od;
    acc[KIN_NX] = __builtin_fma(n2, p * p, acc[KIN_NX]);
    acc[KIN_NY] += n2;
    acc[KIN_L] += term;
    acc[KIN_A] += mag;
    acc[KIN_C] += cl.a ? 0.0 : 1.0;
  }
  gene_fold<KIN_NACC>(acc, part, tot, lane, wave);
  __syncthreads();                                                   // part / tot are written again by the next fold
}

// The point's gradient G, the matrix A its step is taken with (observed where positive definite, else Fisher; priors included), A^-1
// packed (xx, yx, yy), the step A^-1 G, the decrement and the prior's penalty
struct KinStep {
  double gx, gy, inv[3], dx, dy, dec, pen;
  bool observed;
};

__device__ __forceinline__ KinStep kin_step(const double (&acc)[KIN_NACC], double x, double y, double mx, double px, double my, double py,
                                            bool fisher) {
  KinStep s;
  const double ux = x - mx, uy = y - my;
  s.gx = __builtin_fma(-px, ux, acc[KIN_GX]);
  s.gy = __builtin_fma(-py, uy, acc[KIN_GY]);
  s.pen = __builtin_fma(0.5 * px * ux, ux, 0.5 * py * uy * uy);
  double a = acc[KIN_OXX] + px, b = acc[KIN_OXY], c = acc[KIN_OYY] + py;
  double det = __builtin_fma(a, c, -b * b);
  s.observed = !fisher && a > 0.0 && det > 0.0 && a < 1.0e300 && c < 1.0e300;
  if (!s.observed) {
    a = acc[KIN_FXX] + px;
    b = acc[KIN_FXY];
    c = acc[KIN_FYY] + py;
    det = __builtin_fma(a, c, -b * b);
  }
  const double id = 1.0 / det;
  s.inv[0] = c * id;
  s.inv[1] = -b * id;
  s.inv[2] = a * id;
  s.dx = __builtin_fma(s.inv[0], s.gx, s.inv[1] * s.gy);
  s.dy = __builtin_fma(s.inv[1], s.gx, s.inv[2] * s.gy);
  s.dec = __builtin_fma(s.gx, s.dx, s.gy * s.dy);
  return s;
}

// The pass at the returned point for nuw: score_i = sum res q W_i and the profile information I_ww - I_wt (I_tt + Lambda)^-1 I_tw,
// I = sum w g g' (Fisher), t = (x, y)
template <int H, int NW, int NOISE, bool U16>
__device__ __forceinline__ void kin_profile(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                            const float* __restrict__ logm, const float* __restrict__ W, const KinGene<H, NW>& G, double x,
                                            double y, double px, double py, double (&score)[KinGene<H, NW>::NWA],
                                            double (&info)[KinGene<H, NW>::NWA * (KinGene<H, NW>::NWA + 1) / 2],
                                            double (*part)[KIN_NLDS], double* tot, int lane, int wave) {
  constexpr int NWA = KinGene<H, NW>::NWA, NH = NWA * (NWA + 1) / 2;
  constexpr int OS = 0, OI = NWA, OX = OI + NH, OY = OX + NWA, OF = OY + NWA, N = OF + 3;
  double acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.0;
  const double ex = exp(x);
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float k = gene_count<U16>(row, c);
    double wr[NWA];
    const KinCell cl = kin_cell<H, NW>(B, logm, W, Nc, c, G, ex, y, wr);
    const float zpf = (float)cl.zp;
    const float mu = cl.m0 * zpf;
    const double etaU = cl.e0 + (double)(VC_LN2 * __builtin_amdgcn_logf(zpf));
    float res, w, wo;
    double term, mag;
    gene_lik<NOISE>(k, mu, etaU, G.r, G.lnr, res, w, wo, term, mag);
    const double izp = 1.0 / cl.zp;
    const double p = cl.a ? ex * izp : 0.0, q = cl.a ? cl.d * izp : 0.0;
    const double rd = (double)res, wd = (double)w;
    const double rq = rd * q, wq = wd * q, wp = wd * p;
#pragma unroll
    for (int i = 0; i < NWA; ++i) {
      acc[OS + i] = __builtin_fma(rq, wr[i], acc[OS + i]);
      const double wqi = wq * wr[i];
#pragma unroll
      for (int j = 0; j <= i; ++j) acc[OI + i * (i + 1) / 2 + j] = __builtin_fma(wqi * q, wr[j], acc[OI + i * (i + 1) / 2 + j]);
      acc[OX + i] = __builtin_fma(wqi, p, acc[OX + i]);
      acc[OY + i] -= wqi;
    }
    acc[OF + 0] = __builtin_fma(wp, p, acc[OF + 0]);
    acc[OF + 1] -= wp;
    acc[OF + 2] += wd;
  }
  gene_fold<N>(acc, part, tot, lane, wave);
  __syncthreads();                                                   // part / tot are written again by the next fold
  const double a = acc[OF + 0] + px, b = acc[OF + 1], cc = acc[OF + 2] + py;
  const double id = 1.0 / __builtin_fma(a, cc, -b * b);
  const double ixx = cc * id, ixy = -b * id, iyy = a * id;
#pragma unroll
  for (int i = 0; i < NWA; ++i) {
    score[i] = acc[OS + i];
    const double tx = __builtin_fma(ixx, acc[OX + i], ixy * acc[OY + i]);      // (I_tt + Lambda)^-1 I_tw, column i
    const double ty = __builtin_fma(ixy, acc[OX + i], iyy * acc[OY + i]);
#pragma unroll
    for (int j = 0; j <= i; ++j)
      info[i * (i + 1) / 2 + j] = acc[OI + i * (i + 1) / 2 + j] - __builtin_fma(acc[OX + j], tx, acc[OY + j] * ty);
  }
}

template <int H, int NW, int NOISE, bool U16>
__global__ __launch_bounds__(GENE_NT) void vc_gene_kinetics_kernel(const void* __restrict__ counts, long long Nc, long long gene_stride,
                                                                  const float* __restrict__ B, const float* __restrict__ logm,
                                                                  const double* __restrict__ nu_in, const float* __restrict__ W,
                                                                  const double* __restrict__ nuw_in, const float* __restrict__ rg,
                                                                  const double* __restrict__ prior, const double* __restrict__ start,
                                                                  double tol, int max_iter, double* __restrict__ xy_out,
                                                                  double* __restrict__ cov_out, double* __restrict__ loglik_out,
                                                                  double* __restrict__ dec_out, int* __restrict__ iter_out,
                                                                  int* __restrict__ status_out, int* __restrict__ clamped_out,
                                                                  double* __restrict__ score_out, double* __restrict__ info_out) {
  typedef KinGene<H, NW> GT;
  constexpr int K = GT::K, NWA = GT::NWA, NWH = NWA * (NWA + 1) / 2;
  __shared__ double part[GENE_NW][KIN_NLDS];
  __shared__ double tot[KIN_NLDS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long g = blockIdx.x;
  const void* row = U16 ? (const void*)((const unsigned short*)counts + g * gene_stride) : (const void*)((const float*)counts + g * gene_stride);
  const double nan = __builtin_nan("");

  GT G;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    G.nu[i] = nu_in[g * K + i];
    finite = finite && __builtin_fabs(G.nu[i]) < 1.0e300;
  }
  G.dc[0] = 0.0;
#pragma unroll
  for (int h = 1; h <= H; ++h) {
    G.dc[2 * h] = (double)h * G.nu[2 * h - 1];
    G.dc[2 * h - 1] = -(double)h * G.nu[2 * h];
  }
  G.nuw[0] = 0.0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    G.nuw[i] = nuw_in[i];
    finite = finite && __builtin_fabs(G.nuw[i]) < 1.0e300;
  }
  G.r = NOISE == VC_NOISE_NB ? rg[g] : 1.f;
  G.lnr = NOISE == VC_NOISE_NB ? log((double)G.r) : 0.0;
  finite = finite && G.r > 0.f && G.r < 3.0e38f;
  const double mx = prior[g * 4 + 0], sx = prior[g * 4 + 1], my = prior[g * 4 + 2], sy = prior[g * 4 + 3];
  finite = finite && __builtin_fabs(mx) < 1.0e300 && __builtin_fabs(my) < 1.0e300 && sx > 0.0 && sx < 1.0e300 && sy > 0.0 && sy < 1.0e300;
  const double px = 1.0 / (sx * sx), py = 1.0 / (sy * sy);
  finite = finite && px < 1.0e300 && py < 1.0e300;

  // start: given, or x = mx, y = ln(sum e^etaS zp / sum k); a gene without a count has no fit
  double x = mx, y = 0.0;
  if (finite) {
    double s2[2] = {0.0, 0.0};
    const double ex = exp(mx);
    for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
      double wr[NWA];
      const KinCell cl = kin_cell<H, NW>(B, logm, W, Nc, c, G, ex, 0.0, wr);
      s2[0] += (double)gene_count<U16>(row, c);
      s2[1] = __builtin_fma((double)cl.m0, cl.zp, s2[1]);
    }
    gene_fold<2>(s2, part, tot, lane, wave);
    __syncthreads();                                                 // part / tot are written again by the next fold
    y = log(s2[1] / s2[0]);
    finite = s2[0] > 0.0 && __builtin_fabs(y) < 1.0e300;
    if (start) {
      x = start[g * 2 + 0];
      y = start[g * 2 + 1];
      finite = finite && __builtin_fabs(x) < 1.0e300 && __builtin_fabs(y) < 1.0e300;
    }
  }
  if (!finite) {                                                     // the same decision in every lane
    if (threadIdx.x == 0) {
      xy_out[g * 2 + 0] = nan;
      xy_out[g * 2 + 1] = nan;
      for (int i = 0; i < 3; ++i) cov_out[g * 3 + i] = nan;
      loglik_out[g] = nan;
      dec_out[g] = nan;
      iter_out[g] = 0;
      status_out[g] = VC_KIN_NO_DATA;
      clamped_out[g] = 0;
      for (int i = 0; i < NW; ++i) score_out[g * NW + i] = nan;
      for (int i = 0; i < NW * (NW + 1) / 2; ++i) info_out[g * (NW * (NW + 1) / 2) + i] = nan;
    }
    return;
  }
  x = x > KIN_BOUND ? KIN_BOUND : (x < -KIN_BOUND ? -KIN_BOUND : x);
  y = y > KIN_BOUND ? KIN_BOUND : (y < -KIN_BOUND ? -KIN_BOUND : y);

#define KIN_AT(X, Y) kin_pass<H, NW, NOISE, U16>(row, Nc, B, logm, W, G, (X), (Y), acc, part, tot, lane, wave)
  double acc[KIN_NACC];
  KIN_AT(x, y);
  int status = VC_KIN_MAX_ITER, steps = 0, halvings = KIN_MAX_HALVINGS;
  double Lcur, clamped;
  KinStep st;
  for (;;) {
    // acc holds the sums at (x, y); only L, A and the count of clamped cells outlive the next pass
    Lcur = acc[KIN_L];
    clamped = acc[KIN_C];
    const double Acur = acc[KIN_A];
    st = kin_step(acc, x, y, mx, px, my, py, false);
    if (max_iter == 0) { status = VC_KIN_EVALUATED; break; }
    if (!(__builtin_fabs(st.dec) < 1.0e300)) { status = VC_KIN_MAX_ITER; break; }
    if (st.dec <= tol) { status = VC_KIN_CONVERGED; break; }
    if (__builtin_fabs(st.gx) <= 4.0 * GENE_EPS32 * __builtin_sqrt(acc[KIN_NX]) &&
        __builtin_fabs(st.gy) <= 4.0 * GENE_EPS32 * __builtin_sqrt(acc[KIN_NY])) { status = VC_KIN_ROUNDING; break; }
    if (steps >= max_iter) { status = VC_KIN_MAX_ITER; break; }
    // a barely positive definite observed matrix throws the step out of the box: the Fisher step, which the priors bound, before giving up
    if (st.observed && !(__builtin_fabs(x + st.dx) <= KIN_BOUND && __builtin_fabs(y + st.dy) <= KIN_BOUND))
      st = kin_step(acc, x, y, mx, px, my, py, true);
    const double fcur = Lcur - st.pen;
    double t = 1.0;
    bool moved = false, overwritten = false;
    for (;;) {
      const double tx = __builtin_fma(t, st.dx, x), ty = __builtin_fma(t, st.dy, y);
      if (!(__builtin_fabs(tx) <= KIN_BOUND && __builtin_fabs(ty) <= KIN_BOUND)) { status = VC_KIN_UNBOUNDED; break; }
      KIN_AT(tx, ty);
      overwritten = true;
      const double ux = tx - mx, uy = ty - my;
      const double pen2 = __builtin_fma(0.5 * px * ux, ux, 0.5 * py * uy * uy);
      const double A = acc[KIN_A] > Acur ? acc[KIN_A] : Acur;
      if (acc[KIN_L] - pen2 >= fcur - 8.0 * GENE_EPS32 * A) {         // false for a NaN: such a step is halved
        x = tx;
        y = ty;
        moved = true;
        break;
      }
      if (halvings == 0) { status = VC_KIN_MAX_ITER; break; }
      --halvings;
      t *= 0.5;
    }
    if (!moved) {
      if (overwritten) {                                             // a refused trial's sums are in acc: form those of (x, y) again
        KIN_AT(x, y);
        Lcur = acc[KIN_L];
        clamped = acc[KIN_C];
        st = kin_step(acc, x, y, mx, px, my, py, false);
      }
      break;
    }
    ++steps;
  }
#undef KIN_AT

  double score[NWA], info[NWH];
  if (NW > 0) kin_profile<H, NW, NOISE, U16>(row, Nc, B, logm, W, G, x, y, px, py, score, info, part, tot, lane, wave);
  if (threadIdx.x == 0) {
    xy_out[g * 2 + 0] = x;
    xy_out[g * 2 + 1] = y;
#pragma unroll
    for (int i = 0; i < 3; ++i) cov_out[g * 3 + i] = st.inv[i];
    loglik_out[g] = Lcur;
    dec_out[g] = st.dec;
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

constexpr char KIN_FN[] = "vc_gene_kinetics";

}  // namespace

extern "C" int vc_gene_kinetics(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev,
                                int K, const float* logm_dev, const double* nu_dev, const float* w_dev, int NW, const double* nuw_dev,
                                int noise, const float* r_dev, const double* prior_dev, const double* start_dev, double tol, int max_iter,
                                double* xy_dev, double* cov_dev, double* loglik_dev, double* dec_dev, int32_t* iterations_dev,
                                int32_t* status_dev, int32_t* n_clamped_dev, double* score_w_dev, double* info_w_dev, void* hip_stream) {
  const char* own = nullptr;                                         // what only this entry point says, reported in its place among the shared refusals
  if (K == 7) own = "K must be 3 or 5: H = 3 is not instantiated";
  else if (K != 3 && K != 5) own = "K must be 3 or 5 (2 H + 1, H in {1, 2}; H = 0 has no velocity)";
  else if (NW < 0 || NW > 3) own = "NW must be in 0..3 (rows of the angular speed's design)";
  const int refused = gene_refuse(KIN_FN, noise, count_kind, own, Ng, Nc, true, gene_stride, 0, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (!counts_dev || !basis_dev || !logm_dev || !nu_dev || !prior_dev) return gene_fail(KIN_FN, VC_ERR_ARG, "null input pointer");
  if (!xy_dev || !cov_dev || !loglik_dev || !dec_dev || !iterations_dev || !status_dev || !n_clamped_dev) return gene_fail(KIN_FN, VC_ERR_ARG, "null output pointer");
  if (NW > 0 && (!w_dev || !nuw_dev)) return gene_fail(KIN_FN, VC_ERR_ARG, "NW > 0 needs w_dev and nuw_dev");
  if (NW > 0 && (!score_w_dev || !info_w_dev)) return gene_fail(KIN_FN, VC_ERR_ARG, "NW > 0 needs score_w_dev and info_w_dev (the NW outputs)");
  if (noise == VC_NOISE_NB && !r_dev) return gene_fail(KIN_FN, VC_ERR_ARG, "the negative binomial needs r_dev (1 / dispersion per gene)");
  if (max_iter == 0 && !start_dev) return gene_fail(KIN_FN, VC_ERR_ARG, "max_iter == 0 (evaluate only) needs start_dev");
  const dim3 grid((unsigned)Ng), block(GENE_NT);
  hipStream_t st = (hipStream_t)hip_stream;
#define KIN_LAUNCH(H, NW_, NOISE, U16)                                                                                                 \
  hipLaunchKernelGGL((vc_gene_kinetics_kernel<H, NW_, NOISE, U16>), grid, block, 0, st, counts_dev, (long long)Nc,                     \
                     (long long)gene_stride, basis_dev, logm_dev, nu_dev, w_dev, nuw_dev, r_dev, prior_dev, start_dev, tol, max_iter,  \
                     xy_dev, cov_dev, loglik_dev, dec_dev, (int*)iterations_dev, (int*)status_dev, (int*)n_clamped_dev, score_w_dev,   \
                     info_w_dev)
#define KIN_LAUNCH_S(H, NW_)                                                                                                          \
  do {                                                                                                                                \
    if (noise == VC_NOISE_NB) { if (u16) KIN_LAUNCH(H, NW_, VC_NOISE_NB, true); else KIN_LAUNCH(H, NW_, VC_NOISE_NB, false); }           \
    else { if (u16) KIN_LAUNCH(H, NW_, VC_NOISE_POISSON, true); else KIN_LAUNCH(H, NW_, VC_NOISE_POISSON, false); }                      \
  } while (0)
#define KIN_LAUNCH_H(H)                                                                                                               \
  switch (NW) {                                                                                                                       \
    case 0: KIN_LAUNCH_S(H, 0); break;                                                                                                \
    case 1: KIN_LAUNCH_S(H, 1); break;                                                                                                \
    case 2: KIN_LAUNCH_S(H, 2); break;                                                                                                \
    default: KIN_LAUNCH_S(H, 3); break;                                                                                               \
  }
  const bool u16 = count_kind == VC_COUNTS_U16;
  if (K == 3) { KIN_LAUNCH_H(1) } else { KIN_LAUNCH_H(2) }
#undef KIN_LAUNCH_H
#undef KIN_LAUNCH_S
#undef KIN_LAUNCH
  return gene_launched(KIN_FN);
}
