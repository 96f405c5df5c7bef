// Per-gene kinetics with case weights: vc_gene_kinetics_weighted of include/velocycle_hip.h.  The model, the mapping of a gene's row onto
// a workgroup, the iteration over (x, y) = (log gamma, log beta) and its status codes are those written at the head of
// vc_gene_kinetics.hip; every cell's contribution is multiplied by a weight w_bc >= 0 read from row b of a float32 table, and one call
// solves R rows of weights for every gene (the cell bootstrap of the velocity fit: Poisson(1) integer weights per row; a held-out fit:
// 0 / 1; the caller's weights).  It takes from vc_gene_kinetics the step vc_gene_glm_weighted takes from vc_gene_glm.
//
// Sums, wt = (double)w_bc: every sum of a pass, of the start's walk and of the profile pass takes its element times wt --
//   res -> wt res,  w -> wt w,  wo -> wt wo  (so the gradient, the Fisher and observed matrices, the score and the information of nuw),
//   L = sum wt term (the negative binomial's r ln r is inside term: weighted with it),  A = sum wt mag,
//   rounding scales  N_x = sum ((wt wo)^2 + (wt res)^2) p^2,  N_y = sum (wt wo)^2 + (wt res)^2,
//   n_clamped = the cells with w > 0 and z <= 0,  default start x = mx, y = ln(sum wt e^etaS zp / sum wt k).
// The priors are not weighted.  Each product with wt is formed first (exact at wt == 1) and the float64 operations that follow are
// those of kin_pass / kin_profile in the same order, so a table of ones gives vc_gene_kinetics' bits.
//
// Per-row inputs: the cycle's coefficients, the angular speed's coefficients and the start may each differ from row to row (a stride
// in numbers from one row's table to the next; 0: shared) -- a jointly resampled cycle, every replicate of an outer iteration at its
// own nuw and its own previous (x, y).
//
// Mapping: one workgroup of GENE_NW waves per (gene, row), grid = (R, genes) with the row in x, the fast index (the workgroups in
// flight share a gene's count row and stream the weight table, as in vc_gene_glm_weighted).  gridDim.y holds at most 65535 genes, so the
// entry point launches slabs of KINW_SLAB genes one after the other on the stream (g_base: the slab's first gene); R <= 65535 keeps
// gridDim.x * blockDim.x below 2^32.  Float64 per-lane sums, shuffle tree, waves in wave order through the LDS: no atomics, identical
// bits on repetition and under any cutting of genes or rows into calls.
//
// KinwGene, kinw_cell, kinw_step and the iteration below are vc_gene_kinetics.hip's, statement for statement, with kin_pass and
// kin_profile replaced by their weighted forms: that file's gfx950 assembly may not move, so nothing of it was factored out.  A change
// to the step or stopping rules has to be made in both files.
#include "vc_gene_math.h"                         // gene_count, gene_exp_f32, gene_lik, gene_fold and the entry point's refusals: shared by the per-gene solvers

// every product-sum is written as the fma it is meant to be; nothing else may be contracted (the same operations in every instantiation)
#pragma clang fp contract(off)

namespace {

constexpr int KINW_MAX_HALVINGS = 30;
constexpr double KINW_BOUND = 30.0;
constexpr double KINW_FLOOR = 1.0e-5;     // the model's relu(z) + 1e-5
// sums of a pass: gradient, Fisher matrix, observed matrix, rounding scales of the gradient, objective, sum |terms|, clamped cells
constexpr int KINW_GX = 0, KINW_GY = 1, KINW_FXX = 2, KINW_FXY = 3, KINW_FYY = 4, KINW_OXX = 5, KINW_OXY = 6, KINW_OYY = 7, KINW_NX = 8,
              KINW_NY = 9, KINW_L = 10, KINW_A = 11, KINW_C = 12, KINW_NACC = 13;
constexpr int KINW_NLDS = 18;             // the longest row folded: the profile pass at NW = 3

// The parameters of a (gene, row) pair that every pass reads
template <int H, int NW>
struct KinwGene {
  static constexpr int K = 2 * H + 1;
  static constexpr int NWA = NW > 0 ? NW : 1;
  double nu[K];        // the cycle's coefficients
  double dc[K];        // d = sum_{i >= 1} dc[i] B[i]: dc[2h] = h nu[2h - 1] (cos row), dc[2h - 1] = -h nu[2h] (sin row)
  double nuw[NWA];
  float r;
  double lnr;
};

// What a cell contributes through the link, float64 except mu
struct KinwCell {
  double e0;           // etaS - y
  double d, zp;
  bool a;
  float m0;            // e^(etaS - y), one float32 rounding
};

template <int H, int NW>
__device__ __forceinline__ KinwCell kinw_cell(const float* __restrict__ B, const float* __restrict__ logm, const float* __restrict__ W,
                                              long long Nc, long long c, const KinwGene<H, NW>& G, double ex, double y,
                                              double (&wr)[KinwGene<H, NW>::NWA]) {
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
  KinwCell o;
  const double z = __builtin_fma(om, d, ex);
  o.a = z > 0.0;
  o.zp = o.a ? z + KINW_FLOOR : KINW_FLOOR;
  o.d = d;
  o.e0 = eta - y;
  o.m0 = gene_exp_f32(o.e0);
  return o;
}

// One pass over the gene's cells at (x, y) under the row's weights: the KINW_NACC sums, folded over the workgroup
template <int H, int NW, int NOISE, bool U16>
__device__ __forceinline__ void kinw_pass(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                          const float* __restrict__ logm, const float* __restrict__ W, const float* __restrict__ wrow,
                                          const KinwGene<H, NW>& G, double x, double y, double (&acc)[KINW_NACC],
                                          double (*part)[KINW_NLDS], double* tot, int lane, int wave) {
#pragma unroll
  for (int i = 0; i < KINW_NACC; ++i) acc[i] = 0.0;
  const double ex = exp(x);
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float k = gene_count<U16>(row, c);
    const double wt = (double)wrow[c];
    double wr[KinwGene<H, NW>::NWA];
    const KinwCell cl = kinw_cell<H, NW>(B, logm, W, Nc, c, G, ex, y, wr);
    const float zpf = (float)cl.zp;
    const float mu = cl.m0 * zpf;
    const double etaU = cl.e0 + (double)(VC_LN2 * __builtin_amdgcn_logf(zpf));
    float res, w, wo;
    double term, mag;
    gene_lik<NOISE>(k, mu, etaU, G.r, G.lnr, res, w, wo, term, mag);
    const double p = cl.a ? ex / cl.zp : 0.0;
    const double rd = wt * (double)res, wd = wt * (double)w, od = wt * (double)wo;
    const double n2 = __builtin_fma(od, od, rd * rd);
    const double wp = wd * p, op = od * p;
    acc[KINW_GX] = __builtin_fma(rd, p, acc[KINW_GX]);
    acc[KINW_GY] -= rd;
    acc[KINW_FXX] = __builtin_fma(wp, p, acc[KINW_FXX]);
    acc[KINW_FXY] -= wp;
    acc[KINW_FYY] += wd;
    acc[KINW_OXX] = __builtin_fma(op, p, acc[KINW_OXX]);
    acc[KINW_OXX] = __builtin_fma(-rd * p, 1.0 - p, acc[KINW_OXX]);
    acc[KINW_OXY] -= op;
    acc[KINW_OYY] += od;
    acc[KINW_NX] = __builtin_fma(n2, p * p, acc[KINW_NX]);
    acc[KINW_NY] += n2;
    acc[KINW_L] += wt * term;
    acc[KINW_A] += wt * mag;
    acc[KINW_C] += cl.a || !(wt > 0.0) ? 0.0 : 1.0;
  }
  gene_fold<KINW_NACC>(acc, part, tot, lane, wave);
  __syncthreads();                                                   // part / tot are written again by the next fold
}

// The point's gradient G, the matrix A its step is taken with (observed where positive definite, else Fisher; priors included), A^-1
// packed (xx, yx, yy), the step A^-1 G, the decrement and the prior's penalty
struct KinwStep {
  double gx, gy, inv[3], dx, dy, dec, pen;
  bool observed;
};

__device__ __forceinline__ KinwStep kinw_step(const double (&acc)[KINW_NACC], double x, double y, double mx, double px, double my,
                                              double py, bool fisher) {
  KinwStep s;
  const double ux = x - mx, uy = y - my;
  s.gx = __builtin_fma(-px, ux, acc[KINW_GX]);
  s.gy = __builtin_fma(-py, uy, acc[KINW_GY]);
  s.pen = __builtin_fma(0.5 * px * ux, ux, 0.5 * py * uy * uy);
  double a = acc[KINW_OXX] + px, b = acc[KINW_OXY], c = acc[KINW_OYY] + py;
  double det = __builtin_fma(a, c, -b * b);
  s.observed = !fisher && a > 0.0 && det > 0.0 && a < 1.0e300 && c < 1.0e300;
  if (!s.observed) {
    a = acc[KINW_FXX] + px;
    b = acc[KINW_FXY];
    c = acc[KINW_FYY] + py;
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

// The pass at the returned point for nuw under the row's weights: score_i = sum (wt res) q W_i and the profile information
// I_ww - I_wt (I_tt + Lambda)^-1 I_tw, I = sum (wt w) g g' (Fisher), t = (x, y)
template <int H, int NW, int NOISE, bool U16>
__device__ __forceinline__ void kinw_profile(const void* __restrict__ row, long long Nc, const float* __restrict__ B,
                                             const float* __restrict__ logm, const float* __restrict__ W,
                                             const float* __restrict__ wrow, const KinwGene<H, NW>& G, double x, double y, double px,
                                             double py, double (&score)[KinwGene<H, NW>::NWA],
                                             double (&info)[KinwGene<H, NW>::NWA * (KinwGene<H, NW>::NWA + 1) / 2],
                                             double (*part)[KINW_NLDS], double* tot, int lane, int wave) {
  constexpr int NWA = KinwGene<H, NW>::NWA, NH = NWA * (NWA + 1) / 2;
  constexpr int OS = 0, OI = NWA, OX = OI + NH, OY = OX + NWA, OF = OY + NWA, N = OF + 3;
  double acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.0;
  const double ex = exp(x);
  for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
    const float k = gene_count<U16>(row, c);
    const double wt = (double)wrow[c];
    double wr[NWA];
    const KinwCell cl = kinw_cell<H, NW>(B, logm, W, Nc, c, G, ex, y, wr);
    const float zpf = (float)cl.zp;
    const float mu = cl.m0 * zpf;
    const double etaU = cl.e0 + (double)(VC_LN2 * __builtin_amdgcn_logf(zpf));
    float res, w, wo;
    double term, mag;
    gene_lik<NOISE>(k, mu, etaU, G.r, G.lnr, res, w, wo, term, mag);
    const double izp = 1.0 / cl.zp;
    const double p = cl.a ? ex * izp : 0.0, q = cl.a ? cl.d * izp : 0.0;
    const double rd = wt * (double)res, wd = wt * (double)w;
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
__global__ __launch_bounds__(GENE_NT) void vc_gene_kinetics_weighted_kernel(
    const void* __restrict__ counts, long long g_base, long long Ng, long long Nc, long long gene_stride, const float* __restrict__ B,
    const float* __restrict__ logm, const double* __restrict__ nu_in, long long nu_row_stride, const float* __restrict__ W,
    const double* __restrict__ nuw_in, long long nuw_row_stride, const float* __restrict__ rg, const double* __restrict__ prior,
    const float* __restrict__ weights, long long weight_stride, const double* __restrict__ start, long long start_row_stride, double tol,
    int max_iter, double* __restrict__ xy_out, double* __restrict__ cov_out, double* __restrict__ loglik_out,
    double* __restrict__ dec_out, int* __restrict__ iter_out, int* __restrict__ status_out, int* __restrict__ clamped_out,
    double* __restrict__ score_out, double* __restrict__ info_out) {
  typedef KinwGene<H, NW> GT;
  constexpr int K = GT::K, NWA = GT::NWA, NWH = NWA * (NWA + 1) / 2;
  __shared__ double part[GENE_NW][KINW_NLDS];
  __shared__ double tot[KINW_NLDS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long g = g_base + blockIdx.y, b = blockIdx.x;          // the row is the fast index
  const long long at = b * Ng + g;                                   // the (row, gene) pair's place in every output
  const void* row = U16 ? (const void*)((const unsigned short*)counts + g * gene_stride) : (const void*)((const float*)counts + g * gene_stride);
  const float* wrow = weights + b * weight_stride;
  const double* nu_row = nu_in + b * nu_row_stride;                  // a stride of 0: the table all rows share
  const double* nuw_row = nuw_in + b * nuw_row_stride;
  const double nan = __builtin_nan("");

  GT G;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    G.nu[i] = nu_row[g * K + i];
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
    G.nuw[i] = nuw_row[i];
    finite = finite && __builtin_fabs(G.nuw[i]) < 1.0e300;
  }
  G.r = NOISE == VC_NOISE_NB ? rg[g] : 1.f;
  G.lnr = NOISE == VC_NOISE_NB ? log((double)G.r) : 0.0;
  finite = finite && G.r > 0.f && G.r < 3.0e38f;
  const double mx = prior[g * 4 + 0], sx = prior[g * 4 + 1], my = prior[g * 4 + 2], sy = prior[g * 4 + 3];
  finite = finite && __builtin_fabs(mx) < 1.0e300 && __builtin_fabs(my) < 1.0e300 && sx > 0.0 && sx < 1.0e300 && sy > 0.0 && sy < 1.0e300;
  const double px = 1.0 / (sx * sx), py = 1.0 / (sy * sy);
  finite = finite && px < 1.0e300 && py < 1.0e300;

  // start: given, or x = mx, y = ln(sum wt e^etaS zp / sum wt k); a row without a weighted count has no fit, whatever the start
  double x = mx, y = 0.0;
  if (finite) {
    double s2[2] = {0.0, 0.0};
    const double ex = exp(mx);
    for (long long c = threadIdx.x; c < Nc; c += GENE_NT) {
      const double wt = (double)wrow[c];
      double wr[NWA];
      const KinwCell cl = kinw_cell<H, NW>(B, logm, W, Nc, c, G, ex, 0.0, wr);
      s2[0] += wt * (double)gene_count<U16>(row, c);
      s2[1] = __builtin_fma(wt * (double)cl.m0, cl.zp, s2[1]);
    }
    gene_fold<2>(s2, part, tot, lane, wave);
    __syncthreads();                                                 // part / tot are written again by the next fold
    y = log(s2[1] / s2[0]);
    finite = s2[0] > 0.0 && s2[0] < 1.0e300 && __builtin_fabs(y) < 1.0e300;      // false for a NaN weight
    if (start) {
      const double* sr = start + b * start_row_stride;
      x = sr[g * 2 + 0];
      y = sr[g * 2 + 1];
      finite = finite && __builtin_fabs(x) < 1.0e300 && __builtin_fabs(y) < 1.0e300;
    }
  }
  if (!finite) {                                                     // the same decision in every lane
    if (threadIdx.x == 0) {
      xy_out[at * 2 + 0] = nan;
      xy_out[at * 2 + 1] = nan;
      if (cov_out) for (int i = 0; i < 3; ++i) cov_out[at * 3 + i] = nan;
      loglik_out[at] = nan;
      dec_out[at] = nan;
      iter_out[at] = 0;
      status_out[at] = VC_KIN_NO_DATA;
      clamped_out[at] = 0;
      for (int i = 0; i < NW; ++i) score_out[at * NW + i] = nan;
      for (int i = 0; i < NW * (NW + 1) / 2; ++i) info_out[at * (NW * (NW + 1) / 2) + i] = nan;
    }
    return;
  }
  x = x > KINW_BOUND ? KINW_BOUND : (x < -KINW_BOUND ? -KINW_BOUND : x);
  y = y > KINW_BOUND ? KINW_BOUND : (y < -KINW_BOUND ? -KINW_BOUND : y);

#define KINW_AT(X, Y) kinw_pass<H, NW, NOISE, U16>(row, Nc, B, logm, W, wrow, G, (X), (Y), acc, part, tot, lane, wave)
  double acc[KINW_NACC];
  KINW_AT(x, y);
  int status = VC_KIN_MAX_ITER, steps = 0, halvings = KINW_MAX_HALVINGS;
  double Lcur, clamped;
  KinwStep st;
  for (;;) {
    // acc holds the sums at (x, y); only L, A and the count of clamped cells outlive the next pass
    Lcur = acc[KINW_L];
    clamped = acc[KINW_C];
    const double Acur = acc[KINW_A];
    st = kinw_step(acc, x, y, mx, px, my, py, false);
    if (max_iter == 0) { status = VC_KIN_EVALUATED; break; }
    if (!(__builtin_fabs(st.dec) < 1.0e300)) { status = VC_KIN_MAX_ITER; break; }
    if (st.dec <= tol) { status = VC_KIN_CONVERGED; break; }
    if (__builtin_fabs(st.gx) <= 4.0 * GENE_EPS32 * __builtin_sqrt(acc[KINW_NX]) &&
        __builtin_fabs(st.gy) <= 4.0 * GENE_EPS32 * __builtin_sqrt(acc[KINW_NY])) { status = VC_KIN_ROUNDING; break; }
    if (steps >= max_iter) { status = VC_KIN_MAX_ITER; break; }
    // a barely positive definite observed matrix throws the step out of the box: the Fisher step, which the priors bound, before giving up
    if (st.observed && !(__builtin_fabs(x + st.dx) <= KINW_BOUND && __builtin_fabs(y + st.dy) <= KINW_BOUND))
      st = kinw_step(acc, x, y, mx, px, my, py, true);
    const double fcur = Lcur - st.pen;
    double t = 1.0;
    bool moved = false, overwritten = false;
    for (;;) {
      const double tx = __builtin_fma(t, st.dx, x), ty = __builtin_fma(t, st.dy, y);
      if (!(__builtin_fabs(tx) <= KINW_BOUND && __builtin_fabs(ty) <= KINW_BOUND)) { status = VC_KIN_UNBOUNDED; break; }
      KINW_AT(tx, ty);
      overwritten = true;
      const double ux = tx - mx, uy = ty - my;
      const double pen2 = __builtin_fma(0.5 * px * ux, ux, 0.5 * py * uy * uy);
      const double A = acc[KINW_A] > Acur ? acc[KINW_A] : Acur;
      if (acc[KINW_L] - pen2 >= fcur - 8.0 * GENE_EPS32 * A) {        // false for a NaN: such a step is halved
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
        KINW_AT(x, y);
        Lcur = acc[KINW_L];
        clamped = acc[KINW_C];
        st = kinw_step(acc, x, y, mx, px, my, py, false);
      }
      break;
    }
    ++steps;
  }
#undef KINW_AT

  double score[NWA], info[NWH];
  if (NW > 0) kinw_profile<H, NW, NOISE, U16>(row, Nc, B, logm, W, wrow, G, x, y, px, py, score, info, part, tot, lane, wave);
  if (threadIdx.x == 0) {
    xy_out[at * 2 + 0] = x;
    xy_out[at * 2 + 1] = y;
    if (cov_out) {
#pragma unroll
      for (int i = 0; i < 3; ++i) cov_out[at * 3 + i] = st.inv[i];
    }
    loglik_out[at] = Lcur;
    dec_out[at] = st.dec;
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

constexpr char KINW_FN[] = "vc_gene_kinetics_weighted";
constexpr int64_t KINW_MAX_ROWS = 65535;          // gridDim.x, and 65535 * GENE_NT < 2^32
constexpr int64_t KINW_SLAB = 65535;              // genes per launch: gridDim.y

}  // namespace

extern "C" int vc_gene_kinetics_weighted(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride,
                                         const float* basis_dev, int K, const float* logm_dev, const double* nu_dev, int64_t nu_row_stride,
                                         const float* w_dev, int NW, const double* nuw_dev, int64_t nuw_row_stride, int noise,
                                         const float* r_dev, const double* prior_dev, const float* weights_dev, int64_t R,
                                         int64_t weight_stride, const double* start_dev, int64_t start_row_stride, double tol, int max_iter,
                                         double* xy_dev, double* cov_dev, double* loglik_dev, double* dec_dev, int32_t* iterations_dev,
                                         int32_t* status_dev, int32_t* n_clamped_dev, double* score_w_dev, double* info_w_dev,
                                         void* hip_stream) {
  const char* own = nullptr;                                         // what only this entry point says, reported in its place among the shared refusals
  if (K == 7) own = "K must be 3 or 5: H = 3 is not instantiated";
  else if (K != 3 && K != 5) own = "K must be 3 or 5 (2 H + 1, H in {1, 2}; H = 0 has no velocity)";
  else if (NW < 0 || NW > 3) own = "NW must be in 0..3 (rows of the angular speed's design)";
  const int refused = gene_refuse(KINW_FN, noise, count_kind, own, Ng, Nc, true, gene_stride, 0, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (!counts_dev || !basis_dev || !logm_dev || !nu_dev || !prior_dev) return gene_fail(KINW_FN, VC_ERR_ARG, "null input pointer");
  if (!xy_dev || !loglik_dev || !dec_dev || !iterations_dev || !status_dev || !n_clamped_dev) return gene_fail(KINW_FN, VC_ERR_ARG, "null output pointer (only cov_dev may be NULL)");
  if (NW > 0 && (!w_dev || !nuw_dev)) return gene_fail(KINW_FN, VC_ERR_ARG, "NW > 0 needs w_dev and nuw_dev");
  if (NW > 0 && (!score_w_dev || !info_w_dev)) return gene_fail(KINW_FN, VC_ERR_ARG, "NW > 0 needs score_w_dev and info_w_dev (the NW outputs)");
  if (noise == VC_NOISE_NB && !r_dev) return gene_fail(KINW_FN, VC_ERR_ARG, "the negative binomial needs r_dev (1 / dispersion per gene)");
  if (max_iter == 0 && !start_dev) return gene_fail(KINW_FN, VC_ERR_ARG, "max_iter == 0 (evaluate only) needs start_dev");
  if (!weights_dev) return gene_fail(KINW_FN, VC_ERR_ARG, "null weights_dev");
  if (R < 1 || R > KINW_MAX_ROWS) return gene_fail(KINW_FN, VC_ERR_ARG, "R must be in 1..65535 rows of weights per call");
  if (weight_stride < Nc) return gene_fail(KINW_FN, VC_ERR_ARG, "weight_stride < Nc");
  if (nu_row_stride != 0 && nu_row_stride < Ng * K) return gene_fail(KINW_FN, VC_ERR_ARG, "nu_row_stride must be 0 (shared) or >= Ng * K");
  if (NW > 0 && nuw_row_stride != 0 && nuw_row_stride < NW) return gene_fail(KINW_FN, VC_ERR_ARG, "nuw_row_stride must be 0 (shared) or >= NW");
  if (start_dev && start_row_stride != 0 && start_row_stride < Ng * 2) return gene_fail(KINW_FN, VC_ERR_ARG, "start_row_stride must be 0 (shared) or >= Ng * 2");
  const dim3 block(GENE_NT);
  hipStream_t st = (hipStream_t)hip_stream;
  const long long nuw_stride = NW > 0 ? (long long)nuw_row_stride : 0, start_stride = start_dev ? (long long)start_row_stride : 0;
#define KINW_LAUNCH(H, NW_, NOISE, U16)                                                                                                \
  hipLaunchKernelGGL((vc_gene_kinetics_weighted_kernel<H, NW_, NOISE, U16>), grid, block, 0, st, counts_dev, (long long)g0,            \
                     (long long)Ng, (long long)Nc, (long long)gene_stride, basis_dev, logm_dev, nu_dev, (long long)nu_row_stride,      \
                     w_dev, nuw_dev, nuw_stride, r_dev, prior_dev, weights_dev, (long long)weight_stride, start_dev, start_stride,     \
                     tol, max_iter, xy_dev, cov_dev, loglik_dev, dec_dev, (int*)iterations_dev, (int*)status_dev,                      \
                     (int*)n_clamped_dev, score_w_dev, info_w_dev)
#define KINW_LAUNCH_S(H, NW_)                                                                                                         \
  do {                                                                                                                                \
    if (noise == VC_NOISE_NB) { if (u16) KINW_LAUNCH(H, NW_, VC_NOISE_NB, true); else KINW_LAUNCH(H, NW_, VC_NOISE_NB, false); }         \
    else { if (u16) KINW_LAUNCH(H, NW_, VC_NOISE_POISSON, true); else KINW_LAUNCH(H, NW_, VC_NOISE_POISSON, false); }                    \
  } while (0)
#define KINW_LAUNCH_H(H)                                                                                                              \
  switch (NW) {                                                                                                                       \
    case 0: KINW_LAUNCH_S(H, 0); break;                                                                                               \
    case 1: KINW_LAUNCH_S(H, 1); break;                                                                                               \
    case 2: KINW_LAUNCH_S(H, 2); break;                                                                                               \
    default: KINW_LAUNCH_S(H, 3); break;                                                                                              \
  }
  const bool u16 = count_kind == VC_COUNTS_U16;
  for (int64_t g0 = 0; g0 < Ng; g0 += KINW_SLAB) {                 // every slab reads and writes at its genes' own places
    const int64_t n = Ng - g0 < KINW_SLAB ? Ng - g0 : KINW_SLAB;
    const dim3 grid((unsigned)R, (unsigned)n);
    if (K == 3) { KINW_LAUNCH_H(1) } else { KINW_LAUNCH_H(2) }
  }
#undef KINW_LAUNCH_H
#undef KINW_LAUNCH_S
#undef KINW_LAUNCH
  return gene_launched(KINW_FN);
}
