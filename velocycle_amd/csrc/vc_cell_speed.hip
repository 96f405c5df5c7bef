// Per-cell angular speed of the velocity model with the cycle, the phases and the kinetics known: vc_cell_speed of
// include/velocycle_hip.h, the model of vc_gene_kinetics with the roles swapped -- (log gamma, log beta) of every gene are given and
// every CELL's angular speed om_c is the one unknown of that cell's unspliced counts.  Stand-alone like vc_phase_mle and the per-gene
// solvers: no engine, no workspace, one launch; the whole one-parameter iteration of a cell runs inside the kernel.
//
// Per cell c and gene g, with x = log gamma_g, y = log beta_g and B the rows [1, sin phi, cos phi, sin 2 phi, ...]:
//   etaS = nu_g . B[:, c] + logm_c
//   d    = sum_h h (nu_sin_h cos h phi - nu_cos_h sin h phi)                  (d etaS / d phi, from the same basis rows)
//   z = om_c d + e^x,   a = [z > 0],   zp = a z + 1e-5,   etaU = etaS - y + ln zp,   mu = e^(etaS - y) zp,   q = a d / zp
//   res = k - mu | (k - mu) r / (r + mu)     w (Fisher) = mu | mu r / (r + mu)     wo (observed) = mu | mu r (k + r) / (r + mu)^2
//   L = sum_g term (gene_lik: k etaU - mu | k etaU - (k + r) ln(r + mu) + r ln r)      score = sum_g res q      fisher = sum_g w q^2
//   observed = sum_g (wo + res) q^2  (d2 etaU / d om2 = -q^2)      N = sum_g (wo^2 + res^2) q^2      A = sum_g |terms|
//   f = L - (om - m_c)^2 / 2 s_c^2                                            (the optional Normal prior of the cell)
//
// Mapping: vc_phase_mle's.  Lane = cell, a wave owns 64 consecutive cells, the CSP_NW waves of a workgroup split the genes into
// contiguous shares that depend on Ng alone.  Every count load is 64 consecutive cells of one gene row.  nu, y and r of a gene are
// wave-uniform and read through the constant address space; e^x and ln r are formed for 64 genes at a time, one gene per lane, and
// handed round by v_readlane, so the float64 exponential costs one evaluation per 64 elements.  Per lane eight float64 accumulators;
// the waves' partials are added in wave order through the LDS, after which EVERY wave holds the totals of its 64 cells and runs the
// same per-lane state machine: the workgroup's control flow is uniform, a lane that has stopped keeps its values while the others
// go on, and the workgroup ends with its last cell.  etaS, d, z and etaS - y are float64; e^(etaS - y) is gene_exp_f32's one float32
// exp2; res, w, wo, the NB logarithm and ln zp are float32 (gene_lik); every sum is float64 in a fixed order.  No atomics.
//
// Iteration over om in [-30, 30] (status codes: velocycle_hip.h), vc_gene_kinetics' rules in one dimension:
//   at om    G = score - (om - m) / s^2;  A = observed + 1 / s^2 where that is positive, else fisher + 1 / s^2;  dec = G^2 / A
//            max_iter == 0 -> EVALUATED;  dec not finite -> MAX_ITER;  dec <= tol -> CONVERGED;  |G| <= 4 eps32 sqrt(N) -> ROUNDING;
//            steps taken == max_iter -> MAX_ITER
//   step     om + t G / A, t = 1; outside the box -> UNBOUNDED (om is kept); accepted unless f' < f - 8 eps32 max(A, A'), else
//            t /= 2; CSP_MAX_HALVINGS halvings per cell in all (then MAX_ITER).  Every pass of the workgroup takes a step or a halving
//            from each cell still running: at most max_iter + CSP_MAX_HALVINGS + 1 passes.
//   A cell without a count, a start that is not finite, a prior that is not finite (sd: or not > 0) -> NO_DATA, NaN.
#include "vc_gene_math.h"                         // gene_count, gene_exp_f32, gene_lik and the entry point's refusals: shared with the per-gene solvers

// every product-sum is written as the fma it is meant to be; nothing else may be contracted (the same operations in every instantiation)
#pragma clang fp contract(off)

namespace {

constexpr int CSP_NW = 4;                 // waves per workgroup (= gene shares)
constexpr int CSP_MAX_HALVINGS = 30;
constexpr double CSP_BOUND = 30.0;
constexpr double CSP_FLOOR = 1.0e-5;      // the model's relu(z) + 1e-5
// sums of a pass: objective, score, Fisher, observed, rounding scale, sum |terms| (the six of sums_dev), clamped genes, sum of counts
constexpr int CSP_L = 0, CSP_S = 1, CSP_F = 2, CSP_O = 3, CSP_N = 4, CSP_A = 5, CSP_C = 6, CSP_K = 7, CSP_NACC = 8;
constexpr int CSP_NOUT = 6;

typedef const __attribute__((address_space(4))) double* csp_cdptr;
typedef const __attribute__((address_space(4))) float* csp_cfptr;

// lane j's v in every lane (j wave-uniform): two v_readlane, the result is wave-uniform
__device__ __forceinline__ double csp_bcast(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

// One pass of this wave's gene share [g_lo, g_hi) at the lanes' om: acc[] of the share, then of all genes (every wave holds them)
template <int H, int NOISE, bool U16>
__device__ __forceinline__ void csp_pass(const void* __restrict__ counts, long long gene_stride, long long c, long long g_lo, long long g_hi,
                                         const double (&b)[2 * H + 1], double logm, csp_cdptr nu, csp_cdptr xy, csp_cfptr rg, double om,
                                         double (&acc)[CSP_NACC], double (*part)[CSP_NACC][64], int lane, int wave) {
  constexpr int K = 2 * H + 1;
#pragma unroll
  for (int i = 0; i < CSP_NACC; ++i) acc[i] = 0.0;
  for (long long g0 = g_lo; g0 < g_hi; g0 += 64) {
    const int n = g_hi - g0 < 64 ? (int)(g_hi - g0) : 64;
    const long long gl = g0 + lane < g_hi ? g0 + lane : g_hi - 1;     // lane j prepares gene g0 + j
    const double ex_l = exp(xy[gl * 2]);
    const double lnr_l = NOISE == VC_NOISE_NB ? log((double)rg[gl]) : 0.0;
    for (int j = 0; j < n; ++j) {
      const long long g = g0 + j;
      const float k = gene_count<U16>(counts, g * gene_stride + c);
      const double ex = csp_bcast(ex_l, j);
      const double lnr = NOISE == VC_NOISE_NB ? csp_bcast(lnr_l, j) : 0.0;
      const double y = xy[g * 2 + 1];
      const float r = NOISE == VC_NOISE_NB ? rg[g] : 1.f;
      double v[K];
#pragma unroll
      for (int i = 0; i < K; ++i) v[i] = nu[g * K + i];
      double eta = logm + v[0];
      double d = 0.0;
#pragma unroll
      for (int h = 1; h <= H; ++h) {                                  // d = sum dc[i] b[i]: dc[2h] = h nu[2h - 1] (cos row), dc[2h - 1] = -h nu[2h] (sin row)
        eta = __builtin_fma(v[2 * h - 1], b[2 * h - 1], eta);
        d = __builtin_fma(-(double)h * v[2 * h], b[2 * h - 1], d);
        eta = __builtin_fma(v[2 * h], b[2 * h], eta);
        d = __builtin_fma((double)h * v[2 * h - 1], b[2 * h], d);
      }
      const double z = __builtin_fma(om, d, ex);
      const bool a = z > 0.0;
      const double zp = a ? z + CSP_FLOOR : CSP_FLOOR;
      const double e0 = eta - y;
      const float zpf = (float)zp;
      const float mu = gene_exp_f32(e0) * zpf;
      const double etaU = e0 + (double)(VC_LN2 * __builtin_amdgcn_logf(zpf));
      float res, w, wo;
      double term, mag;
      gene_lik<NOISE>(k, mu, etaU, r, lnr, res, w, wo, term, mag);
      const double q = a ? d / zp : 0.0;
      const double q2 = q * q;
      const double rd = (double)res, wd = (double)w, od = (double)wo;
      acc[CSP_L] += term;
      acc[CSP_S] = __builtin_fma(rd, q, acc[CSP_S]);
      acc[CSP_F] = __builtin_fma(wd, q2, acc[CSP_F]);
      acc[CSP_O] = __builtin_fma(od + rd, q2, acc[CSP_O]);
      acc[CSP_N] = __builtin_fma(__builtin_fma(od, od, rd * rd), q2, acc[CSP_N]);
      acc[CSP_A] += mag;
      acc[CSP_C] += a ? 0.0 : 1.0;
      acc[CSP_K] += (double)k;
    }
  }
  // the waves' partials, added in wave order; every wave ends with the totals of its 64 cells
  __syncthreads();                                                    // the previous pass has been read
#pragma unroll
  for (int i = 0; i < CSP_NACC; ++i) part[wave][i][lane] = acc[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CSP_NACC; ++i) {
    double s = part[0][i][lane];
#pragma unroll
    for (int w = 1; w < CSP_NW; ++w) s += part[w][i][lane];
    acc[i] = s;
  }
}

template <int H, int NOISE, bool U16>
__global__ __launch_bounds__(CSP_NW * 64) void vc_cell_speed_kernel(const void* __restrict__ counts, long long Ng, long long Nc,
                                                                    long long gene_stride, const float* __restrict__ B,
                                                                    const float* __restrict__ logm_in, const double* __restrict__ nu_in,
                                                                    const double* __restrict__ xy_in, const float* __restrict__ r_in,
                                                                    const double* __restrict__ prior, const double* __restrict__ start,
                                                                    double tol, int max_iter, double* __restrict__ omega_out,
                                                                    double* __restrict__ var_out, double* __restrict__ sums_out,
                                                                    double* __restrict__ dec_out, int* __restrict__ iter_out,
                                                                    int* __restrict__ status_out, int* __restrict__ clamped_out) {
  constexpr int K = 2 * H + 1;
  __shared__ double part[CSP_NW][CSP_NACC][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long c_raw = (long long)blockIdx.x * 64 + lane;
  const bool live = c_raw < Nc;
  const long long c = live ? c_raw : Nc - 1;                          // idle lanes of the last block repeat the last cell, store nothing
  csp_cdptr nu = (csp_cdptr)(const void*)nu_in;
  csp_cdptr xy = (csp_cdptr)(const void*)xy_in;
  csp_cfptr rg = (csp_cfptr)(const void*)r_in;
  const long long per = (Ng + CSP_NW - 1) / CSP_NW;                   // the gene share of this wave: contiguous, a function of Ng alone
  const long long g_lo = per * wave < Ng ? per * wave : Ng;
  const long long g_hi = g_lo + per < Ng ? g_lo + per : Ng;
  const double nan = __builtin_nan("");

  double b[K];
  b[0] = 1.0;
#pragma unroll
  for (int i = 1; i < K; ++i) b[i] = (double)B[(long long)i * Nc + c];
  const double logm = (double)logm_in[c];
  double pm = 0.0, pp = 0.0;
  bool valid = true;
  if (prior) {
    pm = prior[c * 2 + 0];
    const double sd = prior[c * 2 + 1];
    valid = __builtin_fabs(pm) < 1.0e300 && sd > 0.0 && sd < 1.0e300;
    pp = 1.0 / (sd * sd);
    valid = valid && pp < 1.0e300;
    if (!valid) { pm = 0.0; pp = 0.0; }
  }
  double om = start[c];
  valid = valid && __builtin_fabs(om) < 1.0e300;
  if (!valid) om = 0.0;
  om = om > CSP_BOUND ? CSP_BOUND : (om < -CSP_BOUND ? -CSP_BOUND : om);

#define CSP_AT(OM) csp_pass<H, NOISE, U16>(counts, gene_stride, c, g_lo, g_hi, b, logm, nu, xy, rg, (OM), acc, part, lane, wave)
  double acc[CSP_NACC], cur[CSP_NACC];
  // what the lane's point says: gradient, the matrix of its step, the decrement, and whether and how the cell stops there
  double Gc = 0.0, Ac = 0.0, dec = 0.0, fcur = 0.0, step = 0.0, t = 1.0, trial = om;
  int status = VC_CSP_MAX_ITER, steps = 0, halvings = CSP_MAX_HALVINGS;
  bool active = true;
  bool first = true;
  for (;;) {
    CSP_AT(trial);
    bool accepted = false;
    if (first) {
      if (!(acc[CSP_K] > 0.0)) valid = false;                          // a cell without a count has no fit
      if (!valid) { status = VC_CSP_NO_DATA; active = false; }
      accepted = active;
    } else if (active) {
      const double u = trial - pm;
      const double f2 = acc[CSP_L] - 0.5 * pp * u * u;
      const double Am = acc[CSP_A] > cur[CSP_A] ? acc[CSP_A] : cur[CSP_A];
      if (f2 >= fcur - 8.0 * GENE_EPS32 * Am) {                       // false for a NaN: such a step is halved
        accepted = true;
        om = trial;
        ++steps;
      } else if (halvings == 0) {
        status = VC_CSP_MAX_ITER;
        active = false;
      } else {
        --halvings;
        t *= 0.5;
        trial = __builtin_fma(t, step, om);
      }
    }
    if (accepted) {                                                   // acc holds the sums at om: decide there
#pragma unroll
      for (int i = 0; i < CSP_NACC; ++i) cur[i] = acc[i];
      const double u = om - pm;
      Gc = __builtin_fma(-pp, u, cur[CSP_S]);
      fcur = cur[CSP_L] - 0.5 * pp * u * u;
      Ac = cur[CSP_O] + pp;
      if (!(Ac > 0.0 && Ac < 1.0e300)) Ac = cur[CSP_F] + pp;
      step = Gc / Ac;
      dec = Gc * step;
      if (max_iter == 0) { status = VC_CSP_EVALUATED; active = false; }
      else if (!(__builtin_fabs(dec) < 1.0e300)) { status = VC_CSP_MAX_ITER; active = false; }
      else if (dec <= tol) { status = VC_CSP_CONVERGED; active = false; }
      else if (__builtin_fabs(Gc) <= 4.0 * GENE_EPS32 * __builtin_sqrt(cur[CSP_N])) { status = VC_CSP_ROUNDING; active = false; }
      else if (steps >= max_iter) { status = VC_CSP_MAX_ITER; active = false; }
      else {
        t = 1.0;
        trial = om + step;
        if (!(__builtin_fabs(trial) <= CSP_BOUND)) { status = VC_CSP_UNBOUNDED; active = false; }
      }
    }
    first = false;
    if (!active) trial = om;                                          // a stopped lane rides along at its own point; its sums are not read
    if (!__any(active)) break;                                        // the same lanes in every wave: uniform over the workgroup
  }
#undef CSP_AT

  if (wave == 0 && live) {
    const bool ok = status != VC_CSP_NO_DATA;
    omega_out[c] = ok ? om : nan;
    var_out[c] = ok ? 1.0 / Ac : nan;
#pragma unroll
    for (int i = 0; i < CSP_NOUT; ++i) sums_out[c * CSP_NOUT + i] = ok ? cur[i] : nan;
    dec_out[c] = ok ? dec : nan;
    iter_out[c] = ok ? steps : 0;
    status_out[c] = status;
    clamped_out[c] = ok ? (int)cur[CSP_C] : 0;
  }
}

constexpr char CSP_FN[] = "vc_cell_speed";

}  // namespace

extern "C" int vc_cell_speed(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev,
                             int K, const float* logm_dev, const double* nu_dev, const double* xy_dev, int noise, const float* r_dev,
                             const double* prior_dev, const double* start_dev, double tol, int max_iter, double* omega_dev,
                             double* var_dev, double* sums_dev, double* dec_dev, int32_t* iterations_dev, int32_t* status_dev,
                             int32_t* n_clamped_dev, void* hip_stream) {
  const char* own = nullptr;                                         // what only this entry point says, reported in its place among the shared refusals
  if (K == 7) own = "K must be 3 or 5: H = 3 is not instantiated";
  else if (K != 3 && K != 5) own = "K must be 3 or 5 (2 H + 1, H in {1, 2}; H = 0 has no velocity)";
  const int refused = gene_refuse(CSP_FN, noise, count_kind, own, Ng, Nc, true, gene_stride, 0, max_iter, tol);
  if (refused != VC_OK) return refused;
  if (!counts_dev || !basis_dev || !logm_dev || !nu_dev || !xy_dev) return gene_fail(CSP_FN, VC_ERR_ARG, "null input pointer");
  if (!start_dev) return gene_fail(CSP_FN, VC_ERR_ARG, "start_dev is required: the angular speed every cell starts from");
  if (!omega_dev || !var_dev || !sums_dev || !dec_dev || !iterations_dev || !status_dev || !n_clamped_dev) return gene_fail(CSP_FN, VC_ERR_ARG, "null output pointer");
  if (noise == VC_NOISE_NB && !r_dev) return gene_fail(CSP_FN, VC_ERR_ARG, "the negative binomial needs r_dev (1 / dispersion per gene)");
  const dim3 grid((unsigned)((Nc + 63) / 64)), block(CSP_NW * 64);
  hipStream_t st = (hipStream_t)hip_stream;
#define CSP_LAUNCH(H, NOISE, U16)                                                                                                      \
  hipLaunchKernelGGL((vc_cell_speed_kernel<H, NOISE, U16>), grid, block, 0, st, counts_dev, (long long)Ng, (long long)Nc,                \
                     (long long)gene_stride, basis_dev, logm_dev, nu_dev, xy_dev, r_dev, prior_dev, start_dev, tol, max_iter, omega_dev, \
                     var_dev, sums_dev, dec_dev, (int*)iterations_dev, (int*)status_dev, (int*)n_clamped_dev)
#define CSP_LAUNCH_H(H)                                                                                                               \
  do {                                                                                                                                \
    if (noise == VC_NOISE_NB) { if (u16) CSP_LAUNCH(H, VC_NOISE_NB, true); else CSP_LAUNCH(H, VC_NOISE_NB, false); }                     \
    else { if (u16) CSP_LAUNCH(H, VC_NOISE_POISSON, true); else CSP_LAUNCH(H, VC_NOISE_POISSON, false); }                                \
  } while (0)
  const bool u16 = count_kind == VC_COUNTS_U16;
  if (K == 3) CSP_LAUNCH_H(1); else CSP_LAUNCH_H(2);
#undef CSP_LAUNCH_H
#undef CSP_LAUNCH
  return gene_launched(CSP_FN);
}
