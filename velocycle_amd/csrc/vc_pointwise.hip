// Pointwise predictive density over posterior draws: the kernels behind vc_pointwise_density of include/velocycle_hip.h.
// The reference has no function for it; its model code (velocity_inference_model.py:338-386, phase_inference_model.py:343-395)
// defines the quantity: for draw d, gene g, cell c the log-probability l_d of the observed count, and per element
//   lppd = log((1/D) sum_d exp l_d),   mean = (1/D) sum_d l_d,   pwaic = sum_d (l_d - mean)^2 / (D - 1).
//
// Mapping.  A workgroup owns 64 consecutive cells (in the caller's order) and ALL genes; its PW_NW waves deal out the blocks of 64
// genes (lane = gene).  For a gene block a wave walks the 64 cells in tiles of TC cells whose per-element state -- first draw's
// value, running maximum, rescaled sum of exponentials, shifted Welford mean and M2, per count matrix -- lives in VGPRs; the draw
// loop is inside.  Per draw a lane fetches its gene's latents (coalesced, L2-resident); the tile's cell records (sin / cos of
// k phi, omega) are formed by the lanes 0 .. TC-1 (one cell each) and handed to the wave as wave-uniform values (v_readlane).
// The counts are read once per launch, where vc_finalize put them (blocked layout, uint16 or float32, through cell_pos).
//
// Arithmetic: log2 units on the raw hardware exp2 / log2, as vc_main_math.h; per element and draw (velocity, negative binomial)
// exp2(eta_S), log2(r + mu_S), log2(relu(z) + 1e-5), exp2(eta_U), log2(r + mu_U) and one exp2 per matrix for the running
// log-sum-exp.  lgamma never appears here: lgamma(r + k) - lgamma(r) - lgamma(k + 1) (Poisson: -lgamma(k + 1)) is a constant of the
// (gene, count) pair, evaluated once per histogram entry in float64 (vc_pw_const_kernel) and added to lppd and mean behind the draw loop.
//
// Reductions: every element value becomes a float64 and is added (a) over the cells of the workgroup in cell order by the gene's lane
// -> one partial row per workgroup, folded over the workgroups in order by vc_pw_fold_kernel, continuing from what gene_out holds;
// (b) over the 64 genes of the block by a fixed DPP tree, over the wave's gene blocks in order, over the waves in wave order through
// the LDS.  No atomics; identical bits for any cutting of the cells into calls at multiples of 64.
#include "vc_common.h"

// Every product-sum below is written as the fma it is meant to be; nothing else may be contracted: a ragged tile then performs the
// operations of a full one.
#pragma clang fp contract(off)
#include "vc_draw_model.h"      // eta_S / eta_U of one (draw, gene, cell) and the count access, shared with vc_ppc.hip
#include "vc_pw_lik.h"          // pw_lik / pw_const: the log2 bracket and its lgamma constant, shared with vc_pit.hip

namespace {

constexpr int PW_NW = 8;                    // waves per workgroup
constexpr double PW_LN2 = 0.693147180559945309417;

__device__ __forceinline__ float pw_rl(float v, int lane) {      // lane `lane` (compile-time) of v as a wave-uniform value
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

struct PwState { float l0, m, s, mean, m2; };
__device__ __forceinline__ void pw_init(PwState& q) { q.l0 = 0.f; q.m = -__builtin_inff(); q.s = 0.f; q.mean = 0.f; q.m2 = 0.f; }
// one draw: running maximum + rescaled sum of 2^(l - m); Welford on t = l - l0 (l0: the first draw's value)
__device__ __forceinline__ void pw_update(PwState& q, float l, bool first, float inv_n) {
  const float dl = l - q.m;
  const float e = __builtin_amdgcn_exp2f(-__builtin_fabsf(dl));
  if (dl > 0.f) { q.s = __builtin_fmaf(q.s, e, 1.f); q.m = l; } else q.s += e;
  q.l0 = first ? l : q.l0;
  const float t = l - q.l0;
  const float del = t - q.mean;
  q.mean = __builtin_fmaf(del, inv_n, q.mean);
  q.m2 = __builtin_fmaf(del, t - q.mean, q.m2);
}

// KIND 0: phase model (S) | 1: velocity (S and U per draw) | 2: velocity, everything eta_S depends on is the same in every draw
template <int H, int KIND, int NOISE, bool U16, int TC>
__global__ __launch_bounds__(PW_NW * 64) void vc_pointwise_kernel(const VcPwArgs a) {
  constexpr bool VEL = KIND != 0, SINV = KIND == 2;
  constexpr int NM = VEL ? 2 : 1, NQ = 3 * NM, NH = 2 * H + 1;
  __shared__ double cellacc[PW_NW][NQ][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < PW_NW * NQ * 64; i += PW_NW * 64) (&cellacc[0][0][0])[i] = 0.0;
  __syncthreads();
  const int super = blockIdx.x;
  const int cs0 = a.c_begin + super * 64;
  const int D = a.n_draws;
  const double inv_d = 1.0 / (double)D;
  const double inv_dm1 = 1.0 / (double)(D - 1);
  const bool rec_var = a.phixy_ds != 0;
  const bool om_var = rec_var || a.nw_ds != 0;
  const int nblk = (a.Ng + 63) >> 6;
  for (int gb = wave; gb < nblk; gb += PW_NW) {
    const int g_raw = gb * 64 + lane;
    const bool glive = g_raw < a.Ng;
    const int g = glive ? g_raw : a.Ng - 1;
    float r = 0.f, rl2 = 0.f;
    if (NOISE == VC_NOISE_NB) {
      r = 1.f / a.shape_inv[g];
      rl2 = r * __builtin_amdgcn_logf(r);
    }
    const size_t lay_blk = (size_t)(g_raw / a.gbw), lay_in = (size_t)(g_raw % a.gbw);      // (g_raw < Ng_pad: the layout is zero padded)
    double gacc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) gacc[q] = 0.0;
    for (int t0 = 0; t0 < 64 && cs0 + t0 < a.c_end; t0 += TC) {
      // the cell this lane forms the record of (lanes >= TC: cell 0 of the tile again, never read)
      const int cm_raw = cs0 + t0 + (lane < TC ? lane : 0);
      const int cm = cm_raw < a.c_end ? cm_raw : a.c_end - 1;
      float kS[TC], kU[TC], e0[TC], etaS[TC];
#pragma unroll
      for (int t = 0; t < TC; ++t) {
        const int c_raw = cs0 + t0 + t;
        const int c = c_raw < a.c_end ? c_raw : a.c_end - 1;                 // wave-uniform
        const int pos = a.cell_pos ? a.cell_pos[c] : c;
        const size_t idx = vc_dm_count_index(lay_blk, a.Nc, pos, a.gbw, lay_in);
        kS[t] = vc_dm_count<U16>(a.S, idx);
        kU[t] = VEL ? vc_dm_count<U16>(a.U, idx) : 0.f;
        e0[t] = vc_dm_e0(a.cf[c], a.Dbm, a.dnu, a.Nb, a.Nc, a.Ng, c, g);
        etaS[t] = 0.f;
      }
      PwState stS[TC], stU[TC];
#pragma unroll
      for (int t = 0; t < TC; ++t) { pw_init(stS[t]); pw_init(stU[t]); }
      float sk[VC_MAXH], ck[VC_MAXH], oml = 0.f;
#pragma unroll
      for (int k = 0; k < VC_MAXH; ++k) { sk[k] = 0.f; ck[k] = 0.f; }
#pragma unroll 1
      for (int dr = 0; dr < D; ++dr) {
        const bool first = dr == 0;
        if (first || rec_var) {
          const float* xy = a.phixy + (size_t)dr * a.phixy_ds + 2 * (size_t)cm;
          vc_dm_basis(xy[0], xy[1], sk, ck);
        }
        if (VEL && (first || om_var)) oml = vc_dm_omega_l2(a.nuomega + (size_t)dr * a.nw_ds, a.Dm, a.Nx, a.Hw, a.Nc, cm, sk, ck);
        // this gene's latents of draw dr, in log2 units
        float an[NH], gam = 0.f, lb2 = 0.f;
        vc_dm_latents<H, VEL>(a.nu, a.nu_ds, a.loggamma, a.lg_ds, a.logbeta, a.lb_ds, dr, g, an, gam, lb2);
        const float inv_n = 1.f / (float)(dr + 1);
#pragma unroll
        for (int t = 0; t < TC; ++t) {
          float sc[H], cc[H];
#pragma unroll
          for (int k = 0; k < H; ++k) { sc[k] = pw_rl(sk[k], t); cc[k] = pw_rl(ck[k], t); }
          if (!SINV || first) {
            etaS[t] = vc_dm_eta_S<H>(an, e0[t], sc, cc);
            pw_update(stS[t], pw_lik<NOISE>(kS[t], etaS[t], r, rl2), first, inv_n);
          }
          if (VEL) {
            const float etaU = vc_dm_eta_U<H>(an, etaS[t], lb2, gam, pw_rl(oml, t), sc, cc);
            pw_update(stU[t], pw_lik<NOISE>(kU[t], etaU, r, rl2), first, inv_n);
          }
        }
      }
      // behind the draw loop: float64 element values, the lgamma constants, the two families of sums
#pragma unroll
      for (int t = 0; t < TC; ++t) {
        const int c = cs0 + t0 + t;
        const bool live = glive && c < a.c_end;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const PwState& q = m == 0 ? stS[t] : stU[t];
          const double cst = pw_const(a, m, g, m == 0 ? kS[t] : kU[t]);
          double lp, mn, pw;
          if (SINV && m == 0) {
            lp = (double)q.l0 * PW_LN2 + cst;
            mn = lp;
            pw = 0.0;
          } else {
            // (s / D lies next to 1 where the draws agree: its logarithm in float64, once per element -- the hardware log2 of s and of
            // D apart would leave an absolute error of an ulp of log2 D, whatever the size of the element's own terms)
            lp = (double)q.m * PW_LN2 + log((double)q.s * inv_d) + cst;
            mn = ((double)q.l0 + (double)q.mean) * PW_LN2 + cst;
            pw = (double)q.m2 * (PW_LN2 * PW_LN2) * inv_dm1;
          }
          if (a.dense && live) a.dense[((size_t)m * a.Ng + g) * (size_t)a.Nc + c] = (float)lp;
          const double v[3] = {live ? lp : 0.0, live ? mn : 0.0, live ? pw : 0.0};
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            gacc[3 * m + j] += v[j];
            const double tot = vc_wave_sum_d63(v[j]);
            if (lane == 63) cellacc[wave][3 * m + j][t0 + t] += tot;
          }
        }
      }
    }
    if (glive) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) a.ws[((size_t)super * NQ + q) * (size_t)a.Ng + g] = gacc[q];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NQ * 64; i += PW_NW * 64) {
    const int q = i >> 6, t = i & 63;
    const int c = cs0 + t;
    if (c < a.c_end) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < PW_NW; ++w) s += cellacc[w][q][t];
      a.cell_out[(size_t)q * a.Nc + c] = s;
    }
  }
}

// gene_out[q][g] += the partial rows of the launch's workgroups, in workgroup (= cell) order
__global__ __launch_bounds__(256) void vc_pw_fold_kernel(const double* __restrict__ ws, int n_super, int NQ, int Ng, double* __restrict__ gene_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)NQ * Ng) return;
  double acc = gene_out[i];
  for (int s = 0; s < n_super; ++s) acc += ws[(size_t)s * NQ * Ng + i];
  gene_out[i] = acc;
}

// the lgamma constant of every histogram entry, in float64
__global__ __launch_bounds__(256) void vc_pw_const_kernel(int n, int Ng, int nmat, const int* __restrict__ h_ptr, const float* __restrict__ h_val,
                                                           const float* __restrict__ shape_inv, int noise, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = nmat * Ng;                   // the row j with h_ptr[j] <= i < h_ptr[j + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (h_ptr[mid] <= i) lo = mid; else hi = mid;
  }
  const int g = lo % Ng;
  const double k = (double)h_val[i];
  double v = -lgamma(k + 1.0);
  if (noise == VC_NOISE_NB) {
    const double r = 1.0 / (double)shape_inv[g];
    v += lgamma(r + k) - lgamma(r);
  }
  out[i] = v;
}

typedef void (*pw_kernel_t)(const VcPwArgs);

template <int H, int KIND, int NOISE>
pw_kernel_t pw_pick3(bool u16) {
  constexpr int TC = KIND == 1 ? 4 : 8;
  return u16 ? (pw_kernel_t)vc_pointwise_kernel<H, KIND, NOISE, true, TC> : (pw_kernel_t)vc_pointwise_kernel<H, KIND, NOISE, false, TC>;
}
template <int H, int KIND>
pw_kernel_t pw_pick2(int noise, bool u16) {
  return noise == VC_NOISE_NB ? pw_pick3<H, KIND, VC_NOISE_NB>(u16) : pw_pick3<H, KIND, VC_NOISE_POISSON>(u16);
}
template <int H>
pw_kernel_t pw_pick1(int kind, int noise, bool u16) {
  return kind == 0 ? pw_pick2<H, 0>(noise, u16) : (kind == 1 ? pw_pick2<H, 1>(noise, u16) : pw_pick2<H, 2>(noise, u16));
}

}  // namespace

void vc_launch_pw_const(int n_entries, int Ng, int nmat, const int* h_ptr, const float* h_val, const float* shape_inv, int noise,
                        double* out, hipStream_t st) {
  if (n_entries <= 0) return;
  hipLaunchKernelGGL(vc_pw_const_kernel, dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, st, n_entries, Ng, nmat, h_ptr, h_val,
                     shape_inv, noise, out);
}

int vc_launch_pointwise(const VcPwArgs& a, int H, int kind, int noise, int n_super, double* gene_out, hipStream_t st) {
  pw_kernel_t k = H == 1 ? pw_pick1<1>(kind, noise, a.c16 != 0) : (H == 2 ? pw_pick1<2>(kind, noise, a.c16 != 0) : (H == 3 ? pw_pick1<3>(kind, noise, a.c16 != 0) : nullptr));
  if (!k) return VC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k, dim3((unsigned)n_super), dim3(PW_NW * 64), 0, st, a);
  const int NQ = kind == 0 ? 3 : 6;
  hipLaunchKernelGGL(vc_pw_fold_kernel, dim3((unsigned)(((long long)NQ * a.Ng + 255) / 256)), dim3(256), 0, st, a.ws, n_super, NQ, a.Ng, gene_out);
  return VC_OK;
}
