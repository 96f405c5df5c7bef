// Predictive PIT (randomized quantile residuals, Dunn & Smyth 1996) of every observed count: the kernel behind vc_predictive_pit of
// include/velocycle_hip.h.  The reference has no function for it; its model code (velocity_inference_model.py:338-386,
// phase_inference_model.py:343-395) defines the likelihood.  For count matrix m, gene g, cell c with observed count k and D draws
//   F_lo = (1/D) sum_d P(K <= k - 1 | theta_d),   F_hi = (1/D) sum_d P(K <= k | theta_d),   u = F_lo + v (F_hi - F_lo),
// v the uniform of word 0 of the count sampler's Philox block (seed, g << 32 | GLOBAL cell, draw 0, matrix m, stage 2, attempt 0).
//
// Mapping.  That of vc_pointwise_kernel: a workgroup owns 64 consecutive cells (in the caller's order) and ALL genes; its PIT_NW waves
// deal out the blocks of 64 genes (lane = gene); a wave walks the 64 cells in tiles of TC cells whose per-element state -- the lgamma
// constant of (gene, count), looked up once, and the two running sums over the draws per matrix -- lives in VGPRs; the draw loop is
// inside.  Cell records reach the wave through v_readlane.  The price: the lanes of a wave hold different genes, so their CDF loops
// have different lengths and the wave runs the longest (DESIGN.md section 5 has the alternative and why it was not taken).
//
// The CDF.  k = 0: F_lo = 0, F_hi = pmf(0), no loop.  Otherwise the LOWER tail, downward from k, relative to pmf(k):
//   t_k = 1,  t_(j-1) = t_j j / ((r + j - 1) q),  q = mu / (r + mu)   (Poisson: t_j j / mu),
//   F_lo = pmf(k) sum_(j<k) t_j,  F_hi = pmf(k) (1 + sum_(j<k) t_j),
// pmf(k) = 2^(bracket + constant): the log2 bracket of pw_lik (float32) plus the float64 lgamma constant of the histogram entry, added in
// float64 BEFORE the exp2.  The terms grow down to the mode when k lies in the upper tail (pmf(k) = 6e-161 occurs on the fixtures): t
// and the sum are rescaled by 2^-60 whenever t passes 2^30 and the exponent is carried into the exp2, so nothing overflows.  Past
// the mode (ratio < 1; the ratio falls with j for r > 1 and for Poisson, and never drops below 1 for r <= 1, whose pmf decreases from 0)
// the loop stops once the geometric bound of what is left, t / (1 - ratio), is below 2^-26 of the sum.  A rate below 2^-30 has
// P(K >= 1) <= mu < eps32: F_hi = pmf(0), F_lo = [k > 0] pmf(0).  Counts are integers below 2^24 (the host refuses others): float32
// holds every j on the way down, and the trip count is an integer.
//
// Sums.  Integers only.  The bin of u, min(B - 1, floor(u B)), is counted per (matrix, cell) in the LDS (the workgroup owns its cells:
// 32-bit LDS atomics over the waves' genes, then plain stores) and per (matrix, gene) with one 64-bit atomicAdd to global: exact, hence
// identical bits under any cutting of the cells into calls, storage type, cell order and repetition.  No float atomics.
#include "vc_count_sampler.h"   // vc_cs_block / vc_cs_uniform: the Philox stream v comes from
#pragma clang fp contract(off)
#include "vc_draw_model.h"      // eta_S / eta_U of one (draw, gene, cell) and the count access
#include "vc_pw_lik.h"          // the log2 bracket and its lgamma constant, shared with vc_pointwise.hip

namespace {

constexpr int PIT_NW = 8;                   // waves per workgroup
constexpr int PIT_MAXB = 64;                // bins (vc_predictive_pit refuses more)
constexpr float PIT_TINY = 9.313225746154785e-10f;        // 2^-30: below this rate every count >= 1 has F_lo = F_hi = pmf(0) to eps32
constexpr float PIT_BIG = 1073741824.f;                   // 2^30: rescale threshold of a relative term
constexpr float PIT_DOWN = 8.673617379884035e-19f;        // 2^-60
constexpr float PIT_STOP = 1.4901161193847656e-08f;       // 2^-26
constexpr double PIT_LOG2E = 1.44269504088896340736;

typedef unsigned long long u64;

__device__ __forceinline__ float pit_rl(float v, int lane) {     // lane `lane` (compile-time) of v as a wave-uniform value
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// P(K <= k - 1) and P(K <= k) of one (draw, element); c2: the lgamma constant of (gene, k) / ln 2
template <int NOISE>
__device__ __forceinline__ void pit_cdf(float k, float eta2, float r, float rl2, double c2, float& lo, float& hi) {
  const float mu = __builtin_amdgcn_exp2f(eta2);
  if (k == 0.f || mu < PIT_TINY) {
    const float p0 = __builtin_fminf(__builtin_amdgcn_exp2f(pw_lik<NOISE>(0.f, eta2, r, rl2)), 1.f);
    lo = k == 0.f ? 0.f : p0;
    hi = p0;
    return;
  }
  const float br = pw_lik<NOISE>(k, eta2, r, rl2);
  const float inv = NOISE == VC_NOISE_NB ? (r + mu) / mu : 1.f / mu;     // 1 / q, or 1 / mu
  float t = 1.f, s = 0.f, j = k;
  int e = 0;
  // (the trip count is an integer: the loop ends whatever float32 makes of j - 1; the host admits counts below 2^24 only)
#pragma unroll 1
  for (int n = k < 16777216.f ? (int)k : 0; n >= 1; --n) {
    float ratio = j * inv;
    if (NOISE == VC_NOISE_NB) ratio = ratio * __builtin_amdgcn_rcpf(r + (j - 1.f));
    t = t * ratio;
    s = s + t;
    j = j - 1.f;
    if (t >= PIT_BIG) { t = t * PIT_DOWN; s = s * PIT_DOWN; e += 60; }
    // past the mode the ratio keeps falling: what is left is below t ratio / (1 - ratio) < t / (1 - ratio)
    if (ratio < 1.f && t < (PIT_STOP * s) * (1.f - ratio)) break;
  }
  const float tk = __builtin_amdgcn_exp2f(-(float)e);                     // the term of k itself on the scale of s (1 when e = 0)
  const float P = __builtin_amdgcn_exp2f((float)(((double)br + c2) + (double)e));
  lo = __builtin_fminf(P * s, 1.f);
  hi = __builtin_fminf(P * (s + tk), 1.f);
}

template <int H, bool VEL, int NOISE, bool U16, int TC>
__global__ __launch_bounds__(PIT_NW * 64) void vc_pit_kernel(const VcPitArgs a) {
  constexpr int NM = VEL ? 2 : 1, NH = 2 * H + 1;
  __shared__ unsigned cellh[NM * 64 * PIT_MAXB];          // [matrix][cell of the workgroup][bin], bins at stride n_bins
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int B = a.n_bins;
  for (int i = threadIdx.x; i < NM * 64 * B; i += PIT_NW * 64) cellh[i] = 0u;
  __syncthreads();
  const int cs0 = a.c_begin + (int)blockIdx.x * 64;
  const int D = a.n_draws;
  const float fD = (float)D, fB = (float)B;
  const bool rec_var = a.phixy_ds != 0;
  const bool om_var = rec_var || a.nw_ds != 0;
  const int nblk = (a.Ng + 63) >> 6;
  for (int gb = wave; gb < nblk; gb += PIT_NW) {
    const int g_raw = gb * 64 + lane;
    const bool glive = g_raw < a.Ng;
    const int g = glive ? g_raw : a.Ng - 1;
    float r = 0.f, rl2 = 0.f;
    if (NOISE == VC_NOISE_NB) {
      r = 1.f / a.shape_inv[g];
      rl2 = r * __builtin_amdgcn_logf(r);
    }
    const size_t lay_blk = (size_t)(g_raw / a.gbw), lay_in = (size_t)(g_raw % a.gbw);      // (g_raw < Ng_pad: the layout is zero padded)
    for (int t0 = 0; t0 < 64 && cs0 + t0 < a.c_end; t0 += TC) {
      // the cell this lane forms the record of (lanes >= TC: cell 0 of the tile again, never read)
      const int cm_raw = cs0 + t0 + (lane < TC ? lane : 0);
      const int cm = cm_raw < a.c_end ? cm_raw : a.c_end - 1;
      float kk[NM][TC], e0[TC], lo[NM][TC], hi[NM][TC];
      double c2[NM][TC];
#pragma unroll
      for (int t = 0; t < TC; ++t) {
        const int c_raw = cs0 + t0 + t;
        const int c = c_raw < a.c_end ? c_raw : a.c_end - 1;                 // wave-uniform
        const int pos = a.cell_pos ? a.cell_pos[c] : c;
        const size_t idx = vc_dm_count_index(lay_blk, a.Nc, pos, a.gbw, lay_in);
        kk[0][t] = vc_dm_count<U16>(a.S, idx);
        if (VEL) kk[NM - 1][t] = vc_dm_count<U16>(a.U, idx);
        e0[t] = vc_dm_e0(a.cf[c], a.Dbm, a.dnu, a.Nb, a.Nc, a.Ng, c, g);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          c2[m][t] = pw_const(a, m, g, kk[m][t]) * PIT_LOG2E;
          lo[m][t] = 0.f;
          hi[m][t] = 0.f;
        }
      }
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
#pragma unroll
        for (int t = 0; t < TC; ++t) {
          float sc[H], cc[H];
#pragma unroll
          for (int k = 0; k < H; ++k) { sc[k] = pit_rl(sk[k], t); cc[k] = pit_rl(ck[k], t); }
          float eta[NM];
          eta[0] = vc_dm_eta_S<H>(an, e0[t], sc, cc);
          if (VEL) eta[NM - 1] = vc_dm_eta_U<H>(an, eta[0], lb2, gam, pit_rl(oml, t), sc, cc);
#pragma unroll
          for (int m = 0; m < NM; ++m) {
            float l1, h1;
            pit_cdf<NOISE>(kk[m][t], eta[m], r, rl2, c2[m][t], l1, h1);
            lo[m][t] = lo[m][t] + l1;
            hi[m][t] = hi[m][t] + h1;
          }
        }
      }
      // behind the draw loop: the averages, the uniform of (matrix, gene, global cell), u and its bin
#pragma unroll
      for (int t = 0; t < TC; ++t) {
        const int c = cs0 + t0 + t;
        const bool live = glive && c < a.c_end;
        const uint64_t idx = ((uint64_t)g << 32) | (uint64_t)(a.cell_offset + c);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const float Flo = __builtin_fminf(lo[m][t] / fD, 1.f), Fhi = __builtin_fminf(hi[m][t] / fD, 1.f);
          uint32_t w[4];
          vc_cs_block(a.seed, idx, 0u, (uint32_t)m, 2u, 0u, w);
          const float v = vc_cs_uniform(w[0]);
          float u = __builtin_fmaf(v, Fhi - Flo, Flo);
          u = __builtin_fminf(__builtin_fmaxf(u, 0.f), 0.99999994f);          // [0, 1): the largest float32 below 1
          int bin = (int)__builtin_floorf(u * fB);
          bin = bin > B - 1 ? B - 1 : (bin < 0 ? 0 : bin);
          if (live) {
            if (a.dense) {
              float* dst = a.dense + ((size_t)(3 * m) * a.Ng + g) * (size_t)a.Nc + c;
              const size_t plane = (size_t)a.Ng * (size_t)a.Nc;
              dst[0] = Flo;
              dst[plane] = Fhi;
              dst[2 * plane] = u;
            }
            atomicAdd(&cellh[(m * 64 + t0 + t) * B + bin], 1u);
            atomicAdd(a.gene_hist + ((size_t)m * a.Ng + g) * (size_t)B + bin, (u64)1);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NM * 64 * B; i += PIT_NW * 64) {
    const int m = i / (64 * B), rem = i - m * 64 * B;
    const int c = cs0 + rem / B;
    if (c < a.c_end) a.cell_hist[((size_t)m * a.Nc + c) * (size_t)B + rem % B] = (u64)cellh[i];
  }
}

typedef void (*pit_kernel_t)(const VcPitArgs);

template <int H, bool VEL, int NOISE>
pit_kernel_t pit_pick3(bool u16) {
  constexpr int TC = 4;
  return u16 ? (pit_kernel_t)vc_pit_kernel<H, VEL, NOISE, true, TC> : (pit_kernel_t)vc_pit_kernel<H, VEL, NOISE, false, TC>;
}
template <int H, bool VEL>
pit_kernel_t pit_pick2(int noise, bool u16) {
  return noise == VC_NOISE_NB ? pit_pick3<H, VEL, VC_NOISE_NB>(u16) : pit_pick3<H, VEL, VC_NOISE_POISSON>(u16);
}
template <int H>
pit_kernel_t pit_pick1(bool vel, int noise, bool u16) {
  return vel ? pit_pick2<H, true>(noise, u16) : pit_pick2<H, false>(noise, u16);
}

}  // namespace

int vc_launch_pit(const VcPitArgs& a, int H, bool vel, int noise, hipStream_t st) {
  pit_kernel_t k = H == 1 ? pit_pick1<1>(vel, noise, a.c16 != 0) : (H == 2 ? pit_pick1<2>(vel, noise, a.c16 != 0) : (H == 3 ? pit_pick1<3>(vel, noise, a.c16 != 0) : nullptr));
  if (!k || a.n_bins < 2 || a.n_bins > PIT_MAXB) return VC_ERR_UNSUPPORTED;
  const unsigned n_super = (unsigned)((a.c_end - a.c_begin + 63) / 64);
  hipLaunchKernelGGL(k, dim3(n_super), dim3(PIT_NW * 64), 0, st, a);
  return VC_OK;
}
