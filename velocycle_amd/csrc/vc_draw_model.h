// The model's mean under one posterior draw, shared by everything that consumes draws: the pointwise predictive density
// (vc_pointwise.hip) and the posterior predictive check (vc_ppc.hip).  eta_S / eta_U of one (draw, gene, cell) in log2 units, as
// vc_main_math.h has them, and the access to the engine's blocked counts.  The density that is scored and the density the
// replicates are sampled from are the statements below, once.
// Every function takes the pointers and scalars it needs, not an args struct, and returns results; where a load belongs to it (the
// latents of one (draw, gene), nuomega of one draw) it is written here, so every kernel performs the same loads in the same order.
// Every product-sum is written as the fma, or the separate multiply and add, it is meant to be.  That relies on the including
// translation unit's `#pragma clang fp contract(off)`: include this header after it (vc_pointwise.hip has its own, vc_ppc.hip
// receives the one of vc_count_sampler.h).  The same statement then gives the same bits in every kernel it is inlined into.
// Reference: velocity_inference_model.py:338-386, phase_inference_model.py:343-395.
#pragma once
#include "vc_site_math.h"

// sin / cos of k phi, k = 1 .. VC_MAXH, of the packed direction (x, y) (compile-time count: sk / ck stay in registers)
__device__ __forceinline__ void vc_dm_basis(float x, float y, float* sk, float* ck) {
  float s1, c1;
  vc_dir_sincos(x, y, &s1, &c1);
  vc_harmonics(s1, c1, VC_MAXH, sk, ck);
}

// omega ln 2 of cell c: omega = sum_x Dm[x, c] (nw[x, 0] + sum_k nw[x, 2k + 1] sin + nw[x, 2k + 2] cos), nw = nuomega of the draw
__device__ __forceinline__ float vc_dm_omega_l2(const float* nw, const float* Dm, int Nx, int Hw, int Nc, int c, const float* sk,
                                                const float* ck) {
  const int nhw = 2 * Hw + 1;
  float omega = 0.f;
  for (int xq = 0; xq < Nx; ++xq) {
    float o = nw[xq * nhw];
#pragma unroll
    for (int k = 0; k < VC_MAXH; ++k)
      if (k < Hw) o += nw[xq * nhw + 2 * k + 1] * sk[k] + nw[xq * nhw + 2 * k + 2] * ck[k];
    omega += Dm[(size_t)xq * Nc + c] * o;
  }
  return omega * VC_LN2;
}

// gene g's latents of draw dr in log2 units: an[2 H + 1] = nu log2 e and, for the velocity model, gam = gamma, lb2 = log2 beta
template <int H, bool VEL>
__device__ __forceinline__ void vc_dm_latents(const float* nu, long long nu_ds, const float* loggamma, long long lg_ds,
                                              const float* logbeta, long long lb_ds, int dr, int g, float* an, float& gam, float& lb2) {
  constexpr int NH = 2 * H + 1;
  const float* nud = nu + (size_t)dr * nu_ds + (size_t)g * NH;
#pragma unroll
  for (int h = 0; h < NH; ++h) an[h] = nud[h] * VC_LOG2E;
  if (VEL) {
    gam = __builtin_amdgcn_exp2f(loggamma[(size_t)dr * lg_ds + g] * VC_LOG2E);
    lb2 = logbeta[(size_t)dr * lb_ds + g] * VC_LOG2E;
  }
}

// (log count factor + batch offset of gene g in cell c) log2 e; cf: the cell's count factor, loaded by the caller
__device__ __forceinline__ float vc_dm_e0(float cf, const float* Dbm, const float* dnu, int Nb, int Nc, int Ng, int c, int g) {
  float e = cf;
  for (int q = 0; q < Nb; ++q) e = __builtin_fmaf(Dbm[(size_t)q * Nc + c], dnu[(size_t)q * Ng + g], e);
  return e * VC_LOG2E;
}

// log2 of the spliced mean; s / c = sin, cos of k phi of the cell
template <int H>
__device__ __forceinline__ float vc_dm_eta_S(const float* an, float e0, const float* s, const float* c) {
  float eta = an[0] + e0;
#pragma unroll
  for (int k = 0; k < H; ++k) {
    eta = __builtin_fmaf(an[2 * k + 1], s[k], eta);
    eta = __builtin_fmaf(an[2 * k + 2], c[k], eta);
  }
  return eta;
}

// log2 of the unspliced mean: eta_S - log2 beta + log2(relu(d eta_S / d phi omega + gamma) + 1e-5), oml = omega ln 2
template <int H>
__device__ __forceinline__ float vc_dm_eta_U(const float* an, float etaS, float lb2, float gam, float oml, const float* s, const float* c) {
  float dd = 0.f;
#pragma unroll
  for (int k = 0; k < H; ++k) {
    dd = __builtin_fmaf((float)(k + 1) * an[2 * k + 1], c[k], dd);
    dd = __builtin_fmaf(-(float)(k + 1) * an[2 * k + 2], s[k], dd);
  }
  const float z = __builtin_fmaf(dd, oml, gam);
  const float zz = __builtin_fmaxf(z, 0.f) + 1e-5f;
  return (etaS - lb2) + __builtin_amdgcn_logf(zz);
}

// the engine's blocked counts [gene block][cell position][gbw] as vc_finalize left them: element (gene g, position pos) with
// lay_blk = g / gbw, lay_in = g % gbw (g < Ng_pad: the layout is zero padded); U16: uint16 storage, else float32
__device__ __forceinline__ size_t vc_dm_count_index(size_t lay_blk, int Nc, int pos, int gbw, size_t lay_in) {
  return (lay_blk * (size_t)Nc + (size_t)pos) * (size_t)gbw + lay_in;
}
template <bool U16>
__device__ __forceinline__ float vc_dm_count(const void* p, size_t i) {
  if (U16) return (float)((const unsigned short*)p)[i];
  return ((const float*)p)[i];
}
