// Per-site model arithmetic of the SVI step, shared by every step path: the unfused kernels (vc_small_kernels.hip), the
// fused / sharded tails (vc_fused_kernels.hip) and the run-time-sized set (vc_generic_kernels.hip).  Guide samples
// (reparameterised draws), their log q terms, prior log-densities and the chain rule from K_main's reduced sums to the
// parameter gradients.  Every function works on values the caller has already loaded and returns results: none reads or
// writes a buffer, so each kernel keeps its own load schedule.
// Included by those three translation units, and for vc_harmonics by vc_draw_model.h (the consumers of posterior draws), after
// their `#pragma clang fp contract(off)`: the same statement gives the same bits in every kernel it is inlined into.  The
// likelihood kernels (vc_main_*.hip) do not see this header.
// Reference: velocity_inference_guide.py:9-141, phase_inference_guide.py:10-56, the priors of
// velocity_inference_model.py:322-353,383 / phase_inference_model.py:360-366,392.
#pragma once
#include "vc_common.h"

#define VC_PG_WAVES 16                                  // waves of a gene block of K_post / K_tail (lanes = 64 genes)
#define VC_MAXQ (2 * VC_MAXH + 1 + VC_MAXNB + 3)        // rows of K_main's gene-level partials at most

// ---- mean-field sites ----------------------------------------------------------------------------------------
// x = loc + exp(u) e, and log q(x) = -e^2 / 2 - u - log(2 pi) / 2
__device__ __forceinline__ float vc_mf_draw(float loc, float u, float e, float& lq) {
  lq = -0.5f * e * e - u - 0.5f * VC_LOG_2PI;
  return loc + expf(u) * e;
}
// d log p / d x of a site with a Normal(mu, sd) prior: the likelihood part `lik` plus the (root_w-weighted) prior term
__device__ __forceinline__ float vc_prior_grad(float lik, float x, float mu, float sd, float rw) {
  return lik - rw * (x - mu) / (sd * sd);
}
// d loss / d u (log scale) of a mean-field site, gx = d log p / d x; the entropy term of q contributes -rw
__device__ __forceinline__ float vc_mf_uscale_grad(float gx, float u, float e, float rw) {
  return -gx * expf(u) * e - rw;
}

// ---- shape_inv: Gamma(alpha, beta) log prior --------------------------------------------------------------------
__device__ __forceinline__ float vc_gamma_lp(const VcDims& d, float si) {
  return d.gamma_alpha * logf(d.gamma_beta) + (d.gamma_alpha - 1.f) * logf(si) - d.gamma_beta * si - d.lgamma_alpha;
}

// ---- log gamma / log beta: their reduced K_main rows by kernel kind ----------------------------------------------
// U_lb = d loglik / d log beta, U_lg = d loglik / d log gamma; T(q) = reduced row q (evaluated for the two rows read only)
template <class F>
__device__ __forceinline__ void vc_lb_lg_lik(int kind, int K, float gam, F T, float& U_lb, float& U_lg) {
  if (kind == VC_KIND_VFULL) { U_lb = -T(K); U_lg = T(K + 1) * gam; }
  else { U_lb = -T(0); U_lg = T(1) * gam; }
}

// ---- LRMN guide of (log gamma, log beta) ----------------------------------------------------------------------
// LowRankMultivariateNormal.rsample, X = loc + W eps_W + sqrt(cov_diag) eps_D, for the gene's row of the joint guide;
// q(log beta | log gamma) = N(a + rho s_b delta / s_gamma, s_b sqrt(1 - rho^2)).  delta, w2: sum_k W[k] eps_W[k] and
// sum_k W[k]^2 as the caller added them up (the association differs between the paths)
struct VcLrmnDraw { float lg, lb, delta, sgam, lq; };
__device__ __forceinline__ VcLrmnDraw vc_lrmn_draw(const VcDims& d, float delta, float w2, float udiag, float ed, float loc_g,
                                                   float loc_b, float ub, float rho_real, float eb) {
  VcLrmnDraw r;
  const float dg = expf(udiag);
  delta += sqrtf(dg) * ed;
  r.sgam = sqrtf(w2 + dg);
  r.lg = loc_g + delta;
  const float rho = sigmoidf_(rho_real / d.rho_scale) * 1.998f - 0.999f;
  const float sb = expf(ub);
  const float tt = sb * sqrtf(1.f - rho * rho);
  r.lb = loc_b + rho * sb * delta / r.sgam + tt * eb;
  r.lq = -0.5f * eb * eb - logf(tt) - 0.5f * VC_LOG_2PI;
  r.delta = delta;
  return r;
}
// the nu_omega rows of the LRMN guide (no conditional part): loc + delta, delta completed by the cov_diag term
__device__ __forceinline__ float vc_lrmn_row_draw(float loc, float delta, float udiag, float ed, float& delta_out) {
  delta += sqrtf(expf(udiag)) * ed;
  delta_out = delta;
  return loc + delta;
}
// chain rule of the joint guide, the part every LRMN role needs: g_lg, g_lb = d log p / d log gamma, d log beta
struct VcLrmnChain { float sb, sg, rho, om, sq, dl_ddelta, dl_dsg; };
__device__ __forceinline__ VcLrmnChain vc_lrmn_chain(const VcDims& d, float g_lg, float g_lb, float delta, float sgam, float ub,
                                                     float rho_real) {
  VcLrmnChain c;
  c.sb = expf(ub);
  c.sg = sigmoidf_(rho_real / d.rho_scale);
  c.rho = c.sg * 1.998f - 0.999f;
  c.om = 1.f - c.rho * c.rho;
  c.sq = sqrtf(c.om);
  c.dl_ddelta = -g_lg - g_lb * c.rho * c.sb / sgam;
  c.dl_dsg = g_lb * c.rho * c.sb * delta / (sgam * sgam);
  return c;
}
// ... the gradients of the gene's core parameters: log beta loc / log scale, rho_real, LRMN loc, log cov_diag.
// cb, cr: log beta / rho_real conditioned (cb drops the guide's -log(std) term)
struct VcLrmnCoreGrad { float loc_b, uscale_b, rho_real, loc, udiag; };
__device__ __forceinline__ VcLrmnCoreGrad vc_lrmn_core_grad(const VcDims& d, const VcLrmnChain& c, float g_lg, float g_lb, bool cb,
                                                            bool cr, float delta, float sgam, float rho_real, float eb,
                                                            float udiag, float ed, float rw) {
  VcLrmnCoreGrad r;
  const float A = g_lb;
  const float ent = cb ? 0.f : rw;        // weight of the guide's -log(std) term
  r.loc_b = -A;
  r.uscale_b = -A * (c.rho * delta / sgam + c.sq * eb) * c.sb - ent;
  const float g_rho = -A * (c.sb * delta / sgam - c.sb * c.rho * eb / c.sq) + ent * c.rho / c.om;
  r.rho_real = g_rho * 1.998f * c.sg * (1.f - c.sg) / d.rho_scale;
  if (!cr) r.rho_real += rw * (rho_real - d.rho_mean) / (d.rho_std * d.rho_std);
  r.loc = -g_lg;
  const float dg = expf(udiag);
  r.udiag = (c.dl_ddelta * ed / (2.f * sqrtf(dg)) + c.dl_dsg / (2.f * sgam)) * dg;
  return r;
}
// ... and of one cov_factor entry (log W, eps_W of its column)
__device__ __forceinline__ float vc_lrmn_cov_grad(const VcLrmnChain& c, float sgam, float u, float ew) {
  const float w = expf(u);
  return (w > 0.f) ? (c.dl_ddelta * ew + c.dl_dsg * w / sgam) * w : 0.f;
}

// ---- nu_omega -------------------------------------------------------------------------------------------------
// gradient of parameter element ce of coefficient j, gx = d log p / d nu_omega_j, p = the parameter, e = its eps:
// mean-field ce = 0 loc, 1 log scale (cnd: conditioned); LRMN ce = 0 loc, 1..R cov_factor entries, R + 1 log cov_diag
__device__ __forceinline__ float vc_nuw_elem_grad(bool lrmn, int R, int ce, float gx, float p, float e, bool cnd, float rw) {
  if (ce == 0) return -gx;
  if (!lrmn) return cnd ? 0.f : vc_mf_uscale_grad(gx, p, e, rw);
  if (ce <= R) {
    const float w = expf(p);
    return (w > 0.f) ? -gx * e * w : 0.f;
  }
  const float dg = expf(p);
  return -gx * e / (2.f * sqrtf(dg)) * dg;
}

// ---- phi_xy (the cell's phase as a point of the plane, prior N(pxy, 1), guide N(loc, 1)) ----------------------------
// -(log p - log q) of the sample (x, y) = loc + (ex, ey): the -log(2 pi) of prior and guide cancel; conditioned: prior only
__device__ __forceinline__ double vc_phixy_loss(float x, float y, float px, float py, float ex, float ey, bool cnd) {
  return cnd ? 0.5 * ((double)(x - px) * (x - px) + (double)(y - py) * (y - py)) + (double)VC_LOG_2PI
             : 0.5 * ((double)(x - px) * (x - px) + (double)(y - py) * (y - py)) - 0.5 * ((double)ex * ex + (double)ey * ey);
}
// d loss / d loc from K_main's per-cell sums A[] (d loglik / d phi = A0, + omega A1 + d omega / d phi A2 for the S+U kernel)
// through phi = atan2(y, x)
__device__ __forceinline__ float2 vc_phixy_grad(int kind, const float* A, float om, float dom, float x, float y, float px, float py) {
  float dphi = A[0];
  if (kind == VC_KIND_VFULL) dphi += om * A[1] + A[2] * dom;
  const float inv = 1.0f / (x * x + y * y);
  return make_float2(-(dphi * (-y * inv) - (x - px)), -(dphi * (x * inv) - (y - py)));
}

// ---- Fourier basis ------------------------------------------------------------------------------------------
// sin / cos of k phi, k = 1 .. n (n <= VC_MAXH), by the angle-addition recurrence from s1, c1 = sin, cos of phi
__device__ __forceinline__ void vc_harmonics(float s1, float c1, int n, float* sk, float* ck) {
  sk[0] = s1; ck[0] = c1;
  for (int k = 1; k < n && k < VC_MAXH; ++k) {
    sk[k] = sk[k - 1] * c1 + ck[k - 1] * s1;
    ck[k] = ck[k - 1] * c1 - sk[k - 1] * s1;
  }
}
