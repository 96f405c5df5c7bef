// Phase-marginal scoring: the kernel behind vc_phase_marginal of include/velocycle_hip.h.  The reference has no function for it; its
// model code (velocity_inference_model.py:338-386, phase_inference_model.py:343-395) defines the likelihood and Phases.from_cycle_mle
// (phases.py:471-509) the grid phi_j = 2 pi j / B (:495) and the point-estimate special case.  For cell c, draw d of the gene-level and
// global sites and grid phase j
//   a[d,c,j]      = lw[c,j] + sum_matrices sum_g log p(k_gc | theta_d, phi_j)
//   evidence[c]   = log((1/D) sum_d sum_j exp a),   post[c,j] = sum_d exp a[d,c,j] / sum_d sum_j' exp a[d,c,j'],
//   per_draw[d,c] = log sum_j exp a[d,c,j].
//
// Mapping: lane = cell, as vc_phase_mle_kernel.  A workgroup owns 64 consecutive cells (in the caller's order); its PM_NW waves split
// the genes into contiguous shares of whole chunks.  The bins are walked in tiles of PM_BT; the draw loop is inside a tile.  Per
// (tile, draw) a wave takes PM_GC genes at a time: their counts (through cell_pos, blocked layout: a strided read that is reused
// PM_BT times and does not matter), count-factor + batch offset, and the gene's latents of the draw, which are wave-uniform (scalar
// loads, as vc_ppc_kernel).  For every bin of the tile the PM_GC log2 brackets of pw_lik are summed in float32 and that short sum is added
// to the bin's float64 accumulator -- one for the spliced, one for the unspliced matrix.  The bin's sin / cos row comes from a table
// the host formed in float64 (scalar loads); gfx950 has no scalar float arithmetic, so nu . zeta(phi_j), nu . zeta'(phi_j) and
// nuomega . zeta_omega(phi_j) are recomputed per lane with vc_dm_eta_S / vc_dm_eta_U / vc_dm_omega_l2: no table of size draws x genes x
// bins and no workspace for one.  The waves' float64 partials meet in the LDS and are added by wave 0 in wave order (no atomics).
//
// The spliced term.  When nothing it depends on varies over the draws (nu given once; dnu and shape_inv are single values) the S sums
// of a tile are formed once, before the draw loop; otherwise per draw, by the same statements into the same accumulator: equal bits.
//
// lgamma.  The constant of an element depends on neither bin nor draw: it is looked up in the engine's histogram (pw_const, float64)
// and summed once per cell, in gene order within a wave and wave order across them, then added to every a of the cell.
//
// Reduction over bins and draws (wave 0, float64, library exp / log, once per (cell, bin, draw)).  Per (tile, draw): m = max_j a,
// e_j = exp(a_j - m); the draw's running log-sum-exp over the tiles lives in per_draw itself; the bins' sums over the draws are kept
// relative to the tile's running maximum M (rescaled when it rises) and leave the tile as log masses M + log sum in the workspace
// [n_bins][cells of the launch] (float64).  Behind the last tile the lane reads its column back: evidence = logsumexp - log D, post =
// exp(log mass - logsumexp) as float32.  Everything is relative to a maximum: finite a, however negative, give finite results.
// Every output of a cell is a function of that cell's lane alone: identical bits under any cutting of the cells, count storage type,
// cell order and sharding.
#include "vc_common.h"

#pragma clang fp contract(off)
#include "vc_draw_model.h"      // eta_S / eta_U of one (draw, gene, cell), omega, the latents' loads and the count access
#include "vc_pw_lik.h"          // the log2 bracket and its lgamma constant

namespace {

constexpr int PM_NW = 4;         // waves per workgroup (= gene shares)
constexpr int PM_BT = 16;        // bins per tile
constexpr int PM_GC = 4;         // genes per chunk
constexpr double PM_LN2 = 0.693147180559945309417;

typedef double pm_part_t[PM_BT][64];

// v[jj] += the other waves' v[jj], in wave order, in wave 0 (the other waves keep their own)
__device__ __forceinline__ void pm_combine(double (&v)[PM_BT], pm_part_t* part, int wave, int lane) {
  __syncthreads();                                   // the readers of the previous round are done
  if (wave > 0) {
#pragma unroll
    for (int jj = 0; jj < PM_BT; ++jj) part[wave - 1][jj][lane] = v[jj];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll 1
    for (int w = 0; w < PM_NW - 1; ++w) {
#pragma unroll
      for (int jj = 0; jj < PM_BT; ++jj) v[jj] += part[w][jj][lane];
    }
  }
}

// the sin / cos of k phi_j, k = 1 .. H, of grid row j (wave-uniform)
template <int H>
__device__ __forceinline__ void pm_row(const float* grid, int j, float* s, float* c) {
  const float* row = grid + 8 * (size_t)j;
#pragma unroll
  for (int k = 0; k < H; ++k) { s[k] = row[k]; c[k] = row[VC_MAXH + k]; }
}

// One chunk of G genes [g0, g0 + G) under draw dr for the bins [j0, j0 + nb) of a tile: accS[jj] += sum_q bracket_S, accU likewise
template <int H, bool VEL, int NOISE, bool U16, int G>
__device__ __forceinline__ void pm_chunk(const VcPmArgs& a, int dr, int g0, int c, int pos, float cf, bool doS, bool doU, int j0, int nb,
                                         const float (&oml)[PM_BT], double (&accS)[PM_BT], double (&accU)[PM_BT]) {
  constexpr int NH = 2 * H + 1;
  float kS[G], kU[G], e0[G], r[G], rl2[G], an[G][NH], gam[G], lb2[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    const int g = g0 + q;                                                   // wave-uniform, < Ng
    const size_t idx = vc_dm_count_index((size_t)(g / a.gbw), a.Nc, pos, a.gbw, (size_t)(g % a.gbw));
    kS[q] = vc_dm_count<U16>(a.S, idx);
    kU[q] = VEL ? vc_dm_count<U16>(a.U, idx) : 0.f;
    e0[q] = vc_dm_e0(cf, a.Dbm, a.dnu, a.Nb, a.Nc, a.Ng, c, g);
    r[q] = 0.f;
    rl2[q] = 0.f;
    if (NOISE == VC_NOISE_NB) {
      r[q] = 1.f / a.shape_inv[g];
      rl2[q] = r[q] * __builtin_amdgcn_logf(r[q]);
    }
    gam[q] = 0.f;
    lb2[q] = 0.f;
    vc_dm_latents<H, VEL>(a.nu, a.nu_ds, a.loggamma, a.lg_ds, a.logbeta, a.lb_ds, dr, g, an[q], gam[q], lb2[q]);
  }
#pragma unroll
  for (int jj = 0; jj < PM_BT; ++jj) {
    if (jj < nb) {                                                          // uniform
      float s[H], cc[H];
      pm_row<H>(a.grid, j0 + jj, s, cc);
      float pS = 0.f, pU = 0.f;
#pragma unroll
      for (int q = 0; q < G; ++q) {
        const float etaS = vc_dm_eta_S<H>(an[q], e0[q], s, cc);
        if (doS) pS += pw_lik<NOISE>(kS[q], etaS, r[q], rl2[q]);
        if (VEL && doU) {
          const float etaU = vc_dm_eta_U<H>(an[q], etaS, lb2[q], gam[q], oml[jj], s, cc);
          pU += pw_lik<NOISE>(kU[q], etaU, r[q], rl2[q]);
        }
      }
      if (doS) accS[jj] += (double)pS;
      if (VEL && doU) accU[jj] += (double)pU;
    }
  }
}

// this wave's genes [g_lo, g_hi) under draw dr for one tile
template <int H, bool VEL, int NOISE, bool U16>
__device__ __forceinline__ void pm_genes(const VcPmArgs& a, int dr, int g_lo, int g_hi, int c, int pos, float cf, bool doS, bool doU, int j0,
                                         int nb, const float (&oml)[PM_BT], double (&accS)[PM_BT], double (&accU)[PM_BT]) {
  int g = g_lo;
#pragma unroll 1
  for (; g + PM_GC <= g_hi; g += PM_GC) pm_chunk<H, VEL, NOISE, U16, PM_GC>(a, dr, g, c, pos, cf, doS, doU, j0, nb, oml, accS, accU);
#pragma unroll 1
  for (; g < g_hi; ++g) pm_chunk<H, VEL, NOISE, U16, 1>(a, dr, g, c, pos, cf, doS, doU, j0, nb, oml, accS, accU);
}

template <int H, bool VEL, int NOISE, bool U16>
__global__ __launch_bounds__(PM_NW * 64) void vc_phase_marginal_kernel(const VcPmArgs a) {
  constexpr int NM = VEL ? 2 : 1;
  __shared__ pm_part_t part[PM_NW - 1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cl = (int)blockIdx.x * 64 + lane;                               // cell of the launch: the workspace column
  const int c_raw = a.c_begin + cl;
  const bool live = c_raw < a.c_end;
  const int c = live ? c_raw : a.c_end - 1;                                 // idle lanes of the last block re-read the last cell, store nothing
  const int pos = a.cell_pos ? a.cell_pos[c] : c;
  const float cf = a.cf[c];
  const int B = a.n_bins, D = a.n_draws;
  const bool s_once = a.s_once != 0;
  // gene share of this wave: whole chunks, contiguous
  const int chunks = (a.Ng + PM_GC - 1) / PM_GC;
  const int per = (chunks + PM_NW - 1) / PM_NW * PM_GC;
  const int g_lo = per * wave < a.Ng ? per * wave : a.Ng;
  const int g_hi = g_lo + per < a.Ng ? g_lo + per : a.Ng;

  double accS[PM_BT], accU[PM_BT], sj[PM_BT];
  float oml[PM_BT];
#pragma unroll
  for (int jj = 0; jj < PM_BT; ++jj) { accS[jj] = 0.0; accU[jj] = 0.0; sj[jj] = 0.0; oml[jj] = 0.f; }

  // the lgamma constants of the cell's elements, once: slot 0 of the combine carries the sum
#pragma unroll 1
  for (int g = g_lo; g < g_hi; ++g) {
    const size_t idx = vc_dm_count_index((size_t)(g / a.gbw), a.Nc, pos, a.gbw, (size_t)(g % a.gbw));
    accS[0] += pw_const(a, 0, g, vc_dm_count<U16>(a.S, idx));
    if (VEL) accS[0] += pw_const(a, NM - 1, g, vc_dm_count<U16>(a.U, idx));
  }
  pm_combine(accS, part, wave, lane);
  const double cst = accS[0];
  const double lw_flat = (double)a.lw_flat;

#pragma unroll 1
  for (int j0 = 0; j0 < B; j0 += PM_BT) {
    const int nb = B - j0 < PM_BT ? B - j0 : PM_BT;
    double M = 0.0;
    // pass -1 (s_once only): the spliced sums of the tile, once, under draw 0; passes 0 .. D-1: the draws.  One call site of the gene
    // loop serves both, so that the S sums are the work of the same instructions whether they are formed once or per draw
#pragma unroll 1
    for (int it = s_once ? -1 : 0; it < D; ++it) {
      const bool pre = it < 0;
      const int dr = pre ? 0 : it;
      const bool doS = pre || !s_once, doU = VEL && !pre;
      if (VEL && !pre && (dr == 0 || a.nw_ds != 0)) {
        const float* nw = a.nuomega + (size_t)dr * a.nw_ds;
#pragma unroll
        for (int jj = 0; jj < PM_BT; ++jj) {
          if (jj < nb) {
            float sk[VC_MAXH], ck[VC_MAXH];
            const float* row = a.grid + 8 * (size_t)(j0 + jj);
#pragma unroll
            for (int k = 0; k < VC_MAXH; ++k) { sk[k] = row[k]; ck[k] = row[VC_MAXH + k]; }
            oml[jj] = vc_dm_omega_l2(nw, a.Dm, a.Nx, a.Hw, a.Nc, c, sk, ck);
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < PM_BT; ++jj) {
        if (doS) accS[jj] = 0.0;
        accU[jj] = 0.0;
      }
      if (doS || doU) pm_genes<H, VEL, NOISE, U16>(a, dr, g_lo, g_hi, c, pos, cf, doS, doU, j0, nb, oml, accS, accU);
      if (doS) pm_combine(accS, part, wave, lane);
      if (doU) pm_combine(accU, part, wave, lane);
      if (pre) continue;
      if (wave == 0) {
        // a of the tile's bins under this draw, relative to their maximum
        double av[PM_BT], mt = 0.0;
#pragma unroll
        for (int jj = 0; jj < PM_BT; ++jj) {
          av[jj] = 0.0;
          if (jj < nb) {
            const double lw = a.log_prior ? (double)a.log_prior[(size_t)c * B + j0 + jj] : lw_flat;
            av[jj] = ((accS[jj] + accU[jj]) * PM_LN2 + cst) + lw;
            mt = (jj == 0 || av[jj] > mt) ? av[jj] : mt;
          }
        }
        if (dr == 0) {
          M = mt;
        } else if (mt > M) {
          const double down = exp(M - mt);
#pragma unroll
          for (int jj = 0; jj < PM_BT; ++jj) sj[jj] *= down;
          M = mt;
        }
        const double w = exp(mt - M);
        double dsum = 0.0;
#pragma unroll
        for (int jj = 0; jj < PM_BT; ++jj) {
          if (dr == 0) sj[jj] = 0.0;
          if (jj < nb) {
            const double e = exp(av[jj] - mt);
            dsum += e;
            sj[jj] += e * w;
          }
        }
        if (a.per_draw && live) {
          double* p = a.per_draw + (size_t)dr * a.Nc + c;
          const double tl = mt + log(dsum);
          if (j0 == 0) {
            *p = tl;
          } else {
            const double o = *p;
            const double hi = o > tl ? o : tl, lo = o > tl ? tl : o;
            *p = hi + log1p(exp(lo - hi));
          }
        }
      }
    }
    if (wave == 0 && live) {
#pragma unroll
      for (int jj = 0; jj < PM_BT; ++jj)
        if (jj < nb) a.ws[(size_t)(j0 + jj) * a.ws_ld + cl] = M + log(sj[jj]);          // (-inf where every draw's term underflowed)
    }
  }
  // behind the last tile: this lane's own stores read back
  if (wave == 0 && live) {
    double mx = a.ws[cl];
    for (int j = 1; j < B; ++j) {
      const double b = a.ws[(size_t)j * a.ws_ld + cl];
      mx = b > mx ? b : mx;
    }
    double sum = 0.0;
    for (int j = 0; j < B; ++j) sum += exp(a.ws[(size_t)j * a.ws_ld + cl] - mx);
    const double tot = mx + log(sum);
    a.evidence[c] = tot - log((double)D);
    if (a.post)
      for (int j = 0; j < B; ++j) a.post[(size_t)c * B + j] = (float)exp(a.ws[(size_t)j * a.ws_ld + cl] - tot);
  }
}

typedef void (*pm_kernel_t)(const VcPmArgs);

template <int H, bool VEL, int NOISE>
pm_kernel_t pm_pick3(bool u16) {
  return u16 ? (pm_kernel_t)vc_phase_marginal_kernel<H, VEL, NOISE, true> : (pm_kernel_t)vc_phase_marginal_kernel<H, VEL, NOISE, false>;
}
template <int H, bool VEL>
pm_kernel_t pm_pick2(int noise, bool u16) {
  return noise == VC_NOISE_NB ? pm_pick3<H, VEL, VC_NOISE_NB>(u16) : pm_pick3<H, VEL, VC_NOISE_POISSON>(u16);
}
template <int H>
pm_kernel_t pm_pick1(bool vel, int noise, bool u16) {
  return vel ? pm_pick2<H, true>(noise, u16) : pm_pick2<H, false>(noise, u16);
}

}  // namespace

int vc_launch_phase_marginal(const VcPmArgs& a, int H, bool vel, int noise, hipStream_t st) {
  pm_kernel_t k = H == 1 ? pm_pick1<1>(vel, noise, a.c16 != 0) : (H == 2 ? pm_pick1<2>(vel, noise, a.c16 != 0) : (H == 3 ? pm_pick1<3>(vel, noise, a.c16 != 0) : nullptr));
  if (!k || a.n_bins < 2 || a.n_bins > VC_PM_MAX_BINS || a.c_end <= a.c_begin) return VC_ERR_UNSUPPORTED;
  const unsigned n_super = (unsigned)((a.c_end - a.c_begin + 63) / 64);
  if ((long long)n_super * 64 > a.ws_ld) return VC_ERR_UNSUPPORTED;            // the workspace holds a column per lane of the launch
  hipLaunchKernelGGL(k, dim3(n_super), dim3(PM_NW * 64), 0, st, a);
  return VC_OK;
}
