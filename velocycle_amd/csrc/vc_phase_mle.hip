// Maximum-likelihood phase assignment on a grid of bins: vc_phase_mle of include/velocycle_hip.h, the counterpart of the
// reference's Phases.from_cycle_mle (velocycle/phases.py:471-509).  Stand-alone: no engine, no workspace, one launch.
//
// Per cell c and bin j the kernel sums over the genes the part of log p(k_gc | bin j) that depends on the bin, written so that every
// term has the size of the log-probability itself and not of its large cancelling parts (mu = E[j,g] m_c, E = exp T):
//   negative binomial   k d - r w,   d = ln(mu / (r + mu)) = T[j,g] - ln(E[j,g] + r_g / m_c)         (<= 0)
//                                    w = ln((r + mu) / r)  = ln(E[j,g] + r_g / m_c) - ln(r_g / m_c)  (>= 0)
//   Poisson             k d - v,     d = ln(mu / max(k, 1)) = T[j,g] + ln(m_c / max(k, 1)),   v = mu - k
// (the differences to the full log p -- lgamma terms, k ln max(k,1) - k -- do not depend on the bin).  One v_log_f32 per element
// for the negative binomial, none for Poisson; no lgamma anywhere.
//
// Mapping: lane = cell, a wave owns 64 consecutive cells, the NW waves of a workgroup split the genes.  A workgroup walks the bins
// in tiles of BT; per tile every lane holds BT float64 accumulators (2 BT VGPRs).  Inside a tile a wave takes GC genes at a time:
// it loads their counts (64 consecutive cells of one gene row: coalesced), forms the per-(gene, cell) constants once, and for every
// bin of the tile sums the GC terms in float32 and adds that short sum to the bin's float64 accumulator -- the float32 running sums
// never grow beyond GC terms, so the result carries the rounding of the terms, not of a 2 000-term float32 sum.  T[j, g..g+GC) and
// E[j, g..g+GC) are wave-uniform and read through the constant address space (scalar loads, as vc_main_math.h reads its cell record).
// The waves' float64 partials are combined through the LDS in the fixed order wave 0, 1, ..., NW-1 (no atomics: bit-reproducible);
// wave 0 keeps the running maximum (strict >, ascending bins: the FIRST of equal bins wins, like torch.argmax) and writes the outputs
// with ordinary vector stores.  The count block is re-read per bin tile (from L2 / HBM): the kernel is bound by the logarithms.
#include <string>

#include "vc_common.h"

void vc_set_global_error(const char* msg);      // vc_engine.hip: the message vc_last_error(NULL) returns

// Every product-sum below is written as the fma it is meant to be; nothing else may be contracted.  The full-tile and the
// ragged-tile instantiations of a chunk then perform the same operations, and equal table rows give equal bits wherever they stand.
#pragma clang fp contract(off)

namespace {

constexpr int MLE_NW = 4;        // waves per workgroup (= gene shares)
constexpr int MLE_BT = 32;       // bins per tile
constexpr int MLE_GC = 8;        // genes per chunk (two s_load_dwordx8 per bin and chunk)
constexpr int MLE_MAX_BINS = 4096;

typedef const __attribute__((address_space(4))) float* mle_cptr;

template <bool U16>
__device__ __forceinline__ float mle_count(const void* counts, long long row, long long c) {
  if (U16) return (float)((const unsigned short*)counts)[row + c];
  return ((const float*)counts)[row + c];
}

// One chunk of G genes [g, g + G) for the bins [j0, j0 + nb) of a tile: acc[jj] += sum_q term(j0 + jj, g + q)
template <int NOISE, bool U16, int G, bool FULL>
__device__ __forceinline__ void mle_chunk(const void* __restrict__ counts, long long gene_stride, long long c, long long Ng, long long g,
                                          mle_cptr T, mle_cptr E, const float* __restrict__ r, float m, float im, float nln2, int j0, int nb,
                                          double (&acc)[MLE_BT]) {
  float k[G], a[G], b[G], nr[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    k[q] = mle_count<U16>(counts, (g + q) * gene_stride, c);
    if (NOISE == VC_NOISE_NB) {
      const float rq = r[g + q];                                   // wave-uniform
      a[q] = rq * im;                                              // r / m
      b[q] = VC_LN2 * __builtin_amdgcn_logf(a[q]);                 // ln(r / m)
      nr[q] = -rq;
    } else {
      const float k1 = fmaxf(k[q], 1.f);
      a[q] = VC_LN2 * __builtin_amdgcn_logf(m * __builtin_amdgcn_rcpf(k1));     // ln(m / max(k, 1))
      b[q] = k[q];
    }
  }
  // T / E of the next bin are fetched (scalar loads into SGPRs) while the current bin computes; the scheduling barrier keeps the
  // compiler from hoisting the loads of all BT bins to the top (16 SGPRs per bin: it would spill them through v_writelane)
  // (running row pointers, opaque to the compiler: otherwise it keeps the BT row offsets of a tile as loop invariants in SGPRs it has not got)
  float tt[2][G], ee[2][G];
  mle_cptr tp = T + ((long long)j0 * Ng + g), ep = E + ((long long)j0 * Ng + g);
#pragma unroll
  for (int q = 0; q < G; ++q) { tt[0][q] = tp[q]; ee[0][q] = ep[q]; }
#pragma unroll
  for (int jj = 0; jj < MLE_BT; ++jj) {
    if (FULL || jj < nb) {                                         // uniform; FULL: a whole tile, no tests
      const float(&tc)[G] = tt[jj & 1];
      const float(&ec)[G] = ee[jj & 1];
      if (jj + 1 < (FULL ? MLE_BT : nb)) {
        tp += Ng;
        ep += Ng;
        asm volatile("" : "+s"(tp), "+s"(ep));
#pragma unroll
        for (int q = 0; q < G; ++q) { tt[(jj + 1) & 1][q] = tp[q]; ee[(jj + 1) & 1][q] = ep[q]; }
      }
      float p = 0.f;
#pragma unroll
      for (int q = 0; q < G; ++q) {
        if (NOISE == VC_NOISE_NB) {
          const float u2 = __builtin_amdgcn_logf(ec[q] + a[q]);    // log2(E + r / m)
          p = __builtin_fmaf(k[q], __builtin_fmaf(u2, nln2, tc[q]), p);          // d = T - ln(E + r / m)
          p = __builtin_fmaf(nr[q], __builtin_fmaf(u2, VC_LN2, -b[q]), p);       // w = ln(E + r / m) - ln(r / m)
        } else {
          p = __builtin_fmaf(k[q], tc[q] + a[q], p);
          p -= __builtin_fmaf(ec[q], m, -b[q]);
        }
      }
      acc[jj] += (double)p;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int NOISE, bool U16>
__global__ __launch_bounds__(MLE_NW * 64) void vc_phase_mle_kernel(const void* __restrict__ counts, long long Ng, long long Nc,
                                                                   long long gene_stride, const float* __restrict__ Tg,
                                                                   const float* __restrict__ Eg, int bins, const float* __restrict__ mg,
                                                                   const float* __restrict__ r, int* __restrict__ best_bin,
                                                                   float* __restrict__ logp_rel) {
  __shared__ double part[MLE_BT][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long c_raw = (long long)blockIdx.x * 64 + lane;
  const bool live = c_raw < Nc;
  const long long c = live ? c_raw : Nc - 1;                      // idle lanes of the last block re-read the last cell, store nothing
  mle_cptr T = (mle_cptr)(const void*)Tg;
  mle_cptr E = (mle_cptr)(const void*)Eg;
  const float m = mg[c];
  const float im = 1.f / m;
  // -ln 2 held in a VGPR: as a literal it would share the one constant slot of v_fma_f32 with the SGPR that holds T (a v_mov per element)
  float nln2;
  asm volatile("v_mov_b32 %0, 0xbf317218" : "=v"(nln2));
  // gene share of this wave: whole chunks, contiguous
  const long long chunks = (Ng + MLE_GC - 1) / MLE_GC;
  const long long per = (chunks + MLE_NW - 1) / MLE_NW * MLE_GC;
  const long long g_lo = per * wave < Ng ? per * wave : Ng;
  const long long g_hi = g_lo + per < Ng ? g_lo + per : Ng;

  double best = 0.0, base = 0.0;
  int best_j = 0;
  for (int j0 = 0; j0 < bins; j0 += MLE_BT) {
    const int nb = bins - j0 < MLE_BT ? bins - j0 : MLE_BT;
    double acc[MLE_BT];
#pragma unroll
    for (int jj = 0; jj < MLE_BT; ++jj) acc[jj] = 0.0;
    long long g = g_lo;
    if (nb == MLE_BT) {
      for (; g + MLE_GC <= g_hi; g += MLE_GC) mle_chunk<NOISE, U16, MLE_GC, true>(counts, gene_stride, c, Ng, g, T, E, r, m, im, nln2, j0, nb, acc);
    } else {
      for (; g + MLE_GC <= g_hi; g += MLE_GC) mle_chunk<NOISE, U16, MLE_GC, false>(counts, gene_stride, c, Ng, g, T, E, r, m, im, nln2, j0, nb, acc);
    }
    for (; g < g_hi; ++g) mle_chunk<NOISE, U16, 1, false>(counts, gene_stride, c, Ng, g, T, E, r, m, im, nln2, j0, nb, acc);
    // the waves' partials, added in wave order
#pragma unroll 1
    for (int w = 1; w < MLE_NW; ++w) {
      __syncthreads();
      if (wave == w) {
#pragma unroll
        for (int jj = 0; jj < MLE_BT; ++jj) part[jj][lane] = acc[jj];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int jj = 0; jj < MLE_BT; ++jj) acc[jj] += part[jj][lane];
      }
    }
    if (wave == 0) {
      if (j0 == 0) { best = acc[0]; base = acc[0]; }
#pragma unroll
      for (int jj = 0; jj < MLE_BT; ++jj) {
        if (jj < nb) {
          if (acc[jj] > best) { best = acc[jj]; best_j = j0 + jj; }
          // relative to bin 0 for now (small numbers keep their digits as floats); the maximum is taken off below
          if (logp_rel && live) logp_rel[(long long)(j0 + jj) * Nc + c] = (float)(acc[jj] - base);
        }
      }
    }
  }
  if (wave == 0 && live) {
    best_bin[c] = best_j;
    if (logp_rel) {
      const float top = (float)(best - base);
      for (int j = 0; j < bins; ++j) logp_rel[(long long)j * Nc + c] -= top;     // this lane's own stores: <= 0, exactly 0 at best_j
    }
  }
}

int mle_fail(int code, const char* msg) {
  vc_set_global_error(msg);
  return code;
}

}  // namespace

extern "C" int vc_phase_mle(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* T_dev,
                            const float* expT_dev, int bins, const float* m_dev, int noise, const float* r_dev, int32_t* best_bin_dev,
                            float* logp_rel_dev, void* hip_stream) {
  if (noise == VC_NOISE_LOGNORMAL) return mle_fail(VC_ERR_UNSUPPORTED, "vc_phase_mle: Lognormal noise is not implemented (Poisson or NegativeBinomial)");
  if (noise != VC_NOISE_NB && noise != VC_NOISE_POISSON) return mle_fail(VC_ERR_ARG, "vc_phase_mle: noise must be VC_NOISE_POISSON or VC_NOISE_NB");
  if (count_kind != VC_COUNTS_F32 && count_kind != VC_COUNTS_U16) return mle_fail(VC_ERR_ARG, "vc_phase_mle: count_kind must be VC_COUNTS_F32 or VC_COUNTS_U16");
  if (Ng < 1 || Nc < 1) return mle_fail(VC_ERR_ARG, "vc_phase_mle: Ng and Nc must be >= 1");
  if (bins < 1 || bins > MLE_MAX_BINS) return mle_fail(VC_ERR_ARG, "vc_phase_mle: bins must be in 1..4096");
  if (gene_stride < Nc) return mle_fail(VC_ERR_ARG, "vc_phase_mle: gene_stride < Nc");
  if (!counts_dev || !T_dev || !expT_dev || !m_dev || !best_bin_dev) return mle_fail(VC_ERR_ARG, "vc_phase_mle: null pointer");
  if (noise == VC_NOISE_NB && !r_dev) return mle_fail(VC_ERR_ARG, "vc_phase_mle: the negative binomial needs r_dev (1 / dispersion per gene)");
  if ((Nc + 63) / 64 > 0x7fffffffLL) return mle_fail(VC_ERR_ARG, "vc_phase_mle: more than 2^37 cells");
  const dim3 grid((unsigned)((Nc + 63) / 64)), block(MLE_NW * 64);
  hipStream_t st = (hipStream_t)hip_stream;
#define MLE_LAUNCH(NOISE, U16)                                                                                                         \
  hipLaunchKernelGGL((vc_phase_mle_kernel<NOISE, U16>), grid, block, 0, st, counts_dev, (long long)Ng, (long long)Nc,                    \
                     (long long)gene_stride, T_dev, expT_dev, bins, m_dev, r_dev, (int*)best_bin_dev, logp_rel_dev)
  const bool u16 = count_kind == VC_COUNTS_U16;
  if (noise == VC_NOISE_NB) { if (u16) MLE_LAUNCH(VC_NOISE_NB, true); else MLE_LAUNCH(VC_NOISE_NB, false); }
  else { if (u16) MLE_LAUNCH(VC_NOISE_POISSON, true); else MLE_LAUNCH(VC_NOISE_POISSON, false); }
#undef MLE_LAUNCH
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    try { vc_set_global_error((std::string("vc_phase_mle: launch failed: ") + hipGetErrorString(err)).c_str()); } catch (...) {}
    return VC_ERR_HIP;
  }
  return VC_OK;
}
