// The two device passes behind the PCA phase prior (Phases.from_pca_heuristic(device=...), velocycle_amd/phase_prior.py; reference
// velocycle/phases.py:307-382): vc_pca_stage and vc_pca_apply of include/velocycle_hip.h.  Stand-alone: no engine.
//
// vc_pca_stage   X[c][g] = float32(log(v[c][g] + small_count)) for a range of cells (ocml's logf: correct to 1 ulp; once per element),
//                and the float64 column sums of X: one partial per (64-cell tile, gene) summed in cell order, folded into the running
//                sums in tile order -- the sums do not depend on how the cells are cut into calls (cuts at multiples of 64).
// vc_pca_apply   Y = (X - mu) Q  [Nc][8] float32   and   Z = (X - mu)^T Y  [Ng][8] float64   in ONE read of X from memory:
//                the block power iteration's only large operation.
//
// Mapping of vc_pca_apply.  Persistent workgroups of 8 waves (at most PCA_MAX_WG), each walking a contiguous range of 64-cell tiles.
//   Phase A of a tile: a wave owns 8 cells; lane = gene within a 64-gene block (a row segment is one coalesced load); per gene block
//     the lane forms x - mu for its 8 cells and adds x q[k] into 8 x 8 accumulators (Q's row of the lane's gene: two 16-byte loads,
//     shared by the 8 cells).  The 64 accumulators are then reduced over the lanes TOGETHER: a butterfly in which at distance s a lane
//     keeps half of its values and hands the other half to lane ^ s (32 + 16 + ... + 1 = 63 exchanges instead of 64 x 6); lane l ends
//     with the total of (cell l / 8, column l % 8), stores it to Y (256 contiguous bytes per wave) and into the tile's Y in the LDS.
//   Phase B: the genes are dealt out in groups of 2 048 (8 waves x 4 blocks x 64 lanes); a lane keeps 4 x 8 float32 accumulators of
//     Z, walks the cells of the tile (y[c][0..8) is wave-uniform: a broadcast read of the LDS) and re-reads its row segments, which
//     phase A has just pulled through the caches: X comes from memory once per call.  With one group (Ng <= 2 048) the accumulators
//     stay on chip over all the workgroup's tiles (in registers during phase B, in the LDS during phase A, whose 64 sums need the
//     registers: 128 VGPRs = 2 workgroups per CU); with more groups they are parked in the workgroup's own partial row between tiles.
//   Each workgroup stores ONE float32 partial row [Ng][8]; vc_pca_fold_kernel adds the rows in workgroup order in float64.
// No atomics, a fixed order of every sum: bit-identical on repetition.  Workspace: workgroups x Ng x 8 floats.  No scratch.
#include <string>

#include "vc_common.h"

void vc_set_global_error(const char* msg);      // vc_engine.hip: the message vc_last_error(NULL) returns

// every product-sum is written as the fma it is meant to be
#pragma clang fp contract(off)

namespace {

constexpr int PCA_K = 8;                 // block size of the power iteration
constexpr int PCA_NW = 8;                // waves per workgroup
constexpr int PCA_TILE = 64;             // cells per tile (= PCA_NW waves x PCA_CW cells)
constexpr int PCA_CW = 8;                // cells per wave in phase A
constexpr int PCA_NB = 4;                // gene blocks per wave and group in phase B
constexpr int PCA_GROUP = PCA_NW * PCA_NB * 64;
constexpr int PCA_MAX_WG = 512;
constexpr int PCA_CU = 2;                // cells whose row segments phase B requests together

__global__ __launch_bounds__(256) void vc_pca_stage_kernel(const float* __restrict__ raw, long long n, long long Ng, long long raw_stride,
                                                           float small, float* __restrict__ X, long long x_stride,
                                                           double* __restrict__ partial, int* __restrict__ flag) {
  const long long g = (long long)blockIdx.y * 256 + threadIdx.x;
  const long long t = blockIdx.x;
  if (g >= Ng) return;
  const long long c_lo = t * 64, c_hi = c_lo + 64 < n ? c_lo + 64 : n;
  double s = 0.0;
  bool bad = false;
  for (long long c = c_lo; c < c_hi; ++c) {
    const float x = logf(raw[c * raw_stride + g] + small);
    bad |= !(fabsf(x) <= 3.0e38f);                                 // -inf (v + small == 0), NaN (v + small < 0, NaN), +inf
    X[c * x_stride + g] = x;
    s += (double)x;
  }
  partial[t * Ng + g] = s;
  if (bad) *flag = 1;
}

__global__ __launch_bounds__(256) void vc_pca_colsum_kernel(const double* __restrict__ partial, long long tiles, long long Ng,
                                                            double* __restrict__ colsum) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= Ng) return;
  double s = colsum[g];
  for (long long t = 0; t < tiles; ++t) s += partial[t * Ng + g];
  colsum[g] = s;
}

// phase B for U consecutive cells: all U x PCA_NB row segments are requested before the first is used; per accumulator the cells
// are still added in ascending order
template <int U>
__device__ __forceinline__ void pca_cells(const float* __restrict__ xrow, long long stride, const unsigned (&gcl)[PCA_NB],
                                          const float (&m)[PCA_NB], const float* ytile_c, float (&zacc)[PCA_NB][PCA_K]) {
  float x[U][PCA_NB];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < PCA_NB; ++j) x[u][j] = (xrow + u * stride)[gcl[j]];        // uniform row address + 32-bit lane offset
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float4 ya = *(const float4*)(ytile_c + u * PCA_K), yb = *(const float4*)(ytile_c + u * PCA_K + 4);
    const float y[PCA_K] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
#pragma unroll
    for (int j = 0; j < PCA_NB; ++j) {
      const float xc = x[u][j] - m[j];
#pragma unroll
      for (int k = 0; k < PCA_K; ++k) zacc[j][k] = __builtin_fmaf(xc, y[k], zacc[j][k]);
    }
  }
}

__global__ __launch_bounds__(PCA_NW * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void vc_pca_apply_kernel(const float* __restrict__ X, long long Nc, long long Ng, long long stride,
                                                                   const float* __restrict__ mu, const float* __restrict__ Q,
                                                                   float* __restrict__ Y, float* __restrict__ ws, long long tiles,
                                                                   long long tiles_per_wg) {
  __shared__ __attribute__((aligned(16))) float ytile[PCA_TILE][PCA_K];
  __shared__ float zpark[PCA_NB * PCA_K][PCA_NW * 64];              // one group: Z's accumulators rest here during phase A (64 KiB)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long t_lo = (long long)blockIdx.x * tiles_per_wg;
  const long long t_hi = t_lo + tiles_per_wg < tiles ? t_lo + tiles_per_wg : tiles;
  const long long groups = (Ng + PCA_GROUP - 1) / PCA_GROUP;
  float* __restrict__ wrow = ws + (long long)blockIdx.x * Ng * PCA_K;

  float zacc[PCA_NB][PCA_K];
  for (long long t = t_lo; t < t_hi; ++t) {
    const long long c0 = t * PCA_TILE;
    const int ncell = (int)(Nc - c0 < PCA_TILE ? Nc - c0 : PCA_TILE);
    // ---- phase A: Y of this wave's 8 cells
    {
      const float* xr[PCA_CW];
#pragma unroll
      for (int i = 0; i < PCA_CW; ++i) {
        const long long c = c0 + wave * PCA_CW + i;
        xr[i] = X + (c < Nc ? c : Nc - 1) * stride;                // cells past the end re-read the last one; nothing of them is stored
      }
      float acc[PCA_CW * PCA_K];
#pragma unroll
      for (int i = 0; i < PCA_CW * PCA_K; ++i) acc[i] = 0.f;
      for (long long g0 = 0; g0 < Ng; g0 += 64) {
        const long long g = g0 + lane;
        const bool live = g < Ng;
        const long long gc = live ? g : Ng - 1;
        const float m = mu[gc];
        const float4 qa = *(const float4*)(Q + gc * PCA_K), qb = *(const float4*)(Q + gc * PCA_K + 4);
        float q[PCA_K] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
        for (int k = 0; k < PCA_K; ++k) q[k] = live ? q[k] : 0.f;
        float x[PCA_CW];
#pragma unroll
        for (int i = 0; i < PCA_CW; ++i) x[i] = xr[i][gc];
#pragma unroll
        for (int i = 0; i < PCA_CW; ++i) {
          const float xc = x[i] - m;
#pragma unroll
          for (int k = 0; k < PCA_K; ++k) acc[i * PCA_K + k] = __builtin_fmaf(xc, q[k], acc[i * PCA_K + k]);
        }
      }
      // all 64 sums over the lanes at once: at distance s a lane with bit s set keeps the upper half of its values
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) {
        const bool up = (lane & s) != 0;
#pragma unroll
        for (int i = 0; i < s; ++i) {
          const float send = up ? acc[i] : acc[i + s];
          const float keep = up ? acc[i + s] : acc[i];
          acc[i] = keep + __shfl_xor(send, s, 64);
        }
      }
      const int cl = wave * PCA_CW + (lane >> 3);                    // lane l holds (cell l / 8, column l % 8)
      ytile[cl][lane & 7] = acc[0];
      if (c0 + cl < Nc) Y[(c0 + cl) * PCA_K + (lane & 7)] = acc[0];
    }
    __syncthreads();
    // ---- phase B: Z of this workgroup's cells, gene group by gene group
    for (long long gr = 0; gr < groups; ++gr) {
      // (what phase B derives from the lane number is formed here, per tile, behind a value the compiler cannot see through: hoisted
      // out of the tile loop it would sit in registers that phase A's 64 sums need, and be spilled)
      int lane_b = lane;
      asm volatile("" : "+v"(lane_b));
      const long long gbase = gr * PCA_GROUP + (long long)wave * 64 + lane_b;        // block j of this wave: + j * PCA_NW * 64
      const long long left = Ng - (gr * PCA_GROUP + (long long)wave * 64);           // uniform: genes from this wave's first block on
      const int nb = left <= 0 ? 0 : (int)((left + PCA_NW * 64 - 1) / (PCA_NW * 64) < PCA_NB ? (left + PCA_NW * 64 - 1) / (PCA_NW * 64) : PCA_NB);
      unsigned gcl[PCA_NB];                                          // (Ng < 2^31: checked at the entry point)
      float m[PCA_NB];
#pragma unroll
      for (int j = 0; j < PCA_NB; ++j) {
        const long long g = gbase + (long long)j * PCA_NW * 64;
        gcl[j] = (unsigned)(g < Ng ? g : Ng - 1);
        m[j] = mu[gcl[j]];
      }
      if (groups == 1 && t != t_lo) {
#pragma unroll
        for (int j = 0; j < PCA_NB; ++j)
#pragma unroll
          for (int k = 0; k < PCA_K; ++k) zacc[j][k] = zpark[j * PCA_K + k][threadIdx.x];
      } else {
#pragma unroll
        for (int j = 0; j < PCA_NB; ++j) {
          if (t == t_lo) {
#pragma unroll
            for (int k = 0; k < PCA_K; ++k) zacc[j][k] = 0.f;
          } else {
            const float4 a = *(const float4*)(wrow + (long long)gcl[j] * PCA_K), b = *(const float4*)(wrow + (long long)gcl[j] * PCA_K + 4);
            zacc[j][0] = a.x; zacc[j][1] = a.y; zacc[j][2] = a.z; zacc[j][3] = a.w;
            zacc[j][4] = b.x; zacc[j][5] = b.y; zacc[j][6] = b.z; zacc[j][7] = b.w;
          }
        }
      }
      // blocks past the end (j >= nb) load the last gene again and sum what is never stored: no branch between a load and its use
      if (nb > 0) {
        const float* xrow = X + c0 * stride;
        int c = 0;
        for (; c + PCA_CU <= ncell; c += PCA_CU, xrow += PCA_CU * stride) pca_cells<PCA_CU>(xrow, stride, gcl, m, &ytile[c][0], zacc);
        for (; c < ncell; ++c, xrow += stride) pca_cells<1>(xrow, stride, gcl, m, &ytile[c][0], zacc);
      }
      if (groups > 1 || t == t_hi - 1) {
#pragma unroll
        for (int j = 0; j < PCA_NB; ++j) {
          const long long g = gbase + (long long)j * PCA_NW * 64;
          if (g < Ng) {
            *(float4*)(wrow + g * PCA_K) = make_float4(zacc[j][0], zacc[j][1], zacc[j][2], zacc[j][3]);
            *(float4*)(wrow + g * PCA_K + 4) = make_float4(zacc[j][4], zacc[j][5], zacc[j][6], zacc[j][7]);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < PCA_NB; ++j)
#pragma unroll
          for (int k = 0; k < PCA_K; ++k) zpark[j * PCA_K + k][threadIdx.x] = zacc[j][k];      // this thread's own slots: no barrier
      }
    }
    __syncthreads();                                                 // the next tile's phase A overwrites ytile
  }
}

__global__ __launch_bounds__(256) void vc_pca_fold_kernel(const float* __restrict__ ws, long long rows, long long n, double* __restrict__ Z) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (long long w = 0; w < rows; ++w) s += (double)ws[w * n + i];
  Z[i] = s;
}

int pca_fail(int code, const char* msg) {
  vc_set_global_error(msg);
  return code;
}

int pca_launched(const char* what) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return VC_OK;
  try { vc_set_global_error((std::string(what) + ": launch failed: " + hipGetErrorString(err)).c_str()); } catch (...) {}
  return VC_ERR_HIP;
}

void pca_grid(int64_t Nc, int max_workgroups, long long* tiles, long long* per, long long* wgs) {
  const long long cap = max_workgroups >= 1 && max_workgroups < PCA_MAX_WG ? max_workgroups : PCA_MAX_WG;
  *tiles = (Nc + PCA_TILE - 1) / PCA_TILE;
  *per = (*tiles + cap - 1) / cap;
  *wgs = (*tiles + *per - 1) / *per;
}

}  // namespace

extern "C" int64_t vc_pca_apply_workspace(int64_t Nc, int64_t Ng, int max_workgroups) {
  if (Nc < 1 || Ng < 1) return 0;
  long long tiles, per, wgs;
  pca_grid(Nc, max_workgroups, &tiles, &per, &wgs);
  return (int64_t)(wgs * Ng * PCA_K);
}

extern "C" int vc_pca_stage(const float* raw_dev, int64_t n_cells, int64_t Ng, int64_t raw_stride, float small_count, float* X_dev,
                            int64_t x_stride, double* colsum_dev, double* partial_dev, int32_t* flag_dev, void* hip_stream) {
  if (n_cells < 1 || Ng < 1) return pca_fail(VC_ERR_ARG, "vc_pca_stage: n_cells and Ng must be >= 1");
  if (raw_stride < Ng || x_stride < Ng) return pca_fail(VC_ERR_ARG, "vc_pca_stage: a row stride < Ng");
  if (!raw_dev || !X_dev || !colsum_dev || !partial_dev || !flag_dev) return pca_fail(VC_ERR_ARG, "vc_pca_stage: null pointer");
  const long long tiles = (n_cells + 63) / 64;
  if (tiles > 0x7fffffffLL) return pca_fail(VC_ERR_ARG, "vc_pca_stage: more than 2^37 cells in one call");
  if ((Ng + 255) / 256 > 65535) return pca_fail(VC_ERR_ARG, "vc_pca_stage: more than 65535 x 256 genes");
  hipStream_t st = (hipStream_t)hip_stream;
  const unsigned gx = (unsigned)((Ng + 255) / 256);
  hipLaunchKernelGGL(vc_pca_stage_kernel, dim3((unsigned)tiles, gx), dim3(256), 0, st, raw_dev, (long long)n_cells, (long long)Ng,
                     (long long)raw_stride, small_count, X_dev, (long long)x_stride, partial_dev, (int*)flag_dev);
  hipLaunchKernelGGL(vc_pca_colsum_kernel, dim3(gx), dim3(256), 0, st, (const double*)partial_dev, tiles, (long long)Ng, colsum_dev);
  return pca_launched("vc_pca_stage");
}

extern "C" int vc_pca_apply(const float* X_dev, int64_t Nc, int64_t Ng, int64_t x_stride, const float* mu_dev, const float* Q_dev,
                            float* Y_dev, double* Z_dev, float* ws_dev, int64_t ws_floats, int max_workgroups, void* hip_stream) {
  if (Nc < 1 || Ng < 1) return pca_fail(VC_ERR_ARG, "vc_pca_apply: Nc and Ng must be >= 1");
  if (x_stride < Ng) return pca_fail(VC_ERR_ARG, "vc_pca_apply: x_stride < Ng");
  if (!X_dev || !mu_dev || !Q_dev || !Y_dev || !Z_dev || !ws_dev) return pca_fail(VC_ERR_ARG, "vc_pca_apply: null pointer");
  if ((((uintptr_t)Q_dev) | ((uintptr_t)ws_dev)) & 15) return pca_fail(VC_ERR_ARG, "vc_pca_apply: Q_dev and ws_dev must be 16-byte aligned");
  long long tiles, per, wgs;
  pca_grid(Nc, max_workgroups, &tiles, &per, &wgs);
  if (ws_floats < wgs * Ng * PCA_K) return pca_fail(VC_ERR_ARG, "vc_pca_apply: workspace smaller than vc_pca_apply_workspace(Nc, Ng, max_workgroups) floats");
  if (Ng > 0x0fffffffLL) return pca_fail(VC_ERR_ARG, "vc_pca_apply: more than 2^28 genes");
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(vc_pca_apply_kernel, dim3((unsigned)wgs), dim3(PCA_NW * 64), 0, st, X_dev, (long long)Nc, (long long)Ng,
                     (long long)x_stride, mu_dev, Q_dev, Y_dev, ws_dev, tiles, per);
  const long long n = Ng * PCA_K;
  hipLaunchKernelGGL(vc_pca_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)ws_dev, wgs, n, Z_dev);
  return pca_launched("vc_pca_apply");
}
