// Posterior predictive check: the kernels behind vc_predictive_check and vc_sample_counts of include/velocycle_hip.h.
// On the reference's stack this is Predictive with the observations removed (velocity_inference_model.py:338-386,
// phase_inference_model.py:343-395 define the likelihood the replicates are drawn from) and [D][Ng][Nc] count tensors per matrix;
// here every replicate k_rep[d, m, g, c] is drawn (vc_count_sampler.h), reduced to statistics and forgotten.
//
// Mapping.  Grid (64-cell blocks of the call's range, draws of the call's range); a workgroup owns ONE draw and 64 consecutive cells
// (in the caller's order), lane = cell.  A lane forms its cell's record once (sin / cos of k phi, omega, count factor); the
// PPC_NW waves deal out the genes (gene = wave + PPC_NW i: wave-uniform, its latents arrive through scalar loads).  eta_S / eta_U are
// the statements of vc_draw_model.h, the ones vc_pointwise.hip scores the observed counts with.
//
// Sums.  All replicate statistics are integers.  Per (gene, matrix) a wave reduces its 64 cells' k, k^2, [k = 0] and max k by
// xor-shuffles and lane 0 adds them to the [D][nmat][4][Ng] table with 64-bit integer atomics (atomicAdd / atomicMax): exact, so
// independent of the order and of how cells and draws are cut into calls.  The library size of a cell (sum over genes) is kept per
// lane, added over the waves through the LDS in wave order and stored by the one workgroup that owns (draw, cell).  No float atomics.
// The observed statistics come from the engine's own copy of the counts in a fixed order (vc_ppc_observed_*).
#include "vc_count_sampler.h"
#include "vc_draw_model.h"      // behind the sampler's `#pragma clang fp contract(off)`
#include <mutex>

void vc_set_global_error(const char* msg);      // vc_engine.hip: the message vc_last_error(NULL) returns

namespace {

constexpr int PPC_NW = 8;                   // waves per workgroup

typedef unsigned long long u64;

__device__ __forceinline__ u64 ppc_wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off, 64);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}
__device__ __forceinline__ unsigned ppc_wave_max(unsigned v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

template <int H, bool VEL, bool NB>
__global__ __launch_bounds__(PPC_NW * 64) void vc_ppc_kernel(const VcPpcArgs a) {
  constexpr int NM = VEL ? 2 : 1, NH = 2 * H + 1;
  __shared__ u64 cellacc[PPC_NW][NM][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int dr = a.d_begin + (int)blockIdx.y;                  // the draw of this workgroup
  const int c_raw = a.c_begin + (int)blockIdx.x * 64 + lane;
  const bool live = c_raw < a.c_end;
  const int c = live ? c_raw : a.c_end - 1;
  const uint64_t gcell = (uint64_t)(a.cell_offset + c);
  // the cell's record under draw dr
  float sk[VC_MAXH], ck[VC_MAXH], oml = 0.f;
  {
    const float* xy = a.phixy + (size_t)dr * a.phixy_ds + 2 * (size_t)c;
    vc_dm_basis(xy[0], xy[1], sk, ck);
    if (VEL) oml = vc_dm_omega_l2(a.nuomega + (size_t)dr * a.nw_ds, a.Dm, a.Nx, a.Hw, a.Nc, c, sk, ck);
  }
  const float cf = a.cf[c];
  u64 lib[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) lib[m] = 0;
  unsigned n_fail = 0;
  const bool keep = a.keep && dr < a.n_keep;
#pragma unroll 1
  for (int g = wave; g < a.Ng; g += PPC_NW) {
    float r = 0.f;
    if (NB) r = 1.f / a.shape_inv[g];
    const float e0 = vc_dm_e0(cf, a.Dbm, a.dnu, a.Nb, a.Nc, a.Ng, c, g);
    float an[NH], gam = 0.f, lb2 = 0.f;
    vc_dm_latents<H, VEL>(a.nu, a.nu_ds, a.loggamma, a.lg_ds, a.logbeta, a.lb_ds, dr, g, an, gam, lb2);
    float eta[NM];
    eta[0] = vc_dm_eta_S<H>(an, e0, sk, ck);
    if (VEL) eta[NM - 1] = vc_dm_eta_U<H>(an, eta[0], lb2, gam, oml, sk, ck);
    const uint64_t idx = ((uint64_t)g << 32) | gcell;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      int k = vc_cs_count(a.seed, idx, (uint32_t)dr, (uint32_t)m, eta[m], r, NB);
      if (k < 0) { n_fail += live ? 1u : 0u; k = 0; }
      const unsigned ku = live ? (unsigned)k : 0u;
      if (keep && live) a.keep[(((size_t)dr * NM + m) * a.Ng + g) * (size_t)a.Nc + c] = (int)ku;
      lib[m] += ku;
      const u64 s1 = ppc_wave_sum((u64)ku);
      const u64 s2 = ppc_wave_sum((u64)ku * (u64)ku);
      const u64 s0 = ppc_wave_sum((u64)((live && ku == 0u) ? 1u : 0u));
      const unsigned mx = ppc_wave_max(ku);
      if (lane == 0) {
        u64* row = a.gene_rep + (((size_t)dr * NM + m) * 4) * (size_t)a.Ng + g;
        atomicAdd(row, s1);
        atomicAdd(row + (size_t)a.Ng, s2);
        atomicAdd(row + 2 * (size_t)a.Ng, s0);
        atomicMax(row + 3 * (size_t)a.Ng, (u64)mx);
      }
    }
  }
  if (n_fail) atomicAdd(a.status, (u64)n_fail);
#pragma unroll
  for (int m = 0; m < NM; ++m) cellacc[wave][m][lane] = lib[m];
  __syncthreads();
  if (threadIdx.x < NM * 64) {
    const int m = threadIdx.x >> 6;
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < PPC_NW; ++w) s += cellacc[w][m][lane];
    if (live) a.cell_rep[((size_t)dr * NM + m) * (size_t)a.Nc + c] = s;
  }
}

// observed counts, per gene over the cells [c_begin, c_end) in the caller's order, continued from what gene_obs holds: one thread per
// (matrix, gene), a fixed order of float64 additions
template <bool U16>
__global__ __launch_bounds__(64) void vc_ppc_observed_gene_kernel(const VcPpcArgs a, int nmat) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= nmat * a.Ng) return;
  const int m = i / a.Ng, g = i % a.Ng;
  const void* src = m == 0 ? a.S : a.U;
  double* row = a.gene_obs + ((size_t)m * 4) * (size_t)a.Ng + g;
  double s1 = row[0], s2 = row[(size_t)a.Ng], s0 = row[2 * (size_t)a.Ng], mx = row[3 * (size_t)a.Ng];
  const size_t lay_blk = (size_t)(g / a.gbw), lay_in = (size_t)(g % a.gbw);
  for (int c = a.c_begin; c < a.c_end; ++c) {
    const int pos = a.cell_pos ? a.cell_pos[c] : c;
    const double k = (double)vc_dm_count<U16>(src, vc_dm_count_index(lay_blk, a.Nc, pos, a.gbw, lay_in));
    s1 += k;
    s2 += k * k;
    s0 += k == 0.0 ? 1.0 : 0.0;
    mx = k > mx ? k : mx;
  }
  row[0] = s1; row[(size_t)a.Ng] = s2; row[2 * (size_t)a.Ng] = s0; row[3 * (size_t)a.Ng] = mx;
}

// observed library size of every cell of the range: one thread per (matrix, cell), genes in ascending order
template <bool U16>
__global__ __launch_bounds__(64) void vc_ppc_observed_cell_kernel(const VcPpcArgs a, int nmat) {
  const int n = a.c_end - a.c_begin;
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= nmat * n) return;
  const int m = i / n, c = a.c_begin + i % n;
  const void* src = m == 0 ? a.S : a.U;
  const int pos = a.cell_pos ? a.cell_pos[c] : c;
  double s = 0.0;
  for (int g = 0; g < a.Ng; ++g)
    s += (double)vc_dm_count<U16>(src, vc_dm_count_index((size_t)(g / a.gbw), a.Nc, pos, a.gbw, (size_t)(g % a.gbw)));
  a.cell_obs[(size_t)m * a.Nc + c] = s;
}

// element (row i, column j) of eta[n_rows][n_cols]: Philox index origin + i row_stride + j; failures are stored as -1 and counted
template <bool NB>
__global__ __launch_bounds__(256) void vc_sample_counts_kernel(const float* __restrict__ eta, long long n_rows, long long n_cols,
                                                               const float* __restrict__ shape_inv, uint64_t seed, uint32_t draw,
                                                               uint32_t mat, uint64_t origin, uint64_t row_stride, int* __restrict__ out,
                                                               u64* status) {
  const long long n = n_rows * n_cols;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long row = i / n_cols, col = i - row * n_cols;
    const float r = NB ? 1.f / shape_inv[row] : 0.f;
    const int k = vc_cs_count(seed, origin + (uint64_t)row * row_stride + (uint64_t)col, draw, mat, eta[i] * VC_LOG2E, r, NB);
    out[i] = k;
    if (k < 0) atomicAdd(status, (u64)1);
  }
}

typedef void (*ppc_kernel_t)(const VcPpcArgs);
template <int H>
ppc_kernel_t ppc_pick(bool vel, bool nb) {
  if (vel) return nb ? (ppc_kernel_t)vc_ppc_kernel<H, true, true> : (ppc_kernel_t)vc_ppc_kernel<H, true, false>;
  return nb ? (ppc_kernel_t)vc_ppc_kernel<H, false, true> : (ppc_kernel_t)vc_ppc_kernel<H, false, false>;
}

int sc_fail(int code, const char* msg) {
  vc_set_global_error(msg);
  return code;
}

// vc_sample_counts has no engine to keep its failure counter in: one 8-byte device word per device, allocated on the first call
// there and kept for the life of the process (no hipMalloc / hipFree, which synchronises the whole device, per call).  sc_mutex
// serialises the calls, which wait for their own stream anyway.
constexpr int SC_MAX_DEVICES = 64;
std::mutex sc_mutex;
u64* sc_status_word[SC_MAX_DEVICES] = {};

u64* sc_status(void) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SC_MAX_DEVICES) return nullptr;
  if (!sc_status_word[dev] && hipMalloc((void**)&sc_status_word[dev], sizeof(u64)) != hipSuccess) sc_status_word[dev] = nullptr;
  return sc_status_word[dev];
}

}  // namespace

int vc_launch_ppc(const VcPpcArgs& a0, int H, bool vel, bool nb, int d_end, hipStream_t st) {
  ppc_kernel_t k = H == 1 ? ppc_pick<1>(vel, nb) : (H == 2 ? ppc_pick<2>(vel, nb) : (H == 3 ? ppc_pick<3>(vel, nb) : nullptr));
  if (!k) return VC_ERR_UNSUPPORTED;
  VcPpcArgs a = a0;
  const unsigned n_super = (unsigned)((a.c_end - a.c_begin + 63) / 64);
  for (int d0 = a0.d_begin; d0 < d_end; d0 += 32768) {        // (grid.y is limited to 65535)
    a.d_begin = d0;
    const int nd = d_end - d0 < 32768 ? d_end - d0 : 32768;
    hipLaunchKernelGGL(k, dim3(n_super, (unsigned)nd), dim3(PPC_NW * 64), 0, st, a);
  }
  return VC_OK;
}

void vc_launch_ppc_observed(const VcPpcArgs& a, int nmat, hipStream_t st) {
  const int ng = nmat * a.Ng, nc = nmat * (a.c_end - a.c_begin);
  if (a.c16) {
    hipLaunchKernelGGL(vc_ppc_observed_gene_kernel<true>, dim3((unsigned)((ng + 63) / 64)), dim3(64), 0, st, a, nmat);
    hipLaunchKernelGGL(vc_ppc_observed_cell_kernel<true>, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, st, a, nmat);
  } else {
    hipLaunchKernelGGL(vc_ppc_observed_gene_kernel<false>, dim3((unsigned)((ng + 63) / 64)), dim3(64), 0, st, a, nmat);
    hipLaunchKernelGGL(vc_ppc_observed_cell_kernel<false>, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, st, a, nmat);
  }
}

extern "C" int vc_sample_counts(const float* eta_dev, int64_t n_rows, int64_t n_cols, const float* shape_inv_dev, uint64_t seed,
                                int64_t draw, int matrix, int64_t index_origin, int64_t row_index_stride, int32_t* out_dev,
                                void* hip_stream) {
  if (!eta_dev || !out_dev) return sc_fail(VC_ERR_ARG, "vc_sample_counts: null eta_dev / out_dev");
  if (n_rows < 1 || n_cols < 1 || n_rows > (1LL << 40) / n_cols) return sc_fail(VC_ERR_ARG, "vc_sample_counts: n_rows and n_cols must be >= 1, at most 2^40 elements");
  if (draw < 0 || draw > 0xffffffffLL) return sc_fail(VC_ERR_ARG, "vc_sample_counts: draw must be in [0, 2^32)");
  if (matrix < 0 || matrix > 0xffff) return sc_fail(VC_ERR_ARG, "vc_sample_counts: matrix must be in [0, 65536)");
  if (index_origin < 0 || row_index_stride < 0) return sc_fail(VC_ERR_ARG, "vc_sample_counts: negative index_origin / row_index_stride");
  hipStream_t st = (hipStream_t)hip_stream;
  std::lock_guard<std::mutex> lock(sc_mutex);
  u64* status = sc_status();
  if (!status) return sc_fail(VC_ERR_HIP, "vc_sample_counts: no device, or hipMalloc of the status word failed");
  hipError_t err = hipMemsetAsync(status, 0, sizeof(u64), st);
  const long long n = n_rows * n_cols;
  const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 1 << 16);
  if (err == hipSuccess) {
    if (shape_inv_dev)
      hipLaunchKernelGGL(vc_sample_counts_kernel<true>, dim3(grid), dim3(256), 0, st, eta_dev, (long long)n_rows, (long long)n_cols, shape_inv_dev,
                         seed, (uint32_t)draw, (uint32_t)matrix, (uint64_t)index_origin, (uint64_t)row_index_stride, (int*)out_dev, status);
    else
      hipLaunchKernelGGL(vc_sample_counts_kernel<false>, dim3(grid), dim3(256), 0, st, eta_dev, (long long)n_rows, (long long)n_cols, shape_inv_dev,
                         seed, (uint32_t)draw, (uint32_t)matrix, (uint64_t)index_origin, (uint64_t)row_index_stride, (int*)out_dev, status);
    err = hipGetLastError();
  }
  u64 bad = 0;
  if (err == hipSuccess) err = hipMemcpyAsync(&bad, status, sizeof bad, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) {
    try { vc_set_global_error((std::string("vc_sample_counts: ") + hipGetErrorString(err)).c_str()); } catch (...) {}
    return VC_ERR_HIP;
  }
  if (bad) {
    char msg[256];
    snprintf(msg, sizeof msg, "vc_sample_counts: %llu element(s) outside the sampler's range (rate not finite or above 2^20, shape_inv <= 0, or "
             "a rejection loop out of attempts); they are stored as -1", bad);
    return sc_fail(VC_ERR_RANGE, msg);
  }
  return VC_OK;
}
