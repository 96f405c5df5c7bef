/*
 * velocycle_hip.h -- C ABI of the MI355X (gfx950) engine for VeloCycle's SVI hot path.
 *
 * One engine = one fit (one model + guide + data shard) on one GPU.  One process per GPU; the
 * caller (velocycle_amd/engine.py through ctypes) owns the flat parameter / gradient buffers
 * (PyTorch-ROCm tensors passed as device pointers) and does the optimiser update and the
 * all-reduce; the library owns the count matrices (re-laid-out in HBM), per-step workspaces and
 * all kernels.  No C++ exception crosses this boundary: every call returns 0 (VC_OK) or a negative
 * code, with a message available from vc_last_error().
 *
 * Reference interfaces each entry point replaces (reference = lamanno-epfl/velocycle v0.1.0.5; the
 * reference has no FFI of its own -- its "interface" for this path is the set of Python objects
 * that `pyro.infer.SVI.step` drives):
 *
 *   vc_create / vc_set_*        the MetaparContainer built by preprocess_for_phase_estimation
 *                               (velocycle/preprocessing.py:168-205) and
 *                               preprocess_for_velocity_estimation (preprocessing.py:270-323),
 *                               plus poutine.condition/block wiring of
 *                               PhaseFitModel.__init__ (phase_inference_model.py:109-123) and
 *                               VelocityFitModel.__init__ (velocity_inference_model.py:60-74)
 *   vc_get_layout               the pyro.param store created by the guides
 *                               (phase_inference_guide.py:36-45, velocity_inference_guide.py:25-43, 78-102)
 *   vc_elbo_grad                one Trace_ELBO(num_particles=1).loss_and_grads(model, guide, mp):
 *                               guide trace + model replay + log-prob sums + backward, i.e. the body
 *                               of `svi.step` (phase_inference_model.py:169, velocity_inference_model.py:120)
 *                               for phase_latent_variable_model/guide (phase_inference_model.py:343-395,
 *                               phase_inference_guide.py:10-56) and velocity_latent_variable_model/guide
 *                               [_LRMN] (velocity_inference_model.py:304-471, velocity_inference_guide.py:9-141)
 *   vc_sample_posterior         Predictive(model, guide=guide, num_samples=n) as used by posterior_sampling
 *                               (velocity_inference_model.py:189-291, phase_inference_model.py:203-302)
 *   vc_expected_logs            the ElogS / ElogU / ElogS2 / ElogU2 einsums of posterior_sampling
 *                               (velocity_inference_model.py:236-258, phase_inference_model.py:248-262)
 *   vc_read_site                the sampled / deterministic sites a trace exposes
 *                               (pyro.deterministic calls at velocity_inference_model.py:327-369)
 *   vc_phase_mle                Phases.from_cycle_mle (phases.py:471-509): the log-likelihood of every cell's spliced counts
 *                               on a grid of phases (ElogS / exp / Poisson | GammaPoisson log_prob / sum over genes, :499-507)
 *                               and its arg-max per cell (:508); stand-alone, no engine
 *   vc_gene_glm                 no counterpart (a host loop of one GLM per gene would be it): the model of Phases.from_cycle_mle
 *                               (phases.py:487-507) solved for the gene harmonics with the phases known -- a Poisson or
 *                               negative-binomial log-link regression on the Fourier design per gene; stand-alone, no engine
 *   vc_gene_glm_batch           no counterpart: vc_gene_glm with the phase model's per-batch offsets (phase_inference_model.py: ElogS =
 *                               nu . zeta + Db . dnu + count_factor), nu and dnu estimated jointly per gene; stand-alone, no engine
 *   vc_gene_glm_weighted        no counterpart: vc_gene_glm with case weights per cell, R rows of weights per call (the cell bootstrap
 *                               of the harmonic fit, held-out fits, weighted regression); stand-alone, no engine
 *   vc_gene_glm_batch_weighted  no counterpart: vc_gene_glm_batch with case weights per cell, R rows of weights per call (the cell
 *                               bootstrap of the batch-aware fit: nu and dnu resampled jointly); stand-alone, no engine
 *   vc_gene_dispersion          no counterpart (the reference learns shape_inv only inside the SVI, velocity_inference_model.py:383):
 *                               the maximum-likelihood (or Gamma-prior mode) negative-binomial dispersion per gene with the means of
 *                               vc_gene_glm known; stand-alone, no engine
 *   vc_gene_kinetics            no counterpart (the reference learns logγg, logβg and νω only inside the SVI): the unspliced half of
 *                               velocity_inference_model.py:360-386 solved per gene for (log gamma, log beta) with the cycle, the
 *                               phases and the angular speed known, and the score and profile information of νω; stand-alone
 *   vc_gene_kinetics_weighted   no counterpart: vc_gene_kinetics with case weights per cell, R rows of weights per call, each row at
 *                               its own cycle, angular speed and start (the cell bootstrap of the kinetics fit and of the MAP
 *                               angular speed); stand-alone, no engine
 *   vc_gene_joint               no counterpart (the deterministic side of the V-joint configuration): velocity_inference_model.py:
 *                               360-386 solved per gene for (nu, log gamma, log beta) jointly from the spliced and the unspliced counts
 *                               with the phases and the angular speed known, and the score and profile information of νω; stand-alone
 *   vc_gene_joint_weighted      no counterpart: vc_gene_joint with case weights per cell, R rows of weights per call, each row at its
 *                               own angular speed and start (the cell bootstrap of the joint fit and of its MAP angular speed);
 *                               stand-alone, no engine
 *   vc_pca_stage, vc_pca_apply  Phases.from_pca_heuristic (phases.py:307-382): np.log(layer + small_count) and the one large
 *                               operation of a block power iteration that replaces sklearn's PCA(n_components).fit_transform
 *                               (:343-349); stand-alone, no engine
 *   vc_pointwise_density        no counterpart (Predictive + a traced model run per draw would be it): lppd / WAIC of every
 *                               observed count over posterior draws, summed per gene and per cell
 *   vc_sample_counts            the samplers behind pyro.sample("S" | "U", Poisson(mu) | GammaPoisson(1 / si, 1 / (si mu)))
 *                               (velocity_inference_model.py:385-386, phase_inference_model.py:343-395); stand-alone, no engine
 *   vc_predictive_check         Predictive(model, guide=guide, num_samples=n) with the observations removed
 *                               (the call pattern of velocity_inference_model.py:189-291 on the model of :338-386): replicated
 *                               counts per draw, reduced to statistics per gene and per cell
 *   vc_predictive_pit           no counterpart (Predictive + a [D][Ng][Nc] CDF tensor per matrix would be it): the randomized
 *                               probability integral transform of every observed count under the posterior predictive
 *                               distribution of the model of velocity_inference_model.py:338-386 / phase_inference_model.py:343-395
 *   vc_phase_marginal           the Bayesian twin of Phases.from_cycle_mle (phases.py:471-509): on its grid of phases (:495) the
 *                               likelihood of velocity_inference_model.py:338-386 / phase_inference_model.py:343-395 of every cell
 *                               (both matrices, batch offsets, per-gene shape_inv, posterior draws), as the cell's phase posterior
 *                               and its evidence with the phase integrated out
 */
#ifndef VELOCYCLE_HIP_H
#define VELOCYCLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): vc_stats ends with onehot_batches, tail_spec, tail_spec_matched, tail_spec_name[32], pw_lane, hist_split (a consumer built against
 * version 1 would have its smaller vc_stats overrun by vc_get_stats: vc_create refuses it); vc_tuning, vc_set_tuning / vc_get_tuning,
 * vc_dbg_signature, vc_set_optimizer / vc_adam_update exist. */
#define VC_ABI_VERSION 2

/* return codes */
#define VC_OK 0
#define VC_ERR_ARG (-1)          /* bad argument / shape */
#define VC_ERR_HIP (-2)          /* a HIP runtime call failed */
#define VC_ERR_UNSUPPORTED (-3)  /* configuration outside the compiled kernel set */
#define VC_ERR_STATE (-4)        /* call order violated (e.g. step before finalize) */
#define VC_ERR_NONFINITE (-5)    /* a step produced a NaN / Inf loss (vc_get_status) */
#define VC_ERR_RANGE (-6)        /* the count sampler met a rate outside its range (vc_sample_counts, vc_predictive_check) */

/* model / guide / noise selectors */
#define VC_MODEL_PHASE 0         /* phase_latent_variable_model */
#define VC_MODEL_VELOCITY 1      /* velocity_latent_variable_model[_LRMN] */
#define VC_GUIDE_MEANFIELD 0
#define VC_GUIDE_LRMN 1
#define VC_NOISE_NB 0            /* "NegativeBinomial" (GammaPoisson) */
#define VC_NOISE_POISSON 1
#define VC_NOISE_LOGNORMAL 2

/* sample sites (bit mask for conditioning, id for vc_set_conditioned / vc_read_site) */
#define VC_SITE_PHIXY 0      /* "ϕxy"       (Nc_local, 2) */
#define VC_SITE_NU 1         /* "ν"         (Ng, Nh)      */
#define VC_SITE_DNU 2        /* "Δν"        (Nb, Ng)      */
#define VC_SITE_SHAPE_INV 3  /* "shape_inv" (Ng)          */
#define VC_SITE_LOGGAMMA 4   /* "logγg"     (Ng)          */
#define VC_SITE_LOGBETA 5    /* "logβg"     (Ng)          */
#define VC_SITE_NUOMEGA 6    /* "νω"        (Nx, Nhw)     */
#define VC_SITE_RHO_REAL 7   /* "rho_real"  (Ng)          */
#define VC_SITE_COUNT 8
/* deterministic sites readable through vc_read_site */
#define VC_DET_PHI 16        /* "ϕ"     (Nc_local)        */
#define VC_DET_OMEGA 17      /* "ω"     (Nc_local)        */
#define VC_DET_EPS 18        /* the eps vector used by the last step (layout: vc_layout.eps_*) */

/* variational parameters (the guide's pyro.param store), all stored UNCONSTRAINED:
 * positive parameters are stored as their log (Pyro's transform_to(positive) = exp). */
#define VC_P_NU_LOCS 0          /* "ν_locs"        (Ng, Nh) */
#define VC_P_NU_USCALES 1       /* "ν_scales"      (Ng, Nh)  log */
#define VC_P_DNU_LOCS 2         /* "Δν_locs"       (Nb, Ng) */
#define VC_P_LOGGAMMA_LOCS 3    /* "logγg_locs"    (Ng) */
#define VC_P_LOGGAMMA_USCALES 4 /* "logγg_scales"  (Ng)      log */
#define VC_P_LOGBETA_LOCS 5     /* "logβg_locs"    (Ng) */
#define VC_P_LOGBETA_USCALES 6  /* "logβg_scales"  (Ng)      log */
#define VC_P_NUOMEGA_LOCS 7     /* "νω_locs"       (Nx, Nhw) */
#define VC_P_NUOMEGA_USCALES 8  /* "νω_scales"     (Nx, Nhw) log */
#define VC_P_SHAPE_INV_ULOCS 9  /* "shape_inv_locs"(Ng)      log */
#define VC_P_LRMN_LOC 10        /* "loc"           (Ng + Nx*Nhw) */
#define VC_P_LRMN_UCOV_FACTOR 11/* "cov_factor"    (Ng + Nx*Nhw, rank) log */
#define VC_P_LRMN_UCOV_DIAG 12  /* "cov_diag"      (Ng + Nx*Nhw) log */
#define VC_P_RHO_REAL_LOC 13    /* "rho_real_loc"  (Ng) */
#define VC_P_PHIXY_LOCS 14      /* "ϕxy_locs"      (Nc_local, 2)   -- the only rank-local block */
#define VC_P_COUNT 15

/* standard-normal draws of one guide call */
#define VC_E_LOGGAMMA 0   /* (Ng)       mean-field only */
#define VC_E_LOGBETA 1    /* (Ng)       */
#define VC_E_NU 2         /* (Ng, Nh)   */
#define VC_E_NUOMEGA 3    /* (Nx, Nhw)  mean-field only */
#define VC_E_LRMN_W 4     /* (rank)     LRMN only */
#define VC_E_LRMN_D 5     /* (Ng + Nx*Nhw) LRMN only */
#define VC_E_PHIXY 6      /* (Nc_local, 2)  -- rank-local block */
#define VC_E_COUNT 7

/* per-gene / global prior arrays for vc_set_prior (host pointers, float32) */
#define VC_PRIOR_MU_NU 0      /* μνg (Ng, Nh) */
#define VC_PRIOR_SD_NU 1      /* σνg (Ng, Nh) */
#define VC_PRIOR_MU_GAMMA 2   /* μγ (Ng) */
#define VC_PRIOR_SD_GAMMA 3
#define VC_PRIOR_MU_BETA 4
#define VC_PRIOR_SD_BETA 5
#define VC_PRIOR_MU_NUOMEGA 6 /* μνω (Nx, Nhw) */
#define VC_PRIOR_SD_NUOMEGA 7
#define VC_PRIOR_SD_DNU 8     /* σΔν (Nb, Ng) -- phase model; velocity hard-codes 0.01 (velocity_inference_model.py:332) */
#define VC_PRIOR_COUNT 9

typedef struct vc_engine vc_engine;

typedef struct vc_config {
  int32_t abi_version;     /* = VC_ABI_VERSION */
  int32_t model;           /* VC_MODEL_* */
  int32_t guide;           /* VC_GUIDE_* (phase: MEANFIELD) */
  int32_t noise;           /* VC_NOISE_* */
  int32_t with_delta_nu;   /* 0/1 */
  int32_t n_harmonics;     /* H   (Nh  = 2H+1), 1..3 */
  int32_t n_harmonics_w;   /* Hw  (Nhw = 2Hw+1), velocity only */
  int32_t Nb;              /* batches (rows of Db) */
  int32_t Nx;              /* conditions (rows of D), velocity only */
  int32_t lrmn_rank;       /* rho_rank (5) */
  int32_t rank;            /* data-parallel rank; rank 0 adds the replicated (gene-level) prior/entropy terms */
  int32_t world_size;
  int64_t Ng;              /* genes */
  int64_t Nc_local;        /* cells held by this rank */
  int64_t Nc_global;       /* cells over all ranks */
  int64_t cell_offset;     /* global index of this rank's first cell (eps stream slicing) */
  float gamma_alpha, gamma_beta;      /* shape_inv ~ Gamma(alpha, beta) */
  float sigma_ln_s, sigma_ln_u;       /* Lognormal noise scales (phase 0.5; velocity 0.1, 0.1) */
  float rho_mean, rho_std, rho_scale; /* LRMN */
  float reserved0;
} vc_config;

/* Tuning of the engine: DATA handed over by the caller, never ambient state (the library reads no environment variable).
 * All-zero = the measured defaults of DESIGN.md.  The reference has no counterpart (its "tuning" is the kwargs of
 * preprocess_for_* and the dict given to ClippedAdam: preprocessing.py:103-122, 207-240); SURVEY.md section 5 asks for "engine
 * config = plain C struct mirrored by a Python dataclass": this is it (velocycle_amd.tuning.Tuning).  Every rank of a sharded
 * run must pass the same values (the exchange buffer's layout follows genes_per_lane); the host side checks that. */
typedef struct vc_tuning {
  int32_t genes_per_lane;    /* 0: the rule of vc_finalize | 4 | 8 (8 is honoured only where that kernel has no scratch) */
  int32_t blocks_per_cu;     /* 0: the occupancy the code object reports | n: tile the likelihood kernel for n resident workgroups per CU */
  int32_t cells_per_wave;    /* 0: one balanced resident round | n: fixed cells per wave (ragged tiles in tests; no pass shares) */
  int32_t pass_min_cw;       /* cells per wave below which the dispatch passes take equal shares; 0 = 12 */
  int32_t n_pass_shares;     /* 0: measured defaults | 1: equal shares | 2..4: pass_shares[0..n) (later passes continue the last ratio) */
  float pass_shares[4];
  int32_t tail_cells;        /* cells per cell block of the second launch: 0 auto | 256 | 512 | 1024 */
  int32_t count_storage;     /* 0: uint16 whenever every count is an integer <= 65535 | 1: keep float32 */
  int32_t host_hist;         /* 1: per-gene count histograms by the host pass (the checker of the device pass) */
  int32_t hist_dense;        /* histogram form of the negative binomial's lgamma terms: 0 auto | 1 (value, multiplicity) lists | 2 dense tables */
  int32_t pw_inline;         /* the likelihood kernel's own d loglik / d nu_omega partials: 0 auto | 1 never | 2 even where they cost a resident workgroup */
  int32_t no_tail2;          /* 1: three launches per single-rank step where two (vc_tail2_kernel) are the default */
  int32_t no_tail_merged;    /* 1: the tutorial flow without its merged second launch */
  int32_t force_generic;     /* 1: the run-time-sized kernel set on a configuration the compiled fast set covers */
  int32_t particles_layout;  /* vc_svi_run_particles: 0 batched (K + 3 launches) | 1 serial | 2 streams */
  int32_t dense_batches;     /* 1: batch offsets as the dense Db contraction even when Db is one-hot (A/B, tests) */
  float p2p_timeout_s;       /* bound of the peer-to-peer exchange's wait; 0 = 2 s */
  int32_t no_tail_spec;      /* 1: the run-time-flag small kernels even where an instantiation compiled for this configuration exists (A/B, tests) */
  int32_t no_pw_lane;        /* 1: the U-only kernel reduces its per-cell sums over the wave even where the per-lane accumulation of the
                                nu_omega partials applies (one condition, D == 1; A/B, tests) */
  int32_t p2p_separate;      /* 1: the peer-to-peer exchange as a launch of its own between phases A and B (rounds 3-5); 0: folded into
                                phase B (its blocks pass the exchange's gate and add the ranks' slots where they read them) */
  int32_t p2p_one_launch;    /* 1 (with the peer-to-peer exchange): phases A and B of a sharded step in ONE launch, the exchange at block
                                granularity inside it -- K_main + one launch per step; needs 256-cell cell blocks and gene + cell + loss
                                blocks <= 240 (else the folded three-launch step).  Opt-in: it has run between processes on one device only */
  int32_t reserved[3];
} vc_tuning;

typedef struct vc_layout {
  int64_t header;                 /* floats reserved at the front of params/grad (grad[0..1] = loss hi/lo) */
  int64_t n_global;               /* floats of replicated parameters (after the header) */
  int64_t n_local;                /* floats of rank-local parameters (ϕxy_locs) */
  int64_t total;                  /* header + n_global + n_local */
  int64_t offset[VC_P_COUNT];     /* absolute float offset of each parameter block, -1 if absent */
  int64_t size[VC_P_COUNT];
  int64_t eps_n_global, eps_total;
  int64_t eps_offset[VC_E_COUNT]; /* float offset in the eps vector, -1 if absent */
  int64_t eps_size[VC_E_COUNT];
} vc_layout;

typedef struct vc_stats {
  int64_t algorithmic_bytes;      /* count-matrix bytes one step must read in the reference's fp32 storage */
  int64_t streamed_bytes;         /* bytes the main kernel actually streams (padded layout, uint16 or float32 elements) */
  int64_t main_grid, main_block;  /* launch geometry of the likelihood kernel */
  int32_t main_kind;              /* 0 phase(S) 1 velocity(S+U) 2 velocity, S-term hoisted (U only) */
  int32_t hist_on_device;         /* 1: the per-gene count histograms were built on the device during the re-layout */
  char main_kernel_name[96];
  int64_t setup_transient_bytes;  /* device memory vc_finalize held only while it ran (histogram tables, owned uploads) */
  int64_t count_storage_bytes;    /* bytes per count element in HBM: 2 (uint16: every count an integer <= 65535) or 4 */
  int32_t pass_cells[4];          /* cells per wave of the likelihood kernel's workgroups in dispatch pass 0..3 (all equal:
                                     balanced tiling; falling: the older passes take larger shares) */
  int32_t launches_per_step;      /* kernel launches of one steady-state step of vc_svi_run_fused on this engine: 2 or 3 */
  int32_t pw_inline;              /* floats per row of the likelihood kernel's own d loglik / d nu_omega partials (4 | 8), 0: off */
  int32_t generic;                /* 1: the run-time-sized (slower) kernel set is in use: a configuration outside the compiled
                                     fast set (H > 3, > 4 batches, LRMN rank > 8, > 64 angular-speed coefficients) */
  int32_t onehot_batches;         /* n > 0: the batch design matrix Db is one-hot, its n batch offsets are folded into the constant
                                     harmonic per workgroup of the likelihood kernel (the kernel's NB is 0: nothing per cell) */
  int32_t tail_spec;              /* > 0: the small kernels of this engine's fused steps (vc_svi_run_fused on one rank, vc_svi_run_sharded
                                     on a shard) RUN in the instantiation compiled for this configuration (row of
                                     csrc/vc_tail_spec_rows.inc, name in tail_spec_name); 0: run-time flags */
  int32_t tail_spec_matched;      /* the row the configuration's signature matched, whether or not that row is compiled for the launch
                                     structure in use (e.g. a "*_rank" row matched by a single-rank engine kept at three launches) */
  char tail_spec_name[32];
  int32_t pw_lane;                /* 1: the U-only likelihood kernel accumulates its d loglik / d nu_omega partials per lane from the cell
                                     record (one condition, D == 1: W_c = (1, sin k phi_c, cos k phi_c)) and stores no per-cell rows */
  int32_t hist_split;             /* gene blocks (per count matrix) whose dense histogram sums the one-launch tail evaluates in four quarter blocks:
                                     those whose largest count exceeds 255; 0 with the (value, multiplicity) lists (was reserved: same layout) */
} vc_stats;

/* lifecycle ------------------------------------------------------------------------------- */
int vc_abi_version(void);
int vc_create(const vc_config* cfg, vc_engine** out);
void vc_destroy(vc_engine* e);
/* message of the last failing call on `e` (e == NULL: of this thread's last failing vc_create / engine-less call such as vc_phase_mle) */
const char* vc_last_error(const vc_engine* e);

/* Tuning (optional): after vc_create and before the first vc_set_counts* call; NULL or never calling it = all defaults.
 * VC_ERR_ARG for a value outside the ranges documented at vc_tuning, VC_ERR_STATE once counts have been handed over. */
int vc_set_tuning(vc_engine* e, const vc_tuning* t);
/* The tuning in effect (what vc_set_tuning stored; all-zero if it was never called). */
int vc_get_tuning(const vc_engine* e, vc_tuning* out);
/* Builds of the library with -DVC_DBG_TIMES only (profiles/tools): writes the per-wave / per-block time stamps of the last
 * launches to `path`; VC_ERR_UNSUPPORTED in the product build. */
int vc_dbg_dump_times(vc_engine* e, const char* path);
/* the size-independent signature of the finalized configuration (csrc/vc_common.h: VcSig), n >= 27 ints: what
 * profiles/tools/print_signature.py turns into a row of csrc/vc_tail_spec_rows.inc */
int vc_dbg_signature(const vc_engine* e, int32_t* out, int n);

/* inputs (call before vc_finalize) ---------------------------------------------------------- */
/* Count matrices, element (g, c) at ptr[g*gene_stride + c*cell_stride] (so both the reference's
 * `S.T.float()` view -- gene_stride 1, cell_stride Ng -- and a contiguous (Ng,Nc) array work).
 * U may be NULL for the phase model.  on_device: pointers are device (1) or host (0) memory.  Device memory is NOT
 * copied: it is read by vc_finalize and must stay valid until vc_finalize has returned.  Host memory is uploaded
 * row by row (this rank's cells only).  Values must be finite and >= 0 (checked on the device; vc_finalize returns
 * VC_ERR_ARG otherwise). */
int vc_set_counts(vc_engine* e, const float* S, const float* U, int64_t gene_stride,
                  int64_t cell_stride, int on_device);
/* The same matrices as canonical CSR (rows = this rank's cells, columns = genes; no duplicate entries): what AnnData
 * layers hold before the reference densifies them (preprocessing.py:141-147 `.A`, 243-252).  which: 0 = spliced,
 * 1 = unspliced (velocity model).  indptr int64[Nc_local + 1], indices int32[nnz], data float[nnz]; on_device as above
 * (device arrays must stay valid until vc_finalize has returned).  The dense matrix is never formed on the host: the
 * blocked HBM layout is filled by a scatter kernel that also builds the per-gene count histograms.
 * Host arrays (on_device = 0) are validated here: indptr[0] == 0, indptr[Nc_local] == nnz, indptr non-decreasing; gene
 * indices and values are checked by the scatter kernel (vc_finalize returns VC_ERR_ARG).  On-device arrays
 * (on_device = 1) are TRUSTED: indptr is not read back or validated, and an indptr that is inconsistent with nnz makes
 * the scatter kernel read out of bounds.  The Python package never takes that path. */
int vc_set_counts_csr(vc_engine* e, int which, const int64_t* indptr, const int32_t* indices, const float* data,
                      int64_t nnz, int on_device);
/* count_factor (Nc_local), D (Nx, Nc_local) row-major [NULL for phase], Db (Nb, Nc_local) row-major
 * [NULL when Nb == 0], phixy_prior (Nc_local, 2).  Host pointers. */
int vc_set_cell_data(vc_engine* e, const float* count_factor, const float* D, const float* Db,
                     const float* phixy_prior);
int vc_set_prior(vc_engine* e, int which, const float* data, int64_t n);      /* host pointer */
/* poutine.condition: fix a sample site to `values` (host pointer, canonical shape of VC_SITE_*). */
int vc_set_conditioned(vc_engine* e, int site, const float* values, int64_t n);
/* Builds the HBM layout, per-gene count histograms, hoisted constants and workspaces. */
int vc_finalize(vc_engine* e, void* hip_stream);

/* hot path ---------------------------------------------------------------------------------- */
int vc_get_layout(const vc_engine* e, vc_layout* out);
/* One ELBO + gradient evaluation.  params/grad: device float[layout.total]; eps: device
 * float[layout.eps_total] or NULL (then eps = Philox4x32-10(seed, step, index), identical on every
 * rank for replicated sites and sliced by cell_offset for ϕxy).  step_dev: optional device int64
 * read instead of `step` and INCREMENTED by one at the end of the call (lets the call be replayed
 * from a captured hipGraph).  loss_dev: device double[loss_slots] (loss_slots >= 1); this rank's loss
 * contribution is written to slot step % loss_slots (and as float hi/lo to grad[0..1]).
 * Asynchronous on `hip_stream`; no allocation, no synchronisation. */
int vc_elbo_grad(vc_engine* e, const float* params, const float* eps, uint64_t seed, int64_t step,
                 int64_t* step_dev, float* grad, double* loss_dev, int64_t loss_slots, void* hip_stream);

/* pyro.optim.ClippedAdam (pyro-ppl 1.8.6 optim/clipped_adam.py; call sites: tutorial cells 27/43/56)
 * as ONE launch on a flat buffer of n floats: lr_t = lr*lrd^t, g = clamp(g, +-clip_norm),
 * m/v moments, p -= lr_t*sqrt(1-beta2^t)/(1-beta1^t) * m/(sqrt(v)+eps).  t is the 1-based step, read
 * from t_dev (device int64) when non-NULL.  An alternative to the PyTorch-op update of svi.py.
 * loss_hdr / loss_ring (optional, may be NULL): after an all-reduce of the gradient header the summed loss
 * (float hi + lo at loss_hdr[0..1]) is stored as a double into loss_ring[(t-1) % loss_slots]. */
int vc_clipped_adam(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                    double lr, double lrd, double beta1, double beta2, double eps, double clip_norm,
                    int64_t t, const int64_t* t_dev, const float* loss_hdr, double* loss_ring,
                    int64_t loss_slots, void* hip_stream);

/* The optimisers fit() accepts.  The reference hands whatever PyroOptim object it is given to pyro.infer.SVI
 * (velocity_inference_model.py:76-84,111; phase_inference_model.py:125-133,162): every package tutorial passes
 * pyro.optim.ClippedAdam (cells 27/43/56), tutorials/1D_Pancreas_Analysis.ipynb cell 26 passes pyro.optim.Adam (= torch.optim.Adam).
 *   VC_OPT_CLIPPED_ADAM  lr_t = lr * lrd^t, g = clamp(g, +-clip_norm), [g += weight_decay * p], m / v moments,
 *                        p -= lr_t sqrt(1 - beta2^t) / (1 - beta1^t) * m / (sqrt(v) + eps)
 *   VC_OPT_ADAM          [g += weight_decay * p], no clamp, no decay (lrd and clip_norm are ignored),
 *                        p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)       (amsgrad / maximize: not supported)
 * vc_set_optimizer selects what the step entry points of an engine apply (default: ClippedAdam, no weight decay);
 * vc_adam_update is the optimiser as a call of its own (vc_clipped_adam = kind VC_OPT_CLIPPED_ADAM, weight_decay 0).
 * `frozen` (DEVICE bytes, one per float of the flat parameter buffer / of the n updated floats; may be NULL; caller-owned, must stay
 * valid while the engine uses it): 1 marks a parameter TENSOR that has no path to the loss because its sample site is conditioned
 * (poutine.block: velocity_inference_model.py:65-66) -- PyroOptim never steps such a tensor (its .grad is None), so weight decay
 * must not move it either; without weight decay a frozen tensor stays where it is by itself (zero gradient, zero moments). */
#define VC_OPT_CLIPPED_ADAM 0
#define VC_OPT_ADAM 1
int vc_set_optimizer(vc_engine* e, int kind, double weight_decay, const uint8_t* frozen);
int vc_adam_update(int kind, float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double lrd,
                   double beta1, double beta2, double eps, double clip_norm, double weight_decay, const uint8_t* frozen, int64_t t,
                   const int64_t* t_dev, const float* loss_hdr, double* loss_ring, int64_t loss_slots, void* hip_stream);

/* One whole SVI step (single rank): vc_elbo_grad with pyro's ClippedAdam merged into its last kernel -- 4
 * launches instead of 5.  exp_avg / exp_avg_sq: device float[total - header], zero-initialised by the caller;
 * the optimiser step is step + 1.  Equivalent to vc_elbo_grad followed by vc_clipped_adam on params[header:].
 * grad still receives the gradient and the loss header.  Returns VC_ERR_STATE when world_size > 1: with sharded
 * cells the all-reduce has to sit between the two halves. */
int vc_svi_step(vc_engine* e, float* params, const float* eps, uint64_t seed, int64_t step, int64_t* step_dev,
                float* grad, double* loss_dev, int64_t loss_slots, float* exp_avg, float* exp_avg_sq, double lr,
                double lrd, double beta1, double beta2, double adam_eps, double clip_norm, void* hip_stream);

/* One whole SVI step (single rank) in THREE launches, every O(Ng + Nc) latency chain of the step run once: the
 * likelihood kernel; a per-gene-block / per-cell-block kernel that finishes the reductions, applies the chain rule,
 * pyro's ClippedAdam AND draws the guide sample of the next step from the fresh parameters (gene table, cell table,
 * prior / guide log-densities); and a small kernel for the one global dependency, the angular-speed coefficients
 * (gradient, optimiser, next sample, omega_c into the cell records) that also assembles the loss of the finished step.
 * eps is the Philox stream (seed, step, index) only.  step_dev (device int64, required) holds the number of finished
 * steps t: the call evaluates step t, stores its loss into loss_dev[t % loss_slots] and leaves step_dev = t + 1.
 * prime != 0: first draw the sample of step t from `params` as they are (needed for the first call, and again after the
 * caller has changed params / step_dev / seed behind the engine's back, e.g. on resume); prime = 0 continues from the
 * tables the previous call left.  Same trajectory as vc_svi_step (tests/test_hip_fused.py).  VC_ERR_STATE when
 * world_size > 1. */
int vc_svi_step_fused(vc_engine* e, float* params, uint64_t seed, int64_t* step_dev, float* grad, double* loss_dev,
                      int64_t loss_slots, float* exp_avg, float* exp_avg_sq, double lr, double lrd, double beta1,
                      double beta2, double adam_eps, double clip_norm, int prime, void* hip_stream);
/* n_steps of the above, back to back (the body of `for step in range(num_steps): svi.step(...)`,
 * velocity_inference_model.py:118-121, with verbose=False): 3 * n_steps asynchronous launches on hip_stream from one
 * call, no host round trip in between -- measured faster than replaying the same launches from a hipGraph (ROCm 7.2:
 * ~2 us per kernel node, profiles/r02_step_overhead.md).  loss_slots >= n_steps keeps every loss of the run. */
int vc_svi_run_fused(vc_engine* e, float* params, uint64_t seed, int64_t* step_dev, float* grad, double* loss_dev,
                     int64_t loss_slots, float* exp_avg, float* exp_avg_sq, double lr, double lrd, double beta1,
                     double beta2, double adam_eps, double clip_norm, int prime, int64_t n_steps, void* hip_stream);

/* --- opt-in: the loss every k-th step only ("or every k steps in perf mode") -----------------------------
 * The reference's loop takes the loss of EVERY step from `svi.step` (velocity_inference_model.py:118-121); that stays the default
 * (k = 1).  vc_set_loss_every(e, k > 1) lets the launches of vc_svi_run_fused run a gradient-only instantiation of the likelihood
 * kernel except at every k-th one (counted from this call: launches 0, k, 2k, ... form the loss).  What that instantiation leaves
 * out is what serves the loss VALUE only: with phi_xy, nu, delta nu and shape_inv conditioned (the tutorials' velocity stage)
 * both logarithms per element (the gradients then agree with the full kernel's to float32 rounding: mu = 2^eta * z instead of
 * 2^(eta + log2 z)); with shape_inv learned only log2(z) and the loss accumulations (the same gradient bits).  The loss slots of
 * the other steps hold the prior / guide terms without the likelihood -- the caller must not read them as losses (velocycle_amd
 * reports NaN there).  Negative-binomial noise on the compiled fast kernel set; VC_ERR_UNSUPPORTED otherwise.
 * vc_svi_step_fused, vc_svi_run_sharded, vc_elbo_grad and vc_svi_run_particles always form the loss. */
int vc_set_loss_every(vc_engine* e, int32_t k);

/* --- Trace_ELBO(num_particles = K) from one call (single rank) -----------------------------------------------------------
 * Replaces, for `fit(loss=Trace_ELBO(num_particles=K))` (velocity_inference_model.py:79,111, phase_inference_model.py:128,162:
 * the user's ELBO object goes into SVI; K guide draws per step, loss and gradients averaged before the optimiser step), the
 * host loop  K x vc_elbo_grad + average + vc_clipped_adam:  n_steps steps are enqueued from this one call, per step
 *   particle k < K:  K_pre (Philox stream (seed, t K + k), t read from step_dev) -> K_main -> K_post -> K_fin, with its own
 *               per-step workspaces and gradient buffer and, for k >= 1, on a HIP stream of the engine's (created at the first
 *               call; the parameters do not change between particles, so every K_pre starts at once, the likelihood kernels
 *               follow one another, K_post / K_fin of particle k run beside K_main of particle k + 1);
 *   hip_stream joins them: the K gradients and losses are added in particle order and multiplied by 1 / K -- left in `grad`
 *   (header: the averaged loss, hi / lo) and in loss_dev[t % loss_slots]; step_dev := t + 1; ClippedAdam.
 * The same kernels and arithmetic as the host loop -- the same numbers.  step0 = the value step_dev holds when the call is made
 * (the host's mirror: used for the non-finite-loss latch).  grad_acc: DEVICE float[total], caller-owned (kept in the signature;
 * not written since the particles have buffers of their own).  At most 16 particles (VC_ERR_UNSUPPORTED beyond).  Cells sharded:
 * VC_ERR_STATE (the average has to cross the all-reduce before the optimiser; the host loop does that). */
int vc_svi_run_particles(vc_engine* e, float* params, uint64_t seed, int64_t* step_dev, int64_t step0, float* grad,
                         float* grad_acc, double* loss_dev, int64_t loss_slots, float* exp_avg, float* exp_avg_sq, double lr,
                         double lrd, double beta1, double beta2, double adam_eps, double clip_norm, int num_particles,
                         int64_t n_steps, void* hip_stream);

/* --- cells sharded over ranks: the fused step cut at its one exchange ------------------------------
 * The per-step sequence of a rank is  K_main -> phase A -> [sum of the exchange buffer over all ranks] -> phase B  (three
 * launches + the exchange; the single-rank step of vc_svi_run_fused is the same code with nothing to sum).  It replaces, for
 * `svi.step` under a process group (velocity_inference_model.py:118-121 has no multi-GPU form: SURVEY.md F1), the
 * five-kernel sequence vc_elbo_grad + all-reduce + vc_clipped_adam.
 *
 * Exchange buffer `xbuf`: DEVICE float[vc_exchange_size], caller-owned like params / grad, zero-initialised once.
 *   [0, header + n_global)                         gradient partials of the replicated parameters, offsets of `grad`
 *   [pw_off, pw_off + pw_cap * Nx * Nhw)           per-cell-block partials of d loglik / d nu_omega (rows beyond a rank's
 *                                                  own cell blocks are zero), pw_cap = ceil(ceil(Nc_global / world) / 256)
 *   [loss_off, loss_off + 4 * (1 + ceil(Ng/64)))   the rank's loss terms, each double as four floats on fixed grids (their
 *                                                  float32 sum over <= 16 ranks is exact)
 * Every element is additive over ranks; replicated prior / entropy terms are contributed by rank 0 only.  After the sum
 * every rank holds the complete gradient and applies the identical update: parameters stay replicated bit for bit.
 *
 * phase = VC_PHASE_A : K_main + phase A of ONE step (n_steps must be 1); the caller then sums xbuf over the ranks
 *                      (e.g. torch.distributed.all_reduce -- any backend) on the same stream and calls
 * phase = VC_PHASE_B : phase B of that step (optimiser on the summed gradient, next guide sample, loss of the step into
 *                      loss_dev[t % loss_slots], step_dev = t + 1 was already set by phase A's K_main).
 * phase = VC_PHASE_AB: n_steps whole steps enqueued from this one call, the exchange made by the engine's own communicator
 *                      (vc_comm_init_rccl: ncclAllReduce on hip_stream between the two phases; world_size 1 needs none).
 * prime: as vc_svi_run_fused (sampling is rank-local: no exchange).  Same arguments otherwise. */
#define VC_PHASE_A 1
#define VC_PHASE_B 2
#define VC_PHASE_AB 3
int vc_exchange_size(const vc_engine* e, int64_t* n_floats);
int vc_svi_run_sharded(vc_engine* e, float* params, uint64_t seed, int64_t* step_dev, float* grad, float* xbuf,
                       double* loss_dev, int64_t loss_slots, float* exp_avg, float* exp_avg_sq, double lr, double lrd,
                       double beta1, double beta2, double adam_eps, double clip_norm, int prime, int phase,
                       int64_t n_steps, void* hip_stream);
/* The engine's own communicator for VC_PHASE_AB: RCCL, loaded at run time from `rccl_path` (the librccl.so the process
 * already uses, e.g. the one bundled with PyTorch -- the library itself does not link RCCL).  Rank 0 creates the 128-byte
 * unique id (vc_comm_rccl_unique_id), the host side broadcasts it (any transport), every rank of the engine's world_size
 * calls vc_comm_init_rccl with it (collective).  vc_destroy releases the communicator. */
int vc_comm_rccl_unique_id(const char* rccl_path, void* id_out_128_bytes);
int vc_comm_init_rccl(vc_engine* e, const char* rccl_path, const void* id_128_bytes);
/* Sum of a DEVICE float buffer over the ranks of that communicator, in place, on hip_stream (the collective of VC_PHASE_AB as a
 * call of its own: the host side uses it once to check the communicator against torch.distributed's sum of the same buffer). */
int vc_comm_allreduce(vc_engine* e, float* buf, int64_t n, void* hip_stream);

/* The one-shot exchange for VC_PHASE_AB over peer-mapped device memory (SURVEY.md section 5's latency-optimised variant;
 * velocycle_amd/csrc/vc_p2p_exchange.hip): every rank publishes its exchange buffer in a region of its own HBM and a
 * step-stamped flag in every peer's region, then reads all N buffers directly and adds them in fixed rank order (identical
 * bits on every rank, no float atomics).  vc_p2p_alloc creates this rank's region and returns its 64-byte hipIpcMemHandle_t;
 * the host side gathers the handles of all ranks in rank order (any transport) and hands the world_size x 64 bytes to
 * vc_p2p_connect (collective in effect: every rank must do it before the first step).  When connected, VC_PHASE_AB uses
 * this exchange instead of RCCL -- since round 6 without a launch of its own: phase B's blocks run the publish / wait protocol
 * and add the ranks' buffers in rank order where they read them (vc_tuning.p2p_separate = 1: the separate exchange kernel).  A peer that never publishes is detected by a bounded wait (vc_tuning.p2p_timeout_s, default 2 s):
 * vc_get_status then returns VC_ERR_STATE.  Opt-in: it has run across processes on one device only. */
int vc_p2p_alloc(vc_engine* e, void* ipc_handle_out_64_bytes);
int vc_p2p_connect(vc_engine* e, const void* all_handles_world_x_64_bytes);

/* One draw of the guide pushed through the deterministic part of the model (what
 * `Predictive(model, guide=guide, num_samples=1)` evaluates for the latent and deterministic sites;
 * velocity_inference_model.py:279-291, phase_inference_model.py:274-302): runs the sampling kernel only, no
 * likelihood.  The site values are then available through vc_read_site. */
int vc_sample_guide(vc_engine* e, const float* params, const float* eps, uint64_t seed, int64_t step,
                    void* hip_stream);

/* n_draws guide draws pushed through the deterministic part of the model, batched on the device: what
 * `Predictive(model, guide=guide, num_samples=n_draws)` evaluates for the latent and deterministic sites
 * (velocity_inference_model.py:279-291 / posterior_sampling :189-262, phase_inference_model.py:274-302).  Draw i
 * uses the Philox stream (seed, step0 + i), i.e. it equals vc_sample_guide(e, params, NULL, seed, step0 + i).
 * sites[k] is a VC_SITE_* id or VC_DET_PHI / VC_DET_OMEGA; out_dev[k] is DEVICE memory, float
 * [n_draws][length of that site], filled draw-major.  Asynchronous on hip_stream: nothing is copied to the host. */
int vc_sample_posterior(vc_engine* e, const float* params, uint64_t seed, int64_t step0, int64_t n_draws,
                        int n_sites, const int* sites, float* const* out_dev, void* hip_stream);

/* The dense E[log S] / E[log U] summaries that posterior_sampling adds to the posterior
 * (velocity_inference_model.py:236-258, phase_inference_model.py:248-262), evaluated on the device:
 *   out_S [g][c] = nu[g,:] . zeta(phi_c) + sum_b Db[b,c] dnu[b,g] + count_factor[c]
 *   out_S2[g][c] = the same with the constant count factor cf_avg
 *   out_U [g][c] = -logbeta[g] + log(relu(nu[g,:] . zeta'(phi_c) * omega[c] + gamma[g]) + 1e-5) + out_S[g][c]
 *   out_U2       = the same on out_S2
 * Every pointer is DEVICE memory: nu float[Ng][Nh], dnu float[Nb][Ng] (NULL without batches), phi / omega float[Nc_local],
 * logbeta / gamma float[Ng]; outputs float[Ng][Nc_local] row-major.  omega, logbeta, gamma, out_U, out_U2 are NULL for the
 * phase model.  count_factor and Db are the ones handed to vc_set_cell_data.  Asynchronous on hip_stream. */
int vc_expected_logs(vc_engine* e, const float* nu, const float* dnu, const float* phi, const float* omega,
                     const float* logbeta, const float* gamma, float cf_avg, float* out_S, float* out_S2,
                     float* out_U, float* out_U2, void* hip_stream);

/* --- maximum-likelihood phase assignment on a grid (stand-alone: no engine handle) -----------------------------------------
 * Replaces the body of Phases.from_cycle_mle (phases.py:487-508): for every cell c and bin j < bins the log-likelihood of the
 * cell's counts under  mu = exp(T[j,g]) * m[c]  summed over the genes, then the best bin per cell.  The reference materialises
 * [bins][Ng][Nc] float32 tensors for this; here nothing of that size exists: one launch, no workspace, no allocation, no
 * synchronisation (asynchronous on hip_stream).  Every pointer is DEVICE memory.
 *   counts_dev   element (g, c) at index g * gene_stride + c (gene_stride >= Nc); float (VC_COUNTS_F32) or uint16_t (VC_COUNTS_U16)
 *   T_dev        float[bins][Ng]: zeta(phi_j) . means (natural log units);  expT_dev: its exponential, same layout
 *   m_dev        float[Nc] > 0: n_c^a (phases.py:492-494)
 *   noise        VC_NOISE_POISSON | VC_NOISE_NB; VC_NOISE_LOGNORMAL returns VC_ERR_UNSUPPORTED (the reference raises
 *                NotImplementedError, phases.py:504)
 *   r_dev        float[Ng] > 0: 1 / dispersion per gene (GammaPoisson(1 / si, 1 / (si mu)), phases.py:503); NULL for Poisson
 *   best_bin_dev int32[Nc]: arg max over j; of equal bins the FIRST wins (torch.argmax, phases.py:508)
 *   logp_rel_dev NULL, or float[bins][Nc]: logP[j,c] - max_j logP[j,c] (<= 0, exactly 0 at best_bin): the terms of the
 *                log-likelihood that do not depend on the bin (lgamma, r log r) cancel in it and are never formed
 * Magnitudes: the sums are formed from exp(T) + r / m and m / k, so the caller should hand over T and m on comparable scales
 * (mu is unchanged by T + s, m * exp(-s); velocycle_amd.phase_mle centres T).  bins 1..4096, any Ng >= 1, Nc >= 1.  Results are
 * bit-reproducible and do not depend on how the caller cuts the cells into calls.  Errors: vc_last_error(NULL). */
#define VC_COUNTS_F32 0
#define VC_COUNTS_U16 1
int vc_phase_mle(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* T_dev,
                 const float* expT_dev, int bins, const float* m_dev, int noise, const float* r_dev, int32_t* best_bin_dev,
                 float* logp_rel_dev, void* hip_stream);

/* --- per-gene harmonic regression given the phases (stand-alone: no engine handle) -------------------------------------------
 * The model of Phases.from_cycle_mle (phases.py:487-507), mu_gc = exp(nu_g . zeta(phi_c)) n_c^a, solved for nu with the phases known:
 * one Poisson or negative-binomial log-link regression on a Fourier design per gene, by a damped Newton iteration that runs inside
 * the kernel (one workgroup per gene, one launch, no workspace, no allocation, no synchronisation; asynchronous on hip_stream).
 * Every pointer is DEVICE memory.
 *   counts_dev      element (g, c) at index g * gene_stride + c (gene_stride >= Nc); float (VC_COUNTS_F32) or uint16_t (VC_COUNTS_U16)
 *   basis_dev       float[K][Nc], K = 2 H + 1 in {1, 3, 5, 7}: rows [1, sin phi, cos phi, sin 2 phi, ...] (utils.torch_fourier_basis);
 *                   row 0 is taken to be 1 and is not read
 *   logm_dev        float[Nc]: a log n_c (phases.py:492-494), the offset of eta = nu . basis[:, c] + logm[c]
 *   noise           VC_NOISE_POISSON | VC_NOISE_NB; VC_NOISE_LOGNORMAL returns VC_ERR_UNSUPPORTED
 *   r_dev           float[Ng] > 0: 1 / dispersion per gene; NULL for Poisson
 *   prior_mean_dev, prior_prec_dev   both NULL (maximum likelihood), or double[Ng][K] each: a Gaussian prior per coefficient, its
 *                   penalty sum_i prec_i (nu_i - mean_i)^2 / 2 taken off the objective; a coefficient whose mean is not finite or
 *                   whose precision is not a positive finite number has none
 *   tol, max_iter   stop at the Newton decrement g' H^-1 g <= tol (>= 0), after at most max_iter (>= 1) steps
 * Objective (the part of the log-likelihood that depends on nu), mu = exp(eta):
 *   Poisson  sum_c k eta - mu         NB  sum_c k ln(mu / (r + mu)) - r ln((r + mu) / r)  =  sum_c k eta - (k + r) ln(r + mu)  +  Nc r ln r
 * (the negative binomial's r ln r is inside, so that every term has the size of a log-probability); the Hessian is the observed one,
 * w = mu | mu r (k + r) / (r + mu)^2, with the prior precisions on its diagonal.  Start: nu_0 = ln(sum k / sum e^logm), harmonics 0
 * (with a prior: its means, except nu_0).  Per-element arithmetic is float32 (eta itself is formed in float64 from the float32 tables),
 * every sum float64 in a fixed order, the K x K algebra float64: identical bits under repetition, uint16 or float32 storage, and any
 * cutting of the genes into calls.  Outputs, per gene, of the last accepted point:
 *   nu_dev          double[Ng][K]
 *   cov_dev         double[Ng][K (K + 1) / 2]: H^-1, lower triangle packed row by row ((i, j), j <= i, at i (i + 1) / 2 + j); NaN when SINGULAR
 *   loglik_dev      double[Ng]: the objective above, without the prior term
 *   dec_dev         double[Ng]: the last Newton decrement;  iterations_dev int32[Ng]: Newton steps taken
 *   status_dev      int32[Ng]:
 *     VC_GLM_CONVERGED  dec <= tol
 *     VC_GLM_ROUNDING   the gradient cannot be told from its float32 rounding: every |g_i| <= 4 eps32 sqrt(sum_c (w_c^2 + res_c^2) B_ic^2),
 *                       res the residual k - mu | (k - mu) r / (r + mu) (a relative error e of mu moves res by w e; res itself rounds by
 *                       |res| e).  At counts of 10^4 this floor of dec lies above a tol of 1e-10
 *     VC_GLM_UNBOUNDED  a step would take a harmonic coefficient out of [-50, 50] (separation: no finite maximum), or the gene has no
 *                       count at all; nu is the last point inside (no count: nu_0 = -inf, the other outputs NaN)
 *     VC_GLM_SINGULAR   the Cholesky factorisation of the Hessian failed (a pivot <= 0 or not finite)
 *     VC_GLM_MAX_ITER   max_iter steps were taken, or the gene used up its 30 step halvings (a step is halved while the objective drops
 *                       by more than its own float32 rounding, 8 eps32 sum |terms|)
 * A gene's status touches no other gene's outputs; every path is bounded.  VC_ERR_ARG (NULL input or output, K not in {1, 3, 5, 7},
 * Nc < 1, Ng < 1, gene_stride < Nc, max_iter < 1, tol < 0, one prior pointer without the other, NB without r_dev), VC_ERR_UNSUPPORTED
 * (Lognormal): all decided before anything is launched.  Errors: vc_last_error(NULL). */
#define VC_GLM_CONVERGED 0
#define VC_GLM_ROUNDING 1
#define VC_GLM_UNBOUNDED 2
#define VC_GLM_SINGULAR 3
#define VC_GLM_MAX_ITER 4
int vc_gene_glm(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev, int K,
                const float* logm_dev, int noise, const float* r_dev, const double* prior_mean_dev, const double* prior_prec_dev,
                double tol, int max_iter, double* nu_dev, double* cov_dev, double* loglik_dev, double* dec_dev,
                int32_t* iterations_dev, int32_t* status_dev, void* hip_stream);

/* --- per-gene harmonic regression with per-batch offsets (stand-alone: no engine handle) --------------------------------------
 * vc_gene_glm with the phase model's batch factor, ElogS = nu . zeta(phi) + Db . dnu + count_factor: per gene, nu (K coefficients) and
 * one offset delta_b per batch are estimated jointly,
 *   eta_c = nu . basis[:, c] + delta_b(c) + logm[c],   mu = exp(eta),
 * by maximising vc_gene_glm's Poisson / negative-binomial objective minus sum_b q_b (delta_b - m_b)^2 / 2 (and minus the optional
 * Gaussian prior of nu).  Every delta_b ALWAYS has its prior: it is what separates nu_0 from the mean of delta.  One workgroup per
 * gene, one launch, no workspace, no allocation, no synchronisation; asynchronous on hip_stream.  counts_dev, count_kind, Ng, Nc,
 * gene_stride, basis_dev, K, logm_dev, noise, r_dev, prior_mean_dev, prior_prec_dev, tol, max_iter: as for vc_gene_glm.
 *   Nb, seg_host    the cells of a batch are contiguous: batch b owns the cells [seg[b], seg[b + 1]).  seg_host is int64_t[Nb + 1] in
 *                   HOST memory (it is checked here and travels in the kernel's arguments): seg[0] = 0, seg[Nb] = Nc, strictly
 *                   increasing (an empty segment is refused); 1 <= Nb <= VC_GLM_MAX_BATCHES
 *   delta_prior_mean_dev, delta_prior_prec_dev   double[Ng][Nb] in device memory, never NULL: m_b and q_b = 1 / std_b^2.  A gene with
 *                   an m_b that is not finite or a q_b that is not a positive finite number ends VC_GLM_SINGULAR (device memory is not
 *                   read before the launch)
 * Per-element arithmetic and every sum are vc_gene_glm's; a pass walks the segments in order and folds after each, the (K + Nb)-square
 * Newton system is solved through the Schur complement of its diagonal delta block in float64.  Identical bits under repetition,
 * uint16 or float32 storage and any cutting of the genes into calls.  Rules and status codes are vc_gene_glm's over the K + Nb
 * coefficients: start nu_0 = ln(sum k / sum e^logm), harmonics 0 (their prior means), delta = m; VC_GLM_CONVERGED on the full
 * decrement g' H^-1 g <= tol; VC_GLM_ROUNDING when every one of the K + Nb gradient entries is within 4 eps32 sqrt(N_i);
 * VC_GLM_UNBOUNDED when a harmonic or a delta_b of a step leaves [-50, 50], or the gene has no count; VC_GLM_SINGULAR when a pivot of
 * the Schur complement or a D_b = sum_{c in b} w + q_b is not a positive finite number; VC_GLM_MAX_ITER (or 30 halvings of the
 * penalised objective used up).  Outputs per gene, of the last accepted point:
 *   nu_dev          double[Ng][K];   delta_dev  double[Ng][Nb]
 *   cov_nu_dev      double[Ng][K (K + 1) / 2]: the nu block of the inverse Hessian, packed as vc_gene_glm's cov_dev; NaN when SINGULAR
 *   delta_var_dev   double[Ng][Nb]: the diagonal of the delta block of the inverse Hessian; NaN when SINGULAR
 *   loglik_dev      the objective without any prior term;  dec_dev, iterations_dev, status_dev: as for vc_gene_glm
 * A gene's status touches no other gene's outputs; every path is bounded.  VC_ERR_ARG (vc_gene_glm's, Nb out of range, a NULL seg_host
 * or delta prior, a seg that does not start at 0, end at Nc or increase strictly): all decided before anything is launched. */
#define VC_GLM_MAX_BATCHES 32
int vc_gene_glm_batch(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev, int K,
                      const float* logm_dev, int noise, const float* r_dev, int Nb, const int64_t* seg_host,
                      const double* delta_prior_mean_dev, const double* delta_prior_prec_dev, const double* prior_mean_dev,
                      const double* prior_prec_dev, double tol, int max_iter, double* nu_dev, double* delta_dev, double* cov_nu_dev,
                      double* delta_var_dev, double* loglik_dev, double* dec_dev, int32_t* iterations_dev, int32_t* status_dev,
                      void* hip_stream);

/* --- per-gene harmonic regression with case weights (stand-alone: no engine handle) -------------------------------------------
 * vc_gene_glm with every cell's contribution multiplied by a weight w_bc >= 0: one call solves R rows of weights for every gene (a
 * cell bootstrap: Poisson(1) integers per row; a held-out fit: 0 / 1; the ordinary weighted regression: the caller's weights).  One
 * workgroup per (gene, row), grid (R, genes) with the row as the fast index, one launch per 65535 genes, no workspace, no allocation, no synchronisation; asynchronous on hip_stream.
 * counts_dev, count_kind, Ng, Nc, gene_stride, basis_dev, K, logm_dev, noise, r_dev, prior_mean_dev, prior_prec_dev, tol, max_iter:
 * as for vc_gene_glm.  Every pointer is DEVICE memory.
 *   weights_dev     float: w_bc at index b * weight_stride + c (weight_stride >= Nc; what lies between Nc and the stride is not read).
 *                   Weights are taken to be finite and >= 0 (device memory is not read before the launch); a row with a NaN weight ends
 *                   VC_GLM_UNBOUNDED like a row without counts
 *   R               rows of weights, 1..65535 per call
 *   start_dev       NULL, or double[Ng][K]: where every entry of gene g is finite and its harmonics lie in [-50, 50], the first point of
 *                   every row of gene g (the bootstrap warm-starts from the full-data fit); otherwise the row's default start
 * With wt = (double)w_bc and res, wo, term, mag the per-element numbers of vc_gene_glm:
 *   gradient sum_c (wt res) B_i      Hessian sum_c (wt wo) B_i B_j      objective sum_c wt term      A = sum_c wt mag
 *   N_i = sum_c ((wt wo)^2 + (wt res)^2) B_i^2                            default start nu_0 = ln(sum_c wt k / sum_c wt e^logm)
 * The negative binomial's r ln r is inside term and weighted with it; the prior is not weighted.  Each product with wt is formed first and
 * is exact at wt == 1; the float64 operations that follow, the fold, the K x K algebra, the step rules (halving, the [-50, 50] bound,
 * VC_GLM_ROUNDING on the weighted N_i, max_iter) and the status codes are vc_gene_glm's.  A row whose sum_c wt k is not a positive finite
 * number (or whose default nu_0 is not finite) ends VC_GLM_UNBOUNDED with the outputs vc_gene_glm gives a gene without counts: nu_0 as
 * formed (-inf or NaN), harmonics 0, cov, loglik and dec NaN, 0 iterations -- whatever start_dev holds.
 * Outputs, of row b and gene g at index b * Ng + g:
 *   nu_dev double[R][Ng][K];  cov_dev NULL (not stored) or double[R][Ng][K (K + 1) / 2], packed as vc_gene_glm's;
 *   loglik_dev, dec_dev double[R][Ng];  iterations_dev, status_dev int32[R][Ng]
 * Bits: identical under repetition; identical between uint16 and float32 storage; identical under any cutting of the genes or of the
 * rows into calls (row b of an R-row call equals the call on that row alone); with a table of ones, R = 1 and start_dev NULL every
 * output equals vc_gene_glm's on the same inputs bit for bit.  A (gene, row) pair's status touches no other pair's outputs; every path
 * is bounded.  VC_ERR_ARG / VC_ERR_UNSUPPORTED as vc_gene_glm's in its order (cov_dev may be NULL here), then weights_dev NULL, R outside
 * 1..65535, weight_stride < Nc: all decided before anything is launched.  Errors: vc_last_error(NULL). */
int vc_gene_glm_weighted(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev,
                         int K, const float* logm_dev, int noise, const float* r_dev, const double* prior_mean_dev,
                         const double* prior_prec_dev, const float* weights_dev, int64_t R, int64_t weight_stride,
                         const double* start_dev, double tol, int max_iter, double* nu_dev, double* cov_dev, double* loglik_dev,
                         double* dec_dev, int32_t* iterations_dev, int32_t* status_dev, void* hip_stream);

/* --- per-gene harmonic regression with per-batch offsets and case weights (stand-alone: no engine handle) ----------------------
 * vc_gene_glm_batch with every cell's contribution multiplied by a weight w_bc >= 0, R rows of weights per call: the step
 * vc_gene_glm_weighted takes from vc_gene_glm (the cell bootstrap of the batch-aware fit resamples nu and the offsets jointly).  One
 * workgroup per (gene, row), grid (R, genes) with the row as the fast index, one launch per 65535 genes, the segment table in the
 * kernel's arguments, no workspace, no allocation, no synchronisation; asynchronous on hip_stream.  counts_dev, count_kind, Ng, Nc,
 * gene_stride, basis_dev, K, logm_dev, noise, r_dev, Nb, seg_host, delta_prior_mean_dev, delta_prior_prec_dev, prior_mean_dev,
 * prior_prec_dev, tol, max_iter: as for vc_gene_glm_batch.  Every pointer but seg_host is DEVICE memory.
 *   weights_dev     float: w_bc at index b * weight_stride + c (weight_stride >= Nc; what lies between Nc and the stride is not read),
 *                   in the cell order of counts, basis and logm: the sorted one, with the segments of seg_host.  Weights are taken to
 *                   be finite and >= 0 (device memory is not read before the launch)
 *   R               rows of weights, 1..65535 per call
 *   start_nu_dev, start_delta_dev   both NULL, or double[Ng][K] and double[Ng][Nb]: where every entry of gene g is finite, its
 *                   harmonics lie in [-50, 50] and every offset lies in [-50, 50], the first point of every row of gene g; otherwise
 *                   the row's default start, nu_0 = ln(sum_c wt k / sum_c wt e^logm), harmonics at their prior means or 0, delta = m
 * With wt = (double)w_bc the sums of segment b are  sum (wt res) = dL/d delta_b,  h_b = sum (wt wo) B_i (W_b = h_b0),
 * N with (wt wo)^2 + (wt res)^2,  L = sum wt term,  A = sum wt mag.  The priors of nu and delta are not weighted.  Each product with wt
 * is formed first and is exact at wt == 1; the float64 operations that follow, the fold after each segment, the Schur complement with
 * its cancellation-free row 0, the step and halving rules, the [-50, 50] bound, VC_GLM_ROUNDING over the K + Nb entries and the status
 * codes are vc_gene_glm_batch's.  A batch whose cells all weigh 0 in a row is no error: D_b = q_b and its offset goes to its prior
 * mean.  A row whose sum_c wt k is not a positive finite number (a NaN weight included) ends VC_GLM_UNBOUNDED with the outputs
 * vc_gene_glm_batch gives a gene without counts: nu_0 as formed, harmonics 0, delta = m, cov_nu, delta_var, loglik and dec NaN,
 * 0 iterations -- whatever the start holds.  Outputs, of row b and gene g at index b * Ng + g:
 *   nu_dev double[R][Ng][K];  delta_dev double[R][Ng][Nb];
 *   cov_nu_dev double[R][Ng][K (K + 1) / 2] and delta_var_dev double[R][Ng][Nb]: both NULL (not stored) or both given;
 *   loglik_dev, dec_dev double[R][Ng];  iterations_dev, status_dev int32[R][Ng]
 * Bits: identical under repetition; identical between uint16 and float32 storage; identical under any cutting of the genes or of the
 * rows into calls (row b of an R-row call equals the call on that row alone); with a table of ones, R = 1 and no start all eight
 * outputs equal vc_gene_glm_batch's on the same inputs bit for bit.  A (gene, row) pair's status touches no other pair's outputs; every
 * path is bounded.  VC_ERR_ARG / VC_ERR_UNSUPPORTED as vc_gene_glm_batch's in its order (the two variance outputs may be NULL here),
 * then weights_dev NULL, R outside 1..65535, weight_stride < Nc, one start pointer without the other, one variance pointer without
 * the other: all decided before anything is launched.  Errors: vc_last_error(NULL). */
int vc_gene_glm_batch_weighted(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev,
                               int K, const float* logm_dev, int noise, const float* r_dev, int Nb, const int64_t* seg_host,
                               const double* delta_prior_mean_dev, const double* delta_prior_prec_dev, const double* prior_mean_dev,
                               const double* prior_prec_dev, const float* weights_dev, int64_t R, int64_t weight_stride,
                               const double* start_nu_dev, const double* start_delta_dev, double tol, int max_iter, double* nu_dev,
                               double* delta_dev, double* cov_nu_dev, double* delta_var_dev, double* loglik_dev, double* dec_dev,
                               int32_t* iterations_dev, int32_t* status_dev, void* hip_stream);

/* --- per-gene negative-binomial dispersion given the means (stand-alone: no engine handle) -----------------------------------
 * The third factor of the model of vc_gene_glm: with eta_c = nu_g . basis[:, c] + logm[c], mu = exp(eta) known, maximise over
 * rho = ln r (r = 1 / dispersion = 1 / shape_inv) the r-dependent log-likelihood of the gene
 *   L(rho) = sum_c lgamma(k + r) - lgamma(r) + k (eta - ln(r + mu)) - r (ln(r + mu) - ln r)         (L + sum_c -lgamma(k + 1) is the whole)
 * plus, with a prior shape_inv ~ Gamma(alpha, beta) (velocity_inference_model.py:383), -(alpha - 1) rho - beta e^-rho: f(rho).
 * One workgroup per gene, one launch, no workspace, no allocation, no synchronisation; asynchronous on hip_stream.  Every pointer is
 * DEVICE memory.  counts_dev, count_kind, Ng, Nc, gene_stride, basis_dev, K, logm_dev: as for vc_gene_glm (counts are taken to be
 * integers; Nc <= 2^31 - 1).
 *   nu_dev          double[Ng][K]: the coefficients (vc_gene_glm's nu_dev)
 *   r_start_dev     float[Ng] or NULL: where the iteration starts; NULL: the moment estimate sum mu^2 / sum((k - mu)^2 - mu)
 *   prior_alpha_dev, prior_beta_dev   both NULL, or double[Ng] each; a gene whose alpha or beta is not a positive finite number has none
 *   tol, max_iter   stop at f'^2 / -f'' <= tol (>= 0) after at most max_iter steps; max_iter == 0 evaluates at r_start_dev only
 * mu is formed exactly as in vc_gene_glm (eta float64, one float32 exp2); everything that depends on r is float64, every sum float64
 * in a fixed order; the gamma terms come from the histogram of the counts (sum_c psi(k + r) - psi(r) = sum_j #{k > j} / (r + j)).
 * rho is confined to [VC_DISP_RHO_MIN, VC_DISP_RHO_MAX] = [ln 1e-3, ln 1e6].  With
 *   noise = 4 eps32 sqrt(sum_c [r mu (k - mu) / (r + mu)^2]^2) + 64 eps64 r sum_c |parts of dL/dr|
 * (what one float32 rounding of mu does to f', and the float64 cancellation of the sum) the status is
 *   VC_DISP_CONVERGED  f'' < 0 and f'^2 / -f'' <= tol
 *   VC_DISP_ROUNDING   |f'| <= noise
 *   VC_DISP_AT_UPPER   f'(VC_DISP_RHO_MAX) > -noise: no detectable overdispersion (decided first)
 *   VC_DISP_AT_LOWER   f'(VC_DISP_RHO_MIN) < noise (decided second)
 *   VC_DISP_MAX_ITER   max_iter steps of the bracketed Newton iteration were taken (Newton step where f'' < 0 and it stays strictly
 *                      inside the sign bracket of f', else its midpoint)
 *   VC_DISP_EVALUATED  max_iter == 0
 *   VC_DISP_NO_DATA    a coefficient of the gene is not finite: every output NaN
 * Outputs per gene, at the last point: rho_dev double[Ng]; r_dev float[Ng] = e^rho rounded (what vc_gene_glm and vc_phase_mle read;
 * evaluate-only: r_start itself); info_dev double[Ng] = -f'' (NaN at a bound); loglik_dev double[Ng] = L without the prior term;
 * score_dev double[Ng] = f'; iterations_dev, status_dev int32[Ng].  A gene's status touches no other gene's outputs; every path is
 * bounded.  VC_ERR_ARG (as vc_gene_glm's, max_iter < 0, one prior pointer without the other, max_iter == 0 without r_start_dev): all
 * decided before anything is launched.  Errors: vc_last_error(NULL). */
#define VC_DISP_RHO_MIN (-6.907755278982137)  /* ln 1e-3 */
#define VC_DISP_RHO_MAX 13.815510557964274    /* ln 1e6 */
#define VC_DISP_CONVERGED 0
#define VC_DISP_ROUNDING 1
#define VC_DISP_AT_UPPER 2
#define VC_DISP_AT_LOWER 3
#define VC_DISP_MAX_ITER 4
#define VC_DISP_EVALUATED 5
#define VC_DISP_NO_DATA 6
int vc_gene_dispersion(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev, int K,
                       const float* logm_dev, const double* nu_dev, const float* r_start_dev, const double* prior_alpha_dev,
                       const double* prior_beta_dev, double tol, int max_iter, double* rho_dev, float* r_dev, double* info_dev,
                       double* loglik_dev, double* score_dev, int32_t* iterations_dev, int32_t* status_dev, void* hip_stream);

/* --- per-gene kinetics of the velocity model given the cycle, the phases and the angular speed (stand-alone: no engine handle) ---
 * The unspliced half of velocity_inference_model.py:360-386 (with_delta_nu=False) solved for x = log gamma_g, y = log beta_g:
 *   etaS = nu_g . basis[:, c] + logm[c]                                        (vc_gene_glm's eta)
 *   d    = sum_h h (nu_sin_h cos h phi - nu_cos_h sin h phi)                   (from the same basis rows)
 *   om   = sum_i nuw[i] w[i][c],   z = om d + e^x,   a = [z > 0],   zp = a z + 1e-5
 *   etaU = etaS - y + ln zp,   mu = e^(etaS - y) zp
 *   L(x, y) = Poisson  sum_c k etaU - mu     NB  sum_c k etaU - (k + r) ln(r + mu) + Nc r ln r          (vc_gene_glm's convention)
 *   f(x, y) = L - (x - mu_gamma)^2 / 2 sd_gamma^2 - (y - mu_beta)^2 / 2 sd_beta^2                       (the model's Normal priors)
 * One workgroup per gene, one launch, no workspace, no allocation, no synchronisation; asynchronous on hip_stream.  Every pointer is
 * DEVICE memory.  counts_dev (the UNSPLICED counts), count_kind, Ng, Nc, gene_stride, basis_dev, logm_dev: as for vc_gene_glm, with
 * K = 2 H + 1 in {3, 5} (H = 0 has no velocity; H = 3 is not instantiated); Nc <= 2^31 - 1.
 *   nu_dev          double[Ng][K]: the cycle's coefficients (vc_gene_glm's nu_dev)
 *   w_dev, NW, nuw_dev   float[NW][Nc] and double[NW], NW in 0..3: the rows of the angular speed's design (condition indicator times
 *                   zeta_omega(phi_c)) and its coefficients, shared by the genes; NW = 0 (both NULL): om = 0
 *   noise, r_dev    as for vc_gene_glm
 *   prior_dev       double[Ng][4]: mu_gamma, sd_gamma, mu_beta, sd_beta (the model's defaults: 0, 0.5, 2, 3)
 *   start_dev       double[Ng][2] or NULL: where the iteration starts; NULL: x = mu_gamma, y = ln(sum_c e^etaS zp / sum_c k)
 *   tol, max_iter   stop at the decrement G' A^-1 G <= tol (>= 0) after at most max_iter steps; max_iter == 0 evaluates at start_dev only
 * etaS, d, om, z and etaS - y are float64 (the set of clamped cells z <= 0 is that of a float64 evaluation of the float32 tables);
 * e^(etaS - y) is formed as vc_gene_glm forms mu (one float32 exp2) and multiplied by zp in float32; the residual, the weights, the
 * NB logarithm and ln zp are float32; every sum is float64 in a fixed order, the 2 x 2 algebra float64: identical bits under
 * repetition, uint16 or float32 storage, and any cutting of the genes into calls.  With g = (p, -1), p = a e^x / zp, the gradient is
 * G = sum_c res g - prior terms (res = k - mu | (k - mu) r / (r + mu)), and a step is A^-1 G with A the observed matrix
 * sum_c wo g g' - [sum_c res p (1 - p)]_xx + diag(1 / sd^2) (wo = mu | mu r (k + r) / (r + mu)^2) where that is positive definite,
 * else the Fisher matrix sum_c w g g' + diag(1 / sd^2) (w = mu | mu r / (r + mu)); (x, y) stays in [-30, 30]^2.  Status per gene:
 *   VC_KIN_CONVERGED  dec <= tol
 *   VC_KIN_ROUNDING   vc_gene_glm's rule on the two gradients: |G_x| <= 4 eps32 sqrt(sum_c (wo^2 + res^2) p^2) and
 *                     |G_y| <= 4 eps32 sqrt(sum_c wo^2 + res^2)
 *   VC_KIN_MAX_ITER   max_iter steps were taken, the gene used up its 30 step halvings (a step is halved while f drops by more than
 *                     its own float32 rounding, 8 eps32 sum |terms|), or the decrement is not finite
 *   VC_KIN_UNBOUNDED  a step would take x or y out of [-30, 30] (a full step of the observed matrix that would is first replaced by
 *                     the Fisher matrix's: a barely positive definite observed matrix is no sign of an unbounded fit); the last point
 *                     inside is kept
 *   VC_KIN_NO_DATA    a coefficient (nu, nuw), a prior or r is not finite (sd, r: or not > 0), a start is not finite, or the gene has
 *                     no count: every output NaN (iterations, n_clamped 0)
 *   VC_KIN_EVALUATED  max_iter == 0
 * Outputs per gene, at the last accepted point:
 *   xy_dev          double[Ng][2]: x, y
 *   cov_dev         double[Ng][3]: A^-1 of the matrix A the decrement there was formed with, packed (xx, yx, yy)
 *   loglik_dev      double[Ng]: L, without the prior term;  dec_dev double[Ng];  iterations_dev int32[Ng]: steps taken
 *   status_dev      int32[Ng];  n_clamped_dev int32[Ng]: the number of cells with z <= 0
 *   score_w_dev     double[Ng][NW]: sum_c res q w[i][c], q = a d / zp -- d f / d nuw_i at the point (NW > 0)
 *   info_w_dev      double[Ng][NW (NW + 1) / 2]: the profile information I_ww - I_wt (I_tt + diag(1 / sd^2))^-1 I_tw of nuw, with
 *                   I = sum_c w g g' over g = (q w[.][c], p, -1), lower triangle packed row by row (NW > 0; one further pass)
 * A gene's status touches no other gene's outputs; every path is bounded.  VC_ERR_ARG (NULL input or output, K not in {3, 5}, NW
 * outside 0..3, NW > 0 without w_dev, nuw_dev, score_w_dev or info_w_dev, NB without r_dev, Nc < 1, Ng < 1, gene_stride < Nc,
 * max_iter < 0, max_iter == 0 without start_dev, tol < 0), VC_ERR_UNSUPPORTED (Lognormal): all decided before anything is launched.
 * Errors: vc_last_error(NULL). */
#define VC_KIN_CONVERGED 0
#define VC_KIN_ROUNDING 1
#define VC_KIN_MAX_ITER 2
#define VC_KIN_UNBOUNDED 3
#define VC_KIN_NO_DATA 4
#define VC_KIN_EVALUATED 5
int vc_gene_kinetics(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev, int K,
                     const float* logm_dev, const double* nu_dev, const float* w_dev, int NW, const double* nuw_dev, int noise,
                     const float* r_dev, const double* prior_dev, const double* start_dev, double tol, int max_iter, double* xy_dev,
                     double* cov_dev, double* loglik_dev, double* dec_dev, int32_t* iterations_dev, int32_t* status_dev,
                     int32_t* n_clamped_dev, double* score_w_dev, double* info_w_dev, void* hip_stream);

/* --- per-gene kinetics with case weights (stand-alone: no engine handle) --------------------------------------------------------
 * vc_gene_kinetics with every cell's contribution multiplied by a weight w_bc >= 0, R rows of weights per call: the step
 * vc_gene_glm_weighted takes from vc_gene_glm (the cell bootstrap of the kinetics fit and of the MAP angular speed; held-out fits).  One
 * workgroup per (gene, row), grid (R, genes) with the row as the fast index, one launch per 65535 genes, no workspace, no allocation, no
 * synchronisation; asynchronous on hip_stream.  counts_dev, count_kind, Ng, Nc, gene_stride, basis_dev, K, logm_dev, w_dev, NW, noise,
 * r_dev, prior_dev, tol, max_iter: as for vc_gene_kinetics.  Every pointer is DEVICE memory.
 *   weights_dev     float: w_bc at index b * weight_stride + c (weight_stride >= Nc; what lies between Nc and the stride is not read).
 *                   Weights are taken to be finite and >= 0 (device memory is not read before the launch)
 *   R               rows of weights, 1..65535 per call
 * Per-row inputs, each with a stride in numbers from one row's table to the next; a stride of 0: one table shared by all rows.
 *   nu_dev, nu_row_stride         double[Ng][K] (0), or double[R][Ng][K] (>= Ng K): a jointly resampled cycle
 *   nuw_dev, nuw_row_stride       double[NW] (0), or double[R][NW] (>= NW): every replicate of an outer iteration at its own nuw
 *   start_dev, start_row_stride   NULL, double[Ng][2] (0), or double[R][Ng][2] (>= 2 Ng): each row starts at its own (x, y)
 * With wt = (double)w_bc every sum of a pass, of the default start's walk and of the profile pass takes its element times wt: res, w and
 * wo of vc_gene_kinetics become wt res, wt w, wt wo in the gradient, both matrices, the score and the information; L = sum_c wt term
 * (the negative binomial's r ln r is inside term and weighted with it), A = sum_c wt mag; the rounding scales are
 * N_x = sum_c ((wt wo)^2 + (wt res)^2) p^2 and N_y = sum_c (wt wo)^2 + (wt res)^2; n_clamped counts the cells with w > 0 and z <= 0;
 * the default start is x = mu_gamma, y = ln(sum_c wt e^etaS zp / sum_c wt k).  The priors are not weighted.  Each product with wt is
 * formed first and is exact at wt == 1; the float64 operations that follow, the fold, the 2 x 2 algebra (observed where positive
 * definite, else Fisher; the Fisher retry for a step out of the box; halving; the [-30, 30]^2 box; VC_KIN_ROUNDING; max_iter;
 * max_iter == 0 -> VC_KIN_EVALUATED) and the status codes are vc_gene_kinetics'.  A row whose sum_c wt k is not a positive finite number
 * (a NaN weight included) ends VC_KIN_NO_DATA with NaN outputs (iterations, n_clamped 0), whatever start_dev holds.
 * Outputs, of row b and gene g at index b * Ng + g:
 *   xy_dev double[R][Ng][2];  cov_dev NULL (not stored) or double[R][Ng][3];  loglik_dev, dec_dev double[R][Ng];
 *   iterations_dev, status_dev, n_clamped_dev int32[R][Ng];  with NW > 0 score_w_dev double[R][Ng][NW] and
 *   info_w_dev double[R][Ng][NW (NW + 1) / 2]
 * Bits: identical under repetition; identical between uint16 and float32 storage; identical under any cutting of the genes or of the
 * rows into calls (row b of an R-row call equals the call on that row alone, with that row's nu, nuw and start); with a table of ones,
 * R = 1 and all strides 0 every one of the eleven outputs equals vc_gene_kinetics' on the same inputs bit for bit.  A (gene, row)
 * pair's status touches no other pair's outputs; every path is bounded.  VC_ERR_ARG / VC_ERR_UNSUPPORTED as vc_gene_kinetics' in its
 * order (cov_dev may be NULL here), then weights_dev NULL, R outside 1..65535, weight_stride < Nc, a non-zero stride smaller than one
 * row's table (nu_row_stride < Ng K, nuw_row_stride < NW, start_row_stride < 2 Ng): all decided before anything is launched.
 * Errors: vc_last_error(NULL). */
int vc_gene_kinetics_weighted(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev,
                              int K, const float* logm_dev, const double* nu_dev, int64_t nu_row_stride, const float* w_dev, int NW,
                              const double* nuw_dev, int64_t nuw_row_stride, int noise, const float* r_dev, const double* prior_dev,
                              const float* weights_dev, int64_t R, int64_t weight_stride, const double* start_dev,
                              int64_t start_row_stride, double tol, int max_iter, double* xy_dev, double* cov_dev, double* loglik_dev,
                              double* dec_dev, int32_t* iterations_dev, int32_t* status_dev, int32_t* n_clamped_dev, double* score_w_dev,
                              double* info_w_dev, void* hip_stream);

/* --- per-cell angular speed of the velocity model given the cycle, the phases and the kinetics (stand-alone: no engine handle) ---
 * vc_gene_kinetics' model with the roles swapped: x_g = log gamma_g and y_g = log beta_g are given, and every cell's angular speed om_c
 * is the one unknown of that cell's unspliced counts (local velocity; any group of cells is fitted by the caller from evaluate-only
 * passes, whose sums add over cells).  Per cell c and gene g:
 *   etaS = nu_g . basis[:, c] + logm[c],   d = sum_h h (nu_sin_h cos h phi - nu_cos_h sin h phi)     (as vc_gene_kinetics)
 *   z = om_c d + e^x_g,   a = [z > 0],   zp = a z + 1e-5,   etaU = etaS - y_g + ln zp,   mu = e^(etaS - y_g) zp,   q = a d / zp
 *   res = k - mu | (k - mu) r / (r + mu)     w = mu | mu r / (r + mu)     wo = mu | mu r (k + r) / (r + mu)^2     (Poisson | NB at r_g)
 *   L_c(om) = sum_g  k etaU - mu  |  k etaU - (k + r) ln(r + mu) + r ln r
 *   score_c = sum_g res q     fisher_c = sum_g w q^2     observed_c = sum_g (wo + res) q^2        (d2 etaU / d om2 = -q^2)
 *   N_c = sum_g (wo^2 + res^2) q^2     A_c = sum_g |terms|     n_clamped_c = #{g : z <= 0}
 *   f_c = L_c - (om - m_c)^2 / 2 s_c^2                                              (the optional Normal prior of the cell)
 * One workgroup per 64 consecutive cells (lane = cell, the waves split the genes in a split that depends on Ng alone), one launch, no
 * workspace, no allocation, no synchronisation; asynchronous on hip_stream.  Every pointer is DEVICE memory.  counts_dev (the UNSPLICED
 * counts, dense [Ng][gene_stride], uint16 or float32), count_kind, Ng, Nc, gene_stride, basis_dev (float[K][Nc]), K in {3, 5},
 * logm_dev, nu_dev, noise, r_dev: as for vc_gene_kinetics; Nc <= 2^31 - 1.
 *   xy_dev          double[Ng][2]: log gamma, log beta of every gene
 *   prior_dev       double[Nc][2]: mean and sd of the cell's Normal prior, or NULL: none
 *   start_dev       double[Nc]: where every cell starts (required; a start outside [-30, 30] is moved to the nearer bound)
 *   tol, max_iter   stop at the decrement G^2 / A <= tol (>= 0) after at most max_iter steps; max_iter == 0 evaluates at start_dev only
 * Arithmetic as vc_gene_kinetics': etaS, d, z and etaS - y float64 from the float32 tables and the float64 parameters (the set of
 * clamped genes is that of a float64 evaluation of the tables); e^(etaS - y) one float32 exp2 (vc_gene_glm's statements); res, w, wo,
 * the NB logarithm and ln zp float32; every sum float64 in a fixed order, no atomics: identical bits under repetition, uint16 or
 * float32 storage, any gene_stride, and any cutting of the cells into calls.  With G = score - (om - m) / s^2 a step is G / A, where
 * A = observed + 1 / s^2 where that is positive, else fisher + 1 / s^2; om stays in [-30, 30].  Status per cell:
 *   VC_CSP_CONVERGED  dec = G^2 / A <= tol
 *   VC_CSP_ROUNDING   |G| <= 4 eps32 sqrt(N)
 *   VC_CSP_MAX_ITER   max_iter steps were taken, the cell used up its 30 step halvings (a step is halved while f drops by more than
 *                     8 eps32 max(A, A')), or the decrement is not finite
 *   VC_CSP_UNBOUNDED  a full step would take om out of [-30, 30]; the last point inside is kept
 *   VC_CSP_NO_DATA    the cell has no count, its start is not finite, or its prior is not finite (sd: or not > 0): every
 *                     floating-point output NaN, iterations and n_clamped 0
 *   VC_CSP_EVALUATED  max_iter == 0
 * Outputs per cell, at the last accepted point:
 *   omega_dev       double[Nc]
 *   var_dev         double[Nc]: 1 / A of the A the decrement there was formed with
 *   sums_dev        double[Nc][6]: L, score (without the prior term), fisher, observed, N, A
 *   dec_dev double[Nc];  iterations_dev int32[Nc]: steps taken;  status_dev int32[Nc];  n_clamped_dev int32[Nc]
 * A cell's status touches no other cell's outputs; every path is bounded (a workgroup makes at most max_iter + 31 passes).
 * VC_ERR_ARG (NULL input or output, start_dev NULL, K not in {3, 5}, NB without r_dev, Nc < 1, Ng < 1, gene_stride < Nc, max_iter < 0,
 * tol < 0), VC_ERR_UNSUPPORTED (Lognormal): all decided before anything is launched.  Errors: vc_last_error(NULL). */
#define VC_CSP_CONVERGED 0
#define VC_CSP_ROUNDING 1
#define VC_CSP_MAX_ITER 2
#define VC_CSP_UNBOUNDED 3
#define VC_CSP_NO_DATA 4
#define VC_CSP_EVALUATED 5
int vc_cell_speed(const void* counts_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride, const float* basis_dev, int K,
                  const float* logm_dev, const double* nu_dev, const double* xy_dev, int noise, const float* r_dev,
                  const double* prior_dev, const double* start_dev, double tol, int max_iter, double* omega_dev, double* var_dev,
                  double* sums_dev, double* dec_dev, int32_t* iterations_dev, int32_t* status_dev, int32_t* n_clamped_dev,
                  void* hip_stream);

/* --- joint per-gene fit of the harmonics and the kinetics over both layers (stand-alone: no engine handle) -----------------------
 * velocity_inference_model.py:360-386 (with_delta_nu=False) with the phases and the angular speed known, solved per gene for
 * theta = (nu [K], x = log gamma, y = log beta) from one row of spliced and one row of unspliced counts: vc_gene_glm and
 * vc_gene_kinetics in one problem, in which nu also sees the unspliced layer (through etaS and through d inside the relu).  With
 * b = basis[:, c], db its phi-derivative from the same rows (db_0 = 0, db_{2h-1} = h b_{2h}, db_{2h} = -h b_{2h-1}):
 *   etaS = nu . b + logm[c],   d = nu . db,   om = sum_i nuw[i] w[i][c],   z = om d + e^x,   a = [z > 0],   zp = a z + 1e-5
 *   etaU = etaS - y + ln zp,   muS = e^etaS,   muU = e^(etaS - y) zp
 *   L_S, L_U = Poisson  sum_c k eta - mu     NB  sum_c k eta - (k + r) ln(r + mu) + Nc r ln r   (vc_gene_glm's convention; one r per gene)
 *   f = L_S + L_U - (theta - m)' Lambda (theta - m) / 2     (Lambda diagonal: nu's from the two tables, x's and y's from prior_dev)
 * One workgroup per gene, one launch, no workspace, no allocation, no synchronisation; asynchronous on hip_stream.  Every pointer is
 * DEVICE memory.
 *   counts_s_dev, counts_u_dev   the SPLICED and the UNSPLICED counts, each dense [Ng][gene_stride] of the same count_kind
 *   count_kind, Ng, Nc, gene_stride, basis_dev, K, logm_dev, w_dev, NW, nuw_dev, noise, r_dev   as for vc_gene_kinetics (K in {3, 5},
 *                   NW in 0..3, Nc <= 2^31 - 1)
 *   prior_mean_dev, prior_prec_dev   double[Ng][K] each, as vc_gene_glm takes them, but REQUIRED here (without a prior on nu a gene with
 *                   few cells has no maximum): every mean finite, every precision a positive finite number
 *   prior_dev       double[Ng][4]: mu_gamma, sd_gamma, mu_beta, sd_beta (vc_gene_kinetics')
 *   start_dev       double[Ng][K + 2] or NULL.  A gene whose start has an entry that is not finite or lies outside the box takes the
 *                   default start, which is also NULL's: nu_0 = ln(sum_c k_S / sum_c e^logm), the harmonics at their prior means,
 *                   x = mu_gamma, y = ln(sum_c e^etaS zp / sum_c k_U), clipped to the box
 *   tol, max_iter   stop at the decrement G' A^-1 G <= tol (>= 0) after at most max_iter steps; max_iter == 0 evaluates at the start only
 * Arithmetic as vc_gene_kinetics': etaS, d, om, z and etaS - y float64 from the float32 tables and the float64 parameters; e^etaS and
 * e^(etaS - y) one float32 exp2 each; residuals, weights, the NB logarithm and ln zp float32; every sum float64 in a fixed order, the
 * (K + 2)-dimensional algebra float64 (packed Cholesky).  With s = a om / zp, p = a e^x / zp, u = (s db, p, 0), gS = (b, 0, 0) and
 * gU = (b + s db, p, -1):
 *   G = sum_c resS gS + resU gU - Lambda (theta - m)
 *   O = sum_c woS gS gS' + woU gU gU' + resU u u' - [sum_c resU p]_xx + Lambda     (observed)
 *   F = sum_c wS gS gS' + wU gU gU' + Lambda                                       (Fisher, always positive definite)
 *   N_i = sum_c (woS^2 + resS^2) gS_i^2 + (woU^2 + resU^2) gU_i^2                  (rounding scale of G_i)
 * A step is A^-1 G with A = O where its Cholesky factorisation succeeds, else F (formed in a pass of its own, only then); nu stays
 * in [-50, 50]^K, x and y in [-30, 30].  Status per gene (numbered like VC_KIN_*):
 *   VC_JNT_CONVERGED  dec <= tol
 *   VC_JNT_ROUNDING   every |G_i| <= 4 eps32 sqrt(N_i)
 *   VC_JNT_MAX_ITER   max_iter steps were taken, the gene used up its 30 step halvings (a step is halved while f drops by more than
 *                     8 eps32 max(sum |terms|, sum |terms|')), or the decrement is not finite
 *   VC_JNT_UNBOUNDED  a full step would leave the box (one taken with O is first replaced by F's); the last point inside is kept
 *   VC_JNT_NO_DATA    a prior, nuw or r is not finite (precision, sd, r: or not > 0), or a layer of the gene has no count: every
 *                     floating-point output NaN, iterations and n_clamped 0
 *   VC_JNT_EVALUATED  max_iter == 0
 * Outputs per gene, at the last accepted point:
 *   theta_dev       double[Ng][K + 2]: nu, x, y
 *   cov_dev         double[Ng][(K + 2)(K + 3) / 2]: A^-1 of the matrix A the decrement there was formed with, lower triangle packed
 *                   row by row like vc_gene_glm's
 *   loglik_s_dev, loglik_u_dev   double[Ng]: L_S and L_U, without the prior terms;  dec_dev double[Ng]
 *   iterations_dev int32[Ng]: steps taken;  status_dev int32[Ng];  n_clamped_dev int32[Ng]: the number of cells with z <= 0
 *   score_w_dev     double[Ng][NW]: sum_c resU q w[i][c], q = a d / zp (NW > 0)
 *   info_w_dev      double[Ng][NW (NW + 1) / 2]: I_ww - I_wt (I_tt + Lambda)^-1 I_tw with I the Fisher information over
 *                   (q w[.][c], gU) for the unspliced plus gS for the spliced layer, t = all K + 2 parameters (NW > 0; one further pass)
 * Bits: identical under repetition, uint16 or float32 storage, any gene_stride and any cutting of the genes into calls; at
 * max_iter == 0 loglik_u_dev and n_clamped_dev equal vc_gene_kinetics' evaluate-only outputs at the same (nu, x, y, w, nuw).  A gene's
 * status touches no other gene's outputs; every path is bounded.  VC_ERR_ARG (NULL input or output, the nu prior tables included; K
 * not in {3, 5}; NW outside 0..3; NW > 0 without w_dev, nuw_dev, score_w_dev or info_w_dev; score_w_dev or info_w_dev with NW == 0; NB
 * without r_dev; Nc < 1, Ng < 1, gene_stride < Nc, max_iter < 0, max_iter == 0 without start_dev, tol < 0), VC_ERR_UNSUPPORTED
 * (Lognormal): all decided before anything is launched.  Errors: vc_last_error(NULL). */
#define VC_JNT_CONVERGED 0
#define VC_JNT_ROUNDING 1
#define VC_JNT_MAX_ITER 2
#define VC_JNT_UNBOUNDED 3
#define VC_JNT_NO_DATA 4
#define VC_JNT_EVALUATED 5
int vc_gene_joint(const void* counts_s_dev, const void* counts_u_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride,
                  const float* basis_dev, int K, const float* logm_dev, const float* w_dev, int NW, const double* nuw_dev, int noise,
                  const float* r_dev, const double* prior_mean_dev, const double* prior_prec_dev, const double* prior_dev,
                  const double* start_dev, double tol, int max_iter, double* theta_dev, double* cov_dev, double* loglik_s_dev,
                  double* loglik_u_dev, double* dec_dev, int32_t* iterations_dev, int32_t* status_dev, int32_t* n_clamped_dev,
                  double* score_w_dev, double* info_w_dev, void* hip_stream);

/* --- joint per-gene fit with case weights (stand-alone: no engine handle) ---------------------------------------------------------
 * vc_gene_joint with every cell's contribution multiplied by a weight w_bc >= 0, R rows of weights per call: the step
 * vc_gene_kinetics_weighted takes from vc_gene_kinetics (the cell bootstrap of the joint fit and of its MAP angular speed; held-out
 * fits).  One workgroup per (gene, row), grid (R, genes) with the row as the fast index, one launch per 65535 genes, no workspace, no
 * allocation, no synchronisation; asynchronous on hip_stream.  counts_s_dev, counts_u_dev, count_kind, Ng, Nc, gene_stride, basis_dev,
 * K, logm_dev, w_dev, NW, noise, r_dev, prior_mean_dev, prior_prec_dev, prior_dev, tol, max_iter: as for vc_gene_joint (the priors are
 * shared by the rows and are not weighted; there is no nu table: nu is an unknown here).  Every pointer is DEVICE memory.
 *   weights_dev     float: w_bc at index b * weight_stride + c (weight_stride >= Nc; what lies between Nc and the stride is not read).
 *                   Weights are taken to be finite and >= 0 (device memory is not read before the launch)
 *   R               rows of weights, 1..65535 per call
 * Per-row inputs, each with a stride in numbers from one row's table to the next; a stride of 0: one table shared by all rows.
 *   nuw_dev, nuw_row_stride       double[NW] (0), or double[R][NW] (>= NW): every replicate of an outer iteration at its own nuw
 *   start_dev, start_row_stride   NULL, double[Ng][K + 2] (0), or double[R][Ng][K + 2] (>= Ng (K + 2)): each row starts at its own theta
 *                                 (a pair whose start has an entry that is not finite or lies outside the box takes the default start)
 * With wt = (double)w_bc every sum of a regular pass, of the Fisher pass, of the default start's walk and of the profile pass takes its
 * element times wt: res, w and wo of both layers become wt res, wt w, wt wo in G, O, F, the score and the information; L_S and L_U are
 * sum_c wt term (the negative binomial's r ln r is inside term and weighted with it); the halving allowance uses A = sum_c wt |terms|;
 * the rounding scales are N_i = sum_c ((wt woS)^2 + (wt resS)^2) gS_i^2 + ((wt woU)^2 + (wt resU)^2) gU_i^2; n_clamped counts the
 * cells with w > 0 and z <= 0; the default start is nu_0 = ln(sum_c wt k_S / sum_c wt e^logm), y = ln(sum_c wt e^etaS zp / sum_c wt k_U).
 * Each product with wt is formed first and is exact at wt == 1; the float64 operations that follow, the fold, the packed Cholesky
 * algebra (observed where its factorisation succeeds, else Fisher from a pass of its own; the Fisher retry for a step out of the box;
 * halving; the boxes; VC_JNT_ROUNDING; max_iter; max_iter == 0 -> VC_JNT_EVALUATED) and the status codes are vc_gene_joint's.  A
 * (gene, row) pair whose sum_c wt k_S or sum_c wt k_U is not a positive finite number (a NaN weight included) ends VC_JNT_NO_DATA with
 * NaN outputs (iterations, n_clamped 0), whatever start_dev holds.
 * Outputs, of row b and gene g at index b * Ng + g:
 *   theta_dev double[R][Ng][K + 2];  cov_dev NULL (not stored) or double[R][Ng][(K + 2)(K + 3) / 2];
 *   loglik_s_dev, loglik_u_dev, dec_dev double[R][Ng];  iterations_dev, status_dev, n_clamped_dev int32[R][Ng];
 *   with NW > 0 score_w_dev double[R][Ng][NW] and info_w_dev double[R][Ng][NW (NW + 1) / 2]
 * Bits: identical under repetition; identical between uint16 and float32 storage; identical under any gene_stride and weight_stride and
 * any cutting of the genes or of the rows into calls (row b of an R-row call equals the call on that row alone, with that row's nuw and
 * start); with a table of ones, R = 1 and all strides 0 every one of vc_gene_joint's outputs is reproduced bit for bit.  A (gene, row)
 * pair's status touches no other pair's outputs; every path is bounded.  VC_ERR_ARG / VC_ERR_UNSUPPORTED as vc_gene_joint's in its
 * order (cov_dev may be NULL here), then weights_dev NULL, R outside 1..65535, weight_stride < Nc, a non-zero stride smaller than one
 * row's table (nuw_row_stride < NW, start_row_stride < Ng (K + 2)): all decided before anything is launched.
 * Errors: vc_last_error(NULL). */
int vc_gene_joint_weighted(const void* counts_s_dev, const void* counts_u_dev, int count_kind, int64_t Ng, int64_t Nc, int64_t gene_stride,
                           const float* basis_dev, int K, const float* logm_dev, const float* w_dev, int NW, const double* nuw_dev,
                           int64_t nuw_row_stride, int noise, const float* r_dev, const double* prior_mean_dev,
                           const double* prior_prec_dev, const double* prior_dev, const float* weights_dev, int64_t R,
                           int64_t weight_stride, const double* start_dev, int64_t start_row_stride, double tol, int max_iter,
                           double* theta_dev, double* cov_dev, double* loglik_s_dev, double* loglik_u_dev, double* dec_dev,
                           int32_t* iterations_dev, int32_t* status_dev, int32_t* n_clamped_dev, double* score_w_dev, double* info_w_dev,
                           void* hip_stream);

/* --- PCA phase prior (Phases.from_pca_heuristic, phases.py:307-382): staging and the power iteration's pass ------------------
 * Stand-alone (no engine); the iteration itself (QR, Rayleigh-Ritz on 8 x 8 matrices, float64) is the caller's:
 * velocycle_amd/phase_prior.py.  Both calls only enqueue on hip_stream.  Errors: vc_last_error(NULL).
 *
 * vc_pca_stage: for cells [0, n_cells) of a dense block, X[c][g] = float32(log(raw[c][g] + small_count)) (a logarithm correct to
 * 1 ulp), and colsum[g] += sum_c X[c][g] in float64: one partial per (64-cell tile, gene) summed in cell order, then added to
 * colsum_dev in tile order -- a matrix staged in several calls cut at multiples of 64 cells gives the bits of one call.
 *   raw_dev      float[n_cells][raw_stride] (raw_stride >= Ng);  X_dev: float[n_cells][x_stride] (x_stride >= Ng), the caller
 *                passes the address of the block's first row inside the whole staged matrix
 *   colsum_dev   double[Ng], zeroed by the caller before the first block;  partial_dev: double[ceil(n_cells / 64)][Ng] scratch
 *   flag_dev     int32, zeroed by the caller: set to 1 (never cleared) when a staged value is not finite (v + small_count <= 0,
 *                or v not finite)
 * vc_pca_apply: Y = (X - mu) Q, float[Nc][8], and Z = (X - mu)^T Y, double[Ng][8], with X read from memory once.
 *   mu_dev       float[Ng];  Q_dev: float[Ng][8], 16-byte aligned
 *   ws_dev       float[ws_floats] scratch, 16-byte aligned, ws_floats >= vc_pca_apply_workspace(Nc, Ng, max_workgroups)
 *                (= workgroups x Ng x 8)
 *   max_workgroups  bound of the persistent workgroups, each of which walks ceil(tiles / workgroups) consecutive 64-cell tiles;
 *                0 (or anything outside 1..512): 512.  It sets the size of the workspace and the order of Z's sums
 * Sums: float32 fma chains per lane (Y: Ng / 64 terms, then a fixed tree over the 64 lanes; Z: the cells of one workgroup, at
 * least 64), the workgroups' rows added in workgroup order in float64.  No atomics: bit-identical on repetition.  Any Nc >= 1,
 * Ng >= 1, x_stride >= Ng. */
int vc_pca_stage(const float* raw_dev, int64_t n_cells, int64_t Ng, int64_t raw_stride, float small_count, float* X_dev,
                 int64_t x_stride, double* colsum_dev, double* partial_dev, int32_t* flag_dev, void* hip_stream);
int64_t vc_pca_apply_workspace(int64_t Nc, int64_t Ng, int max_workgroups);
int vc_pca_apply(const float* X_dev, int64_t Nc, int64_t Ng, int64_t x_stride, const float* mu_dev, const float* Q_dev,
                 float* Y_dev, double* Z_dev, float* ws_dev, int64_t ws_floats, int max_workgroups, void* hip_stream);

/* --- pointwise predictive density over posterior draws (lppd, WAIC) -------------------------------------------------------
 * The reference has no function for it (on its stack: Predictive + one traced model run per draw and a [D][Ng][Nc] tensor of
 * log-probs); the quantity is defined by the reference's own model code (velocity_inference_model.py:338-386,
 * phase_inference_model.py:343-395).  For draw d (site values as vc_sample_posterior delivers them), gene g, cell c:
 *   eta_S = nu_d[g,:] . zeta(phi_dc) + sum_b Db[b,c] dnu[b,g] + count_factor[c]
 *   omega = sum_x sum_h nuomega_d[x,h] zeta_omega_h(phi_dc) D[x,c]                                             (velocity)
 *   z     = (nu_d[g,:] . zeta'(phi_dc)) omega + exp(loggamma_d[g]);  eta_U = -logbeta_d[g] + log(relu(z) + 1e-5) + eta_S
 *   NegativeBinomial  l(k; r, eta) = lgamma(r+k) - lgamma(r) - lgamma(k+1) + r log r + k eta - (r+k) log(r + e^eta),  r = 1 / shape_inv[g]
 *   Poisson           l(k; eta)    = k eta - e^eta - lgamma(k+1)
 * phi_dc = the angle of the draw's phixy (the basis is formed from the direction, not from the rounded angle).  Per count matrix
 * M (S; velocity: S then U) and element:
 *   lppd = log((1/D) sum_d exp l_d)      mean = (1/D) sum_d l_d      pwaic = sum_d (l_d - mean)^2 / (D - 1)
 * Outputs (DEVICE float64), quantity q = 3 M + {0 lppd, 1 mean, 2 pwaic}:
 *   gene_out_dev [3 nmat][Ng]        sums over the cells [cell_begin, cell_begin + cell_count), ADDED to what the buffer holds (zero it
 *                                    before the first call over a set of cells; cut into calls in ascending cell order)
 *   cell_out_dev [3 nmat][Nc_local]  sums over the genes, written for the cells of the call, in the caller's cell order
 *   dense_lppd_dev  NULL, or float[nmat][Ng][Nc_local]: lppd per element, written for the cells of the call
 * Inputs: every pointer is DEVICE memory, draw-major float[n_draws][length of the site] with a draw stride in floats that is the
 * site's length, or 0 for a site that is the same in every draw (conditioned: hand over one copy).  dnu (Delta site) and shape_inv
 * (Delta site) cannot vary over draws in this model and have no stride; dnu is NULL without batch offsets, shape_inv for Poisson,
 * loggamma / logbeta / nuomega for the phase model.  With phixy_stride == 0 and nu_stride == 0 (the tutorials' velocity stage)
 * the S matrix is evaluated once: its pwaic is exactly 0 and its lppd equals its mean.
 * The counts are read where vc_finalize put them; the only workspaces are one float64 per histogram entry (the lgamma terms:
 * formed once per distinct (gene, count) pair in float64, never per draw) and [min(512, ceil(Nc_local / 64))][3 nmat][Ng] float64
 * of per-gene partial rows, both kept by the engine from the first call on.  All sums are float64 in a fixed order, no atomics:
 * two calls give the same bits, and so does any cutting of the cells into calls whose cell_begin is a multiple of 64.
 * Asynchronous on hip_stream; one call at a time per engine.  Supported: what the compiled fast kernel set covers (both models and
 * guides, NegativeBinomial and Poisson, H 1..3, Hw 0..3, any one-hot batches, the dense design up to 4).  VC_ERR_UNSUPPORTED (with
 * the reason in vc_last_error) for Lognormal noise and the run-time-sized configurations; VC_ERR_ARG for a NULL engine (message:
 * vc_last_error(NULL)), n_draws < 2, a NULL output or input, a stride or cell range out of bounds; VC_ERR_STATE before vc_finalize:
 * all decided before anything is launched. */
int vc_pointwise_density(vc_engine* e, int64_t n_draws, const float* phixy, int64_t phixy_stride, const float* nu, int64_t nu_stride,
                         const float* dnu, const float* shape_inv, const float* loggamma, int64_t loggamma_stride, const float* logbeta,
                         int64_t logbeta_stride, const float* nuomega, int64_t nuomega_stride, int64_t cell_begin, int64_t cell_count,
                         double* gene_out_dev, double* cell_out_dev, float* dense_lppd_dev, void* hip_stream);

/* --- device count sampler (stand-alone: no engine handle) ------------------------------------------------------------------
 * k ~ Poisson(mu) (shape_inv_dev == NULL) or k ~ GammaPoisson(r, r / mu), r = 1 / shape_inv (the reference's negative binomial,
 * velocity_inference_model.py:385-386, phase_inference_model.py), mu = exp(eta), for every element of eta_dev[n_rows][n_cols]
 * (float32, natural log); shape_inv_dev holds one value per ROW.  Exact algorithms (no normal approximation): Marsaglia-Tsang gamma
 * on polar normals with the u^(1/r) boost below r = 1, inversion by sequential search below a rate of 10, Hoermann's PTRS from there
 * on.  Counter based: the count of element (i, j) is a pure function of
 *   (seed, draw, matrix, index_origin + i * row_index_stride + j, eta, shape_inv)
 * through Philox4x32-10 blocks (counter: index low, index high, draw, matrix << 16 | stage << 8 | attempt; key: seed), whatever the
 * launch shape or the cutting into calls.  vc_predictive_check draws element (gene g, global cell c) of count matrix m under draw d
 * at index g << 32 | c, matrix m, draw d.  Supported range: rates (after the gamma mixing) in [0, 2^20], shape_inv > 0.  An element
 * outside it, or a rejection loop out of its 64 attempts, is stored as -1 and the call returns VC_ERR_RANGE: no value is made up.
 * out_dev: int32[n_rows][n_cols].  draw in [0, 2^32), matrix in [0, 65536).  Synchronises hip_stream.  Errors: vc_last_error(NULL). */
int vc_sample_counts(const float* eta_dev, int64_t n_rows, int64_t n_cols, const float* shape_inv_dev, uint64_t seed, int64_t draw,
                     int matrix, int64_t index_origin, int64_t row_index_stride, int32_t* out_dev, void* hip_stream);

/* --- posterior predictive check: replicated counts over posterior draws, reduced to statistics ------------------------------
 * On the reference's stack: Predictive with the observations removed and [D][Ng][Nc] count tensors per matrix
 * (velocity_inference_model.py:338-386, phase_inference_model.py:343-395 define the likelihood).  For draw d, count matrix m (S;
 * velocity: S then U), gene g, cell c the replicate k_rep ~ the model's likelihood at eta_S / eta_U of vc_pointwise_density, drawn
 * by the sampler of vc_sample_counts at index g << 32 | (cell_offset + c).  Draw pointers and strides as vc_pointwise_density.
 * The call covers cells [cell_begin, cell_begin + cell_count) and draws [draw_begin, draw_begin + draw_count) of n_draws.  Outputs (DEVICE):
 *   gene_rep_dev int64[n_draws][nmat][4][Ng]    sum k, sum k^2, #{k = 0}, max k over the call's cells, ADDED (max: maxed) into what the
 *                                               buffer holds: zero it before the first call
 *   cell_rep_dev int64[n_draws][nmat][Nc_local] sum k over the genes (the replicated library size), written for the call's cells and draws
 *   gene_obs_dev double[nmat][4][Ng], cell_obs_dev double[nmat][Nc_local]: the same statistics of the engine's stored counts over the
 *                                               call's cells (gene rows continued from what the buffer holds); both NULL: skipped (hand
 *                                               them over with ONE of the draw ranges a set of cells is visited with)
 *   keep_dev     NULL, or int32[n_keep][nmat][Ng][Nc_local]: the replicates of the draws < n_keep
 * Replicate statistics are integers accumulated with 64-bit integer atomics; the observed ones are float64 sums in a fixed order: all
 * of them are bit-identical under any cutting of cells and draws into calls, uint16 or float32 count storage, interleaved batches and
 * repetition.  No workspace.  Synchronises hip_stream.  VC_ERR_UNSUPPORTED for Lognormal noise and the run-time-sized configurations,
 * VC_ERR_ARG / VC_ERR_STATE as vc_pointwise_density (n_draws >= 1 here), all before anything is launched; VC_ERR_RANGE when a replicate
 * left the sampler's range: latched in the engine (vc_get_status reports it too) until vc_clear_status. */
int vc_predictive_check(vc_engine* e, int64_t n_draws, const float* phixy, int64_t phixy_stride, const float* nu, int64_t nu_stride,
                        const float* dnu, const float* shape_inv, const float* loggamma, int64_t loggamma_stride, const float* logbeta,
                        int64_t logbeta_stride, const float* nuomega, int64_t nuomega_stride, uint64_t seed, int64_t cell_begin,
                        int64_t cell_count, int64_t draw_begin, int64_t draw_count, int64_t* gene_rep_dev, int64_t* cell_rep_dev,
                        double* gene_obs_dev, double* cell_obs_dev, int32_t* keep_dev, int64_t n_keep, void* hip_stream);

/* --- predictive PIT: randomized quantile residuals of every observed count over posterior draws ------------------------------
 * No counterpart in the reference (Predictive plus a [D][Ng][Nc] CDF tensor per matrix would be it); the likelihood is the one of
 * velocity_inference_model.py:338-386, phase_inference_model.py:343-395.  For count matrix m (S; velocity: S then U), gene g, cell c
 * with the observed integer count k, under the draws theta_d:
 *   F_lo = (1/D) sum_d P(K <= k - 1 | theta_d)      F_hi = (1/D) sum_d P(K <= k | theta_d)      u = F_lo + v (F_hi - F_lo)
 * K ~ Poisson(mu) or GammaPoisson(r, r / mu), r = 1 / shape_inv[g], mu = exp(eta_S | eta_U) of vc_pointwise_density; v is the uniform
 * of word 0 of the Philox4x32-10 block of vc_sample_counts at index g << 32 | (cell_offset + c), draw 0, matrix m, stage 2 (stages 0
 * and 1 are the sampler's gamma and Poisson variates), attempt 0.  u is one float32 fma, clamped to [0, 1); its bin is
 * min(n_bins - 1, floor(u n_bins)).  u is a pure function of (seed, m, g, global cell) and the draws (Dunn & Smyth 1996): uniform under
 * a calibrated fit, U-shaped histograms under an under-dispersed model, hump-shaped under an over-dispersed one, skewed under bias.
 * Draw pointers and strides as vc_pointwise_density (n_draws >= 1 here).  Outputs (DEVICE):
 *   gene_hist_dev int64[nmat][Ng][n_bins]        bins of u over the cells [cell_begin, cell_begin + cell_count), ADDED to what the buffer
 *                                                holds: zero it before the first call over a set of cells
 *   cell_hist_dev int64[nmat][Nc_local][n_bins]  bins of u over the genes, written for the cells of the call
 *   dense_dev     NULL, or float[nmat][3][Ng][Nc_local]: F_lo, F_hi and u per element, written for the cells of the call
 * The CDF is the lower tail summed downward from k relative to pmf(k), rescaled so that no count of the upper tail overflows; every
 * element comes out with 0 <= F_lo <= F_hi <= 1.  The loop is at most k long (it stops past the mode once the geometric bound of the
 * remaining terms is below 2^-26 of the sum).  All sums are integers (LDS and 64-bit global integer atomics): identical bits under any cutting of the cells into calls
 * (no alignment is asked of cell_begin), uint16 or float32 count storage, interleaved batches and repetition.  Workspace: the
 * histogram tables of vc_pointwise_density (one float64 per distinct (gene, count) pair), shared with it.  Asynchronous on hip_stream;
 * one call at a time per engine.  Supported: what vc_pointwise_density supports, COUNTS THAT ARE INTEGERS BELOW 2^24 (float32 holds every
 * integer only up to there), rates that are finite, shape_inv < 2^30, n_bins in [2, 64].  VC_ERR_UNSUPPORTED (with the reason in
 * vc_last_error) for Lognormal noise, the run-time-sized configurations and an engine that holds non-integer counts (they have no CDF
 * on the integers) or a count of 2^24 or more; VC_ERR_ARG for a NULL engine (message: vc_last_error(NULL)),
 * n_draws < 1, n_bins out of range, a NULL table or input, a stride or cell range out of bounds; VC_ERR_STATE before vc_finalize: all
 * decided before anything is launched. */
int vc_predictive_pit(vc_engine* e, int64_t n_draws, const float* phixy, int64_t phixy_stride, const float* nu, int64_t nu_stride,
                      const float* dnu, const float* shape_inv, const float* loggamma, int64_t loggamma_stride, const float* logbeta,
                      int64_t logbeta_stride, const float* nuomega, int64_t nuomega_stride, uint64_t seed, int32_t n_bins,
                      int64_t cell_begin, int64_t cell_count, int64_t* gene_hist_dev, int64_t* cell_hist_dev, float* dense_dev,
                      void* hip_stream);

/* --- phase-marginal scoring: per-cell phase posterior and evidence on a grid of phases -------------------------------------------
 * The Bayesian twin of Phases.from_cycle_mle (phases.py:471-509), which scores the spliced matrix at point estimates with one
 * dispersion and keeps the arg-max bin.  Here, for cell c, draw d of the gene-level and global sites theta_d = (nu, dnu, shape_inv,
 * loggamma, logbeta, nuomega) and grid phase phi_j = 2 pi j / n_bins (the grid of phases.py:495), with the likelihood of
 * velocity_inference_model.py:338-386, phase_inference_model.py:343-395 (eta_S, eta_U, lgamma terms as vc_pointwise_density) evaluated
 * with the cell's direction set to phi_j:
 *   a[d,c,j]      = lw[c,j] + sum_matrices sum_g log p(k_gc | theta_d, phi_j)
 *   evidence[c]   = log((1/D) sum_d sum_j exp a[d,c,j])             the cell's log predictive density with the phase integrated out
 *   post[c,j]     = sum_d exp a[d,c,j] / sum_d sum_j' exp a[d,c,j']  the phase posterior on the grid (rows sum to 1)
 *   per_draw[d,c] = log sum_j exp a[d,c,j]
 * lw[c,j] is the log prior mass of bin j (sum_j exp lw = 1 is the caller's business): log_prior_dev float[Nc_local][n_bins], or NULL
 * for the flat prior, whose lw is -log(n_bins) rounded to float32 (a table of that value gives the bits of NULL).  The engine holds
 * the cells to be scored -- they need not be cells any fit has seen -- and no phixy is read.  Draw pointers and strides as
 * vc_pointwise_density WITHOUT phixy; n_draws in [1, 2^20], n_bins in [2, 4096].  When nu_stride is 0 the spliced sums of a (cell, bin)
 * are formed once instead of per draw, by the same statements: the bits do not depend on it.  Outputs (DEVICE, written for the cells
 * [cell_begin, cell_begin + cell_count)):
 *   evidence_dev  double[Nc_local]
 *   post_dev      NULL, or float[Nc_local][n_bins]
 *   per_draw_dev  NULL, or double[n_draws][Nc_local]
 * One kernel (csrc/vc_phase_marginal.hip): lane = cell, float32 partial sums of 4 genes into float64 accumulators per (cell, bin),
 * the lgamma constants summed once per cell in float64 from the histogram tables of vc_pointwise_density, an online log-sum-exp in
 * float64 over bins and draws; no atomics.  Finite a, however negative, give finite outputs.  Identical bits under repetition, any
 * cutting of the cells into calls (no alignment is asked of cell_begin), uint16 or float32 count storage, interleaved batches and
 * sharding.  For the velocity model the integrand is not smooth in phi (the relu(z) + 1e-5 floor): the evidence is that of the
 * discrete grid.  Workspace (engine-owned, allocated at the first call, again when a call needs more): the grid's sin / cos table,
 * 32 n_bins bytes, and the bins' log masses of one launch, 8 n_bins min(cells of the call rounded up to 64, max(64, 2^23 / n_bins
 * rounded down to 64)) bytes <= 64 MiB; a call of more cells is cut into launches.  Asynchronous on hip_stream; one call at a time
 * per engine.  VC_ERR_UNSUPPORTED (with the reason in vc_last_error) for Lognormal noise and the run-time-sized configurations;
 * VC_ERR_ARG for a NULL engine (message: vc_last_error(NULL)), n_draws or n_bins out of range, a NULL evidence_dev or input, a stride
 * or cell range out of bounds; VC_ERR_STATE before vc_finalize: all decided before anything is launched. */
int vc_phase_marginal(vc_engine* e, int64_t n_draws, const float* nu, int64_t nu_stride, const float* dnu, const float* shape_inv,
                      const float* loggamma, int64_t loggamma_stride, const float* logbeta, int64_t logbeta_stride,
                      const float* nuomega, int64_t nuomega_stride, int32_t n_bins, const float* log_prior_dev, int64_t cell_begin,
                      int64_t cell_count, double* evidence_dev, float* post_dev, double* per_draw_dev, void* hip_stream);

/* introspection ----------------------------------------------------------------------------- */
/* Copies the value a site took in the last vc_elbo_grad to host memory (synchronises the stream). */
int vc_read_site(vc_engine* e, int site, float* host_out, int64_t n, void* hip_stream);
int vc_get_stats(const vc_engine* e, vc_stats* out);
/* The per-gene count histograms vc_finalize built (CSR over [S genes..., U genes...]: ptr int32[2*Ng + 1], distinct
 * non-zero count values and their multiplicities) -- the sufficient statistic of the negative binomial's lgamma /
 * digamma terms.  Pass NULL arrays to query *n_entries first.  Lets tests hold the device-built histograms against the
 * host pass (vc_tuning.host_hist). */
int vc_get_histogram(const vc_engine* e, int64_t* n_entries, int32_t* ptr_out, float* val_out, float* cnt_out);
/* Failure detection (the reference's counterpart: pyro.util.warn_if_nan(loss, "loss") inside SVI.step, call sites
 * phase_inference_model.py:169 / velocity_inference_model.py:120).  The last kernel of every step checks this rank's
 * loss on the device and latches the first step whose loss was NaN / Inf, so the check costs no host round trip per
 * step.  Synchronises `hip_stream`, returns VC_OK, or VC_ERR_NONFINITE with *first_bad_step (may be NULL) = the
 * 0-based index of the first such step and *n_bad (may be NULL) = how many steps were affected since vc_finalize /
 * the last vc_clear_status. */
int vc_get_status(vc_engine* e, int64_t* first_bad_step, int64_t* n_bad, void* hip_stream);
int vc_clear_status(vc_engine* e, void* hip_stream);
/* Kernel timing for bench.py's roofline: while enabled, every vc_elbo_grad brackets the likelihood
 * kernel with a pair of hipEvents recorded on the launch stream (not capturable into a hipGraph).
 * vc_get_timing synchronises the pending events and returns the accumulated duration (ms) and the
 * number of launches since timing was enabled. */
/* Shader clock the device is running at right now, measured on the device: one wave spins for `window_us` of the
 * constant 100 MHz wall clock (s_memrealtime) and counts shader-clock ticks (s_memtime).  Lets bench.py tell a
 * clock that has not ramped from a slower kernel.  Synchronises `hip_stream`. */
int vc_device_clock_mhz(double window_us, double* mhz_out, void* hip_stream);
int vc_set_timing(vc_engine* e, int enable);
int vc_get_timing(vc_engine* e, double* main_ms_total, int64_t* n_launches);

#ifdef __cplusplus
}
#endif
#endif /* VELOCYCLE_HIP_H */
