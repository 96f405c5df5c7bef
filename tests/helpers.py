"""Shared test helpers: fixtures -> oracle Problem / product ModelSpec."""
import glob
import math
import os

import numpy as np
import torch

from oracle import velocycle_oracle as orc
from velocycle_amd.spec import ModelSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP_CASES = sorted(os.path.basename(p)[len("ref_step_"):-4] for p in glob.glob(os.path.join(GOLDEN, "ref_step_*.npz")))
FIT_CASES = sorted(os.path.basename(p)[len("ref_fit_"):-4] for p in glob.glob(os.path.join(GOLDEN, "ref_fit_*.npz"))
                   if not os.path.basename(p).startswith("ref_fit_continue_"))
CONTINUE_CASES = sorted(os.path.basename(p)[len("ref_fit_continue_"):-4] for p in glob.glob(os.path.join(GOLDEN, "ref_fit_continue_*.npz")))

_TENSOR_FIELDS = ["S", "U", "count_factor", "Db", "D", "mu_nu", "sd_nu", "phixy_prior", "mu_gamma", "sd_gamma",
                  "mu_beta", "sd_beta", "mu_nuw", "sd_nuw"]
_SCALAR_FIELDS = ["kind", "guide", "noisemodel", "with_delta_nu", "H", "Hw", "mu_dnu", "gamma_alpha", "gamma_beta",
                  "sigma_ln_s", "sigma_ln_u", "rho_mean", "rho_std", "rho_scale", "rho_rank"]


def load_fixture(path):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def _fields(z, dtype):
    kw = {}
    for f in _TENSOR_FIELDS:
        if "in_" + f in z:
            kw[f] = torch.tensor(z["in_" + f]).to(dtype)
    for f in _SCALAR_FIELDS:
        if "in_" + f in z:
            v = z["in_" + f].item()
            kw[f] = v
    if "in_sd_dnu" in z:
        v = z["in_sd_dnu"]
        kw["sd_dnu"] = float(v) if v.ndim == 0 else torch.tensor(v).to(dtype)
    kw["condition_on"] = {k[len("cond_"):]: torch.tensor(v).to(dtype) for k, v in z.items() if k.startswith("cond_")}
    kw["with_delta_nu"] = bool(kw["with_delta_nu"])
    return kw


def problem_from_fixture(z, dtype=torch.float64) -> orc.Problem:
    return orc.Problem(**_fields(z, dtype))


def spec_from_fixture(z) -> ModelSpec:
    return ModelSpec(**_fields(z, torch.float32))


def spec_from_problem(p: orc.Problem) -> ModelSpec:
    kw = {}
    for k, v in p.__dict__.items():
        if isinstance(v, torch.Tensor):
            kw[k] = v.float()
        elif k == "condition_on":
            kw[k] = {a: b.float() for a, b in v.items()}
        else:
            kw[k] = v
    return ModelSpec(**kw)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    return float(np.abs(a - b).max() / scale)


def problem_from_spec(spec, dtype=torch.float64) -> orc.Problem:
    """The oracle's view of a product ModelSpec (CPU, `dtype`)."""
    kw = {}
    for k, v in spec.__dict__.items():
        if k in ("truth", "S_csr", "U_csr"):
            continue
        kw[k] = v.detach().cpu().to(dtype) if (isinstance(v, torch.Tensor) and v.is_floating_point()) else v
    # a spec that carries its counts as CSR only (cells x genes; what the engine then ingests): the oracle gets them densified
    # (callers also pass an oracle Problem, which has no such fields)
    for k, csr in (("S", getattr(spec, "S_csr", None)), ("U", getattr(spec, "U_csr", None))):
        if kw.get(k) is None and csr is not None:
            kw[k] = torch.tensor(np.asarray(csr.toarray(), dtype=np.float64).T.copy()).to(dtype)
    kw["condition_on"] = {k: v.detach().cpu().to(dtype) for k, v in spec.condition_on.items()}
    return orc.Problem(**kw)


def assert_step_matches_oracle(eng, spec, eps, loss_rtol=1e-5, grad_rtol=2e-3):
    """One ELBO + gradient evaluation already launched on `eng` with the host eps dict `eps`: loss within `loss_rtol`
    of the float64 oracle, every gradient block within `grad_rtol` of its max-norm -- or no worse than 4x the error of
    the oracle's own float32 run (= what the reference computes in) where the 1/(z + 1e-5) relu kink amplifies rounding."""
    torch.cuda.synchronize()
    return assert_grads_match_oracle(eng.loss(), eng.named(eng.grad), eng.named(), spec, eps, loss_rtol, grad_rtol)


def assert_grads_match_oracle(loss, grads, params, spec, eps, loss_rtol=1e-5, grad_rtol=2e-3):
    """assert_step_matches_oracle's bars on a loss, named gradient blocks and the named parameters they were evaluated at, wherever
    they come from (a fused step's gradient buffer and the parameters recorded in front of it, the ranks of a sharded step)."""
    p64 = problem_from_spec(spec, torch.float64)
    par = {n: v.detach().cpu().double() for n, v in params.items()}
    e64 = {k: v.double() for k, v in eps.items() if not k.startswith("_")}
    l64, g64, _, _ = orc.loss_and_grads(p64, par, e64)
    _, g32, _, _ = orc.loss_and_grads(p64.to(torch.float32), {k: v.float() for k, v in par.items()},
                                      {k: v.float() for k, v in e64.items()})
    if loss is not None:          # (None: a step of the gradient-only kernels, whose loss is not formed -- the caller asserts the NaN)
        assert abs(loss - l64) <= loss_rtol * abs(l64), (loss, l64)
    assert set(grads) == set(params), (sorted(grads), sorted(params))
    for name, got in grads.items():
        want = g64[name].numpy()
        fin = np.isfinite(want)
        err = np.abs(got.detach().cpu().numpy()[fin] - want[fin]).max()
        ref32 = np.abs(g32[name].numpy().astype(np.float64)[fin] - want[fin]).max()
        strict = grad_rtol * max(np.abs(want[fin]).max(), 1e-3)
        assert err <= max(strict, 4 * ref32), (name, err, ref32)
        CLAUSE_STATS["blocks"] += 1
        if err > strict:
            # the block passed only because the float32 oracle itself is this far from float64 (the 1 / (z + 1e-5) relu kink):
            # counted and printed, so that a suite that leans on this clause says so (pytest -s / the summary line of conftest.py)
            CLAUSE_STATS["by_ref32_clause"].append((name, float(err / max(np.abs(want[fin]).max(), 1e-3)), float(ref32 / max(np.abs(want[fin]).max(), 1e-3))))
            print(f"[assert_step_matches_oracle] block {name!r} passed through the 4 x float32-oracle clause only: err {err:.3e} "
                  f"(strict bar {strict:.3e}), float32 oracle's own error {ref32:.3e}")
    return l64, g64


DNU_ROW_RTOL, DNU_ROW_FLOOR = 2e-3, 1e-3


def assert_dnu_rows_match_oracle(got, want64, label):
    """The gradient of the per-batch offsets, `Δν_locs` (Nb, Ng), against the float64 oracle ROW BY ROW: for every batch q
    max |got[q] - want[q]| <= 2e-3 x max(max |want[q]|, 1e-3) -- the gradient tolerance of DESIGN section 4 and the floor of
    assert_step_matches_oracle, taken per batch instead of per block, and without its float32-oracle clause (Δν enters the constant
    harmonic only: no path through the relu kink of ElogU; the float32 oracle's own row error is ~2e-4 of this bar,
    tests/test_batch_rows_cpu.py).  An empty batch's row is exactly zero in the oracle and falls under the floor.

    The CALLER asserts that the Δν values the gradient was evaluated at are exactly 0: there the Normal(0, sd) prior's term of the
    gradient vanishes and row q is the likelihood sum over the workgroups (cells) of batch q alone -- a cell dropped, doubled or
    accounted to a neighbouring batch moves the row by a cell's share, which a prior term of ~Δν / sd^2 (sd = 0.01 in the velocity
    model: 500 per element at Δν = 0.05) otherwise buries under the block's max-norm.

    Returns the worst err / bar of every row (numpy, (Nb,)) for the caller to print."""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want64.detach().cpu().numpy() if torch.is_tensor(want64) else want64, dtype=np.float64)
    assert got.shape == want.shape and got.ndim == 2, (label, got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all(), label
    err = np.abs(got - want).max(axis=1)
    bar = DNU_ROW_RTOL * np.maximum(np.abs(want).max(axis=1), DNU_ROW_FLOOR)
    ratio = err / bar
    bad = np.nonzero(ratio > 1.0)[0]
    assert bad.size == 0, (label, [(int(q), float(err[q]), float(bar[q])) for q in bad])
    return ratio


PLANTED_SIZES = (400, 264, 0, 3)       # batch 0, batch 7, the empty batch, the tiny batch of onehot_layout's planted layouts


def onehot_layout(Nc, name, Nb, ids=None):
    """A batch id per cell (int64, (Nc,)) of the layouts the per-batch tests run:
      "interleaved": `ids` as they are (the random ids tests.test_hip_sweep._problem drew; without `ids`: drawn here from a generator
                     seeded by (Nc, Nb)) -- the engine reorders the cells by batch;
      "contiguous":  the same ids stably sorted (anndata.concat(..., label="batch"));
      "planted":     contiguous batches of planted sizes, Nb = 9 or 8: batch 0 has 400 cells and batch 7 has 264 (at 8 cells per
                     chunk, Tuning(cells_per_wave=2), 50 and 33 chunks: past the 32 rows the range sums request per trip), batch 2
                     is EMPTY, batch 4 has 3 cells (fewer than the 4 waves of a workgroup), the other batches share the rest evenly."""
    if name in ("interleaved", "contiguous"):
        if ids is None:
            ids = torch.randint(0, Nb, (Nc,), generator=torch.Generator().manual_seed(1000 * Nb + Nc))
        ids = torch.as_tensor(ids).long().reshape(-1)
        assert ids.numel() == Nc and int(ids.min()) >= 0 and int(ids.max()) < Nb
        return ids if name == "interleaved" else ids[torch.argsort(ids, stable=True)]
    if name != "planted" or Nb not in (8, 9):
        raise ValueError((name, Nb))
    sizes = {0: PLANTED_SIZES[0], 7: PLANTED_SIZES[1], 2: PLANTED_SIZES[2], 4: PLANTED_SIZES[3]}
    rest = [q for q in range(Nb) if q not in sizes]
    left = Nc - sum(sizes.values())
    assert left >= len(rest), (Nc, Nb)
    for i, q in enumerate(rest):
        sizes[q] = left // len(rest) + (1 if i < left % len(rest) else 0)
    return torch.cat([torch.full((sizes[q],), q, dtype=torch.long) for q in range(Nb)])


def onehot_Db(ids, Nb, dtype=torch.float64):
    return torch.stack([(ids == q).to(dtype) for q in range(Nb)])


# ---------------------------------------------------------------------------------------------------------------------
# The angular-speed coefficients: d loglik / d nu_omega[x, h] = sum_c A3_c D[x, c] zeta_omega_h(phi_c), one row per CONDITION x.
# ---------------------------------------------------------------------------------------------------------------------
NUW_ROW_RTOL, NUW_ROW_FLOOR, NUW_REST_RTOL = 2e-3, 1e-3, 1e-6
# |sin k phi, cos k phi of the kernels (float32: vc_dir_sincos + the harmonics' recurrence) - the float64 oracle's| <= k x this;
# see assert_omega_matches_oracle
OMEGA_SINCOS_ERR = 4e-7


def condition_layout(ids, Nb, Nx, name):
    """A (Nx, Nc) one-hot condition design D (float64) from a batch id per cell (onehot_layout; "planted": batch 4 has three cells,
    batch 2 none).  The TINY batch is the smallest batch that has cells, the tiny condition is the LAST one, Nx - 1:
      "tiny_last":  the tiny batch is alone in the last condition (the empty batches are nominally there too: no cell says so);
                    batch q of the others is in condition q mod (Nx - 1) -- constant within every batch;
      "empty_cond": the same with condition 1 left without any cell (Nx >= 3): the others are dealt out over 0, 2, .., Nx - 2;
      "scattered":  NOT constant within the batches (`ids` only gives Nc): the tiny condition's three cells are cell 0, cell Nc // 2
                    and cell Nc - 1, every other cell c is in condition c mod (Nx - 1)."""
    ids = torch.as_tensor(ids).long().reshape(-1)
    Nc = ids.numel()
    assert Nx >= 2 and Nc >= 4, (Nx, Nc)
    if name == "scattered":
        cond = torch.arange(Nc) % (Nx - 1)
        cond[[0, Nc // 2, Nc - 1]] = Nx - 1
    elif name in ("tiny_last", "empty_cond"):
        n = torch.bincount(ids, minlength=Nb)
        assert n.numel() == Nb
        tiny = int(torch.where(n > 0, n, n.max() + 1).argmin())
        slots = list(range(Nx - 1))
        if name == "empty_cond":
            if Nx < 3:
                raise ValueError("an empty condition beside the tiny one needs Nx >= 3")
            slots.remove(1)
        of_batch = torch.tensor([Nx - 1 if (q == tiny or int(n[q]) == 0) else slots[q % len(slots)] for q in range(Nb)])
        cond = of_batch[ids]
    else:
        raise ValueError(name)
    return torch.stack([(cond == x).double() for x in range(Nx)])


def nuw_row_blocks(grads, spec):
    """{name: float64 array (Nx, Nhw * k)} of every parameter block with one row per (condition, coefficient): mean-field `νω_locs`,
    `νω_scales` (k = 1); LRMN the last Nx Nhw entries of `loc` and `cov_diag` (k = 1) and the last Nx Nhw rows of `cov_factor`
    (k = R).  Non-finite entries (log-parameters at -inf: cov_factor zeros) are NaN in the result: the callers keep them out of every
    maximum, as assert_grads_match_oracle does."""
    Nx, Nhw = spec.Nx, spec.Nhw
    n = Nx * Nhw
    out = {}

    def put(name, t, key=None):
        a = np.array(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)
        a = a.reshape(-1, a.shape[-1])[-n:] if name == "cov_factor" else a.reshape(-1)[-n:]
        a = a.reshape(Nx, -1)
        a[~np.isfinite(a)] = np.nan
        out[key or name] = a

    if spec.guide == "meanfield":
        put("νω_locs", grads["νω_locs"])
        put("νω_scales", grads["νω_scales"])
    else:
        put("loc", grads["loc"], "loc[νω]")
        put("cov_diag", grads["cov_diag"], "cov_diag[νω]")
        put("cov_factor", grads["cov_factor"], "cov_factor[νω]")
    return out


def _rowmax(a):
    """max |a| of every row, NaN (kept out) entries aside; 0 for a row of nothing else."""
    return np.nan_to_num(np.abs(a), nan=0.0).max(axis=1)


def nuw_row_bars(params, spec, eps):
    """(want, lik, rest, bar): the float64 oracle's nuw_row_blocks at `params` / `eps`; `rest` = the same call with D = 0 -- then
    omega == 0, no nu_omega-related parameter has a path to the likelihood, and what is left of those rows is exactly their prior +
    entropy part; lik = want - rest; bar[name] (Nx,) = 2e-3 x max(max |lik[x]|, 1e-3) + 1e-6 x max |rest[x]| -- the gradient tolerance
    of DESIGN section 4 per CONDITION on the likelihood sum alone, plus 8 float32 roundings of the prior / entropy part (all there is
    in the row of a condition without cells)."""
    p64 = problem_from_spec(spec, torch.float64)
    par = {n: v.detach().cpu().double() for n, v in params.items()}
    e64 = {k: v.detach().cpu().double() for k, v in eps.items() if not k.startswith("_")}
    _, g, _, _ = orc.loss_and_grads(p64, par, e64)
    p0 = orc.Problem(**{**p64.__dict__, "D": torch.zeros_like(p64.D)})
    _, g0, _, _ = orc.loss_and_grads(p0, par, e64)
    want, rest = nuw_row_blocks(g, spec), nuw_row_blocks(g0, spec)
    lik = {k: want[k] - rest[k] for k in want}
    bar = {k: NUW_ROW_RTOL * np.maximum(_rowmax(lik[k]), NUW_ROW_FLOOR) + NUW_REST_RTOL * _rowmax(rest[k]) for k in want}
    return want, lik, rest, bar


def assert_nuw_rows_match_oracle(grads, params, spec, eps, label):
    """Every nu_omega-related gradient row against the float64 oracle PER CONDITION (nuw_row_bars): for every block of nuw_row_blocks
    and every condition x, max |got[x] - want[x]| <= bar[x].  No float32-oracle clause: tests/test_nuw_rows_cpu.py holds the float32
    oracle's own rows to <= 0.25 of this bar on every case the GPU tests run.  A block-wide bar cannot see a small condition: a row
    of three cells is 100-900 times smaller than the block's max-norm, a cell of a neighbouring batch added to it passes, and so does
    the row stored as zero.  Returns {block: err / bar per condition (Nx,)} for the caller to print."""
    want, _, _, bar = nuw_row_bars(params, spec, eps)
    got = nuw_row_blocks(grads, spec)
    assert set(got) == set(want), (label, sorted(got), sorted(want))
    out, bad = {}, []
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (label, k)
        err = _rowmax(got[k] - want[k])
        out[k] = err / bar[k]
        bad += [(k, int(x), float(err[x]), float(bar[k][x])) for x in np.nonzero(out[k] > 1.0)[0]]
    assert not bad, (label, bad)
    return out


def assert_omega_matches_oracle(omega, params, spec, eps, label):
    """The forward side: the angular speed of every cell (read_site("ω") behind a sample at `params` with the draws `eps`) against
    the float64 oracle's det["ω"] = sum_x D[x, c] sum_h nu_omega[x, h] zeta_omega_h(phi_c).  Bar per cell:
        16 eps32 x sum_x D[x, c] sum_h |nu_omega[x, h] zeta_omega_h(phi_c)|          (the sample, the products, the sum)
      + OMEGA_SINCOS_ERR x sum_x D[x, c] sum_k k (|nu_omega[x, 2k - 1]| + |nu_omega[x, 2k]|)   (sin k phi, cos k phi in float32).
    OMEGA_SINCOS_ERR = 4e-7 = 4 x the 9.6e-8 measured once on an MI355X against the float64 oracle, on the mean-field joint cases of
    tests/test_nuw_rows_cpu.py (800, 2 100 and 3 200 cells, Hw = 1 and 3) with the constant coefficient set to 0 and every harmonic
    coefficient to 1, so that omega_c = sum_k sin k phi_c + cos k phi_c: max_c |omega_c - float64| / sum_k 2 k = 6.0e-8 .. 9.6e-8 per
    case (median 1.5e-8) -- the rounding of that sum included.  On the cases as they are the whole error was at most 2.9 eps32 of the
    first term's scale (the K_pre sample; 2.6 for the chain's), so the first term's 16 leaves 5 x.
    With the cases' coefficients 0.2 apart between conditions, a cell evaluated with another condition's row is ~1e5 bars off.
    Returns the worst err / bar."""
    p64 = problem_from_spec(spec, torch.float64)
    par = {n: v.detach().cpu().double() for n, v in params.items()}
    e64 = {k: v.detach().cpu().double() for k, v in eps.items() if not k.startswith("_")}
    _, val, det = orc.elbo_loss(p64, par, e64)
    nuw, zw, D = val["νω"].detach().numpy(), det["ζω"].detach().numpy(), p64.D.numpy()        # (Nx, Nhw), (Nhw, Nc), (Nx, Nc)
    want = det["ω"].detach().numpy()
    k = (np.arange(spec.Nhw) + 1) // 2
    scale = np.einsum("xc,xh,hc->c", np.abs(D), np.abs(nuw), np.abs(zw))
    bar = 16 * float(np.finfo(np.float32).eps) * scale + OMEGA_SINCOS_ERR * (np.abs(D).T @ (np.abs(nuw) @ k))
    got = np.asarray(omega.detach().cpu().numpy() if torch.is_tensor(omega) else omega, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape and np.isfinite(got).all(), (label, got.shape, want.shape)
    ratio = np.abs(got - want) / np.maximum(bar, 1e-300)
    bad = np.nonzero(ratio > 1.0)[0]
    assert bad.size == 0, (label, [(int(c), float(got[c]), float(want[c]), float(bar[c])) for c in bad[:8]], int(bad.size))
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------------
# The likelihood kernel's cell loop: every gene-level gradient is a sum over ALL cells, and in the U-only kernels a cell reaches nothing
# else.  Lit-cell probe data make one cell a large share of one gene's row; the rows are then held to the oracle per GENE.
# ---------------------------------------------------------------------------------------------------------------------
LIT_COUNT = 200.0          # the lit entries: an integer < 2048 (uint16 storage and the dense histogram tables stay selectable)
LIT_LEVEL = -4.0           # mu_nu[:, 0] of the count models: an unlit entry's mean term is ~1e-2 of a lit entry's
LIT_Z_MIN = 0.3            # z = omega nu.zeta' + gamma of every (gene, cell): nowhere near the relu kink of ElogU
GENE_ROW_RTOL, GENE_ROW_FLOOR = DNU_ROW_RTOL, DNU_ROW_FLOOR


def lit_cell_problem(p, amp=None, seed=0):
    """A problem of tests.test_hip_sweep._problem (float64 oracle Problem) turned into a lit-cell probe; returns a new Problem.
      counts:  zero except S[c mod Ng, c] = U[(c + 1) mod Ng, c] = LIT_COUNT: every cell lit in exactly one gene per matrix, every
               gene in m ~ Nc / Ng cells;
      level:   mu_nu[:, 0] = LIT_LEVEL + 0.1 x noise; a conditioned nu follows.  Lognormal noise: the data are log(k + 1) and an unlit
               entry's residual is its own log-mean / sigma^2, so the means are put where the unlit entries ARE -- mu_nu[:, 0],
               mu_beta and mu_gamma 0 + 0.005 x noise, sd_nu[:, 0] 0.02, sd_beta 0.01: a gene's ~1 000 unlit residuals then stay
               under its m lit ones;
      phases:  cell c sits at phi_c = c (pi + 0.37) + 0.1 x noise (prior and conditioned value), the first harmonic of gene g at the
               angle g pi / 2 + 0.1 x noise: neighbouring cells lie opposite each other, neighbouring genes a quarter turn apart, so
               of the two genes lit in a pair of neighbouring cells at least one sees |cos| differ by ~1.4 between the two (random
               phases leave pairs whose gamma / z coincide: an exchange there moved no row by more than 2.1 bars);
      kink:    the harmonics' amplitudes a_k (all of `amp` = 0.65 for H = 1; else `amp` = 0.5, 0.8 amp for k = 1 and the rest shared
               as 1 / k at random angles) have sum_k k a_k = amp, so |nu.zeta'| <= amp; gamma = exp(0.05 x noise),
               nu_omega's constant as `p` has it (0.4 + 0.05 x noise), prior sds of the harmonics of nu, of log gamma and of nu_omega
               0.01 / 0.05 / 0.02 so that a draw stays where the mean is.  Asserted here, in float64 at the prior means:
               z = omega nu.zeta' + gamma >= LIT_Z_MIN + 0.15 for every (gene, cell); assert_gene_rows_match_oracle asserts
               z >= LIT_Z_MIN at the point a gradient was evaluated at.
    gamma / z then ranges over ~[0.75, 1.6] from cell to cell: a cell evaluated with its neighbour's record shows in d / d log gamma."""
    g = torch.Generator().manual_seed(977 + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Ng, Nc, Hh = p.Ng, p.Nc, p.H
    cells = torch.arange(Nc)
    S = torch.zeros(Ng, Nc, dtype=torch.float64)
    S[cells % Ng, cells] = LIT_COUNT
    kw = dict(p.__dict__)
    kw["S"] = S
    lognormal = p.noisemodel == "Lognormal"
    mu_nu, sd_nu = p.mu_nu.clone(), p.sd_nu.clone()
    amp = amp if amp is not None else (0.65 if Hh == 1 else 0.5)
    mu_nu[:, 0] = 0.005 * r(Ng) if lognormal else LIT_LEVEL + 0.1 * r(Ng)
    first = 1.0 if Hh == 1 else 0.8
    for k in range(1, Hh + 1):
        a_k = amp * first if k == 1 else amp * (1.0 - first) / ((Hh - 1) * k)
        ang = (0.5 * math.pi * torch.arange(Ng, dtype=torch.float64) + 0.1 * r(Ng)) if k == 1 else \
            2 * math.pi * torch.rand(Ng, generator=g, dtype=torch.float64)
        mu_nu[:, 2 * k - 1], mu_nu[:, 2 * k] = a_k * torch.cos(ang), a_k * torch.sin(ang)
    sd_nu[:, 1:] = 0.01
    if lognormal:
        sd_nu[:, 0] = 0.02
    kw["mu_nu"], kw["sd_nu"] = mu_nu, sd_nu
    phi = (math.pi + 0.37) * cells.double() + 0.1 * r(Nc)
    kw["phixy_prior"] = 2.0 * torch.stack([torch.cos(phi), torch.sin(phi)], 1)
    cond = {k: v.clone() for k, v in p.condition_on.items()}
    if "ϕxy" in cond:
        cond["ϕxy"] = kw["phixy_prior"] + 0.02 * r(Nc, 2)
    if "ν" in cond:
        cond["ν"] = mu_nu + torch.cat([(0.005 if lognormal else 0.05) * r(Ng, 1), 0.01 * r(Ng, 2 * Hh)], 1)
    if p.kind == "velocity":
        U = torch.zeros(Ng, Nc, dtype=torch.float64)
        U[(cells + 1) % Ng, cells] = LIT_COUNT
        kw["U"] = U
        kw["mu_gamma"], kw["sd_gamma"] = (0.005 if lognormal else 0.05) * r(Ng), torch.full((Ng,), 0.05, dtype=torch.float64)
        kw["sd_nuw"] = torch.full_like(p.sd_nuw, 0.02)
        if lognormal:
            kw["mu_beta"], kw["sd_beta"] = 0.005 * r(Ng), torch.full((Ng,), 0.01, dtype=torch.float64)
        if "logγg" in cond:
            cond["logγg"] = kw["mu_gamma"] + 0.02 * r(Ng)
        if "logβg" in cond and lognormal:
            cond["logβg"] = kw["mu_beta"] + 0.02 * r(Ng)
    kw["condition_on"] = cond
    q = type(p)(**kw)
    if q.kind == "velocity":
        par = orc.init_params(q, torch.zeros(q.Ng + q.Nx * q.Nhw, q.rho_rank, dtype=torch.float64))
        zero = {k: torch.zeros_like(v) for k, v in orc.draw_eps(q, torch.Generator().manual_seed(0)).items()}
        zmin = lit_z_min(q, par, zero)
        assert zmin >= LIT_Z_MIN + 0.15, zmin
    return q


def lit_z_min(p, par, eps):
    """min over (gene, cell) of z = omega nu.zeta'(phi) + gamma at the parameters `par` and draws `eps`, float64 (velocity models)."""
    p64 = p if isinstance(p, orc.Problem) else problem_from_spec(p, torch.float64)
    par = {n: v.detach().cpu().double() for n, v in par.items()}
    e64 = {k: v.detach().cpu().double() for k, v in eps.items() if not k.startswith("_")}
    _, val, det = orc.elbo_loss(p64, par, e64)
    z = torch.einsum("gh,ch->gc", val["ν"], det["ζ_dϕ"]) * det["ω"] + det["γg"][:, None]
    return float(z.min())


def gene_row_blocks(grads, spec):
    """{name: float64 array (rows, k)} of every parameter block with one row per GENE -- mean-field `ν_locs`, `ν_scales` (k = Nh),
    `logγg_*`, `logβg_*`, `shape_inv_locs` (k = 1); LRMN the first Ng entries of `loc` and `cov_diag`, the first Ng rows of
    `cov_factor` (k = R) and `rho_real_loc` -- and, where phi_xy is learned, `ϕxy_locs` with one row per CELL (k = 2).  Non-finite
    entries are NaN in the result and kept out of every maximum (nuw_row_blocks)."""
    Ng = spec.Ng
    out = {}

    def put(key, t, rows):
        a = np.array(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)
        a = a.reshape(a.shape[0], -1)[:rows].copy()
        a[~np.isfinite(a)] = np.nan
        out[key] = a

    for name in ("ν_locs", "ν_scales", "logγg_locs", "logγg_scales", "logβg_locs", "logβg_scales", "shape_inv_locs", "rho_real_loc"):
        if name in grads:
            put(name, grads[name], Ng)
    for name in ("loc", "cov_diag", "cov_factor"):
        if name in grads:
            put(name + "[γ]", grads[name], Ng)
    if "ϕxy" not in spec.condition_on and "ϕxy_locs" in grads:
        put("ϕxy_locs", grads["ϕxy_locs"], spec.Nc)
    return out


def gene_row_ratios(got, want):
    """{block: err / bar per row}: |got[g] - want[g]|_max / (GENE_ROW_RTOL x max(|want[g]|_max, GENE_ROW_FLOOR)) of gene_row_blocks."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    out = {}
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        out[k] = _rowmax(got[k] - want[k]) / (GENE_ROW_RTOL * np.maximum(_rowmax(want[k]), GENE_ROW_FLOOR))
    return out


def assert_gene_rows_match_oracle(grads, params, spec, eps, label):
    """Every gene-indexed gradient block against the float64 oracle (on the float32-rounded parameters and draws) ROW BY ROW: for
    every block of gene_row_blocks and every gene g, max |got[g] - want[g]| <= 2e-3 x max(max |want[g]|, 1e-3) -- DNU_ROW_RTOL /
    DNU_ROW_FLOOR per gene, per cell for a learned `ϕxy_locs`.  No float32-oracle clause: the caller's data keep every element off
    the relu kink (asserted here for the velocity models: z >= LIT_Z_MIN at `params` / `eps`), and tests/test_cell_rows_cpu.py holds
    the float32 oracle's own rows to <= 0.25 of this bar on lit_cell_problem's data, where one cell left out, counted twice or
    evaluated with its neighbour's record moves a row by several bars.  Returns {block: worst err / bar} for the caller to print."""
    p64 = problem_from_spec(spec, torch.float64)
    par = {n: v.detach().cpu().double() for n, v in params.items()}
    e64 = {k: v.detach().cpu().double() for k, v in eps.items() if not k.startswith("_")}
    if p64.kind == "velocity":
        zmin = lit_z_min(p64, par, e64)
        assert zmin >= LIT_Z_MIN, (label, zmin)
    _, g64, _, _ = orc.loss_and_grads(p64, par, e64)
    ratio = gene_row_ratios(gene_row_blocks(grads, spec), gene_row_blocks(g64, spec))
    bad = [(k, int(g), float(v[g])) for k, v in ratio.items() for g in np.nonzero(v > 1.0)[0]]
    assert not bad, (label, bad[:12], len(bad))
    return {k: float(v.max()) for k, v in ratio.items()}


# how often assert_step_matches_oracle's second clause (<= 4 x the float32 oracle's own error) was what let a gradient block pass;
# tests/conftest.py prints the tally at the end of a run
CLAUSE_STATS = {"blocks": 0, "by_ref32_clause": []}


def assert_trajectory_within_float32_spread(spec, opt, n, seed, losses, named_params, snapshots=None):
    """SURVEY §8(d) ELBO-match over n SVI steps on the same host eps stream: the first steps agree with the float64
    oracle to 1e-5; afterwards float32 and float64 Adam trajectories separate by themselves, so the yardstick is the
    oracle's own float32 run (x4); fitted parameters within 1e-3 of each block's max-norm wherever float32 itself is.

    `snapshots` = {t: named parameters at the START of step t}, recorded by the caller: teacher forcing.  Adam's first steps
    move every parameter by ~lr * sign(gradient); where a gradient is zero to within float32 rounding (|g| = 23 next to a
    block max of 1e6 and a float32 error of 5e3 -- observed on this very workload) its sign is a coin toss in ANY float32
    evaluation, and the parameter starts 2 lr away from the float64 run's: a 1e-4 step in the loss one step later that says
    nothing about the kernels.  With snapshots the strict 1e-5 bar is therefore held where it tests the kernels -- the loss
    of step t against the float64 oracle evaluated AT the run's own parameters with the same draws -- and the free-running
    comparison allows 5e-4 (and the fitted parameters the quantile criterion of assert_params_track_oracle)."""
    p64 = problem_from_spec(spec, torch.float64)
    l64, par64 = orc.fit(p64, opt, n, seed=seed)
    l32, par32 = orc.fit(p64.to(torch.float32), opt, n, seed=seed)
    l64, l32, losses = np.array(l64), np.array(l32), np.array(losses)
    rel_hip, rel_32 = np.abs(losses - l64) / np.abs(l64), np.abs(l32 - l64) / np.abs(l64)
    assert rel_hip[0] <= 1e-5, rel_hip[:5]
    allow = 1e-5
    if snapshots:
        from velocycle_amd.rng import draw_eps
        g = torch.Generator().manual_seed(seed)
        draw_eps(spec, g)                                   # the guide's warm-up draw (SVIRunner parity mode, orc.fit)
        eps_t = [draw_eps(spec, g) for _ in range(max(snapshots) + 1)]
        for t, par in sorted(snapshots.items()):
            e64 = {k: v.double() for k, v in eps_t[t].items() if not k.startswith("_")}
            l_tf, _, _, _ = orc.loss_and_grads(p64, {k: v.detach().cpu().double() for k, v in par.items()}, e64)
            assert abs(losses[t] - l_tf) <= 1e-5 * abs(l_tf), (t, losses[t], l_tf)
        allow = 5e-4
    else:
        assert rel_hip[:5].max() <= 1e-5, rel_hip[:5]
    # free-running comparison: step by step against the float32 oracle's accumulated drift -- or, with teacher forcing (the
    # run may have left the float64 trajectory a few steps EARLIER than the float32 oracle happened to), against its largest
    # (x 8 there: two float32 runs of a flow that has left the float64 one are as far from each other as from it)
    yard = (8 * np.full_like(rel_32, rel_32.max())) if snapshots else 4 * np.maximum.accumulate(rel_32)
    assert (rel_hip <= np.maximum(allow, yard)).all(), (rel_hip.max(), rel_32.max())
    if snapshots:
        assert_params_track_oracle({k: v.detach().cpu().numpy() for k, v in named_params.items()},
                                   {k: v.numpy() for k, v in par64.items()}, {k: v.double().numpy() for k, v in par32.items()})
        return
    for k, v in named_params.items():
        want, got = par64[k].numpy(), v.detach().cpu().numpy().astype(np.float64)
        ref32 = par32[k].double().numpy()
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin), k
        if not fin.any():
            continue
        scale = max(np.abs(want[fin]).max(), 1e-2)
        err, spread = np.abs(got[fin] - want[fin]).max(), np.abs(ref32[fin] - want[fin]).max()
        assert err <= max(1e-3 * scale, 4 * spread), (k, err, spread, scale)


# philox_eps_list pins every step's draws while n * eps_total is at most this (a numpy Philox over that many indices: well under a
# second); past it (a slice of the 50 000-cell workload) the first and the last step, and it prints which steps it left unpinned
ANCHOR_ALL_STEPS_UP_TO = 1 << 19


def philox_eps_list(spec, params_flat, seed, n):
    """The standard-normal draws the performance path uses at steps 0..n-1 (Philox4x32-10 keyed by (seed, step, index)),
    rebuilt by the DEVICE -- a second engine's sampling kernel at (seed, t), read back through vc_read_site(eps) -- and PINNED by
    the float64 restatement of the stream that shares no code with it (tests/noise_checker.py): every flat vector read back must
    equal noise_checker.normals(seed, t, global index) within noise_checker.TOL, apart from the alignment slot no site owns.
    Returned as the oracle's per-site eps dicts (float64, CPU): the device's own float32 draws, so that the oracle replays exactly
    what the run under test drew."""
    from tests import noise_checker as NC
    from velocycle_amd.engine import HipEngine
    eng = HipEngine(spec)
    eng.params.copy_(params_flat.to(eng.device))
    shapes = {"ν": (spec.Ng, spec.Nh), "νω": (spec.Nx, spec.Nhw), "ϕxy": (spec.Nc, 2)}
    owned = NC.slot_names(eng) != "align"
    gidx = NC.global_index(eng)[owned]
    pinned = set(range(n)) if n * eng.eps_total <= ANCHOR_ALL_STEPS_UP_TO else {0, n - 1}
    if len(pinned) < n:
        print(f"\n[philox_eps_list] {n} steps x {eng.eps_total} draws > {ANCHOR_ALL_STEPS_UP_TO}: steps 0 and {n - 1} are pinned to "
              f"tests/noise_checker.py, steps 1..{n - 2} are NOT")
    out = []
    for t in range(n):
        eng.sample_guide(eps=None, seed=seed, step=t)
        flat = eng.read_site("eps")
        if t in pinned:
            err = np.abs(flat.double().numpy()[owned] - NC.normals(seed, t, gidx))
            assert err.max() <= NC.TOL, (seed, t, int(err.argmax()), float(err.max()))
        out.append({k: flat[o:o + s].double().reshape(shapes.get(k, (s,))) for k, (o, s) in eng.eps_slices.items()})
    eng.close()
    return out


def oracle_replay(spec, opt, par0_named, eps_list, dtype=torch.float64):
    """orc.fit on explicit initial parameters and eps draws: (losses, final unconstrained params)."""
    p = problem_from_spec(spec, dtype)
    par0 = {k: v.detach().cpu().to(dtype).clone() for k, v in par0_named.items()}
    eps = [{k: v.to(dtype) for k, v in e.items()} for e in eps_list]
    return orc.fit(p, opt, len(eps), eps_list=eps, params=par0)


def assert_params_track_oracle(got, par64, par32, frac=0.99, report=None):
    """Fitted parameters of a multi-step run against the float64 oracle trajectory on the same eps draws: per block,
    |got - want| <= max(1e-3 x the block's max-norm, 4 x the float32 oracle's own distance from float64).  ElogU has a relu
    kink with a 1/(z + 1e-5) factor behind it: a gene that crosses it sees its gradient change by orders of magnitude for a
    1e-4 change of its parameters (observed: -2137 vs +174 one step after a 1.7e-4 difference), so single elements of a
    float32 trajectory -- any float32 trajectory, the reference's own included -- can leave the float64 one by O(lr) per step.
    Blocks of >= 100 elements therefore have to hold the bar on `frac` of their elements (and may not do worse than the float32
    oracle by more than 1 - frac); small blocks on all of them.  Returns {block: (fraction within, max err / max-norm)}."""
    out = {}
    for k, g in got.items():
        want, ref32 = np.asarray(par64[k], dtype=np.float64), np.asarray(par32[k], dtype=np.float64)
        g = np.asarray(g, dtype=np.float64).reshape(want.shape)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(g), fin), k
        if not fin.any():
            continue
        scale = max(np.abs(want[fin]).max(), 1e-2)
        err, e32 = np.abs(g[fin] - want[fin]), np.abs(ref32[fin] - want[fin])
        tol = np.maximum(1e-3 * scale, 4 * e32.max())
        within, within32 = float((err <= tol).mean()), float((e32 <= 1e-3 * scale).mean())
        out[k] = (within, float(err.max() / scale), within32, float(e32.max() / scale))
        need = 1.0 if err.size < 100 else min(frac, within32 - (1 - frac))
        assert within >= need, (k, within, need, float(err.max()), float(e32.max()), scale)
    if report is not None:
        print(f"\n[{report}] per block: fraction within tolerance, max |err| / max-norm (HIP | float32 oracle): "
              + ", ".join(f"{k} {a:.4f} {b:.1e} | {c:.4f} {d:.1e}" for k, (a, b, c, d) in out.items()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Boundary counts: the per-gene count histograms behind every lgamma / digamma term of the negative binomial have their own
# special cases (vc_host_logic.h: dense tail-count tables for integer counts < 2048; vc_common.h: the first 256 levels
# prefetched, levels 256 .. 639 read only by blocks past 256, a second loop from 640, quarter blocks for blocks past 256 levels;
# the (value, multiplicity) lists with the Stirling difference as soon as one count is >= 2048 or not an integer; uint16 count
# storage while every count is an integer <= 65535).  These data put genes at those boundaries.
# ---------------------------------------------------------------------------------------------------------------------
BOUNDARY_LEVELS = (255, 256, 257, 639, 640, 641, 2047)
# the per-gene bar of the shape_inv_locs gradient: |got - float64| <= GENE_RTOL x the gene's sum of absolute terms
# (nb_shape_inv_terms); tests/test_count_extremes_cpu.py checks that one count level more or less moves it by > 3 GENE_RTOL
GENE_RTOL = 1e-6
# one extra count planted in one cell -> (histogram form it forces, count storage it forces on a u16-capable kernel)
OVERFLOW_VARIANTS = {None: ("dense-capable", "u16"), 2048.0: ("lists", "u16"), 65535.0: ("lists", "u16"),
                     65536.0: ("lists", "f32"), 7.5: ("lists", "f32"), 100000.5: ("lists", "f32")}


def boundary_plan(Ng=200):
    """{matrix: {gene: largest count}} of the planted genes (gene blocks of 64, quarters of 16 genes), the same genes in S and U.
    Every boundary level is the largest count of a QUARTER of its own (the quarter blocks run to their quarter's largest count):
      block 0: 2047 (gene 0, quarter 0; gene 7 beside it all zero), 257 (gene 16), 256 (gene 32), 255 (gene 48);
      block 1: quarter 0 (genes 64..79) all zero, 700 (gene 85), 641 (gene 96), 640 (gene 112);
      block 2: all zero (genes 128..191);  block 3, the ragged last block (Ng = 200): 639 (gene Ng - 3)."""
    S = {0: 2047, 16: 257, 32: 256, 48: 255, 85: 700, 96: 641, 112: 640, Ng - 3: 639}
    zero = [7] + list(range(64, 80)) + list(range(128, 192))
    return {"S": S, "U": dict(S)}, zero


def plant_boundary_counts(M, plan, zero, seed, top=80, split_ranks=True):
    """M: (Ng, Nc) float32 counts, changed in place.  Gene g of `plan` gets its largest count K on `top` cells of the FIRST half
    of the cells, counts uniform in [0, K) on the rest of that half and below min(K, 200) on the second half -- so that with the
    cells split in two shards only the first shard's table goes past 256 levels in that block.  Genes in `zero` are all zero."""
    g = torch.Generator().manual_seed(seed)
    Nc = M.shape[1]
    h = Nc // 2
    for gene, K in plan.items():
        row = torch.empty(Nc)
        row[:h] = torch.floor(torch.rand(h, generator=g) * K)
        row[h:] = torch.floor(torch.rand(Nc - h, generator=g) * (min(K, 200) if split_ranks else K))
        row[torch.randperm(h, generator=g)[:top]] = float(K)
        M[gene] = row
    for gene in zero:
        M[gene] = 0.0
    return M


def boundary_spec(kind="phase", noisemodel="NegativeBinomial", Nc=200, Ng=200, overflow=None, overflow_cell=None, seed=3):
    """A small problem (Nc cells x Ng genes, four gene blocks) with the genes of boundary_plan planted in S (and U).
    kind: "phase" | "vjoint" | "vjoint_lrmn" | "vcond" (make_velocity_spec's modes).  `overflow`: one extra count (a key of
    OVERFLOW_VARIANTS) written into gene 20, cell `overflow_cell` (default: the last cell) of S -- and of U -- which forces the
    lists form, and float32 storage where it is > 65535 or not an integer.  The prior of every planted gene is re-centred on its
    data like the workloads centre theirs (log of the mean, half the std of log(S + 1))."""
    from velocycle_amd.workloads import make_phase_spec, make_velocity_spec
    if kind == "phase":
        spec = make_phase_spec(Nc, Ng, seed=seed, noisemodel=noisemodel)
    else:
        spec = make_velocity_spec(Nc, Ng, kind, 1, 1, seed=seed, noisemodel=noisemodel)
    plan, zero = boundary_plan(Ng)
    S = plant_boundary_counts(spec.S.contiguous().clone(), plan["S"], zero, seed + 100)
    mats = {"S": S}
    if spec.kind == "velocity":
        mats["U"] = plant_boundary_counts(spec.U.contiguous().clone(), plan["U"], zero, seed + 200)
    if overflow is not None:
        c = Nc - 1 if overflow_cell is None else overflow_cell
        for M in mats.values():
            M[20, c] = float(overflow)
    spec.S = mats["S"]
    if "U" in mats:
        spec.U = mats["U"]
    mu, sd = spec.mu_nu.clone(), spec.sd_nu.clone()
    for gene in set(plan["S"]) | set(zero):
        mu[gene, 0] = torch.log(S[gene].mean().clamp_min(1e-3))
        sd[gene, 0] = (torch.log(S[gene] + 1).std() / 2).clamp_min(0.05)
        mu[gene, 1:], sd[gene, 1:] = 0.0, 0.05     # (a flat gene: no cell of it on the relu kink of ElogU at the initial parameters)
    spec.mu_nu, spec.sd_nu = mu, sd
    if spec.kind == "velocity":
        # unspliced counts as large as the spliced ones: E[U] = E[S] at the initial parameters (log beta = 0, gamma = 1, omega = 0)
        mb = spec.mu_beta.clone()
        mb[list(plan["U"])] = 0.0
        spec.mu_beta = mb
    if "ν" in spec.condition_on:
        nu = spec.condition_on["ν"].clone()
        nu[:, 0] = mu[:, 0]
        spec.condition_on["ν"] = nu
    spec.truth = None
    return spec


def nb_shape_inv_terms(spec, par, eps):
    """Float64, on the host, per gene of a negative binomial problem at parameters `par` and draws `eps` (oracle site values):
    r = 1 / shape_inv, and the pieces of d(-ELBO) / d shape_inv_locs (the chain rule of vc_si_grad: d/d log si = -r dL/dr ... ):
      scale[g]  = r * (sum_j C_j / (r + j) + n_mat Nc |log r + 1| + sum_c |log(r + mu_c)| + (r + k_c) / (r + mu_c)) + |prior|
                  -- the gene's sum of absolute terms, the yardstick of its shape_inv_locs gradient;
      tables[m] = {gene: C (float64 array, C[j] = cells with count > j)} of the integer-count genes of matrix m."""
    import math
    p64 = problem_from_spec(spec, torch.float64)
    par64 = {k: v.detach().cpu().double() for k, v in par.items()}
    _, _, val, det = orc.loss_and_grads(p64, par64, {k: v.double() for k, v in eps.items() if not k.startswith("_")})
    si = val["shape_inv"].double().numpy().reshape(-1)
    r = 1.0 / si
    mats = [(p64.S.numpy(), det["ElogS"].numpy())]
    if spec.kind == "velocity":
        mats.append((p64.U.numpy(), det["ElogU"].numpy()))
    scale = np.zeros(spec.Ng)
    tables = []
    for M, Elog in mats:
        mu = np.exp(Elog)
        t = {}
        for g in range(spec.Ng):
            k = M[g]
            per_cell = np.abs(np.log(r[g] + mu[g])) + (r[g] + k) / (r[g] + mu[g])
            kmax = int(k.max()) if k.size else 0
            hist = 0.0
            if np.all(k == np.floor(k)) and kmax < (1 << 17):
                C = (k[None, :] > np.arange(kmax)[:, None]).sum(1).astype(np.float64)
                t[g] = C
                hist = float((C / (r[g] + np.arange(kmax))).sum())
            else:
                from scipy.special import digamma
                hist = float(np.abs(digamma(r[g] + k) - digamma(r[g])).sum())
            scale[g] += r[g] * (hist + spec.Nc * abs(math.log(r[g]) + 1.0) + per_cell.sum())
        tables.append(t)
    scale += np.abs((spec.gamma_alpha - 1.0) - spec.gamma_beta * si)
    return r, scale, tables


# ---------------------------------------------------------------------------------------------------------------------
# Count ingest: the blocked count layout and the per-gene histograms are filled by vc_pack_counts_kernel (dense input) or
# vc_scatter_csr_kernel (CSR input).  The oracle is handed the same matrix as the engine, not what the engine stored, so the
# bar between two ingest forms of one matrix is equality of engines (tests/test_hip_ingest.py, tests/test_hip_ingest_paths.py).
# ---------------------------------------------------------------------------------------------------------------------
def _mk(spec, **kw):
    from velocycle_amd.engine import HipEngine
    return HipEngine(spec, **kw)


def _hist_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _host_checker(spec, tuning=None, **kw):
    from velocycle_amd.tuning import Tuning
    e = _mk(spec, tuning=(tuning or Tuning()).replace(host_hist=True), **kw)
    assert not e.stats["hist_on_device"]
    return e


SPARSE_EDGE_ROW_LENGTHS = (1, 63, 64, 65, 129, 200)     # around the 64 lanes of the scatter kernel's wave, and past two trips
SPARSE_EDGE_EMPTY_GENE = 5


def sparse_edge_counts(Nc, Ng, seed):
    """(dense, csr): counts of Nc cells x Ng genes (Ng >= 260, Nc >= 3 * (len(SPARSE_EDGE_ROW_LENGTHS) + 3)) as a NON-canonical
    scipy CSR matrix built from (data, indices, indptr) -- what a caller may hand to the engine -- and the dense (Nc, Ng) float32
    matrix it stands for: the float64 sum of the stored entries of every (cell, gene), cast to float32.  Planted:
      * cells 0 and Nc - 1 and, of the middle shard of a 3-way split (engine.shard_bounds(Nc, 1, 3)), the first and the last cell
        without any stored entry;
      * rows of exactly SPARSE_EDGE_ROW_LENGTHS stored entries, distinct genes, once from cell 1 on (ascending indices) and once from
        the second cell of the middle shard on (indices stored in DESCENDING order); the 200-entry rows hold the last gene Ng - 1;
      * gene SPARSE_EDGE_EMPTY_GENE without any entry;
      * every other cell: ~8 % of the genes with counts 1 .. 12, indices in random order; 24 of these rows get an explicitly
        stored 0.0 at a gene they do not hold otherwise, 24 others one (cell, gene) entry stored TWICE (a + b: the values add).
    The planted-length rows have neither zeros nor duplicates: their lengths are what the kernel sees after sum_duplicates()."""
    from velocycle_amd.engine import shard_bounds
    rng = np.random.default_rng(seed)
    c0, c1 = shard_bounds(Nc, 1, 3)
    empty = {0, Nc - 1, c0, c1 - 1}
    genes = np.array([g for g in range(Ng) if g != SPARSE_EDGE_EMPTY_GENE])
    planted = {}
    for start, descending in ((1, False), (c0 + 1, True)):
        for i, n in enumerate(SPARSE_EDGE_ROW_LENGTHS):
            planted[start + i] = (n, descending)
    assert not (set(planted) & empty) and max(planted) < Nc - 1 and len(planted) == 2 * len(SPARSE_EDGE_ROW_LENGTHS)
    plain = [c for c in range(Nc) if c not in empty and c not in planted]
    special = rng.permutation(plain)[:48]
    zeros, dups = set(special[:24].tolist()), set(special[24:].tolist())
    indptr, indices, data = [0], [], []
    for c in range(Nc):
        if c in empty:
            idx, val = np.zeros(0, np.int64), np.zeros(0)
        elif c in planted:
            n, descending = planted[c]
            idx = np.sort(rng.choice(genes[:-1], size=n - (n >= 200), replace=False))
            if n >= 200:
                idx = np.append(idx, Ng - 1)
            idx = idx[::-1] if descending else idx
            val = rng.integers(1, 13, size=idx.size).astype(np.float64)
        else:
            idx = rng.permutation(genes[rng.random(genes.size) < 0.08])
            if idx.size < 2:
                idx = rng.choice(genes, size=2, replace=False)
            val = rng.integers(1, 13, size=idx.size).astype(np.float64)
            if c in zeros:
                free = np.setdiff1d(genes, idx)
                at = int(rng.integers(0, idx.size + 1))
                idx, val = np.insert(idx, at, rng.choice(free)), np.insert(val, at, 0.0)
            if c in dups:
                k = int(rng.integers(0, idx.size))
                idx, val = np.append(idx, idx[k]), np.append(val, float(rng.integers(1, 13)))
        indices.append(idx)
        data.append(val)
        indptr.append(indptr[-1] + idx.size)
    indices, data = np.concatenate(indices), np.concatenate(data)
    dense = np.zeros((Nc, Ng), dtype=np.float64)
    np.add.at(dense, (np.repeat(np.arange(Nc), np.diff(indptr)), indices), data)
    import scipy.sparse as sp
    csr = sp.csr_matrix((data.astype(np.float32), indices.astype(np.int32), np.asarray(indptr, dtype=np.int64)), shape=(Nc, Ng))
    return dense.astype(np.float32), csr
