"""Result / prior containers with the reference's public surface (data holders only):
`Cycle` (reference velocycle/cycle.py:10-466), `AngularSpeed` (angularspeed.py:10-354),
`Phases` (phases.py:103-305).  They are what `fit()` returns and what `preprocess_for_*` consume.

Shared design here: Cycle and AngularSpeed are both "a (2H+1) x N table of means plus one of stds",
so both derive from `_HarmonicTable`.  Quirk kept on purpose: `from_array` labels the
rows nu0, nu1_cos, nu1_sin, ... although the arithmetic order of the basis is [1, sin, cos, ...].
On-disk format (`save`/`load`): one CSV, the means table stacked over the stds table.
"""
from __future__ import annotations

import copy as _copy

import numpy as np
import pandas as pd
import torch


def _row_labels(n_rows: int, swapped: bool):
    first, second = ("cos", "sin") if swapped else ("sin", "cos")
    return ["nu0"] + [f"nu{i // 2 + 1}_{second if i % 2 else first}" for i in range(n_rows - 1)]


def _as_frame(new, like: pd.DataFrame) -> pd.DataFrame:
    if isinstance(new, pd.DataFrame):
        return new
    if torch.is_tensor(new):
        new = new.detach().cpu().numpy()
    if isinstance(new, np.ndarray):
        return pd.DataFrame(new, index=like.index, columns=like.columns)
    raise Exception("Error: invalid type for new values")


class _HarmonicTable:
    def __init__(self):
        self.means: pd.DataFrame = None
        self.stds: pd.DataFrame = None

    def __len__(self):
        return self.shape[-1]

    def __getitem__(self, key):
        out = type(self)()
        out.means = self.means.__getitem__(key)
        out.stds = self.stds.__getitem__(key)
        return out

    def set_means(self, new_means):
        self.means = _as_frame(new_means, self.means)

    def set_stds(self, new_stds):
        self.stds = _as_frame(new_stds, self.stds)

    @property
    def harmonics(self):
        return (self.means.shape[0] - 1) // 2

    @property
    def shape(self):
        return self.means.shape

    @property
    def means_tensor(self):
        return torch.tensor(self.means.values.astype(np.float32))

    @property
    def stds_tensor(self):
        return torch.tensor(self.stds.values.astype(np.float32))

    def save(self, pathname):
        pd.concat([self.means, self.stds]).to_csv(pathname)

    @classmethod
    def load(cls, filepath):
        df = pd.read_csv(filepath, index_col=0)
        half = df.shape[0] // 2
        out = cls()
        out.means, out.stds = df.iloc[:half, :], df.iloc[half:, :]
        return out

    from_file = load

    def copy(self):
        return _copy.deepcopy(self)


class Cycle(_HarmonicTable):
    """Fourier coefficients of every gene: means/stds are (2H+1) x Ng DataFrames."""

    def __init__(self):
        super().__init__()
        self.log_gammas = None
        self.log_betas = None
        self.disp_pyro = None
        self.periodic = None

    def set_log_gammas(self, v):
        self.log_gammas = v

    def set_log_betas(self, v):
        self.log_betas = v

    def set_disp_pyro(self, v):
        self.disp_pyro = v

    @property
    def genes(self):
        return list(self.means.columns)

    @classmethod
    def from_array(cls, means_array, stds_array, gene_names=None):
        means_array, stds_array = np.asarray(means_array), np.asarray(stds_array)
        assert means_array.shape == stds_array.shape, "Shapes of the arrays must be equal"
        if gene_names is not None:
            assert len(gene_names) == means_array.shape[1]
        rows = _row_labels(means_array.shape[0], swapped=True)          # reference cycle.py:321-323
        out = cls()
        out.means = pd.DataFrame(means_array, index=rows, columns=gene_names)
        out.stds = pd.DataFrame(stds_array, index=rows, columns=gene_names)
        return out

    @classmethod
    def trivial_prior(cls, gene_names, harmonics=2, means=0.0, stds=3.0):
        if harmonics == 1:
            stds = np.array([.1, .2, .2])[:, None]
        if harmonics == 2:
            stds = np.array([.1, .2, .2, .1, .1])[:, None]
        nrow = 2 * harmonics + 1
        rows = _row_labels(nrow, swapped=True)
        out = cls()
        out.means = pd.DataFrame(np.broadcast_to(means, (nrow, len(gene_names))).copy(), index=rows, columns=gene_names)
        out.stds = pd.DataFrame(np.broadcast_to(stds, (nrow, len(gene_names))).copy(), index=rows, columns=gene_names)
        return out

    @classmethod
    def from_phases_mle(cls, phases, data, harmonics=1, a=1, noisemodel='Poisson', dispersion=0.3, *, layer='spliced', prior=None,
                        return_fit=False, **worker_kw):
        """The cycle of every gene of `data` given the cells' `phases`: the model of `Phases.from_cycle_mle`
        (mu = exp(nu . zeta(phi)) n_scounts^a, Poisson or NegativeBinomial; reference phases.py:487-507) solved for the gene harmonics,
        one log-link regression on the Fourier design per gene, by the HIP kernel behind `velocycle_amd.gene_harmonics.gene_harmonics`.
        means = the maximum-likelihood coefficients (with `prior`, a Cycle over the same genes and harmonics: the posterior modes under
        its Gaussians), stds = sqrt of the diagonal of the inverse observed Hessian.  `dispersion` may be one value per gene, or "mle"
        (NegativeBinomial): the dispersion of every gene is then estimated with its harmonics and stored as `disp_pyro`, which
        `Phases.from_cycle_mle(cycle, data, noisemodel="NegativeBinomial", dispersion=cycle.disp_pyro)` consumes; the layer may
        be dense or sparse.  Keyword-only: `layer`, `prior`, `return_fit=True` returns (Cycle, GeneHarmonicFit) -- the fit holds the
        log-likelihoods, the likelihood-ratio statistic for periodicity and its p-value, and how every gene's iteration ended; anything
        else goes to the worker (tol, max_iter, device, chunk_genes, storage).  `bootstrap=n > 0` (by name, default 0): the Cycle's
        stds are those of n cell bootstrap replicates (`velocycle_amd.gene_bootstrap.gene_harmonics_bootstrap`, seeded by
        `bootstrap_seed`, default 0) instead of the Hessian's, which understate the spread whenever the noise model does; the means
        are unchanged, and with `return_fit=True` the fit carries the `GeneHarmonicBootstrap` as `fit.bootstrap`.  Not with
        `dispersion="mle"`."""
        from .gene_harmonics import NOISEMODELS, gene_harmonics
        if noisemodel not in NOISEMODELS:
            raise NotImplementedError("Not implemented yet, sorry")
        bootstrap, bootstrap_seed = worker_kw.pop("bootstrap", 0), worker_kw.pop("bootstrap_seed", 0)      # by name only
        if int(bootstrap) != bootstrap or bootstrap < 0:
            raise ValueError("bootstrap must be an integer >= 0 (the number of replicates)")
        if bootstrap and isinstance(dispersion, str):
            raise ValueError("bootstrap with dispersion='mle' is not supported: vc_gene_dispersion knows no weights")
        if layer not in data.layers:
            raise ValueError(f"{layer=} is not a layer of the data")
        counts = data.layers[layer]
        Nc, Ng = counts.shape
        cells_p, cells_d = list(phases.phi_xy.columns), list(data.obs.index)
        named = not isinstance(phases.phi_xy.columns, pd.RangeIndex)
        if phases.phi_xy.shape[1] != Nc or (named and cells_p != cells_d):
            raise ValueError("the cells of the phases do not match the cells of the data (same cells, same order)")
        genes = list(data.var.index)
        prior_means = prior_stds = None
        if prior is not None:
            named = not isinstance(prior.means.columns, pd.RangeIndex)
            if prior.means.shape[1] != Ng or (named and list(prior.means.columns) != genes):
                raise ValueError("the genes of the prior do not match the genes of the data (same genes, same order)")
            if prior.harmonics != harmonics:
                raise ValueError(f"the prior has {prior.harmonics} harmonics, the fit {harmonics}")
            prior_means = np.asarray(prior.means.values, dtype=np.float64)
            prior_stds = np.asarray(prior.stds.values, dtype=np.float64)
        if not (hasattr(counts, "tocsr") or torch.is_tensor(counts)):
            counts = np.asarray(counts)
        fit = gene_harmonics(counts, np.asarray(phases.phi_xy.values, dtype=np.float64), np.asarray(data.obs.n_scounts.values),
                             harmonics=harmonics, a=a, noisemodel=noisemodel, dispersion=dispersion, prior_means=prior_means,
                             prior_stds=prior_stds, **worker_kw)
        stds = fit.stds
        if bootstrap:
            from .gene_bootstrap import gene_harmonics_bootstrap
            run_kw = {k: worker_kw[k] for k in ("tol", "max_iter", "device", "chunk_genes", "storage") if k in worker_kw}
            fit.bootstrap = gene_harmonics_bootstrap(counts, np.asarray(phases.phi_xy.values, dtype=np.float64),
                                                     np.asarray(data.obs.n_scounts.values), harmonics=harmonics, a=a,
                                                     noisemodel=noisemodel, dispersion=dispersion, n_boot=int(bootstrap),
                                                     seed=bootstrap_seed, fit=fit, prior_means=prior_means, prior_stds=prior_stds, **run_kw)
            stds = fit.bootstrap.stds
        out = cls.from_array(fit.means, stds, gene_names=data.var.index)
        if fit.dispersion is not None:                                  # dispersion="mle": the field the reference keeps shape_inv in
            out.set_disp_pyro(fit.dispersion)
        return (out, fit) if return_fit else out

    @classmethod
    def from_joint_mle(cls, phases, data, angular_speed, harmonics=1, condition_design=None, a=1, noisemodel='Poisson', dispersion=0.3, *,
                       prior=None, return_fit=False, **worker_kw):
        """The cycle AND the kinetics of every gene given the cells' `phases` and an `angular_speed` (an `AngularSpeed`, or a scalar or
        one value per cell), fitted jointly to the `spliced` and `unspliced` layers by the HIP kernel behind
        `velocycle_amd.gene_joint.gene_joint` (the V-joint configuration; reference velocity_inference_model.py:360-386,
        with_delta_nu=False).  means / stds = the modes of ν and their Laplace standard errors, `log_gammas` and `log_betas` are set.
        prior: a Cycle over the same genes and harmonics (None: Normal(0, 3)).  `return_fit=True` returns (Cycle, GeneJointFit);
        anything else goes to the worker (kinetics_prior, start, tol, max_iter, device, chunk_genes, storage).
        `bootstrap=n > 0` (by name, default 0): the Cycle's stds are those of n cell bootstrap replicates of the joint fit
        (`velocycle_amd.joint_bootstrap.gene_joint_bootstrap`, seeded by `bootstrap_seed`, default 0: `gene_stds()`) instead of
        Laplace's; the means and the kinetics are unchanged, and with `return_fit=True` the fit carries the `GeneJointBootstrap` as
        `fit.bootstrap`.  Those replicates hold `angular_speed` FIXED at what was handed over: the stds leave out what the uncertainty
        of ω adds to ν, log γ and log β.  For stds that resample ω with the genes use `AngularSpeed.from_joint_mle(..., bootstrap=n,
        return_fit=True)` and `fit.bootstrap.to_cycle(gene_names)`."""
        from .gene_joint import gene_joint
        bootstrap, bootstrap_seed = _bootstrap_options(worker_kw)
        counts_S, counts_U, xy, n, prior_means, prior_stds = _joint_inputs(phases, data, harmonics, noisemodel, prior)
        if isinstance(angular_speed, AngularSpeed):
            Hw = (angular_speed.means.shape[0] - 1) // 2
            speed = dict(nu_omega=np.ascontiguousarray(np.asarray(angular_speed.means.values, dtype=np.float64).T).reshape(-1),
                         harmonics_w=Hw, condition_design=condition_design)
        else:
            speed = dict(omega=angular_speed)
        fit = gene_joint(counts_S, counts_U, xy, n, harmonics=harmonics, a=a, noisemodel=noisemodel, dispersion=dispersion,
                         prior_means=prior_means, prior_stds=prior_stds, **speed, **worker_kw)
        out = fit.to_cycle(list(data.var.index))
        if bootstrap:
            from .joint_bootstrap import gene_joint_bootstrap
            run_kw = {k: worker_kw[k] for k in ("kinetics_prior", "tol", "max_iter", "device", "chunk_genes", "storage") if k in worker_kw}
            fit.bootstrap = gene_joint_bootstrap(counts_S, counts_U, xy, n, harmonics=harmonics, a=a, noisemodel=noisemodel,
                                                 dispersion=dispersion, n_boot=int(bootstrap), seed=bootstrap_seed, fit=fit,
                                                 prior_means=prior_means, prior_stds=prior_stds, **speed, **run_kw)
            out = fit.bootstrap.to_cycle(list(data.var.index))
        return (out, fit) if return_fit else out

    @classmethod
    def from_phases_batch_mle(cls, phases, data, batch_design, harmonics=1, a=1, noisemodel='Poisson', dispersion=0.3, *,
                              layer='spliced', delta_nu_prior=(0.0, 0.5), prior=None, return_fit=False, **worker_kw):
        """`from_phases_mle` for data pooled from several samples: the phase model's per-batch offsets (ElogS = nu . zeta(phi) +
        Db . dnu + count_factor, dnu ~ Normal(mu_dnu, sigma_dnu)) are estimated jointly with the harmonics of every gene, by the HIP
        kernel behind `velocycle_amd.gene_batch.gene_harmonics_batched`.  `batch_design`: the one-hot [cells, batches] matrix of
        `make_design_matrix` (or an integer label per cell); `delta_nu_prior`: (mean, std) of the offsets, scalars or
        [batches, genes].  `dispersion` is a number or one per gene ("mle" is refused).  Returns a Cycle, or with `return_fit=True`
        (Cycle, GeneBatchHarmonicFit): the fit holds `delta_nu` / `delta_nu_stds` [batches, genes], which
        `Phases.from_cycle_batch_mle` consumes, and the likelihood-ratio statistic for periodicity given the batches.
        `bootstrap=n > 0` (by name, default 0): the Cycle's stds are those of n cell bootstrap replicates
        (`velocycle_amd.gene_bootstrap.gene_harmonics_batched_bootstrap`, seeded by `bootstrap_seed`, default 0) instead of the
        Hessian's; the means are unchanged, and with `return_fit=True` the fit carries the `GeneBatchHarmonicBootstrap` (the
        resampled offsets among it) as `fit.bootstrap`."""
        from .gene_batch import gene_harmonics_batched
        from .gene_harmonics import NOISEMODELS
        if noisemodel not in NOISEMODELS:
            raise NotImplementedError("Not implemented yet, sorry")
        bootstrap, bootstrap_seed = worker_kw.pop("bootstrap", 0), worker_kw.pop("bootstrap_seed", 0)      # by name only
        if int(bootstrap) != bootstrap or bootstrap < 0:
            raise ValueError("bootstrap must be an integer >= 0 (the number of replicates)")
        if layer not in data.layers:
            raise ValueError(f"{layer=} is not a layer of the data")
        counts = data.layers[layer]
        Nc, Ng = counts.shape
        cells_p, cells_d = list(phases.phi_xy.columns), list(data.obs.index)
        named = not isinstance(phases.phi_xy.columns, pd.RangeIndex)
        if phases.phi_xy.shape[1] != Nc or (named and cells_p != cells_d):
            raise ValueError("the cells of the phases do not match the cells of the data (same cells, same order)")
        genes = list(data.var.index)
        prior_means = prior_stds = None
        if prior is not None:
            named = not isinstance(prior.means.columns, pd.RangeIndex)
            if prior.means.shape[1] != Ng or (named and list(prior.means.columns) != genes):
                raise ValueError("the genes of the prior do not match the genes of the data (same genes, same order)")
            if prior.harmonics != harmonics:
                raise ValueError(f"the prior has {prior.harmonics} harmonics, the fit {harmonics}")
            prior_means = np.asarray(prior.means.values, dtype=np.float64)
            prior_stds = np.asarray(prior.stds.values, dtype=np.float64)
        if not (hasattr(counts, "tocsr") or torch.is_tensor(counts)):
            counts = np.asarray(counts)
        fit = gene_harmonics_batched(counts, np.asarray(phases.phi_xy.values, dtype=np.float64), np.asarray(data.obs.n_scounts.values),
                                     batch_design, harmonics=harmonics, a=a, noisemodel=noisemodel, dispersion=dispersion,
                                     delta_nu_prior=delta_nu_prior, prior_means=prior_means, prior_stds=prior_stds, **worker_kw)
        stds = fit.stds
        if bootstrap:
            from .gene_bootstrap import gene_harmonics_batched_bootstrap
            run_kw = {k: worker_kw[k] for k in ("tol", "max_iter", "device", "chunk_genes", "storage") if k in worker_kw}
            fit.bootstrap = gene_harmonics_batched_bootstrap(counts, np.asarray(phases.phi_xy.values, dtype=np.float64),
                                                             np.asarray(data.obs.n_scounts.values), batch_design, harmonics=harmonics,
                                                             a=a, noisemodel=noisemodel, dispersion=dispersion, n_boot=int(bootstrap),
                                                             seed=bootstrap_seed, fit=fit, delta_nu_prior=delta_nu_prior,
                                                             prior_means=prior_means, prior_stds=prior_stds, **run_kw)
            stds = fit.bootstrap.stds
        out = cls.from_array(fit.means, stds, gene_names=data.var.index)
        return (out, fit) if return_fit else out


def reorder(cycle: Cycle, gene_list):
    return Cycle.from_array(means_array=cycle.means[gene_list], stds_array=cycle.stds[gene_list])


class AngularSpeed(_HarmonicTable):
    """Fourier coefficients of the angular speed of every condition: (2Hw+1) x Nx DataFrames."""

    @property
    def conditions(self):
        return list(self.means.columns)

    @classmethod
    def from_array(cls, means_array, stds_array, condition_names=None, Nhω=0):
        means_array, stds_array = np.asarray(means_array), np.asarray(stds_array)
        assert means_array.shape == stds_array.shape, "Shapes of the arrays must be equal"
        rows = _row_labels(max(int(Nhω), 1), swapped=True)

        def table(a):
            df = pd.DataFrame([a]) if len(rows) == 1 else pd.DataFrame(np.asarray(a).squeeze())
            if len(df.index) == len(rows):
                df.index, df.columns = rows, condition_names
                return df
            df.index, df.columns = condition_names, rows
            return df.T
        out = cls()
        out.means, out.stds = table(means_array), table(stds_array)
        return out

    @classmethod
    def trivial_prior(cls, condition_names, harmonics=1, means=0.0, stds=3.0):
        nrow = 2 * harmonics + 1
        rows = _row_labels(nrow, swapped=True)
        mu = np.array([means] + [0.0] * (nrow - 1), dtype=np.float32)[:, None]
        sd = np.array([stds] + [0.05] * (nrow - 1), dtype=np.float32)[:, None]
        out = cls()
        out.means = pd.DataFrame(np.broadcast_to(mu, (nrow, len(condition_names))).copy(), index=rows, columns=condition_names)
        out.stds = pd.DataFrame(np.broadcast_to(sd, (nrow, len(condition_names))).copy(), index=rows, columns=condition_names)
        return out

    @classmethod
    def from_kinetics_mle(cls, cycle, phases, data, harmonics=0, condition_design=None, noisemodel='Poisson', dispersion=0.3, *,
                          layer='unspliced', prior=None, return_fit=False, **worker_kw):
        """The MAP angular speed of the velocity stage conditioned on `cycle` (ν) and `phases` (ϕxy), with every gene's log γ and log β
        profiled out under the model's priors (reference velocity_inference_model.py:360-386, with_delta_nu=False; Poisson or
        NegativeBinomial), by the HIP kernel behind `velocycle_amd.gene_kinetics.velocity_map`.  harmonics: Hω; condition_design:
        [Nx, Nc] (None: one condition); prior: an `AngularSpeed` over the conditions (None: `trivial_prior`).  means = the mode, stds =
        sqrt of the diagonal of the inverse profile information (a Laplace standard error), both in this class's row layout.
        `return_fit=True` returns (AngularSpeed, VelocityMapFit); `fit.to_cycle(cycle)` is a copy of the cycle with `log_gammas` and
        `log_betas` set.  Anything else goes to the worker (a, tol, max_iter, tol_outer, max_rounds, device, chunk_genes, storage, ...).
        `bootstrap=n > 0` (by name, default 0): n cell bootstrap replicates of the fit
        (`velocycle_amd.kinetics_bootstrap.velocity_map_bootstrap`, seeded by `bootstrap_seed`, default 0) are run as well and, with
        `return_fit=True`, hang on the fit as `fit.bootstrap` (a `VelocityMapBootstrap`: `contrast_std(a, b)` is the standard error of
        ln(ω_a / ω_b) whatever the noise model).  The returned means and stds are unchanged: the replicates carry sampling
        variability and do not replace the Laplace width of an absolute ω."""
        from .gene_kinetics import NOISEMODELS, velocity_map
        bootstrap, bootstrap_seed = worker_kw.pop("bootstrap", 0), worker_kw.pop("bootstrap_seed", 0)      # by name only
        if isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, np.integer)) or bootstrap < 0:
            raise ValueError("bootstrap must be an integer >= 0 (the number of replicates)")
        if noisemodel not in NOISEMODELS:
            raise NotImplementedError("Not implemented yet, sorry")
        if layer not in data.layers:
            raise ValueError(f"{layer=} is not a layer of the data")
        counts = data.layers[layer]
        Nc, Ng = counts.shape
        named = not isinstance(phases.phi_xy.columns, pd.RangeIndex)
        if phases.phi_xy.shape[1] != Nc or (named and list(phases.phi_xy.columns) != list(data.obs.index)):
            raise ValueError("the cells of the phases do not match the cells of the data (same cells, same order)")
        named = not isinstance(cycle.means.columns, pd.RangeIndex)
        if cycle.means.shape[1] != Ng or (named and list(cycle.means.columns) != list(data.var.index)):
            raise ValueError("the genes of the cycle do not match the genes of the data (same genes, same order)")
        Nx = 1 if condition_design is None else int(np.asarray(condition_design).shape[0])
        names = list(prior.means.columns) if prior is not None else list(range(Nx))
        if not (hasattr(counts, "tocsr") or torch.is_tensor(counts)):
            counts = np.asarray(counts)
        fit = velocity_map(counts, np.asarray(phases.phi_xy.values, dtype=np.float64), np.asarray(data.obs.n_scounts.values),
                           np.asarray(cycle.means.values, dtype=np.float64), harmonics_w=harmonics, condition_design=condition_design,
                           noisemodel=noisemodel, dispersion=dispersion, nuw_prior=prior, **worker_kw)
        if bootstrap:
            from .kinetics_bootstrap import velocity_map_bootstrap
            fit.bootstrap = velocity_map_bootstrap(counts, np.asarray(phases.phi_xy.values, dtype=np.float64),
                                                   np.asarray(data.obs.n_scounts.values), np.asarray(cycle.means.values, dtype=np.float64),
                                                   harmonics_w=harmonics, condition_design=condition_design, noisemodel=noisemodel,
                                                   dispersion=dispersion, n_boot=int(bootstrap), seed=bootstrap_seed, fit=fit,
                                                   nuw_prior=prior, **worker_kw)
        rows = _row_labels(fit.nu_omega.shape[0], swapped=True)
        out = cls()
        out.means = pd.DataFrame(fit.nu_omega, index=rows, columns=names)
        out.stds = pd.DataFrame(fit.stds, index=rows, columns=names)
        return (out, fit) if return_fit else out

    @classmethod
    def from_joint_mle(cls, cycle_prior, phases, data, harmonics=0, condition_design=None, noisemodel='Poisson', dispersion=0.3, *,
                       cycle_harmonics=1, prior=None, return_fit=False, **worker_kw):
        """The MAP angular speed of the V-joint configuration: conditioned on the `phases` only, with every gene's ν, log γ and log β
        profiled out over the `spliced` and `unspliced` layers under their priors, by the HIP kernel behind
        `velocycle_amd.gene_joint.velocity_map_joint`.  cycle_prior: a Cycle over the same genes whose means and stds are ν's prior
        (None: Normal(0, 3) at `cycle_harmonics` harmonics); harmonics: Hω; condition_design: [Nx, Nc] (None: one condition); prior:
        an `AngularSpeed` over the conditions (None: `trivial_prior`).  `return_fit=True` returns (AngularSpeed, JointVelocityMapFit);
        `fit.to_cycle(gene_names)` is the jointly fitted Cycle.  Anything else goes to the worker (a, kinetics_prior, start, tol,
        max_iter, tol_outer, max_rounds, device, chunk_genes, storage).
        `bootstrap=n > 0` (by name, default 0): n cell bootstrap replicates of the fit
        (`velocycle_amd.joint_bootstrap.velocity_map_joint_bootstrap`, seeded by `bootstrap_seed`, default 0, genes kept) are run as
        well and, with `return_fit=True`, hang on the fit as `fit.bootstrap` (a `JointVelocityMapBootstrap`: `contrast_std(a, b)` is the
        standard error of ln(ω_a / ω_b) whatever the noise model; `to_cycle` the joint cycle with bootstrap stds).  The returned means
        and stds are unchanged: the replicates carry sampling variability and do not replace the Laplace width of an absolute ω."""
        from .gene_joint import velocity_map_joint
        bootstrap, bootstrap_seed = _bootstrap_options(worker_kw)
        H = cycle_prior.harmonics if cycle_prior is not None else cycle_harmonics
        counts_S, counts_U, xy, n, prior_means, prior_stds = _joint_inputs(phases, data, H, noisemodel, cycle_prior)
        Nx = 1 if condition_design is None else int(np.asarray(condition_design).shape[0])
        names = list(prior.means.columns) if prior is not None else list(range(Nx))
        fit = velocity_map_joint(counts_S, counts_U, xy, n, harmonics=H, harmonics_w=harmonics, condition_design=condition_design,
                                 noisemodel=noisemodel, dispersion=dispersion, prior_means=prior_means, prior_stds=prior_stds,
                                 nuw_prior=prior, **worker_kw)
        if bootstrap:
            from .joint_bootstrap import velocity_map_joint_bootstrap
            run_kw = {k: v for k, v in worker_kw.items() if k != "start"}          # the replicates start at the fit
            fit.bootstrap = velocity_map_joint_bootstrap(counts_S, counts_U, xy, n, harmonics=H, harmonics_w=harmonics,
                                                         condition_design=condition_design, noisemodel=noisemodel, dispersion=dispersion,
                                                         n_boot=int(bootstrap), seed=bootstrap_seed, fit=fit, keep_genes=True,
                                                         prior_means=prior_means, prior_stds=prior_stds, nuw_prior=prior, **run_kw)
        rows = _row_labels(fit.nu_omega.shape[0], swapped=True)
        out = cls()
        out.means = pd.DataFrame(fit.nu_omega, index=rows, columns=names)
        out.stds = pd.DataFrame(fit.stds, index=rows, columns=names)
        return (out, fit) if return_fit else out


def _bootstrap_options(worker_kw):
    """(bootstrap, bootstrap_seed) taken out of a worker's keywords: by name only, default 0."""
    bootstrap, bootstrap_seed = worker_kw.pop("bootstrap", 0), worker_kw.pop("bootstrap_seed", 0)
    if isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, np.integer)) or bootstrap < 0:
        raise ValueError("bootstrap must be an integer >= 0 (the number of replicates)")
    if isinstance(bootstrap_seed, bool) or not isinstance(bootstrap_seed, (int, np.integer)) or bootstrap_seed < 0:
        raise ValueError("bootstrap_seed must be an integer >= 0")
    return int(bootstrap), int(bootstrap_seed)


def _joint_inputs(phases, data, harmonics, noisemodel, prior):
    """What `Cycle.from_joint_mle` and `AngularSpeed.from_joint_mle` read from their containers: (spliced, unspliced, directions,
    n_scounts, prior means, prior stds), refused as `from_phases_mle` / `from_kinetics_mle` refuse."""
    if noisemodel not in ("Poisson", "NegativeBinomial"):
        raise NotImplementedError("Not implemented yet, sorry")
    for layer in ("spliced", "unspliced"):
        if layer not in data.layers:
            raise ValueError(f"{layer=} is not a layer of the data")
    counts = [data.layers["spliced"], data.layers["unspliced"]]
    Nc, Ng = counts[0].shape
    named = not isinstance(phases.phi_xy.columns, pd.RangeIndex)
    if phases.phi_xy.shape[1] != Nc or (named and list(phases.phi_xy.columns) != list(data.obs.index)):
        raise ValueError("the cells of the phases do not match the cells of the data (same cells, same order)")
    prior_means = prior_stds = None
    if prior is not None:
        named = not isinstance(prior.means.columns, pd.RangeIndex)
        if prior.means.shape[1] != Ng or (named and list(prior.means.columns) != list(data.var.index)):
            raise ValueError("the genes of the prior do not match the genes of the data (same genes, same order)")
        if prior.harmonics != harmonics:
            raise ValueError(f"the prior has {prior.harmonics} harmonics, the fit {harmonics}")
        prior_means = np.asarray(prior.means.values, dtype=np.float64)
        prior_stds = np.asarray(prior.stds.values, dtype=np.float64)
    counts = [c if (hasattr(c, "tocsr") or torch.is_tensor(c)) else np.asarray(c) for c in counts]
    return counts[0], counts[1], np.asarray(phases.phi_xy.values, dtype=np.float64), np.asarray(data.obs.n_scounts.values), prior_means, prior_stds


class Phases:
    """Cell phases as 2 x Nc direction vectors (rows phi_x, phi_y)."""

    def __init__(self):
        self.phi_xy: pd.DataFrame = None
        self.omegas = None

    def __len__(self):
        return self.shape[-1]

    @property
    def shape(self):
        return self.phi_xy.shape

    def set_phixy(self, new_phixy):
        self.phi_xy = _as_frame(new_phixy, self.phi_xy)

    def set_omegas(self, new_omegas):
        self.omegas = new_omegas

    @property
    def phi_xy_tensor(self):
        return torch.tensor(self.phi_xy.values.astype(np.float32))

    @property
    def phis(self):
        xy = self.phi_xy_tensor.T
        phis = torch.atan2(xy[..., 1], xy[..., 0])
        phis[phis < 0] = phis[phis < 0] + 2 * np.pi
        return phis

    @property
    def directions(self):
        return np.arctan2(self.phi_xy.values[1, :], self.phi_xy.values[0, :]) % (2 * np.pi)

    @property
    def concentrations(self):
        return np.sqrt(np.sum(self.phi_xy.values ** 2, 0))

    @classmethod
    def from_array(cls, phi_xy_array, cell_names=None):
        phi_xy_array = np.asarray(phi_xy_array)
        assert phi_xy_array.shape[0] == 2, "Shape of the array is incorrect"
        if cell_names is not None:
            assert len(cell_names) == phi_xy_array.shape[1]
        out = cls()
        out.phi_xy = pd.DataFrame(phi_xy_array, index=["phi_x", "phi_y"], columns=cell_names)
        return out

    @classmethod
    def from_pca_heuristic(cls, anndata_object, genes_to_use=None, concentration=1.0, layer="S_sz", small_count=1.0e-1,
                           normalize_pcs=True, zero_at_min_density=False, random_state=0, plot=False, n_components=2, *,
                           device=None, tol=1e-6, max_iter=200, chunk_cells=None):
        """Phase prior from the angle in the plane of the first two principal components of the log counts
        (reference phases.py:307-382; the step right before phase inference in the tutorials).
        Keyword-only: with `device` ("cuda", "cuda:N"; "cpu" runs the same loop on torch) the logarithm and the components are
        computed on the device by `velocycle_amd.phase_prior.pca_scores` (a block power iteration to `tol`, at most `max_iter`
        passes, the layer staged in chunks of `chunk_cells` cells; `random_state` seeds its start block); `.pca` is then that
        function's record and not an sklearn object.  With device=None: the host path, sklearn's PCA."""
        if layer not in anndata_object.layers:
            raise ValueError(f"{layer=} is not a valid entry anndata.obs")
        sub = anndata_object if genes_to_use is None else \
            anndata_object[:, [g in genes_to_use for g in anndata_object.var.index]]
        mat = sub.layers[layer]
        if device is not None:
            if plot:
                raise ValueError("plot=True is not available with device=...: plot from the returned .pcs")
            if n_components < 2:
                raise ValueError("the phase is an angle in the plane of two components: n_components must be >= 2")
            from .phase_prior import pca_scores
            pca = pca_scores(mat, small_count, n_components, device=device, random_state=random_state, tol=tol, max_iter=max_iter,
                             chunk_cells=chunk_cells)
            pcs = pca.pcs.cpu().numpy()
        else:
            from sklearn.decomposition import PCA
            mat = mat.toarray() if hasattr(mat, "toarray") else np.asarray(mat)
            X = np.log(mat + small_count)                                   # cells x genes
            pca = PCA(n_components, random_state=random_state)
            pcs = pca.fit_transform(X)
        if normalize_pcs:
            lo, hi, med = np.percentile(pcs, [0.5, 99.5, 50], 0)
            pcs = (pcs - med) / (hi - lo)
        angle = np.arctan2(pcs[:, 1], pcs[:, 0]) % (2 * np.pi)
        if zero_at_min_density:          # put phase 0 right after the widest gap of the sorted angles
            order = np.argsort(angle)
            start = order[np.diff(angle[order]).argmax() + 1]
            angle = (angle - angle[start]) % (2 * np.pi)
        out = cls.from_array(np.vstack([np.cos(angle), np.sin(angle)]) * concentration,
                             cell_names=anndata_object.obs.index)
        out.pcs, out.pca = pcs, pca
        return out

    def max_corr(self, counts, npoints=100):
        """Shift (out of `npoints` equally spaced ones) maximising the correlation of the phases with `counts`
        (reference phases.py:450-469).  Returns (shift, correlation, all correlations)."""
        shifts = np.arange(0, npoints) / npoints * 2 * np.pi
        phis = self.phis.numpy()
        corr = []
        for s in shifts:
            x = phis - s
            x[x < 0] += 2 * np.pi
            corr.append(np.corrcoef(x, counts)[0, 1])
        i = int(np.argmax(np.array(corr)))
        return shifts[i], corr[i], corr

    def from_cycle_mle(self, cycle, data, a=1, bins=100, concentration=10., noisemodel='Poisson', dispersion=0.3, *,
                       device=None, chunk_cells=None, return_profile=False):
        """Gives every cell the phase, out of `bins` equally spaced ones, that maximises the likelihood of its spliced counts
        under the fitted `cycle` (reference phases.py:471-509; in place: `set_phixy(concentration * (cos phi, sin phi))`).
        The likelihood grid is evaluated by the HIP kernel behind `velocycle_amd.phase_mle.phase_mle`; nothing of size
        bins x genes x cells is stored.  `dispersion` may also be one value per gene (e.g. a fitted cycle's `disp_pyro`).
        Keyword-only: `device`, `chunk_cells` (cells per device block; the result does not depend on it),
        `return_profile=True` returns (best_bin, logP - max logP) as device tensors; otherwise None like the reference."""
        from .phase_mle import NOISEMODELS, phase_mle
        from .utils import torch_fourier_basis, unpack_direction
        if noisemodel not in NOISEMODELS:
            raise NotImplementedError("Not implemented yet, sorry")
        if int(bins) != bins or bins < 1:
            raise ValueError("bins must be an integer >= 1")
        bins = int(bins)
        means = np.asarray(cycle.means.values, dtype=np.float64)
        layer = data.layers['spliced']
        Nc, Ng = layer.shape
        genes_c, genes_d = list(cycle.means.columns), list(data.var.index)
        named = not isinstance(cycle.means.columns, pd.RangeIndex)
        if means.shape[1] != Ng or (named and genes_c != genes_d):
            raise ValueError("the genes of the cycle do not match the genes of the data (same genes, same order)")
        n_scounts = np.asarray(data.obs.n_scounts.values, dtype=np.float64)
        if not (np.isfinite(n_scounts).all() and (n_scounts > 0).all()):
            raise ValueError("every cell needs n_scounts > 0")
        if noisemodel == 'NegativeBinomial' and not (np.asarray(dispersion, dtype=np.float64) > 0).all():
            raise ValueError("dispersion must be > 0")
        # the grid exactly as the reference builds it (float32 phases; :495-498), the table itself in float64
        phis = (2 * np.pi * torch.arange(0, 1, 1. / bins, dtype=torch.float32))[:bins]
        basis = torch_fourier_basis(phis, num_harmonics=(means.shape[0] - 1) // 2)
        T = basis.double() @ torch.tensor(means)
        m = torch.tensor(n_scounts) ** float(a)
        if not (hasattr(layer, "tocsr") or torch.is_tensor(layer)):
            layer = np.asarray(layer)
        best, prof = phase_mle(layer, T, m, noisemodel=noisemodel, dispersion=dispersion, device=device,
                               chunk_cells=chunk_cells, return_profile=return_profile)
        xy = (concentration * unpack_direction(phis[best.cpu()])).T
        if self.phi_xy is None:
            self.phi_xy = pd.DataFrame(xy.numpy(), index=["phi_x", "phi_y"], columns=data.obs.index)
        else:
            self.set_phixy(xy)
        return (best, prof) if return_profile else None

    def from_cycle_batch_mle(self, cycle, data, batch_design, delta_nu, a=1, bins=100, concentration=10., noisemodel='Poisson',
                             dispersion=0.3, *, device=None, chunk_cells=None):
        """`from_cycle_mle` under given per-batch offsets `delta_nu` [batches, genes] (a `GeneBatchHarmonicFit.delta_nu`, or the SVI's
        Δν means): the cells of batch b are assigned on the table T + delta_nu[b], one call of the same HIP grid kernel per batch on
        that batch's cells, and the bins are scattered back.  `batch_design`: one-hot [cells, batches] or an integer label per cell.
        In place like `from_cycle_mle`; with one batch and delta_nu = 0 it gives its bits."""
        from .gene_batch import batch_labels
        from .phase_mle import NOISEMODELS, phase_mle
        from .utils import torch_fourier_basis, unpack_direction
        if noisemodel not in NOISEMODELS:
            raise NotImplementedError("Not implemented yet, sorry")
        if int(bins) != bins or bins < 1:
            raise ValueError("bins must be an integer >= 1")
        bins = int(bins)
        means = np.asarray(cycle.means.values, dtype=np.float64)
        layer = data.layers['spliced']
        Nc, Ng = layer.shape
        genes_c, genes_d = list(cycle.means.columns), list(data.var.index)
        named = not isinstance(cycle.means.columns, pd.RangeIndex)
        if means.shape[1] != Ng or (named and genes_c != genes_d):
            raise ValueError("the genes of the cycle do not match the genes of the data (same genes, same order)")
        n_scounts = np.asarray(data.obs.n_scounts.values, dtype=np.float64)
        if not (np.isfinite(n_scounts).all() and (n_scounts > 0).all()):
            raise ValueError("every cell needs n_scounts > 0")
        if noisemodel == 'NegativeBinomial' and not (np.asarray(dispersion, dtype=np.float64) > 0).all():
            raise ValueError("dispersion must be > 0")
        labels, Nb = batch_labels(batch_design, Nc)
        dnu = np.asarray(delta_nu.detach().cpu().numpy() if torch.is_tensor(delta_nu) else delta_nu, dtype=np.float64)
        if dnu.shape != (Nb, Ng):
            raise ValueError(f"delta_nu must be [batches, genes] = ({Nb}, {Ng}), got {dnu.shape}")
        if not np.isfinite(dnu).all():
            raise ValueError("delta_nu must be finite")
        phis = (2 * np.pi * torch.arange(0, 1, 1. / bins, dtype=torch.float32))[:bins]
        basis = torch_fourier_basis(phis, num_harmonics=(means.shape[0] - 1) // 2)
        T = basis.double() @ torch.tensor(means)
        m = torch.tensor(n_scounts) ** float(a)
        if not (hasattr(layer, "tocsr") or torch.is_tensor(layer)):
            layer = np.asarray(layer)
        elif hasattr(layer, "tocsr"):
            layer = layer.tocsr()
        best = torch.empty(Nc, dtype=torch.int64)
        for b in range(Nb):
            idx = np.flatnonzero(labels == b)
            sub = layer[torch.as_tensor(idx)] if torch.is_tensor(layer) else layer[idx]
            got, _ = phase_mle(sub, T + torch.tensor(dnu[b])[None, :], m[idx], noisemodel=noisemodel, dispersion=dispersion, device=device,
                               chunk_cells=chunk_cells)
            best[idx] = got.cpu()
        xy = (concentration * unpack_direction(phis[best])).T
        if self.phi_xy is None:
            self.phi_xy = pd.DataFrame(xy.numpy(), index=["phi_x", "phi_y"], columns=data.obs.index)
        else:
            self.set_phixy(xy)
        return None

    @classmethod
    def from_phase_marginal(cls, record, cell_names=None, concentration=None):
        """Phases from a `velocycle_amd.predictive.PhaseMarginal`: ϕxy = kappa (cos, sin) of every cell's posterior circular mean.
        kappa: `concentration` if given; otherwise, per cell, the kappa whose projected normal -- the angle of Normal(kappa u, I), which
        is what the model makes of a ϕxy prior -- has the record's mean resultant length (a monotone 1-D inversion on the host)."""
        from .predictive import concentration_of_resultant
        mean = record.mean_phase.double().numpy()
        kappa = np.full(mean.shape, float(concentration)) if concentration is not None else \
            concentration_of_resultant(record.resultant_length).numpy()
        return cls.from_array(np.vstack([np.cos(mean), np.sin(mean)]) * kappa, cell_names=cell_names)

    def shift_zero(self, gene=None, phase=None):
        if gene is not None:
            raise Exception("Error: must phase for desired shift")
        if phase is None:
            raise Exception("Error: must specify gene or phase for desired shift")
        ph = self.phis - phase
        self.set_phixy(torch.stack([torch.cos(ph), torch.sin(ph)], dim=-1).T)

    @classmethod
    def flat_prior(cls, anndata_object):
        n = anndata_object.shape[0]
        return cls.from_array(np.zeros((2, n)), cell_names=list(anndata_object.obs.index))

    def rotate(self, angle=None):
        if angle is None:
            raise Exception("Error: must specify angle for desired rotation")
        c, s = np.cos(angle), np.sin(angle)
        rot = np.array([[c, -s], [s, c]])
        self.phi_xy = pd.DataFrame(rot @ self.phi_xy.values, index=self.phi_xy.index, columns=self.phi_xy.columns)

    def invert_direction(self):
        self.phi_xy = pd.DataFrame(self.phi_xy.values * np.array([[1.0], [-1.0]]), index=self.phi_xy.index,
                                   columns=self.phi_xy.columns)

    def save(self, pathname):
        self.phi_xy.to_csv(pathname)

    @classmethod
    def load(cls, filepath):
        out = cls()
        out.phi_xy = pd.read_csv(filepath, index_col=0)
        return out

    from_file = load
