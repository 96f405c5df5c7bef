"""Cell bootstrap of the MAP angular speed (`gene_kinetics.velocity_map` / `AngularSpeed.from_kinetics_mle`) on the HIP kernel
`vc_gene_kinetics_weighted`.

`VelocityMapFit.stds` are Laplace standard errors from the Fisher profile information of the assumed noise model: right when that model
is, too narrow when a Poisson fit (the default) meets overdispersed counts.  Replicate b draws a Poisson(1) integer weight per cell
(the draw of `gene_bootstrap.draw_weights`: the same seed resamples the same cells as `gene_harmonics_bootstrap`) and runs
`velocity_map`'s outer iteration again under those case weights; all replicates iterate side by side, one kernel call per chunk and
round over the rows still iterating, each row at its own trial νω and its own previous (log gamma, log beta).

What the replicates measure is SAMPLING VARIABILITY.  For identified contrasts between conditions -- ln(ω_a / ω_b), the comparison the
method exists for -- their spread validates the Laplace error where the noise model holds and replaces it where it does not (a Poisson
fit of negative-binomial counts at r = 3: Laplace 0.022, bootstrap 0.066).  It is NOT a replacement for the Laplace width of the
absolute ω: that width is limited by the prior of gamma, which fixes the time scale and is common to all conditions, and resampling
cells cannot see it (there the bootstrap spread is 4-6 times narrower than the Laplace std).  Nothing here overwrites
`VelocityMapFit.stds`.

Limits: the cycle is held at `means` unless jointly resampled replicates are handed over (`means_replicates`); the dispersion is not
estimated again (`vc_gene_dispersion` knows no weights); no batch offsets; at most 3 coefficients of the angular speed; the cells are not
sharded; no Lognormal noise.  There is no CPU fallback."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from .gene_harmonics import MAX_WEIGHT_ROWS, _check_run_options, _row_sums, check_weights
from .gene_kinetics import (DEFAULT_PRIOR, EPS32, MAP_STATUS, MAX_OUTER_HALVINGS, VelocityMapFit, _nuw_prior, _Problem, _solve_spd,
                            check_arguments, omega_design, velocity_map)

MAX_OUTPUT_BYTES = 1 << 30           # the device outputs of one kernel call over all rows


@dataclass
class VelocityMapBootstrap:
    """Host arrays.  nu_omega_replicates: float64 [R, 2 Hω + 1, Nx] in `AngularSpeed`'s row layout; status: [R] strings of
    `gene_kinetics.MAP_STATUS`; rounds, n_excluded: int64 [R]; F, dec: float64 [R] (the profiled log-posterior under the replicate's
    weights and its last outer decrement); fit: the full-data `VelocityMapFit`; log_gamma_replicates, log_beta_replicates float64
    [R, Ng] and kinetics_status int32 [R, Ng] when they were kept; weights: the float32 [R, Nc] table when it was asked for.

    Every summary runs over the `ok` replicates (CONVERGED).  The replicates carry sampling variability: use `contrast` and its
    standard error for comparisons between conditions; the spread of an absolute ω leaves out what the prior of gamma contributes to
    `fit.stds` and does not replace them (see the module's docstring)."""
    nu_omega_replicates: np.ndarray
    status: np.ndarray
    rounds: np.ndarray
    n_excluded: np.ndarray
    F: np.ndarray
    dec: np.ndarray
    fit: Optional[VelocityMapFit] = None
    log_gamma_replicates: Optional[np.ndarray] = None
    log_beta_replicates: Optional[np.ndarray] = None
    kinetics_status: Optional[np.ndarray] = None
    weights: Optional[np.ndarray] = None

    @property
    def ok(self):
        """bool [R]"""
        return np.asarray(self.status) == "CONVERGED"

    @property
    def n_ok(self):
        return int(self.ok.sum())

    def _kept(self):
        return self.nu_omega_replicates[self.ok]

    @property
    def means(self):
        """[2 Hω + 1, Nx]; NaN without an ok replicate."""
        k = self._kept()
        return k.mean(0) if len(k) else np.full(self.nu_omega_replicates.shape[1:], np.nan)

    @property
    def cov(self):
        """[NW, NW] over the coefficients condition-major (i = x (2 Hω + 1) + h, like `VelocityMapFit.cov`), ddof 1; NaN below 2 ok
        replicates."""
        k = self._kept()
        flat = k.transpose(0, 2, 1).reshape(len(k), k.shape[1] * k.shape[2])
        if len(k) < 2:
            return np.full((flat.shape[1], flat.shape[1]), np.nan)
        d = flat - flat.mean(0)
        return d.T @ d / (len(k) - 1)

    @property
    def stds(self):
        """[2 Hω + 1, Nx], ddof 1; NaN below 2 ok replicates.  Sampling variability only: not the width of an absolute ω."""
        Nhw, Nx = self.nu_omega_replicates.shape[1:]
        return np.ascontiguousarray(np.sqrt(np.diag(self.cov)).reshape(Nx, Nhw).T)

    @property
    def bias(self):
        return self.means - self.fit.nu_omega

    def interval(self, level=0.95):
        """Percentile interval (low, high) at `level` over the ok replicates, [2 Hω + 1, Nx] each."""
        return _percentiles(self._kept(), level)

    def contrast(self, a, b, log=True):
        """[R]: ln(ν0[a] / ν0[b]) of every replicate, ν0 the constant coefficient of conditions a and b (log=False: ν0[a] - ν0[b]);
        NaN where a speed is not positive."""
        Nx = self.nu_omega_replicates.shape[2]
        if not (int(a) == a and int(b) == b and 0 <= a < Nx and 0 <= b < Nx):
            raise ValueError(f"conditions {a}, {b} of a fit with {Nx}")
        va, vb = self.nu_omega_replicates[:, 0, int(a)], self.nu_omega_replicates[:, 0, int(b)]
        if not log:
            return va - vb
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where((va > 0) & (vb > 0), np.log(va / vb), np.nan)

    def contrast_std(self, a, b, log=True):
        """The standard deviation (ddof 1) of the contrast over the ok replicates; NaN below 2."""
        c = self.contrast(a, b, log)[self.ok]
        return float(np.std(c, ddof=1)) if len(c) >= 2 else float("nan")

    def contrast_interval(self, a, b, level=0.95, log=True):
        """Percentile interval (low, high) of the contrast at `level` over the ok replicates."""
        lo, hi = _percentiles(self.contrast(a, b, log)[self.ok], level)
        return float(lo), float(hi)


def _percentiles(kept, level):
    if not 0 < level < 1:
        raise ValueError("level must be in (0, 1)")
    if not len(kept):
        nan = np.full(kept.shape[1:], np.nan)
        return nan, nan.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanquantile(kept, (1 - level) / 2, axis=0), np.nanquantile(kept, (1 + level) / 2, axis=0)


def check_bootstrap_arguments(Nc, Ng, K, NW, Nhw, n_boot, weights, means_replicates, fit):
    """The refusals of `velocity_map_bootstrap` that need no device.  Returns (the float32 host table or None, R, the per-row cycles
    float64 [R, Ng, K] or None)."""
    w_host = None
    if weights is not None:
        w_host = check_weights(weights.detach().cpu() if torch.is_tensor(weights) else weights, Nc)
        R = w_host.shape[0]
    else:
        if isinstance(n_boot, bool) or int(n_boot) != n_boot or not 1 <= n_boot <= MAX_WEIGHT_ROWS:
            raise ValueError(f"n_boot must be an integer in 1..{MAX_WEIGHT_ROWS}")
        R = int(n_boot)
    NWH = NW * (NW + 1) // 2
    if R * Ng * (8 * (2 + 1 + 1 + NW + NWH) + 4 * 3) > MAX_OUTPUT_BYTES:
        raise ValueError(f"the device outputs of {R} replicates x {Ng} genes exceed 1 GiB: bootstrap fewer genes or replicates per call")
    nu_rep = None
    if means_replicates is not None:
        rep = np.asarray(means_replicates, dtype=np.float64)
        if rep.shape != (R, K, Ng):
            raise ValueError(f"means_replicates must be [replicates, 2 harmonics + 1, genes] = ({R}, {K}, {Ng}), got {rep.shape}")
        nu_rep = np.ascontiguousarray(rep.transpose(0, 2, 1))
    if fit is not None:
        shapes = (np.shape(fit.nu_omega), np.shape(fit.included), np.shape(fit.kinetics.log_gamma), np.shape(fit.kinetics.log_beta))
        if shapes != ((Nhw, NW // Nhw), (Ng,), (Ng,), (Ng,)):
            raise ValueError(f"fit must be the VelocityMapFit of this problem: nu_omega [{Nhw}, {NW // Nhw}], included and kinetics [{Ng}]; "
                             f"got {shapes}")
    return w_host, R, nu_rep


def velocity_map_bootstrap(counts_U, directions, n_scounts, means, harmonics_w=0, condition_design=None, a=1, noisemodel="Poisson",
                           dispersion=0.3, *, n_boot=200, seed=0, weights=None, fit=None, means_replicates=None, warm_start=True,
                           keep_kinetics=False, return_weights=False, prior=DEFAULT_PRIOR, nuw_prior=None, nuw_start=None, tol=1e-10,
                           max_iter=25, tol_outer=1e-8, max_rounds=30, device=None, chunk_genes=None, storage="auto"):
    """counts_U, directions, n_scounts, means, harmonics_w, condition_design, a, noisemodel, dispersion (a number or one per gene), prior,
    nuw_prior, nuw_start, tol, max_iter, tol_outer, max_rounds, device, chunk_genes, storage: as for `velocity_map`.  Returns a
    `VelocityMapBootstrap` of `n_boot` replicates of the MAP angular speed.

    weights=None: the table is `gene_bootstrap.draw_weights(n_boot, Nc, seed, dev)`, a pure function of (seed, b, c): the same seed
    resamples the same cells as `gene_harmonics_bootstrap`, and the first 2 rows of a 4-row run are the 2-row run's.  weights=[R, Nc]:
    the caller's table (finite, >= 0; n_boot is then R).  fit: the full-data `VelocityMapFit` (None: `velocity_map` is run first with the
    same arguments); it is returned as `.fit`.  warm_start: every replicate starts at `fit`'s νω and at `fit.kinetics`' (log gamma,
    log beta) (False: at `nuw_start` or the prior means and the kernel's default start, as `velocity_map` does).

    The outer iteration is `velocity_map`'s, per row: G, J, the step, the decrement, the halving (at most 10), `max_rounds` and the
    statuses are its own rules, the genes' values summed per row by halving.  A replicate leaves out the genes `fit` left out, those
    whose first-round status under its weights is not CONVERGED / ROUNDING, and with `means_replicates` ([R, 2H+1, Ng], e.g.
    `GeneHarmonicBootstrap.replicates` drawn with the same seed: the cycle resampled jointly) those whose replicate ν is not finite.
    A replicate whose J is not positive definite ends STALLED.  A replicate's result is a function of its weight row and its starts
    alone: not of R, of the other rows or of the chunking.  keep_kinetics: also return every replicate's (log gamma, log beta) and
    kernel status; return_weights: the table.

    tol_outer: `velocity_map` has no rounding rule in its outer iteration and neither has this: where the float32 sums of a large problem
    (50 000 x 2 000) do not resolve the default 1e-8, replicates sit just above it until `max_rounds` and end MAX_ROUNDS; the summaries
    over the CONVERGED ones are then a biased selection.  A RuntimeWarning says so; 1e-6 (a thousandth of a standard error) is safe there.

    Refused: `dispersion` as a string (`vc_gene_dispersion` knows no weights), n_boot outside 1..65535, device outputs above 1 GiB,
    shapes that do not match -- all before any device work.  What the replicates mean, and what they do not: the module's docstring."""
    if isinstance(dispersion, str):
        raise ValueError(f"the bootstrap does not support dispersion={dispersion!r}: vc_gene_dispersion knows no weights; hand over the "
                         "estimated dispersions instead")
    basis, logm, nu, r, pr, _ = check_arguments(counts_U, directions, n_scounts, means, a, noisemodel, dispersion, prior, None, False,
                                                tol, max_iter)
    W64 = omega_design(directions, harmonics_w, condition_design)
    Nhw = 2 * int(harmonics_w) + 1
    NW, Nx = W64.shape[0], W64.shape[0] // Nhw
    pm, pp = _nuw_prior(nuw_prior, Nx, Nhw)
    if not (tol_outer >= 0):
        raise ValueError("tol_outer must be >= 0")
    if int(max_rounds) != max_rounds or max_rounds < 0:
        raise ValueError("max_rounds must be an integer >= 0")
    first = pm.copy() if nuw_start is None else np.asarray(nuw_start, dtype=np.float64).reshape(-1).copy()
    if first.shape != (NW,) or not np.isfinite(first).all():
        raise ValueError(f"nuw_start must be {NW} finite coefficients (condition-major)")
    _check_run_options(storage, chunk_genes)
    Nc, Ng, K = int(counts_U.shape[0]), int(counts_U.shape[1]), int(basis.shape[0])
    w_host, R, nu_rep = check_bootstrap_arguments(Nc, Ng, K, NW, Nhw, n_boot, weights, means_replicates, fit)
    run_kw = dict(a=a, noisemodel=noisemodel, dispersion=dispersion, prior=prior, nuw_prior=nuw_prior, nuw_start=nuw_start, tol=tol,
                  max_iter=max_iter, tol_outer=tol_outer, max_rounds=max_rounds, device=device, chunk_genes=chunk_genes, storage=storage)
    if fit is None:
        fit = velocity_map(counts_U, directions, n_scounts, means, harmonics_w, condition_design, **run_kw)
    if w_host is None:
        from .gene_bootstrap import draw_weights
        from .gene_harmonics import _open_device
        w_table = draw_weights(R, Nc, seed, _open_device(device)[1])
    else:
        w_table = w_host
    prob = _Problem(counts_U, basis, logm, nu, r, pr, noisemodel, device, chunk_genes, storage, weights=w_table)
    dev = prob.dev
    ok_codes = (_lib.VC_KIN_CONVERGED, _lib.VC_KIN_ROUNDING)
    M = 2 + NW + NW * (NW + 1) // 2
    with torch.cuda.device(dev):
        W = torch.as_tensor(W64).to(torch.float32).to(dev).contiguous()
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        nu_rows = torch.as_tensor(nu_rep).to(dev) if nu_rep is not None else None
        base = torch.as_tensor(np.asarray(fit.included, dtype=bool)).to(dev)[None, :].expand(R, Ng)
        if nu_rows is not None:
            base = base & torch.isfinite(nu_rows).all(2)

        def evaluate(idx, V, start, inc):
            """The rows idx (ascending) at their coefficients V [A, NW]: per row what `velocity_map`'s evaluate returns."""
            rows = None if len(idx) == R else torch.as_tensor(idx, device=dev)
            take = (lambda t: t) if rows is None else (lambda t: t[rows])
            o = prob.run_rows(W, V, start, tol, max_iter, rows=rows, nu_rows=take(nu_rows) if nu_rows is not None else None, want_cov=False)
            good = (o["st"] == ok_codes[0]) | (o["st"] == ok_codes[1])
            inc = (good & take(base)) if inc is None else inc
            f = torch.where(inc, o["ll"] + take(prob.const) - prob.penalty(o["xy"]), zero)
            mag = torch.where(inc, o["ll"].abs(), zero)
            parts = torch.cat([f[:, None, :], mag[:, None, :], torch.where(inc[:, :, None], o["score"], zero).transpose(1, 2),
                               torch.where(inc[:, :, None], o["info"], zero).transpose(1, 2)], 1)
            sums = _row_sums(parts.reshape(-1, Ng).contiguous()).reshape(len(idx), M).cpu().numpy()
            failed = (inc & ~good).any(1).cpu().numpy()
            res = []
            for j in range(len(idx)):
                J = np.zeros((NW, NW))
                J[np.tril_indices(NW)] = sums[j, 2 + NW:]
                J = J + np.tril(J, -1).T + np.diag(pp)
                d = V[j] - pm
                res.append(dict(failed=bool(failed[j]), F=float(sums[j, 0] - 0.5 * (pp * d * d).sum()), allow=8.0 * EPS32 * float(sums[j, 1]),
                                G=sums[j, 2:2 + NW] - pp * d, J=J))
            return o, inc, res

        every = np.arange(R)
        if warm_start:
            nuw = np.tile(np.ascontiguousarray(np.asarray(fit.nu_omega, dtype=np.float64).T).reshape(-1), (R, 1))
            start = torch.as_tensor(np.ascontiguousarray(np.stack([fit.kinetics.log_gamma, fit.kinetics.log_beta], 1), dtype=np.float64)).to(dev)
        else:
            nuw, start = np.tile(first, (R, 1)), None
        o, inc, cur = evaluate(every, nuw, start, None)
        xy, st = o["xy"].clone(), o["st"].clone()
        n_excluded = (~inc).sum(1).cpu().numpy()
        status = np.array(["MAX_ROUNDS"] * R, dtype=object)
        rounds, dec = np.zeros(R, dtype=np.int64), np.full(R, np.nan)
        step, t, halved = np.zeros((R, NW)), np.ones(R), np.zeros(R, dtype=np.int64)
        active = np.ones(R, dtype=bool)

        def finish(b, word):
            status[b], active[b] = word, False

        def next_trial(b):
            """`velocity_map`'s head of a round for row b: the step and its decrement, or the end of the row."""
            try:
                step[b] = _solve_spd(cur[b]["J"], cur[b]["G"])
            except np.linalg.LinAlgError:
                return finish(b, "STALLED")
            dec[b] = float(cur[b]["G"] @ step[b])
            if dec[b] <= tol_outer:
                return finish(b, "CONVERGED")
            if rounds[b] >= max_rounds:
                return finish(b, "MAX_ROUNDS")
            t[b], halved[b] = 1.0, 0

        for b in every:
            if n_excluded[b] == Ng:
                finish(b, "GENE_FAILED")
            else:
                next_trial(b)
        while active.any():
            idx = np.flatnonzero(active)
            V = np.stack([nuw[b] + t[b] * step[b] for b in idx])
            rows = torch.as_tensor(idx, device=dev)
            o, _, trial = evaluate(idx, V, xy[rows], inc[rows])
            moved = []
            for j, b in enumerate(idx):
                if trial[j]["failed"]:
                    finish(b, "GENE_FAILED")
                elif trial[j]["F"] >= cur[b]["F"] - max(cur[b]["allow"], trial[j]["allow"]):
                    nuw[b], cur[b] = V[j], trial[j]
                    moved.append(j)
                    rounds[b] += 1
                    next_trial(b)
                else:
                    t[b] *= 0.5
                    halved[b] += 1
                    if halved[b] > MAX_OUTER_HALVINGS:
                        finish(b, "STALLED")
            if moved:
                src = torch.as_tensor(np.asarray(moved), device=dev)
                xy[rows[src]], st[rows[src]] = o["xy"][src], o["st"][src]
        assert set(status) <= set(MAP_STATUS)
        late = status == "MAX_ROUNDS"
        if max_rounds > 0 and late.any():                  # the summaries run over the CONVERGED rows: a selection, when the others only missed tol_outer
            warnings.warn(f"{int(late.sum())} of {R} replicates took max_rounds = {max_rounds} steps without reaching tol_outer = {tol_outer:g} "
                          f"(their last decrements: {np.nanmin(dec[late]):.3g} .. {np.nanmax(dec[late]):.3g}).  Where these are small the float32 "
                          "sums of this problem do not resolve tol_outer and the converged replicates are a biased selection: raise tol_outer "
                          "(1e-6 is a thousandth of a standard error)", RuntimeWarning, stacklevel=2)
        table = nuw.reshape(R, Nx, Nhw).transpose(0, 2, 1)
        kin = dict(log_gamma_replicates=xy[:, :, 0].cpu().numpy().copy(), log_beta_replicates=xy[:, :, 1].cpu().numpy().copy(),
                   kinetics_status=st.cpu().numpy()) if keep_kinetics else {}
        return VelocityMapBootstrap(nu_omega_replicates=np.ascontiguousarray(table), status=status.astype(str), rounds=rounds,
                                    n_excluded=n_excluded.astype(np.int64), F=np.array([c["F"] for c in cur]), dec=dec, fit=fit,
                                    weights=prob.Wt.cpu().numpy() if return_weights else None, **kin)
