"""Worker of tests/test_hip_phase_marginal_sharded.py: a short phase fit with the cells sharded over the ranks of a torch.distributed
job, then fit.phase_marginal() on explicit draws through the multi-rank branch of the fit driver.

  python -m torch.distributed.run --nproc-per-node 2 ... tests/phase_marginal_shard_worker.py OUT_PREFIX

Every rank writes its OWN record (predictive.phase_marginal on its engine, nothing gathered) to OUT_PREFIX.rank<r>.npz; rank 0 also
writes what fit.phase_marginal returned to OUT_PREFIX.merged.npz and the record of ONE engine that holds all cells of the same
problem, scored with the same draws, to OUT_PREFIX.whole.npz.

Test hook VC_BENCH_ONE_DEVICE=1: every rank on cuda:0 and gloo instead of RCCL (a 1-GPU box cannot host two RCCL ranks)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

BINS, DRAWS = 24, 5


def flat(rec):
    return dict(log_evidence=rec.log_evidence.numpy(), posterior=rec.posterior.numpy(), per_draw=rec.per_draw.numpy(), phis=rec.phis.numpy(),
                n_draws=np.array(rec.n_draws))


def main():
    prefix = sys.argv[1]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    one_device = os.environ.get("VC_BENCH_ONE_DEVICE", "0") == "1"
    device = torch.device("cuda:0" if one_device else f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
    torch.cuda.set_device(device)
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo") if one_device else dist.init_process_group(backend="nccl", device_id=device)

    from velocycle_amd import containers as C, fit_models, predictive, preprocessing as P
    from velocycle_amd import pyro_compat as pyro
    from velocycle_amd.anndata_lite import AnnDataLite
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.optim import ClippedAdam
    from velocycle_amd.workloads import make_velocity_spec

    sp = make_velocity_spec(301, 70, "vjoint", n_conditions=2, Hw=0, seed=12)      # 602 cells: shards of 301, not multiples of 64
    ad = AnnDataLite(sp.S.t().numpy().copy(), sp.U.t().numpy().copy())
    ad.obs["batch"] = [f"d{int(b)}" for b in sp.truth["batch"]]
    cyc = C.Cycle.from_array(sp.mu_nu.T.numpy(), sp.sd_nu.T.numpy(), list(ad.var.index))
    ph = C.Phases.from_array(sp.phixy_prior.T.numpy(), cell_names=list(ad.obs.index))
    Db = P.make_design_matrix(ad, ids="batch")
    torch.manual_seed(100)
    pyro.clear_param_store()
    mp = P.preprocess_for_phase_estimation(ad, cyc, ph, Db, n_harmonics=1)
    pf = fit_models.PhaseFitModel(mp, num_samples=4, n_per_bin=2)
    pf.fit(ClippedAdam({"lr": 0.03, "lrd": 0.99, "betas": (0.80, 0.99)}), num_steps=10, verbose=False, seed=21)
    eng = pf.engine
    assert eng.world_size == world == 2 and eng.Nc_local == 301
    names = [k for k in ("ν", "Δν", "shape_inv") if pf._site_exists(k)]
    draws = {k: v.cpu() for k, v in eng.sample_posterior(names, DRAWS, seed=5).items()}      # gene-level sites: the same on every rank
    own = predictive.phase_marginal(eng, draws, bins=BINS, return_per_draw=True)             # the model's prior, this rank's rows
    np.savez(f"{prefix}.rank{rank}.npz", **flat(own))
    merged = pf.phase_marginal(draws=draws, bins=BINS, return_per_draw=True)
    drawn = pf.phase_marginal(num_samples=3, seed=9, bins=16, phase_prior="flat")            # the driver's own draws: the same key on every rank
    assert drawn.n_draws == 3 and drawn.posterior.shape == (602, 16) and drawn.log_evidence.shape == (602,) and drawn.per_draw is None
    assert bool(torch.isfinite(drawn.log_evidence).all())
    if rank == 0:
        one = HipEngine(eng.spec, device=device)                                             # all 602 cells on one engine
        np.savez(f"{prefix}.whole.npz", **flat(predictive.phase_marginal(one, draws, bins=BINS, return_per_draw=True)))
        one.close()
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        np.savez(f"{prefix}.merged.npz", **flat(merged))


if __name__ == "__main__":
    main()
