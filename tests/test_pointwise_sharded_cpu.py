"""CPU, two processes over gloo: the multi-rank branch of fit.predictive_density() -- the gathers of the per-cell results, of the
per-gene rows and of the dense matrix, and their merge -- with the device evaluation replaced by a planted record per rank.  What
the branch returns must be predictive.merge_shards of the planted records, on every rank.  (The evaluation itself, and the same
branch on real engines, are tests/test_hip_pointwise.py and tests/test_hip_pointwise_sharded.py.)"""
import multiprocessing as mp
import os
import types

import torch
import torch.distributed as dist

FIELDS = ("lppd_gene", "lppd_cell", "mean_gene", "mean_cell", "p_waic_gene", "p_waic_cell")
NG, NC, WORLD = 5, 11, 2


def planted(rank, n_cells):
    from velocycle_amd.predictive import PredictiveDensity
    g = torch.Generator().manual_seed(40 + rank)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 1e3          # (sums of unequal size: the order of additions shows)
    kw = {f: {m: rnd(NG if f.endswith("_gene") else n_cells) for m in ("S", "U")} for f in FIELDS}
    return PredictiveDensity(n_draws=4, pointwise={m: rnd(NG, n_cells).float() for m in ("S", "U")}, **kw)


def _worker(rank, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from velocycle_amd import predictive
    from velocycle_amd.distributed import dist_context
    from velocycle_amd.engine import shard_bounds
    from velocycle_amd.fit_models import VelocityFitModel
    sizes = [b - a for a, b in (shard_bounds(NC, r, WORLD) for r in range(WORLD))]
    f = VelocityFitModel(types.SimpleNamespace(model_fn=None, guide_fn=None, Ng=NG, Nc=NC))
    f.spec = types.SimpleNamespace(kind="velocity", noisemodel="NegativeBinomial", Ng=NG, Nc=NC)
    f.engine = types.SimpleNamespace(spec=f.spec, Nc_local=sizes[rank], device=torch.device("cpu"))
    f.losses = [1.0]
    f._rank, f._world, f._pg = dist_context(None)
    f._shard_sizes = sizes
    predictive.pointwise_density = lambda eng, draws, return_pointwise=False: planted(rank, sizes[rank])
    got = f.predictive_density(draws={"ν": torch.zeros(4, NG, 3), "ϕxy": torch.zeros(4, sizes[rank], 2)}, return_pointwise=True)
    want = predictive.merge_shards([planted(r, sizes[r]) for r in range(WORLD)])
    same = all(torch.equal(getattr(got, fl)[m], getattr(want, fl)[m]) for fl in FIELDS for m in ("S", "U"))
    same = same and all(torch.equal(got.pointwise[m], want.pointwise[m]) for m in ("S", "U"))
    q.put((rank, same, tuple(got.lppd_cell["U"].shape), tuple(got.pointwise["S"].shape), got.n_draws, sizes))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_predictive_density_is_the_merge_of_the_ranks_records():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(WORLD)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r, (rank, same, cshape, pshape, nd, sizes) in enumerate(res):
        assert rank == r and same and cshape == (NC,) and pshape == (NG, NC) and nd == 4 and sizes == [6, 5]
