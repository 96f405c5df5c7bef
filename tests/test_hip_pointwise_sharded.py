"""GPU, two real processes: fit.predictive_density() with the cells sharded over the ranks of a torch.distributed job -- the gathers
of the fit driver (per-cell results, per-gene rows in rank order, the dense matrix) against predictive.merge_shards of the records
the two ranks computed by themselves.  On a 1-GPU box both ranks sit on cuda:0 and exchange through gloo (VC_BENCH_ONE_DEVICE hook,
as tests/test_hip_fit_sharded.py); the worker checks that every tensor handed to a collective is a device tensor, which is what an
RCCL-only group needs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.predictive_shard_worker import FIELDS
from tests.test_hip_fit_sharded import _free_port, _tb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(z):
    from velocycle_amd.predictive import PredictiveDensity
    kw = {f: {"S": torch.tensor(z[f + "_S"])} for f in FIELDS}
    return PredictiveDensity(n_draws=int(z["n_draws"]), pointwise={"S": torch.tensor(z["pointwise_S"])}, **kw)


def test_sharded_predictive_density_equals_the_merge_of_the_ranks_records(tmp_path):
    from velocycle_amd.predictive import merge_shards
    prefix = str(tmp_path / "pd")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VC_BENCH_ONE_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), "tests/predictive_shard_worker.py", prefix],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, _tb(r.stderr)
    parts = [_record(np.load(f"{prefix}.rank{k}.npz")) for k in range(2)]
    got, want = _record(np.load(f"{prefix}.merged.npz")), merge_shards(parts)
    assert got.n_draws == want.n_draws == 6 and got.lppd_cell["S"].shape == (602,) and got.pointwise["S"].shape == (70, 602)
    for f in FIELDS:
        assert torch.equal(getattr(got, f)["S"], getattr(want, f)["S"]), f          # the same float64 additions in the same order
    assert torch.equal(got.pointwise["S"], want.pointwise["S"])
    assert torch.equal(got.lppd_cell["S"][:301], parts[0].lppd_cell["S"]) and torch.equal(got.lppd_cell["S"][301:], parts[1].lppd_cell["S"])
    assert bool(torch.isfinite(got.lppd_gene["S"]).all()) and bool((got.p_waic_cell["S"] > 0).all())
