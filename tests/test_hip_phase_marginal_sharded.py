"""GPU, two real processes: fit.phase_marginal() with the cells sharded over the ranks of a torch.distributed job -- the gathers of the
fit driver against predictive.merge_marginal_shards of the records the two ranks computed by themselves, and both against the record
of one engine that holds all cells: bit for bit.  On a 1-GPU box both ranks sit on cuda:0 and exchange through gloo
(VC_BENCH_ONE_DEVICE hook, as tests/test_hip_fit_sharded.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.phase_marginal_shard_worker import BINS, DRAWS
from tests.test_hip_fit_sharded import _free_port, _tb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("log_evidence", "posterior", "per_draw", "phis")


def _record(z):
    from velocycle_amd.predictive import PhaseMarginal
    return PhaseMarginal(n_draws=int(z["n_draws"]), **{f: torch.tensor(z[f]) for f in FIELDS})


def test_sharded_marginal_equals_the_merge_and_the_single_rank_record(tmp_path):
    from velocycle_amd.predictive import merge_marginal_shards
    prefix = str(tmp_path / "pm")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VC_BENCH_ONE_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), "tests/phase_marginal_shard_worker.py", prefix],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, _tb(r.stderr)
    parts = [_record(np.load(f"{prefix}.rank{k}.npz")) for k in range(2)]
    got, whole, want = _record(np.load(f"{prefix}.merged.npz")), _record(np.load(f"{prefix}.whole.npz")), merge_marginal_shards(parts)
    assert got.n_draws == DRAWS and got.posterior.shape == (602, BINS) and got.per_draw.shape == (DRAWS, 602) and got.log_evidence.shape == (602,)
    assert got.log_evidence.dtype == torch.float64 and got.posterior.dtype == torch.float32
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), f
        assert torch.equal(getattr(got, f), getattr(whole, f)), f                # two ranks merged == one rank, bit for bit
    assert torch.equal(got.posterior[:301], parts[0].posterior) and torch.equal(got.log_evidence[301:], parts[1].log_evidence)
    assert bool(torch.isfinite(got.log_evidence).all()) and float((got.posterior.double().sum(1) - 1).abs().max()) < 1e-5
