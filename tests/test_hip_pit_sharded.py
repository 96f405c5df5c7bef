"""GPU, two real processes: fit.predictive_pit() with the cells sharded over the ranks of a torch.distributed job -- the gathers of
the fit driver against predictive.merge_pit_shards of the records the two ranks computed by themselves.  On a 1-GPU box both ranks
sit on cuda:0 and exchange through gloo (VC_BENCH_ONE_DEVICE hook, as tests/test_hip_fit_sharded.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pit_checker as Q
from tests.pit_shard_worker import FIELDS
from tests.test_hip_fit_sharded import _free_port, _tb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(z):
    from velocycle_amd.predictive import PredictivePIT
    kw = {f: {"S": torch.tensor(z[f + "_S"])} for f in FIELDS}
    return PredictivePIT(n_draws=int(z["n_draws"]), bins=int(z["bins"]), seed=int(z["seed"]), **kw)


def test_sharded_pit_equals_the_merge_of_the_ranks_records(tmp_path):
    from velocycle_amd.predictive import merge_pit_shards
    prefix = str(tmp_path / "pit")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VC_BENCH_ONE_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), "tests/pit_shard_worker.py", prefix],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, _tb(r.stderr)
    parts = [_record(np.load(f"{prefix}.rank{k}.npz")) for k in range(2)]
    got, want = _record(np.load(f"{prefix}.merged.npz")), merge_pit_shards(parts)
    assert (got.n_draws, got.bins, got.seed) == (6, 16, 77) and got.cell_hist["S"].shape == (602, 16) and got.pointwise["S"].shape == (3, 70, 602)
    for f in FIELDS:
        assert torch.equal(getattr(got, f)["S"], getattr(want, f)["S"]), f
    assert torch.equal(got.cell_hist["S"][:301], parts[0].cell_hist["S"]) and torch.equal(got.cell_hist["S"][301:], parts[1].cell_hist["S"])
    # the merged tables follow from the merged u: the second rank randomized with ITS global cell indices
    gene, cell = Q.histograms(got.pointwise["S"][2].numpy(), 16, np.float32)
    assert np.array_equal(got.gene_hist["S"].numpy(), gene) and np.array_equal(got.cell_hist["S"].numpy(), cell)
    lo, hi, u = (got.pointwise["S"][j].numpy() for j in range(3))
    v = Q.uniforms(70, 602, 77, 0, dt=np.float32)
    want_u = np.clip((v.astype(np.float64) * (hi - lo).astype(np.float64) + lo.astype(np.float64)).astype(np.float32), 0, np.float32(0.99999994))
    assert (np.abs(u - want_u) <= np.spacing(want_u)).all()
