"""GPU, two real processes: fit.posterior_predictive_check() with the cells sharded over the ranks of a torch.distributed job -- the
gathers of the fit driver against predictive.merge_check_shards of the records the two ranks computed by themselves.  On a 1-GPU box
both ranks sit on cuda:0 and exchange through gloo (VC_BENCH_ONE_DEVICE hook, as tests/test_hip_fit_sharded.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ppc_checker as K
from tests.ppc_shard_worker import FIELDS
from tests.test_hip_fit_sharded import _free_port, _tb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(z):
    from velocycle_amd.predictive import PredictiveCheck
    kw = {f: {"S": torch.tensor(z[f + "_S"])} for f in FIELDS}
    return PredictiveCheck(n_draws=int(z["n_draws"]), n_cells=int(z["n_cells"]), seed=int(z["seed"]), **kw)


def test_sharded_check_equals_the_merge_of_the_ranks_records(tmp_path):
    from velocycle_amd.predictive import merge_check_shards
    prefix = str(tmp_path / "ppc")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VC_BENCH_ONE_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), "tests/ppc_shard_worker.py", prefix],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, _tb(r.stderr)
    parts = [_record(np.load(f"{prefix}.rank{k}.npz")) for k in range(2)]
    got, want = _record(np.load(f"{prefix}.merged.npz")), merge_check_shards(parts)
    assert got.n_draws == want.n_draws == 6 and got.n_cells == 602 and got.cell_rep["S"].shape == (6, 602)
    assert got.replicates["S"].shape == (2, 70, 602)
    for f in FIELDS:
        assert torch.equal(getattr(got, f)["S"], getattr(want, f)["S"]), f
    assert torch.equal(got.cell_rep["S"][:, :301], parts[0].cell_rep["S"]) and torch.equal(got.cell_rep["S"][:, 301:], parts[1].cell_rep["S"])
    # the merged tables follow from the merged replicates of the kept draws: the second rank drew with ITS global cell indices
    gene, cell = K.rep_stats(got.replicates["S"].numpy())
    assert np.array_equal(got.gene_rep["S"][:2].numpy(), gene) and np.array_equal(got.cell_rep["S"][:2].numpy(), cell)
    assert not torch.equal(parts[0].replicates["S"], parts[1].replicates["S"])
