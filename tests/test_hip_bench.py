"""GPU: bench.py's plain run -- one timed region of exactly --steps steps, nothing measured besides it -- and --dump-outputs,
which writes what the timed path hands its caller after its last step; two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = ["--cells", "6000", "--genes", "300", "--steps", "12", "--warmup", "3"]


def _plain_run(outdir):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *SIZE, "--dump-outputs", str(outdir)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path):
    j = _plain_run(tmp_path / "a")
    assert j["steps"] == 12 and j["warmup"] == 3 and j["n_gpus"] == 1 and j["nonfinite_loss_steps"] == 0
    assert j["unit"] == "SVI steps/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["ms_per_step"] > 0 and abs(j["value"] * j["ms_per_step"] - 1e3) <= 1e-2 * 1e3
    for key in ("roofline", "modes", "cpu_baseline", "repeat_ms_per_step", "device_clock_mhz", "opt_in_loss_every_10",
                "with_loss_readback_each_step"):
        assert key not in j, key                        # --full only
    names = j["outputs"]["arrays"]
    assert sorted(f[:-4] for f in os.listdir(tmp_path / "a")) == sorted(names)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 2 ** 20
    assert got["param_phixy_locs"].shape == (6000, 2) and "param_nu_locs" in got
    assert got["loss"].shape == (1,) and got["loss"][0] == j["loss_first_last"][1]      # the loss of the last timed step
    # the same arguments: the same data, the same Philox draws, fixed-order reductions -- the same arrays, bit for bit
    j2 = _plain_run(tmp_path / "b")
    assert j2["outputs"]["arrays"] == names
    for n in names:
        assert np.array_equal(np.load(tmp_path / "b" / f"{n}.npy"), got[n]), n
