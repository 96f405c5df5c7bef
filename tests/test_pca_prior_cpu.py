"""CPU: the PCA phase prior's device path with device="cpu" (the loop of velocycle_amd/phase_prior.py on torch matmuls: everything
but the two kernels) against the float64 checker of tests/pca_checker.py; the refusals; the code object of csrc/vc_pca.hip."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pca_checker as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = range(len(PC.FIXTURES))


def test_fixtures_are_hard_and_the_bars_come_from_the_host_path():
    for i in FIX:
        o = PC.oracle(i)
        ratio = o["s"][2] / o["s"][1]
        print(PC.FIXTURES[i], "s3/s2", round(float(ratio), 3), "host 'full' error", PC.bar(i) / PC.SAFETY)
        assert 0.85 <= ratio <= 0.99
        assert 1e-7 < PC.bar(i) / PC.SAFETY < 1e-4
    assert min(ng for _, ng, _ in PC.FIXTURES) < 64


@pytest.mark.parametrize("i", FIX)
def test_scores_against_the_oracle(i):
    PC.check_scores(i, "cpu")


@pytest.mark.parametrize("i", FIX)
def test_angles_against_the_oracle(i):
    PC.check_angles(i, "cpu")


@pytest.mark.parametrize("i", FIX)
def test_signs_are_sklearns(i):
    PC.check_signs(i, "cpu")


def test_zero_at_min_density_picks_the_oracles_cell():
    PC.check_min_density("cpu")


def test_variants_give_the_same_bits():
    PC.check_variants("cpu")


def test_refusals(monkeypatch):
    PC.check_refusals("cpu", monkeypatch)


def test_host_path_is_unchanged():
    from sklearn.decomposition import PCA
    from velocycle_amd.containers import Phases
    v = PC.layer(3)
    p = Phases.from_pca_heuristic(PC.adata(v), layer="S_sz", small_count=PC.SMALL)
    assert isinstance(p.pca, PCA) and isinstance(p.pcs, np.ndarray)
    q = Phases.from_pca_heuristic(PC.adata(v), layer="S_sz", small_count=PC.SMALL, device=None)
    assert isinstance(q.pca, PCA) and np.array_equal(p.phi_xy.values, q.phi_xy.values)


def test_header_declares_and_lib_binds_the_entry_points():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    for name, arity in (("vc_pca_stage", 11), ("vc_pca_apply", 12), ("vc_pca_apply_workspace", 3)):
        m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", hdr)
        assert m and m.group(1).count(",") + 1 == arity == len(_lib.EXPORTS[name][1]), name


def test_every_kernel_is_free_of_scratch(tmp_path):
    """.private_segment_fixed_size 0 for every kernel of vc_pca.hip, read from the metadata of a cross-compile for gfx950."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_pca.hip")
    out = str(tmp_path / "pca.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    found = re.findall(r"\.name:\s+(\S*vc_pca_\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read())
    assert sorted(re.search(r"vc_pca_[a-z]+_kernel", n).group(0) for n, _ in found) == \
        ["vc_pca_apply_kernel", "vc_pca_colsum_kernel", "vc_pca_fold_kernel", "vc_pca_stage_kernel"], found
    assert all(int(n) == 0 for _, n in found), found
