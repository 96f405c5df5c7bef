"""CPU: the boundary-count data of tests/helpers.py (boundary_spec) and the sensitivity of the bars that
tests/test_hip_count_extremes.py holds the kernels to.  In float64 on the host: for every boundary level L of every planted gene,
leaving that level's term out -- C_L log(r + L) of the loss, r C_L / (r + L) of the gene's shape_inv_locs gradient (the chain rule
of vc_si_grad: d/d log(shape_inv) = -r^2 si d/dr) -- moves the loss by more than 3 x its 1e-5 bar and the gradient by more than
3 x GENE_RTOL of the gene's sum of absolute terms: a missing or duplicated count level cannot pass the GPU bars."""
import numpy as np
import pytest
import torch

from oracle import velocycle_oracle as orc
from tests import helpers as H

LOSS_RTOL = 1e-5            # assert_step_matches_oracle's loss bar


def _expected_form_and_storage(spec):
    """The admission rules of the engine restated: dense tables need every non-zero count an integer < 2048 (vc_count_dense);
    uint16 storage every count an integer <= 65535 (the pack kernels' bad[2] flag)."""
    mats = [spec.S] + ([spec.U] if spec.kind == "velocity" else [])
    dense = all(bool(((M == 0) | ((M == M.floor()) & (M > 0) & (M < 2048))).all()) for M in mats)
    u16 = all(bool(((M == M.floor()) & (M <= 65535)).all()) for M in mats)
    return ("dense-capable" if dense else "lists"), ("u16" if u16 else "f32")


def test_boundary_data_has_the_planted_structure():
    spec = H.boundary_spec("vjoint")
    plan, zero = H.boundary_plan(spec.Ng)
    assert spec.Ng == 200 and spec.Ng % 64 != 0
    for name, M in (("S", spec.S), ("U", spec.U)):
        for g, K in plan[name].items():
            assert float(M[g].max()) == K and int((M[g] == K).sum()) >= 20, (name, g)
            h = spec.Nc // 2
            assert float(M[g, h:].max()) < 256 and float(M[g, :h].max()) == K      # the second shard stays below 256 levels
        for g in zero:
            assert float(M[g].abs().max()) == 0.0
        assert float(M[128:192].abs().max()) == 0.0                                 # an all-zero gene block
        assert float(M[64:80].abs().max()) == 0.0 and float(M[80:96].max()) > 640    # an empty quarter beside one past 640
        assert sorted(plan[name].values()) == sorted(H.BOUNDARY_LEVELS + (700,))
        for g, K in plan[name].items():                                              # each level the largest count of its quarter
            q = g // 16 * 16
            assert float(M[q:min(q + 16, spec.Ng)].max()) == K, (name, g)
    assert _expected_form_and_storage(spec) == ("dense-capable", "u16")


@pytest.mark.parametrize("overflow", [k for k in H.OVERFLOW_VARIANTS if k is not None])
def test_overflow_variants_state_their_form_and_storage(overflow):
    spec = H.boundary_spec("vjoint", overflow=overflow)
    assert _expected_form_and_storage(spec) == H.OVERFLOW_VARIANTS[overflow]
    assert float(spec.S[20, -1]) == overflow and float(spec.U[20, -1]) == overflow


@pytest.mark.parametrize("kind", ["phase", "vjoint", "vjoint_lrmn", "vcond"])
def test_one_count_level_moves_the_compared_quantities_past_their_bars(kind):
    from velocycle_amd.rng import draw_eps
    spec = H.boundary_spec(kind)
    p64 = H.problem_from_spec(spec)
    cov = None
    if spec.guide == "lrmn":
        g = torch.Generator().manual_seed(0)
        M = spec.Ng + spec.Nx * spec.Nhw
        cov = torch.normal(torch.zeros((M, spec.rho_rank)), torch.ones((M, spec.rho_rank)) * 0.02, generator=g)
    par = orc.init_params(p64, cov)
    eps = draw_eps(spec, torch.Generator().manual_seed(1))
    l64, _, _, _ = orc.loss_and_grads(p64, par, {k: v.double() for k, v in eps.items() if not k.startswith("_")})
    r, scale, tables = H.nb_shape_inv_terms(spec, par, eps)
    plan, _ = H.boundary_plan(spec.Ng)
    # the per-gene gradient bar is held where shape_inv is a free parameter and the unspliced mean follows the spliced one: under the
    # LRMN guide the drawn nu_omega puts cells on the relu kink of ElogU (mean 1e-5 x ...), whose (r + k) / (r + mu) terms swamp one
    # level of a 2047-count gene (1.2e-6 of its absolute terms); there the loss bar and the block bars stand alone
    grad_free = "shape_inv" not in spec.condition_on and spec.guide == "meanfield"
    n = 0
    for m, name in enumerate(["S", "U"][:len(tables)]):
        for g, K in plan[name].items():
            C = tables[m][g]
            assert len(C) == K and C[K - 1] >= 20
            for L in sorted({K - 1} | {x for x in (255, 256, 639, 640) if x < K}):
                dl = C[L] * np.log(r[g] + L)
                assert dl > 3 * LOSS_RTOL * abs(l64), (name, g, L, dl, l64)
                if grad_free:
                    dg = r[g] * C[L] / (r[g] + L)
                    assert dg > 3 * H.GENE_RTOL * scale[g], (name, g, L, dg / scale[g])
                n += 1
    assert n >= 20
