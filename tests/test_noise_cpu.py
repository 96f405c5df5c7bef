"""The float64 restatement of the SVI noise stream (tests/noise_checker.py) held to what it claims to be, without a GPU: N(0, 1),
independent across steps, seeds, pair members and neighbours; every bit of the 64-bit seed and step matters; the two rounding
edges of the 24-bit uniform; bounded draws.  The GPU suite (tests/test_hip_noise.py) then holds the device to this restatement.

Bar 6.0 on every |z|.  Measured for the restatement: goodness of fit |z| <= 1.53 (chi-square -1.52 .. +0.80),
independence |z| <= 1.13, largest |draw| 5.16.
"""
import numpy as np
import pytest

from tests import noise_checker as NC

N = 1 << 20
STREAMS = [(20240917, 0), (20240917, 1), (1, 7), (0x0123456789ABCDEF, (1 << 33) + 5)]
EDGE_ONE, EDGE_SMALL = NC.EDGE_ONE, NC.EDGE_SMALL      # (seed, step) of the two rounding edges at index 0

_IDX = np.arange(N, dtype=np.uint64)


@pytest.fixture(scope="module")
def draws():
    """{(seed, step): 2^20 consecutive draws}, computed once, read-only."""
    keys = STREAMS + [(20240918, 0)]
    out = {k: NC.normals(k[0], k[1], _IDX) for k in keys}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("key", STREAMS, ids=lambda k: f"seed{k[0]:#x}-step{k[1]}")
def test_restatement_is_standard_normal(draws, key):
    z = NC.gof(draws[key])
    print(f"\n[noise restatement] seed {key[0]:#x} step {key[1]}: " + ", ".join(f"{k} {v:+.2f}" for k, v in z.items()))
    for k, v in z.items():
        assert abs(v) <= NC.BAR, (key, k, v)


def test_restatement_is_independent(draws):
    a = draws[(20240917, 0)]
    z = {"step 0 vs step 1": NC.cross(a, draws[(20240917, 1)]), "seed vs seed + 1": NC.cross(a, draws[(20240918, 0)])}
    z.update(NC.within(a))
    print("\n[noise restatement] independence: " + ", ".join(f"{k} {v:+.2f}" for k, v in z.items()))
    assert set(z) == {"step 0 vs step 1", "seed vs seed + 1", "pair", "lag1", "lag2", "pair_squares"}
    for k, v in z.items():
        assert abs(v) <= NC.BAR, (k, v)


def test_every_bit_of_seed_and_step_matters():
    idx = np.arange(64)
    base = NC.normals(5, 3, idx)
    assert np.array_equal(base, NC.normals(5, 3, idx))
    assert not np.array_equal(base, NC.normals(5, 3 + (1 << 32), idx))
    assert not np.array_equal(base, NC.normals(5 + (1 << 32), 3, idx))
    # none of the 64 draws survives either change (each draw is its own Philox block's)
    assert (base != NC.normals(5, 3 + (1 << 32), idx)).all() and (base != NC.normals(5 + (1 << 32), 3, idx)).all()
    # a negative step is its two's-complement uint64
    assert np.array_equal(NC.normals(5, -1, idx), NC.normals(5, (1 << 64) - 1, idx))
    assert np.array_equal(NC.normals(5, -(1 << 32), idx), NC.normals(5, (1 << 64) - (1 << 32), idx))
    assert not np.array_equal(NC.normals(5, -1, idx), NC.normals(5, 1, idx))
    # a pair is one block: indices 2k, 2k + 1 share the radius and are the cos / sin of one angle
    r = NC.radius(5, 3, idx)
    assert np.array_equal(r[0::2], r[1::2])
    assert np.allclose(base[0::2] ** 2 + base[1::2] ** 2, r[0::2] ** 2, rtol=1e-14, atol=0)
    # ... and no two pairs share a word
    w = NC.words(5, 3, idx[0::2])
    assert len(set(map(int, w[0]))) == 32 and len(set(map(int, w[1]))) == 32


def test_rounding_edges_of_the_24_bit_uniform():
    i01 = np.array([0, 1])
    w = NC.words(*EDGE_ONE, i01)
    assert int(w[0][0]) >> 8 == 0xFFFFFF
    assert NC.uniform24(w[0])[0] == np.float32(1.0)            # 16777215.5 is not a float32: the add rounds to even, 2^24
    e = NC.normals(*EDGE_ONE, i01)
    assert np.isfinite(e).all() and (e == 0.0).all(), e
    assert NC.radius(*EDGE_ONE, i01)[0] == 0.0
    assert np.isfinite(NC.normals32(*EDGE_ONE, i01)).all()

    w = NC.words(*EDGE_SMALL, i01)
    assert int(w[0][0]) >> 8 == 0
    assert NC.uniform24(w[0])[0] == np.float32(2.0 ** -25)
    rad = NC.radius(*EDGE_SMALL, i01)[0]
    assert abs(rad - NC.RAD_MAX) <= 1e-12 and abs(NC.RAD_MAX - 5.887) < 1e-3, rad
    e = NC.normals(*EDGE_SMALL, i01)
    assert np.isfinite(e).all() and abs(np.hypot(e[0], e[1]) - rad) <= 1e-12, e


def test_draws_are_finite_and_bounded(draws):
    worst = 0.0
    for key, x in draws.items():
        assert np.isfinite(x).all(), key
        worst = max(worst, float(np.abs(x).max()))
    for key in (EDGE_ONE, EDGE_SMALL):
        x = NC.normals(*key, np.arange(2))
        assert np.isfinite(x).all()
        worst = max(worst, float(np.abs(x).max()))
    print(f"\n[noise restatement] largest |draw| {worst:.3f} (bound sqrt(50 ln 2) = {NC.RAD_MAX:.3f})")
    assert worst <= NC.RAD_MAX < 5.9


def test_float32_formation_of_the_uniform_is_part_of_the_specification(draws):
    """The scale of float32 rounding (normals32) and what forming the uniforms in float64 instead would move."""
    seed, step = STREAMS[0]
    e32 = float(np.abs(NC.normals32(seed, step, _IDX) - draws[(seed, step)]).max())
    w = NC.words(seed, step, _IDX)
    u1 = ((w[0] >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    u2 = ((w[1] >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    rad = np.sqrt(-2.0 * np.log(u1))
    alt = rad * np.where((_IDX & np.uint64(1)).astype(bool), np.sin(2 * np.pi * u2), np.cos(2 * np.pi * u2))
    e64 = float(np.abs(alt - draws[(seed, step)]).max())
    print(f"\n[noise restatement] all-float32 evaluation: max |diff| {e32:.2e}; uniforms formed in float64 instead: {e64:.2e}")
    assert e32 <= NC.TOL / 10          # float32 rounding leaves an order of magnitude of the elementwise bar to the hardware functions
    assert e64 <= NC.TOL               # (and shows why the restatement forms them in float32: this is ten times the rounding scale)
