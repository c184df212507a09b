"""tests/raygen_refs.py, the numpy float32 restatement of the perspective and lidar ray kernels, pinned to the reference's own
outputs (tests/golden/raygen.npz, made on the CPU by oracle/make_golden_raygen.py).  No GPU: this is what entitles
tests/test_gpu_raygen_exact.py to ask the kernels for the restatement's bits.

The fixture's camera pixel area is the one quantity the restatement does not reproduce on every ray: it equals it on 507 of
512 rays and is at most 2 ulp off on the other five, which come from the order torch's sum takes over a 3-element inner
dimension.  Hence its bound here: at most 2 ulp everywhere, bit-equal on at least 98 % of rays."""
import numpy as np
import pytest
import torch

import raygen_refs as rr
from conftest import load_golden

LIDAR_NAMES = {"directions_norm": "distance"}  # the fixture's name of the lidar's norm


@pytest.fixture(scope="module")
def g():
    return load_golden("raygen")


def unequal_rays(ours, theirs):
    """rays on which any element differs in a bit"""
    return int((~rr.same_bits(ours, theirs.reshape(ours.shape))).any(-1).sum())


@pytest.mark.parametrize("tag", list(rr.FIXTURE_CAMERA_MODES))
def test_camera_restatement_gives_the_bits_of_the_reference(g, tag):
    got = rr.fixture_camera(g, tag)
    for q in ("origins", "times", "directions", "directions_norm"):
        assert unequal_rays(got[q], g[f"cam_{tag}_{q}"]) == 0, q
    u = rr.ulps(got["pixel_area"], g[f"cam_{tag}_pixel_area"].reshape(-1, 1))
    print(f"cam_{tag} pixel_area: {int((u == 0).sum())}/{u.size} rays bit-equal, max {int(u.max())} ulp")
    assert u.max() <= 2 and (u == 0).mean() >= 0.98


@pytest.mark.parametrize("ego", [True, False])
def test_lidar_restatement_gives_the_bits_of_the_reference(g, ego):
    tag = "ego" if ego else "noego"
    got = rr.fixture_lidar(g, ego)
    for q in rr.QUANTITIES:
        assert unequal_rays(got[q], g[f"lid_{tag}_{LIDAR_NAMES.get(q, q)}"]) == 0, q
    np.testing.assert_array_equal(got["did_return"].astype(bool), g[f"lid_{tag}_did_return"].reshape(-1, 1))
    assert 0 < got["did_return"].sum() < got["did_return"].size


def test_the_fixture_tells_the_two_roundings_of_the_norm_apart(g):
    """negative control: the separately rounded norm, which the kernels had, does not reproduce the fixture"""
    for tag in rr.FIXTURE_CAMERA_MODES:
        old = rr.fixture_camera(g, tag, fused=False)
        counts = {q: unequal_rays(old[q], g[f"cam_{tag}_{q}"]) for q in rr.QUANTITIES}
        worst = int(rr.ulps(old["pixel_area"], g[f"cam_{tag}_pixel_area"].reshape(-1, 1)).max())
        print(f"cam_{tag}, separately rounded norm: rays unequal {counts}, pixel area up to {worst} ulp")
        assert counts["directions"] >= 20 and counts["directions_norm"] >= 20, (tag, counts)
        assert counts["origins"] == counts["times"] == 0  # the norm is all that changed
    for ego, tag in ((True, "ego"), (False, "noego")):
        old = rr.fixture_lidar(g, ego, fused=False)
        counts = {q: unequal_rays(old[q], g[f"lid_{tag}_{LIDAR_NAMES.get(q, q)}"]) for q in rr.QUANTITIES}
        print(f"lid_{tag}, separately rounded norm: rays unequal {counts}")
        assert counts["directions"] >= 40 and counts["directions_norm"] >= 40, (tag, counts)
        assert counts["origins"] == counts["times"] == counts["pixel_area"] == 0


def torch_norm(v):
    """camera_utils.normalize_with_norm's denominator, on the CPU"""
    t = torch.from_numpy(np.ascontiguousarray(v))
    return torch.maximum(torch.linalg.vector_norm(t, dim=-1, keepdim=True), torch.tensor(float(rr.EPS))).numpy()


def synthetic_vectors():
    """name -> [N,3]: every vector that a synthetic case of the exact tests normalises.  The cases are built row by row from
    hashed indices, so the 1000-ray case holds every smaller one; a camera's vectors do not depend on the shutter mode."""
    tab, idx, coords = rr.camera_case(1000)
    out = {"camera": rr.camera_rays(tab, idx, coords, 1)["vectors"].reshape(-1, 3)}
    for point_dim in (3, 4, 5, 6):
        for ego in (True, False):
            for drop in ((), ("velocities",)):
                tab, idx, pts = rr.lidar_case(1000, point_dim)
                out[f"lidar, point_dim {point_dim}, ego {ego}, without {drop}"] = rr.lidar_rays(
                    rr.without(tab, *drop), idx, pts, ego)["vectors"].reshape(-1, 3)
    return out


def test_norm_helper_is_torchs_clamped_vector_norm():
    seen_eps = seen_nan = differs = 0
    for name, v in synthetic_vectors().items():
        want = torch_norm(v)[:, 0]
        got = rr.clamped_norm(v[:, 0], v[:, 1], v[:, 2])
        assert rr.same_bits(got, want).all(), name
        seen_eps += int((want == rr.EPS).sum())
        seen_nan += int(np.isnan(want).sum())
        differs += int((~rr.same_bits(rr.clamped_norm(v[:, 0], v[:, 1], v[:, 2], fused=False), want)).sum())
    # the cases hold what they are meant to: zero vectors, NaN vectors, and vectors on which the two roundings differ
    assert seen_eps > 0 and seen_nan > 0 and differs > 100, (seen_eps, seen_nan, differs)
    zero_and_nan = np.array([[0.0, 0.0, 0.0], [1.0, np.nan, 2.0]], rr.F)
    got = rr.clamped_norm(*zero_and_nan.T)
    assert got[0] == rr.EPS and np.isnan(got[1]) and rr.same_bits(got, torch_norm(zero_and_nan)[:, 0]).all()


def test_one_rounding_differs_from_two():
    """round_f32 and fma against cases worked by hand: a tie that float64 would break the wrong way, subnormals, overflow"""
    from fractions import Fraction as Q

    one, ulp = Q(1), Q(1, 2 ** 23)
    assert rr.round_f32(one + ulp / 2) == rr.F(1.0)  # tie: to even
    assert rr.round_f32(one + ulp / 2 + Q(1, 2 ** 80)) == np.nextafter(rr.F(1), rr.F(2))  # float64 loses the 2**-80: a tie
    assert rr.round_f32(one + 3 * ulp / 2) == rr.F(1.0) + rr.F(2.0 ** -22)
    # subnormals: 0.5 and 1.5 units of 2**-149 are ties (to 0 and to 2 units), 0.75 and 1.25 units are not
    assert rr.round_f32(Q(1, 2 ** 150)) == 0 and rr.round_f32(Q(3, 2 ** 150)) == rr.F(2.0 ** -148)
    assert rr.round_f32(Q(3, 2 ** 151)) == rr.F(2.0 ** -149) and rr.round_f32(-Q(5, 2 ** 151)) == -rr.F(2.0 ** -149)
    assert np.isinf(rr.round_f32(Q(2) ** 128 - Q(2) ** 103)) and rr.round_f32(Q(2) ** 128 - Q(2) ** 103 - 1) == np.finfo(rr.F).max
    # a = 1 + 2**-12: a*a = 1 + 2**-11 + 2**-24, a tie at float32 that the addend 2**-60 lifts
    a = rr.F(1 + 2.0 ** -12)
    assert rr.fma(a, a, rr.F(2.0 ** -60))[()] == rr.F(1 + 2.0 ** -11 + 2.0 ** -23)
    assert rr.F(np.float64(a) * np.float64(a) + np.float64(2.0 ** -60)) == rr.F(1 + 2.0 ** -11)  # two roundings: wrong
    assert np.isnan(rr.fma(rr.F(np.nan), a, a)) and np.isinf(rr.fma(rr.F(np.inf), a, a))
    assert rr.ulps(np.array([1.0, -0.0, -1.0], rr.F), np.array([np.nextafter(rr.F(1), rr.F(2)), 0.0, 1.0], rr.F)).tolist() == \
        [1, 0, 2 * 0x3F800000]
