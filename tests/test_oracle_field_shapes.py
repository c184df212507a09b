"""Pin the numpy oracle for the small grids of the fused field kernels (L * F < 32) against the reference's own outputs
(tests/golden/field_tiny.npz, field_neurad_tiny.npz, field_neurad_tiny_actors.npz; scripts/make_golden_field_shapes.py)."""
import numpy as np
import pytest

import neurad_oracle as O
from conftest import load_golden, rel_l2
from builders import actor_params, tagged_field_params

TOL = 1e-5  # the oracle restates the same fp32 ops

@pytest.mark.parametrize("tag", ["tiny", "neurad_tiny"])
def test_small_grid_field_matches_reference(tag):
    g = load_golden(f"field_{tag}")
    p = tagged_field_params(tag)
    assert p.geo_w[0].shape == g["geo_dw0"].shape  # geo layer 0 is [H, L*F]
    out = O.field_fwd(p, g["o"], g["d"], g["area"], g["starts"], g["ends"])
    assert rel_l2(out["feature"], g["feature"]) < TOL
    assert rel_l2(out["sdf"], g["sdf"]) < TOL
    assert rel_l2(out["alpha"], g["alpha"]) < TOL
    # ... and composited (what the fused render kernel is checked against)
    ref = O.render_rays(p, g["o"], g["d"], g["area"], g["starts"], g["ends"])
    w, _ = O.render_weight_from_alpha(g["alpha"])
    want = O.composite(w, g["feature"], g["starts"], g["ends"])
    for got, exp in zip((ref["features"], ref["depth"], ref["accumulation"]), want):
        assert rel_l2(got, exp) < TOL


def test_small_grid_field_with_actors_matches_reference():
    g = load_golden("field_neurad_tiny_actors")
    a = actor_params(g, 2, 2)
    mean, _ = O.fast_isotropic_gaussian(g["o"], g["d"], g["area"], g["starts"], g["ends"])
    b2w, valid = O.actor_boxes2world(a, g["times"])
    r, s, k = O.actor_hits(a, mean, b2w, valid, O.pose_inverse(b2w))
    np.testing.assert_array_equal(r, g["hit_ray"])
    np.testing.assert_array_equal(s, g["hit_sample"])
    np.testing.assert_array_equal(k, g["hit_actor"])
    assert len(r) > 0
    out = O.field_fwd_actors(tagged_field_params("neurad_tiny"), a, g["o"], g["d"], g["area"], g["starts"], g["ends"], g["times"])
    assert rel_l2(out["enc"], g["enc"]) < TOL
    # the actor rows are zero-padded past the actor grid's 2 levels (neurad_encoding.py:183)
    assert np.all(out["enc"].reshape(g["starts"].shape + (8,))[r, s, 4:] == 0)
    assert rel_l2(out["directions"], g["directions"]) < 1e-6
    assert rel_l2(out["feature"], g["feature"]) < TOL
    assert rel_l2(out["alpha"], g["alpha"]) < TOL
