"""Pin the numpy oracle for the small grids of the fused field kernels (L * F < 32) against the reference's own outputs
(tests/golden/field_tiny.npz, field_neurad_tiny.npz, field_neurad_tiny_actors.npz; scripts/make_golden_field_shapes.py)."""
import numpy as np
import pytest

import neurad_oracle as O
import synth
from conftest import load_golden, rel_l2

TOL = 1e-5  # the oracle restates the same fp32 ops

# fixture tag -> (L, F, min_res, max_res, log2_hashmap_size, table seed); the generator's SHAPES
SHAPES = {"tiny": (1, 4, 32, 32, 10, 53), "neurad_tiny": (4, 2, 32, 8192, 11, 57)}


def grid_params(tag):
    L, F, mn, mx, lg, seed = SHAPES[tag]
    return O.GridParams(synth.hash_table(L * 2**lg, F, seed=seed, scale=0.5), L, mn, mx, lg)


def field_params(tag, use_sdf=True, H=32):
    """the fixture's field (32-wide MLPs, the seeds of oracle/make_golden.py's golden_field); H = 64: the same grid with
    64-wide MLPs (oracle-only shapes)"""
    grid = grid_params(tag)
    LF = grid.num_levels * grid.n_feat
    gw, gb, fw, fb = [], [], [], []
    for k, (o, i) in enumerate([(H, LF), (33, H)]):
        w, b = synth.linear(o, i, 200 + 10 * k)
        gw.append(w), gb.append(b)
    for k, (o, i) in enumerate([(H, 48), (H, H), (32, H)]):
        w, b = synth.linear(o, i, 300 + 10 * k)
        fw.append(w), fb.append(b)
    return O.FieldParams(grid, 100.0, gw, gb, fw, fb, use_sdf=use_sdf)


def actor_params(g):
    """NeuRAD tiny's actor grids: 2 levels x 2 features (the generator's ActorSettings)"""
    grids = [O.GridParams(synth.hash_table(2 * 2**9, 2, seed=400 + i, scale=0.7), 2, 64, 1024, 9) for i in range(3)]
    return O.ActorParams(g["timestamps"], g["positions"], g["rotations_6d"], g["present"], g["sizes"], g["padding"],
                         grids, actor_scale=10.0)


@pytest.mark.parametrize("tag", ["tiny", "neurad_tiny"])
def test_small_grid_field_matches_reference(tag):
    g = load_golden(f"field_{tag}")
    p = field_params(tag)
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
    a = actor_params(g)
    mean, _ = O.fast_isotropic_gaussian(g["o"], g["d"], g["area"], g["starts"], g["ends"])
    b2w, valid = O.actor_boxes2world(a, g["times"])
    r, s, k = O.actor_hits(a, mean, b2w, valid, O.pose_inverse(b2w))
    np.testing.assert_array_equal(r, g["hit_ray"])
    np.testing.assert_array_equal(s, g["hit_sample"])
    np.testing.assert_array_equal(k, g["hit_actor"])
    assert len(r) > 0
    out = O.field_fwd_actors(field_params("neurad_tiny"), a, g["o"], g["d"], g["area"], g["starts"], g["ends"], g["times"])
    assert rel_l2(out["enc"], g["enc"]) < TOL
    # the actor rows are zero-padded past the actor grid's 2 levels (neurad_encoding.py:183)
    assert np.all(out["enc"].reshape(g["starts"].shape + (8,))[r, s, 4:] == 0)
    assert rel_l2(out["directions"], g["directions"]) < 1e-6
    assert rel_l2(out["feature"], g["feature"]) < TOL
    assert rel_l2(out["alpha"], g["alpha"]) < TOL
