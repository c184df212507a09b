"""CPU checks of tests/march_exact_refs.py: the float64 reference equals both fp32 restatements of the march bit for bit on
every dyadic scene (the proof that the design is exact: if this fails the scene is wrong, not the kernel), and every
property of the scenes that tests/test_gpu_march_exact.py leans on holds, asserted from the reference alone."""
import numpy as np
import pytest

import march_exact_refs as MX
import occgrid_oracle as OO
import occgrid_update_restatement as UR

f32 = np.float32
CONFIGS = [(step, opt) for step in MX.STEPS for opt in (True, False)]
IDS = [f"step{step}-{'options' if opt else 'plain'}" for step, opt in CONFIGS]


# ---- the design is exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step,opt", CONFIGS, ids=IDS)
def test_reference_equals_the_single_grid_restatement_bit_for_bit(step, opt):
    rays = MX.dyadic_rays()
    t_min, t_max, t_rand = MX.ray_options(rays, opt)
    ref = MX.dyadic_reference(1, step, opt)
    for kind in ("random", "ones", "zeros"):
        b = MX.binaries_for(kind, 1)
        ri, ts, te = OO.occgrid_march(MX.level_boxes(1)[0], b[0], rays["o"], rays["d"], step, MX.NEAR, MX.FAR, t_min, t_max,
                                      0.0, t_rand)
        want = MX.expected(ref, b)
        np.testing.assert_array_equal(ri, want[0])
        np.testing.assert_array_equal(MX.bits(ts), MX.bits(want[1]))
        np.testing.assert_array_equal(MX.bits(te), MX.bits(want[2]))
    assert len(MX.expected(ref, MX.binaries_for("ones", 1))[0]) == len(ref["ray"]) > 500
    assert len(MX.expected(ref, MX.binaries_for("zeros", 1))[0]) == 0


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("step,opt", CONFIGS, ids=IDS)
def test_reference_equals_the_levels_restatement_bit_for_bit(step, opt, levels):
    """march_levels takes no t_rand: the near plane it would shift, max(near_plane, t_min) + t_rand * step, goes in as t_min
    (exact on the lattice and never below near_plane).  Keep flags are compared with no exclusion."""
    rays = MX.dyadic_rays()
    t_min, t_max, t_rand = MX.ray_options(rays, opt)
    if opt:
        t_min = (np.maximum(f32(MX.NEAR), t_min) + t_rand * f32(step)).astype(f32)
    b = MX.binaries_for("random", levels)
    m = UR.march_levels(MX.level_boxes(levels), b, rays["o"], rays["d"], step, MX.NEAR, MX.FAR, t_min, t_max)
    ref = MX.dyadic_reference(levels, step, opt)
    np.testing.assert_array_equal(m["ray"], ref["ray"])
    np.testing.assert_array_equal(MX.bits(m["t_start"]), MX.bits(ref["t_start"].astype(f32)))
    np.testing.assert_array_equal(MX.bits(m["t_end"]), MX.bits(ref["t_end"].astype(f32)))
    np.testing.assert_array_equal(m["keep"], MX.keep(ref, b))
    # the casts lose nothing: every t of the reference is an fp32 number
    assert np.all(ref["t_start"].astype(f32) == ref["t_start"]) and np.all(ref["t_end"].astype(f32) == ref["t_end"])


# ---- what the scenes cover -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step,opt", CONFIGS, ids=IDS)
def test_coverage_of_faces_chunks_and_empty_rays(step, opt):
    ref = MX.dyadic_reference(3, step, opt)
    kept = MX.keep(ref, MX.binaries_for("random", 3))
    n = MX.per_ray(ref)
    on_face = [(int(ref["on_box_face"][:, l].sum()), int((ref["on_box_face"][:, l] & kept).sum())) for l in range(3)]
    print(f"{len(ref['ray'])} candidates, {kept.sum()} kept; midpoint on a cell face: {ref['on_cell_face'].sum()}; on the box "
          f"face of level 0 / 1 / 2 (of which kept): {on_face}; levels: {np.bincount(ref['level'], minlength=3)}; rays with 0 / "
          f">= 65 / >= 129 candidates: {(n == 0).sum()} / {(n >= 65).sum()} / {(n >= 129).sum()}")
    assert ref["on_cell_face"].sum() >= 100
    for l in (0, 1):  # the inner boxes: the closed-box rule decides the level there; both outcomes occur
        total, k = on_face[l]
        assert total >= 10 and 0 < k < total, (l, total, k)
    assert on_face[2][0] >= 10  # hi_face and lo_face slide along the outermost box
    assert np.all(np.bincount(ref["level"], minlength=3) >= 100)
    assert (n == 0).sum() >= 5 and (n >= 65).sum() >= 2
    if step == 0.25:  # (at step 0.5 a ray has at most (far - near) / 0.5 = 127 candidates; the cap tests run at 0.25)
        assert (n >= 129).sum() >= 2
    # empty rays first, last and between non-empty ones; every prefix ends in a ragged workgroup of 4 rays
    assert n[0] == 0 and n[1] > 0 and n[2] == 0 and n[3] > 0 and n[4] > 0 and n[-1] == 0 and n[-2] > 0
    assert all(r % 4 for r in MX.RAY_COUNTS) and max(MX.RAY_COUNTS) == len(n) == MX.N_RAYS


@pytest.mark.parametrize("levels", [1, 3])
def test_designed_rays_have_the_counts_worked_out_by_hand(levels):
    rays = MX.dyadic_rays()
    for step, key in ((0.25, "n25"), (0.5, "n50")):
        ref = MX.dyadic_reference(levels, step, True)
        n = MX.per_ray(ref)
        for r, ray in enumerate(MX.DESIGNED_HEAD + [None] * (MX.N_RAYS - len(MX.DESIGNED_HEAD) - 1) + MX.DESIGNED_TAIL):
            if ray is not None:
                assert rays["names"][r] == ray["name"] and n[r] == ray[key], (ray["name"], step, n[r], ray[key])
    ref = MX.dyadic_reference(levels, 0.25, True)
    of = lambda name: ref["ray"] == rays["names"].index(name)  # noqa: E731
    last = lambda name: np.nonzero(of(name))[0][-1]  # noqa: E731
    x, y = ref["cell"] // 64, ref["cell"] // 8 % 8
    assert np.all(x[of("hi_face")] == 7) and np.all(ref["level"][of("hi_face")] == levels - 1)  # u == 1: clamped from 8
    assert np.all(y[of("lo_face")] == 0) and np.all(ref["on_box_face"][of("hi_face") | of("lo_face"), levels - 1])
    for name, t_far in (("cut_by_t_far", 5.125), ("inside_l0", 18.5), ("t_min_above_near", 8.0)):
        i, r = last(name), rays["names"].index(name)
        assert ref["t_end"][i] == ref["t_far"][r] == t_far and ref["t_end"][i] - ref["t_start"][i] < 0.25
    assert ref["t_far"][rays["names"].index("t_max_beyond_far")] == MX.FAR and ref["t_far"][rays["names"].index("long_222")] == 56.0
    assert ref["t_near"][rays["names"].index("t_min_below_near")] == MX.NEAR
    assert ref["t_near"][rays["names"].index("t_min_above_near")] == 3.125
    if levels == 3:
        inner = of("inner_hi_face")
        assert set(ref["level"][inner]) == {0, 1, 2} and np.all(x[inner & (ref["level"] == 0)] == 7)
        assert ref["level"][of("inside_l0")][0] == 0 and ref["level"][of("inside_l1")][0] == 1
        assert ref["level"][of("outside_all")][0] == 2


# ---- the scenes tell the rule from the rule with one line changed ----------------------------------------------------------
def test_caps_tell_a_per_candidate_cap_from_a_per_chunk_cap():
    """A march that looks at max_candidates once per 64 candidates emits up to 64 * ceil(cap / 64) per ray: on these rays that
    differs from the rule at every cap that is no multiple of 64, and at none that is."""
    ref = MX.dyadic_reference(3, 0.25, True)
    n = MX.per_ray(ref)
    for kind in ("ones", "random"):
        b = MX.binaries_for(kind, 3)
        for cap in MX.CAPS:
            want, broken = MX.expected(ref, b, cap), MX.expected(ref, b, cap, chunked=True)
            assert (len(want[0]) != len(broken[0])) == (cap % 64 != 0), (kind, cap)
            if kind == "ones":
                np.testing.assert_array_equal(np.diff(want[3]), np.minimum(n, cap))
    assert (n > 200).sum() >= 1  # every cap binds some ray


@pytest.mark.parametrize("broken", MX.MUTATIONS)
def test_scenes_tell_the_rule_from_a_broken_one(broken):
    """<= to < (and >= to >) in the level-box test, no clamp of the cell index, o > hi to o >= hi in the slab test: each
    changes what the march emits on the random binaries (no clamp: counting only reads that stay inside the array)."""
    ref, bad = MX.dyadic_reference(3, 0.25, True), MX.dyadic_reference(3, 0.25, True, broken)
    b = MX.binaries_for("random", 3)
    if broken == "open_hi_slab":
        assert len(bad["ray"]) < len(ref["ray"]) and MX.per_ray(bad)[MX.dyadic_rays()["names"].index("hi_face")] == 0
        return
    np.testing.assert_array_equal(bad["t_start"], ref["t_start"])
    if broken == "no_clamp":
        k, ok = MX.keep_unclamped(bad, b)
        differs = ok & (k != MX.keep(ref, b))
    else:
        differs = MX.keep(bad, b) != MX.keep(ref, b)
        assert np.all(ref["on_box_face"][differs][:, :2].any(1))
    print(f"{broken}: {differs.sum()} keep decisions differ")
    assert differs.sum() >= 5


# ---- cone scenes -----------------------------------------------------------------------------------------------------------
def test_cone_scenes_switch_where_designed_and_stay_clear_of_faces():
    rays, ref = MX.cone_rays(), MX.cone_reference()
    assert ref["k1"] == rays["k1"] == [None, 56, 64, 63, 0, 0]
    n = MX.per_ray(ref)
    print(f"cone scene: candidates per ray {n.tolist()}, ambiguous {ref['ambiguous'].sum()} of {len(ref['ray'])}")
    assert n[0] == 0 and np.all(n[1:] > 128)  # every ray runs past its second chunk
    m = UR.march_levels(MX.level_boxes(3), MX.binaries_for("random", 3), rays["o"], rays["d"], MX.CONE_STEP, 0.0, 1e10,
                        rays["t_min"], rays["t_max"], cone_angle=MX.CONE, margin=1e-4)
    assert m["ambiguous"].mean() <= 0.005 and ref["ambiguous"].mean() <= 0.005
    # the fp32 restatement marches the same candidates: the counts are decided away from rounding ...
    tol = MX.cone_tolerance()
    np.testing.assert_array_equal(m["ray"], ref["ray"])
    assert np.abs(m["t_start"] - ref["t_start"]).max() <= tol and np.abs(m["t_end"] - ref["t_end"]).max() <= tol
    sure = ~(ref["ambiguous"] | m["ambiguous"])
    np.testing.assert_array_equal(m["keep"][sure], MX.keep(ref, MX.binaries_for("random", 3))[sure])
    for r in range(1, len(n)):
        mine = ref["ray"] == r
        ts, te, t_far = ref["t_start"][mine], ref["t_end"][mine], ref["t_far"][r]
        assert t_far - ts[-1] > 100 * tol and te[-1] == t_far  # ... the last candidate starts well before t_far,
        growth = 1.0 + MX.CONE
        assert ts[-1] * growth - t_far > 100 * tol             # and the next one would start well beyond it
        # the uniform part is exact in fp32, and so is the first cone candidate's start, t1 = 16 (or t_near)
        uniform = ref["k"][mine] < ref["k1"][r]
        assert np.all(ts[uniform].astype(f32) == ts[uniform]) and np.all(te[uniform].astype(f32) == te[uniform])
        assert uniform.sum() == ref["k1"][r] and ts[ref["k1"][r]] == max(16.0, ref["t_near"][r])
        assert not ref["ambiguous"][mine][uniform].any()
    # caps cut every ray of the cone scene, before, at and after k1 and the chunk seams
    assert all((np.minimum(n, cap) < n)[1:].all() for cap in MX.CAPS if cap <= 129)
