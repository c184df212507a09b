"""CPU side of the occupancy-grid update: the restatement's own invariants (tests/occgrid_update_restatement.py), the
preconditions the GPU tests rely on, and the argument validation of the new entry points that needs no device.
The rule is modelled on nerfacc 0.5; parity with nerfacc itself is unpinned (un-vendored)."""
import ctypes

import numpy as np
import pytest
import torch

import occgrid_update_restatement as UR

# ---- the restatement's invariants ------------------------------------------------------------------------------------------
def test_level_boxes_are_nested_doublings():
    a = UR.level_aabbs([-1, -2, 0, 3, 2, 1], 3)
    np.testing.assert_array_equal(a[0], np.array([-1, -2, 0, 3, 2, 1], np.float32))
    np.testing.assert_array_equal(a[1], np.array([-3, -4, -0.5, 5, 4, 1.5], np.float32))
    np.testing.assert_array_equal(a[2], np.array([-7, -8, -1.5, 9, 8, 2.5], np.float32))
    from neurad_studio_amd import ops

    np.testing.assert_array_equal(ops.occgrid_level_aabbs([-1, -2, 0, 3, 2, 1], 3).numpy(), a)


@pytest.mark.parametrize("occ_thre", [1e-3, 1e-2], ids=["mean_above_occ_thre", "mean_below_occ_thre"])
def test_shell_scenario_threshold_gap_and_invariants(occ_thre):
    """binaries == occs > thre on every cell, invisible cells excluded; both regimes really occur; and no visible cell's
    value lies within 1e-3 (relative) of the threshold -- the precondition of the GPU test's exact comparison (a reordered
    fp32 sum would move the mean by ~2e-7)."""
    for step, d, out in UR.shell_run(occ_thre):
        occs = out["occs"]
        np.testing.assert_array_equal(out["binaries"].reshape(-1), occs > out["thre"])
        assert out["thre"] == (np.float32(occ_thre) if occ_thre < 5e-3 else np.float32(out["mean"]))
        assert (out["mean"] > occ_thre) == (occ_thre < 5e-3)
        gap = UR.threshold_gap(occs, out["thre"])
        print(f"step {step}: mean {out['mean']:.6g} thre {out['thre']:.6g} nearest value {gap:.3g} (relative)")
        assert gap > 1e-3
        n, cap = UR.capacity(32, step < 256)
        assert out["ids"].shape == (2, cap) and np.all(out["counts"] <= cap)
        if step >= 256:  # level 0 has more than n occupied cells (selection with replacement), level 1 fewer
            assert out["counts"][0] == 2 * n and n < out["counts"][1] < 2 * n


def test_candidates_positions_and_ema_invariants():
    res, L = 8, 2
    rng = np.random.default_rng(1)
    aabbs = UR.level_aabbs([-1, -1, -1, 1, 1, 1], L)
    occs = rng.random(L * res ** 3).astype(np.float32)
    occs[rng.random(occs.shape) < 0.2] = -1.0
    binaries = rng.random(L * res ** 3) < 0.5
    d = UR.draws(res, L, False, 2)
    ids, counts = UR.candidates(occs, binaries, res, L, False, None, d["cell_draws"], d["sel_draws"])
    for l in range(L):
        got = ids[l, :counts[l]]
        assert np.all(got >= 0) and np.all(ids[l, counts[l]:] == -1)
        assert np.all(occs.reshape(L, -1)[l][got] >= 0)  # never an invisible cell
    pos = UR.positions(aabbs, res, ids, d["jitter"])
    lo, hi = UR.cell_boxes(aabbs, res, ids)
    ok = ids >= 0
    assert np.all((pos >= lo)[ok]) and np.all((pos <= hi)[ok])  # power-of-two boxes: exact
    np.testing.assert_array_equal(pos[~ok], np.zeros_like(pos[~ok]))  # the boxes' centre
    vals = rng.normal(0, 1, ids.shape).astype(np.float32)
    new = UR.ema(occs, res, ids, counts, vals, 0.95)
    touched = np.zeros((L, res ** 3), bool)
    for l in range(L):
        touched[l][ids[l, :counts[l]]] = True
    touched = touched.reshape(-1)
    np.testing.assert_array_equal(new[~touched].view(np.uint32), occs[~touched].view(np.uint32))
    assert np.all(new[occs < 0] == -1.0)


def test_mark_invisible_fp32_restatement_stays_inside_the_margin():
    """fp32 and float64 evaluations of the visibility rule agree on every cell whose tests are not within 1e-3 of a bound,
    and fewer than 1 % of the cells are that close: the GPU test's bound"""
    K, c2w, w, h = UR.cameras()
    aabbs = UR.level_aabbs([-4, -4, -4, 4, 4, 4], 2)
    v32 = UR.mark_invisible(aabbs, 32, K, c2w, w, h, 0.5)
    v64, amb = UR.mark_invisible(aabbs, 32, K, c2w, w, h, 0.5, dtype=np.float64, margin=1e-3)
    print(f"visible {v64.mean():.3f}, ambiguous {amb.mean():.5f}, fp32 != float64 on {(v32 != v64).sum()} cells")
    assert 0.05 < v64.mean() < 0.95 and amb.mean() < 0.01
    np.testing.assert_array_equal(v32[~amb], v64[~amb])
    # the near plane matters: cameras inside the grid make cells invisible that they would otherwise see
    assert (UR.mark_invisible(aabbs, 32, K, c2w, w, h, 0.0) & ~v32).any()


def test_march_levels_restatement_matches_the_single_level_oracle():
    import occgrid_oracle as OO
    import synth

    rng = np.random.default_rng(0)
    binaries = rng.random((1, 16, 16, 16)) < 0.3
    aabb = np.array([-2, -2, -1, 2, 2, 1], np.float32)
    o = (synth.normal((20, 3), 1) * 0.8).astype(np.float32)
    d = synth.normal((20, 3), 2)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    m = UR.march_levels(aabb[None], binaries, o, d, 0.1, 0.05, 10.0)
    ri, ts, te = OO.occgrid_march(aabb, binaries[0], o, d, 0.1, 0.05, 10.0)
    k = m["keep"]
    np.testing.assert_array_equal(m["ray"][k], ri)
    np.testing.assert_array_equal(m["t_start"][k], ts)
    np.testing.assert_array_equal(m["t_end"][k], te)
    assert m["ambiguous"].mean() < 0.005


# ---- argument validation that needs no device ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from neurad_studio_amd import _lib

    return _lib.load()


def _levels(L=2, res=8, binaries=0x1000):
    from neurad_studio_amd import _lib

    g = _lib.OccGridLevels()
    g.levels, g.resolution, g.binaries = L, res, binaries
    for l, box in enumerate(UR.level_aabbs([-1, -1, -1, 1, 1, 1], min(max(L, 1), 8))):
        for i, v in enumerate(box):
            g.aabbs[l][i] = float(v)
    return g


def test_version_and_workspace_query(lib):
    from neurad_studio_amd import _lib

    assert lib.nrhip_version() >= 513
    need = ctypes.c_int64(0)
    _lib.call("nrhip_occgrid_update_workspace", 2, 32, ctypes.byref(need))
    cells = 32 ** 3
    assert 2 * cells * 8 <= need.value <= 2 * cells * 8 + (1 << 20)  # max keys + occupied list, + bookkeeping
    with pytest.raises(_lib.NeuradHipError, match="levels"):
        _lib.call("nrhip_occgrid_update_workspace", 9, 32, ctypes.byref(need))
    with pytest.raises(_lib.NeuradHipError, match="NULL"):
        _lib.call("nrhip_occgrid_update_workspace", 2, 32, None)


def test_entry_points_validate_on_the_host(lib):
    from neurad_studio_amd import _lib

    one, ref = ctypes.c_void_p(0x1000), ctypes.byref
    big = 1 << 40
    march = lambda g, r, step=0.1: _lib.call("nrhip_occgrid_march_levels", ref(g), None, None, None, None, None, r, step,  # noqa: E731
                                             0.0, 1e10, 0.0, 1024, None, None, None, None, None, None)
    march(_levels(), 0)  # no rays: a no-op that reads no pointer
    with pytest.raises(_lib.NeuradHipError, match="levels"):
        march(_levels(L=0), 0)
    with pytest.raises(_lib.NeuradHipError, match="levels"):
        march(_levels(L=9), 0)
    with pytest.raises(_lib.NeuradHipError, match="NULL"):
        march(_levels(binaries=None), 0)
    with pytest.raises(_lib.NeuradHipError, match="bad argument"):
        march(_levels(), 0, step=0.0)
    with pytest.raises(_lib.NeuradHipError, match="null rays"):
        march(_levels(), 4)
    g = _levels()
    g.aabbs[1][0] = -0.5  # level 1 no longer contains level 0
    with pytest.raises(_lib.NeuradHipError, match="does not contain"):
        march(g, 0)
    g = _levels()
    g.aabbs[0][3] = -1.0
    with pytest.raises(_lib.NeuradHipError, match="empty AABB"):
        march(g, 0)

    cand = lambda g, warm, n, ws=one, wsb=big, occs=one: _lib.call(  # noqa: E731
        "nrhip_occgrid_update_candidates", ref(g), occs, warm, n, one, one, one, one, one, one, ws, wsb, None)
    cand(_levels(res=1), 0, 0)  # res^3 // 4 == 0 draws: nothing to do, nothing read
    cand(_levels(res=1), 0, 0, ws=None, wsb=0, occs=None)  # ... not even the workspace
    with pytest.raises(_lib.NeuradHipError, match="workspace"):
        cand(_levels(), 1, 128, ws=None)
    with pytest.raises(_lib.NeuradHipError, match="workspace"):
        cand(_levels(), 1, 128, wsb=16)
    with pytest.raises(_lib.NeuradHipError, match="outside"):
        cand(_levels(), 0, 8 ** 3 + 1)
    with pytest.raises(_lib.NeuradHipError, match="NULL"):
        cand(_levels(), 1, 128, occs=None)
    with pytest.raises(_lib.NeuradHipError, match="draws"):
        _lib.call("nrhip_occgrid_update_candidates", ref(_levels()), one, 0, 128, None, None, one, one, one, one, one, big, None)

    with pytest.raises(_lib.NeuradHipError, match="capacity"):
        _lib.call("nrhip_occgrid_update_apply", ref(_levels()), one, 8 ** 3 + 1, one, one, one, 0.95, 0.01, one, big, None)
    with pytest.raises(_lib.NeuradHipError, match="NULL"):
        _lib.call("nrhip_occgrid_update_apply", ref(_levels()), one, 16, None, one, one, 0.95, 0.01, one, big, None)
    with pytest.raises(_lib.NeuradHipError, match="workspace"):
        _lib.call("nrhip_occgrid_update_apply", ref(_levels()), one, 16, one, one, one, 0.95, 0.01, one, 8, None)

    with pytest.raises(_lib.NeuradHipError, match="intrinsics"):
        _lib.call("nrhip_occgrid_mark_invisible", ref(_levels()), one, 3, one, 8, 64, 48, 0.0, one, None)
    with pytest.raises(_lib.NeuradHipError, match="empty image"):
        _lib.call("nrhip_occgrid_mark_invisible", ref(_levels()), one, 1, one, 8, 0, 48, 0.0, one, None)
    with pytest.raises(_lib.NeuradHipError, match="NULL"):
        _lib.call("nrhip_occgrid_mark_invisible", ref(_levels()), None, 1, one, 8, 64, 48, 0.0, one, None)


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from neurad_studio_amd import _lib, ops

    grid = ops.OccGridSpec(torch.tensor([-1.0, -1, -1, 1, 1, 1]), torch.ones(2, 8, 8, 8, dtype=torch.bool))
    with pytest.raises(_lib.NeuradHipError):
        ops.occgrid_update_candidates(grid, torch.zeros(2 * 512), True)
    with pytest.raises(_lib.NeuradHipError):
        ops.occgrid_mark_invisible(grid, torch.zeros(2 * 512), torch.eye(3)[None], torch.zeros(4, 3, 4), 64, 48)
    assert ops.occgrid_update_capacity(8, True) == (128, 512) and ops.occgrid_update_capacity(8, False) == (128, 256)
    assert grid.levels == 2 and grid.resolution == 8


def test_estimator_is_a_module_with_gating_and_state():
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    est = OccGridEstimator([-1, -1, -1, 1, 1, 1], resolution=8, levels=3, device="cpu")
    assert isinstance(est, torch.nn.Module)
    assert set(est.state_dict()) == {"aabbs", "occs", "binaries", "resolution", "fresh"}
    assert est.binaries.shape == (3, 8, 8, 8) and est.binaries.all() and est.occs.shape == (3 * 512,) and (est.occs == 1).all()
    np.testing.assert_array_equal(est.aabbs.numpy(), UR.level_aabbs([-1, -1, -1, 1, 1, 1], 3))
    assert bool(est.fresh) and est.resolution.tolist() == [8, 8, 8]
    called = []
    fn = lambda x: called.append(x) or x[:, :1]  # noqa: E731
    est.update_every_n_steps(step=5, occ_eval_fn=fn, n=16)  # not a multiple of n: nothing happens, not even on a CPU grid
    assert not called and bool(est.fresh) and (est.occs == 1).all()
    est.eval()
    with pytest.raises(RuntimeError, match="training"):
        est.update_every_n_steps(step=0, occ_eval_fn=fn)
    with pytest.raises(ValueError):
        OccGridEstimator([-1, -1, -1, 1, 1, 1], resolution=8, levels=0, device="cpu")
    other = OccGridEstimator([-2, -2, -2, 2, 2, 2], resolution=8, levels=3, device="cpu")
    sd = est.state_dict()
    sd["fresh"] = torch.tensor(False)
    other.load_state_dict(sd)
    np.testing.assert_array_equal(other._spec().aabb.numpy(), est.aabbs.numpy())  # the host copy of the boxes follows
    other._end_fresh()
    assert (other.occs == 1).all()  # not fresh any more: nothing is zeroed
