"""S6: occupancy-grid march (ballot/popcount compaction) vs its CPU restatement + invariants.  Parity with nerfacc is
unpinned (un-vendored, no caller, no golden in the reference) -- see DESIGN.md."""
import numpy as np
import pytest
import torch

import occgrid_oracle as OO
import occgrid_update_restatement as UR
import scan_refs as SR
import synth
from gpu_util import cuda

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cone", [0.0, 0.01])
def test_occgrid_march_vs_restatement(cone):
    from neurad_studio_amd import ops

    res, R = 32, 200
    rng = np.random.default_rng(0)
    binaries = rng.random((res, res, res)) < 0.3
    aabb = np.array([-10, -10, -2, 10, 10, 6], np.float32)
    o = (synth.normal((R, 3), 1) * np.array([6.0, 6.0, 2.0])).astype(np.float32)
    d = synth.normal((R, 3), 2)
    d[:5, 0] = 0.0  # axis-parallel components
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    t_max = synth.uniform((R,), 5.0, 60.0, 3)
    ri, ts, te, seg = ops.occgrid_march(ops.OccGridSpec(torch.from_numpy(aabb), cuda(binaries)), cuda(o), cuda(d), 0.25,
                                        near_plane=0.1, far_plane=40.0, t_max=cuda(t_max), cone_angle=cone)
    ri, ts, te = ri.cpu().numpy(), ts.cpu().numpy(), te.cpu().numpy()
    # every candidate interval whose float64 midpoint is further than 1e-4 (in cells) from a cell face and from the box is
    # kept or dropped exactly as the restatement says; at most 0.5 % may be that close (the three-level test's comparison)
    m = UR.march_levels(aabb[None], binaries[None], o, d, 0.25, 0.1, 40.0, None, t_max, cone_angle=cone)
    share = m["ambiguous"].mean()
    print(f"{len(m['ray'])} candidates, {m['keep'].sum()} kept, {len(ri)} emitted, ambiguous share {share:.2e}")
    assert len(m["ray"]) > 4000 and share <= 0.005
    emitted = np.zeros(len(m["ray"]), bool)
    first = np.searchsorted(m["ray"], np.arange(R + 1))
    tol = 4 * 2.0 ** -23 * 40.0  # candidates are a step apart; powf may differ from the restatement's by an ulp or two
    for r in range(R):
        cand_ts, cand_te = m["t_start"][first[r]:first[r + 1]], m["t_end"][first[r]:first[r + 1]]
        mine = ri == r
        if not mine.any():
            continue
        assert len(cand_ts), f"ray {r}: samples from a ray the restatement never marches"
        k = np.abs(ts[mine][:, None] - cand_ts[None]).argmin(1)
        assert np.all(np.diff(k) > 0)
        assert np.abs(ts[mine] - cand_ts[k]).max() <= tol and np.abs(te[mine] - cand_te[k]).max() <= tol
        if cone == 0.0:
            np.testing.assert_array_equal(ts[mine].view(np.int32), cand_ts[k].view(np.int32))
        emitted[first[r] + k] = True
    sure = ~m["ambiguous"]
    np.testing.assert_array_equal(emitted[sure], m["keep"][sure])
    # invariants: packed order, segments, sorted non-overlapping intervals inside [near, min(far, t_max)]
    assert np.all(np.diff(ri) >= 0) and seg[-1].item() == len(ri)
    for r in np.unique(ri)[:50]:
        m = ri == r
        assert np.all(ts[m][1:] >= te[m][:-1] - 1e-5) and np.all(te[m] > ts[m])
        assert ts[m].min() >= 0.1 - 1e-6 and te[m].max() <= min(40.0, t_max[r]) + 1e-5
    # every emitted midpoint sits in an occupied cell
    p = o[ri] + d[ri] * (0.5 * (ts + te))[:, None]
    idx = np.clip(np.floor((p - aabb[:3]) / (aabb[3:] - aabb[:3]) * res).astype(int), 0, res - 1)
    assert binaries[idx[:, 0], idx[:, 1], idx[:, 2]].mean() > 0.995


def test_estimator_sampling_with_alpha_pruning_and_empty_grid():
    from neurad_studio_amd import ops
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    est = OccGridEstimator([-5, -5, -5, 5, 5, 5], resolution=16)
    R = 64
    o = cuda(np.zeros((R, 3), np.float32))
    d = synth.normal((R, 3), 5)
    d = cuda((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32))
    ri, ts, te = est.sampling(o, d, render_step_size=0.5, far_plane=100.0)
    assert ri.numel() > 0 and float(te.max()) <= 5 * np.sqrt(3) + 1e-3
    alpha_fn = lambda ts, te, ri: torch.full_like(ts, 0.5)  # noqa: E731
    ri2, ts2, te2 = est.sampling(o, d, alpha_fn=alpha_fn, render_step_size=0.5, far_plane=100.0, early_stop_eps=1e-2)
    # T = 0.5^k >= 1e-2  ->  at most 7 samples per ray survive
    assert ri2.numel() <= 7 * R and ri2.numel() < ri.numel()
    a = torch.full((ri.numel(),), 0.5, device="cuda")
    seg = torch.zeros(R + 1, dtype=torch.int64, device="cuda")
    seg[1:] = torch.cumsum(torch.bincount(ri, minlength=R), 0)
    keep = ops.packed_visibility_from_alpha(a, seg, 1e-2, 0.0).cpu().numpy()
    np.testing.assert_array_equal(keep, OO.packed_visibility_from_alpha(a.cpu().numpy(), seg.cpu().numpy(), 1e-2, 0.0))
    est.binaries[:] = False
    ri3, _, _ = est.sampling(o, d, render_step_size=0.5)
    assert ri3.numel() == 0


# ---- packed_visibility_from_alpha past a ray's first 64-sample chunk (tests/scan_refs.py; the designed crossings and the
# band are checked in tests/test_scan_refs_host.py) ---------------------------------------------------------------------------
@pytest.mark.parametrize("alpha_thre", SR.VIS_ALPHA_THRES)
def test_packed_visibility_exact_across_chunks(alpha_thre):
    """Rays of 0 to 700 samples, 13 of them (a ragged last workgroup), every 1 - alpha in {1, 1/2, 1/4} and eps = 2^-20: each
    transmittance is a power of two, each comparison exact.  T first drops below eps inside chunk 0, at samples 63, 64 and
    65, inside chunk 2, inside a ragged last chunk, or never; some samples see T == eps and are kept."""
    from neurad_studio_amd import ops

    seg, a = SR.vis_segments(), SR.vis_exact_alphas()
    want = OO.packed_visibility_from_alpha(a, seg, SR.VIS_EXACT_EPS, alpha_thre)
    keep = ops.packed_visibility_from_alpha(cuda(a), cuda(seg), SR.VIS_EXACT_EPS, alpha_thre).cpu().numpy()
    assert 0 < want.sum() < len(want)
    np.testing.assert_array_equal(keep, want)


def test_packed_visibility_writes_every_entry_and_nothing_else():
    """The mask comes from torch.empty: behind an early termination the kernel itself has to write the zeros, when the ray
    ends one, two or several chunks later.  Into a buffer of 0xFF with a guard byte on each side."""
    from neurad_studio_amd import ops

    seg, a = SR.vis_segments(), SR.vis_exact_alphas()
    buf = torch.full((len(a) + 2,), 0xFF, dtype=torch.uint8, device="cuda")
    ops.launch("nrhip_packed_visibility_from_alpha", cuda(a), cuda(seg), len(seg) - 1, SR.VIS_EXACT_EPS, 0.0, buf[1:-1])
    got = buf.cpu().numpy()
    assert got[0] == 0xFF and got[-1] == 0xFF
    assert set(np.unique(got[1:-1])) == {0, 1}
    np.testing.assert_array_equal(got[1:-1].astype(bool), OO.packed_visibility_from_alpha(a, seg, SR.VIS_EXACT_EPS, 0.0))


def test_packed_visibility_generic_alphas_vs_float64():
    """alphas from U[0, 0.05], eps 1e-3, alpha_thre 0.02: three rays cross eps beyond their first chunk.  Samples whose
    float64 T lies within a relative 1e-4 of eps are left out (the fp32 T is a product through fewer than 1024 roundings:
    1024 * 2^-24 = 6.1e-5); at most 0.5 % may be, asserted from the reference alone."""
    from neurad_studio_amd import ops

    seg, a = SR.vis_segments(), SR.vis_generic_alphas()
    eps, thre = SR.VIS_GENERIC_EPS, SR.VIS_GENERIC_ALPHA_THRE
    want, T = SR.visibility64(a, seg, eps, thre)
    left_out = np.abs(T - eps) <= SR.VIS_BAND * eps
    print(f"{left_out.sum()} of {len(a)} samples left out")
    assert left_out.mean() <= SR.VIS_MAX_LEFT_OUT
    assert sum(c is not None and c >= SR.CHUNK for c in SR.first_below(T, seg, eps)) >= 3
    keep = ops.packed_visibility_from_alpha(cuda(a), cuda(seg), eps, thre).cpu().numpy()
    np.testing.assert_array_equal(keep[~left_out], want[~left_out])


def test_volumetric_sampler_module():
    from neurad_studio_amd.cameras.rays import RayBundle
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    est = OccGridEstimator([-5, -5, -5, 5, 5, 5], resolution=16)
    R = 32
    d = synth.normal((R, 3), 6)
    rb = RayBundle(origins=torch.zeros(R, 3, device="cuda"),
                   directions=cuda((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)),
                   pixel_area=torch.full((R, 1), 1e-6, device="cuda"), nears=torch.zeros(R, 1, device="cuda"),
                   fars=torch.full((R, 1), 3.0, device="cuda"))
    s = VolumetricSampler(est).eval()
    rs, ri = s(rb, render_step_size=0.25)
    assert rs.frustums.starts.shape == (ri.shape[0], 1) and float(rs.frustums.ends.max()) <= 3.0 + 1e-5
    assert ri.shape[0] == R * 12  # 3.0 / 0.25 intervals per ray in a fully occupied grid
    with pytest.raises(RuntimeError):
        s.generate_ray_samples()
    est.binaries[:] = False
    rs2, ri2 = s(rb, render_step_size=0.25)
    assert ri2.shape[0] == 1 and float(rs2.frustums.starts[0, 0]) == 1.0  # fake-sample fallback
