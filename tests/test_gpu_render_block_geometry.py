"""The fused render kernel computes a sample's geometry (interval, gaussian, contraction) once per BLOCK of four consecutive
tiles = 64 samples of a ray and hands it to the block's tiles (csrc/render.hip: fill_block): every way a block can be cut
short or entered -- S around the tile and the block size, processing orders, a launch over a slice of the order that starts
in its middle (the actor route's second launch), packed segments including empty ones, early termination inside a block --
for the composited, the actor, the override and the activation-saving kernels.

References and bounds are the existing render tests': the numpy oracle at TOL (tests/test_gpu_render_variants.py,
tests/test_gpu_render_packed.py, tests/test_gpu_actors.py), bit equality between processing orders, the early-termination
properties of test_early_ray_termination_bounded, and for the training forward the same kernel on every sample as a ray of
its own at 1e-5 (tests/test_gpu_render_train_packed.py) with the encoding and the feature against the oracle at TIGHT
(tests/test_gpu_field_shapes.py)."""
import functools

import numpy as np
import pytest
import torch

import neurad_oracle as O
import packed_actor_refs as PA
import packed_train_refs as T
import synth
from builders import field_params, sample_rays
from conftest import rel_l2
from gpu_util import TIGHT, TOL, cuda, dev, host, to_spec
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 63, 64, 65, 128, 130)  # around one tile, one block, two blocks
ORDER = np.array([3, 0, 4, 1, 2], np.int32)
R = 5


@functools.lru_cache(maxsize=None)
def headline_params():
    p = field_params(use_sdf=True, L=16, F=2, lg=12, H=64, mn=16, mx=1024, scale=2.0)
    p.beta = 3.0  # alphas away from saturation: the compositing is exercised
    return p


@functools.lru_cache(maxsize=None)
def block_rays(S):
    """5 rays x S samples.  Ray 0 runs along +x from the origin with even bins out to 260 m: the contraction boundary
    |x|_inf = 1 (100 m at static_scale 100) falls at sample 0.385 S, inside the ray's first block.  Ray 1 starts 150 m out
    and lies wholly outside the boundary.  Rays 2-4: the power sampler's bins on synthetic rays."""
    o, d, area, s, e, _ = sample_rays(R, S, seed=40 + S)
    o, d, s, e = o.copy(), d.copy(), s.copy(), e.copy()
    edges = np.linspace(0.5, 260.0, S + 1, dtype=np.float32)
    o[0], d[0] = (0.3, -0.2, 0.1), (1.0, 0.0, 0.0)
    o[1], d[1] = (150.0, 20.0, 5.0), (1.0, 0.0, 0.0)
    s[:2], e[:2] = edges[:-1], edges[1:]
    mag = np.abs(o[:2, None, :] + d[:2, None, :] * ((s[:2] + e[:2]) / 2)[..., None]).max(-1) / 100.0  # [2, S]
    if S >= 15:
        blk = mag[0, :64]
        assert (blk < 1).any() and (blk >= 1).any(), "ray 0's first block must straddle the contraction boundary"
    assert (mag[1] > 1).all()
    return o, d, area, s, e


@functools.lru_cache(maxsize=None)
def dense_reference(S):
    return O.render_rays(headline_params(), *block_rays(S))


def check_render(got, ref):
    feats, depth, acc, w = got
    assert rel_l2(host(w), ref["weights"]) < TOL
    assert rel_l2(host(feats), ref["features"]) < TOL
    assert rel_l2(host(depth), ref["depth"]) < TOL or np.abs(host(depth) - ref["depth"]).max() < 1e-5
    assert rel_l2(host(acc), ref["accumulation"]) < TOL


# ---- 1. dense layout, with and without a processing order --------------------------------------------------------------
@pytest.mark.parametrize("ordered", [False, True], ids=["batch-order", "permuted"])
@pytest.mark.parametrize("S", SIZES)
def test_dense_blocks_vs_oracle(ops, S, ordered):
    fs = to_spec(ops, headline_params())
    o, d, area, s, e = (dev(a) for a in block_rays(S))
    got = ops.render_fwd(fs, o, d, area, s, e, return_weights=True, order=cuda(ORDER) if ordered else None)
    check_render(got, dense_reference(S))
    if ordered:  # an order moves rays between waves and must not change a bit
        for a, b in zip(got, ops.render_fwd(fs, o, d, area, s, e, return_weights=True)):
            assert torch.equal(a, b)


# ---- 2. a launch over a slice of the order that starts mid-order; the actor kernel ------------------------------------
@functools.lru_cache(maxsize=None)
def actor_field():
    return PA.make_actor_field("street")  # 8 x 4, H = 32: the smallest actor shape of tests/test_gpu_packed_actors.py


@pytest.mark.parametrize("S", SIZES)
def test_actor_route_slices_the_order_mid_way(S):
    """The actor route renders one order as two launches over slices of it: the rays without candidates through the static
    kernel, the others -- a slice that starts in the middle of the order -- through the actor kernel, whose box test reads
    the block's gaussians.  Rays 0 and 3 of the street scene pass no actor; the other three run through the row of boxes
    and out past the contraction boundary (108 m)."""
    fld, p, ap = actor_field()
    sc = PA.scene("street")
    o, d, area, times = (sc[k][:R] for k in ("o", "d", "area", "times"))
    edges = np.linspace(0.0, 108.0, S + 1, dtype=np.float32)[None].repeat(R, 0)
    st, en = np.ascontiguousarray(edges[:, :-1]), np.ascontiguousarray(edges[:, 1:])
    ref = O.field_fwd_actors(p, ap, o, d, area, st, en, times)
    w_ref = O.render_weight_from_alpha(ref["alpha"])[0]
    f_ref, d_ref, a_ref = O.composite(w_ref, ref["feature"], st, en)
    want = {"weights": w_ref, "features": f_ref, "depth": d_ref, "accumulation": a_ref}
    args = (cuda(o), cuda(d), cuda(area), cuda(st), cuda(en))
    cnt = fld.hashgrid.prepare_actors(*args, cuda(times))[1][0]
    if S > 1:  # (one sample per ray: the candidate test's line has no direction and keeps every actor for every ray)
        assert 0 < int((cnt > 0).sum()) < R, "both launches must get rays"
    with torch.no_grad():
        plain = fld.render(*args, return_weights=True, times=cuda(times))
        permuted = fld.render(*args, return_weights=True, times=cuda(times), order=cuda(ORDER))
    check_render(plain, want)
    for a, b in zip(plain, permuted):
        assert torch.equal(a, b)


# ---- 3. packed layout ----------------------------------------------------------------------------------------------------
PACKED_COUNTS = (0, 1, 16, 17, 64, 70)


@pytest.mark.parametrize("counts", [PACKED_COUNTS, PACKED_COUNTS[::-1]], ids=["empty-first", "empty-last"])
def test_packed_segments_vs_oracle(ops, counts):
    p = T.params(16, 2, 64, True)
    fs = to_spec(ops, p)
    rays = T.packed_rays(tuple(counts), 7)
    o, d, area, ts, te, seg, _ = T.on_device(rays)
    got = ops.render_fwd_packed(fs, o, d, area, ts, te, seg, return_weights=True)
    for name, g, w in zip(("features", "depth", "accumulation", "weights"), got, T.oracle_route(p, rays)):
        err = rel_l2(host(g).reshape(-1), w.reshape(-1))
        assert err < TOL or (name == "depth" and np.abs(host(g).reshape(-1) - w.reshape(-1)).max() < 1e-5), (name, err)
    empty = torch.from_numpy(np.asarray(counts) == 0).cuda()
    for t in got[:3]:  # a ray without samples: exactly zero
        assert bool((t[empty] == 0).all())
    order = cuda(np.array([4, 0, 5, 2, 1, 3], np.int32))
    for a, b in zip(got, ops.render_fwd_packed(fs, o, d, area, ts, te, seg, return_weights=True, order=order)):
        assert torch.equal(a, b)


# ---- 4. early termination inside a block -------------------------------------------------------------------------------
def test_early_termination_inside_a_block(ops):
    """More rays than the persistent grid has waves (2 workgroups x 4 waves per CU), two blocks per ray, rays that stop in
    tile 1 or 2 of their first block: the wave's next ray must open a block of its own.  The properties of
    test_early_ray_termination_bounded: skipped weights are zero, everything in front of the cut keeps its bits, what was
    dropped weighs less than eps."""
    p = field_params(use_sdf=True, L=8, F=4, lg=11, H=32, scale=2.0)
    p.beta = 6.0  # alphas around 0.5: the transmittance is below 1e-3 after a dozen samples
    n_rays, S, eps = 4500, 128, 1e-3
    o, d, area, s, e, _ = sample_rays(n_rays, S, seed=21)
    fs = to_spec(ops, p)
    args = (fs, dev(o), dev(d), dev(area), dev(s), dev(e))
    f0, d0, a0, w0 = ops.render_fwd(*args, return_weights=True)
    f1, d1, a1, w1 = ops.render_fwd(*args, return_weights=True, early_stop_eps=eps)
    T_enter = 1.0 - torch.cumsum(w0.double(), -1)[:, 15::16]  # behind tiles 0, 1, ...
    T_enter = torch.cat([torch.ones_like(T_enter[:, :1]), T_enter[:, :-1]], 1)
    stop = T_enter < eps * 0.5  # margin: the fp32 carry against this fp64 sum
    last = torch.where(stop.any(1), stop.float().argmax(1), torch.full((n_rays,), S // 16 - 1, device="cuda"))
    inside = ((last + 1) % 4 != 0).float().mean()
    assert float(inside) > 0.5, "most rays must stop inside a block"
    skipped = torch.arange(S, device="cuda")[None, :] >= (16 * (last + 1))[:, None]
    assert bool((w1[skipped] == 0).all())
    kept = ~((w1 == 0) & (w0 != 0))
    assert torch.equal(w1[kept], w0[kept])
    assert float((w0 * (~kept)).sum(-1).max()) <= eps * 1.01
    assert float((a1 - a0).abs().max()) <= eps * 1.01
    assert float((f1 - f0).abs().max()) <= 3 * eps * (float(f0.abs().max()) + 1.0)


# ---- 5. the activation-saving kernel and its override variant ----------------------------------------------------------
NAMES7 = ("feature", "geo_out", "head", "save_enc", "save_geo_hidden", "save_feat_in", "save_feat_hidden")


def every_sample_a_ray(ops, fs, o, d, area, s, e, override=None):
    """the same kernel on [N, 1]: every sample is tile 0, lane 0 of a ray of its own"""
    n_rays, S = s.shape
    rep = lambda t: t.repeat_interleave(S, 0)  # noqa: E731
    out, saved = ops.field_fwd_train(fs, rep(o), rep(d), rep(area), s.reshape(-1, 1), e.reshape(-1, 1), override=override)
    return (*out, *saved)


@pytest.mark.parametrize("S", [17, 65])
def test_training_forward_saves_the_same_rows(ops, S):
    p = headline_params()
    fs = to_spec(ops, p)
    rays = block_rays(S)
    o, d, area, s, e = (dev(a) for a in rays)
    out, saved = ops.field_fwd_train(fs, o, d, area, s, e)
    for name, g, w in zip(NAMES7, (*out, *saved), every_sample_a_ray(ops, fs, o, d, area, s, e)):
        err = rel_l2(host(g).reshape(-1), host(w).reshape(-1))
        assert g.numel() == w.numel() and err < 1e-5, (name, err)
    assert rel_l2(host(saved[0]), O.encode_static(p.grid, 100.0, *rays)) < TIGHT
    ref = O.field_fwd(p, *rays)
    assert rel_l2(host(out[0]).reshape(-1, 32), ref["feature"].reshape(-1, 32)) < TIGHT
    assert rel_l2(host(out[1]).reshape(-1), ref["sdf"].reshape(-1)) < TOL
    assert rel_l2(host(out[2]).reshape(-1), ref["alpha"].reshape(-1)) < TOL


def test_override_rows_in_a_partial_block(ops):
    """23 rays x 37 samples (two full tiles and five samples of one block), the shape of
    test_forward_kernel_is_the_dense_override_kernel_bit_for_bit, 8 x 4 levels, H = 32"""
    n_rays, S, L, F, H = 23, 37, 8, 4, 32
    p = PA.shape_params(L, F, H)
    fs = to_spec(ops, p)
    o, d, area, s, e, _ = sample_rays(n_rays, S, seed=9)
    o, d, area, s, e = (dev(a) for a in (o, d, area, s, e))
    M, P = n_rays * S, 97
    rng = np.random.default_rng(5)
    where = rng.permutation(M)[:P]
    where[:3] = (0, S - 1, M - 1)  # a ray's first and last sample, the batch's last
    ovr = np.full(M, -1, np.int32)
    ovr[where] = rng.permutation(P).astype(np.int32)
    dirs = rng.standard_normal((P, 3))
    override = (cuda(ovr), dev(rng.standard_normal((P, L * F))), dev(dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)))
    out, saved = ops.field_fwd_train(fs, o, d, area, s, e, override=override)
    for name, g, w in zip(NAMES7, (*out, *saved), every_sample_a_ray(ops, fs, o, d, area, s, e, override)):
        err = rel_l2(host(g).reshape(-1), host(w).reshape(-1))
        assert g.numel() == w.numel() and err < 1e-5, (name, err)
    assert torch.equal(saved[0].reshape(M, -1)[cuda(where.astype(np.int64))], override[1][cuda(ovr[where].astype(np.int64))])
    plain = O.field_fwd(p, *(host(t) for t in (o, d, area, s, e)))["feature"].reshape(M, 32)
    free = ovr < 0  # the samples without an override row: the static scene's feature
    assert rel_l2(host(out[0]).reshape(M, 32)[free], plain[free]) < TIGHT
