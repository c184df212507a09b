"""Training on PACKED samples as one node (autograd.NffRenderTrainFn on autograd.PackedSamples / NeuRADField.render_train_packed /
VolumetricSampler.render_train): the fused field forward storing at the packed sample index
(nrhip_field_fwd_train_packed), head + packed compositing forward and backward (nrhip_sdf_render_packed_fwd / _bwd), and
the table gradient from packed samples (nrhip_encode_bwd_binned_packed).

References: the operator route the node replaces (ops.field_fwd_train on gathered [M,1] rays; field.forward with
fused_training = False + renderers.render_packed), the numpy oracle composited in float64, and a float64 torch restatement
of head + compositing with autograd (tests/packed_train_refs.py).  Bounds: 1e-5 fused vs operator forward, TIGHT / TOL for
the compositing kernel (test_composite_backward), 2e-5 / 2e-4 / 1e-3 for the node's outputs / parameter gradients / beta
(test_small_grid_render_train_vs_operator_path)."""
import numpy as np
import pytest
import torch

import packed_restatement as PR
import packed_train_refs as T
import synth
from conftest import rel_l2
from gpu_util import TIGHT, TOL, dev, host, host64, ray_bundle, to_spec
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NAMES7 = ("feature", "geo_out", "head", "save_enc", "save_geo_hidden", "save_feat_in", "save_feat_hidden")
M_RAGGED = sum(T.RAGGED)  # 745


def widths(L, F, H):
    return ((32,), (), (), (L * F,), (H,), (48,), (2 * H,))


def nan_buffers(M, L, F, H, pad=64):
    return [torch.full((M + pad, *w), float("nan"), device="cuda") for w in widths(L, F, H)]


def operator_forward(ops, fs, dr):
    """ops.field_fwd_train on the gathered [M,1] rays -> the seven tensors"""
    o, d, a, ts, te, _, ri = dr
    out, saved = ops.field_fwd_train(fs, o[ri], d[ri], a[ri], ts[:, None], te[:, None])
    return (*out, *saved)


# ---- 1. forward kernel, every fused shape ----------------------------------------------------------------------------
@pytest.mark.parametrize("L,F,H,use_sdf,half", T.RAGGED_CASES, ids=T.CASE_IDS)
def test_forward_kernel_every_fused_shape(ops, L, F, H, use_sdf, half):
    fs = to_spec(ops, T.params(L, F, H, use_sdf, half=half), half=half)
    dr = T.on_device(T.packed_rays(T.RAGGED, 7))
    o, d, a, ts, te, seg, _ = dr
    M = M_RAGGED
    want = operator_forward(ops, fs, dr)
    bufs = nan_buffers(M, L, F, H)
    out, saved = ops.field_fwd_train_packed(fs, o, d, a, ts, te, seg, out=bufs)
    got = (*out, *saved)
    bitwise = []
    for name, g, w in zip(NAMES7, got, want):
        assert g.shape[0] == M + 64
        assert bool(torch.isfinite(g[:M]).all()), f"{name}: a live row was not written"
        assert bool(torch.isnan(g[M:]).all()), f"{name}: a row past M was written"
        err = rel_l2(host(g[:M]).reshape(-1), host(w).reshape(-1))
        bitwise.append(torch.equal(g[:M].reshape(-1), w.reshape(-1)))
        print(f"{name}: rel-L2 vs operator forward {err:.3e}, bitwise {bitwise[-1]}")
        assert err < 1e-5, (name, err)
    print("all seven bitwise equal:", all(bitwise))
    order = dev(np.random.default_rng(23).permutation(len(T.RAGGED)).astype(np.int32), torch.int32)
    bufs2 = nan_buffers(M, L, F, H)
    ops.field_fwd_train_packed(fs, o, d, a, ts, te, seg, order=order, out=bufs2)
    for name, g, g2 in zip(NAMES7, bufs, bufs2):
        assert torch.equal(g[:M], g2[:M]), f"{name}: the processing order changed a bit"
        assert bool(torch.isnan(g2[M:]).all()), name


# ---- 2. a wave walks many rays ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,F,H,use_sdf", [(8, 4, 32, True), (16, 2, 64, False)], ids=["8x4-H32-sdf", "16x2-H64-density"])
def test_a_wave_walks_many_rays_in_any_order(ops, L, F, H, use_sdf):
    R = 9001
    counts = np.random.default_rng(17).integers(0, 41, R)
    assert (counts == 0).sum() >= 100 and (counts > 32).sum() >= 100
    dr = T.on_device(T.packed_rays(tuple(int(c) for c in counts), 19))
    o, d, a, ts, te, seg, _ = dr
    fs = to_spec(ops, T.params(L, F, H, use_sdf))
    out, saved = ops.field_fwd_train_packed(fs, o, d, a, ts, te, seg)
    got = (*out, *saved)
    for name, g, w in zip(NAMES7, got, operator_forward(ops, fs, dr)):
        err = rel_l2(host(g).reshape(-1), host(w).reshape(-1))
        print(f"{name}: rel-L2 vs operator forward {err:.3e}, bitwise {torch.equal(g.reshape(-1), w.reshape(-1))}")
        assert err < 1e-5, (name, err)
    order = dev(np.random.default_rng(23).permutation(R).astype(np.int32), torch.int32)
    out2, saved2 = ops.field_fwd_train_packed(fs, o, d, a, ts, te, seg, order=order)
    for name, g, g2 in zip(NAMES7, got, (*out2, *saved2)):
        assert torch.equal(g, g2), name


# ---- 3. head + compositing kernel alone --------------------------------------------------------------------------------
# inputs of the two heads.  SDF head: in the float64 restatement |d beta| = 0.43 x the sum of the absolute per-sample terms at
# this seed (0.06 - 0.15 at its neighbours), far above the 1e-2 the test asserts: the ratio measures the kernel
HEAD_SEED = {True: 44, False: 43}


def head_inputs(use_sdf, C=32):
    _, _, _, ts, te, seg = T.packed_rays(T.RAGGED, 7)
    M, R, seed = ts.shape[0], len(seg) - 1, HEAD_SEED[use_sdf]
    x = synth.normal((M,), seed) * np.float32(0.4 if use_sdf else 1.0) - np.float32(0.0 if use_sdf else 2.0)
    feat = synth.normal((M, C), seed + 1)
    cot = (synth.normal((R, C), seed + 2), synth.normal((R, 1), seed + 3), synth.normal((R, 1), seed + 4),
           synth.normal((M,), seed + 5))
    return ts, te, seg, x, feat, cot


def head_reference(use_sdf, beta_value=3.0, beta_min=1e-4):
    """float64 restatement + autograd -> forward values, (d x, d feat, d beta), and the per-sample terms of d beta"""
    ts, te, seg, x, feat, cot = head_inputs(use_sdf)
    x64, f64 = PR.f64(x, True), PR.f64(feat, True)
    beta = PR.f64(np.asarray([beta_value]), True) if use_sdf else None
    head, F_, D_, A_, W_ = T.head_composite_f64(x64, beta, beta_min, PR.f64(ts), PR.f64(te), f64, seg)
    head.retain_grad()
    gF, gD, gA, gW = (PR.f64(c) for c in cot)
    ((F_ * gF).sum() + (D_ * gD).sum() + (A_ * gA).sum() + (W_ * gW).sum()).backward()
    terms = None
    if use_sdf:  # d alpha_i / d beta = alpha_i (1 - alpha_i) (-x_i) sign(beta)
        a = head.detach()
        terms = (head.grad * a * (1 - a) * (-x64.detach())).numpy()
    fwd = [t.detach().numpy() for t in (head, W_, F_, D_, A_)]
    return fwd, (x64.grad.numpy(), f64.grad.numpy(), None if beta is None else beta.grad.numpy()), terms


@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
def test_head_and_compositing_kernel(ops, use_sdf):
    ts, te, seg, x, feat, cot = head_inputs(use_sdf)
    fwd_ref, (gx_ref, gf_ref, gb_ref), terms = head_reference(use_sdf)
    if use_sdf:  # otherwise the ratio below measures cancellation, not the kernel
        assert abs(terms.sum()) >= 1e-2 * np.abs(terms).sum(), (terms.sum(), np.abs(terms).sum())
        assert abs(terms.sum() - gb_ref[0]) <= 1e-9 * np.abs(terms).sum()
    beta_min = 1e-4
    beta = torch.tensor([3.0], device="cuda") if use_sdf else None
    d = [dev(v) for v in (x, feat, ts, te)] + [dev(seg, torch.int64)]
    xs, fs_, tsd, ted, segd = d
    gF, gD, gA, gW = (dev(c) for c in cot)
    fwd = ops.sdf_render_packed_fwd(xs, beta, beta_min, fs_, tsd, ted, segd)
    alpha, w, F_, D_, A_ = fwd
    M, R = x.shape[0], len(seg) - 1
    assert alpha.shape == (M,) and w.shape == (M,) and F_.shape == (R, 32) and D_.shape == (R, 1) and A_.shape == (R, 1)
    # (the density head's restatement returns sigma; the kernel saves alpha = 1 - exp(-sigma (t_end - t_start)))
    a_ref = fwd_ref[0] if use_sdf else -np.expm1(-fwd_ref[0] * (te.astype(np.float64) - ts.astype(np.float64)))
    for name, g, r in zip(("alpha", "weights", "features", "depth", "accumulation"), fwd, [a_ref] + fwd_ref[1:]):
        err = rel_l2(host64(g).reshape(-1), r.reshape(-1))
        print(f"{name}: rel-L2 {err:.3e}")
        assert err < TIGHT, (name, err)
    empty = torch.from_numpy(np.diff(seg) == 0).cuda()
    for t in (F_, D_, A_):
        assert bool((t[empty] == 0).all())
    bwd = ops.sdf_render_packed_bwd(xs, beta, beta_min, alpha, fs_, tsd, ted, segd, gF, gD, gA, gW)
    gf, gx, gb = bwd
    e_x, e_f = rel_l2(host64(gx), gx_ref), rel_l2(host64(gf).reshape(-1), gf_ref.reshape(-1))
    print(f"grad_geo_out: rel-L2 {e_x:.3e}   grad_features: rel-L2 {e_f:.3e}")
    assert e_x < TOL and e_f < TIGHT
    if use_sdf:
        ratio = float(gb[0]) / float(gb_ref[0])
        print(f"grad_beta: {float(gb[0]):.6e} vs {float(gb_ref[0]):.6e}, ratio - 1 = {ratio - 1:.3e}")
        assert abs(ratio - 1) < 1e-3
        # a negative raw parameter: the same |beta|, the sign on d beta alone
        nb = ops.sdf_render_packed_bwd(xs, -beta, beta_min, alpha, fs_, tsd, ted, segd, gF, gD, gA, gW)
        assert torch.equal(nb[0], gf) and torch.equal(nb[1], gx) and torch.equal(nb[2], -gb)
    else:
        assert gb is None
    # two runs: the same bits, grad_beta included
    again = ops.sdf_render_packed_fwd(xs, beta, beta_min, fs_, tsd, ted, segd)
    again_b = ops.sdf_render_packed_bwd(xs, beta, beta_min, alpha, fs_, tsd, ted, segd, gF, gD, gA, gW)
    for a_, b_ in zip((*fwd, *bwd), (*again, *again_b)):
        assert (a_ is None and b_ is None) or torch.equal(a_, b_)
    # unused outputs send no gradient: NULL upstreams equal zero tensors
    zero = ops.sdf_render_packed_bwd(xs, beta, beta_min, alpha, fs_, tsd, ted, segd, gF, torch.zeros_like(gD),
                                     torch.zeros_like(gA), torch.zeros_like(gW))
    null = ops.sdf_render_packed_bwd(xs, beta, beta_min, alpha, fs_, tsd, ted, segd, gF, None, None, None)
    for a_, b_ in zip(zero, null):
        assert (a_ is None and b_ is None) or torch.equal(a_, b_)
    zero = ops.sdf_render_packed_bwd(xs, beta, beta_min, alpha, fs_, tsd, ted, segd, torch.zeros_like(gF), gD, gA, gW)
    null = ops.sdf_render_packed_bwd(xs, beta, beta_min, alpha, fs_, tsd, ted, segd, None, gD, gA, gW)
    for a_, b_ in zip(zero, null):
        assert (a_ is None and b_ is None) or torch.equal(a_, b_)
    # extremes, finiteness only: geo_out = +-80 (density head), sdf * beta = +-200 (SDF head)
    big = torch.where(torch.arange(M, device="cuda") % 3 == 0, 1.0, -1.0) * (200.0 / 3.0 if use_sdf else 80.0)
    big[::7] = xs[::7]
    f2 = ops.sdf_render_packed_fwd(big, beta, beta_min, fs_, tsd, ted, segd)
    b2 = ops.sdf_render_packed_bwd(big, beta, beta_min, f2[0], fs_, tsd, ted, segd, gF, gD, gA, gW)
    for t in (*f2, *b2):
        assert t is None or bool(torch.isfinite(t).all())


# ---- 4. whole node vs the operator route -----------------------------------------------------------------------------
def cotangents(R, M, seed=81):
    return (dev(synth.normal((R, 32), seed)), dev(synth.normal((R, 1), seed + 1)), dev(synth.normal((R, 1), seed + 2)),
            dev(synth.normal((M,), seed + 3)))


def run_route(fld, dr, fused, cot):
    """-> (features, depth, accumulation, weights), parameter gradients"""
    o, d, a, ts, te, seg, ri = dr
    if fused:
        outs = fld.render_train_packed(o, d, a, ts, te, segments=seg)
    else:
        outs = T.operator_route(fld, dr)
    sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot)).backward()
    return [t.detach() for t in outs], T.field_grads(fld)


def compare_routes(fused, operator, half=False):
    (fo, fg), (oo, og) = fused, operator
    for name, a, b in zip(("features", "depth", "accumulation", "weights"), fo, oo):
        err = rel_l2(host64(a).reshape(-1), host64(b).reshape(-1))
        print(f"{name}: fused vs operator rel-L2 {err:.3e}")
        assert err < 2e-5, (name, err)
    assert set(fg) == set(og), set(fg) ^ set(og)
    for n in fg:  # (beta's gradient sums every sample's heavily cancelling terms)
        bound = 1e-3 if n == "sdf_to_density.beta" else 2e-4
        err = rel_l2(host64(fg[n].float()).reshape(-1), host64(og[n].float()).reshape(-1))
        print(f"d {n}: fused vs operator rel-L2 {err:.3e} (bound {bound:g})")
        assert fg[n].dtype == og[n].dtype and err < bound, (n, err)
    if half:
        assert fg["hashgrid.static_grid.hash_table"].dtype == torch.float16


NODE_CASES = [(8, 4, 32, True, False), (16, 2, 64, False, False), (4, 2, 32, True, False), (8, 4, 32, True, True)]
NODE_IDS = ["8x4-H32-sdf", "16x2-H64-density", "4x2-H32-sdf", "8x4-H32-sdf-fp16"]


@pytest.mark.parametrize("L,F,H,use_sdf,half", NODE_CASES, ids=NODE_IDS)
def test_node_vs_operator_route_small_batch(ops, L, F, H, use_sdf, half):
    rays = T.packed_rays(T.RAGGED, 7)
    dr = T.on_device(rays)
    cot = cotangents(len(T.RAGGED), M_RAGGED)
    assert M_RAGGED < ops._BINNED_MIN_SAMPLES  # the small-batch table-gradient route
    res = {}
    for fused in (True, False):
        fld, p = T.make_field(L, F, H, use_sdf, half)
        assert fld.fused_packed_train_supported()
        res[fused] = run_route(fld, dr, fused, cot)
    compare_routes(res[True], res[False], half)
    assert ("sdf_to_density.beta" in res[True][1]) == use_sdf
    for name, got, want in zip(("features", "depth", "accumulation", "weights"), res[True][0], T.oracle_route(p, rays)):
        err = rel_l2(host64(got).reshape(-1), want.reshape(-1))
        print(f"{name}: fused vs oracle rel-L2 {err:.3e}")
        assert err < TOL, (name, err)


def large_rays():
    counts = np.random.default_rng(29).integers(0, 61, 1500)
    return T.packed_rays(tuple(int(c) for c in counts), 31)


@pytest.mark.parametrize("L,F,H,use_sdf,half", NODE_CASES[:2], ids=NODE_IDS[:2])
def test_node_vs_operator_route_partition_source(ops, L, F, H, use_sdf, half):
    rays = large_rays()
    dr = T.on_device(rays)
    M = rays[3].shape[0]
    assert M >= ops._BINNED_MIN_SAMPLES == 1 << 15  # the packed partition source computes the table gradient
    cot = cotangents(1500, M)
    res = {}
    for key, fused in (("fused", True), ("operator", False), ("again", True)):
        fld, _ = T.make_field(L, F, H, use_sdf, half)
        res[key] = run_route(fld, dr, fused, cot)
    compare_routes(res["fused"], res["operator"])
    name = "hashgrid.static_grid.hash_table"
    assert torch.equal(res["fused"][1][name], res["again"][1][name])
    for a, b in zip(res["fused"][0], res["again"][0]):
        assert torch.equal(a, b)


def test_node_without_samples(ops):
    dr = T.on_device(T.packed_rays((0,) * 7, 3))
    fld, _ = T.make_field(8, 4, 32, True)
    outs = fld.render_train_packed(*dr[:5], segments=dr[5])
    assert [tuple(t.shape) for t in outs] == [(7, 32), (7, 1), (7, 1), (0,)]
    assert all(bool((t == 0).all()) for t in outs)
    sum(t.sum() for t in outs).backward()
    for n, p in fld.named_parameters():
        assert p.grad is None or bool((p.grad == 0).all()), n
    ri = fld.render_train_packed(*dr[:5], ray_indices=dr[6], num_rays=7)
    assert ri[0].shape == (7, 32) and ri[3].shape == (0,)


# ---- 5. VolumetricSampler.render_train ---------------------------------------------------------------------------------
@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
def test_volumetric_sampler_render_train(ops, use_sdf, monkeypatch):
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    R = 96
    est = OccGridEstimator([-5, -5, -5, 5, 5, 5], resolution=16)
    est.binaries[0] = dev(np.random.default_rng(3).random((16, 16, 16)) < 0.3)
    rb = ray_bundle(R, 90, far=9.0)
    sampler = VolumetricSampler(est).train()
    kw = dict(render_step_size=0.1, cone_angle=0.0)
    keys = {"features", "depth", "accumulation", "weights", "ray_indices", "t_starts", "t_ends"}

    def refuse(*a, **k):
        raise AssertionError("the wrong route ran")

    fld, _ = T.make_field(8, 4, 32, use_sdf)
    with monkeypatch.context() as m:  # the fused route reads the bundle's own tensors: no gather of the ray constants
        m.setattr(VolumetricSampler, "_gather", staticmethod(refuse))
        got = sampler.render_train(fld, rb, **kw)
    assert set(got) == keys
    ri, ts, te = got["ray_indices"], got["t_starts"], got["t_ends"]
    M = ri.shape[0]
    counts = torch.bincount(ri, minlength=R)
    assert M > 1000 and int((counts == 0).sum()) >= 4 and got["weights"].shape == (M, 1)
    cot = cotangents(R, M, 91)
    outs = [got[k] for k in ("features", "depth", "accumulation", "weights")]
    sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot)).backward()
    fused = ([t.detach().reshape(c.shape) for t, c in zip(outs, cot)], T.field_grads(fld))
    # the operator route fed the RETURNED samples: the stratified draw is shared
    fld2, _ = T.make_field(8, 4, 32, use_sdf)
    dr = (rb.origins, rb.directions, rb.pixel_area.reshape(-1), ts, te, None, ri)
    op_outs = T.operator_route(fld2, dr)
    sum((t.reshape(c.shape) * c).sum() for t, c in zip(op_outs, cot)).backward()
    compare_routes(fused, ([t.detach() for t in op_outs], T.field_grads(fld2)))

    def finite_grads(f_):
        grads = T.field_grads(f_)
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads.values())

    # a field outside the gate: the same keys and finite gradients through the fallback
    cfg = NeuRADFieldConfig(use_sdf=use_sdf)
    cfg.grid.static.log2_hashmap_size, cfg.grid.static.num_levels = T.LG, 3
    torch.manual_seed(4)
    odd = NeuRADField(cfg, actors=None, static_scale=100.0).cuda()
    assert not odd.fused_packed_train_supported()
    fb = sampler.render_train(odd, rb, **kw)
    assert set(fb) == keys and fb["features"].shape == (R, 32) and fb["weights"].shape == (fb["ray_indices"].shape[0], 1)
    (fb["features"].sum() + fb["depth"].sum() + fb["accumulation"].sum() + fb["weights"].sum()).backward()
    finite_grads(odd)
    # rays that require grad, and fused_training = False: the fallback
    for mode in ("ray_grad", "operator"):
        f3, _ = T.make_field(8, 4, 32, use_sdf)
        rb3 = ray_bundle(R, 90, far=9.0)
        if mode == "ray_grad":
            rb3.origins.requires_grad_(True)
        else:
            f3.fused_training = False
        with monkeypatch.context() as m:
            m.setattr(f3, "render_train_packed", refuse)
            out3 = sampler.render_train(f3, rb3, **kw)
        assert set(out3) == keys
        (out3["features"].sum() + out3["depth"].sum()).backward()
        finite_grads(f3)
        if mode == "ray_grad":
            assert rb3.origins.grad is not None and bool(torch.isfinite(rb3.origins.grad).all())
            assert float(rb3.origins.grad.abs().sum()) > 0
    with pytest.raises(RuntimeError, match="eval"):
        sampler.render(fld, rb, **kw)


# ---- 6. graph replay ---------------------------------------------------------------------------------------------------
def test_node_forward_and_backward_replay_in_a_graph(ops):
    rays = large_rays()  # (the partition source: the small batch's table gradient is formed by memory-side atomics)
    dr = T.on_device(rays)
    M = rays[3].shape[0]
    cot = cotangents(1500, M)
    fld, _ = T.make_field(8, 4, 32, True)
    ps = [p for p in fld.parameters() if p.requires_grad]

    def step():
        outs = fld.render_train_packed(*dr[:5], segments=dr[5])
        loss = sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot))
        grads = torch.autograd.grad(loss, ps, allow_unused=True)
        return [*outs, *[g for g in grads if g is not None]]

    eager = [t.detach().clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert len(captured) == len(eager)
        for a, b in zip(eager, captured):
            assert torch.equal(a, b.detach())


# ---- 7. the table gradient's two ray-sample sources ------------------------------------------------------------------------
def source_batch():
    """48 rays of 0 .. 40 samples, the first, the last and two more empty; with the contraction at 20 m the samples (out to
    60 m from origins ~N(0, 5 m)) lie on both sides of it"""
    counts = np.random.default_rng(41).integers(1, 41, 48)
    counts[[0, 9, 30, 47]] = 0
    counts[[3, 21]] = 40, 1
    return T.packed_rays(tuple(int(c) for c in counts), 37)


@pytest.mark.parametrize("F", [2, 4])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_packed_source_equals_the_dense_source_on_one_sample_rays(ops, monkeypatch, F, out_dtype):
    """ops.encode_bwd_packed against ops.encode_bwd on the same samples as [M,1] rays (ray constants gathered by
    ray_indices).  Both run the partition over the same sample order with the ray-major walk (S = 1 < 16 on the dense side,
    the packed source never transposes), the same positions and the same gradient rows: the same bits."""
    L, lg, scale = 2, 8, 20.0
    rays = source_batch()
    o, d, a, ts, te, seg, ri = T.on_device(rays)
    counts = np.diff(rays[5])
    M = int(counts.sum())
    assert len(counts) == 48 and counts.max() == 40 and counts[0] == 0 and counts[-1] == 0 and (counts == 0).sum() >= 3
    mid = rays[0][host(ri)] + rays[1][host(ri)] * ((rays[3] + rays[4]) / 2)[:, None]
    mag = np.abs(mid / scale).max(-1)
    assert (mag < 1).sum() > 100 and (mag >= 1).sum() > 100
    spec = ops.GridSpec(L, F, lg, 16, 1024)
    g = synth.normal((M, L * F), 61)
    g[::9] = 0.0  # silent samples: dropped by `prep` on both sides
    g = dev(g)
    monkeypatch.setattr(ops, "_BINNED_MIN_SAMPLES", 1)
    assert ops._table_grad_workspace(spec.c_grid(out_dtype), M, g.device) is not None  # the partition, not the atomics
    packed = ops.encode_bwd_packed(spec, scale, o, d, a, ts, te, ri, g, out_dtype=out_dtype)
    dense = ops.encode_bwd(spec, scale, o[ri], d[ri], a[ri], ts[:, None], te[:, None], g, out_dtype=out_dtype)
    assert packed.dtype == dense.dtype == out_dtype and packed.shape == (L << lg, F)
    diff = (packed.double() - dense.double()).abs()
    print(f"F={F} {out_dtype}: M={M}, non-zero entries {int((dense != 0).sum())}, max |packed - dense| {float(diff.max()):.3e}, "
          f"bitwise {torch.equal(packed, dense)}")
    assert float(dense.float().abs().max()) > 0
    assert torch.equal(packed, dense)
