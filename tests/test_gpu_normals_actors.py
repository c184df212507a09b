"""Surface normals in a scene with dynamic actors on the device (csrc/normals.hip: nrhip_field_normals_actors / _packed_actors;
the contract and the bound: include/neurad_hip.h) against the numpy restatement of tests/normals_actor_refs.py, which
tests/test_normals_actor_refs_host.py pins to the reference's own autograd.  The restatement is fed the DEVICE's in-box primal
(hit, box_position, the winner's cand_w2b row): per element |g_gpu - g| <= 2^-24 |g| + (c + 1) 2^-24 A with
c = NRHIP_NORMALS_ACTORS_C(La, F, H) inside a box and NRHIP_NORMALS_C(L, F, H) outside.  A sample whose ReLU mask or whose box
test is decided within rounding is left out of the element-wise comparison (at most 1 % of a case) and must still be finite."""
import functools

import numpy as np
import pytest
import torch

import builders
import normals_actor_refs as AR
import normals_refs as NR
import packed_actor_refs as PA
from conftest import load_golden
from gpu_util import actor_rays, cuda, dev, host, host64, make_actor_field, ops, to_spec  # noqa: F401

pytestmark = pytest.mark.gpu
ALL = ("geo", "gradient", "normals")
PRIMAL = ("hit", "box_position")


def to_actor_spec(ops, ap, half=False):
    g = ap.grids[0]
    spec = ops.GridSpec(g.num_levels, g.n_feat, g.log2_hashmap_size, g.min_res, g.max_res)
    return ops.ActorSpec(dev(ap.timestamps), dev(ap.positions), dev(ap.rotations_6d), cuda(ap.present), dev(ap.bounds), spec,
                         [dev(t.table, torch.float16 if half else torch.float32) for t in ap.grids], ap.actor_scale)


def rays_dev(rays):
    return tuple(dev(a) for a in rays[:5])


@functools.lru_cache(maxsize=None)
def near_face(edit=False):
    """the samples of the scene within rounding of a box face (from the oracle; the edit moves the boxes)"""
    sc = AR.scene()
    ap = AR.actor_params(8, 4)
    _, mean, w2b, valid = AR.containment(ap, *AR.scene_rays(sc), sc["times"], AR.EDIT if edit else None)
    return AR.near_a_face(ap, mean, w2b, valid)


def device_primal(out, cand, S):
    """the kernel's own in-box primal as arrays: hit [N], box_position [N,3] and the winner's fp32 world2box row [N,3,4]"""
    hit, bp = host(out["hit"]).reshape(-1), host(out["box_position"]).reshape(-1, 3)
    cnt, act, w2b = host(cand[0]), host(cand[1]), host(cand[2])
    rows = np.zeros((hit.shape[0], 3, 4), np.float32)
    for n in np.nonzero(hit >= 0)[0]:
        ray = n // S
        (c,) = np.nonzero(act[ray, :cnt[ray]] == hit[n])[0]
        rows[n] = w2b[ray, c].reshape(3, 4)
    return hit, np.where((hit >= 0)[:, None], bp, 0).astype(np.float32), rows


def constants(p, ap, hit):
    """[N,1]: the bound's constant per sample"""
    return np.where(hit >= 0, AR.constant(p, ap), NR.constant(p))[:, None].astype(np.float64)


def check(out, r, c, left_out, rows=None, factor=1, what=""):
    sel = slice(None) if rows is None else rows
    keep = ~left_out[sel]
    assert (~keep).mean() <= NR.LEFT_OUT_CAP
    g, A, c = r["g"][sel], r["A"][sel], c[sel]
    if "gradient" in out:
        got = host64(out["gradient"]).reshape(-1, 3)
        assert np.isfinite(got).all()
        ex = (np.abs(got - g) - NR.U * np.abs(g)) / (NR.U * np.maximum(A, 1e-300))
        inbox = (r["hit"][sel] >= 0) & keep
        print(f"{what} gradient: max excess {ex[inbox].max() if inbox.any() else 0:.2f} (in a box, c = {c.max():.0f}), "
              f"{ex[keep & ~inbox].max() if (keep & ~inbox).any() else 0:.2f} (outside, c = {c.min():.0f}) units of 2^-24 A")
        assert (np.abs(got - g) <= factor * NR.bound(g, A, c))[keep].all()
    if "normals" in out:
        got = host64(out["normals"]).reshape(-1, 3)
        assert np.isfinite(got).all()
        assert (np.abs(got - r["normals"][sel]) <= factor * NR.normal_tolerance(g, A, c))[keep].all()
        assert np.abs(np.linalg.norm(got, axis=-1) - 1).max() < 1e-6
    if "geo" in out:
        got = host64(out["geo"]).reshape(-1)
        assert np.isfinite(got).all()
        assert (np.abs(got - r["geo"][sel]) <= factor * NR.bound(r["geo"][sel], r["A_geo"][sel], c[:, 0]))[keep].all()


def run_case(ops, name, flip=None, want=ALL + PRIMAL, **kw):
    """the scene through the fused kernel -> (out, restatement on the device's primal, constants, left_out, pieces)"""
    L, F, H, use_sdf, half = AR.CASES[name]
    p, ap = AR.case_params(name)
    sc = AR.scene()
    rays = AR.scene_rays(sc)
    fs, aspec = to_spec(ops, p, half), to_actor_spec(ops, ap, half)
    rd = rays_dev(rays)
    cand = ops.actor_prepare(aspec, *rd, dev(sc["times"]))
    out = ops.field_normals(fs, *rd, want=want, actors=(aspec, cand), ray_flip=None if flip is None else dev(flip), **kw)
    hit, bp, rows = device_primal(out, cand, AR.S)
    r = AR.restatement(p, ap, *rays, hit, bp, rows, flip)
    r["hit"] = hit
    return out, r, constants(p, ap, hit), r["left_out"] | near_face(), dict(p=p, ap=ap, fs=fs, aspec=aspec, cand=cand, rd=rd)


# ---- 1. the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AR.CASES))
def test_kernel_against_the_restatement(ops, name):
    out, r, c, left_out, _ = run_case(ops, name)
    assert out["geo"].shape == (AR.R, AR.S) and out["gradient"].shape == (AR.R, AR.S, 3) and out["hit"].dtype == torch.int32
    assert (r["hit"] >= 0).mean() >= 0.15
    check(out, r, c, left_out, what=name)
    if not AR.CASES[name][3]:  # the density head's sign: against the gradient
        assert (host64(out["normals"]) * host64(out["gradient"])).sum(-1).max() < 0


# ---- 2. hit and box position -------------------------------------------------------------------------------------------
def test_hit_is_actor_encodes_and_the_box_position_is_the_oracles(ops):
    out, r, c, left_out, k = run_case(ops, "8x4_h32_sdf")
    feats = torch.zeros((AR.R * AR.S, 32), device="cuda")
    _, hit = ops.actor_encode(k["aspec"], k["cand"], *k["rd"], feats)
    assert torch.equal(out["hit"].reshape(-1), hit)
    # the encoding row of an in-box sample is the row actor_encode writes: the geometry MLP on the spliced rows gives geo within
    # the bound the header states for geo against the matrix-core products, 2 (L F + H + 2) 2^-24 A_geo
    fs = k["fs"]
    enc = ops.encode_fwd(fs.grid, fs.table, fs.static_scale, *k["rd"])
    ops.actor_encode(k["aspec"], k["cand"], *k["rd"], enc)
    y = host64(ops.mlp_fwd(enc, fs.geo_w, fs.geo_b)[:, 0])
    assert (np.abs(host64(out["geo"]).reshape(-1) - y) <= 2 * (32 + 32 + 2) * NR.U * r["A_geo"]).all()
    sc = AR.scene()
    rays = AR.scene_rays(sc)
    o_hit, o_pos, o_rows, n_boxes = AR.oracle_primal(k["ap"], *rays, sc["times"])
    safe = ~near_face()
    assert np.array_equal(r["hit"][safe], o_hit[safe])
    assert (r["hit"][safe & (n_boxes >= 2)] == 2).all() and (safe & (n_boxes >= 2)).sum() >= 50  # the highest index wins
    inbox = safe & (o_hit >= 0)
    hitd, bp, rows = device_primal(out, k["cand"], AR.S)
    # (a) the 3 x 4 product: three products and three sums, each rounded once (fewer where fused): <= 4 u of the terms
    mean, _ = NR.O.fast_isotropic_gaussian(*rays)
    x = mean.reshape(-1, 3).astype(np.float64)
    W = rows.astype(np.float64)
    exact = (W[:, :, :3] * x[:, None, :]).sum(-1) + W[:, :, 3]
    terms = (np.abs(W[:, :, :3]) * np.abs(x[:, None, :])).sum(-1) + np.abs(W[:, :, 3])
    assert (np.abs(bp - exact) <= 4 * NR.U * terms)[inbox].all()
    # (b) the device's world2box row against the oracle's: both round the same ~30 fp32 operations of the pose chain
    # (two normalisations, the lerp, Gram-Schmidt, the cross product, -R^T t with |t| up to 30 m) in their own order
    tol = 64 * NR.U * np.concatenate([np.ones((1, 3, 3)), np.full((1, 3, 1), 64.0)], -1)
    assert (np.abs(rows - o_rows) <= tol)[inbox].all()
    assert (np.abs(bp - o_pos) <= 4 * NR.U * terms + (tol[..., :3] * np.abs(x[:, None, :])).sum(-1) + tol[..., 3])[inbox].all()
    # box_position is left untouched where hit < 0: the entry point itself on a pre-filled buffer
    N = AR.R * AR.S
    f_, keep_f = k["fs"].c_field()
    a_, keep_a = k["aspec"].c_actors()
    r_, keep_r = ops._c_rays(*k["rd"], None)
    cnt, act, w2b = k["cand"][:3]
    buf = torch.full((N, 3), 7.0, device="cuda")
    hit2 = torch.full((N,), -9, dtype=torch.int32, device="cuda")
    ops.launch("nrhip_field_normals_actors", f_, a_, r_, cnt, act, w2b, None, None, 0, None, None, None, None, hit2, buf)
    assert torch.equal(hit2, hit)
    assert (buf[hit2 < 0] == 7.0).all() and (hit2 < 0).any()
    assert torch.equal(buf[hit2 >= 0], out["box_position"].reshape(-1, 3)[hit2 >= 0])


# ---- 3. samples outside every box --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["8x4_h32_sdf", "16x2_h64_sdf", "8x4_h32_fp16"])
def test_outside_every_box_the_static_kernels_bits(ops, name):
    out, r, c, left_out, k = run_case(ops, name)
    static = ops.field_normals(k["fs"], *k["rd"], want=ALL)
    outside = out["hit"] < 0
    assert outside.any() and (~outside).any()
    for key in ALL:
        assert torch.equal(out[key][outside], static[key][outside]), key
        assert not torch.equal(out[key][~outside], static[key][~outside]), key
    # a batch in which no ray has a candidate: every output, ray_normals included, is the static kernel's
    w = dev(np.random.default_rng(4).random((AR.R, AR.S)).astype(np.float32))
    none = (torch.zeros_like(k["cand"][0]), k["cand"][1], k["cand"][2], None)
    a = ops.field_normals(k["fs"], *k["rd"], weights=w, want=ALL + ("ray_normals", "hit"), actors=(k["aspec"], none))
    b = ops.field_normals(k["fs"], *k["rd"], weights=w, want=ALL + ("ray_normals",))
    assert (a["hit"] == -1).all()
    for key in ALL + ("ray_normals",):
        assert torch.equal(a[key], b[key]), key


# ---- 4. flip and edit --------------------------------------------------------------------------------------------------
def test_explicit_ray_flip(ops):
    flip = AR.ray_flips()
    out, r, c, left_out, k = run_case(ops, "8x4_h32_sdf", flip=flip)
    check(out, r, c, left_out, what="flip")
    base = ops.field_normals(k["fs"], *k["rd"], want=PRIMAL + ("gradient",), actors=(k["aspec"], k["cand"]))
    f = dev(flip)[:, None]
    inbox = out["hit"] >= 0
    assert torch.equal(out["hit"], base["hit"])
    assert torch.equal(out["box_position"][inbox][:, 0], (base["box_position"][..., 0] * f)[inbox])
    assert torch.equal(out["box_position"][inbox][:, 1:], base["box_position"][inbox][:, 1:])
    same = (out["gradient"] == base["gradient"]).all(-1)
    assert same[~inbox].all() and same[inbox & (f > 0)].all() and not same[inbox & (f < 0)].any()


def test_eval_time_edit_through_the_field(ops):
    fld, p, ap = PA.make_actor_field("golden", 8, 4, 32)
    sc = AR.scene()
    rays = AR.scene_rays(sc)
    rd, times = rays_dev(rays), dev(sc["times"])
    hg = fld.hashgrid
    with torch.no_grad():
        base = fld.normals(*rd, times=times, want=("hit",))
        hg.actors.actor_editing = dict(AR.EDIT)
        assert hg.actor_edit() is not None
        out = fld.normals(*rd, times=times, want=ALL + PRIMAL)
        cand = hg.prepare_actors(*rd, times)[1]
    assert (out["hit"] != base["hit"]).sum() >= 5  # the boxes moved
    hit, bp, rows = device_primal(out, cand, AR.S)
    r = AR.restatement(p, ap, *rays, hit, bp, rows)
    r["hit"] = hit
    check(out, r, constants(p, ap, hit), r["left_out"] | near_face(edit=True), what="edit")
    o_hit = AR.oracle_primal(ap, *rays, sc["times"], edit=AR.EDIT)[0]
    safe = ~near_face(edit=True)
    assert np.array_equal(hit[safe], o_hit[safe])


# ---- 5. small and reordered --------------------------------------------------------------------------------------------
def test_one_sample_bin_edges_in_place_and_a_permuted_order(ops):
    out, r, c, left_out, k = run_case(ops, "8x4_h32_sdf")
    o, d, a, s, e = k["rd"]
    act = (k["aspec"], k["cand"])
    edges = dev(AR.scene()["edges"])
    assert edges[:, :-1].stride(0) == AR.S + 1
    view = ops.field_normals(k["fs"], o, d, a, edges[:, :-1], edges[:, 1:], want=ALL + PRIMAL, actors=act)
    order = torch.randperm(AR.R, generator=torch.Generator().manual_seed(1)).to("cuda", torch.int32)
    perm = ops.field_normals(k["fs"], o, d, a, s, e, want=ALL + PRIMAL, order=order, actors=act)
    inbox = out["hit"] >= 0
    for key in ALL + ("hit",):
        assert torch.equal(view[key], out[key]) and torch.equal(perm[key], out[key]), key
    assert torch.equal(view["box_position"][inbox], out["box_position"][inbox])
    assert torch.equal(perm["box_position"][inbox], out["box_position"][inbox])
    col = int(inbox.sum(0).argmax())  # S = 1: one column of the batch, the one with most samples in a box
    assert inbox[:, col].sum() >= 5
    one = ops.field_normals(k["fs"], o, d, a, s[:, col:col + 1].contiguous(), e[:, col:col + 1].contiguous(), want=ALL + PRIMAL,
                            actors=act)
    for key in ALL + ("hit",):
        assert torch.equal(one[key][:, 0], out[key][:, col]), key


# ---- 6. packed -----------------------------------------------------------------------------------------------------------
def packed_batch(rays, counts):
    """the first counts[r] samples of every ray, packed -> (t_starts, t_ends, segments, rows of the dense [R,S] batch)"""
    S = rays[3].shape[1]
    rows = np.concatenate([np.arange(c) + k * S for k, c in enumerate(counts)]).astype(np.int64)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return dev(rays[3].reshape(-1)[rows]), dev(rays[4].reshape(-1)[rows]), cuda(seg), rows


@functools.lru_cache(maxsize=None)
def ragged():
    """six rays of the scene that cross the boxes, 80 bins each up to 10 m, and the segment lengths 0, 1, 80, 17, 64, 5"""
    sc = AR.scene()
    pick = np.array([1, 2, 5, 6, 7, 9])  # (none of every fourth: those look away)
    _, eu, _ = NR.O.power_sampler(np.zeros(6), np.full(6, AR.FAR, np.float32), 80)
    rays = (sc["o"][pick], sc["d"][pick], sc["area"][pick], np.ascontiguousarray(eu[:, :-1]), np.ascontiguousarray(eu[:, 1:]))
    return rays, sc["times"][pick], np.array([0, 1, 80, 17, 64, 5])


def test_packed_samples(ops):
    rays, times, counts = ragged()
    p, ap = AR.case_params("8x4_h32_sdf")
    fs, aspec = to_spec(ops, p), to_actor_spec(ops, ap)
    o, d, a, s, e = rays_dev(rays)
    ts, te, seg, rows = packed_batch(rays, counts)
    M = rows.shape[0]
    cand_line = ops.actor_prepare_line(aspec, o, d, 0.0, 1.0, dev(times))
    cand = ops.actor_prepare(aspec, o, d, a, s, e, dev(times))
    w = np.random.default_rng(9).random(M).astype(np.float32)
    w[::5] = 0
    out = ops.field_normals_packed(fs, o, d, a, ts, te, seg, weights=dev(w), want=ALL + PRIMAL + ("ray_normals",),
                                   actors=(aspec, cand_line))
    assert out["geo"].shape == (M,) and out["gradient"].shape == (M, 3) and out["hit"].shape == (M,)
    dense = ops.field_normals(fs, o, d, a, s, e, want=ALL + PRIMAL, actors=(aspec, cand))
    inbox = out["hit"] >= 0
    assert inbox.sum() >= 30 and (~inbox).sum() >= 30
    idx = cuda(rows)
    for k in ALL + ("hit",):  # per-sample outputs: the dense call's bits on the same samples
        assert torch.equal(out[k], dense[k].reshape(80 * 6, *dense[k].shape[2:])[idx]), k
    assert torch.equal(out["box_position"][inbox], dense["box_position"].reshape(-1, 3)[idx][inbox])
    # ... and the dense call against the restatement on all 6 x 80 samples
    hit, bp, wrows = device_primal(dense, cand, 80)
    r = AR.restatement(p, ap, *rays, hit, bp, wrows)
    r["hit"] = hit
    _, mean, w2b, valid = AR.containment(ap, *rays, times)
    check(dense, r, constants(p, ap, hit), r["left_out"] | AR.near_a_face(ap, mean, w2b, valid), what="ragged")
    # per ray: the kernel's own order bit for bit, and the exactly rounded sum within the roundings
    row, nh = host(out["ray_normals"]), host(out["normals"])
    G = NR.lanes_per_ray(-(-M // len(counts)))
    segs = np.concatenate([[0], np.cumsum(counts)])
    for k in range(len(counts)):
        wk, nk = w[segs[k]:segs[k + 1]], nh[segs[k]:segs[k + 1]]
        assert np.array_equal(row[k], NR.ray_sum_sequential(wk, nk, G)), k
        exact, mag = NR.ray_sum_exact(wk, nk)
        assert (np.abs(row[k] - exact) <= (counts[k] + 8) * NR.U * mag).all()
    assert (row[0] == 0).all()  # the empty segment
    # samples of weight zero are skipped: NaN intervals there leave every row as it was
    ts2, te2 = ts.clone(), te.clone()
    ts2[dev(w) == 0] = float("nan")
    te2[dev(w) == 0] = float("nan")
    nan = ops.field_normals_packed(fs, o, d, a, ts2, te2, seg, weights=dev(w), want=("ray_normals",), actors=(aspec, cand_line))
    assert torch.equal(nan["ray_normals"], out["ray_normals"])
    # no samples at all: rows of zeros
    none = torch.empty(0, device="cuda")
    out0 = ops.field_normals_packed(fs, o, d, a, none, none, torch.zeros(7, dtype=torch.int64, device="cuda"), weights=none,
                                    want=("hit", "ray_normals"), actors=(aspec, cand_line))
    assert out0["hit"].shape == (0,) and not out0["ray_normals"].any()


# ---- 7. the operator composition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["8x4_h32_sdf", "4x2_h64_density"])
def test_operator_composition_agrees_within_twice_the_bound(ops, name):
    out, r, c, left_out, k = run_case(ops, name)
    sc = AR.scene()
    oper = ops.field_normals_operators(k["fs"], *k["rd"], want=ALL + ("hit",), actors=(k["aspec"], k["cand"]),
                                       times=dev(sc["times"]))
    assert torch.equal(oper["hit"], out["hit"])
    keep = ~left_out
    dg = np.abs(host64(oper["gradient"]) - host64(out["gradient"])).reshape(-1, 3)
    ex = dg / (NR.U * np.maximum(r["A"], 1e-300))
    print(f"{name}: operators vs fused, largest difference {ex[keep].max():.2f} units of 2^-24 A")
    assert (dg <= 2 * NR.bound(r["g"], r["A"], c))[keep].all()
    dn = np.abs(host64(oper["normals"]) - host64(out["normals"])).reshape(-1, 3)
    assert (dn <= 2 * NR.normal_tolerance(r["g"], r["A"], c))[keep].all()
    dgeo = np.abs(host64(oper["geo"]) - host64(out["geo"])).reshape(-1)
    assert (dgeo <= 2 * NR.bound(r["geo"], r["A_geo"], c[:, 0]))[keep].all()
    check(oper, r, c, left_out, factor=2, what=f"{name} operators")


def test_actor_field_without_a_fused_shape_takes_the_operator_route(ops):
    """H = 48: no kernel is instantiated and fld.normals composes the operators.  There is no fused answer to hold it to, so:
    outside the boxes the static composition's bits, and inside them the restatement on the oracle's own primal at the
    project's parity bar (rel-L2 <= 1e-4; the oracle's box position is not the device's to the bit, so no per-element bound)"""
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    O = NR.O
    cfg = NeuRADFieldConfig(geo_hidden_dim=48, nff_hidden_dim=48)
    st, ac = cfg.grid.static, cfg.grid.actor
    st.log2_hashmap_size, ac.log2_hashmap_size = 11, 9
    torch.manual_seed(0)
    actors = DynamicActors(DynamicActorsConfig(), trajectories=builders.trajectories())
    fld = NeuRADField(cfg, actors=actors, static_scale=100.0).cuda().eval()
    with torch.no_grad():
        fld.hashgrid.static_grid.hash_table.mul_(1000.0)
        for g in fld.hashgrid.actor_grids:
            g.hash_table.mul_(3000.0)
    assert not fld.normals_fused()
    sc = AR.scene()
    rays = AR.scene_rays(sc)
    rd, times = rays_dev(rays), dev(sc["times"])
    spec, cand = fld.hashgrid.prepare_actors(*rd, times)
    with pytest.raises(Exception, match="code 2"):  # the fused entry point refuses the shape by name
        ops.field_normals(fld.field_spec(), *rd, actors=(spec, cand))
    out = fld.normals(*rd, times=times, want=("gradient", "normals", "hit"))
    g, n, hit = out["gradient"], out["normals"], out["hit"]
    assert g.shape == (AR.R, AR.S, 3) and torch.isfinite(g).all() and (hit >= 0).float().mean() >= 0.15
    assert torch.allclose(n, g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12), atol=1e-6)
    static = ops.field_normals_operators(fld.field_spec(), *rd, want=("gradient",))["gradient"]
    assert torch.equal(g[hit < 0], static[hit < 0]) and not torch.equal(g[hit >= 0], static[hit >= 0])
    p = O.FieldParams(O.GridParams(host(fld.hashgrid.static_grid.hash_table), st.num_levels, st.base_res, st.max_res, 11), 100.0,
                      [host(l.weight) for l in fld.mlp_geo.layers], [host(l.bias) for l in fld.mlp_geo.layers], [], [],
                      use_sdf=cfg.use_sdf)
    ap = O.ActorParams(host(actors.unique_timestamps), host(actors.actor_positions), host(actors.actor_rotations_6d),
                       host(actors.actor_present_at_time), host(actors.actor_sizes), host(actors.actor_padding),
                       [O.GridParams(host(gr.hash_table), ac.num_levels, ac.base_res, ac.max_res, 9)
                        for gr in fld.hashgrid.actor_grids], actor_scale=10.0)
    r = AR.oracle_restatement(p, ap)
    keep = ~r["left_out"]
    assert np.array_equal(host(hit).reshape(-1)[keep], r["hit"][keep])
    gh = host64(g).reshape(-1, 3)
    for what, m in (("in a box", keep & (r["hit"] >= 0)), ("outside", keep & (r["hit"] < 0))):
        err = AR.rel_l2(gh[m], r["g"][m])
        print(f"H = 48 operators vs the restatement on the oracle's primal, {what}: rel-L2 {err:.3e}")
        assert err <= 1e-4


# ---- 8. the field's forward --------------------------------------------------------------------------------------------
def field_samples(rays, times, packed=False):
    from neurad_studio_amd.cameras.rays import Frustums, RaySamples

    o, d, a, s, e = rays_dev(rays)
    R, S = s.shape
    per = lambda t, c: t.reshape(R, 1, c).expand(R, S, c)  # noqa: E731
    fr = dict(origins=per(o, 3), directions=per(d, 3), starts=s[..., None], ends=e[..., None], pixel_area=per(a, 1))
    t = per(dev(times), 1)
    if packed:
        fr = {k: v.reshape(R * S, -1).contiguous() for k, v in fr.items()}
        t = t.reshape(R * S, 1).contiguous()
    return RaySamples(frustums=Frustums(**fr), times=t)


def test_field_forward_with_compute_normals(ops):
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as H

    fld = make_actor_field()  # the field of tests/golden/field_actors.npz: 4 x 4 actor grids
    p, ap = builders.field_params(), builders.actor_params(load_golden("field_actors"))
    sc = AR.scene()
    rays = AR.scene_rays(sc)
    rd, times = rays_dev(rays), dev(sc["times"])
    with torch.no_grad():
        prim = fld.normals(*rd, times=times, want=PRIMAL)
        cand = fld.hashgrid.prepare_actors(*rd, times)[1]
    hit, bp, rows = device_primal(prim, cand, AR.S)
    r = AR.restatement(p, ap, *rays, hit, bp, rows)
    r["hit"] = hit
    c, left_out = constants(p, ap, hit), r["left_out"] | near_face()
    for packed in (False, True):
        rs = field_samples(rays, sc["times"], packed)
        with torch.no_grad():
            plain, out = fld(rs), fld(rs, compute_normals=True)
        assert set(out) == set(plain) | {H.NORMALS, H.GRADIENT}
        for k in plain:  # the other heads: bit for bit
            assert torch.equal(out[k], plain[k]), k
        shape = (AR.R * AR.S, 3) if packed else (AR.R, AR.S, 3)
        assert out[H.NORMALS].shape == shape and out[H.GRADIENT].shape == shape
        check({"gradient": out[H.GRADIENT], "normals": out[H.NORMALS]}, r, c, left_out, what=f"forward packed={packed}")
    out = fld(field_samples(rays, sc["times"]), compute_normals=True)  # grad enabled: the two heads are detached all the same
    assert not out[H.NORMALS].requires_grad and not out[H.GRADIENT].requires_grad


# ---- 9. the model flag ---------------------------------------------------------------------------------------------------
def test_model_outputs_carry_the_normals():
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig
    from neurad_studio_amd.models.neurad import NeuRADHotPath, NeuRADHotPathConfig

    torch.manual_seed(1)
    c = NeuRADHotPathConfig(appearance_dim=0)
    c.field.grid.static.log2_hashmap_size, c.field.grid.actor.log2_hashmap_size, c.field.sdf_beta = 12, 10, 3.0
    for pf in (c.sampling.proposal_field_1, c.sampling.proposal_field_2):
        pf.grid.static.log2_hashmap_size, pf.grid.actor.log2_hashmap_size = 11, 9
    m = NeuRADHotPath(c, static_scale=100.0, actors=DynamicActors(DynamicActorsConfig(), trajectories=builders.trajectories()))
    m = m.cuda().eval()
    with torch.no_grad():
        m.field.hashgrid.static_grid.hash_table.mul_(500.0)
        for gr in m.field.hashgrid.actor_grids:
            gr.hash_table.mul_(3000.0)
        for pfield in m.proposal_fields:
            pfield.hashgrid.static_grid.hash_table.mul_(500.0)
            for gr in pfield.hashgrid.actor_grids:
                gr.hash_table.mul_(2000.0)
    R = 96
    with torch.no_grad():
        assert m.fused_eval_possible()
        before = m.get_nff_outputs(actor_rays(R))
    assert "normals" not in before
    seen = {}
    render = m.field.render

    def spy(o_, d_, area_, starts, ends, **kw):
        out = render(o_, d_, area_, starts, ends, **kw)
        seen.update(o=o_, d=d_, area=area_, starts=starts, ends=ends, out=out, kw=kw)
        return out

    m.field.render = spy
    m.normals = True
    with torch.no_grad():
        out = m.get_nff_outputs(actor_rays(R))
    assert set(out) == set(before) | {"normals"} and seen["kw"]["return_weights"] is True
    for k in before:
        assert torch.equal(out[k], before[k]), k
    w, s, e = seen["out"][3][:, :-1], seen["starts"][:, :-1], seen["ends"][:, :-1]  # the non-sky samples
    with torch.no_grad():
        per = m.field.normals(seen["o"], seen["d"], seen["area"], s, e, want=("normals", "hit"), times=seen["kw"]["times"],
                              actor_cand=seen["kw"]["actor_cand"])
    assert (per["hit"] >= 0).float().mean() > 0.02  # some of the render's samples lie in a box
    wn = (w[..., None] * per["normals"]).double().sum(1)
    want = wn / (wn.norm(dim=-1, keepdim=True) + 1e-10)
    got = out["normals"]
    assert got.shape == (R, 3) and got.dtype == torch.float32
    rel = float((got.double() - want).norm() / want.norm())
    print("model normals vs the normalised sum of w n: rel-L2", rel)
    assert rel <= 1e-6
    lit = w.sum(-1) > 1e-3
    assert lit.any() and (got[lit].norm(dim=-1) - 1).abs().max() < 1e-5
    m.normals = False
    with torch.no_grad():
        assert set(m.get_nff_outputs(actor_rays(R))) == set(before)
