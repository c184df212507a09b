"""Surface normals in a scene with dynamic actors, in numpy, restated from the oracle's existing functions (no kernel code):
what tests/test_normals_actor_refs_host.py pins to the reference's own autograd (tests/golden/normals_actors.npz, made by
scripts/make_golden_normals_actors.py) and tests/test_gpu_normals_actors.py holds csrc/normals.hip's actor form to.  The
definition and the bound are stated in include/neurad_hip.h at nrhip_field_normals_actors.

  outside every box   the static chain of tests/normals_refs.py.
  inside a box        the encoding row is the winner's (highest actor index): its own grid at the contraction (ACTOR scale) of
                      the box-frame position p with the sample's own std, zero columns from La * F on.  g_box = d geo / d p is
                      encode_static_ray_grads on a ray of one sample whose origin is p and whose direction is zero (mean = p
                      exactly, the std is the sample's); g_world = W^T diag(f, 1, 1) g_box, A = |W|^T A_box.

The in-box primal -- the winner, the box-frame position after the flip, the winner's world2box row -- is an ARGUMENT: the
GPU tests pass the device's (hit, box_position, cand_w2b), the host test the oracle's own (`oracle_primal`)."""
import functools

import numpy as np
import torch

import builders
import neurad_oracle as O
import normals_refs as NR
import synth

U, f32, f64 = NR.U, np.float32, np.float64
SHAPES = ((8, 4, 32), (8, 4, 64), (16, 2, 64), (4, 2, 32), (4, 2, 64))  # csrc/render_variants.h: `Composite, Actors, F32`
LG, ALG = 11, 9        # table sizes
R, S, FAR = 48, 24, 10.0
# the cases of the GPU tests: name -> (L, F, H, use_sdf, fp16 tables); every frame of SHAPES, and fp16 storage on (8, 4, 32)
CASES = {
    "8x4_h32_sdf": (8, 4, 32, True, False),
    "8x4_h64_density": (8, 4, 64, False, False),
    "16x2_h64_sdf": (16, 2, 64, True, False),
    "4x2_h32_sdf": (4, 2, 32, True, False),
    "4x2_h64_density": (4, 2, 64, False, False),
    "8x4_h32_fp16": (8, 4, 32, True, True),
}
EDIT = {"lateral": 0.4, "longitudinal": 0.0, "height": 0.0, "rotation": 0.3, "index": 1}  # the eval-time edit of the edit test
VARIANTS = ("rotate_with_W", "no_rotation", "static_gradient_kept", "static_scale_in_the_actor_contraction")


# ---- the scene ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    """builders.trajectories(): 3 actors, actor 2 overlaps actor 1, actor 0 present early only.  48 rays aimed from ~4 m at
    where their actor is at the ray's time, every fourth looking away; 24 power-sampler bins up to 10 m; times in [0, 4].
    -> dict o, d, area, times, starts, ends, edges"""
    gen = torch.Generator().manual_seed(5)
    times = 4.0 * torch.rand(R, generator=gen)
    a = torch.arange(R) % 3
    tgt = torch.stack([12.0 + 2.0 * times + a, torch.tensor([8.0, -6.0, -5.0])[a], torch.full((R,), 0.5)], -1)
    side = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen) * torch.tensor([1.0, 1.0, 0.15]), dim=-1)
    o = tgt + 4.0 * side
    d = torch.nn.functional.normalize(tgt + 0.3 * torch.randn(R, 3, generator=gen) - o, dim=-1)
    d[::4] = -d[::4]
    _, eu, _ = O.power_sampler(np.zeros(R), np.full(R, FAR, f32), S)
    return dict(o=o.numpy().astype(f32), d=d.numpy().astype(f32), area=np.full((R,), 2.7e-7, f32),
                times=times.numpy().astype(f32), starts=np.ascontiguousarray(eu[:, :-1]),
                ends=np.ascontiguousarray(eu[:, 1:]), edges=eu)


def ray_flips():
    """+-1 per ray of the scene, about half of each"""
    return np.where(np.random.default_rng(17).random(R) < 0.5, -1.0, 1.0).astype(f32)


def case_params(name):
    L, F, H, use_sdf, half = CASES[name]
    return field_params(L, F, H, use_sdf, half), actor_params(L, F, half)


def scene_rays(sc=None):
    sc = scene() if sc is None else sc
    return sc["o"], sc["d"], sc["area"], sc["starts"], sc["ends"]


@functools.lru_cache(maxsize=None)
def actor_params(L, F, half=False):
    """the oracle's ActorParams of the scene: packed_actor_refs.actor_tables' grids (La = min(4, L), table 2^9)"""
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    a = DynamicActors(DynamicActorsConfig(), trajectories=builders.trajectories())
    n = lambda t: t.detach().numpy()  # noqa: E731
    La = min(4, L)
    tabs = [synth.hash_table(La * 2**ALG, F, seed=900 + i, scale=0.7) for i in range(3)]
    if half:
        tabs = [t.astype(np.float16).astype(f32) for t in tabs]
    return O.ActorParams(n(a.unique_timestamps), n(a.actor_positions), n(a.actor_rotations_6d), n(a.actor_present_at_time),
                         n(a.actor_sizes), n(a.actor_padding), [O.GridParams(t, La, 64, 1024, ALG) for t in tabs],
                         actor_scale=10.0)


@functools.lru_cache(maxsize=None)
def field_params(L, F, H, use_sdf=True, half=False):
    """the static field of a shape: O(1) features on a 2^11 table"""
    p = builders.field_params(use_sdf, L, F, LG, H, 32, 2048, scale=2.0, seed=70 + L + F)
    p.geo_b[0] = synth.linear(H, 32, 200)[1]
    if half:
        p.grid.table = p.grid.table.astype(np.float16).astype(f32)
    return p


def constant(p, ap):
    """NRHIP_NORMALS_ACTORS_C(La, F, H) of include/neurad_hip.h"""
    return p.geo_w[0].shape[0] + ap.grids[0].num_levels + p.grid.n_feat + 240 + 6


# ---- the primal, from the oracle alone ---------------------------------------------------------------------------------
def box_frames(ap, times, edit=None):
    """-> world2box [R,A,3,4] fp32 and valid [R,A] at the rays' times"""
    b2w, valid = O.actor_boxes2world(ap, times, edit)
    return O.pose_inverse(b2w), valid


def containment(ap, o, d, area, starts, ends, times, edit=None):
    """-> inside [R,S,A] bool (O.actor_hits: every (sample, containing actor)), mean [R,S,3], w2b [R,A,3,4], valid [R,A]"""
    mean, _ = O.fast_isotropic_gaussian(o, d, area, starts, ends)
    b2w, valid = O.actor_boxes2world(ap, times, edit)
    w2b = O.pose_inverse(b2w)
    r, s, k = O.actor_hits(ap, mean, b2w, valid, w2b)
    inside = np.zeros(mean.shape[:2] + (valid.shape[1],), bool)
    inside[r, s, k] = True
    return inside, mean, w2b, valid


def candidates(ap, o, d, area, starts, ends, times, edit=None):
    """[R,A] bool: the actors on a ray's candidate list (the line cull of neurad_encoding.py:231-239)"""
    mean, _ = O.fast_isotropic_gaussian(o, d, area, starts, ends)
    b2w, valid = O.actor_boxes2world(ap, times, edit)
    radii = np.sqrt((ap.bounds * ap.bounds).sum(-1)).astype(f32)
    p0 = mean[:, 0, :]
    ld = mean[:, -1, :] - p0
    ld = ld / (np.linalg.norm(ld, axis=-1, keepdims=True).astype(f32) + f32(1e-7))
    dist = np.linalg.norm(np.cross(b2w[..., :3, 3] - p0[:, None, :], ld[:, None, :]), axis=-1).astype(f32)
    return (dist < radii[None, :]) & valid


def oracle_primal(ap, o, d, area, starts, ends, times, ray_flip=None, edit=None):
    """the in-box primal as the oracle has it: hit [N] (the highest containing actor or -1), box_position [N,3] fp32 after the
    flip, w2b rows [N,3,4] of the winner, and how many boxes contain each sample [N]"""
    inside, mean, w2b, _ = containment(ap, o, d, area, starts, ends, times, edit)
    Rn, Sn, A = inside.shape
    hit = np.where(inside.any(-1), A - 1 - np.argmax(inside[..., ::-1], -1), -1).reshape(-1)
    ray = np.repeat(np.arange(Rn), Sn)
    rows = w2b[ray, np.maximum(hit, 0)]
    x = mean.reshape(-1, 3)
    pos = ((rows[:, :, :3] @ x[:, :, None])[:, :, 0] + rows[:, :, 3]).astype(f32)
    if ray_flip is not None:
        pos[:, 0] *= np.asarray(ray_flip, f32)[ray]
    return hit, pos, rows, inside.sum(-1).reshape(-1)


def near_a_face(ap, mean, w2b, valid):
    """[N] bool: one of the box test's three |.| < bound comparisons of some present actor is within 8 u of its own absolute
    terms -- the test is compiled with contraction allowed, so its bits cannot be restated"""
    Rn, Sn = mean.shape[:2]
    m = mean.astype(f64)[:, :, None, None, :]                     # [R,S,1,1,3]
    W = w2b.astype(f64)[:, None]                                  # [R,1,A,3,4]
    pos = (W[..., :3] * m).sum(-1) + W[..., 3]                    # [R,S,A,3]
    terms = (np.abs(W[..., :3]) * np.abs(m)).sum(-1) + np.abs(W[..., 3])
    b = ap.bounds.astype(f64)[None, None]
    close = np.abs(np.abs(pos) - b) <= 8 * U * (terms + b)
    return (close.any(-1) & valid[:, None, :]).any(-1).reshape(-1)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def restatement(p, ap, o, d, area, starts, ends, hit, box_position, w2b_rows, ray_flip=None, variant=None):
    """-> dict like normals_refs.restatement: g, A [N,3] float64, geo, A_geo [N], normals [N,3], left_out [N] (the ReLU rule
    alone: the caller adds `near_a_face`), enc [N, L F].  hit [N], box_position [N,3] fp32, w2b_rows [N,3,4] fp32: the
    in-box primal; ray_flip [R] or None.  variant: one of VARIANTS, a wrong chain the golden must tell apart."""
    assert variant is None or variant in VARIANTS
    rays = NR.per_sample_rays(o, d, area, starts, ends)
    Sn = np.asarray(starts).shape[1]
    hit = np.asarray(hit).reshape(-1)
    bp = np.asarray(box_position, f32).reshape(-1, 3)
    W = np.asarray(w2b_rows, f64).reshape(-1, 3, 4)[:, :, :3]
    N, LF = hit.shape[0], p.grid.num_levels * p.grid.n_feat
    flip = np.ones(N) if ray_flip is None else np.repeat(np.asarray(ray_flip, f64), Sn)
    ascale = p.static_scale if variant == "static_scale_in_the_actor_contraction" else ap.actor_scale
    zero = np.zeros((N, 3), f32)
    enc = O.encode_static(p.grid, p.static_scale, *rays).copy()
    for k, gk in enumerate(ap.grids):
        sel = hit == k
        if sel.any():
            row = O.encode_static(gk, ascale, bp[sel], zero[sel], rays[2][sel], rays[3][sel], rays[4][sel])
            enc[sel] = np.pad(row, ((0, 0), (0, LF - row.shape[1])))
    y, hidden = O.mlp_fwd(enc, p.geo_w, p.geo_b, return_hidden=True)
    cot = np.zeros_like(y)
    cot[:, 0] = 1
    g_enc = O.mlp_bwd(hidden, p.geo_w, cot)[0]
    w0, b0 = np.asarray(p.geo_w[0], f64), np.asarray(p.geo_b[0], f64)
    w1, b1 = np.asarray(p.geo_w[1], f64)[0], float(np.asarray(p.geo_b[1], f64)[0])
    g_enc_abs = (np.abs(w1)[None, :] * (hidden[1] > 0)) @ np.abs(w0)
    chain = lambda grid, scale, r5, ge: O.encode_static_ray_grads(grid, scale, *r5, ge, with_abs=True)  # noqa: E731
    g = chain(p.grid, p.static_scale, rays, g_enc)[0]
    A = chain(p.grid, p.static_scale, rays, g_enc_abs)[2]
    if variant != "static_gradient_kept":
        for k, gk in enumerate(ap.grids):
            sel = hit == k
            if not sel.any():
                continue
            r5 = (bp[sel], zero[sel], rays[2][sel], rays[3][sel], rays[4][sel])
            cols = gk.num_levels * gk.n_feat
            gb = chain(gk, ascale, r5, g_enc[sel, :cols])[0] * np.stack([flip[sel], np.ones(sel.sum()), np.ones(sel.sum())], -1)
            Ab = chain(gk, ascale, r5, g_enc_abs[sel, :cols])[2]
            if variant == "rotate_with_W":
                g[sel], A[sel] = np.einsum("nkc,nc->nk", W[sel], gb), np.einsum("nkc,nc->nk", np.abs(W[sel]), Ab)
            elif variant == "no_rotation":
                g[sel], A[sel] = gb, Ab
            else:  # g_world = W^T diag(f, 1, 1) g_box
                g[sel], A[sel] = np.einsum("nkc,nk->nc", W[sel], gb), np.einsum("nkc,nk->nc", np.abs(W[sel]), Ab)
    e64 = enc.astype(f64)
    z = e64 @ w0.T + b0
    z_terms = np.abs(e64) @ np.abs(w0).T + np.abs(b0)
    geo = np.maximum(z, 0.0) @ w1 + b1
    A_geo = z_terms @ np.abs(w1) + abs(b1)
    left_out = (np.abs(z) <= 64 * U * z_terms).any(-1)
    return dict(g=g, A=A, geo=geo, A_geo=A_geo, normals=NR.normalise(g, p.use_sdf), left_out=left_out, enc=enc)


def oracle_restatement(p, ap, sc=None, ray_flip=None, edit=None, variant=None):
    """the restatement on the oracle's own primal -> (dict with `hit`, `n_boxes`, and `left_out` including the samples near a
    face)"""
    sc = scene() if sc is None else sc
    rays = scene_rays(sc)
    hit, pos, rows, n_boxes = oracle_primal(ap, *rays, sc["times"], ray_flip, edit)
    r = restatement(p, ap, *rays, hit, pos, rows, ray_flip, variant)
    _, mean, w2b, valid = containment(ap, *rays, sc["times"], edit)
    r["left_out"] = r["left_out"] | near_a_face(ap, mean, w2b, valid)
    r.update(hit=hit, n_boxes=n_boxes, box_position=pos, w2b_rows=rows)
    return r


def rel_l2(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
