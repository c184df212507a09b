"""Scenes and references of the dynamic-actor kernels' own tests (tests/test_actor_refs_host.py,
tests/test_gpu_actor_kernels.py): csrc/actors.hip's candidate lists, containment tables, pair positions and density
splice, each compared per element.  No GPU, no test functions.

Two tiers of scenes.

EXACT: every fp32 operation of the kernels is exact, so the results are compared bit for bit (zeros by value: -0 == +0),
ties included.  Actors are parked (the same pose at every keyframe, so pl + (pr - pl) * frac == pl whatever frac is),
stored rotations are (1,0,0, 0,1,0) and its quarter turns, positions / origins / sample edges are small dyadic numbers,
rays run along +x over at least 2 m (|p1 - p0| + 1e-7f rounds back to |p1 - p0|), bounds have an exact diagonal:
(1,2,2) b -> 3 b, (2,3,6) -> 7.  The reference is the fp32 numpy oracle (neurad_oracle.actor_boxes2world, pose_inverse,
actor_hits; packed_actor_refs.in_box).  `exact_check` recomputes every intermediate in float64 and requires equality.

GENERIC: moving actors with non-orthonormal stored 6-D rotations (both Gram-Schmidt steps work).  The references are
float64 restatements of the same formulas (utils/poses.py:90-150, neurad_encoding.py:225-263): `frames64`, `prepare64`,
`hits64` in numpy; grad_edge_refs.actor_pair_grads64 (world2box_pairs + the contraction, torch.float64 autograd) for the
pair positions; `splice64` for the density splice.  Bracket indices come from the fp32 timestamps and times, which are
exact in float64.  The rule is sharp_refs.check's: per element |got - ref| <= atol + c U mag with U = 2^-24, mag the
float64 sum of magnitudes the fp32 arithmetic adds up for the element, and c the roundings along the longest chain:

  stored pose    normalize (3-term dot 3, sqrt 1, division 1) 5, a1.a2 5, a2 - dt a1 2, normalize 5          -> 17
  lerp           frac (q - lt, rt - lt, + 1e-6, division) 4, pr - pl, * frac, + pl 3                         ->  7
  interpolated   the same Gram-Schmidt 17, cross product 3                                                   -> 20
  w2b            rotation entries: 17 + 7 + 20 = 44 (C_ROT); translation -(b . t): 3 products, 2 sums on top
                 of the lerp of t, 7 + 5 = 12 more (C_TR = 56); an edit adds cosf / sinf (2 ulp each) and their
                 products: 8 (C_EDIT)
  mag            rotation entries: kappa, the amplification of the two Gram-Schmidt steps (|r2| / |r2 - (a1.r2) a1| of
                 the stored rows, the same of the interpolated rows, 1 / |u1|): the roundings are relative to the
                 vectors before they are projected; translation: kappa tmag, tmag = max(|t_l|_1, |t_r|_1) + |t_r - t_l|_1 (+ |shift|_1),
                 the sizes the lerp adds up
  cull           p0, p1 (t0 + (t1 - t0) / 2: 3, o + d t: 2) 5, line (difference 1, norm 5, division 1) 7, v = t - p0 1,
                 cross 3, norm 5 on top of t's 7 -> 28, C_DIST = 32 on kappa tmag + |p0|_1 + |v|_1 + radius
  box position   w2b C_TR, the sample mean 5, 3 products and 3 sums 6 -> 67, C_POS = 72 on
                 kappa (tmag + |mean|_1)

A discrete decision (candidate, containment) whose float64 margin (dist - radius, |pos_k| - bound_k) lies within that
quantity's own bound is left out of the exact comparison; MAX_LEFT_OUT caps the share of such decisions per scene."""
import functools

import numpy as np
import torch

import neurad_oracle as O

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
KH = 8  # NRHIP_MAX_SAMPLE_CONTAINMENTS
C_ROT, C_TR, C_EDIT, C_DIST, C_POS = 44, 56, 8, 32, 72
C_X01, C_CSTD = 8, 64  # see pair_forward_bounds
MAX_LEFT_OUT = 0.005
SENTINEL_I, SENTINEL_F = -12345, f32(-777.25)
EPS_T, EPS_L = f32(1e-6), f32(1e-7)

IDENT = (1, 0, 0, 0, 1, 0)
TURNS = (IDENT, (0, 1, 0, -1, 0, 0), (-1, 0, 0, 0, -1, 0), (0, -1, 0, 1, 0, 0))  # yaw by 0, 90, 180, 270 degrees


def bits(x):
    """fp32 array -> its bit patterns with -0 folded onto +0"""
    return (np.asarray(x, f32) + f32(0)).view(np.uint32)


def scene_dict(ts, pos, rot, present, bounds, o, d, starts, ends, times, scale=10.0, area=None):
    R = np.asarray(o).shape[0]
    return dict(timestamps=np.asarray(ts, f32), positions=np.ascontiguousarray(pos, f32),
                rotations_6d=np.ascontiguousarray(rot, f32), present=np.ascontiguousarray(present, bool),
                bounds=np.ascontiguousarray(bounds, f32), scale=float(scale), o=np.ascontiguousarray(o, f32),
                d=np.ascontiguousarray(d, f32), starts=np.ascontiguousarray(starts, f32),
                ends=np.ascontiguousarray(ends, f32), times=np.asarray(times, f32),
                area=np.full((R,), 2.5e-6, f32) if area is None else np.asarray(area, f32))


def actor_params(sc):
    """the oracle's view of a scene: sizes = 2 bounds, no padding (bounds = sizes / 2 + padding exactly), no grids"""
    return O.ActorParams(sc["timestamps"], sc["positions"], sc["rotations_6d"], sc["present"], sc["bounds"] * f32(2),
                         np.zeros(3, f32), [], actor_scale=sc["scale"])


def sub_scene(sc, rays):
    """the same actors, the rays `rays` only"""
    out = dict(sc)
    for k in ("o", "d", "starts", "ends", "times", "area"):
        out[k] = np.ascontiguousarray(sc[k][rays])
    return out


# ---- the fp32 oracle's candidate lists and containment tables -----------------------------------------------------------
def oracle_lists(sc, edit=None):
    """-> count [R], close [R,A] bool, w2b [R,A,12] fp32, hits [R*S, KH] (the KH highest containing actors, ascending, -1
    behind), n_contain [R*S]: neurad_oracle's fp32 arithmetic -- the cull as neurad_oracle.actor_hits forms it"""
    ap = actor_params(sc)
    mean, _ = O.fast_isotropic_gaussian(sc["o"], sc["d"], sc["area"], sc["starts"], sc["ends"])
    b2w, valid = O.actor_boxes2world(ap, sc["times"], edit)
    w2b = O.pose_inverse(b2w)
    radii = np.sqrt((ap.bounds * ap.bounds).sum(-1)).astype(f32)
    p0 = mean[:, 0, :]
    ld = mean[:, -1, :] - p0
    ld = ld / (np.linalg.norm(ld, axis=-1, keepdims=True).astype(f32) + EPS_L)
    vec = b2w[..., :3, 3] - p0[:, None, :]
    dist = np.linalg.norm(np.cross(vec, ld[:, None, :]), axis=-1).astype(f32)
    close = (dist < radii[None, :]) & valid
    R, S = sc["starts"].shape
    pos = np.einsum("rakc,rsc->rsak", w2b[..., :3], mean).astype(f32) + w2b[:, None, :, :, 3]
    inside = np.all(np.abs(pos) < ap.bounds[None, None], axis=-1) & close[:, None, :]  # [R,S,A]
    return dict(count=close.sum(-1).astype(np.int32), close=close, w2b=w2b.reshape(R, -1, 12), dist=dist, radii=radii,
                hits=hits_table(inside.reshape(R * S, -1)), n_contain=inside.reshape(R * S, -1).sum(-1), inside=inside,
                valid=valid, mean=mean, pos=pos)


def hits_table(inside):
    """[N,A] bool -> [N,KH] int32: the KH highest set indices of each row, ascending, -1 behind"""
    N, A = inside.shape
    out = np.full((N, KH), -1, np.int32)
    for n in np.nonzero(inside.any(-1))[0]:
        k = np.nonzero(inside[n])[0][-KH:]
        out[n, :len(k)] = k
    return out


def lists_from_close(close, w2b, K=None, fill_i=SENTINEL_I, fill_f=SENTINEL_F):
    """what nrhip_actor_prepare leaves in sentinel-prefilled buffers: -> count [R], actor [R,K], w2b [R,K,12], overflow"""
    R, A = close.shape
    K = A if K is None else K
    act = np.full((R, K), fill_i, np.int32)
    w = np.full((R, K, 12), fill_f, f32)
    for r in range(R):
        k = np.nonzero(close[r])[0][:K]
        act[r, :len(k)], w[r, :len(k)] = k, w2b[r, k]
    n = close.sum(-1)
    return np.minimum(n, K).astype(np.int32), act, w, int((n > K).any())


# ---- EXACT tier ---------------------------------------------------------------------------------------------------------
CLUSTER_Y = 32.0  # clusters of actors lie 32 m apart in y: no ray of one cluster is near an actor of another


def _cluster_of(i):
    """pass scene: which cluster actor i belongs to.  0: actors 70, 90, 100 (pass 2 only); 1: actor 128 (pass 3 only);
    2: actors of all three passes; 4: actor 5 alone (the cull ties); 3: everyone else (the overflow cluster)"""
    if i in (70, 90, 100):
        return 0
    if i == 128:
        return 1
    if i in (3, 10, 63, 64, 65, 127, 129):
        return 2
    if i == 5:
        return 4
    return 3


@functools.lru_cache(maxsize=None)
def exact_pass_scene(A, S=5, R=None):
    """A parked actors in clusters along y; rays along +x at y = the clusters' lines, one ray at a line without actors and
    the four tie rays of cluster 4 (actor 5, radius 3): dist == radius on either side (rejected) and 2^-10 inside."""
    idx = np.arange(A)
    cl = np.array([_cluster_of(i) for i in idx])
    pos = np.stack([2.5 + 0.5 * (idx % 4), CLUSTER_Y * cl + 0.25 * (idx % 5), np.zeros(A)], -1)  # z = 0: dist = |dy| exactly
    big = (idx % 2 == 1) & (idx != 5)
    bounds = np.where(big[:, None], np.array([2.0, 3.0, 6.0]), np.array([1.0, 2.0, 2.0]))
    rot = np.array([TURNS[i % 4] for i in idx], f64)
    ys = [CLUSTER_Y * c + off for c in (0, 1, 2, 3, 7) for off in (0.0, 0.5, 1.0)]
    y5 = CLUSTER_Y * 4 + 0.25 * (5 % 5)
    ys += [y5 + 3.0, y5 + 3.0 - 2.0 ** -10, y5 - 3.0, y5 - 3.0 + 2.0 ** -10]
    ys = np.array(ys if R is None else (ys * (R // len(ys) + 1))[:R])
    Rn = len(ys)
    o = np.stack([np.zeros(Rn), ys, np.zeros(Rn)], -1)
    d = np.tile(np.array([1.0, 0.0, 0.0]), (Rn, 1))
    edges = np.tile(np.arange(S + 1, dtype=f64), (Rn, 1)) if S > 1 else np.tile(np.array([1.0, 2.0]), (Rn, 1))
    present = np.ones((2, A), bool)
    present[:, idx % 13 == 6] = False  # some actors are absent at both keyframes: never a candidate
    return scene_dict([0.0, 1.0], np.tile(pos[None], (2, 1, 1)), np.tile(rot[None], (2, 1, 1)), present, bounds, o, d,
                      edges[:, :-1], edges[:, 1:], 0.25 + 0.5 * (np.arange(Rn) % 2))


@functools.lru_cache(maxsize=None)
def exact_time_scene(Tn):
    """4 parked actors, present flags in every (left, right) combination over the keyframes, query times below / on / inside
    / above the timestamps (Tn = 4) or anywhere (Tn = 1: left == right).  Parked, so only `valid` depends on the time."""
    ts = [0.0, 0.5, 1.25, 2.0][:Tn]
    A = 4
    pos = np.array([[3.0, 0.0, 0.0], [3.5, 0.5, 0.0], [2.5, -0.5, 0.0], [3.0, 0.25, 0.0]])
    present = np.array([[0, 1, 0, 1], [0, 0, 1, 1], [1, 0, 0, 1], [0, 1, 1, 0]], bool)[:Tn]
    q = np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 1.25, 1.5, 2.0, 3.0])
    R = len(q)
    o = np.stack([np.zeros(R), 0.25 * (np.arange(R) % 3), np.zeros(R)], -1)
    edges = np.tile(np.arange(6, dtype=f64), (R, 1))
    return scene_dict(ts, np.tile(pos[None], (Tn, 1, 1)), np.tile(np.array(TURNS, f64)[None], (Tn, 1, 1)), present,
                      np.tile(np.array([1.0, 2.0, 2.0]), (A, 1)), o, np.tile(np.array([1.0, 0.0, 0.0]), (R, 1)),
                      edges[:, :-1], edges[:, 1:], q)


NEST = 12


@functools.lru_cache(maxsize=None)
def exact_nest_scene():
    """12 boxes (1,2,2) b_j, b_j = (j + 1) / 2, around (8, 0, 0) (j odd: turned by 180 degrees).
    Ray 0 along y = z = 0 with sample means at 0.25 + s / 2: a sample lies in 0 .. 12 boxes.  Ray 1: the same with means
    at s / 2 + 0.5, each one ON an x face (outside).  Rays 2 / 3: at y = 12 = the y bound of box 11 (outside it) and 2^-8
    inside; rays 4 / 5: the same in z.  Ray 6: far from every actor.  Ray 7: ray 0 again."""
    j = np.arange(NEST)
    b = (j + 1) / 2.0
    pos = np.tile(np.array([8.0, 0.0, 0.0]), (NEST, 1))
    bounds = b[:, None] * np.array([1.0, 2.0, 2.0])
    rot = np.array([TURNS[2 * (i % 2)] for i in range(NEST)], f64)
    yz = [(0, 0), (0, 0), (12.0, 0), (12.0 - 2.0 ** -8, 0), (0, 12.0), (0, 12.0 - 2.0 ** -8), (1000.0, 0), (0, 0)]
    R, S = len(yz), 16
    o = np.array([[0.25 if r == 1 else 0.0, y, z] for r, (y, z) in enumerate(yz)])
    edges = np.tile(np.arange(S + 1, dtype=f64) / 2, (R, 1))
    return scene_dict([0.0, 1.0], np.tile(pos[None], (2, 1, 1)), np.tile(rot[None], (2, 1, 1)), np.ones((2, NEST), bool),
                      bounds, o, np.tile(np.array([1.0, 0.0, 0.0]), (R, 1)), edges[:, :-1], edges[:, 1:], np.full(R, 0.5))


def exact_check(sc):
    """The scene is exact: every intermediate of the oracle's fp32 chain, recomputed in float64 from the fp32 inputs,
    equals the fp32 value.  -> the oracle's lists"""
    ref = oracle_lists(sc)
    R, S = sc["starts"].shape
    g = prepare64(sc, eps_l=0.0 if S > 1 else f64(EPS_L))  # S > 1: |p1 - p0| + 1e-7f == |p1 - p0| in fp32, asserted below
    assert np.array_equal(g["w2b"], ref["w2b"].astype(f64)), "w2b is not exact"
    assert np.array_equal(g["dist"], ref["dist"].astype(f64)) and np.array_equal(g["radius"], ref["radii"].astype(f64))
    assert np.array_equal(g["mean"], ref["mean"].astype(f64)), "sample means are not exact"
    assert np.array_equal(g["kappa"], np.ones_like(g["kappa"]))
    pos64 = np.einsum("rakc,rsc->rsak", g["w2b"].reshape(R, -1, 3, 4)[..., :3], g["mean"]) + \
        g["w2b"].reshape(R, 1, -1, 3, 4)[..., 3]
    assert np.array_equal(pos64, ref["pos"].astype(f64)), "box positions are not exact"
    if S > 1:  # the line direction is a unit axis
        ln = np.linalg.norm(g["mean"][:, -1] - g["mean"][:, 0], axis=-1)
        assert (ln >= 2).all() and np.array_equal((ln.astype(f32) + EPS_L), ln.astype(f32))
    return ref


# ---- GENERIC tier: float64 restatements --------------------------------------------------------------------------------
def _gs64(r1, r2):
    n1 = np.maximum(np.linalg.norm(r1, axis=-1, keepdims=True), 1e-12)
    a1 = r1 / n1
    c = r2 - (a1 * r2).sum(-1, keepdims=True) * a1
    nc = np.maximum(np.linalg.norm(c, axis=-1, keepdims=True), 1e-12)
    return a1, c / nc, (np.linalg.norm(r2, axis=-1, keepdims=True) / nc)[..., 0], n1[..., 0]


def brackets(ts, q):
    """torch.searchsorted(side=left) on the fp32 values -> left, right, frac (float64 of the fp32 formula)"""
    ts, q = np.asarray(ts, f32).astype(f64), np.asarray(q, f32).astype(f64)
    right = np.searchsorted(ts, q, side="left")
    left = np.maximum(right - 1, 0)
    right = np.minimum(right, len(ts) - 1)
    frac = np.clip((q - ts[left]) / (ts[right] - ts[left] + f64(EPS_T)), 0.0, 1.0)
    return left, right, frac


def frac32(ts, q):
    """the kernels' own fp32 frac: exactly 0 or 1 where the fp32 operations round to it"""
    ts, q = np.asarray(ts, f32), np.asarray(q, f32)
    left, right, _ = brackets(ts, q)
    return np.clip((q - ts[left]) / (ts[right] - ts[left] + EPS_T), f32(0), f32(1)).astype(f32)


def frames64(sc, q, act, edit=None):
    """interpolate_trajectories_6d + rotation_6d_to_matrix + the eval-time edit for N (time, actor) pairs, float64.
    -> b [N,3,3] (rows b1, b2, b3 of boxes2world), t [N,3], left, right, frac, kappa [N], tmag [N] = what the lerp of the
    translation adds up, max(|t_l|_1, |t_r|_1) + |t_r - t_l|_1 (+ the edit's shift)"""
    left, right, frac = brackets(sc["timestamps"], q)
    rot, pos = sc["rotations_6d"].astype(f64), sc["positions"].astype(f64)
    a1, a2, k1, _ = _gs64(rot[..., :3], rot[..., 3:])
    poses = np.concatenate([a1, a2, pos], -1)
    pl, pr = poses[left, act], poses[right, act]
    ip = pl + (pr - pl) * frac[:, None]
    b1, b2, k2, n1 = _gs64(ip[:, :3], ip[:, 3:6])
    b3 = np.cross(b1, b2)
    t = ip[:, 6:].copy()
    kappa = np.maximum(k1[left, act], k1[right, act]) * k2 / np.minimum(n1, 1.0)
    tmag = np.maximum(np.abs(pl[:, 6:]).sum(-1), np.abs(pr[:, 6:]).sum(-1)) + np.abs(pr[:, 6:] - pl[:, 6:]).sum(-1)
    if edit is not None and (edit.get("longitudinal", 0.0) != 0 or edit.get("lateral", 0.0) != 0 or edit.get("rotation", 0.0) != 0):
        A = rot.shape[1]
        on = np.ones(len(act), bool) if edit.get("index", -1) < 0 else act == min(int(edit["index"]), A - 1)
        v = np.array([f32(edit.get("lateral", 0.0)), f32(edit.get("longitudinal", 0.0)), f32(edit.get("height", 0.0))], f64)
        if (v != 0).any():
            t[on] += np.stack([b1 @ v, b2 @ v, b3 @ v], -1)[on]
            tmag = tmag + on * np.abs(v).sum()
        if edit.get("rotation", 0.0) != 0:
            c, s = np.cos(f64(f32(edit["rotation"]))), np.sin(f64(f32(edit["rotation"])))
            n1_, n2_ = c * b1 - s * b2, s * b1 + c * b2
            b1, b2 = np.where(on[:, None], n1_, b1), np.where(on[:, None], n2_, b2)
    return np.stack([b1, b2, b3], -2), t, left, right, frac, kappa, tmag


def sample_means64(sc):
    o, d = sc["o"].astype(f64), sc["d"].astype(f64)
    t0, t1 = sc["starts"].astype(f64), sc["ends"].astype(f64)
    t = t0 + (t1 - t0) / 2
    return o[:, None, :] + d[:, None, :] * t[..., None]


def prepare64(sc, edit=None, eps_l=f64(EPS_L)):
    """nrhip_actor_prepare[_edited] in float64 (eps_l: the 1e-7 behind the line's length; exact_check passes 0 where fp32's
    sum rounds it away) -> w2b [R,A,12] with its bound [R,A,12], valid, dist / radius and the cull's
    bound [R,A], close (decision), unsure (margin within the bound), kappa, tmag"""
    R, A = sc["o"].shape[0], sc["positions"].shape[1]
    rr, aa = np.repeat(np.arange(R), A), np.tile(np.arange(A), R)
    b, t, left, right, frac, kappa, tmag = frames64(sc, sc["times"][rr], aa, edit)
    w = np.concatenate([np.swapaxes(b, -1, -2), -np.einsum("nkc,nk->nc", b, t)[..., None]], -1)  # [N,3,4]: [R^T | -R^T t]
    c_e = C_EDIT if edit is not None else 0
    wb = np.empty_like(w)
    wb[..., :3] = ((C_ROT + c_e) * U * kappa)[:, None, None]
    wb[..., 3] = ((C_TR + c_e) * U * kappa * tmag)[:, None]
    valid = sc["present"][left, aa] | sc["present"][right, aa]
    mean = sample_means64(sc)
    p0 = mean[:, 0]
    ld = mean[:, -1] - p0
    ld = ld / (np.linalg.norm(ld, axis=-1, keepdims=True) + eps_l)
    v = t - p0[rr]
    dist = np.linalg.norm(np.cross(v, ld[rr]), axis=-1)
    radius = np.linalg.norm(sc["bounds"].astype(f64), axis=-1)
    dband = C_DIST * U * (kappa * tmag + np.abs(p0[rr]).sum(-1) + np.abs(v).sum(-1) + radius[aa])
    sh = lambda x: x.reshape((R, A) + x.shape[1:])  # noqa: E731
    close = valid & (dist < radius[aa])
    unsure = valid & (np.abs(dist - radius[aa]) <= dband)
    return dict(w2b=sh(w.reshape(-1, 12)), w2b_bound=sh(wb.reshape(-1, 12)), valid=sh(valid), dist=sh(dist), radius=radius,
                dist_band=sh(dband), close=sh(close), unsure=sh(unsure), kappa=sh(kappa), tmag=sh(tmag), mean=mean,
                left=sh(left), right=sh(right), frac=sh(frac))


def hits64(sc, prep=None, edit=None):
    """nrhip_actor_hits in float64 on prepare64's candidates -> inside [R,S,A] (decision), unsure [R,S,A]: the margin of an
    axis within the box position's bound, or the cull itself unsure"""
    g = prepare64(sc, edit) if prep is None else prep
    R, A = g["close"].shape
    w = g["w2b"].reshape(R, A, 3, 4)
    pos = np.einsum("rakc,rsc->rsak", w[..., :3], g["mean"]) + w[:, None, :, :, 3]
    bnd = sc["bounds"].astype(f64)[None, None]
    band = (C_POS * U * g["kappa"][:, None, :] * (g["tmag"][:, None, :] + np.abs(g["mean"]).sum(-1)[:, :, None]))[..., None]
    margin = np.abs(pos) - bnd
    inside_box = (margin < 0).all(-1)
    maybe = (margin < band).all(-1)  # no axis decisively outside
    near = (np.abs(margin) <= band).any(-1) & maybe
    inside = inside_box & g["close"][:, None, :]
    unsure = g["valid"][:, None, :] & (near & (g["close"] | g["unsure"])[:, None, :] | (g["unsure"][:, None, :] & maybe))
    return dict(inside=inside, unsure=unsure, pos=pos)


def left_out_share(unsure, decisions):
    return float(unsure.sum()) / max(int(decisions), 1)


@functools.lru_cache(maxsize=None)
def generic_scene(seed=0, A=12, R=64, S=16, wide=False, scale=10.0):
    """A moving, yawing actors with non-orthonormal stored rotations over Tn = 4 keyframes; rays from near the origin
    at the place of actor r % A at the ray's time.  Times: below ts[0], on ts[0], ts[2], ts[3], above ts[3], inside a
    bracket.  wide: keyframes 64 s apart, where rt - lt + 1e-6 == rt - lt and frac == 1 exactly on a keyframe."""
    rng = np.random.default_rng(100 + seed)
    ts = np.array([0.0, 0.5, 1.25, 2.0]) * (128.0 if wide else 1.0)
    Tn = len(ts)
    base = np.stack([rng.uniform(8, 40, A), rng.uniform(-6, 6, A), rng.uniform(-0.5, 0.5, A)], -1)
    vel = np.stack([rng.uniform(-2, 2, A), rng.uniform(-1, 1, A), np.zeros(A)], -1)
    tn = ts / ts[-1] * 2.0
    pos = base[None] + vel[None] * tn[:, None, None]
    yaw = rng.uniform(0, 2 * np.pi, A)[None] + 0.3 * np.arange(Tn)[:, None]
    r1 = np.stack([np.cos(yaw), np.sin(yaw), np.full_like(yaw, 0.05)], -1) * rng.uniform(0.7, 1.4, (Tn, A, 1))
    r2 = np.stack([-np.sin(yaw), np.cos(yaw), np.full_like(yaw, 0.03)], -1) * rng.uniform(0.7, 1.4, (Tn, A, 1)) + 0.2 * r1
    bounds = np.stack([rng.uniform(0.8, 1.6, A), rng.uniform(1.5, 2.5, A), rng.uniform(0.7, 1.0, A)], -1)
    present = rng.random((Tn, A)) < 0.7
    present[:, 0], present[:, 1] = [0, 0, 1, 1], [1, 0, 0, 1]  # every (left, right) combination, whatever the draw
    special = np.array([-1.0, ts[0], ts[2], ts[3], ts[3] + 1.0])
    q = rng.uniform(ts[0], ts[-1], R)
    q[:2 * len(special)] = np.tile(special, 2)
    q = q.astype(f32)
    left, right, frac = brackets(ts, q)
    tgt_a = np.arange(R) % A
    tgt = pos[left, tgt_a] + (pos[right, tgt_a] - pos[left, tgt_a]) * frac[:, None] + rng.normal(0, 0.4, (R, 3))
    o = np.stack([rng.uniform(-1, 1, R), rng.uniform(-2, 2, R), rng.uniform(0.2, 0.8, R)], -1)
    d = tgt - o
    far = np.linalg.norm(d, axis=-1)
    d /= far[:, None]
    # S sorted samples, dense around the target: most rays put several consecutive samples into a box
    u = np.sort(rng.uniform(0, 1, (R, S + 1)), -1)
    edges = np.maximum(far[:, None] - 4.0, 0.5) + 8.0 * u
    edges[:, 0], edges[:, -1] = 0.25, far + 8.0
    return scene_dict(ts, pos, np.concatenate([r1, r2], -1), present, bounds, o, d, edges[:, :-1], edges[:, 1:], q,
                      scale=scale)


# ---- pairs: production order and designed runs -------------------------------------------------------------------------
RUNS = (1, 2, 15, 16, 17, 40)
# (position, run length): a 16-run from lane 5 (crosses a row), a 2-run, a 40-run over 40..79 (rows and the wave boundary at
# 64), a 15-run inside the row 80..95, a 17-run over 250..266 (the 256-pair block); singletons everywhere else below 267
RUN_LAYOUT = ((5, 16), (21, 2), (40, 40), (80, 15), (250, 17))
RUN_END = 267


def pairs_of_hits(hits):
    """ops.actor_pairs on the host: every (sample, containing actor) in (sample, slot) order"""
    n, s = np.nonzero(hits >= 0)
    return n.astype(np.int64), hits[n, s].astype(np.int32)


def designed_pairs(sc, total=1500, tail_random=False):
    """-> sample_idx [P] int64, actor_idx [P] int32: RUN_LAYOUT's runs of equal (actor, bracket) among singletons, then the
    scene's own pairs in production order (hits64's table), cycled up to `total`.  tail_random: random (sample, actor) pairs
    behind the runs instead, most of them far outside their box (the contracted branch)"""
    R, S = sc["starts"].shape
    A = sc["positions"].shape[1]
    left, right, _ = brackets(sc["timestamps"], sc["times"])
    br = left * 16 + right
    common = np.bincount(br).argmax()  # the bracket most rays fall into
    rays_in = np.nonzero(br == common)[0]
    pool = (rays_in[:, None] * S + np.arange(S)[None]).reshape(-1)  # consecutive samples of rays of one bracket
    assert len(pool) >= 40
    si = (np.arange(RUN_END, dtype=np.int64) * 7) % (R * S)
    ai = (np.arange(RUN_END) % 2 + 2 * ((np.arange(RUN_END) // 2) % (A // 2))).astype(np.int32)  # neighbours differ
    for n, (p, ln) in enumerate(RUN_LAYOUT):
        si[p:p + ln], ai[p:p + ln] = pool[:ln], (3 + 2 * n) % A
        for e in (p - 1, p + ln):  # the singletons next to a run do not extend it
            if 0 <= e < RUN_END and ai[e] == ai[p]:
                ai[e] = (ai[p] + 1) % A
    if tail_random:
        rng = np.random.default_rng(77)
        psi, pai = rng.integers(0, R * S, total).astype(np.int64), rng.integers(0, A, total).astype(np.int32)
    else:
        psi, pai = pairs_of_hits(hits_table(hits64(sc)["inside"].reshape(R * S, A)))
    assert len(psi) > 0
    reps = -(-(total - RUN_END) // len(psi))
    si = np.concatenate([si] + [psi] * reps)[:total]
    ai = np.concatenate([ai] + [pai] * reps)[:total]
    return np.ascontiguousarray(si), np.ascontiguousarray(ai)


def run_lengths(sc, si, ai):
    """-> (start, length) of the maximal runs of equal (actor, left, right) among consecutive pairs"""
    S = sc["starts"].shape[1]
    left, right, _ = brackets(sc["timestamps"], sc["times"])
    ray = si // S
    key = (ai.astype(np.int64) * 64 + left[ray]) * 64 + right[ray]
    cut = np.concatenate([[0], np.nonzero(np.diff(key) != 0)[0] + 1, [len(key)]])
    return cut[:-1], np.diff(cut)


def pair_case(sc, si, ai, flip, seed):
    """float64 autograd of the pair chain with grad_edge_refs' sums of |terms| (A_*: what one pair's own arithmetic adds up,
    summed over the pairs of a slot) -> its dict, plus gx, gs and S_dpos / S_drot / S_go / S_gd: the sum of the magnitudes
    of the per-pair contributions to a slot, which is what the DPP merges and the atomics add up.  The per-pair
    contributions come from the same chain with every pair on a pose column and a ray of its own."""
    from grad_edge_refs import actor_pair_grads64

    rng = np.random.default_rng(seed)
    P, S = len(si), sc["starts"].shape[1]
    gx, gs = rng.normal(size=(P, 3)).astype(f32), rng.normal(size=P).astype(f32)
    a = dict(positions=sc["positions"], rotations_6d=sc["rotations_6d"], timestamps=sc["timestamps"], scale=sc["scale"])
    ref = actor_pair_grads64(a, sc["o"], sc["d"], sc["area"], sc["starts"], sc["ends"], sc["times"], si, ai, flip, gx, gs)
    ray, smp = si // S, si % S
    own = dict(a, positions=sc["positions"][:, ai], rotations_6d=sc["rotations_6d"][:, ai])
    per = actor_pair_grads64(own, sc["o"][ray], sc["d"][ray], sc["area"][ray], sc["starts"][ray, smp][:, None],
                             sc["ends"][ray, smp][:, None], sc["times"][ray], np.arange(P, dtype=np.int64),
                             np.arange(P, dtype=np.int32), None if flip is None else flip[ray], gx, gs)
    for key in ("dpos", "drot"):
        acc = np.zeros_like(ref[key])
        for t in range(acc.shape[0]):
            np.add.at(acc[t], ai, np.abs(per[key][t]))
        ref["S_" + key] = acc
    for key in ("go", "gd"):
        acc = np.zeros_like(ref[key])
        np.add.at(acc, ray, np.abs(per[key]))
        ref["S_" + key] = acc
    # grad_edge_refs' A_drot of a pair is 4 |gpos|_1 (M + 1), M = |mean|_1 + |t_left|_1: the size of what v = mean - t is made
    # of.  Only v's own roundings act on that size; the chain behind v acts on |v|_1 + 1.  Av: A_drot with |v|_1 for M.
    _, t, left, _, _, _, _ = frames64(sc, sc["times"][ray], ai)
    mean = sample_means64(sc).reshape(-1, 3)[si]
    M = np.abs(mean).sum(-1) + np.abs(sc["positions"].astype(f64)[left, ai]).sum(-1)
    share = (np.abs(mean - t).sum(-1) + 1.0) / (M + 1.0)
    acc = np.zeros_like(ref["drot"])
    for k in range(acc.shape[0]):
        np.add.at(acc[k], ai, per["A_drot"][k] * share[:, None])
    ref["Av_drot"] = acc
    ref["gx"], ref["gs"] = gx, gs
    return ref


def pair_grad_bound(ref, key, dpp=4):
    """|got - ref| <= U (|ref| + 60 A + (n + dpp) S): one pair's chain is tests/test_gpu_position_grad_precision.py's 58
    roundings on its own sum of |terms| A (60: the two spare cover the fp32 output and the lerp weight's own rounding);
    the n contributions of a slot then meet in `dpp` levels of DPP merges and n - 1 atomic sums, in any order, each a
    rounding on the sum S of the contributions' magnitudes.  drot: A is the size of mean and t, which only the roundings
    that make v = mean - t see (the sample's t 3, d t and o + . 2, the lerp of t 3 of its 7 on |t|, the difference 1: 8);
    the other 52 act on Av, the same sum with |v|_1 in the place of |mean|_1 + |t|_1 -- 60 Av + 8 A."""
    n = ref["n_slot"][..., None] if key in ("dpos", "drot") else ref["n_ray"][:, None]
    own = 60 * ref["Av_drot"] + 8 * ref["A_drot"] if key == "drot" else 60 * ref["A_" + key]
    return U * (np.abs(ref[key]) + own + (n + dpp) * ref["S_" + key]), n


def pair_forward_bounds(sc, si, ai, ref):
    """per element bounds of x01 [P,3] and cstd [P].  The box position carries C_POS U kappa (tmag + |mean|_1);
    the contraction (/ scale, 1 / cm, 2 - ., m / cm, k *, + 2, / 4: 7, C_X01 = 8, on values <= 2) has a slope <= 1 in m, and
    x01 = (m' + 2) / 4.  cstd: (area t^2 dist)^(1/3) through v_log_f32 / v_exp_f32 (1 ulp each on log2's ~20: 8 U relative
    after the third) twice (the std, the contraction's cube root, squared: 3 x 8), the products around them 12, the position
    through d q / d mag <= 2 q: C_CSTD = 64 relative, plus 2 cstd / scale per unit of the position's error."""
    S = sc["starts"].shape[1]
    ray = si // S
    _, _, _, _, _, kappa, tmag = frames64(sc, sc["times"][ray], ai)
    mean = sample_means64(sc).reshape(-1, 3)[si]
    epos = C_POS * U * kappa * (tmag + np.abs(mean).sum(-1))
    bx = (epos / sc["scale"] / 4 + C_X01 * U)[:, None] * np.ones((1, 3))
    bs = np.abs(ref["cstd"]) * (C_CSTD * U + 2 * epos / sc["scale"])
    return bx, bs


# ---- the density splice --------------------------------------------------------------------------------------------------
class _TruncExp64(torch.autograd.Function):  # field_components/activations.py:28-41
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        return g * torch.exp(ctx.saved_tensors[0].clamp(-15, 15))


def splice_case(P, la, seed, N=None):
    """-> dens [N], rows [P,la], w [la], idx [P] int64, winner [P] bool, g_out [N]: samples with one winner and 0, 1 or 2
    shadowed pairs in front of it ((sample, slot) order: the winner is a sample's last pair), samples without pairs, logits
    inside and beyond +-15 (every 7th sample's rows are scaled up)"""
    rng = np.random.default_rng(seed)
    idx, winner, s = [], [], 0
    while len(idx) < P:
        s += int(rng.integers(1, 3))  # a gap of samples without pairs now and then
        n = min(int(rng.integers(1, 4)), P - len(idx))
        idx += [s] * n
        winner += [False] * (n - 1) + [True]
    N = s + 3 if N is None else N
    idx, winner = np.array(idx, np.int64), np.array(winner, bool)
    rows = rng.normal(size=(P, la)).astype(f32)
    w = rng.normal(size=la).astype(f32)
    rows[idx % 7 == 0] *= f32(12.0)
    logit = np.abs((rows.astype(f64) * w.astype(f64)).sum(-1))
    rows = (rows * np.minimum(1.0, 40.0 / np.maximum(logit, 1e-30))[:, None]).astype(f32)  # |logit| <= 40: exp stays finite
    return dict(dens=rng.uniform(0.1, 3.0, N).astype(f32), rows=rows, w=w, idx=idx, winner=winner,
                g_out=rng.normal(size=N).astype(f32))


def splice64(c):
    """The reference's features[ray, sample] = actor rows; density = trunc_exp(decoder(features)) (neurad_field.py:208-213,
    neurad_encoding.py:184-185) in float64 autograd: the merged row is the winner's, index_put's backward hands its gradient
    to every duplicate, so each shadowed row enters as (shadow - shadow.detach()).  -> logit [P], density [N], g_dens [N],
    g_rows [P,la], g_w [la], and the magnitudes: A_w [la] = sum over winners |go| exp(clamp) |row_k|, A_rows [P,la], and
    A_logit [P] = sum_k |row_k w_k|"""
    T = lambda x: torch.from_numpy(np.asarray(x, f64))  # noqa: E731
    dens, rows, w = T(c["dens"]).requires_grad_(True), T(c["rows"]).requires_grad_(True), T(c["w"]).requires_grad_(True)
    idx, win = torch.from_numpy(c["idx"]), torch.from_numpy(c["winner"])
    N, la = dens.shape[0], rows.shape[1]
    merged = torch.zeros((N, la), dtype=torch.float64).index_add(0, idx, torch.where(win[:, None], rows, rows - rows.detach()))
    hit = torch.zeros(N, dtype=torch.bool)
    hit[idx] = True
    out = torch.where(hit, _TruncExp64.apply(merged @ w), dens)
    (out * T(c["g_out"])).sum().backward()
    logit = (rows.detach() * w.detach()).sum(-1)
    go = np.abs(c["g_out"].astype(f64))[c["idx"]]
    lw = np.zeros(N)
    lw[c["idx"][c["winner"]]] = logit.numpy()[c["winner"]]
    gl = go * np.exp(np.clip(lw[c["idx"]], -15, 15))  # |d L / d logit| of the pair's sample
    A_w = (np.where(c["winner"], gl, 0.0)[:, None] * np.abs(c["rows"].astype(f64))).sum(0)
    return dict(logit=logit.numpy(), density=out.detach().numpy(), g_dens=dens.grad.numpy(), g_rows=rows.grad.numpy(),
                g_w=w.grad.numpy(), A_w=A_w, A_rows=gl[:, None] * np.abs(c["w"].astype(f64))[None],
                A_logit=(np.abs(c["rows"].astype(f64)) * np.abs(c["w"].astype(f64))).sum(-1), hit=hit.numpy(),
                win_logit=lw, gl=gl, n_win=int(c["winner"].sum()))
