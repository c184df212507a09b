"""camera_rays_kernel, finish_camera_ray and lidar_rays_kernel (csrc/raygen.hip) restated in numpy float32, operation by
operation, and the synthetic cases the exact tests run.

Every operation is its own numpy statement on float32 arrays, so every one is rounded on its own, in the kernel's order.
The one exception is the norm of a direction, which the reference takes with torch.linalg.vector_norm: its CPU kernel
accumulates the squares as an FMA chain, sqrt(fma(z, z, fma(y, y, x * x))).  ``fma`` here rounds ONCE: the exact rational
value of a * b + c (fractions.Fraction), rounded to float32 by integer arithmetic.  A float64 evaluation cast to float32
would round twice.  tests/test_raygen_refs_host.py pins this file to the reference's own outputs (tests/golden/raygen.npz)
bit for bit; ``fused=False`` is the separately rounded norm that the kernels had before, kept as the negative control."""
from fractions import Fraction

import numpy as np

import synth

F = np.float32
EPS = F(4 * np.finfo(np.float64).eps)  # camera_utils._EPS as the float32 tensor torch.maximum sees
QUANTITIES = ("origins", "directions", "pixel_area", "directions_norm", "times")


# ---- bits --------------------------------------------------------------------------------------------------------------
def ulps(a, b):
    """distance of two float32 arrays in units of the last place, on their int32 views (negative floats mirrored, so that
    the integers are ordered like the floats and -0 sits on +0)"""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def same_bits(a, b):
    """per element: the same 32 bits, or a NaN on both sides (a NaN's sign and payload are not arithmetic: 0 / 0 is
    0xFFC00000 on one machine and 0x7FC00000 on another)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype != F:
        return a == b
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- one rounding ------------------------------------------------------------------------------------------------------
def round_f32(q: Fraction) -> np.float32:
    """the float32 nearest to the rational q, ties to even, subnormals and overflow included"""
    if q == 0:
        return F(0.0)
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()  # 2**(e-1) < q < 2**(e+1)
    if Fraction(2) ** e > q:
        e -= 1  # 2**e <= q < 2**(e+1)
    e = max(e, -126) - 23  # the unit in the last place; subnormals share the exponent of the smallest normal
    scaled = q / Fraction(2) ** e
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m & 1):
        m += 1
    if m.bit_length() + e > 128:  # 2**128 or more
        return F(sign * np.inf)
    return F(sign * np.ldexp(float(m), e))  # m < 2**25: exact in float64, and m * 2**e is a float32


def fma(a, b, c):
    """a * b + c on float32 arrays with one rounding.  A non-finite operand or an infinite product goes through float64,
    which propagates NaN and infinity the same way."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    out = np.empty(a.shape, F)
    for i in np.ndindex(a.shape):
        x, y, z = a[i], b[i], c[i]
        if np.isfinite(x) and np.isfinite(y) and np.isfinite(z):
            out[i] = round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
        else:
            with np.errstate(all="ignore"):
                out[i] = F(np.float64(x) * np.float64(y) + np.float64(z))
    return out


def clamped_norm(x, y, z, fused=True):
    """torch.maximum(torch.linalg.vector_norm((x, y, z), dim=-1), EPS): the squares accumulated as vector_norm's CPU kernel
    does, a NaN kept.  fused=False: every product and sum rounded on its own, left to right."""
    with np.errstate(all="ignore"):
        if fused:
            s = x * x
            s = fma(y, y, s)
            s = fma(z, z, s)
        else:
            xx = x * x
            yy = y * y
            zz = z * z
            s = xx + yy
            s = s + zz
        n = np.sqrt(s)
        return np.maximum(n, EPS)


def rotate(m, a, b, c):
    """m [R,12], a row-major 3x4 pose per ray: torch.sum(d[..., None, :] * R, dim=-1), products summed left to right"""
    out = []
    for r in range(3):
        p0 = a * m[:, 4 * r]
        p1 = b * m[:, 4 * r + 1]
        p2 = c * m[:, 4 * r + 2]
        s = p0 + p1
        out.append(s + p2)
    return out


# ---- the kernels -------------------------------------------------------------------------------------------------------
def camera_rays(tab, cam_idx, coords, rs_mode, fused=True):
    """camera_rays_kernel + finish_camera_ray.  tab: c2w [C,3,4], fx fy cx cy [C], times [C] | None and, for rs_mode 1-3,
    rolling_shutter_time, time_to_center_pixel [C], velocities [C,3], extent [C].  coords [R,2] = (y, x).
    -> QUANTITIES as [R,3] / [R,1] arrays (times: zeros without a times table, what the kernel writes into a times output)
    and "vectors" [3,R,3], the three directions before their normalisation."""
    c = np.asarray(cam_idx)
    R = c.shape[0]
    one = lambda k: np.asarray(tab[k], F).reshape(-1)[c]
    m = np.asarray(tab["c2w"], F).reshape(-1, 12)[c]
    y, x = np.asarray(coords, F)[:, 0], np.asarray(coords, F)[:, 1]
    fx, fy, cx, cy = one("fx"), one("fy"), one("cx"), one("cy")
    with np.errstate(all="ignore"):
        xc = x - cx
        yc = y - cy
        u0 = xc / fx
        xc1 = xc + F(1)
        u1 = xc1 / fx
        v0 = yc / fy
        v0 = -v0
        yc1 = yc + F(1)
        v1 = yc1 / fy
        v1 = -v1
        back = np.full(R, -1, F)
        d = [rotate(m, *v) for v in ((u0, v0, back), (u1, v0, back), (u0, v1, back))]
        vectors = np.stack([np.stack(v, -1) for v in d])
        n = [clamped_norm(*v, fused=fused) for v in d]
        d = [[v[k] / nv for k in range(3)] for v, nv in zip(d, n)]
        a = [d[0][k] - d[1][k] for k in range(3)]
        b = [d[0][k] - d[2][k] for k in range(3)]
        aa = [a[k] * a[k] for k in range(3)]
        bb = [b[k] * b[k] for k in range(3)]
        sa = aa[0] + aa[1]
        sa = sa + aa[2]
        sb = bb[0] + bb[1]
        sb = sb + bb[2]
        dx = np.sqrt(sa)
        dy = np.sqrt(sb)
        area = dx * dy
        o = [m[:, 3], m[:, 7], m[:, 11]]
        tm = one("times") if tab.get("times") is not None else np.zeros(R, F)
        if rs_mode:
            pos = y if rs_mode == 1 else x
            off = pos / one("extent")
            off = off - F(0.5)
            off = off * one("rolling_shutter_time")
            off = off + one("time_to_center_pixel")
            if rs_mode == 3:
                off = -off
            vel = np.asarray(tab["velocities"], F).reshape(-1, 3)[c]
            for k in range(3):
                step = vel[:, k] * off
                o[k] = o[k] + step
            tm = tm + off
    return dict(origins=np.stack(o, -1), directions=np.stack(d[0], -1), pixel_area=area[:, None],
                directions_norm=n[0][:, None], times=tm[:, None], vectors=vectors)


def lidar_rays(tab, lidar_idx, points, ego, threshold=1000.0, fused=True):
    """lidar_rays_kernel.  tab: l2w [L,3,4], hdiv vdiv [L], times [L] | None, velocities [L,3] | None.  points [R,D], D >= 3:
    xyz, intensity, the time offset in column 4; further columns are not read.
    -> QUANTITIES (directions_norm is the distance), "did_return" [R,1] uint8 and "vectors" [1,R,3]"""
    l = np.asarray(lidar_idx)
    R = l.shape[0]
    p = np.asarray(points, F)
    m = np.asarray(tab["l2w"], F).reshape(-1, 12)[l]
    with np.errstate(all="ignore"):
        w = rotate(m, p[:, 0], p[:, 1], p[:, 2])
        o = [m[:, 3], m[:, 7], m[:, 11]]
        w = [w[k] + o[k] for k in range(3)]
        dt = p[:, 4] if p.shape[1] >= 5 else np.zeros(R, F)
        if p.shape[1] >= 5 and tab.get("velocities") is not None:
            vel = np.asarray(tab["velocities"], F).reshape(-1, 3)[l]
            v = [dt * vel[:, k] for k in range(3)]
            o = [o[k] + v[k] for k in range(3)]
            if not ego:
                w = [w[k] + v[k] for k in range(3)]
        d = [w[k] - o[k] for k in range(3)]
        dist = clamped_norm(*d, fused=fused)
        direction = [d[k] / dist for k in range(3)]
        area = np.asarray(tab["hdiv"], F).reshape(-1)[l] * np.asarray(tab["vdiv"], F).reshape(-1)[l]
        tm = np.asarray(tab["times"], F).reshape(-1)[l] if tab.get("times") is not None else np.zeros(R, F)
        tm = tm + dt
        ret = (dist < F(threshold)).astype(np.uint8)
    return dict(origins=np.stack(o, -1), directions=np.stack(direction, -1), pixel_area=area[:, None],
                directions_norm=dist[:, None], times=tm[:, None], did_return=ret[:, None], vectors=np.stack(d, -1)[None])


# ---- the inputs of tests/golden/raygen.npz -----------------------------------------------------------------------------
FIXTURE_CAMERA_MODES = {"rows": 1, "cols": 2, "cols_rev": 3}


def fixture_camera(g, tag, fused=True):
    mode = FIXTURE_CAMERA_MODES[tag]
    C = g["c2w"].shape[0]
    tab = dict(c2w=g["c2w"], fx=g["fx"], fy=g["fy"], cx=g["cx"], cy=g["cy"], times=g["cam_times"],
               rolling_shutter_time=g["rolling_shutter_time"], time_to_center_pixel=g["time_to_center_pixel"],
               velocities=g["cam_velocities"], extent=np.full(C, 1080.0 if mode == 1 else 1920.0, F))
    return camera_rays(tab, g["cam_idx"], g["coords"], mode, fused=fused)


def fixture_lidar(g, ego, fused=True):
    tab = dict(l2w=g["l2w"], times=g["lidar_times"], velocities=g["lidar_velocities"], hdiv=g["hdiv"], vdiv=g["vdiv"])
    return lidar_rays(tab, g["lidar_idx"], g["points"], ego, 1000.0, fused=fused)


# ---- synthetic cases ---------------------------------------------------------------------------------------------------
def poses(n, seed):
    """[n,3,4] rigid poses: rotations from the QR of a hashed matrix, translations along a drive"""
    out = []
    for i in range(n):
        q, _ = np.linalg.qr(synth.normal((3, 3), seed + i).astype(np.float64))
        t = np.array([4.0 * i, 0.3 * i, 1.6]) + synth.normal((3,), seed + 100 + i) * 0.1
        out.append(np.concatenate([q, t[:, None]], 1))
    return np.stack(out).astype(F)


# cameras of camera_case: plain, rotation block * 1e-3, * 1e3, zero rotation block, one NaN entry, plain
CAM_SMALL, CAM_LARGE, CAM_ZERO, CAM_NAN = 1, 2, 3, 4


def camera_case(R, seed=0, nan_pose=True):
    """-> (tab, cam_idx [R], coords [R,2]) for six cameras, the camera varying from ray to ray.  Coordinates cycle through
    half-integers, negative values, the principal point of the ray's camera (u = v = 0) and 1e6.  nan_pose=False puts a
    finite number where the NaN is: the rays of the other cameras must not notice."""
    C = 6
    c2w = poses(C, 10 + seed)
    c2w[CAM_SMALL, :, :3] *= F(1e-3)  # norms far from 1: the two roundings of the norm then differ on many rays
    c2w[CAM_LARGE, :, :3] *= F(1e3)
    c2w[CAM_ZERO, :, :3] = 0.0
    c2w[CAM_NAN, 0, 0] = np.nan if nan_pose else 0.25
    tab = dict(c2w=c2w, fx=synth.uniform((C,), 1800, 2000, seed + 1), fy=synth.uniform((C,), 1800, 2000, seed + 2),
               cx=synth.uniform((C,), 940, 980, seed + 3), cy=synth.uniform((C,), 520, 560, seed + 4),
               times=synth.uniform((C,), 0, 8, seed + 5), rolling_shutter_time=synth.uniform((C,), 0.01, 0.03, seed + 6),
               time_to_center_pixel=synth.uniform((C,), -0.01, 0.01, seed + 7), velocities=synth.normal((C, 3), seed + 8) * F(5),
               extent=np.array([1080, 1920, 1080, 2168, 3848, 1080], F))
    cam_idx = synth.uniform((R,), 0, C, seed + 9).astype(np.int64).clip(0, C - 1)
    coords = np.stack([np.floor(synth.uniform((R,), 0, 1080, seed + 11)) + 0.5,
                       np.floor(synth.uniform((R,), 0, 1920, seed + 12)) + 0.5], -1).astype(F)
    kind = np.arange(R) % 8
    coords[kind == 1] = -coords[kind == 1]
    coords[kind == 2] = np.stack([tab["cy"], tab["cx"]], -1)[cam_idx[kind == 2]]
    coords[kind == 3, 0] = 1e6
    coords[kind == 5, 1] = 1e6
    return tab, cam_idx, coords


def without(tab, *keys):
    return {k: (None if k in keys else v) for k, v in tab.items()}


# rows of lidar_case with a meaning; all of them belong to lidar 0, whose pose is the identity with no translation
ROW_ORIGIN, ROW_AT_THRESHOLD, ROW_BELOW_THRESHOLD, ROW_NAN = 3, 4, 5, 7
THRESHOLD = 1000.0


def lidar_case(R, point_dim, seed=0, nan_point=True):
    """-> (tab, lidar_idx [R], points [R, point_dim]) for four lidars.  Where R allows, the rows named above hold a point at
    the sensor origin, the point (1000, 0, 0), the point one float32 below it, and a point with a NaN coordinate; their time
    offset is 0, so that the sensor does not move under them.  Column 5 holds numbers that nothing may read."""
    Ln = 4
    l2w = poses(Ln, 40 + seed)
    l2w[0] = np.eye(3, 4, dtype=F)
    tab = dict(l2w=l2w, times=synth.uniform((Ln,), 0, 8, seed + 41), velocities=synth.normal((Ln, 3), seed + 42) * F(6),
               hdiv=synth.uniform((Ln,), 1e-3, 4e-3, seed + 47), vdiv=synth.uniform((Ln,), 1e-3, 4e-3, seed + 48))
    lidar_idx = synth.uniform((R,), 0, Ln, seed + 43).astype(np.int64).clip(0, Ln - 1)
    pts = np.concatenate([synth.normal((R, 3), seed + 44) * np.array([30.0, 30.0, 2.0], F), synth.uniform((R, 1), 0, 1, seed + 45),
                          synth.uniform((R, 1), -0.05, 0.05, seed + 46), synth.uniform((R, 1), -1e6, 1e6, seed + 49)],
                         -1).astype(F)
    pts[::16, :3] *= F(60.0)  # beyond the valid-distance threshold
    special = {ROW_ORIGIN: (0.0, 0.0, 0.0), ROW_AT_THRESHOLD: (THRESHOLD, 0.0, 0.0),
               ROW_BELOW_THRESHOLD: (np.nextafter(F(THRESHOLD), F(0)), 0.0, 0.0),
               ROW_NAN: (12.5, np.nan if nan_point else -3.0, 0.75)}
    for row, xyz in special.items():
        if row < R:
            pts[row, :3], pts[row, 4], lidar_idx[row] = xyz, 0.0, 0
    return tab, lidar_idx, np.ascontiguousarray(pts[:, :point_dim])
