"""Camera pose correction (csrc/pose_opt.hip, cameras/camera_optimizers.py): restatement, cases and emulation for
tests/test_camera_opt_host.py, test_gpu_camera_opt.py and the plugin tests.  No tests in here.

* ``tangent`` / ``exp_map`` / ``pose_apply``: the formula of include/neurad_hip.h in torch for any dtype, differentiable,
  written from the mathematics there (a = fl32(pose * weights); nrms = |w|^2; theta = sqrt(max(nrms, 1e-4f));
  R = sin(theta) / theta K + (1 - cos(theta)) / theta^2 K^2 + I, K v = w x v; o' = o + t, d' = R d).  The fp32 rounding of
  the weighted parameter is part of the definition, so in float64 it is applied to the exact product with a straight-through
  gradient: the float64 result is the exact value of what the kernels approximate, on the same fp32 inputs.
* ``cases()``: the smallest shapes at which the kernels can go wrong -- ray counts around one wave, one workgroup (256) and
  four of them, camera counts 1, 2 and 70, five index patterns, rotation sizes on both sides of the clamp (|w| = 1e-2), with
  and without the scaled module's weights.  An exact tie nrms == 1e-4f cannot be constructed reliably (the fp32 sum of three
  rounded squares would have to land on one particular value) and is not tested; 9.9e-3 and 1.01e-2 sit 2 % either side.
* ``emulate_sums``: passes 2-3 of the backward in int64 (numpy): per-camera max as the bits of a float, power-of-two
  scale, round to nearest, integer sums.  ``finish_autograd`` takes the sums through the chain by float64 autograd,
  ``finish_closed_form`` by the closed form the kernel evaluates.
* ``grad_bound``: the backward bound of include/neurad_hip.h.
"""
import math

import numpy as np
import torch

CLAMP = float(np.float32(1e-4))
FLT_MAX = float(np.finfo(np.float32).max)
U = 2.0 ** -24
SCALED_WEIGHTS = (1.0, 1.0, 0.01, 0.01, 0.01, 1.0)  # (the scaled module's: translation first, as the reference's code applies them)

RAY_COUNTS = (1, 63, 64, 65, 256, 257, 1025)
CAMERA_COUNTS = (1, 2, 70)
PATTERNS = ("one", "runs64", "runs100", "random", "ends")
ROTATIONS = (0.0, 1e-3, 9.9e-3, 1.01e-2, 0.1, 1.0, 3.0)


def tangent(pose, weights, dtype):
    """pose [C, 6] (fp32 values in any dtype, may require grad), weights [6] or None -> a = fl32(pose * weights) in ``dtype``"""
    p = pose.to(dtype)
    if weights is None:
        return p
    if dtype == torch.float32:
        return p * weights.to(dtype)
    exact = p * weights.to(dtype)  # 24 x 24 bits: exact in float64
    return exact + (exact.float().to(dtype) - exact).detach()


def exp_map(a):
    """a [n, 6] -> (R [n, 3, 3], t [n, 3])"""
    t, w = a[:, :3], a[:, 3:]
    nrms = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
    theta = torch.sqrt(torch.clamp(nrms, min=CLAMP))
    f1 = torch.sin(theta) / theta
    f2 = (1.0 - torch.cos(theta)) / (theta * theta)
    eye = torch.eye(3, dtype=a.dtype)
    # K_ij = -eps_ijk w_k;  K^2 = w w^T - |w|^2 I
    K = torch.stack([torch.cross(w, eye[j].expand_as(w), dim=-1) for j in range(3)], -1)
    K2 = w[:, :, None] * w[:, None, :] - nrms[:, None, None] * eye
    return f1[:, None, None] * K + f2[:, None, None] * K2 + eye, t


def pose_apply(pose, weights, idx, o, d, dtype=torch.float64):
    """-> (o', d') in ``dtype``; rays whose index is outside [0, C) pass through"""
    C = pose.shape[0]
    ok = (idx >= 0) & (idx < C)
    R, t = exp_map(tangent(pose, weights, dtype)[idx.clamp(0, max(C - 1, 0))])
    o, d = o.to(dtype), d.to(dtype)
    o2 = torch.where(ok[:, None], o + t, o)
    d2 = torch.where(ok[:, None], (R * d[:, None, :]).sum(-1), d)
    return o2, d2


def pose_grad64(pose, weights, idx, d, g_o, g_d, need_rays=False):
    """float64 autograd of the restatement: d (sum g_o . o' + g_d . d') / d pose [C, 6] (float64) -- and, with ``need_rays``, the
    gradients with respect to the incoming origins and directions"""
    p = pose.double().clone().requires_grad_(True)
    o_in = torch.zeros(len(idx), 3, dtype=torch.float64, requires_grad=need_rays)
    d_in = d.double().clone().requires_grad_(need_rays)
    o2, d2 = pose_apply(p, weights, idx, o_in, d_in)
    loss = (o2 * g_o.double()).sum() + (d2 * g_d.double()).sum()
    if need_rays:
        return torch.autograd.grad(loss, [p, o_in, d_in])
    return torch.autograd.grad(loss, [p])[0]


# ---- cases -------------------------------------------------------------------------------------------------------------------
def indices(pattern, R, C, gen):
    i = torch.arange(R)
    if pattern == "one":
        return torch.full((R,), (C - 1) // 2, dtype=torch.int64)
    if pattern == "runs64":  # aligned to waves
        return (i // 64) % C
    if pattern == "runs100":  # runs that cross wave and workgroup boundaries
        return (i // 100 + 1) % C
    if pattern == "random":
        return torch.randint(0, C, (R,), generator=gen)
    if pattern == "ends":  # cameras 0 and C - 1 used, every other one never
        return torch.where(torch.rand(R, generator=gen) < 0.5, 0, C - 1).to(torch.int64)
    raise ValueError(pattern)


def case(R, C, pattern, rotation, scaled, seed=0):
    """-> dict of CPU tensors: pose [C,6], weights [6] or None, idx [R] int64, o, d, g_o, g_d [R,3] fp32; |w| = rotation for
    every camera (after the weights), translations ~ 0.5, origins ~ 50 m, unit directions, gradients ~ 1 and ~ 30"""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * R + 13 * C + PATTERNS.index(pattern))
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    weights = torch.tensor(SCALED_WEIGHTS) if scaled else None
    pose = rn(C, 6) * 0.5
    axis = torch.nn.functional.normalize(rn(C, 3), dim=1)
    pose[:, 3:] = axis * rotation / (weights[3:] if scaled else 1.0)
    return dict(R=R, C=C, pattern=pattern, rotation=rotation, scaled=scaled, pose=pose.contiguous(), weights=weights,
                idx=indices(pattern, R, C, gen), o=rn(R, 3) * 50.0, d=torch.nn.functional.normalize(rn(R, 3), dim=1),
                g_o=rn(R, 3), g_d=rn(R, 3) * 30.0)


def case_list():
    """every ray count x every index pattern; camera counts, rotation sizes and the weights cycle through them so that each
    value meets each ray count and each pattern at least once (35 cases x 7 rotations would say no more about the kernels:
    the rotation size only enters per camera, the index pattern only per wave)"""
    out = []
    for a, R in enumerate(RAY_COUNTS):
        for b, pattern in enumerate(PATTERNS):
            k = a * len(PATTERNS) + b
            out.append((R, CAMERA_COUNTS[(a + b) % 3], pattern, ROTATIONS[(a + 3 * b) % 7], k % 2 == 1))
    # every rotation size with and without weights at the largest shape, mixed waves
    for k, rot in enumerate(ROTATIONS):
        out.append((1025, 70, "random", rot, k % 2 == 0))
        out.append((257, 2, "runs100", rot, k % 2 == 1))
    return out


def case_id(c):
    return f"R{c[0]}-C{c[1]}-{c[2]}-w{c[3]:g}-{'scaled' if c[4] else 'plain'}"


# ---- the backward's integer sums ---------------------------------------------------------------------------------------------
def bits_B(R):
    return 62 - math.ceil(math.log2(max(R, 2)))


def ray_terms(d, g_o, g_d):
    """[R, 12] float64: g_o[0..2], then g_d[i] d[j] at 3 + 3 i + j (products of two fp32: exact)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([g_o.double().numpy(), (g_d.double().numpy()[:, :, None] * d.double().numpy()[:, None, :])
                               .reshape(-1, 9)], 1)


def emulate_sums(idx, d, g_o, g_d, C):
    """-> dict: S [C, 12] float64 (the sums as the finish pass reads them), m [C] (largest finite |term|, rounded up to fp32),
    flag [C] bool, n [C] ray counts, B, q_sums [C, 12] int64"""
    R = len(idx)
    B = bits_B(R)
    idx = idx.numpy()
    terms = ray_terms(d, g_o, g_d)
    inputs = np.concatenate([d.numpy(), g_o.numpy(), g_d.numpy()], 1)
    with np.errstate(invalid="ignore"):
        amax = np.abs(terms).max(1)
        finite = np.isfinite(inputs).all(1) & (amax <= FLT_MAX)
    valid = (idx >= 0) & (idx < C)
    live = valid & finite
    up = amax[live].astype(np.float32)
    up = np.where(up.astype(np.float64) < amax[live], np.nextafter(up, np.float32(np.inf)), up)
    m = np.zeros(C, np.float32)
    np.maximum.at(m, idx[live], up)
    e = (m.view(np.int32) >> 23).astype(np.int64) - 126  # 2^e: the smallest power of two above m (2^-126 below the normals)
    q = np.rint(terms[live] * np.ldexp(1.0, B - e[idx[live]])[:, None]).astype(np.int64)
    assert np.abs(q).max(initial=0) <= 2 ** B
    q_sums = np.zeros((C, 12), np.int64)
    np.add.at(q_sums, idx[live], q)
    flag = np.zeros(C, bool)
    flag[idx[valid & ~finite]] = True
    n = np.bincount(idx[valid], minlength=C)
    return dict(S=torch.from_numpy(q_sums.astype(np.float64) * np.ldexp(1.0, e - B)[:, None]), m=torch.from_numpy(m.astype(np.float64)),
                flag=torch.from_numpy(flag), n=torch.from_numpy(n), B=B, q_sums=q_sums)


def finish_autograd(pose, weights, S, flag):
    """the per-camera sums through the chain by float64 autograd -> [C, 6] fp32 (one rounding); NaN rows where flagged"""
    p = pose.double().clone().requires_grad_(True)
    R, t = exp_map(tangent(p, weights, torch.float64))
    g = torch.autograd.grad((t * S[:, :3]).sum() + (R.reshape(-1, 9) * S[:, 3:]).sum(), [p])[0]
    g = g.float() + 0.0
    g[flag] = float("nan")
    return g


def finish_closed_form(pose, weights, S, flag):
    """the same chain as the kernel evaluates it: with A = S[3:] as a 3 x 3 matrix, u the vector with <A, K> = w . u,
    G = (f1' (w . u) + f2' (w^T A w - |w|^2 tr A)) w / theta + f1 u + f2 (A w + A^T w - 2 w tr A); f1', f2' = 0 below the clamp,
    which is decided on the fp32 nrms"""
    a32 = tangent(pose, weights, torch.float32)
    w32 = a32[:, 3:]
    clamped = ((w32[:, 0] * w32[:, 0] + w32[:, 1] * w32[:, 1]) + w32[:, 2] * w32[:, 2]) < np.float32(1e-4)
    w = w32.double()
    A = S[:, 3:].reshape(-1, 3, 3)
    n = (w * w).sum(1)
    th = torch.where(clamped, torch.full_like(n, math.sqrt(CLAMP)), n.sqrt())
    s, c = th.sin(), th.cos()
    f1, f2 = s / th, (1 - c) / (th * th)
    d1 = torch.where(clamped, torch.zeros_like(th), (th * c - s) / (th * th))
    d2 = torch.where(clamped, torch.zeros_like(th), (th * s - 2 * (1 - c)) / (th * th * th))
    u = torch.stack([A[:, 2, 1] - A[:, 1, 2], A[:, 0, 2] - A[:, 2, 0], A[:, 1, 0] - A[:, 0, 1]], -1)
    tr = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
    Aw, Atw = (A * w[:, None, :]).sum(-1), (A * w[:, :, None]).sum(-2)
    radial = (d1 * (w * u).sum(1) + d2 * ((w * Aw).sum(1) - n * tr)) / th
    G = radial[:, None] * w + f1[:, None] * u + f2[:, None] * (Aw + Atw - 2 * w * tr[:, None])
    wt = torch.ones(6, dtype=torch.float64) if weights is None else weights.double()
    g = (torch.cat([S[:, :3], G], 1) * wt).float() + 0.0
    g[flag] = float("nan")
    return g


def grad_bound(g64, n, m, B, weights):
    """|g - g64| <= 2^-22 |g64| + 16 n_c 2^-B m_c |w_k|, [C, 6] float64"""
    wt = torch.ones(6, dtype=torch.float64) if weights is None else weights.double().abs()
    return 2.0 ** -22 * g64.abs() + 16.0 * n.double()[:, None] * 2.0 ** -B * m[:, None] * wt[None]


def forward_bounds(pose, weights, idx, o, d):
    """(|o' - o'_64| <= 2 u (|o| + |t|) per element, |d' - d'_64| <= 16 u ||d||_2 per ray), float64"""
    t = tangent(pose, weights, torch.float64)[:, :3].abs()
    C = pose.shape[0]
    ok = (idx >= 0) & (idx < C)
    t = torch.where(ok[:, None], t[idx.clamp(0, C - 1)], torch.zeros(len(idx), 3, dtype=torch.float64))
    return 2 * U * (o.double().abs() + t), (16 * U * d.double().norm(dim=1))[:, None].expand(-1, 3)
