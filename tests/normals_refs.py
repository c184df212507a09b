"""Surface normals of the geometry head in numpy, restated from the oracle's existing functions (no kernel code): what
tests/test_normals_refs_host.py pins to the reference's own autograd (tests/golden/normals.npz, made by
scripts/make_golden_normals.py) and tests/test_gpu_normals.py holds csrc/normals.hip to.  The definition, the sign and the
error bound are stated in include/neurad_hip.h at nrhip_field_normals.

  g     = d geo_out / d position at the sample's gaussian mean: encode_static on [N,1] rays -> mlp_fwd(return_hidden) ->
          mlp_bwd of the unit cotangent on column 0 -> encode_static_ray_grads (the origin gradient of a one-sample ray is the
          gradient at its position), float64 on the fp32 primal.
  A     = per element, the same chain on |W0|^T (|w1[0]| mask) and |table| with every product and difference in absolute value.
  n     = +g / max(|g|, 1e-12) for an SDF, -g / max(|g|, 1e-12) in density mode (fields/base_field.py:80-101).
"""
import math

import numpy as np

import builders
import neurad_oracle as O

U = 2.0 ** -24
f32, f64 = np.float32, np.float64

# the cases of the GPU tests: name -> (L, F, H, use_sdf, R, S, fp16 table)
CASES = {
    "neurad_sdf": (8, 4, 32, True, 50, 32, False),
    "neurad_density_h64": (8, 4, 64, False, 21, 33, False),
    "c2_sdf_h64": (16, 2, 64, True, 5, 7, False),
    "tiny_1x4": (1, 4, 32, True, 13, 7, False),
    "neurad_tiny_4x2": (4, 2, 32, True, 11, 19, False),
    "neurad_fp16_table": (8, 4, 32, True, 9, 17, True),
    "one_sample": (8, 4, 64, False, 9, 1, False),
}
RAY_SEED = 7
LEFT_OUT_CAP = 0.01  # share of a case's samples a ReLU mask within rounding of zero may take out of the comparison


def case_params(name):
    """-> (oracle FieldParams, (o, d, area, starts, ends, edges)) of a case; fp16 table: the oracle sees the rounded table"""
    L, F, H, use_sdf, R, S, half = CASES[name]
    if (L, F) == (8, 4):
        p = builders.field_params(use_sdf, H=H)
    elif (L, F) == (16, 2):
        p = builders.field_params(use_sdf, 16, 2, 12, H, 16, 1024)
    elif (L, F) == (1, 4):
        p = builders.tagged_field_params("tiny", use_sdf, H)
    else:
        p = builders.tagged_field_params("neurad_tiny", use_sdf, H)
    if half:
        p.grid.table = p.grid.table.astype(np.float16).astype(f32)
    return p, builders.sample_rays(R, S, RAY_SEED)


def constant(p):
    """NRHIP_NORMALS_C(L, F, H) of include/neurad_hip.h: the kernel's first-order rounding count (not fitted to any output)"""
    return p.geo_w[0].shape[0] + p.grid.num_levels + p.grid.n_feat + 240


def per_sample_rays(o, d, area, starts, ends):
    """[R,S] samples as N = R S rays of one sample each"""
    S = np.asarray(starts).shape[1]
    rep = lambda a: np.repeat(np.asarray(a, f32), S, axis=0)  # noqa: E731
    return rep(o), rep(d), rep(area), np.asarray(starts, f32).reshape(-1, 1), np.asarray(ends, f32).reshape(-1, 1)


def restatement(p, o, d, area, starts, ends, ties="split", clamp_at_one=True):
    """-> dict of, per sample (N = R S rows in ray-major order):
    g [N,3] float64, A [N,3] float64, geo [N] float64, A_geo [N], normals [N,3] float64, left_out [N] bool (a hidden
    pre-activation within 64 u of its own |terms|: the mask is a discrete choice), enc [N, L F] fp32.
    ties / clamp_at_one: encode_static_ray_grads' wrong-subgradient control."""
    rays = per_sample_rays(o, d, area, starts, ends)
    enc = O.encode_static(p.grid, p.static_scale, *rays)
    y, hidden = O.mlp_fwd(enc, p.geo_w, p.geo_b, return_hidden=True)
    cot = np.zeros_like(y)
    cot[:, 0] = 1
    g_enc = O.mlp_bwd(hidden, p.geo_w, cot)[0]  # (rounded to fp32 by the oracle: one unit of A, see bound())
    g = O.encode_static_ray_grads(p.grid, p.static_scale, *rays, g_enc, with_abs=True, ties=ties, clamp_at_one=clamp_at_one)[0]
    w0, b0 = np.asarray(p.geo_w[0], f64), np.asarray(p.geo_b[0], f64)
    w1, b1 = np.asarray(p.geo_w[1], f64)[0], float(np.asarray(p.geo_b[1], f64)[0])
    mask = hidden[1] > 0
    g_enc_abs = (np.abs(w1)[None, :] * mask) @ np.abs(w0)
    A = O.encode_static_ray_grads(p.grid, p.static_scale, *rays, g_enc_abs, with_abs=True, ties=ties,
                                  clamp_at_one=clamp_at_one)[2]
    e64 = enc.astype(f64)
    z = e64 @ w0.T + b0
    z_terms = np.abs(e64) @ np.abs(w0).T + np.abs(b0)
    geo = np.maximum(z, 0.0) @ w1 + b1
    A_geo = z_terms @ np.abs(w1) + abs(b1)
    left_out = (np.abs(z) <= 64 * U * z_terms).any(-1)
    return dict(g=g, A=A, geo=geo, A_geo=A_geo, normals=normalise(g, p.use_sdf), left_out=left_out, enc=enc)


def normalise(g, use_sdf):
    g = np.asarray(g, f64)
    n = g / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-12)
    return n if use_sdf else -n


def bound(ref, A, c):
    """|got - ref| <= u |ref| + c u A, per element; the oracle rounds d geo / d enc to fp32 itself: one more unit of A"""
    return U * np.abs(ref) + (c + 1) * U * np.asarray(A, f64)


def normal_tolerance(g, A, c):
    """per component of the unit normal: 2 |bound|_2 / |g| + 2^-22 (the normalisation's first-order perturbation) -> [N,1]"""
    b = np.linalg.norm(bound(g, A, c), axis=-1, keepdims=True)
    return 2 * b / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-300) + 2.0 ** -22


def lanes_per_ray(samples_per_ray):
    """the kernel's group width: the power of two >= the count, in [1, 64]"""
    g = 1
    while g < 64 and g < samples_per_ray:
        g <<= 1
    return g


def ray_sum_sequential(w, n, G):
    """The kernel's fp32 order for one ray: w [S], n [S,3] fp32 -> [3] fp32.  Lane i of G adds the products w_s n_s of the
    samples i, i + G, ... in that order (samples of weight zero are skipped), then an xor butterfly: lane 0's value."""
    w, n = np.asarray(w, f32), np.asarray(n, f32)
    acc = np.zeros((G, 3), f32)
    for s in range(w.shape[0]):
        if w[s] != 0:
            acc[s % G] = acc[s % G] + (w[s] * n[s]).astype(f32)
    off = 1
    while off < G:
        acc = (acc + acc[np.arange(G) ^ off]).astype(f32)
        off <<= 1
    return acc[0]


def ray_sum_exact(w, n):
    """the exactly rounded sum of the fp32 products' exact values -> [3] float64, and the sum of their magnitudes"""
    w, n = np.asarray(w, f64), np.asarray(n, f64)
    keep = w != 0
    prod = w[keep, None] * n[keep]
    return (np.array([math.fsum(prod[:, c]) for c in range(3)]), np.abs(prod).sum(0))
