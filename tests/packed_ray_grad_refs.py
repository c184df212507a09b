"""Ray gradients through PACKED samples (nrhip_encode_bwd_rays_packed): the float64 reference and the per-element bound that
tests/test_packed_ray_grads_host.py and tests/test_gpu_packed_ray_grads.py share.  No kernel code is shared.

Reference.  The oracle's analytic chain (neurad_oracle.encode_static_ray_grads, pinned to the reference's own autograd by
tests/test_oracle_golden.py and tests/test_oracle_grad_edges.py) on the gathered [M,1] "rays of one sample" gives every
sample's share of dL/d origin and dL/d direction and, with_abs, the sum A of the absolute values of the terms behind it.
Both are added per ray in float64 over the ray's segment; a ray without samples gets 0.

Bound.  The project's per-element form (tests/test_gpu_position_grad_precision.py, whose derivation this restates for the
packed kernel's sums):

    |got - ref| <= gamma u A + u |ref|        (u = 2^-24)

One sample's arithmetic is the dense kernel's op for op, so its share of gamma is that test's: trilinear derivative times g
(7), feature and level sums and the rescale weight with the cube root behind std' (F - 1 + L - 1 + 3 + ...  -> 12 + F + L in
all), the contraction backward (31), / scale and * t (2), and the 5 spare for the fp32 output rounding and the oracle's fp32
primals: 48 + F + L.  What differs is the shape of the sum over a ray's samples.  A group of G lanes owns the ray; lane
`sub` adds the samples sub, sub + G, sub + 2G, ... of the ray's segment one after the other -- the longest such sum has
ceil(n_ray / G) terms, n_ray the RAY'S OWN sample count, not a batch-wide S -- and the G partial sums are merged by an
xor-butterfly of log2 G levels, one rounding each.  So, per ray,

    gamma = 48 + F + L + ceil(n_ray / G) + log2 G

with G the group size the launch used: the forced lanes_per_ray, or for 0 the host's choice from the mean count M / R by the
dense rule (> 32 -> 64, > 16 -> 32, else 16)."""
import functools
import math

import numpy as np

import neurad_oracle as O
import packed_restatement as PR
import synth
from grad_edge_refs import excess

SCALES = (1.0, 2.0 ** 16, 2.0 ** 24)  # unscaled, and a GradScaler's 2^16 / 2^24
STATIC_SCALE = 20.0  # the ragged batches reach 60 m from origins ~N(0, 5 m): samples on both sides of the contraction


def sharp_gradients(n, width, seed, scale):
    """tests/test_gpu_position_grad_precision.py's incoming gradients, restated (tests import helper modules, not each other):
    transmittance 1e-12 .. 1 times O(1e-2 .. 1e2) -> 1e-14 .. 1e2; a tenth of the rows silent; times a loss scale"""
    T = 10.0 ** synth.uniform((n, 1), -12.0, 0.0, seed)
    mag = 10.0 ** synth.uniform((n, width), -2.0, 2.0, seed + 1)
    g = (synth.normal((n, width), seed + 2) * mag * T * scale).astype(np.float32)
    g[synth.uniform((n,), 0, 1, seed + 3) < 0.1] = 0.0
    return g


def layout(F):
    return (4 if F == 8 else 8), F  # L * F <= 32 as the fields use


@functools.lru_cache(maxsize=None)
def grid_for(F, half, seed=51):
    """L x F grid on 2^11-entry levels (packed_train_refs.LG); half: the oracle reads the fp16-rounded values"""
    L, _ = layout(F)
    t = synth.hash_table(L * 2**11, F, seed=seed, scale=0.5).astype(np.float16 if half else np.float32).astype(np.float32)
    return O.GridParams(t, L, 32, 8192, 11)


def chosen_group(M, R):
    """the group size lanes_per_ray = 0 stands for"""
    return 64 if M > 32 * R else (32 if M > 16 * R else 16)


def gamma(counts, G, L, F):
    """per ray [R,1]; G = 0: the host's choice"""
    counts = np.asarray(counts, np.int64)
    if G == 0:
        G = chosen_group(int(counts.sum()), len(counts))
    return (48 + F + L + np.ceil(counts / G) + int(math.log2(G)))[:, None]


def reference(grid, static_scale, rays, grad_enc):
    """rays = (o [R,3], d [R,3], area [R], t_starts [M], t_ends [M], seg [R+1]) as packed_train_refs.packed_rays gives them
    -> (dL/d origins, dL/d directions, A_origins, A_directions), float64 [R,3] each"""
    o, d, area, ts, te, seg = rays
    R = len(seg) - 1
    out = [np.zeros((R, 3)) for _ in range(4)]
    if len(ts):
        ri = PR.ray_indices_from_segments(seg)
        per_sample = O.encode_static_ray_grads(grid, static_scale, o[ri], d[ri], np.asarray(area)[ri], ts[:, None], te[:, None],
                                               grad_enc, with_abs=True)
        for acc, v in zip(out, per_sample):
            np.add.at(acc, ri, np.asarray(v, np.float64))
    return tuple(out)


def worst_excess(got_o, got_d, ref, gam, rows=None):
    """max over the elements (of `rows`) of excess / gamma for both outputs: <= 1 where the bound holds"""
    ref_o, ref_d, ao, ad = ref
    rows = slice(None) if rows is None else rows
    gam = np.broadcast_to(gam, ref_o.shape)
    return max((excess(got_o[rows], ref_o[rows], ao[rows]) / gam[rows]).max(initial=0.0),
               (excess(got_d[rows], ref_d[rows], ad[rows]) / gam[rows]).max(initial=0.0))


def permuted(rays, perm):
    """the batch with its rays in the order perm (segments rebuilt) -> rays, the packed sample order (new <- old)"""
    o, d, area, ts, te, seg = rays
    counts = np.diff(seg)
    take = np.concatenate([np.arange(seg[r], seg[r + 1]) for r in perm]) if len(perm) else np.zeros((0,), np.int64)
    take = take.astype(np.int64)
    return (o[perm], d[perm], np.asarray(area)[perm], ts[take], te[take], PR.segments_from_counts(counts[perm])), take


# ---- the node and the sampler: what tests/test_gpu_render_train_packed.py uses for the same purpose, restated -------------
def large_rays():
    """1500 rays of 0 .. 60 samples: M >= ops._BINNED_MIN_SAMPLES, the table gradient's partition path"""
    import packed_train_refs as T

    counts = np.random.default_rng(29).integers(0, 61, 1500)
    return T.packed_rays(tuple(int(c) for c in counts), 31)


def cotangents(R, M, seed=81):
    from gpu_util import dev

    return (dev(synth.normal((R, 32), seed)), dev(synth.normal((R, 1), seed + 1)), dev(synth.normal((R, 1), seed + 2)),
            dev(synth.normal((M,), seed + 3)))


def compare_routes(fused, operator):
    """(outputs, parameter gradients) of the node against the operator route: 2e-5 on the outputs, 2e-4 on the parameter
    gradients, 1e-3 on beta's (it sums every sample's heavily cancelling terms)"""
    from conftest import rel_l2
    from gpu_util import host64

    (fo, fg), (oo, og) = fused, operator
    for name, a, b in zip(("features", "depth", "accumulation", "weights"), fo, oo):
        err = rel_l2(host64(a).reshape(-1), host64(b).reshape(-1))
        print(f"{name}: fused vs operator rel-L2 {err:.3e}")
        assert err < 2e-5, (name, err)
    assert set(fg) == set(og), set(fg) ^ set(og)
    for n in fg:
        bound = 1e-3 if n == "sdf_to_density.beta" else 2e-4
        err = rel_l2(host64(fg[n].float()).reshape(-1), host64(og[n].float()).reshape(-1))
        print(f"d {n}: fused vs operator rel-L2 {err:.3e} (bound {bound:g})")
        assert fg[n].dtype == og[n].dtype and err < bound, (n, err)
