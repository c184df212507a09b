"""What the tests of the packed training route share (tests/test_gpu_render_train_packed.py): the ragged batches and field
parameters of the packed eval tests restated as a helper module, fields of any fused shape with those parameters, the
operator route the fused node replaces, and a float64 restatement of head + packed compositing (torch on the CPU, so
autograd gives the reference gradients).  No kernel code is shared."""
import functools

import numpy as np
import torch

import neurad_oracle as O
import packed_restatement as PR
import synth
from builders import field_params

FUSED_GRIDS = ((16, 2), (8, 4), (4, 8), (1, 4), (4, 2), (4, 4), (8, 2))  # fields/neurad_field.py: _FUSED_GRIDS
# first / last ray empty, consecutive empties, exact multiples of 16, one long ray (carried scan), R not a multiple of 4
RAGGED = (0, 1, 15, 16, 17, 0, 0, 31, 32, 33, 48, 2, 64, 65, 130, 1, 0, 16, 16, 5, 250, 3, 0)
LG = 11  # T = 2^11 per level: seconds per test
# (L, F, H, use_sdf, fp16 table): every fused grid, widths and heads alternating, plus one fp16 table
RAGGED_CASES = [(L, F, (32, 64)[(i + k) % 2], bool(k), False) for i, (L, F) in enumerate(FUSED_GRIDS) for k in (1, 0)] + \
    [(8, 4, 32, True, True)]
CASE_IDS = [f"{L}x{F}-H{H}-{'sdf' if s else 'density'}{'-fp16' if h else ''}" for L, F, H, s, h in RAGGED_CASES]


def params(L, F, H, use_sdf, beta=3.0, half=False):
    """field_params for any fused grid: geo layer 0 takes L * F inputs; half: the oracle sees the fp16-rounded table"""
    p = field_params(use_sdf=use_sdf, L=L, F=F, lg=LG, H=H, mn=16, mx=1024, scale=2.0 if use_sdf else 0.5)
    p.geo_b[0] = synth.linear(H, 32, 200)[1]  # this bias keeps the range of a 32-input layer whatever L * F is
    if use_sdf:
        p.beta = beta  # keeps alpha off saturation so that the compositing is exercised
    if half:
        p.grid.table = p.grid.table.astype(np.float16).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def packed_rays(counts, seed):
    """-> o [R,3], d [R,3], area [R], t_starts [M], t_ends [M], seg [R+1]: sorted, contiguous intervals inside 0.1 .. 60 m"""
    counts = np.asarray(counts, np.int64)
    R = len(counts)
    o, d, area, _ = synth.rays(R, seed)
    rng = np.random.default_rng(seed)
    ts, te = [], []
    for n in counts:
        edges = np.sort(rng.uniform(0.1, 60.0, int(n) + 1)).astype(np.float32)
        ts.append(edges[:-1]), te.append(edges[1:])
    cat = lambda parts: np.concatenate(parts).astype(np.float32) if parts else np.zeros((0,), np.float32)  # noqa: E731
    return o, d, np.asarray(area, np.float32).reshape(-1), cat(ts), cat(te), PR.segments_from_counts(counts)


def on_device(rays):
    """packed_rays -> device tensors (o, d, area, ts, te, seg int64, ray_indices int64)"""
    o, d, area, ts, te, seg = rays
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return f(o), f(d), f(area), f(ts), f(te), f(seg), f(PR.ray_indices_from_segments(seg))


def oracle_route(p, rays):
    """the numpy oracle's field on M rays of one sample, composited in float64 -> features, depth, accumulation, weights"""
    o, d, area, ts, te, seg = rays
    ri = PR.ray_indices_from_segments(seg)
    f = O.field_fwd(p, o[ri], d[ri], area[ri], ts[:, None], te[:, None])
    x = f["alpha"] if p.use_sdf else f["density"]
    feat, depth, acc, w = PR.composite(PR.f64(ts), PR.f64(te), PR.f64(x[:, 0]), PR.f64(f["feature"][:, 0]), seg, not p.use_sdf)
    return feat.numpy(), depth.numpy(), acc.numpy(), w.numpy()


class _TruncExp64(torch.autograd.Function):  # field_components/activations.py:28-41
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        return g * torch.exp(ctx.saved_tensors[0].clamp(-15, 15))


def head_composite_f64(x, beta, beta_min, ts, te, feat, seg):
    """float64 restatement of head + packed compositing.  x [M]: the geometry MLP's first output; beta: the RAW parameter
    (one element) or None for the density head.  -> alpha [M] (SDF head) or sigma [M], features [R,C], depth [R,1],
    accumulation [R,1], weights [M]"""
    if beta is None:
        head = _TruncExp64.apply(x)
    else:
        head = torch.sigmoid(-x * (beta.abs() + beta_min))
    return (head, *PR.composite(ts, te, head, feat, seg, beta is None))


def make_field(L, F, H, use_sdf, half=False, beta=3.0):
    """NeuRADField of a fused shape carrying params(L, F, H, use_sdf) -> (field, the oracle's parameters)"""
    from gpu_util import load_field_weights
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig

    cfg = NeuRADFieldConfig(use_sdf=use_sdf, geo_hidden_dim=H, nff_hidden_dim=H, sdf_beta=beta)
    st = cfg.grid.static
    st.num_levels, st.hashgrid_dim, st.base_res, st.max_res, st.log2_hashmap_size = L, F, 16, 1024, LG
    p = params(L, F, H, use_sdf, beta, half)
    return load_field_weights(NeuRADField(cfg, actors=None, static_scale=100.0).cuda(), p, half), p


def packed_samples(dev_rays):
    """the gathered packed RaySamples [M,1] the operator route evaluates (VolumetricSampler._gather's layout)"""
    from neurad_studio_amd.cameras.rays import Frustums, RaySamples

    o, d, area, ts, te, _, ri = dev_rays
    return RaySamples(frustums=Frustums(origins=o[ri], directions=d[ri], starts=ts[:, None], ends=te[:, None],
                                        pixel_area=area[ri][:, None]))


def operator_route(fld, dev_rays):
    """field.forward on the gathered packed RaySamples with fused_training = False + renderers.render_packed"""
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as FH
    from neurad_studio_amd.model_components.renderers import render_packed

    fld.fused_training = False
    rs = packed_samples(dev_rays)
    out = fld(rs)
    kw = {"alpha": out[FH.ALPHA]} if FH.ALPHA in out else {"density": out[FH.DENSITY]}
    r = render_packed(out[FH.FEATURE], rs, dev_rays[6], dev_rays[0].shape[0], **kw)
    return r["features"], r["depth"], r["accumulation"], r["weights"][:, 0]


def field_grads(fld):
    return {n: p.grad.detach().clone() for n, p in fld.named_parameters() if p.grad is not None}
