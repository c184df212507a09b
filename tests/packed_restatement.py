"""Float64 restatement of packed (ragged) compositing, one ray at a time: nerfacc's packed render_weight_from_density /
render_weight_from_alpha / accumulate_along_rays and their fusion, written from the formulas (no kernel code is shared).
``seg`` is int64 [R+1]: ray r owns the packed samples [seg[r], seg[r+1]).  Every function takes and returns float64 torch
tensors on the CPU, so the same code gives the forward values and -- through torch autograd -- the gradients."""
import numpy as np
import torch


def f64(a, grad=False):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def segments_from_counts(counts):
    seg = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts, np.int64), out=seg[1:])
    return seg


def ray_indices_from_segments(seg):
    seg = np.asarray(seg, np.int64)
    return np.repeat(np.arange(len(seg) - 1, dtype=np.int64), np.diff(seg))


def _rays(seg):
    seg = np.asarray(seg, np.int64)
    return [(int(seg[r]), int(seg[r + 1])) for r in range(len(seg) - 1)]


def _cat(parts, like):
    return torch.cat(parts) if parts else like.new_zeros((0,))


def weight_from_density(ts, te, sig, seg):
    """alpha_i = 1 - exp(-sigma_i delta_i), T_i = exp(-sum_{j<i} sigma_j delta_j), w_i = T_i alpha_i  -> w, T, alpha [M]"""
    w, T, A = [], [], []
    for b, e in _rays(seg):
        sd = sig[b:e] * (te[b:e] - ts[b:e])
        t = torch.exp(-(torch.cumsum(sd, 0) - sd))
        a = -torch.expm1(-sd)
        w.append(t * a), T.append(t), A.append(a)
    return _cat(w, sig), _cat(T, sig), _cat(A, sig)


def weight_from_alpha(alpha, seg):
    """T_i = prod_{j<i} (1 - alpha_j), w_i = T_i alpha_i  -> w, T [M]"""
    w, T = [], []
    for b, e in _rays(seg):
        a = alpha[b:e]
        t = torch.cumprod(torch.cat([a.new_ones(1), 1 - a[:-1]]), 0) if e > b else a
        w.append(t * a), T.append(t)
    return _cat(w, alpha), _cat(T, alpha)


def accumulate(w, v, seg):
    """out[r, c] = sum_{i in ray r} w_i v_ic  (v None: [R,1], the plain sum); zeros for a ray without samples"""
    if v is None:
        v = w.new_ones((w.shape[0], 1))
    return torch.stack([(w[b:e, None] * v[b:e]).sum(0) for b, e in _rays(seg)]) if len(seg) > 1 else v.new_zeros((0, v.shape[1]))


def composite(ts, te, x, feat, seg, density_mode):
    """the fused form -> features [R,C], depth [R,1] = sum w (ts + te) / 2, accumulation [R,1], weights [M]"""
    w = weight_from_density(ts, te, x, seg)[0] if density_mode else weight_from_alpha(x, seg)[0]
    mid = ((ts + te) / 2)[:, None]
    return accumulate(w, feat, seg), accumulate(w, mid, seg), accumulate(w, None, seg), w
