"""The saturated input families and float64 references of the compositing kernels, dense (tests/test_gpu_saturation.py)
and packed (tests/test_gpu_packed.py, section 5): sharp surfaces, alphas of exactly 1 and 1 - 2^-24, transmittance that
underflows, sigma * delta past exp's range, zero-length bins and a sky bin far away.  The references carry the per-element
error bounds the kernels are held to."""
import numpy as np
import torch

import synth

U = 2.0 ** -24  # fp32 unit roundoff
TINY = 2.0 ** -126  # fp32's smallest normal number
ONE_BELOW = np.float32(1.0 - 2.0 ** -24)  # the largest fp32 below 1
R = 13  # not a multiple of the 4 rays per workgroup
SAMPLES = [1, 16, 63, 64, 65, 130]  # one sample, one chunk, the 64-sample carry and the ragged last chunk


def f64(a):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)


def check(got, ref, bound, what):
    """per element: finite wherever the reference is, and |got - ref| <= bound"""
    got, ref, bound = (np.broadcast_to(np.asarray(v, np.float64), np.shape(got)) for v in (got, ref, bound))
    fin = np.isfinite(ref)
    bad_inf = fin & ~np.isfinite(got)
    assert not bad_inf.any(), f"{what}: non-finite where the reference is finite at {np.argwhere(bad_inf)[:5].tolist()}"
    err = np.where(fin, np.abs(got - ref), 0.0)
    over = err > bound
    if over.any():
        k = tuple(np.argwhere(over)[0])
        raise AssertionError(f"{what}: {int(over.sum())} elements off, first {k}: got {got[k]!r} want {ref[k]!r} "
                             f"bound {bound[k]!r} (max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3g})")


# ---- inputs -----------------------------------------------------------------------------------------------------------
def sharp_alphas(S, seed, R=R):
    """rays of ordinary alphas with exact 1, 1 - 2^-24 and exact 0 sprinkled in, and rays with runs of each; one ray with
    no special value at all (the path the kernels took before), one ray opaque from its first sample on"""
    a = synth.uniform((R, S), 0.0, 1.0, seed)
    pick = synth.uniform((R, S), 0.0, 1.0, seed + 1)
    a = np.where(pick < 0.06, np.float32(1.0), a)
    a = np.where((pick >= 0.06) & (pick < 0.14), ONE_BELOW, a)
    a = np.where((pick >= 0.14) & (pick < 0.24), np.float32(0.0), a)
    a = np.where((pick >= 0.24) & (pick < 0.5), a * np.float32(1e-3), a)
    lo, hi = S // 3, S // 3 + max(1, S // 4)
    a[1, lo:hi] = 1.0
    a[2, lo:hi] = ONE_BELOW
    a[3, lo:hi] = 0.0
    a[4, lo:] = ONE_BELOW  # transmittance through the subnormals to 0 without an exact zero factor
    a[5] = synth.uniform((S,), 0.0, 0.2, seed + 2)
    a[6, 0] = 1.0
    a[7, -1] = 1.0
    a[8, : S // 2] = 0.0
    a[8, S // 2] = 1.0
    return np.ascontiguousarray(a, np.float32)


def sharp_bins(S, seed, R=R):
    """(starts, ends, sigmas): sigma * delta from 1e-4 past 88 (exp underflows), zero-length bins, a sky bin at 1e10"""
    e = np.cumsum(synth.uniform((R, S + 1), 0.0, 2.0, seed), -1).astype(np.float32)
    zero = synth.uniform((R, S), 0, 1, seed + 1) < 0.15
    for s in range(S):  # zero-length bins: e[s+1] == e[s]
        e[:, s + 1] = np.where(zero[:, s], e[:, s], np.maximum(e[:, s + 1], e[:, s]))
    e[::3, -1] = 1e10  # sky
    sig = np.exp(synth.uniform((R, S), -9.0, 5.0, seed + 2)).astype(np.float32)
    big = synth.uniform((R, S), 0, 1, seed + 3) < 0.1
    sig = np.where(big, np.float32(200.0), sig)  # sigma * delta > 88 wherever delta > 0.44
    sig[1] = 1e-3
    st, en = np.ascontiguousarray(e[:, :-1]), np.ascontiguousarray(e[:, 1:])
    return st, en, np.ascontiguousarray(sig), e


# ---- float64 references -----------------------------------------------------------------------------------------------
def excl_trans(a):
    return torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), 1 - a[:, :-1]], -1), -1)


def ref_alpha(a32, gw, gt):
    """nerfacc dense render_weight_from_alpha (cumprod) in float64 autograd -> w, T, dL/dalpha, mag(dL/dalpha)"""
    a = f64(a32).requires_grad_(True)
    T = excl_trans(a)
    w = a * T
    (w * f64(gw) + T * f64(gt)).sum().backward()
    # the same with |upstream|: d/da_i sum(|gw| w + |gt| T) = |gw_i| T_i - sum_{k>i} |G_k| prod_{j<k, j!=i}(1 - a_j), so
    # |gw_i| T_i + sum_{k>i} |G_k| prod(...) = 2 |gw_i| T_i - that
    b = f64(a32).requires_grad_(True)
    Tb = excl_trans(b)
    (b * Tb * f64(np.abs(gw)) + Tb * f64(np.abs(gt))).sum().backward()
    mag = 2 * np.abs(gw) * T.detach().numpy() - b.grad.numpy()
    return w.detach().numpy(), T.detach().numpy(), a.grad.numpy(), mag


def suffix_excl(v):
    """sum_{k>i} v_k in float64, summed from the end: its rounding is relative to the suffix's own terms"""
    return np.concatenate([np.flip(np.cumsum(np.flip(v[:, 1:], -1), -1), -1), np.zeros_like(v[:, :1])], -1)


def ref_density(delta32, sig32, gw):
    """render_weight_from_density in float64 (sd = sigma * delta) -> w, T, alpha, dL/dsigma, and the per-element error
    scale of the fp32 kernels: T = exp(-(sum of sd)) carries the sum's absolute rounding (S u sum sd) as a relative
    error, alpha = 1 - exp(-sd) an absolute one (2u), and the suffix sum of the backward S u of its terms' magnitudes.
    dL/dsigma_i = delta_i (gw_i T_i e^(-sd_i) - sum_{k>i} gw_k w_k) is written out rather than taken from autograd: torch's
    float64 backward of the exclusive cumsum leaves ~2^-53 of the ray's LARGEST term in every entry, more than the
    1e-24-sized gradients behind an opaque sample that this test holds the kernels to."""
    S = sig32.shape[1]
    dl = np.asarray(delta32, np.float64)
    sd = np.asarray(sig32, np.float64) * dl
    cinn = np.cumsum(sd, -1)
    cexn = np.concatenate([np.zeros_like(sd[:, :1]), cinn[:, :-1]], -1)
    Tn = np.exp(-cexn)
    an = -np.expm1(-sd)
    w = an * Tn
    g = np.asarray(gw, np.float64)
    head = g * Tn * np.exp(-sd)
    grad = dl * (head - suffix_excl(g * w))
    ag = np.abs(g)
    e_head = ag * Tn * np.exp(-sd) * (1 + cinn)
    e_term = ag * Tn * (an * (1 + cexn) + 1.0 / (S + 4))
    gscale = 4 * (S + 4) * U * dl * (e_head + suffix_excl(e_term))
    fscale = 4 * (S + 4) * U * Tn * (1 + cexn)
    return w, Tn, an, grad, fscale, gscale
