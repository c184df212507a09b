"""Pin the position-gradient references at the exact edges of the contraction and the feature rescale against the
REFERENCE's own fp32 autograd (tests/golden/ray_grads_edges.npz, oracle/make_golden_grad_edges.py), element by element:

  E1 |u|_inf tied on 2 or 3 axes outside the unit cube, E2 |u|_inf == 1, E3 2 scal_0 std' == 1 on an E2 sample.

The float64 derivatives of the oracle (static encoding) and of the float64 torch chain (actor pairs; the GPU tests use
both as references) must sit within the reference's own fp32 rounding of them, |ref - got| <= 2 u A + u |ref|, where A is
the float64 sum of |terms| of the element.  The wrong subgradients (whole dL/dm to the first maximal axis; no clamp
gradient at equality) must fall far outside that bound on the edge rows: the fixture really hits the edges."""
from types import SimpleNamespace

import numpy as np
import torch

import neurad_oracle as O
import synth
from conftest import load_golden

U = 2.0 ** -24
KINDS = {"control": 0, "E1": 1, "E2": 2, "E3": 3}


def edge_grid():
    return O.GridParams(synth.hash_table(8 * 2**11, 4, seed=61, scale=0.5), 8, 32, 8192, 11)


def edge_g_enc(g):
    R, S = g["starts"].shape
    return synth.normal((R * S, 32), seed=181)


def excess(got, ref, A):
    """(|got - ref| - u |ref|) / (u A): <= gamma where the bound holds"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return (np.abs(got - ref) - U * np.abs(ref)) / (U * np.maximum(A, 1e-300))


def actor_pair_grads64(a, o, d, area, starts, ends, times, sample_idx, actor_idx, flip, gx, gs, ties="split"):
    """float64 torch autograd of sum(x01 gx) + sum(cstd gs) over (sample, actor) pairs: the chain of
    test_gpu_actors.test_actor_pair_positions_kernel_vs_torch_autograd (world2box_pairs -> training flip -> contraction),
    whose amax backward splits ties as the reference's inf-norm does.  No hash cells are selected, so a float64 primal is
    a valid reference.  ties="first": the whole dL/dm to the first maximal axis (negative control).
    -> dict of dpos [Tn,A,3], drot [Tn,A,6], go, gd [R,3] and, per element, A (a sum of |terms|: exact for the
    contraction and the box transform; for rot6 an upper bound |gpos|_1 (|v|_1 + |t|_1 + 1) * 4 per pair for the
    Gram-Schmidt backward of unit-scale rows) and n (pairs summed into the element)."""
    from neurad_studio_amd.model_components.dynamic_actors import world2box_pairs

    T = lambda x: torch.from_numpy(np.asarray(x, np.float64))  # noqa: E731
    pos, rot = T(a["positions"]).requires_grad_(True), T(a["rotations_6d"]).requires_grad_(True)
    act = SimpleNamespace(actor_positions=pos, actor_rotations_6d=rot, unique_timestamps=T(a["timestamps"]))
    o_, d_ = T(o).requires_grad_(True), T(d).requires_grad_(True)
    S = np.asarray(starts).shape[1]
    si, ai = torch.from_numpy(np.asarray(sample_idx, np.int64)), torch.from_numpy(np.asarray(actor_idx, np.int64))
    ray, smp = si // S, si % S
    t0, t1 = T(starts)[ray, smp], T(ends)[ray, smp]
    dist = (t1 - t0) / 2
    t = t0 + dist
    mean = o_[ray] + d_[ray] * t[:, None]
    std = (T(area)[ray] * t.pow(2) * dist).pow(1 / 3)
    r_inv, t_inv = world2box_pairs(act, T(times)[ray], ai)
    p = (r_inv * mean[:, None, :]).sum(-1) + t_inv
    fl = T(flip)[ray] if flip is not None else torch.ones_like(t)
    p = torch.cat([p[:, :1] * fl[:, None], p[:, 1:]], dim=-1)
    scale = float(a["scale"])
    m, s = p / scale, std / scale
    if ties == "split":
        mag = m.abs().amax(dim=-1, keepdim=True)
    else:
        mag = m.abs().max(dim=-1, keepdim=True).values
    cm = mag.clamp_min(1.0)
    mc = torch.where(mag < 1, m, (2 - 1 / cm) * (m / cm))
    sc = torch.where(mag[:, 0] < 1, s, s * (((2 * cm[:, 0] - 1).pow(1 / 3) / cm[:, 0]) ** 2))
    x01, cstd = (mc + 2.0) / 4.0, sc / 4.0
    ((x01 * T(gx)).sum() + (cstd * T(gs)).sum()).backward()
    out = dict(dpos=pos.grad.numpy(), drot=rot.grad.numpy(), go=o_.grad.numpy(), gd=d_.grad.numpy(),
               x01=x01.detach().numpy(), cstd=cstd.detach().numpy())
    # ---- per element sums of |terms| ------------------------------------------------------------------------------------
    mm = m.detach().numpy()
    am = np.abs(mm)
    mg = am.max(-1)
    outside = ~(mg < 1.0)
    mo = np.where(outside, mg, 1.0)
    cr = np.cbrt(2.0 * mo - 1.0)
    ka, dka = 2.0 / mo + 1.0 / mo**2, 2.0 / mo**2 + 2.0 / mo**3
    dqa = 2.0 * (cr / mo) * ((2.0 / 3.0) / (cr * cr * mo) + cr / mo**2)
    gm = np.abs(np.asarray(gx, np.float64)) / 4.0
    sd = (std / scale).detach().numpy()
    gmag = (gm * am).sum(-1) * dka + np.abs(np.asarray(gs, np.float64)) * sd * dqa / 4.0
    tied = am == mg[:, None]
    gposa = np.where(outside[:, None], gm * ka[:, None] + tied / tied.sum(-1, keepdims=True) * gmag[:, None], gm) / scale
    ra = np.abs(r_inv.detach().numpy())                       # [P,3,3]: pos_i = sum_j r_inv[i,j] mean_j + t_inv_i
    amean = np.einsum("pij,pi->pj", ra, gposa)                # |d L/d mean| terms
    R = np.asarray(o).shape[0]
    rr, tt = ray.numpy(), t.detach().numpy()
    ao, ad, nr = np.zeros((R, 3)), np.zeros((R, 3)), np.zeros(R)
    np.add.at(ao, rr, amean), np.add.at(ad, rr, amean * np.abs(tt)[:, None]), np.add.at(nr, rr, 1)
    ts = np.asarray(a["timestamps"], np.float64)
    q = np.asarray(times, np.float64)[rr]
    right = np.searchsorted(ts, q, side="left")
    left, right = np.maximum(right - 1, 0), np.minimum(right, len(ts) - 1)
    tra = np.abs(np.asarray(a["positions"], np.float64))
    Tn, A = tra.shape[:2]
    apos, arot, ns = np.zeros((Tn, A, 3)), np.zeros((Tn, A, 6)), np.zeros((Tn, A))
    an = ai.numpy()
    intra = 4.0 * gposa.sum(-1) * (np.abs(mean.detach().numpy()).sum(-1) + tra[left, an].sum(-1) + 1.0)
    for e in (left, right):
        np.add.at(apos, (e, an), np.einsum("pij,pi->pj", ra, gposa).clip(min=0) + gposa.sum(-1, keepdims=True))
        np.add.at(arot, (e, an), intra[:, None])
        np.add.at(ns, (e, an), 1)
    out.update(A_go=ao, A_gd=ad, n_ray=nr, A_dpos=apos, A_drot=arot, n_slot=ns, tied=tied.sum(-1), outside=outside,
               mag=mg)
    return out


def actor_case(g, ties="split"):
    a = dict(positions=g["a_positions"], rotations_6d=g["a_rotations_6d"], timestamps=g["a_timestamps"],
             scale=g["a_scale"])
    S = g["a_starts"].shape[1]
    sidx = g["a_ray"].astype(np.int64) * S + g["a_sample"]
    return actor_pair_grads64(a, g["a_o"], g["a_d"], g["a_area"], g["a_starts"], g["a_ends"], g["a_times"], sidx,
                              g["a_actor"], None, g["a_gx"], g["a_gs"], ties=ties)


def test_static_edges_oracle_vs_reference_autograd():
    g = load_golden("ray_grads_edges")
    grid, sc = edge_grid(), float(g["static_scale"])
    args = (g["o"], g["d"], g["area"], g["starts"], g["ends"], edge_g_enc(g))
    go, gd, goa, gda = O.encode_static_ray_grads(grid, sc, *args, with_abs=True)
    # the edges are in the fixture, exactly
    mean, std = O.fast_isotropic_gaussian(g["o"], g["d"], g["area"], g["starts"], g["ends"])
    u = np.abs(mean / np.float32(sc))
    mag = u.max(-1)
    ties = ((u == mag[..., None]).sum(-1) >= 2) & (mag >= 1)
    k = g["kind"]
    assert ties[k == 1].all(1).sum() >= 40 and (((u == mag[..., None]).sum(-1) == 3) & (mag >= 1)).any()
    assert (mag[k >= 2] == 1).any(1).all() and not (mag[k == 0] == 1).any()
    _, cstd = O.contract_gaussian(mean, std, sc)
    a0 = (np.float32(32) * np.float32(2)) * cstd
    assert (a0[k == 3] == 1).any(1).all() and ((a0 == 1) & (mag == 1)).sum() == (k == 3).sum()
    for got, ref, A in ((go, g["enc_go"], goa), (gd, g["enc_gd"], gda)):
        assert excess(got, ref, A).max() <= 2.0, excess(got, ref, A).max()
    # the wrong subgradients are outside that bound on every edge kind they touch
    for ties_, clamp, kinds in (("first", True, (1, 2, 3)), ("split", False, (3,))):
        bo, bd = O.encode_static_ray_grads(grid, sc, *args, ties=ties_, clamp_at_one=clamp)
        for kk in kinds:
            worst = max(excess(bo, g["enc_go"], goa)[k == kk].max(), excess(bd, g["enc_gd"], gda)[k == kk].max())
            assert worst > 100.0, (ties_, clamp, kk, worst)
        assert excess(bo, g["enc_go"], goa)[k == 0].max() <= 2.0


def test_actor_edges_chain_vs_reference_autograd():
    g = load_golden("ray_grads_edges")
    out = actor_case(g)
    assert np.abs(out["x01"] - g["a_x01"]).max() < 2e-7 and np.abs(out["cstd"] / g["a_cstd"] - 1).max() < 1e-6
    assert (out["outside"] & (out["tied"] == 2)).sum() >= 10 and (out["outside"] & (out["tied"] == 3)).sum() >= 5
    assert (out["mag"] == 1).sum() >= 4
    for key, ref in (("dpos", "a_dpos"), ("drot", "a_drot"), ("go", "a_go"), ("gd", "a_gd")):
        e = excess(out[key], g[ref], out["A_" + key] if "A_" + key in out else out["A_g" + key[1]])
        assert e.max() <= 2.0 * 16, (key, e.max())
    bad = actor_case(g, ties="first")
    worst = max(excess(bad["go"], g["a_go"], out["A_go"]).max(), excess(bad["gd"], g["a_gd"], out["A_gd"]).max())
    assert worst > 1000.0, worst


def test_hashgrid_input_grads_vs_reference_autograd():
    """dL/dx of a plain HashEncoding, per element (golden field_actors_grads: the reference's autograd)"""
    g = load_golden("field_actors_grads")
    sc = O.hash_scalings(4, 64, 1024)
    gx, ga = O.hashgrid_input_grads(g["hx"], synth.hash_table(4 * 2**9, 4, seed=400, scale=0.7), sc, 2**9, g["hgy"],
                                    with_abs=True)
    assert excess(gx, g["hdx"], ga).max() <= 4.0
