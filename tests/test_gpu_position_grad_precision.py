"""The backwards that move geometry, element by element: dL/d(origins, directions) of the static encoding
(nrhip_encode_bwd_rays), dL/dx of one hash grid and of the per-actor grids (nrhip_hashgrid_bwd_input,
nrhip_hashgrid_multi_bwd_input), and dL/d(actor trajectory, origins, directions) of the (sample, actor) pairs
(nrhip_actor_pair_positions_bwd[_rays]).  Each output element is held to a float64 reference with the primal values
(positions, cells, offsets, masks) in fp32 op for op:

    |got - ref| <= gamma u A + u |ref|        (u = 2^-24; A = float64 sum of |terms| of the element)

gamma counts the roundings on the longest path of a term through the kernel's arithmetic (each correctly rounded op one
u; a sequential sum of n terms n - 1):
  trilinear derivative  d03 = f0 - f3, (d03 oy + d12 my) oz + (...) mz, and my = 1 - oy itself: 6; times g: 1
  feature sum           F - 1 per level; level sum L - 1; sc * w and w = 1 / max(2 sc std', 1): 3, plus std's own
                        error: the kernels' cube root is exp2(log2(x) / 3) with v_log_f32 / v_exp_f32, ASSUMED within
                        2 ulp of pow(x, 1/3) (not measured here; the dq term's cbrtf the same)           -> 12 + F + L
  contraction (mag>=1)  k = 2/m - 1/m^2: 4; g_mag: dot 4, dk 5, std term with dq 12 + 2 (cube root), sum 1;
                        the tie share g_mag / count 1; k gm + share 2                                  -> 31
  ray sums              / scale 1, * t 1, ceil(S/G) samples per lane sequentially, log2 G xor-butterfly levels
so gamma = 48 + F + L + ceil(S/G) + log2 G for encode_bwd_rays (the 5 spare cover the fp32 output rounding and the
oracle's fp32 primals against the kernel's: the same ops, except the cube root above).  hashgrid_bwd_input is the first
two rows without w: gamma = 12 + F + L.  The actor pairs: contraction 31, box transform (3-term dot + translation) 4,
cross product 2, two Gram-Schmidt backwards of unit rows 10 each, lerp weight 1 -> 58; each trajectory slot and each ray
then adds its pairs in atomics (any order): n - 1, plus 4 DPP merge levels; gamma = 64 + n.  For the trajectory
elements A is an upper bound of the Gram-Schmidt terms (test_oracle_grad_edges.actor_pair_grads64).

The incoming gradients are a trained scene's: 1e-14 .. 1e2 in one batch, a tenth of the rows exactly zero, unscaled and
times a GradScaler's 2^16 / 2^24.  The edge rows of tests/golden/ray_grads_edges.npz (E1 ties of |u|_inf, E2 |u|_inf == 1,
E3 2 scal std' == 1) are checked against the reference's autograd and the oracle; the wrong subgradients (first-axis
ties, strict clamp) are asserted to fall outside the bound there."""
import math

import numpy as np
import pytest
import torch

import neurad_oracle as O
import synth
from conftest import load_golden
from gpu_util import dev, host64_via32
from gpu_util import ops  # noqa: F401  (fixture)
from grad_edge_refs import actor_case, actor_pair_grads64, edge_g_enc, edge_grid, excess

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SCALES = (1.0, 2.0 ** 16, 2.0 ** 24)


def sharp_gradients(n, width, seed, scale):
    """transmittance 1e-12 .. 1 times O(1e-2 .. 1e2) -> 1e-14 .. 1e2; a tenth of the rows silent; times a loss scale"""
    T = 10.0 ** synth.uniform((n, 1), -12.0, 0.0, seed)
    mag = 10.0 ** synth.uniform((n, width), -2.0, 2.0, seed + 1)
    g = (synth.normal((n, width), seed + 2) * mag * T * scale).astype(np.float32)
    g[synth.uniform((n,), 0, 1, seed + 3) < 0.1] = 0.0
    return g


def gamma_rays(S, L, F):
    G = 64 if S > 32 else (32 if S > 16 else 16)
    return 48 + F + L + math.ceil(S / G) + int(math.log2(G))


def layout(F):
    return (4 if F == 8 else 8), F  # L * F <= 32 as the fields use


def grid_for(F, dtype, seed=51):
    L, _ = layout(F)
    t = synth.hash_table(L * 2**11, F, seed=seed, scale=0.5).astype(dtype).astype(np.float32)
    return O.GridParams(t, L, 32, 8192, 11)


def run_rays(ops, grid, scale, o, d, area, st, en, ge, tdt):
    spec = ops.GridSpec(grid.num_levels, grid.n_feat, grid.log2_hashmap_size, grid.min_res, grid.max_res)
    go, gd = ops.encode_bwd_rays(spec, dev(grid.table).to(tdt), scale, dev(o), dev(d), dev(area), dev(st), dev(en),
                                 dev(ge))
    return host64_via32(go), host64_via32(gd)


@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("S", [1, 7, 15, 16, 17, 33, 63, 64, 65, 128, 130])
def test_encode_bwd_rays_per_element(ops, S, F):
    """every lanes-per-ray group (16 / 32 / 64) and its ragged ends, F = 1 (proposal) .. 8, fp32 and fp16-storage
    tables (the reference reads the fp16-rounded values), gradients over 16 decades and at GradScaler scales"""
    R = 41
    o, d, area, _ = synth.rays(R, 7 + S)
    _, eu, _ = O.power_sampler(np.zeros(R), np.full(R, 3000.0, np.float32), S)
    st, en = eu[:, :-1].copy(), eu[:, 1:].copy()
    L, _ = layout(F)
    gam = gamma_rays(S, L, F)
    for dtype, tdt in ((np.float32, torch.float32), (np.float16, torch.float16)):
        grid = grid_for(F, dtype)
        for k, sc in enumerate(SCALES):
            ge = sharp_gradients(R * S, L * F, 100 * S + 10 * F + k, sc)
            ref_o, ref_d, ao, ad = O.encode_static_ray_grads(grid, 100.0, o, d, area, st, en, ge, with_abs=True)
            go, gd = run_rays(ops, grid, 100.0, o, d, area, st, en, ge, tdt)
            for got, ref, A, name in ((go, ref_o, ao, "o"), (gd, ref_d, ad, "d")):
                e = excess(got, ref, A)
                assert np.isfinite(got).all() and e.max() <= gam, (name, dtype.__name__, sc, e.max(), gam)


@pytest.mark.parametrize("S", [7, 64, 130])
def test_encode_bwd_rays_non_finite_row_stays_in_its_ray(ops, S):
    """a NaN or inf in one sample's row makes that ray's gradient non-finite and leaves every other ray in its bound"""
    R, F = 23, 4
    o, d, area, _ = synth.rays(R, 3)
    _, eu, _ = O.power_sampler(np.zeros(R), np.full(R, 3000.0, np.float32), S)
    st, en = eu[:, :-1].copy(), eu[:, 1:].copy()
    grid = grid_for(F, np.float32)
    ge = sharp_gradients(R * S, 32, 77, 1.0)
    ref_o, ref_d, ao, ad = O.encode_static_ray_grads(grid, 100.0, o, d, area, st, en, ge, with_abs=True)
    for bad, ray in ((np.nan, 5), (np.inf, 17)):
        gb = ge.copy()
        gb[ray * S + S // 2, 3] = bad
        go, gd = run_rays(ops, grid, 100.0, o, d, area, st, en, gb, torch.float32)
        others = np.arange(R) != ray
        assert not np.isfinite(go[ray]).all() and not np.isfinite(gd[ray]).all()
        assert np.isfinite(go[others]).all() and np.isfinite(gd[others]).all()
        gam = gamma_rays(S, 8, F)
        assert excess(go[others], ref_o[others], ao[others]).max() <= gam
        assert excess(gd[others], ref_d[others], ad[others]).max() <= gam


def test_encode_bwd_rays_edges(ops):
    """E1-E3 rows of the fixture: the kernel against the reference's autograd and the float64 oracle; the wrong
    subgradients are outside the bound on those rows"""
    g = load_golden("ray_grads_edges")
    grid, sc = edge_grid(), float(g["static_scale"])
    args = (g["o"], g["d"], g["area"], g["starts"], g["ends"])
    ge = edge_g_enc(g)
    ref_o, ref_d, ao, ad = O.encode_static_ray_grads(grid, sc, *args, ge, with_abs=True)
    S = g["starts"].shape[1]
    gam = gamma_rays(S, 8, 4)
    k = g["kind"]
    for tdt in (torch.float32, torch.float16):
        if tdt == torch.float16:
            grid = O.GridParams(grid.table.astype(np.float16).astype(np.float32), 8, 32, 8192, 11)
            ref_o, ref_d, ao, ad = O.encode_static_ray_grads(grid, sc, *args, ge, with_abs=True)
        go, gd = run_rays(ops, grid, sc, *args, ge, tdt)
        for got, ref, A in ((go, ref_o, ao), (gd, ref_d, ad)):
            assert excess(got, ref, A).max() <= gam, excess(got, ref, A).max()
        if tdt == torch.float32:  # the fixture was made with the fp32 table
            for got, ref, A in ((go, g["enc_go"], ao), (gd, g["enc_gd"], ad)):
                assert excess(got, ref, A).max() <= gam + 2, excess(got, ref, A).max()
    for ties, clamp, kinds in (("first", True, (1, 2, 3)), ("split", False, (3,))):
        bo, bd = O.encode_static_ray_grads(grid, sc, *args, ge, ties=ties, clamp_at_one=clamp)
        for kk in kinds:
            worst = max(excess(bo, ref_o, ao)[k == kk].max(), excess(bd, ref_d, ad)[k == kk].max())
            assert worst > 10 * gam, (ties, clamp, kk, worst)


@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("half", [False, True])
def test_hashgrid_bwd_input_per_element(ops, F, half):
    L, _ = layout(F)
    n = 3000
    grid = grid_for(F, np.float16 if half else np.float32, seed=71)
    x = synth.uniform((n, 3), 0.0, 1.0, 5 + F)
    x[:8] = np.array([0.0, 0.5, 1.0 - 2**-24, 0.25], np.float32)[np.arange(24) % 4].reshape(8, 3)  # cell corners
    spec = ops.GridSpec(L, F, 11, 32, 8192)
    tab = dev(grid.table).to(torch.float16 if half else torch.float32)
    for k, sc in enumerate(SCALES):
        go = sharp_gradients(n, L * F, 300 + k, sc)
        ref, A = O.hashgrid_input_grads(x, grid.table, grid.scalings, 2**11, go, with_abs=True)
        got = host64_via32(ops.hashgrid_bwd_input(spec, tab, dev(x), dev(go)))
        assert excess(got, ref, A).max() <= 12 + F + L, (sc, excess(got, ref, A).max())


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_hashgrid_multi_bwd_input_per_element(ops, order):
    """several actor grids (one of them touched by no row), grid ids sorted and shuffled; only valid ids (the kernel
    reads tables[grid_id[i]] unchecked)"""
    L, F, lg, n, G = 4, 4, 9, 2500, 5
    tabs = [synth.hash_table(L * 2**lg, F, seed=500 + i, scale=0.7) for i in range(G)]
    ids = (np.arange(n) * G // n).astype(np.int32)
    ids[ids == 3] = 2                                  # grid 3: no row
    if order == "shuffled":
        ids = ids[np.argsort(synth.uniform((n,), 0, 1, 9))]
    assert ids.min() >= 0 and ids.max() < G and not (ids == 3).any()
    x = synth.uniform((n, 3), 0.0, 1.0, 11)
    spec = ops.GridSpec(L, F, lg, 64, 1024)
    scal = O.hash_scalings(L, 64, 1024)
    for k, sc in enumerate(SCALES):
        go = sharp_gradients(n, L * F, 400 + k, sc)
        ref, A = np.zeros((n, 3)), np.zeros((n, 3))
        for i in range(G):
            m = ids == i
            if m.any():
                ref[m], A[m] = O.hashgrid_input_grads(x[m], tabs[i], scal, 2**lg, go[m], with_abs=True)
        got = host64_via32(ops.hashgrid_multi_bwd_input(spec, [dev(t) for t in tabs], dev(ids, torch.int32), dev(x), dev(go)))
        assert excess(got, ref, A).max() <= 12 + F + L, (sc, excess(got, ref, A).max())


@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_hashgrid_multi_bwd_input_every_feature_width_and_storage_type(ops, F, half):
    """the kernel is picked by (F, storage type): the smallest shape that separates the instantiations, same bound"""
    L, lg, n, G = 2, 8, 257, 3
    tabs = [synth.hash_table(L * 2**lg, F, seed=520 + 10 * F + i, scale=0.7) for i in range(G)]
    if half:
        tabs = [t.astype(np.float16).astype(np.float32) for t in tabs]
    ids = (np.arange(n) % G).astype(np.int32)
    x = synth.uniform((n, 3), 0.0, 1.0, 13 + F)
    spec = ops.GridSpec(L, F, lg, 16, 64)
    scal = O.hash_scalings(L, 16, 64)
    go = sharp_gradients(n, L * F, 450 + F, 1.0)
    ref, A = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(G):
        m = ids == i
        ref[m], A[m] = O.hashgrid_input_grads(x[m], tabs[i], scal, 2**lg, go[m], with_abs=True)
    dtabs = [dev(t).to(torch.float16 if half else torch.float32) for t in tabs]
    got = host64_via32(ops.hashgrid_multi_bwd_input(spec, dtabs, dev(ids, torch.int32), dev(x), dev(go)))
    assert excess(got, ref, A).max() <= 12 + F + L, excess(got, ref, A).max()


def _actor_spec(ops, a, A):
    tabs = [torch.zeros((4 * 2**9, 4), device="cuda") for _ in range(A)]
    return ops.ActorSpec(timestamps=dev(a["timestamps"]), positions=dev(a["positions"]),
                         rotations_6d=dev(a["rotations_6d"]), present=torch.ones(a["positions"].shape[:2], dtype=torch.bool,
                                                                                 device="cuda"),
                         bounds=torch.full((A, 3), 100.0, device="cuda"), grid=ops.GridSpec(4, 4, 9, 64, 1024),
                         tables=tabs, actor_scale=float(a["scale"]))


def _run_pairs(ops, a, A, o, d, area, st, en, times, sidx, aidx, flip, gx, gs):
    spec = _actor_spec(ops, a, A)
    gp, gr, go, gd = ops.actor_pair_positions_bwd(spec, dev(o), dev(d), dev(area), dev(st), dev(en), dev(times),
                                                  dev(sidx, torch.int64), dev(aidx, torch.int32),
                                                  None if flip is None else dev(flip), dev(gx), dev(gs), ray_grads=True)
    gp2, gr2 = ops.actor_pair_positions_bwd(spec, dev(o), dev(d), dev(area), dev(st), dev(en), dev(times),
                                            dev(sidx, torch.int64), dev(aidx, torch.int32),
                                            None if flip is None else dev(flip), dev(gx), dev(gs))
    return dict(dpos=host64_via32(gp), drot=host64_via32(gr), go=host64_via32(go), gd=host64_via32(gd),
                dpos2=host64_via32(gp2), drot2=host64_via32(gr2))


@pytest.mark.parametrize("n_pairs", [1, 15, 16, 17, 1023, 1025])
def test_actor_pair_positions_bwd_per_element(ops, n_pairs):
    """random trajectories (interpolated between poses), training flip on some rays, runs of equal (pose, actor) slots
    for the 16-lane merges and a ragged tail; each actor owns a few pairs so the trajectory sums stay short"""
    R, S, Tn = 64, 24, 4
    A = max(1, n_pairs // 4)
    o, d, area, _ = synth.rays(R, 21)
    _, eu, _ = O.power_sampler(np.zeros(R), np.full(R, 60.0, np.float32), S)
    st, en = eu[:, :-1].copy(), eu[:, 1:].copy()
    times = synth.uniform((R,), -0.2, 3.2, 22)
    ts = np.array([0.0, 1.0, 2.0, 3.0], np.float32)
    rot = synth.normal((Tn, A, 6), 23)
    pos = synth.normal((Tn, A, 3), 24) * np.float32(4.0)
    a = dict(timestamps=ts, positions=pos, rotations_6d=rot, scale=np.float32(1.5))
    sidx = np.sort((synth.uniform((n_pairs,), 0, 1, 25) * R * S).astype(np.int64))
    aidx = ((np.arange(n_pairs) // 4) % A).astype(np.int32)
    flip = np.where(synth.uniform((R,), 0, 1, 26) < 0.3, -1.0, 1.0).astype(np.float32)
    gx, gs = synth.normal((n_pairs, 3), 27), synth.normal((n_pairs,), 28)
    ref = actor_pair_grads64(a, o, d, area, st, en, times, sidx, aidx, flip, gx, gs)
    got = _run_pairs(ops, a, A, o, d, area, st, en, times, sidx, aidx, flip, gx, gs)
    assert ref["outside"].any() and (n_pairs < 16 or (flip[sidx // S] < 0).any())
    for key, n in (("dpos", ref["n_slot"][..., None]), ("drot", ref["n_slot"][..., None]), ("go", ref["n_ray"][:, None]),
                   ("gd", ref["n_ray"][:, None])):
        A_ = ref["A_" + key] if key in ("dpos", "drot") else ref["A_" + key]
        e = excess(got[key], ref[key], A_) - n
        assert e.max() <= 64, (key, e.max())
    for key in ("dpos", "drot"):  # without the ray gradients: the same trajectory gradients
        assert excess(got[key + "2"], ref[key], ref["A_" + key]).max() - ref["n_slot"].max() <= 64


def test_actor_pair_positions_bwd_many_pairs_per_actor(ops):
    """one long sum: 3 actors own 4096 pairs; n u A with n the slot's pair count"""
    R, S, n_pairs, A = 128, 32, 4096, 3
    o, d, area, _ = synth.rays(R, 31)
    _, eu, _ = O.power_sampler(np.zeros(R), np.full(R, 60.0, np.float32), S)
    st, en = eu[:, :-1].copy(), eu[:, 1:].copy()
    times = synth.uniform((R,), 0.0, 2.0, 32)
    a = dict(timestamps=np.array([0.0, 1.0, 2.0], np.float32), positions=synth.normal((3, A, 3), 33) * np.float32(4.0),
             rotations_6d=synth.normal((3, A, 6), 34), scale=np.float32(2.0))
    sidx = np.sort((synth.uniform((n_pairs,), 0, 1, 35) * R * S).astype(np.int64))
    aidx = (sidx // S % A).astype(np.int32)
    gx, gs = synth.normal((n_pairs, 3), 36), synth.normal((n_pairs,), 37)
    ref = actor_pair_grads64(a, o, d, area, st, en, times, sidx, aidx, None, gx, gs)
    got = _run_pairs(ops, a, A, o, d, area, st, en, times, sidx, aidx, None, gx, gs)
    for key in ("dpos", "drot"):
        assert (excess(got[key], ref[key], ref["A_" + key]) / (64 + ref["n_slot"][..., None])).max() <= 1.0, key


def test_actor_pair_positions_bwd_edges(ops):
    """box-frame E1 ties (2 and 3 axes, identity and 90-degree-yaw boxes) and E2 faces of the fixture: against the
    reference's autograd and the float64 chain; first-axis ties fall outside the bound"""
    g = load_golden("ray_grads_edges")
    ref = actor_case(g)
    a = dict(positions=g["a_positions"], rotations_6d=g["a_rotations_6d"], timestamps=g["a_timestamps"], scale=g["a_scale"])
    S = g["a_starts"].shape[1]
    sidx = g["a_ray"].astype(np.int64) * S + g["a_sample"]
    got = _run_pairs(ops, a, a["positions"].shape[1], g["a_o"], g["a_d"], g["a_area"], g["a_starts"], g["a_ends"],
                     g["a_times"], sidx, g["a_actor"].astype(np.int32), None, g["a_gx"], g["a_gs"])
    for key, fx in (("dpos", "a_dpos"), ("drot", "a_drot"), ("go", "a_go"), ("gd", "a_gd")):
        n = ref["n_slot"][..., None] if key in ("dpos", "drot") else ref["n_ray"][:, None]
        assert (excess(got[key], ref[key], ref["A_" + key]) - n).max() <= 64, key
        assert (excess(got[key], g[fx], ref["A_" + key]) - n).max() <= 64 + 32, key
    bad = actor_case(g, ties="first")
    worst = max(excess(bad["go"], ref["go"], ref["A_go"]).max(), excess(bad["gd"], ref["gd"], ref["A_gd"]).max())
    assert worst > 10 * (64 + ref["n_ray"].max()), worst
