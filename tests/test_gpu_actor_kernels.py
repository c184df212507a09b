"""csrc/actors.hip kernel by kernel against tests/actor_refs.py: the candidate lists of nrhip_actor_prepare[_edited], the
containment tables and winners of nrhip_actor_hits / _find_packed / _encode / _density, the pair positions with their
hand-written backward, and the density splice.  Exact-tier scenes are compared bit for bit (ties on a box face and on
dist == radius included), generic scenes per element, |got - ref| <= atol + c U mag, with the counts of actor_refs.py:

  w2b                 C_ROT = 44 on kappa; C_TR = 56 on kappa tmag; + C_EDIT = 8 under an edit
  directions (hit)    the rotation's 44 kappa on |d|_1, a 3-term product 5, norm + 1e-7 and the division 7 -> 44 kappa |d|_1 + 12
  x01, cstd           actor_refs.pair_forward_bounds (C_POS = 72, C_X01 = 8, C_CSTD = 64)
  pair gradients      actor_refs.pair_grad_bound: tests/test_gpu_position_grad_precision.py's 58 (+ 2) per pair on
                      grad_edge_refs' sums of |terms| A, and n + 4 (4 DPP merge levels, n - 1 atomics; rays: n) on the sum S
                      of the magnitudes of the n contributions a slot (a ray) receives, + u |ref|
  splice logit        la fused multiply-adds                                                  -> la on sum |row_k w_k|
  splice density      expf (1 ulp = 2 U) and its stored rounding: 4, the logit's absolute error as a relative one
                                                                                               -> 4 + la A_logit
  splice g_rows       exp 4, two products 2, the clamped logit's error (none beyond +-15)      -> 6 + la A_logit
  splice g_w          exp 4 and the product with go 1 per winner, the product with the row 1, 6 butterfly levels, 3 sums of
                      the four waves, one atomic per block                                     -> 15 + blocks + la A_logit

Each test prints its worst err / bound before it asserts.  The rotation gradient's stays near 1 / 250: its A is
grad_edge_refs' stated upper bound (L1 norms and a factor 4 for the two Gram-Schmidt backwards), and c carries the up to
163 pairs of a slot, whose rounding errors do not line up.  A dropped or doubled contribution is 1 / n of S, far outside."""
import ctypes

import numpy as np
import pytest
import torch

import actor_refs as AR
import synth
from gpu_util import cuda, host
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
f32, f64, U = np.float32, np.float64, AR.U
OUT_DIM = 12


# ---- plumbing ------------------------------------------------------------------------------------------------------------
def make_spec(ops, sc, F=2):
    """ops.ActorSpec straight from a scene's arrays; the geometry kernels never read the tables: one small table for all"""
    A = sc["positions"].shape[1]
    table = cuda(synth.hash_table(4 * 2**9, F, seed=900, scale=0.7))
    return ops.ActorSpec(cuda(sc["timestamps"]), cuda(sc["positions"]), cuda(sc["rotations_6d"]), cuda(sc["present"]),
                         cuda(sc["bounds"]), ops.GridSpec(4, F, 9, 64, 1024), [table] * A, actor_scale=sc["scale"])


def ray_args(sc):
    return tuple(cuda(sc[k]) for k in ("o", "d", "area", "starts", "ends"))


def prepare(ops, spec, sc, K=None, edit=None):
    """nrhip_actor_prepare[_edited] into sentinel-prefilled lists of row length K -> count, actor, w2b (host), flag"""
    from neurad_studio_amd import _lib

    a_full, keep = spec.c_actors()
    a = type(a_full)()
    ctypes.pointer(a)[0] = a_full
    if K is not None:
        a.max_candidates = K
    r, keep_r = ops._c_rays(*ray_args(sc))
    R, K = sc["o"].shape[0], a.max_candidates
    cnt = torch.full((R,), AR.SENTINEL_I, dtype=torch.int32, device="cuda")
    act = torch.full((R, K), AR.SENTINEL_I, dtype=torch.int32, device="cuda")
    w2b = torch.full((R, K, 12), float(AR.SENTINEL_F), dtype=torch.float32, device="cuda")
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    t = cuda(sc["times"])
    if edit is None:
        ops.launch("nrhip_actor_prepare", a, r, t, cnt, act, w2b, flag)
    else:
        e = _lib.ActorEdit(float(edit.get("lateral", 0.0)), float(edit.get("longitudinal", 0.0)),
                           float(edit.get("height", 0.0)), float(edit.get("rotation", 0.0)), int(edit.get("index", -1)))
        ops.launch("nrhip_actor_prepare_edited", a, r, t, e, cnt, act, w2b, flag)
    return host(cnt), host(act), host(w2b), int(flag)


def check_exact_lists(got, ref, K=None):
    cnt, act, w, flag = AR.lists_from_close(ref["close"], ref["w2b"], K)
    assert np.array_equal(got[0], cnt), (got[0], cnt)
    assert np.array_equal(got[1], act), "candidate indices (or a slot behind the count was written)"
    assert np.array_equal(AR.bits(got[2]), AR.bits(w)), "w2b bits (or a slot behind the count was written)"
    assert got[3] == flag


def check_generic_lists(got, g, what):
    """count / indices against prepare64's decisions (the unsure ones either way), w2b per element, sentinels behind"""
    cnt, act, w, flag = got
    R, A = g["close"].shape
    worst = 0.0
    for r in range(R):
        n = int(cnt[r])
        k = act[r, :n]
        assert (np.diff(k) > 0).all() and (act[r, n:] == AR.SENTINEL_I).all() and (w[r, n:] == AR.SENTINEL_F).all(), (what, r)
        have = np.zeros(A, bool)
        have[k] = True
        sure = ~g["unsure"][r]
        assert np.array_equal(have[sure], g["close"][r][sure]), (what, r, np.nonzero(have != g["close"][r])[0])
        err = np.abs(w[r, :n].astype(f64) - g["w2b"][r, k])
        worst = max(worst, float((err / g["w2b_bound"][r, k]).max()) if n else 0.0)
    print(f"{what}: w2b worst err / bound {worst:.3f}")
    assert worst <= 1.0 and flag == 0, (what, worst)
    return worst


# ---- nrhip_actor_prepare / _edited ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,R", [(1, None), (63, None), (64, None), (65, None), (130, None), (65, 61), (65, 1)])
def test_prepare_exact_actor_passes(ops, A, R):
    """the 64-actor passes with their carried count: candidates only in pass 2, only in pass 3, in all three, nowhere; the
    cull ties; R = 1 and a ragged last workgroup"""
    sc = AR.exact_pass_scene(A, R=R)
    check_exact_lists(prepare(ops, make_spec(ops, sc), sc), AR.oracle_lists(sc))


def test_prepare_overflow_cut_inside_pass_two(ops):
    sc = AR.exact_pass_scene(130)
    ref = AR.oracle_lists(sc)
    spec = make_spec(ops, sc)
    got = prepare(ops, spec, sc, K=70)
    assert got[3] == 1 and int(got[0].max()) == 70
    check_exact_lists(got, ref, K=70)
    fits = np.nonzero(ref["close"].sum(-1) <= 70)[0]  # no ray exceeds K: the flag stays 0
    sub = AR.sub_scene(sc, fits)
    got = prepare(ops, spec, sub, K=70)
    assert got[3] == 0
    check_exact_lists(got, AR.oracle_lists(sub), K=70)


@pytest.mark.parametrize("Tn", [1, 4])
def test_prepare_exact_time_brackets_and_present_flags(ops, Tn):
    sc = AR.exact_time_scene(Tn)
    check_exact_lists(prepare(ops, make_spec(ops, sc), sc), AR.oracle_lists(sc))


def test_prepare_exact_single_sample(ops):
    sc = AR.exact_pass_scene(65, S=1)
    ref = AR.oracle_lists(sc)
    assert (ref["count"] == sc["present"].any(0).sum()).all()
    check_exact_lists(prepare(ops, make_spec(ops, sc), sc), ref)


@pytest.mark.parametrize("kw", [dict(seed=0), dict(seed=1, wide=True), dict(seed=3, A=65, R=61)],
                         ids=["Tn4", "wide", "A65-R61"])
def test_prepare_generic(ops, kw):
    """moving actors: a wrong bracket or a wrong frac changes w2b"""
    sc = AR.generic_scene(**kw)
    check_generic_lists(prepare(ops, make_spec(ops, sc), sc), AR.prepare64(sc), f"prepare {kw}")
    one = dict(sc, timestamps=sc["timestamps"][:1], positions=sc["positions"][:1], rotations_6d=sc["rotations_6d"][:1],
               present=sc["present"][:1])  # Tn = 1
    check_generic_lists(prepare(ops, make_spec(ops, one), one), AR.prepare64(one), f"prepare Tn=1 {kw}")


EDITS = [dict(lateral=0.5, longitudinal=-0.25, rotation=0.5, index=-1), dict(lateral=0.5, longitudinal=-0.25, rotation=0.5, index=64),
         dict(lateral=0.5, longitudinal=-0.25, rotation=0.5, index=200), dict(lateral=0.75, longitudinal=0.5, index=-1),
         dict(rotation=-0.75, index=-1)]


def test_prepare_edited(ops):
    sc = AR.generic_scene(seed=3, A=65, R=61)
    spec = make_spec(ops, sc)
    plain = prepare(ops, spec, sc)
    for e in EDITS:
        g = AR.prepare64(sc, e)
        got = prepare(ops, spec, sc, edit=e)
        check_generic_lists(got, g, f"edit {e}")
        moved = np.abs(g["w2b"] - AR.prepare64(sc)["w2b"]).max(-1) > 1e-3
        want = np.ones(65, bool) if e["index"] < 0 else np.arange(65) == min(e["index"], 64)
        assert np.array_equal(moved.any(0), want), "the edit moves the actors it names"
    got = prepare(ops, spec, sc, edit=dict(height=1.5, index=-1))  # a height-only edit is a no-op, as in the reference
    for a, b in zip(got[:3], plain[:3]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- nrhip_actor_hits, _find_packed, and the hit / directions of _encode and _density ---------------------------------
def geometry(ops, sc, flip=None, cand=None, F=2):
    """every geometry output of the dense and the packed kernels on one scene (host arrays)"""
    spec = make_spec(ops, sc, F)
    args = ray_args(sc)
    R, S = sc["starts"].shape
    cand = ops.actor_prepare(spec, *args, cuda(sc["times"])) if cand is None else cand
    fl = None if flip is None else cuda(flip)
    hits = ops.actor_hits(spec, cand, *args)
    feats = torch.full((R * S, OUT_DIM), float(AR.SENTINEL_F), device="cuda")
    dirs, hit = ops.actor_encode(spec, cand, *args, feats, fl)
    ri = torch.arange(R, device="cuda").repeat_interleave(S)
    phits, phit, pdirs = ops.actor_find_packed(spec, cand, args[0], args[1], args[2], args[3].reshape(-1).contiguous(),
                                               args[4].reshape(-1).contiguous(), ri, fl)
    for a, b in ((hits, phits), (hit, phit)):
        assert torch.equal(a, b), "dense and packed layouts"
    assert torch.equal(dirs.view(torch.int32), pdirs.view(torch.int32)), "dense and packed directions, bit for bit"
    return dict(hits=host(hits), hit=host(hit), dirs=host(dirs), feats=host(feats), cand=cand, spec=spec, args=args)


def check_rows(out, sc, L=4, F=2):
    """rows of samples outside every box are untouched; hit rows: L F features, zero padding behind"""
    miss = out["hit"] < 0
    assert (out["feats"][miss] == AR.SENTINEL_F).all()
    assert (out["feats"][~miss][:, L * F:] == 0).all() and np.isfinite(out["feats"][~miss]).all()
    assert (out["feats"][~miss][:, :L * F] != AR.SENTINEL_F).all()
    R, S = sc["starts"].shape
    ray_d = np.repeat(sc["d"], S, 0)
    assert np.array_equal(out["dirs"][miss].view(np.uint32), ray_d[miss].view(np.uint32)), "no hit: the ray's own bits"
    last = np.where(out["hits"] >= 0, out["hits"], -1).max(-1)
    assert np.array_equal(out["hit"], last), "the winner is the highest containing index"


def test_hits_exact_nested_boxes_and_face_ties(ops):
    sc = AR.exact_nest_scene()
    ref = AR.oracle_lists(sc)
    R, S = sc["starts"].shape
    out = geometry(ops, sc)
    assert np.array_equal(out["hits"], ref["hits"]), np.nonzero((out["hits"] != ref["hits"]).any(-1))[0]
    check_rows(out, sc)
    # directions of the hit samples: the winner's rotation of (1, 0, 0), over |.| + 1e-7 -- fp32, one division
    hitm = out["hit"] >= 0
    w = ref["w2b"].reshape(R, -1, 3, 4)[np.repeat(np.arange(R), S)[hitm], out["hit"][hitm]]
    dd = np.einsum("nkc,nc->nk", w[..., :3], np.repeat(sc["d"], S, 0)[hitm]).astype(f32)
    dd = dd / (np.linalg.norm(dd, axis=-1, keepdims=True).astype(f32) + AR.EPS_L)
    assert np.array_equal(AR.bits(out["dirs"][hitm]), AR.bits(dd))
    # flip = -1 on the odd rays: the sign of dx (and px) only
    flip = np.where(np.arange(R) % 2 == 1, -1.0, 1.0).astype(f32)
    fl = geometry(ops, sc, flip)
    assert np.array_equal(fl["hits"], out["hits"])
    want = out["dirs"].copy()
    odd = np.repeat(flip, S) < 0
    want[odd & hitm, 0] *= f32(-1)
    assert np.array_equal(AR.bits(fl["dirs"]), AR.bits(want)) and (odd & hitm).any()
    # density: rows outside every box untouched, the same winners
    spec1 = make_spec(ops, sc, F=1)
    dens = torch.full((R, S), float(AR.SENTINEL_F), device="cuda")
    cand1 = ops.actor_prepare(spec1, *out["args"], cuda(sc["times"]))
    winner = ops.actor_density(spec1, cand1, *out["args"], cuda(np.array([0.3, -0.2, 0.1, 0.4], f32)), dens, return_actor=True)
    assert np.array_equal(host(winner).reshape(-1), out["hit"])
    d = host(dens).reshape(-1)
    assert (d[~hitm] == AR.SENTINEL_F).all() and (d[hitm] > 0).all() and np.isfinite(d[hitm]).all()
    # rays without candidates: with the count zeroed and the rows still naming boxes that contain the samples, nothing is read
    cnt, act, w2b, _ = out["cand"]
    none = geometry(ops, sc, cand=(torch.zeros_like(cnt), act, w2b, None))
    assert (none["hits"] == -1).all() and (none["hit"] == -1).all() and (none["feats"] == AR.SENTINEL_F).all()
    assert np.array_equal(none["dirs"].view(np.uint32), np.repeat(sc["d"], S, 0).view(np.uint32))
    # N = 1: one ray, one sample, inside all twelve boxes
    one = AR.sub_scene(sc, [0])
    one["starts"], one["ends"] = one["starts"][:, 15:16].copy(), one["ends"][:, 15:16].copy()
    o1 = geometry(ops, one)
    assert np.array_equal(o1["hits"], AR.oracle_lists(one)["hits"]) and o1["hits"][0].tolist() == list(range(4, 12))


@pytest.mark.parametrize("kw", [dict(seed=0), dict(seed=3, A=65, R=61)], ids=["N1024", "N976"])
def test_hits_generic(ops, kw):
    sc = AR.generic_scene(**kw)
    g = AR.prepare64(sc)
    h = AR.hits64(sc, g)
    R, S = sc["starts"].shape
    A = sc["positions"].shape[1]
    flip = np.where(np.arange(R) % 3 == 0, -1.0, 1.0).astype(f32)
    out, fl = geometry(ops, sc), geometry(ops, sc, flip)
    check_rows(out, sc)
    inside, unsure = h["inside"].reshape(R * S, A), h["unsure"].reshape(R * S, A)
    clean = ~unsure.any(-1)
    want = AR.hits_table(inside)
    assert np.array_equal(out["hits"][clean], want[clean]), np.nonzero((out["hits"] != want).any(-1) & clean)[0]
    for n in np.nonzero(~clean)[0]:  # an unsure containment may go either way
        got = set(out["hits"][n][out["hits"][n] >= 0].tolist())
        assert set(np.nonzero(inside[n] & ~unsure[n])[0][-AR.KH:].tolist()) - got == set() or len(got) == AR.KH
        assert got <= set(np.nonzero(inside[n] | unsure[n])[0].tolist())
    assert clean.mean() > 0.99 and (want[clean] >= 0).sum() > 2 * R
    # the winner's box-frame direction
    hitm = (out["hit"] >= 0) & clean
    ray = np.repeat(np.arange(R), S)
    w = g["w2b"].reshape(R, A, 3, 4)[ray[hitm], out["hit"][hitm]]
    dd = np.einsum("nkc,nc->nk", w[..., :3], sc["d"].astype(f64)[ray[hitm]])
    dd = dd / (np.linalg.norm(dd, axis=-1, keepdims=True) + f64(AR.EPS_L))
    bound = (U * (44 * g["kappa"][ray[hitm], out["hit"][hitm]] * np.abs(sc["d"][ray[hitm]]).sum(-1) + 12))[:, None]
    worst = float((np.abs(out["dirs"][hitm] - dd) / bound).max())
    print(f"directions {kw}: worst err / bound {worst:.3f}")
    assert worst <= 1.0
    fh = (np.repeat(flip, S) < 0) & (out["hit"] >= 0)
    want_d = out["dirs"].copy()
    want_d[fh, 0] *= f32(-1)
    assert np.array_equal(AR.bits(fl["dirs"]), AR.bits(want_d)) and np.array_equal(fl["hits"], out["hits"]) and fh.any()
    # production order: ops.actor_pairs of the table
    si, ai = ops.actor_pairs(cuda(out["hits"]))
    wsi, wai = AR.pairs_of_hits(out["hits"])
    assert np.array_equal(host(si), wsi) and np.array_equal(host(ai), wai)


# ---- pair positions ------------------------------------------------------------------------------------------------------
def run_pairs(ops, sc, si, ai, flip, gx, gs):
    spec = make_spec(ops, sc)
    args = ray_args(sc)
    R, S = sc["starts"].shape
    t, fl = cuda(sc["times"]), None if flip is None else cuda(flip)
    dsi, dai = cuda(si), cuda(ai)
    x01, cstd = ops.actor_pair_positions(spec, *args, t, dsi, dai, fl)
    ri = torch.arange(R, device="cuda").repeat_interleave(S)
    pk = (args[0], args[1], args[2], args[3].reshape(-1).contiguous(), args[4].reshape(-1).contiguous(), ri, t, dsi, dai, fl)
    px, ps = ops.actor_pair_positions_packed(spec, *pk)
    assert torch.equal(x01.view(torch.int32), px.view(torch.int32)) and torch.equal(cstd.view(torch.int32), ps.view(torch.int32))
    dgx, dgs = cuda(gx), cuda(gs)
    gp, gr, go, gd = ops.actor_pair_positions_bwd(spec, *args, t, dsi, dai, fl, dgx, dgs, ray_grads=True)
    gp2, gr2 = ops.actor_pair_positions_bwd(spec, *args, t, dsi, dai, fl, dgx, dgs)
    gp3, gr3 = ops.actor_pair_positions_packed_bwd(spec, *pk, dgx, dgs)
    h = lambda v: host(v).astype(f64)  # noqa: E731
    return dict(x01=h(x01), cstd=h(cstd), dpos=h(gp), drot=h(gr), go=h(go), gd=h(gd), dpos2=h(gp2), drot2=h(gr2),
                dpos3=h(gp3), drot3=h(gr3))


def check_pairs(got, ref, sc, si, ai, what):
    bx, bs = AR.pair_forward_bounds(sc, si, ai, ref)
    worst = {"x01": float((np.abs(got["x01"] - ref["x01"]) / bx).max()), "cstd": float((np.abs(got["cstd"] - ref["cstd"]) / bs).max())}
    for key, rk in (("dpos", "dpos"), ("drot", "drot"), ("go", "go"), ("gd", "gd"), ("dpos2", "dpos"), ("drot2", "drot"),
                    ("dpos3", "dpos"), ("drot3", "drot")):
        bound, n = AR.pair_grad_bound(ref, rk, dpp=4 if rk in ("dpos", "drot") else 0)
        assert np.isfinite(got[key]).all(), (what, key)
        assert (got[key][np.broadcast_to(n == 0, got[key].shape)] == 0).all(), (what, key, "a slot no pair lands in")
        worst[key] = float((np.abs(got[key] - ref[rk]) / np.maximum(bound, 1e-300)).max())
    print(f"{what}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (what, worst)
    return worst


PAIR_SCENES = {"mag<1": (dict(seed=2), False), "mag>1": (dict(seed=2, scale=1.5), True), "wide": (dict(seed=1, wide=True), False)}


@pytest.mark.parametrize("runs", ["1", "0"])
@pytest.mark.parametrize("name", list(PAIR_SCENES))
def test_pair_positions_runs_blocks_and_flip(ops, switches, name, runs):
    """pairs in production order behind the designed runs (1, 2, 15, 16, 17, 40 equal keys across rows, a wave and a block),
    P = 1 .. 1500 (a last block with one live lane), run combining on and off, flip on and off"""
    kw, tail_random = PAIR_SCENES[name]
    sc = AR.generic_scene(**kw)
    R = sc["o"].shape[0]
    si_all, ai_all = AR.designed_pairs(sc, 1500, tail_random=tail_random)
    flip = np.where(np.arange(R) % 3 == 1, -1.0, 1.0).astype(f32)
    switches.set("NRHIP_PAIR_BWD_RUNS", runs)
    for P, fl in ((1, None), (255, None), (256, flip), (257, None), (1500, None), (1500, flip)):
        si, ai = si_all[:P].copy(), ai_all[:P].copy()
        ref = AR.pair_case(sc, si, ai, fl, 40 + P)
        got = run_pairs(ops, sc, si, ai, fl, ref["gx"], ref["gs"])
        check_pairs(got, ref, sc, si, ai, f"{name} runs={runs} P={P} flip={fl is not None}")


def test_pair_positions_time_edges(ops):
    """frac == 1 exactly (a keyframe 64 s from its neighbour): the left pose's weight 1 - frac is exactly 0 and the kernel
    skips it -- its gradient is exactly 0.0.  (frac == 0 with left != right cannot happen: side=left puts a query on a
    keyframe into the bracket that ends there.)  Tn = 1: every gradient lands on the one pose."""
    sc = AR.generic_scene(seed=1, wide=True)
    R, S = sc["starts"].shape
    A = sc["positions"].shape[1]
    rays = np.nonzero(sc["times"] == sc["timestamps"][3])[0]
    assert len(rays) >= 2 and (AR.frac32(sc["timestamps"], sc["times"])[rays] == 1.0).all()
    si = (rays[:, None] * S + np.arange(S)[None]).reshape(-1).astype(np.int64)
    ai = (np.arange(len(si)) // 3 % A).astype(np.int32)
    ref = AR.pair_case(sc, si, ai, None, 9)
    got = run_pairs(ops, sc, si, ai, None, ref["gx"], ref["gs"])
    check_pairs(got, ref, sc, si, ai, "q on the last keyframe")
    for key in ("dpos", "drot", "dpos2", "drot2", "dpos3", "drot3"):
        assert (got[key][:3] == 0).all() and (got[key][3] != 0).any(), key
    # keyframes 0.75 s apart: frac = 0.75 / (0.75 + 1e-6) < 1 on the keyframe, and the left pose keeps the weight 1 - frac =
    # 1.3e-6 (17 ulp of 0.75 in fp32, 16.8 in float64: its gradient is the reference's within 10 %, not zero)
    near = AR.generic_scene(seed=0)
    rays = np.nonzero(near["times"] == near["timestamps"][2])[0]
    f = AR.frac32(near["timestamps"], near["times"])[rays]
    assert len(rays) >= 2 and (f < 1.0).all() and (f > 0.999).all()
    si = (rays[:, None] * S + np.arange(S)[None]).reshape(-1).astype(np.int64)
    ai = (np.arange(len(si)) // 3 % A).astype(np.int32)
    ref = AR.pair_case(near, si, ai, None, 10)
    got = run_pairs(ops, near, si, ai, None, ref["gx"], ref["gs"])
    check_pairs(got, ref, near, si, ai, "q on a keyframe, frac < 1")
    k = np.unravel_index(np.abs(ref["dpos"][1]).argmax(), ref["dpos"][1].shape)
    assert ref["dpos"][1][k] != 0 and 0.9 < got["dpos"][1][k] / ref["dpos"][1][k] < 1.1, (got["dpos"][1][k], ref["dpos"][1][k])
    one = dict(sc, timestamps=sc["timestamps"][:1], positions=sc["positions"][:1], rotations_6d=sc["rotations_6d"][:1],
               present=sc["present"][:1])
    si, ai = AR.designed_pairs(sc, 600)
    ref = AR.pair_case(one, si, ai, None, 11)
    got = run_pairs(ops, one, si, ai, None, ref["gx"], ref["gs"])
    check_pairs(got, ref, one, si, ai, "Tn = 1")
    assert got["dpos"].shape[0] == 1 and (got["dpos"] != 0).any()


def test_pair_position_mag_equal_one_is_contracted(ops):
    sc = dict(AR.exact_nest_scene(), scale=2.0)
    S = sc["starts"].shape[1]
    m = np.abs(AR.oracle_lists(sc)["pos"][1, :, 11]).max(-1) / f32(2.0)
    si, ai = np.array([S + int(np.nonzero(m == 1.0)[0][0])], np.int64), np.array([11], np.int32)
    ref = AR.pair_case(sc, si, ai, None, 1)
    assert ref["mag"][0] == 1.0 and bool(ref["outside"][0])
    got = run_pairs(ops, sc, si, ai, None, ref["gx"], ref["gs"])
    assert np.array_equal(got["x01"], ref["x01"]), "at mag == 1 the contracted branch returns m itself: exact"
    check_pairs(got, ref, sc, si, ai, "mag == 1")


# ---- the density splice --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,la", [(1, 1), (256, 4), (257, 6), (1000, 4)])
def test_density_splice(ops, P, la):
    c = AR.splice_case(P, la, 10 + P)
    r = AR.splice64(c)
    dens = cuda(c["dens"]).clone()
    rows, w, idx, win = cuda(c["rows"]), cuda(c["w"]), cuda(c["idx"]), cuda(c["winner"])
    logit = ops.actor_density_splice_fwd(dens, rows, w, idx, win)
    g_dens, g_rows, g_w = ops.actor_density_splice_bwd(rows, w, idx, win, logit, dens, cuda(c["g_out"]))
    got = {k: host(v).astype(f64) for k, v in dict(logit=logit, density=dens, g_dens=g_dens, g_rows=g_rows, g_w=g_w).items()}
    hit = r["hit"]
    assert np.array_equal(host(dens)[~hit].view(np.uint32), c["dens"][~hit].view(np.uint32)), "samples without pairs"
    assert (got["g_dens"][hit] == 0).all() and np.array_equal(got["g_dens"][~hit], c["g_out"][~hit].astype(f64))
    e_logit = la * U * r["A_logit"]  # [P]
    e_win = np.zeros(len(c["dens"]))
    e_win[c["idx"][c["winner"]]] = e_logit[c["winner"]]  # the winner's logit error, per sample
    # the backward sees the winner's logit through the clamp: beyond +-15 (by more than its own error) its error is gone
    e_bwd = np.where(np.abs(r["win_logit"]) >= 15 + e_win, 0.0, e_win)
    blocks = -(-P // 256)
    bounds = dict(logit=e_logit, density=np.where(hit, np.abs(r["density"]) * (4 * U + e_win), 0.0),
                  g_rows=np.abs(r["g_rows"]) * (6 * U + e_bwd[c["idx"]])[:, None] + 2.0 ** -126,
                  g_w=(np.where(c["winner"], r["gl"] * ((15 + blocks) * U + e_bwd[c["idx"]]), 0.0)[:, None]
                       * np.abs(c["rows"].astype(f64))).sum(0))
    worst = {k: float((np.abs(got[k] - r[k]) / np.maximum(b, 1e-300)).max()) for k, b in bounds.items()}
    print(f"splice P={P} la={la}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
