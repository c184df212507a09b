"""The scenes and references of tests/test_gpu_actor_kernels.py, checked without a GPU (tests/actor_refs.py): the exact tier
is exact, every scene enters the branch it was built for, the share of discrete decisions the generic tier leaves out is
within its cap, and the float64 restatements agree with the fp32 oracle on the golden field_actors scene."""
import numpy as np
import pytest

import actor_refs as AR
import neurad_oracle as O
from builders import actor_params
from conftest import load_golden

f32, f64 = np.float32, np.float64


# ---- the exact tier is exact, and enters its branches ------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 63, 64, 65, 130])
def test_exact_pass_scene(A):
    sc = AR.exact_pass_scene(A)
    ref = AR.exact_check(sc)
    close = ref["close"]
    per_pass = np.stack([close[:, a0:a0 + 64].sum(-1) for a0 in range(0, 192, 64)], -1)  # [R,3]
    print(f"A = {A}: candidates per ray and pass\n{per_pass}")
    assert (per_pass.sum(-1) == 0).any(), "a ray without candidates"
    if A >= 6:  # the cull ties of actor 5: dist == radius is rejected, one step inside is accepted
        tie = (ref["dist"][:, 5] == ref["radii"][5])
        step = (ref["radii"][5] - ref["dist"][:, 5] == f32(2.0 ** -10))
        assert tie.sum() == 2 and not close[tie, 5].any() and step.sum() == 2 and close[step, 5].all()
    if A == 130:
        assert ((per_pass[:, 0] == 0) & (per_pass[:, 1] > 0) & (per_pass[:, 2] == 0)).any(), "pass 2 only"
        assert ((per_pass[:, 0] == 0) & (per_pass[:, 1] == 0) & (per_pass[:, 2] > 0)).any(), "pass 3 only"
        assert (per_pass > 0).all(-1).any(), "all three passes: a non-zero carry twice"
        # K = 70: a ray with more than 70 close actors whose 70th falls inside pass 2
        over = close.sum(-1) > 70
        assert over.any() and (per_pass[over, 0] < 70).all() and (per_pass[over, :2].sum(-1) > 70).all()
        assert (close[~over].sum(-1) <= 70).all() and (~over).sum() >= 4
        cnt, act, w, flag = AR.lists_from_close(close, ref["w2b"], K=70)
        assert flag == 1 and (cnt[over] == 70).all()
        for r in np.nonzero(over)[0]:
            assert np.array_equal(act[r], np.nonzero(close[r])[0][:70])
    if A == 65:
        assert close[:, 64].any(), "lane 0 of pass 2 is a candidate somewhere"
    assert not close[:, ~sc["present"].any(0)].any()


def test_exact_single_sample_scene():
    """S = 1: the line direction is 0 / 1e-7 = 0, dist = 0, every valid actor is a candidate -- in the oracle as well"""
    sc = AR.exact_pass_scene(65, S=1)
    ref = AR.exact_check(sc)
    assert (ref["dist"] == 0).all() and np.array_equal(ref["close"], np.broadcast_to(sc["present"].any(0), ref["close"].shape))


@pytest.mark.parametrize("Tn", [1, 4])
def test_exact_time_scene(Tn):
    sc = AR.exact_time_scene(Tn)
    ref = AR.exact_check(sc)
    left, right, frac = AR.brackets(sc["timestamps"], sc["times"])
    if Tn == 1:
        assert (left == 0).all() and (right == 0).all() and set(frac.tolist()) <= {0.0, 1.0}  # 0 / 1e-6 or clamped
        return
    ts, q = sc["timestamps"], sc["times"]
    for want in (q < ts[0], q == ts[0], q == ts[2], q == ts[3], q > ts[3], (q > ts[1]) & (q < ts[2])):
        assert want.any()
    assert (left[q <= ts[0]] == 0).all() and (right[q <= ts[0]] == 0).all() and (left[q > ts[3]] == 3).all()
    assert (right[q == ts[2]] == 2).all() and (left[q == ts[2]] == 1).all()
    combos = {(bool(sc["present"][l, a]), bool(sc["present"][r, a]), l == r) for l, r in zip(left, right) for a in range(4)}
    for same in (False, True):
        for pl_, pr_ in ((0, 0), (1, 0), (0, 1), (1, 1)):
            if same and pl_ != pr_:
                continue
            assert (bool(pl_), bool(pr_), same) in combos, (pl_, pr_, same)
    assert ref["valid"].any() and not ref["valid"].all()


def test_exact_nest_scene():
    sc = AR.exact_nest_scene()
    ref = AR.exact_check(sc)
    R, S = sc["starts"].shape
    n = ref["n_contain"].reshape(R, S)
    print("containing boxes per sample\n", n)
    assert {0, 1, 7, 8, 9, 12} <= set(n[0].tolist())
    for s in range(S):  # the table: the 8 highest indices ascending, -1 behind; the winner is the highest
        row = ref["hits"][s]
        k = min(n[0, s], 8)
        assert np.array_equal(row[:k], np.arange(AR.NEST - k, AR.NEST)) and (row[k:] == -1).all()
    # face ties: a coordinate equal to its bound is outside, on each axis in turn
    pos, bnd = np.abs(ref["pos"]), sc["bounds"][None, None]
    for axis, ray in ((0, 1), (1, 2), (2, 4)):
        on_face = (pos[ray, :, :, axis] == bnd[0, :, :, axis]) & (np.delete(pos[ray] < bnd[0], axis, -1)).all(-1)
        assert on_face.any() and not ref["inside"][ray][on_face].any(), axis
    # ... and one step inside the y / z face is inside, for the samples within the box's x extent
    assert ref["inside"][3, :, 11].any() and not ref["inside"][2, :, 11].any()
    assert ref["inside"][5, :, 11].any() and not ref["inside"][4, :, 11].any()
    assert ref["close"][2, 11] and ref["close"][4, 11], "the tie rays are candidates: the box test decides"
    assert ref["count"][6] == 0 and np.array_equal(ref["hits"][:S], ref["hits"][7 * S:])
    # the oracle's own hit list and the march's in-box test see the same samples
    mean = ref["mean"]
    ap = AR.actor_params(sc)
    b2w, valid = O.actor_boxes2world(ap, sc["times"])
    r, s, k = O.actor_hits(ap, mean, b2w, valid, O.pose_inverse(b2w))
    got = np.zeros_like(ref["inside"])
    got[r, s, k] = True
    assert np.array_equal(got, ref["inside"])
    import packed_actor_refs as PA

    ray = np.repeat(np.arange(R), S)
    assert np.array_equal(PA.in_box(ap, sc["o"], sc["d"], sc["times"], ray, sc["starts"].reshape(-1), sc["ends"].reshape(-1)),
                          ref["inside"].any(-1).reshape(-1))


# ---- the generic tier ----------------------------------------------------------------------------------------------------
GENERIC = [dict(seed=0), dict(seed=1, wide=True), dict(seed=2, scale=1.5), dict(seed=3, A=65, R=61)]


@pytest.mark.parametrize("kw", GENERIC, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_generic_scene_left_out_shares(kw):
    sc = AR.generic_scene(**kw)
    for edit in (None, dict(lateral=0.5, longitudinal=-0.25, rotation=0.5, index=-1)):
        g = AR.prepare64(sc, edit)
        h = AR.hits64(sc, g)
        R, S = sc["starts"].shape
        A = sc["positions"].shape[1]
        cull = AR.left_out_share(g["unsure"], g["valid"].sum())
        box = AR.left_out_share(h["unsure"], (g["close"] | g["unsure"]).sum() * S)
        print(f"{kw} edit={edit is not None}: candidates {int(g['close'].sum())} of {R * A}, containments "
              f"{int(h['inside'].sum())}; left out: cull {cull:.4%}, box {box:.4%}; kappa max {g['kappa'].max():.3f}")
        assert cull <= AR.MAX_LEFT_OUT and box <= AR.MAX_LEFT_OUT
        assert g["kappa"].max() < 4 and g["kappa"].min() > 1.001, "non-orthonormal rows, moderately conditioned"
        assert g["close"].sum() > R and h["inside"].sum() > 2 * R
    ts, q = sc["timestamps"], sc["times"]
    for want in (q < ts[0], q == ts[0], q == ts[2], q == ts[3], q > ts[3]):
        assert want.any()
    left, right, frac = AR.brackets(ts, q)
    if kw.get("wide"):
        f = AR.frac32(ts, q)
        assert (f[(q == ts[2]) | (q == ts[3])] == 1.0).all(), "fp32 frac == 1 exactly on a keyframe 64 s from its neighbour"
    else:
        assert (AR.frac32(ts, q)[q == ts[2]] < 1.0).all()
    combos = {(bool(sc["present"][l, a]), bool(sc["present"][r, a])) for l, r in zip(left, right) for a in (0, 1)}
    assert combos == {(False, False), (True, False), (False, True), (True, True)}


@pytest.mark.parametrize("scale", [10.0, 1.5])
def test_designed_pairs_runs_and_contraction(scale):
    sc = AR.generic_scene(seed=2, scale=scale)
    si, ai = AR.designed_pairs(sc, 1500, tail_random=scale < 5)
    assert len(si) == 1500
    start, ln = AR.run_lengths(sc, si[:AR.RUN_END], ai[:AR.RUN_END])
    assert set(AR.RUNS) <= set(ln.tolist()), sorted(set(ln.tolist()))
    for p, n in AR.RUN_LAYOUT:
        assert n in ln[start == p], (p, n)
    inside = lambda p, n, m: (p % m) != 0 and (p // m) != ((p + n - 1) // m)  # noqa: E731  (starts mid-way and crosses)
    assert inside(5, 16, 16) and inside(40, 40, 64) and inside(250, 17, 256) and not inside(80, 15, 16)
    # the production-order tail has runs of its own (consecutive samples of a ray in one box)
    _, tail = AR.run_lengths(sc, si[AR.RUN_END:], ai[AR.RUN_END:])
    assert tail.max() >= 3 or scale < 5
    ref = AR.pair_case(sc, si, ai, None, 5)
    share = float(ref["outside"].mean())
    print(f"scale {scale}: {share:.1%} of the pairs contracted (mag >= 1)")
    assert share > 0.5 if scale < 5 else share < 0.5
    assert ref["outside"].any() and (~ref["outside"]).any()


def test_mag_equal_one_pair_is_contracted():
    """exact tier: a sample exactly actor_scale away along one box axis: m == 1, not < 1 -- the contracted branch, whose
    value at mag == 1 is m itself"""
    sc = AR.exact_nest_scene()
    sc = dict(sc, scale=2.0)
    ref = AR.oracle_lists(sc)
    S = sc["starts"].shape[1]
    m = np.abs(ref["pos"][1, :, 11]).max(-1) / f32(2.0)  # ray 1, box 11
    s = S + int(np.nonzero(m == 1.0)[0][0])
    out = AR.pair_case(sc, np.array([s], np.int64), np.array([11], np.int32), None, 1)
    assert out["mag"][0] == 1.0 and bool(out["outside"][0])


def test_splice_cases():
    for P, la in ((1, 1), (256, 4), (257, 6), (1000, 4)):
        c = AR.splice_case(P, la, 10 + P)
        r = AR.splice64(c)
        per = np.bincount(c["idx"], minlength=len(c["dens"]))
        if P > 1:
            assert {0, 1, 2, 3} <= set(per.tolist()), "samples with no pair, a winner alone, one and two shadowed pairs"
            lw = r["win_logit"][r["hit"]]
            assert (np.abs(lw) > 15).any() and (np.abs(lw) < 15).any() and (lw > 15).any() and (lw < -15).any()
            sh = ~c["winner"]
            assert (np.abs(r["win_logit"][c["idx"][sh]]) > 15).any(), "a shadowed pair behind a clamped winner"
        assert np.array_equal(np.bincount(c["idx"][c["winner"]], minlength=len(per)), (per > 0).astype(int))
        # the restated gradients: winners go * exp(clamp) row / w; every pair of a sample the same row gradient
        gl = c["g_out"].astype(f64)[c["idx"]] * np.exp(np.clip(r["win_logit"][c["idx"]], -15, 15))
        np.testing.assert_allclose(r["g_rows"], gl[:, None] * c["w"].astype(f64)[None], rtol=1e-12, atol=0)
        np.testing.assert_allclose(r["g_w"], (gl[:, None] * c["rows"].astype(f64))[c["winner"]].sum(0), rtol=1e-9, atol=1e-12)
        assert (r["g_dens"][r["hit"]] == 0).all() and np.array_equal(r["g_dens"][~r["hit"]], c["g_out"][~r["hit"]].astype(f64))
        assert np.array_equal(r["density"][~r["hit"]], c["dens"][~r["hit"]].astype(f64))


# ---- the restatements against the fp32 oracle on the golden scene ------------------------------------------------------
def test_restatements_vs_oracle_on_golden_scene():
    g = load_golden("field_actors")
    ap = actor_params(g)
    sc = AR.scene_dict(ap.timestamps, ap.positions, ap.rotations_6d, ap.present, ap.bounds, g["o"], g["d"], g["starts"],
                       g["ends"], g["times"], area=g["area"])
    assert np.array_equal(AR.actor_params(sc).bounds, ap.bounds)
    ref = AR.oracle_lists(sc)
    p = AR.prepare64(sc)
    h = AR.hits64(sc, p)
    R, S = g["starts"].shape
    # the oracle's own tolerance for its fp32 chain: 1e-6 relative of the translation's size (tests/test_oracle_actors.py)
    err = np.abs(p["w2b"] - ref["w2b"].astype(f64))
    assert (err <= p["w2b_bound"]).all(), float((err / p["w2b_bound"]).max())
    assert np.array_equal(p["valid"], ref["valid"])
    sure = ~p["unsure"]
    assert np.array_equal(p["close"][sure], ref["close"][sure]) and sure.mean() > 0.995
    sure = ~h["unsure"]
    assert np.array_equal(h["inside"][sure], ref["inside"][sure]) and sure.mean() > 0.995
    want = np.zeros((R, S), bool)
    want[g["hit_ray"], g["hit_sample"]] = True  # the reference's own hit set
    assert np.array_equal(h["inside"].any(-1) | (h["unsure"].any(-1) & want), want)
    # the pair chain: float64 x01 of the oracle's hits against the oracle's fp32 contraction of its own box positions
    si, ai = AR.pairs_of_hits(ref["hits"])
    out = AR.pair_case(sc, si, ai, None, 3)
    pos = ref["pos"].reshape(R * S, -1, 3)[si, ai]
    _, std = O.fast_isotropic_gaussian(g["o"], g["d"], g["area"], g["starts"], g["ends"])
    x01, cstd = O.contract_gaussian(pos, std.reshape(-1)[si], sc["scale"])
    bx, bs = AR.pair_forward_bounds(sc, si, ai, out)
    assert (np.abs(x01 - out["x01"]) <= bx).all() and (np.abs(cstd - out["cstd"]) <= bs).all()
