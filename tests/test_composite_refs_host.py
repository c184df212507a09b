"""tests/composite_refs.py on the CPU: the case tables reach every branch the classifier knows, the lattice family is exact
by its own numbers, its references agree with plain float64 evaluations, every planted defect fails the comparison that
tests/test_gpu_composite_exact.py makes, and the graded family is not degenerate."""
import numpy as np
import pytest

import composite_refs as CR
from sharp_refs import check, ref_density


def _kernels(op):
    return CR.OP_KERNELS.get(op, ())


def test_classifier_restates_the_dispatch_conditions():
    for C in CR.C_ALL:
        LP = C // 4
        v4 = C % 4 == 0 and LP <= 64 and LP & (LP - 1) == 0
        flat = C <= 64 and 64 % C == 0
        for k in CR.VEC4_KERNELS:
            assert (CR.feature_path(k, C) == "vec4") == v4
            assert CR.feature_path(k, C, aligned=False) == ("flat" if k == "sdf_render_fwd" and flat else "generic")
        for k in CR.FLAT_KERNELS:
            assert CR.feature_path(k, C) == CR.feature_path(k, C, False) == ("flat" if flat else "generic")
    assert [C for C in CR.C_ALL if CR.feature_path("composite_bwd", C) == "vec4"] == [4, 8, 16, 32, 64, 128, 256]
    assert CR.feature_path("sdf_render_fwd", 512) == "generic" and CR.feature_path("sdf_render_fwd", 2) == "flat"
    assert CR.WIDTH_PATHS["accumulate"] == CR.WIDTH_PATHS["composite_fwd"] == {
        1: "flat", 2: "flat", 3: "generic", 4: "flat", 8: "flat", 12: "generic", 16: "flat", 32: "flat", 64: "flat",
        65: "generic", 100: "generic", 128: "generic", 256: "generic", 512: "generic"}
    assert CR.WIDTH_PATHS["sdf_render_fwd"] == {
        1: "flat", 2: "flat", 3: "generic", 4: "vec4", 8: "vec4", 12: "generic", 16: "vec4", 32: "vec4", 64: "vec4",
        65: "generic", 100: "generic", 128: "vec4", 256: "vec4", 512: "generic"}
    assert CR.WIDTH_PATHS["composite_bwd"] == CR.WIDTH_PATHS["sdf_render_bwd"] == {
        **CR.WIDTH_PATHS["sdf_render_fwd"], 1: "generic", 2: "generic"}
    assert CR.pair_taken(32, 32, 32, True, True) and not CR.pair_taken(33, 32, 32, True, True)
    assert not CR.pair_taken(32, 32, 33, True, True) and not CR.pair_taken(32, 32, 32, False, True)
    assert not CR.pair_taken(32, 32, 32, True, False) and not CR.pair_taken(32, 16, 16, True, True)
    assert not CR.pair_taken(32, 32, 32, True, True, head="density")


@pytest.mark.parametrize("kernel", sorted(CR.COVER))
def test_cover_is_complete(kernel):
    """every (path, class) of COVER has a case, and no case takes a branch that COVER does not list"""
    base = kernel.replace("_pair", "")
    op = next(o for o, ks in CR.OP_KERNELS.items() if base in ks)
    got = set()
    for c in CR.CASES[op]:
        for sw in (False, True):
            b = CR.branches(c, base, sw)
            if kernel in CR.PAIR_KERNELS:
                got |= b if CR.case_pair(c, base, sw) else set()
            elif not CR.case_pair(c, base, sw):
                got |= b
                for r in range(c.R):  # the claimed path of every ray agrees with the classifier
                    assert CR.branch(base, c.C, CR.ray_aligned(c, base, r))[0] == CR.feature_path(
                        base, c.C, CR.ray_aligned(c, base, r))
    assert got == set(CR.COVER[kernel]), (set(CR.COVER[kernel]) - got, got - set(CR.COVER[kernel]))


def test_tables_hold_what_the_issue_lists():
    for op, s_list in (("accumulate", CR.S_COMP), ("composite", CR.S_COMP), ("sdf_render", CR.S_SCAN),
                       ("prop_weights", CR.S_PROP)):
        cs = CR.CASES[op]
        assert {c.S for c in cs} >= set(s_list) and {c.R for c in cs} >= set(CR.R_ALL), op
        assert len({c.id for c in cs}) == len(cs)
    assert {c.C for c in CR.COMP_CASES} == {c.C for c in CR.SDF_CASES} == set(CR.C_ALL)
    for op in ("composite", "sdf_render"):  # a tail behind the last full pass at every float4 width below LP = 64
        for C in (4, 8, 16, 32, 64, 128):
            assert any(c.C == C and c.S % (64 // (C // 4)) for c in CR.CASES[op]), (op, C)
    assert all(c.S <= 17 for op in CR.CASES for c in CR.CASES[op] if c.C == 512)
    assert [(c.R, c.S, c.C) for c in CR.SDF_LONG] == [(2, 2048, 4), (2, 1024, 4)]
    sw = [c for c in CR.SDF_CASES if CR.case_pair(c, "sdf_render_fwd", True)]
    assert {c.R for c in sw} == set(CR.R_ALL) and {c.S for c in sw} >= {2, 31, 32}
    assert any(c.es_extra for c in CR.PROP_CASES) and any(c.S == 193 and c.es_extra for c in CR.PROP_CASES)


def test_saturated_head_is_exact_in_fp32():
    """sigmoidf_(-sdf beta) = 1 / (1 + exp(sdf beta)) at the lattice's three values, for every beta of the family"""
    for beta in (0.5, 1.0, 2.0, 4.0):
        a = CR.alpha_of_lattice_sdf(np.array([0.0, CR.BIG, -CR.BIG], np.float32), beta)
        assert a.dtype == np.float32 and a.tolist() == [0.5, 0.0, 1.0]
    with np.errstate(over="ignore"):
        assert np.exp(np.float32(CR.BIG)) == np.inf and np.exp(np.float32(-CR.BIG)) == 0
        assert -np.expm1(-np.exp(np.float32(CR.BIG)) * np.float32(2)) == 1 and -np.expm1(np.float32(-0.0)) == 0
        assert np.exp(-np.float32(CR.DENSE)) == 0


@pytest.mark.parametrize("op", sorted(CR.CASES))
def test_lattice_cases_are_exact(op):
    top = 0.0
    for c in CR.CASES[op]:
        d = CR.lattice_inputs(c)
        top = max(top, CR.assert_exact(c, d))
        for k, v in CR.lattice_ref(c, d).items():  # every reference value is an fp32 number
            assert np.array_equal(np.asarray(v, np.float64), np.asarray(v, np.float32).astype(np.float64)), (c.id, k)
    print(f"{op}: largest sum {top:.0f} quanta of 2^24 = {CR.LIMIT}")


def test_lattice_holds_the_edge_weights():
    c = CR.Case("composite", 5, 129, 32)
    w = CR.lattice_weights(c)
    assert (w[0, [0, 63, 64, 65, 127, 128]] > 0).all() and (w[-1] == 0).all() and ((w > 0).sum(-1) <= 16).all()
    a = CR.lattice_alpha(CR.Case("sdf_render", 5, 129, 32), CR.lattice_inputs(CR.Case("sdf_render", 5, 129, 32)))
    assert (a[0, [0, 63, 64, 65, 127, 128]] == 0.5).all() and (a[1] == 1).sum() == 1 and (a[2] == 0).all()
    assert ((a == 0.5).sum(-1) <= 8).all()


@pytest.mark.parametrize("op", sorted(CR.CASES))
def test_lattice_reference_is_the_float64_formula(op):
    for c in CR.CASES[op]:
        d = CR.lattice_inputs(c)
        ref = CR.lattice_ref(c, d)
        if op == "sdf_render":
            plain = CR.graded_sdf_render(c, {**d, "beta_min": 0.0}, CR.lattice_alpha(c, d).astype(np.float32))
            for k, (v, _) in plain.items():
                if not (c.head == "density" and k == "gsdf"):
                    assert np.allclose(ref[k], v, rtol=1e-13, atol=0), (c.id, k)
        elif op == "prop_weights":
            for k, (v, _) in CR.ref_prop_weights(c, d).items():
                assert np.allclose(ref[k], v, rtol=1e-13, atol=0), (c.id, k)
        else:
            w, f, g = (d[k].astype(np.float64) for k in ("w", "f", "gF"))
            w2 = w.copy()
            w2[:, -1] += 1 - w.sum(-1)
            want = np.einsum("rs,rsc->rc", w2 if op == "composite" else w, f)
            assert np.array_equal(ref["features" if op == "composite" else "out"], want), c.id
            assert np.array_equal(ref["d weights"] - (0 if op == "accumulate" else
                                                      CR.ref_composite_bwd(w2 * 0, d["f"] * 0, ((d["st"] + d["en"]) / 2).astype(np.float64), d["gF"],
                                                                           d["gD"], d["gA"])[1]),
                                  np.einsum("rc,rsc->rs", g, f) - (0 if op == "accumulate" else
                                                                    np.einsum("rc,rc->r", g, f[:, -1])[:, None])), c.id


def _fails_lattice(c, defect):
    d = CR.lattice_inputs(c)
    ref, bad = CR.lattice_ref(c, d), CR.lattice_ref(c, d, defect)
    for k in ref:
        try:
            CR.same(np.asarray(bad[k], np.float32), ref[k], k)
        except AssertionError:
            return True
    return False


def _fails_graded(c, defect):
    d = CR.graded_inputs(c)
    if c.op == "sdf_render":
        a32 = CR.graded_alpha(c, d)[0].astype(np.float32)
        ref, bad = CR.graded_sdf_render(c, d, a32), CR.graded_sdf_render(c, d, a32, defect)
        bad = CR._pair_defect({k: v[0].copy() for k, v in bad.items()}, defect)
        bad = {k: (v, None) for k, v in bad.items()}
    elif c.op == "prop_weights":
        ref, bad = CR.ref_prop_weights(c, d), CR.ref_prop_weights(c, d, defect=defect)
    else:
        fn = CR.graded_accumulate if c.op == "accumulate" else CR.graded_composite
        ref, bad = fn(c, d), fn(c, d, defect)
    for k, (v, bound) in ref.items():
        try:
            check(bad[k][0], v, bound, k)
        except AssertionError:
            return True
    return False


@pytest.mark.parametrize("defect", CR.DEFECTS)
def test_planted_defect_fails_the_gpu_comparison(defect):
    """in both families, for at least one case of every op the defect applies to -- and for the pair cases where it is theirs"""
    for op in CR.DEFECT_OPS[defect]:
        cs = CR.CASES[op]
        if defect == "upper_half_wrong_ray":
            cs = [c for c in cs if CR.case_pair(c, "sdf_render_fwd", True) and c.R > 1]
            assert cs
        hit_l = [c.id for c in cs if _fails_lattice(c, defect)]
        hit_g = [c.id for c in cs if c.S <= 129 and c.C <= 128 and _fails_graded(c, defect)]
        assert hit_l and hit_g, (defect, op, hit_l, hit_g)
        print(f"{defect} / {op}: fails {len(hit_l)} lattice and {len(hit_g)} graded cases of {len(cs)}")


@pytest.mark.parametrize("op", sorted(CR.CASES))
def test_graded_cases_are_not_degenerate(op):
    """sdf_render: at least half of a case's samples have alpha in [0.02, 0.98];  composite / accumulate: the same of the
    alphas the weights are made from (by construction: [0.02, 0.5]), no weight is 0;  prop_weights: from 31 samples on every
    ray ends with a transmittance in [1e-4, 0.5].  No reference feature row is all zero and no upstream gradient row is."""
    for c in CR.CASES[op]:
        d = CR.graded_inputs(c)
        if op == "prop_weights":
            S = c.S
            _, T, a, _, _, _ = ref_density(d["e"][:, 1:S + 1] - d["e"][:, :S], d["dens"], d["gw"])
            end = T[:, -1] * (1 - a[:, -1])
            assert S < 31 or ((end >= 1e-4) & (end <= 0.5)).all(), (c.id, end)
            continue
        if op == "sdf_render":
            a = CR.graded_alpha(c, d)[0]
            assert ((a >= 0.02) & (a <= 0.98)).mean() >= 0.5, c.id
            ref = CR.graded_sdf_render(c, d, a.astype(np.float32))["out"][0]
        else:
            assert (d["w"] > 0).all()
            ref = (CR.graded_accumulate if op == "accumulate" else CR.graded_composite)(c, d)
            ref = ref["out" if op == "accumulate" else "features"][0]
        assert (np.abs(ref).max(-1) > 0).all() and (np.abs(d["gF"]).max(-1) > 0).all(), c.id


def test_embedding_cases():
    names = {c.name: c for c in CR.EMBED_CASES}
    assert names["lds-boundary"].E * names["lds-boundary"].D == CR.EMBED_LDS and names["lds-boundary"].in_lds
    assert names["one-row-over"].E * names["one-row-over"].D == CR.EMBED_LDS + names["one-row-over"].D
    assert not names["one-row-over"].in_lds
    for n in ("grid-stride-lds", "grid-stride-global"):
        assert names[n].R * names[n].D == CR.GRID_CAP + names[n].D
    for c in CR.EMBED_CASES:
        d = CR.embed_inputs(c)
        lo, hi, frac = CR.embed_slots(c, d)
        fwd, gw = CR.ref_embed(c, d)
        assert lo.min() >= 0 and hi.max() < c.E and np.array_equal(frac * 8, np.rint(frac * 8))
        assert np.array_equal(fwd * 8, np.rint(fwd * 8)) and np.array_equal(gw * 8, np.rint(gw * 8))
        if c.temporal and c.times:
            assert d["times"][0] == 0 and d["times"][1] == c.duration and frac[1] == 1 and frac.max() == 1
            assert (hi != lo).any()
        if c.bad_sensors:
            assert (d["sensor"] < 0).any() and (d["sensor"] >= c.n_sensors).any()
