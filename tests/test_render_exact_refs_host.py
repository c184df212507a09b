"""tests/render_exact_refs.py is what it claims, shown on the CPU with numpy and the fp32 oracle: the lattice family's
operands meet every condition its exactness argument uses, its int64 reference equals oracle/neurad_oracle.py bit for bit,
the graded family's float64 reference holds the fp32 oracle inside its own bounds, and each planted defect passes the older
tests' rel-L2 check while the comparison made here flags it."""
import dataclasses

import numpy as np
import pytest

import neurad_oracle as O
import render_exact_refs as X
from conftest import rel_l2

f32 = np.float32
TOL = 1e-4  # the older render tests' rel-L2 tolerance (tests/gpu_util.py)
S_ALL = (1, 15, 16, 17, 63, 64, 65, 129)
NETS = sorted({r[:3] for r in X.rows()})
ORACLE_NETS = [(8, 4, 32), (16, 2, 64), (4, 2, 32)]


def test_grids_are_powers_of_two():
    for (L, F), (mn, mx) in X.GRIDS.items():
        sc = O.hash_scalings(L, mn, mx)
        assert sc.shape == (L,) and (sc >= 64).all() and (np.log2(sc) % 1 == 0).all(), (L, F, sc)


def test_rows_in_scope():
    rows = X.rows()
    assert len(rows) == 49 and {r[4] for r in rows} == set(X.SOURCES)
    assert {(r[0], r[1]) for r in rows} == set(X.GRIDS)
    assert {r[2] for r in rows} == {32, 64}


@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
@pytest.mark.parametrize("L,F,H", NETS)
def test_lattice_operands(L, F, H, use_sdf):
    p = X.network(L, F, H, use_sdf)
    for a in [p.grid.table, *p.geo_w, *p.geo_b, *p.feat_w, *p.feat_b]:
        assert a.dtype == f32 and (a == np.rint(a)).all()
    assert np.abs(p.grid.table).max() == 3 and p.grid.table.shape == (L << X.LOG2_T, F)
    assert (p.grid.table.astype(np.float16).astype(f32) == p.grid.table).all()
    assert not p.feat_w[0][:, 32:].any() and p.feat_w[0].shape == (H, 48)
    assert max(np.abs(w).max() for w in [p.geo_w[0], p.geo_w[1][1:], *p.feat_w]) <= 3  # |w| < 2^8 and 128 |w| < 65000
    assert ((p.geo_w[1][0] / 256) % 1 == 0).all() and (p.geo_b[1][0] - 128) % 256 == 0
    c = X.dense_case(L, F, H, use_sdf, 29, 129)
    ref = X.sample_ref(p, c.q)
    X.is_hit(p, ref.sdf)  # (asserts |raw| beta >= 100)
    assert (np.abs(ref.sdf) >= 128).all() and ((ref.sdf - 128) % 256 == 0).all()
    assert X.assert_exact_operands(ref, split=(H == 64 and L * F == 32)) < 2 ** 18
    # positions, by the oracle's own fp32 arithmetic: multiples of 1 / 64 inside (1/4, 3/4), std 0, and at every level the
    # eight corners are one row -- the one lattice_rows names
    mean, std = O.fast_isotropic_gaussian(*X.oracle_inputs(c))
    pos, cstd = O.contract_gaussian(mean, std, p.static_scale)
    assert not cstd.any() and (np.abs(mean) <= X.QMAX).all() and (pos * 64 % 1 == 0).all() and 0.25 < pos.min() <= pos.max() < 0.75
    idx, off = O.hashgrid_corner_indices(pos.reshape(-1, 3), p.grid.scalings, p.grid.table_size)
    assert not off.any() and (idx == idx[..., :1]).all()
    assert np.array_equal(idx[..., 0], X.lattice_rows(p.grid, c.q))
    assert (np.abs(c.d).sum(1) <= 1).all() and (c.o % 1 == 0).all() and ((c.d == 0).all(1)).any()


@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
@pytest.mark.parametrize("S", [17, 129])
@pytest.mark.parametrize("L,F,H", ORACLE_NETS)
def test_int64_reference_is_the_oracle_bit_for_bit(L, F, H, S, use_sdf):
    p = X.network(L, F, H, use_sdf)
    c = X.dense_case(L, F, H, use_sdf, 29, S)
    ref = X.sample_ref(p, c.q)
    rays = X.oracle_inputs(c)
    with np.errstate(over="ignore"):
        got = O.render_rays(p, *rays)
        fld = O.field_fwd(p, *rays)
    enc = O.encode_static(p.grid, p.static_scale, *rays)
    geo, hid = O.mlp_fwd(enc, p.geo_w, p.geo_b, return_hidden=True)
    sh = O.sh_deg4(np.repeat((c.d + f32(1)) / f32(2), S, 0))
    _, fh = O.mlp_fwd(np.concatenate([geo[:, 1:], sh], -1), p.feat_w, p.feat_b, return_hidden=True)
    eq = lambda a, b: np.array_equal(np.asarray(a, f32).reshape(-1), np.asarray(b).astype(f32).reshape(-1))  # noqa: E731
    assert eq(enc, ref.enc) and eq(hid[1], ref.hg) and eq(geo[:, 1:], ref.emb) and eq(geo[:, 0], ref.sdf)
    assert eq(np.concatenate([fh[1], fh[2]], 1), ref.hf) and eq(fld["feature"], ref.feature)
    hit = X.is_hit(p, ref.sdf)
    if use_sdf:
        assert eq(fld["sdf"], ref.sdf) and eq(fld["alpha"], hit)
    else:
        assert eq(fld["density"], np.where(hit, np.inf, 0.0))
    sel = X.selector_ref(p, c, ref, packed=False)
    assert eq(got["weights"], sel.weights) and eq(got["features"], sel.features)
    assert eq(got["depth"], sel.depth) and eq(got["accumulation"], sel.accumulation)
    assert set(np.unique(sel.weights)) <= {0.0, 1.0} and sel.weights.sum() == sel.accumulation.sum()


def test_packed_selector_reference_against_the_oracle_ray_by_ray():
    """packed compositing: no sky residual, the last sample's depth counts, zeros for a ray without samples"""
    L, F, H = 8, 4, 32
    p = X.network(L, F, H, True)
    c = X.packed_case(L, F, H, True, X.PACKED_COUNTS["mixed"])
    ref = X.sample_ref(p, c.q)
    sel = X.selector_ref(p, c, ref, packed=True)
    alpha = X.is_hit(p, ref.sdf).astype(f32)
    for r in range(c.R):
        sl = slice(c.seg[r], c.seg[r + 1])
        if sl.start == sl.stop:
            assert not sel.features[r].any() and sel.depth[r] == 0 and sel.accumulation[r] == 0
            continue
        w, _ = O.render_weight_from_alpha(alpha[None, sl])
        assert np.array_equal(w[0], sel.weights[sl])
        assert np.array_equal(O.accumulate_along_rays(w, ref.feature[None, sl].astype(f32))[0], sel.features[r])
        assert np.array_equal(O.accumulate_along_rays(w, c.t[None, sl, None].astype(f32))[0], sel.depth[r])
        assert np.array_equal(O.accumulate_along_rays(w)[0], sel.accumulation[r])


@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
@pytest.mark.parametrize("L,F,H", NETS)
def test_every_prescribed_first_hit_is_realised(L, F, H, use_sdf):
    p = X.network(L, F, H, use_sdf)
    for S in S_ALL:
        c = X.dense_case(L, F, H, use_sdf, 29, S)
        first = X.first_hits(c, X.is_hit(p, X.sample_ref(p, c.q).sdf))
        assert [None if f < 0 else int(f) for f in first] == c.want
        assert set(c.want) == set(X.prescribed(S)), S
    seen = {}
    for name, counts in X.PACKED_COUNTS.items():
        c = X.packed_case(L, F, H, use_sdf, counts)
        assert tuple(c.counts) == counts
        first = X.first_hits(c, X.is_hit(p, X.sample_ref(p, c.q).sdf))
        assert [None if f < 0 else int(f) for f in first] == c.want
        for n, w in zip(counts, c.want):
            seen.setdefault(n, set()).add(w)
    assert set(seen) == {0, 1, 15, 16, 17, 64, 65}
    for n in seen:
        assert seen[n] == (set(X.prescribed(n)) if n else {None}), (n, seen[n])


def test_lattice_family_holds_pair_and_fallback_tiles():
    """every pair row's cases hold tiles whose four layers all take the fp16-pair products and tiles with a layer that falls
    back to fp32 (an input at or beyond 65000 / 64)"""
    for L, F, H in sorted({r[:3] for r in X.rows(products=("F16Pairs",))}):
        kinds = np.concatenate([X.pair_layers(c, X.sample_ref(X.network(L, F, H), c.q))
                                for c in (X.dense_case(L, F, H, True, 29, 129), X.dense_case(L, F, H, True, 29, 17))])
        assert kinds.all(1).sum() >= 4 and (~kinds.all(1)).sum() >= 4, (L, F, H, kinds.mean(0))


def test_override_cases_reach_full_ragged_and_block_end_tiles():
    c = X.dense_case(8, 4, 32, True, 29, 65)
    ovr, rows, dirs = X.override_case(8, 4, c)
    s = np.flatnonzero(ovr >= 0) % 65
    assert set(s) == {5, 50, 64} and len(np.unique(ovr[ovr >= 0])) == len(s) and ovr.max() < len(rows)
    assert (np.abs(rows) <= 3).all() and (rows % 1 == 0).all() and np.allclose(np.linalg.norm(dirs, axis=1), 1)
    p = X.network(8, 4, 32)
    ref = X.sample_ref(p, c.q, ovr, rows)
    assert np.array_equal(ref.enc[ovr >= 0], rows[ovr[ovr >= 0]]) and X.assert_exact_operands(ref) < 2 ** 18
    base = X.sample_ref(p, c.q)
    assert np.array_equal(ref.feature[ovr < 0], base.feature[ovr < 0]) and (ref.feature[ovr >= 0] != base.feature[ovr >= 0]).any()


# ---- the graded family -------------------------------------------------------------------------------------------------------
def oracle_rays(p, c):
    with np.errstate(over="ignore"):
        return O.render_rays(p, *X.oracle_inputs(c))


@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
@pytest.mark.parametrize("L,F,H", NETS)
def test_graded_family_keeps_its_rays_and_its_sdf_is_exact(L, F, H, use_sdf):
    p = X.network(L, F, H, use_sdf, graded=True)
    assert p.beta_min == 0 and np.log2(abs(p.beta)) % 1 == 0 and np.log2(X.row0_scale(p)) % 1 == 0
    for S in (17, 65):
        c = X.dense_case(L, F, H, use_sdf, 29, S)
        ref = X.sample_ref(p, c.q)
        X.assert_exact_operands(ref)
        g = X.composite_model(p, c, ref, packed=False)
        assert g.keep.mean() >= 0.9, (S, g.keep.mean())
        if use_sdf:
            a = g.alpha[np.repeat(g.keep, S)]
            assert 0.0179 < a.min() and a.max() < 0.983
        assert (g.rays.weights >= 0).all() and (g.bound.weights > 0).all() and (g.bound.features > 0).all()


@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
@pytest.mark.parametrize("L,F,H", ORACLE_NETS)
def test_graded_reference_holds_the_fp32_oracle_inside_its_bounds(L, F, H, use_sdf):
    p = X.network(L, F, H, use_sdf, graded=True)
    for S in (17, 65):
        c = X.dense_case(L, F, H, use_sdf, 29, S)
        ref = X.sample_ref(p, c.q)
        g = X.composite_model(p, c, ref, packed=False)
        got = oracle_rays(p, c)
        assert np.array_equal(got["feature"].reshape(-1, 32), ref.feature.astype(f32))  # the per-sample part stays exact
        head = got["alpha" if use_sdf else "density"].reshape(-1).astype(np.float64)
        assert (np.abs(head - g.alpha) <= g.alpha_bound).all()
        k = g.keep
        for name, val, bnd in (("weights", g.rays.weights.reshape(c.R, S), g.bound.weights.reshape(c.R, S)),
                               ("features", g.rays.features, g.bound.features), ("depth", g.rays.depth, g.bound.depth),
                               ("accumulation", g.rays.accumulation, g.bound.accumulation)):
            err = np.abs(got[name].astype(np.float64).reshape(val.shape) - val)
            assert (err[k] <= bnd[k]).all(), (name, S, float((err[k] / bnd[k]).max()))
            assert bnd[k].max() <= 1e-4 * np.abs(val[k]).max(), name  # (no vacuous bound: far below the older tolerance)


# ---- the interpolating family ------------------------------------------------------------------------------------------------
def test_interpolating_grids_are_powers_of_two_from_16():
    for (L, F), (mn, mx) in X.INTERP_GRIDS.items():
        sc = O.hash_scalings(L, mn, mx)
        assert sc.shape == (L,) and sc.min() == 16 and (np.log2(sc) % 1 == 0).all(), (L, F, sc)
    assert set(X.INTERP_GRIDS) == set(X.GRIDS)


@pytest.mark.parametrize("L,F,H", NETS)
def test_interpolating_encoding_is_exact_and_the_oracle_is_inside_the_bounds(L, F, H):
    p = X.network(L, F, H, True, interp=True)
    for n, shape in ((1, None), (17, None), (195, (65, 3))):
        c = X.interp_case(n, seed=40, shape=shape)
        assert c.R * c.S == n
        ref = X.interp_ref(p, c)
        assert (ref.enc.astype(f32) == ref.enc).all()  # the float64 lerp has nothing fp32 would round ...
        assert np.array_equal(O.encode_static(p.grid, p.static_scale, *c.rays()), ref.enc.astype(f32))  # ... nor the oracle's
        if n == 195:
            off = O.hashgrid_corner_indices(X.interp_positions(c).astype(f32), p.grid.scalings, p.grid.table_size)[1]
            assert (off * 128 % 1 == 0).all() and (off[:, 0] * 64 % 1 != 0).any() and (ref.enc % 1 != 0).mean() > 0.25
        fld = O.field_fwd(p, *c.rays())
        for name, got in (("feature", fld["feature"].reshape(-1, 32)), ("sdf", fld["sdf"].reshape(-1))):
            assert (np.abs(got - ref.val[name]) <= ref.bound[name]).all(), name
        for pairs in (False, True):  # (the bounds stay far below the older tolerance times the tensor's size)
            r = X.interp_ref(p, c, pairs) if pairs else ref
            assert r.bound["feature"].max() < 0.02 * max(np.abs(r.val["feature"]).max(), 1.0)


def test_interpolating_sh_case():
    p = X.network(8, 4, 32, True, sh=True, interp=True)
    c = X.interp_sh_case(29, 5, seed=41)
    ref = X.interp_ref(p, c)
    assert (ref.enc.astype(f32) == ref.enc).all() and (ref.enc % 1 != 0).any()
    assert np.array_equal(O.encode_static(p.grid, p.static_scale, *c.rays()), ref.enc.astype(f32))
    assert np.allclose(np.linalg.norm(c.d, axis=1), 1, atol=1e-6) and (np.abs(c.d) > 0.01).all(1).any()
    sh = O.sh_deg4(np.repeat((c.d + f32(1)) / f32(2), c.S, 0))
    assert (np.abs(sh - ref.val["sh"]) <= ref.bound["sh"]).all() and ref.bound["sh"].max() < 2e-6
    fld = O.field_fwd(p, *c.rays())
    assert (np.abs(fld["feature"].reshape(-1, 32) - ref.val["feature"]) <= ref.bound["feature"]).all()


# ---- sensitivity: each planted defect passes the older check and fails this one ---------------------------------------------------
DEFECT_NET, DEFECT_R, DEFECT_S = (8, 4, 32), 300, 27  # (one ragged tile behind a full one; what such a ray has left at its
# end -- the last weight, the residual -- is then small enough for the norm and far above the bounds)


@pytest.fixture(scope="module")
def graded_base():
    L, F, H = DEFECT_NET
    p = X.network(L, F, H, True, graded=True)
    c = X.dense_case(L, F, H, True, DEFECT_R, DEFECT_S)
    ref = X.sample_ref(p, c.q)
    return p, c, ref, X.composite_model(p, c, ref, packed=False)


def _weight_column_candidates(p, ref):
    """(unit, input a, input b) of fw1 with different weights on the two inputs, the rarest-firing inputs first"""
    H = ref.hg.shape[1]
    order = np.argsort((ref.hf[:, :H] > 0).mean(0), kind="stable")
    return [(n, int(a), int(b)) for i, a in enumerate(order[:6]) for b in order[i + 1:6] for n in range(H)
            if p.feat_w[2][:, n].any() and p.feat_w[1][n, a] != p.feat_w[1][n, b]]


def _with_rare_units(p, ref, k):
    """the network with the biases of units 3 and 4 of feature layer 0 lowered until each fires at k samples of the case at the
    most: an exchange of their two weights in a unit of fw1 then moves those samples alone"""
    z = ref.emb @ p.feat_w[0][:, :32].astype(np.int64).T + p.feat_b[0].astype(np.int64)
    fb0 = p.feat_b[0].copy()
    for u in (3, 4):
        fb0[u] -= max(int(np.sort(z[:, u])[-k - 1]), 0)
    return dataclasses.replace(p, feat_b=[fb0, *p.feat_b[1:]])


def _defective(p, c, ref, defect):
    """-> (right, defective) evaluations, smaller variants of the defect last"""
    good = X.composite_model(p, c, ref, packed=False)
    if defect == "level_swap":  # at a sample that weighs about 2e-4
        bad = X.sample_ref(p, c.q, defect=("level_swap", 150 * DEFECT_S + 14))
        assert (bad.enc != ref.enc).any()
        yield good, X.composite_model(p, c, bad, packed=False, bounds=False)
    elif defect == "weight_column":
        for k in (64, 16, 4):
            p2 = _with_rare_units(p, ref, k)
            ref2 = X.sample_ref(p2, c.q)
            good2 = X.composite_model(p2, c, ref2, packed=False)
            for n in [n for n in range(ref.hg.shape[1]) if p.feat_w[2][:, n].any() and p.feat_w[1][n, 3] != p.feat_w[1][n, 4]][:4]:
                bad = X.sample_ref(p2, c.q, defect=("weight_column", n, 3, 4))
                yield good2, X.composite_model(p2, c, bad, packed=False, bounds=False)
    else:
        yield good, X.composite_model(p, c, ref, packed=False, defect=defect, bounds=False)


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_defect_passes_the_norm_and_fails_the_bounds(graded_base, defect):
    """weight_column: in a network whose units all fire often, exchanging two weights of one unit moves every sample and the
    norm sees it; the variant that slips through sits on inputs that rarely fire (_with_rare_units), as dead and nearly dead
    units of a trained network do"""
    p, c, ref, _ = graded_base
    found = None
    for good, bad in _defective(p, c, ref, defect):
        assert good.keep.mean() >= 0.9
        pairs = [(getattr(bad.rays, n), getattr(good.rays, n), getattr(good.bound, n))
                 for n in ("weights", "features", "depth", "accumulation")]
        norms = [rel_l2(b, g) for b, g, _ in pairs]
        keep = lambda a: a.reshape(c.R, -1)[good.keep]  # noqa: E731
        flagged = any((keep(np.abs(b - g)) > keep(bd)).any() for b, g, bd in pairs)
        if max(norms) > 0 and max(norms) < TOL:
            found = (norms, flagged)
            if flagged:
                break
    assert found is not None, "no variant of this defect is small enough in norm"
    assert found[1], (defect, found[0])


def test_lattice_comparison_flags_the_per_sample_defects():
    """the same two per-sample defects in the lattice family: one sample's integers change, which bit equality sees and a
    norm over the 300 x 72 samples of the older tests barely does"""
    L, F, H = 8, 4, 32
    p = X.network(L, F, H)
    c = X.dense_case(L, F, H, True, 29, 65)
    ref = X.sample_ref(p, c.q)
    bad = X.sample_ref(p, c.q, defect=("level_swap", 700))
    assert (bad.feature != ref.feature).any(1).sum() == 1 and (bad.enc != ref.enc).any(1).sum() == 1
    n, a, b = _weight_column_candidates(p, ref)[0]
    bad = X.sample_ref(p, c.q, defect=("weight_column", n, a, b))
    assert 0 < (bad.hf != ref.hf).any(1).sum() and np.array_equal(bad.hf[:, :H + n], ref.hf[:, :H + n])
    # the compositing defects move a ray's selected sample: a first hit at S - 1 (depth), no hit at all (sky residual)
    sel = X.selector_ref(p, c, ref, packed=False)
    first = X.first_hits(c, X.is_hit(p, ref.sdf))
    assert (sel.depth[first == 64] == 0).all() and (first == 64).any() and (first == -1).any()
    assert np.array_equal(sel.features[first == -1], ref.feature[c.seg[1:][first == -1] - 1])
