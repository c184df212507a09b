"""The fused render kernel, sample by sample and ray by ray, in every row of csrc/render_variants.h whose source is Static,
EvalTable or Overrides -- fp32 and fp16 tables, SDF and density heads, dense and packed samples, every product form
(NRHIP_MLP_PAIRS / NRHIP_MLP_PAIRS_TRAIN / NRHIP_MLP_SPLIT_BF16).  Cases, references, the exactness argument and the
derivation of every bound: tests/render_exact_refs.py; that the cases are what they claim and that the comparisons made here
tell wrong kernels apart: tests/test_render_exact_refs_host.py.

Lattice family: every output and every saved activation bit for bit against the int64 reference, written into NaN-filled
buffers between guard values (an unwritten element and a write outside both show).  Graded family: every per-ray output and
every weight within its own bound of the float64 reference.  Interpolating family: the saved encoding rows bit for bit
against the float64 lerp, the activations behind them within their forward interval bounds.  All product forms return the same bits on the lattice family,
so these tests cannot say which kernel ran: tests/test_gpu_render_variants.py does that.

The eval-table rows run on the lattice family's 2^11-entry tables, where no level qualifies for a shadow copy (64^3 lattice
points against 2^11 entries): their table is the plain re-layout the library builds for such a grid, every level under the
reference hash; one more case at T = 2^21 reads level 0 from a real shadow copy.  The rows with actor sources (Actors,
PackedActors) are not covered here.

Measured on an MI355X (printed by the tests, largest over their cases): every lattice comparison holds bit for bit in every
row; graded family, err / bound <= 0.09 features, 0.17 depth, 0.14 accumulation, 0.47 weights; interpolating family, `enc` bit
for bit, err / bound <= 0.08 hg, 0.03 emb, 0.30 SH, 0.01 hf, 0.03 sdf, 0.001 feature (a forward interval bound through |W| is a
worst case over signs: it grows by a layer's absolute row sums, the error does not)."""
import functools

import numpy as np
import pytest
import torch

import render_exact_refs as X
from gpu_util import dev, host64, to_spec
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GUARD = 12345.0
S_ALL = (1, 15, 16, 17, 63, 64, 65, 129)
R_SMALL = (1, 3, 5)
R_LARGE, S_LARGE = 4133, 17  # more rays than resident waves: every wave walks several rays, the eight ranges are uneven


def row_id(r):
    return "%dx%d-H%d-%s-%s-%s" % r


def select_form(switches, prod, out):
    """the switches under which the dispatcher prefers `prod` for a static-scene row (render.hip: choose_variant)"""
    switches.unset("NRHIP_MLP_SPLIT_BF16")
    switches.unset("NRHIP_MLP_PAIRS_TRAIN")
    switches.set("NRHIP_MLP_PAIRS", "1" if prod == "F16Pairs" else "0")
    if prod == "F16Pairs" and out == "PerSample":
        switches.set("NRHIP_MLP_PAIRS_TRAIN", "1")
    if prod == "Bf16Split":
        switches.set("NRHIP_MLP_SPLIT_BF16", "1")


def plain_eval_table(ops):
    """ops.eval_table without its "no level qualifies" exit: the re-layout of a grid whose levels all keep the reference hash"""
    def build(spec, table):
        lay, rows, _ = ops.eval_layout_plan(spec, table.dtype)
        out = torch.empty((rows, spec.features_per_level), device=table.device, dtype=table.dtype)
        ops.launch("nrhip_eval_layout_build", spec.c_grid(table), table, lay, out)
        return out, lay
    return build


class Guarded:
    """NaN-filled output windows, 32 bytes into buffers of guard values"""

    def __init__(self):
        self.bufs = []

    def new(self, *shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 16,), GUARD, device="cuda")
        win = buf[8:8 + n]
        win.fill_(float("nan"))
        self.bufs.append((buf, n))
        return win.view(*shape)

    def intact(self):
        return all(bool((b[:8] == GUARD).all() and (b[8 + n:] == GUARD).all()) for b, n in self.bufs)


def same(got, want, what):
    want = dev(np.asarray(want, np.float64)).reshape(got.shape)
    if not torch.equal(got, want):
        bad = torch.nonzero(~(got == want))
        raise AssertionError(f"{what}: {bad.shape[0]} elements differ, first at {bad[:4].tolist()}: "
                             f"{got[tuple(bad[0])].item()} != {want[tuple(bad[0])].item()}")


def rays_of(case, edge_views=False):
    o, d, a = dev(case.o), dev(case.d), dev(case.area)
    if edge_views:
        e = dev(case.edges())
        return o, d, a, e[:, :-1], e[:, 1:]
    s, t = case.dense()
    return o, d, a, dev(s), dev(t)


def orders_of(R):
    g = np.random.default_rng([R, 11])
    return [None, torch.arange(R - 1, -1, -1, device="cuda", dtype=torch.int32),
            torch.from_numpy(g.permutation(R).astype(np.int32)).cuda()]


def override_of(L, F, case):
    ovr, rows, dirs = X.override_case(L, F, case)
    return (ovr, rows), (torch.from_numpy(ovr).cuda(), dev(rows), dev(dirs))


# ---- launches on this test's own buffers ---------------------------------------------------------------------------------------
def per_sample(ops, fs, case, packed, train, order=None, override=None, edge_views=False):
    """nrhip_field_fwd / nrhip_field_fwd_train[_packed][_ovr] -> dict of outputs and saved rows"""
    if packed:
        ts, te, seg = case.packed()
        r, keep = ops._c_packed_rays("test", dev(case.o), dev(case.d), dev(case.area), dev(ts), dev(te),
                                     torch.from_numpy(seg).cuda(), order)
    else:
        r, keep = ops._c_rays(*rays_of(case, edge_views), order)
    f, keep2 = fs.c_field()
    n, H, LF = len(case.t), fs.geo_w[0].shape[0], fs.grid.out_dim
    g = Guarded()
    out = {"feature": g.new(n, 32), "sdf": g.new(n), "head": g.new(n)}
    if train:
        out.update(enc=g.new(n, LF), hg=g.new(n, H), xf=g.new(n, 48), hf=g.new(n, 2 * H))
    name = "nrhip_field_fwd_train" + ("_packed" if packed else "") if train else "nrhip_field_fwd"
    if override is not None:
        ops.launch(name + "_ovr", f, r, *override, *out.values())
    else:
        ops.launch(name, f, r, *out.values())
    torch.cuda.synchronize()
    assert g.intact(), "a write outside the outputs"
    return out


def check_per_sample(p, out, ref, what):
    hit = X.is_hit(p, ref.sdf)
    same(out["feature"], ref.feature, what + " feature")
    same(out["sdf"], ref.sdf, what + " sdf")
    same(out["head"], hit if p.use_sdf else np.where(hit, np.inf, 0.0), what + " head")
    if "enc" in out:
        same(out["enc"], ref.enc, what + " enc")
        same(out["hg"], ref.hg, what + " hg")
        same(out["xf"][:, :32], ref.emb, what + " xf[:, :32]")
        same(out["hf"], ref.hf, what + " hf")
        assert bool(torch.isfinite(out["xf"][:, 32:]).all()), what + " xf[:, 32:] not written"


def composite(ops, fs, case, packed, order=None, eps=0.0, edge_views=False):
    """nrhip_render_fwd_ex / nrhip_render_fwd_packed -> features, depth, accumulation, weights"""
    if packed:
        ts, te, seg = case.packed()
        r, keep = ops._c_packed_rays("test", dev(case.o), dev(case.d), dev(case.area), dev(ts), dev(te),
                                     torch.from_numpy(seg).cuda(), order)
        f, keep2 = fs.c_field()
    else:
        r, keep = ops._c_rays(*rays_of(case, edge_views), order)
        f, keep2 = fs.c_field(eval_layout=True)
    g = Guarded()
    out = (g.new(case.R, 32), g.new(case.R, 1), g.new(case.R, 1), g.new(len(case.t)))
    ops.launch("nrhip_render_fwd_packed" if packed else "nrhip_render_fwd_ex", f, r, *out, float(eps))
    torch.cuda.synchronize()
    assert g.intact(), "a write outside the outputs"
    return out


def check_composite(out, sel, what):
    for got, want, name in zip(out, (sel.features, sel.depth, sel.accumulation, sel.weights),
                               ("features", "depth", "accumulation", "weights")):
        same(got, want, f"{what} {name}")


@functools.lru_cache(maxsize=64)
def dense_ref(L, F, H, use_sdf, R, S):
    """a dense lattice case and its reference, computed once for the tests that share it"""
    c = X.dense_case(L, F, H, use_sdf, R, S)
    return c, X.sample_ref(X.network(L, F, H, use_sdf), c.q)


def dense_cases(L, F, H, use_sdf):
    return [dense_ref(L, F, H, use_sdf, 29, S) for S in S_ALL] + [dense_ref(L, F, H, use_sdf, R, 17) for R in R_SMALL]


HEADS = pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
HALF = pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])


# ---- lattice family, per-sample kernels ------------------------------------------------------------------------------------------
@HEADS
@HALF
@pytest.mark.parametrize("row", X.rows(outputs=("PerSample",)), ids=row_id)
def test_lattice_per_sample_rows(ops, switches, row, half, use_sdf):
    L, F, H, _, src, prod = row
    select_form(switches, prod, "PerSample")
    p = X.network(L, F, H, use_sdf)
    fs = to_spec(ops, p, half)
    ovr = src == "Overrides"
    for c, ref in dense_cases(L, F, H, use_sdf):
        S = int(c.counts[0])
        what = f"dense R={c.R} S={S}"
        od = None
        if ovr:
            oh, od = override_of(L, F, c)
            ref = X.sample_ref(p, c.q, *oh)
        X.assert_exact_operands(ref)
        check_per_sample(p, per_sample(ops, fs, c, False, True, override=od), ref, what + " train")
        if not ovr:
            check_per_sample(p, per_sample(ops, fs, c, False, False), ref, what + " field_fwd")
        if S == 17:
            for order in orders_of(c.R)[1:]:
                check_per_sample(p, per_sample(ops, fs, c, False, True, order, od), ref, what + " ordered")
    if prod != "F32":
        return  # packed rows: fp32 products only (render_variant_ok)
    for name, counts in X.PACKED_COUNTS.items():
        c = X.packed_case(L, F, H, use_sdf, counts)
        (oh, od) = override_of(L, F, c) if ovr else ((None, None), None)
        ref = X.sample_ref(p, c.q, *oh)
        for order in orders_of(c.R) if name == "mixed" else [None]:
            check_per_sample(p, per_sample(ops, fs, c, True, True, order, od), ref, f"packed {name}")


# ---- lattice family, composited kernels ------------------------------------------------------------------------------------------
@HEADS
@HALF
@pytest.mark.parametrize("row", X.rows(outputs=("Composite",)), ids=row_id)
def test_lattice_composite_rows(ops, switches, monkeypatch, row, half, use_sdf):
    L, F, H, _, src, prod = row
    select_form(switches, prod, "Composite")
    if src == "EvalTable":
        monkeypatch.setattr(ops, "eval_table", plain_eval_table(ops))
    p = X.network(L, F, H, use_sdf)
    fs = to_spec(ops, p, half)
    for c, ref in dense_cases(L, F, H, use_sdf):
        S = int(c.counts[0])
        what = f"dense R={c.R} S={S}"
        X.assert_exact_operands(ref, split=prod == "Bf16Split")
        sel = X.selector_ref(p, c, ref, packed=False)
        check_composite(composite(ops, fs, c, False), sel, what)
        for eps in (1e-3, 0.5) if S in (17, 65, 129) else ():  # early termination: the same bits, zeros behind the stop
            check_composite(composite(ops, fs, c, False, eps=eps), sel, f"{what} stop_eps={eps}")
        if S == 17:
            for order in orders_of(c.R)[1:]:
                check_composite(composite(ops, fs, c, False, order), sel, what + " ordered")
    c = X.edge_case(29, 17, half=0.5)  # starts / ends as views of one [R, S + 1] edge tensor
    r = rays_of(c, edge_views=True)
    assert r[3].stride(0) == 18 and r[3].data_ptr() + 4 == r[4].data_ptr()
    sel = X.selector_ref(p, c, X.sample_ref(p, c.q), packed=False)
    check_composite(composite(ops, fs, c, False, edge_views=True), sel, "edge views")
    if src != "Static" or prod == "Bf16Split":
        return  # packed samples: the static-scene kernel with fp32 or pair products (render_variant_ok)
    for name, counts in X.PACKED_COUNTS.items():
        c = X.packed_case(L, F, H, use_sdf, counts)
        sel = X.selector_ref(p, c, X.sample_ref(p, c.q), packed=True)
        empty = torch.from_numpy(c.counts == 0).cuda()
        for order in orders_of(c.R) if name == "mixed" else [None]:
            for eps in (0.0, 1e-3, 0.5) if name in ("mixed", "many") else (0.0,):
                out = composite(ops, fs, c, True, order, eps)
                check_composite(out, sel, f"packed {name} stop_eps={eps}")
                assert not out[0][empty].any() and not out[1][empty].any() and not out[2][empty].any()


def test_lattice_eval_table_with_a_shadow_level(ops, switches, monkeypatch):
    """the one thing the 2^11-entry tables cannot reach: a level read from its shadow copy.  At T = 2^21 level 0 of the 8 x 4
    ladder (scaling 64: coordinates of 7 bits) qualifies, its lattice point (ix, iy, iz) sits at row ix | iy << 7 | iz << 14
    of the eval table; the other seven levels keep the reference hash.  fp16 storage keeps the table at 128 MiB"""
    L, F, H, lg = 8, 4, 32, 21
    select_form(switches, "F32", "Composite")
    monkeypatch.setattr(ops, "_EVAL_RELAYOUT", True)
    monkeypatch.setattr(ops, "_EVAL_TABLES", {})
    p = X.network.__wrapped__(L, F, H, True, lg=lg)
    fs = to_spec(ops, p, half=True)
    lay, rows, n_shadow = ops.eval_layout_plan(fs.grid, torch.float16)
    assert n_shadow == 1 and lay[0] == 1 << 7 and rows == (1 << 21) + 7 * (1 << 21)
    hits = X.classify_lattice(p)
    for S in (17, 65):
        c = X.ray_lists(hits, [S] * 29, seed=0)
        ref = X.sample_ref(p, c.q)
        sel = X.selector_ref(p, c, ref, packed=False)
        assert sel.weights.sum() >= 20
        check_composite(composite(ops, fs, c, False), sel, f"shadow level S={S}")
    assert len(ops._EVAL_TABLES) == 1  # (the eval table was built and used)


def test_edge_views_per_sample(ops, switches):
    L, F, H = 8, 4, 32
    select_form(switches, "F32", "PerSample")
    p = X.network(L, F, H)
    c = X.edge_case(29, 17, half=0.5)
    check_per_sample(p, per_sample(ops, to_spec(ops, p), c, False, True, edge_views=True), X.sample_ref(p, c.q), "edge views")


# ---- more rays than resident waves -----------------------------------------------------------------------------------------------
LARGE = [r for r in X.rows(outputs=("Composite",), sources=("Static",)) if r[:3] in ((8, 4, 32), (16, 2, 64), (4, 2, 32))]


@pytest.mark.parametrize("row", LARGE, ids=row_id)
def test_lattice_more_rays_than_waves(ops, switches, row):
    L, F, H, _, _, prod = row
    p = X.network(L, F, H)
    fs = to_spec(ops, p)
    c, ref = dense_ref(L, F, H, True, R_LARGE, S_LARGE)
    X.assert_exact_operands(ref, split=prod == "Bf16Split")
    sel = X.selector_ref(p, c, ref, packed=False)
    select_form(switches, prod, "Composite")
    for order in orders_of(c.R):
        check_composite(composite(ops, fs, c, False, order), sel, "dense")
    if prod != "Bf16Split":
        check_composite(composite(ops, fs, c, True), X.selector_ref(p, c, ref, packed=True), "packed")
    if prod == "F32" or (L, F, H, "PerSample", "Static", prod) in X.rows():
        select_form(switches, prod, "PerSample")
        check_per_sample(p, per_sample(ops, fs, c, False, True, orders_of(c.R)[2]), ref, "train")
        if prod == "F32":
            check_per_sample(p, per_sample(ops, fs, c, True, True), ref, "train packed")


# ---- graded family ---------------------------------------------------------------------------------------------------------------
@HEADS
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("row", X.rows(outputs=("Composite",), sources=("Static",), products=("F32", "F16Pairs")), ids=row_id)
def test_graded_composite_rows(ops, switches, row, packed, use_sdf):
    L, F, H, _, _, prod = row
    select_form(switches, prod, "Composite")
    p = X.network(L, F, H, use_sdf, graded=True)
    fs = to_spec(ops, p)
    worst = {}
    for S in (17, 65):
        c = X.dense_case(L, F, H, use_sdf, 29, S)
        ref = X.sample_ref(p, c.q)
        X.assert_exact_operands(ref)
        g = X.composite_model(p, c, ref, packed)
        assert g.keep.mean() >= 0.9
        out = composite(ops, fs, c, packed)
        k = g.keep
        for got, name in zip(out, ("features", "depth", "accumulation", "weights")):
            val, bnd = getattr(g.rays, name).reshape(c.R, -1), getattr(g.bound, name).reshape(c.R, -1)
            err = np.abs(host64(got).reshape(c.R, -1) - val)
            worst[name] = max(worst.get(name, 0.0), float((err[k] / bnd[k]).max()))
            over = np.argwhere(~(err[k] <= bnd[k]))
            assert not len(over), (name, S, len(over), over[:4].tolist(), float((err[k] / bnd[k]).max()))
    print(f"\n[graded {row_id(row)} {'packed' if packed else 'dense'} {'sdf' if use_sdf else 'density'}] err / bound <= "
          + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))


# ---- interpolating family --------------------------------------------------------------------------------------------------------
def interp_launch(ops, fs, c, packed):
    """nrhip_field_fwd_train / _packed (every ray S samples) on guarded buffers"""
    n, H, LF = c.R * c.S, fs.geo_w[0].shape[0], fs.grid.out_dim
    if packed:
        seg = torch.arange(c.R + 1, device="cuda", dtype=torch.int64) * c.S
        r, keep = ops._c_packed_rays("test", dev(c.o), dev(c.d), dev(c.area), dev(c.starts), dev(c.ends), seg)
    else:
        r, keep = ops._c_rays(dev(c.o), dev(c.d), dev(c.area), dev(c.starts), dev(c.ends))
    f, keep2 = fs.c_field()
    g = Guarded()
    out = {"feature": g.new(n, 32), "sdf": g.new(n), "head": g.new(n), "enc": g.new(n, LF), "hg": g.new(n, H),
           "xf": g.new(n, 48), "hf": g.new(n, 2 * H)}
    ops.launch("nrhip_field_fwd_train_packed" if packed else "nrhip_field_fwd_train", f, r, *out.values())
    torch.cuda.synchronize()
    assert g.intact(), "a write outside the outputs"
    return out


def check_interp(out, ref, what, worst):
    same(out["enc"], ref.enc, what + " enc")
    got = {"hg": out["hg"], "emb": out["xf"][:, :32], "sh": out["xf"][:, 32:], "hf": out["hf"], "sdf": out["sdf"],
           "feature": out["feature"]}
    for name, t in got.items():
        err = np.abs(host64(t) - ref.val[name])
        bnd = ref.bound[name]
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[name] = max(worst.get(name, 0.0), float(np.nan_to_num(err / bnd).max()))
        over = np.argwhere(~(err <= bnd))
        assert not len(over), (what, name, len(over), over[:4].tolist())
    assert bool(torch.isfinite(out["head"]).all())


@HALF
@pytest.mark.parametrize("row", X.rows(outputs=("PerSample",), sources=("Static",)), ids=row_id)
def test_interpolating_per_sample_rows(ops, switches, row, half):
    L, F, H, _, _, prod = row
    select_form(switches, prod, "PerSample")
    p = X.network(L, F, H, True, interp=True)
    fs = to_spec(ops, p, half)
    worst = {}
    for n, shape in ((1, None), (17, None), (195, (65, 3))):
        c = X.interp_case(n, seed=40, shape=shape)
        ref = X.interp_ref(p, c, pairs=prod == "F16Pairs")
        check_interp(interp_launch(ops, fs, c, False), ref, f"dense n={n}", worst)
        if prod == "F32":
            check_interp(interp_launch(ops, fs, c, True), ref, f"packed n={n}", worst)
    print(f"\n[interp {row_id(row)} {'fp16' if half else 'fp32'}] err / bound <= " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_interpolating_sh_columns(ops, switches):
    """nonzero SH columns in fw0, directions from synth.rays, every sample at its ray's origin: the SH values within a few U
    per polynomial term, and through them feature layer 0 and the feature"""
    L, F, H = 8, 4, 32
    select_form(switches, "F32", "PerSample")
    p = X.network(L, F, H, True, sh=True, interp=True)
    assert p.feat_w[0][:, 32:].any()
    c = X.interp_sh_case(29, 5, seed=41)
    worst = {}
    ref = X.interp_ref(p, c)
    for packed in (False, True):
        check_interp(interp_launch(ops, to_spec(ops, p), c, packed), ref, "sh", worst)
    print("\n[interp sh] err / bound <= " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
