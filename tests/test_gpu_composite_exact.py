"""The per-ray compositing and glue kernels at every channel-width branch, per element (cases, references and bounds:
tests/composite_refs.py; their own checks: tests/test_composite_refs_host.py).

  accumulate_kernel / accumulate_bwd_kernel   flat C = 1 .. 64, generic C = 3 / 12, 65 / 100 (the ch += 64 stride steps), 512;
                                              values = None; gw only, gv only
  composite_fwd_kernel / composite_bwd_kernel the same widths and the float4 path at LP = 1 .. 64 (C = 4 .. 256), C = 512 (LP = 128:
                                              falls back), features one float off the 16-byte grid; gD, gA absent; gf not wanted
  sdf_render_fwd / _bwd and their pair forms  float4 LP = 1 .. 64, flat C = 1, 2 and misaligned, generic, rays that part ways on an odd
                                              row stride; S = 2 .. 129 across the 64-sample carry, 1024 and 2048; both heads;
                                              NRHIP_SDF_RENDER_PAIR 0 and 1; the unsupported error one past each limit
  prop_weights_fwd / _bwd                     S = 1 .. 193 (the carry loop of the backward runs three times), gw only, gdepth only,
                                              edge rows wider than S + 1
  appearance_fwd / _bwd, embedding_lerp       the LDS image at exactly 8192 cells, one row over (global atomics), the grid-stride
                                              loop's second step, the clamp of bad sensor indices beside sentinel rows, temporal
                                              without times
Two families per case: the LATTICE family has one right answer per element and is compared bit for bit, outputs prefilled
with NaN, a second run held to the first; the GRADED family is held per element to a float64 reference within a bound
that counts roundings.  Every graded test prints its worst err / bound."""
import numpy as np
import pytest
import torch

import composite_refs as CR
from gpu_util import cuda, dev, host
from gpu_util import ops  # noqa: F401  (fixture)
from sharp_refs import check

pytestmark = pytest.mark.gpu
FAMILIES = ("lattice", "graded")


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def off1(a):
    """`a` on the device as a contiguous view one float off the 16-byte grid"""
    buf = torch.empty(a.size + 8, device="cuda", dtype=torch.float32)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(dev(a))
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def inputs(c, family):
    return CR.lattice_inputs(c) if family == "lattice" else CR.graded_inputs(c)


def compare(c, family, got, ref):
    """got: {name or "name|variant": tensor}; ref: {name: value} (lattice) or {name: (value, bound)} (graded)"""
    ratios = {}
    for k, t in got.items():
        name = k.split("|")[0]
        if name not in ref:
            assert not torch.isnan(t).any(), f"{c.id} {k}: unwritten elements"
            continue
        if family == "lattice":
            CR.same(host(t), ref[name], f"{c.id} {k}")
        else:
            v, bound = ref[name]
            ratios[k] = CR.worst(host(t), v, bound)
    if family == "graded":
        print(f"\n{c.op} {c.id}: worst err/bound " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()), end="")
        for k, t in got.items():
            name = k.split("|")[0]
            if name in ref:
                check(host(t), ref[name][0], ref[name][1], f"{c.id} {k}")


def twice(run, *args):
    """run a kernel set twice: the second run's bits are the first's"""
    a, b = run(*args), run(*args)
    for k in a:
        assert torch.equal(a[k], b[k]) or torch.isnan(a[k]).any(), f"{k}: a second run differs"
    return a


def params(cases):
    return [pytest.param(c, f, id=f"{c.id}-{f}") for c in cases for f in FAMILIES]


# ---- accumulate_along_rays ----------------------------------------------------------------------------------------------
def run_accumulate(ops, c, d):
    R, S, C = c.R, c.S, c.C
    w, v, g = dev(d["w"]), dev(d["f"]), dev(d["gF"])
    out, sw = nan(R, C), nan(R, 1)
    ops.launch("nrhip_accumulate_along_rays", w, v, R, S, C, out)
    ops.launch("nrhip_accumulate_along_rays", w, None, R, S, 1, sw)
    gw, gv, gw1, gv1 = nan(R, S), nan(R, S, C), nan(R, S), nan(R, S, C)
    ops.launch("nrhip_accumulate_along_rays_bwd", w, v, g, R, S, C, gw, gv)
    ops.launch("nrhip_accumulate_along_rays_bwd", w, v, g, R, S, C, gw1, None)
    ops.launch("nrhip_accumulate_along_rays_bwd", w, v, g, R, S, C, None, gv1)
    return {"out": out, "sum w": sw, "d weights": gw, "d values": gv, "d weights|gw only": gw1, "d values|gv only": gv1}


@pytest.mark.parametrize("c,family", params(CR.ACC_CASES))
def test_accumulate(ops, c, family):
    d = inputs(c, family)
    got = twice(run_accumulate, ops, c, d)
    compare(c, family, got, CR.lattice_ref(c, d) if family == "lattice" else CR.graded_accumulate(c, d))
    # the wrappers launch the same thing
    assert torch.equal(ops.accumulate_along_rays(dev(d["w"]), dev(d["f"])), got["out"])
    assert torch.equal(ops.accumulate_along_rays(dev(d["w"])), got["sum w"])
    gw, gv = ops.accumulate_along_rays_bwd(dev(d["w"]), dev(d["f"]), dev(d["gF"]))
    assert torch.equal(gw, got["d weights"]) and torch.equal(gv, got["d values"])


# ---- composite_fwd / composite_bwd --------------------------------------------------------------------------------------
def run_composite(ops, c, d):
    R, S, C = c.R, c.S, c.C
    st, en = (dev(v) for v in CR.bins(d, S))
    w, g, gD, gA = dev(d["w"]), dev(d["gF"]), dev(d["gD"]), dev(d["gA"])
    f = off1(d["f"]) if c.align == "feat_off" else dev(d["f"])
    of, od, oa = nan(R, C), nan(R, 1), nan(R, 1)
    ops.launch("nrhip_composite_fwd", w, f, st, en, R, S, C, of, od, oa)
    gw, gf, gw1, gw2, gf2 = nan(R, S), nan(R, S, C), nan(R, S), nan(R, S), nan(R, S, C)
    ops.launch("nrhip_composite_bwd", w, f, st, en, g, gD, gA, R, S, C, gw, gf)
    ops.launch("nrhip_composite_bwd", w, f, st, en, g, gD, gA, R, S, C, gw1, None)  # gf not wanted
    ops.launch("nrhip_composite_bwd", w, f, st, en, g, None, None, R, S, C, gw2, gf2)  # gD, gA absent
    return {"acc": oa, "features": of, "depth": od, "d features": gf, "d weights": gw, "d weights|no gf": gw1,
            "d features|no gD gA": gf2, "d weights 0|no gD gA": gw2}


def composite_ref(c, family, d):
    ref = CR.lattice_ref(c, d) if family == "lattice" else CR.graded_composite(c, d)
    st, en = CR.bins(d, c.S)
    w2, _, _, _, mid = CR.ref_composite(d["w"], d["f"], st, en)
    _, gw0, mag0 = CR.ref_composite_bwd(w2, d["f"], mid, d["gF"])
    ref["d weights 0"] = gw0 if family == "lattice" else (gw0, 2 * (c.C + 4) * CR.U * mag0)
    return ref


@pytest.mark.parametrize("c,family", params(CR.COMP_CASES))
def test_composite(ops, c, family):
    d = inputs(c, family)
    got = twice(run_composite, ops, c, d)
    compare(c, family, got, composite_ref(c, family, d))
    if c.align == "feat_off":  # the misaligned call leaves the float4 path and gives the aligned call's bits
        assert CR.branches(c, "composite_bwd") == {(CR.feature_path("composite_bwd", c.C, False), "misaligned")}
        if family == "lattice":
            twin = run_composite(ops, CR.Case(c.op, c.R, c.S, c.C), d)
            assert all(torch.equal(twin[k], got[k]) for k in got)
    else:
        st, en = (dev(v) for v in CR.bins(d, c.S))
        of, od, oa = ops.composite_fwd(dev(d["w"]), dev(d["f"]), st, en)
        assert torch.equal(of, got["features"]) and torch.equal(od, got["depth"]) and torch.equal(oa, got["acc"])
        gw, gf = ops.composite_bwd(dev(d["w"]), dev(d["f"]), st, en, dev(d["gF"]), dev(d["gD"]), dev(d["gA"]))
        assert torch.equal(gw, got["d weights"]) and torch.equal(gf, got["d features"])
        gw, gf = ops.composite_bwd(dev(d["w"]), dev(d["f"]), st, en, dev(d["gF"]), need_grad_features=False)
        assert gf is None and torch.equal(gw, got["d weights 0|no gD gA"])


# ---- sdf_render ---------------------------------------------------------------------------------------------------------
def run_sdf_render(ops, c, d):
    R, S, C = c.R, c.S, c.C
    x, e = dev(d["x"]), dev(d["e"])
    beta = dev(d["beta"]) if c.head == "sdf" else None
    bmin = float(d.get("beta_min", 0.0))
    f = off1(d["f"]) if c.align == "feat_off" else dev(d["f"])
    extra = 1 if c.align == "odd_out" else 0
    alpha, w_ns, out, depth, acc = nan(R, S), nan(R, S - 1), nan(R, C + extra), nan(R, 1), nan(R, 1)
    ops.launch("nrhip_sdf_render_fwd", x, beta, bmin, f, e, e.shape[1], R, S, C, alpha, w_ns, out, C + extra, depth, acc)
    assert torch.isnan(out[:, C:]).all(), "the column beside the written block was touched"
    got = {"alpha": alpha, "w_ns": w_ns, "out": out[:, :C].contiguous(), "depth": depth, "acc": acc}
    if not CR.has_backward(c):
        return got
    if c.align == "odd_g":  # gF as a column block of a wider row with an odd stride
        gbuf = nan(R, C + 1)
        gbuf[:, :C] = dev(d["gF"])
        g, gs = gbuf[:, :C], C + 1
    else:
        g, gs = dev(d["gF"]), C
    gfeat, gsdf = nan(R, S, C), nan(R, S)
    gbeta = nan(1) if c.head == "sdf" else None
    ws, _ = ops._workspace("nrhip_sdf_render_bwd_workspace", R, device=x.device, dtype=torch.float32)
    ops.launch("nrhip_sdf_render_bwd", x, beta, bmin, alpha, f, e, e.shape[1], g, gs, dev(d["gD"]), dev(d["gA"]),
               dev(d["gWns"]), R, S, C, gfeat, gsdf, gbeta, ws)
    got.update({"gfeat": gfeat, "gsdf": gsdf})
    if gbeta is not None:
        got["gbeta"] = gbeta
    return got


def sdf_ref(c, family, d, got):
    if family == "lattice":
        return CR.lattice_ref(c, d)
    ra, bound = CR.graded_alpha(c, d)
    ref = CR.graded_sdf_render(c, d, host(got["alpha"]))
    ref["alpha"] = (ra, bound)
    return ref


def sdf_params(cases):
    """every case with the switch off; the cases the switch can move (C = 32, S <= 33) with it on as well"""
    return [pytest.param(c, f, p, id=f"{c.id}-{f}-pair{p}") for c in cases for f in FAMILIES
            for p in ("0", "1") if p == "0" or (c.C == 32 and c.S <= 33)]


@pytest.mark.parametrize("c,family,pair", sdf_params(CR.SDF_CASES))
def test_sdf_render(ops, switches, c, family, pair):
    switches.set("NRHIP_SDF_RENDER_PAIR", pair)
    d = inputs(c, family)
    got = twice(run_sdf_render, ops, c, d)
    compare(c, family, got, sdf_ref(c, family, d, got))
    if c.align == "aligned" and CR.has_backward(c):  # the wrappers launch the same thing
        beta = dev(d["beta"]) if c.head == "sdf" else None
        bmin = float(d.get("beta_min", 0.0))
        a, w_ns, out, depth, acc = ops.sdf_render_fwd(dev(d["x"]), beta, bmin, dev(d["f"]), dev(d["e"]))
        for k, t in (("alpha", a), ("w_ns", w_ns), ("out", out), ("depth", depth), ("acc", acc)):
            assert torch.equal(t, got[k]), k
        gfeat, gsdf, gbeta = ops.sdf_render_bwd(dev(d["x"]), beta, bmin, a, dev(d["f"]), dev(d["e"]), dev(d["gF"]),
                                                dev(d["gD"]), dev(d["gA"]), dev(d["gWns"]))
        assert torch.equal(gfeat, got["gfeat"]) and torch.equal(gsdf, got["gsdf"])
        assert (gbeta is None) == (c.head == "density") and (gbeta is None or torch.equal(gbeta, got["gbeta"]))


@pytest.mark.parametrize("pair", ["0", "1"])
@pytest.mark.parametrize("c", CR.SDF_ALIGN, ids=lambda c: c.id)
def test_sdf_render_alignment(ops, switches, c, pair):
    """features one float off, an odd output stride, gF in a wider odd row: the launch leaves the pair kernels (where the
    misaligned pointer is that kernel's), rays take the path their own row's alignment gives, and the lattice family's
    bits are the aligned call's"""
    switches.set("NRHIP_SDF_RENDER_PAIR", pair)
    twin = CR.Case(c.op, c.R, c.S, c.C)
    on = pair == "1"
    stride = c.C + (c.align != "feat_off")
    for kernel, mine in (("sdf_render_fwd", ("feat_off", "odd_out")), ("sdf_render_bwd", ("feat_off", "odd_g"))):
        if c.align in mine:
            assert not CR.pair_taken(c.S, c.C, stride, c.align != "feat_off", on)
            assert not CR.case_pair(c, kernel, on)
            assert CR.branches(c, kernel, on) != CR.branches(twin, kernel, on)
        else:
            assert CR.case_pair(c, kernel, on) == CR.case_pair(twin, kernel, on)
    d = CR.lattice_inputs(c)
    got, want = run_sdf_render(ops, c, d), run_sdf_render(ops, twin, d)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # the same through the wrappers: extra_cols = 1 is the odd output stride, and g_out may be any [R, C] view
    x, beta, f, e = dev(d["x"]), dev(d["beta"]), (off1(d["f"]) if c.align == "feat_off" else dev(d["f"])), dev(d["e"])
    a, w_ns, out, depth, acc = ops.sdf_render_fwd(x, beta, 0.0, f, e, extra_cols=1 if c.align == "odd_out" else 0)
    assert out.shape == (c.R, c.C + (c.align == "odd_out"))
    for k, t in (("alpha", a), ("w_ns", w_ns), ("out", out[:, :c.C]), ("depth", depth), ("acc", acc)):
        assert torch.equal(t, want[k]), k
    g = dev(d["gF"])
    if c.align == "odd_g":
        g = torch.cat([g, nan(c.R, 1)], -1)[:, :c.C]
        assert g.stride(0) == c.C + 1
    gfeat, gsdf, gbeta = ops.sdf_render_bwd(x, beta, 0.0, a, f, e, g, dev(d["gD"]), dev(d["gA"]), dev(d["gWns"]))
    assert torch.equal(gfeat, want["gfeat"]) and torch.equal(gsdf, want["gsdf"]) and torch.equal(gbeta, want["gbeta"])


def test_sdf_render_refuses_one_sample_past_its_limits(ops):
    """S = 2049 forward, S = 1025 backward: NRHIP_ERR_UNSUPPORTED, and nothing is launched -- the outputs keep their NaNs"""
    from neurad_studio_amd._lib import NeuradHipError

    R, C = 1, 4
    beta = dev(np.array([1.0], np.float32))
    for S, fwd_ok in ((CR.S_FWD_MAX + 1, False), (CR.S_BWD_MAX + 1, True)):
        x, f, e = torch.zeros(R, S, device="cuda"), torch.ones(R, S, C, device="cuda"), dev(CR.int_edges(R, S, 1))
        outs = [nan(R, S), nan(R, S - 1), nan(R, C), nan(R, 1), nan(R, 1)]
        fwd = lambda: ops.launch("nrhip_sdf_render_fwd", x, beta, 0.0, f, e, S + 1, R, S, C, outs[0], outs[1], outs[2], C,  # noqa: E731
                                 outs[3], outs[4])
        if fwd_ok:
            fwd()
            assert not any(torch.isnan(t).any() for t in outs)
        else:
            with pytest.raises(NeuradHipError, match=rf"code {CR.ERR_UNSUPPORTED}\).*max {CR.S_FWD_MAX}"):
                fwd()
            with pytest.raises(NeuradHipError, match=rf"code {CR.ERR_UNSUPPORTED}\)"):
                ops.sdf_render_fwd(x, beta, 0.0, f, e)
            assert all(torch.isnan(t).all() for t in outs)
        alpha = torch.full((R, S), 0.5, device="cuda")
        gouts = [nan(R, S, C), nan(R, S), nan(1)]
        ws = torch.zeros(4, device="cuda")
        with pytest.raises(NeuradHipError, match=rf"code {CR.ERR_UNSUPPORTED}\).*max {CR.S_BWD_MAX}"):
            ops.launch("nrhip_sdf_render_bwd", x, beta, 0.0, alpha, f, e, S + 1, torch.ones(R, C, device="cuda"), C, None, None,
                       None, R, S, C, gouts[0], gouts[1], gouts[2], ws)
        assert all(torch.isnan(t).all() for t in gouts) and (ws == 0).all()


# ---- prop_weights -------------------------------------------------------------------------------------------------------
def run_prop_weights(ops, c, d):
    R, S = c.R, c.S
    e, dens, gw, gd = dev(d["e"]), dev(d["dens"]), dev(d["gw"]), dev(d["gd"])
    assert e.shape[1] == S + 1 + c.es_extra
    w, depth, w1 = nan(R, S), nan(R, 1), nan(R, S)
    ops.launch("nrhip_prop_weights_fwd", e, e.shape[1], dens, R, S, w, depth)
    ops.launch("nrhip_prop_weights_fwd", e, e.shape[1], dens, R, S, w1, None)
    got = {"weights": w, "depth": depth, "weights|no depth": w1}
    for k, a, b in (("both", gw, gd), ("gw only", gw, None), ("gdepth only", None, gd)):
        g = nan(R, S)
        ops.launch("nrhip_prop_weights_bwd", e, e.shape[1], dens, a, b, R, S, g)
        got[f"d dens {k}"] = g
    return got


@pytest.mark.parametrize("c,family", params(CR.PROP_CASES))
def test_prop_weights(ops, c, family):
    d = inputs(c, family)
    got = twice(run_prop_weights, ops, c, d)
    fn = CR.lattice_prop_weights if family == "lattice" else CR.ref_prop_weights
    ref = fn(c, d)
    ref["d dens both"] = ref.pop("d dens")
    ref["d dens gw only"] = fn(c, d, use_gd=False)["d dens"]
    ref["d dens gdepth only"] = fn(c, d, use_gw=False)["d dens"]
    compare(c, family, got, ref)
    w, depth = ops.prop_weights_fwd(dev(d["e"]), dev(d["dens"]))  # the wrappers take the wide rows as they are
    assert torch.equal(w, got["weights"]) and torch.equal(depth, got["depth"])
    g = ops.prop_weights_bwd(dev(d["e"]), dev(d["dens"]), dev(d["gw"]), dev(d["gd"]))
    assert torch.equal(g, got["d dens both"])


# ---- appearance / embedding_lerp ----------------------------------------------------------------------------------------
PAD = 9  # sentinel rows on either side of the table and of its gradient: an unclamped bad sensor lands at most n_per = 8 rows out


def guarded(rows, D, fill=None):
    """[rows, D] view in the middle of a buffer whose other rows hold the sentinel"""
    buf = torch.full((rows + 2 * PAD, D), float(CR.SENTINEL), device="cuda", dtype=torch.float32)
    if fill is not None:
        buf[PAD:PAD + rows] = fill
    return buf, buf[PAD:PAD + rows]


def guard_intact(buf, rows):
    return bool((buf[:PAD] == float(CR.SENTINEL)).all() and (buf[PAD + rows:] == float(CR.SENTINEL)).all())


@pytest.mark.parametrize("c", CR.EMBED_CASES, ids=lambda c: c.name)
def test_appearance_and_embedding(ops, c):
    d = CR.embed_inputs(c)
    fwd, gw_ref = CR.ref_embed(c, d)
    R, D, E = c.R, c.D, c.E
    _, table = guarded(E, D, dev(d["table"]))
    sensor = cuda(d["sensor"])
    times = None if d["times"] is None else dev(d["times"])
    # forward into a column block of a wider NaN row: a read beside the table would show as the sentinel
    obuf = nan(R, D + 3)
    out = ops.appearance_fwd(table, sensor, times, c.duration, c.n_per, c.temporal, R, out=obuf[:, 1:1 + D])
    CR.same(host(out), fwd, f"{c.name} forward")
    assert torch.isnan(obuf[:, 0]).all() and torch.isnan(obuf[:, 1 + D:]).all()
    CR.same(host(ops.appearance_fwd(table, sensor, times, c.duration, c.n_per, c.temporal, R)), fwd, f"{c.name} forward, own out")
    # backward from a column block of a wider row into a table between sentinel rows
    gbuf = nan(R, D + 1)
    gbuf[:, :D] = dev(d["g"])
    for _ in range(2):  # (exact sums: a second run gives the same bits in any atomic order)
        buf, gw = guarded(E, D)
        ops.launch("nrhip_appearance_bwd", gbuf, D + 1, sensor, times, float(c.duration), c.n_per, 1 if c.temporal else 0, R, E,
                   D, gw)
        CR.same(host(gw), gw_ref, f"{c.name} backward")
        assert guard_intact(buf, E), "the backward added beside the table"
    CR.same(host(ops.appearance_bwd(gbuf[:, :D], sensor, times, c.duration, c.n_per, c.temporal, E)), gw_ref,
            f"{c.name} backward through the wrapper")
    # embedding_lerp with the same slots, unclamped where the case has bad sensors: the kernels clamp
    lo, hi, frac = CR.embed_slots(c, d, clamp=not c.bad_sensors)
    lerp = c.temporal and c.times
    assert not c.bad_sensors or (lo.min() < 0 and lo.max() >= E)
    lo_t, hi_t, fr_t = cuda(lo), (cuda(hi) if lerp else None), (dev(frac) if lerp else None)
    CR.same(host(ops.embedding_lerp(table, lo_t, hi_t, fr_t)), fwd, f"{c.name} embedding_lerp")
    CR.same(host(ops.embedding_lerp_bwd(dev(d["g"]), lo_t, hi_t, fr_t, E)), gw_ref, f"{c.name} embedding_lerp_bwd")
