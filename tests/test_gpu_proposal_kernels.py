"""The stand-alone proposal-density kernels, sample by sample and entry by entry, in every launch branch (csrc/hashgrid.hip,
ProposalSrc in csrc/encode_bwd_binned.hip).  Cases, float64 references and the derivation of every tolerance:
tests/proposal_refs.py; that the cases are what they claim and tell wrong kernels apart: tests/test_proposal_refs_host.py.

Forward: `level_features` of the exact family bit for bit, densities of the fused / VEC = 4 / VEC = 1 paths bit-identical and
within 2 ulp + the logit's roundings of float64, NaN-prefilled outputs (an unwritten sample shows) inside guarded buffers.
Backward: per-element bounds from the roundings; the grid-stride loop's second pass and the fp16-table runs exactly.

NaN: a NaN density (one NaN table entry) with a finite non-zero g poisons the decoder gradient at every level and exactly the
table entries its samples touch, as torch's clamp does (trunc_exp_bwd_factor in common.h; before it the kernels returned
g e^-15 there).  A sample with g == 0 sends no records by design (ProposalGrad::silent) and the atomic kernel would send
0 * NaN: such samples are left out of the NaN set.

The C entry point takes the level-partitioned route whenever it is given a `level_features` buffer, so the fused kernel's own
write of that buffer cannot be reached through it; the fused kernel is held to the densities.

Measured on an MI355X (printed by the tests, largest over their cases):
  rescaled features  err / |ref| <= 4.78e-7 where rtol_rw allows up to 1.94e-6: err / rtol_rw <= 0.46
  density            err / bound <= 0.30
  decoder gradient   err / bound <= 0.03
  table, atomic      err / bound <= 0.16
  table, binned      err / bound <= 0.20"""
import numpy as np
import pytest
import torch

import proposal_refs as P
from gpu_util import dev, host, host64
from gpu_util import ops  # noqa: F401  (fixture)
from table_grad_refs import bound_for

pytestmark = pytest.mark.gpu

GUARD = 12345.0  # around every output the kernels write: the bytes beyond n stay as they were
MODES = ("atomic", "binned_lf", "binned")


def spec_of(ops, c, half=False):
    L, F, lg, mn, mx = c.grid
    return ops.ProposalSpec(ops.GridSpec(L, F, lg, mn, mx), dev(c.table, torch.float16 if half else torch.float32),
                            P.STATIC_SCALE, dev(c.dec))


def rays_of(c, edge_views=False):
    """(origins, directions, pixel_area, starts, ends); edge_views: starts / ends as views into ONE [R, S + 1] tensor"""
    e = dev(c.edges)
    s, t = (e[:, :-1], e[:, 1:]) if edge_views else (e[:, :-1].contiguous(), e[:, 1:].contiguous())
    return dev(c.o), dev(c.d), dev(c.area), s, t


def guarded(count, offset=0):
    """a NaN-filled window of `count` floats, `offset` floats into a 16-byte aligned buffer with guard values around it"""
    buf = torch.full((offset + count + 8,), GUARD, device="cuda")
    win = buf[offset:offset + count]
    win.fill_(float("nan"))
    return buf, win


def guards_intact(buf, win, offset):
    return bool((buf[:offset] == GUARD).all() and (buf[offset + win.numel():] == GUARD).all())


def forward(ops, ps, rays, n, L, features, off_dens=0, off_lf=0):
    """nrhip_proposal_density_fwd through the launch helper ops uses, on this test's own buffers"""
    r, keep = ops._c_rays(*rays)
    p, keep2 = ps.c_prop()
    dbuf, dens = guarded(n, off_dens)
    lbuf, lf = guarded(L * n, off_lf) if features else (None, None)
    ops.launch("nrhip_proposal_density_fwd", p, r, dens, lf)
    torch.cuda.synchronize()
    assert guards_intact(dbuf, dens, off_dens) and (lf is None or guards_intact(lbuf, lf, off_lf))
    return dens, (None if lf is None else lf.view(L, n))


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


# ---- forward ------------------------------------------------------------------------------------------------------------------
# n -> what the size reaches.  Fused kernel: one thread per sample, 256 per block: 255 / 256 / 257 are one block short, one
# full, one sample in a second block.  Level-partitioned kernel: per_quarter = ceil(ceil(n / 4) / 256) * 256 -- 1, 3: quarter 0
# alone has samples; 1023: the last quarter one short; 1024: four exactly full quarters; 1025: per_quarter 512, quarter 2 holds
# ONE sample and quarter 3 none; 2049: per_quarter 768 = three blocks per unit.  L = 1, 2, 3, 6, 8 are 4, 8, 12, 24, 32 (level,
# quarter) units over 8 slots: half a round, one, one and a half, three, four.  from_levels: VEC = 4 where n % 4 == 0 and
# both buffers are 16-byte aligned (256, 1024), VEC = 1 otherwise -- and at 256 / 1024 once `density` or `level_features`
# starts one float into its buffer.
FWD_SIZES = (1, 3, 255, 256, 257, 1023, 1024, 1025, 2049)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("L", sorted(P.GRIDS))
@pytest.mark.parametrize("n", FWD_SIZES)
def test_forward_every_sample_every_branch(ops, n, L, half):
    c = P.exact_case(n, L, seed=10)
    ref = P.forward_ref(c)
    ps, rays = spec_of(ops, c, half), rays_of(c)
    fused, _ = forward(ops, ps, rays, n, L, features=False)
    runs = [forward(ops, ps, rays, n, L, True),  # VEC = 4 iff n % 4 == 0
            forward(ops, ps, rays, n, L, True, off_dens=1),  # VEC = 1: density misaligned
            forward(ops, ps, rays, n, L, True, off_lf=1)]  # VEC = 1: level features misaligned
    want_lf = dev(ref.lf.T)  # [L, N]; exact in fp32 (test_exact_family_is_exact)
    for dens, lf in runs:
        assert same_bits(lf, want_lf), f"level features differ at (level, sample) {torch.nonzero(lf != want_lf)[:4].tolist()}"
        assert same_bits(dens, fused)
    err = np.abs(host64(fused) - np.exp(ref.x))
    bound = P.density_bound(c, ref)
    print(f"\n[fwd n={n} L={L} {'fp16' if half else 'fp32'}] density err / bound <= {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_forward_on_edge_views(ops):
    """starts / ends as views into one [R, S + 1] edge tensor (row stride S + 1): the same bits as from two [R, S] tensors"""
    n, L = 1025, 6
    c = P.exact_case(n, L, seed=11)
    ps = spec_of(ops, c)
    rays = rays_of(c, edge_views=True)
    assert rays[3].stride(0) == c.S + 1 and rays[3].data_ptr() + 4 == rays[4].data_ptr()
    want_lf = dev(P.forward_ref(c).lf.T)
    fused, _ = forward(ops, ps, rays, n, L, False)
    dens, lf = forward(ops, ps, rays, n, L, True)
    assert same_bits(lf, want_lf) and same_bits(dens, fused)
    assert same_bits(fused, forward(ops, ps, rays_of(c), n, L, False)[0])


@pytest.mark.parametrize("n", [1025, 2049])
def test_forward_rescaled_features_within_rtol_rw(ops, n):
    """pixel_area > 0: interp is still exact, the rescale weight goes through fast_cbrt and v_rcp_f32"""
    L = 6
    c = P.rescaled_case(n, L, seed=12)
    ref = P.forward_ref(c)
    rt = P.rtol_rw(c, ref)
    ps, rays = spec_of(ops, c), rays_of(c)
    dens, lf = forward(ops, ps, rays, n, L, True)
    fused, _ = forward(ops, ps, rays, n, L, False)
    assert same_bits(dens, fused)
    err = np.abs(host64(lf).T - ref.lf)
    nz = ref.lf != 0
    rel = (err[nz] / np.abs(ref.lf[nz])).max()
    ratio = (err[nz] / (rt * np.abs(ref.lf))[nz]).max()
    print(f"\n[rescaled n={n}] features err / |ref| <= {rel:.3e}; against rtol_rw (<= {rt.max():.3e}): ratio {ratio:.3f}")
    assert (err <= rt * np.abs(ref.lf)).all()
    assert (host64(lf).T[~nz] == 0).all()


# ---- backward -----------------------------------------------------------------------------------------------------------------
def backward(ops, mp, ps, rays, dens, g, mode, lf=None):
    mp.setattr(ops, "_FORCE_ATOMIC_SCATTER", mode == "atomic")
    mp.setattr(ops, "_BINNED_MIN_SAMPLES", 1)
    gt, gdec = ops.proposal_density_bwd(ps, *rays, dens, g, level_features=lf if mode == "binned_lf" else None)
    torch.cuda.synchronize()
    return gt, gdec


def check_backward(c, ref, gt, gdec, mode, what, poisoned=None):
    """decoder gradient and every table entry within its bound; entries no sample touches, and entries only silent samples
    (g == 0) touch, exactly 0; poisoned: the entries that must be NaN (and the decoder gradient with them)"""
    got_t, got_d = host64(gt).reshape(-1), host64(gdec).reshape(-1)
    bound = ref.atomic_bound() if mode == "atomic" else \
        bound_for(ref.table, ref.a, ref.nt, ref.recs, ref.tmax, ref.amax, ref.ts, c.L, 1, P.LOG2_T, True)[0] + ref.soft
    if poisoned is None:
        poisoned = np.zeros(got_t.shape, bool)
        err_d = np.abs(got_d - ref.ddec)
        assert (err_d <= ref.ddec_bound).all(), (what, got_d, ref.ddec, ref.ddec_bound)
        rd = (err_d / np.maximum(ref.ddec_bound, 1e-300)).max()
    else:
        assert np.isnan(got_d).all(), (what, got_d)
        rd = float("nan")
    assert np.array_equal(np.isnan(got_t), poisoned), \
        (what, np.flatnonzero(np.isnan(got_t) & ~poisoned)[:5], np.flatnonzero(poisoned & ~np.isnan(got_t))[:5])
    ok = ~poisoned
    err = np.abs(got_t - ref.table)[ok]
    over = ~(err <= bound[ok])
    assert not over.any(), (what, int(over.sum()), got_t[ok][over][:3], ref.table[ok][over][:3], bound[ok][over][:3])
    assert (got_t[ref.nt == 0] == 0).all(), what  # untouched, or touched by silent samples alone
    live = ok & (ref.nt > 0)
    rt = (np.abs(got_t - ref.table)[live] / bound[live]).max() if live.any() else 0.0
    print(f"\n[{what} {mode}] decoder err / bound <= {rd:.3f}, table err / bound <= {rt:.3f}")


def exact_inputs(ops, c):
    """(spec, rays, the fused forward's densities [R, S], the level features [L, N])"""
    ps, rays = spec_of(ops, c), rays_of(c)
    dens, lf = ops.proposal_density_fwd(ps, *rays, save_features=True)
    return ps, rays, dens, lf


# proposal_density_bwd_kernel<true>: one thread per sample, block-reduced decoder gradient -- the dead lanes of the last block
# (n = 1: 255 of them; 255: one; 257 and 1025: a second / fifth block of ONE live lane) take part in the reduction.
@pytest.mark.parametrize("L", [1, 6, 8])
@pytest.mark.parametrize("n", [1, 255, 257, 1025])
def test_backward_atomic(ops, monkeypatch, n, L):
    c = P.exact_case(n, L, seed=20)
    fwd = P.forward_ref(c)
    g = P.grad_with_silent_windows(n, seed=20)
    ps, rays, dens, _ = exact_inputs(ops, c)
    gt, gdec = backward(ops, monkeypatch, ps, rays, dens, dev(g).view(c.R, c.S), "atomic")
    check_backward(c, P.backward_ref(c, fwd, g), gt, gdec, "atomic", f"n={n} L={L}")


def shifted(t):
    """the same values one float into a larger buffer: contiguous, 4-byte aligned only"""
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


# proposal_decoder_grad_kernel: <4> needs n % 4 == 0 and level_features, density and grad_density all 16-byte aligned
# (1024, nothing shifted); <1> otherwise -- 1023, and 1024 with any one of the three one float off.  With g == 0 over whole
# and partial 64-sample windows (ProposalGrad::silent): check_backward holds the entries only they touch to exactly 0.
@pytest.mark.parametrize("n,shift", [(1024, None), (1023, None), (1024, "lf"), (1024, "density"), (1024, "grad")])
def test_backward_binned_with_features(ops, monkeypatch, n, shift):
    L = 6
    c = P.exact_case(n, L, seed=21)
    fwd = P.forward_ref(c)
    g = P.grad_with_silent_windows(n, seed=21)
    ps, rays, dens, lf = exact_inputs(ops, c)
    gd = dev(g).view(c.R, c.S)
    args = {"lf": lf, "density": dens, "grad": gd}
    if shift:
        args[shift] = shifted(args[shift])
        assert args[shift].data_ptr() % 16 == 4
    gt, gdec = backward(ops, monkeypatch, ps, rays, args["density"], args["grad"], "binned_lf", args["lf"])
    check_backward(c, P.backward_ref(c, fwd, g), gt, gdec, "binned_lf", f"n={n} shift={shift}")
    if shift:  # the table gradient never reads the level features and walks samples one by one: same bits either way
        gt0, _ = backward(ops, monkeypatch, ps, rays, dens, gd, "binned_lf", lf)
        assert same_bits(gt, gt0)


# proposal_density_bwd_kernel<false>: the binned entry without saved level features recomputes them for the decoder gradient;
# the table gradient is the same partition over the same inputs as with them -- the same bits.
@pytest.mark.parametrize("n", [257, 1025])
def test_backward_binned_without_features(ops, monkeypatch, n):
    L = 6
    c = P.exact_case(n, L, seed=22)
    fwd = P.forward_ref(c)
    g = P.grad_with_silent_windows(n, seed=22)
    ps, rays, dens, lf = exact_inputs(ops, c)
    gd = dev(g).view(c.R, c.S)
    gt, gdec = backward(ops, monkeypatch, ps, rays, dens, gd, "binned")
    check_backward(c, P.backward_ref(c, fwd, g), gt, gdec, "binned", f"n={n}")
    gt_lf, _ = backward(ops, monkeypatch, ps, rays, dens, gd, "binned_lf", lf)
    assert same_bits(gt, gt_lf)


# The decoder-gradient kernel caps its grid at 1024 blocks of 256 threads and strides: a second loop iteration needs more than
# 1024 * 256 = 262 144 samples in the scalar form (n odd: 2049 x 129 = 264 321) and more than 4 * 262 144 = 1 048 576 in the
# vector form (n % 4 == 0: 4105 x 256 = 1 050 880, L = 2 to keep the buffers small).  Decoder weight 0: density 1, gx = g.
@pytest.mark.parametrize("R,S,L,vec", [(2049, 129, 6, 1), (4105, 256, 2, 4)], ids=["scalar", "vector"])
def test_decoder_gradient_second_pass_is_exact(ops, monkeypatch, R, S, L, vec):
    n = R * S
    lf, g, chosen, ddec = P.stride_case(n, L, vec)
    mn, mx = P.GRIDS[L]
    table = torch.ones((L << P.LOG2_T, 1), device="cuda")
    ps = ops.ProposalSpec(ops.GridSpec(L, 1, P.LOG2_T, mn, mx), table, P.STATIC_SCALE, torch.zeros((1, L), device="cuda"))
    edges = (torch.arange(S + 1, device="cuda", dtype=torch.float32) / 32.0).repeat(R, 1)
    o = dev(np.random.default_rng(5).integers(-64, 65, (R, 3)) / 16.0)
    d = dev(np.random.default_rng(6).choice([-1.0, 0.0, 1.0], (R, 3)))
    rays = (o, d, torch.zeros(R, device="cuda"), edges[:, :-1], edges[:, 1:])
    dens = torch.ones((R, S), device="cuda")
    assert n % 4 == (0 if vec == 4 else 1) and dens.data_ptr() % 16 == 0
    gt, gdec = backward(ops, monkeypatch, ps, rays, dens, dev(g).view(R, S), "binned_lf", dev(lf))
    assert np.array_equal(host64(gdec).reshape(-1), ddec), (host(gdec), ddec)
    assert not gt.any()  # every record is g * 0: the table gradient is all zeros


def test_backward_rescaled(ops, monkeypatch):
    """pixel_area > 0: the rescale weight is in the table term (a kernel without it is off by up to 1 / rw, see the host
    test) and in the level features of the decoder gradient"""
    n, L = 1025, 6
    c = P.rescaled_case(n, L, seed=23)
    fwd = P.forward_ref(c)
    g = P.grad_with_silent_windows(n, seed=23)
    ref = P.backward_ref(c, fwd, g, rw_rtol=P.rtol_rw(c, fwd))
    ps, rays, dens, lf = exact_inputs(ops, c)
    for mode in MODES:
        gt, gdec = backward(ops, monkeypatch, ps, rays, dens, dev(g).view(c.R, c.S), mode, lf)
        check_backward(c, ref, gt, gdec, mode, "rescaled")


def test_backward_fp16_table(ops, monkeypatch):
    """an fp16-storage table of the same integer values: the binned entry with level features never reads the table -- the
    fp32 run's bits; without them it is refused; ops' atomic path (it widens the table) equals the fp32 run"""
    n, L = 1025, 6
    c = P.exact_case(n, L, seed=24)
    g = dev(P.grad_with_silent_windows(n, seed=24)).view(c.R, c.S)
    ps, rays, dens, lf = exact_inputs(ops, c)
    ph = spec_of(ops, c, half=True)
    dens_h, lf_h = ops.proposal_density_fwd(ph, *rays, save_features=True)
    assert same_bits(dens_h, dens) and same_bits(lf_h, lf)
    gt, gdec = backward(ops, monkeypatch, ps, rays, dens, g, "binned_lf", lf)
    gt_h, gdec_h = backward(ops, monkeypatch, ph, rays, dens, g, "binned_lf", lf)
    assert gt_h.dtype == torch.float32 and same_bits(gt_h, gt)
    check_backward(c, P.backward_ref(c, P.forward_ref(c), host(g).reshape(-1)), gt_h, gdec_h, "binned_lf", "fp16 table")
    with pytest.raises(ops._lib.NeuradHipError, match="fp32 table unless the forward's level features"):
        backward(ops, monkeypatch, ph, rays, dens, g, "binned")
    # atomic path: memory-side fp32 atomics land in no fixed order, so "equal" is as far as that order allows -- each entry
    # where at most two terms meet (a + b is commutative) bit for bit, every entry within the bound
    ref = P.backward_ref(c, P.forward_ref(c), host(g).reshape(-1))
    gt_a, gdec_a = backward(ops, monkeypatch, ps, rays, dens, g, "atomic")
    gt_ah, gdec_ah = backward(ops, monkeypatch, ph, rays, dens, g, "atomic")
    check_backward(c, ref, gt_ah, gdec_ah, "atomic", "fp16 table")
    few = torch.from_numpy(ref.nt <= 2).cuda()
    assert few.sum() > 1000 and same_bits(gt_ah.reshape(-1)[few], gt_a.reshape(-1)[few])


@pytest.mark.parametrize("mode", MODES)
def test_backward_clamp_and_saturation(ops, monkeypatch, mode):
    """a hot decoder row (+-16): logits inside (-15, 15), on both sides of +-15, exactly 0 and +-16, and beyond +-88 -- the
    densities the backward reads hold inf, subnormals and 0.  References clip at +-15; g == 0 at half the inf densities
    gives 0, never inf * 0"""
    c = P.saturation_case(2049, 6, seed=2)
    fwd = P.forward_ref(c)
    g = P.saturation_grad(fwd, seed=2)
    ps, rays, dens, lf = exact_inputs(ops, c)
    d = host(dens).reshape(-1)
    assert np.isinf(d).sum() >= 4 and (d < np.finfo(np.float32).tiny).sum() >= 2 and np.array_equal(np.isinf(d), fwd.x > 88.73)
    gt, gdec = backward(ops, monkeypatch, ps, rays, dens, dev(g).view(c.R, c.S), mode, lf)
    assert torch.isfinite(gt).all() and torch.isfinite(gdec).all()
    check_backward(c, P.backward_ref(c, fwd, g), gt, gdec, mode, "saturation")


@pytest.mark.parametrize("mode", MODES)
def test_backward_nan_density_poisons_like_torch(ops, monkeypatch, mode):
    n, L = 1025, 6
    c, bad = P.nan_case(n, L, seed=3)
    fwd = P.forward_ref(c)
    g = P.grad_with_silent_windows(n, seed=3)
    g[bad] = 0.5  # finite and non-zero at every NaN density (a g of 0 is silent by design, see the module docstring)
    ps, rays, dens, lf = exact_inputs(ops, c)
    assert np.array_equal(np.flatnonzero(np.isnan(host(dens).reshape(-1))), bad)
    gt, gdec = backward(ops, monkeypatch, ps, rays, dens, dev(g).view(c.R, c.S), mode, lf)
    poisoned = np.zeros(L << P.LOG2_T, bool)
    poisoned[fwd.idx[bad].reshape(-1)] = True  # all 8 corners at every level (every decoder weight is non-zero)
    check_backward(c, P.backward_ref(c, fwd, g), gt, gdec, mode, "nan", poisoned)


# ---- the autograd node --------------------------------------------------------------------------------------------------------
def test_autograd_node_against_ops(ops, monkeypatch):
    from neurad_studio_amd import autograd as A

    monkeypatch.setattr(ops, "_FORCE_ATOMIC_SCATTER", False)
    monkeypatch.setattr(ops, "_BINNED_MIN_SAMPLES", 1)  # the partition: the same bits run to run
    n, L = 257, 6
    c = P.exact_case(n, L, seed=30)
    ps, rays, dens, lf = exact_inputs(ops, c)
    o, d, area, s, e = rays
    g = dev(P.grad_with_silent_windows(n, seed=30)).view(c.R, c.S)
    gt, gdec = ops.proposal_density_bwd(ps, *rays, dens, g, level_features=lf)

    def node(table, dec, o_, d_):
        return A.ProposalDensityFn.apply(table, dec, ps.grid, ps.static_scale, o_, d_, area, s, e)

    # nothing requires grad: the fused forward, nothing saved
    out = node(ps.table, ps.decoder_weight, o, d)
    assert out.grad_fn is None and same_bits(out, ops.proposal_density_fwd(ps, *rays)) and same_bits(out, dens)
    # table and decoder: the level-feature path
    table, dec = ps.table.clone().requires_grad_(), ps.decoder_weight.clone().requires_grad_()
    out = node(table, dec, o, d)
    assert same_bits(out, dens)
    out.backward(g)
    assert same_bits(table.grad, gt) and dec.grad.shape == (1, L) and same_bits(dec.grad, gdec)
    # table frozen, rays moving: ray gradients only
    o2, d2 = o.clone().requires_grad_(), d.clone().requires_grad_()
    out = node(ps.table, ps.decoder_weight, o2, d2)
    got = torch.autograd.grad(out, (o2, d2), g)
    want = A.DenseSamples(s, e).ray_grads(ps.grid, ps.table, ps.static_scale, o, d, area,
                                          A._proposal_genc(dens, g, ps.decoder_weight))
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[0].abs().sum() > 0
    table = ps.table.clone().requires_grad_(False)
    out = node(table, ps.decoder_weight, o2, d2)
    out.backward(g)
    assert table.grad is None and ps.decoder_weight.grad is None
    # an fp16-storage table: the gradient comes back in the table's dtype
    th = ps.table.half().requires_grad_()
    out = node(th, ps.decoder_weight, o, d)
    assert same_bits(out, dens)
    out.backward(g)
    assert th.grad.dtype == torch.float16 and torch.equal(th.grad, gt.half())
