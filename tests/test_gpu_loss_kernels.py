"""The loss kernels per element, at every size branch and boundary: lidar_carving_kernel, interlevel_loss_kernel and
distortion_loss_kernel (csrc/losses.hip), mask_compact_kernel, lidar_rays_kernel, lidar_finish_kernel and
lidar_losses_bwd_kernel (csrc/train_fused.hip) against the references of tests/loss_refs.py (which
tests/test_loss_refs_host.py checks on the CPU).  Masks, error vectors, the quantile threshold, the kept set and its counts
are compared bit for bit; the bounds of everything else are stated where they are used."""
import numpy as np
import pytest
import torch

import loss_refs as LR
import neurad_oracle as O
from gpu_util import TIGHT, TOL
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ULP4 = 4 * 2.0 ** -24  # two or three fp32 roundings of an exact value


def _cuda(t):
    return None if t is None else t.cuda()


# ---- lidar_carving_kernel ----------------------------------------------------------------------------------------------
def _carve(ops, c, starts, ends, is_lidar, did_return, **kw):
    return ops.lidar_carving(starts, ends, _cuda(is_lidar), _cuda(did_return), c["distance"].cuda(), LR.EPS, LR.NON_RETURN,
                             **kw)


@pytest.mark.parametrize("shape", LR.CARVING_SHAPES, ids=lambda s: f"R{s[0]}_S{s[1]}")
def test_lidar_carving_per_element(ops, shape):
    R, S = shape
    c = LR.carving_case(R, S)
    assert c["share"][0] > 0 and (R == 1 or c["share"][1] > 0)  # samples exactly on |d - mid| == eps / mid == non_return
    e = c["edges"].cuda()
    # `starts[ray * stride + s]`: overlapping views of one wider tensor (row stride S + 4, as models/neurad.py passes them)
    starts, ends = e[:, :S], e[:, 1:S + 1]
    assert starts.stride(0) == S + 4 and starts.data_ptr() + 4 == ends.data_ptr()
    w = c["weights"].cuda()
    none, ones, zeros = None, torch.ones(R, dtype=torch.bool), torch.zeros(R, dtype=torch.bool)
    # `did_return ? ... : true`, `lidar &&`: did_return given / NULL, is_lidar mixed / all true / all false
    for did_return in (c["did_return"], none):
        for is_lidar in (c["is_lidar"], ones, zeros):
            rc, rl, rg = LR.carving_ref(c["edges"][:, :S], c["edges"][:, 1:S + 1], is_lidar, did_return, c["distance"],
                                        LR.EPS, LR.NON_RETURN, c["weights"])
            close, loss, gw = _carve(ops, c, starts, ends, is_lidar, did_return, weights=w)
            assert close.dtype == torch.bool and torch.equal(close.cpu(), rc)
            assert torch.equal(gw.cpu().double(), rg)  # 2 w far: doubling is exact
            # per ray: S products rounded once and summed in fp32 against fp64
            assert bool(((loss.cpu().double() - rl).abs() <= TIGHT * rl).all())
            assert bool((loss.cpu()[~is_lidar] == 0).all())
            # contiguous copies: the same bits
            c2, l2, g2 = _carve(ops, c, starts.contiguous(), ends.contiguous(), is_lidar, did_return, weights=w)
            assert torch.equal(c2, close) and torch.equal(l2, loss) and torch.equal(g2, gw)
            # `if (is_close)`, `if (weights)`, `if (grad_w)`: the mask-only call, the loss-only call, no gradient
            m_only = _carve(ops, c, starts, ends, is_lidar, did_return)
            assert torch.equal(m_only[0], close) and m_only[1] is None and m_only[2] is None
            l_only = _carve(ops, c, starts, ends, is_lidar, did_return, weights=w, want_mask=False)
            assert l_only[0] is None and torch.equal(l_only[1], loss) and torch.equal(l_only[2], gw)
            no_g = _carve(ops, c, starts, ends, is_lidar, did_return, weights=w, want_grad=False)
            assert torch.equal(no_g[0], close) and torch.equal(no_g[1], loss) and no_g[2] is None


def test_lidar_carving_no_rays_and_autograd(ops):
    from neurad_studio_amd.autograd import CarvingLossFn

    e = torch.zeros(0, 9, device="cuda")
    close, loss, gw = ops.lidar_carving(e[:, :8], e[:, 1:9], torch.zeros(0, dtype=torch.bool, device="cuda"), None,
                                        torch.zeros(0, device="cuda"), LR.EPS, LR.NON_RETURN,
                                        weights=torch.zeros(0, 8, device="cuda"))
    assert close.shape == (0, 8) and loss.shape == (0,) and gw.shape == (0, 8)
    # CarvingLossFn: the sum of the per-ray losses; the saved gradient times the upstream scalar
    R, S = 5, 129
    c = LR.carving_case(R, S)
    ed = c["edges"].cuda()
    args = (ed[:, :S], ed[:, 1:S + 1], c["is_lidar"].cuda(), c["did_return"].cuda(), c["distance"].cuda(), LR.EPS,
            LR.NON_RETURN)
    w = c["weights"].cuda().requires_grad_(True)
    _, loss, gw = ops.lidar_carving(*args, weights=w.detach())
    total = CarvingLossFn.apply(w, *args)
    assert torch.equal(total, loss.sum())
    (total * 0.375).backward()
    assert torch.equal(w.grad, gw * 0.375)


# ---- lidar_rays_kernel, lidar_finish_kernel, lidar_losses_bwd_kernel ---------------------------------------------------
def _run_lidar(ops, c, need_depth=None, need_intensity=True, need_logits=True):
    n, nl = c["n"], c["levels"]
    rows, inverse = ops.mask_compact(c["is_lidar"].cuda(), n)
    metrics, saved = ops.lidar_losses([d.cuda() for d in c["depths"]], rows, c["distance"].cuda(), c["did_return"].cuda(),
                                      c["intensity"].cuda(), c["target"].cuda(), c["logits"].cuda(), c["nr_dist"],
                                      c["nr_mult"], c["q"])
    gds, gi, gl = ops.lidar_losses_bwd(saved, inverse, c["up"].cuda(), nl, c["R"],
                                       [True] * nl if need_depth is None else need_depth, need_intensity, need_logits)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().reshape(-1)  # noqa: E731
    return {"rows": rows.cpu(), "metrics": metrics.cpu(), "scratch": saved[1].cpu(), "gdepth": [host(g) for g in gds],
            "gint": host(gi), "glogit": host(gl)}


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(LR.bits(a), LR.bits(b)))


def _close_per_element(got, ref, rel):
    """max over the elements of |got - ref| - rel |ref| <= 0, and exact zeros where the reference is zero"""
    got = got.double()
    assert got.shape == ref.shape
    bad = (got - ref).abs() > rel * ref.abs()
    assert not bool(bad.any()), (int(bad.sum()), got[bad][:4], ref[bad][:4])


def _check_lidar(c, out):
    n, nl = c["n"], c["levels"]
    ref = LR.lidar_ref(c)
    assert torch.equal(out["rows"], c["rows"])
    s = out["scratch"]
    assert np.array_equal(LR.bits(s[:n]), LR.bits(ref["err"]))            # the error vector, bit for bit
    assert LR.bits(s[n:n + 1])[0] == LR.bits(ref["thr"].reshape(1))[0], (float(s[n]), float(ref["thr"]))  # torch.quantile
    assert float(s[n + 1]) == ref["n_keep"] and float(s[n + 2]) == ref["n_sel"]
    for k in range(2 + nl):  # the project's 2e-5 relative against fp64, or both NaN (0 / 0), or the same infinity
        a, b = float(out["metrics"][k]), float(ref["metrics"][k])
        assert (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= 2e-5 * abs(b), (k, a, b)
    for l in range(nl):
        _close_per_element(out["gdepth"][l], ref["gdepth"][l], ULP4)
        assert bool((out["gdepth"][l][~c["is_lidar"]] == 0).all())  # camera rows
    assert bool((out["gdepth"][0][c["rows"]][~ref["keep"]] == 0).all())  # outside the kept set
    _close_per_element(out["gint"], ref["gint"], ULP4)
    assert bool((out["gint"][~(ref["keep"] & c["did_return"])] == 0).all())  # not kept, or no return
    # the logit gradient goes through 1 / (1 + __expf(-x)), whose error is relative to 1 and not to sigmoid(x) - y:
    # the project's 2e-5 of the bound |up| / n of an element
    scale = abs(float(c["up"][2])) / n
    assert float((out["glogit"].double() - ref["glogit"]).abs().max()) <= 2e-5 * scale
    return ref


CASES = LR.lidar_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_lidar_losses_per_element(ops, name):
    """every case group of loss_refs.lidar_cases (the kernel line each group is for is named there)"""
    c = CASES[name]
    out = _run_lidar(ops, c)
    ref = _check_lidar(c, out)
    if name.startswith("tie_all_equal") or name == "q_0.0":
        assert ref["n_keep"] == 0 and np.isnan(float(out["metrics"][0]))  # nothing is below the threshold
    if name == "none_returned":
        assert ref["n_sel"] == 0 and np.isnan(float(out["metrics"][1])) and bool((out["gint"] == 0).all())
    if name == "mixed_inf_hi":
        assert np.isinf(float(ref["thr"])) and ref["n_keep"] == c["n"] - 15
    if name == "size_40000":  # determinism: two runs give the same bits
        again = _run_lidar(ops, c)
        assert _same(again["metrics"], out["metrics"]) and _same(again["scratch"][:c["n"] + 3], out["scratch"][:c["n"] + 3])
        for a, b in zip(again["gdepth"] + [again["gint"], again["glogit"]], out["gdepth"] + [out["gint"], out["glogit"]]):
            assert _same(a, b)


@pytest.mark.parametrize("levels", [1, 2, 4])
def test_lidar_losses_bwd_absent_outputs(ops, levels):
    """lidar_losses_bwd_kernel: `if (!A.gdepth[l]) continue`, `if (A.gint)`, `if (A.glogit)` -- an output that is not asked
    for is None and the others keep their bits"""
    c = CASES[f"levels_{levels}"]
    full = _run_lidar(ops, c)
    for off in range(levels):
        need = [l != off for l in range(levels)]
        part = _run_lidar(ops, c, need_depth=need)
        assert part["gdepth"][off] is None
        assert all(_same(part["gdepth"][l], full["gdepth"][l]) for l in range(levels) if l != off)
        assert _same(part["gint"], full["gint"]) and _same(part["glogit"], full["glogit"])
    for ni, nlg in ((False, True), (True, False), (False, False)):
        part = _run_lidar(ops, c, need_intensity=ni, need_logits=nlg)
        assert (part["gint"] is None) == (not ni) and (part["glogit"] is None) == (not nlg)
        assert all(_same(part["gdepth"][l], full["gdepth"][l]) for l in range(levels))
        assert (not ni or _same(part["gint"], full["gint"])) and (not nlg or _same(part["glogit"], full["glogit"]))
    none = _run_lidar(ops, c, need_depth=[False] * levels)
    assert all(g is None for g in none["gdepth"]) and _same(none["gint"], full["gint"])


# ---- mask_compact_kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", LR.MASK_RS)
def test_mask_compact_unaligned_and_pass_boundaries(ops, R):
    """`aligned` false (byte loads) at 1, 3 and 7 bytes off an 8-byte boundary and true at 0; `start += 8192` pass
    boundaries; `i0 + 8 <= R` tails"""
    big = torch.zeros(R + 16, dtype=torch.bool, device="cuda")
    assert big.data_ptr() % 8 == 0
    for name, m in LR.mask_cases(R).items():
        rows_ref, inv_ref = LR.compact_ref(m)
        for off in (0,) + LR.MASK_OFFSETS:
            big.fill_(True)  # whatever surrounds the slice is set: a read outside [off, off + R) would count
            view = big[off:off + R]
            view.copy_(m.cuda())
            assert R == 0 or (view.data_ptr() % 8 == off and view.is_contiguous())
            rows, inv = ops.mask_compact(view, rows_ref.numel())
            assert torch.equal(rows.cpu(), rows_ref) and torch.equal(inv.cpu(), inv_ref), (R, name, off)


@pytest.mark.parametrize("R", [9, 8193, 16389])
def test_mask_compact_other_dtypes_and_wrong_counts(ops, R):
    m = LR.mask_cases(R)["half"]
    rows_ref, inv_ref = LR.compact_ref(m)
    n = rows_ref.numel()
    # any non-zero byte is set (`& 0xff ? 1 : 0` / `mask[i0 + k]`), aligned and not; a float mask
    u8 = torch.where(m, torch.where(torch.arange(R) % 2 == 0, 2, 255), 0).to(torch.uint8)
    big = torch.zeros(R + 8, dtype=torch.uint8, device="cuda")
    for off in (0, 3):
        big[off:off + R] = u8.cuda()
        rows, inv = ops.mask_compact(big[off:off + R], n)
        assert torch.equal(rows.cpu(), rows_ref) and torch.equal(inv.cpu(), inv_ref)
    rows, inv = ops.mask_compact(torch.where(m, -0.5, 0.0).cuda(), n)
    assert torch.equal(rows.cpu(), rows_ref) and torch.equal(inv.cpu(), inv_ref)
    # `(int64_t)pos < n_out`: n_out too large -- rows past the count are 0; too small -- the first n_out rows, and the
    # inverse still holds every position
    rows, inv = ops.mask_compact(m.cuda(), n + 5)
    assert torch.equal(rows.cpu()[:n], rows_ref) and bool((rows.cpu()[n:] == 0).all()) and torch.equal(inv.cpu(), inv_ref)
    for short in (0, n // 2, n - 1):
        rows, inv = ops.mask_compact(m.cuda(), short)
        assert rows.shape == (short,) and torch.equal(rows.cpu(), rows_ref[:short]) and torch.equal(inv.cpu(), inv_ref)


# ---- interlevel_loss_kernel, distortion_loss_kernel --------------------------------------------------------------------
def _per_ray(got, ref, tol):
    """|got - ref| relative to the ray's own scale (|loss| of the ray, max |gradient| over the ray): -> worst ratio / tol"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref) if ref.ndim == 1 else np.abs(ref).max(-1, keepdims=True)
    return np.abs(got - ref) / np.maximum(scale, 1e-300) / tol


# A ray that does not hold TOL against the fp32 oracle is judged against the fp64 evaluation of the same formula: the
# kernel's distance to it must stay within four times the oracle's own (the two differ in summation order only).  No ray
# of these cases needs that on an MI355X: the worst loss is 7.2e-7 and the worst gradient element 1.5e-6 of the ray's scale.
@pytest.mark.parametrize("zero_wp", [False, True], ids=["wp>0", "wp0=0"])
@pytest.mark.parametrize("shape", LR.SAMPLER_SHAPES, ids=lambda s: "R%d_sf%d_sp%d" % s)
def test_interlevel_loss_per_ray(ops, shape, zero_wp):
    """scan_inplace's 64-lane chunks (2 sf + 1 knots), the tail workgroup (R % 4), searchsorted's left rule on proposal
    edges that equal a knot, zero-width proposal bins, a 2^-12 fine bin.  Loss per ray and gradient per element against the
    fp32 oracle at TOL (as test_sampler_losses_vs_reference_autograd assigns it), relative to the ray's own scale."""
    R, sf, sp = shape
    c, w, cp, wp = LR.sampler_case(R, sf, sp, zero_wp=zero_wp)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    loss, grad = ops.interlevel_loss_level(dev(c), dev(w), dev(cp), dev(wp), LR.PULSE)
    rl, _, rg = O.interlevel_loss_level(c, w, cp, wp, LR.PULSE)
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    el, eg = _per_ray(loss, rl, TOL), _per_ray(grad, rg, TOL).max(-1)
    print(f"interlevel {shape} zero_wp={zero_wp}: worst loss {el.max() * TOL:.2e} worst grad {eg.max() * TOL:.2e}")
    over = np.nonzero((el > 1) | (eg > 1))[0]
    if over.size:
        l64, g64 = LR.interlevel_ref64(c[over], w[over], cp[over], wp[over], LR.PULSE)
        for k, r in enumerate(over):
            dk = (abs(loss[r] - l64[k]), np.abs(grad[r] - g64[k]).max())
            do = (abs(rl[r] - l64[k]), np.abs(rg[r] - g64[k]).max())
            print(f"  ray {r}: kernel to fp64 {dk[0]:.3e} / {dk[1]:.3e}, oracle to fp64 {do[0]:.3e} / {do[1]:.3e}")
            assert dk[0] <= 4 * do[0] and dk[1] <= 4 * do[1], (shape, r, dk, do)
    # `if (gwp)`: without the gradient the loss keeps its bits
    l2, g2 = ops.interlevel_loss_level(dev(c), dev(w), dev(cp), dev(wp), LR.PULSE, need_grad=False)
    assert g2 is None and np.array_equal(LR.bits(l2), LR.bits(loss))


@pytest.mark.parametrize("shape", LR.SAMPLER_SHAPES, ids=lambda s: "R%d_sf%d_sp%d" % s)
def test_distortion_loss_per_ray(ops, shape):
    """on the proposal samples (up to kMaxProp = 512) and on the fine ones: loss per ray and gradient per element against
    the fp32 oracle at TIGHT, relative to the ray's own scale"""
    R, sf, sp = shape
    c, w, cp, wp = LR.sampler_case(R, sf, sp)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    for e, x in ((cp, wp), (c, w)):
        loss, grad = ops.distortion_loss_rays(dev(e), dev(x))
        rl, rg = O.distortion_loss_rays(e, x)
        el, eg = _per_ray(loss.cpu().numpy(), rl, TIGHT), _per_ray(grad.cpu().numpy(), rg, TIGHT)
        print(f"distortion {shape} s={x.shape[1]}: worst loss {el.max() * TIGHT:.2e} worst grad {eg.max() * TIGHT:.2e}")
        assert el.max() <= 1 and eg.max() <= 1, (shape, x.shape, el.max() * TIGHT, eg.max() * TIGHT)
        l2, g2 = ops.distortion_loss_rays(dev(e), dev(x), need_grad=False)
        assert g2 is None and torch.equal(l2, loss)


def test_interlevel_loss_keeps_the_nan_of_a_fine_bin_without_width(ops):
    """a fine bin of no width next to a zero-width proposal bin: w / 0 = inf, inf - inf in the blurred histogram; torch's
    clamp_min keeps the NaN and the reference's loss of that ray is NaN (the oracle agrees).  The other rays of the
    workgroup are untouched."""
    c, w, cp, wp = LR.degenerate_sampler_case()
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    loss, grad = ops.interlevel_loss_level(dev(c), dev(w), dev(cp), dev(wp), LR.PULSE)
    with np.errstate(all="ignore"):
        rl, _, rg = O.interlevel_loss_level(c, w, cp, wp, LR.PULSE)
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    assert np.isnan(rl[0]) and np.isnan(loss[0])
    assert np.array_equal(np.isnan(grad), np.isnan(rg))
    assert _per_ray(loss[1:], rl[1:], TOL).max() <= 1 and _per_ray(grad[1:], rg[1:], TOL).max() <= 1


def test_sampler_losses_reject_too_many_samples(ops):
    """kMaxFine = 128, kMaxProp = 512: the library's error, and nothing is launched (the outputs keep their contents)"""
    from neurad_studio_amd._lib import NeuradHipError

    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    with pytest.raises(NeuradHipError, match="exceed"):
        ops.interlevel_loss_level(z(2, 130), z(2, 129), z(2, 65), z(2, 64), LR.PULSE)
    with pytest.raises(NeuradHipError, match="exceed"):
        ops.interlevel_loss_level(z(2, 33), z(2, 32), z(2, 514), z(2, 513), LR.PULSE)
    with pytest.raises(NeuradHipError, match="exceed"):
        ops.distortion_loss_rays(z(2, 514), z(2, 513))
    loss = torch.full((2,), -7.0, device="cuda")
    with pytest.raises(NeuradHipError, match="exceed"):
        ops.launch("nrhip_interlevel_loss", z(2, 130), z(2, 129), 129, z(2, 65), z(2, 64), 64, LR.PULSE, 2, loss, None)
    with pytest.raises(NeuradHipError, match="exceed"):
        ops.launch("nrhip_distortion_loss", z(2, 514), z(2, 513), 513, 2, loss, None)
    torch.cuda.synchronize()
    assert bool((loss == -7.0).all())
