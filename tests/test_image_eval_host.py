"""Camera image evaluation, the part that needs no GPU: the restatements of tests/image_eval_refs.py against each other (the
padded-and-cropped form torchmetrics uses and the valid-window form the kernel computes; the variance clamp), the fp32
emulation of the kernel's accumulation order inside the per-window bound B, B against five deliberately wrong restatements
(it is not vacuous), the distance of torchmetrics' fp32 arithmetic from float64 (printed for DESIGN.md, not asserted), the
host-side argument checks of nrhip_image_metrics / nrhip_image_psnr, the workspace query as host logic, the refusal of CPU
tensors, the float64 fallback of model_components/image_metrics.py and the plugin's opt-in flag."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

import image_eval_refs as R
from host_gate import ROOT

I32, I64, F32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
ONE = ctypes.c_void_p(0x1000)  # any non-null, 16-byte aligned address: validation fails before anything is dereferenced
INVALID_ARG, UNSUPPORTED = 1, 2
T = R.TILE
SIZES = R.sizes()
case = R.case


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(ge.LIB):
        ge.build()
    lib = ctypes.CDLL(ge.LIB)
    lib.nrhip_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("kind", R.KINDS)
def test_padded_and_cropped_equals_the_valid_windows_in_float64(kind):
    """torchmetrics' reflect pad and crop leave exactly the windows that lie inside the image: in float64 arithmetic that
    does not cancel (two passes per window) the two layouts agree to 1e-14 per window.  torchmetrics' own arithmetic, one
    conv2d and E[x^2] - mu^2 on the raw values, loses up to 4e-13 to float64's rounding on smooth content, and differently for
    every image size (another summation order inside conv2d): its float64 value is held to that first-order size against
    the two-pass reference, and the figure is printed."""
    worst = 0.0
    for h, w in SIZES:
        a, b, want, _ = case(kind, h, w)
        value, got = R.ssim_padded(a, b, torch.float64, return_map=True)
        laid_out = R.ssim_valid_padded(a, b)
        assert got.shape == laid_out.shape == want.shape == (h - 10, w - 10, 3)
        assert np.abs(laid_out - want).max() <= 1e-14, (kind, h, w, np.abs(laid_out - want).max())
        assert abs(laid_out.mean() - want.mean()) <= 1e-14
        inside = R.ssim_padded(a, b, torch.float64, return_map=True, pad=False)[1]
        assert np.abs(inside - want).max() <= R.conv_form_float64_error(a, b)
        # in exact arithmetic the variances are >= 0: in float64 the clamp of newer torchmetrics versions changes nothing
        clamped = R.ssim_padded(a, b, torch.float64, clamp=True, return_map=True)[1]
        assert np.array_equal(clamped, got), (kind, h, w, np.abs(clamped - got).max())
        gap = float(np.abs(got - want).max())
        assert gap <= R.conv_form_float64_error(a, b), (kind, h, w, gap)
        worst = max(worst, gap)
    print(f"{kind}: float64 in torchmetrics' form is up to {worst:.1e} per window from the two-pass float64 reference")


@pytest.mark.parametrize("kind", R.KINDS)
def test_identical_images_give_one_and_infinity(kind):
    from neurad_studio_amd.model_components import image_metrics as IM

    a, _, _, _ = case(kind, 96, 160)
    assert np.abs(R.ssim_valid(a, a) - 1.0).max() <= 1e-12
    assert abs(R.ssim_padded(a, a) - 1.0) <= 1e-12
    assert R.psnr(a, a) == np.inf
    psnr, ssim = IM.image_metrics_torch(torch.from_numpy(a.copy()), torch.from_numpy(a.copy()))
    assert float(psnr) == np.inf and abs(float(ssim) - 1.0) <= 1e-12
    assert np.abs(R.emulate(a, a).astype(np.float64) - 1.0).max() <= R.window_bound(a, a).max()


@pytest.mark.parametrize("kind", R.KINDS)
def test_emulated_accumulation_order_stays_inside_the_bound(kind):
    worst = 0.0
    for h, w in SIZES:
        a, b, want, bound = case(kind, h, w)
        got = R.emulate(a, b).astype(np.float64)
        assert np.isfinite(got).all()
        err = np.abs(got - want)
        assert (err <= bound).all(), (kind, h, w, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    a, b, want, bound = case(kind, 96, 160)
    print(f"{kind}: emulation uses {worst:.3f} of B at worst; B at 96 x 160: max {bound.max():.2e}, mean {bound.mean():.2e}, "
          f"ssim {want.mean():.6f}")
    for c, (h, w) in ((1, SIZES[0]), (1, SIZES[3]), (1, SIZES[-1])):
        a, b, want, bound = case(kind, h, w, c)
        assert (np.abs(R.emulate(a, b).astype(np.float64) - want) <= bound).all(), (kind, h, w, c)


WRONG = {
    "sigma 1.45": lambda a, b: R.ssim_valid(a, b, g=R.window(sigma=1.45)),
    "window shifted by one pixel": lambda a, b: R.ssim_valid(a, b, shift=1),
    "k2 0.029": lambda a, b: R.ssim_valid(a, b, k2=0.029),
    "window sums to 1.001": lambda a, b: R.ssim_valid(a, b, g=R.window(total=1.001)),
    "R from one image only": lambda a, b: R.ssim_valid(a, b, r=float(a.astype(np.float64).max() - a.astype(np.float64).min())),
}


@pytest.mark.parametrize("what", sorted(WRONG))
def test_the_bound_is_not_vacuous(what):
    """each wrong restatement leaves B on at least one window of at least one test image"""
    over = {}
    for kind in R.KINDS:
        a, b, want, bound = case(kind, 96, 160)
        over[kind] = float((np.abs(WRONG[what](a, b) - want) / bound).max())
    print(what, {k: f"{v:.3g} B" for k, v in over.items()})
    assert max(over.values()) > 1.0, (what, over)


def test_fp32_torchmetrics_arithmetic_against_float64_recorded_not_asserted():
    """how far the reference's own fp32 formulation is from the float64 value, per window and for the mean, with and without
    the variance clamp: the figures of DESIGN.md section 8 (expected: 1e-6 on noise, 1e-3 on smooth or near-flat content)"""
    for kind in R.KINDS:
        a, b, want, bound = case(kind, 96, 160)
        row = []
        for clamp in (False, True):
            value, got = R.ssim_padded(a, b, torch.float32, clamp=clamp, return_map=True)
            assert got.shape == want.shape
            row.append((float(np.abs(got - want).max()), abs(value - float(want.mean()))))
        emu = float(np.abs(R.emulate(a, b).astype(np.float64) - want).max())
        print(f"{kind:7s} fp32 torchmetrics form: per window {row[0][0]:.2e} (clamped {row[1][0]:.2e}), mean {row[0][1]:.2e} "
              f"(clamped {row[1][1]:.2e}); kernel's order emulated: per window {emu:.2e}; B max {bound.max():.2e}")


def test_float64_fallback_is_the_restatement():
    from neurad_studio_amd.model_components import image_metrics as IM

    a, b, want, _ = case("smooth", 45, 51)
    ta, tb = torch.from_numpy(a.copy()), torch.from_numpy(b.copy())
    psnr, ssim, m = IM.image_metrics_torch(ta, tb, return_map=True)
    assert psnr.dtype == ssim.dtype == torch.float64
    tol = R.conv_form_float64_error(a, b)  # (the fallback is torchmetrics' one-conv2d form, in float64)
    assert np.abs(m.numpy() - want).max() <= tol and abs(float(ssim) - want.mean()) <= tol
    assert abs(float(psnr) - R.psnr(a, b)) <= 1e-12
    nchw = lambda t: torch.moveaxis(t, -1, 0)[None]  # noqa: E731  (models/neurad.py:581-582)
    transfers = []
    got = IM.image_eval_metrics(nchw(ta), nchw(tb), to_host=lambda v: (transfers.append(tuple(v.shape)), v.tolist())[1])
    assert transfers == [(2,)] and tuple(got) == IM.IMAGE_EVAL_KEYS == ("psnr", "ssim")
    assert all(type(v) is float for v in got.values())
    assert got["ssim"] == float(ssim) and got["psnr"] == float(psnr)
    pair = IM.ImageEvalPair(to_host=lambda v: (transfers.append(tuple(v.shape)), v.tolist())[1])
    x, y = nchw(ta), nchw(tb)
    assert (pair.psnr(x, y), pair.ssim(x, y)) == (got["psnr"], got["ssim"]) and transfers == [(2,)] * 2  # one read for the two
    assert float(IM.ssim(x, y)) == pytest.approx(float(ssim), abs=1e-6) and float(IM.psnr(ta, tb)) == pytest.approx(float(psnr), abs=1e-4)
    with pytest.raises(ValueError):
        IM.image_eval_metrics(ta[:10], tb[:10])
    with pytest.raises(ValueError):
        IM.image_eval_metrics(ta[:, :10], tb[:, :10])
    nan = ta.clone()
    nan[20, 30, 1] = float("nan")
    got = IM.image_eval_metrics(nan, tb)
    assert np.isnan(got["psnr"]) and np.isnan(got["ssim"])


def _metrics(lib, a=ONE, b=ONE, h=20, w=30, c=3, rng=1.0, ws=ONE, ws_bytes=1 << 20, out=ONE):
    fn = lib.nrhip_image_metrics
    fn.restype = ctypes.c_int
    rc = fn(a, b, I32(h), I32(w), I32(c), F32(rng), None, ws, I64(ws_bytes), out, None)
    return rc, lib.nrhip_last_error()


def _psnr(lib, a=ONE, b=ONE, n=100, rng=1.0, ws=ONE, out=ONE):
    fn = lib.nrhip_image_psnr
    fn.restype = ctypes.c_int
    rc = fn(a, b, I64(n), F32(rng), ws, out, None)
    return rc, lib.nrhip_last_error()


def test_argument_checks_run_on_the_host(lib):
    for kw, code, word in [({"a": None}, INVALID_ARG, b"NULL"), ({"b": None}, INVALID_ARG, b"NULL"),
                           ({"out": None}, INVALID_ARG, b"out"), ({"h": 10}, INVALID_ARG, b"window"),
                           ({"w": 10}, INVALID_ARG, b"window"), ({"h": -1}, INVALID_ARG, b"window"),
                           ({"c": 2}, UNSUPPORTED, b"channels"), ({"c": 0}, UNSUPPORTED, b"channels"),
                           ({"c": 4}, UNSUPPORTED, b"channels"), ({"h": 1 << 15, "w": 1 << 15}, UNSUPPORTED, b"2^31"),
                           ({"rng": 0.0}, INVALID_ARG, b"psnr_range"), ({"ws": None}, INVALID_ARG, b"workspace"),
                           ({"ws_bytes": 16}, INVALID_ARG, b"workspace"),
                           ({"ws": ctypes.c_void_p(0x1008)}, INVALID_ARG, b"aligned")]:
        rc, msg = _metrics(lib, **kw)
        assert rc == code and word in msg and b"image_metrics" in msg, (kw, rc, msg)
    for kw, code, word in [({"a": None}, INVALID_ARG, b"NULL"), ({"b": None}, INVALID_ARG, b"NULL"),
                           ({"out": None}, INVALID_ARG, b"out"), ({"n": 0}, INVALID_ARG, b"n = 0"),
                           ({"n": -5}, INVALID_ARG, b"n = -5"), ({"n": 1 << 31}, UNSUPPORTED, b"2^31"),
                           ({"rng": -1.0}, INVALID_ARG, b"psnr_range"), ({"ws": None}, INVALID_ARG, b"workspace"),
                           ({"ws": ctypes.c_void_p(0x1004)}, INVALID_ARG, b"aligned")]:
        rc, msg = _psnr(lib, **kw)
        assert rc == code and word in msg and b"image_psnr" in msg, (kw, rc, msg)


def test_workspace_query_is_host_logic(lib):
    from neurad_studio_amd import _lib

    fn = lib.nrhip_image_metrics_workspace
    fn.restype = ctypes.c_int
    assert _lib.SSIM_TILE == T == 32 and _lib.IMAGE_STAT_ITEMS == 4096

    def need(h, w, c):
        out = I64(-1)
        assert fn(I32(h), I32(w), I32(c), ctypes.byref(out)) == 0, lib.nrhip_last_error()
        return out.value

    up = lambda n, d: (n + d - 1) // d  # noqa: E731
    for h, w, c in [(11, 11, 1), (11, 11, 3), (96, 160, 3), (T + 10, T + 11, 3), (1080, 1920, 3), (900, 1600, 1)]:
        blocks, tiles = up(h * w * c, 4096), up(h - 10, T) * up(w - 10, T) * c
        # float64 squared-error partials, float64 ssim partials, four fp32 min / max per block, c1 / c2 / the NaN carrier
        assert need(h, w, c) == 8 * blocks + 8 * tiles + 16 * blocks + 16, (h, w, c)
        assert need(h, w, c) % 8 == 0
    out = I64(0)
    assert fn(I32(10), I32(11), I32(3), ctypes.byref(out)) == INVALID_ARG and b"window" in lib.nrhip_last_error()
    assert fn(I32(11), I32(11), I32(2), ctypes.byref(out)) == UNSUPPORTED
    assert fn(I32(11), I32(11), I32(3), None) == INVALID_ARG


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from neurad_studio_amd import _lib, ops

    a, b = torch.rand(20, 30, 3), torch.rand(20, 30, 3)
    with pytest.raises(_lib.NeuradHipError):
        ops.image_metrics(a, b)
    with pytest.raises(_lib.NeuradHipError):
        ops.image_psnr(a, b)
    assert ops.SSIM_TILE == T and ops.SSIM_WINDOW == R.TAPS


def test_fused_image_eval_is_opt_in():
    """read from the module's source: importing it needs nerfstudio"""
    src = open(os.path.join(ROOT, "neurad_studio_amd", "integration", "neurad_hip.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "NeuRADHipModelConfig")
    field = next(n for n in cls.body if isinstance(n, ast.AnnAssign) and n.target.id == "fused_image_eval")
    assert ast.literal_eval(field.value) is False and ast.unparse(field.annotation) == "bool"
