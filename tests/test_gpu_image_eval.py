"""csrc/image_eval.hip on the GPU: the SSIM map per window against the two-pass float64 restatement within the bound B
(tests/image_eval_refs.py: its derivation), the two scalars, the data range taken on the device, bitwise reproducibility, NaN
containment, nrhip_image_psnr at every size where pass 1 takes another path, capture in a HIP graph, and the Python layer's
one transfer.  Sizes: one window, one row / column of windows, one window short of, at and past a tile edge in each
direction, several ragged tiles."""
import numpy as np
import pytest
import torch

import image_eval_refs as R
import synth
from gpu_util import cuda, host, ops  # noqa: F401

pytestmark = pytest.mark.gpu

T = R.TILE
SIZES = R.sizes()
SHAPES = [(h, w, 3) for h, w in SIZES] + [(h, w, 1) for h, w in (SIZES[0], SIZES[3], SIZES[-1])]
STAT = 4096  # NRHIP_IMAGE_STAT_ITEMS: elements per workgroup of the squared-error pass
ULP = lambda v: float(np.spacing(np.float32(abs(v))))  # noqa: E731


def bits(*tensors):
    return [host(t).view(np.uint32).tolist() for t in tensors]


@pytest.mark.parametrize("kind", R.KINDS)
def test_map_per_window_and_both_scalars(ops, kind):
    assert ops.SSIM_TILE == T and ops.IMAGE_STAT_ITEMS == STAT
    for h, w, c in SHAPES:
        a, b, want, bound = R.case(kind, h, w, c)
        what = (kind, h, w, c)
        psnr, ssim, m = ops.image_metrics(cuda(a), cuda(b), return_map=True)
        got = host(m).astype(np.float64)
        assert got.shape == want.shape and not np.isnan(got).any(), what
        err = np.abs(got - want)
        print(f"{what}: map uses {float((err / bound).max()):.3f} of B (B max {bound.max():.2e}, mean {bound.mean():.2e}); "
              f"ssim {float(ssim):.8f} - float64 {float(ssim) - want.mean():+.2e}; psnr {float(psnr):.5f} - float64 "
              f"{float(psnr) - R.psnr(a, b):+.2e}")
        assert (err <= bound).all(), (what, float((err / bound).max()))
        # the scalar is the float64 sum of the kernel's own fp32 values, rounded once
        own = np.float32(got.mean())
        assert abs(float(ssim) - float(own)) <= ULP(own), (what, float(ssim), float(own))
        assert abs(float(ssim) - want.mean()) <= bound.mean(), (what, float(ssim) - want.mean(), bound.mean())
        assert abs(float(psnr) - R.psnr(a, b)) <= R.psnr_bound(R.psnr(a, b)), (what, float(psnr), R.psnr(a, b))
        # without a map: the same two bits
        assert bits(*ops.image_metrics(cuda(a), cuda(b))) == bits(psnr, ssim), what


def test_data_range_comes_from_both_images_on_the_device(ops):
    a, b, want, bound = R.case("range", T + 11, T + 17)
    assert R.data_range(a, b) == 1.0 and float(a.max() - a.min()) < 0.5  # R is b's
    for scale in (1.0, 0.5):  # scaled by 0.5: c1 and c2 scale by 0.25; a power of two, so every value scales exactly
        sa, sb = a * np.float32(scale), b * np.float32(scale)
        ref, bnd = (want, bound) if scale == 1.0 else (R.ssim_valid(sa, sb), R.window_bound(sa, sb))
        psnr, ssim, m = ops.image_metrics(cuda(sa), cuda(sb), return_map=True)
        err = np.abs(host(m).astype(np.float64) - ref)
        assert (err <= bnd).all(), (scale, float((err / bnd).max()))
        assert abs(float(ssim) - ref.mean()) <= bnd.mean()
        assert abs(float(psnr) - R.psnr(sa, sb)) <= R.psnr_bound(R.psnr(sa, sb))
        # taking R from a alone would be far outside: the bound tells the two apart
        wrong = R.ssim_valid(sa, sb, r=float(sa.max()) - float(sa.min()))
        assert (np.abs(wrong - ref) > bnd).any()
    # psnr_range enters as D^2
    p2 = ops.image_metrics(cuda(a), cuda(b), psnr_range=2.0)[0]
    assert abs(float(p2) - R.psnr(a, b, 2.0)) <= R.psnr_bound(R.psnr(a, b, 2.0))


def test_same_inputs_same_bits_and_nan_stays_contained(ops):
    h, w = 2 * T + 13, T + 17
    a, b, want, bound = R.case("noise", h, w)
    da, db = cuda(a), cuda(b)
    first = ops.image_metrics(da, db, return_map=True)
    again = ops.image_metrics(da, db, return_map=True)
    assert bits(*first) == bits(*again)
    for y, x, ch in [(h // 2, w // 2, 1), (T + 9, T + 9, 0), (T + 10, T, 2), (h - 1, w - 1, 2), (0, 0, 0)]:
        for which in (0, 1):
            pair = [da.clone(), db.clone()]
            pair[which][y, x, ch] = float("nan")
            psnr, ssim, m = ops.image_metrics(*pair, return_map=True)
            assert np.isnan(float(psnr)) and np.isnan(float(ssim)), (y, x, ch, which)
            # in the map: every window over the pixel (where it is a tile's pivot: the whole tile), and only in its channel
            bad = np.isnan(host(m))
            assert bad[max(y - 10, 0):y + 1, max(x - 10, 0):x + 1, ch].all() and not bad[..., [k for k in range(3) if k != ch]].any()
    # the process goes on, and the results are what they were
    assert bits(*ops.image_metrics(da, db, return_map=True)) == bits(*first)


@pytest.mark.parametrize("kind", R.KINDS)
def test_identical_images(ops, kind):
    a, _, _, _ = R.case(kind, T + 11, T + 9)
    psnr, ssim, m = ops.image_metrics(cuda(a), cuda(a), return_map=True)
    bound = R.window_bound(a, a)
    assert float(psnr) == float("inf")
    assert (np.abs(host(m).astype(np.float64) - 1.0) <= bound).all()
    assert abs(float(ssim) - 1.0) <= bound.mean(), (float(ssim) - 1.0, bound.mean())


def test_psnr_alone_at_every_size_branch(ops):
    n_max = 3 * 96 * 96 * 3
    a = synth.uniform((n_max,), 0.0, 1.0, 971)
    b = np.clip(a + 0.05 * synth.normal((n_max,), 972), 0.0, 1.0).astype(np.float32)
    da, db = cuda(a), cuda(b)
    for n in (1, 63, 64, 65, STAT - 1, STAT, STAT + 1, n_max):
        want = R.psnr(a[:n], b[:n])
        got = ops.image_psnr(da[:n], db[:n])
        assert got.shape == () and got.dtype == torch.float32
        assert abs(float(got) - want) <= R.psnr_bound(want), (n, float(got), want)
        assert float(ops.image_psnr(da[:n], da[:n])) == float("inf")
    img = (96, 96, 9)  # any shape: flat elements; the same bits as the two-metric entry's psnr on a [H,W,3] image
    assert bits(ops.image_psnr(da[:82944].reshape(img), db[:82944].reshape(img))) == bits(ops.image_psnr(da[:82944], db[:82944]))
    three = (96, 288, 3)
    assert bits(ops.image_metrics(da[:82944].reshape(three), db[:82944].reshape(three))[0]) == bits(ops.image_psnr(da[:82944], db[:82944]))
    bad = db.clone()
    bad[STAT + 5] = float("nan")
    assert np.isnan(float(ops.image_psnr(da, bad)))
    assert float(ops.image_psnr(da, db, psnr_range=2.0)) == pytest.approx(R.psnr(a, b, 2.0), abs=R.psnr_bound(R.psnr(a, b, 2.0)))


def test_graph_replay_on_new_contents_equals_eager(ops):
    h, w = T + 11, 2 * T + 13
    a, b, _, _ = R.case("smooth", h, w)
    a2, b2, _, _ = R.case("noise", h, w)
    da, db = cuda(a), cuda(b)
    ops.image_metrics(da, db, return_map=True), ops.image_psnr(da, db)  # (library loaded, kernels resident)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (a device->host read or a synchronisation inside the capture is an error)
        captured = ops.image_metrics(da, db, return_map=True) + (ops.image_psnr(da, db),)
    for src_a, src_b in ((a2, b2), (a, b)):
        da.copy_(cuda(src_a)), db.copy_(cuda(src_b))
        for x in captured:
            x.fill_(float("nan"))
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")
        try:
            graph.replay()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        replayed = bits(*captured)
        eager = ops.image_metrics(cuda(src_a), cuda(src_b), return_map=True) + (ops.image_psnr(cuda(src_a), cuda(src_b)),)
        assert replayed == bits(*eager)


def test_python_layer_one_transfer_views_and_small_images(ops):
    from neurad_studio_amd.model_components import image_metrics as IM

    a, b, want, bound = R.case("smooth", T + 10, T + 11)
    da, db = cuda(a), cuda(b)
    transfers = []

    def to_host(values):
        torch.cuda.set_sync_debug_mode("default")
        transfers.append(tuple(values.shape))
        return IM.scalars_to_host(values)

    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # nothing before the transfer synchronises
    try:
        got = IM.image_eval_metrics(da, db, to_host=to_host)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert transfers == [(2,)] and tuple(got) == IM.IMAGE_EVAL_KEYS and all(type(v) is float for v in got.values())
    psnr, ssim = ops.image_metrics(da, db)
    assert got == {"psnr": float(psnr), "ssim": float(ssim)}
    assert abs(got["ssim"] - want.mean()) <= bound.mean()
    # the reference's [1,C,H,W] views (models/neurad.py:581-582) and the [H,W,C] tensors: the same bits
    nchw = lambda t: torch.moveaxis(t, -1, 0)[None]  # noqa: E731
    assert bits(*ops.image_metrics(nchw(da), nchw(db))) == bits(psnr, ssim)
    pair = IM.ImageEvalPair(to_host=to_host)
    x, y = nchw(da), nchw(db)
    assert (pair.psnr(x, y), pair.ssim(x, y)) == (got["psnr"], got["ssim"]) and transfers == [(2,)] * 2
    assert bits(IM.ssim(x, y), IM.PSNR(1.0)(x, y)) == bits(ssim, psnr)
    # non-fp32 inputs are cast by the wrapper
    assert bits(*ops.image_metrics(da.double(), db.double())) == bits(psnr, ssim)
    for bad in ((10, 40, 3), (40, 10, 3)):
        with pytest.raises(ValueError):
            ops.image_metrics(torch.zeros(bad, device="cuda"), torch.zeros(bad, device="cuda"))
    with pytest.raises(ValueError):
        ops.image_metrics(torch.zeros(20, 20, 2, device="cuda"), torch.zeros(20, 20, 2, device="cuda"))
    with pytest.raises(ValueError):
        ops.image_metrics(da, db[:-1])
    # two constant images: R = 0, every window 0 / 0 (documented: NaN, as the reference's arithmetic gives); psnr is finite
    flat = ops.image_metrics(torch.full((20, 30, 3), 0.25, device="cuda"), torch.full((20, 30, 3), 0.5, device="cuda"))
    assert np.isnan(float(flat[1])) and float(flat[0]) == pytest.approx(R.psnr(np.float32(0.25), np.float32(0.5)), abs=1e-5)
