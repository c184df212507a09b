"""Median depth on the device (csrc/median_depth.hip: nrhip_median_depth, nrhip_median_depth_packed) against the numpy
restatement of its contract (tests/median_depth_refs.py, pinned to the reference's DepthRenderer("median") on the CPU by
tests/test_median_depth_refs_host.py): exact equality of depth and index.  Every weight is a multiple of 2^-24 (2^-28 for the
constructed rays) with exact float64 partial sums, so the order in which the wave scan adds them cannot show; what shows is
an fp32 accumulator, a comparison made in float64, a lost carry between 64-sample chunks, a wrong clamp or a wrong tie.
Then the layers above: DepthRenderer("median"), render_packed(median_depth=True) and FusedEvalMixin.median_depth."""
import numpy as np
import pytest
import torch

import median_depth_refs as M
from gpu_util import bundle, cuda, host, small_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from neurad_studio_amd import ops

    return ops


def run_dense(ops, w, s, e, thresholds=(0.5,)):
    d, i = ops.median_depth(cuda(w), cuda(s), cuda(e), thresholds, return_index=True)
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and d.shape == i.shape == (w.shape[0], len(thresholds))
    return host(d), host(i)


def same(got, want):
    """exact, a NaN equal to a NaN"""
    return got.dtype == want.dtype and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


# ---- dense ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", M.SHAPES)
def test_dense_equals_the_restatement(ops, S):
    w, s, e = M.dense_case(S)
    want_d, want_i = M.median_depth(w, s, e)
    got_d, got_i = run_dense(ops, w, s, e)
    assert same(got_i, want_i), np.flatnonzero(got_i != want_i)[:8]
    assert same(got_d, want_d)
    assert same(host(ops.median_depth(cuda(w), cuda(s), cuda(e))), want_d)  # without the index output
    # crossings at sample 0, 63, 64, S - 1 and never: all present where S has them
    never = np.cumsum(w.astype(np.float64), -1)[:, -1] < 0.5
    assert never.any() and np.all(got_i[never, 0] == S - 1)
    have = set(got_i[~never, 0].tolist())
    assert {0, S - 1} <= have and (S < 65 or {63, 64} <= have)


def test_all_five_crossing_places_occur(ops):
    w, s, e = M.dense_case(200)
    _, i = run_dense(ops, w, s, e)
    never = np.cumsum(w.astype(np.float64), -1)[:, -1] < 0.5
    assert i[:5, 0].tolist() == [0, 63, 64, 199, 199] and never[:5].tolist() == [False, False, False, False, True]


def test_constructed_rays(ops):
    w, s, e, want_i = M.constructed_case()
    want_d, ref_i = M.median_depth(w, s, e)
    got_d, got_i = run_dense(ops, w, s, e)
    assert np.array_equal(ref_i[:, 0], want_i)
    assert got_i[:, 0].tolist() == want_i.tolist(), dict(zip(M.constructed_rays(), got_i[:, 0]))
    assert same(got_d, want_d)


def test_nan_rule(ops):
    """a NaN behind the crossing is never looked at; a NaN at or before it: NaN depth, the index of the first NaN sum --
    across the chunk boundary as well"""
    S = 130
    w, s, e = M.dense_case(S, seed=4242)
    w, s, e = w[:8].copy(), s[:8], e[:8]
    w[:] = np.float32(3 * M.UNIT)
    for r, at in enumerate((0, 5, 63, 64, 100, 129, 70, 2)):
        w[r, at] = 0.75
    clean_d, clean_i = M.median_depth(w, s, e)
    late = w.copy()
    for r, at in enumerate((1, 6, 64, 65, 101, 129, 128, 64)):
        if at > clean_i[r, 0]:
            late[r, at] = np.nan
    got_d, got_i = run_dense(ops, late, s, e)
    assert same(got_i, clean_i) and same(got_d, clean_d) and np.isfinite(got_d).all()
    assert same(got_d, M.median_depth(late, s, e)[0])
    early = w.copy()
    nan_at = (0, 3, 10, 63, 64, 128, 0, 1)
    for r, at in enumerate(nan_at):
        early[r, at] = np.nan
    want_d, want_i = M.median_depth(early, s, e)
    got_d, got_i = run_dense(ops, early, s, e)
    assert same(got_i, want_i) and same(got_d, want_d)
    hit = np.array([at <= clean_i[r, 0] for r, at in enumerate(nan_at)])
    assert hit.sum() >= 6 and np.isnan(got_d[hit, 0]).all() and got_i[hit, 0].tolist() == [a for a, h in zip(nan_at, hit) if h]
    assert np.isfinite(got_d[~hit, 0]).all()


def test_thresholds(ops):
    from neurad_studio_amd._lib import NeuradHipError

    w, s, e = M.dense_case(129)
    q3 = (0.1, 0.5, 0.9)
    want_d, want_i = M.median_depth(w, s, e, q3)
    got_d, got_i = run_dense(ops, w, s, e, q3)
    assert same(got_d, want_d) and same(got_i, want_i)
    for k, q in enumerate(q3):  # one call with K = 3 == three calls with K = 1
        d1, i1 = run_dense(ops, w, s, e, (q,))
        assert same(d1[:, 0], got_d[:, k]) and same(i1[:, 0], got_i[:, k])
    assert len({tuple(r) for r in got_i.tolist()}) > 50 and (got_i[:, 0] <= got_i[:, 1]).all()
    q8 = (0.9, 0.05, 0.5, 0.25, 1.25, 0.0, 0.75, 0.5)  # unordered, a repeat, one nothing reaches, one everything does
    want_d, want_i = M.median_depth(w, s, e, q8)
    got_d, got_i = run_dense(ops, w, s, e, q8)
    assert same(got_d, want_d) and same(got_i, want_i) and (got_i[:, 5] == 0).all()
    W, Sx, E = cuda(w), cuda(s), cuda(e)
    for bad in ((), (0.5,) * 9, (0.5, float("nan")), (float("inf"),)):
        with pytest.raises(NeuradHipError):
            ops.median_depth(W, Sx, E, bad)
    with pytest.raises(NeuradHipError):
        ops.median_depth(W[:, :0], Sx[:, :0], E[:, :0])  # S = 0
    with pytest.raises(NeuradHipError):
        ops.median_depth(W.cpu(), Sx.cpu(), E.cpu())
    d0, i0 = ops.median_depth(W[:0], Sx[:0], E[:0], q3, return_index=True)  # R = 0
    assert d0.shape == i0.shape == (0, 3)


# ---- packed ---------------------------------------------------------------------------------------------------------------
def test_packed_equals_the_restatement(ops):
    from neurad_studio_amd._lib import NeuradHipError

    w, s, e, seg, counts = M.packed_case()
    assert counts[0] == 0 and counts[-1] == 0 and set(counts.tolist()) == set(M.PACKED_LENGTHS)
    q3 = (0.1, 0.5, 0.9)
    want_d, want_i = M.median_depth_packed(w, s, e, seg, q3)
    got_d, got_i = ops.median_depth_packed(cuda(w), cuda(s), cuda(e), cuda(seg), q3, return_index=True)
    got_d, got_i = host(got_d), host(got_i)
    assert same(got_i, want_i) and same(got_d, want_d)
    empty = counts == 0
    assert empty.sum() >= 3 and (got_d[empty] == 0).all() and (got_i[empty] == -1).all()
    assert same(host(ops.median_depth_packed(cuda(w), cuda(s), cuda(e), cuda(seg))), want_d[:, 1:2])
    # segments from ray_indices
    ri = cuda(np.repeat(np.arange(len(counts)), counts))
    assert torch.equal(ops.packed_segments(ri, len(counts)), cuda(seg))
    # M = 0: every ray empty
    z, zseg = torch.empty(0, device="cuda"), torch.zeros(6, dtype=torch.int64, device="cuda")
    d0, i0 = ops.median_depth_packed(z, z, z, zseg, q3, return_index=True)
    assert d0.shape == (5, 3) and (d0 == 0).all() and (i0 == -1).all()
    dr, ir = ops.median_depth_packed(z, z, z, zseg[:1], q3, return_index=True)  # R = 0
    assert dr.shape == ir.shape == (0, 3)
    for bad in ((), (0.5,) * 9, (float("nan"),)):
        with pytest.raises(NeuradHipError):
            ops.median_depth_packed(cuda(w), cuda(s), cuda(e), cuda(seg), bad)
    with pytest.raises(NeuradHipError):
        ops.median_depth_packed(torch.from_numpy(w), torch.from_numpy(s), torch.from_numpy(e), torch.from_numpy(seg))


@pytest.mark.parametrize("S", (1, 65, 200))
def test_a_dense_batch_packed_gives_the_dense_bits(ops, S):
    w, s, e = M.dense_case(S)
    q3 = (0.1, 0.5, 0.9)
    d, i = ops.median_depth(cuda(w), cuda(s), cuda(e), q3, return_index=True)
    seg = torch.arange(M.R + 1, device="cuda", dtype=torch.int64) * S
    dp, ip = ops.median_depth_packed(cuda(w).reshape(-1), cuda(s).reshape(-1), cuda(e).reshape(-1), seg, q3, return_index=True)
    assert torch.equal(d, dp) and torch.equal(i, ip)


# ---- modules --------------------------------------------------------------------------------------------------------------
def _samples(s, e):
    from neurad_studio_amd.cameras.rays import Frustums, RaySamples

    S, E = cuda(s)[..., None], cuda(e)[..., None]
    z = torch.zeros((*S.shape[:-1], 3), device="cuda")
    return RaySamples(frustums=Frustums(origins=z, directions=z, starts=S, ends=E, pixel_area=torch.ones_like(S)))


def test_depth_renderer_median_dense_and_packed(ops):
    from neurad_studio_amd.model_components.renderers import DepthRenderer

    w, s, e = M.dense_case(65)
    r = DepthRenderer("median")
    got = r(cuda(w)[..., None], _samples(s, e))
    assert got.shape == (M.R, 1) and not got.requires_grad
    assert torch.equal(got, ops.median_depth(cuda(w), cuda(s), cuda(e)))
    assert same(host(got), M.median_depth(w, s, e)[0])
    got_q = DepthRenderer("median", quantile=0.9)(cuda(w)[..., None], _samples(s, e))
    assert torch.equal(got_q, ops.median_depth(cuda(w), cuda(s), cuda(e), (0.9,))) and not torch.equal(got_q, got)
    # weights that carry a graph are fine (the result is detached); starts that require grad are refused
    wg = cuda(w)[..., None].requires_grad_()
    assert torch.equal(r(wg, _samples(s, e)), got)
    rs = _samples(s, e)
    rs.frustums.starts.requires_grad_()
    with pytest.raises(NotImplementedError, match="piecewise constant"):
        r(cuda(w)[..., None], rs)
    # packed
    pw, ps, pe, seg, counts = M.packed_case()
    ri = cuda(np.repeat(np.arange(len(counts)), counts))
    gotp = r(cuda(pw)[:, None], _samples(ps, pe), ray_indices=ri, num_rays=len(counts))
    assert gotp.shape == (len(counts), 1)
    assert torch.equal(gotp, ops.median_depth_packed(cuda(pw), cuda(ps), cuda(pe), cuda(seg)))
    assert same(host(gotp), M.median_depth_packed(pw, ps, pe, seg)[0])


def test_render_packed_carries_the_median_depth(ops):
    from neurad_studio_amd.model_components.renderers import render_packed

    pw, ps, pe, seg, counts = M.packed_case()
    ri = cuda(np.repeat(np.arange(len(counts)), counts))
    alpha = cuda(np.clip(pw * 8, 0.0, 0.9).astype(np.float32))
    feat = torch.ones((pw.shape[0], 4), device="cuda")
    rs = _samples(ps, pe)
    plain = render_packed(feat, rs, ri, len(counts), alpha=alpha)
    out = render_packed(feat, rs, ri, len(counts), alpha=alpha, median_depth=True)
    assert set(out) == set(plain) | {"median_depth"} and "median_depth" not in plain
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    md = out["median_depth"]
    assert md.shape == (len(counts), 1) and not md.requires_grad
    assert torch.equal(md, ops.median_depth_packed(out["weights"][:, 0], cuda(ps), cuda(pe), cuda(seg)))
    want, _ = M.median_depth_packed(host(out["weights"][:, 0]), ps, pe, seg)
    # (these weights are products, their float64 sums not exact: the restatement's sequential sum and the wave scan may
    # round a sum differently in its last float64 bit, which reaches float32 only in a tie of probability ~2^-29 per sample)
    assert same(host(md), want)


# ---- model ----------------------------------------------------------------------------------------------------------------
def test_fused_eval_outputs_carry_the_median_depth():
    import synth

    m = small_model(use_sdf=False).eval()  # (the density head: the crossing moves with the sample lengths along a ray)
    R = 300
    o, d, area, _ = synth.rays(R, 21)
    fars = np.full(R, 20000.0, np.float32)
    fars[:100] = 0.05  # 5 cm of this field: these rays never reach one half before the sky sample

    def rays():
        return bundle(o, d, area / 9, fars=fars)

    with torch.no_grad():
        before = m.get_nff_outputs(rays())
    assert "median_depth" not in before
    seen = {}
    render = m.field.render

    def spy(o_, d_, area_, starts, ends, **kw):
        out = render(o_, d_, area_, starts, ends, **kw)
        seen.update(starts=starts, ends=ends, out=out, kw=kw)
        return out

    m.field.render = spy
    m.median_depth = True
    with torch.no_grad():
        out = m.get_nff_outputs(rays())
    assert set(out) == set(before) | {"median_depth"} and seen["kw"]["return_weights"] is True
    for k in before:  # the other outputs do not move
        assert torch.equal(out[k], before[k]), k
    md = out["median_depth"]
    assert md.shape == (R, 1) and md.dtype == torch.float32
    w, s, e = (host(t[:, :-1]) for t in (seen["out"][3], seen["starts"], seen["ends"]))  # the non-sky samples
    want, idx = M.median_depth(w, s, e)
    assert same(host(md), want)
    S = seen["starts"].shape[1]
    assert len(set(idx[:, 0].tolist())) > 3 and int(idx.max()) <= S - 2  # never the sky sample
    never = w.astype(np.float64).sum(-1) < 0.49
    assert never[:100].all() and not never[100:].all()
    assert same(host(md)[never, 0], ((s[:, -1] + e[:, -1]) * np.float32(0.5))[never])  # the last non-sky midpoint
    m.median_depth = False
    with torch.no_grad():
        assert set(m.get_nff_outputs(rays())) == set(before)
