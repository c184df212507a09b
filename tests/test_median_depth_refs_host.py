"""The numpy restatement of the median-depth contract (tests/median_depth_refs.py) against the reference's own
DepthRenderer("median") on the CPU (tests/golden/median_depth.npz, scripts/make_golden_median_depth.py), bit for bit; the
exactness of every fixture input's float64 partial sums -- the condition under which the order of the additions, and with it
a wave-level scan, cannot move an index; and the host-side surface of the two entry points: header, prototype table, argument
checks before any launch, the refusal of CPU tensors."""
import ctypes

import numpy as np
import pytest

import median_depth_refs as M
from conftest import load_golden
from host_gate import header_functions

NAMES = ("nrhip_median_depth", "nrhip_median_depth_packed")


@pytest.fixture(scope="module")
def gold():
    return load_golden("median_depth")


@pytest.mark.parametrize("S", M.SHAPES)
def test_restatement_equals_the_reference_bit_for_bit(gold, S):
    assert tuple(gold["shapes"]) == M.SHAPES and int(gold["n_rays"]) == M.R
    w, s, e = M.dense_case(S)
    for tag, a in (("w", w), ("s", s), ("e", e)):  # the regenerated inputs are the ones the reference saw
        assert np.array_equal(M.checksum(a), gold[f"{tag}_sum_{S}"]), (tag, S)
    depth, index = M.median_depth(w, s, e)
    assert depth.dtype == np.float32 and np.array_equal(depth, gold[f"depth_{S}"])
    assert M.partial_sums_exact(w)
    # the cases the recipe is there for: the clamp, and crossings on both sides of the 64-sample chunk
    never = np.cumsum(w.astype(np.float64), -1)[:, -1] < 0.5
    assert 60 <= int(never.sum()) <= 140 and np.all(index[never, 0] == S - 1)
    have = set(index[~never, 0].tolist())
    assert {0, S - 1} <= have and (S < 65 or {63, 64} <= have) and (S < 63 or len(have) >= 45)


def test_constructed_rays(gold):
    w, s, e, want = M.constructed_case()
    for k in ("w", "starts", "ends"):
        assert np.array_equal(gold[f"constructed_{k}"], {"w": w, "starts": s, "ends": e}[k]), k
    depth, index = M.median_depth(w, s, e)
    assert np.array_equal(index[:, 0], want) and np.array_equal(want, gold["constructed_index"])
    assert np.array_equal(depth, gold["constructed_depth"])
    assert M.partial_sums_exact(w, unit_log2=-28)
    # what the two telling rays tell apart
    names = list(M.constructed_rays())
    tiny, half = w[names.index("fp32_accumulator")], w[names.index("float64_compare")]
    acc = np.float32(0)
    for v in tiny:
        acc = np.float32(acc + v)
    assert acc < np.float32(0.5)  # an fp32 accumulator never crosses -> the last sample, not 4
    c64 = np.cumsum(half.astype(np.float64))
    assert int(np.argmax(~(c64 < 0.5))) == 2 and np.float32(c64[1]) == np.float32(0.5)  # a float64 comparison gives 2
    assert np.array_equal(w[names.index("tie")][:3], np.full(3, 0.25, np.float32))  # c_1 == 0.5 exactly: side="left"


def test_restatement_nan_tie_and_empty_rules():
    n = 8
    s, e = M.edges(1, n, 5)
    w = np.full(n, 0.125, np.float32)
    assert M.median_depth_ray(w, s[0], e[0])[1] == 3  # c_3 == 0.5 exactly: side="left"
    late = w.copy()
    late[5] = np.nan
    assert M.median_depth_ray(late, s[0], e[0]) == M.median_depth_ray(w, s[0], e[0])  # behind the crossing: never looked at
    early = w.copy()
    early[1] = np.nan
    d, k = M.median_depth_ray(early, s[0], e[0])
    assert np.isnan(d) and k == 1  # kept, at the first NaN sum
    assert M.median_depth_ray(np.zeros(0, np.float32), s[0, :0], e[0, :0]) == (0.0, -1)
    neg = np.array([0.6, -0.4, 0.1, 0.3], np.float32)
    assert M.median_depth_ray(neg, s[0, :4], e[0, :4])[1] == 0  # non-monotone sums: still the FIRST crossing
    d3, i3 = M.median_depth(w[None], s, e, (0.1, 0.5, 0.9))
    assert i3.tolist() == [[0, 3, 7]] and d3.shape == (1, 3)


def test_packed_case_covers_every_length():
    w, s, e, seg, counts = M.packed_case()
    assert counts[0] == 0 and counts[-1] == 0 and set(counts.tolist()) == set(M.PACKED_LENGTHS) and len(counts) == M.R
    assert seg[-1] == w.shape[0] == s.shape[0] == e.shape[0]
    assert all(M.partial_sums_exact(w[a:b]) for a, b in zip(seg[:-1], seg[1:]) if b > a)
    depth, index = M.median_depth_packed(w, s, e, seg)
    assert np.all(index[counts == 0, 0] == -1) and np.all(depth[counts == 0, 0] == 0)
    assert np.all((index[counts > 0, 0] >= 0) & (index[counts > 0, 0] < counts[counts > 0]))


# ---- the entry points on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from neurad_studio_amd import _lib

    return _lib.load()


def test_header_prototypes_and_exports(lib):
    from neurad_studio_amd import _lib, ops

    for name, n_args in zip(NAMES, (10, 11)):
        assert name in header_functions(), f"{name} is not declared in include/neurad_hip.h"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name]) == n_args
        assert hasattr(lib, name), f"{name} is not exported"
    assert ops.MEDIAN_MAX_THRESHOLDS == _lib.MEDIAN_MAX_THRESHOLDS == 8


def test_arguments_are_checked_on_the_host_before_any_launch(lib):
    I32, I64 = ctypes.c_int32, ctypes.c_int64
    one = ctypes.c_void_p(0x1000)  # any non-null address: validation fails before anything is dereferenced
    q = lambda *v: (ctypes.c_float * len(v))(*v)  # noqa: E731
    dense = lambda r, s, th, k: lib.nrhip_median_depth(one, one, one, I64(r), I32(s), th, I32(k), one, None, None)  # noqa: E731
    packed = lambda r, m, th, k: lib.nrhip_median_depth_packed(one, one, one, one, I64(r), I64(m), th, I32(k), one, None,  # noqa: E731
                                                               None)
    for fn in (dense, packed):
        assert fn(5, 4, q(), 0) == 1                         # K = 0
        assert fn(5, 4, q(*[0.5] * 9), 9) == 1               # K = 9
        assert fn(5, 4, q(0.5, float("nan")), 2) == 1        # a NaN threshold
        assert fn(5, 4, q(float("inf")), 1) == 1             # an infinite one
        assert fn(5, 4, None, 1) == 1                        # no thresholds
        assert fn(-1, 4, q(0.5), 1) == 1
        assert fn(0, 4, q(*[0.5] * 8), 8) == 0               # R = 0: a no-op, K = 8 accepted
    assert dense(5, 0, q(0.5), 1) == 1 and b"at least one" in lib.nrhip_last_error()  # S = 0
    assert packed(5, -1, q(0.5), 1) == 1
    assert packed(5, 1 << 31, q(0.5), 1) == 2                # NRHIP_ERR_UNSUPPORTED
    assert lib.nrhip_median_depth(None, one, one, I64(5), I32(4), q(0.5), I32(1), one, None, None) == 1
    assert lib.nrhip_median_depth_packed(one, one, one, None, I64(5), I64(3), q(0.5), I32(1), one, None, None) == 1
    assert lib.nrhip_median_depth_packed(None, one, one, one, I64(5), I64(3), q(0.5), I32(1), one, None, None) == 1


def test_wrappers_and_renderer_refuse_cpu_tensors_and_gradients():
    import torch

    from neurad_studio_amd import _lib, ops
    from neurad_studio_amd.cameras.rays import Frustums, RaySamples
    from neurad_studio_amd.model_components.renderers import DepthRenderer

    z = torch.zeros
    with pytest.raises(_lib.NeuradHipError):
        ops.median_depth(z(3, 4), z(3, 4), z(3, 4))
    with pytest.raises(_lib.NeuradHipError):
        ops.median_depth_packed(z(5), z(5), z(5), z(3, dtype=torch.int64))
    assert DepthRenderer().method == "expected"  # the default stays
    r = DepthRenderer("median", quantile=0.25)
    assert (r.method, r.quantile) == ("median", 0.25)
    with pytest.raises(NotImplementedError):
        DepthRenderer("mean")
    fr = Frustums(origins=z(3, 4, 3), directions=z(3, 4, 3), starts=z(3, 4, 1, requires_grad=True), ends=z(3, 4, 1),
                  pixel_area=z(3, 4, 1))
    with pytest.raises(NotImplementedError, match="piecewise constant"):
        r(z(3, 4, 1), RaySamples(frustums=fr))
    with torch.no_grad(), pytest.raises(_lib.NeuradHipError):  # grad disabled: goes on to the op, which has no CPU path
        r(z(3, 4, 1), RaySamples(frustums=fr))
