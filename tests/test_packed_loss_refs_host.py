"""The packed loss terms, the part that needs no GPU: the numpy restatements of tests/packed_loss_refs.py (which the GPU tests
compare the kernels with) are pinned to the reference's own results in tests/golden/packed_losses.npz, the two forms of the
distortion loss agree within the header's bound, and the C ABI's argument checks run on the host before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import packed_loss_refs as P
from host_gate import HEADER, header_functions

I64, F32 = ctypes.c_int64, ctypes.c_float
ONE = ctypes.c_void_p(0x1000)  # any non-null address: validation fails before anything is dereferenced
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 2
ENTRY_POINTS = ("nrhip_packed_distortion_loss", "nrhip_packed_lidar_carving")


@pytest.fixture(scope="module")
def gold():
    return P.gold()


@pytest.fixture(scope="module")
def dist(gold):
    """the fixture's rays with both restatements evaluated once -> dict"""
    s, e, w, seg = (gold[f"dist_{k}"] for k in ("s", "e", "w", "seg"))
    n, X, S = P.distortion_scales(s, e, w, seg)
    return {"in": (s, e, w, seg), "prefix": P.distortion_prefix(s, e, w, seg),
            "quadratic": P.distortion_quadratic(s, e, w, seg), "loss_term": P.float64_term(n, X, S, 2),
            "grad_term": np.repeat(P.float64_term(n, X, S, 1), np.diff(seg)), "n": n}


def test_the_fixture_holds_the_helper_s_inputs_and_every_kind_of_ray(gold):
    s, e, w, seg = P.distortion_case(P.GOLD_COUNTS)
    for k, a in (("s", s), ("e", e), ("w", w), ("seg", seg)):
        assert np.array_equal(gold[f"dist_{k}"], a), k
    assert np.array_equal(np.diff(seg), P.GOLD_COUNTS)
    # the long case starts with the fixture's rays: the recorded results pin its first rays too
    sl, el, wl, segl = P.distortion_case()
    M = int(seg[-1])
    assert np.array_equal(sl[:M], s) and np.array_equal(el[:M], e) and np.array_equal(wl[:M], w) and segl[-1] == M + 1000
    m = (s.astype(np.float64) + e) / 2
    tied = zero = gap = 0
    for r in range(len(seg) - 1):
        b, c = int(seg[r]), int(seg[r + 1])
        assert np.all(np.diff(m[b:c]) >= 0) and np.all(e[b:c] >= s[b:c]), f"ray {r}: the precondition"
        tied += int((np.diff(m[b:c]) == 0).sum())
        zero += int((e[b:c] == s[b:c]).sum())
        gap += int((s[b + 1:c] > e[b:max(c - 1, b)]).sum())
    assert tied > 20 and zero > 20 and gap > 100 and len(gold["dist_contiguous_rays"]) >= 4 and (w == 0).sum() > 20
    c = P.carving_case()
    for k, a in c.items():
        assert np.array_equal(gold[f"carve_{k}"], a), k
    assert float(gold["carve_eps"]) == P.EPS and float(gold["carve_non_return"]) == P.NON_RETURN


def test_quadratic_restatement_is_the_reference_s_expression(gold, dist):
    """math.fsum against torch's float64 sums of the same products: within the float64 term of the bound alone"""
    loss, grad = dist["quadratic"]
    assert np.all(np.abs(loss - gold["dist_loss"]) <= dist["loss_term"])
    assert np.all(np.abs(grad - gold["dist_grad"]) <= dist["grad_term"])
    assert np.all(gold["dist_loss"][dist["n"] == 0] == 0) and gold["dist_loss"].max() > 1e-3


def test_lossfun_distortion_agrees_on_the_contiguous_rays(gold, dist):
    rays = gold["dist_contiguous_rays"]
    assert np.all(np.abs(dist["quadratic"][0][rays] - gold["dist_contiguous_loss"]) <= dist["loss_term"][rays])
    assert np.all(np.abs(gold["dist_loss"][rays] - gold["dist_contiguous_loss"]) <= dist["loss_term"][rays])


def test_prefix_contract_agrees_with_the_quadratic_form_within_the_bound(gold, dist):
    """the O(n) contract in float64 against the O(n^2) form and against the reference: the float64 term of the bound (no
    fp32 rounding here), on the fixture's rays and on the ray of 1000 samples"""
    (pl, pg), (ql, qg) = dist["prefix"], dist["quadratic"]
    assert np.all(np.abs(pl - ql) <= dist["loss_term"]) and np.all(np.abs(pg - qg) <= dist["grad_term"])
    assert np.all(np.abs(pl - gold["dist_loss"]) <= dist["loss_term"])
    assert np.all(np.abs(pg - gold["dist_grad"]) <= dist["grad_term"])
    s, e, w, seg = P.distortion_case()
    b = int(seg[-2])
    one = (s[b:], e[b:], w[b:], np.array([0, 1000], np.int64))
    n, X, S = P.distortion_scales(*one)
    (pl, pg), (ql, qg) = P.distortion_prefix(*one), P.distortion_quadratic(*one)
    assert ql[0] > 0 and np.abs(pl - ql)[0] <= P.float64_term(n, X, S, 2)[0]
    assert np.all(np.abs(pg - qg) <= P.float64_term(n, X, S, 1)[0])
    # the bound is not vacuous: far below the values it guards
    assert P.float64_term(n, X, S, 2)[0] < 1e-9 * ql[0]


def test_gradient_restatement_is_the_derivative_of_the_loss(dist):
    """analytic check on one ray: the loss is a quadratic form in w, so a central difference is exact up to rounding"""
    s, e, w, seg = dist["in"]
    r = 20  # 250 samples
    b, c = int(seg[r]), int(seg[r + 1])
    one = lambda wr: P.distortion_prefix(s[b:c], e[b:c], wr, np.array([0, c - b]))[0][0]  # noqa: E731
    w64 = w[b:c].astype(np.float64)
    for k in (0, 17, 128, 249):
        h = np.zeros(c - b)
        h[k] = 1e-3
        fd = (one(w64 + h) - one(w64 - h)) / 2e-3
        assert abs(fd - dist["prefix"][1][b + k]) <= 1e-9 * max(1.0, abs(fd))


def test_mask_restatement_is_the_reference_s_bit_for_bit(gold):
    c = P.carving_case()
    args = (c["t_starts"], c["t_ends"], c["seg"], c["is_lidar"])
    mask = P.carving_mask(*args, c["did_return"], c["distance"])
    assert mask.dtype == np.bool_ and np.array_equal(mask, gold["carve_mask"])
    assert np.array_equal(P.carving_mask(*args, None, c["distance"]), gold["carve_mask_all_returned"])
    assert not np.array_equal(gold["carve_mask"], gold["carve_mask_all_returned"])
    # the boundaries, both strict: |10 - 9.5| < 0.5 is false, one float inside is true; mid == non_return is false
    b13, b14 = int(c["seg"][13]), int(c["seg"][14])
    assert list(mask[b13 + 20:b13 + 24]) == [False, True, True, False]
    assert list(mask[b14 + 30:b14 + 32]) == [True, False]
    rep = np.diff(c["seg"])
    lid = np.repeat(c["is_lidar"], rep)
    assert not mask[~lid].any() and mask[lid].any() and (~mask[lid]).any()
    assert (~c["is_lidar"]).sum() >= 7 and (c["is_lidar"] & c["did_return"]).sum() >= 7 and \
        (c["is_lidar"] & ~c["did_return"]).sum() >= 7


def test_power_spacing_to_spacing_inverts_the_spacing_map_and_keeps_the_order():
    from neurad_studio_amd.model_components.ray_samplers import PowerSpacing

    near, far = torch.full((5, 1), 0.05, dtype=torch.float64), torch.full((5, 1), 2000.0, dtype=torch.float64)
    sp = PowerSpacing(near, far, -1.5, 2.0)
    x = torch.linspace(0.0, 1.0, 33, dtype=torch.float64)[None].expand(5, -1)
    t = sp(x)
    assert torch.allclose(sp.to_spacing(t), x, atol=1e-9) and bool((t[:, 1:] > t[:, :-1]).all())


# ---- the C ABI, without a device ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import os

    import __graft_entry__ as ge
    from neurad_studio_amd import _lib

    if not os.path.exists(ge.LIB):
        ge.build()
    return _lib.load()


def _distortion(lib, r, m, s=ONE, e=ONE, w=ONE, seg=ONE, loss=ONE, grad=ONE):
    return lib.nrhip_packed_distortion_loss(s, e, w, seg, I64(r), I64(m), loss, grad, None)


def _carving(lib, r, m, ts=ONE, te=ONE, w=ONE, seg=ONE, lid=ONE, ret=ONE, dist=ONE, close=ONE, loss=ONE, grad=ONE):
    return lib.nrhip_packed_lidar_carving(ts, te, w, seg, lid, ret, dist, F32(0.5), F32(150.0), I64(r), I64(m), close, loss,
                                          grad, None)


def test_header_prototypes_and_exports_agree(lib):
    from neurad_studio_amd import _lib, ops

    fns = header_functions()
    for name in ENTRY_POINTS:
        assert name in fns, f"{name} is not declared in include/neurad_hip.h"
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.nrhip_version() >= 520
    assert ops.PACKED_DISTORTION_C == _lib.PACKED_DISTORTION_C == P.C_BOUND == 16
    assert "#define NRHIP_PACKED_DISTORTION_C 16" in open(HEADER).read()


def test_zero_rays_is_a_no_op_with_every_pointer_null(lib):
    n = None
    assert _distortion(lib, 0, 0, n, n, n, n, n, n) == OK
    assert _distortion(lib, 0, 8, n, n, n, n, n, n) == OK
    assert _carving(lib, 0, 0, n, n, n, n, n, n, n, n, n, n) == OK


def test_null_pointers_and_bad_counts_are_invalid_arguments(lib):
    err = lib.nrhip_last_error
    for call, who in ((_distortion, b"packed_distortion_loss:"), (_carving, b"packed_lidar_carving:")):
        for r, m in ((-1, 8), (4, -8)):
            assert call(lib, r, m) == INVALID_ARG
            assert err().startswith(who) and b"negative" in err(), err()
        assert call(lib, 4, 8, seg=None) == INVALID_ARG
        assert err().startswith(who) and b"segments" in err(), err()
        assert call(lib, 4, 8, loss=None, grad=None, **({"close": None} if call is _carving else {})) == INVALID_ARG
        assert err().startswith(who) and b"NULL" in err(), err()
    for null in ("s", "e", "w"):
        assert _distortion(lib, 4, 8, **{null: None}) == INVALID_ARG
        assert b"NULL sample pointer" in err(), err()
    for null in ("ts", "te"):
        assert _carving(lib, 4, 8, **{null: None}) == INVALID_ARG
        assert b"NULL sample pointer" in err(), err()
    for null in ("lid", "dist"):
        assert _carving(lib, 4, 8, **{null: None}) == INVALID_ARG
        assert b"NULL" in err(), err()
    assert _carving(lib, 4, 8, w=None) == INVALID_ARG  # the loss and the gradient need the weights
    assert b"weights" in err(), err()


def test_two_to_the_31_samples_are_unsupported_and_say_so(lib):
    for call, who in ((_distortion, b"packed_distortion_loss:"), (_carving, b"packed_lidar_carving:")):
        assert call(lib, 4, 1 << 31) == UNSUPPORTED
        assert lib.nrhip_last_error().startswith(who) and b"2^31" in lib.nrhip_last_error()


def test_wrappers_and_public_functions_refuse_cpu_tensors_and_bad_addressing():
    from neurad_studio_amd import _lib, ops
    from neurad_studio_amd.model_components.lidar_losses import packed_carving_loss, packed_is_close_to_lidar
    from neurad_studio_amd.model_components.losses import packed_distortion_loss

    z = torch.zeros
    seg, ri = torch.tensor([0, 2, 2, 6]), torch.tensor([0, 0, 2, 2, 2, 2])
    lid = torch.tensor([True, False, True])
    calls = [lambda: ops.packed_distortion_loss_rays(z(6), z(6), z(6), seg),
             lambda: ops.packed_lidar_carving(z(6), z(6), seg, lid, lid, z(3), 0.5, 150.0, weights=z(6)),
             lambda: packed_distortion_loss(z(6, 1), z(6), z(6), segments=seg),
             lambda: packed_carving_loss(z(6, 1), z(6), z(6), lid, None, z(3), 0.5, 150.0, segments=seg),
             lambda: packed_is_close_to_lidar(z(6), z(6), lid, lid, z(3, 1), 0.5, 150.0, segments=seg)]
    for k, fn in enumerate(calls):
        with pytest.raises(_lib.NeuradHipError):
            fn()
            pytest.fail(f"call {k} computed on CPU tensors")
    for kw in ({}, {"segments": seg, "ray_indices": ri, "num_rays": 3}, {"ray_indices": ri}):
        with pytest.raises(ValueError):  # exactly one addressing; ray_indices need num_rays
            packed_distortion_loss(z(6), z(6), z(6), **kw)
        with pytest.raises(ValueError):
            packed_carving_loss(z(6), z(6), z(6), lid, None, z(3), 0.5, 150.0, **kw)
