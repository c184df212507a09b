"""The VGG perceptual loss, the part that needs no GPU: the additive C ABI (header, ctypes table, exported symbols, version
still 520), the convolution's plan query and host-side argument checks, the module's state-dict names against a stand-in
built the way the reference builds its network (tests/vgg_refs.py), storage sharing of from_reference, the CPU path against
the restated torch network, the float64 restatements against torch's own kernels, and the plugin's opt-in flag."""
import ctypes
import os

import pytest
import torch

import ref_import
import vgg_refs as R
from host_gate import header_functions
from plugin_harness import ref  # noqa: F401

I32, I64 = ctypes.c_int32, ctypes.c_int64
ONE = ctypes.c_void_p(0x1000)  # any non-null, 16-byte aligned address: validation fails before anything is dereferenced
INVALID_ARG, UNSUPPORTED = 1, 2
NEW = ["nrhip_conv3x3_pack_bytes", "nrhip_conv3x3_pack", "nrhip_conv3x3_plan", "nrhip_conv3x3", "nrhip_maxpool2_fwd",
       "nrhip_maxpool2_bwd", "nrhip_l1_feature_workspace", "nrhip_l1_feature_fwd", "nrhip_l1_feature_bwd",
       "nrhip_vgg_stage_images", "nrhip_vgg_image_grad"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(ge.LIB):
        ge.build()
    lib = ctypes.CDLL(ge.LIB)
    lib.nrhip_last_error.restype = ctypes.c_char_p
    return lib


def test_new_entry_points_are_declared_bound_and_exported_and_the_version_stays(lib):
    from neurad_studio_amd import _lib

    declared = header_functions()
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.nrhip_version() == 520
    assert _lib.VGG_IMAGE_CHANNELS == R.IMAGE_CHANNELS == 16 and _lib.L1_ITEMS == 2048


def _plan(lib, m, cin, cout, plan=0):
    mt, nt, waves = I32(-1), I32(-1), I64(-1)
    rc = lib.nrhip_conv3x3_plan(I64(m), I32(cin), I32(cout), I32(plan), ctypes.byref(mt), ctypes.byref(nt), ctypes.byref(waves))
    return rc, (mt.value, nt.value, waves.value), lib.nrhip_last_error()


def test_plan_query_is_host_logic(lib):
    """two 32-channel blocks per wave wherever the output has them; 64 pixels per wave from 2048 such waves on"""
    for cin, cout in R.CHANNEL_PAIRS:
        for a, b in ((cin, cout), (cout, cin)):
            rc, (mt, nt, waves), _ = _plan(lib, 108, a, b)
            nb = 1 if b == 3 else b // 32
            assert rc == 0 and mt == 1 and nt == min(nb, 2) and waves == 4 * (nb // nt)
    # the threshold, at 64 output channels (one wave column): 2048 waves of 64 pixels
    assert _plan(lib, 2048 * 64, 3, 64)[1] == (2, 2, 2048)
    assert _plan(lib, 2047 * 64, 3, 64)[1] == (1, 2, 2 * 2047)
    assert _plan(lib, 2047 * 64 + 1, 3, 64)[1] == (2, 2, 2048)  # a ragged last tile counts
    # the flagship batch: 80 images of 96 x 96 forward, 40 backward
    assert _plan(lib, 80 * 96 * 96, 64, 64)[1] == (2, 2, 11520)
    assert _plan(lib, 80 * 6 * 6, 512, 512)[1] == (1, 2, 90 * 8)
    assert _plan(lib, 40 * 96 * 96, 64, 3)[1] == (2, 1, 5760)
    # a forced plan overrides the pixel blocks only
    assert _plan(lib, 108, 64, 128, plan=2)[1] == (2, 2, 2 * 2)
    assert _plan(lib, 80 * 96 * 96, 64, 64, plan=1)[1] == (1, 2, 23040)
    assert _plan(lib, 0, 64, 64)[1] == (1, 2, 0)


def test_unsupported_arguments_give_a_code_and_a_message(lib):
    rc, _, msg = _plan(lib, 100, 32, 64)
    assert rc == UNSUPPORTED and b"channels 32 -> 64" in msg
    rc, _, msg = _plan(lib, 100, 3, 3)
    assert rc == UNSUPPORTED and b"3 -> 3" in msg
    rc, _, msg = _plan(lib, 100, 64, 64, plan=3)
    assert rc == INVALID_ARG and b"plan 3" in msg
    rc, _, msg = _plan(lib, -1, 64, 64)
    assert rc == INVALID_ARG and b"pixels" in msg
    rc, _, msg = _plan(lib, 1 << 31, 64, 64)
    assert rc == UNSUPPORTED
    assert lib.nrhip_conv3x3_plan(I64(1), I32(64), I32(64), I32(0), None, None, None) == INVALID_ARG
    need = I64(0)
    assert lib.nrhip_conv3x3_pack_bytes(I32(64), I32(3), I32(0), ctypes.byref(need)) == 0 and need.value == 9 * 1 * 2 * 1024
    assert lib.nrhip_conv3x3_pack_bytes(I32(64), I32(3), I32(1), ctypes.byref(need)) == 0 and need.value == 9 * 4 * 1 * 1024
    assert lib.nrhip_conv3x3_pack_bytes(I32(512), I32(512), I32(1), ctypes.byref(need)) == 0 and need.value == 9 * 512 * 512 * 2
    assert lib.nrhip_conv3x3_pack_bytes(I32(48), I32(64), I32(0), ctypes.byref(need)) == UNSUPPORTED
    assert lib.nrhip_conv3x3_pack_bytes(I32(64), I32(64), I32(2), ctypes.byref(need)) == INVALID_ARG
    # the launching entry points validate before they launch
    conv = lambda **k: lib.nrhip_conv3x3(k.get("x", ONE), ONE, k.get("bias"), None, None, None, ONE, I32(k.get("b", 1)),  # noqa: E731
                                         I32(k.get("h", 4)), I32(4), I32(k.get("cin", 64)), I32(k.get("cout", 64)), I32(1),
                                         I32(0), None)
    assert conv(h=0) == INVALID_ARG and b"bad shape" in lib.nrhip_last_error()
    assert conv(cin=100) == UNSUPPORTED
    assert conv(x=None) == INVALID_ARG and b"NULL" in lib.nrhip_last_error()
    assert conv(x=ctypes.c_void_p(0x1002)) == INVALID_ARG and b"aligned" in lib.nrhip_last_error()
    assert conv(cout=3, bias=ONE) == UNSUPPORTED and b"bias" in lib.nrhip_last_error()
    assert conv(b=0) == 0  # an empty batch: nothing to do
    assert lib.nrhip_maxpool2_fwd(ONE, ONE, I64(1), I32(4), I32(4), I32(12), None) == INVALID_ARG
    assert b"multiple of 8" in lib.nrhip_last_error()
    assert lib.nrhip_maxpool2_bwd(ONE, None, None, None, ONE, I64(1), I32(4), I32(4), I32(64), None) == INVALID_ARG
    assert lib.nrhip_l1_feature_fwd(ONE, ONE, I64(0), ctypes.c_float(1), None, ONE, I64(8), ONE, None) == INVALID_ARG
    assert lib.nrhip_l1_feature_fwd(ONE, ONE, I64(5000), ctypes.c_float(1), None, ONE, I64(16), ONE, None) == INVALID_ARG
    assert b"workspace" in lib.nrhip_last_error()
    assert lib.nrhip_l1_feature_workspace(I64(5000), ctypes.byref(need)) == 0 and need.value == 3 * 8
    assert lib.nrhip_l1_feature_bwd(ONE, ONE, I64(8), ctypes.c_float(1), ONE, I32(0), ONE, None, ONE, ONE, None) == INVALID_ARG
    assert b"state" in lib.nrhip_last_error()
    assert lib.nrhip_vgg_stage_images(None, None, I64(4), ONE, None) == INVALID_ARG
    assert lib.nrhip_vgg_image_grad(ONE, None, I64(4), ONE, None) == INVALID_ARG


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from neurad_studio_amd import _lib, ops_vgg

    with pytest.raises(_lib.NeuradHipError):
        ops_vgg.conv3x3_pack(torch.zeros(64, 64, 3, 3))
    with pytest.raises(ValueError):
        ops_vgg.conv3x3(torch.zeros((1, 4, 4, 64), dtype=torch.float16), torch.zeros(8, dtype=torch.float16), 64, 64)
    with pytest.raises(ValueError):
        ops_vgg.maxpool2_fwd(torch.zeros((1, 4, 4, 64), dtype=torch.float16))
    with pytest.raises(_lib.NeuradHipError):
        ops_vgg.stage_images(torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, 3))
    assert ops_vgg.conv3x3_plan(108, 512, 512) == (1, 2, 32)


# ---- the module -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def module():
    from neurad_studio_amd.model_components.perceptual import VGGPerceptualLoss

    m = VGGPerceptualLoss()
    m.load_state_dict(R.make_weights(0))
    return m


def test_state_dict_has_the_reference_names(module):
    keys = list(module.state_dict())
    assert keys == R.state_dict_keys() == list(R.ReferenceStyleLoss().state_dict())
    assert len(keys) == 26 and keys[0] == "vgg.slice1.0.0.weight" and keys[-1] == "vgg.slice5.0.28.bias"
    params = list(module.parameters())
    assert len(params) == 26 and sum(p.numel() for p in params) == 12944960 and not any(p.requires_grad for p in params)
    assert module.weights == [1 / 32, 1 / 16, 1 / 8, 1 / 4, 1.0]
    assert [s[:3] for s in module.steps() if s[0] != "conv"] == [s[:3] for s in R.steps() if s[0] != "conv"]
    assert [(s[1], s[2], s[3].in_channels, s[3].out_channels) for s in module.steps() if s[0] == "conv"] == \
        [s[1:] for s in R.steps() if s[0] == "conv"]


def test_from_reference_shares_storage_and_checkpoints_interchange(module):
    from neurad_studio_amd.model_components.perceptual import VGGPerceptualLoss

    ref = R.ReferenceStyleLoss(weights=[1, 2, 3, 4, 5])
    ours = VGGPerceptualLoss.from_reference(ref)
    assert ours.weights == [1.0, 2.0, 3.0, 4.0, 5.0]
    a, b = ref.state_dict(), ours.state_dict()
    assert list(a) == list(b) and all(a[k].data_ptr() == b[k].data_ptr() for k in a)
    ref.load_state_dict(module.state_dict())  # our checkpoint into the reference-style tree ...
    ours2 = VGGPerceptualLoss()
    ours2.load_state_dict(ref.state_dict())   # ... and back
    assert all(torch.equal(ours2.state_dict()[k], module.state_dict()[k]) for k in a)
    key = ours.cache_key()
    dict(ours.named_parameters())["vgg.slice4.0.12.weight"].mul_(1.0)  # an in-place edit moves the cache key
    assert ours.cache_key() != key
    with pytest.raises(ValueError):
        VGGPerceptualLoss(weights=[1, 2, 3])


def test_cpu_path_equals_the_restated_torch_network(module):
    ref = R.ReferenceStyleLoss()
    ref.load_state_dict(module.state_dict())
    x, y = R.make_images(2, 16, 16)
    x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y1 = y.clone().requires_grad_(True)
    l1, l2 = module(x1, y1), ref(x2, y)
    assert torch.equal(l1, l2) and float(l1.detach()) > 0
    l1.backward(), l2.backward()
    assert torch.equal(x1.grad, x2.grad) and float(x1.grad.abs().max()) > 0
    assert y1.grad is None or not y1.grad.any()  # (the reference's cat hands the target half zeros)
    for bad in ((2, 15, 16, 3), (2, 16, 8, 3), (2, 16, 16, 4)):
        with pytest.raises(ValueError):
            module(torch.zeros(bad), torch.zeros(bad))
    with pytest.raises(ValueError):
        module(torch.zeros(2, 16, 16, 3), torch.zeros(1, 16, 16, 3))


# ---- the restatements against torch's own kernels ---------------------------------------------------------------------------
def test_pool_restatement_is_torchs_max_pool_with_the_first_maximum():
    g = torch.Generator().manual_seed(3)
    for shape in ((2, 16, 16, 8), (1, 17, 19, 8), (1, 2, 2, 8)):
        x = torch.randint(0, 3, shape, generator=g).double().requires_grad_(True)  # few values: ties everywhere
        out = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 2, 2)
        go = torch.randn(out.shape, generator=g, dtype=torch.float64)
        out.backward(go)
        assert torch.equal(R.pool_fwd(x.detach()), R.nhwc(out.detach()))
        assert torch.equal(R.pool_bwd(x.detach(), R.nhwc(go)), x.grad)


def test_backward_restatement_is_the_float64_networks_gradient(module):
    """on float64 activations of its own the linearised chain IS autograd's gradient; rounding the inter-layer gradients to
    fp16 at their working scales moves it by a few 1e-4"""
    net = R.ReferenceStyleLoss()
    net.load_state_dict(module.state_dict())
    net = net.double()
    x, y = R.make_images(1, 16, 16, seed=5)
    xd = x.double().requires_grad_(True)
    saved, cur = {}, torch.cat([R.nchw(xd), R.nchw(y.double())], dim=0)
    weights = module.state_dict()
    loss = 0
    for st in R.steps():
        if st[0] == "conv":
            w, b = weights[R.key_of(st[2], "weight")].double(), weights[R.key_of(st[2], "bias")].double()
            cur = torch.nn.functional.conv2d(cur, w, b, padding=1).clamp_min(0)
            saved[st[2]] = R.nhwc(cur.detach())
        elif st[0] == "pool":
            cur = torch.nn.functional.max_pool2d(cur, 2, 2)
            saved[st[2]] = R.nhwc(cur.detach())
        else:
            loss = loss + R.TAP_WEIGHTS[st[2]] * (cur[:1] - cur[1:].detach()).abs().mean()
    loss.backward()
    assert abs(R.loss_ref(saved, 1) - float(loss)) <= 1e-12 * float(loss)
    a = R.backward_ref(saved, weights, 1)
    assert R.rel_l2(a, xd.grad) < 1e-12
    b = R.backward_ref(saved, weights, 1, rounded=True)
    assert 1e-5 < R.rel_l2(b, a) < 2e-3
    for k in (2.0 ** 16, 2.0 ** -16):  # the working scale carries any power of two exactly
        assert torch.equal(R.backward_ref(saved, weights, 1, g=k, rounded=True), b * k)


def test_integer_operands_are_exact_by_construction():
    for cin, cout in R.CHANNEL_PAIRS:
        c = R.conv_case(3, 6, 6, cin, cout, seed=cin + cout)
        assert c["x"].shape == (3, 6, 6, R.stored(cin)) and c["out"].shape == (3, 6, 6, cout)
        for k in ("x", "g", "out", "gx"):
            assert torch.equal(c[k].double(), c[k].double().round()) and float(c[k].abs().max()) <= 2048
        assert float(c["out"].abs().max()) > 0 and float(c["gx"].abs().max()) > 0
        if cin == 3:
            assert not c["x"][..., 3:].any() and not c["gx"][..., 3:].any()


# ---- the plugin -----------------------------------------------------------------------------------------------------------
def _plugin_model(ref_neurad, monkeypatch, flag):
    """the plugin's model on the CPU with the restated torch network standing in for the reference's module (whose
    constructor downloads torchvision's weights)"""
    from copy import deepcopy

    import plugin_harness as t
    from nerfstudio.data.scene_box import SceneBox

    monkeypatch.setattr(ref_neurad, "VGGPerceptualLossPix2Pix", R.ReferenceStyleLoss)
    mcfg = t.shrink(deepcopy(t.methods()["neurad-hip"].pipeline.model))
    assert mcfg.fused_vgg_loss is False  # the default
    mcfg.fused_vgg_loss = flag
    return mcfg.setup(scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])), num_train_data=2,
                      metadata={"duration": 5.0, "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"}, "trajectories": []})


@pytest.mark.skipif(not ref_import.reference_available(), reason="no reference tree")
def test_plugin_flag_off_leaves_vgg_loss_untouched_and_on_adopts_it(ref, monkeypatch):  # noqa: F811
    from neurad_studio_amd.integration.neurad_hip import NeuRADHipModelConfig
    from neurad_studio_amd.model_components.perceptual import VGGPerceptualLoss

    assert NeuRADHipModelConfig().fused_vgg_loss is False
    off = _plugin_model(ref, monkeypatch, False)
    assert type(off.vgg_loss) is R.ReferenceStyleLoss
    on = _plugin_model(ref, monkeypatch, True)
    assert type(on.vgg_loss) is VGGPerceptualLoss and type(on.vgg_loss.vgg) is R.ReferenceStyleVgg
    names = [k for k in off.state_dict() if k.startswith("vgg_loss.")]
    assert names == ["vgg_loss." + k for k in R.state_dict_keys()] == [k for k in on.state_dict() if k.startswith("vgg_loss.")]
    assert list(off.state_dict()) == list(on.state_dict())
    x, y = R.make_images(1, 16, 16)
    on.vgg_loss.load_state_dict(R.make_weights(0)), off.vgg_loss.load_state_dict(R.make_weights(0))
    assert torch.equal(on.vgg_loss(x, y), off.vgg_loss(x, y))
