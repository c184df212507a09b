"""LPIPS, the part that needs no GPU: the additive C ABI (header, ctypes table, exported symbols), the convolution's plan
query and packed size, host-side argument checks of every entry point, the module's state-dict names, storage sharing of
from_reference on a stand-in built the way the LPIPS packages build their network (tests/lpips_refs.py), the CPU path
against the float64 restatement, the one-transfer triple on its CPU fallback, and the plugin's opt-in flag."""
import ctypes
import os

import pytest
import torch

import lpips_refs as R
import ref_import
from host_gate import header_functions
from plugin_harness import ref  # noqa: F401

I32, I64, F32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
ONE = ctypes.c_void_p(0x1000)  # any non-null, 16-byte aligned address: validation fails before anything is dereferenced
INVALID_ARG, UNSUPPORTED = 1, 2
NEW = ["nrhip_lpips_stage_images", "nrhip_conv2d_plan", "nrhip_conv2d_pack_bytes", "nrhip_conv2d_pack", "nrhip_conv2d",
       "nrhip_maxpool3s2_fwd", "nrhip_lpips_head_workspace", "nrhip_lpips_head"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(ge.LIB):
        ge.build()
    lib = ctypes.CDLL(ge.LIB)
    lib.nrhip_last_error.restype = ctypes.c_char_p
    return lib


def test_new_entry_points_are_declared_bound_and_exported(lib):
    from neurad_studio_amd import _lib, ops_lpips

    declared = header_functions()
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert _lib.LPIPS_IMAGE_CHANNELS == R.IMAGE_CHANNELS == 4 and _lib.LPIPS_MIN_SIZE == R.MIN_SIZE == 31
    assert ops_lpips.CONV_SHAPES == R.CONV_SHAPES and ops_lpips.DEFAULT_EPS == R.EPS


def _plan(lib, m, shape, plan=0):
    mt, nt, waves = I32(-1), I32(-1), I64(-1)
    rc = lib.nrhip_conv2d_plan(I64(m), *(I32(v) for v in shape), I32(plan), ctypes.byref(mt), ctypes.byref(nt), ctypes.byref(waves))
    return rc, (mt.value, nt.value, waves.value), lib.nrhip_last_error()


@pytest.mark.parametrize("layer", range(5))
def test_plan_covers_every_pixel_and_channel(lib, layer):
    """1 pixel, one tile of each size +- 1 pixel, and the layer's output of a 1080 x 1920 pair: waves x tile >= the work,
    with less than one tile to spare along the pixels"""
    shape = R.CONV_SHAPES[layer]
    cout = shape[1]
    h, w = 1080, 1920
    for pool, _, _, ks, stride, pad, _ in R.LAYERS[:layer + 1]:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = R.out_size(h, ks, stride, pad), R.out_size(w, ks, stride, pad)
    for plan in (0, 1, 2):
        for m in (1, 31, 32, 33, 63, 64, 65, 2 * h * w):
            rc, (mt, nt, waves), _ = _plan(lib, m, shape, plan)
            assert rc == 0 and mt in (1, 2) and (plan == 0 or mt == plan) and nt == 2
            cols = cout // (32 * nt)
            assert cols * 32 * nt == cout and waves % cols == 0
            tiles = waves // cols
            assert tiles * 32 * mt >= m > (tiles - 1) * 32 * mt
    assert (h, w) == {0: (269, 479), 1: (134, 239)}.get(layer, (66, 119))
    # the plan's own choice: 64 pixels per wave once that still leaves 2048 waves
    assert _plan(lib, 2 * h * w, shape)[1][0] == (2 if -(-2 * h * w // 64) * (cout // 64) >= 2048 else 1)
    assert _plan(lib, 0, shape)[1] == (1, 2, 0)


def test_pack_bytes_agree_with_the_packer_layout(lib):
    """one 16-byte fragment per (k-step, 32-channel block, lane); k-steps: conv1 11 rows x 3 (12 taps x 4 stored channels per
    row: 528 reduction indices, 363 of them real), the others k * k * cin / 16"""
    need = I64(0)
    for cin, cout, ks, _, _ in R.CONV_SHAPES:
        steps = 33 if cin == 3 else ks * ks * cin // 16
        assert lib.nrhip_conv2d_pack_bytes(I32(cout), I32(cin), I32(ks), ctypes.byref(need)) == 0
        assert need.value == steps * (cout // 32) * 64 * 16
        if cin != 3:
            assert need.value == cout * cin * ks * ks * 2  # no padding anywhere
    assert lib.nrhip_conv2d_pack_bytes(I32(64), I32(3), I32(11), ctypes.byref(need)) == 0 and need.value == 528 * 64 * 2


def test_bad_arguments_give_a_code_and_a_message(lib):
    rc, _, msg = _plan(lib, 100, (64, 64, 3, 1, 1))
    assert rc == UNSUPPORTED and b"64 -> 64" in msg
    rc, _, msg = _plan(lib, 100, (3, 64, 11, 2, 2))  # the right channels, the wrong stride
    assert rc == UNSUPPORTED and b"stride 2" in msg
    rc, _, msg = _plan(lib, 100, R.CONV_SHAPES[1], plan=3)
    assert rc == INVALID_ARG and b"plan 3" in msg
    assert _plan(lib, -1, R.CONV_SHAPES[1])[0] == INVALID_ARG and _plan(lib, 1 << 31, R.CONV_SHAPES[1])[0] == UNSUPPORTED
    assert lib.nrhip_conv2d_plan(I64(1), *(I32(v) for v in R.CONV_SHAPES[0]), I32(0), None, None, None) == INVALID_ARG
    need = I64(0)
    assert lib.nrhip_conv2d_pack_bytes(I32(64), I32(3), I32(11), None) == INVALID_ARG
    assert lib.nrhip_conv2d_pack_bytes(I32(192), I32(3), I32(11), ctypes.byref(need)) == UNSUPPORTED  # channel mismatch
    assert b"[192, 3, 11, 11]" in lib.nrhip_last_error()
    assert lib.nrhip_conv2d_pack(None, I32(64), I32(3), I32(11), ONE, None) == INVALID_ARG and b"NULL" in lib.nrhip_last_error()
    assert lib.nrhip_conv2d_pack(ONE, I32(64), I32(3), I32(11), ctypes.c_void_p(0x1008), None) == INVALID_ARG
    assert lib.nrhip_conv2d_pack(ONE, I32(64), I32(64), I32(3), ONE, None) == UNSUPPORTED

    def conv(shape=R.CONV_SHAPES[0], x=ONE, b=1, h=31, w=31, plan=0):
        return lib.nrhip_conv2d(x, ONE, None, ONE, I32(b), I32(h), I32(w), *(I32(v) for v in shape), I32(1), I32(plan), None)

    assert conv(h=30) == INVALID_ARG and b"smaller than 31 x 31" in lib.nrhip_last_error()
    assert conv(w=30) == INVALID_ARG
    assert conv(x=None) == INVALID_ARG and b"NULL" in lib.nrhip_last_error()
    assert conv(x=ctypes.c_void_p(0x1004)) == INVALID_ARG and b"misaligned" in lib.nrhip_last_error()
    assert conv(shape=R.CONV_SHAPES[2], x=ctypes.c_void_p(0x1008), h=4, w=4) == INVALID_ARG
    assert conv(shape=(3, 64, 11, 4, 3)) == UNSUPPORTED and b"pad 3" in lib.nrhip_last_error()
    assert conv(shape=(192, 256, 3, 1, 1), h=4, w=4) == UNSUPPORTED  # channel mismatch between two real layers
    assert conv(h=0) == INVALID_ARG and conv(plan=5) == INVALID_ARG
    assert conv(b=0) == 0  # an empty batch: nothing to do
    pool = lambda x=ONE, h=3, w=3, c=64: lib.nrhip_maxpool3s2_fwd(x, ONE, I64(1), I32(h), I32(w), I32(c), None)  # noqa: E731
    assert pool(h=2) == INVALID_ARG and b"at least 3 x 3" in lib.nrhip_last_error()
    assert pool(c=12) == INVALID_ARG and pool(x=None) == INVALID_ARG and pool(x=ctypes.c_void_p(0x1002)) == INVALID_ARG
    stage = lambda a=ONE, flag=ONE, n=4: lib.nrhip_lpips_stage_images(a, ONE, I64(n), ONE, ONE, ONE, flag, None)  # noqa: E731
    assert stage(a=None) == INVALID_ARG and stage(flag=None) == INVALID_ARG and stage(n=-1) == INVALID_ARG and stage(n=0) == 0

    def head(feat=ONE, b=1, n=10, c=64, eps=1e-8, mode=0, ws=ONE, ws_bytes=8):
        return lib.nrhip_lpips_head(feat, ONE, I64(b), I64(n), I32(c), F32(eps), I32(mode), I32(0), ws, I64(ws_bytes), ONE, None)

    assert head(feat=None) == INVALID_ARG and b"NULL" in lib.nrhip_last_error()
    assert head(c=60) == INVALID_ARG and b"60 channels" in lib.nrhip_last_error()
    assert head(mode=2) == INVALID_ARG and b"eps_mode 2" in lib.nrhip_last_error()
    assert head(eps=-1.0) == INVALID_ARG and head(eps=float("nan")) == INVALID_ARG
    assert head(b=0) == INVALID_ARG and head(n=0) == INVALID_ARG
    assert head(n=33, ws_bytes=8) == INVALID_ARG and b"workspace" in lib.nrhip_last_error()
    assert head(ws=None) == INVALID_ARG
    assert lib.nrhip_lpips_head_workspace(I64(3), I64(257), ctypes.byref(need)) == 0 and need.value == 3 * 9 * 8
    assert lib.nrhip_lpips_head_workspace(I64(3), I64(257), None) == INVALID_ARG


def test_wrappers_name_the_argument_they_refuse():
    from neurad_studio_amd import ops_lpips as L

    h16 = lambda *s: torch.zeros(s, dtype=torch.float16)  # noqa: E731
    with pytest.raises(ValueError, match="weight"):
        L.conv2d_pack(torch.zeros(64, 3, 11, 11))  # a CPU tensor
    with pytest.raises(ValueError, match="x:"):
        L.conv2d(h16(1, 31, 31, 4), h16(8), R.CONV_SHAPES[0])
    with pytest.raises(ValueError, match="unsupported"):
        L.conv2d(h16(1, 31, 31, 4), h16(8), (3, 64, 11, 4, 1))
    with pytest.raises(ValueError, match="x:"):
        L.maxpool3s2_fwd(h16(1, 4, 4, 64))
    with pytest.raises(ValueError, match="a:"):
        L.stage_images(torch.zeros(1, 31, 31, 3), torch.zeros(1, 31, 31, 3), torch.zeros(3), torch.ones(3))
    with pytest.raises(ValueError, match="feat"):
        L.lpips_head(h16(2, 1, 4, 64), torch.ones(64))
    assert L.conv2d_plan(147, R.CONV_SHAPES[0]) == (1, 2, 5) and L.conv2d_plan(147, R.CONV_SHAPES[2], 2) == (2, 2, 3 * 6)
    with pytest.raises(Exception, match="unsupported"):
        L.conv2d_plan(10, (3, 64, 11, 4, 1))


# ---- the module -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    return R.make_weights(0)


@pytest.fixture(scope="module")
def module(weights):
    from neurad_studio_amd.model_components.lpips import LPIPS

    m = LPIPS()
    m.load_state_dict(weights, strict=True)
    return m


def test_state_dict_keys_are_exactly_the_documented_list(module):
    keys = list(module.state_dict())
    assert keys == R.state_dict_keys() == list(R.ReferenceStyleLPIPS().state_dict())
    assert keys == (["net.scaling_layer.shift", "net.scaling_layer.scale"]
                    + [f"net.net.slice{k}.{i}.{leaf}" for k, i in zip(range(1, 6), (0, 3, 6, 8, 10)) for leaf in ("weight", "bias")]
                    + [f"net.lin{k}.model.1.weight" for k in range(5)])
    assert not any(p.requires_grad for p in module.parameters()) and not module.train().net.training
    steps = module.steps()
    assert [s[0] for s in steps] == ["conv", "tap", "pool", "conv", "tap", "pool", "conv", "tap", "conv", "tap", "conv", "tap"]
    assert [s[4] for s in steps if s[0] == "conv"] == list(R.CONV_SHAPES)
    assert [s[3].in_channels for s in steps if s[0] == "tap"] == list(R.TAP_CHANNELS)


def test_from_reference_shares_storage(module, weights):
    from neurad_studio_amd.model_components.lpips import LPIPS

    standin = R.ReferenceStyleLPIPS()
    ours = LPIPS.from_reference(standin)
    a, b = standin.state_dict(), ours.state_dict()
    assert list(a) == list(b) and all(a[k].data_ptr() == b[k].data_ptr() for k in a)
    assert ours.net is standin.net
    standin.load_state_dict(weights)  # a checkpoint into the reference-style tree is ours at once
    x, y = R.make_pair(1, 35, 47, "noise")
    assert torch.equal(ours(x, y), module(x, y))
    key = ours.cache_key()
    standin.net.lin2.model[1].weight.mul_(1.0)  # an in-place edit moves the cache key
    assert ours.cache_key() != key
    with pytest.raises(ValueError, match="normalize"):
        LPIPS.from_reference(R.ReferenceStyleLPIPS(normalize=False))
    broken = R.ReferenceStyleLPIPS()
    broken.net.net.slice2[1] = torch.nn.Conv2d(64, 192, 3, padding=1)
    with pytest.raises(ValueError, match="not AlexNet"):
        LPIPS.from_reference(broken).steps()


@pytest.mark.parametrize("content", R.CONTENTS)
def test_cpu_path_agrees_with_float64_to_fp32_round_off(module, weights, content):
    """the module's own fp32 nn.Conv2d layers against the float64 restatement; the budget is the restatement's own fp32
    evaluation error (tests/lpips_refs.py:emulation_table measures 2e-7 at most) with room: 2e-6"""
    x, y = R.make_pair(2, 35, 47, content)
    want = R.lpips_pairs_ref(x, y, weights)
    got, flag = module.pairs(x, y)
    assert flag is None and got.dtype == torch.float32 and tuple(got.shape) == (2,)
    assert float((got.double() - want).abs().max()) <= 2e-6
    value = module(x, y)
    assert value.shape == () and abs(float(value) - float(want.mean())) <= 2e-6
    if content == "same":
        assert float(value) == 0.0
    else:
        assert float(want.min()) > R.FLOOR
    hwc = module(x[0].permute(1, 2, 0), y[0].permute(1, 2, 0))  # the [H, W, 3] form
    assert abs(float(hwc) - float(want[0])) <= 2e-6


def test_fp16_operand_emulation_meets_the_condition_on_every_end_to_end_case():
    """the decision behind the kernels' operand format: the staged image, the weights and every stored
    activation rounded to fp16, sums in float64 -- within 5e-4 of float64 on every case of tests/test_gpu_lpips.py, and every
    case but the identical pair above 5e-3, so that the absolute bound says something"""
    rows = R.emulation_table()
    assert len(rows) == len(R.E2E_SIZES) * 2 * len(R.CONTENTS)
    for case, value, emulated, fp32 in rows:
        print("%-22s float64 %.6f  fp16-emulated %.2e  fp32 %.2e" % (case, value, emulated, fp32))
        assert emulated <= R.TOL and fp32 <= emulated, case
        assert value == 0.0 and emulated == 0.0 if case.endswith("same") else value > R.FLOOR, case


def test_both_eps_placements_on_the_cpu(weights):
    from neurad_studio_amd.model_components.lpips import EPS_OUTSIDE, LPIPS

    m = LPIPS(eps_mode=EPS_OUTSIDE)
    m.load_state_dict(weights)
    assert m.eps == 1e-10
    x, y = R.make_pair(1, 31, 31, "noise")
    assert abs(float(m(x, y)) - float(R.lpips_pairs_ref(x, y, weights, eps_mode=R.EPS_OUTSIDE))) <= 2e-6
    with pytest.raises(ValueError):
        LPIPS(eps_mode=2)


def test_refusals(module):
    x, y = R.make_pair(1, 31, 31, "near")
    with pytest.raises(NotImplementedError):
        module(x.clone().requires_grad_(), y)
    for bad in ((1, 3, 30, 31), (1, 3, 31, 30), (1, 4, 31, 31), (31, 31, 4)):
        with pytest.raises(ValueError):
            module(torch.zeros(bad), torch.zeros(bad))
    with pytest.raises(ValueError, match="differ"):
        module(x, y[..., :30])
    for v in (-1e-3, 1 + 1e-3, float("nan"), float("inf")):
        z = y.clone()
        z[0, 0, -1, -1] = v
        with pytest.raises(ValueError, match=r"\[0,1\] range"):
            module(x, z)


def test_triple_on_the_cpu_is_one_transfer_of_four_scalars(module, weights):
    from neurad_studio_amd.model_components import image_metrics as IM

    x, y = R.make_pair(1, 35, 47, "near")
    transfers = []
    to_host = lambda v: (transfers.append(tuple(v.shape)), IM.scalars_to_host(v))[1]  # noqa: E731
    got = IM.image_eval_metrics3(x, y, module, to_host=to_host)
    assert list(got) == ["psnr", "ssim", "lpips"] and all(type(v) is float for v in got.values()) and transfers == [(4,)]
    psnr, ssim = IM.image_metrics_torch(x, y)
    assert got["psnr"] == float(psnr) and got["ssim"] == float(ssim)
    assert abs(got["lpips"] - R.lpips_ref(x, y, weights)) <= 2e-6
    triple = IM.ImageEvalTriple(module, to_host=to_host)
    assert (triple.ssim(x, y), triple.lpips(x, y), triple.psnr(x, y)) == (got["ssim"], got["lpips"], got["psnr"])
    assert transfers == [(4,)] * 2
    assert triple.psnr(y, x) == got["psnr"] and transfers == [(4,)] * 3  # another pair of tensors: another launch
    assert IM.lpips_eval_metric(x, y, module, to_host=to_host) == got["lpips"] and transfers[-1] == (2,)
    # a set flag raises after the read (here a stand-in for the device flag: the CPU path checks at once)
    with pytest.raises(ValueError, match=r"\[0,1\] range"):
        IM.image_eval_metrics3(x, y, module, to_host=lambda v: IM.scalars_to_host(v)[:3] + [1.0])


# ---- the plugin -----------------------------------------------------------------------------------------------------------
H, W = 40, 33


def _plugin_model(ref_neurad, monkeypatch, fused_lpips, fused_image_eval):
    """the plugin's model on the CPU; torchmetrics is a stub in this harness, so the stand-in tree takes the place of the
    reference's LearnedPerceptualImagePatchSimilarity"""
    from copy import deepcopy

    import plugin_harness as t
    from nerfstudio.data.scene_box import SceneBox

    monkeypatch.setattr(ref_neurad, "LearnedPerceptualImagePatchSimilarity", R.ReferenceStyleLPIPS)
    mcfg = t.shrink(deepcopy(t.methods()["neurad-hip"].pipeline.model))
    assert mcfg.fused_lpips is False  # the default
    mcfg.fused_decoder, mcfg.fused_lpips, mcfg.fused_image_eval = False, fused_lpips, fused_image_eval
    m = mcfg.setup(scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])), num_train_data=2,
                   metadata={"duration": 5.0, "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"}, "trajectories": []}).eval()
    return m


def _render():
    x, y = R.make_pair(1, H, W, "near", seed=9)
    return {"rgb": y[0].permute(1, 2, 0).contiguous(), "depth": torch.full((H, 1), 5.0)}, {"image": x[0].permute(1, 2, 0).contiguous()}


@pytest.fixture
def gray_depth(ref, monkeypatch):  # noqa: F811
    from nerfstudio.utils import colormaps

    monkeypatch.setattr(colormaps, "apply_depth_colormap", lambda depth, *a, **k: depth.expand(*depth.shape[:-1], 3) / 100.0)


def _count_transfers(hip, monkeypatch):
    transfers = []
    to_host = type(hip)._scalars_to_host
    monkeypatch.setattr(type(hip), "_scalars_to_host", staticmethod(lambda v: (transfers.append(tuple(v.shape)), to_host(v))[1]))
    return transfers


@pytest.mark.skipif(not ref_import.reference_available(), reason="no reference tree")
def test_plugin_flag_off_calls_the_references_lpips_object(ref, gray_depth, monkeypatch):  # noqa: F811
    from neurad_studio_amd.integration.neurad_hip import NeuRADHipModelConfig

    assert NeuRADHipModelConfig().fused_lpips is False
    hip = _plugin_model(ref, monkeypatch, False, False)
    assert type(hip.lpips) is R.ReferenceStyleLPIPS
    outputs, batch = _render()
    transfers = _count_transfers(hip, monkeypatch)
    calls = []
    hip.__dict__["psnr"] = lambda a, b: torch.tensor(31.0)
    hip.__dict__["ssim"] = lambda a, b: torch.tensor(0.5)
    hip.__dict__["lpips"] = lambda a, b: calls.append((tuple(a.shape), tuple(b.shape))) or torch.tensor(0.25)
    metrics, _ = hip.get_image_metrics_and_images(outputs, dict(batch))
    assert metrics == {"psnr": 31.0, "ssim": 0.5, "lpips": 0.25} and calls == [((1, 3, H, W), (1, 3, H, W))] and transfers == []


@pytest.mark.skipif(not ref_import.reference_available(), reason="no reference tree")
@pytest.mark.parametrize("fused_image_eval", [True, False], ids=["with-image-eval", "alone"])
def test_plugin_flag_on_adopts_the_object_and_answers_lpips(ref, gray_depth, monkeypatch, weights, fused_image_eval):  # noqa: F811
    from neurad_studio_amd.model_components import image_metrics as IM
    from neurad_studio_amd.model_components.lpips import LPIPS

    off = _plugin_model(ref, monkeypatch, False, fused_image_eval)
    hip = _plugin_model(ref, monkeypatch, True, fused_image_eval)
    assert type(hip.lpips) is LPIPS and type(hip.lpips.net).__name__ == "_StandInNet"
    assert list(off.state_dict()) == list(hip.state_dict())  # the state dict stays the reference's
    assert [k for k in hip.state_dict() if k.startswith("lpips.")] == ["lpips." + k for k in R.state_dict_keys()]
    hip.lpips.load_state_dict(weights)
    outputs, batch = _render()
    transfers = _count_transfers(hip, monkeypatch)
    reference_calls = []
    mocked = lambda name, v: lambda a, b: reference_calls.append(name) or torch.tensor(v)  # noqa: E731
    adopted = hip.lpips
    monkeypatch.setattr(type(adopted), "forward", lambda self, a, b: reference_calls.append("lpips.forward") or torch.tensor(0.0))
    if not fused_image_eval:
        hip.__dict__["psnr"], hip.__dict__["ssim"] = mocked("psnr", 31.0), mocked("ssim", 0.5)
    before = (dict(hip._modules), set(hip.__dict__))
    metrics, images = hip.get_image_metrics_and_images(outputs, dict(batch))
    assert list(metrics) == ["psnr", "ssim", "lpips"] and all(type(v) is float for v in metrics.values())
    image, rgb = batch["image"].permute(2, 0, 1)[None], outputs["rgb"].permute(2, 0, 1)[None]
    assert abs(metrics["lpips"] - R.lpips_ref(image, rgb, weights)) <= 2e-6 and metrics["lpips"] > R.FLOOR
    if fused_image_eval:  # the three from ONE transfer (with the range flag); no object of the reference's is called
        assert transfers == [(4,)] and reference_calls == []
        psnr, ssim = IM.image_metrics_torch(image, rgb)
        assert (metrics["psnr"], metrics["ssim"]) == (float(psnr), float(ssim))
    else:  # only lpips is replaced: its value and flag in one transfer
        assert transfers == [(2,)] and reference_calls == ["psnr", "ssim"]
        assert (metrics["psnr"], metrics["ssim"]) == (31.0, 0.5)
    assert (dict(hip._modules), set(hip.__dict__)) == before and hip.lpips is adopted
    assert list(images) == ["img", "depth"]
    bad = dict(batch)
    bad["image"] = batch["image"].clone()
    bad["image"][-1, -1, 0] = 1.5
    with pytest.raises(ValueError, match=r"\[0,1\] range"):
        hip.get_image_metrics_and_images(outputs, bad)
    assert (dict(hip._modules), set(hip.__dict__)) == before
