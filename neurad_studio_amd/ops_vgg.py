"""ctypes wrappers of csrc/vgg_loss.hip: the kernels of the VGG-19 perceptual loss.  Activations and gradients are NHWC fp16
tensors [B, H, W, C]; the 3-channel image side is stored with IMAGE_CHANNELS channels (the rest zero); no CPU path.

A fp16 gradient tensor travels with a device ``state`` [2] fp32 = {amax, S}: stored = S * true, S a power of two (see
include/neurad_hip.h).  ``new_states(n)`` hands out zeroed states; a state is written by exactly one producer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
from torch import Tensor

from ._lib import L1_ITEMS, VGG_IMAGE_CHANNELS as IMAGE_CHANNELS, call
from .ops import _chk, launch

CHANNELS = (3, 64, 128, 256, 512)


def _stored(c: int) -> int:
    return IMAGE_CHANNELS if c == 3 else c


def _act16(t: Tensor, name: str, channels: Optional[int] = None) -> Tensor:
    if not isinstance(t, Tensor) or not t.is_cuda or t.dtype != torch.float16 or not t.is_contiguous() or t.dim() != 4:
        raise ValueError(f"{name}: expected a contiguous cuda fp16 [B, H, W, C] tensor, got "
                         f"{tuple(t.shape) if isinstance(t, Tensor) else type(t)} {getattr(t, 'dtype', '')} on "
                         f"{getattr(t, 'device', '?')}")
    if channels is not None and t.shape[-1] != channels:
        raise ValueError(f"{name}: {t.shape[-1]} channels stored, expected {channels}")
    return t


def _state(t: Optional[Tensor], name: str) -> Optional[Tensor]:
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.float32 or t.numel() != 2 or not t.is_contiguous():
        raise ValueError(f"{name}: a scale state is a contiguous cuda fp32 [2] tensor")
    return t


def new_states(n: int, device) -> Tensor:
    """[n, 2] zeroed {amax, S} states"""
    return torch.zeros((n, 2), device=device, dtype=torch.float32)


def conv3x3_pack(weight: Tensor, mode: int = 0) -> Tensor:
    """torch Conv2d weight [cout, cin, 3, 3] fp32 -> fragment-ordered fp16 weights.  mode 0: forward; 1: input gradient."""
    w = _chk(weight.detach(), "weight")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"conv3x3_pack: weight {tuple(w.shape)}, expected [cout, cin, 3, 3]")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    need = C.c_int64(0)
    call("nrhip_conv3x3_pack_bytes", cout, cin, mode, C.byref(need))
    out = torch.empty((need.value // 2,), device=w.device, dtype=torch.float16)
    launch("nrhip_conv3x3_pack", w, cout, cin, mode, out)
    return out


def conv3x3_plan(n_pixels: int, cin: int, cout: int, plan: int = 0) -> Tuple[int, int, int]:
    """-> (32-pixel blocks per wave, 32-channel blocks per wave, waves): host logic, no GPU"""
    mt, nt, waves = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    call("nrhip_conv3x3_plan", n_pixels, cin, cout, plan, C.byref(mt), C.byref(nt), C.byref(waves))
    return mt.value, nt.value, waves.value


def conv3x3(x: Tensor, wfrag: Tensor, cin: int, cout: int, bias: Optional[Tensor] = None, relu: bool = False,
            mask: Optional[Tensor] = None, in_state: Optional[Tensor] = None, out_state: Optional[Tensor] = None,
            plan: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """x [B,H,W,cin] fp16 -> fp16(conv3x3(x) * p + bias) (ReLU) (zero where mask <= 0) as [B,H,W,cout]; wfrag from
    conv3x3_pack: mode 0 of a [cout, cin] weight, or mode 1 of a [cin, cout] weight (then this is its input gradient)"""
    if cin not in CHANNELS or cout not in CHANNELS or (cin == 3 and cout == 3):
        raise ValueError(f"conv3x3: channels {cin} -> {cout} unsupported")
    _act16(x, "x", _stored(cin))
    b, h, w, _ = x.shape
    need = C.c_int64(0)
    call("nrhip_conv3x3_pack_bytes", cout, cin, 0, C.byref(need))
    if wfrag.dtype != torch.float16 or not wfrag.is_cuda or wfrag.numel() * 2 != need.value or not wfrag.is_contiguous():
        raise ValueError(f"conv3x3: wfrag is not a packed {cin} -> {cout} weight")
    if out is None:
        out = torch.empty((b, h, w, _stored(cout)), device=x.device, dtype=torch.float16)
    _act16(out, "out", _stored(cout))
    if tuple(out.shape[:3]) != (b, h, w):
        raise ValueError("conv3x3: out differs from x in shape")
    if mask is not None:
        _act16(mask, "mask", _stored(cout))
        if mask.shape != out.shape:
            raise ValueError("conv3x3: mask differs from the output in shape")
    bias_f = None if bias is None else _chk(bias.detach(), "bias")
    if bias_f is not None and bias_f.numel() != cout:
        raise ValueError("conv3x3: bias has the wrong length")
    launch("nrhip_conv3x3", x, wfrag, bias_f, mask, _state(in_state, "in_state"), _state(out_state, "out_state"), out, b, h,
           w, cin, cout, int(relu), plan)
    return out


def maxpool2_fwd(x: Tensor) -> Tensor:
    _act16(x, "x")
    b, h, w, c = x.shape
    if c % 8:
        raise ValueError("maxpool2_fwd: channels must be a multiple of 8")
    out = torch.empty((b, h // 2, w // 2, c), device=x.device, dtype=torch.float16)
    launch("nrhip_maxpool2_fwd", x, out, b, h, w, c)
    return out


def maxpool2_bwd(x: Tensor, grad_out: Tensor, in_state: Optional[Tensor] = None,
                 out_state: Optional[Tensor] = None) -> Tensor:
    """gradient of maxpool2_fwd(x) w.r.t. x (all of it written), times the power of two that normalises in_state"""
    _act16(x, "x"), _act16(grad_out, "grad_out")
    b, h, w, c = x.shape
    if c % 8 or tuple(grad_out.shape) != (b, h // 2, w // 2, c):
        raise ValueError("maxpool2_bwd: grad_out must be [B, H // 2, W // 2, C], C a multiple of 8")
    gin = torch.empty_like(x)
    launch("nrhip_maxpool2_bwd", x, grad_out, _state(in_state, "in_state"), _state(out_state, "out_state"), gin, b, h, w, c)
    return gin


def _pair16(fx: Tensor, fy: Tensor, who: str) -> int:
    for t, n in ((fx, "fx"), (fy, "fy")):
        if not isinstance(t, Tensor) or not t.is_cuda or t.dtype != torch.float16 or not t.is_contiguous():
            raise ValueError(f"{who}: {n} must be a contiguous cuda fp16 tensor")
    if fx.shape != fy.shape or fx.numel() == 0:
        raise ValueError(f"{who}: fx and fy must have the same, non-empty shape")
    return fx.numel()


def l1_feature_fwd(fx: Tensor, fy: Tensor, weight: float = 1.0, accum: Optional[Tensor] = None,
                   out: Optional[Tensor] = None) -> Tensor:
    """-> [1] fp32 = (accum or 0) + weight * mean |fx - fy| (float64 partials in a fixed order, one rounding)"""
    n = _pair16(fx, fy, "l1_feature_fwd")
    parts = (n + L1_ITEMS - 1) // L1_ITEMS
    ws = torch.empty((parts,), device=fx.device, dtype=torch.float64)
    if out is None:
        out = torch.empty((1,), device=fx.device, dtype=torch.float32)
    launch("nrhip_l1_feature_fwd", fx, fy, n, float(weight), None if accum is None else _chk(accum, "accum"), ws, parts * 8,
           _chk(out, "out"))
    return out


def l1_feature_bwd(fx: Tensor, fy: Tensor, weight: float, grad_loss: Tensor, out_state: Tensor, mask_fx: bool = False,
                   above: Optional[Tensor] = None, above_state: Optional[Tensor] = None) -> Tensor:
    """-> fp16 S * (weight * grad_loss / numel * sign(fx - fy) (* [fx > 0]) + above / S_above), S into out_state"""
    n = _pair16(fx, fy, "l1_feature_bwd")
    g = _chk(grad_loss.reshape(-1), "grad_loss")
    if g.numel() != 1:
        raise ValueError("l1_feature_bwd: grad_loss is a scalar")
    if (above is None) != (above_state is None):
        raise ValueError("l1_feature_bwd: above and above_state go together")
    if above is not None:
        _pair16(fx, above, "l1_feature_bwd")
    out = torch.empty_like(fx)
    launch("nrhip_l1_feature_bwd", fx, fy, n, float(weight), g, int(mask_fx), above, _state(above_state, "above_state"),
           _state(out_state, "out_state"), out)
    return out


def stage_images(x: Tensor, y: Tensor) -> Tensor:
    """two fp32 NHWC [B, H, W, 3] images -> cat([x, y]) as fp16 [2 B, H, W, IMAGE_CHANNELS]"""
    x, y = _chk(x, "x"), _chk(y, "y")
    if x.dim() != 4 or x.shape[-1] != 3 or x.shape != y.shape:
        raise ValueError(f"stage_images: expected two [B, H, W, 3] images, got {tuple(x.shape)} and {tuple(y.shape)}")
    b, h, w, _ = x.shape
    out = torch.empty((2 * b, h, w, IMAGE_CHANNELS), device=x.device, dtype=torch.float16)
    launch("nrhip_vgg_stage_images", x, y, b * h * w, out)
    return out


def image_grad(grad16: Tensor, state: Tensor) -> Tensor:
    """fp16 [B, H, W, IMAGE_CHANNELS] at its working scale -> the fp32 [B, H, W, 3] gradient"""
    _act16(grad16, "grad16", IMAGE_CHANNELS)
    b, h, w, _ = grad16.shape
    out = torch.empty((b, h, w, 3), device=grad16.device, dtype=torch.float32)
    launch("nrhip_vgg_image_grad", grad16, _state(state, "state"), b * h * w, out)
    return out
