"""ctypes wrappers of csrc/lpips.hip: the kernels of LPIPS (AlexNet).  Activations are NHWC fp16 tensors [B, H, W, C]; the
3-channel image is stored with IMAGE_CHANNELS channels (the last zero); forward only; no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
from torch import Tensor

from ._lib import (LPIPS_EPS_INSIDE as EPS_INSIDE, LPIPS_EPS_OUTSIDE as EPS_OUTSIDE, LPIPS_IMAGE_CHANNELS as IMAGE_CHANNELS,
                   LPIPS_MIN_SIZE as MIN_SIZE, call)
from .ops import launch
from .ops_vgg import _act16

# (cin, cout, kernel, stride, pad) of AlexNet's five convolutions: the only ones the library has
CONV_SHAPES = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
DEFAULT_EPS = {EPS_INSIDE: 1e-8, EPS_OUTSIDE: 1e-10}


def _chk(t, name: str, dtype=torch.float32) -> Tensor:
    if not isinstance(t, Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous cuda {dtype} tensor, got "
                         f"{tuple(t.shape) if isinstance(t, Tensor) else type(t)} {getattr(t, 'dtype', '')} on "
                         f"{getattr(t, 'device', '?')}")
    return t


def _stored(c: int) -> int:
    return IMAGE_CHANNELS if c == 3 else c


def out_size(n: int, ksize: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - ksize) // stride + 1


def _pack_bytes(cout: int, cin: int, ksize: int) -> int:
    need = C.c_int64(0)
    call("nrhip_conv2d_pack_bytes", cout, cin, ksize, C.byref(need))
    return need.value


def conv2d_pack(weight: Tensor) -> Tensor:
    """torch Conv2d weight [cout, cin, k, k] fp32 of one of CONV_SHAPES -> fragment-ordered fp16 weights"""
    w = _chk(weight.detach(), "weight")
    if w.dim() != 4 or w.shape[2] != w.shape[3]:
        raise ValueError(f"conv2d_pack: weight {tuple(w.shape)}, expected [cout, cin, k, k]")
    cout, cin, ks = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    out = torch.empty((_pack_bytes(cout, cin, ks) // 2,), device=w.device, dtype=torch.float16)
    launch("nrhip_conv2d_pack", w, cout, cin, ks, out)
    return out


def conv2d_plan(n_pixels: int, shape: Tuple[int, int, int, int, int], plan: int = 0) -> Tuple[int, int, int]:
    """-> (32-pixel blocks per wave, 32-channel blocks per wave, waves) over n_pixels OUTPUT pixels: host logic, no GPU"""
    mt, nt, waves = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    call("nrhip_conv2d_plan", n_pixels, *shape, plan, C.byref(mt), C.byref(nt), C.byref(waves))
    return mt.value, nt.value, waves.value


def conv2d(x: Tensor, wfrag: Tensor, shape: Tuple[int, int, int, int, int], bias: Optional[Tensor] = None, relu: bool = True,
           plan: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """x [B,H,W,cin] fp16 -> fp16(conv(x) + bias) (ReLU) as [B,Ho,Wo,cout]; ``shape`` = (cin, cout, kernel, stride, pad), one
    of CONV_SHAPES; wfrag from conv2d_pack"""
    shape = tuple(int(v) for v in shape)
    if shape not in CONV_SHAPES:
        raise ValueError(f"conv2d: shape {shape} unsupported; one of {CONV_SHAPES}")
    cin, cout, ks, stride, pad = shape
    _act16(x, "x", _stored(cin))
    b, h, w, _ = x.shape
    if cin == 3 and (h < MIN_SIZE or w < MIN_SIZE):
        raise ValueError(f"x: an image of {h} x {w} is smaller than {MIN_SIZE} x {MIN_SIZE}")
    if (not isinstance(wfrag, Tensor) or wfrag.dtype != torch.float16 or not wfrag.is_cuda or not wfrag.is_contiguous()
            or wfrag.numel() * 2 != _pack_bytes(cout, cin, ks)):
        raise ValueError(f"wfrag: not a packed {cin} -> {cout}, {ks} x {ks} weight")
    ho, wo = out_size(h, ks, stride, pad), out_size(w, ks, stride, pad)
    if out is None:
        out = torch.empty((b, ho, wo, cout), device=x.device, dtype=torch.float16)
    _act16(out, "out", cout)
    if tuple(out.shape[:3]) != (b, ho, wo):
        raise ValueError(f"out: shape {tuple(out.shape)}, expected {(b, ho, wo, cout)}")
    bias_f = None if bias is None else _chk(bias.detach(), "bias")
    if bias_f is not None and bias_f.numel() != cout:
        raise ValueError(f"bias: {bias_f.numel()} elements, expected {cout}")
    launch("nrhip_conv2d", x, wfrag, bias_f, out, b, h, w, cin, cout, ks, stride, pad, int(relu), plan)
    return out


def maxpool3s2_fwd(x: Tensor) -> Tensor:
    """max_pool2d(3, 2) (floor, no padding) of an NHWC fp16 tensor"""
    _act16(x, "x")
    b, h, w, c = x.shape
    if c % 8 or h < 3 or w < 3:
        raise ValueError(f"x: {tuple(x.shape)}; channels must be a multiple of 8 and the map at least 3 x 3")
    out = torch.empty((b, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c), device=x.device, dtype=torch.float16)
    launch("nrhip_maxpool3s2_fwd", x, out, b, h, w, c)
    return out


def stage_images(a: Tensor, b: Tensor, shift: Tensor, scale: Tensor, flag: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """two fp32 NHWC [B, H, W, 3] images in [0, 1] -> (cat([a, b]) after (2 v - 1 - shift) / scale as fp16
    [2 B, H, W, IMAGE_CHANNELS], flag [1] int32: 1 when a value is outside [0, 1] or not finite -- on the device, not read)"""
    a, b = _chk(a, "a"), _chk(b, "b")
    if a.dim() != 4 or a.shape[-1] != 3 or a.shape != b.shape:
        raise ValueError(f"a, b: expected two [B, H, W, 3] images, got {tuple(a.shape)} and {tuple(b.shape)}")
    shift, scale = _chk(shift.detach().reshape(-1), "shift"), _chk(scale.detach().reshape(-1), "scale")
    if shift.numel() != 3 or scale.numel() != 3:
        raise ValueError("shift, scale: expected 3 values each")
    if flag is None:
        flag = torch.zeros((1,), device=a.device, dtype=torch.int32)
    flag = _chk(flag, "flag", torch.int32)
    if flag.numel() != 1:
        raise ValueError("flag: expected one int32")
    n, h, w, _ = a.shape
    out = torch.empty((2 * n, h, w, IMAGE_CHANNELS), device=a.device, dtype=torch.float16)
    launch("nrhip_lpips_stage_images", a, b, n * h * w, shift, scale, out, flag)
    return out, flag


def lpips_head(feat: Tensor, lin: Tensor, eps_mode: int = EPS_INSIDE, eps: Optional[float] = None,
               out: Optional[Tensor] = None) -> Tensor:
    """feat [2 B, H, W, C] fp16 (the first B images against the second B), lin [C] fp32 -> out [B] fp32 (+)= the pixel mean of
    sum_c lin_c (n(fa)_c - n(fb)_c)^2; an ``out`` that is passed in is accumulated into.  eps_mode EPS_INSIDE: n(f) = f /
    sqrt(eps + sum f^2); EPS_OUTSIDE: f / (sqrt(sum f^2) + eps)."""
    _act16(feat, "feat")
    n2, h, w, c = feat.shape
    if n2 < 2 or n2 % 2 or c % 8 or h * w == 0:
        raise ValueError(f"feat: {tuple(feat.shape)}; expected an even, non-empty batch and channels a multiple of 8")
    if eps_mode not in DEFAULT_EPS:
        raise ValueError(f"eps_mode: {eps_mode} not in {{EPS_INSIDE, EPS_OUTSIDE}}")
    lin = _chk(lin.detach().reshape(-1), "lin")
    if lin.numel() != c:
        raise ValueError(f"lin: {lin.numel()} weights for {c} channels")
    b, accumulate = n2 // 2, out is not None
    if out is None:
        out = torch.empty((b,), device=feat.device, dtype=torch.float32)
    if _chk(out, "out").numel() != b:
        raise ValueError(f"out: expected a contiguous fp32 [{b}] tensor")
    need = C.c_int64(0)
    call("nrhip_lpips_head_workspace", b, h * w, C.byref(need))
    ws = torch.empty((max(need.value // 8, 1),), device=feat.device, dtype=torch.float64)
    launch("nrhip_lpips_head", feat, lin, b, h * w, c, float(DEFAULT_EPS[eps_mode] if eps is None else eps), eps_mode,
           int(accumulate), ws, need.value, out)
    return out
