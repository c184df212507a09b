"""VGG-19 perceptual loss (model_components/losses.py:582-625 of the reference; LossSettings.vgg_mult, models/neurad.py:69,
260,537-538): VGG-19 up to relu5_1 on cat([rgb, image]), five L1 terms on the relu{1..5}_1 features, a gradient into the
rendered half only.

On a GPU the whole term is ONE autograd node on csrc/vgg_loss.hip (ops_vgg.py): a staging kernel, 13 convolutions on the
fp16 matrix cores (fp32 accumulation -- the arithmetic of the reference's mixed-precision trainer), 4 pools and 5 loss
kernels forward; the backward walks the rendered half with a power-of-two working scale per gradient tensor and never reads
the device.  On any other device the same module runs its own ``nn.Conv2d`` layers: there is no second implementation.

The parameter names are the reference module's (``vgg.slice{1..5}.0.{i}.{weight,bias}``, i = torchvision's index in
``vgg19().features``), so checkpoints interchange."""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn
from torch.amp import custom_bwd, custom_fwd

# torchvision's configuration "E" up to relu5_1, cut where the reference cuts it: features[:2], [2:7], [7:12], [12:21], [21:30]
_LAYOUT = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512)
_CUTS = ((0, 2), (2, 7), (7, 12), (12, 21), (21, 30))
DEFAULT_TAP_WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
MIN_SIZE = 16  # four 2 x 2 pools leave at least one pixel


def _feature_layers() -> List[nn.Module]:
    layers: List[nn.Module] = []
    cin = 3
    for v in _LAYOUT:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, int(v), kernel_size=3, padding=1), nn.ReLU(inplace=False)]
            cin = int(v)
    return layers


class Vgg19Slices(nn.Module):
    """the five feature slices, with the keys a sliced torchvision ``features`` keeps (its own indices) one level down"""

    def __init__(self):
        super().__init__()
        layers = _feature_layers()
        for k, (a, b) in enumerate(_CUTS):
            inner = nn.Sequential(OrderedDict((str(i), layers[i]) for i in range(a, b)))
            setattr(self, f"slice{k + 1}", nn.Sequential(inner))

    def forward(self, x: Tensor) -> List[Tensor]:
        out = []
        for k in range(5):
            x = getattr(self, f"slice{k + 1}")(x)
            out.append(x)
        return out


def _program(vgg: nn.Module):
    """the network as a list of steps over named tensors: ("conv", src, dst, Conv2d) | ("pool", src, dst) | ("tap", src, i);
    read off the module tree, so an adopted reference tree and our own give the same program"""
    steps, cur = [], "image"
    n_conv = n_pool = 0
    block, within = 1, 0
    for k in range(5):
        sl = getattr(vgg, f"slice{k + 1}")
        mods = list(sl.modules())[1:]
        for m in mods:
            if isinstance(m, nn.Sequential) or isinstance(m, nn.ReLU):
                continue
            if isinstance(m, nn.Conv2d):
                if m.kernel_size != (3, 3) or m.padding != (1, 1) or m.stride != (1, 1) or m.bias is None:
                    raise ValueError("VGGPerceptualLoss: expected 3x3 / stride 1 / pad 1 convolutions with a bias")
                within += 1
                dst = f"conv{block}_{within}"
                steps.append(("conv", cur, dst, m))
                cur, n_conv = dst, n_conv + 1
            elif isinstance(m, nn.MaxPool2d):
                dst = f"pool{block}"
                steps.append(("pool", cur, dst))
                cur, n_pool, block, within = dst, n_pool + 1, block + 1, 0
            else:
                raise ValueError(f"VGGPerceptualLoss: unexpected layer {type(m).__name__}")
        steps.append(("tap", cur, k))
    if n_conv != 13 or n_pool != 4:
        raise ValueError(f"VGGPerceptualLoss: {n_conv} convolutions and {n_pool} pools, expected 13 and 4")
    return steps


class _Packs:
    """fragment-ordered weights of both directions; rebuilt by VGGPerceptualLoss when a weight's storage or version moves"""

    def __init__(self, steps):
        from neurad_studio_amd import ops_vgg

        self.steps = []
        for st in steps:
            if st[0] != "conv":
                self.steps.append(st)
                continue
            _, src, dst, m = st
            w = m.weight.detach()
            w = w if w.dtype == torch.float32 else w.float()
            b = m.bias.detach()
            b = b if b.dtype == torch.float32 else b.float()
            self.steps.append(("conv", src, dst, ops_vgg.conv3x3_pack(w, 0), ops_vgg.conv3x3_pack(w, 1), b.contiguous(),
                               int(w.shape[1]), int(w.shape[0])))


def _check_images(x: Tensor, y: Tensor) -> None:
    if x.dim() != 4 or x.shape[-1] != 3 or x.shape != y.shape or x.shape[0] < 1:
        raise ValueError(f"VGGPerceptualLoss: expected two NHWC [B, H, W, 3] images, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[1] < MIN_SIZE or x.shape[2] < MIN_SIZE:
        raise ValueError(f"VGGPerceptualLoss: images of {x.shape[1]} x {x.shape[2]} are smaller than {MIN_SIZE} x {MIN_SIZE}")


class VGGPerceptualLossFn(torch.autograd.Function):
    """loss [] fp32 = sum_i w_i * mean |relu{i}_1(x) - relu{i}_1(y)|.  ``sink`` (a dict or None) receives what the node keeps
    for its backward -- name -> fp16 NHWC tensor of the WHOLE batch cat([x, y]) -- and stays empty when x needs no gradient."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, y, packs, tap_weights, sink):
        from neurad_studio_amd import ops_vgg

        _check_images(x, y)
        keep = ctx.needs_input_grad[0]
        b = x.shape[0]
        t = {"image": ops_vgg.stage_images(x.detach(), y.detach())}
        loss = None
        for st in packs.steps:
            if st[0] == "conv":
                _, src, dst, wf, _, bias, cin, cout = st
                t[dst] = ops_vgg.conv3x3(t[src], wf, cin, cout, bias=bias, relu=True)
            elif st[0] == "pool":
                t[st[2]] = ops_vgg.maxpool2_fwd(t[st[1]])
            else:
                f = t[st[1]]
                loss = ops_vgg.l1_feature_fwd(f[:b], f[b:], tap_weights[st[2]], accum=loss)
            if not keep and st[0] != "tap" and st[1] in t:
                del t[st[1]]  # nothing is kept: an input is dead once its only consumer has run (a tap reads the same tensor
                #               as the layer after it, which drops it)
        ctx.packs, ctx.tap_weights, ctx.batch = packs, tuple(tap_weights), b
        ctx.names = []
        if keep:
            ctx.names = [n for n in t if n != "image"]
            ctx.save_for_backward(*[t[n] for n in ctx.names])
            if sink is not None:
                sink.update(t)
        return loss.reshape(())

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_loss):
        from neurad_studio_amd import ops_vgg

        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        t = dict(zip(ctx.names, ctx.saved_tensors))
        b = ctx.batch
        g = grad_loss.detach().float().reshape(1)
        states = ops_vgg.new_states(len(ctx.packs.steps) + 1, g.device)
        grads, gstate, n_state = {}, {}, 0
        for st in reversed(ctx.packs.steps):
            s_out = states[n_state]
            n_state += 1
            if st[0] == "tap":
                f = t[st[1]]
                grads[st[1]] = ops_vgg.l1_feature_bwd(f[:b], f[b:], ctx.tap_weights[st[2]], g, s_out, mask_fx=True,
                                                      above=grads.pop(st[1], None), above_state=gstate.pop(st[1], None))
                gstate[st[1]] = s_out
            elif st[0] == "conv":
                _, src, dst, _, wb, _, cin, cout = st
                mask = None if src == "image" else t[src][:b]
                grads[src] = ops_vgg.conv3x3(grads.pop(dst), wb, cout, cin, mask=mask, in_state=gstate.pop(dst),
                                             out_state=s_out)
                gstate[src] = s_out
            else:
                _, src, dst = st
                grads[src] = ops_vgg.maxpool2_bwd(t[src][:b], grads.pop(dst), in_state=gstate.pop(dst), out_state=s_out)
                gstate[src] = s_out
        return ops_vgg.image_grad(grads["image"], gstate["image"]), None, None, None, None


def vgg_perceptual_loss(x: Tensor, y: Tensor, packs: _Packs, tap_weights: Sequence[float] = DEFAULT_TAP_WEIGHTS,
                        return_saved: bool = False):
    """the node on two cuda NHWC images; ``return_saved``: -> (loss, {name: tensor the node kept for its backward})"""
    sink = {} if return_saved else None
    loss = VGGPerceptualLossFn.apply(x, y, packs, tuple(float(w) for w in tap_weights), sink)
    return (loss, sink) if return_saved else loss


class VGGPerceptualLoss(nn.Module):
    """``loss = m(x, y)`` on NHWC [B, H, W, 3] images, as the reference's VGGPerceptualLossPix2Pix; the frozen VGG weights are
    part of the state dict under the reference's names"""

    def __init__(self, weights: Optional[Sequence[float]] = None, vgg: Optional[nn.Module] = None):
        super().__init__()
        self.vgg = (Vgg19Slices() if vgg is None else vgg).eval()
        self.vgg.requires_grad_(False)
        if weights is None:
            weights = DEFAULT_TAP_WEIGHTS
        if len(weights) != 5:
            raise ValueError("VGGPerceptualLoss: expected 5 tap weights")
        self.weights = [float(w) for w in weights]
        self._steps = None
        self._packs: Optional[_Packs] = None
        self._packs_key: Optional[Tuple] = None

    @classmethod
    def from_reference(cls, module: nn.Module) -> "VGGPerceptualLoss":
        """adopt a reference VGGPerceptualLossPix2Pix: its ``vgg`` tree becomes ours, no tensor is copied"""
        return cls(weights=list(module.weights), vgg=module.vgg)

    @classmethod
    def from_torchvision(cls, weights: Optional[Sequence[float]] = None) -> "VGGPerceptualLoss":
        """torchvision's pretrained VGG-19 (only where torchvision is importable)"""
        import torchvision

        feats = torchvision.models.vgg19(weights=torchvision.models.VGG19_Weights.DEFAULT).features
        m = cls(weights=weights)
        own = dict(m.vgg.named_parameters())
        with torch.no_grad():
            for name, p in own.items():  # name = slice{k}.0.{i}.{weight|bias}
                i, leaf = name.split(".")[2:]
                p.copy_(getattr(feats[int(i)], leaf))
        return m

    def steps(self):
        if self._steps is None:
            self._steps = _program(self.vgg)
        return self._steps

    def cache_key(self) -> Tuple:
        return tuple((m.weight.data_ptr(), m.weight._version, m.bias.data_ptr(), m.bias._version, m.weight.dtype)
                     for st in self.steps() if st[0] == "conv" for m in (st[3],))

    def packs(self) -> _Packs:
        key = self.cache_key()
        if self._packs is None or key != self._packs_key:
            self._packs, self._packs_key = _Packs(self.steps()), key
        return self._packs

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        _check_images(x, y)
        if x.is_cuda:
            return vgg_perceptual_loss(x, y, self.packs(), self.weights)
        feats = self.vgg(torch.cat([x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)], dim=0))
        loss = 0
        for w, f in zip(self.weights, feats):
            fx, fy = f.chunk(2, dim=0)
            loss = loss + w * torch.nn.functional.l1_loss(fx, fy.detach())
        return loss
