"""The residual trunk's convolutions on the HIP library (include/dagl_ce.h: dagl_trunk_*, csrc/trunk.hip): opt-in.

``convert(model)`` re-classes every plain ``nn.Conv2d`` of a model -- RR's head, ResBlock, body and tail convolutions and CES's 1x1
stage mixes -- as ``trunk.Conv2d``: same parameters (the very tensors), names and ``state_dict``, whose forward and backward run
on the library's fp32 matrix-core kernels.  A converted ``ResBlock`` (net.py) takes a two-launch fused forward.  Nothing changes
for a model that is not converted: the stock trunk stays the default.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._lib import DaglError

MAX_CHANNELS = 64


def unsupported(conv: nn.Conv2d) -> "str | None":
    """Why the library cannot run ``conv`` (None when it can): stride 1, padding ksize // 2, ksize 1 or 3, dilation 1, groups 1,
    zero padding, 1..64 input and output channels."""
    k = conv.kernel_size
    if k not in ((1, 1), (3, 3)):
        return f"kernel size {k} (1x1 or 3x3 only)"
    if tuple(conv.stride) != (1, 1):
        return f"stride {conv.stride} (1 only)"
    if tuple(conv.dilation) != (1, 1):
        return f"dilation {conv.dilation} (1 only)"
    if conv.padding != (k[0] // 2, k[1] // 2):
        return f"padding {conv.padding} (ksize // 2 only)"
    if conv.groups != 1:
        return f"groups {conv.groups} (1 only)"
    if conv.padding_mode != "zeros":
        return f"padding mode {conv.padding_mode!r} (zeros only)"
    if not (1 <= conv.in_channels <= MAX_CHANNELS and 1 <= conv.out_channels <= MAX_CHANNELS):
        return f"{conv.in_channels} -> {conv.out_channels} channels (1..{MAX_CHANNELS} only)"
    return None


def _check_params(conv: "Conv2d", device):
    for name, p in (("weight", conv.weight), ("bias", conv.bias)):
        if p is not None and (p.dtype != torch.float32 or p.device != device):
            raise DaglError(f"trunk.Conv2d: {name} is {p.dtype} on {p.device}, the input fp32 on {device}")


def _check_call(conv: "Conv2d", x: torch.Tensor):
    """Refuse what the library does not run -- before the library is loaded; there is no silent fall-back to the stock layer."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        what = f"{x.dtype} on {x.device}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise DaglError(f"trunk.Conv2d: input {what}; the library runs fp32 GPU tensors only (no stock fall-back)")
    if x.dim() != 4 or x.shape[1] != conv.in_channels:
        raise DaglError(f"trunk.Conv2d: input {tuple(x.shape)} does not fit {conv.in_channels} input channels")
    _check_params(conv, x.device)


class Conv2d(nn.Conv2d):
    """``nn.Conv2d`` (stride 1, same padding, 1x1 / 3x3, <= 64 channels) whose forward and backward run on the library.  The
    packed weight layouts are cached until the parameter's storage or version changes: an optimizer step, an in-place op on the
    parameter, ``load_state_dict``, ``weight.data = t`` and ``.to(device)`` are all followed.  Writing THROUGH ``weight.data``
    (``weight.data.mul_(2)``, ``.data.copy_(t)``, ``.data.normal_()``, ``.data.clamp_()``) changes neither, so the layer would go
    on convolving with the old weights: call ``invalidate_packed()`` (or ``trunk.invalidate_packed(model)``) after such a write."""

    def _packed(self, transposed: bool) -> torch.Tensor:
        w = self.weight
        key = (w.data_ptr(), w._version, w.device, bool(transposed))
        cache = self.__dict__.setdefault("_trunk_packed", {})
        hit = cache.get(bool(transposed))
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, ops.trunk_pack_weights(w.detach().contiguous(), transposed))
            cache[bool(transposed)] = hit
        return hit[1]

    def invalidate_packed(self):
        self.__dict__.pop("_trunk_packed", None)

    def forward(self, x):
        _check_call(self, x)
        return _ConvFn.apply(x, self.weight, self.bias, self)


class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, conv):
        x = x.contiguous()
        out, _ = ops.trunk_conv_forward(x, conv._packed(False), bias.detach().contiguous() if bias is not None else None,
                                        conv.out_channels, conv.kernel_size[0])
        ctx.conv = conv
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, _ = ctx.saved_tensors
        conv = ctx.conv
        d_out = d_out.contiguous()
        k = conv.kernel_size[0]
        d_x = d_w = d_b = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            d_w, d_b, _ = ops.trunk_conv_weight_grad(x, d_out, k, want_bias=ctx.has_bias)
        if ctx.needs_input_grad[0]:
            d_x, _ = ops.trunk_conv_input_grad(d_out, conv._packed(True), conv.in_channels, k)
        return d_x, d_w, d_b, None


class _ResBlockFn(torch.autograd.Function):
    """conv3x3 - PReLU - conv3x3, * res_scale + skip (common.py:59-79) in two launches: the first convolution's epilogue adds the
    bias and applies the PReLU (keeping the pre-activation for the backward), the second's adds the bias, scales and adds the
    skip.  Backward: the second conv's input gradient with the PReLU backward (and slope partials) in its epilogue, both weight
    gradients (the slope partials added up with the first), the first conv's input gradient with the skip gradient added."""

    @staticmethod
    def forward(ctx, x, w1, b1, slope, w2, b2, c1, c2, res_scale):
        x = x.contiguous()
        a = slope.detach().contiguous()
        u, pre = ops.trunk_conv_forward(x, c1._packed(False), b1.detach().contiguous(), c1.out_channels, 3, slope=a, want_pre=True)
        out, _ = ops.trunk_conv_forward(u, c2._packed(False), b2.detach().contiguous(), c2.out_channels, 3,
                                        res_scale=res_scale, residual=x)
        ctx.mods = (c1, c2)
        ctx.res_scale = float(res_scale)
        ctx.save_for_backward(x, pre, u, slope, w1, w2)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, pre, u, slope, _, _ = ctx.saved_tensors
        c1, c2 = ctx.mods
        rs = ctx.res_scale
        d_out = d_out.contiguous()
        a = slope.detach().contiguous()
        d_pre, part = ops.trunk_conv_input_grad(d_out, c2._packed(True), c2.in_channels, 3, alpha=rs, slope=a, pre=pre)
        d_w2, d_b2, _ = ops.trunk_conv_weight_grad(u, d_out, 3, alpha=rs)
        d_w1, d_b1, d_a = ops.trunk_conv_weight_grad(x, d_pre, 3, slope_part=part)
        d_x = None
        if ctx.needs_input_grad[0]:
            d_x, _ = ops.trunk_conv_input_grad(d_pre, c1._packed(True), c1.in_channels, 3, skip=d_out)
        return d_x, d_w1, d_b1, d_a.view_as(slope), d_w2, d_b2, None, None, None


def fused_resblock_ok(c1, act, c2) -> bool:
    """A ResBlock body the fused path runs: two converted 3x3 convolutions with biases around the one-slope library PReLU."""
    from .train_ops import PReLU
    return (type(c1) is Conv2d and type(c2) is Conv2d and type(act) is PReLU and act.weight.numel() == 1
            and c1.kernel_size == (3, 3) and c2.kernel_size == (3, 3) and c1.bias is not None and c2.bias is not None
            and c1.out_channels == c2.in_channels)


def resblock(x, c1, act, c2, res_scale):
    _check_call(c1, x)
    if act.weight.dtype != torch.float32 or act.weight.device != x.device:
        raise DaglError(f"trunk: PReLU slope is {act.weight.dtype} on {act.weight.device}, the input fp32 on {x.device}")
    _check_params(c2, x.device)
    return _ResBlockFn.apply(x, c1.weight, c1.bias, act.weight, c2.weight, c2.bias, c1, c2, float(res_scale))


def convert(module: nn.Module) -> nn.Module:
    """Re-class, in place, every plain ``nn.Conv2d`` of ``module`` (``type(m) is nn.Conv2d``) as ``trunk.Conv2d``, keeping its parameter
    tensors; returns ``module``.  The convolutions inside a ``CE`` (parameters of the library's prologue kernels, never applied as
    layers) and the never-applied ``_MeanShift`` are left alone.  A plain ``nn.Conv2d`` outside the library's scope (``unsupported``)
    raises ``DaglError`` naming it, before anything is changed: a converted model never reaches the stock convolution unnoticed."""
    from .ce import CE
    from .net import _MeanShift
    todo = []

    def visit(m, name):
        if isinstance(m, (CE, _MeanShift)):
            return
        if type(m) is nn.Conv2d:
            why = unsupported(m)
            if why is not None:
                raise DaglError(f"trunk.convert: {name or type(m).__name__} is outside the library's scope: {why}")
            todo.append(m)
            return
        for n, child in m.named_children():
            visit(child, f"{name}.{n}" if name else n)

    visit(module, "")
    for m in todo:
        m.__class__ = Conv2d
    return module


def invalidate_packed(module: nn.Module) -> nn.Module:
    """Drop the cached packed weights of every converted convolution of ``module``: the next call packs them again.  Needed after
    weights were written through ``.data`` (``Conv2d``); returns ``module``."""
    for m in module.modules():
        if isinstance(m, Conv2d):
            m.invalidate_packed()
    return module
