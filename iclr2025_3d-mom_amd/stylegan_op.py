"""The `op` package of the reference's StyleGAN2 (thirdparty/StyleCineGAN/models/stylegan2/op, and the encoder's copy of it) on
libmom4d, by its names:

    op/upfirdn2d.py    upfirdn2d, UpFirDn2d, UpFirDn2dBackward
    op/fused_act.py    FusedLeakyReLU, fused_leaky_relu, FusedLeakyReLUFunction, FusedLeakyReLUFunctionBackward

The reference compiles two CUDA sources when that package is imported and has no other path, so its `Generator` cannot be imported
on ROCm.  Here the same names run on ops.upfirdn2d and ops.fused_bias_act (csrc/stylegan_ops.hip); `install_video_dropin()` of the
package registers this module under `thirdparty.StyleCineGAN.models.stylegan2.op`, `.op.fused_act` and `.op.upfirdn2d`.  The
autograd wiring is the reference's, forward and both backward orders: the gradient of upfirdn2d is upfirdn2d with the flipped
kernel, up and down exchanged and the pads of op/upfirdn2d.py:108-111; the gradient of the activation selects by the sign of the
saved output.  The model files (model.py, the encoders) and the checkpoints are the user's own; `conv2d_gradfix` is not mirrored
(nothing imports it).
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd import Function

from . import ops


def grad_pad(kernel_shape, in_hw, out_hw, up, down, pad):
    """The pads of the gradient's upfirdn2d (op/upfirdn2d.py:108-111)."""
    (kh, kw), (in_h, in_w), (out_h, out_w), (up_x, up_y), (down_x, down_y) = kernel_shape, in_hw, out_hw, up, down
    pad_x0, pad_x1, pad_y0, pad_y1 = pad
    return (kw - pad_x0 - 1, in_w * up_x - out_w * down_x + pad_x0 - up_x + 1,
            kh - pad_y0 - 1, in_h * up_y - out_h * down_y + pad_y0 - up_y + 1)


def _planes(t, h, w):
    return t.detach().reshape(1, -1, h, w).contiguous()


class UpFirDn2dBackward(Function):
    @staticmethod
    def forward(ctx, grad_output, kernel, grad_kernel, up, down, pad, g_pad, in_size, out_size):
        grad_input = ops.upfirdn2d(_planes(grad_output, out_size[0], out_size[1]), grad_kernel, down, up, g_pad)
        grad_input = grad_input.view(in_size[0], in_size[1], in_size[2], in_size[3])
        ctx.save_for_backward(kernel)
        ctx.up, ctx.down, ctx.pad, ctx.in_size, ctx.out_size = up, down, pad, in_size, out_size
        return grad_input

    @staticmethod
    def backward(ctx, gradgrad_input):
        kernel, = ctx.saved_tensors
        gradgrad_out = ops.upfirdn2d(_planes(gradgrad_input, ctx.in_size[2], ctx.in_size[3]), kernel, ctx.up, ctx.down, ctx.pad)
        gradgrad_out = gradgrad_out.view(ctx.in_size[0], ctx.in_size[1], ctx.out_size[0], ctx.out_size[1])
        return gradgrad_out, None, None, None, None, None, None, None, None


class UpFirDn2d(Function):
    @staticmethod
    def forward(ctx, input, kernel, up, down, pad):
        up, down, pad = tuple(up), tuple(down), tuple(pad)
        kernel = kernel.detach().contiguous()
        kernel_h, kernel_w = kernel.shape
        batch, channel, in_h, in_w = input.shape
        ctx.in_size = input.shape
        ctx.save_for_backward(kernel, torch.flip(kernel, [0, 1]).contiguous())
        out_h, out_w = ops.upfirdn2d_out_size(in_h, in_w, kernel_h, kernel_w, up, down, pad)
        ctx.out_size = (out_h, out_w)
        ctx.up, ctx.down, ctx.pad = up, down, pad
        ctx.g_pad = grad_pad((kernel_h, kernel_w), (in_h, in_w), (out_h, out_w), up, down, pad)
        out = ops.upfirdn2d(_planes(input, in_h, in_w), kernel, up, down, pad)
        return out.view(-1, channel, out_h, out_w)

    @staticmethod
    def backward(ctx, grad_output):
        kernel, grad_kernel = ctx.saved_tensors
        grad_input = UpFirDn2dBackward.apply(grad_output, kernel, grad_kernel, ctx.up, ctx.down, ctx.pad, ctx.g_pad, ctx.in_size,
                                             ctx.out_size)
        return grad_input, None, None, None, None


def upfirdn2d(input, kernel, up=1, down=1, pad=(0, 0)):
    return UpFirDn2d.apply(input, kernel, (up, up), (down, down), (pad[0], pad[1], pad[0], pad[1]))


class FusedLeakyReLUFunctionBackward(Function):
    @staticmethod
    def forward(ctx, grad_output, out, negative_slope, scale):
        ctx.save_for_backward(out)
        ctx.negative_slope = negative_slope
        ctx.scale = scale
        grad_input = ops.fused_bias_act(grad_output.detach().contiguous(), None, out.detach(), 3, 1, negative_slope, scale)
        dim = [0]
        if grad_input.ndim > 2:
            dim += list(range(2, grad_input.ndim))
        grad_bias = grad_input.sum(dim).detach()
        return grad_input, grad_bias

    @staticmethod
    def backward(ctx, gradgrad_input, gradgrad_bias):
        out, = ctx.saved_tensors
        gradgrad_out = ops.fused_bias_act(gradgrad_input.detach().contiguous(), gradgrad_bias.detach().contiguous(), out.detach(),
                                          3, 1, ctx.negative_slope, ctx.scale)
        return gradgrad_out, None, None, None


class FusedLeakyReLUFunction(Function):
    @staticmethod
    def forward(ctx, input, bias, negative_slope, scale):
        out = ops.fused_bias_act(input.detach().contiguous(), bias.detach().contiguous(), None, 3, 0, negative_slope, scale)
        ctx.save_for_backward(out)
        ctx.negative_slope = negative_slope
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, grad_output):
        out, = ctx.saved_tensors
        grad_input, grad_bias = FusedLeakyReLUFunctionBackward.apply(grad_output, out, ctx.negative_slope, ctx.scale)
        return grad_input, grad_bias, None, None


class FusedLeakyReLU(nn.Module):
    def __init__(self, channel, negative_slope=0.2, scale=2 ** 0.5):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(channel))
        self.negative_slope = negative_slope
        self.scale = scale

    def forward(self, input):
        return fused_leaky_relu(input, self.bias, self.negative_slope, self.scale)


def fused_leaky_relu(input, bias, negative_slope=0.2, scale=2 ** 0.5):
    return FusedLeakyReLUFunction.apply(input, bias, negative_slope, scale)
