"""``spconv.SubMConv3d`` / ``spconv.SparseConv3d`` of spconv 1.2 on ``modest_amd.ops.spconv_*``."""
import math

import torch
from torch import nn

from ... import ops
from .modules import SparseModule
from .tensor import SparseConvTensor


class _SparseConvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, weight, bias, rulebook):
        features, weight = features.contiguous(), weight.contiguous()
        ctx.rulebook = rulebook
        ctx.has_bias = bias is not None
        ctx.save_for_backward(features, weight)
        return ops.spconv_forward(features, weight, bias.contiguous() if bias is not None else None, rulebook)

    @staticmethod
    def backward(ctx, grad_out):
        features, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dw, db = ops.spconv_backward(features, weight, grad_out.contiguous(), ctx.rulebook, need_input_grad=need[0],
                                         need_weight_grad=need[1], need_bias_grad=ctx.has_bias and need[2])
        return dx, dw, db, None


class SparseConvolution(SparseModule):
    """weight (kz, ky, kx, Cin, Cout), bias (Cout,): spconv 1.2's layout, so a checkpoint's state_dict loads"""

    def __init__(self, ndim, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 subm=False, output_padding=0, transposed=False, inverse=False, indice_key=None, fused_bn=False,
                 use_hash=False, algo=None):
        super().__init__()
        if ndim != 3:
            raise NotImplementedError("only 3-D sparse convolutions are provided by modest_amd")
        if transposed or inverse or groups != 1 or fused_bn:
            raise NotImplementedError("groups, transposed, inverse and fused sparse convolutions are not provided by modest_amd")
        if ops._triple(dilation, "dilation") != (1, 1, 1):
            raise NotImplementedError("dilation is accepted at 1 only")
        if ops._triple(output_padding, "output_padding") != (0, 0, 0):
            raise NotImplementedError("output_padding belongs to transposed convolutions, which are not provided")
        if not (1 <= in_channels <= 128 and 1 <= out_channels <= 128):
            raise ValueError("channels must lie in 1 .. 128")
        self.ndim = ndim
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size = list(ops._triple(kernel_size, "kernel_size"))
        self.stride = list(ops._triple(stride, "stride"))
        self.padding = list(ops._triple(padding, "padding"))
        self.dilation = [1, 1, 1]
        self.subm = bool(subm)
        self.indice_key = indice_key
        if self.subm and any(k % 2 == 0 for k in self.kernel_size):
            raise ValueError(f"a submanifold convolution needs odd kernel sizes, got {self.kernel_size}")
        if min(self.kernel_size) < 1 or max(self.kernel_size) > 7:
            raise ValueError("kernel sizes must lie in 1 .. 7")
        self.weight = nn.Parameter(torch.empty(*self.kernel_size, self.in_channels, self.out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        # kaiming_uniform_(a=sqrt(5)) on fan-in K * Cin: the bound is sqrt(6 / ((1 + 5) fan_in)) = 1 / sqrt(fan_in)
        fan_in = self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2] * self.in_channels
        bound = 1.0 / math.sqrt(fan_in)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.uniform_(-bound, bound)

    def output_shape(self, spatial_shape):
        return ops.spconv_out_shape(spatial_shape, self.kernel_size, self.stride, self.padding, self.subm)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, subm={self.subm}, bias={self.bias is not None}, indice_key={self.indice_key!r}")

    def forward(self, input):
        assert isinstance(input, SparseConvTensor)
        out_shape = self.output_shape(input.spatial_shape)   # raises on an extent <= 0
        rulebook = input.find_indice_pair(self.indice_key)
        if rulebook is not None:
            if not rulebook.same_geometry(input.batch_size, input.spatial_shape, self.kernel_size, self.stride, self.padding,
                                          self.subm) or rulebook.n_in != input.indices.shape[0]:
                raise ValueError(f"indice_key {self.indice_key!r} was built for another kernel, stride, padding or input")
        else:
            rulebook = ops.spconv_rulebook(input.indices, input.batch_size, input.spatial_shape, self.kernel_size, self.stride,
                                           self.padding, self.subm)
            if self.indice_key is not None:
                input.indice_dict[self.indice_key] = rulebook
        features = _SparseConvFunction.apply(input.features, self.weight, self.bias, rulebook)
        out = SparseConvTensor(features, input.indices if self.subm else rulebook.out_indices, out_shape, input.batch_size, input.grid)
        out.indice_dict = input.indice_dict
        return out


class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None, use_hash=False, algo=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias,
                         indice_key=indice_key, use_hash=use_hash, algo=algo)


class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None, use_hash=False, algo=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, True,
                         indice_key=indice_key, use_hash=use_hash, algo=algo)
