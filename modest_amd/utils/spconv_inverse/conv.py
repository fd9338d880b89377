"""``spconv.SparseInverseConv3d`` of spconv 1.2 on ``modest_amd.ops.spconv_inverse_*``."""
import math

import torch
from torch import nn

from ... import ops
from ..spconv.modules import SparseModule
from ..spconv.tensor import SparseConvTensor


class _SparseInverseConvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, weight, bias, rulebook):
        features, weight = features.contiguous(), weight.contiguous()
        ctx.rulebook = rulebook
        ctx.has_bias = bias is not None
        ctx.save_for_backward(features, weight)
        return ops.spconv_inverse_forward(features, weight, bias.contiguous() if bias is not None else None, rulebook)

    @staticmethod
    def backward(ctx, grad_out):
        features, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dw, db = ops.spconv_inverse_backward(features, weight, grad_out.contiguous(), ctx.rulebook, need_input_grad=need[0],
                                                 need_weight_grad=need[1], need_bias_grad=ctx.has_bias and need[2])
        return dx, dw, db, None


class SparseInverseConv3d(SparseModule):
    """Runs the rulebook that the strided convolution with the same ``indice_key`` built backwards: the output lives on
    that convolution's input sites and carries its ``indices`` tensor.  weight (kz, ky, kx, Cin, Cout), bias (Cout,):
    spconv 1.2's layout, so a checkpoint's state_dict loads."""

    def __init__(self, in_channels, out_channels, kernel_size, indice_key=None, bias=True, use_hash=False, algo=None):
        super().__init__()
        if not (1 <= in_channels <= 128 and 1 <= out_channels <= 128):
            raise ValueError("channels must lie in 1 .. 128")
        self.ndim = 3
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size = list(ops._triple(kernel_size, "kernel_size"))
        if min(self.kernel_size) < 1 or max(self.kernel_size) > 7:
            raise ValueError("kernel sizes must lie in 1 .. 7")
        self.inverse = True
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.empty(*self.kernel_size, self.in_channels, self.out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        # as SparseConvolution: kaiming_uniform_(a=sqrt(5)) on fan-in K * Cin, the bound is 1 / sqrt(fan_in)
        fan_in = self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2] * self.in_channels
        bound = 1.0 / math.sqrt(fan_in)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.uniform_(-bound, bound)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, bias={self.bias is not None}, "
                f"indice_key={self.indice_key!r}")

    def rulebook_of(self, input):
        """the strided rulebook this layer inverts, checked against the input: raises ValueError before any launch"""
        if self.indice_key is None:
            raise ValueError("SparseInverseConv3d needs the indice_key of the strided convolution it inverts")
        rb = input.find_indice_pair(self.indice_key)
        if rb is None:
            raise ValueError(f"indice_key {self.indice_key!r} names no rulebook: the strided convolution has not run on this tensor")
        if getattr(rb, "subm", True):
            raise ValueError(f"indice_key {self.indice_key!r} names a submanifold rulebook, an inverse convolution needs a strided one")
        if tuple(rb.kernel) != tuple(self.kernel_size):
            raise ValueError(f"indice_key {self.indice_key!r} was built for kernel {list(rb.kernel)}, this layer has {self.kernel_size}")
        if input.features.shape[0] != rb.n_out or input.indices.shape[0] != rb.n_out:
            raise ValueError(f"the input has {input.features.shape[0]} rows, the rulebook of {self.indice_key!r} has {rb.n_out} outputs")
        if list(input.spatial_shape) != list(rb.out_shape) or input.batch_size != rb.batch_size:
            raise ValueError(f"the input has spatial shape {input.spatial_shape} and batch size {input.batch_size}, the rulebook "
                             f"of {self.indice_key!r} writes {list(rb.out_shape)} and {rb.batch_size}")
        return rb

    def forward(self, input):
        assert isinstance(input, SparseConvTensor)
        rb = self.rulebook_of(input)
        features = _SparseInverseConvFunction.apply(input.features, self.weight, self.bias, rb)
        out = SparseConvTensor(features, rb.indices, rb.in_shape, input.batch_size, input.grid)
        out.indice_dict = input.indice_dict
        return out
