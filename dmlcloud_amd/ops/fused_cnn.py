"""Autograd integration of the fused conv3x3+ReLU+maxpool2x2 kernels.

`ConvReluPool2d` is a drop-in module computing
conv2d(x, W, b, padding=1) -> relu -> max_pool2d(2) in ONE gfx950 kernel
per direction (ops/csrc/smallcnn.hip) on device tensors, with an exact
torch-semantics backward (first-index pool tie-break, relu gating). On
CPU it falls back to the equivalent torch ops, which also serve as the
differential-test oracle.
"""

import torch
from torch import nn
from torch.nn import functional as F

from . import _C, is_available


class _ConvReluPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, need_input_grad):
        N, CIN, H, W = x.shape
        COUT = weight.shape[0]
        pooled = torch.empty(N, COUT, H // 2, W // 2, device=x.device, dtype=x.dtype)
        argmax = torch.empty(N, COUT, H // 2, W // 2, device=x.device, dtype=torch.uint8)
        _C.conv3x3_relu_pool_fwd(x, weight, bias, pooled, argmax)
        # argmax carries the ReLU gate (bit 2), so backward needs no pooled values
        ctx.save_for_backward(x, weight, argmax)
        ctx.need_input_grad = need_input_grad
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        x, weight, argmax = ctx.saved_tensors
        dpooled = dpooled.contiguous()
        # the ordered second-stage sum stores every element of dw and db
        dw = torch.empty_like(weight)
        db = torch.empty(weight.shape[0], device=weight.device, dtype=weight.dtype)
        _C.conv3x3_relu_pool_bwd_weight(dpooled, argmax, x, dw, db)
        dx = None
        if ctx.need_input_grad:
            dx = torch.empty_like(x)
            _C.conv3x3_relu_pool_bwd_data(dpooled, argmax, weight, dx)
        return dx, dw, db, None


class _ConvStack2Fn(torch.autograd.Function):
    """Two fused layers whose first needs no input gradient (the image layer).

    Forward is the two layers' forward kernels. Backward is layer 2's
    bwd_weight and then ONE call for layer 2's bwd_data and layer 1's
    bwd_weight: the gradient between the layers never goes to memory
    (conv3x3_relu_pool_bwd_data_weight in ops/csrc/smallcnn.hip, which runs
    the two separate kernels on a temporary for shapes it has no merged
    kernel for). Bit for bit the layer-by-layer path.
    """

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        N, _, H, W = x.shape
        C1, C2 = w1.shape[0], w2.shape[0]

        def empty(c, h, w, dtype):
            return torch.empty(N, c, h, w, device=x.device, dtype=dtype)

        pooled1, argmax1 = empty(C1, H // 2, W // 2, x.dtype), empty(C1, H // 2, W // 2, torch.uint8)
        _C.conv3x3_relu_pool_fwd(x, w1, b1, pooled1, argmax1)
        pooled2, argmax2 = empty(C2, H // 4, W // 4, x.dtype), empty(C2, H // 4, W // 4, torch.uint8)
        _C.conv3x3_relu_pool_fwd(pooled1, w2, b2, pooled2, argmax2)
        ctx.save_for_backward(x, pooled1, argmax1, argmax2, w2)
        ctx.w1_shape = w1.shape
        return pooled2

    @staticmethod
    def backward(ctx, dpooled2):
        x, pooled1, argmax1, argmax2, w2 = ctx.saved_tensors
        dpooled2 = dpooled2.contiguous()
        dw2 = torch.empty_like(w2)
        db2 = torch.empty(w2.shape[0], device=w2.device, dtype=w2.dtype)
        _C.conv3x3_relu_pool_bwd_weight(dpooled2, argmax2, pooled1, dw2, db2)
        dw1 = torch.empty(ctx.w1_shape, device=w2.device, dtype=w2.dtype)
        db1 = torch.empty(ctx.w1_shape[0], device=w2.device, dtype=w2.dtype)
        _C.conv3x3_relu_pool_bwd_data_weight(dpooled2, argmax2, w2, argmax1, x, dw1, db1)
        return None, dw1, db1, dw2, db2


class ConvReluPool2d(nn.Module):
    """conv3x3(pad=1) + ReLU + maxpool2x2, fused on gfx950.

    first_layer=True skips the input gradient (e.g. the image layer).
    """

    def __init__(self, in_channels: int, out_channels: int, first_layer: bool = False):
        super().__init__()
        self.first_layer = first_layer
        conv = nn.Conv2d(in_channels, out_channels, 3, padding=1)  # init only
        self.weight = nn.Parameter(conv.weight.detach().clone())
        self.bias = nn.Parameter(conv.bias.detach().clone())

    def forward(self, x):
        if x.is_cuda and is_available():
            need_dx = (not self.first_layer) or x.requires_grad
            return _ConvReluPoolFn.apply(x, self.weight, self.bias, need_dx)
        # CPU fallback / oracle
        y = F.conv2d(x, self.weight, self.bias, padding=1)
        return F.max_pool2d(F.relu(y), 2)


class FusedMnistCNN(nn.Module):
    """The benchmark MNIST-CNN built from fused layers + nn.Linear.

    Architecture identical to models/mnist.mnist_cnn (reference
    examples/mnist.py:27-37); state_dict-compatible keys differ (fused
    modules), parameter count identical.
    """

    def __init__(self):
        super().__init__()
        self.layer1 = ConvReluPool2d(1, 16, first_layer=True)
        self.layer2 = ConvReluPool2d(16, 16)
        self.fc = nn.Linear(784, 10)

    def forward(self, x):
        if x.is_cuda and is_available() and not x.requires_grad:
            # one autograd node over both conv layers: see _ConvStack2Fn
            l1, l2 = self.layer1, self.layer2
            x = _ConvStack2Fn.apply(x, l1.weight, l1.bias, l2.weight, l2.bias)
        else:
            x = self.layer1(x)
            x = self.layer2(x)
        return self.fc(x.flatten(1))
