"""Micro-benchmark of the fused smallcnn kernels per layer shape.

Run on a GPU box:  python tools/bench_smallcnn.py [--no-torch] [batch ...]
Prints per-kernel times (cuda events, 100 reps) for the two MNIST-CNN
layer shapes, plus the torch/MIOpen equivalents for comparison (left out
with --no-torch). Shapes that take the f32 MFMA path get a second row with
DMLCLOUD_SMALLCNN_MFMA=0, the VALU kernels. The last row per batch is the
two-layer stack's backward between the layers: conv2 bwd_data plus conv1
bwd_weight as two calls, as the one merged call, and as that call with
DMLCLOUD_SMALLCNN_MERGE_BWD=0.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from dmlcloud_amd import _C

DEV = 'cuda:0'


def time_fn(fn, reps=100, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps * 1e3  # us


def bench_shape(n, cin, cout, hw, with_torch=True, mfma=True):
    os.environ['DMLCLOUD_SMALLCNN_MFMA'] = '1' if mfma else '0'  # read per call
    torch.manual_seed(0)
    x = torch.randn(n, cin, hw, hw, device=DEV)
    w = torch.randn(cout, cin, 3, 3, device=DEV) * 0.1
    b = torch.randn(cout, device=DEV) * 0.1
    pooled = torch.empty(n, cout, hw // 2, hw // 2, device=DEV)
    argmax = torch.empty(n, cout, hw // 2, hw // 2, device=DEV, dtype=torch.uint8)
    _C.conv3x3_relu_pool_fwd(x, w, b, pooled, argmax)
    dpooled = torch.randn_like(pooled)
    din = torch.empty_like(x)
    dw = torch.empty_like(w)
    db = torch.empty_like(b)

    t_fwd = time_fn(lambda: _C.conv3x3_relu_pool_fwd(x, w, b, pooled, argmax))
    t_bwdd = time_fn(lambda: _C.conv3x3_relu_pool_bwd_data(dpooled, argmax, w, din))
    t_bwdw = time_fn(lambda: _C.conv3x3_relu_pool_bwd_weight(dpooled, argmax, x, dw, db))

    os.environ.pop('DMLCLOUD_SMALLCNN_MFMA')
    line = (
        f'N={n:6d} cin={cin:2d} cout={cout:2d} hw={hw:2d} mfma={int(mfma)} | '
        f'fwd {t_fwd:8.1f}us bwd_data {t_bwdd:8.1f}us bwd_w {t_bwdw:8.1f}us '
        f'(sum {t_fwd + t_bwdd + t_bwdw:8.1f}us)'
    )
    if not with_torch:
        print(line)
        return

    # torch eager equivalents
    def torch_fwd():
        F.max_pool2d(F.relu(F.conv2d(x, w, b, padding=1)), 2)

    x2 = x.detach().requires_grad_(True)
    w2 = w.detach().requires_grad_(True)
    b2 = b.detach().requires_grad_(True)

    def torch_fwdbwd():
        out = F.max_pool2d(F.relu(F.conv2d(x2, w2, b2, padding=1)), 2)
        out.backward(dpooled)
        x2.grad = None
        w2.grad = None
        b2.grad = None

    t_tfwd = time_fn(torch_fwd, reps=50)
    t_tfb = time_fn(torch_fwdbwd, reps=50)

    print(f'{line} | torch fwd {t_tfwd:8.1f}us fwd+bwd {t_tfb:8.1f}us')


def bench_stack(n, cin1=1, c1=16, hw=28, c2=16):
    """conv2 bwd_data + conv1 bwd_weight on the stacked shapes: two calls
    against conv3x3_relu_pool_bwd_data_weight on the same tensors."""
    torch.manual_seed(0)
    x = torch.randn(n, cin1, hw, hw, device=DEV)
    w1 = torch.randn(c1, cin1, 3, 3, device=DEV) * 0.1
    b1 = torch.randn(c1, device=DEV) * 0.1
    w2 = torch.randn(c2, c1, 3, 3, device=DEV) * 0.1
    b2 = torch.randn(c2, device=DEV) * 0.1
    pooled1 = torch.empty(n, c1, hw // 2, hw // 2, device=DEV)
    argmax1 = torch.empty_like(pooled1, dtype=torch.uint8)
    _C.conv3x3_relu_pool_fwd(x, w1, b1, pooled1, argmax1)
    pooled2 = torch.empty(n, c2, hw // 4, hw // 4, device=DEV)
    argmax2 = torch.empty_like(pooled2, dtype=torch.uint8)
    _C.conv3x3_relu_pool_fwd(pooled1, w2, b2, pooled2, argmax2)
    dpooled2 = torch.randn_like(pooled2)
    din = torch.empty_like(pooled1)
    dw1, db1 = torch.empty_like(w1), torch.empty_like(b1)

    def two_calls():
        _C.conv3x3_relu_pool_bwd_data(dpooled2, argmax2, w2, din)
        _C.conv3x3_relu_pool_bwd_weight(din, argmax1, x, dw1, db1)

    def one_call():
        _C.conv3x3_relu_pool_bwd_data_weight(dpooled2, argmax2, w2, argmax1, x, dw1, db1)

    t_two = time_fn(two_calls)
    t_one = time_fn(one_call)
    os.environ['DMLCLOUD_SMALLCNN_MERGE_BWD'] = '0'  # read per call
    t_off = time_fn(one_call)
    os.environ.pop('DMLCLOUD_SMALLCNN_MERGE_BWD')
    print(
        f'N={n:6d} stack {cin1}->{c1}->{c2} hw={hw:2d} | bwd_data2 + bwd_w1 {t_two:8.1f}us '
        f'merged {t_one:8.1f}us merged, switch 0 {t_off:8.1f}us'
    )


if __name__ == '__main__':
    args = sys.argv[1:]
    with_torch = '--no-torch' not in args
    batches = [int(a) for a in args if not a.startswith('--')] or [1024, 4096, 16384]
    for n in batches:
        bench_shape(n, 1, 16, 28, with_torch)  # conv1 shape
        bench_shape(n, 16, 16, 14, with_torch)  # conv2 shape
        bench_shape(n, 16, 16, 14, False, mfma=False)  # conv2 shape, VALU kernels
        bench_stack(n)
