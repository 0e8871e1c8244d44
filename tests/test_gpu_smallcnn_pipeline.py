"""smallcnn sample pipeline: exact semantics, pipeline edges, store bounds.

The fused conv3x3+ReLU+maxpool kernels walk a sequence of samples per
workgroup, stage each through registers in 16-byte pieces and carry the
ReLU gate in the argmax byte. These tests pin down what that must not change:
the exact torch semantics (ties, all-negative windows), the first/last
sample of every workgroup, chunk boundaries of the weight gradient,
stores that stay inside their tensors at any alignment, and graph replay.
The oracle is always float64 torch on the CPU.
Run on an MI355X box: python -m pytest tests -m gpu
"""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from dmlcloud_amd import ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _oracle(x, w, b, g):
    """conv -> relu -> maxpool with autograd in float64 on the CPU.
    Returns out, dx, dw, db and the relu output (for counting windows)."""
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    b = b.double().requires_grad_(True)
    act = F.relu(F.conv2d(x, w, b, padding=1))
    out = F.max_pool2d(act, 2)
    out.backward(g.double())
    return out.detach(), x.grad, w.grad, b.grad, act.detach()


@functools.lru_cache(maxsize=None)
def _int_case(cin, cout, H, W, N):
    """Small-integer inputs (every fp32 sum is exact) and their oracle."""
    # the seed is one for which even the smallest case holds both kinds of window
    gen = torch.Generator().manual_seed(1 + 1000 * cin + 100 * cout + 10 * H + W + N)

    def draw(*shape):
        return torch.randint(-3, 4, shape, generator=gen).float()

    x, w, b = draw(N, cin, H, W), draw(cout, cin, 3, 3), draw(cout)
    g = draw(N, cout, H // 2, W // 2)
    out, dx, dw, db, act = _oracle(x, w, b, g)
    # 2x2 windows of the relu output: [N, cout, PH, PW, 4]
    win = act.unfold(2, 2, 2).unfold(3, 2, 2).reshape(N, cout, H // 2, W // 2, 4)
    top = win.max(dim=-1, keepdim=True).values
    tied = ((win == top).sum(dim=-1) > 1) & (top[..., 0] > 0)
    zero = top[..., 0] == 0
    return {
        'x': x, 'w': w, 'b': b, 'g': g,
        'out': out.float(), 'dx': dx.float(), 'dw': dw.float(), 'db': db.float(),
        'tied': int(tied.sum()), 'zero': int(zero.sum()),
    }  # fmt: skip


def _layer_like(w, b, first_layer=False):
    from dmlcloud_amd.ops.fused_cnn import ConvReluPool2d

    layer = ConvReluPool2d(w.shape[1], w.shape[0], first_layer=first_layer).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(w)
        layer.bias.copy_(b)
    return layer


INT_CASES = [
    (1, 2, 4, 4, 3),
    (3, 4, 6, 10, 5),  # H != W, PH odd
    (16, 16, 14, 14, 3),  # conv2 geometry
    (1, 16, 28, 28, 2),  # conv1 geometry
    (5, 7, 12, 12, 3),
]


class TestExactSemantics:
    @pytest.mark.parametrize('cin,cout,H,W,N', INT_CASES)
    def test_integer_data_bitwise(self, cin, cout, H, W, N):
        """On integer data the kernels reproduce the oracle exactly; the
        data hold tied windows and windows whose pooled value is 0, so the
        first-index rule and the gate bit of the argmax byte are exercised."""
        assert ops.is_available()
        c = _int_case(cin, cout, H, W, N)
        assert c['tied'] >= 1, 'data hold no tied window'
        assert c['zero'] >= 1, 'data hold no window with pooled value 0'

        layer = _layer_like(c['w'], c['b'])
        x = c['x'].to(DEV).requires_grad_(True)
        out = layer(x)
        out.backward(c['g'].to(DEV))
        assert torch.equal(out.detach().cpu(), c['out'])
        assert torch.equal(x.grad.cpu(), c['dx'])
        assert torch.equal(layer.weight.grad.cpu(), c['dw'])
        assert torch.equal(layer.bias.grad.cpu(), c['db'])


def _random_case(cin, cout, H, W, N, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, 3, 3, generator=gen) * 0.2
    b = torch.randn(cout, generator=gen) * 0.2
    g = torch.randn(N, cout, H // 2, W // 2, generator=gen)
    return x, w, b, g, _oracle(x, w, b, g)


def _check_against_oracle(layer, x_dev, out, oracle, dx=True):
    ref_out, ref_dx, ref_dw, ref_db, _ = oracle
    torch.testing.assert_close(out.detach().cpu().double(), ref_out, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(layer.weight.grad.cpu().double(), ref_dw, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(layer.bias.grad.cpu().double(), ref_db, rtol=1e-4, atol=1e-4)
    if dx:
        torch.testing.assert_close(x_dev.grad.cpu().double(), ref_dx, rtol=1e-4, atol=1e-4)


class TestPipelineEdges:
    @pytest.mark.parametrize(
        'cin,cout,H,W,N',
        [
            (16, 16, 14, 14, 1),  # no second sample anywhere
            (16, 16, 14, 14, 2),
            (16, 16, 14, 14, 3),
            (2, 3, 4, 4, 2048 + 5),  # past the 2048-workgroup cap: 5 workgroups take a second sample
        ],
    )
    def test_first_and_last_sample(self, cin, cout, H, W, N):
        x, w, b, g, oracle = _random_case(cin, cout, H, W, N, seed=N)
        layer = _layer_like(w, b)
        x_dev = x.to(DEV).requires_grad_(True)
        out = layer(x_dev)
        out.backward(g.to(DEV))
        _check_against_oracle(layer, x_dev, out, oracle)

    @pytest.mark.parametrize(
        'cin,cout,H,W,N,chunk',
        [
            (2, 3, 8, 8, 7, '3'),  # chunks of 3, 3 and 1
            (2, 3, 4, 4, 2 * 2048 + 3, '2'),  # capped grid, several chunks per workgroup, last chunk partial
        ],
    )
    def test_weight_grad_chunk_boundaries(self, cin, cout, H, W, N, chunk, monkeypatch):
        """The sample sequence of a weight-gradient workgroup runs across
        chunk boundaries and stops at the last sample of the last chunk."""
        monkeypatch.setenv('DMLCLOUD_SMALLCNN_BWDW_CHUNK', chunk)
        x, w, b, g, oracle = _random_case(cin, cout, H, W, N, seed=N)
        layer = _layer_like(w, b, first_layer=True)
        x_dev, g_dev = x.to(DEV), g.to(DEV)
        grads = []
        for _ in range(2):
            layer.zero_grad(set_to_none=True)
            out = layer(x_dev)
            out.backward(g_dev)
            grads.append((layer.weight.grad.clone(), layer.bias.grad.clone()))
        assert torch.equal(grads[0][0], grads[1][0])
        assert torch.equal(grads[0][1], grads[1][1])
        _check_against_oracle(layer, x_dev, out, oracle, dx=False)


def _view_in(buf, offset, shape):
    n = 1
    for s in shape:
        n *= s
    return buf[offset : offset + n].view(shape)


def _untouched_outside(buf, offset, numel, is_sentinel):
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    mask[offset : offset + numel] = False
    return bool(is_sentinel(buf[mask]).all())


class TestStoreBounds:
    # (3, 5, 6, 6): a pooled plane of 5 * 9 = 45 elements, no multiple of 4, so
    # sample starts are misaligned for vector stores and the pooled-side loads
    # go cell by cell; (3, 4, 4, 4): 16 cells per sample, the float4 /
    # packed-word loads at offset 0 and the cell-by-cell ones at offset 1
    @pytest.mark.parametrize('cin,cout,H,W,N', [(3, 5, 6, 6, 3), (3, 4, 4, 4, 3)])
    @pytest.mark.parametrize('out_off,in_off', [(0, 0), (1, 0), (0, 1), (1, 1)])
    def test_views_into_larger_buffers(self, cin, cout, H, W, N, out_off, in_off):
        """Outputs are views at element offset `out_off` into sentinel-filled
        buffers, inputs views at offset `in_off` (offset 1 takes the scalar
        load paths). Nothing outside the views is written, dw/db need no
        initialisation, and the results equal the integer oracle."""
        from dmlcloud_amd import _C

        c = _int_case(cin, cout, H, W, N)
        PH, PW = H // 2, W // 2
        pad = 16
        nan = float('nan')

        def fbuf(numel):
            return torch.full((numel + pad,), nan, device=DEV)

        def as_input(t):
            buf = torch.zeros(t.numel() + pad, device=DEV, dtype=t.dtype)
            view = _view_in(buf, in_off, t.shape)
            view.copy_(t)
            return view

        x, g = as_input(c['x']), as_input(c['g'])
        w, b = c['w'].to(DEV), c['b'].to(DEV)
        n_out, n_x = N * cout * PH * PW, c['x'].numel()

        out_buf, din_buf = fbuf(n_out), fbuf(n_x)
        dw_buf, db_buf = fbuf(w.numel()), fbuf(cout)
        arg_buf = torch.full((n_out + pad,), 0xAA, device=DEV, dtype=torch.uint8)
        out = _view_in(out_buf, out_off, (N, cout, PH, PW))
        argmax = _view_in(arg_buf, out_off, (N, cout, PH, PW))
        din = _view_in(din_buf, out_off, c['x'].shape)
        dw = _view_in(dw_buf, out_off, w.shape)
        db = _view_in(db_buf, out_off, (cout,))

        _C.conv3x3_relu_pool_fwd(x, w, b, out, argmax)
        if in_off:  # the backward kernels read argmax: give it the inputs' offset too
            argmax = as_input(argmax)
        _C.conv3x3_relu_pool_bwd_data(g, argmax, w, din)
        _C.conv3x3_relu_pool_bwd_weight(g, argmax, x, dw, db)
        torch.cuda.synchronize()

        assert torch.equal(out.cpu(), c['out'])
        assert torch.equal(din.cpu(), c['dx'])
        assert torch.isfinite(dw).all() and torch.isfinite(db).all()
        assert torch.equal(dw.cpu(), c['dw'])
        assert torch.equal(db.cpu(), c['db'])
        assert _untouched_outside(out_buf, out_off, n_out, torch.isnan)
        assert _untouched_outside(din_buf, out_off, n_x, torch.isnan)
        assert _untouched_outside(dw_buf, out_off, w.numel(), torch.isnan)
        assert _untouched_outside(db_buf, out_off, cout, torch.isnan)
        assert _untouched_outside(arg_buf, out_off, n_out, lambda t: t == 0xAA)


class TestGraphReplay:
    def test_replayed_gradients_equal_eager(self):
        """A captured forward+backward replayed on a second batch gives
        exactly the eager gradients of that batch."""
        from dmlcloud_amd.ops.fused_cnn import FusedMnistCNN

        torch.manual_seed(0)
        model = FusedMnistCNN().to(DEV)
        eager = copy.deepcopy(model)
        batches = [
            (torch.randn(8, 1, 28, 28, device=DEV), torch.randint(0, 10, (8,), device=DEV)) for _ in range(2)
        ]
        x_static, y_static = batches[0][0].clone(), batches[0][1].clone()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                model.zero_grad(set_to_none=True)
                F.cross_entropy(model(x_static), y_static).backward()
        torch.cuda.current_stream().wait_stream(side)

        model.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            F.cross_entropy(model(x_static), y_static).backward()

        x_static.copy_(batches[1][0])
        y_static.copy_(batches[1][1])
        graph.replay()
        torch.cuda.synchronize()

        F.cross_entropy(eager(batches[1][0]), batches[1][1]).backward()
        for (name, p), q in zip(model.named_parameters(), eager.parameters()):
            assert torch.equal(p.grad, q.grad), name
