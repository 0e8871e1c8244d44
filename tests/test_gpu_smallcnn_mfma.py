"""smallcnn f32 MFMA forms of forward and bwd_data (16 output channels).

Layers with COUT == 16 and CIN in {4, 8, 12, 16} run forward and bwd_data as
an implicit GEMM on v_mfma_f32_16x16x4_f32; DMLCLOUD_SMALLCNN_MFMA=0 forces
the VALU kernels. The instruction is a k-ordered fmaf chain, so the two
paths must agree bit for bit: every path comparison here is torch.equal, with
no tolerance. The oracle for the integer cases is float64 torch on the CPU.
Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools

import pytest
import torch
import torch.nn.functional as F

from dmlcloud_amd import ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SWITCH = 'DMLCLOUD_SMALLCNN_MFMA'

# (CIN, COUT, H, W, N) -> seed for which the integer data hold a tied window
# and a window with pooled value 0 (searched on the CPU)
ELIGIBLE = {
    (4, 16, 2, 2, 1): 1,  # one window; a tile with three padded window-rows; din 4 positions
    (4, 16, 4, 4, 1): 2,  # exactly one full tile in both kernels; K = 36 (9 steps)
    (8, 16, 6, 10, 5): 0,  # H != W, odd PH; 15 windows (ragged tile); din groups of 4 straddle rows of 10
    (12, 16, 8, 8, 2): 0,  # K = 108
    (16, 16, 14, 14, 3): 0,  # the workload's geometry: 12 full tiles + 1 window; 196 = 12*16 + 4 positions
    (16, 16, 14, 14, 2051): 0,  # past the 2048-workgroup cap: three workgroups take a second sample
}
INELIGIBLE = [(5, 7, 12, 12, 3), (1, 16, 28, 28, 2), (16, 32, 8, 8, 2)]


def _oracle(x, w, b, g):
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    b = b.double().requires_grad_(True)
    act = F.relu(F.conv2d(x, w, b, padding=1))
    out = F.max_pool2d(act, 2)
    out.backward(g.double())
    return out.detach(), x.grad, w.grad, b.grad, act.detach()


def _draw_int(shape, seed):
    cin, cout, H, W, N = shape
    gen = torch.Generator().manual_seed(seed)

    def draw(*s):
        return torch.randint(-3, 4, s, generator=gen).float()

    return draw(N, cin, H, W), draw(cout, cin, 3, 3), draw(cout), draw(N, cout, H // 2, W // 2)


def _window_counts(act):
    N, cout, H, W = act.shape
    win = act.unfold(2, 2, 2).unfold(3, 2, 2).reshape(N, cout, H // 2, W // 2, 4)
    top = win.max(dim=-1, keepdim=True).values
    tied = ((win == top).sum(dim=-1) > 1) & (top[..., 0] > 0)
    zero = top[..., 0] == 0
    return int(tied.sum()), int(zero.sum())


@functools.lru_cache(maxsize=None)
def _int_case(shape):
    """Small-integer inputs (every fp32 sum is exact) and their oracle."""
    x, w, b, g = _draw_int(shape, ELIGIBLE[shape])
    out, dx, dw, db, act = _oracle(x, w, b, g)
    tied, zero = _window_counts(act)
    return {
        'x': x, 'w': w, 'b': b, 'g': g,
        'out': out.float(), 'dx': dx.float(), 'dw': dw.float(), 'db': db.float(),
        'tied': tied, 'zero': zero,
    }  # fmt: skip


def _random_inputs(shape, seed):
    cin, cout, H, W, N = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, 3, 3, generator=gen) * 0.2
    b = torch.randn(cout, generator=gen) * 0.2
    g = torch.randn(N, cout, H // 2, W // 2, generator=gen)
    return x, w, b, g


def _run(x, w, b, g, weight_grad=False):
    """fwd, bwd_data (and bwd_weight) through the bindings on device tensors."""
    from dmlcloud_amd import _C

    N, cin, H, W = x.shape
    cout = w.shape[0]
    out = torch.full((N, cout, H // 2, W // 2), float('nan'), device=DEV)
    argmax = torch.full(out.shape, 0xAA, device=DEV, dtype=torch.uint8)
    din = torch.full(x.shape, float('nan'), device=DEV)
    _C.conv3x3_relu_pool_fwd(x, w, b, out, argmax)
    _C.conv3x3_relu_pool_bwd_data(g, argmax, w, din)
    res = {'out': out, 'argmax': argmax, 'din': din}
    if weight_grad:
        res['dw'], res['db'] = torch.empty_like(w), torch.empty_like(b)
        _C.conv3x3_relu_pool_bwd_weight(g, argmax, x, res['dw'], res['db'])
    torch.cuda.synchronize()
    return res


def _both_paths(monkeypatch, x, w, b, g):
    """The same device tensors through the default path and the forced VALU path."""
    monkeypatch.delenv(SWITCH, raising=False)
    new = _run(x, w, b, g)
    monkeypatch.setenv(SWITCH, '0')
    old = _run(x, w, b, g)
    monkeypatch.delenv(SWITCH, raising=False)
    return new, old


def _assert_paths_equal(new, old):
    # bit patterns, so that -0.0 against +0.0 would count as a difference
    assert torch.equal(new['out'].view(torch.int32), old['out'].view(torch.int32))
    assert torch.equal(new['argmax'], old['argmax'])
    assert torch.equal(new['din'].view(torch.int32), old['din'].view(torch.int32))


@pytest.mark.parametrize('shape', list(ELIGIBLE))
def test_integer_data_bitwise(shape, monkeypatch):
    """Integer data: out, dx, dw and db equal the float64 oracle exactly. The
    data hold tied windows and windows with pooled value 0, so the
    first-index rule and the gate bit are exercised."""
    assert ops.is_available()
    monkeypatch.delenv(SWITCH, raising=False)
    c = _int_case(shape)
    assert c['tied'] >= 1, 'data hold no tied window'
    assert c['zero'] >= 1, 'data hold no window with pooled value 0'
    r = _run(*(c[k].to(DEV) for k in 'xwbg'), weight_grad=True)
    assert torch.equal(r['out'].cpu(), c['out'])
    assert torch.equal(r['din'].cpu(), c['dx'])
    assert torch.equal(r['dw'].cpu(), c['dw'])
    assert torch.equal(r['db'].cpu(), c['db'])


@pytest.mark.parametrize('shape', list(ELIGIBLE))
def test_random_data_mfma_equals_valu(shape, monkeypatch):
    """Random data: the MFMA path reproduces the VALU path bit for bit."""
    x, w, b, g = (t.to(DEV) for t in _random_inputs(shape, seed=sum(shape)))
    new, old = _both_paths(monkeypatch, x, w, b, g)
    _assert_paths_equal(new, old)
    assert torch.isfinite(new['out']).all() and torch.isfinite(new['din']).all()


@pytest.mark.parametrize('shape', [(8, 16, 6, 10, 5), (16, 16, 14, 14, 3)])
def test_subnormals_and_signed_zeros(shape, monkeypatch):
    """Inputs scaled into the subnormal range, with some +0 and -0 among
    them: both paths keep subnormals and agree bit for bit."""
    x, w, b, g = _random_inputs(shape, seed=7 + sum(shape))
    gen = torch.Generator().manual_seed(11)
    scale = 2.0**-130
    x, b, g = x * scale, b * scale, g * scale
    for t in (x, w, g):
        flat = t.view(-1)
        idx = torch.randperm(flat.numel(), generator=gen)[: max(2, flat.numel() // 8)]
        flat[idx[::2]] = 0.0
        flat[idx[1::2]] = -0.0
    assert (x != 0).any() and (x.abs() < torch.finfo(torch.float32).tiny).all()
    new, old = _both_paths(monkeypatch, *(t.to(DEV) for t in (x, w, b, g)))
    _assert_paths_equal(new, old)
    tiny = torch.finfo(torch.float32).tiny
    for name in ('out', 'din'):
        v = new[name]
        assert ((v != 0) & (v.abs() < tiny)).any(), f'{name} holds no subnormal: flushed?'


def _view_in(buf, offset, shape):
    n = 1
    for s in shape:
        n *= s
    return buf[offset : offset + n].view(shape)


def _untouched_outside(buf, offset, numel, is_sentinel):
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    mask[offset : offset + numel] = False
    return bool(is_sentinel(buf[mask]).all())


@pytest.mark.parametrize('shape', [(8, 16, 6, 10, 5), (16, 16, 14, 14, 3)])
@pytest.mark.parametrize('off', [1, 2])
def test_unaligned_bases_and_margins(shape, off, monkeypatch):
    """x, dpooled, argmax, out and din are views at element offset `off` into
    larger buffers: offset 1 takes the scalar loads and stores, offset 2 the
    8-byte din pairs. Results equal the integer oracle and nothing outside
    the views is written."""
    from dmlcloud_amd import _C

    monkeypatch.delenv(SWITCH, raising=False)
    cin, cout, H, W, N = shape
    c = _int_case(shape)
    pad = 16
    nan = float('nan')

    def as_input(t):
        buf = torch.zeros(t.numel() + pad, device=DEV, dtype=t.dtype)
        view = _view_in(buf, off, t.shape)
        view.copy_(t)
        return view

    x, g = as_input(c['x']), as_input(c['g'])
    w, b = c['w'].to(DEV), c['b'].to(DEV)
    oshape = (N, cout, H // 2, W // 2)
    n_out, n_x = c['out'].numel(), c['x'].numel()
    out_buf = torch.full((n_out + pad,), nan, device=DEV)
    din_buf = torch.full((n_x + pad,), nan, device=DEV)
    arg_buf = torch.full((n_out + pad,), 0xAA, device=DEV, dtype=torch.uint8)
    out, argmax = _view_in(out_buf, off, oshape), _view_in(arg_buf, off, oshape)
    din = _view_in(din_buf, off, c['x'].shape)

    _C.conv3x3_relu_pool_fwd(x, w, b, out, argmax)
    _C.conv3x3_relu_pool_bwd_data(g, argmax, w, din)
    torch.cuda.synchronize()

    assert torch.equal(out.cpu(), c['out'])
    assert torch.equal(din.cpu(), c['dx'])
    assert _untouched_outside(out_buf, off, n_out, torch.isnan)
    assert _untouched_outside(din_buf, off, n_x, torch.isnan)
    assert _untouched_outside(arg_buf, off, n_out, lambda t: t == 0xAA)


@pytest.mark.parametrize('shape', INELIGIBLE)
def test_ineligible_shapes_ignore_the_switch(shape, monkeypatch):
    """Shapes outside COUT == 16, CIN in {4, 8, 12, 16} never take the MFMA
    path: the switch changes nothing."""
    x, w, b, g = (t.to(DEV) for t in _random_inputs(shape, seed=sum(shape)))
    new, old = _both_paths(monkeypatch, x, w, b, g)
    _assert_paths_equal(new, old)


def test_replay_is_bitwise(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    x, w, b, g = (t.to(DEV) for t in _random_inputs((16, 16, 14, 14, 3), seed=3))
    _assert_paths_equal(_run(x, w, b, g), _run(x, w, b, g))
