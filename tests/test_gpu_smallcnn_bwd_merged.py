"""smallcnn: layer 2's bwd_data and layer 1's bwd_weight in one kernel.

For a two-layer stack whose first layer needs no input gradient,
conv3x3_relu_pool_bwd_data_weight computes dw1/db1 from layer 2's pool
gradient without a din tensor. The MFMA phase, the gather's chains and the
workgroups' sample sequences are those of the two separate kernels, so the
results must agree under torch.equal with no tolerance.
DMLCLOUD_SMALLCNN_MERGE_BWD=0 forces the two-kernel path. The expected value
is always that path or float64 torch on the CPU, never the merged kernel.
`argmax1` and `argmax2` always come from the forward kernels.

Shapes are (CIN1, COUT1, H1, W1, N); layer 2 is COUT1 -> 16 on H1/2 x W1/2.
Run on an MI355X box: python -m pytest tests -m gpu
"""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MERGE = 'DMLCLOUD_SMALLCNN_MERGE_BWD'
MFMA = 'DMLCLOUD_SMALLCNN_MFMA'
CHUNK = 'DMLCLOUD_SMALLCNN_BWDW_CHUNK'
C2 = 16

# shape -> seed for which layer 1 holds a tied window with positive maximum
# and a window with pooled value 0 (searched on the CPU)
INT_SEEDS = {
    (1, 16, 4, 4, 1): 0,  # the smallest: layer 2 is 2x2 and pools to 1x1
    (1, 16, 28, 28, 3): 0,  # the workload's geometry
    (3, 8, 12, 20, 5): 0,  # H != W, odd PH2 = 3, inactive threads in the gather
    (16, 16, 8, 8, 2): 0,  # pairs == 256: one slice
}
# shape, chunk override
RANDOM_CASES = [(s, None) for s in INT_SEEDS] + [
    ((1, 16, 28, 28, 11), '4'),  # chunks of 4, 4 and 3
    ((1, 16, 4, 4, 2051), None),  # past the 2048-workgroup cap: three take a second chunk
    ((1, 16, 4, 4, 4099), '2'),  # 2050 chunks: the cap and a ragged last chunk
]


def _draw_int(shape, seed):
    cin, c1, H, W, N = shape
    gen = torch.Generator().manual_seed(seed)

    def draw(lo, hi, *s):
        return torch.randint(lo, hi + 1, s, generator=gen).float()

    # layer 2 sums 9 * c1 products of layer 1's outputs: keep its weights small
    return {
        'x': draw(-3, 3, N, cin, H, W),
        'w1': draw(-3, 3, c1, cin, 3, 3),
        'b1': draw(-3, 3, c1),
        'w2': draw(-2, 2, C2, c1, 3, 3),
        'b2': draw(-3, 3, C2),
        'g': draw(-3, 3, N, C2, H // 4, W // 4),
    }


def _window_counts(act):
    N, c, H, W = act.shape
    win = act.unfold(2, 2, 2).unfold(3, 2, 2).reshape(N, c, H // 2, W // 2, 4)
    top = win.max(dim=-1, keepdim=True).values
    tied = ((win == top).sum(dim=-1) > 1) & (top[..., 0] > 0)
    zero = top[..., 0] == 0
    return int(tied.sum()), int(zero.sum())


@functools.lru_cache(maxsize=None)
def _int_case(shape, seed=None):
    """Small-integer inputs (every fp32 sum is exact), the float64 oracle of
    dw1/db1 through both layers, and a bound on every partial sum."""
    c = _draw_int(shape, INT_SEEDS[shape] if seed is None else seed)
    x = c['x'].double()
    w1 = c['w1'].double().requires_grad_(True)
    b1 = c['b1'].double().requires_grad_(True)
    w2, b2 = c['w2'].double(), c['b2'].double()
    act1 = F.relu(F.conv2d(x, w1, b1, padding=1))
    pooled1 = F.max_pool2d(act1, 2)
    pooled1.retain_grad()
    act2 = F.relu(F.conv2d(pooled1, w2, b2, padding=1))
    act2.retain_grad()
    F.max_pool2d(act2, 2).backward(c['g'].double())
    # the largest sum of absolute values along any chain of either direction
    dconv2, din = act2.grad.abs(), pooled1.grad.abs()
    bound = max(
        float((F.conv2d(x.abs(), w1.detach().abs(), padding=1) + b1.detach().abs().view(1, -1, 1, 1)).max()),
        float((F.conv2d(pooled1.detach().abs(), w2.abs(), padding=1) + b2.abs().view(1, -1, 1, 1)).max()),
        float(F.conv_transpose2d(dconv2, w2.abs(), padding=1).max()),
        # |din| lands on one position of each window: spread it over all four
        float(
            torch.nn.grad.conv2d_weight(
                x.abs(), w1.shape, din.repeat_interleave(2, 2).repeat_interleave(2, 3), padding=1
            ).max()
        ),
        float(din.sum(dim=(0, 2, 3)).max()),
    )
    tied, zero = _window_counts(act1.detach())
    c.update(dw1=w1.grad.float(), db1=b1.grad.float(), tied=tied, zero=zero, bound=bound)
    return c


def _random_inputs(shape, seed):
    cin, c1, H, W, N = shape
    gen = torch.Generator().manual_seed(seed)
    return {
        'x': torch.randn(N, cin, H, W, generator=gen),
        'w1': torch.randn(c1, cin, 3, 3, generator=gen) * 0.2,
        'b1': torch.randn(c1, generator=gen) * 0.2,
        'w2': torch.randn(C2, c1, 3, 3, generator=gen) * 0.2,
        'b2': torch.randn(C2, generator=gen) * 0.2,
        'g': torch.randn(N, C2, H // 4, W // 4, generator=gen),
    }


def _forward(x, w1, b1, w2, b2, argmax1=None, argmax2=None):
    """Both forward kernels on device tensors: (argmax1, argmax2), written
    into the given tensors when there are any."""
    from dmlcloud_amd import _C

    N, _, H, W = x.shape
    pooled1 = torch.empty(N, w1.shape[0], H // 2, W // 2, device=DEV)
    if argmax1 is None:
        argmax1 = torch.empty(pooled1.shape, device=DEV, dtype=torch.uint8)
    _C.conv3x3_relu_pool_fwd(x, w1, b1, pooled1, argmax1)
    pooled2 = torch.empty(N, w2.shape[0], H // 4, W // 4, device=DEV)
    if argmax2 is None:
        argmax2 = torch.empty(pooled2.shape, device=DEV, dtype=torch.uint8)
    _C.conv3x3_relu_pool_fwd(pooled1, w2, b2, pooled2, argmax2)
    return argmax1, argmax2


def _nan_grads(w1_shape):
    return torch.full(tuple(w1_shape), float('nan'), device=DEV), torch.full((w1_shape[0],), float('nan'), device=DEV)


def _call(g, argmax2, w2, argmax1, x, w1_shape):
    """The launcher under the environment as it is."""
    from dmlcloud_amd import _C

    dw1, db1 = _nan_grads(w1_shape)
    _C.conv3x3_relu_pool_bwd_data_weight(g, argmax2, w2, argmax1, x, dw1, db1)
    torch.cuda.synchronize()
    return dw1, db1


def _two_kernels(g, argmax2, w2, argmax1, x, w1_shape):
    """The two existing launchers on a din tensor, under the environment as it is."""
    from dmlcloud_amd import _C

    N, _, H, W = x.shape
    din = torch.full((N, w1_shape[0], H // 2, W // 2), float('nan'), device=DEV)
    _C.conv3x3_relu_pool_bwd_data(g, argmax2, w2, din)
    dw1, db1 = _nan_grads(w1_shape)
    _C.conv3x3_relu_pool_bwd_weight(din, argmax1, x, dw1, db1)
    torch.cuda.synchronize()
    return dw1, db1


def _both_paths(monkeypatch, *args):
    """The same device tensors through the default path and with the merge switched off."""
    monkeypatch.delenv(MERGE, raising=False)
    new = _call(*args)
    monkeypatch.setenv(MERGE, '0')
    old = _call(*args)
    monkeypatch.delenv(MERGE, raising=False)
    return new, old


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _clean_env(monkeypatch):
    for name in (MERGE, MFMA, CHUNK):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize('shape', list(INT_SEEDS))
def test_integer_data_equals_oracle(shape, monkeypatch):
    """Integer data: dw1 and db1 equal the float64 oracle of the two-layer
    stack exactly. Layer 1 holds tied windows and windows with pooled value 0,
    so the first-index rule and the gate bit reach the gather's decode."""
    _clean_env(monkeypatch)
    c = _int_case(shape)
    print(f'{shape}: tied {c["tied"]} zero {c["zero"]} bound {c["bound"]:.0f}')
    assert c['bound'] < 2**24, 'a partial sum may be inexact in fp32'
    assert c['tied'] >= 1, 'layer 1 holds no tied window with positive maximum'
    assert c['zero'] >= 1, 'layer 1 holds no window with pooled value 0'
    x, w1, b1, w2, b2, g = (c[k].to(DEV) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'g'))
    argmax1, argmax2 = _forward(x, w1, b1, w2, b2)
    dw1, db1 = _call(g, argmax2, w2, argmax1, x, w1.shape)
    assert torch.equal(dw1.cpu(), c['dw1'])
    assert torch.equal(db1.cpu(), c['db1'])


@pytest.mark.parametrize('shape,chunk', RANDOM_CASES)
def test_random_data_merged_equals_two_kernel(shape, chunk, monkeypatch):
    """Random data: the merged kernel reproduces the two-kernel path with no
    tolerance, within a chunk, across chunks and past the workgroup cap."""
    _clean_env(monkeypatch)
    if chunk is not None:
        monkeypatch.setenv(CHUNK, chunk)
    c = {k: t.to(DEV) for k, t in _random_inputs(shape, seed=sum(shape)).items()}
    argmax1, argmax2 = _forward(c['x'], c['w1'], c['b1'], c['w2'], c['b2'])
    args = (c['g'], argmax2, c['w2'], argmax1, c['x'], c['w1'].shape)
    (dw1, db1), (dw0, db0) = _both_paths(monkeypatch, *args)
    assert torch.equal(dw1, dw0)
    assert torch.equal(db1, db0)
    assert torch.isfinite(dw1).all() and torch.isfinite(db1).all()
    # and the switched-off launcher is the two existing launchers
    dwk, dbk = _two_kernels(*args)
    assert _bits_equal(dw0, dwk) and _bits_equal(db0, dbk)


@pytest.mark.parametrize('shape', [(3, 8, 12, 20, 5), (1, 16, 28, 28, 3)])
def test_subnormals_and_signed_zeros(shape, monkeypatch):
    """The pool gradient scaled into the subnormal range, an eighth of
    dpooled2, w2 and x set to +0.0 or -0.0 and another eighth of w2 and x to
    subnormals: the paths agree bit for bit, signs of zeros included, and
    nothing is flushed."""
    _clean_env(monkeypatch)
    c = _random_inputs(shape, seed=7 + sum(shape))
    gen = torch.Generator().manual_seed(11)
    c['g'] = c['g'] * 2.0**-130
    for name in ('x', 'w2', 'g'):
        flat = c[name].view(-1)
        idx = torch.randperm(flat.numel(), generator=gen)
        eighth = flat.numel() // 8
        flat[idx[:eighth:2]] = 0.0
        flat[idx[1:eighth:2]] = -0.0
        if name != 'g':
            flat[idx[eighth : 2 * eighth]] *= 2.0**-140
    tiny = torch.finfo(torch.float32).tiny
    assert (c['g'] != 0).any() and (c['g'].abs() < tiny).all()
    for name in ('x', 'w2'):
        assert ((c[name] != 0) & (c[name].abs() < tiny)).any()
    c = {k: t.to(DEV) for k, t in c.items()}
    argmax1, argmax2 = _forward(c['x'], c['w1'], c['b1'], c['w2'], c['b2'])
    (dw1, db1), (dw0, db0) = _both_paths(monkeypatch, c['g'], argmax2, c['w2'], argmax1, c['x'], c['w1'].shape)
    assert torch.equal(dw1, dw0) and _bits_equal(dw1, dw0)
    assert torch.equal(db1, db0) and _bits_equal(db1, db0)
    assert ((dw1 != 0) & (dw1.abs() < tiny)).any(), 'dw1 holds no subnormal: flushed?'


def _view_at_1(t, dtype=None):
    buf = torch.zeros(t.numel() + 16, device=DEV, dtype=dtype or t.dtype)
    return buf[1 : 1 + t.numel()].view(t.shape)


@pytest.mark.parametrize('shape', [(3, 8, 12, 20, 5), (1, 16, 28, 28, 3)])
@pytest.mark.parametrize('which', ['dpooled2', 'argmax2', 'argmax1', 'x', 'all'])
def test_unaligned_bases(shape, which, monkeypatch):
    """One of dpooled2, argmax2, argmax1 and x (or all four) is a view one
    element into a larger buffer, which takes that operand's scalar loads:
    results equal the integer oracle."""
    _clean_env(monkeypatch)
    c = _int_case(shape)

    def off(name):
        return which in (name, 'all')

    x = _view_at_1(c['x']) if off('x') else torch.empty_like(c['x'], device=DEV)
    g = _view_at_1(c['g']) if off('dpooled2') else torch.empty_like(c['g'], device=DEV)
    x.copy_(c['x'])
    g.copy_(c['g'])
    w1, b1, w2, b2 = (c[k].to(DEV) for k in ('w1', 'b1', 'w2', 'b2'))
    N, cin, H, W = c['x'].shape
    am1 = torch.empty(N, w1.shape[0], H // 2, W // 2, device=DEV, dtype=torch.uint8)
    am2 = torch.empty(N, C2, H // 4, W // 4, device=DEV, dtype=torch.uint8)
    argmax1 = _view_at_1(am1) if off('argmax1') else am1
    argmax2 = _view_at_1(am2) if off('argmax2') else am2
    _forward(x, w1, b1, w2, b2, argmax1, argmax2)
    for name, t, align in (('x', x, 16), ('dpooled2', g, 16), ('argmax1', argmax1, 4), ('argmax2', argmax2, 4)):
        assert (t.data_ptr() % align != 0) == off(name)
    dw1, db1 = _call(g, argmax2, w2, argmax1, x, w1.shape)
    assert torch.equal(dw1.cpu(), c['dw1'])
    assert torch.equal(db1.cpu(), c['db1'])


def _view_in(buf, offset, shape):
    n = 1
    for s in shape:
        n *= s
    return buf[offset : offset + n].view(shape)


def _untouched_outside(buf, offset, numel, is_sentinel):
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    mask[offset : offset + numel] = False
    return bool(is_sentinel(buf[mask]).all())


@pytest.mark.parametrize('shape', [(3, 8, 12, 20, 5), (1, 16, 28, 28, 3)])
@pytest.mark.parametrize('out_off', [0, 1])
def test_canaries(shape, out_off, monkeypatch):
    """dw1 and db1 are views into NaN-filled buffers: every element is
    overwritten with the oracle's value and nothing outside the views is
    touched."""
    from dmlcloud_amd import _C

    _clean_env(monkeypatch)
    c = _int_case(shape)
    x, w1, b1, w2, b2, g = (c[k].to(DEV) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'g'))
    argmax1, argmax2 = _forward(x, w1, b1, w2, b2)
    pad = 16
    dw_buf = torch.full((w1.numel() + pad,), float('nan'), device=DEV)
    db_buf = torch.full((w1.shape[0] + pad,), float('nan'), device=DEV)
    dw1 = _view_in(dw_buf, out_off, w1.shape)
    db1 = _view_in(db_buf, out_off, (w1.shape[0],))
    _C.conv3x3_relu_pool_bwd_data_weight(g, argmax2, w2, argmax1, x, dw1, db1)
    torch.cuda.synchronize()
    assert torch.isfinite(dw1).all() and torch.isfinite(db1).all()
    assert torch.equal(dw1.cpu(), c['dw1'])
    assert torch.equal(db1.cpu(), c['db1'])
    assert _untouched_outside(dw_buf, out_off, w1.numel(), torch.isnan)
    assert _untouched_outside(db_buf, out_off, w1.shape[0], torch.isnan)


@pytest.mark.parametrize(
    'shape,env',
    [
        ((1, 32, 8, 8, 2), {}),  # COUT1 = 32: layer 2 is not on the MFMA path
        ((1, 16, 28, 28, 3), {MFMA: '0'}),
        ((3, 8, 12, 20, 5), {MFMA: '0'}),
        ((1, 16, 28, 28, 3), {MERGE: '0'}),
        ((3, 8, 12, 20, 5), {MERGE: '0'}),
    ],
)
def test_ineligible_shapes_and_switches_give_the_two_kernel_result(shape, env, monkeypatch):
    """Where there is no merged kernel, or a switch is off, the launcher's
    result is that of the two existing launchers under the same environment."""
    _clean_env(monkeypatch)
    c = {k: t.to(DEV) for k, t in _random_inputs(shape, seed=3 + sum(shape)).items()}
    argmax1, argmax2 = _forward(c['x'], c['w1'], c['b1'], c['w2'], c['b2'])
    args = (c['g'], argmax2, c['w2'], argmax1, c['x'], c['w1'].shape)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    dw1, db1 = _call(*args)
    dwk, dbk = _two_kernels(*args)
    assert torch.isfinite(dw1).all() and torch.isfinite(db1).all()
    assert _bits_equal(dw1, dwk) and _bits_equal(db1, dbk)


@pytest.mark.parametrize('value', [None, '0'])
def test_h1_of_6_is_refused_like_the_forward(value, monkeypatch):
    """H1 = 6 makes layer 2's plane 3 rows high. No forward kernel pools an
    odd plane (so no argmax2 exists for it) and the two backward launchers
    assume even planes without checking, so there is no two-kernel result to
    equal: the launcher refuses the shape under either switch value, as the
    forward does, and launches nothing."""
    from dmlcloud_amd import _C

    _clean_env(monkeypatch)
    if value is not None:
        monkeypatch.setenv(MERGE, value)
    N, cin, c1, H, W = 2, 1, 16, 6, 8
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, cin, H, W, generator=gen).to(DEV)
    w1 = torch.randn(c1, cin, 3, 3, generator=gen).to(DEV)
    b1 = torch.randn(c1, generator=gen).to(DEV)
    w2 = torch.randn(C2, c1, 3, 3, generator=gen).to(DEV)
    pooled1 = torch.empty(N, c1, H // 2, W // 2, device=DEV)
    argmax1 = torch.empty(pooled1.shape, device=DEV, dtype=torch.uint8)
    _C.conv3x3_relu_pool_fwd(x, w1, b1, pooled1, argmax1)
    pooled2 = torch.empty(N, C2, H // 4, W // 4, device=DEV)
    argmax2 = torch.zeros(pooled2.shape, device=DEV, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='must be even'):
        _C.conv3x3_relu_pool_fwd(pooled1, w2, torch.zeros(C2, device=DEV), pooled2, argmax2)
    dw1, db1 = _nan_grads(w1.shape)
    with pytest.raises(RuntimeError, match='multiples of 4'):
        _C.conv3x3_relu_pool_bwd_data_weight(torch.randn_like(pooled2), argmax2, w2, argmax1, x, dw1, db1)
    torch.cuda.synchronize()
    assert torch.isnan(dw1).all() and torch.isnan(db1).all()


@pytest.mark.parametrize('value', [None, '0'])
def test_empty_batch_gives_zeros(value, monkeypatch):
    _clean_env(monkeypatch)
    if value is not None:
        monkeypatch.setenv(MERGE, value)
    c1 = 16
    x = torch.empty(0, 1, 28, 28, device=DEV)
    argmax1 = torch.empty(0, c1, 14, 14, device=DEV, dtype=torch.uint8)
    g = torch.empty(0, C2, 7, 7, device=DEV)
    argmax2 = torch.empty(0, C2, 7, 7, device=DEV, dtype=torch.uint8)
    w2 = torch.randn(C2, c1, 3, 3, device=DEV)
    dw1, db1 = _call(g, argmax2, w2, argmax1, x, (c1, 1, 3, 3))
    assert torch.equal(dw1, torch.zeros_like(dw1))
    assert torch.equal(db1, torch.zeros_like(db1))


def _model_grads(model, x, y):
    model.zero_grad(set_to_none=True)
    F.cross_entropy(model(x), y).backward()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in model.parameters()]


@pytest.mark.parametrize('N', [8, 40])
def test_whole_model_gradients_equal_two_kernel_path(N, monkeypatch):
    """FusedMnistCNN: all six gradients with the merged backward equal those
    with the merge switched off."""
    from dmlcloud_amd.ops.fused_cnn import FusedMnistCNN

    _clean_env(monkeypatch)
    torch.manual_seed(N)
    model = FusedMnistCNN().to(DEV)
    x = torch.randn(N, 1, 28, 28, device=DEV)
    y = torch.randint(0, 10, (N,), device=DEV)
    new = _model_grads(model, x, y)
    monkeypatch.setenv(MERGE, '0')
    old = _model_grads(model, x, y)
    assert len(new) == 6
    for (name, _), a, b in zip(model.named_parameters(), new, old):
        assert torch.equal(a, b), name
        assert torch.isfinite(a).all(), name


def test_replayed_gradients_equal_eager(monkeypatch):
    """A captured forward+backward replayed on a second batch gives exactly
    the eager gradients of that batch."""
    from dmlcloud_amd.ops.fused_cnn import FusedMnistCNN

    _clean_env(monkeypatch)
    torch.manual_seed(0)
    model = FusedMnistCNN().to(DEV)
    eager = copy.deepcopy(model)
    batches = [(torch.randn(8, 1, 28, 28, device=DEV), torch.randint(0, 10, (8,), device=DEV)) for _ in range(2)]
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
        assert _bits_equal(p.grad, q.grad), name


def _good_args():
    N, c1 = 2, 16
    return {
        'dpooled2': torch.randn(N, C2, 7, 7, device=DEV),
        'argmax2': torch.zeros(N, C2, 7, 7, device=DEV, dtype=torch.uint8),
        'w2': torch.randn(C2, c1, 3, 3, device=DEV),
        'argmax1': torch.zeros(N, c1, 14, 14, device=DEV, dtype=torch.uint8),
        'x': torch.randn(N, 1, 28, 28, device=DEV),
    }


BAD_ARGS = {
    'dpooled2 dtype': lambda a: a.update(dpooled2=a['dpooled2'].double()),
    'x dtype': lambda a: a.update(x=a['x'].half()),
    'argmax1 dtype': lambda a: a.update(argmax1=a['argmax1'].to(torch.int32)),
    'argmax2 dtype': lambda a: a.update(argmax2=a['argmax2'].float()),
    'w2 on the cpu': lambda a: a.update(w2=a['w2'].cpu()),
    'x on the cpu': lambda a: a.update(x=a['x'].cpu()),
    'argmax1 on the cpu': lambda a: a.update(argmax1=a['argmax1'].cpu()),
    'dpooled2 not contiguous': lambda a: a.update(dpooled2=a['dpooled2'].transpose(2, 3)),
    'x not contiguous': lambda a: a.update(x=a['x'].transpose(2, 3)),
    'argmax1 not contiguous': lambda a: a.update(argmax1=a['argmax1'].transpose(2, 3)),
    'dpooled2 shape': lambda a: a.update(dpooled2=a['dpooled2'][:, :, :6].contiguous()),
    'argmax2 shape': lambda a: a.update(argmax2=a['argmax2'][:1].contiguous()),
    'argmax1 shape': lambda a: a.update(argmax1=a['argmax1'][:, :8].contiguous()),
    'w2 shape': lambda a: a.update(w2=a['w2'][:, :8].contiguous()),
    'x shape': lambda a: a.update(x=a['x'][:1].contiguous()),
}


@pytest.mark.parametrize('case', list(BAD_ARGS))
@pytest.mark.parametrize('value', [None, '0'])
def test_argument_checks(case, value, monkeypatch):
    """A wrong dtype, a CPU tensor, a non-contiguous tensor or a mismatched
    shape raises under either switch value and launches nothing."""
    from dmlcloud_amd import _C

    _clean_env(monkeypatch)
    if value is not None:
        monkeypatch.setenv(MERGE, value)
    a = _good_args()
    BAD_ARGS[case](a)
    dw1, db1 = _nan_grads((16, 1, 3, 3))
    with pytest.raises(RuntimeError):
        _C.conv3x3_relu_pool_bwd_data_weight(a['dpooled2'], a['argmax2'], a['w2'], a['argmax1'], a['x'], dw1, db1)
    torch.cuda.synchronize()
    assert torch.isnan(dw1).all() and torch.isnan(db1).all()


def test_bad_outputs_are_refused(monkeypatch):
    """dw1 / db1 of the wrong shape, dtype or device raise too."""
    from dmlcloud_amd import _C

    _clean_env(monkeypatch)
    a = _good_args()
    args = (a['dpooled2'], a['argmax2'], a['w2'], a['argmax1'], a['x'])
    dw1, db1 = _nan_grads((16, 1, 3, 3))
    for bad_dw, bad_db in [
        (dw1[:8].contiguous(), db1),
        (dw1, db1[:8].contiguous()),
        (dw1.double(), db1),
        (dw1, db1.cpu()),
    ]:
        with pytest.raises(RuntimeError):
            _C.conv3x3_relu_pool_bwd_data_weight(*args, bad_dw, bad_db)
    torch.cuda.synchronize()
    assert torch.isnan(dw1).all() and torch.isnan(db1).all()
