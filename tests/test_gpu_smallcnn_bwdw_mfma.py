"""smallcnn bwd_weight as an f32 MFMA implicit GEMM (COUT == CIN == 16).

At COUT == CIN == 16 every (co, ci, tap) of the VALU kernel is one serial
fmaf chain over the workgroup's samples and cells; the MFMA form runs the
same chains with three added fmaf(+0, x, acc) per step, so the two paths
must agree under torch.equal with no tolerance. DMLCLOUD_SMALLCNN_MFMA=0
forces the VALU kernel. The oracle for the integer cases is float64 torch on
the CPU. `argmax` always comes from the forward kernel.
Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SWITCH = 'DMLCLOUD_SMALLCNN_MFMA'
CHUNK = 'DMLCLOUD_SMALLCNN_BWDW_CHUNK'

# (CIN, COUT, H, W, N) -> seed for which the integer data hold a tied window
# and a window with pooled value 0 (searched on the CPU)
INT_SEEDS = {
    (16, 16, 2, 2, 1): 7,  # one window, one k-step
    (16, 16, 4, 4, 1): 2,
    (16, 16, 6, 10, 5): 0,  # H != W, odd PH
    (16, 16, 14, 14, 3): 0,  # the workload's geometry
}
# shape, chunk override: the chain spans samples and chunks
RANDOM_CASES = [(s, None) for s in INT_SEEDS] + [
    ((16, 16, 14, 14, 11), '4'),  # chunks of 4, 4 and 3: ragged last chunk
    ((16, 16, 14, 14, 2051), None),  # past the 2048-workgroup cap: three take a second chunk
    ((16, 16, 4, 4, 4099), '2'),  # 2050 chunks: the cap and a ragged last chunk
]
INELIGIBLE = [(4, 16, 8, 8, 2), (12, 16, 8, 8, 2), (1, 16, 28, 28, 2), (16, 32, 8, 8, 2)]


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
    """Small-integer inputs (every fp32 sum is exact) and their float64 oracle."""
    x, w, b, g = _draw_int(shape, INT_SEEDS[shape])
    wd = w.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    act = F.relu(F.conv2d(x.double(), wd, bd, padding=1))
    F.max_pool2d(act, 2).backward(g.double())
    tied, zero = _window_counts(act.detach())
    return {'x': x, 'w': w, 'b': b, 'g': g, 'dw': wd.grad.float(), 'db': bd.grad.float(),
            'tied': tied, 'zero': zero}  # fmt: skip


def _random_inputs(shape, seed):
    cin, cout, H, W, N = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, 3, 3, generator=gen) * 0.2
    b = torch.randn(cout, generator=gen) * 0.2
    g = torch.randn(N, cout, H // 2, W // 2, generator=gen)
    return x, w, b, g


def _argmax_of(x, w, b, argmax=None):
    """The forward kernel's argmax bytes for device tensors x, w, b."""
    from dmlcloud_amd import _C

    N, _, H, W = x.shape
    out = torch.empty(N, w.shape[0], H // 2, W // 2, device=DEV)
    if argmax is None:
        argmax = torch.empty(out.shape, device=DEV, dtype=torch.uint8)
    _C.conv3x3_relu_pool_fwd(x, w, b, out, argmax)
    return argmax


def _bwd_weight(g, argmax, x, w):
    from dmlcloud_amd import _C

    dw = torch.full(w.shape, float('nan'), device=DEV)
    db = torch.full((w.shape[0],), float('nan'), device=DEV)
    _C.conv3x3_relu_pool_bwd_weight(g, argmax, x, dw, db)
    torch.cuda.synchronize()
    return dw, db


def _both_paths(monkeypatch, g, argmax, x, w):
    """The same device tensors through the default path and the forced VALU path."""
    monkeypatch.delenv(SWITCH, raising=False)
    new = _bwd_weight(g, argmax, x, w)
    monkeypatch.setenv(SWITCH, '0')
    old = _bwd_weight(g, argmax, x, w)
    monkeypatch.delenv(SWITCH, raising=False)
    return new, old


@pytest.mark.parametrize('shape', list(INT_SEEDS))
def test_integer_data_equals_oracle(shape, monkeypatch):
    """Integer data: dw and db equal the float64 oracle exactly. The data hold
    tied windows and windows with pooled value 0, so the first-index rule and
    the gate bit reach the A operand."""
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv(CHUNK, raising=False)
    c = _int_case(shape)
    assert c['tied'] >= 1, 'data hold no tied window'
    assert c['zero'] >= 1, 'data hold no window with pooled value 0'
    x, w, b, g = (c[k].to(DEV) for k in 'xwbg')
    dw, db = _bwd_weight(g, _argmax_of(x, w, b), x, w)
    assert torch.equal(dw.cpu(), c['dw'])
    assert torch.equal(db.cpu(), c['db'])


@pytest.mark.parametrize('shape,chunk', RANDOM_CASES)
def test_random_data_mfma_equals_valu(shape, chunk, monkeypatch):
    """Random data: the MFMA path reproduces the VALU path with no tolerance,
    within a chunk, across chunks and past the workgroup cap."""
    if chunk is None:
        monkeypatch.delenv(CHUNK, raising=False)
    else:
        monkeypatch.setenv(CHUNK, chunk)
    x, w, b, g = (t.to(DEV) for t in _random_inputs(shape, seed=sum(shape)))
    (dw, db), (dw0, db0) = _both_paths(monkeypatch, g, _argmax_of(x, w, b), x, w)
    assert torch.equal(dw, dw0)
    assert torch.equal(db, db0)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()


@pytest.mark.parametrize('shape', [(16, 16, 6, 10, 5), (16, 16, 14, 14, 3)])
def test_subnormals_and_signed_zeros(shape, monkeypatch):
    """Gradients scaled into the subnormal range against inputs of order 1,
    an eighth of both set to +0.0 or -0.0: the paths agree in value (a chain
    at -0.0 may come out +0.0 in the dense form, so no bit-pattern view) and
    nothing is flushed."""
    monkeypatch.delenv(CHUNK, raising=False)
    x, w, b, g = _random_inputs(shape, seed=7 + sum(shape))
    gen = torch.Generator().manual_seed(11)
    g = g * 2.0**-130
    for t in (x, g):
        flat = t.view(-1)
        idx = torch.randperm(flat.numel(), generator=gen)[: flat.numel() // 8]
        flat[idx[::2]] = 0.0
        flat[idx[1::2]] = -0.0
    tiny = torch.finfo(torch.float32).tiny
    assert (g != 0).any() and (g.abs() < tiny).all()
    x, w, b, g = (t.to(DEV) for t in (x, w, b, g))
    (dw, db), (dw0, db0) = _both_paths(monkeypatch, g, _argmax_of(x, w, b), x, w)
    assert torch.equal(dw, dw0)
    assert torch.equal(db, db0)
    assert ((dw != 0) & (dw.abs() < tiny)).any(), 'dw holds no subnormal: flushed?'


@pytest.mark.parametrize('shape', [(16, 16, 6, 10, 5), (16, 16, 14, 14, 3)])
def test_unaligned_bases(shape, monkeypatch):
    """x, dpooled and argmax are views at element offset 1 into larger
    buffers, which takes the scalar loads: results equal the integer oracle."""
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv(CHUNK, raising=False)
    c = _int_case(shape)

    def view_at_1(t, dtype=None):
        buf = torch.zeros(t.numel() + 16, device=DEV, dtype=dtype or t.dtype)
        return buf[1 : 1 + t.numel()].view(t.shape)

    x, g = view_at_1(c['x']), view_at_1(c['g'])
    x.copy_(c['x'])
    g.copy_(c['g'])
    w, b = c['w'].to(DEV), c['b'].to(DEV)
    argmax = _argmax_of(x, w, b, view_at_1(c['g'], torch.uint8))
    assert x.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 4 and argmax.data_ptr() % 4 == 1
    dw, db = _bwd_weight(g, argmax, x, w)
    assert torch.equal(dw.cpu(), c['dw'])
    assert torch.equal(db.cpu(), c['db'])


@pytest.mark.parametrize('shape', INELIGIBLE)
def test_ineligible_shapes_ignore_the_switch(shape, monkeypatch):
    """Only COUT == CIN == 16 takes the MFMA form; elsewhere the switch
    changes no bit. bwd_weight has no kernel for COUT * CIN > 256, which
    (16, 32, 8, 8, 2) is: there the switch must not change the refusal."""
    monkeypatch.delenv(CHUNK, raising=False)
    cin, cout = shape[:2]
    x, w, b, g = (t.to(DEV) for t in _random_inputs(shape, seed=sum(shape)))
    argmax = _argmax_of(x, w, b)
    if cin * cout > 256:
        for value in (None, '0'):
            monkeypatch.delenv(SWITCH, raising=False)
            if value is not None:
                monkeypatch.setenv(SWITCH, value)
            with pytest.raises(RuntimeError, match='COUT\\*CIN <= 256'):
                _bwd_weight(g, argmax, x, w)
        return
    (dw, db), (dw0, db0) = _both_paths(monkeypatch, g, argmax, x, w)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert torch.equal(dw.view(torch.int32), dw0.view(torch.int32))
    assert torch.equal(db.view(torch.int32), db0.view(torch.int32))


def test_replay_is_bitwise(monkeypatch):
    """Two calls on the same tensors give equal bits."""
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv(CHUNK, raising=False)
    x, w, b, g = (t.to(DEV) for t in _random_inputs((16, 16, 14, 14, 37), seed=3))
    argmax = _argmax_of(x, w, b)
    dw, db = _bwd_weight(g, argmax, x, w)
    dw1, db1 = _bwd_weight(g, argmax, x, w)
    assert torch.equal(dw.view(torch.int32), dw1.view(torch.int32))
    assert torch.equal(db.view(torch.int32), db1.view(torch.int32))
