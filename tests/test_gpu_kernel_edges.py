"""Edge-shape fp64 differential tests for the LayerNorm, cross-entropy,
reduce, copy and flat-optimizer kernels.

Every case feeds a kernel bf16/fp32 inputs, evaluates the same operation in
fp64 on the CPU from those inputs, and compares the kernel's raw outputs
(lse, per-row loss, mean, rstd, moments, step counter included) under a
bound that is either a rounding model or measured on torch's fp32 CPU path.
No bound is taken from the kernels. `2^-8 |ref|` is the half-ulp of one
round-to-nearest bf16 store, `2^-24 |ref|` that of an fp32 store.

Shapes are the smallest that reach a code path: one-vector edges, scalar
tails, idle waves, and the first size at which a capped grid starts to
stride. Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools
import math

import pytest
import torch

from dmlcloud_amd import ops
from dmlcloud_amd.ops import OP_MAX, OP_MIN, OP_SUM
from dmlcloud_amd.ops import _reference as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BF16_HALF_ULP = 2.0**-8
FP32_HALF_ULP = 2.0**-24
FP32_MIN_NORMAL = 2.0**-126
SENTINEL = -12345.0


def _C():
    assert ops.is_available(), 'native extension must be present on a GPU box'
    from dmlcloud_amd import _C as ext

    return ext


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _assert_within(got, want, bound, what):
    """|got - want| <= bound elementwise (fp64, CPU); NaN in `got` fails."""
    got, want, bound = got.double(), want.double(), bound.double().expand_as(want)
    err = (got - want).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = int(torch.where(bad.flatten(), err.flatten() / bound.flatten().clamp_min(1e-300), -1.0).argmax())
        pytest.fail(
            f'{what}: {int(bad.sum())} of {bad.numel()} outside the bound; worst at flat index {i}: '
            f'got {got.flatten()[i].item():.9g}, want {want.flatten()[i].item():.9g}, '
            f'bound {bound.flatten()[i].item():.3g}'
        )


# ------------------------------------------------------------------ LayerNorm

LN_EPS = 1e-5
LN_RSTD_RTOL = 1e-5


def _ln_inputs(R, D, seed, offset=0.0, std=1.0):
    g = _gen(seed)
    x = (offset + std * torch.randn(R, D, generator=g)).to(torch.bfloat16)
    gamma = torch.randn(D, generator=g).to(torch.bfloat16)
    beta = torch.randn(D, generator=g).to(torch.bfloat16)
    return x, gamma, beta


def _ln_ref(x, gamma, beta):
    """fp64 LayerNorm of bf16 inputs: y, mean, rstd, xhat."""
    xd = x.double()
    mean = xd.mean(-1)
    var = (xd - mean[:, None]).square().mean(-1)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(LN_EPS, dtype=torch.float32)))
    xhat = (xd - mean[:, None]) * rstd[:, None]
    return xhat * gamma.double() + beta.double(), mean, rstd, xhat


def _ln_forward(x, gamma, beta, slack_rows=3):
    """Run _C.layernorm_fwd with sentinel-filled slack behind the R rows of
    y, mean and rstd; asserts the slack untouched. Returns device tensors."""
    R, D = x.shape
    y_buf = torch.full(((R + slack_rows) * D,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    mean_buf = torch.full((R + slack_rows,), SENTINEL, dtype=torch.float32, device=DEV)
    rstd_buf = torch.full((R + slack_rows,), SENTINEL, dtype=torch.float32, device=DEV)
    y = y_buf[: R * D].view(R, D)
    _C().layernorm_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV), y, mean_buf, rstd_buf, LN_EPS)
    torch.cuda.synchronize()
    sent_bf16 = torch.tensor(SENTINEL, dtype=torch.bfloat16).item()
    assert (y_buf[R * D :] == sent_bf16).all(), 'y slack overwritten'
    assert (mean_buf[R:] == SENTINEL).all(), 'mean slack overwritten'
    assert (rstd_buf[R:] == SENTINEL).all(), 'rstd slack overwritten'
    return y, mean_buf[:R], rstd_buf[:R]


def _check_ln_forward(x, gamma, beta, y, mean, rstd):
    """The forward bounds, written once.

    y:    2^-8 |ref| for the bf16 store + 2^-18 (|xhat gamma| + |beta|) for
          the fp32 arithmetic before it.
    mean: 2^-20 max|x_row| (fp32 sum of <= 2048 terms, one division).
    rstd: relative 1e-5. torch's fp32 native_layer_norm deviates from fp64
          by <= 1.2e-6 on these rows (printed by
          test_ln_forward_offset_rows; the bound stays >= 8x that).
    """
    y_ref, mean_ref, rstd_ref, xhat = _ln_ref(x, gamma, beta)
    _assert_within(mean.cpu(), mean_ref, 2.0**-20 * x.double().abs().amax(-1), 'mean')
    _assert_within(rstd.cpu(), rstd_ref, LN_RSTD_RTOL * rstd_ref, 'rstd')
    bound = BF16_HALF_ULP * y_ref.abs() + 2.0**-18 * ((xhat * gamma.double()).abs() + beta.double().abs())
    _assert_within(y.cpu(), y_ref, bound, 'y')


@pytest.mark.parametrize('R,D', [(1, 8), (3, 8), (5, 512), (7, 520), (4, 2048), (37, 1536), (8197, 64)])
def test_ln_forward_edge_shapes(R, D):
    """R < 4 leaves waves idle; D = 8/512/520 put a lane on or just past the
    one-vector edge; D = 2048 fills all four vectors; R = 8197 > 4 * 2048
    rows makes the row loop iterate."""
    x, gamma, beta = _ln_inputs(R, D, seed=R * 10007 + D)
    _check_ln_forward(x, gamma, beta, *_ln_forward(x, gamma, beta))


@pytest.mark.parametrize('offset,std', [(0.0, 1.0), (64.0, 1.0), (256.0, 2.0), (1024.0, 8.0)])
def test_ln_forward_offset_rows(offset, std):
    """Rows whose mean is far from 0: E[x^2] - mean^2 in fp32 loses the
    variance (rstd off by 1.5e-3 at mean 256, std 2); the two-pass variance
    does not. Also prints torch's own fp32 deviation, which the rstd bound
    has to stay >= 8x of."""
    R, D = 64, 768
    x, gamma, beta = _ln_inputs(R, D, seed=int(offset) + 1, offset=offset, std=std)
    _, _, rstd_ref, _ = _ln_ref(x, gamma, beta)
    _, _, rstd32 = torch.native_layer_norm(x.float(), (D,), gamma.float(), beta.float(), LN_EPS)
    torch_dev = ((rstd32.flatten().double() - rstd_ref).abs() / rstd_ref).max().item()
    print(f'torch fp32 native_layer_norm rstd deviation at offset {offset}, std {std}: {torch_dev:.3g}')
    assert LN_RSTD_RTOL >= 8 * torch_dev
    _check_ln_forward(x, gamma, beta, *_ln_forward(x, gamma, beta))


def test_ln_forward_constant_row():
    """A constant row has var = 0: rstd = 1/sqrt(eps) and y = beta bit-exact."""
    R, D = 5, 768
    x, gamma, beta = _ln_inputs(R, D, seed=5)
    x[2] = 3.140625  # exact in bf16
    y, mean, rstd = _ln_forward(x, gamma, beta)
    _check_ln_forward(x, gamma, beta, y, mean, rstd)
    eps32 = float(torch.tensor(LN_EPS, dtype=torch.float32))
    assert rstd[2].item() == pytest.approx(1.0 / math.sqrt(eps32), rel=LN_RSTD_RTOL)
    assert torch.equal(y[2].cpu().view(torch.int16), beta.view(torch.int16))


def check_ln_backward(x, gamma, beta, dy, dx, dgamma, dbeta, dx_ref, dgamma_ref, dbeta_ref):
    """The backward bounds, written once (CPU tensors; references fp64).

    dx:            2^-8 |ref| + 2^-18 rstd (|a| + |s1| + |xhat s2|), with
                   a = dy gamma, s1 = mean(a), s2 = mean(a xhat) as in the
                   kernel.
    dgamma, dbeta: 2^-8 |ref| + 2^-19 sum_r |term| per column (fp32
                   summation depth <= R/1024 + 16 for R <= 2100).
    """
    _, _, rstd_ref, xhat = _ln_ref(x, gamma, beta)
    a = dy.double() * gamma.double()
    s1 = a.mean(-1, keepdim=True)
    s2 = (a * xhat).mean(-1, keepdim=True)
    dx_bound = BF16_HALF_ULP * dx_ref.abs() + 2.0**-18 * rstd_ref[:, None] * (a.abs() + s1.abs() + (xhat * s2).abs())
    _assert_within(dx, dx_ref, dx_bound, 'dx')
    dg_bound = BF16_HALF_ULP * dgamma_ref.abs() + 2.0**-19 * (dy.double() * xhat).abs().sum(0)
    _assert_within(dgamma, dgamma_ref, dg_bound, 'dgamma')
    db_bound = BF16_HALF_ULP * dbeta_ref.abs() + 2.0**-19 * dy.double().abs().sum(0)
    _assert_within(dbeta, dbeta_ref, db_bound, 'dbeta')


def _ln_backward(x, gamma, dy, mean, rstd):
    R, D = x.shape
    dx = torch.empty(R, D, dtype=torch.bfloat16, device=DEV)
    # NaN-filled: the launcher claims the workspace needs no memset
    dgb_ws = torch.full((256 * 2 * D,), float('nan'), dtype=torch.float32, device=DEV)
    dgamma = torch.empty(D, dtype=torch.bfloat16, device=DEV)
    dbeta = torch.empty(D, dtype=torch.bfloat16, device=DEV)
    _C().layernorm_bwd(dy.to(DEV), x.to(DEV), mean, rstd, gamma.to(DEV), dx, dgb_ws, dgamma, dbeta)
    torch.cuda.synchronize()
    return dx.cpu(), dgamma.cpu(), dbeta.cpu()


@pytest.mark.parametrize('R,D', [(1, 8), (3, 520), (5, 2048), (1029, 64), (2051, 256)])
def test_ln_backward_edge_shapes(R, D):
    """fp64 autograd against the kernel fed its own forward statistics.
    R > 1024 makes a wave carry its dgamma/dbeta accumulators over several
    rows; D = 2048 asks for exactly 65,536 B of dynamic LDS. Bounds:
    check_ln_backward. Two calls must agree bitwise."""
    x, gamma, beta = _ln_inputs(R, D, seed=R * 7919 + D)
    dy = torch.randn(R, D, generator=_gen(R + D)).to(torch.bfloat16)
    _, mean, rstd = _ln_forward(x, gamma, beta)

    xd = x.double().requires_grad_(True)
    gd = gamma.double().requires_grad_(True)
    bd = beta.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xd, (D,), gd, bd, float(torch.tensor(LN_EPS, dtype=torch.float32))).backward(
        dy.double()
    )

    dx, dgamma, dbeta = _ln_backward(x, gamma, dy, mean, rstd)
    assert torch.isfinite(dgamma.float()).all() and torch.isfinite(dbeta.float()).all()

    check_ln_backward(x, gamma, beta, dy, dx, dgamma, dbeta, xd.grad, gd.grad, bd.grad)

    dx2, dgamma2, dbeta2 = _ln_backward(x, gamma, dy, mean, rstd)
    assert torch.equal(dgamma.view(torch.int16), dgamma2.view(torch.int16))
    assert torch.equal(dbeta.view(torch.int16), dbeta2.view(torch.int16))
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16))


def test_ln_backward_rejects_fp32_dy():
    """A fp32 dy must raise, not be read as bf16."""
    R, D = 4, 64
    x, gamma, beta = _ln_inputs(R, D, seed=0)
    _, mean, rstd = _ln_forward(x, gamma, beta)
    dx = torch.empty(R, D, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(256 * 2 * D, dtype=torch.float32, device=DEV)
    dg = torch.empty(D, dtype=torch.bfloat16, device=DEV)
    db = torch.empty(D, dtype=torch.bfloat16, device=DEV)
    dy32 = torch.randn(R, D, device=DEV)
    with pytest.raises(RuntimeError):
        _C().layernorm_bwd(dy32, x.to(DEV), mean, rstd, gamma.to(DEV), dx, ws, dg, db)


# -------------------------------------------------------------- cross-entropy

CE_FWD_SHAPES = [(3, 1), (5, 7), (4, 8), (9, 1003), (6, 2063), (128, 50257), (2051, 24)]
CE_BWD_SHAPES = CE_FWD_SHAPES + [(1030, 4104), (64, 50257)]
IGNORE = -100


def ce_reference(logits, targets):
    """fp64 cross-entropy of bf16 logits on the CPU: lse, per-row loss
    (garbage where the target is ignored), softmax p, and tol_lse = 16 x the
    largest deviation of fp32 torch.logsumexp (CPU) from fp64 on these rows.
    The margin of 16 is for the hardware exp2/log2 approximations against
    libm. tol_lse comes from the reference alone, never from the kernel."""
    xd = logits.double()
    lse = torch.logsumexp(xd, -1)
    loss = lse - xd.gather(1, targets.clamp_min(0)[:, None]).squeeze(1)
    p = torch.exp(xd - lse[:, None])
    tol_lse = 16 * (torch.logsumexp(logits.float(), -1).double() - lse).abs().max().item()
    return lse, loss, p, tol_lse


def ce_grad_reference(logits, targets, upstream=1.0, ignore_index=-100):
    """fp64 dlogits of upstream * mean-CE over the non-ignored rows, and the
    per-element bound, written once:

        |err| <= (2^-8 + 4 tol_lse) |ref| + 4 tol_lse |scale| p_ref

    plus 2^-126 (1 + |scale|): below the smallest normal fp32 the hardware
    exp flushes p to zero and the bf16 store of p * scale is subnormal, which
    no relative bound can express. No flat atol. Ignored rows have reference
    and bound 0. Returns grad_ref, bound, the fp64 mean loss and tol_lse."""
    _, loss_rows, p, tol_lse = ce_reference(logits, targets)
    valid = targets != ignore_index
    n_valid = int(valid.sum())
    scale = upstream / n_valid
    onehot = torch.zeros_like(p)
    onehot[valid, targets[valid]] = 1.0
    grad_ref = (p - onehot) * scale * valid[:, None]
    bound = (BF16_HALF_ULP + 4 * tol_lse) * grad_ref.abs() + 4 * tol_lse * abs(scale) * p
    bound = (bound + FP32_MIN_NORMAL * (1 + abs(scale))) * valid[:, None]
    return grad_ref, bound, loss_rows[valid].sum() / n_valid, tol_lse


@functools.lru_cache(maxsize=None)
def _ce_case(R, V):
    """bf16 logits with rows scaled by 3 and by 30 alternately; row 0 has
    half its vocabulary masked to -inf, row 1 everything but the target.
    Read-only: callers clone."""
    g = _gen(R * 100003 + V)
    scale = torch.where(torch.arange(R) % 2 == 0, 3.0, 30.0)[:, None]
    logits = (torch.randn(R, V, generator=g) * scale).to(torch.bfloat16)
    targets = torch.randint(0, V, (R,), generator=g)
    if V > 1:
        mask = torch.rand(V, generator=g) < 0.5
        mask[targets[0]] = False
        logits[0, mask] = float('-inf')
        keep = logits[1, targets[1]].clone()
        logits[1] = float('-inf')
        logits[1, targets[1]] = keep
    return logits, targets


@pytest.mark.parametrize('R,V', CE_FWD_SHAPES)
def test_ce_forward_rows(R, V):
    """Per-row loss and lse of _C.ce_fwd within tol_lse. V < 8 and
    V % 8 != 0 run the scalar tail; R = 2051 > kMaxGrid makes the row loop
    iterate."""
    logits, targets = _ce_case(R, V)
    lse_ref, loss_ref, _, tol_lse = ce_reference(logits, targets)
    print(f'tol_lse at ({R}, {V}): {tol_lse:.3g}')
    loss = torch.full((R + 2,), SENTINEL, dtype=torch.float32, device=DEV)
    lse = torch.full((R + 2,), SENTINEL, dtype=torch.float32, device=DEV)
    _C().ce_fwd(logits.to(DEV), targets.to(DEV), loss, lse, IGNORE)
    torch.cuda.synchronize()
    assert (loss[R:] == SENTINEL).all() and (lse[R:] == SENTINEL).all()
    tol = torch.tensor(tol_lse, dtype=torch.float64)
    _assert_within(lse[:R].cpu(), lse_ref, tol, 'lse')
    _assert_within(loss[:R].cpu(), loss_ref, tol, 'loss')
    if V > 1:
        assert loss[1].item() == 0.0, 'a row with only its target unmasked has loss 0'


@pytest.mark.parametrize('R,V', CE_BWD_SHAPES)
def test_ce_backward_scaled_and_ignored(R, V):
    """(3 * loss).backward() through cross_entropy with every third target
    ignored, under ce_grad_reference's bound. (1030, 4104) makes
    ce_bwd_kernel stride (R * V/8 > 524,288)."""
    from dmlcloud_amd.ops.fused_loss import cross_entropy

    logits, targets = _ce_case(R, V)
    targets = targets.clone()
    targets[2::3] = IGNORE  # rows 0 and 1 (the masked ones) stay valid
    grad_ref, bound, mean_ref, tol_lse = ce_grad_reference(logits, targets, upstream=3.0, ignore_index=IGNORE)

    x = logits.to(DEV).requires_grad_(True)
    loss = cross_entropy(x, targets.to(DEV), ignore_index=IGNORE)
    (3 * loss).backward()
    grad = x.grad.cpu()

    # the mean sums <= 2051 fp32 row losses
    assert abs(loss.item() - mean_ref.item()) <= tol_lse + 2.0**-20 * abs(mean_ref.item())
    assert (grad[targets == IGNORE] == 0).all(), 'ignored rows must have exactly zero gradient'
    _assert_within(grad, grad_ref, bound, 'dlogits')
    if V > 1:
        assert (grad[1] == 0).all(), 'a row with only its target unmasked has gradient 0'


# --------------------------------------------------------------------- reduce

OPS3 = [OP_SUM, OP_MIN, OP_MAX]


def _acc_init(op, dtype=torch.float64):
    if dtype == torch.int64:
        info = torch.iinfo(torch.int64)
        return {OP_SUM: 0, OP_MIN: info.max, OP_MAX: info.min}[op]
    return {OP_SUM: 0.0, OP_MIN: float('inf'), OP_MAX: float('-inf')}[op]


def _reduce_both(value, op, acc_dtype=torch.float64, init=None):
    """metric_reduce_into on the device and ops/_reference.py on the CPU,
    from the same accumulator start."""
    init = _acc_init(op, acc_dtype) if init is None else init
    acc_ref = torch.full((1,), init, dtype=acc_dtype)
    acc_dev = acc_ref.to(DEV)
    cnt_ref = torch.zeros(1, dtype=torch.int64)
    cnt_dev = cnt_ref.to(DEV)
    ref.reduce_into_acc(value, acc_ref, cnt_ref, op)
    ops.metric_reduce_into(value.to(DEV), acc_dev, cnt_dev, op)
    assert cnt_dev.item() == cnt_ref.item() == 1
    return acc_dev.cpu(), acc_ref


@pytest.mark.parametrize('op', OPS3)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('n,pos', [(300, 5), (20000, 12345)])
def test_reduce_into_nan_parity(op, dtype, n, pos):
    """A NaN in the value reaches the accumulator, as torch.minimum /
    v.min() in the reference do, whichever lane it sits in; small path
    (n = 300) and two-stage path (n = 20,000)."""
    _C()
    value = torch.randn(n, generator=_gen(n)).to(dtype)
    value[pos] = float('nan')
    got, want = _reduce_both(value, op)
    assert torch.isnan(want).all()
    assert torch.isnan(got).all(), f'NaN at index {pos} was dropped: {got.item()}'


@pytest.mark.parametrize('op', OPS3)
def test_reduce_nan_accumulator_sticks(op):
    _C()
    value = torch.randn(300, generator=_gen(3))
    got, want = _reduce_both(value, op, init=float('nan'))
    assert torch.isnan(want).all() and torch.isnan(got).all()


@pytest.mark.parametrize('op', OPS3)
@pytest.mark.parametrize('n', [300, 20000])
def test_reduce_into_infinities(op, n):
    _C()
    value = torch.randn(n, generator=_gen(n + 1))
    value[n // 3] = float('inf')
    if op != OP_SUM:  # +inf and -inf together sum to NaN; covered by parity below
        value[n // 2] = float('-inf')
    got, want = _reduce_both(value, op)
    assert torch.equal(got, want)
    value[n // 2] = float('-inf')
    got, want = _reduce_both(value, op)
    torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize('op', OPS3)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_accumulate_elementwise_nan_parity(op, dtype):
    _C()
    values = [torch.randn(7, 9, generator=_gen(k)).to(dtype) for k in range(3)]
    values[0][1, 2] = float('nan')  # NaN first, finite values later
    values[2][3, 4] = float('nan')  # NaN last
    values[1][5, 6] = float('inf')
    values[1][6, 6] = float('-inf')
    acc_ref = torch.full((7, 9), _acc_init(op), dtype=torch.float64)
    acc_dev = acc_ref.to(DEV)
    cnt_ref = torch.zeros(1, dtype=torch.int64)
    cnt_dev = cnt_ref.to(DEV)
    for v in values:
        ref.accumulate_elementwise(v, acc_ref, cnt_ref, op)
        ops.metric_accumulate_elementwise(v.to(DEV), acc_dev, cnt_dev, op)
    assert cnt_dev.item() == 3
    assert torch.isnan(acc_ref[1, 2]) and torch.isnan(acc_ref[3, 4])
    torch.testing.assert_close(acc_dev.cpu(), acc_ref, rtol=1e-15, atol=0, equal_nan=True)


@pytest.mark.parametrize('op', OPS3)
@pytest.mark.parametrize('dims', [[0], [2], [0, 1]])
def test_finalize_dims_nan_parity(op, dims):
    _C()
    acc = torch.randn(3, 4, 5, generator=_gen(11), dtype=torch.float64)
    acc[0, 1, 2] = float('nan')  # first along dim 0
    acc[2, 3, 4] = float('nan')  # last along every dim
    acc[1, 0, 0] = float('inf')
    acc[1, 2, 3] = float('-inf')
    want = ref.finalize_dims(acc, dims, op)
    got = ops.metric_finalize_dims(acc.to(DEV), dims, op).cpu()
    assert torch.isnan(want).any()
    torch.testing.assert_close(got, want, rtol=1e-14, atol=1e-14, equal_nan=True)


@pytest.mark.parametrize('op', OPS3)
@pytest.mark.parametrize('dtype', [torch.int32, torch.uint8, torch.float64, torch.int64])
def test_reduce_into_other_dtypes_large_path(op, dtype):
    """n = 16,385 is the first size on the two-stage path."""
    _C()
    n = 16385
    g = _gen(n)
    if dtype == torch.float64:
        value = torch.randn(n, generator=g, dtype=torch.float64) + 1.0
    elif dtype == torch.uint8:
        value = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
    else:
        value = torch.randint(-(2**31), 2**31, (n,), generator=g, dtype=torch.int64).to(dtype)
    acc_dtype = ref.acc_dtype_for(dtype)
    got, want = _reduce_both(value, op, acc_dtype=acc_dtype)
    if acc_dtype == torch.int64 or op != OP_SUM:
        assert torch.equal(got, want)
    else:
        exact = math.fsum(value.tolist())
        assert got.item() == pytest.approx(exact, rel=1e-12)


def test_reduce_into_grid_stride_sum():
    """n = 4,200,003 > 2048 * 256 * 8 makes reduce_partials_kernel stride."""
    _C()
    n = 4_200_003
    value = torch.randn(n, generator=_gen(n)) + 0.5
    want = value.double().sum().item()
    dev = value.to(DEV)
    results = []
    for _ in range(2):
        acc = torch.zeros(1, dtype=torch.float64, device=DEV)
        cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
        ops.metric_reduce_into(dev, acc, cnt, OP_SUM)
        results.append(acc.item())
    assert results[0] == pytest.approx(want, rel=1e-12)
    assert results[0] == results[1]
    for op, exact in [(OP_MIN, value.min().item()), (OP_MAX, value.max().item())]:
        acc = torch.full((1,), _acc_init(op), dtype=torch.float64, device=DEV)
        ops.metric_reduce_into(dev, acc, torch.zeros(1, dtype=torch.int64, device=DEV), op)
        assert acc.item() == exact


# ------------------------------------------------------------------ optimizers

LR, BETA1, BETA2, ADAM_EPS, GRAD_SCALE = 1e-2, 0.9, 0.999, 1e-8, 0.5


def _f32(v):
    """The fp32 value a launcher's (float) cast hands the kernel."""
    return float(torch.tensor(v, dtype=torch.float32))


TOL_SAMPLE = 1027


@functools.lru_cache(maxsize=None)
def _optim_inputs(n, bf16):
    """fp32 param (the master for the bf16 kernels), grad, non-zero moments
    and a momentum buffer, max(n, 1027) elements of each. Read-only: callers
    clone. A case with n < 1027 runs the kernel on the first n elements; the
    references and the 8x tolerance are evaluated on all 1027, because the
    largest deviation among 1 to 5 elements is no estimate of the fp32
    path's error. From n = 1027 on they use exactly the case's inputs."""
    n = max(n, TOL_SAMPLE)
    g = _gen(n + (1 if bf16 else 0))
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g)
    if bf16:
        grad = grad.to(torch.bfloat16)
    m = 0.1 * torch.randn(n, generator=g)
    v = 0.01 * torch.rand(n, generator=g) + 1e-4
    mom = 0.5 * torch.randn(n, generator=g)
    return p, grad, m, v, mom


def _adam_fp64(p, grad, m, v, t, wd):
    """One Adam step of ref.fused_adam_step's formula in fp64, on the fp32
    hyperparameters the kernel receives. Returns update, exp_avg, exp_avg_sq."""
    lr, b1, b2, eps, wd, gs = (_f32(h) for h in (LR, BETA1, BETA2, ADAM_EPS, wd, GRAD_SCALE))
    p, g, m, v = p.double(), grad.double() * gs, m.double(), v.double()
    if wd != 0:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    update = -lr * (m / (1 - b1**t)) / ((v / (1 - b2**t)).sqrt() + eps)
    return update, m, v


def _tol8(ref32, ref64):
    """8 x the deviation of the fp32 CPU reference from the fp64 evaluation."""
    return 8 * (ref32.double() - ref64).abs().max().item()


def _check_step(n, p0, p_dev, upd64, upd_tol, pairs):
    """update = p_after - p_before within upd_tol + 2^-23 |p| for the stored
    parameter; each (name, device, fp64, tol) of state within its tol. The
    device tensors hold the first n elements of the references."""
    p0 = p0[:n].double()
    _assert_within(p_dev.cpu().double() - p0, upd64[:n], upd_tol + 2.0**-23 * p0.abs(), 'update')
    for name, dev, want, tol in pairs:
        _assert_within(dev.cpu(), want[:n], torch.tensor(tol, dtype=torch.float64), name)


ADAM_SIZES = [1, 3, 5, 1027, 2_097_159]  # the last: n/4 > 2048 * 256, the loop strides
ADAM_BF16_SIZES = [1, 3, 5, 1027, 4_194_311]  # n/8 > 2048 * 256


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('step0', [0, 9, 999])
@pytest.mark.parametrize('n', ADAM_SIZES)
def test_fused_adam_one_step(n, step0, wd):
    _C()
    p0, grad, m0, v0, _ = _optim_inputs(n, False)
    upd64, m64, v64 = _adam_fp64(p0, grad, m0, v0, step0 + 1, wd)

    p32, m32, v32 = p0.clone(), m0.clone(), v0.clone()
    st32 = torch.full((1,), step0, dtype=torch.int32)
    ref.fused_adam_step(p32, grad, m32, v32, st32, LR, BETA1, BETA2, ADAM_EPS, wd, GRAD_SCALE)
    upd_tol = _tol8(p32.double() - p0.double(), upd64)

    p, m, v = p0[:n].to(DEV), m0[:n].to(DEV), v0[:n].to(DEV)
    st = torch.full((1,), step0, dtype=torch.int32, device=DEV)
    ops.fused_adam(p, grad[:n].to(DEV), m, v, st, LR, BETA1, BETA2, ADAM_EPS, wd, GRAD_SCALE)
    assert st.item() == step0 + 1 == st32.item()
    _check_step(n, p0, p, upd64, upd_tol, [('exp_avg', m, m64, _tol8(m32, m64)), ('exp_avg_sq', v, v64, _tol8(v32, v64))])


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('step0', [0, 9, 999])
@pytest.mark.parametrize('n', ADAM_BF16_SIZES)
def test_fused_adam_bf16_one_step(n, step0, wd):
    _C()
    w0, grad, m0, v0, _ = _optim_inputs(n, True)
    upd64, m64, v64 = _adam_fp64(w0, grad, m0, v0, step0 + 1, wd)

    w32, m32, v32 = w0.clone(), m0.clone(), v0.clone()
    p32 = w0.to(torch.bfloat16)
    st32 = torch.full((1,), step0, dtype=torch.int32)
    ref.fused_adam_bf16_step(p32, grad, w32, m32, v32, st32, LR, BETA1, BETA2, ADAM_EPS, wd, GRAD_SCALE)
    upd_tol = _tol8(w32.double() - w0.double(), upd64)

    w, m, v = w0[:n].to(DEV), m0[:n].to(DEV), v0[:n].to(DEV)
    p = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    st = torch.full((1,), step0, dtype=torch.int32, device=DEV)
    ops.fused_adam_bf16(p, grad[:n].to(DEV), w, m, v, st, LR, BETA1, BETA2, ADAM_EPS, wd, GRAD_SCALE)
    assert st.item() == step0 + 1
    _check_step(n, w0, w, upd64, upd_tol, [('exp_avg', m, m64, _tol8(m32, m64)), ('exp_avg_sq', v, v64, _tol8(v32, v64))])
    assert torch.equal(p.view(torch.int16), w.to(torch.bfloat16).view(torch.int16)), 'param != bf16(master)'


SGD_LR, SGD_WD = 0.1, 0.01


def _sgd_fp64(p, grad, mom, momentum):
    lr, mu, wd, gs = (_f32(h) for h in (SGD_LR, momentum, SGD_WD, GRAD_SCALE))
    g = grad.double() * gs + wd * p.double()
    if mom is not None and momentum != 0:
        mom = mu * mom.double() + g
        g = mom
    return -lr * g, mom


@pytest.mark.parametrize('momentum', [0.0, 0.9])
@pytest.mark.parametrize('n', [1, 5, 1027, 2_097_159])
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_fused_sgd_one_step(bf16, n, momentum):
    """momentum 0 passes momentum_buf=None. n = 2,097,159 makes both
    kernels stride (n/4 and n/1024 blocks exceed the 2048-block cap)."""
    _C()
    p0, grad, _, _, mom0 = _optim_inputs(n, bf16)
    mom0 = mom0 if momentum != 0 else None
    upd64, mom64 = _sgd_fp64(p0, grad, mom0, momentum)

    p32 = p0.clone()
    mom32 = mom0.clone() if mom0 is not None else None
    if bf16:
        ref.fused_sgd_bf16_step(p0.to(torch.bfloat16), grad, p32, mom32, SGD_LR, momentum, SGD_WD, GRAD_SCALE)
    else:
        ref.fused_sgd_step(p32, grad, mom32, SGD_LR, momentum, SGD_WD, GRAD_SCALE)
    upd_tol = _tol8(p32.double() - p0.double(), upd64)

    w = p0[:n].to(DEV)
    mom = mom0[:n].to(DEV) if mom0 is not None else None
    if bf16:
        p = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        ops.fused_sgd_bf16(p, grad[:n].to(DEV), w, mom, SGD_LR, momentum, SGD_WD, GRAD_SCALE)
        assert torch.equal(p.view(torch.int16), w.to(torch.bfloat16).view(torch.int16)), 'param != bf16(master)'
    else:
        ops.fused_sgd(w, grad[:n].to(DEV), mom, SGD_LR, momentum, SGD_WD, GRAD_SCALE)
    pairs = [('momentum_buf', mom, mom64, _tol8(mom32, mom64))] if mom is not None else []
    _check_step(n, p0, w, upd64, upd_tol, pairs)


@pytest.mark.parametrize('n', [1, 3, 1027, 8_388_613])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_l2_norm_and_clip_tails(dtype, n):
    """n % 8 != 0 runs the four scalar tails; n = 8,388,613 makes the norm
    and scale kernels stride.

    norm:    relative 2^-22 against fp64 (fp64 accumulation, one fp32 store).
    clipped: one rounding of x * s, 2^-24 (fp32) or 2^-8 (bf16) relative,
             plus 2^-21 for the fp32 norm, the + 1e-6 and the division
             behind s."""
    _C()
    x = torch.randn(n, generator=_gen(n)).to(dtype)
    norm64 = x.double().square().sum().sqrt().item()
    half_ulp = FP32_HALF_ULP if dtype == torch.float32 else BF16_HALF_ULP

    dev = x.to(DEV)
    assert ops.l2_norm(dev).item() == pytest.approx(norm64, rel=2.0**-22)
    assert torch.equal(dev.cpu().view(torch.int16), x.view(torch.int16)), 'l2_norm must not write'

    # norm below max_norm: bitwise unchanged
    norm = ops.clip_grad_norm_(dev, 2.0 * norm64)
    assert norm.item() == pytest.approx(norm64, rel=2.0**-22)
    assert torch.equal(dev.cpu().view(torch.int16), x.view(torch.int16))

    # clipped
    max_norm = 0.5 * norm64
    norm = ops.clip_grad_norm_(dev, max_norm)
    assert norm.item() == pytest.approx(norm64, rel=2.0**-22)
    want = x.double() * (_f32(max_norm) / (norm64 + 1e-6))
    _assert_within(dev.cpu(), want, (half_ulp + 2.0**-21) * want.abs(), 'clipped')

    # all-zero: stays zero, no NaN
    zero = torch.zeros(n, dtype=dtype, device=DEV)
    assert ops.clip_grad_norm_(zero, 1.0).item() == 0.0
    assert (zero == 0).all()


# ----------------------------------------------------------------------- copy

GUARD = 64
GUARD_BYTE = 0xA5
COPY_OFFSETS = [0, 1, 2, 4, 16]


def _guarded_dst(doff, nbytes):
    """A sentinel-filled uint8 buffer and the view at 64 + doff inside it."""
    buf = torch.full((GUARD + doff + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + doff : GUARD + doff + nbytes]


def _assert_guards(buf, doff, nbytes):
    assert (buf[: GUARD + doff] == GUARD_BYTE).all(), 'bytes before the destination were written'
    assert (buf[GUARD + doff + nbytes :] == GUARD_BYTE).all(), 'bytes after the destination were written'


@pytest.mark.parametrize('nbytes', [1, 3, 15, 16, 17, 1027, 2**20 + 5])
def test_chunked_copy_offsets_and_tails(nbytes):
    """All 25 (src offset, dst offset) pairs in one call: equal congruence
    takes the 16 B or 4 B path with its byte tail, mismatched congruence the
    byte path. 2^20 + 5 bytes split into two units."""
    _C()
    srcs, dsts, bufs = [], [], []
    for soff in COPY_OFFSETS:
        for doff in COPY_OFFSETS:
            sbuf = torch.randint(0, 256, (soff + nbytes,), generator=_gen(soff * 31 + doff), dtype=torch.uint8).to(DEV)
            assert sbuf.data_ptr() % 16 == 0
            buf, dst = _guarded_dst(doff, nbytes)
            srcs.append(sbuf[soff:])
            dsts.append(dst)
            bufs.append((buf, doff))
    ops.chunked_copy(srcs, dsts)
    torch.cuda.synchronize()
    for src, dst, (buf, doff) in zip(srcs, dsts, bufs):
        assert torch.equal(dst, src), f'copy differs at src offset {src.storage_offset()}, dst offset {doff}'
        _assert_guards(buf, doff, nbytes)


def test_chunked_copy_odd_bf16_many_units_and_empties():
    _C()
    # an odd-length bf16 tensor: the 4 B path with a 2-byte tail
    src = torch.randn(1001, generator=_gen(1)).to(torch.bfloat16).to(DEV)
    buf, dst8 = _guarded_dst(4, 999 * 2)
    ops.chunked_copy([src[2:1001]], [dst8.view(torch.bfloat16)])
    assert torch.equal(dst8.view(torch.bfloat16).view(torch.int16), src[2:1001].view(torch.int16))
    _assert_guards(buf, 4, 999 * 2)

    # 2,100 units of 24 bytes in one call (> the 2048-block grid), scattered
    # in reverse order, with an empty tensor in the list
    nunits = 2100
    big = torch.randint(0, 256, (nunits * 24,), generator=_gen(2), dtype=torch.uint8).to(DEV)
    buf, out = _guarded_dst(0, nunits * 24)
    empty = torch.empty(0, dtype=torch.uint8, device=DEV)
    srcs = [big[24 * i : 24 * (i + 1)] for i in range(nunits)]
    dsts = [out[24 * (nunits - 1 - i) : 24 * (nunits - i)] for i in range(nunits)]
    srcs.insert(7, empty)
    dsts.insert(7, empty.clone())
    ops.chunked_copy(srcs, dsts)
    assert torch.equal(out.view(nunits, 24), big.view(nunits, 24).flip(0))
    _assert_guards(buf, 0, nunits * 24)

    # nothing but empty tensors: no launch, no error
    ops.chunked_copy([empty, empty], [empty.clone(), empty.clone()])
    torch.cuda.synchronize()
