"""MFMA flash attention at sequence lengths that are not a multiple of 64
(the kernels' kRagged instantiations: clamped row loads, masked tail,
per-row predicated stores).

B = 2, H = 3 and N in {1, 17, 33, 65, 100, 129, 200}: the smallest
lengths that cross each tile edge of the three kernels — the 16-row
sub-tile, the 32-row wave tile / q-step, the 64-key tile and dkdv/dq
block, and the 128-row forward block.

Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools
import math

import pytest
import torch

from attn_testlib import assert_fwd_bwd_close, run_with_canaries

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B, H, D = 2, 3, 64
LENGTHS = [1, 17, 33, 65, 100, 129, 200]
SCALE = 1.0 / math.sqrt(D)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """q, k, v, dO for one length (bf16, on the device); never modified."""
    g = torch.Generator().manual_seed(1000 + n)
    return tuple((torch.randn(B, H, n, D, generator=g) * 0.5).to(torch.bfloat16).to(DEV) for _ in range(4))


@functools.lru_cache(maxsize=None)
def _reference(n, causal):
    """fp32 SDPA forward + autograd on the bf16-rounded inputs, computed
    once per (n, causal) and shared: (out, dq, dk, dv)."""
    q, k, v, do = _inputs(n)
    q2, k2, v2 = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(q2, k2, v2, is_causal=causal)
    ref.backward(do.float())
    return ref.detach(), q2.grad, k2.grad, v2.grad


def _check_fwd_bwd(n, causal, out, dq, dk, dv):
    assert_fwd_bwd_close(f'N={n} causal={causal}', (out, dq, dk, dv), _reference(n, causal))


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', LENGTHS)
def test_fwd_direct_matches_sdpa_and_blueprint(causal, n):
    from dmlcloud_amd import _C
    from dmlcloud_amd.ops._attention_ref import mha_fwd_tiled

    q, k, v, _ = _inputs(n)
    o = torch.empty(B, H, n, D, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, H, n, dtype=torch.float32, device=DEV)
    _C.attn_fwd(q, k, v, o, lse, SCALE, causal)

    torch.testing.assert_close(o.float(), _reference(n, causal)[0], rtol=3e-2, atol=3e-2)
    _, ref_lse = mha_fwd_tiled(q.cpu().float(), k.cpu().float(), v.cpu().float(), causal)
    torch.testing.assert_close(lse.cpu(), ref_lse, rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', LENGTHS)
def test_sdpa_fwd_bwd_matches_autograd(causal, n):
    from dmlcloud_amd.ops.fused_attn import fused_attention_usable, sdpa

    q, k, v, do = _inputs(n)
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    assert fused_attention_usable(q, k, v) is True
    out = sdpa(q, k, v, causal=causal)
    out.backward(do)
    _check_fwd_bwd(n, causal, out.detach(), q.grad, k.grad, v.grad)


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', LENGTHS)
def test_poisoned_slack(causal, n):
    """The rows behind the sequence end hold 30.0 and live in the same
    allocation: a kernel that reads a padded row without masking it
    produces outputs near 30 instead of ~0.2."""
    from dmlcloud_amd.ops.fused_attn import fused_attention_usable, sdpa

    rows = (n + 127) // 128 * 128
    views = []
    for t in _inputs(n):
        buf = torch.full((B, H, rows, D), 30.0, dtype=torch.bfloat16, device=DEV)
        buf[..., :n, :] = t
        views.append(buf[..., :n, :])
    q, k, v = (t.detach().requires_grad_(True) for t in views[:3])
    do = views[3]
    assert q.stride() == (H * rows * D, rows * D, D, 1)  # a view, no copy
    assert fused_attention_usable(q, k, v) is True

    out = sdpa(q, k, v, causal=causal)
    out.backward(do)
    _check_fwd_bwd(n, causal, out.detach(), q.grad, k.grad, v.grad)


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', LENGTHS)
def test_canaries_untouched(causal, n):
    """Every output is the front of a larger buffer; the 128 rows' worth
    of sentinel behind it must come back bit-identical, and every element
    in front of it must have been written (no NaN fill left)."""
    run_with_canaries(_inputs(n), causal)


def test_exact_counting():
    """Full attention, q = 0, v[j, :] = j, N = 100: every p is exactly 1,
    so o = mean(0..99) = 49.5 and lse = log(100). A dropped tail tile
    gives 31.5; a counted pad row moves lse to log(128)."""
    from dmlcloud_amd import _C

    n = 100
    k = _inputs(n)[1]
    q = torch.zeros(B, H, n, D, dtype=torch.bfloat16, device=DEV)
    v = torch.arange(n, dtype=torch.float32, device=DEV).view(1, 1, n, 1).expand(B, H, n, D)
    v = v.to(torch.bfloat16).contiguous()  # integers < 256 are exact in bf16
    do = torch.ones(B, H, n, D, dtype=torch.bfloat16, device=DEV)

    o = torch.empty_like(q)
    lse = torch.empty(B, H, n, dtype=torch.float32, device=DEV)
    _C.attn_fwd(q, k, v, o, lse, SCALE, False)
    torch.testing.assert_close(o.float(), torch.full_like(o, 49.5, dtype=torch.float32), rtol=1e-2, atol=0.0)
    torch.testing.assert_close(lse, torch.full_like(lse, math.log(100.0)), rtol=0.0, atol=1e-3)

    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    delta = torch.empty(B * H * n, dtype=torch.float32, device=DEV)
    _C.attn_bwd(q, k, v, do, o, lse, dq, dk, dv, delta, SCALE, False)
    # dv[j] = sum_i p[i, j] * 1 = 100 * (1/100); P is stored in bf16, so
    # 1/100 carries up to 2^-9 relative error
    torch.testing.assert_close(dv.float(), torch.ones_like(dv, dtype=torch.float32), rtol=0.0, atol=1e-2)


def test_transpose_views_bit_identical():
    """[B, T, H, D] memory seen as [B, H, T, D] at N = 100 matches the
    contiguous path bit for bit."""
    from dmlcloud_amd.ops.fused_attn import sdpa

    n = 100
    g = torch.Generator().manual_seed(5)
    base = [(torch.randn(B, n, H, D, generator=g) * 0.5).to(torch.bfloat16).to(DEV) for _ in range(3)]
    q, k, v = (t.transpose(1, 2).requires_grad_(True) for t in base)
    assert not q.is_contiguous()
    do = _inputs(n)[3]

    out = sdpa(q, k, v, causal=True)
    out.backward(do)

    q2, k2, v2 = (t.detach().contiguous().requires_grad_(True) for t in (q, k, v))
    out2 = sdpa(q2, k2, v2, causal=True)
    out2.backward(do)

    assert torch.equal(out, out2)
    assert torch.equal(q.grad, q2.grad)
    assert torch.equal(k.grad, k2.grad)
    assert torch.equal(v.grad, v2.grad)


def test_gpt2_ragged_sequence_end_to_end(monkeypatch):
    """A D = 64 GPT-2 on a (2, 50) batch reaches the native kernels (the
    stock gpt2_tiny has D = 32 and never does) and its bf16 loss matches
    the same weights in fp32."""
    from dmlcloud_amd.models.gpt2 import GPT2, GPT2Config
    from dmlcloud_amd.ops import fused_attn

    cfg = GPT2Config(vocab_size=512, n_positions=64, n_embd=128, n_layer=2, n_head=2)
    torch.manual_seed(0)
    model = GPT2(cfg).to(DEV)
    idx = torch.randint(0, cfg.vocab_size, (2, 50), device=DEV)
    _, loss32 = model(idx, targets=idx)

    model16 = GPT2(cfg).to(DEV)
    model16.load_state_dict(model.state_dict())
    model16 = model16.to(torch.bfloat16)

    native_calls = []
    real_fwd = fused_attn._C.attn_fwd

    def counting_fwd(q, *rest):
        native_calls.append(q.shape[-2])
        return real_fwd(q, *rest)

    monkeypatch.setattr(fused_attn._C, 'attn_fwd', counting_fwd)
    _, loss16 = model16(idx, targets=idx)
    loss16.backward()
    assert native_calls == [50] * cfg.n_layer
    assert loss16.item() == pytest.approx(loss32.item(), rel=5e-2)
    assert all(torch.isfinite(p.grad).all() for p in model16.parameters())
