"""Grouped-query attention on the CPU: the blueprint's emulation of the
kernels' kGqa instantiations (query head h reads K/V head h // G; one
dK/dV block per K/V head walks the group's heads into one accumulator)
against fp32 SDPA with enable_gqa=True + autograd, and sdpa's fallback."""

import sys

import pytest
import torch
from torch.nn import functional as F

from dmlcloud_amd.ops._attention_ref import gqa_bwd_padded, gqa_fwd_padded
from dmlcloud_amd.ops.fused_attn import document_mask, fused_attention_usable, sdpa

B, D = 2, 64


def _inputs(h, hkv, n, seed):
    """q, k, v, dO: an independent K/V per K/V head, so that a wrong head
    mapping (h % Hkv for h // G) shows."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, h, n, D, generator=g)
    k = torch.randn(B, hkv, n, D, generator=g)
    v = torch.randn(B, hkv, n, D, generator=g)
    do = torch.randn(B, h, n, D, generator=g)
    return q, k, v, do


def _doc_start(n, bounds):
    ds = torch.empty(n, dtype=torch.int32)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ds[lo:hi] = lo
    return ds


def _check_blueprint(q, k, v, do, causal, doc_start=None):
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (q, k, v))
    if doc_start is None:
        ref = F.scaled_dot_product_attention(q2, k2, v2, is_causal=causal, enable_gqa=True)
    else:
        ref = F.scaled_dot_product_attention(q2, k2, v2, attn_mask=document_mask(doc_start, causal), enable_gqa=True)
    ref.backward(do)

    o, lse = gqa_fwd_padded(q, k, v, causal=causal, doc_start=doc_start)
    dq, dk, dv = gqa_bwd_padded(do, q, k, v, o, lse, causal=causal, doc_start=doc_start)
    assert dk.shape == k.shape and dv.shape == v.shape
    for name, got, want in (('o', o, ref.detach()), ('dq', dq, q2.grad), ('dk', dk, k2.grad), ('dv', dv, v2.grad)):
        print(f'{name}: max abs err {(got - want).abs().max().item():.3e}')
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', [33, 100])
@pytest.mark.parametrize('h,hkv', [(4, 1), (6, 2)])
def test_blueprint_matches_gqa_sdpa_and_autograd(h, hkv, n, causal):
    _check_blueprint(*_inputs(h, hkv, n, seed=100 * h + n), causal)


def test_blueprint_with_three_documents():
    n = 100
    ds = torch.stack([_doc_start(n, [0, 21, 70, n]), _doc_start(n, [0, 5, 37, n])])
    _check_blueprint(*_inputs(6, 2, n, seed=7), True, ds)


def test_blueprint_gqa_equals_mha_on_expanded_kv():
    """With G = 1 heads per group nothing is summed: the wrapper on
    expanded K/V gives, per query head, dk/dv whose sum over the group is
    the grouped result (to fp32 round-off: another summation order)."""
    h, hkv, n = 4, 2, 33
    q, k, v, do = _inputs(h, hkv, n, seed=3)
    ke, ve = k.repeat_interleave(h // hkv, 1), v.repeat_interleave(h // hkv, 1)
    o, lse = gqa_fwd_padded(q, k, v)
    oe, lsee = gqa_fwd_padded(q, ke, ve)
    assert torch.equal(o, oe) and torch.equal(lse, lsee)
    dq, dk, dv = gqa_bwd_padded(do, q, k, v, o, lse)
    dqe, dke, dve = gqa_bwd_padded(do, q, ke, ve, o, lse)
    assert torch.equal(dq, dqe)
    torch.testing.assert_close(dk, dke.view(B, hkv, h // hkv, n, D).sum(2), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dv, dve.view(B, hkv, h // hkv, n, D).sum(2), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('h,hkv', [(4, 1), (6, 2)])
def test_sdpa_cpu_gqa_equals_expanded_call(h, hkv, causal):
    q, k, v, _ = _inputs(h, hkv, 33, seed=11)
    assert fused_attention_usable(q, k, v) is False  # CPU fp32: the fallback
    got = sdpa(q, k, v, causal=causal)
    want = sdpa(q, k.repeat_interleave(h // hkv, 1), v.repeat_interleave(h // hkv, 1), causal=causal)
    assert got.shape == q.shape
    assert torch.equal(got, want)


def test_sdpa_cpu_gqa_with_doc_start_equals_expanded_call():
    h, hkv, n = 6, 2, 33
    q, k, v, _ = _inputs(h, hkv, n, seed=12)
    ds = _doc_start(n, [0, 9, 20, n]).unsqueeze(0).expand(B, n)
    assert fused_attention_usable(q, k, v, doc_start=ds) is False
    got = sdpa(q, k, v, causal=True, doc_start=ds)
    want = sdpa(q, k.repeat_interleave(3, 1), v.repeat_interleave(3, 1), causal=True, doc_start=ds)
    assert torch.equal(got, want)


def test_sdpa_cpu_gqa_bf16_and_gradients():
    """The fallback also takes bf16, and autograd hands k.grad back in k's
    shape."""
    q, k, v, do = (t.to(torch.bfloat16) for t in _inputs(4, 2, 33, seed=13))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    out = sdpa(q, k, v, causal=True)
    out.backward(do)
    assert out.dtype == torch.bfloat16 and k.grad.shape == k.shape and v.grad.shape == v.shape
    assert torch.isfinite(k.grad.float()).all()


if __name__ == '__main__':
    sys.exit(pytest.main([__file__]))
