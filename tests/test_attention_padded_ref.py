"""The ragged-N blueprint (full tiles, clamped row gathers, -1e30 / p = 0
masks, predicated stores — the literal emulation of the kernels'
kRagged instantiations) must match plain softmax attention and autograd
for sequence lengths that are not a multiple of any tile size."""

import math
import sys

import pytest
import torch

from dmlcloud_amd.ops._attention_ref import flash_attn_bwd_padded, flash_attn_fwd_padded

# below one 16-row sub-tile, across the 16/32/64/128 tile edges
LENGTHS = [1, 17, 33, 65, 100, 129]
D = 64


def _plain_attention(q, k, v, causal):
    n = q.shape[0]
    s = (q @ k.T) / math.sqrt(q.shape[1])
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool), diagonal=1), -float('inf'))
    return torch.softmax(s, dim=-1) @ v, torch.logsumexp(s, dim=-1)


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', LENGTHS)
def test_fwd_padded_matches_plain(causal, n):
    torch.manual_seed(n)
    q, k, v = (torch.randn(n, D) for _ in range(3))
    o, lse = flash_attn_fwd_padded(q, k, v, causal=causal)
    ref, ref_lse = _plain_attention(q, k, v, causal)
    # every row < N was stored (no NaN poison left), none was polluted
    torch.testing.assert_close(o, ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lse, ref_lse, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', LENGTHS)
def test_bwd_padded_matches_autograd(causal, n):
    torch.manual_seed(100 + n)
    q = torch.randn(n, D, requires_grad=True)
    k = torch.randn(n, D, requires_grad=True)
    v = torch.randn(n, D, requires_grad=True)
    out, _ = _plain_attention(q, k, v, causal)
    do = torch.randn(n, D)
    out.backward(do)

    with torch.no_grad():
        qd, kd, vd = q.detach(), k.detach(), v.detach()
        o, lse = flash_attn_fwd_padded(qd, kd, vd, causal=causal)
        dq, dk, dv = flash_attn_bwd_padded(do, qd, kd, vd, o, lse, causal=causal)

    torch.testing.assert_close(dq, q.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dk, k.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dv, v.grad, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('causal', [True, False])
def test_padded_equals_tiled_when_aligned(causal):
    """At N % 64 == 0 nothing is clamped or masked: same numbers as the
    aligned blueprint."""
    from dmlcloud_amd.ops._attention_ref import flash_attn_fwd_tiled

    torch.manual_seed(7)
    q, k, v = (torch.randn(128, D) for _ in range(3))
    o, lse = flash_attn_fwd_padded(q, k, v, causal=causal)
    o2, lse2 = flash_attn_fwd_tiled(q, k, v, causal=causal)
    torch.testing.assert_close(o, o2, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lse, lse2, rtol=1e-5, atol=1e-5)


if __name__ == '__main__':
    sys.exit(pytest.main([__file__]))
