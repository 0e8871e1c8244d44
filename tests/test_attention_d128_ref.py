"""Head dim 128 off the GPU: sdpa's fallback is unchanged, and the decode
path does not claim D = 128 (its kernels are head dim 64 only)."""

import pytest
import torch

from dmlcloud_amd.ops.fused_attn import fused_attention_usable, fused_kvcache_usable, sdpa

B, D = 2, 128


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('h,hkv', [(2, 2), (4, 1)])
def test_sdpa_cpu_d128_equals_expanded_call(h, hkv, causal):
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, x, 33, D, generator=g) for x in (h, hkv, hkv))
    assert fused_attention_usable(q, k, v) is False  # CPU fp32: the fallback
    ke, ve = k.repeat_interleave(h // hkv, 1), v.repeat_interleave(h // hkv, 1)
    want = torch.nn.functional.scaled_dot_product_attention(q, ke, ve, is_causal=causal)
    assert torch.equal(sdpa(q, k, v, causal=causal), want)


def test_kvcache_d128_is_not_native():
    q = torch.zeros(B, 4, 1, D, dtype=torch.bfloat16)
    cache = torch.zeros(B, 2, 64, D, dtype=torch.bfloat16)
    kv_len = torch.full((B,), 5, dtype=torch.int32)
    assert fused_kvcache_usable(q, cache, cache, kv_len) is False
