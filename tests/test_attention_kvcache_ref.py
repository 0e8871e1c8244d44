"""KV-cache decode attention on the CPU: `kvcache_attention_ref` (the CPU
path of `sdpa_kvcache` and the oracle of the GPU tests) against a literal
per-row fp64 softmax, and GPT2.decode_step / generate against the plain
forward on the growing sequence.
"""

import math

import pytest
import torch

from dmlcloud_amd.models.gpt2 import gpt2_tiny
from dmlcloud_amd.ops import sdpa_kvcache
from dmlcloud_amd.ops._attention_ref import kvcache_attention_ref

NMAX, D = 40, 64


def literal_softmax(q, k, v, kv_len, causal):
    """Row by row in fp64 over the valid keys only: (o, lse)."""
    B, H, Nq, _ = q.shape
    G = H // k.shape[1]
    o = torch.zeros(B, H, Nq, D, dtype=torch.float64)
    lse = torch.zeros(B, H, Nq, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            for i in range(Nq):
                n = kv_len[b] - Nq + i + 1 if causal else kv_len[b]
                s = (k[b, h // G, :n].double() @ q[b, h, i].double()) / math.sqrt(D)
                lse[b, h, i] = torch.logsumexp(s, 0)
                o[b, h, i] = torch.softmax(s, 0) @ v[b, h // G, :n].double()
    return o, lse


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('kv_len', [[1, 40], [33, 7]])
@pytest.mark.parametrize('h,hkv,nq', [(4, 4, 1), (4, 1, 1), (6, 2, 1), (4, 4, 4), (4, 2, 5)])
def test_reference_matches_literal_fp64_softmax(h, hkv, nq, kv_len, causal):
    g = torch.Generator().manual_seed(100 * h + 10 * hkv + nq)
    q = torch.randn(2, h, nq, D, generator=g)
    k = torch.randn(2, hkv, NMAX, D, generator=g)
    v = torch.randn(2, hkv, NMAX, D, generator=g)
    lens = [max(n, nq) if causal else n for n in kv_len]  # the clamp, where it acts
    for b, n in enumerate(lens):  # the slack rows must not show
        k[b, :, n:] = float('nan')
        v[b, :, n:] = float('nan')
    want_o, want_lse = literal_softmax(q, k, v, lens, causal)
    o, lse = kvcache_attention_ref(q, k, v, torch.tensor(kv_len), causal, return_lse=True)
    torch.testing.assert_close(o.double(), want_o, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lse.double(), want_lse, rtol=1e-5, atol=1e-5)
    # the public op takes the same path on the CPU
    assert torch.equal(sdpa_kvcache(q, k, v, torch.tensor(kv_len), causal=causal), o)


@pytest.mark.parametrize('n_kv_head', [None, 1])
def test_decode_step_and_generate_match_the_plain_forward(n_kv_head):
    torch.manual_seed(0)
    model = gpt2_tiny(n_kv_head=n_kv_head).eval()
    prompt = torch.randint(0, model.cfg.vocab_size, (2, 5))
    cache = model.init_cache(2, 5 + 6, prompt.device, torch.float32)
    seq = prompt
    with torch.no_grad():
        logits = model.prefill(prompt, cache)
        for _ in range(6):
            torch.testing.assert_close(logits, model(seq)[:, -1], rtol=0, atol=1e-4)
            seq = torch.cat([seq, logits.argmax(-1, keepdim=True)], dim=1)
            logits = model.decode_step(seq[:, -1], cache)
        torch.testing.assert_close(logits, model(seq)[:, -1], rtol=0, atol=1e-4)
    assert cache.kv_len.tolist() == [11, 11]
    out = model.generate(prompt, 6, temperature=0.0)
    assert out.shape == (2, 5 + 6) and torch.equal(out[:, :5], prompt)
    assert torch.equal(out, seq)  # greedy: the tokens decode_step led to


def test_forward_only():
    q, kv = torch.randn(1, 2, 1, D, requires_grad=True), torch.randn(1, 2, 8, D)
    with pytest.raises(RuntimeError, match='forward only'):
        sdpa_kvcache(q, kv, kv, torch.tensor([3]))
