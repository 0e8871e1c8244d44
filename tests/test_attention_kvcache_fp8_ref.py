"""FP8 (float8_e4m3fn) K/V cache on the CPU: the references that define the
format for the kernels of ops/csrc/attention_decode_fp8.h, and GPT2 on them.
kvcache_attention_ref is held to a literal fp64 softmax over
cache.double() * scale, kvcache_append_ref to the quantisation formula
(uint8 views), dense and paged."""

import math

import pytest
import torch

from dmlcloud_amd.models import gpt2
from dmlcloud_amd.ops import kvcache_append, sdpa_kvcache
from dmlcloud_amd.ops._attention_ref import gather_pages, kvcache_append_ref, kvcache_attention_ref

FP8 = torch.float8_e4m3fn
B, H, HKV, NQ, D, CAP = 2, 4, 2, 5, 64, 96
K_SCALE, V_SCALE = torch.tensor([0.37, 1.9]), torch.tensor([2.3, 0.61])  # per head, distinct, no powers of two


def _caches(paged):
    """(q, k, v, kv_len, table): e4m3 caches, NaN bytes at and past kv_len[b]."""
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, H, NQ, D, generator=g).to(torch.bfloat16)
    k, v = (torch.randn(B, HKV, CAP, D, generator=g).to(FP8) for _ in range(2))
    lens = (NQ, 70)
    for b, n in enumerate(lens):
        k.view(torch.uint8)[b, :, n:] = v.view(torch.uint8)[b, :, n:] = 0x7F
    table = None
    if paged:  # 3 pages of 32 per row, scattered over a pool of 7
        table = torch.tensor([[5, 0, 3], [2, 6, 1]])
        pools = [torch.full((7, HKV, 32, D), 0x7F, dtype=torch.uint8) for _ in range(2)]
        for pool, dense in zip(pools, (k, v)):
            pool[table.flatten()] = dense.view(torch.uint8).view(B, HKV, 3, 32, D).transpose(1, 2).reshape(6, HKV, 32, D)
        k, v = (p.view(FP8) for p in pools)
    return q, k, v, torch.tensor(lens, dtype=torch.int32), table


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('scaled', [True, False])
@pytest.mark.parametrize('paged', [False, True])
def test_attention_ref_is_the_fp64_softmax_over_the_dequantised_cache(paged, scaled, causal):
    q, k, v, kv_len, table = _caches(paged)
    ks, vs = (K_SCALE, V_SCALE) if scaled else (None, None)
    o, lse = kvcache_attention_ref(q, k, v, kv_len, causal, True, table, ks, vs)
    kd, vd = ((gather_pages(t.view(torch.uint8), table).view(FP8) if paged else t).double() for t in (k, v))
    if scaled:
        kd, vd = kd * K_SCALE.double().view(1, -1, 1, 1), vd * V_SCALE.double().view(1, -1, 1, 1)
    for b in range(B):
        for h in range(H):
            for i in range(NQ):
                n = int(kv_len[b]) - NQ + i + 1 if causal else int(kv_len[b])
                s = (kd[b, h // 2, :n] @ q[b, h, i].double()) / math.sqrt(D)
                want = torch.softmax(s, 0) @ vd[b, h // 2, :n]
                torch.testing.assert_close(o[b, h, i].double(), want, rtol=1e-2, atol=1e-2)  # o is bf16
                torch.testing.assert_close(lse[b, h, i].double(), torch.logsumexp(s, 0), rtol=1e-5, atol=1e-5)
    assert sdpa_kvcache(q, k, v, kv_len, causal, block_table=table, k_scale=ks, v_scale=vs).equal(o)


@pytest.mark.parametrize('page_size', [None, 32, 48])
def test_append_ref_stores_the_quantisation_formula(page_size):
    g = torch.Generator().manual_seed(6)
    k_new, v_new = (torch.randn(B, HKV, NQ, D, generator=g).to(torch.bfloat16) * 3 for _ in range(2))
    k_new[0, 0, 0, :4] = torch.tensor([1e4, -1e4, 1e-3, 0.37 * 0.40625])  # saturates twice, subnormal, a tie
    table = None if page_size is None else torch.tensor([[2, 0, 4], [1, 5, 3]])
    shape = (B, HKV, CAP, D) if page_size is None else (6, HKV, page_size, D)
    k, v = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).view(FP8) for _ in range(2))
    kv_len = torch.tensor([(page_size or 32) + 2, NQ], dtype=torch.int32)  # row 0 straddles a page boundary
    before = k.view(torch.uint8).clone()
    kvcache_append(k_new, v_new, k, v, kv_len, table, k_scale=K_SCALE, v_scale=V_SCALE)
    formula = lambda x, s: (x.float() / s.view(1, -1, 1, 1)).clamp(-448, 448).to(FP8).view(torch.uint8)
    changed = 0
    for cache, new, s in ((k, k_new, K_SCALE), (v, v_new, V_SCALE)):
        dense = cache.view(torch.uint8) if table is None else gather_pages(cache.view(torch.uint8), table)
        for b in range(B):
            rows = slice(int(kv_len[b]) - NQ, int(kv_len[b]))
            assert dense[b, :, rows].equal(formula(new, s)[b])
            changed += NQ * HKV * D
    assert (k.view(torch.uint8) != before).sum() <= B * NQ * HKV * D < changed
    assert not k.float().isnan()[0, 0].all() and k_new.float().abs().max() > 448 * 1.9


def test_a_scale_with_a_bf16_cache_is_an_error():
    q, k, v, kv_len, _ = _caches(False)
    k, v = k.to(torch.bfloat16), v.to(torch.bfloat16)
    for call in (
        lambda: sdpa_kvcache(q, k, v, kv_len, k_scale=K_SCALE),
        lambda: kvcache_attention_ref(q, k, v, kv_len, v_scale=V_SCALE),
        lambda: kvcache_append(k[:, :, :NQ], v[:, :, :NQ], k, v, kv_len, v_scale=V_SCALE),
        lambda: kvcache_append_ref(k[:, :, :NQ], v[:, :, :NQ], k, v, kv_len, k_scale=K_SCALE),
    ):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize('page_size', [None, 32])
@pytest.mark.parametrize('n_kv_head', [None, 1])
def test_gpt2_on_an_fp8_cache_matches_a_bf16_cache_of_the_dequantised_rows(n_kv_head, page_size, monkeypatch):
    monkeypatch.setenv('DMLCLOUD_DISABLE_FUSED_ATTN', '1')
    torch.manual_seed(0)
    model = gpt2.gpt2_tiny(n_kv_head).eval()
    seq = torch.randint(0, 512, (2, 40))
    make = model.init_cache if page_size is None else lambda *a, **kw: model.init_paged_cache(*a, page_size=page_size, **kw)
    fp8, ref = make(2, 64, dtype=FP8), make(2, 64, dtype=torch.float32)
    assert fp8.k_scale[0].shape == (n_kv_head or 2,) and ref.k_scale is None
    for layer in range(2):
        fp8.k_scale[layer] = torch.full_like(fp8.k_scale[layer], 0.013)  # assignable
        fp8.v_scale[layer].fill_(0.007)

    def requantise():  # the reference cache holds exactly what the fp8 one dequantises to
        ref.kv_len.copy_(fp8.kv_len)
        for layer in range(2):
            ref.k[layer].copy_(fp8.k[layer].float() * 0.013)
            ref.v[layer].copy_(fp8.v[layer].float() * 0.007)

    for t in fp8.k + fp8.v:
        t.view(torch.uint8).fill_(0x7F)
    model.prefill(seq[:, :5], fp8)
    for step in (lambda c: model.decode_step(seq[:, 5], c), lambda c: model.extend(seq[:, 6:30], c)):
        requantise()
        got = step(fp8)
        # the new rows reach `ref` unquantised: only they differ, by at most e4m3's half ulp
        torch.testing.assert_close(got, step(ref), rtol=2e-2, atol=2e-2)
    assert int(fp8.kv_len[0]) == 30 and torch.isfinite(got).all()
