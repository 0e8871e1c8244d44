"""The paged K/V cache on the CPU: `kvcache_attention_ref(block_table=)` against
the dense reference on the gathered cache, `kvcache_append`'s torch path
against explicit index writes, and `GPT2.generate(page_size=)` against
`generate()`."""

import pytest
import torch

from dmlcloud_amd.models.gpt2 import gpt2_tiny
from dmlcloud_amd.ops import kvcache_append, sdpa_kvcache
from dmlcloud_amd.ops._attention_ref import kvcache_attention_ref


def _pools(num_pages, hkv, page_size, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(num_pages, hkv, page_size, d, generator=g), torch.randn(num_pages, hkv, page_size, d, generator=g)


@pytest.mark.parametrize('page_size', [32, 24])  # 24: not a multiple of 32
@pytest.mark.parametrize('nq,causal', [(1, True), (5, True), (4, False)])
def test_paged_reference_is_the_dense_reference_on_the_gathered_cache(page_size, nq, causal):
    B, H, Hkv, D, num_pages, max_pages = 2, 4, 2, 16, 9, 4
    k, v = _pools(num_pages, Hkv, page_size, D, 1)
    q = torch.randn(B, H, nq, D, generator=torch.Generator().manual_seed(2))
    # live entries out of range on both sides: they read as pages 0 and num_pages - 1
    table = torch.tensor([[7, -3, 2, 100], [num_pages + 5, 4, 1, 0]])
    clamped = table.clamp(0, num_pages - 1)
    kv_len = torch.tensor([3 * page_size + 1, 2 * page_size])
    dense = [torch.stack([torch.cat(list(t[clamped[b]]), dim=1) for b in range(B)]) for t in (k, v)]
    want = kvcache_attention_ref(q, *dense, kv_len, causal, return_lse=True)
    for tbl in (table, clamped):
        got = sdpa_kvcache(q, k, v, kv_len, causal=causal, return_lse=True, block_table=tbl)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize('paged', [False, True])
@pytest.mark.parametrize('nq', [1, 5])
def test_append_torch_path_is_index_writes(nq, paged):
    B, Hkv, D, page_size, num_pages = 2, 2, 16, 8, 7
    k_new, v_new = _pools(B, Hkv, nq, D, 3)
    table = torch.tensor([[5, 2, 6], [0, 3, 1]]) if paged else None
    shape = (num_pages, Hkv, page_size, D) if paged else (B, Hkv, 3 * page_size, D)
    k, v = torch.zeros(shape), torch.zeros(shape)
    want_k, want_v = k.clone(), v.clone()
    kv_len = [page_size + 2, nq]  # row 0 straddles a page boundary when nq = 5
    for b in range(B):
        for i in range(nq):
            pos = kv_len[b] - nq + i
            page, row = (int(table[b, pos // page_size]), pos % page_size) if paged else (b, pos)
            want_k[page, :, row], want_v[page, :, row] = k_new[b, :, i], v_new[b, :, i]
    kvcache_append(k_new, v_new, k, v, torch.tensor(kv_len), block_table=table)
    assert torch.equal(k, want_k) and torch.equal(v, want_v)


@pytest.mark.parametrize('n_kv_head', [None, 1])
def test_generate_on_a_paged_cache_returns_the_same_tokens(n_kv_head):
    torch.manual_seed(0)
    model = gpt2_tiny(n_kv_head).eval()
    prompt = torch.randint(0, 512, (2, 7))
    want = model.generate(prompt, 12)
    assert torch.equal(model.generate(prompt, 12, page_size=8), want)
    assert torch.equal(model.generate(prompt, 12, page_size=32, prefill_chunk=3), want)
