"""sdpa_kvcache over a PAGED K/V cache (the paged instantiations of the tiled
split-KV kernels, _C.attn_decode_tiled(..., block_table)) and kvcache_append.
B = 2; a logical cache of 384 keys as pages of 32 / 64 / 128, and 512 keys as
pages of 256. The pool holds more pages than the table names; pages are handed
out by a fixed random permutation, interleaved between the batch rows. NaN
fills every unused page, every row at or past kv_len[b] of a live page, and
one poison page that all dead table entries name. Two checks per case: an fp64
softmax on the CPU over the gathered keys (o 3e-2, lse 1e-2), and bit identity
with _C.attn_decode_tiled on the dense cache gathered from the same pages.
Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools
import math

import pytest
import torch

from attn_testlib import bits

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B = 2
CAPACITY = {32: 384, 64: 384, 128: 384, 256: 512}  # page_size -> logical capacity
# (H, Hkv, Nq, causal)
CONFIGS = [(4, 4, 1, True), (16, 1, 1, True), (4, 1, 5, True), (3, 1, 11, True), (4, 1, 20, False)]
# one key | the first row of a second page | a page and chunk boundary | a full table
LENS = lambda nq, causal: [n for n in [(nq, 300), (32, 33), (64, 129), (128, 384)] if not (causal and min(n) < nq)]


@functools.lru_cache(maxsize=None)
def _inputs(h, hkv, nq, d, cap):
    """q [B, H, Nq, D], the logical k and v [B, Hkv, cap, D]: bf16, CPU, never modified."""
    g = torch.Generator().manual_seed(9000 + 100 * h + 10 * hkv + nq + d + cap)
    mk = lambda *shape: (torch.randn(*shape, generator=g) * 0.5).to(torch.bfloat16)
    return mk(B, h, nq, d), mk(B, hkv, cap, d), mk(B, hkv, cap, d)


@functools.lru_cache(maxsize=None)
def _oracle(h, hkv, nq, causal, d, cap, lens):
    q, k, v = (t.double() for t in _inputs(h, hkv, nq, d, cap))
    ln = torch.tensor(lens)
    last = ln[:, None] - nq + torch.arange(nq) if causal else (ln[:, None] - 1).expand(B, nq)
    s = torch.einsum('bkgqd,bknd->bkgqn', q.view(B, hkv, h // hkv, nq, d), k) / math.sqrt(d)
    s = s.masked_fill(torch.arange(cap) > last[:, None, None, :, None], -float('inf'))
    o = torch.einsum('bkgqn,bknd->bkgqd', torch.softmax(s, -1), v)
    return o.reshape(B, h, nq, d), torch.logsumexp(s, -1).reshape(B, h, nq)


def _table(max_pages, shift=0):
    """(table [B, max_pages] CPU, poison page, num_pages): fixed permutation, interleaved."""
    num_pages = B * max_pages + 3
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(max_pages)).roll(shift)
    return perm[: B * max_pages].view(max_pages, B).t().contiguous(), int(perm[B * max_pages]), num_pages


def _paged(dense, lens, page_size, shift=0):
    """dense [B, Hkv, cap, D] (device) -> (NaN-poisoned pool, int32 device table)."""
    max_pages = dense.shape[2] // page_size
    table, poison, num_pages = _table(max_pages, shift)
    pool = torch.full((num_pages, dense.shape[1], page_size, dense.shape[3]), float('nan'), dtype=dense.dtype, device=DEV)
    for b, n in enumerate(lens):
        for p in range(max_pages):
            if p * page_size >= n:
                table[b, p] = poison
                continue
            rows = min(page_size, n - p * page_size)
            pool[table[b, p], :, :rows] = dense[b, :, p * page_size : p * page_size + rows]
    return pool, table.to(DEV, torch.int32)


def _device(h, hkv, nq, d, cap, lens):
    q, k, v = (t.to(DEV) for t in _inputs(h, hkv, nq, d, cap))
    for b, n in enumerate(lens):
        k[b, :, n:] = float('nan')
        v[b, :, n:] = float('nan')
    return q, k, v, torch.tensor(lens, dtype=torch.int32, device=DEV)


def _dense_tiled(q, k, v, kv_len, causal, splits):
    from dmlcloud_amd import _C

    (_, h, nq, d), hkv = q.shape, k.shape[1]
    o, lse = torch.empty_like(q), torch.empty(B, h, nq, dtype=torch.float32, device=DEV)
    ws = torch.empty(_C.attn_decode_tiled_workspace_floats(B, hkv, h // hkv * nq, splits, d), dtype=torch.float32, device=DEV)
    _C.attn_decode_tiled(q, k, v, kv_len, o, lse, ws, 1.0 / math.sqrt(d), causal, splits)
    return o, lse


def _same_bits(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize('page_size', list(CAPACITY))
@pytest.mark.parametrize('splits', [1, 3])
@pytest.mark.parametrize('cfg', CONFIGS)
@pytest.mark.parametrize('d', [64, 128])
def test_parity_with_fp64_softmax_and_the_dense_kernels(d, cfg, splits, page_size):
    from dmlcloud_amd.ops import fused_kvcache_usable, sdpa_kvcache

    (h, hkv, nq, causal), cap = cfg, CAPACITY[page_size]
    for lens in LENS(nq, causal):
        q, k, v, kv_len = _device(h, hkv, nq, d, cap, lens)
        (kp, table), (vp, _) = _paged(k, lens, page_size), _paged(v, lens, page_size)
        assert fused_kvcache_usable(q, kp, vp, kv_len, table) is True
        got = sdpa_kvcache(q, kp, vp, kv_len, causal=causal, num_splits=splits, return_lse=True, block_table=table)
        want = _oracle(h, hkv, nq, causal, d, cap, lens)
        o, lse = got[0].float().cpu(), got[1].cpu()
        assert torch.isfinite(o).all() and torch.isfinite(lse).all(), f'{lens}: not finite'
        print(f'{lens}: o err {(o - want[0]).abs().max():.3e}, lse err {(lse - want[1]).abs().max():.3e}')
        torch.testing.assert_close(o.double(), want[0], rtol=3e-2, atol=3e-2)
        torch.testing.assert_close(lse.double(), want[1], rtol=1e-2, atol=1e-2)
        assert _same_bits(got, _dense_tiled(q, k, v, kv_len, causal, splits)), f'{lens}: bits differ from the dense cache'


@pytest.mark.parametrize('d', [64, 128])
def test_transposed_pool_and_repeat_are_bit_identical(d):
    """[num_pages, page_size, Hkv, D] memory viewed as [num_pages, Hkv, page_size, D], no copy."""
    from dmlcloud_amd.ops import sdpa_kvcache

    h, hkv, nq, lens = 4, 2, 5, (64, 129)
    q, k, v, kv_len = _device(h, hkv, nq, d, 384, lens)
    (kp, table), (vp, _) = _paged(k, lens, 64), _paged(v, lens, 64)
    run = lambda a, b: sdpa_kvcache(q, a, b, kv_len, num_splits=3, return_lse=True, block_table=table)
    ks, vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (kp, vp))
    assert ks.stride(2) == hkv * d and not ks.is_contiguous()
    first = run(kp, vp)
    assert _same_bits(first, run(ks, vs)) and _same_bits(first, run(kp, vp))


@pytest.mark.parametrize('paged', [False, True])
@pytest.mark.parametrize('page_size', [32, 48])
@pytest.mark.parametrize('nq', [1, 5])
@pytest.mark.parametrize('d', [64, 128])
def test_append_writes_the_target_rows_and_nothing_else(d, nq, page_size, paged):
    from dmlcloud_amd import _C
    from dmlcloud_amd.ops._attention_ref import kvcache_append_ref

    h, hkv = 2, 2
    g = torch.Generator().manual_seed(d + nq + page_size)
    qkv = torch.randn(B, nq, (h + 2 * hkv) * d, generator=g).to(DEV, torch.bfloat16)
    k_new, v_new = (t.view(B, nq, hkv, d).transpose(1, 2) for t in qkv.split([h * d, hkv * d, hkv * d], dim=2)[1:])
    table, _, num_pages = _table(3)
    table = table.to(DEV, torch.int32) if paged else None
    shape = (num_pages, hkv, page_size, d) if paged else (B, hkv, 3 * page_size, d)
    k, v = (torch.randn(shape, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    kv_len = torch.tensor([page_size + 2, nq], dtype=torch.int32, device=DEV)  # Nq = 5 straddles a page boundary
    want_k, want_v = k.clone(), v.clone()
    kvcache_append_ref(k_new, v_new, want_k, want_v, kv_len, table)
    assert not torch.equal(want_k, k)
    _C.kvcache_append(k_new, v_new, k, v, kv_len, table)
    assert torch.equal(bits(k), bits(want_k)) and torch.equal(bits(v), bits(want_v))


def test_hipgraph_replay_follows_moved_pages():
    from dmlcloud_amd.ops import kvcache_append, sdpa_kvcache

    h, hkv, nq, d, lens, page_size = 4, 1, 5, 64, (64, 129), 64
    q, k, v, kv_len = _device(h, hkv, nq, d, 384, lens)
    rows = torch.tensor(lens, device=DEV)[:, None] - nq + torch.arange(nq, device=DEV)  # the new tokens' rows
    batch = torch.arange(B, device=DEV)[:, None]
    k_new, v_new = k[batch, :, rows].transpose(1, 2), v[batch, :, rows].transpose(1, 2)

    def pools(shift):  # the new rows are NaN until kvcache_append writes them
        kd, vd = k.clone(), v.clone()
        kd[batch, :, rows] = vd[batch, :, rows] = float('nan')
        return _paged(kd, lens, page_size, shift) + _paged(vd, lens, page_size, shift)[:1]

    kp, table, vp = pools(0)

    def call():
        kvcache_append(k_new, v_new, kp, vp, kv_len, table)
        return sdpa_kvcache(q, kp, vp, kv_len, num_splits=3, return_lse=True, block_table=table)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in call()]
    torch.cuda.current_stream().wait_stream(side)
    assert _same_bits(eager, _dense_tiled(q, k, v, kv_len, True, 3))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for shift in (0, 3, 7):  # every live page in another pool slot, the table rewritten on the device
        kp2, table2, vp2 = pools(shift)
        assert shift == 0 or not torch.equal(table2, table)
        kp.copy_(kp2), vp.copy_(vp2), table.copy_(table2)
        graph.replay()
        assert _same_bits(out, eager), f'replay after shift {shift}'


@pytest.mark.parametrize('n_kv_head', [None, 1])
def test_gpt2_paged_cache_is_bit_identical_to_the_dense_cache(n_kv_head):
    from dmlcloud_amd.models import gpt2

    cfg = gpt2.GPT2Config(vocab_size=512, n_positions=64, n_embd=128, n_layer=2, n_head=2, n_kv_head=n_kv_head)
    torch.manual_seed(0)
    model = gpt2.GPT2(cfg).to(DEV).to(torch.bfloat16).eval()
    seq = torch.randint(0, cfg.vocab_size, (2, 40), device=DEV)
    dense = model.init_cache(2, 64, DEV, torch.bfloat16)
    table = torch.tensor([[3, 0], [1, 4]], device=DEV)
    paged = model.init_paged_cache(2, 64, page_size=32, num_pages=5, block_table=table)
    for cache in (dense, paged):
        cache.logits = [model.prefill(seq[:, :5], cache), model.decode_step(seq[:, 5], cache)]
        cache.logits += [model.extend(seq[:, 6:36], cache), model.decode_step(seq[:, 36], cache)]  # crosses row 32
    for a, b in zip(dense.logits, paged.logits):
        assert torch.isfinite(a.float()).all() and torch.equal(bits(a), bits(b))


def test_launcher_rejections():
    """Each refused before any launch; the same buffers then serve a valid call."""
    from dmlcloud_amd import _C

    h, hkv, nq, d, lens = 4, 2, 1, 64, (64, 129)
    q, k, v, kv_len = _device(h, hkv, nq, d, 384, lens)
    (kp, table), (vp, _) = _paged(k, lens, 64), _paged(v, lens, 64)
    o, lse = torch.empty_like(q), torch.empty(B, h, nq, dtype=torch.float32, device=DEV)
    ws = torch.empty(_C.attn_decode_tiled_workspace_floats(B, hkv, h // hkv * nq, 2, d), dtype=torch.float32, device=DEV)
    k48 = torch.zeros(kp.shape[0], hkv, 48, d, dtype=torch.bfloat16, device=DEV)
    for bad in (dict(k=k48, v=k48), dict(table=table.cpu()), dict(table=table.float()), dict(v=vp[:-1])):
        a = dict(k=kp, v=vp, table=table)
        a.update(bad)
        with pytest.raises(RuntimeError):
            _C.attn_decode_tiled(q, a['k'], a['v'], kv_len, o, lse, ws, 0.125, True, 2, a['table'])
    _C.attn_decode_tiled(q, kp, vp, kv_len, o, lse, ws, 0.125, True, 2, table)
    assert _same_bits((o, lse), _dense_tiled(q, k, v, kv_len, True, 2))
