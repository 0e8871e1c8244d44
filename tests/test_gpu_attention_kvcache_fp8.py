"""sdpa_kvcache and kvcache_append over an FP8 (float8_e4m3fn) K/V cache:
attn_decode_fp8_kernel and kvcache_append_fp8_kernel of
ops/csrc/attention_decode_fp8.h. B = 2, capacity 320, dense and as pages of
32 / 64; q = randn * 4, k = randn * 0.5, v = randn, quantised on the CPU with
per-head scales that are distinct and no powers of two; byte 0x7F (NaN) in
every cache row >= kv_len[b] and in every dead page. The oracle is an fp64
softmax on the CPU over the DEQUANTISED cache, which is exactly what the kernel
multiplies (e4m3 -> bf16 is exact), so the bounds are the bf16 kernels', with no
extra margin (docs/KERNELS.md, "Head dim 128 in sdpa_kvcache"): o 3e-2, lse
1e-2, and max|o - ref| <= 6.3778e-3 * max|ref| per case. The largest normalised
error measured on an MI355X over the parity cases is in docs/KERNELS.md.
Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools
import math

import pytest
import torch

from attn_testlib import bits, carve

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FP8, NAN8 = torch.float8_e4m3fn, 0x7F
B, CAP = 2, 320
C_NORM = 6.3778e-3
# (H, Hkv, Nq, causal): R = 1; GQA decode; a short chunk; T = 2 with one column
# in the second tile; three live tiles; two tile groups, causal and full
CONFIGS = [(4, 4, 1, True), (6, 2, 1, True), (4, 2, 5, True), (1, 1, 17, True), (3, 1, 11, True), (4, 1, 20, True), (4, 1, 20, False)]
LENS = lambda nq: [(nq, 300), (128, 129), (129, 320)]


def _quant(x, s):
    return (x.float() / s.view(1, -1, 1, 1)).clamp(-448, 448).to(FP8)


@functools.lru_cache(maxsize=None)
def _inputs(h, hkv, nq, d):
    """q bf16, the e4m3 caches [B, Hkv, CAP, D] and their scales: CPU, never modified."""
    g = torch.Generator().manual_seed(7000 + 100 * h + 10 * hkv + nq + d)
    q = (torch.randn(B, h, nq, d, generator=g) * 4).to(torch.bfloat16)
    ks = 0.0071 + 0.0023 * torch.arange(hkv, dtype=torch.float32)
    vs = 0.0130 + 0.0041 * torch.arange(hkv, dtype=torch.float32)
    k = _quant(torch.randn(B, hkv, CAP, d, generator=g) * 0.5, ks)
    return q, k, _quant(torch.randn(B, hkv, CAP, d, generator=g), vs), ks, vs


@functools.lru_cache(maxsize=None)
def _oracle(h, hkv, nq, causal, d, lens):
    q, k, v, ks, vs = _inputs(h, hkv, nq, d)
    q, k, v = q.double(), k.double() * ks.double().view(1, -1, 1, 1), v.double() * vs.double().view(1, -1, 1, 1)
    ln = torch.tensor(lens)
    last = ln[:, None] - nq + torch.arange(nq) if causal else (ln[:, None] - 1).expand(B, nq)
    s = torch.einsum('bkgqd,bknd->bkgqn', q.view(B, hkv, h // hkv, nq, d), k) / math.sqrt(d)
    s = s.masked_fill(torch.arange(CAP) > last[:, None, None, :, None], -float('inf'))
    o = torch.einsum('bkgqn,bknd->bkgqd', torch.softmax(s, -1), v)
    return o.reshape(B, h, nq, d), torch.logsumexp(s, -1).reshape(B, h, nq)


def _device(h, hkv, nq, d, lens, page=0):
    """(q, k, v, kv_len, table, k_scale, v_scale) on the device, NaN bytes in
    all slack; page > 0: pools of 3 spare pages, scattered, dead entries -> a NaN page."""
    q, k, v, ks, vs = _inputs(h, hkv, nq, d)
    caches, table = [], None
    for c in (k, v):
        c = c.view(torch.uint8).clone()
        for b, n in enumerate(lens):
            c[b, :, n:] = NAN8
        if page:
            mp = CAP // page
            perm = torch.randperm(B * mp + 3, generator=torch.Generator().manual_seed(mp))
            table = perm[: B * mp].view(mp, B).t().contiguous()
            pool = torch.full((B * mp + 3, hkv, page, d), NAN8, dtype=torch.uint8)
            pool[table.flatten()] = c.view(B, hkv, mp, page, d).transpose(1, 2).reshape(B * mp, hkv, page, d)
            for b, n in enumerate(lens):
                table[b, -(-n // page) :] = perm[-1]
            c, table = pool, table.to(DEV, torch.int32)
        caches.append(c.to(DEV).view(FP8))
    return q.to(DEV), caches[0], caches[1], torch.tensor(lens, dtype=torch.int32, device=DEV), table, ks.to(DEV), vs.to(DEV)


def _run(args, causal=True, splits=3, **kw):
    from dmlcloud_amd.ops import fused_kvcache_usable, sdpa_kvcache

    q, k, v, kv_len, table, ks, vs = args
    assert fused_kvcache_usable(q, k, v, kv_len, table, ks, vs) is True
    kw = dict(dict(k_scale=ks, v_scale=vs), **kw)
    return sdpa_kvcache(q, k, v, kv_len, causal=causal, num_splits=splits, return_lse=True, block_table=table, **kw)


def _same_bits(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


def _assert_close(tag, got, want):
    o, lse = got[0].double().cpu(), got[1].double().cpu()
    err = float((o - want[0]).abs().max() / want[0].abs().max())
    print(f'{tag}: normalised o err {err:.4e}, lse err {(lse - want[1]).abs().max():.3e}')
    torch.testing.assert_close(o, want[0], rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(lse, want[1], rtol=1e-2, atol=1e-2)
    assert err <= C_NORM, f'{tag}: normalised error {err:.4e} > {C_NORM}'


@pytest.mark.parametrize('cfg', CONFIGS)
@pytest.mark.parametrize('splits', [1, 3])
@pytest.mark.parametrize('page', [0, 32, 64])
@pytest.mark.parametrize('d', [64, 128])
def test_parity_with_fp64_softmax_over_the_dequantised_cache(d, page, splits, cfg):
    h, hkv, nq, causal = cfg
    for lens in LENS(nq):
        got = _run(_device(h, hkv, nq, d, lens, page), causal, splits)
        _assert_close(f'D={d} page={page} S={splits} {cfg} {lens}', got, _oracle(h, hkv, nq, causal, d, lens))


@pytest.mark.parametrize('page', [0, 64])
@pytest.mark.parametrize('d', [64, 128])
def test_unit_scales_repeats_and_transposed_views_are_bit_identical(d, page):
    args = _device(4, 2, 5, d, (128, 300), page)
    first = _run(args)
    assert _same_bits(first, _run(args)), 'not repeatable'
    ones = torch.ones(2, device=DEV)
    assert _same_bits(_run(args, k_scale=None, v_scale=None), _run(args, k_scale=ones, v_scale=ones))
    ks, vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in args[1:3])  # [.., rows, Hkv, D] memory
    assert ks.stride(2) == 2 * d and not ks.is_contiguous()
    assert _same_bits(first, _run((args[0], ks, vs) + args[3:]))


@pytest.mark.parametrize('splits', [1, 3])
@pytest.mark.parametrize('h,hkv,nq,d', [(4, 4, 1, 64), (3, 1, 11, 128)])
def test_canaries_nan_workspace_and_malformed_kv_len(h, hkv, nq, d, splits):
    from dmlcloud_amd import _C

    q, k, v, kv_len, _, ks, vs = _device(h, hkv, nq, d, (nq, CAP))
    floats = _C.attn_decode_tiled_workspace_floats(B, hkv, h // hkv * nq, splits, d)
    bufs = {
        'o': carve(B * h * nq * d, 128 * d, torch.bfloat16, -7.5, DEV),
        'lse': carve(B * h * nq, 128, torch.float32, -12345.0, DEV),
        'ws': carve(floats, 128, torch.float32, -12345.0, DEV),
    }
    before = {name: bits(flat).clone() for name, (flat, _) in bufs.items()}
    o, lse = bufs['o'][1].view(B, h, nq, d), bufs['lse'][1].view(B, h, nq)
    bad_len = torch.tensor([-5, 10_000], dtype=torch.int32, device=DEV)  # reads as [Nq, CAP]
    _C.attn_decode_fp8(q, k, v, bad_len, o, lse, bufs['ws'][1], 1.0 / math.sqrt(d), True, splits, ks, vs)
    torch.cuda.synchronize()
    for name, (flat, front) in bufs.items():
        assert torch.equal(bits(flat)[front.numel() :], before[name][front.numel() :]), f'{name}: sentinel overwritten'
    assert _same_bits((o, lse), _run((q, k, v, kv_len, None, ks, vs), True, splits))
    _assert_close(f'canaries D={d} R={h // hkv * nq} S={splits}', (o, lse), _oracle(h, hkv, nq, True, d, (nq, CAP)))


@pytest.mark.parametrize('page', [0, 32, 48])
@pytest.mark.parametrize('nq', [1, 5])
@pytest.mark.parametrize('d', [64, 128])
def test_append_stores_the_torch_formula_and_nothing_else(d, nq, page):
    """Row 0 of every head: ties between e4m3 neighbours from the subnormals
    (|x / s| < 2^-6) to 432 (x = midpoint * s is exact in bf16 for these scales,
    so x / s IS the midpoint), and +-1e4, which must saturate to +-448."""
    from dmlcloud_amd import _C
    from dmlcloud_amd.ops._attention_ref import kvcache_append_ref

    hkv, g = 2, torch.Generator().manual_seed(d + nq + page)
    scales = torch.tensor([[0.75, 1.25], [1.5, 0.625]])
    vals = torch.arange(127, dtype=torch.uint8).view(FP8).float()  # 0 .. 448, ascending
    mids = ((vals[:-1] + vals[1:]) / 2)[::2][:63] * torch.tensor([1.0, -1.0]).repeat(32)[:63]
    new = (torch.randn(2, B, hkv, nq, d, generator=g) * 3).to(torch.bfloat16)
    new[:, :, :, 0, :63] = (mids * scales[:, None, :, None]).to(torch.bfloat16)
    new[:, :, :, 0, 63] = torch.tensor([1e4, -1e4])[:, None]  # per batch row
    assert torch.equal(new[0, 0, 1, 0, :63].float() / 1.25, mids)
    table = torch.tensor([[2, 0, 4], [1, 5, 3]], dtype=torch.int32) if page else None
    shape = (7, hkv, page, d) if page else (B, hkv, 96, d)
    caches = [torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) for _ in range(2)]
    kv_len = torch.tensor([(page or 32) + 2, nq], dtype=torch.int32)  # Nq = 5 straddles a page boundary
    want = [c.clone().view(FP8) for c in caches]
    kvcache_append_ref(new[0], new[1], want[0], want[1], kv_len, table, scales[0], scales[1])
    assert (want[0].view(torch.uint8) == 0x7E).any() and (want[0].view(torch.uint8) == 0xFE).any()  # +-448
    got = [c.to(DEV).view(FP8) for c in caches]
    on = lambda t: None if t is None else t.to(DEV)
    _C.kvcache_append_fp8(on(new[0]), on(new[1]), got[0], got[1], on(kv_len), on(scales[0]), on(scales[1]), on(table))
    for name, a, b in zip('kv', got, want):
        diff = a.cpu().view(torch.uint8) != b.view(torch.uint8)
        assert not diff.any(), f'{name}: {int(diff.sum())} bytes differ, first at {diff.nonzero()[0].tolist()}'


def test_hipgraph_replay_follows_kv_len_a_scale_and_the_table():
    from dmlcloud_amd.ops import kvcache_append, sdpa_kvcache

    h, hkv, nq, d = 4, 2, 5, 64
    q, kp, vp, kv_len, table, ks, vs = _device(h, hkv, nq, d, (70, 140), 64)  # rows up to (70, 140) are real
    g = torch.Generator().manual_seed(1)
    k_new, v_new = ((torch.randn(B, hkv, nq, d, generator=g) * 0.5).to(DEV, torch.bfloat16) for _ in range(2))
    kv_len.copy_(torch.tensor([64, 129]))

    def call():
        kvcache_append(k_new, v_new, kp, vp, kv_len, table, k_scale=ks, v_scale=vs)
        return sdpa_kvcache(q, kp, vp, kv_len, num_splits=3, return_lse=True, block_table=table, k_scale=ks, v_scale=vs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [t.clone() for t in call()]
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for _ in range(2):
        graph.replay()
        assert _same_bits(out, first)
    kv_len.copy_(torch.tensor([70, 140])), ks[1].mul_(1.37), table[0, 0].copy_(table[1, 0])
    for _ in range(2):
        graph.replay()
        replayed = [t.clone() for t in out]
        assert _same_bits(replayed, call()) and not _same_bits(replayed, first)


@pytest.mark.parametrize('page', [None, 32])
@pytest.mark.parametrize('n_kv_head', [None, 1])
def test_gpt2_fp8_cache_native_against_the_reference_path(n_kv_head, page, monkeypatch):
    from dmlcloud_amd.models import gpt2

    cfg = gpt2.GPT2Config(vocab_size=512, n_positions=64, n_embd=128, n_layer=2, n_head=2, n_kv_head=n_kv_head)
    torch.manual_seed(0)
    model = gpt2.GPT2(cfg).to(DEV).to(torch.bfloat16).eval()
    seq = torch.randint(0, cfg.vocab_size, (2, 40), device=DEV)
    logits = []
    for disable in ('0', '1'):
        monkeypatch.setenv('DMLCLOUD_DISABLE_FUSED_ATTN', disable)
        cache = model.init_cache(2, 64, dtype=FP8) if page is None else model.init_paged_cache(2, 64, page, dtype=FP8)
        for layer in range(cfg.n_layer):
            cache.k_scale[layer].fill_(0.013), cache.v_scale[layer].fill_(0.007)
        out = [model.prefill(seq[:, :5], cache)] + [model.decode_step(seq[:, 5 + i], cache) for i in range(3)]
        logits.append(out + [model.extend(seq[:, 8:28], cache)])
    for a, b in zip(*logits):
        assert torch.isfinite(a.float()).all()
        torch.testing.assert_close(a.float(), b.float(), rtol=3e-2, atol=3e-2)


def test_launcher_rejections():
    """Each refused before any launch; the same buffers then serve a valid call."""
    from dmlcloud_amd import _C
    from dmlcloud_amd.ops import fused_kvcache_usable

    h, hkv, nq, d, lens = 4, 2, 1, 64, (64, 129)
    q, k, v, kv_len, _, ks, vs = _device(h, hkv, nq, d, lens)
    o, lse = torch.empty_like(q), torch.empty(B, h, nq, dtype=torch.float32, device=DEV)
    ws = torch.empty(_C.attn_decode_tiled_workspace_floats(B, hkv, h // hkv * nq, 2, d), dtype=torch.float32, device=DEV)
    wide = torch.zeros(B, hkv, CAP, d + 8, dtype=torch.uint8, device=DEV).view(FP8)[..., :d]  # row stride 72
    k48 = torch.zeros(7, hkv, 48, d, dtype=torch.uint8, device=DEV).view(FP8)
    table = torch.zeros(B, 7, dtype=torch.int32, device=DEV)
    assert fused_kvcache_usable(q, k48, k48, kv_len, table) is False
    other = [ks.to('cuda:1')] if torch.cuda.device_count() > 1 else []
    bad = [dict(k=k.view(torch.float8_e5m2)), dict(ks=ks.bfloat16()), dict(ks=torch.ones(hkv + 1, device=DEV))]
    bad += [dict(vs=s) for s in [vs.cpu()] + other] + [dict(k=wide), dict(k=k48, v=k48, table=table)]
    for change in bad:
        a = dict(dict(k=k, v=v, ks=ks, vs=vs, table=None), **change)
        with pytest.raises(RuntimeError):
            _C.attn_decode_fp8(q, a['k'], a['v'], kv_len, o, lse, ws, 0.125, True, 2, a['ks'], a['vs'], a['table'])
    _C.attn_decode_fp8(q, k, v, kv_len, o, lse, ws, 0.125, True, 2, ks, vs)
    assert _same_bits((o, lse), _run((q, k, v, kv_len, None, ks, vs), True, 2))
