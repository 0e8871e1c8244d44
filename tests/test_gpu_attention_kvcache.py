"""Split-KV decode attention over a K/V cache (ops.sdpa_kvcache) against an
fp64 softmax on the CPU over the valid keys of the same bf16 inputs. On the
device every cache row at or past kv_len[b] holds NaN. num_splits 1 / 2 / 3
gives chunks of 384 / 256 / 128 keys; at S = 3 a length of 1 leaves two
splits without a key. Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools
import math

import pytest
import torch

from attn_testlib import bits, carve

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B, NMAX, D = 2, 320, 64
SCALE = 1.0 / math.sqrt(D)
# (H, Hkv, Nq, causal)
CONFIGS = [(4, 4, 1, True), (4, 1, 1, True), (16, 1, 1, True), (6, 2, 1, True)]
CONFIGS += [(4, 4, 4, True), (4, 4, 4, False), (4, 2, 5, True), (2, 2, 16, True)]
LENS = [(1, 300), (32, 33), (127, 129), (128, 320)]
# kv_len >= Nq is the causal contract: (1, 300) only with one query row
CASES = [(c, n) for c in CONFIGS for n in LENS if not (c[3] and c[2] > 1 and n == (1, 300))]


@functools.lru_cache(maxsize=None)
def _inputs(h, hkv, nq):
    """q [B, H, Nq, D], k and v [B, Hkv, NMAX, D]: bf16, CPU, never modified."""
    g = torch.Generator().manual_seed(7000 + 100 * h + 10 * hkv + nq)
    mk = lambda *shape: (torch.randn(*shape, generator=g) * 0.5).to(torch.bfloat16)
    return mk(B, h, nq, D), mk(B, hkv, NMAX, D), mk(B, hkv, NMAX, D)


@functools.lru_cache(maxsize=None)
def _oracle(h, hkv, nq, causal, lens):
    q, k, v = (t.double() for t in _inputs(h, hkv, nq))
    ln = torch.tensor(lens)
    last = ln[:, None] - nq + torch.arange(nq) if causal else (ln[:, None] - 1).expand(B, nq)
    s = torch.einsum('bkgqd,bknd->bkgqn', q.view(B, hkv, h // hkv, nq, D), k) * SCALE
    s = s.masked_fill(torch.arange(NMAX) > last[:, None, None, :, None], -float('inf'))
    o = torch.einsum('bkgqn,bknd->bkgqd', torch.softmax(s, -1), v)
    return o.reshape(B, h, nq, D), torch.logsumexp(s, -1).reshape(B, h, nq)


def _device(h, hkv, nq, lens):
    """The inputs on the device, NaN in the cache slack, and kv_len."""
    q, k, v = (t.to(DEV) for t in _inputs(h, hkv, nq))
    for b, n in enumerate(lens):
        k[b, :, n:] = float('nan')
        v[b, :, n:] = float('nan')
    return q, k, v, torch.tensor(lens, dtype=torch.int32, device=DEV)


def _run(h, hkv, nq, causal, lens, splits):
    from dmlcloud_amd.ops import fused_kvcache_usable, sdpa_kvcache

    q, k, v, kv_len = _device(h, hkv, nq, lens)
    assert fused_kvcache_usable(q, k, v, kv_len) is True
    return sdpa_kvcache(q, k, v, kv_len, causal=causal, num_splits=splits, return_lse=True)


def _assert_close(tag, got, want):
    o, lse = got[0].float().cpu(), got[1].cpu()
    assert torch.isfinite(o).all() and torch.isfinite(lse).all(), f'{tag}: not finite'
    print(f'{tag}: o err {(o - want[0]).abs().max():.3e}, lse err {(lse - want[1]).abs().max():.3e}')
    torch.testing.assert_close(o.double(), want[0], rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(lse.double(), want[1], rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize('splits', [1, 2, 3])
@pytest.mark.parametrize('cfg,lens', CASES)
def test_parity_with_fp64_softmax(cfg, lens, splits):
    _assert_close(f'{cfg} {lens} S={splits}', _run(*cfg, lens, splits), _oracle(*cfg, lens))


def test_auto_split_count():
    _assert_close('auto', _run(16, 1, 1, True, (129, 300), 0), _oracle(16, 1, 1, True, (129, 300)))


@pytest.mark.parametrize('h,hkv,nq', [(4, 1, 1), (4, 2, 5)])
def test_strided_cache_bit_identical(h, hkv, nq):
    """[B, Nmax, Hkv, 64] memory viewed as [B, Hkv, Nmax, 64], no copy."""
    from dmlcloud_amd.ops import sdpa_kvcache

    q, k, v, kv_len = _device(h, hkv, nq, (127, 300))
    ks, vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (k, v))
    assert ks.stride(2) == hkv * D and (hkv == 1 or not ks.is_contiguous())
    for a, b in zip(sdpa_kvcache(q, ks, vs, kv_len, num_splits=2, return_lse=True), _run(h, hkv, nq, True, (127, 300), 2)):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize('lens', [(1, 300), (128, 320)])
@pytest.mark.parametrize('splits', [1, 3])
def test_canaries_and_nan_workspace(splits, lens):
    from dmlcloud_amd import _C

    h, hkv, nq = 6, 2, 1
    q, k, v, kv_len = _device(h, hkv, nq, lens)
    bufs = {
        'o': carve(B * h * nq * D, 128 * D, torch.bfloat16, -7.5, DEV),
        'lse': carve(B * h * nq, 128, torch.float32, -12345.0, DEV),
        'ws': carve(_C.attn_decode_workspace_floats(B, hkv, splits), 128, torch.float32, -12345.0, DEV),
    }
    before = {name: bits(flat).clone() for name, (flat, _) in bufs.items()}
    o, lse = bufs['o'][1].view(B, h, nq, D), bufs['lse'][1].view(B, h, nq)
    _C.attn_decode(q, k, v, kv_len, o, lse, bufs['ws'][1], SCALE, True, splits)
    torch.cuda.synchronize()
    for name, (flat, front) in bufs.items():
        assert torch.equal(bits(flat)[front.numel() :], before[name][front.numel() :]), f'{name}: sentinel overwritten'
    assert not torch.isnan(o).any() and not torch.isnan(lse).any(), 'rows left unwritten'
    _assert_close(f'canaries S={splits} {lens}', (o, lse), _oracle(h, hkv, nq, True, lens))


def test_bitwise_repeatable():
    first, again = _run(4, 2, 5, True, (127, 300), 3), _run(4, 2, 5, True, (127, 300), 3)
    assert torch.equal(bits(first[0]), bits(again[0])) and torch.equal(bits(first[1]), bits(again[1]))


@pytest.mark.parametrize('h,hkv,nq,causal', [(4, 2, 5, True), (4, 4, 4, False)])
def test_malformed_kv_len_is_clamped(h, hkv, nq, causal):
    """[-5, 10_000] reads as [Nq or 1, Nmax]; the cache is then all valid."""
    from dmlcloud_amd.ops import sdpa_kvcache

    q, k, v = (t.to(DEV) for t in _inputs(h, hkv, nq))
    run = lambda lens: sdpa_kvcache(
        q, k, v, torch.tensor(lens, dtype=torch.int32, device=DEV), causal=causal, num_splits=3, return_lse=True
    )
    bad, good = run([-5, 10_000]), run([nq if causal else 1, NMAX])
    assert torch.isfinite(bad[0].float()).all() and torch.isfinite(bad[1]).all()
    assert torch.equal(bits(bad[0]), bits(good[0])) and torch.equal(bits(bad[1]), bits(good[1]))


def test_hipgraph_replay_follows_kv_len_and_cache():
    from dmlcloud_amd.ops import sdpa_kvcache

    h, hkv, nq, lens = 4, 1, 1, (129, 200)
    q, k, v, kv_len = _device(h, hkv, nq, lens)
    call = lambda: sdpa_kvcache(q, k, v, kv_len, num_splits=2, return_lse=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    graph.replay()
    _assert_close('replay 1', out, _oracle(h, hkv, nq, True, lens))
    # one more token per row: its cache row written and kv_len advanced on the device
    _, k_full, v_full = (t.to(DEV) for t in _inputs(h, hkv, nq))
    rows, batch = kv_len.long(), torch.arange(B, device=DEV)
    k[batch, :, rows] = k_full[batch, :, rows]
    v[batch, :, rows] = v_full[batch, :, rows]
    kv_len += 1
    for replay in (2, 3):
        graph.replay()
        _assert_close(f'replay {replay}', out, _oracle(h, hkv, nq, True, (130, 201)))


def test_launcher_rejections():
    """Each refused before any launch; the same buffers then serve a valid call."""
    from dmlcloud_amd import _C

    h, hkv, nq = 4, 2, 1
    q, k, v, kv_len = _device(h, hkv, nq, (127, 300))
    o, lse = torch.empty_like(q), torch.empty(B, h, nq, dtype=torch.float32, device=DEV)
    ws = torch.empty(_C.attn_decode_workspace_floats(B, hkv, 2), dtype=torch.float32, device=DEV)
    q20 = torch.zeros(B, 4, 10, D, dtype=torch.bfloat16, device=DEV)  # G * Nq = 20
    k3 = torch.zeros(B, 3, NMAX, D, dtype=torch.bfloat16, device=DEV)  # 3 does not divide 4
    q9 = torch.zeros(B, 2, 9, D, dtype=torch.bfloat16, device=DEV)  # Nmax = 8 < Nq = 9
    for bad in (
        dict(q=q.half()),
        dict(q=q20, o=torch.empty_like(q20), lse=torch.empty(B, 4, 10, dtype=torch.float32, device=DEV)),
        dict(k=k3, v=k3),
        dict(kv_len=kv_len.long()),
        dict(kv_len=kv_len.cpu()),
        dict(ws=ws[:-1]),
        dict(splits=math.ceil(NMAX / 128) + 1),
        dict(q=q9, k=k[:, :, :8], v=v[:, :, :8], o=torch.empty_like(q9), lse=torch.empty(B, 2, 9, dtype=torch.float32, device=DEV)),
    ):
        a = dict(q=q, k=k, v=v, kv_len=kv_len, o=o, lse=lse, ws=ws, splits=2)
        a.update(bad)
        with pytest.raises(RuntimeError):
            _C.attn_decode(a['q'], a['k'], a['v'], a['kv_len'], a['o'], a['lse'], a['ws'], SCALE, True, a['splits'])
    _C.attn_decode(q, k, v, kv_len, o, lse, ws, SCALE, True, 2)
    _assert_close('after rejections', (o, lse), _oracle(h, hkv, nq, True, (127, 300)))


@pytest.mark.parametrize('n_kv_head', [None, 1])
def test_gpt2_decode_end_to_end(n_kv_head, monkeypatch):
    """A D = 64 GPT-2 in bf16: every decode step takes the native path and
    its logits match the same model's full forward on the grown sequence."""
    from dmlcloud_amd.models import gpt2
    from dmlcloud_amd.ops import fused_attn

    cfg = gpt2.GPT2Config(vocab_size=512, n_positions=64, n_embd=128, n_layer=2, n_head=2, n_kv_head=n_kv_head)
    torch.manual_seed(0)
    model = gpt2.GPT2(cfg).to(DEV).to(torch.bfloat16).eval()
    native = []

    def checked(q, k_cache, v_cache, kv_len, **kw):
        native.append(fused_attn.fused_kvcache_usable(q, k_cache, v_cache, kv_len))
        return fused_attn.sdpa_kvcache(q, k_cache, v_cache, kv_len, **kw)

    monkeypatch.setattr(gpt2, 'sdpa_kvcache', checked)
    seq = torch.randint(0, cfg.vocab_size, (2, 5), device=DEV)
    cache = model.init_cache(2, 5 + 4, DEV, torch.bfloat16)
    with torch.no_grad():
        logits = model.prefill(seq, cache)
        for _ in range(4):
            seq = torch.cat([seq, logits.argmax(-1, keepdim=True)], dim=1)
            logits = model.decode_step(seq[:, -1], cache)
            torch.testing.assert_close(logits.float(), model(seq)[:, -1].float(), rtol=3e-2, atol=3e-2)
    assert native == [True] * (4 * cfg.n_layer)
