"""sdpa_kvcache with more than 16 query columns per K/V head (the tiled
split-KV kernels, _C.attn_decode_tiled) against an fp64 softmax on the CPU
over the valid keys of the same bf16 inputs. On the device every cache row at
or past kv_len[b] holds NaN. num_splits 1 / 2 / 3 gives chunks of 384 / 256 /
128 keys. Run on an MI355X box: python -m pytest tests -m gpu
"""

import math

import pytest
import torch

from attn_testlib import bits, carve

# the decode tests' inputs (B = 2, Nmax = 320, NaN in the cache slack), fp64
# oracle and tolerances (o 3e-2, lse 1e-2) serve any (H, Hkv, Nq)
from test_gpu_attention_kvcache import B, D, DEV, NMAX, SCALE, _assert_close, _device, _inputs, _oracle, _run

pytestmark = pytest.mark.gpu

# (H, Hkv, Nq, causal): R = 17 (T = 2, one column in the second tile), 20 (head
# boundaries inside tiles), 32, 33 (three live tiles), 64, 80 (two tile groups)
CONFIGS = [(1, 1, 17, True), (4, 1, 5, True), (2, 2, 32, True), (3, 1, 11, True)]
CONFIGS += [(4, 1, 16, True), (4, 1, 20, True), (4, 1, 20, False)]
# kv_len >= Nq is the causal contract: a pair with a shorter length would be dropped
CASES = [(c, n) for c in CONFIGS for n in [(c[2], 300), (128, 129), (129, 320)] if not (c[3] and min(n) < c[2])]


def _direct(h, hkv, nq, causal, lens, splits):
    """_C.attn_decode_tiled itself, whatever R is."""
    from dmlcloud_amd import _C

    q, k, v, kv_len = _device(h, hkv, nq, lens)
    o, lse = torch.empty_like(q), torch.empty(B, h, nq, dtype=torch.float32, device=DEV)
    ws = torch.empty(_C.attn_decode_tiled_workspace_floats(B, hkv, h // hkv * nq, splits), dtype=torch.float32, device=DEV)
    _C.attn_decode_tiled(q, k, v, kv_len, o, lse, ws, SCALE, causal, splits)
    return o, lse


def _same_bits(a, b):
    return torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize('splits', [1, 2, 3])
@pytest.mark.parametrize('cfg,lens', CASES)
def test_parity_with_fp64_softmax(cfg, lens, splits):
    _assert_close(f'{cfg} {lens} S={splits}', _run(*cfg, lens, splits), _oracle(*cfg, lens))


def test_auto_split_count_and_usable():
    _assert_close('auto', _run(4, 1, 5, True, (129, 300), 0), _oracle(4, 1, 5, True, (129, 300)))


def test_sixteen_columns_keep_the_decode_path():
    from dmlcloud_amd import _C

    q, k, v, kv_len = _device(2, 2, 16, (128, 320))
    o, lse = torch.empty_like(q), torch.empty(B, 2, 16, dtype=torch.float32, device=DEV)
    ws = torch.empty(_C.attn_decode_workspace_floats(B, 2, 2), dtype=torch.float32, device=DEV)
    _C.attn_decode(q, k, v, kv_len, o, lse, ws, SCALE, True, 2)
    assert _same_bits(_run(2, 2, 16, True, (128, 320), 2), (o, lse))


@pytest.mark.parametrize('splits', [1, 3])
@pytest.mark.parametrize('h,hkv,nq', [(4, 2, 5), (2, 2, 16), (1, 1, 1)])
def test_tiled_binding_at_one_tile(h, hkv, nq, splits):
    lens = (128, 320)
    _assert_close(f'T=1 R={h // hkv * nq} S={splits}', _direct(h, hkv, nq, True, lens, splits), _oracle(h, hkv, nq, True, lens))


@pytest.mark.parametrize('lens', [(20, 300), (129, 320)])
@pytest.mark.parametrize('splits', [1, 3])
def test_canaries_and_nan_workspace(splits, lens):
    from dmlcloud_amd import _C

    h, hkv, nq = 4, 1, 20
    q, k, v, kv_len = _device(h, hkv, nq, lens)
    bufs = {
        'o': carve(B * h * nq * D, 128 * D, torch.bfloat16, -7.5, DEV),
        'lse': carve(B * h * nq, 128, torch.float32, -12345.0, DEV),
        'ws': carve(_C.attn_decode_tiled_workspace_floats(B, hkv, h * nq, splits), 128, torch.float32, -12345.0, DEV),
    }
    before = {name: bits(flat).clone() for name, (flat, _) in bufs.items()}
    o, lse = bufs['o'][1].view(B, h, nq, D), bufs['lse'][1].view(B, h, nq)
    _C.attn_decode_tiled(q, k, v, kv_len, o, lse, bufs['ws'][1], SCALE, True, splits)
    torch.cuda.synchronize()
    for name, (flat, front) in bufs.items():
        assert torch.equal(bits(flat)[front.numel() :], before[name][front.numel() :]), f'{name}: sentinel overwritten'
    assert not torch.isnan(o).any() and not torch.isnan(lse).any(), 'rows left unwritten'
    _assert_close(f'canaries S={splits} {lens}', (o, lse), _oracle(h, hkv, nq, True, lens))


def test_bitwise_repeatable():
    assert _same_bits(_run(3, 1, 11, True, (128, 300), 3), _run(3, 1, 11, True, (128, 300), 3))


@pytest.mark.parametrize('h,hkv,nq,causal', [(4, 1, 5, True), (4, 1, 20, False)])
def test_malformed_kv_len_is_clamped(h, hkv, nq, causal):
    """[-5, 10_000] reads as [Nq or 1, Nmax]; the cache is then all valid."""
    from dmlcloud_amd.ops import sdpa_kvcache

    q, k, v = (t.to(DEV) for t in _inputs(h, hkv, nq))
    run = lambda lens: sdpa_kvcache(
        q, k, v, torch.tensor(lens, dtype=torch.int32, device=DEV), causal=causal, num_splits=3, return_lse=True
    )
    bad, good = run([-5, 10_000]), run([nq if causal else 1, NMAX])
    assert torch.isfinite(bad[0].float()).all() and torch.isfinite(bad[1]).all()
    assert _same_bits(bad, good)


def test_strided_cache_bit_identical():
    """[B, Nmax, Hkv, 64] memory viewed as [B, Hkv, Nmax, 64], no copy."""
    from dmlcloud_amd.ops import sdpa_kvcache

    h, hkv, nq = 2, 2, 32
    q, k, v, kv_len = _device(h, hkv, nq, (128, 300))
    ks, vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (k, v))
    assert ks.stride(2) == hkv * D and not ks.is_contiguous()
    got = sdpa_kvcache(q, ks, vs, kv_len, num_splits=2, return_lse=True)
    assert _same_bits(got, _run(h, hkv, nq, True, (128, 300), 2))


def test_empty_cache_chunk_agrees_with_sdpa():
    """kv_len = Nq is plain causal self-attention over the chunk."""
    from dmlcloud_amd.ops import sdpa

    h, hkv, nq = 2, 2, 32
    q, k, v, _ = _device(h, hkv, nq, (nq, nq))
    want = sdpa(q, k[:, :, :nq], v[:, :, :nq], causal=True)
    got = _run(h, hkv, nq, True, (nq, nq), 1)[0]
    torch.testing.assert_close(got.float(), want.float(), rtol=3e-2, atol=3e-2)


def test_launcher_rejections():
    """Each refused before any launch; the same buffers then serve a valid call."""
    from dmlcloud_amd import _C

    h, hkv, nq = 4, 2, 10
    q, k, v, kv_len = _device(h, hkv, nq, (128, 300))
    o, lse = torch.empty_like(q), torch.empty(B, h, nq, dtype=torch.float32, device=DEV)
    ws = torch.empty(_C.attn_decode_tiled_workspace_floats(B, hkv, 20, 2), dtype=torch.float32, device=DEV)
    k3 = torch.zeros(B, 3, NMAX, D, dtype=torch.bfloat16, device=DEV)  # 3 does not divide 4
    for bad in (
        dict(q=q.half()),
        dict(k=k3, v=k3),
        dict(kv_len=kv_len.long()),
        dict(kv_len=kv_len.cpu()),
        dict(ws=ws[:-1]),
        dict(splits=math.ceil(NMAX / 128) + 1),
        dict(k=k[:, :, :8], v=v[:, :, :8]),  # Nmax = 8 < Nq = 10
    ):
        a = dict(q=q, k=k, v=v, kv_len=kv_len, o=o, lse=lse, ws=ws, splits=2)
        a.update(bad)
        with pytest.raises(RuntimeError):
            _C.attn_decode_tiled(a['q'], a['k'], a['v'], a['kv_len'], a['o'], a['lse'], a['ws'], SCALE, True, a['splits'])
    _C.attn_decode_tiled(q, k, v, kv_len, o, lse, ws, SCALE, True, 2)
    _assert_close('after rejections', (o, lse), _oracle(h, hkv, nq, True, (128, 300)))


@pytest.mark.parametrize('n_kv_head', [None, 1])
def test_gpt2_extend_end_to_end(n_kv_head, monkeypatch):
    """A D = 64 GPT-2 in bf16: a 40-token prompt in chunks of 24 and 16, then
    20 more tokens on the filled cache; every layer's call takes the native
    path and the logits match the model's full forward on the grown sequence."""
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
    seq = torch.randint(0, cfg.vocab_size, (2, 60), device=DEV)
    cache = model.init_cache(2, 60, DEV, torch.bfloat16)
    with torch.no_grad():
        for end, chunk in ((24, 24), (40, 16), (60, 20)):
            logits = model.extend(seq[:, end - chunk : end], cache)
            torch.testing.assert_close(logits.float(), model(seq[:, :end])[:, -1].float(), rtol=3e-2, atol=3e-2)
    assert native == [True] * (3 * cfg.n_layer)
