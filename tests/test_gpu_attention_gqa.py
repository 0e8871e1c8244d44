"""Grouped-query attention in the MFMA kernels (their kGqa instantiations:
query head h reads K/V head h // G in place; one dK/dV block per K/V head
sums the group's heads in its fp32 accumulators).

B = 2, D = 64, bf16; (H, Hkv) = (4, 1) MQA, (4, 2) G = 2, (6, 2) a group of
3; N = 1 (one row), 33 (the 32-row step), 64 (one aligned block), 100 and
129 (ragged, on each side of the 128-row forward block). K/V are drawn
independently per K/V head, so a wrong head mapping shows.

Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools
import math

import pytest
import torch

from attn_testlib import assert_fwd_bwd_close as _assert_close
from attn_testlib import bits, carve

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B, D = 2, 64
SCALE = 1.0 / math.sqrt(D)
HEADS = [(4, 1), (4, 2), (6, 2)]
LENGTHS = [1, 33, 64, 100, 129]
# three documents per row, boundaries off the 32- and 64-row edges
DOC_N = 129
DOC_BOUNDS = ([0, 37, 91, DOC_N], [0, 50, 101, DOC_N])


@functools.lru_cache(maxsize=None)
def _inputs(h, hkv, n):
    """q, dO [B, H, n, D] and k, v [B, Hkv, n, D], bf16 on the device; never
    modified."""
    g = torch.Generator().manual_seed(3000 + 100 * h + 10 * hkv + n)

    def mk(heads):
        return (torch.randn(B, heads, n, D, generator=g) * 0.5).to(torch.bfloat16).to(DEV)

    return mk(h), mk(hkv), mk(hkv), mk(h)


@functools.lru_cache(maxsize=None)
def _doc_start():
    rows = []
    for bounds in DOC_BOUNDS:
        ds = torch.empty(DOC_N, dtype=torch.int32)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            ds[lo:hi] = lo
        rows.append(ds)
    return torch.stack(rows).to(DEV)


def _direct(q, k, v, do, causal, doc_start=None):
    """Forward and backward through the direct bindings into NaN-filled
    outputs: (o, lse, dq, dk, dv)."""
    from dmlcloud_amd import _C

    b, h, n, d = q.shape
    nan16 = lambda shape: torch.full(shape, float('nan'), dtype=torch.bfloat16, device=DEV)
    o, dq, dk, dv = nan16(q.shape), nan16(q.shape), nan16(k.shape), nan16(k.shape)
    lse = torch.full((b, h, n), float('nan'), dtype=torch.float32, device=DEV)
    delta = torch.empty(b * h * n, dtype=torch.float32, device=DEV)
    _C.attn_fwd(q, k, v, o, lse, SCALE, causal, doc_start)
    _C.attn_bwd(q, k, v, do, o, lse, dq, dk, dv, delta, SCALE, causal, doc_start)
    return o, lse, dq, dk, dv


@functools.lru_cache(maxsize=None)
def _gqa(h, hkv, n, causal, doc=False):
    q, k, v, do = _inputs(h, hkv, n)
    return _direct(q, k, v, do, causal, _doc_start() if doc else None)


@functools.lru_cache(maxsize=None)
def _mha_on_expanded(h, hkv, n, causal, doc=False):
    """The native MHA kernels on repeat_interleave'd K and V."""
    q, k, v, do = _inputs(h, hkv, n)
    g = h // hkv
    return _direct(q, k.repeat_interleave(g, 1), v.repeat_interleave(g, 1), do, causal, _doc_start() if doc else None)


@functools.lru_cache(maxsize=None)
def _reference(h, hkv, n, causal, doc=False):
    """fp32 SDPA with enable_gqa=True + autograd on the bf16-rounded inputs:
    (out, dq, dk, dv)."""
    from dmlcloud_amd.ops.fused_attn import document_mask

    q, k, v, do = _inputs(h, hkv, n)
    q2, k2, v2 = (t.float().requires_grad_(True) for t in (q, k, v))
    if doc:
        ref = torch.nn.functional.scaled_dot_product_attention(
            q2, k2, v2, attn_mask=document_mask(_doc_start(), True), enable_gqa=True
        )
    else:
        ref = torch.nn.functional.scaled_dot_product_attention(q2, k2, v2, is_causal=causal, enable_gqa=True)
    ref.backward(do.float())
    return ref.detach(), q2.grad, k2.grad, v2.grad


def _sdpa_native(h, hkv, n, causal, doc=False):
    from dmlcloud_amd.ops.fused_attn import fused_attention_usable, sdpa

    q, k, v, do = _inputs(h, hkv, n)
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    ds = _doc_start() if doc else None
    assert fused_attention_usable(q, k, v, doc_start=ds, causal=causal) is True
    out = sdpa(q, k, v, causal=causal, doc_start=ds)
    out.backward(do)
    assert k.grad.shape == k.shape and v.grad.shape == v.shape
    return out.detach(), q.grad, k.grad, v.grad


def _assert_same_bits(tag, gqa, mha):
    """o, lse and dq: per (b, h) the same operations on the same data."""
    for name, a, b in zip(('o', 'lse', 'dq'), gqa[:3], mha[:3]):
        assert not torch.isnan(a).any(), f'{tag} {name}: rows left unwritten'
        assert torch.equal(bits(a), bits(b)), f'{tag} {name}: differs from the MHA kernels on expanded K/V'


def _assert_group_sum(tag, gqa, mha, g):
    """|dk_gqa - S| <= 2^-8 (|dk_gqa| + sum_g |dk_mha_g|) + 2^-16 max|S|, S the
    fp32 sum of the group's MHA results; the same for dv. First term: the
    half-ulp of the one bf16 store here and of the G stores there. Second:
    the other fp32 accumulation order, <= ~20 chained MFMA steps at these
    shapes, so <= 2^-19 of the largest partial sum, with an 8x margin."""
    for name, a, m in zip(('dk', 'dv'), gqa[3:], mha[3:]):
        assert not torch.isnan(a).any(), f'{tag} {name}: rows left unwritten'
        b, hkv, n, d = a.shape
        parts = m.float().view(b, hkv, g, n, d)
        s = parts.sum(2)
        bound = 2.0**-8 * (a.float().abs() + parts.abs().sum(2)) + 2.0**-16 * s.abs().max()
        err = (a.float() - s).abs()
        print(f'{tag} {name}: max err {err.max().item():.3e}, max err/bound {(err / bound).max().item():.3f}')
        assert (err <= bound).all(), f'{tag} {name}: group sum outside the bound'


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', LENGTHS)
@pytest.mark.parametrize('h,hkv', HEADS)
def test_same_bits_as_mha_on_expanded_kv(h, hkv, n, causal):
    _assert_same_bits(f'H={h} Hkv={hkv} N={n}', _gqa(h, hkv, n, causal), _mha_on_expanded(h, hkv, n, causal))


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', LENGTHS)
@pytest.mark.parametrize('h,hkv', HEADS)
def test_dkdv_is_the_group_sum(h, hkv, n, causal):
    _assert_group_sum(
        f'H={h} Hkv={hkv} N={n}', _gqa(h, hkv, n, causal), _mha_on_expanded(h, hkv, n, causal), h // hkv
    )


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', LENGTHS)
@pytest.mark.parametrize('h,hkv', HEADS)
def test_sdpa_fwd_bwd_matches_fp32_autograd(h, hkv, n, causal):
    _assert_close(f'H={h} Hkv={hkv} N={n}', _sdpa_native(h, hkv, n, causal), _reference(h, hkv, n, causal))


def test_document_mask():
    h, hkv = 4, 2
    _assert_close('docs', _sdpa_native(h, hkv, DOC_N, True, doc=True), _reference(h, hkv, DOC_N, True, doc=True))
    gqa, mha = _gqa(h, hkv, DOC_N, True, doc=True), _mha_on_expanded(h, hkv, DOC_N, True, doc=True)
    _assert_same_bits('docs', gqa, mha)
    _assert_group_sum('docs', gqa, mha, h // hkv)
    # the mask did something: the dense causal result is another one
    assert not torch.equal(gqa[0], _gqa(h, hkv, DOC_N, True)[0])


@pytest.mark.parametrize('h,hkv', [(4, 1), (6, 2)])
def test_strided_kv_views_bit_identical(h, hkv):
    """q, k, v as the model produces them: transpose views of one
    [B, N, (H + 2 Hkv) * 64] buffer."""
    n = 100
    q, k, v, do = _inputs(h, hkv, n)
    qkv = torch.cat([t.transpose(1, 2).reshape(B, n, -1) for t in (q, k, v)], dim=2)
    assert qkv.shape == (B, n, (h + 2 * hkv) * D)
    qs, ks, vs = qkv.split([h * D, hkv * D, hkv * D], dim=2)
    qs = qs.view(B, n, h, D).transpose(1, 2)
    ks = ks.view(B, n, hkv, D).transpose(1, 2)
    vs = vs.view(B, n, hkv, D).transpose(1, 2)
    assert not ks.is_contiguous() and ks.stride(1) == D and torch.equal(ks, k)
    for causal in (True, False):
        for name, a, b in zip(('o', 'lse', 'dq', 'dk', 'dv'), _direct(qs, ks, vs, do, causal), _gqa(h, hkv, n, causal)):
            assert torch.equal(bits(a), bits(b)), f'{name} causal={causal}'


def _run_with_canaries(q, k, v, do, causal):
    """attn_testlib.run_with_canaries for two shapes: dk/dv sized for Hkv,
    o/dq/lse/delta for H, each the front of a larger buffer with 128 rows'
    worth of sentinel behind it."""
    from dmlcloud_amd import _C

    b, h, n, d = q.shape
    hkv = k.shape[1]
    bufs = {}
    for name, heads in (('o', h), ('dq', h), ('dk', hkv), ('dv', hkv)):
        bufs[name] = carve(b * heads * n * d, 128 * d, torch.bfloat16, -7.5, DEV)
    for name in ('lse', 'delta'):
        bufs[name] = carve(b * h * n, 128, torch.float32, -12345.0, DEV)
    before = {name: bits(flat).clone() for name, (flat, _) in bufs.items()}

    o, dq = (bufs[x][1].view(b, h, n, d) for x in ('o', 'dq'))
    dk, dv = (bufs[x][1].view(b, hkv, n, d) for x in ('dk', 'dv'))
    lse = bufs['lse'][1].view(b, h, n)
    _C.attn_fwd(q, k, v, o, lse, SCALE, causal, None)
    _C.attn_bwd(q, k, v, do, o, lse, dq, dk, dv, bufs['delta'][1], SCALE, causal, None)
    torch.cuda.synchronize()

    for name, (flat, front) in bufs.items():
        numel = front.numel()
        assert torch.equal(bits(flat)[numel:], before[name][numel:]), f'{name}: sentinel overwritten'
        assert not torch.isnan(front).any(), f'{name}: rows left unwritten'
    return o, lse, dq, dk, dv


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('n', [1, 100])
@pytest.mark.parametrize('h,hkv', [(4, 1), (6, 2)])
def test_canaries_untouched(h, hkv, n, causal):
    got = _run_with_canaries(*_inputs(h, hkv, n), causal)
    for name, a, b in zip(('o', 'lse', 'dq', 'dk', 'dv'), got, _gqa(h, hkv, n, causal)):
        assert torch.equal(bits(a), bits(b)), name


@pytest.mark.parametrize('h,hkv,n', [(4, 1, 129), (6, 2, 100), (4, 2, 64)])
def test_backward_is_bitwise_repeatable(h, hkv, n):
    q, k, v, do = _inputs(h, hkv, n)
    first = _gqa(h, hkv, n, True)
    again = _direct(q, k, v, do, True)
    assert torch.equal(bits(first[3]), bits(again[3])) and torch.equal(bits(first[4]), bits(again[4]))
    ds_first, ds_again = _gqa(4, 2, DOC_N, True, doc=True), _direct(*_inputs(4, 2, DOC_N), True, _doc_start())
    assert torch.equal(bits(ds_first[3]), bits(ds_again[3])) and torch.equal(bits(ds_first[4]), bits(ds_again[4]))


def test_launchers_reject_bad_head_geometry():
    """Refused before any launch; the same buffers then serve a valid call."""
    from dmlcloud_amd import _C

    h, hkv, n = 4, 2, 100
    q, k, v, do = _inputs(h, hkv, n)
    k3 = torch.zeros(B, 3, n, D, dtype=torch.bfloat16, device=DEV)  # 3 does not divide 4
    k1 = k[:, :1].contiguous()  # another head count than v's
    k8 = torch.zeros(B, 8, n, D, dtype=torch.bfloat16, device=DEV)  # more K/V heads than query heads
    o, dq, dq_like_dk, dq_like_dv = (torch.empty_like(q) for _ in range(4))
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    lse = torch.empty(B, h, n, dtype=torch.float32, device=DEV)
    delta = torch.empty(B * h * n, dtype=torch.float32, device=DEV)

    for bad_k, bad_v in ((k3, k3), (k1, v), (k, k1), (k8, k8), (k[:, :, : n - 1], v[:, :, : n - 1])):
        with pytest.raises(RuntimeError):
            _C.attn_fwd(q, bad_k, bad_v, o, lse, SCALE, True, None)
    _C.attn_fwd(q, k, v, o, lse, SCALE, True, None)
    for bad in (
        dict(k=k3, v=k3, dk=torch.empty_like(k3), dv=torch.empty_like(k3)),
        dict(k=k1),
        dict(v=k1),
        dict(dk=dq_like_dk),  # shaped like q although Hkv < H
        dict(dv=dq_like_dv),
        dict(dk=dk[:, :1]),
    ):
        a = dict(k=k, v=v, dk=dk, dv=dv)
        a.update(bad)
        with pytest.raises(RuntimeError):
            _C.attn_bwd(q, a['k'], a['v'], do, o, lse, dq, a['dk'], a['dv'], delta, SCALE, True, None)
    _C.attn_bwd(q, k, v, do, o, lse, dq, dk, dv, delta, SCALE, True, None)
    _assert_close('after rejections', (o, dq, dk, dv), _reference(h, hkv, n, True))


def test_gpt2_gqa_end_to_end(monkeypatch):
    """A D = 64 GPT-2 with n_head = 4, n_kv_head = 2 on a (2, 50) batch
    hands the native forward a 2-head K once per layer, and its bf16 loss
    matches the same weights in fp32."""
    from dmlcloud_amd.models.gpt2 import GPT2, GPT2Config
    from dmlcloud_amd.ops import fused_attn

    cfg = GPT2Config(vocab_size=512, n_positions=64, n_embd=256, n_layer=2, n_head=4, n_kv_head=2)
    torch.manual_seed(0)
    model = GPT2(cfg).to(DEV)
    idx = torch.randint(0, cfg.vocab_size, (2, 50), device=DEV)
    _, loss32 = model(idx, targets=idx)

    model16 = GPT2(cfg).to(DEV)
    model16.load_state_dict(model.state_dict())
    model16 = model16.to(torch.bfloat16)

    native_calls = []
    real_fwd = fused_attn._C.attn_fwd

    def counting_fwd(q, k, *rest):
        native_calls.append((q.shape[1], k.shape[1], q.shape[2]))
        return real_fwd(q, k, *rest)

    monkeypatch.setattr(fused_attn._C, 'attn_fwd', counting_fwd)
    _, loss16 = model16(idx, targets=idx)
    loss16.backward()
    assert native_calls == [(4, 2, 50)] * cfg.n_layer
    assert loss16.item() == pytest.approx(loss32.item(), rel=5e-2)
    assert all(torch.isfinite(p.grad).all() for p in model16.parameters())
