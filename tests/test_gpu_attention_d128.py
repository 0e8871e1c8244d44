"""Head dim 128 in the MFMA flash-attention kernels (ops/csrc/attention_d128.h)
against F.scaled_dot_product_attention in fp64 on the CPU, on the same bf16
values. Run on an MI355X box: python -m pytest tests -m gpu

Two bounds per tensor: the project's assert_fwd_bwd_close (3e-2 out, 5e-2
gradients) and a scaled one, max|got - ref| <= C_SCALED * max|ref|, for the
cases whose gradients are small. C_SCALED is twice the largest normalised
error of the D = 64 kernels over the same (B, H, Hkv, N, causal) cases and the
document case against the same oracle (D = 128 doubles the length of every dot
product that passes through a bf16-rounded P or dS). Measured at D = 64 on an
MI355X, largest normalised error per tensor: out 3.867e-3, dq 3.974e-3,
dk 4.064e-3, dv 3.967e-3, so C_SCALED = 2 * 4.064e-3. (The D = 128 kernels
then measured out 3.657e-3, dq 4.547e-3, dk 4.385e-3, dv 3.828e-3.) At N = 1
dq and dk are exactly zero and have no normalised error: there the kernels'
values must stay at fp32 round-off (p = 1 and dP - delta = 0 to a few ulp,
times |q|, |k| of a few units), 1e-5.
"""

import functools

import pytest
import torch
from torch.nn import functional as F

from attn_testlib import assert_fwd_bwd_close, bits, carve

pytestmark = pytest.mark.gpu

DEV = 'cuda'
B, D = 2, 128
C_SCALED = 2 * 4.064e-3

NS = [1, 16, 63, 64, 65, 129, 200]
CASES = [(2, 2, n, True) for n in NS] + [
    (h, hkv, n, causal)
    for h, hkv, causal in [(2, 2, False), (4, 2, True), (4, 2, False), (4, 1, True), (4, 1, False)]
    for n in (65, 200)
]
DOC_BOUNDS = [0, 9, 70, 130, 200]  # inside a tile, across a tile edge, across the block edge


def _doc_start():
    ds = torch.zeros(B, 200, dtype=torch.int32)  # row 1: a single document
    for lo, hi in zip(DOC_BOUNDS[:-1], DOC_BOUNDS[1:]):
        ds[0, lo:hi] = lo
    return ds


@functools.lru_cache(maxsize=None)
def _case(h, hkv, n, causal, doc=False):
    """bf16 (q, k, v, dO) on the CPU and the fp64 (out, dq, dk, dv) of them."""
    g = torch.Generator().manual_seed(1000 * h + 10 * n + hkv)
    shapes = [(B, h, n, D), (B, hkv, n, D), (B, hkv, n, D), (B, h, n, D)]
    inputs = tuple((torch.randn(s, generator=g) * 0.5).to(torch.bfloat16) for s in shapes)
    q, k, v = (t.double().requires_grad_(True) for t in inputs[:3])
    from dmlcloud_amd.ops.fused_attn import document_mask

    mask = dict(attn_mask=document_mask(_doc_start(), True)) if doc else dict(is_causal=causal)
    out = F.scaled_dot_product_attention(q, k, v, enable_gqa=True, **mask)
    out.backward(inputs[3].double())
    return inputs, (out.detach(), q.grad, k.grad, v.grad)


def run_with_canaries(inputs, causal, doc_start=None):
    """attn_testlib.run_with_canaries with dk/dv in k's shape (Hkv heads):
    the direct bindings, every output the front of a larger buffer whose
    tail must come back untouched and whose front must be fully written."""
    from dmlcloud_amd import _C

    q, k, v, do = inputs
    shapes = dict(o=q.shape, dq=q.shape, dk=k.shape, dv=k.shape, lse=q.shape[:3], delta=q.shape[:3])
    bufs = {
        name: carve(shape.numel(), 128 * D, torch.bfloat16, -7.5, DEV)
        if len(shape) == 4
        else carve(shape.numel(), 128, torch.float32, -12345.0, DEV)
        for name, shape in shapes.items()
    }
    before = {name: bits(flat).clone() for name, (flat, _) in bufs.items()}
    o, dq, dk, dv, lse, delta = (bufs[name][1].view(shape) for name, shape in shapes.items())
    _C.attn_fwd(q, k, v, o, lse, D**-0.5, causal, doc_start)
    _C.attn_bwd(q, k, v, do, o, lse, dq, dk, dv, delta.view(-1), D**-0.5, causal, doc_start)
    torch.cuda.synchronize()
    for name, (flat, front) in bufs.items():
        assert torch.equal(bits(flat)[front.numel() :], before[name][front.numel() :]), f'{name}: sentinel overwritten'
        assert not torch.isnan(front).any(), f'{name}: rows left unwritten'
    return o, lse, dq, dk, dv


def _check(tag, h, hkv, n, causal, doc=False):
    inputs, want = _case(h, hkv, n, causal, doc)
    ds = _doc_start().to(DEV) if doc else None
    o, _, dq, dk, dv = run_with_canaries(tuple(t.to(DEV) for t in inputs), causal, ds)
    got = tuple(t.cpu() for t in (o, dq, dk, dv))
    assert_fwd_bwd_close(tag, got, want)
    for name, g, w in zip(('out', 'dq', 'dk', 'dv'), got, want):
        err, ref = (g.double() - w).abs().max().item(), w.abs().max().item()
        print(f'{tag} {name}: max abs err / max |ref| = {err:.3e} / {ref:.3e}')
        assert err <= (C_SCALED * ref if ref > 1e-9 else 1e-5), name


@pytest.mark.parametrize('h,hkv,n,causal', CASES)
def test_matches_fp64_sdpa(h, hkv, n, causal):
    _check(f'H{h}/{hkv} N{n} causal={causal}', h, hkv, n, causal)


@pytest.mark.parametrize('h,hkv', [(2, 2), (4, 2)])
def test_documents_match_fp64_sdpa(h, hkv):
    _check(f'H{h}/{hkv} documents', h, hkv, 200, True, doc=True)


def test_dk_dv_are_bitwise_repeatable():
    inputs = tuple(t.to(DEV) for t in _case(4, 1, 200, True)[0])
    first, second = (run_with_canaries(inputs, True)[3:] for _ in range(2))
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


@pytest.mark.parametrize('packed', [False, True])
def test_sdpa_on_views_matches_contiguous(packed):
    """sdpa under autograd on [B, N, H, 128] memory viewed transposed, and on
    the q/k/v split of one projection output: native, and equal to the call
    on contiguous copies."""
    from dmlcloud_amd.ops.fused_attn import fused_attention_usable, sdpa

    torch.manual_seed(5)
    h, hkv, n = 4, 2, 100
    if packed:
        qkv = (torch.randn(B, n, (h + 2 * hkv) * D, device=DEV) * 0.5).to(torch.bfloat16)
        bases = [t.view(B, n, -1, D) for t in qkv.split([h * D, hkv * D, hkv * D], dim=2)]
    else:
        bases = [(torch.randn(B, n, x, D, device=DEV) * 0.5).to(torch.bfloat16) for x in (h, hkv, hkv)]
    views = [t.transpose(1, 2).requires_grad_(True) for t in bases]
    copies = [t.detach().contiguous().requires_grad_(True) for t in views]
    assert not views[0].is_contiguous()
    assert fused_attention_usable(*views) is True
    do = (torch.randn(B, h, n, D, device=DEV) * 0.5).to(torch.bfloat16)
    out, out2 = sdpa(*views, causal=True), sdpa(*copies, causal=True)
    out.backward(do)
    out2.backward(do)
    torch.testing.assert_close(out, out2)
    for a, b in zip(views, copies):
        torch.testing.assert_close(a.grad, b.grad)


def test_gpt2_head_dim_128_runs_native(monkeypatch):
    from dmlcloud_amd.models import gpt2 as gpt2_mod
    from dmlcloud_amd.models.gpt2 import GPT2, GPT2Config
    from dmlcloud_amd.ops import fused_attn

    cfg = GPT2Config(vocab_size=512, n_positions=128, n_embd=256, n_layer=2, n_head=2, n_kv_head=1)
    torch.manual_seed(0)
    ref_model = GPT2(cfg)
    idx = torch.randint(0, cfg.vocab_size, (2, 100))
    _, ref_loss = ref_model(idx, targets=idx)

    usable = []

    def spying_sdpa(q, k, v, causal=True, **kw):
        usable.append(q.shape[-1] == D and fused_attn.fused_attention_usable(q, k, v, causal=causal, **kw))
        return fused_attn.sdpa(q, k, v, causal=causal, **kw)

    monkeypatch.setattr(gpt2_mod, 'sdpa', spying_sdpa)
    model = GPT2(cfg)
    model.load_state_dict(ref_model.state_dict())
    model = model.to(DEV).to(torch.bfloat16)
    _, loss = model(idx.to(DEV), targets=idx.to(DEV))
    loss.backward()
    assert usable == [True] * cfg.n_layer
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    assert loss.item() == pytest.approx(ref_loss.item(), rel=5e-2)
