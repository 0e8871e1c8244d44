"""Helpers shared by the GPU attention tests (test_gpu.py,
test_gpu_attention_ragged.py, test_gpu_attention_docmask.py)."""

import math

import torch


def carve(numel, tail, dtype, sentinel, device):
    """A tensor of `numel` NaNs at the front of a larger flat buffer whose
    last `tail` elements hold `sentinel`."""
    flat = torch.full((numel + tail,), sentinel, dtype=dtype, device=device)
    flat[:numel] = float('nan')
    return flat, flat[:numel]


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def run_with_canaries(inputs, causal, doc_start=None):
    """Forward and backward through the direct bindings on `inputs` =
    (q, k, v, dO), every output being the front of a larger buffer with
    128 rows' worth of sentinel behind it. Checks that the sentinels come
    back bit-identical and that every element in front of them was written
    (no NaN fill left); returns (o, lse, dq, dk, dv)."""
    from dmlcloud_amd import _C

    q, k, v, do = inputs
    b, h, n, d = q.shape
    bufs = {}
    for name in ('o', 'dq', 'dk', 'dv'):
        bufs[name] = carve(b * h * n * d, 128 * d, torch.bfloat16, -7.5, q.device)
    for name in ('lse', 'delta'):
        bufs[name] = carve(b * h * n, 128, torch.float32, -12345.0, q.device)
    before = {name: bits(flat).clone() for name, (flat, _) in bufs.items()}

    o, dq, dk, dv = (bufs[x][1].view(b, h, n, d) for x in ('o', 'dq', 'dk', 'dv'))
    lse = bufs['lse'][1].view(b, h, n)
    scale = 1.0 / math.sqrt(d)
    _C.attn_fwd(q, k, v, o, lse, scale, causal, doc_start)
    _C.attn_bwd(q, k, v, do, o, lse, dq, dk, dv, bufs['delta'][1], scale, causal, doc_start)
    torch.cuda.synchronize()

    for name, (flat, front) in bufs.items():
        numel = front.numel()
        assert torch.equal(bits(flat)[numel:], before[name][numel:]), f'{name}: sentinel overwritten'
        assert not torch.isnan(front).any(), f'{name}: rows left unwritten'
    return o, lse, dq, dk, dv


def assert_fwd_bwd_close(tag, got, want):
    """(out, dq, dk, dv) against a reference: 3e-2 for out, 5e-2 for the
    gradients, relative and absolute."""
    for name, g, w, tol in zip(('out', 'dq', 'dk', 'dv'), got, want, (3e-2, 5e-2, 5e-2, 5e-2)):
        print(f'{tag} {name}: max abs err {(g.float() - w.float()).abs().max().item():.3e}')
        torch.testing.assert_close(g.float(), w.float(), rtol=tol, atol=tol)
