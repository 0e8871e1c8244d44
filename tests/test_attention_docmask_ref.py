"""Packed sequences (document mask) on the CPU: the blueprint's literal
emulation of the kernels' kDoc instantiations (block / sub-tile skips, the
dkdv break, the clamp, the -1e30 wipe) against fp32 masked softmax +
autograd, the doc_start helpers, and sdpa's fallback path."""

import math
import sys

import pytest
import torch

from dmlcloud_amd.ops._attention_ref import flash_attn_bwd_padded, flash_attn_fwd_padded
from dmlcloud_amd.ops.fused_attn import (
    check_document_starts,
    document_starts,
    document_starts_from_eos,
    fused_attention_usable,
    sdpa,
)

D = 64

# name -> (N, document boundaries)
LAYOUTS = {
    'ONE': (200, [0, 200]),
    # boundaries on the 64-key tile edge and the 128-row block edge
    'EDGES': (256, [0, 64, 128, 256]),
    # boundaries inside a 16-row sub-tile; sub-tile 192..207 holds rows
    # whose start is 70 and rows whose start is 200 (the wipe case)
    'MID': (256, [0, 7, 70, 200, 256]),
    'SINGLETONS': (130, list(range(131))),
    # N % 64 != 0: kRagged and kDoc together
    'RAGGED': (200, [0, 33, 129, 200]),
}


def _doc_start(name):
    n, bounds = LAYOUTS[name]
    ds = torch.empty(n, dtype=torch.int32)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ds[lo:hi] = lo
    return ds


def _definition_mask(ds, causal=True):
    """Query i may attend key j iff doc_start[i] == doc_start[j], and
    j <= i when causal."""
    n = ds.shape[0]
    mask = ds.unsqueeze(1) == ds.unsqueeze(0)
    if causal:
        mask = mask & torch.ones(n, n, dtype=torch.bool).tril()
    return mask


def _plain_attention(q, k, v, mask):
    s = (q @ k.T) / math.sqrt(q.shape[1])
    s = s.masked_fill(~mask, -float('inf'))
    return torch.softmax(s, dim=-1) @ v, torch.logsumexp(s, dim=-1)


@pytest.mark.parametrize('name', list(LAYOUTS))
def test_blueprint_matches_masked_softmax_and_autograd(name):
    n, _ = LAYOUTS[name]
    ds = _doc_start(name)
    torch.manual_seed(n + len(name))
    q = torch.randn(n, D, requires_grad=True)
    k = torch.randn(n, D, requires_grad=True)
    v = torch.randn(n, D, requires_grad=True)
    do = torch.randn(n, D)
    ref, ref_lse = _plain_attention(q, k, v, _definition_mask(ds))
    ref.backward(do)

    with torch.no_grad():
        qd, kd, vd = q.detach(), k.detach(), v.detach()
        o, lse = flash_attn_fwd_padded(qd, kd, vd, causal=True, doc_start=ds)
        dq, dk, dv = flash_attn_bwd_padded(do, qd, kd, vd, o, lse, causal=True, doc_start=ds)

    # every row was stored (no NaN poison left) and the garbage a straddling
    # sub-tile gathers on fully masked tiles was wiped
    for got, want in ((o, ref.detach()), (lse, ref_lse.detach()), (dq, q.grad), (dk, k.grad), (dv, v.grad)):
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('n', [100, 128])
def test_blueprint_without_doc_start_is_bit_identical(n):
    torch.manual_seed(n)
    q, k, v, do = (torch.randn(n, D) for _ in range(4))
    o, lse = flash_attn_fwd_padded(q, k, v, causal=True)
    o2, lse2 = flash_attn_fwd_padded(q, k, v, causal=True, doc_start=None)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    grads = flash_attn_bwd_padded(do, q, k, v, o, lse, causal=True)
    grads2 = flash_attn_bwd_padded(do, q, k, v, o, lse, causal=True, doc_start=None)
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)


def test_blueprint_clamps_malformed_doc_start():
    """Values outside [0, q] are clamped: every stored row keeps at least
    its diagonal key, so nothing is NaN or infinite."""
    n = 100
    g = torch.Generator().manual_seed(3)
    ds = torch.randint(0, 10 * n, (n,), generator=g, dtype=torch.int32)
    ds[::7] = -5
    q, k, v, do = (torch.randn(n, D, generator=g) for _ in range(4))
    o, lse = flash_attn_fwd_padded(q, k, v, causal=True, doc_start=ds)
    grads = flash_attn_bwd_padded(do, q, k, v, o, lse, causal=True, doc_start=ds)
    for t in (o, lse, *grads):
        assert torch.isfinite(t).all()


def test_document_starts():
    ids = torch.tensor([[5, 5, 7, 7, 7, 2], [1, 1, 1, 1, 1, 1], [3, 2, 3, 3, 9, 9]])
    want = torch.tensor([[0, 0, 2, 2, 2, 5], [0, 0, 0, 0, 0, 0], [0, 1, 2, 2, 4, 4]], dtype=torch.int32)
    got = document_starts(ids)
    assert got.dtype == torch.int32
    assert torch.equal(got, want)
    # a doc_start is itself a valid doc_ids tensor
    assert torch.equal(document_starts(got), want)
    check_document_starts(got)


def test_document_starts_from_eos():
    idx = torch.tensor([[3, 0, 4, 4, 0, 0, 9], [0, 1, 2, 3, 4, 5, 0]])
    want = torch.tensor([[0, 0, 2, 2, 2, 5, 6], [0, 1, 1, 1, 1, 1, 1]], dtype=torch.int32)
    got = document_starts_from_eos(idx, eos_id=0)
    assert got.dtype == torch.int32
    assert torch.equal(got, want)
    check_document_starts(got)


def test_check_document_starts():
    check_document_starts(torch.tensor([[0, 0, 2, 2, 4]], dtype=torch.int32))
    for name in LAYOUTS:
        check_document_starts(_doc_start(name).unsqueeze(0))
    with pytest.raises(ValueError):  # a start greater than its index
        check_document_starts(torch.tensor([[0, 0, 3, 3, 3]], dtype=torch.int32))
    with pytest.raises(ValueError):  # a decreasing start
        check_document_starts(torch.tensor([[0, 0, 2, 0, 0]], dtype=torch.int32))
    with pytest.raises(ValueError):  # a jump to something other than its own index
        check_document_starts(torch.tensor([[0, 0, 0, 2, 2]], dtype=torch.int32))
    with pytest.raises(ValueError):  # the first token starts the first document
        check_document_starts(torch.tensor([[1, 1, 2]], dtype=torch.int32))
    with pytest.raises(ValueError):
        check_document_starts(torch.zeros(1, 4))  # not an integer tensor


@pytest.mark.parametrize('name', ['MID', 'RAGGED'])
def test_sdpa_cpu_equals_each_document_alone(name):
    n, bounds = LAYOUTS[name]
    ds = _doc_start(name).unsqueeze(0).expand(2, n)
    torch.manual_seed(11)
    q, k, v = (torch.randn(2, 3, n, D) for _ in range(3))
    assert fused_attention_usable(q, k, v, doc_start=ds) is False  # CPU fp32: the mask fallback
    packed = sdpa(q, k, v, causal=True, doc_start=ds)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        alone = sdpa(q[:, :, lo:hi], k[:, :, lo:hi], v[:, :, lo:hi], causal=True)
        torch.testing.assert_close(packed[:, :, lo:hi], alone, rtol=1e-5, atol=1e-5)


def test_sdpa_cpu_non_causal_document_mask():
    n, _ = LAYOUTS['MID']
    ds = _doc_start('MID')
    torch.manual_seed(12)
    q, k, v = (torch.randn(1, 1, n, D) for _ in range(3))
    got = sdpa(q, k, v, causal=False, doc_start=ds.unsqueeze(0))
    want, _ = _plain_attention(q[0, 0], k[0, 0], v[0, 0], _definition_mask(ds, causal=False))
    torch.testing.assert_close(got[0, 0], want, rtol=1e-5, atol=1e-5)


if __name__ == '__main__':
    sys.exit(pytest.main([__file__]))
