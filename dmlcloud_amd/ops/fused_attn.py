"""Autograd wrapper for the MFMA flash-attention kernels.

`sdpa(q, k, v, causal=True)` matches
F.scaled_dot_product_attention(..., is_causal=causal) for bf16
[B, H, N, 64] self-attention device tensors of ANY sequence length
N >= 1: a multiple of 64 runs the aligned kernels, every other length
their ragged instantiation (clamped loads, masked tail, predicated
stores — ops/csrc/attention.hip). Anything else (other head dims,
cross-attention geometry, non-bf16) falls back to torch SDPA
(AOTriton); `fused_attention_usable(q, k, v)` tells which path a call
takes. The fused path is ON by default whenever usable — set
DMLCLOUD_DISABLE_FUSED_ATTN=1 to force the AOTriton path (the A/B
ladder in profiles/ uses this switch). Numerics are verified in
tests/test_gpu.py and tests/test_gpu_attention_ragged.py (shared
helpers: tests/attn_testlib.py).

Grouped-query attention: k and v may have fewer heads than q,
[B, Hkv, N, 64] with Hkv dividing H (MQA is Hkv = 1). Query head h reads
K/V head h // (H // Hkv): the layout of `enable_gqa=True` and of
`repeat_interleave(H // Hkv, dim=1)`. The native kernels read the shared
K/V heads in place and sum a group's dK/dV in their fp32 accumulators, so
k.grad and v.grad come back in k's shape with one rounding; the fallback
passes `enable_gqa=True`. Verified in tests/test_gpu_attention_gqa.py.

Packed sequences: `sdpa(q, k, v, causal=True, doc_start=ds)` keeps
attention inside documents when several are packed into one batch row.
`ds` is an int32 [B, N] tensor, shared by all heads: ds[b, i] is the
index of the first token of the document that token i belongs to
(ds[b, 0] == 0, non-decreasing, ds[b, i] is ds[b, i-1] or i). Query i
attends key j iff ds[b, i] == ds[b, j] (and j <= i when causal); for
causal attention that is ds[b, i] <= j <= i, one integer per query row,
which is what the kernels' kDoc instantiations read from device memory
(no host sync, hipGraph-capturable; tiles that lie wholly in other
documents are skipped, not masked). `document_starts(doc_ids)` and
`document_starts_from_eos(idx, eos_id)` build it. With causal=False, or
whenever the native path is not usable, the same mask is handed to
torch SDPA as a boolean attn_mask. Verified in
tests/test_gpu_attention_docmask.py.
"""

import math
import os

import torch
from torch.nn import functional as F

from . import _C, is_available


class _SdpaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, scale, doc_start=None):
        B, H, N, D = q.shape
        # empty_like would inherit a transpose-view's strides; o is ours
        o = torch.empty(B, H, N, D, dtype=q.dtype, device=q.device)
        lse = torch.empty(B, H, N, dtype=torch.float32, device=q.device)
        _C.attn_fwd(q, k, v, o, lse, scale, causal, doc_start)
        ctx.save_for_backward(q, k, v, o, lse, doc_start)
        ctx.causal = causal
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse, doc_start = ctx.saved_tensors
        B, H, N, D = q.shape
        if dout.stride(-1) != 1:
            dout = dout.contiguous()
        dq = torch.empty(B, H, N, D, dtype=q.dtype, device=q.device)
        # k's shape: [B, Hkv, N, D] under grouped-query attention
        dk = torch.empty(k.shape, dtype=q.dtype, device=q.device)
        dv = torch.empty(k.shape, dtype=q.dtype, device=q.device)
        delta = torch.empty(B * H * N, dtype=torch.float32, device=q.device)
        _C.attn_bwd(q, k, v, dout, o, lse, dq, dk, dv, delta, ctx.scale, ctx.causal, doc_start)
        return dq, dk, dv, None, None, None


_INT_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


def _usable(q, k, v, doc_start=None, causal=True):
    if not fused_attention_enabled():
        return False
    # The kernels assume self-attention geometry: k/v must match q in every
    # dim but the heads (cross-attention with a different kv length falls
    # back), where k's and v's common count must divide q's (GQA/MQA).
    ok = (
        q.is_cuda
        and is_available()
        and q.dtype == torch.bfloat16
        and q.dim() == 4
        and q.shape[-1] == 64
        and q.shape[-2] >= 1
        and k.dim() == 4
        and k.shape[0] == q.shape[0]
        and k.shape[2:] == q.shape[2:]
        and k.shape[1] >= 1
        and q.shape[1] % k.shape[1] == 0
        and v.shape == k.shape
        and k.dtype == q.dtype
        and v.dtype == q.dtype
        and k.device == q.device
        and v.device == q.device
    )
    if ok and doc_start is not None:
        # the native document mask is causal-only; [B, N] integers on q's device
        ok = (
            bool(causal)
            and doc_start.dtype in _INT_DTYPES
            and doc_start.dim() == 2
            and doc_start.shape[0] == q.shape[0]
            and doc_start.shape[1] == q.shape[2]
            and doc_start.device == q.device
        )
    return ok


def fused_attention_usable(q, k, v, doc_start=None, causal=True) -> bool:
    """True when `sdpa(q, k, v, causal, doc_start)` will run the native
    MFMA kernels, False when it will fall back to torch SDPA: exactly the
    decision `sdpa` makes (bf16 device tensors, q [B, H, N, 64] with any
    N >= 1, k and v shaped like q or, for grouped-query attention, alike
    with a head count that divides H, extension built, no
    DMLCLOUD_DISABLE_FUSED_ATTN; with a `doc_start` also causal=True and
    an integer [B, N] tensor on q's device). `causal` only matters when
    `doc_start` is given."""
    return bool(_usable(q, k, v, doc_start, causal))


def _lastdim_ok(t):
    return t.stride(-1) == 1


def document_starts(doc_ids: torch.Tensor) -> torch.Tensor:
    """int32 [B, N] `doc_start` for `sdpa` from any integer [B, N] tensor
    whose runs of equal values are the documents (document ids, or a
    `doc_start` itself). Pure torch, no host sync, CPU or device: flag the
    positions where the value changes, keep their index, and carry it
    forward with a running maximum."""
    if doc_ids.dim() != 2:
        raise ValueError(f'doc_ids must be [B, N], got {tuple(doc_ids.shape)}')
    change = torch.ones_like(doc_ids, dtype=torch.bool)
    change[:, 1:] = doc_ids[:, 1:] != doc_ids[:, :-1]
    return _starts_from_flags(change)


def document_starts_from_eos(idx: torch.Tensor, eos_id: int) -> torch.Tensor:
    """int32 [B, N] `doc_start` for token rows in which a token equal to
    `eos_id` is the LAST token of its document: the token after it starts
    a new one. No host sync."""
    if idx.dim() != 2:
        raise ValueError(f'idx must be [B, N], got {tuple(idx.shape)}')
    change = torch.ones_like(idx, dtype=torch.bool)
    change[:, 1:] = idx[:, :-1] == eos_id
    return _starts_from_flags(change)


def _starts_from_flags(change: torch.Tensor) -> torch.Tensor:
    n = change.shape[1]
    pos = torch.arange(n, device=change.device, dtype=torch.int32).expand_as(change)
    start = torch.where(change, pos, torch.zeros_like(pos))
    return torch.cummax(start, dim=1).values.to(torch.int32)


def check_document_starts(doc_start: torch.Tensor) -> None:
    """Raise ValueError unless `doc_start` is well-formed: integer [B, N],
    doc_start[b, 0] == 0, and every later doc_start[b, i] equal to either
    doc_start[b, i-1] (same document) or i (a new one) — which implies
    non-decreasing and doc_start[b, i] <= i.

    A debug helper: it reads the verdict back to the host (a device
    sync), so it does not belong in the step loop or under graph capture.
    The kernels do not need it to be safe — they clamp every value they
    read — only to be right."""
    if doc_start.dim() != 2 or doc_start.dtype not in _INT_DTYPES:
        raise ValueError('doc_start must be an integer [B, N] tensor')
    ds = doc_start.long()
    n = ds.shape[1]
    pos = torch.arange(n, device=ds.device).expand_as(ds)
    if bool((ds[:, 0] != 0).any()):
        raise ValueError('doc_start[:, 0] must be 0')
    if bool(((ds < 0) | (ds > pos)).any()):
        raise ValueError('doc_start[b, i] must lie in [0, i]')
    if bool((ds[:, 1:] < ds[:, :-1]).any()):
        raise ValueError('doc_start must be non-decreasing along the sequence')
    if bool(((ds[:, 1:] != ds[:, :-1]) & (ds[:, 1:] != pos[:, 1:])).any()):
        raise ValueError('doc_start[b, i] must equal doc_start[b, i-1] or i')


def document_mask(doc_start: torch.Tensor, causal: bool = True) -> torch.Tensor:
    """The boolean [B, 1, N, N] attn_mask (True = attend) of the
    definition: query i sees key j iff they share a document start, and
    j <= i when causal. N^2 bytes — what the fallback path hands to torch
    SDPA; the native kernels never build it."""
    mask = doc_start.unsqueeze(2) == doc_start.unsqueeze(1)  # [B, Nq, Nk]
    if causal:
        n = doc_start.shape[1]
        mask = mask & torch.ones(n, n, dtype=torch.bool, device=doc_start.device).tril()
    return mask.unsqueeze(1)


def sdpa(q, k, v, causal: bool = True, doc_start=None):
    """Scaled dot-product attention; fused MFMA kernels when usable.

    The kernels take per-tensor (batch, head, row) strides, so transpose
    views (e.g. [B,T,H,D] memory viewed as [B,H,T,D]) pass through
    without materialization — only a non-unit last-dim stride forces a
    copy.

    `doc_start` (integer [B, N], see the module docstring) restricts
    attention to the query's own document. It takes no gradient.

    k and v may have fewer heads than q (grouped-query attention, see the
    module docstring), on the native path and on the fallback alike."""
    if _usable(q, k, v, doc_start, causal):
        scale = 1.0 / math.sqrt(q.shape[-1])
        q = q if _lastdim_ok(q) else q.contiguous()
        k = k if _lastdim_ok(k) else k.contiguous()
        v = v if _lastdim_ok(v) else v.contiguous()
        if doc_start is None:
            return _SdpaFn.apply(q, k, v, causal, scale, None)
        # no-ops for the int32 contiguous tensor document_starts() returns
        doc_start = doc_start.detach().to(torch.int32).contiguous()
        return _SdpaFn.apply(q, k, v, causal, scale, doc_start)
    # enable_gqa only where the head counts differ: the plain call is
    # exactly what it was
    gqa = {'enable_gqa': True} if q.dim() == 4 and k.dim() == 4 and k.shape[1] != q.shape[1] else {}
    if doc_start is None:
        return F.scaled_dot_product_attention(q, k, v, is_causal=causal, **gqa)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=document_mask(doc_start, causal), **gqa)


def fused_attention_enabled() -> bool:
    """True unless DMLCLOUD_DISABLE_FUSED_ATTN opts out (the fused path
    is on by default for usable shapes)."""
    return os.environ.get('DMLCLOUD_DISABLE_FUSED_ATTN', '0') in ('0', '', 'false')
