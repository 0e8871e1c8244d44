"""Autograd wrapper for the MFMA flash-attention kernels.

`sdpa(q, k, v, causal=True)` matches
F.scaled_dot_product_attention(..., is_causal=causal) for bf16
[B, H, N, D] self-attention device tensors with head dim D = 64 or 128
and ANY sequence length N >= 1: a multiple of 64 runs the aligned
kernels, every other length their ragged instantiation (clamped loads,
masked tail, predicated stores — ops/csrc/attention.hip; the D = 128
kernels, with every option of the D = 64 ones, are
ops/csrc/attention_d128.h, verified in tests/test_gpu_attention_d128.py).
Anything else (other head dims, cross-attention geometry, non-bf16)
falls back to torch SDPA
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

Decoding: `sdpa_kvcache(q, k_cache, v_cache, kv_len)` attends new query
rows (one token, a few draft tokens, a chunk of a prompt) to a partly
filled [B, Hkv, Nmax, D] K/V cache (D = 64 or 128) whose per-row lengths
live on the device. It has kernels of its own (D = 64: split-KV decode plus
a merge pass, and their tiled form for more than 16 query columns per K/V
head, ops/csrc/attention.hip; D = 128: one tiled pair for any number of
columns, ops/csrc/attention_decode_d128.h) and never goes through `sdpa`,
whose behaviour for kv length != q length (torch SDPA, top-left causal)
is unchanged. Verified in tests/test_gpu_attention_kvcache.py,
tests/test_gpu_attention_kvcache_tiled.py and
tests/test_gpu_attention_kvcache_d128.py.

Paged cache: `sdpa_kvcache(..., block_table=t)` reads K and V from page
pools [num_pages, Hkv, page_size, D] through an integer [B, max_pages] block
table (page_size a multiple of 32: the paged instantiations of the tiled
kernels, one scalar table read per 32-key tile; other page sizes: the torch
reference), and `kvcache_append(k_new, v_new, k_cache, v_cache, kv_len,
block_table=None)` writes the new tokens' K/V rows into a dense or paged
cache in one launch, positions resolved on the device
(ops/csrc/attention_kvcache_append.h). Verified in
tests/test_gpu_attention_kvcache_paged.py.

FP8 cache: k_cache and v_cache may be `torch.float8_e4m3fn` (the MI355X's
native OCP e4m3), dense or paged, with optional per-K/V-head fp32 scales
`k_scale`, `v_scale` [Hkv] on the device (None = ones): key row j of head h
is float(k_cache[.., h, j, :]) * k_scale[h], V alike. q and the appended rows
stay bf16. `sdpa_kvcache(..., k_scale=, v_scale=)` runs one split-KV kernel
for every R and both D that dequantises the bytes to bf16 in registers (exact)
and keeps the bf16 MFMAs, folding k_scale into the softmax scale and v_scale
into the epilogue; `kvcache_append(..., k_scale=, v_scale=)` stores
e4m3_rne(clamp(float(x) / scale[h], -448, 448)) in one launch
(ops/csrc/attention_decode_fp8.h). The scales are read on the device, so a
captured call follows them. A scale passed with a cache of another dtype
raises ValueError. Verified in tests/test_attention_kvcache_fp8_ref.py and
tests/test_gpu_attention_kvcache_fp8.py.
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
_FP8 = torch.float8_e4m3fn


def _fp8_caches(k_cache, v_cache, k_scale, v_scale):
    """True for an e4m3 cache pair; a scale with any other cache is an error."""
    fp8 = k_cache.dtype == _FP8 and v_cache.dtype == _FP8
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError('k_scale / v_scale go with float8_e4m3fn caches only')
    return fp8


def _fp8_scale_ok(scale, like, n_kv_head):
    # what the native kernels read: fp32 [Hkv] on the device (the wrapper makes it contiguous)
    return scale is None or (
        scale.dtype == torch.float32 and scale.shape == (n_kv_head,) and scale.device == like.device
    )


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
        and q.shape[-1] in (64, 128)
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
    decision `sdpa` makes (bf16 device tensors, q [B, H, N, D] with D = 64
    or 128 and any N >= 1, k and v shaped like q or, for grouped-query attention, alike
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
    module docstring), on the native path and on the fallback alike.

    The native path serves head dims 64 and 128, each with kernels of its
    own and the same options (any N, strides, doc_start, GQA)."""
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


def _kvcache_usable(q, k_cache, v_cache, kv_len, block_table=None, k_scale=None, v_scale=None):
    fp8 = _fp8_caches(k_cache, v_cache, k_scale, v_scale)
    if not fused_attention_enabled():
        return False
    if fp8 and not (k_cache.dim() == 4 and all(_fp8_scale_ok(s, q, k_cache.shape[1]) for s in (k_scale, v_scale))):
        return False
    ok = (
        q.is_cuda
        and is_available()
        and q.dtype == torch.bfloat16
        and q.dim() == 4
        and q.shape[-1] in (64, 128)
        and k_cache.dim() == 4
        and k_cache.shape[3] == q.shape[-1]
        and k_cache.shape[1] >= 1
        and q.shape[1] % k_cache.shape[1] == 0
        and (q.shape[1] // k_cache.shape[1]) * q.shape[2] >= 1
        and v_cache.shape == k_cache.shape
        and (fp8 or (k_cache.dtype == q.dtype and v_cache.dtype == q.dtype))
        and k_cache.device == q.device
        and v_cache.device == q.device
        and all(t.stride(-1) == 1 for t in (q, k_cache, v_cache))
        and kv_len.dtype in _INT_DTYPES
        and kv_len.shape == (q.shape[0],)
        and kv_len.device == q.device
    )
    if block_table is None:
        return ok and k_cache.shape[0] == q.shape[0] and k_cache.shape[2] >= q.shape[2]
    return (
        ok
        and k_cache.shape[0] >= 1
        and k_cache.shape[2] >= 32
        and k_cache.shape[2] % 32 == 0
        and block_table.dtype in _INT_DTYPES
        and block_table.dim() == 2
        and block_table.shape[0] == q.shape[0]
        and block_table.shape[1] >= 1
        and block_table.device == q.device
        and block_table.shape[1] * k_cache.shape[2] >= q.shape[2]
    )


def fused_kvcache_usable(q, k_cache, v_cache, kv_len, block_table=None, k_scale=None, v_scale=None) -> bool:
    """True when `sdpa_kvcache(q, k_cache, v_cache, kv_len, block_table=...)`
    will run the native split-KV kernels, False when it will run the
    pure-torch reference: bf16 device tensors, q [B, H, Nq, D] with D = 64 or
    128 and any Nq >= 1, last dims contiguous, an integer [B] kv_len on q's
    device, extension built, no DMLCLOUD_DISABLE_FUSED_ATTN, and
    without a table caches [B, Hkv, Nmax, D] with Hkv dividing H and
    Nmax >= Nq; with one, pools [num_pages, Hkv, page_size, D] with Hkv
    dividing H and page_size a positive multiple of 32, and an integer
    [B, max_pages] table on q's device with max_pages * page_size >= Nq.
    The caches are bf16 like q, or both float8_e4m3fn, then with `k_scale` and
    `v_scale` each None or an fp32 [Hkv] tensor on q's device (a scale with a
    cache of another dtype raises ValueError, as the call itself does)."""
    return bool(_kvcache_usable(q, k_cache, v_cache, kv_len, block_table, k_scale, v_scale))


def _vector_loadable(t):
    # the kernels read rows as 16-byte vectors: 8 bf16 or 16 e4m3 elements
    n = 16 // t.element_size()
    return t.data_ptr() % 16 == 0 and all(s % n == 0 for s in t.stride()[:-1])


def sdpa_kvcache(
    q,
    k_cache,
    v_cache,
    kv_len,
    causal: bool = True,
    num_splits: int = 0,
    return_lse: bool = False,
    block_table=None,
    k_scale=None,
    v_scale=None,
):
    """Attention of new query rows over a partly filled K/V cache: one row
    (decoding), a few (speculative verification) or a whole chunk of a
    prompt (chunked prefill, continuation); forward only.

    q is [B, H, Nq, D]; k_cache and v_cache are [B, Hkv, Nmax, D] with Hkv
    dividing H (query head h reads K/V head h // (H // Hkv), as in `sdpa`);
    kv_len is an integer [B] tensor on q's device: the number of valid
    cache rows of each batch row, the Nq new tokens' rows (already
    written by the caller) included. Query row i of batch row b sits at
    position p = kv_len[b] - Nq + i and attends keys 0..p with causal=True
    (bottom-right aligned) and keys 0..kv_len[b] - 1 otherwise. Cache rows
    at or past kv_len[b] are never read. The value used for kv_len[b] is
    clamped to [Nq, Nmax] (causal) or [1, Nmax].

    Paged cache: with an integer `block_table` [B, max_pages] on q's device,
    k_cache and v_cache are page POOLS [num_pages, Hkv, page_size, D] and
    logical key j of batch row b is row j % page_size of page
    block_table[b, j // page_size]. The capacity max_pages * page_size stands
    wherever Nmax stands above. Only the entries below
    ceil(kv_len[b] / page_size) are read, later ones may hold anything; an
    entry that is read is clamped to [0, num_pages - 1].

    On the native path (`fused_kvcache_usable`) the lengths are read on the
    device: no host sync, hipGraph-capturable, and kv_len and the cache
    contents (and the block table) may change between replays. The keys are
    split over `num_splits` blocks per (b, K/V head), 0 = chosen from the
    shapes and the device's CU count, and merged by a second kernel; any
    batch (page) / head / row strides pass without a copy ([B, Nmax, Hkv, D]
    or [num_pages, page_size, Hkv, D] memory viewed transposed included).
    R = (H / Hkv) * Nq query columns share a K/V head. Without a table, D = 64:
    R <= 16 runs the decode kernels (`_C.attn_decode`), R > 16 the tiled ones
    (`_C.attn_decode_tiled`: 16-column MFMA tiles, up to four per block, key
    tiles past a tile's last causal position skipped); D = 128 has one kernel
    pair of the tiled form for every R (ops/csrc/attention_decode_d128.h),
    reached through `_C.attn_decode_tiled` as well. With a table whose
    page_size is a multiple of 32, every R and both D run the paged
    instantiations of the tiled kernels (`_C.attn_decode_tiled(...,
    block_table)`). Everything else (other head dims, other dtypes, other page
    sizes) runs `_attention_ref.kvcache_attention_ref`.

    FP8 cache: k_cache and v_cache may both be float8_e4m3fn, with `k_scale`
    and `v_scale` None (ones) or fp32 [Hkv] tensors on q's device: key row j
    of K/V head h is float(k_cache[.., h, j, :]) * k_scale[h], V alike. The
    native path (`_C.attn_decode_fp8`, one kernel for every R, both D, dense
    and paged) reads the scales on the device, so they may change between
    replays of a captured call. A scale with a cache of another dtype raises
    ValueError.

    Returns o [B, H, Nq, D] in q's dtype, and with return_lse=True also
    lse [B, H, Nq] fp32."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k_cache, v_cache)):
        raise RuntimeError('sdpa_kvcache is forward only: call it under torch.no_grad() or detach its inputs')
    if not _kvcache_usable(q, k_cache, v_cache, kv_len, block_table, k_scale, v_scale):
        from ._attention_ref import kvcache_attention_ref

        return kvcache_attention_ref(q, k_cache, v_cache, kv_len, causal, return_lse, block_table, k_scale, v_scale)
    B, H, Nq, D = q.shape
    Hkv, Nmax = k_cache.shape[1], k_cache.shape[2]
    q, k_cache, v_cache = (t if _vector_loadable(t) else t.contiguous() for t in (q, k_cache, v_cache))
    kv_len = kv_len.detach().to(torch.int32).contiguous()  # no-ops for an int32 tensor
    R = (H // Hkv) * Nq
    if block_table is not None:
        if block_table.dtype != torch.int32 or not block_table.is_contiguous():
            block_table = block_table.detach().to(torch.int32).contiguous()
        Nmax = block_table.shape[1] * k_cache.shape[2]  # the capacity
    if k_cache.dtype == _FP8:
        splits = _C.attn_decode_tiled_splits(B, Hkv, R, Nmax, num_splits, q.get_device())
        o = torch.empty(B, H, Nq, D, dtype=q.dtype, device=q.device)
        lse = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device)
        # the tiled kernels' partial layout; every element the merge reads is written
        ws = torch.empty(_C.attn_decode_tiled_workspace_floats(B, Hkv, R, splits, D), dtype=torch.float32, device=q.device)
        k_scale, v_scale = (None if s is None else s.detach().contiguous() for s in (k_scale, v_scale))
        _C.attn_decode_fp8(
            q, k_cache, v_cache, kv_len, o, lse, ws, 1.0 / math.sqrt(D), causal, splits, k_scale, v_scale, block_table
        )
        return (o, lse) if return_lse else o
    if block_table is not None or R > 16 or D == 128:
        splits = _C.attn_decode_tiled_splits(B, Hkv, R, Nmax, num_splits, q.get_device())
        o = torch.empty(B, H, Nq, D, dtype=q.dtype, device=q.device)
        lse = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device)
        # one partial per (column tile, split); every element the merge reads is written
        ws = torch.empty(_C.attn_decode_tiled_workspace_floats(B, Hkv, R, splits, D), dtype=torch.float32, device=q.device)
        _C.attn_decode_tiled(q, k_cache, v_cache, kv_len, o, lse, ws, 1.0 / math.sqrt(D), causal, splits, block_table)
        return (o, lse) if return_lse else o
    splits = _C.attn_decode_splits(B, Hkv, Nmax, num_splits, q.get_device())
    o = torch.empty(B, H, Nq, D, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device)
    # partials of the split kernel; it writes every element the merge reads
    ws = torch.empty(_C.attn_decode_workspace_floats(B, Hkv, splits), dtype=torch.float32, device=q.device)
    _C.attn_decode(q, k_cache, v_cache, kv_len, o, lse, ws, 1.0 / math.sqrt(D), causal, splits)
    return (o, lse) if return_lse else o


def _fp8_storable(k_cache, v_cache, k_new, k_scale, v_scale):
    # the append stores 8 bytes per lane; the scales as the kernels read them
    return all(
        t.data_ptr() % 8 == 0 and all(s % 8 == 0 for s in t.stride()[:-1]) for t in (k_cache, v_cache)
    ) and all(_fp8_scale_ok(s, k_new, k_new.shape[1]) for s in (k_scale, v_scale))


def kvcache_append(k_new, v_new, k_cache, v_cache, kv_len, block_table=None, k_scale=None, v_scale=None):
    """Write the K and V rows of Nq new tokens per batch row into a K/V cache,
    in place, at the positions `sdpa_kvcache` gives the same query rows.

    k_new, v_new are [B, Hkv, Nq, D] (strided views of a qkv projection
    pass). kv_len, integer [B], ALREADY counts the new rows, as in
    `sdpa_kvcache`: row i of batch row b goes to logical position
    clamp(kv_len[b], Nq, capacity) - Nq + i. Without a table the caches are
    [B, Hkv, Nmax, D], capacity = Nmax, and that is cache row (b, :, pos).
    With an integer `block_table` [B, max_pages] they are page pools
    [num_pages, Hkv, page_size, D], any page_size >= 1, capacity = max_pages *
    page_size, and it is row pos % page_size of page
    block_table[b, pos // page_size], the entry clamped to [0, num_pages - 1].
    No other cache row is written.

    Native path (`_C.kvcache_append`, one launch for K and V, positions
    resolved on the device: no host sync, hipGraph-capturable): all five
    tensors bf16 (kv_len and the table integer) on one device, D = 64 or 128,
    last dims contiguous, the caches 16-byte loadable (base and strides
    multiples of 8 elements; they are written in place and cannot be copied),
    extension built, no DMLCLOUD_DISABLE_FUSED_ATTN. k_new / v_new that are not
    16-byte loadable are copied first. Everything else runs
    `_attention_ref.kvcache_append_ref`, two index writes.

    FP8 cache: with float8_e4m3fn caches, element x of head h is stored as
    e4m3_rne(clamp(float(x) / scale[h], -448, 448)), `k_scale` / `v_scale`
    None (ones) or fp32 [Hkv] on the device (`_C.kvcache_append_fp8`; the
    caches then need base and strides that are multiples of 8 bytes). A scale
    with a cache of another dtype raises ValueError."""
    fp8 = _fp8_caches(k_cache, v_cache, k_scale, v_scale)
    tensors = (k_new, v_new, k_cache, v_cache)
    native = (
        fused_attention_enabled()
        and k_new.is_cuda
        and is_available()
        and k_new.dim() == 4
        and k_cache.dim() == 4
        and k_new.shape[-1] in (64, 128)
        and all(t.dtype == torch.bfloat16 for t in (tensors[:2] if fp8 else tensors))
        and all(t.device == k_new.device and t.stride(-1) == 1 for t in tensors)
        and (
            _fp8_storable(k_cache, v_cache, k_new, k_scale, v_scale)
            if fp8
            else _vector_loadable(k_cache) and _vector_loadable(v_cache)
        )
        and kv_len.dtype in _INT_DTYPES
        and kv_len.device == k_new.device
        and (block_table is None or (block_table.dtype in _INT_DTYPES and block_table.device == k_new.device))
    )
    if not native:
        from ._attention_ref import kvcache_append_ref

        return kvcache_append_ref(k_new, v_new, k_cache, v_cache, kv_len, block_table, k_scale, v_scale)
    k_new, v_new = (t if _vector_loadable(t) else t.contiguous() for t in (k_new, v_new))
    kv_len = kv_len.detach().to(torch.int32).contiguous()  # no-ops for an int32 tensor
    if block_table is not None and (block_table.dtype != torch.int32 or not block_table.is_contiguous()):
        block_table = block_table.detach().to(torch.int32).contiguous()
    if fp8:
        k_scale, v_scale = (None if s is None else s.detach().contiguous() for s in (k_scale, v_scale))
        _C.kvcache_append_fp8(k_new.detach(), v_new.detach(), k_cache, v_cache, kv_len, k_scale, v_scale, block_table)
        return
    _C.kvcache_append(k_new.detach(), v_new.detach(), k_cache, v_cache, kv_len, block_table)


def fused_attention_enabled() -> bool:
    """True unless DMLCLOUD_DISABLE_FUSED_ATTN opts out (the fused path
    is on by default for usable shapes)."""
    return os.environ.get('DMLCLOUD_DISABLE_FUSED_ATTN', '0') in ('0', '', 'false')
