"""Tile-level flash-attention reference (the blueprint for the CDNA4
attention kernels — see docs/ROADMAP.md item 1).

This mirrors, op for op, the tiling the HIP kernels will use: Q tiles of
BQ rows iterate KV tiles of BK rows with online-softmax rescaling; the
backward recomputes P from the saved per-row lse and accumulates
dq/dk/dv tile by tile. Everything is fp32 math over bf16-roundable
inputs so the GPU kernel can be diff-tested against it tile-for-tile.

Conventions (per batch*head slice):
    q, k, v: [N, D]; causal masking optional.
    fwd returns (o [N, D], lse [N]) with lse = m + log(sumexp) per row.
    bwd consumes (do, q, k, v, o, lse) and returns (dq, dk, dv).
"""

import math
from typing import Optional, Tuple

import torch


def flash_attn_fwd_tiled(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool = True,
    bq: int = 32,
    bk: int = 64,
    scale: Optional[float] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    N, D = q.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    o = torch.zeros(N, D, dtype=torch.float32)
    lse = torch.empty(N, dtype=torch.float32)

    for i0 in range(0, N, bq):
        i1 = min(i0 + bq, N)
        qi = q[i0:i1].float()
        m = torch.full((i1 - i0,), -float('inf'))
        s_sum = torch.zeros(i1 - i0)
        acc = torch.zeros(i1 - i0, D)
        kv_end = i1 if causal else N
        for j0 in range(0, kv_end, bk):
            j1 = min(j0 + bk, N)
            s = (qi @ k[j0:j1].float().T) * scale  # [bq, bk]  (QK^T MFMA)
            if causal:
                row = torch.arange(i0, i1).unsqueeze(1)
                col = torch.arange(j0, j1).unsqueeze(0)
                s = s.masked_fill(col > row, -float('inf'))
            m_new = torch.maximum(m, s.max(dim=1).values)
            # rescale previous accumulator and sum (online softmax)
            alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - m_new))
            p = torch.exp(s - m_new.unsqueeze(1))  # [bq, bk]
            p = torch.nan_to_num(p, nan=0.0)  # -inf - -inf rows
            s_sum = s_sum * alpha + p.sum(dim=1)
            acc = acc * alpha.unsqueeze(1) + p @ v[j0:j1].float()  # (PV MFMA)
            m = m_new
        o[i0:i1] = acc / s_sum.unsqueeze(1)
        lse[i0:i1] = m + torch.log(s_sum)
    return o, lse


def flash_attn_bwd_tiled(
    do: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    o: torch.Tensor,
    lse: torch.Tensor,
    causal: bool = True,
    bq: int = 32,
    bk: int = 64,
    scale: Optional[float] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    N, D = q.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf, kf, vf, dof, of = (t.float() for t in (q, k, v, do, o))

    # delta = rowsum(dO * O)  (the bwd_preprocess kernel)
    delta = (dof * of).sum(dim=1)  # [N]

    dq = torch.zeros(N, D)
    dk = torch.zeros(N, D)
    dv = torch.zeros(N, D)

    # kv-tile outer loop (the dk/dv kernel); q-tile inner loop
    for j0 in range(0, N, bk):
        j1 = min(j0 + bk, N)
        i_start = j0 if causal else 0
        for i0 in range(i_start, N, bq):
            i1 = min(i0 + bq, N)
            s = (qf[i0:i1] @ kf[j0:j1].T) * scale
            if causal:
                row = torch.arange(i0, i1).unsqueeze(1)
                col = torch.arange(j0, j1).unsqueeze(0)
                s = s.masked_fill(col > row, -float('inf'))
            p = torch.exp(s - lse[i0:i1].unsqueeze(1))  # [bq, bk], recomputed
            p = torch.nan_to_num(p, nan=0.0)
            dv[j0:j1] += p.T @ dof[i0:i1]  # (P^T dO MFMA)
            dp = dof[i0:i1] @ vf[j0:j1].T  # (dO V^T MFMA)
            ds = p * (dp - delta[i0:i1].unsqueeze(1)) * scale
            dq[i0:i1] += ds @ kf[j0:j1]  # (dS K MFMA)
            dk[j0:j1] += ds.T @ qf[i0:i1]  # (dS^T Q MFMA)
    return dq, dk, dv


# ---------------------------------------------------------------------------
# Ragged-N emulation of the kernels' <kRagged = true> instantiations
# ---------------------------------------------------------------------------
#
# The HIP kernels never shorten a tile. When N is not a multiple of 64 a
# tile that hangs over the end of the sequence is still walked in full:
# its row loads are CLAMPED to N - 1 (so they re-read the last real row),
# the duplicated rows are MASKED out of the math, and stores are
# PREDICATED on row < N. The two functions below do exactly that, with
# the kernels' block / wave / sub-tile row ranges and loop bounds, so the
# masking logic can be proved on the CPU. Names follow attention.hip.

_NEG = -1e30  # the kernels' finite "minus infinity"
_LOG2E = 1.44269504


def _crow(rows: torch.Tensor, n: int) -> torch.Tensor:
    """crow<true>() of attention.hip: min(row, N - 1)."""
    return rows.clamp(max=n - 1)


def _dstart(doc_start: torch.Tensor, rows: torch.Tensor, n: int) -> torch.Tensor:
    """dstart() of attention.hip: the value read for row r = min(row,
    N - 1), clamped to [0, r]."""
    r = rows.clamp(max=n - 1)
    return torch.minimum(doc_start.long()[r].clamp(min=0), r)


def _dstart1(doc_start: torch.Tensor, row: int, n: int) -> int:
    return int(_dstart(doc_start, torch.tensor([row]), n)[0])


# Packed sequences: both functions below take an optional per-slice
# `doc_start[N]` (see ops/fused_attn.py for the semantics) and then emulate
# the kernels' <kDoc = true> instantiations: the same clamp, the same
# masks, the same block / wave tile skips and the dkdv break. Fully masked
# tiles of a straddling sub-tile are walked, not special-cased, so the
# -1e30 "wipe" (alpha = exp2(-1e30 - m) = 0 at the first valid tile) is
# what makes the result right here exactly as on the device. With
# doc_start=None not one operation changes.


def flash_attn_fwd_padded(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool = True,
    scale: Optional[float] = None,
    doc_start: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """attn_fwd_kernel<true>: 128-row blocks of 4 waves, each wave two
    16-row sub-tiles, full 64-key tiles, log2-domain online softmax."""
    N, D = q.shape
    assert doc_start is None or causal, 'doc_start requires causal attention'
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    scale2 = scale * _LOG2E
    qf, kf, vf = q.float(), k.float(), v.float()
    # poisoned outputs: a store the predicate should have made shows as NaN
    o = torch.full((N, D), float('nan'))
    lse = torch.full((N,), float('nan'))

    nqb = (N + 127) // 128
    for qb0 in range(0, nqb * 128, 128):
        kv_end_block = min(qb0 + 128, N) if causal else N
        ntiles = (kv_end_block + 63) // 64
        # block-level skip: the walk begins at the tile holding start[qb0]
        jt_begin = 0 if doc_start is None else _dstart1(doc_start, qb0, N) // 64
        for wave in range(4):
            i0 = qb0 + 32 * wave
            if not i0 < N:  # `valid`
                continue
            my_kv_end = i0 + 32 if causal else N
            for sub in range(2):
                qi0 = i0 + 16 * sub
                q_g = qi0 + torch.arange(16)
                qrows = qf[_crow(q_g, N)]
                if doc_start is not None:
                    q_start = _dstart(doc_start, q_g, N)
                    q_last = _crow(q_g, N)  # min(q, N - 1): causal and ragged end
                    sub_start = _dstart1(doc_start, qi0, N)
                m_run = torch.full((16,), _NEG)
                s_run = torch.zeros(16)
                acc = torch.zeros(16, D)
                for jt in range(jt_begin, ntiles):
                    j0 = jt * 64
                    if not j0 < my_kv_end:
                        continue
                    if causal and j0 >= qi0 + 16:
                        continue  # tile fully past the diagonal
                    if doc_start is not None and j0 + 64 <= sub_start:
                        continue  # tile wholly in earlier documents
                    key_g = j0 + torch.arange(64)
                    krows = kf[_crow(key_g, N)]
                    vrows = vf[_crow(key_g, N)]
                    s = (qrows @ krows.T) * scale2  # [16 q, 64 keys], log2 domain
                    if doc_start is not None:
                        # one range test: start[q] <= key <= min(q, N - 1)
                        dead = (key_g.unsqueeze(0) < q_start.unsqueeze(1)) | (key_g.unsqueeze(0) > q_last.unsqueeze(1))
                        s = s.masked_fill(dead, _NEG)
                    else:
                        if causal:
                            s = s.masked_fill(key_g.unsqueeze(0) > q_g.unsqueeze(1), _NEG)
                        s = s.masked_fill((key_g >= N).unsqueeze(0), _NEG)
                    m_new = torch.maximum(m_run, s.max(dim=1).values)
                    alpha = torch.exp2(m_run - m_new)
                    p = torch.exp2(s - m_new.unsqueeze(1))
                    s_run = s_run * alpha + p.sum(dim=1)
                    m_run = m_new
                    acc = acc * alpha.unsqueeze(1) + p @ vrows
                keep = q_g < N  # per-row store predicate
                o[q_g[keep]] = (acc / s_run.unsqueeze(1))[keep]
                lse[q_g[keep]] = (0.69314718 * m_run + torch.log(s_run))[keep]
    return o, lse


def flash_attn_bwd_padded(
    do: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    o: torch.Tensor,
    lse: torch.Tensor,
    causal: bool = True,
    scale: Optional[float] = None,
    doc_start: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """attn_bwd_delta_kernel + attn_bwd_dkdv_kernel<true> +
    attn_bwd_dq_kernel<true>."""
    N, D = q.shape
    assert doc_start is None or causal, 'doc_start requires causal attention'
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    scale2 = scale * _LOG2E
    qf, kf, vf, dof, of = (t.float() for t in (q, k, v, do, o))
    lse2 = lse.float() * _LOG2E

    # delta: one row at a time over the N real rows, nothing to clamp
    delta = (dof * of).sum(dim=1)

    dq = torch.full((N, D), float('nan'))
    dk = torch.full((N, D), float('nan'))
    dv = torch.full((N, D), float('nan'))

    def p_and_ds(q_g, key_g):
        """Recomputed P and dS for one [16 q, 16 keys] pair of clamped tiles."""
        qr, kr = _crow(q_g, N), _crow(key_g, N)
        s2 = (qf[qr] @ kf[kr].T) * scale2
        dp = dof[qr] @ vf[kr].T
        live = (key_g < N).unsqueeze(0) & (q_g < N).unsqueeze(1)
        if causal:
            live = live & (key_g.unsqueeze(0) <= q_g.unsqueeze(1))
        if doc_start is not None:  # p = 0 for key < start[q]
            live = live & (key_g.unsqueeze(0) >= _dstart(doc_start, q_g, N).unsqueeze(1))
        p = torch.where(live, torch.exp2(s2 - lse2[qr].unsqueeze(1)), torch.zeros(()))
        ds = p * (dp - delta[qr].unsqueeze(1)) * scale
        return p, ds

    # ---- dK / dV: 64-key blocks of 4 waves x 16 keys, 32-row q steps ----
    # (gqa_bwd_padded below emulates the <kGqa> form of this loop nest)
    nkb = (N + 63) // 64
    for kb0 in range(0, nkb * 64, 64):
        i_start = (kb0 & ~31) if causal else 0
        # the block-uniform break: the first q-step whose first row starts
        # behind the block's last key ends the walk for all four waves
        i_stop = N
        if doc_start is not None:
            for i0 in range(i_start, N, 32):
                if _dstart1(doc_start, i0, N) > kb0 + 63:
                    i_stop = i0
                    break
        for wave in range(4):
            j0 = kb0 + 16 * wave
            if not j0 < N:  # `valid`
                continue
            key_g = j0 + torch.arange(16)
            dv_acc = torch.zeros(16, D)
            dk_acc = torch.zeros(16, D)
            for i0 in range(i_start, i_stop, 32):
                if causal and not i0 + 32 > j0:
                    continue
                for hq in range(2):
                    q_g = i0 + 16 * hq + torch.arange(16)
                    p, ds = p_and_ds(q_g, key_g)
                    dv_acc += p.T @ dof[_crow(q_g, N)]
                    dk_acc += ds.T @ qf[_crow(q_g, N)]
            keep = key_g < N
            dv[key_g[keep]] = dv_acc[keep]
            dk[key_g[keep]] = dk_acc[keep]

    # ---- dQ: 64-row blocks of 4 waves x 16 q rows, 32-key tiles ----
    nqb = (N + 63) // 64
    for qb0 in range(0, nqb * 64, 64):
        kv_end_block = min(qb0 + 64, N) if causal else N
        # block-level skip: the walk begins at the 32-key tile holding start[qb0]
        j_begin = 0 if doc_start is None else _dstart1(doc_start, qb0, N) & ~31
        for wave in range(4):
            i0 = qb0 + 16 * wave
            if not i0 < N:  # `valid`
                continue
            my_kv_end = i0 + 16 if causal else N
            q_g = i0 + torch.arange(16)
            wave_start = 0 if doc_start is None else _dstart1(doc_start, i0, N)
            dq_acc = torch.zeros(16, D)
            for j0 in range(j_begin, kv_end_block, 32):
                if not j0 < my_kv_end:
                    continue
                if not j0 + 32 > wave_start:
                    continue  # tile wholly in earlier documents
                for h in range(2):
                    key_g = j0 + 16 * h + torch.arange(16)
                    _, ds = p_and_ds(q_g, key_g)
                    dq_acc += ds @ kf[_crow(key_g, N)]
            keep = q_g < N
            dq[q_g[keep]] = dq_acc[keep]
    return dq, dk, dv


def mha_fwd_tiled(q, k, v, causal=True, bq=32, bk=64):
    """[B, H, N, D] wrapper over the per-slice tile algorithm."""
    B, H, N, D = q.shape
    o = torch.empty(B, H, N, D, dtype=torch.float32)
    lse = torch.empty(B, H, N, dtype=torch.float32)
    for b in range(B):
        for h in range(H):
            o[b, h], lse[b, h] = flash_attn_fwd_tiled(q[b, h], k[b, h], v[b, h], causal, bq, bk)
    return o, lse


# ---------------------------------------------------------------------------
# Grouped-query attention: the kernels' <kGqa = true> instantiations
# ---------------------------------------------------------------------------
#
# q is [B, H, N, D], k and v are [B, Hkv, N, D], G = H // Hkv, and query
# head h reads K/V head h // G. Forward and dQ are the per-slice functions
# above on another K/V slice. dK/dV is one block per (b, K/V head, 64-key
# block) that walks the q-steps of the group's G heads one head after the
# other, in ascending head order, into ONE accumulator per wave, and stores
# each element once.


def gqa_fwd_padded(q, k, v, causal=True, scale=None, doc_start=None):
    """attn_fwd_kernel<..., kGqa = true>: (o [B, H, N, D], lse [B, H, N]).
    `doc_start` is [B, N] or None."""
    B, H, N, D = q.shape
    Hkv = k.shape[1]
    assert v.shape == k.shape and H % Hkv == 0
    G = H // Hkv
    o = torch.empty(B, H, N, D, dtype=torch.float32)
    lse = torch.empty(B, H, N, dtype=torch.float32)
    for b in range(B):
        ds = None if doc_start is None else doc_start[b]
        for h in range(H):
            o[b, h], lse[b, h] = flash_attn_fwd_padded(q[b, h], k[b, h // G], v[b, h // G], causal, scale, ds)
    return o, lse


def gqa_bwd_padded(do, q, k, v, o, lse, causal=True, scale=None, doc_start=None):
    """attn_bwd_delta_kernel + the <kGqa = true> dK/dV and dQ kernels:
    (dq [B, H, N, D], dk [B, Hkv, N, D], dv [B, Hkv, N, D])."""
    B, H, N, D = q.shape
    Hkv = k.shape[1]
    assert v.shape == k.shape and H % Hkv == 0
    assert doc_start is None or causal, 'doc_start requires causal attention'
    G = H // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    scale2 = scale * _LOG2E
    qf, kf, vf, dof, of = (t.float() for t in (q, k, v, do, o))
    lse2 = lse.float() * _LOG2E
    delta = (dof * of).sum(dim=-1)  # [B, H, N]

    dq = torch.empty(B, H, N, D)
    dk = torch.full((B, Hkv, N, D), float('nan'))
    dv = torch.full((B, Hkv, N, D), float('nan'))

    # dQ: per (b, query head) exactly flash_attn_bwd_padded's, on the
    # group's K/V slice
    for b in range(B):
        ds = None if doc_start is None else doc_start[b]
        for h in range(H):
            dq[b, h], _, _ = flash_attn_bwd_padded(
                do[b, h], q[b, h], k[b, h // G], v[b, h // G], o[b, h], lse[b, h], causal, scale, ds
            )

    # dK / dV: one block per (b, K/V head, 64-key block)
    nkb = (N + 63) // 64
    for b in range(B):
        ds = None if doc_start is None else doc_start[b]
        for kvh in range(Hkv):
            for kb0 in range(0, nkb * 64, 64):
                i_start = (kb0 & ~31) if causal else 0
                # the break depends on (b, kb0, i0) only: the same for every head
                i_stop = N
                if ds is not None:
                    for i0 in range(i_start, N, 32):
                        if _dstart1(ds, i0, N) > kb0 + 63:
                            i_stop = i0
                            break
                for wave in range(4):
                    j0 = kb0 + 16 * wave
                    if not j0 < N:  # `valid`
                        continue
                    key_g = j0 + torch.arange(16)
                    kr = _crow(key_g, N)
                    krows, vrows = kf[b, kvh][kr], vf[b, kvh][kr]  # kf / vf2, loaded once
                    dv_acc = torch.zeros(16, D)
                    dk_acc = torch.zeros(16, D)
                    for g in range(G):  # the group's heads, ascending
                        h = kvh * G + g
                        for i0 in range(i_start, i_stop, 32):
                            if causal and not i0 + 32 > j0:
                                continue
                            for hq in range(2):
                                q_g = i0 + 16 * hq + torch.arange(16)
                                qr = _crow(q_g, N)
                                s2 = (qf[b, h][qr] @ krows.T) * scale2
                                dp = dof[b, h][qr] @ vrows.T
                                live = (key_g < N).unsqueeze(0) & (q_g < N).unsqueeze(1)
                                if causal:
                                    live = live & (key_g.unsqueeze(0) <= q_g.unsqueeze(1))
                                if ds is not None:
                                    live = live & (key_g.unsqueeze(0) >= _dstart(ds, q_g, N).unsqueeze(1))
                                p = torch.where(live, torch.exp2(s2 - lse2[b, h][qr].unsqueeze(1)), torch.zeros(()))
                                dsc = p * (dp - delta[b, h][qr].unsqueeze(1)) * scale
                                dv_acc += p.T @ dof[b, h][qr]
                                dk_acc += dsc.T @ qf[b, h][qr]
                    keep = key_g < N
                    dv[b, kvh][key_g[keep]] = dv_acc[keep]
                    dk[b, kvh][key_g[keep]] = dk_acc[keep]
    return dq, dk, dv
