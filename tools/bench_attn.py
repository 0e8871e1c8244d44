"""Micro-benchmark: MFMA attention forward/backward vs SDPA (AOTriton),
aligned shapes plus one ragged sequence length (N=1000), plus packed
sequences (document mask) at the GPT-2 shape: the native kDoc kernels
beside the dense native causal kernels and beside torch SDPA given the
equivalent boolean attn_mask; plus grouped-query attention (bench_gqa):
the native kGqa kernels beside repeat_interleave + the native MHA kernels,
torch SDPA with enable_gqa=True, and the plain MHA row at the same H.

    python tools/bench_attn.py            # every section
    python tools/bench_attn.py --no-gqa   # the sections before GQA
    python tools/bench_attn.py --gqa      # the GQA section alone
    python tools/bench_attn.py --decode   # KV-cache decode (sdpa_kvcache) alone
    python tools/bench_attn.py --decode-tiled   # sdpa_kvcache, more than 16 columns
    python tools/bench_attn.py --decode-d128    # sdpa_kvcache at head dim 128
    python tools/bench_attn.py --decode-paged   # paged cache against dense; kvcache_append
    python tools/bench_attn.py --decode-fp8     # fp8 (e4m3) cache against bf16; quantising append
    python tools/bench_attn.py --d128     # head dim 128: native against the torch SDPA fallback
"""

import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from dmlcloud_amd import _C

DEV = 'cuda:0'


def time_fn(fn, reps=30, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3  # us


def bench(b, h, n, d=64, causal=True):
    torch.manual_seed(0)
    q = (torch.randn(b, h, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    k = (torch.randn(b, h, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    v = (torch.randn(b, h, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    o = torch.empty_like(q)
    lse = torch.empty(b, h, n, dtype=torch.float32, device=DEV)
    scale = 1.0 / math.sqrt(d)

    t_ours = time_fn(lambda: _C.attn_fwd(q, k, v, o, lse, scale, causal))
    with torch.no_grad():
        t_sdpa = time_fn(
            lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal)
        )
    flops = 4 * b * h * n * n * d * (0.5 if causal else 1.0)
    print(
        f'B={b} H={h} N={n} causal={causal}: ours {t_ours:8.1f}us ({flops/t_ours/1e6:6.1f} TF) '
        f'| sdpa {t_sdpa:8.1f}us ({flops/t_sdpa/1e6:6.1f} TF)'
    )


def bench_bwd(b, h, n, d=64, causal=True):
    from dmlcloud_amd.ops.fused_attn import sdpa

    torch.manual_seed(0)
    mk = lambda: (torch.randn(b, h, n, d, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
    q1, k1, v1 = mk(), mk(), mk()
    do = (torch.randn(b, h, n, d, device=DEV) * 0.5).to(torch.bfloat16)

    out1 = sdpa(q1, k1, v1, causal=causal)

    def ours_bwd():
        q1.grad = k1.grad = v1.grad = None
        out1.backward(do, retain_graph=True)

    q2, k2, v2 = mk(), mk(), mk()
    out2 = torch.nn.functional.scaled_dot_product_attention(q2, k2, v2, is_causal=causal)

    def sdpa_bwd():
        q2.grad = k2.grad = v2.grad = None
        out2.backward(do, retain_graph=True)

    t_ours = time_fn(ours_bwd, reps=20)
    t_ref = time_fn(sdpa_bwd, reps=20)
    flops = 4 * b * h * n * n * d * (0.5 if causal else 1.0) * 2.5  # bwd ~2.5x fwd
    print(
        f'BWD B={b} H={h} N={n} causal={causal}: ours {t_ours:8.1f}us ({flops/t_ours/1e6:6.1f} TF) '
        f'| sdpa {t_ref:8.1f}us ({flops/t_ref/1e6:6.1f} TF)'
    )


def doc_layouts(n):
    """name -> document lengths for one row of n tokens (all rows alike)."""
    g = torch.Generator().manual_seed(1234)
    lengths = []
    while sum(lengths) < n:  # uniform on [1, 399]: mean 200
        lengths.append(min(int(torch.randint(1, 400, (1,), generator=g)), n - sum(lengths)))
    return {
        '1 doc': [n],
        f'{n // 128} docs of 128': [128] * (n // 128),
        f'{len(lengths)} random docs (mean ~200)': lengths,
    }


def bench_doc(b, h, n, d=64):
    """Forward and backward, causal, per layout: native with doc_start |
    native dense causal (no mask: the cost to compare against) | torch
    SDPA with the boolean [B, 1, N, N] mask a user builds today."""
    from dmlcloud_amd.ops.fused_attn import document_mask, sdpa

    torch.manual_seed(0)
    mk = lambda: (torch.randn(b, h, n, d, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
    q, k, v = mk(), mk(), mk()
    do = (torch.randn(b, h, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    o = torch.empty(b, h, n, d, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(b, h, n, dtype=torch.float32, device=DEV)
    scale = 1.0 / math.sqrt(d)

    def bwd_timer(out):
        def run():
            q.grad = k.grad = v.grad = None
            out.backward(do, retain_graph=True)

        return time_fn(run, reps=20)

    with torch.no_grad():
        f_dense = time_fn(lambda: _C.attn_fwd(q, k, v, o, lse, scale, True))
    b_dense = bwd_timer(sdpa(q, k, v, causal=True))

    for name, lengths in doc_layouts(n).items():
        starts = torch.tensor([0] + lengths[:-1]).cumsum(0)
        row = torch.repeat_interleave(starts, torch.tensor(lengths)).to(torch.int32)
        ds = row.unsqueeze(0).expand(b, n).contiguous().to(DEV)
        mask = document_mask(ds, causal=True)
        with torch.no_grad():
            f_doc = time_fn(lambda: _C.attn_fwd(q, k, v, o, lse, scale, True, ds))
            f_mask = time_fn(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask))
        b_doc = bwd_timer(sdpa(q, k, v, causal=True, doc_start=ds))
        b_mask = bwd_timer(torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask))
        for tag, t_doc, t_dense, t_mask in (('DOC FWD', f_doc, f_dense, f_mask), ('DOC BWD', b_doc, b_dense, b_mask)):
            print(
                f'{tag} B={b} H={h} N={n} {name}: doc {t_doc:8.1f}us | dense {t_dense:8.1f}us '
                f'({t_dense / t_doc:4.2f}x) | masked sdpa {t_mask:8.1f}us ({t_mask / t_doc:4.2f}x)'
            )


def bench_gqa(b, h, hkv, n, d=64):
    """Causal forward and backward with `hkv` K/V heads for `h` query
    heads, every native column through `sdpa`: native GQA | what a user
    had before (repeat_interleave + native MHA; the forward times the
    expansion, the backward autograd's sum over the group) | torch SDPA
    with enable_gqa=True | native MHA at the same H on already expanded
    K/V (the same FLOPs, no expansion: the cost to compare against)."""
    from dmlcloud_amd.ops.fused_attn import fused_attention_usable, sdpa

    g = h // hkv
    torch.manual_seed(0)
    mk = lambda heads: (torch.randn(b, heads, n, d, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
    q, k, v = mk(h), mk(hkv), mk(hkv)
    ke, ve = mk(h), mk(h)
    do = (torch.randn(b, h, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    assert fused_attention_usable(q, k, v) and fused_attention_usable(q, ke, ve)

    forwards = {
        'gqa': lambda: sdpa(q, k, v, causal=True),
        'expand': lambda: sdpa(q, k.repeat_interleave(g, 1), v.repeat_interleave(g, 1), causal=True),
        'torch': lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=True),
        'mha': lambda: sdpa(q, ke, ve, causal=True),
    }
    t_fwd, t_bwd = {}, {}
    for name, fwd in forwards.items():
        with torch.no_grad():
            t_fwd[name] = time_fn(fwd)
        out = fwd()

        def bwd():
            q.grad = k.grad = v.grad = ke.grad = ve.grad = None
            out.backward(do, retain_graph=True)

        t_bwd[name] = time_fn(bwd, reps=20)
    for tag, t in (('GQA FWD', t_fwd), ('GQA BWD', t_bwd)):
        print(
            f'{tag} B={b} H={h} Hkv={hkv} N={n}: gqa {t["gqa"]:8.1f}us | expand+mha {t["expand"]:8.1f}us '
            f'({t["expand"] / t["gqa"]:4.2f}x) | torch gqa {t["torch"]:8.1f}us ({t["torch"] / t["gqa"]:4.2f}x) '
            f'| mha H={h} {t["mha"]:8.1f}us ({t["mha"] / t["gqa"]:4.2f}x)'
        )


HBM_COPY_BYTES_PER_S = 4.4e12  # the copy kernel's measured rate (profiles/ops_bandwidth_mi355x.txt)


def bench_decode(b, h, hkv, nmax, d=64):
    """One causal decode step (Nq = 1) over a FULL cache, kv_len = Nmax:
    native with the automatic split count | native num_splits=1 | torch
    SDPA given the boolean [B, 1, 1, Nmax] mask (what a user has today;
    building the mask is not timed) | the HBM floor: the K + V bytes at the
    copy kernel's rate."""
    from dmlcloud_amd.ops.fused_attn import fused_kvcache_usable, sdpa_kvcache

    torch.manual_seed(0)
    mk = lambda heads, n: (torch.randn(b, heads, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    q, k, v = mk(h, 1), mk(hkv, nmax), mk(hkv, nmax)
    kv_len = torch.full((b,), nmax, dtype=torch.int32, device=DEV)
    assert fused_kvcache_usable(q, k, v, kv_len)
    mask = (torch.arange(nmax, device=DEV)[None, :] < kv_len[:, None]).view(b, 1, 1, nmax)
    gqa = {'enable_gqa': True} if hkv != h else {}
    with torch.no_grad():
        t_auto = time_fn(lambda: sdpa_kvcache(q, k, v, kv_len), reps=200, warmup=20)
        t_one = time_fn(lambda: sdpa_kvcache(q, k, v, kv_len, num_splits=1), reps=200, warmup=20)
        t_torch = time_fn(
            lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, **gqa),
            reps=200,
            warmup=20,
        )
    floor = 2 * k.numel() * k.element_size() / HBM_COPY_BYTES_PER_S * 1e6
    splits = _C.attn_decode_splits(b, hkv, nmax, 0, 0)
    print(
        f'DECODE B={b} H={h} Hkv={hkv} Nmax={nmax}: native S={splits} {t_auto:8.1f}us | native S=1 {t_one:8.1f}us '
        f'| masked sdpa {t_torch:8.1f}us | HBM floor {floor:6.1f}us ({floor / t_auto:4.2f} of floor reached)'
    )


def main_decode():
    for rnd in range(3):  # three rounds in one session: the spread
        print(f'-- round {rnd + 1}')
        bench_decode(8, 12, 12, 1024)
        bench_decode(8, 12, 12, 4096)
        bench_decode(64, 12, 12, 1024)
        bench_decode(8, 32, 8, 4096)


def bench_decode_tiled(b, h, hkv, nq, nmax, d=64):
    """Nq new causal rows with (H / Hkv) * Nq > 16 over a FULL cache,
    kv_len = Nmax: native tiled kernels with the automatic split count |
    native num_splits=1 | kvcache_attention_ref on the device (what
    sdpa_kvcache ran for these shapes before the tiled kernels) | for
    Nq >= 64, the training forward sdpa() over the chunk's own Nq keys alone:
    fewer FLOPs, but the project's compute-bound rate."""
    from dmlcloud_amd.ops._attention_ref import kvcache_attention_ref
    from dmlcloud_amd.ops.fused_attn import fused_kvcache_usable, sdpa, sdpa_kvcache

    torch.manual_seed(0)
    mk = lambda heads, n: (torch.randn(b, heads, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    q, k, v = mk(h, nq), mk(hkv, nmax), mk(hkv, nmax)
    kv_len = torch.full((b,), nmax, dtype=torch.int32, device=DEV)
    r = h // hkv * nq
    assert r > 16 and fused_kvcache_usable(q, k, v, kv_len)
    with torch.no_grad():
        t_auto = time_fn(lambda: sdpa_kvcache(q, k, v, kv_len), reps=200, warmup=20)
        t_one = time_fn(lambda: sdpa_kvcache(q, k, v, kv_len, num_splits=1), reps=200, warmup=20)
        t_ref = time_fn(lambda: kvcache_attention_ref(q, k, v, kv_len, True, False), reps=200, warmup=20)
        line = ''
        if nq >= 64:
            t_fwd = time_fn(lambda: sdpa(q, k[:, :, -nq:], v[:, :, -nq:], causal=True), reps=200, warmup=20)
            line = f' | sdpa over the chunk alone {t_fwd:8.1f}us ({2 * b * h * nq * nq * d / t_fwd / 1e6:6.1f} TF)'
    # causal, full cache: row i attends nmax - nq + i + 1 keys
    flops = 4 * b * h * d * (nq * (nmax - nq) + nq * (nq + 1) / 2)
    splits = _C.attn_decode_tiled_splits(b, hkv, r, nmax, 0, 0)
    print(
        f'DECODE-TILED B={b} H={h} Hkv={hkv} Nq={nq} Nmax={nmax} R={r}: native S={splits} {t_auto:8.1f}us '
        f'({flops / t_auto / 1e6:6.1f} TF) | native S=1 {t_one:8.1f}us | torch reference {t_ref:8.1f}us' + line
    )


def main_decode_tiled():
    for rnd in range(3):  # three rounds in one session: the spread
        print(f'-- round {rnd + 1}')
        bench_decode_tiled(8, 12, 12, 32, 1024)
        bench_decode_tiled(8, 32, 4, 4, 4096)
        bench_decode_tiled(8, 12, 12, 256, 1024)
        bench_decode_tiled(1, 12, 12, 512, 4096)


def bench_decode_d128(b, h, hkv, nq, nmax):
    """Head dim 128, Nq new causal rows over a FULL cache, kv_len = Nmax:
    native (attn_decode_d128_kernel) with the automatic split count | native
    num_splits=1 | kvcache_attention_ref on the device (what sdpa_kvcache ran
    at D = 128 before these kernels) | for Nq = 1, the D = 64 native kernels
    at twice the head count: the same K + V bytes."""
    from dmlcloud_amd.ops._attention_ref import kvcache_attention_ref
    from dmlcloud_amd.ops.fused_attn import fused_kvcache_usable, sdpa_kvcache

    torch.manual_seed(0)
    mk = lambda heads, n, d: (torch.randn(b, heads, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    q, k, v = mk(h, nq, 128), mk(hkv, nmax, 128), mk(hkv, nmax, 128)
    kv_len = torch.full((b,), nmax, dtype=torch.int32, device=DEV)
    assert fused_kvcache_usable(q, k, v, kv_len)
    with torch.no_grad():
        t_auto = time_fn(lambda: sdpa_kvcache(q, k, v, kv_len), reps=200, warmup=20)
        t_one = time_fn(lambda: sdpa_kvcache(q, k, v, kv_len, num_splits=1), reps=200, warmup=20)
        t_ref = time_fn(lambda: kvcache_attention_ref(q, k, v, kv_len, True, False), reps=200, warmup=20)
        line = ''
        if nq == 1:
            q6, k6, v6 = mk(2 * h, 1, 64), mk(2 * hkv, nmax, 64), mk(2 * hkv, nmax, 64)
            t_d64 = time_fn(lambda: sdpa_kvcache(q6, k6, v6, kv_len), reps=200, warmup=20)
            line = f' | D=64 native H={2 * h} Hkv={2 * hkv} (same bytes) {t_d64:8.1f}us ({t_auto / t_d64:4.2f}x of it)'
    splits = _C.attn_decode_tiled_splits(b, hkv, h // hkv * nq, nmax, 0, 0)
    best = min(t_auto, t_one)
    print(
        f'DECODE-D128 B={b} H={h} Hkv={hkv} Nq={nq} Nmax={nmax}: native S={splits} {t_auto:8.1f}us '
        f'| native S=1 {t_one:8.1f}us | torch reference {t_ref:8.1f}us ({t_ref / best:5.2f}x the better native)' + line,
        flush=True,
    )


def main_decode_d128():
    for rnd in range(3):  # three rounds in one session: the spread
        print(f'-- round {rnd + 1}')
        bench_decode_d128(8, 6, 6, 1, 1024)
        bench_decode_d128(8, 6, 6, 1, 4096)
        bench_decode_d128(8, 32, 8, 1, 4096)
        bench_decode_d128(8, 6, 6, 32, 1024)
        bench_decode_d128(1, 8, 8, 512, 4096)


def _spread(ts):
    ts = sorted(ts)
    return f'{ts[len(ts) // 2]:7.1f}us [{ts[0]:.1f}..{ts[-1]:.1f}]'


def bench_decode_paged(b, h, hkv, nq, nmax, d, rounds=3):
    """Nq new causal rows over a FULL cache of nmax keys: the dense native
    path | the paged kernels at page_size 64 | at 256, pages shuffled over
    the pool; the three alternate over `rounds` rounds in one process.
    Median and min..max per cell."""
    from dmlcloud_amd.ops.fused_attn import fused_kvcache_usable, sdpa_kvcache

    torch.manual_seed(0)
    mk = lambda heads, n: (torch.randn(b, heads, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    q, k, v = mk(h, nq), mk(hkv, nmax), mk(hkv, nmax)
    kv_len = torch.full((b,), nmax, dtype=torch.int32, device=DEV)
    fns = {'dense': lambda: sdpa_kvcache(q, k, v, kv_len)}
    for ps in (64, 256):
        n = b * nmax // ps
        table = torch.randperm(n, device=DEV).to(torch.int32).view(b, nmax // ps)
        pools = []
        for t in (k, v):  # page table[b, p] holds rows p * ps .. of batch row b
            pool = torch.empty(n, hkv, ps, d, dtype=t.dtype, device=DEV)
            pool[table.long().view(-1)] = t.view(b, hkv, nmax // ps, ps, d).transpose(1, 2).reshape(n, hkv, ps, d)
            pools.append(pool)
        assert fused_kvcache_usable(q, *pools, kv_len, table)
        fns[f'paged {ps}'] = lambda pools=pools, table=table: sdpa_kvcache(q, *pools, kv_len, block_table=table)
    with torch.no_grad():
        want = fns['dense']()
        assert all(torch.equal(fn(), want) for fn in fns.values()), 'paged and dense outputs differ'
        times = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                times[name].append(time_fn(fn, reps=200, warmup=20))
    print(
        f'DECODE-PAGED D={d} B={b} H={h} Hkv={hkv} Nq={nq} Nmax={nmax}: '
        + ' | '.join(f'{name} {_spread(ts)}' for name, ts in times.items()),
        flush=True,
    )


def bench_append(b, hkv, nq, d, nmax=1024, rounds=3):
    """One kvcache_append (dense cache, and paged at page_size 64) against the
    two index_put calls of CausalSelfAttention.decode / extend, new rows
    taken as strided views of a qkv projection, alternated."""
    from dmlcloud_amd.ops.fused_attn import kvcache_append

    torch.manual_seed(0)
    qkv = torch.randn(b, nq, 3 * hkv * d, device=DEV).to(torch.bfloat16)
    k_new, v_new = (t.view(b, nq, hkv, d).transpose(1, 2) for t in qkv.split(hkv * d, dim=2)[1:])
    k, v = (torch.zeros(b, hkv, nmax, d, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    kp, vp = (t.view(b * nmax // 64, hkv, 64, d) for t in (torch.zeros_like(k), torch.zeros_like(v)))
    table = torch.randperm(b * nmax // 64, device=DEV).to(torch.int32).view(b, nmax // 64)
    kv_len = torch.full((b,), 512 + nq, dtype=torch.int32, device=DEV)
    rows = (kv_len.long() - nq).unsqueeze(1) + torch.arange(nq, device=DEV)
    batch = torch.arange(b, device=DEV).unsqueeze(1)

    def index_put():
        k[batch, :, rows] = k_new.transpose(1, 2)
        v[batch, :, rows] = v_new.transpose(1, 2)

    fns = {
        'two index_put': index_put,
        'kvcache_append dense': lambda: kvcache_append(k_new, v_new, k, v, kv_len),
        'kvcache_append paged 64': lambda: kvcache_append(k_new, v_new, kp, vp, kv_len, table),
    }
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(time_fn(fn, reps=200, warmup=20))
    print(
        f'APPEND B={b} Hkv={hkv} Nq={nq} D={d}: ' + ' | '.join(f'{name} {_spread(ts)}' for name, ts in times.items()),
        flush=True,
    )


def main_decode_paged():
    bench_decode_paged(8, 12, 12, 1, 1024, 64)
    bench_decode_paged(8, 32, 8, 1, 4096, 64)
    bench_decode_paged(1, 12, 12, 512, 4096, 64)
    bench_decode_paged(8, 6, 6, 1, 4096, 128)
    bench_decode_paged(1, 8, 8, 512, 4096, 128)
    bench_append(64, 12, 1, 64)
    bench_append(8, 12, 256, 64)


def _fp8_scales(hkv):
    return 0.0071 + 0.0023 * torch.arange(hkv, dtype=torch.float32, device=DEV)


def bench_decode_fp8(b, h, hkv, nq, nmax, d, caches=1, rounds=3):
    """Nq new causal rows over a FULL dense cache of nmax keys: the bf16 native
    kernels | the fp8 kernel on the same keys quantised, alternated over
    `rounds` rounds in one process. caches > 1 rotates the calls of both
    columns over that many distinct cache pairs, so that no call finds its
    keys in the 256 MB Infinity Cache."""
    from dmlcloud_amd.ops._attention_ref import quantize_fp8
    from dmlcloud_amd.ops.fused_attn import fused_kvcache_usable, sdpa_kvcache

    torch.manual_seed(0)
    mk = lambda heads, n: (torch.randn(b, heads, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    q, ks, vs = mk(h, nq), _fp8_scales(hkv), _fp8_scales(hkv) * 2
    kv_len = torch.full((b,), nmax, dtype=torch.int32, device=DEV)
    bf16 = [(mk(hkv, nmax), mk(hkv, nmax)) for _ in range(caches)]
    fp8 = [(quantize_fp8(k, ks), quantize_fp8(v, vs)) for k, v in bf16]
    assert fused_kvcache_usable(q, *fp8[0], kv_len, None, ks, vs)
    turn = {'bf16': 0, 'fp8': 0}

    def run(name):
        i = turn[name] = (turn[name] + 1) % caches
        if name == 'bf16':
            return sdpa_kvcache(q, *bf16[i], kv_len)
        return sdpa_kvcache(q, *fp8[i], kv_len, k_scale=ks, v_scale=vs)

    mb = lambda pairs: sum(t.numel() * t.element_size() for p in pairs for t in p) / 2**20
    with torch.no_grad():
        times = {name: [] for name in turn}
        for _ in range(rounds):
            for name in turn:
                times[name].append(time_fn(lambda: run(name), reps=200, warmup=20))
    print(
        f'DECODE-FP8 D={d} B={b} H={h} Hkv={hkv} Nq={nq} Nmax={nmax} caches={caches} '
        f'({mb(bf16):.0f} MB bf16, {mb(fp8):.0f} MB fp8): ' + ' | '.join(f'{name} {_spread(ts)}' for name, ts in times.items()),
        flush=True,
    )


def bench_append_fp8(b, hkv, nq, d, nmax=1024, rounds=3):
    """kvcache_append into a bf16 dense cache against the quantising append
    into an fp8 one (dense, and paged at page_size 64), alternated."""
    from dmlcloud_amd.ops.fused_attn import kvcache_append

    torch.manual_seed(0)
    qkv = torch.randn(b, nq, 3 * hkv * d, device=DEV).to(torch.bfloat16)
    k_new, v_new = (t.view(b, nq, hkv, d).transpose(1, 2) for t in qkv.split(hkv * d, dim=2)[1:])
    k, v = (torch.zeros(b, hkv, nmax, d, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    k8, v8 = (torch.zeros(b, hkv, nmax, d, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn) for _ in range(2))
    kp, vp = (torch.zeros_like(t).view(b * nmax // 64, hkv, 64, d) for t in (k8, v8))
    table = torch.randperm(b * nmax // 64, device=DEV).to(torch.int32).view(b, nmax // 64)
    kv_len = torch.full((b,), 512 + nq, dtype=torch.int32, device=DEV)
    s = dict(k_scale=_fp8_scales(hkv), v_scale=_fp8_scales(hkv) * 2)
    fns = {
        'bf16 dense': lambda: kvcache_append(k_new, v_new, k, v, kv_len),
        'fp8 dense': lambda: kvcache_append(k_new, v_new, k8, v8, kv_len, **s),
        'fp8 paged 64': lambda: kvcache_append(k_new, v_new, kp, vp, kv_len, table, **s),
    }
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(time_fn(fn, reps=200, warmup=20))
    print(
        f'APPEND-FP8 B={b} Hkv={hkv} Nq={nq} D={d}: ' + ' | '.join(f'{name} {_spread(ts)}' for name, ts in times.items()),
        flush=True,
    )


def main_decode_fp8():
    bench_decode_fp8(8, 12, 12, 1, 1024, 64)
    bench_decode_fp8(8, 32, 8, 1, 4096, 64)
    bench_decode_fp8(1, 12, 12, 512, 4096, 64)
    bench_decode_fp8(8, 6, 6, 1, 4096, 128)
    bench_decode_fp8(1, 8, 8, 512, 4096, 128)
    # 10 x 64 MB of bf16 K and V per column (10 x 32 MB fp8): past the Infinity Cache
    bench_decode_fp8(8, 32, 8, 1, 4096, 64, caches=10)
    bench_decode_fp8(8, 16, 8, 1, 4096, 128, caches=5)
    bench_append_fp8(64, 12, 1, 64)
    bench_append_fp8(8, 12, 256, 64)


def main_gqa():
    bench_gqa(64, 12, 4, 1024)  # the GPT-2 shape with 4 K/V heads
    bench_gqa(64, 12, 1, 1024)  # ... and as MQA
    bench_gqa(16, 16, 2, 2048)  # 1024 dK/dV blocks, each 8 heads long


def bench_d128(b, h, hkv, n, docs=False, rounds=3):
    """Head dim 128, causal, through `sdpa`: forward and forward+backward,
    the native kernels against the fallback (DMLCLOUD_DISABLE_FUSED_ATTN=1:
    torch SDPA, with the boolean mask for documents), the two alternating
    over `rounds` rounds in one process. Prints median and min..max per
    cell, the achieved TF of the medians and the fallback / native ratio."""
    from dmlcloud_amd.ops.fused_attn import document_starts, sdpa

    d = 128
    torch.manual_seed(0)
    mk = lambda heads: (torch.randn(b, heads, n, d, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
    q, k, v = mk(h), mk(hkv), mk(hkv)
    do = (torch.randn(b, h, n, d, device=DEV) * 0.5).to(torch.bfloat16)
    kw = {}
    if docs:  # documents of 512 tokens, a ragged one first
        ids = ((torch.arange(n, device=DEV) + 200) // 512).expand(b, n)
        kw = {'doc_start': document_starts(ids)}

    def fwd():
        with torch.no_grad():
            sdpa(q, k, v, causal=True, **kw)

    def fwd_bwd():
        q.grad = k.grad = v.grad = None
        sdpa(q, k, v, causal=True, **kw).backward(do)

    times = {}
    for _ in range(rounds):
        for path, off in (('native', '0'), ('torch', '1')):
            os.environ['DMLCLOUD_DISABLE_FUSED_ATTN'] = off
            for name, fn in (('fwd', fwd), ('fwd+bwd', fwd_bwd)):
                times.setdefault((path, name), []).append(time_fn(fn, reps=10, warmup=3))
    os.environ['DMLCLOUD_DISABLE_FUSED_ATTN'] = '0'
    flops = 4 * b * h * n * n * d * 0.5  # dense causal count, also for the document row
    for name, mult in (('fwd', 1.0), ('fwd+bwd', 3.5)):
        cell = {}
        for path in ('native', 'torch'):
            t = sorted(times[(path, name)])
            cell[path] = t[len(t) // 2]
            cell[path + '_txt'] = f'{cell[path]:9.1f}us [{t[0]:.1f}..{t[-1]:.1f}] ({flops * mult / cell[path] / 1e6:6.1f} TF)'
        print(
            f'D128 {name:7s} B={b} H={h} Hkv={hkv} N={n}{" docs" if docs else ""}: native {cell["native_txt"]} '
            f'| torch {cell["torch_txt"]} | torch/native {cell["torch"] / cell["native"]:4.2f}x',
            flush=True,
        )


def main_d128():
    bench_d128(8, 16, 16, 1024)
    bench_d128(8, 16, 16, 2048)
    bench_d128(4, 16, 16, 4096)
    bench_d128(8, 16, 4, 2048)  # GQA
    bench_d128(8, 16, 16, 2048, docs=True)  # packed documents


if __name__ == '__main__':
    if '--d128' in sys.argv[1:]:
        main_d128()
        sys.exit(0)
    if '--decode-d128' in sys.argv[1:]:
        main_decode_d128()
        sys.exit(0)
    if '--decode-paged' in sys.argv[1:]:
        main_decode_paged()
        sys.exit(0)
    if '--decode-fp8' in sys.argv[1:]:
        main_decode_fp8()
        sys.exit(0)
    if '--decode' in sys.argv[1:]:
        main_decode()
        sys.exit(0)
    if '--decode-tiled' in sys.argv[1:]:
        main_decode_tiled()
        sys.exit(0)
    if '--gqa' in sys.argv[1:]:
        main_gqa()
        sys.exit(0)
    bench(64, 12, 1024)  # the GPT-2 bench shape
    bench(64, 12, 1024, causal=False)
    bench(16, 16, 2048)
    bench(8, 32, 4096)
    bench_bwd(64, 12, 1024)
    bench_bwd(64, 12, 1024, causal=False)
    bench_bwd(16, 16, 2048)
    # ragged N (not a multiple of 64): the kRagged kernel instantiations
    # walk exactly the tiles of the N=1024 rows above; sdpa beside each
    bench(64, 12, 1000)
    bench_bwd(64, 12, 1000)
    # packed sequences at the GPT-2 shape (needs the doc_start bindings)
    bench_doc(64, 12, 1024)
    # grouped-query attention (needs the kGqa kernels)
    if '--no-gqa' not in sys.argv[1:]:
        main_gqa()
