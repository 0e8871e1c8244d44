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


def main_gqa():
    bench_gqa(64, 12, 4, 1024)  # the GPT-2 shape with 4 K/V heads
    bench_gqa(64, 12, 1, 1024)  # ... and as MQA
    bench_gqa(16, 16, 2, 2048)  # 1024 dK/dV blocks, each 8 heads long


if __name__ == '__main__':
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
