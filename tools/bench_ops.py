"""Micro-benchmarks of the core gfx950 ops: chunked copy bandwidth,
metric reduction, fused Adam. Run on a GPU box."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from dmlcloud_amd import ops

DEV = 'cuda:0'


def time_fn(fn, reps=50, warmup=10):
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


def bench_copy():
    print('== chunked_copy (pack) bandwidth ==')
    for total_mb, ntensors in [(64, 16), (512, 64), (2048, 128)]:
        per = total_mb * (1 << 20) // ntensors // 4
        srcs = [torch.randn(per, device=DEV) for _ in range(ntensors)]
        flat = torch.zeros(per * ntensors, device=DEV)
        dsts = [flat[i * per : (i + 1) * per] for i in range(ntensors)]
        us = time_fn(lambda: ops.chunked_copy(srcs, dsts), reps=20)
        gbs = 2 * total_mb / 1024 / (us / 1e6)  # read+write
        print(f'  {total_mb:5d} MB in {ntensors:4d} tensors: {us:9.1f} us  -> {gbs:7.0f} GB/s (r+w)')


def bench_reduce():
    print('== metric_reduce_into (full reduction into scalar acc) ==')
    for n in [1, 1024, 1 << 20, 1 << 26]:
        v = torch.randn(n, device=DEV)
        acc = torch.zeros(1, dtype=torch.float64, device=DEV)
        cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
        us = time_fn(lambda: ops.metric_reduce_into(v, acc, cnt, ops.OP_SUM))
        gbs = n * 4 / (us / 1e6) / 1e9
        print(f'  n={n:>10}: {us:8.1f} us  ({gbs:7.1f} GB/s)')


def bench_adam():
    print('== fused_adam ==')
    for n in [1 << 16, 1 << 22, 1 << 26]:
        p = torch.randn(n, device=DEV)
        g = torch.randn(n, device=DEV)
        m = torch.zeros(n, device=DEV)
        v = torch.zeros(n, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        us = time_fn(lambda: ops.fused_adam(p, g, m, v, st, 1e-3, 0.9, 0.999, 1e-8, 0.0))
        gbs = n * 4 * 7 / (us / 1e6) / 1e9  # 4 reads + 3 writes
        print(f'  n={n:>10}: {us:8.1f} us  ({gbs:7.1f} GB/s of 7x traffic)')


GPT2_FLAT = 124_439_808  # elements of gpt2_small's flat buffer


def _adam_state(n, bf16):
    p = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV)
    if bf16:
        return dict(param=p.to(torch.bfloat16), grad=g.to(torch.bfloat16), master=p)
    return dict(param=p, grad=g)


def bench_adamw(sizes=(1 << 16, 1 << 22, 1 << 26), rounds=1, reps=50):
    """fused_adamw_grouped(_bf16) next to fused_adam(_bf16), alternating in
    one session. Both move 28 B per element (grad read, param written,
    master/moments read and written; the fp32 kernels read and write param
    instead of a master); the grouped kernels add 1/8 B of group map."""
    print('== fused_adamw_grouped vs fused_adam: us, TB/s of 28 (+1/8) B per element ==')
    for n in sizes:
        for bf16 in (False, True):
            name = 'bf16' if bf16 else 'fp32'
            s = _adam_state(n, bf16)
            m = torch.zeros(n, device=DEV)
            v = torch.zeros(n, device=DEV)
            st = torch.zeros(1, dtype=torch.int32, device=DEV)
            # two groups laid out as weight_decay_groups does: decayed first
            group_map = (torch.arange(n // 8, device=DEV) >= int(n // 8 * 0.7)).to(torch.uint8)
            hyper = torch.tensor(
                [[1e-3, 0.1, 0.9, 0.999, 1e-8, 0, 0, 0], [1e-3, 0.0, 0.9, 0.999, 1e-8, 0, 0, 0]], device=DEV
            )
            sched = torch.tensor([1.0, 100.0, 1e6, 0.1], dtype=torch.float64, device=DEV)  # warmup_cosine
            derived = torch.zeros(2, 8, device=DEV)
            last_lr = torch.zeros(2, device=DEV)

            def base():
                if bf16:
                    ops.fused_adam_bf16(s['param'], s['grad'], s['master'], m, v, st, 1e-3, 0.9, 0.999, 1e-8, 0.0)
                else:
                    ops.fused_adam(s['param'], s['grad'], m, v, st, 1e-3, 0.9, 0.999, 1e-8, 0.0)

            def grouped():
                ops.fused_adamw_grouped(
                    s['param'], s['grad'], m, v, st, group_map, hyper, sched, derived, last_lr, master=s.get('master')
                )

            for r in range(rounds):
                for label, fn, nbytes in (
                    ('fused_adam' + ('_bf16' if bf16 else ''), base, 28.0),
                    ('fused_adamw_grouped' + ('_bf16' if bf16 else ''), grouped, 28.125),
                ):
                    us = time_fn(fn, reps=reps)
                    tbs = n * nbytes / (us / 1e6) / 1e12
                    print(f'  n={n:>10} {name} round {r + 1} {label:>26}: {us:8.1f} us  {tbs:6.3f} TB/s')


def bench_clip():
    print('== clip_grad_norm_ (norm + scale) ==')
    for n in [1 << 22, 1 << 26]:
        g = torch.randn(n, device=DEV)
        us = time_fn(lambda: ops.clip_grad_norm_(g, 1e9))
        gbs = n * 4 * 3 / (us / 1e6) / 1e9  # 2 reads + 1 write
        print(f'  n={n:>10}: {us:8.1f} us  ({gbs:7.1f} GB/s of 3x traffic)')


def bench_layernorm(shapes=((65536, 768),), rounds=1, reps=200):
    """layernorm_fwd / layernorm_bwd at the GPT-2 shape (B*T = 65,536 rows
    of 768). Forward moves 4 B per element (x read, y written), backward
    6 B (dy and x read, dx written)."""
    from dmlcloud_amd import _C

    print('== layernorm fwd / bwd: us, TB/s of 4 / 6 B per element ==')
    for R, D in shapes:
        x = torch.randn(R, D, device=DEV).to(torch.bfloat16)
        dy = torch.randn(R, D, device=DEV).to(torch.bfloat16)
        gamma = torch.randn(D, device=DEV).to(torch.bfloat16)
        beta = torch.randn(D, device=DEV).to(torch.bfloat16)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean = torch.empty(R, dtype=torch.float32, device=DEV)
        rstd = torch.empty(R, dtype=torch.float32, device=DEV)
        ws = torch.empty(256 * 2 * D, dtype=torch.float32, device=DEV)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        for r in range(rounds):
            for label, fn, nbytes in (
                ('layernorm_fwd', lambda: _C.layernorm_fwd(x, gamma, beta, y, mean, rstd, 1e-5), 4.0),
                ('layernorm_bwd', lambda: _C.layernorm_bwd(dy, x, mean, rstd, gamma, dx, ws, dgamma, dbeta), 6.0),
            ):
                us = time_fn(fn, reps=reps)
                tbs = R * D * nbytes / (us / 1e6) / 1e12
                print(f'  ({R}, {D}) round {r + 1} {label:>14}: {us:8.1f} us  {tbs:6.3f} TB/s')


if __name__ == '__main__':
    if '--layernorm-gpt2' in sys.argv[1:]:
        bench_layernorm(rounds=3)
        sys.exit(0)
    if '--adamw-gpt2' in sys.argv[1:]:
        # the optimizer comparison alone, at the GPT-2 flat size: three
        # alternating rounds, ~0.2 s of kernel time per figure
        bench_adamw(sizes=(GPT2_FLAT,), rounds=3, reps=300)
        sys.exit(0)
    bench_copy()
    bench_reduce()
    bench_adam()
    bench_adamw()
    bench_clip()
    bench_layernorm()
