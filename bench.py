"""Flagship benchmark: MNIST-CNN Stage samples/sec on MI355X.

Measures the BASELINE.json headline metric — samples/sec (whole node) of
the MNIST-CNN training Stage. The secondary configs (ResNet-50 bf16,
GPT-2 small) are separate invocations selected with --model; one run
measures one config. Synthetic data (no network access), random-init
weights.

Launch (driver contract):
    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

The timed region is exactly K full training steps (zero_grad, forward,
loss, backward, gradient sync, optimizer step, metric tracking),
bracketed by barrier + torch.cuda.synchronize on both sides; the
reported time is the MAX over ranks.

Fast path (default, --impl flat): the model is a FlatReplica (one flat
fp32 parameter/grad buffer), the optimizer a fused gfx950 Adam kernel,
gradient sync a single RCCL all-reduce, and the whole step is captured
into a hipGraph and replayed — per-step host work is one small D2D batch
copy plus one graph launch. --impl ddp runs the torch-DDP eager path for
comparison.

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, print the result line. --dump-outputs DIR additionally
writes what the last timed step computed (loss.npy, params.npy,
grads.npy; float32) so two builds can be compared output for output —
model init and the synthetic batches are seeded, so the inputs are
identical from run to run. --full is reserved for measurements beyond the
headline figure.
"""

import argparse
import json
import os
import sys
import time

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')  # dmabuf IPC for RCCL

import torch
import torch.distributed as dist

from dmlcloud_amd import TrainingPipeline, TrainValStage
from dmlcloud_amd.metrics import Reduction
from dmlcloud_amd.models import gpt2_small, gpt2_tiny, mnist_cnn, resnet50
from dmlcloud_amd.parallel import (
    FlatAdam,
    FlatSGD,
    GraphedStep,
    init_process_group_auto,
    local_rank,
)


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--steps', type=int, default=200)
    p.add_argument('--warmup', type=int, default=30)
    p.add_argument('--model', choices=['mnist', 'resnet50', 'gpt2'], default='mnist')
    p.add_argument('--impl', choices=['flat', 'ddp'], default='flat')
    p.add_argument('--batch-size', type=int, default=None, help='per-GPU batch size')
    p.add_argument('--no-graph', action='store_true', help='disable hipGraph capture')
    p.add_argument('--no-fused', action='store_true', help='disable the fused smallcnn kernels (MIOpen path)')
    p.add_argument('--tunableop', action='store_true', help='enable PyTorch TunableOp GEMM tuning (hipBLASLt)')
    p.add_argument('--no-channels-last', action='store_true', help='disable NHWC memory format (resnet50)')
    p.add_argument('--seq-len', type=int, default=1024, help='gpt2 sequence length')
    p.add_argument(
        '--ckpt-layers',
        default='',
        help='comma-separated resnet50 stages (e.g. layer1,layer2) to run with '
        'activation recompute — required to fit the bs=8192 reducer-stress '
        'config in 288 GB HBM (activations alone are ~277 GB without it)',
    )
    p.add_argument(
        '--metric-stress',
        type=int,
        default=0,
        metavar='N',
        help='track N distributed reduced metrics per step (BASELINE config #5: '
        'ResNet-50 bs=8192 reducer stress — combine with --model resnet50 --batch-size 8192)',
    )
    p.add_argument(
        '--dump-outputs',
        default=None,
        metavar='DIR',
        help='after the timed steps, write what the last timed step computed (loss, updated '
        'parameters, gradients) to DIR/<name>.npy as float32',
    )
    p.add_argument(
        '--full',
        action='store_true',
        help='also run the measurements beyond the headline figure; a plain run only sets up, '
        'warms up, times the steps and prints the result line (there are none at present: '
        'secondary configs are separate runs selected with --model/--impl)',
    )
    return p.parse_args()


# --dump-outputs budget: 64 MB in all -> two sampled fp32 arrays of <= 24 MB each
DUMP_MAX_ELEMS = 6_000_000


def dump_outputs(out_dir, stage):
    """Write the results of the last timed step as float32 .npy files:
    its loss, and the parameters and gradients it left behind (in
    registration order, flattened and concatenated). Arrays above
    DUMP_MAX_ELEMS are reduced to a fixed seeded sample of their elements,
    so two runs with the same arguments dump the same positions."""
    import numpy as np

    def flat32(tensors):
        return torch.cat([t.detach().reshape(-1).to(torch.float32) for t in tensors]).cpu().numpy()

    def sample(a):
        if a.size <= DUMP_MAX_ELEMS:
            return a
        idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_MAX_ELEMS, replace=False))
        return a[idx]

    params = list(stage.pipeline.models['net'].parameters())
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, 'loss.npy'), flat32([stage.last_loss]))
    np.save(os.path.join(out_dir, 'params.npy'), sample(flat32(params)))
    np.save(os.path.join(out_dir, 'grads.npy'), sample(flat32([p.grad for p in params if p.grad is not None])))


class BenchStage(TrainValStage):
    """TrainValStage driven step-by-step by the benchmark loop."""

    def __init__(self, args, device):
        super().__init__()
        self.args = args
        self.bench_device = device
        self.metric_prefix = self.train_metric_prefix()
        self.loss_fn = torch.nn.CrossEntropyLoss()
        self.static_batch = None

    # -- model-specific setup -------------------------------------------------

    def pre_stage(self):
        args = self.args
        device = self.bench_device
        torch.manual_seed(1234)

        if args.model == 'mnist':
            if device.type == 'cuda' and not args.no_fused:
                from dmlcloud_amd.ops.fused_cnn import FusedMnistCNN

                model = FusedMnistCNN()  # fused gfx950 conv+relu+pool kernels
            else:
                model = mnist_cnn()
            self.batch_shape = (args.batch_size, 1, 28, 28)
            self.dtype = 'fp32'
        elif args.model == 'resnet50':
            model = resnet50()
            args.channels_last = not args.no_channels_last and device.type == 'cuda'
            if args.channels_last:
                model = model.to(memory_format=torch.channels_last)
                # benchmark mode = exhaustive MIOpen find per conv shape:
                # worth minutes of startup at b<=512, but at the b8192
                # stress config the search itself takes >10 min — use
                # MIOpen immediate mode there instead
                torch.backends.cudnn.benchmark = args.batch_size < 2048
            if args.ckpt_layers:
                from torch.utils.checkpoint import checkpoint

                def _recompute(stage_forward):
                    return lambda x: checkpoint(stage_forward, x, use_reentrant=False)

                for stage_name in args.ckpt_layers.split(','):
                    stage = getattr(model, stage_name)
                    stage.forward = _recompute(stage.forward)
            self.batch_shape = (args.batch_size, 3, 224, 224)
            self.dtype = 'bf16'
        else:  # gpt2
            model = gpt2_small() if device.type == 'cuda' else gpt2_tiny()
            self.batch_shape = (args.batch_size, args.seq_len)
            self.dtype = 'bf16'

        # GPT-2 runs as true mixed precision: bf16 flat params/grads, fp32
        # master in the fused optimizer — no autocast casting per layer
        # (+16% tokens/s vs autocast). ResNet-50 keeps fp32 params +
        # autocast: MIOpen's pure-bf16 convs/BN measured ~2x slower than
        # the autocast mix (gpurun_out/bench_resnet50_bf16.json).
        self.flat_bf16 = (
            args.impl == 'flat' and args.model == 'gpt2' and self.dtype == 'bf16' and device.type == 'cuda'
        )
        if args.impl == 'flat':
            flat_dtype = torch.bfloat16 if self.flat_bf16 else torch.float32
            self.pipeline.register_model('net', model, ddp_impl='flat', flat_dtype=flat_dtype, verbose=False)
            replica = self.pipeline.models['net']
            if args.model == 'resnet50':
                self.pipeline.register_optimizer('opt', FlatSGD(replica, lr=1e-3, momentum=0.9))
            else:
                self.pipeline.register_optimizer('opt', FlatAdam(replica, lr=1e-3))
        else:
            use_ddp = dist.is_initialized() and dist.get_world_size() > 1
            self.pipeline.register_model('net', model, use_ddp=use_ddp, verbose=False)
            wrapped = self.pipeline.models['net']
            self.pipeline.register_optimizer('opt', torch.optim.Adam(wrapped.parameters(), lr=1e-3))

        # synthetic data, resident on device: a pool of distinct batches.
        # Huge-batch configs (the bs=8192 reducer stress) need nearly all
        # of the 288 GB HBM for activations: shrink the pool and feed the
        # conv stack bf16 inputs directly (autocast's first op casts to
        # bf16 anyway, so the compute path is identical).
        g = torch.Generator(device='cpu').manual_seed(4242)
        self.big_batch = args.model == 'resnet50' and args.batch_size >= 2048
        batch_bytes = 2 if self.big_batch else 4
        for d in self.batch_shape:
            batch_bytes *= d
        pool_cap = (4 << 30) if batch_bytes > (1 << 30) else (16 << 30)
        self.n_pool = max(2, min(16, pool_cap // batch_bytes))
        if args.model == 'gpt2':
            vocab = self.pipeline.models['net'].module.cfg.vocab_size if hasattr(
                self.pipeline.models['net'], 'module'
            ) else model.cfg.vocab_size
            self.pool = [
                torch.randint(0, vocab, self.batch_shape, generator=g).to(device) for _ in range(self.n_pool)
            ]
            self.labels = None
            self.static_batch = torch.zeros_like(self.pool[0])
        else:
            mf = torch.channels_last if (args.model == 'resnet50' and args.channels_last) else torch.contiguous_format
            in_dtype = (
                torch.bfloat16
                if (args.model == 'resnet50' and (self.flat_bf16 or self.big_batch))
                else torch.float32
            )
            self.pool = [
                torch.randn(self.batch_shape, generator=g).to(device, in_dtype).to(memory_format=mf)
                for _ in range(self.n_pool)
            ]
            self.labels = [
                torch.randint(0, 10 if args.model == 'mnist' else 1000, (args.batch_size,), generator=g).to(device)
                for _ in range(self.n_pool)
            ]
            self.static_batch = torch.zeros_like(self.pool[0])
            self.static_labels = torch.zeros_like(self.labels[0])

    # -- the training step ----------------------------------------------------

    def step(self, batch):
        model = self.pipeline.models['net']
        autocast_on = (
            self.dtype == 'bf16' and self.bench_device.type == 'cuda' and not self.flat_bf16
        )  # bf16 flat replicas compute natively in bf16 — no autocast needed
        if self.args.model == 'gpt2':
            idx = batch
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast_on):
                _, loss = model(idx, targets=idx)
            return loss
        x, y = batch
        if self.args.model == 'resnet50':
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast_on):
                out = model(x)
                loss = self.loss_fn(out, y)
            return loss
        out = model(x)  # mnist: fp32, matching the reference's precision
        return self.loss_fn(out, y)

    def core_step(self):
        """The graph-capturable part of train_batch: full compute + loss
        metric accumulation on static buffers."""
        self.zero_grad()
        if self.args.model == 'gpt2':
            loss = self.train_step(self.static_batch)
        else:
            loss = self.train_step((self.static_batch, self.static_labels))
        self.optimize(loss)
        # kept for --dump-outputs; under graph replay this static tensor
        # holds the loss of the latest replayed step
        self.last_loss = loss.detach()
        self.track_reduce(self.loss_metric_name(), loss)
        if self.args.metric_stress:
            # BASELINE config #5: N device-resident reducer accumulations
            # per step (one metric_reduce_into kernel chain each; the
            # epoch-end RCCL collectives fuse into one per reduction op)
            rotations = (Reduction.MEAN, Reduction.SUM, Reduction.MIN, Reduction.MAX)
            for k in range(self.args.metric_stress):
                self.track_reduce(f'stress_{k}', loss, reduction=rotations[k % 4], prefixed=False)

    def load_batch(self, i):
        """Stage pool batch i into the static buffers (device-side copy)."""
        j = i % self.n_pool
        self.static_batch.copy_(self.pool[j], non_blocking=True)
        if self.labels is not None:
            self.static_labels.copy_(self.labels[j], non_blocking=True)


def main():
    args = parse_args()

    if args.tunableop:
        # hipBLASLt/rocBLAS algorithm search for this config's GEMM shapes;
        # tuning happens during warmup, results cached per rank
        os.environ.setdefault('PYTORCH_TUNABLEOP_ENABLED', '1')
        os.environ.setdefault('PYTORCH_TUNABLEOP_TUNING', '1')
        os.environ.setdefault('PYTORCH_TUNABLEOP_FILENAME', f'gpurun_out/tunableop_{os.environ.get("RANK", 0)}.csv')
    else:
        # pre-tuned GEMM algorithm selections shipped per model config
        # (profiles/tunableop_<model>_gfx950.csv, produced once with
        # --tunableop and committed): load read-only — no tuning cost,
        # every box starts with the searched hipBLASLt algorithms
        pretuned = os.path.join(
            os.path.dirname(os.path.abspath(__file__)), 'profiles', f'tunableop_{args.model}_gfx950.csv'
        )
        if torch.cuda.is_available() and os.path.exists(pretuned):
            torch.cuda.tunable.enable(True)
            torch.cuda.tunable.tuning_enable(False)
            torch.cuda.tunable.read_file(pretuned)

    if 'MASTER_ADDR' not in os.environ and args.gpus == 1:
        pass  # dummy single-process group below
    init_process_group_auto()
    world = dist.get_world_size()
    rank = dist.get_rank()

    if torch.cuda.is_available():
        lr = local_rank() if local_rank() is not None else 0
        device = torch.device('cuda', lr)
        torch.cuda.set_device(device)
    else:
        device = torch.device('cpu')

    if world > 1 and device.type == 'cuda':
        # establish the RCCL communicator before any timed/captured work
        dist.all_reduce(torch.zeros(1, device=device))
        torch.cuda.synchronize()

    if args.batch_size is None:
        args.batch_size = {'mnist': 16384, 'resnet50': 512, 'gpt2': 64}[args.model]

    # Stage + pipeline machinery (the metric path under test runs per step)
    pipeline = TrainingPipeline(name='bench')
    stage = BenchStage(args, device)
    pipeline.append_stage(stage, max_epochs=1)
    pipeline.device = device
    stage.pre_stage()

    use_graph = (not args.no_graph) and args.impl == 'flat' and device.type == 'cuda'

    if use_graph:
        stage.load_batch(0)
        # validate=True: a capture that replays incorrectly (e.g. an RCCL
        # collective that cannot replay at this world size) falls back to
        # eager — measured, not assumed (the JSON reports hipgraph: false)
        graphed = GraphedStep(stage.core_step, warmup=3, validate=True)
        graphed.initialize()

        def run_step(i):
            stage.load_batch(i)
            graphed()

    else:

        def run_step(i):
            stage.load_batch(i)
            stage.core_step()

    # ---- warmup ----
    for i in range(args.warmup):
        run_step(i)

    if device.type == 'cuda':
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    if device.type == 'cuda':
        torch.cuda.synchronize()

    # ---- timed region: exactly K steps ----
    t0 = time.perf_counter()
    for i in range(args.steps):
        run_step(args.warmup + i)
    if device.type == 'cuda':
        torch.cuda.synchronize()
    t1 = time.perf_counter()
    elapsed = t1 - t0

    if world > 1:
        et = torch.tensor([elapsed], dtype=torch.float64, device=device if device.type == 'cuda' else 'cpu')
        dist.all_reduce(et, op=dist.ReduceOp.MAX)
        elapsed = et.item()
        dist.barrier()
    if device.type == 'cuda':
        torch.cuda.synchronize()

    samples = args.steps * args.batch_size * world
    samples_per_sec = samples / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    if args.model == 'gpt2':
        metric, value = 'tokens/s', samples_per_sec * args.seq_len
    else:
        metric, value = 'samples/s', samples_per_sec

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, stage)

    if rank == 0:
        result = {
            'metric': metric,
            'value': value,
            'unit': metric,
            'n_gpus': world,
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': ms_per_step,
            'higher_is_better': True,
            'scaling': 'weak',
            'vs_baseline': None,  # reference publishes no numbers
            'dtype': stage.dtype,
            'data': 'synthetic',
            'config': {
                'model': {'mnist': 'mnist-cnn', 'resnet50': 'resnet-50', 'gpt2': 'gpt2-small'}[args.model],
                'global_batch': args.batch_size * world,
                'per_gpu_batch': args.batch_size,
                'parallelism': f'dp{world}',
                'impl': args.impl,
                'hipgraph': bool(use_graph and getattr(graphed, 'captured', False)) if use_graph else False,
                **({'seq_len': args.seq_len} if args.model == 'gpt2' else {}),
                **({'metric_stress': args.metric_stress} if args.metric_stress else {}),
                **({'ckpt_layers': args.ckpt_layers} if args.ckpt_layers else {}),
            },
        }
        print(json.dumps(result))

    dist.destroy_process_group()


if __name__ == '__main__':
    sys.exit(main() or 0)
