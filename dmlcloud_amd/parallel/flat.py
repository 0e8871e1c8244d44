"""Flat-buffer data parallelism: the MI355X-native DDP fast path.

torch DDP buckets gradients into ~25 MB chunks sized for NVSwitch-era
overlap. On a single 8xMI355X node the xGMI fabric is 7 point-to-point
links per GPU and models that fit comfortably in 288 GB HBM3E per GPU can
afford a flatter layout:

- ALL trainable parameters live in ONE contiguous fp32 HBM buffer
  (parameters are views into it) and all gradients accumulate into a
  second contiguous buffer (``p.grad`` pre-assigned as views, so autograd
  writes gradients in place - no bucket copy pass).
- Gradient sync is a single RCCL all-reduce of the flat gradient buffer
  (optionally chunked for overlap); the 1/world averaging folds into the
  fused optimizer kernel (ops/csrc/optim.hip) for free.
- Everything (zero_grad memset, backward, all-reduce, fused optimizer,
  metric accumulation) is a fixed kernel sequence on fixed pointers, so
  the entire training step can be captured into a hipGraph
  (parallel/graphs.py) and replayed with one launch.

This replaces the reference's DDP construction for the hot benchmarks
(reference dmlcloud/pipeline.py:72-74); `register_model(..., use_ddp=True)`
still offers torch-DDP semantics for arbitrary models.
"""

import math
from contextlib import contextmanager
from typing import List, Optional

import torch
import torch.distributed as dist

from .. import ops


def _flatten_params(params: List[torch.nn.Parameter], dtype=torch.float32, device=None):
    """Move `params` into one flat buffer of `dtype`; returns
    (flat, grads_flat, master) where master is the fp32 copy (None when
    dtype is already fp32)."""
    assert params, 'no trainable parameters'
    device = device or params[0].device
    numels = [p.numel() for p in params]
    # 8-element (16 B for bf16) alignment so every view is vector-load friendly
    offsets = []
    off = 0
    for n in numels:
        offsets.append(off)
        off += (n + 7) // 8 * 8
    total = off

    flat = torch.zeros(total, dtype=dtype, device=device)
    grad_flat = torch.zeros(total, dtype=dtype, device=device)
    master = torch.zeros(total, dtype=torch.float32, device=device) if dtype != torch.float32 else None

    for p, o, n in zip(params, offsets, numels):
        fp32 = p.data.reshape(-1).to(device=device, dtype=torch.float32)
        if master is not None:
            master[o : o + n].copy_(fp32)
        flat[o : o + n].copy_(fp32.to(dtype))
        p.data = flat[o : o + n].view(p.shape)
        p.grad = grad_flat[o : o + n].view(p.shape)
    return flat, grad_flat, master, offsets


class FlatReplica:
    """Replicated data-parallel model over one flat parameter buffer.

    Usage:
        replica = FlatReplica(model)           # after model.to(device)
        ...
        replica.zero_grad()
        loss.backward()
        replica.grad_sync()                    # ONE RCCL all-reduce
        optimizer.step()                       # FlatAdam/FlatSGD
    """

    def __init__(
        self,
        module: torch.nn.Module,
        process_group=None,
        broadcast: bool = True,
        dtype: torch.dtype = torch.float32,
        overlap_buckets_mb: Optional[int] = None,
    ):
        """dtype=torch.bfloat16 enables true mixed precision: the model
        computes in bf16 (no per-layer autocast casts), gradients
        all-reduce in bf16 (half the xGMI bytes), and the fused optimizer
        holds the fp32 master (replica.flat_master).

        overlap_buckets_mb: when set, gradients all-reduce bucket-by-bucket
        DURING backward (post-accumulate-grad hooks fire async collectives
        in backward-completion order over contiguous flat segments) and
        grad_sync() just waits — overlapping communication with the rest
        of backward like DDP does, but over the flat buffer. Leave None
        for the single-collective mode, which is the one to use with
        GraphedStep: hook-driven async collectives rely on host-side
        bookkeeping that a replayed hipGraph would not re-execute."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError('FlatReplica supports fp32 or bf16 parameter buffers')
        self.module = module
        self.dtype = dtype
        self.process_group = process_group
        self.params = [p for p in module.parameters() if p.requires_grad]
        for p in self.params:
            if p.dtype != torch.float32:
                raise ValueError('FlatReplica expects fp32 module parameters at construction')
        self.flat_param, self.flat_grad, self.flat_master, self._offsets = _flatten_params(
            self.params, dtype=dtype
        )
        self.world_size = dist.get_world_size(process_group) if dist.is_initialized() else 1

        self._buckets = None
        self._pending_works = []
        self._sync_enabled = True
        if overlap_buckets_mb:
            self._setup_overlap(overlap_buckets_mb)
        if broadcast and dist.is_initialized() and self.world_size > 1:
            if self.flat_master is not None:
                # the fp32 master is authoritative; params re-derive from it
                dist.broadcast(self.flat_master, src=0, group=process_group)
                self.flat_param.copy_(self.flat_master.to(dtype))
            else:
                dist.broadcast(self.flat_param, src=0, group=process_group)
            # buffers (e.g. BN running stats) follow rank 0 once at init
            for buf in module.buffers():
                dist.broadcast(buf, src=0, group=process_group)

    def __call__(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    def _setup_overlap(self, bucket_mb: int):
        """Partition the flat buffer into contiguous buckets ordered by
        backward completion (params in reverse registration order) and
        hook each param's gradient accumulation."""
        bucket_bytes = bucket_mb << 20
        elsize = self.flat_grad.element_size()
        buckets = []  # list of dicts: {start, end, params:set, done:set}
        current = {'params': [], 'bytes': 0}
        # reverse order: the last registered params finish backward first
        for i in reversed(range(len(self.params))):
            current['params'].append(i)
            current['bytes'] += self.params[i].numel() * elsize
            if current['bytes'] >= bucket_bytes:
                buckets.append(current['params'])
                current = {'params': [], 'bytes': 0}
        if current['params']:
            buckets.append(current['params'])

        self._buckets = []
        self._param_bucket = {}
        for param_ids in buckets:
            start = min(self._offsets[i] for i in param_ids)
            end = max(
                self._offsets[i] + self.params[i].numel() for i in param_ids
            )
            bucket = {'segment': self.flat_grad[start:end], 'params': set(param_ids), 'done': set()}
            self._buckets.append(bucket)
            for i in param_ids:
                self._param_bucket[i] = bucket

        for i, p in enumerate(self.params):
            p.register_post_accumulate_grad_hook(self._make_hook(i))

    @contextmanager
    def no_sync(self):
        """Suspend overlap-mode bucket collectives during gradient
        accumulation (torch DDP ``no_sync`` analog).

        In overlap mode every backward fires async all-reduces from the
        post-accumulate-grad hooks; two backwards before one step would
        re-reduce already rank-summed buckets. Wrap all but the LAST
        micro-batch backward in ``no_sync()`` — local gradients keep
        accumulating into the flat buffer, and the final (unwrapped)
        backward all-reduces the accumulated sums once. Single-collective
        mode needs no guard (sync happens only in grad_sync())."""
        prev = self._sync_enabled
        self._sync_enabled = False
        try:
            yield
        finally:
            self._sync_enabled = prev

    def _make_hook(self, index: int):
        def hook(_param):
            if self.world_size <= 1 or not self._sync_enabled:
                return
            bucket = self._param_bucket[index]
            bucket['done'].add(index)
            if bucket['done'] == bucket['params']:
                bucket['done'] = set()
                work = dist.all_reduce(bucket['segment'], group=self.process_group, async_op=True)
                self._pending_works.append(work)

        return hook

    def zero_grad(self, set_to_none: bool = False):
        # one memset kernel; set_to_none is meaningless for a flat buffer
        self.flat_grad.zero_()

    def grad_sync(self):
        """Make gradients globally consistent. Single-collective mode:
        ONE all-reduce of the flat buffer. Overlap mode: wait on the
        bucket collectives that backward already launched."""
        if self.world_size <= 1:
            return
        if self._buckets is None:
            dist.all_reduce(self.flat_grad, group=self.process_group)
            return
        for work in self._pending_works:
            work.wait()
        self._pending_works.clear()
        for bucket in self._buckets:
            # a bucket whose params got no grads this step never fired
            if bucket['done']:
                bucket['done'] = set()
                dist.all_reduce(bucket['segment'], group=self.process_group)

    @property
    def grad_scale(self) -> float:
        return 1.0 / self.world_size

    def state_dict(self, *args, **kwargs):
        return self.module.state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        res = self.module.load_state_dict(*args, **kwargs)
        # load_state_dict writes THROUGH the views (copy_ semantics), so the
        # flat buffer stays authoritative. Refresh the fp32 master from the
        # loaded params (best available info; an optimizer load_state_dict
        # afterwards restores the exact master).
        if self.flat_master is not None:
            self.flat_master.copy_(self.flat_param.to(torch.float32))
        return res

    def parameters(self):
        return iter(self.params)


class FlatOptimizer(torch.optim.Optimizer):
    """Base for fused flat-buffer optimizers (single kernel per step).

    A real ``torch.optim.Optimizer`` subclass: ``param_groups[0]`` holds
    the live hyperparameters (the fused kernel reads ``lr`` from it each
    step), so torch LR schedulers work unmodified when the step runs
    eagerly — ``register_optimizer('opt', FlatAdam(replica), scheduler)``
    schedules exactly like the stock-optimizer path. The per-param
    ``self.state`` dict stays empty; optimizer state lives in the flat
    moment buffers.

    Caveat under hipGraph replay (``GraphedStep``): ``FlatAdam`` and
    ``FlatSGD`` pass ``lr`` and the other hyperparameters to their kernels
    as launch arguments, so a captured step keeps the values of the
    capture step for good and a scheduler's later changes to
    ``param_groups`` have no effect, without an error. ``FlatAdamW`` keeps
    them in device memory instead: its ``schedule`` follows the device
    step counter inside the graph, and host-side changes reach a captured
    step through ``sync_hyperparameters()`` between replays.
    """

    # one flat buffer = one param group, unless the subclass's kernel can
    # tell groups apart (FlatAdamW)
    _multi_group = False

    def __init__(self, replica: FlatReplica, defaults: dict, params=None):
        self.replica = replica
        super().__init__(replica.params if params is None else params, defaults)
        if not self._multi_group and len(self.param_groups) != 1:
            raise ValueError('FlatOptimizer drives ONE flat buffer = one param group')

    @property
    def lr(self) -> float:
        return self.param_groups[0]['lr']

    @lr.setter
    def lr(self, value: float):
        self.param_groups[0]['lr'] = value

    def zero_grad(self, set_to_none: bool = False):
        self.replica.zero_grad()

    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """Fused global-norm clip on the flat grads (no host sync).

        After grad_sync() the flat buffer holds the SUM over ranks; the
        averaging happens later inside the fused optimizer (grad_scale).
        Passing norm_scale = grad_scale here makes the clip act on the
        averaged-gradient norm, so the result matches torch DDP +
        clip_grad_norm_ at any world size (returned norm is the averaged
        norm too)."""
        return ops.clip_grad_norm_(
            self.replica.flat_grad, max_norm, norm_scale=self.replica.grad_scale
        )

    def state_dict(self):
        raise NotImplementedError

    def load_state_dict(self, state):
        raise NotImplementedError


class FlatAdam(FlatOptimizer):
    def __init__(self, replica: FlatReplica, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(replica, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        n = replica.flat_param.numel()
        dev = replica.flat_param.device
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)

    def step(self, closure=None):
        group = self.param_groups[0]
        beta1, beta2 = group['betas']
        if self.replica.dtype is torch.bfloat16:
            ops.fused_adam_bf16(
                self.replica.flat_param,
                self.replica.flat_grad,
                self.replica.flat_master,
                self.exp_avg,
                self.exp_avg_sq,
                self.step_t,
                group['lr'],
                beta1,
                beta2,
                group['eps'],
                group['weight_decay'],
                grad_scale=self.replica.grad_scale,
            )
        else:
            ops.fused_adam(
                self.replica.flat_param,
                self.replica.flat_grad,
                self.exp_avg,
                self.exp_avg_sq,
                self.step_t,
                group['lr'],
                beta1,
                beta2,
                group['eps'],
                group['weight_decay'],
                grad_scale=self.replica.grad_scale,
            )

    def state_dict(self):
        group = self.param_groups[0]
        return {
            'lr': group['lr'],
            'betas': group['betas'],
            'eps': group['eps'],
            'weight_decay': group['weight_decay'],
            'exp_avg': self.exp_avg,
            'exp_avg_sq': self.exp_avg_sq,
            'step': self.step_t,
            'master': self.replica.flat_master,
        }

    def load_state_dict(self, state):
        group = self.param_groups[0]
        group['lr'] = state['lr']
        group['betas'] = tuple(state['betas'])
        group['eps'] = state['eps']
        group['weight_decay'] = state['weight_decay']
        self.exp_avg.copy_(state['exp_avg'].to(self.exp_avg.device))
        self.exp_avg_sq.copy_(state['exp_avg_sq'].to(self.exp_avg_sq.device))
        self.step_t.copy_(state['step'].to(self.step_t.device))
        if state.get('master') is not None and self.replica.flat_master is not None:
            self.replica.flat_master.copy_(state['master'].to(self.replica.flat_master.device))


class FlatSGD(FlatOptimizer):
    def __init__(self, replica: FlatReplica, lr=1e-2, momentum=0.0, weight_decay=0.0):
        super().__init__(replica, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self.momentum_buf: Optional[torch.Tensor] = None
        if momentum != 0:
            # momentum accumulates in fp32 regardless of the param dtype
            self.momentum_buf = torch.zeros(
                replica.flat_param.numel(), dtype=torch.float32, device=replica.flat_param.device
            )

    def step(self, closure=None):
        group = self.param_groups[0]
        if self.replica.dtype is torch.bfloat16:
            ops.fused_sgd_bf16(
                self.replica.flat_param,
                self.replica.flat_grad,
                self.replica.flat_master,
                self.momentum_buf,
                group['lr'],
                group['momentum'],
                group['weight_decay'],
                grad_scale=self.replica.grad_scale,
            )
        else:
            ops.fused_sgd(
                self.replica.flat_param,
                self.replica.flat_grad,
                self.momentum_buf,
                group['lr'],
                group['momentum'],
                group['weight_decay'],
                grad_scale=self.replica.grad_scale,
            )

    def state_dict(self):
        group = self.param_groups[0]
        return {
            'lr': group['lr'],
            'momentum': group['momentum'],
            'weight_decay': group['weight_decay'],
            'momentum_buf': self.momentum_buf,
            'master': self.replica.flat_master,
        }

    def load_state_dict(self, state):
        group = self.param_groups[0]
        group['lr'] = state['lr']
        group['momentum'] = state['momentum']
        group['weight_decay'] = state['weight_decay']
        if state['momentum_buf'] is not None:
            if self.momentum_buf is None:
                self.momentum_buf = torch.zeros(
                    self.replica.flat_param.numel(),
                    dtype=torch.float32,
                    device=self.replica.flat_param.device,
                )
            self.momentum_buf.copy_(state['momentum_buf'].to(self.momentum_buf.device))
        if state.get('master') is not None and self.replica.flat_master is not None:
            self.replica.flat_master.copy_(state['master'].to(self.replica.flat_master.device))


class LRSchedule:
    """Learning-rate multiplier as a function of the optimizer step, small
    enough to live on the device: ``FlatAdamW`` evaluates it from its
    device step counter, so a captured step follows it under replay with no
    host involvement. ``multiplier()`` is the host mirror of that
    computation.

    For step ``s`` (1-based: the first ``step()`` is 1), warmup ``W``,
    total ``T`` and minimum ratio ``r`` the multiplier is ``s / W`` for
    ``s <= W`` (when ``W > 0``), ``r`` for ``s >= T``, and in between
    ``r + (1 - r) * 0.5 * (1 + cos(pi * (s - W) / (T - W)))`` (cosine) or
    the straight line from 1 to ``r`` (linear).
    """

    KINDS = ('constant', 'warmup_cosine', 'warmup_linear')  # index = device kind code

    def __init__(self, kind: str = 'constant', warmup: int = 0, total: int = 0, min_ratio: float = 0.0):
        if kind not in self.KINDS:
            raise ValueError(f'unknown schedule kind {kind!r}; expected one of {self.KINDS}')
        warmup, total, min_ratio = int(warmup), int(total), float(min_ratio)
        if kind != 'constant':
            if warmup < 0 or total <= warmup:
                raise ValueError('LRSchedule needs 0 <= warmup < total')
            if not 0.0 <= min_ratio <= 1.0:
                raise ValueError('LRSchedule needs 0 <= min_ratio <= 1')
        self.kind = kind
        self.warmup = warmup
        self.total = total
        self.min_ratio = min_ratio

    @classmethod
    def constant(cls) -> 'LRSchedule':
        return cls('constant')

    @classmethod
    def warmup_cosine(cls, warmup: int, total: int, min_ratio: float = 0.0) -> 'LRSchedule':
        return cls('warmup_cosine', warmup, total, min_ratio)

    @classmethod
    def warmup_linear(cls, warmup: int, total: int, min_ratio: float = 0.0) -> 'LRSchedule':
        return cls('warmup_linear', warmup, total, min_ratio)

    def multiplier(self, step: int) -> float:
        if self.kind == 'constant':
            return 1.0
        s, w, t, r = float(step), float(self.warmup), float(self.total), self.min_ratio
        if w > 0 and s <= w:
            return s / w
        if s >= t:
            return r
        progress = (s - w) / (t - w)
        shape = 0.5 * (1.0 + math.cos(math.pi * progress)) if self.kind == 'warmup_cosine' else 1.0 - progress
        return r + (1.0 - r) * shape

    def record(self) -> List[float]:
        """The fp64[4] device record {kind, warmup, total, min_ratio}."""
        return [float(self.KINDS.index(self.kind)), float(self.warmup), float(self.total), self.min_ratio]

    def state_dict(self) -> dict:
        return {'kind': self.kind, 'warmup': self.warmup, 'total': self.total, 'min_ratio': self.min_ratio}

    @classmethod
    def from_state_dict(cls, state: dict) -> 'LRSchedule':
        return cls(state['kind'], state['warmup'], state['total'], state['min_ratio'])

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self.state_dict() == other.state_dict()

    def __repr__(self):
        if self.kind == 'constant':
            return 'LRSchedule.constant()'
        return f'LRSchedule.{self.kind}({self.warmup}, {self.total}, min_ratio={self.min_ratio})'


def weight_decay_groups(module: torch.nn.Module, weight_decay: float, no_decay=None) -> List[dict]:
    """The usual two parameter groups for ``FlatAdamW``: ``[decayed,
    undecayed]``. By default parameters with ``dim() >= 2`` (matrices,
    embedding tables) decay and the rest (biases, norm gains) do not, as
    GPT-2 recipes do. ``no_decay(name, param) -> bool`` replaces that rule.
    Tied weights appear once; frozen parameters are left out, as in
    ``FlatReplica``."""
    decay, rest = [], []
    for name, p in module.named_parameters():  # removes duplicates (tied weights)
        if not p.requires_grad:
            continue
        skip = no_decay(name, p) if no_decay is not None else p.dim() < 2
        (rest if skip else decay).append(p)
    return [{'params': decay, 'weight_decay': weight_decay}, {'params': rest, 'weight_decay': 0.0}]


class FlatAdamW(FlatOptimizer):
    """Fused AdamW on the flat buffer: decoupled weight decay, parameter
    groups and a device-resident learning rate.

    ``params=None`` puts every parameter of the replica in one group;
    otherwise it is a torch-style list of group dicts (at most 16) that
    together hold every replica parameter exactly once, each with optional
    overrides of ``lr``, ``betas``, ``eps`` and ``weight_decay``
    (``weight_decay_groups`` builds the usual decay / no-decay split). One
    kernel still updates the whole buffer: a byte per 8-element chunk tells
    it the chunk's group.

    Hyperparameters: ``param_groups[g]`` is the live host copy, so torch LR
    schedulers and user code change it as usual. The kernels read a device
    table instead; ``sync_hyperparameters()`` uploads the host values, and
    an eager ``step()`` calls it by itself whenever they changed. While a
    hipGraph is being captured ``step()`` uploads nothing, and a replay
    runs no host code at all: under ``GraphedStep``, call
    ``sync_hyperparameters()`` between replays after changing a group.

    ``schedule`` (an ``LRSchedule``, one per optimizer) multiplies every
    group's ``lr``. It is evaluated on the device from the device step
    counter, so a captured step follows warmup and decay under replay with
    no host involvement. ``last_lr`` is a device fp32[G] tensor with the
    rate each group used in the latest step; reading it needs no sync, and
    it can go straight into ``track_reduce``.
    """

    _multi_group = True
    MAX_GROUPS = 16

    def __init__(
        self,
        replica: FlatReplica,
        params=None,
        lr=1e-3,
        betas=(0.9, 0.999),
        eps=1e-8,
        weight_decay=1e-2,
        schedule: Optional[LRSchedule] = None,
    ):
        if params is not None:
            params = self._check_groups(replica, params)
        super().__init__(replica, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), params)
        self.schedule = schedule if schedule is not None else LRSchedule.constant()

        n = replica.flat_param.numel()
        dev = replica.flat_param.device
        ngroups = len(self.param_groups)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)
        self.last_lr = torch.zeros(ngroups, dtype=torch.float32, device=dev)
        self._hyper = torch.zeros(ngroups, 8, dtype=torch.float32, device=dev)
        self._derived = torch.zeros(ngroups, 8, dtype=torch.float32, device=dev)
        self._sched = torch.tensor(self.schedule.record(), dtype=torch.float64, device=dev)
        self.group_map = self._build_group_map().to(dev)
        self._uploaded = None
        self.sync_hyperparameters()

    @classmethod
    def _check_groups(cls, replica: FlatReplica, params) -> List[dict]:
        params = list(params)
        if not params or not all(isinstance(g, dict) and 'params' in g for g in params):
            raise ValueError("FlatAdamW: params must be a list of group dicts with a 'params' entry")
        groups = [dict(g) for g in params]
        if len(groups) > cls.MAX_GROUPS:
            raise ValueError(f'FlatAdamW supports at most {cls.MAX_GROUPS} parameter groups, got {len(groups)}')
        own = {id(p) for p in replica.params}
        seen = set()
        for g in groups:
            g['params'] = list(g['params'])
            for p in g['params']:
                if id(p) not in own:
                    raise ValueError('FlatAdamW: a group holds a parameter that is not in the replica')
                if id(p) in seen:
                    raise ValueError('FlatAdamW: a parameter appears in more than one group')
                seen.add(id(p))
        if len(seen) != len(own):
            raise ValueError(f'FlatAdamW: {len(own) - len(seen)} replica parameter(s) are in no group')
        return groups

    def _build_group_map(self) -> torch.Tensor:
        """uint8[n / 8]: the group of each 8-element chunk. _flatten_params
        aligns every parameter to 8 elements, so no chunk holds two."""
        replica = self.replica
        offset = {id(p): o for p, o in zip(replica.params, replica._offsets)}
        group_map = torch.zeros(replica.flat_param.numel() // 8, dtype=torch.uint8)
        for g, group in enumerate(self.param_groups):
            for p in group['params']:
                o = offset[id(p)]
                group_map[o // 8 : (o + p.numel() + 7) // 8] = g
        assert group_map.numel() == 0 or int(group_map.max()) < len(self.param_groups)
        return group_map

    def _host_hyperparameters(self) -> List[List[float]]:
        rows = []
        for group in self.param_groups:
            beta1, beta2 = group['betas']
            rows.append(
                [float(group['lr']), float(group['weight_decay']), float(beta1), float(beta2), float(group['eps'])]
                + [0.0, 0.0, 0.0]
            )
        return rows

    def sync_hyperparameters(self):
        """Copy the host hyperparameters (``param_groups``) into the device
        table the kernels read. Not capturable; under ``GraphedStep`` call
        it between replays."""
        rows = self._host_hyperparameters()
        for row in rows:
            if not (0.0 <= row[2] < 1.0 and 0.0 <= row[3] < 1.0):
                raise ValueError(f'FlatAdamW: betas must lie in [0, 1), got {(row[2], row[3])}')
        self._hyper.copy_(torch.tensor(rows, dtype=torch.float32))
        self._uploaded = rows

    def _capturing(self) -> bool:
        return self._hyper.is_cuda and torch.cuda.is_current_stream_capturing()

    def step(self, closure=None):
        if not self._capturing() and self._host_hyperparameters() != self._uploaded:
            self.sync_hyperparameters()
        ops.fused_adamw_grouped(
            self.replica.flat_param,
            self.replica.flat_grad,
            self.exp_avg,
            self.exp_avg_sq,
            self.step_t,
            self.group_map,
            self._hyper,
            self._sched,
            self._derived,
            self.last_lr,
            grad_scale=self.replica.grad_scale,
            master=self.replica.flat_master,
        )

    def state_dict(self):
        return {
            'groups': [
                {k: group[k] for k in ('lr', 'betas', 'eps', 'weight_decay')} for group in self.param_groups
            ],
            'schedule': self.schedule.state_dict(),
            'exp_avg': self.exp_avg,
            'exp_avg_sq': self.exp_avg_sq,
            'step': self.step_t,
            'last_lr': self.last_lr,
            'master': self.replica.flat_master,
        }

    def load_state_dict(self, state):
        if len(state['groups']) != len(self.param_groups):
            raise ValueError(
                f"FlatAdamW: state has {len(state['groups'])} groups, optimizer has {len(self.param_groups)}"
            )
        for group, saved in zip(self.param_groups, state['groups']):
            group['lr'] = saved['lr']
            group['betas'] = tuple(saved['betas'])
            group['eps'] = saved['eps']
            group['weight_decay'] = saved['weight_decay']
        self.schedule = LRSchedule.from_state_dict(state['schedule'])
        self._sched.copy_(torch.tensor(self.schedule.record(), dtype=torch.float64))
        self.exp_avg.copy_(state['exp_avg'].to(self.exp_avg.device))
        self.exp_avg_sq.copy_(state['exp_avg_sq'].to(self.exp_avg_sq.device))
        self.step_t.copy_(state['step'].to(self.step_t.device))
        if state.get('last_lr') is not None:
            self.last_lr.copy_(state['last_lr'].to(self.last_lr.device))
        if state.get('master') is not None and self.replica.flat_master is not None:
            self.replica.flat_master.copy_(state['master'].to(self.replica.flat_master.device))
        self.sync_hyperparameters()
