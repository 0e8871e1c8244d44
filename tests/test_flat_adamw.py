"""FlatAdamW on the CPU reference path: decoupled decay, parameter groups,
the LR schedule, host-side hyperparameter changes and state round trips.
tests/test_gpu_adamw.py holds the native kernels to the same reference."""

import math
import types

import pytest
import torch

from dmlcloud_amd import TrainingPipeline, TrainValStage
from dmlcloud_amd.models import gpt2_tiny
from dmlcloud_amd.parallel import (
    FlatAdam,
    FlatAdamW,
    FlatReplica,
    FlatSGD,
    LRSchedule,
    weight_decay_groups,
)

SIZES = [(1,), (7,), (8,), (9,), (3, 5), (33, 31)]


class ParamBag(torch.nn.Module):
    def __init__(self, sizes=SIZES):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s)) for s in sizes])

    def forward(self):
        return sum((p * p * p).sum() for p in self.ps)


def make_bag(seed=0, sizes=SIZES):
    torch.manual_seed(seed)
    return ParamBag(sizes)


def two_groups(bag, wd=0.1, **second):
    """Matrices decay, vectors do not."""
    ps = list(bag.parameters())
    return [
        {'params': [p for p in ps if p.dim() >= 2], 'weight_decay': wd},
        {'params': [p for p in ps if p.dim() < 2], 'weight_decay': 0.0, **second},
    ]


def group_mask(replica, opt, g):
    """Boolean mask over the flat buffer of the real elements of group g."""
    mask = torch.zeros(replica.flat_param.numel(), dtype=torch.bool)
    offset = {id(p): o for p, o in zip(replica.params, replica._offsets)}
    for p in opt.param_groups[g]['params']:
        mask[offset[id(p)] : offset[id(p)] + p.numel()] = True
    return mask


def padding_mask(replica):
    mask = torch.ones(replica.flat_param.numel(), dtype=torch.bool)
    for p, o in zip(replica.params, replica._offsets):
        mask[o : o + p.numel()] = False
    return mask


def train_steps(bag, replica, opt, steps):
    for _ in range(steps):
        replica.zero_grad()
        bag.forward().backward()
        replica.grad_sync()
        opt.step()


class TestParity:
    def test_matches_torch_adamw_two_groups(self):
        m1, m2 = make_bag(), make_bag()
        rep = FlatReplica(m1)
        opt = FlatAdamW(rep, two_groups(m1), lr=1e-2)
        ref = torch.optim.AdamW(two_groups(m2), lr=1e-2)
        assert padding_mask(rep).any()
        for _ in range(5):
            train_steps(m1, rep, opt, 1)
            ref.zero_grad()
            m2.forward().backward()
            ref.step()
            for p1, p2 in zip(m1.parameters(), m2.parameters()):
                torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6)

    def test_one_group_default(self):
        m1, m2 = make_bag(), make_bag()
        rep = FlatReplica(m1)
        opt = FlatAdamW(rep, lr=1e-2, betas=(0.8, 0.95), weight_decay=0.05)
        ref = torch.optim.AdamW(m2.parameters(), lr=1e-2, betas=(0.8, 0.95), weight_decay=0.05)
        assert len(opt.param_groups) == 1
        for _ in range(5):
            train_steps(m1, rep, opt, 1)
            ref.zero_grad()
            m2.forward().backward()
            ref.step()
        for p1, p2 in zip(m1.parameters(), m2.parameters()):
            torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6)

    def test_bf16_master_tracks_fp32(self):
        """The bf16 replica's fp32 master follows an fp32 FlatAdamW that is
        driven by the same bf16-rounded gradients (tolerance of the bf16
        Adam master in tests/test_ops.py), and param == bf16(master)."""
        m16, m32 = make_bag(), make_bag()
        rep16 = FlatReplica(m16, dtype=torch.bfloat16)
        # the fp32 twin starts from the same master values
        rep32 = FlatReplica(m32)
        torch.testing.assert_close(rep16.flat_master, rep32.flat_param, rtol=0, atol=0)
        opt16 = FlatAdamW(rep16, two_groups(m16), lr=1e-2)
        opt32 = FlatAdamW(rep32, two_groups(m32), lr=1e-2)
        for _ in range(5):
            rep16.zero_grad()
            m16.forward().float().backward()
            rep32.flat_grad.copy_(rep16.flat_grad.float())
            opt16.step()
            opt32.step()
            torch.testing.assert_close(rep16.flat_master, rep32.flat_param, rtol=1e-6, atol=1e-7)
            assert torch.equal(rep16.flat_param, rep16.flat_master.to(torch.bfloat16))
        assert not torch.equal(rep16.flat_master, FlatReplica(make_bag()).flat_param)


class TestExactness:
    # lr and wd are powers of two: 1 - lr * wd = 0.96875 is exact in fp32,
    # so "exactly p * (1 - lr * wd)" has one meaning
    LR, WD = 0.25, 0.125

    def test_decoupled_not_l2(self):
        bag = make_bag()
        rep = FlatReplica(bag)
        opt = FlatAdamW(rep, two_groups(bag, wd=self.WD), lr=self.LR)
        before = rep.flat_param.clone()
        rep.zero_grad()
        opt.step()  # zero gradient, zero moments
        decayed, rest = group_mask(rep, opt, 0), group_mask(rep, opt, 1)
        expected = before * torch.tensor(1.0 - self.LR * self.WD, dtype=torch.float32)
        assert torch.equal(rep.flat_param[decayed], expected[decayed])
        assert not torch.equal(rep.flat_param[decayed], before[decayed])
        assert torch.equal(rep.flat_param[rest], before[rest])
        # L2 regularisation would have fed wd * p into the moments
        assert not opt.exp_avg.any() and not opt.exp_avg_sq.any()

    def test_lr_zero_group_keeps_params_moves_moments(self):
        bag = make_bag()
        rep = FlatReplica(bag)
        opt = FlatAdamW(rep, two_groups(bag, lr=0.0), lr=1e-2)
        before = rep.flat_param.clone()
        train_steps(bag, rep, opt, 2)
        frozen, moving = group_mask(rep, opt, 1), group_mask(rep, opt, 0)
        assert torch.equal(rep.flat_param[frozen], before[frozen])
        assert (opt.exp_avg[frozen] != 0).all() and (opt.exp_avg_sq[frozen] != 0).all()
        assert (rep.flat_param[moving] != before[moving]).all()
        assert opt.last_lr.tolist() == [pytest.approx(1e-2), 0.0]

    @pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
    def test_padding_stays_zero(self, dtype):
        bag = make_bag()
        rep = FlatReplica(bag, dtype=dtype)
        opt = FlatAdamW(rep, two_groups(bag), lr=1e-2)
        pad = padding_mask(rep)
        assert pad.sum() == sum((-p.numel()) % 8 for p in bag.parameters()) > 0
        for _ in range(5):
            rep.zero_grad()
            bag.forward().float().backward()
            opt.step()
        assert not rep.flat_param[pad].any()
        assert not opt.exp_avg[pad].any() and not opt.exp_avg_sq[pad].any()
        if rep.flat_master is not None:
            assert not rep.flat_master[pad].any()

    def test_grad_scale_equals_halved_gradients(self):
        from dmlcloud_amd import ops

        torch.manual_seed(0)
        n = 64
        group_map = torch.tensor([0, 1] * (n // 16), dtype=torch.uint8)
        hyper = torch.tensor([[1e-2, 0.1, 0.9, 0.999, 1e-8, 0, 0, 0], [3e-3, 0.0, 0.8, 0.95, 1e-6, 0, 0, 0]])
        sched = torch.tensor(LRSchedule.warmup_cosine(2, 9).record(), dtype=torch.float64)
        p0, grad = torch.randn(n), torch.randn(n)
        results = []
        for g, scale in ((grad, 0.5), (grad * 0.5, 1.0)):
            p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
            step_t = torch.zeros(1, dtype=torch.int32)
            derived, last_lr = torch.zeros(2, 8), torch.zeros(2)
            for _ in range(3):
                ops.fused_adamw_grouped(p, g, m, v, step_t, group_map, hyper, sched, derived, last_lr, grad_scale=scale)
            results.append((p, m, v))
        for a, b in zip(*results):
            assert torch.equal(a, b)
        assert not torch.equal(results[0][0], p0)

    def test_replica_grad_scale_is_used(self):
        bag = make_bag()
        rep = FlatReplica(bag)
        rep.world_size = 2  # grad_scale = 1 / world
        opt = FlatAdamW(rep, two_groups(bag), lr=1e-2)
        bag2 = make_bag()
        rep2 = FlatReplica(bag2)
        opt2 = FlatAdamW(rep2, two_groups(bag2), lr=1e-2)
        rep.flat_grad.copy_(torch.randn(rep.flat_grad.numel()))
        rep2.flat_grad.copy_(rep.flat_grad * 0.5)
        opt.step()
        opt2.step()
        assert torch.equal(rep.flat_param, rep2.flat_param)


def expected_multiplier(kind, s, w, t, r):
    """The issue's formula, written out independently of LRSchedule."""
    if w > 0 and s <= w:
        return s / w
    if s >= t:
        return r
    x = (s - w) / (t - w)
    if kind == 'cosine':
        return r + (1 - r) * 0.5 * (1 + math.cos(math.pi * x))
    return r + (1 - r) * (1 - x)


class TestSchedule:
    W, T, R = 4, 20, 0.1

    @pytest.mark.parametrize('kind', ['cosine', 'linear'])
    def test_multiplier_points(self, kind):
        make = LRSchedule.warmup_cosine if kind == 'cosine' else LRSchedule.warmup_linear
        sched = make(self.W, self.T, min_ratio=self.R)
        mid = (self.W + self.T) // 2
        assert sched.multiplier(1) == pytest.approx(1 / self.W)
        assert sched.multiplier(self.W) == pytest.approx(1.0)
        assert sched.multiplier(mid) == pytest.approx(self.R + (1 - self.R) * 0.5)
        assert sched.multiplier(self.T) == pytest.approx(self.R)
        assert sched.multiplier(self.T + 5) == pytest.approx(self.R)
        for s in (1, self.W, self.W + 1, mid, self.T, self.T + 5):
            assert sched.multiplier(s) == pytest.approx(expected_multiplier(kind, s, self.W, self.T, self.R))
        assert self.R < sched.multiplier(self.W + 1) < 1.0

    def test_constant_and_no_warmup(self):
        assert all(LRSchedule.constant().multiplier(s) == 1.0 for s in (1, 10, 10**6))
        sched = LRSchedule.warmup_linear(0, 10)
        assert sched.multiplier(1) == pytest.approx(0.9)
        assert sched.multiplier(10) == 0.0

    def test_invalid(self):
        with pytest.raises(ValueError):
            LRSchedule.warmup_cosine(5, 5)
        with pytest.raises(ValueError):
            LRSchedule.warmup_linear(2, 10, min_ratio=1.5)
        with pytest.raises(ValueError):
            LRSchedule('exponential')

    @pytest.mark.parametrize('kind', ['cosine', 'linear'])
    def test_last_lr_follows_schedule(self, kind):
        make = LRSchedule.warmup_cosine if kind == 'cosine' else LRSchedule.warmup_linear
        sched = make(3, 10, min_ratio=0.05)
        bag = make_bag()
        rep = FlatReplica(bag)
        opt = FlatAdamW(rep, two_groups(bag, lr=2e-3), lr=1e-2, schedule=sched)
        assert opt.last_lr.dtype is torch.float32 and opt.last_lr.shape == (2,)
        seen = []
        for step in range(1, 13):
            train_steps(bag, rep, opt, 1)
            mult = expected_multiplier(kind, step, 3, 10, 0.05)
            assert sched.multiplier(step) == pytest.approx(mult)
            assert opt.last_lr[0].item() == pytest.approx(1e-2 * mult, rel=1e-6)
            assert opt.last_lr[1].item() == pytest.approx(2e-3 * mult, rel=1e-6)
            seen.append(opt.last_lr[0].item())
        assert seen[2] == max(seen) and seen[-1] == pytest.approx(5e-4, rel=1e-6)

    def test_schedule_changes_the_update(self):
        """The scheduled rate is what the update uses: AdamW's first step
        moves every element by lr_t (up to eps), here 1e-2 / 4."""
        bag = make_bag()
        rep = FlatReplica(bag)
        opt = FlatAdamW(rep, lr=1e-2, weight_decay=0.0, schedule=LRSchedule.warmup_cosine(4, 20))
        before = rep.flat_param.clone()
        rep.flat_grad.fill_(0.5)
        opt.step()
        moved = before - rep.flat_param
        torch.testing.assert_close(moved, torch.full_like(moved, 2.5e-3), rtol=1e-3, atol=0)


class TestHostLR:
    def test_lambda_lr_changes_next_eager_step(self):
        m1, m2 = make_bag(), make_bag()
        rep = FlatReplica(m1)
        opt = FlatAdamW(rep, two_groups(m1, lr=5e-3), lr=1e-2)
        ref = torch.optim.AdamW(two_groups(m2, lr=5e-3), lr=1e-2)
        lam = lambda epoch: 0.5**epoch  # noqa: E731
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
        ref_sched = torch.optim.lr_scheduler.LambdaLR(ref, lam)
        rates = []
        for _ in range(3):
            train_steps(m1, rep, opt, 1)
            ref.zero_grad()
            m2.forward().backward()
            ref.step()
            rates.append(opt.last_lr.tolist())
            sched.step()
            ref_sched.step()
        for k, (r0, r1) in enumerate(rates):
            assert r0 == pytest.approx(1e-2 * 0.5**k, rel=1e-6)
            assert r1 == pytest.approx(5e-3 * 0.5**k, rel=1e-6)
        for p1, p2 in zip(m1.parameters(), m2.parameters()):
            torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6)

    def test_schedule_multiplies_host_lr(self):
        bag = make_bag()
        rep = FlatReplica(bag)
        opt = FlatAdamW(rep, lr=1e-2, schedule=LRSchedule.warmup_linear(2, 6))
        train_steps(bag, rep, opt, 1)
        assert opt.last_lr[0].item() == pytest.approx(5e-3, rel=1e-6)
        opt.param_groups[0]['lr'] = 4e-2
        train_steps(bag, rep, opt, 1)
        assert opt.last_lr[0].item() == pytest.approx(4e-2, rel=1e-6)
        opt.lr = 8e-2
        train_steps(bag, rep, opt, 1)
        assert opt.last_lr[0].item() == pytest.approx(8e-2 * 0.75, rel=1e-6)


class TestErrors:
    def test_parameter_in_two_groups(self):
        bag = make_bag()
        rep = FlatReplica(bag)
        ps = list(bag.parameters())
        with pytest.raises(ValueError, match='more than one group'):
            FlatAdamW(rep, [{'params': ps}, {'params': ps[:1]}])

    def test_parameter_in_no_group(self):
        bag = make_bag()
        rep = FlatReplica(bag)
        ps = list(bag.parameters())
        with pytest.raises(ValueError, match='in no group'):
            FlatAdamW(rep, [{'params': ps[:2]}, {'params': ps[3:]}])

    def test_foreign_parameter(self):
        bag = make_bag()
        rep = FlatReplica(bag)
        ps = list(bag.parameters())
        with pytest.raises(ValueError, match='not in the replica'):
            FlatAdamW(rep, [{'params': ps}, {'params': [torch.nn.Parameter(torch.zeros(3))]}])

    def test_more_than_16_groups(self):
        bag = make_bag(sizes=[(2,)] * 17)
        rep = FlatReplica(bag)
        ps = list(bag.parameters())
        with pytest.raises(ValueError, match='at most 16'):
            FlatAdamW(rep, [{'params': [p]} for p in ps])
        opt = FlatAdamW(rep, [{'params': [p]} for p in ps[:15]] + [{'params': ps[15:]}])
        assert len(opt.param_groups) == 16
        assert opt.group_map.tolist() == list(range(15)) + [15, 15]

    @pytest.mark.parametrize('cls', [FlatAdam, FlatSGD])
    def test_single_group_optimizers_still_refuse_groups(self, cls):
        bag = make_bag()
        rep = FlatReplica(bag)
        ps = list(bag.parameters())
        grouped = types.SimpleNamespace(
            params=[{'params': ps[:2]}, {'params': ps[2:]}],
            flat_param=rep.flat_param,
            dtype=rep.dtype,
        )
        with pytest.raises(ValueError, match='one param group'):
            cls(grouped)


class TestGroupMap:
    def test_map_follows_offsets(self):
        bag = make_bag()
        rep = FlatReplica(bag)
        opt = FlatAdamW(rep, two_groups(bag))
        # sizes 1, 7, 8, 9, 15, 1023 -> 1, 1, 1, 2, 2, 128 chunks
        assert opt.group_map.dtype is torch.uint8
        assert opt.group_map.tolist() == [1] * 5 + [0] * 130
        assert opt.group_map.numel() * 8 == rep.flat_param.numel()


class TestStateDict:
    def test_roundtrip_restores_everything(self):
        bag = make_bag()
        rep = FlatReplica(bag, dtype=torch.bfloat16)
        opt = FlatAdamW(
            rep, two_groups(bag, lr=3e-3, betas=(0.8, 0.9)), lr=1e-2, schedule=LRSchedule.warmup_cosine(2, 9, 0.1)
        )
        for _ in range(3):
            rep.zero_grad()
            bag.forward().float().backward()
            opt.step()
        state = {'model': rep.state_dict(), 'opt': opt.state_dict()}

        bag2 = make_bag(seed=1)
        rep2 = FlatReplica(bag2, dtype=torch.bfloat16)
        opt2 = FlatAdamW(rep2, two_groups(bag2), lr=1.0)
        rep2.load_state_dict(state['model'])
        opt2.load_state_dict(state['opt'])

        assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
        assert opt2.step_t.item() == 3
        assert torch.equal(rep2.flat_master, rep.flat_master)
        assert opt2.schedule == LRSchedule.warmup_cosine(2, 9, 0.1)
        for g2, g in zip(opt2.param_groups, opt.param_groups):
            for key in ('lr', 'betas', 'eps', 'weight_decay'):
                assert g2[key] == g[key]
        assert opt2.param_groups[1]['betas'] == (0.8, 0.9)

        # and both continue identically
        for b, r, o in ((bag, rep, opt), (bag2, rep2, opt2)):
            r.zero_grad()
            b.forward().float().backward()
            o.step()
        assert torch.equal(rep2.flat_param, rep.flat_param)
        assert torch.equal(rep2.flat_master, rep.flat_master)
        assert torch.equal(opt2.last_lr, opt.last_lr)

    def test_group_count_mismatch(self):
        bag = make_bag()
        opt = FlatAdamW(FlatReplica(bag), two_groups(bag))
        bag2 = make_bag()
        opt2 = FlatAdamW(FlatReplica(bag2))
        with pytest.raises(ValueError):
            opt2.load_state_dict(opt.state_dict())


class DS(torch.utils.data.Dataset):
    def __len__(self):
        return 8

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(idx)
        return torch.randn(10, generator=g), idx % 10


class AdamWStage(TrainValStage):
    def pre_stage(self):
        torch.manual_seed(0)
        model = torch.nn.Sequential(torch.nn.Linear(10, 9), torch.nn.Tanh(), torch.nn.Linear(9, 10))
        self.pipeline.register_model('m', model, ddp_impl='flat')
        replica = self.pipeline.models['m']
        opt = FlatAdamW(
            replica, weight_decay_groups(model, 0.1), lr=1e-2, schedule=LRSchedule.warmup_cosine(2, 7, 0.1)
        )
        self.pipeline.register_optimizer('adamw', opt)
        self.pipeline.register_dataset('train', torch.utils.data.DataLoader(DS(), batch_size=4))
        self.pipeline.register_dataset('val', torch.utils.data.DataLoader(DS(), batch_size=4))
        self.loss = torch.nn.CrossEntropyLoss()

    def step(self, batch):
        x, y = (t.to(self.device) for t in batch)
        return self.loss(self.pipeline.models['m'](x), y)


class TestPipelineCheckpoint:
    def test_dmlt_roundtrip_continues_bit_identically(self, torch_distributed, tmp_path):
        pipeline = TrainingPipeline(name='adamw')
        pipeline.enable_checkpointing(str(tmp_path), resume=False)
        stage = AdamWStage()
        pipeline.append_stage(stage, max_epochs=2)
        pipeline.run()
        pipeline.save_checkpoint()
        opt = pipeline.optimizers['adamw']
        assert opt.step_t.item() == 4

        pipeline2 = TrainingPipeline(name='adamw2')
        pipeline2.checkpoint_dir = pipeline.checkpoint_dir
        pipeline2.device = pipeline.device
        stage2 = AdamWStage()
        pipeline2.append_stage(stage2, max_epochs=2)
        stage2.pre_stage()
        opt2 = pipeline2.optimizers['adamw']
        opt2.schedule = LRSchedule.constant()  # the load must bring the saved one back
        pipeline2.load_checkpoint()

        rep, rep2 = pipeline.models['m'], pipeline2.models['m']
        assert torch.equal(rep2.flat_param, rep.flat_param)
        assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
        assert opt2.step_t.item() == 4
        assert opt2.schedule == LRSchedule.warmup_cosine(2, 7, 0.1)

        x, y = (t.to(pipeline.device) for t in next(iter(torch.utils.data.DataLoader(DS(), batch_size=4))))
        for r, o in ((rep, opt), (rep2, opt2)):
            for _ in range(2):
                r.zero_grad()
                torch.nn.functional.cross_entropy(r(x), y).backward()
                r.grad_sync()
                o.step()
        assert torch.equal(rep2.flat_param, rep.flat_param)
        assert torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
        assert torch.equal(opt2.last_lr, opt.last_lr)
        assert opt.last_lr[0].item() == pytest.approx(1e-2 * LRSchedule.warmup_cosine(2, 7, 0.1).multiplier(6), rel=1e-6)


class TestWeightDecayGroups:
    def test_gpt2_tiny_split(self):
        model = gpt2_tiny()
        groups = weight_decay_groups(model, 0.1)
        assert [g['weight_decay'] for g in groups] == [0.1, 0.0]
        listed = [id(p) for g in groups for p in g['params']]
        assert len(listed) == len(set(listed))
        assert set(listed) == {id(p) for p in model.parameters()}
        assert len(listed) == len(list(model.parameters()))

        def is_norm(mod):  # the model's own LayerNorm module or torch's
            return type(mod).__name__ == 'LayerNorm'

        assert sum(is_norm(mod) for mod in model.modules()) == 2 * model.cfg.n_layer + 1
        names = {}
        for mod_name, mod in model.named_modules():
            for p_name, p in mod.named_parameters(recurse=False):
                names.setdefault(id(p), []).append((mod, p_name))
        for p in groups[1]['params']:
            assert all(is_norm(mod) or p_name == 'bias' for mod, p_name in names[id(p)])
        for p in groups[0]['params']:
            assert all(not is_norm(mod) and p_name != 'bias' for mod, p_name in names[id(p)])

        # the tied wte / lm_head weight: two owners, listed once, decayed
        assert model.lm_head.weight is model.wte.weight
        assert len(names[id(model.wte.weight)]) == 2
        assert sum(p is model.wte.weight for g in groups for p in g['params']) == 1
        assert any(p is model.wte.weight for p in groups[0]['params'])

        opt = FlatAdamW(FlatReplica(model), groups, lr=3e-4)
        assert len(opt.param_groups) == 2

    def test_no_decay_override(self):
        model = gpt2_tiny()
        groups = weight_decay_groups(model, 0.1, no_decay=lambda name, p: p.dim() < 2 or 'wpe' in name)
        assert any(p is model.wpe.weight for p in groups[1]['params'])
        assert not any(p is model.wpe.weight for p in groups[0]['params'])
        assert sum(len(g['params']) for g in groups) == len(list(model.parameters()))
