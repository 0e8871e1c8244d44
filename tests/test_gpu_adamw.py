"""The grouped AdamW kernels of optim.hip on the MI355X against
ref.fused_adamw_grouped_step, plus the two properties only a device can
show: nothing is written outside the buffers, and a captured step follows
the schedule and host-side changes under replay.
Run on an MI355X box: python -m pytest tests -m gpu"""

import pytest
import torch

from dmlcloud_amd import ops
from dmlcloud_amd.parallel import FlatAdamW, FlatReplica, GraphedStep, LRSchedule

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = [(1,), (7,), (8,), (9,), (3, 5), (33, 31)]
DTYPES = [torch.float32, torch.bfloat16]
# the project's flat-versus-torch fp32 tolerance (tests/test_properties.py)
TOL = dict(rtol=1e-5, atol=1e-5)


class ParamBag(torch.nn.Module):
    def __init__(self, sizes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s)) for s in sizes])

    def forward(self):
        return sum((p * p * p).sum() for p in self.ps)


def matrices_and_vectors(bag, wd=0.1, **second):
    ps = list(bag.parameters())
    return [
        {'params': [p for p in ps if p.dim() >= 2], 'weight_decay': wd},
        {'params': [p for p in ps if p.dim() < 2], 'weight_decay': 0.0, **second},
    ]


def make(device, dtype, sizes=SIZES, groups=matrices_and_vectors, seed=0, **kwargs):
    assert ops.is_available(), 'native extension must be present on a GPU box'
    torch.manual_seed(seed)
    bag = ParamBag(sizes).to(device)
    rep = FlatReplica(bag, dtype=dtype)
    kwargs.setdefault('lr', 1e-2)
    opt = FlatAdamW(rep, groups(bag), **kwargs)
    return bag, rep, opt


def real_mask(rep):
    mask = torch.zeros(rep.flat_param.numel(), dtype=torch.bool)
    for p, o in zip(rep.params, rep._offsets):
        mask[o : o + p.numel()] = True
    return mask


def group_mask(rep, opt, g):
    mask = torch.zeros(rep.flat_param.numel(), dtype=torch.bool)
    offset = {id(p): o for p, o in zip(rep.params, rep._offsets)}
    for p in opt.param_groups[g]['params']:
        mask[offset[id(p)] : offset[id(p)] + p.numel()] = True
    return mask


def random_grads(rep, seed):
    """Gradients for the real elements, zero in the padding (as autograd
    leaves it), rounded to the replica's dtype."""
    g = torch.Generator().manual_seed(seed)
    grad = torch.randn(rep.flat_param.numel(), generator=g) * real_mask(rep)
    return grad.to(rep.dtype)


def run_pair(dtype, sizes, groups, steps, **kwargs):
    """The same steps natively on the device and through the reference on
    the CPU, from the same values and the same gradients."""
    dev = make(DEV, dtype, sizes, groups, **kwargs)
    cpu = make('cpu', dtype, sizes, groups, **kwargs)
    assert torch.equal(dev[1].flat_param.cpu(), cpu[1].flat_param)
    assert torch.equal(dev[2].group_map.cpu(), cpu[2].group_map)
    before = cpu[1].flat_param.clone()
    for step in range(steps):
        grad = random_grads(cpu[1], 100 + step)
        cpu[1].flat_grad.copy_(grad)
        dev[1].flat_grad.copy_(grad)
        cpu[2].step()
        dev[2].step()
    torch.cuda.synchronize()
    return dev, cpu, before


def assert_matches_reference(dev, cpu):
    (_, rep_d, opt_d), (_, rep_c, opt_c) = dev, cpu
    assert opt_d.step_t.item() == opt_c.step_t.item()
    torch.testing.assert_close(opt_d.last_lr.cpu(), opt_c.last_lr, rtol=1e-6, atol=0)
    torch.testing.assert_close(opt_d.exp_avg.cpu(), opt_c.exp_avg, **TOL)
    torch.testing.assert_close(opt_d.exp_avg_sq.cpu(), opt_c.exp_avg_sq, **TOL)
    if rep_d.dtype is torch.float32:
        torch.testing.assert_close(rep_d.flat_param.cpu(), rep_c.flat_param, **TOL)
    else:
        torch.testing.assert_close(rep_d.flat_master.cpu(), rep_c.flat_master, **TOL)
        assert torch.equal(rep_d.flat_param, rep_d.flat_master.to(torch.bfloat16))


class TestAgainstReference:
    @pytest.mark.parametrize('dtype', DTYPES)
    def test_odd_size_bag(self, dtype):
        dev, cpu, before = run_pair(
            dtype, SIZES, matrices_and_vectors, 5, schedule=LRSchedule.warmup_cosine(2, 9, 0.1)
        )
        assert_matches_reference(dev, cpu)
        real = real_mask(cpu[1])
        assert (dev[1].flat_param.cpu()[real] != before[real]).float().mean() > 0.9

    @pytest.mark.parametrize('dtype', DTYPES)
    def test_grid_stride(self, dtype):
        """4_195_304 elements are 524_413 eight-element vectors: more than
        kMaxGrid * kBlock = 524_288 and no multiple of the block, so the
        tail and the (7,) parameter of the OTHER group behind it are
        reached in the second grid pass only."""
        big = 4_195_304
        assert big // 8 > 2048 * 256 and (big // 8) % 256 != 0

        def groups(bag):
            first, second = bag.parameters()
            return [{'params': [first], 'weight_decay': 0.1}, {'params': [second], 'weight_decay': 0.0, 'lr': 3e-2}]

        dev, cpu, before = run_pair(dtype, [(big,), (7,)], groups, 2)
        assert_matches_reference(dev, cpu)
        assert dev[2].group_map[-1].item() == 1 and dev[2].group_map[-2].item() == 0
        tiny = group_mask(cpu[1], cpu[2], 1)
        assert tiny.sum() == 7 and tiny[-8:-1].all()
        after = dev[1].flat_param.cpu()
        assert (after[tiny] != before[tiny]).all()


class TestExactness:
    @pytest.mark.parametrize('dtype', DTYPES)
    def test_decoupled_decay_zero_gradient(self, dtype):
        # powers of two: 1 - lr * wd = 0.96875 is exact in fp32
        _, rep, opt = make(DEV, dtype, groups=lambda b: matrices_and_vectors(b, wd=0.125), lr=0.25)
        weights = rep.flat_param if rep.flat_master is None else rep.flat_master
        before = weights.clone()
        rep.zero_grad()
        opt.step()
        decayed, rest = group_mask(rep, opt, 0).to(DEV), group_mask(rep, opt, 1).to(DEV)
        assert torch.equal(weights[decayed], (before * 0.96875)[decayed])
        assert not torch.equal(weights[decayed], before[decayed])
        assert torch.equal(weights[rest], before[rest])
        assert not opt.exp_avg.any() and not opt.exp_avg_sq.any()
        if rep.flat_master is not None:
            assert torch.equal(rep.flat_param, rep.flat_master.to(torch.bfloat16))

    @pytest.mark.parametrize('dtype', DTYPES)
    def test_lr_zero_group(self, dtype):
        _, rep, opt = make(DEV, dtype, groups=lambda b: matrices_and_vectors(b, lr=0.0))
        weights = rep.flat_param if rep.flat_master is None else rep.flat_master
        before, before_param = weights.clone(), rep.flat_param.clone()
        for step in range(2):
            rep.flat_grad.copy_(random_grads(rep, step))
            opt.step()
        frozen, moving = group_mask(rep, opt, 1).to(DEV), group_mask(rep, opt, 0).to(DEV)
        assert torch.equal(weights[frozen], before[frozen])
        assert torch.equal(rep.flat_param[frozen], before_param[frozen])
        assert (opt.exp_avg[frozen] != 0).all() and (opt.exp_avg_sq[frozen] != 0).all()
        assert (weights[moving] != before[moving]).all()
        assert opt.last_lr[1].item() == 0.0 and opt.last_lr[0].item() == pytest.approx(1e-2, rel=1e-6)

    @pytest.mark.parametrize('dtype', DTYPES)
    def test_padding_stays_zero(self, dtype):
        _, rep, opt = make(DEV, dtype)
        pad = ~real_mask(rep).to(DEV)
        assert pad.sum().item() == 7 + 1 + 0 + 7 + 1 + 1
        for step in range(5):
            rep.flat_grad.copy_(random_grads(rep, step))
            opt.step()
        assert not rep.flat_param[pad].any()
        assert not opt.exp_avg[pad].any() and not opt.exp_avg_sq[pad].any()
        if rep.flat_master is not None:
            assert not rep.flat_master[pad].any()


class TestCanaries:
    @pytest.mark.parametrize('dtype', DTYPES)
    def test_nothing_written_outside_the_buffers(self, dtype):
        """Moments, master and map are interior slices of larger tensors
        filled with a sentinel; three steps leave the surroundings intact."""
        assert ops.is_available()
        n, guard, ngroups = 8 * 131, 64, 3  # 131 chunks: a partial wave at the end
        sentinel = {torch.float32: -12345.0, torch.uint8: 0xA5}

        def guarded(dt):
            outer = torch.full((n + 2 * guard,), sentinel[dt], dtype=dt, device=DEV)
            return outer, outer[guard : guard + n]

        m_outer, m = guarded(torch.float32)
        v_outer, v = guarded(torch.float32)
        w_outer, w = guarded(torch.float32)
        map_outer = torch.full((n // 8 + 2 * guard,), sentinel[torch.uint8], dtype=torch.uint8, device=DEV)
        group_map = map_outer[guard : guard + n // 8]
        m.zero_()
        v.zero_()
        torch.manual_seed(0)
        w.copy_(torch.randn(n))
        group_map.copy_(torch.arange(n // 8) % ngroups)

        bf16 = dtype is torch.bfloat16
        param = w.to(torch.bfloat16) if bf16 else w
        hyper = torch.tensor(
            [[1e-2, 0.1, 0.9, 0.999, 1e-8, 0, 0, 0], [3e-3, 0.0, 0.8, 0.95, 1e-6, 0, 0, 0], [1e-3, 0.5, 0.9, 0.99, 1e-8, 0, 0, 0]],
            device=DEV,
        )
        sched = torch.tensor(LRSchedule.constant().record(), dtype=torch.float64, device=DEV)
        derived = torch.zeros(ngroups, 8, device=DEV)
        last_lr = torch.zeros(ngroups, device=DEV)
        step_t = torch.zeros(1, dtype=torch.int32, device=DEV)
        before = w.clone()
        for step in range(3):
            grad = torch.randn(n).to(DEV, dtype)
            ops.fused_adamw_grouped(
                param, grad, m, v, step_t, group_map, hyper, sched, derived, last_lr, master=w if bf16 else None
            )
        torch.cuda.synchronize()

        assert step_t.item() == 3
        assert (w != before).all() and (m != 0).all() and (v != 0).all()
        for outer in (m_outer, v_outer, w_outer):
            assert (outer[:guard] == sentinel[torch.float32]).all()
            assert (outer[guard + n :] == sentinel[torch.float32]).all()
        assert (map_outer[:guard] == sentinel[torch.uint8]).all()
        assert (map_outer[guard + n // 8 :] == sentinel[torch.uint8]).all()
        assert torch.equal(group_map.cpu(), (torch.arange(n // 8) % ngroups).to(torch.uint8))


class TestLauncherChecks:
    def test_bad_arguments_raise_before_any_launch(self):
        assert ops.is_available()
        n = 64

        def args(**over):
            a = dict(
                param=torch.zeros(n, device=DEV),
                grad=torch.zeros(n, device=DEV),
                exp_avg=torch.zeros(n, device=DEV),
                exp_avg_sq=torch.zeros(n, device=DEV),
                step_t=torch.zeros(1, dtype=torch.int32, device=DEV),
                group_map=torch.zeros(n // 8, dtype=torch.uint8, device=DEV),
                hyper=torch.tensor([[1e-3, 0.1, 0.9, 0.999, 1e-8, 0, 0, 0]] * 2, device=DEV),
                sched=torch.zeros(4, dtype=torch.float64, device=DEV),
                derived=torch.zeros(2, 8, device=DEV),
                last_lr=torch.zeros(2, device=DEV),
            )
            a.update(over)
            return a

        bad = [
            dict(group_map=torch.zeros(n // 8 + 1, dtype=torch.uint8, device=DEV)),
            dict(group_map=torch.zeros(n // 8, dtype=torch.uint8)),  # on the host
            dict(group_map=torch.zeros(n // 8, dtype=torch.int32, device=DEV)),
            dict(hyper=torch.zeros(17, 8, device=DEV), derived=torch.zeros(17, 8, device=DEV), last_lr=torch.zeros(17, device=DEV)),
            dict(hyper=torch.zeros(2, 5, device=DEV)),
            dict(derived=torch.zeros(3, 8, device=DEV)),
            dict(grad=torch.zeros(n + 8, device=DEV)),
            dict(grad=torch.zeros(n, dtype=torch.bfloat16, device=DEV)),
            dict(step_t=torch.zeros(1, dtype=torch.int64, device=DEV)),
        ]
        for over in bad:
            a = args(**over)
            with pytest.raises(RuntimeError):
                ops.fused_adamw_grouped(**a)
            assert a['step_t'].item() == 0
        odd = args(
            param=torch.zeros(60, device=DEV),
            grad=torch.zeros(60, device=DEV),
            exp_avg=torch.zeros(60, device=DEV),
            exp_avg_sq=torch.zeros(60, device=DEV),
            group_map=torch.zeros(7, dtype=torch.uint8, device=DEV),
        )
        with pytest.raises(RuntimeError):
            ops.fused_adamw_grouped(**odd)
        ops.fused_adamw_grouped(**args())  # the well-formed call goes through


def graph_twin(schedule):
    bag, rep, opt = make(DEV, torch.float32, schedule=schedule)

    def step():
        rep.zero_grad()
        bag.forward().backward()
        rep.grad_sync()
        opt.step()

    return rep, opt, step


@pytest.fixture
def kernels_loaded():
    """One eager step of a throwaway twin, so that the capture (which has
    no warmup of its own here) launches only kernels that ran before."""
    _, _, step = graph_twin(None)
    step()
    torch.cuda.synchronize()


class TestHipGraph:
    def test_replay_follows_device_schedule(self, kernels_loaded):
        k = 6
        schedule = LRSchedule.warmup_cosine(2, 5)
        rep_e, opt_e, step_e = graph_twin(schedule)
        eager_lrs = []
        for _ in range(k):
            step_e()
            eager_lrs.append(opt_e.last_lr.clone())

        rep_g, opt_g, step_g = graph_twin(schedule)
        gs = GraphedStep(step_g, warmup=0, validate=False)
        gs.initialize()
        assert gs.captured, 'hipGraph capture must succeed for the flat path'
        assert opt_g.step_t.item() == 0  # capture runs nothing
        replay_lrs = []
        for _ in range(k):
            gs()
            replay_lrs.append(opt_g.last_lr.clone())
        torch.cuda.synchronize()

        assert opt_g.step_t.item() == opt_e.step_t.item() == k
        assert torch.equal(rep_g.flat_param, rep_e.flat_param)
        assert torch.equal(opt_g.exp_avg, opt_e.exp_avg)
        assert torch.equal(opt_g.exp_avg_sq, opt_e.exp_avg_sq)
        assert torch.equal(opt_g.last_lr, opt_e.last_lr)
        for a, b in zip(replay_lrs, eager_lrs):
            assert torch.equal(a, b)
        # warmup 2, total 5: every replay up to the floor has a rate of its own
        for a, b in zip(replay_lrs[:4], replay_lrs[1:5]):
            assert not torch.equal(a, b)
        for s, lrs in enumerate(replay_lrs, start=1):
            assert lrs[0].item() == pytest.approx(1e-2 * schedule.multiplier(s), rel=1e-6, abs=1e-12)

    def test_host_change_reaches_a_captured_step(self, kernels_loaded):
        rep, opt, step = graph_twin(None)
        gs = GraphedStep(step, warmup=0, validate=False)
        gs.initialize()
        assert gs.captured, 'hipGraph capture must succeed for the flat path'
        gs()
        torch.cuda.synchronize()
        assert opt.last_lr.tolist() == [pytest.approx(1e-2, rel=1e-6)] * 2

        g0, g1 = group_mask(rep, opt, 0).to(DEV), group_mask(rep, opt, 1).to(DEV)
        before = rep.flat_param.clone()
        opt.param_groups[0]['lr'] = 0
        opt.sync_hyperparameters()
        gs()
        torch.cuda.synchronize()
        assert torch.equal(rep.flat_param[g0], before[g0])
        assert (rep.flat_param[g1] != before[g1]).all()
        assert opt.last_lr[0].item() == 0.0 and opt.last_lr[1].item() == pytest.approx(1e-2, rel=1e-6)
