"""GPT2Config.n_kv_head on the CPU: None / n_head leave the model exactly
as it was; a grouped model has the narrower c_attn, trains, and equals a
hand-written expansion of its own k/v."""

import sys

import pytest
import torch
from torch.nn import functional as F

from dmlcloud_amd.models import gpt2 as gpt2_mod
from dmlcloud_amd.models.gpt2 import GPT2, GPT2Config

TINY = dict(vocab_size=128, n_positions=32, n_embd=64, n_layer=2, n_head=4)


def _build(seed=0, **extra):
    torch.manual_seed(seed)
    return GPT2(GPT2Config(**TINY, **extra))


@pytest.mark.parametrize('n_kv_head', [None, TINY['n_head']])
def test_default_and_full_head_count_leave_the_model_unchanged(n_kv_head):
    base = _build()
    after_base = torch.rand(1)  # the RNG state after init: same number of draws
    model = _build(n_kv_head=n_kv_head)
    after = torch.rand(1)
    assert torch.equal(after, after_base)
    sd, sd_base = model.state_dict(), base.state_dict()
    assert list(sd) == list(sd_base)
    for name in sd_base:
        assert sd[name].shape == sd_base[name].shape, name
        assert torch.equal(sd[name], sd_base[name]), name
    assert [type(m) for m in model.modules()] == [type(m) for m in base.modules()]

    idx = torch.randint(0, TINY['vocab_size'], (2, 16))
    _, loss = model(idx, targets=idx)
    _, loss_base = base(idx, targets=idx)
    assert torch.equal(loss, loss_base)


def test_grouped_model_shapes_forward_backward():
    model = _build(n_kv_head=2)
    hd = TINY['n_embd'] // TINY['n_head']
    for blk in model.blocks:
        assert blk.attn.c_attn.weight.shape == (TINY['n_embd'] + 2 * 2 * hd, TINY['n_embd'])
        assert blk.attn.c_attn.bias.shape == (TINY['n_embd'] + 2 * 2 * hd,)
    idx = torch.randint(0, TINY['vocab_size'], (2, 16))
    logits, loss = model(idx, targets=idx)
    assert logits.shape == (2, 16, TINY['vocab_size'])
    loss.backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert model.blocks[0].attn.c_attn.weight.grad.abs().sum() > 0


def test_grouped_model_equals_hand_expanded_kv(monkeypatch):
    """Replace the model's attention call by one that expands k and v with
    repeat_interleave and runs plain multi-head SDPA: same loss and same
    gradients, to fp32 round-off."""
    model = _build(n_kv_head=2)
    idx = torch.randint(0, TINY['vocab_size'], (2, 16))
    seen = []

    def run():
        model.zero_grad(set_to_none=True)
        _, loss = model(idx, targets=idx)
        loss.backward()
        return loss.detach(), [p.grad.clone() for p in model.parameters()]

    loss, grads = run()

    def expanded_sdpa(q, k, v, causal=True, doc_start=None):
        assert doc_start is None and q.shape[1] == 4 and k.shape[1] == 2 and v.shape[1] == 2
        # strided views into the qkv buffer, not copies
        assert not k.is_contiguous() and k.stride(-1) == 1
        seen.append(k.shape)
        return F.scaled_dot_product_attention(q, k.repeat_interleave(2, 1), v.repeat_interleave(2, 1), is_causal=causal)

    monkeypatch.setattr(gpt2_mod, 'sdpa', expanded_sdpa)
    loss_x, grads_x = run()
    assert len(seen) == TINY['n_layer']
    torch.testing.assert_close(loss, loss_x, rtol=1e-5, atol=1e-6)
    for got, want in zip(grads, grads_x):
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('n_kv_head', [3, 0, 8])
def test_head_count_that_does_not_divide_is_refused(n_kv_head):
    with pytest.raises(AssertionError):
        _build(n_kv_head=n_kv_head)


if __name__ == '__main__':
    sys.exit(pytest.main([__file__]))
