"""Packed-sequence (document-masked) causal attention in the MFMA kernels
(their kDoc instantiations: one clamped doc_start per query row, -1e30 /
p = 0 masks, block- and wave-uniform tile skips).

B = 2, H = 2, D = 64, bf16. Layouts put document boundaries on the 64-key
tile and 128-row block edges (EDGES), inside a 16-row sub-tile (MID: the
straddling sub-tile whose garbage must be wiped), at every token
(SINGLETONS) and in a sequence that is no multiple of 64 (RAGGED).

Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools
import math

import pytest
import torch

from attn_testlib import assert_fwd_bwd_close as _assert_close
from attn_testlib import run_with_canaries

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B, H, D = 2, 2, 64
SCALE = 1.0 / math.sqrt(D)

# name -> (N, document boundaries)
LAYOUTS = {
    'ONE': (200, [0, 200]),
    'EDGES': (256, [0, 64, 128, 256]),
    'MID': (256, [0, 7, 70, 200, 256]),
    'SINGLETONS': (130, list(range(131))),
    'RAGGED': (200, [0, 33, 129, 200]),
    'HALVES': (256, [0, 128, 256]),
}
# per batch row; MIXED gives the two rows different layouts
CASES = {
    'ONE': ('ONE', 'ONE'),
    'EDGES': ('EDGES', 'EDGES'),
    'MID': ('MID', 'MID'),
    'SINGLETONS': ('SINGLETONS', 'SINGLETONS'),
    'RAGGED': ('RAGGED', 'RAGGED'),
    'MIXED': ('EDGES', 'MID'),
}


def _row_starts(name):
    n, bounds = LAYOUTS[name]
    ds = torch.empty(n, dtype=torch.int32)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ds[lo:hi] = lo
    return ds


@functools.lru_cache(maxsize=None)
def _doc_start(case):
    """int32 [B, N] on the device; never modified."""
    return torch.stack([_row_starts(name) for name in CASES.get(case, (case, case))]).to(DEV)


def _n(case):
    return _doc_start(case).shape[1]


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """q, k, v, dO for one length (bf16, on the device); never modified."""
    g = torch.Generator().manual_seed(2000 + n)
    return tuple((torch.randn(B, H, n, D, generator=g) * 0.5).to(torch.bfloat16).to(DEV) for _ in range(4))


def _definition_mask(ds):
    """[B, 1, N, N]: query i attends key j iff doc_start[b, i] ==
    doc_start[b, j] and j <= i."""
    n = ds.shape[1]
    same = ds.unsqueeze(2) == ds.unsqueeze(1)
    return (same & torch.ones(n, n, dtype=torch.bool, device=ds.device).tril()).unsqueeze(1)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """fp32 masked SDPA + autograd on the bf16-rounded inputs, once per
    case: (out, dq, dk, dv)."""
    q, k, v, do = _inputs(_n(case))
    q2, k2, v2 = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(q2, k2, v2, attn_mask=_definition_mask(_doc_start(case)))
    ref.backward(do.float())
    return ref.detach(), q2.grad, k2.grad, v2.grad


@functools.lru_cache(maxsize=None)
def _native(case):
    """The packed result through sdpa, once per case: (out, dq, dk, dv)."""
    from dmlcloud_amd.ops.fused_attn import fused_attention_usable, sdpa

    q, k, v, do = _inputs(_n(case))
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    ds = _doc_start(case)
    assert fused_attention_usable(q, k, v, doc_start=ds) is True
    out = sdpa(q, k, v, causal=True, doc_start=ds)
    out.backward(do)
    return out.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize('case', list(CASES))
def test_sdpa_fwd_bwd_matches_masked_autograd(case):
    _assert_close(case, _native(case), _reference(case))


@pytest.mark.parametrize('case', list(CASES))
def test_lse_direct_matches_blueprint(case):
    from dmlcloud_amd import _C
    from dmlcloud_amd.ops._attention_ref import flash_attn_fwd_padded

    n = _n(case)
    q, k, v, _ = _inputs(n)
    ds = _doc_start(case)
    o = torch.empty(B, H, n, D, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, H, n, dtype=torch.float32, device=DEV)
    _C.attn_fwd(q, k, v, o, lse, SCALE, True, ds)
    torch.testing.assert_close(o.float(), _reference(case)[0], rtol=3e-2, atol=3e-2)

    qc, kc, vc, dsc = q.cpu().float(), k.cpu().float(), v.cpu().float(), ds.cpu()
    for b in range(B):
        for h in range(H):
            _, ref_lse = flash_attn_fwd_padded(qc[b, h], kc[b, h], vc[b, h], causal=True, doc_start=dsc[b])
            torch.testing.assert_close(lse[b, h].cpu(), ref_lse, rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize('case', ['EDGES', 'MID', 'RAGGED', 'MIXED'])
def test_packed_equals_each_document_alone(case):
    """Every document run by itself through the dense causal native path."""
    from dmlcloud_amd.ops.fused_attn import fused_attention_usable, sdpa

    q, k, v, do = _inputs(_n(case))
    alone = [torch.empty(B, H, _n(case), D, dtype=torch.bfloat16, device=DEV) for _ in range(4)]
    for b, name in enumerate(CASES[case]):
        _, bounds = LAYOUTS[name]
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            qd, kd, vd = (t[b : b + 1, :, lo:hi].clone().requires_grad_(True) for t in (q, k, v))
            assert fused_attention_usable(qd, kd, vd) is True
            out = sdpa(qd, kd, vd, causal=True)
            out.backward(do[b : b + 1, :, lo:hi])
            for dst, src in zip(alone, (out.detach(), qd.grad, kd.grad, vd.grad)):
                dst[b : b + 1, :, lo:hi] = src
    _assert_close(case + ' vs alone', _native(case), alone)


def test_one_document_equals_dense_causal():
    from dmlcloud_amd.ops.fused_attn import sdpa

    q, k, v, do = _inputs(_n('ONE'))
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = sdpa(q, k, v, causal=True)
    out.backward(do)
    _assert_close('ONE vs dense', _native('ONE'), (out.detach(), q.grad, k.grad, v.grad))


def test_singletons_are_exact():
    """Every token its own document: each softmax weight is exactly 1.0
    (the diagonal) or 0.0, so out = v and dv = dO bit for bit, and
    dq = dk = 0 up to the rounding of dP - delta."""
    out, dq, dk, dv = _native('SINGLETONS')
    _, _, v, do = _inputs(_n('SINGLETONS'))
    assert torch.equal(out, v)
    assert torch.equal(dv, do)
    torch.testing.assert_close(dq.float(), torch.zeros_like(dq, dtype=torch.float32), rtol=0.0, atol=1e-2)
    torch.testing.assert_close(dk.float(), torch.zeros_like(dk, dtype=torch.float32), rtol=0.0, atol=1e-2)


def _half_reference(lo, hi):
    """Dense causal fp32 reference of rows [lo, hi) alone."""
    q, k, v, do = _inputs(256)
    q2, k2, v2 = (t[:, :, lo:hi].float().requires_grad_(True) for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(q2, k2, v2, is_causal=True)
    future = torch.ones(hi - lo, hi - lo, dtype=torch.bool, device=DEV).triu(1)
    scores = (q2.detach() @ k2.detach().transpose(-1, -2)) * SCALE
    lse = torch.logsumexp(scores.masked_fill(future, -float('inf')), dim=-1)
    ref.backward(do[:, :, lo:hi].float())
    return ref.detach(), lse, q2.grad, k2.grad, v2.grad


def test_tiles_of_other_documents_are_skipped_fwd_dq():
    """NaN * 0 inside an MFMA is NaN: with K and V of the first document
    set to NaN, the second document's out, lse and dq stay finite only if
    the first document's tiles are never multiplied in."""
    from dmlcloud_amd import _C

    n = 256
    q, k, v, do = _inputs(n)
    k, v = k.clone(), v.clone()
    k[:, :, :128] = float('nan')
    v[:, :, :128] = float('nan')
    ds = _doc_start('HALVES')
    o, dq, dk, dv = (torch.empty(B, H, n, D, dtype=torch.bfloat16, device=DEV) for _ in range(4))
    lse = torch.empty(B, H, n, dtype=torch.float32, device=DEV)
    delta = torch.empty(B * H * n, dtype=torch.float32, device=DEV)
    _C.attn_fwd(q, k, v, o, lse, SCALE, True, ds)
    _C.attn_bwd(q, k, v, do, o, lse, dq, dk, dv, delta, SCALE, True, ds)

    ref, ref_lse, rdq, _, _ = _half_reference(128, 256)
    for t in (o, lse, dq):
        assert torch.isfinite(t[:, :, 128:]).all()
    torch.testing.assert_close(o[:, :, 128:].float(), ref, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(lse[:, :, 128:], ref_lse, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(dq[:, :, 128:].float(), rdq, rtol=5e-2, atol=5e-2)


def test_tiles_of_other_documents_are_skipped_dkdv():
    """Q and dO of the second document are NaN (and so are its o, lse and
    delta): dk and dv of the first document stay finite only if the dkdv
    loop leaves before the second document's q-steps."""
    from dmlcloud_amd import _C

    n = 256
    q, k, v, do = _inputs(n)
    q, do = q.clone(), do.clone()
    q[:, :, 128:] = float('nan')
    do[:, :, 128:] = float('nan')
    ds = _doc_start('HALVES')
    o, dq, dk, dv = (torch.empty(B, H, n, D, dtype=torch.bfloat16, device=DEV) for _ in range(4))
    lse = torch.empty(B, H, n, dtype=torch.float32, device=DEV)
    delta = torch.empty(B * H * n, dtype=torch.float32, device=DEV)
    _C.attn_fwd(q, k, v, o, lse, SCALE, True, ds)
    _C.attn_bwd(q, k, v, do, o, lse, dq, dk, dv, delta, SCALE, True, ds)

    _, _, _, rdk, rdv = _half_reference(0, 128)
    assert torch.isfinite(dk[:, :, :128]).all() and torch.isfinite(dv[:, :, :128]).all()
    torch.testing.assert_close(dk[:, :, :128].float(), rdk, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(dv[:, :, :128].float(), rdv, rtol=5e-2, atol=5e-2)


def test_canaries_untouched():
    o, _, dq, dk, dv = run_with_canaries(_inputs(_n('RAGGED')), True, _doc_start('RAGGED'))
    _assert_close('RAGGED canaries', (o, dq, dk, dv), _reference('RAGGED'))


def test_transpose_views_bit_identical():
    """[B, T, H, D] memory seen as [B, H, T, D] matches the contiguous
    path bit for bit."""
    from dmlcloud_amd.ops.fused_attn import sdpa

    n, ds = _n('MID'), _doc_start('MID')
    g = torch.Generator().manual_seed(5)
    base = [(torch.randn(B, n, H, D, generator=g) * 0.5).to(torch.bfloat16).to(DEV) for _ in range(3)]
    q, k, v = (t.transpose(1, 2).requires_grad_(True) for t in base)
    assert not q.is_contiguous()
    do = _inputs(n)[3]

    out = sdpa(q, k, v, causal=True, doc_start=ds)
    out.backward(do)

    q2, k2, v2 = (t.detach().contiguous().requires_grad_(True) for t in (q, k, v))
    out2 = sdpa(q2, k2, v2, causal=True, doc_start=ds)
    out2.backward(do)

    assert torch.equal(out, out2)
    assert torch.equal(q.grad, q2.grad)
    assert torch.equal(k.grad, k2.grad)
    assert torch.equal(v.grad, v2.grad)


@pytest.mark.parametrize('n', [200, 256])
def test_malformed_doc_start_is_clamped(n):
    """Values in [0, 10 N), not monotone, plus negatives: the kernels
    clamp what they read to [0, q], so the run completes, every output is
    finite (each row keeps its diagonal key) and nothing is written
    outside the outputs."""
    g = torch.Generator().manual_seed(77 + n)
    ds = torch.randint(0, 10 * n, (B, n), generator=g, dtype=torch.int32)
    ds[:, ::5] = torch.randint(0, n, (B, len(range(0, n, 5))), generator=g, dtype=torch.int32)
    ds[:, 3::11] = -9
    for t in run_with_canaries(_inputs(n), True, ds.to(DEV)):
        assert torch.isfinite(t).all()


def test_bindings_validate_doc_start():
    from dmlcloud_amd import _C

    n = 128
    q, k, v, _ = _inputs(n)
    o = torch.empty_like(q)
    lse = torch.empty(B, H, n, dtype=torch.float32, device=DEV)
    good = torch.zeros(B, n, dtype=torch.int32, device=DEV)
    for bad, causal in (
        (good.long(), True),  # not int32
        (good[:, : n - 1], True),  # not [B, N]
        (torch.zeros(B, 2 * n, dtype=torch.int32, device=DEV)[:, ::2], True),  # not contiguous
        (good.cpu(), True),  # not on q's device
        (good, False),  # not causal
    ):
        with pytest.raises(RuntimeError):
            _C.attn_fwd(q, k, v, o, lse, SCALE, causal, bad)
    _C.attn_fwd(q, k, v, o, lse, SCALE, True, None)  # None is the dense path


def test_non_causal_doc_mask_falls_back():
    from dmlcloud_amd.ops.fused_attn import fused_attention_usable, sdpa

    q, k, v, _ = _inputs(_n('MID'))
    ds = _doc_start('MID')
    assert fused_attention_usable(q, k, v, doc_start=ds, causal=False) is False
    out = sdpa(q, k, v, causal=False, doc_start=ds)
    same = (ds.unsqueeze(2) == ds.unsqueeze(1)).unsqueeze(1)
    ref = torch.nn.functional.scaled_dot_product_attention(q.float(), k.float(), v.float(), attn_mask=same)
    torch.testing.assert_close(out.float(), ref, rtol=3e-2, atol=3e-2)


def test_gpt2_packed_end_to_end(monkeypatch):
    """A D = 64 GPT-2 on a packed (2, 200) batch takes the native
    document-mask path, and its loss and c_attn gradients match the same
    bf16 model with the fused attention switched off (torch SDPA with the
    boolean mask)."""
    from dmlcloud_amd.models import gpt2 as gpt2_mod
    from dmlcloud_amd.models.gpt2 import GPT2, GPT2Config
    from dmlcloud_amd.ops import fused_attn

    cfg = GPT2Config(vocab_size=512, n_positions=256, n_embd=128, n_layer=2, n_head=2)
    torch.manual_seed(0)
    model = GPT2(cfg).to(DEV).to(torch.bfloat16)
    idx = torch.randint(0, cfg.vocab_size, (2, 200), device=DEV)
    doc_ids = torch.stack([_row_starts('RAGGED'), _row_starts('ONE')]).to(DEV)

    usable = []

    def spying_sdpa(q, k, v, causal=True, doc_start=None):
        usable.append(fused_attn.fused_attention_usable(q, k, v, doc_start=doc_start, causal=causal))
        assert doc_start is not None
        return fused_attn.sdpa(q, k, v, causal=causal, doc_start=doc_start)

    monkeypatch.setattr(gpt2_mod, 'sdpa', spying_sdpa)

    def run():
        model.zero_grad(set_to_none=True)
        _, loss = model(idx, targets=idx, doc_ids=doc_ids)
        loss.backward()
        return loss.item(), [blk.attn.c_attn.weight.grad.float().clone() for blk in model.blocks]

    loss_native, grads_native = run()
    assert usable == [True] * cfg.n_layer

    monkeypatch.setenv('DMLCLOUD_DISABLE_FUSED_ATTN', '1')
    loss_torch, grads_torch = run()
    assert usable == [True] * cfg.n_layer + [False] * cfg.n_layer

    assert loss_native == pytest.approx(loss_torch, rel=5e-2)
    for got, want in zip(grads_native, grads_torch):
        assert torch.isfinite(got).all()
        # 5e-2 relative, with an absolute floor scaled to the tensor so
        # bf16 rounding of near-zero elements does not decide the test
        torch.testing.assert_close(got, want, rtol=5e-2, atol=5e-2 * want.abs().max().item())


def test_graph_capture_reads_doc_start_at_replay():
    """One forward + backward captured in a hipGraph with the MID layout
    in the doc_start buffer, replayed after EDGES was copied into the same
    buffer: the replay must give the EDGES result, i.e. the mask is read
    on the device at replay and nothing about it is baked in at capture."""
    from dmlcloud_amd.ops.fused_attn import sdpa

    n = 256
    q, k, v, do = _inputs(n)
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    ds_buf = _doc_start('MID').clone()

    def step():
        out = sdpa(q, k, v, causal=True, doc_start=ds_buf)
        return (out,) + torch.autograd.grad(out, (q, k, v), do)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()

    ds_buf.copy_(_doc_start('EDGES'))
    graph.replay()
    torch.cuda.synchronize()

    for got, want in zip(captured, _native('EDGES')):
        assert torch.equal(got, want)
    assert not torch.equal(captured[0], _native('MID')[0])
