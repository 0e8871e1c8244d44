"""The attention kernels on data that is NOT a near-uniform softmax: the five
value regimes of attn_values_lib.py (flat, peaked, rising, sink, offset)
through `sdpa` forward and backward and through `sdpa_kvcache` (dense bf16,
paged and FP8 caches), D = 64 and 128, B = 2, every output checked element by
element against an fp64 oracle with the bounds derived in attn_values_lib.py's
docstring (docs/KERNELS.md, "Value regimes"): |o - ref| <= 2^-7 P|V|,
|lse - ref| <= 1e-5 + D 2^-24 S_i, |dX - ref| <= 2^-7 G_dX, and delta against
the row sum over the kernel's own o. Every conversion of P, dS and the outputs
in the kernels is round-to-nearest-even (`(__bf16)x`, `__float2bfloat16`):
none truncates, so every kernel is held to the one unit, 2^-7 for the two
roundings between an input and an output.
The bounds are met by the CPU emulation of the kernels' roundings
(test_attention_values_ref.py); none is fitted to a kernel's output. A failure
names the regime, the tensor, its worst element and that element's ratio to
its bound; a pass prints the worst ratio per tensor.

The absolute gates of attn_testlib.assert_fwd_bwd_close stay: 3e-2 on o in
every regime, 5e-2 on the gradients under `flat`, the data they were set for.
Under `rising` and `offset` a correct backward leaves the 5e-2 gate (dq is a
difference of terms 64 |dS| large; the emulation itself is 0.22 off,
test_attention_values_ref.py asserts it), so there the derived bounds stand
alone.

Run on an MI355X box: python -m pytest tests -m gpu
"""

import functools
import math

import pytest
import torch

import attn_values_lib as lib
from attn_testlib import assert_fwd_bwd_close, bits, carve

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B, N, CAP = 2, 200, 320
FP8, NAN8 = torch.float8_e4m3fn, 0x7F
DOC_BOUNDS = [0, 9, 70, 130, 200]  # inside a tile, across a tile edge, across the block edge
HEADS = [(2, 2), (4, 1)]
# (H, Hkv, Nq): the decode kernel (D = 64), one column tile, two tile groups
KV_CONFIGS = [(4, 4, 1), (4, 2, 5), (4, 1, 20)]
KV_LENS = lambda nq: [(nq, 300), (129, 320)]


def _seed(*parts):
    seed = 0
    for x in parts:
        seed = seed * 131 + int(x)
    return seed


# ------------------------------------------------------------------ sdpa
def _doc_start():
    ds = torch.zeros(B, N, dtype=torch.int32)  # batch row 1: a single document
    for lo, hi in zip(DOC_BOUNDS[:-1], DOC_BOUNDS[1:]):
        ds[0, lo:hi] = lo
    return ds


@functools.lru_cache(maxsize=None)
def _sdpa_case(regime, d, h, hkv, causal, doc=False):
    """bf16 (q, k, v, dO) on the CPU and their fp64 oracle; never modified."""
    inputs = lib.make_inputs(regime, B, h, hkv, N, N, d, _seed(lib.REGIME_NAMES.index(regime), d, h, hkv))
    live = lib.causal_live(B, N, causal, _doc_start() if doc else None)
    return inputs, lib.oracle(*inputs, live)


def run_with_canaries(inputs, causal, doc_start=None):
    """The direct bindings on device copies of `inputs`, every output the
    front of a larger buffer whose tail must come back untouched and whose
    front must be fully written (dk, dv in k's shape). A dict of CPU tensors."""
    from dmlcloud_amd import _C

    q, k, v, do = (t.to(DEV) for t in inputs)
    d = q.shape[-1]
    shapes = dict(o=q.shape, dq=q.shape, dk=k.shape, dv=k.shape, lse=q.shape[:3], delta=q.shape[:3])
    bufs = {
        name: carve(shape.numel(), 128 * d, torch.bfloat16, -7.5, DEV)
        if len(shape) == 4
        else carve(shape.numel(), 128, torch.float32, -12345.0, DEV)
        for name, shape in shapes.items()
    }
    before = {name: bits(flat).clone() for name, (flat, _) in bufs.items()}
    out = {name: bufs[name][1].view(shape) for name, shape in shapes.items()}
    _C.attn_fwd(q, k, v, out['o'], out['lse'], d**-0.5, causal, doc_start)
    _C.attn_bwd(
        q, k, v, do, out['o'], out['lse'], out['dq'], out['dk'], out['dv'], out['delta'].view(-1), d**-0.5, causal, doc_start
    )
    torch.cuda.synchronize()
    for name, (flat, front) in bufs.items():
        assert torch.equal(bits(flat)[front.numel() :], before[name][front.numel() :]), f'{name}: sentinel overwritten'
        assert not torch.isnan(front).any(), f'{name}: rows left unwritten'
    return {name: out[name].cpu() for name in lib.TENSORS}


def _check_sdpa(regime, d, h, hkv, causal, doc=False):
    inputs, ref = _sdpa_case(regime, d, h, hkv, causal, doc)
    got = run_with_canaries(inputs, causal, _doc_start().to(DEV) if doc else None)
    tag = f'VALUES sdpa D={d} regime={regime} H{h}/{hkv} ' + ('documents' if doc else f'causal={causal}')
    lib.assert_within_bounds(tag, got, ref, d)
    names = ('o', 'dq', 'dk', 'dv') if regime == 'flat' else ('o',)  # see the module docstring
    assert_fwd_bwd_close(tag, [got[n] for n in names], [ref[n] for n in names])


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('h,hkv', HEADS)
@pytest.mark.parametrize('d', [64, 128])
@pytest.mark.parametrize('regime', lib.REGIME_NAMES)
def test_sdpa_within_per_element_bounds(regime, d, h, hkv, causal):
    _check_sdpa(regime, d, h, hkv, causal)


@pytest.mark.parametrize('d', [64, 128])
def test_sdpa_documents_under_rising(d):
    """A document start makes the first visited tile of a row fully masked:
    the -1e30 wipe, with a real maximum ~100 above the garbage."""
    _check_sdpa('rising', d, 4, 1, True, doc=True)


# ---------------------------------------------------------------- sdpa_kvcache
def _quant(x, s):
    return (x.float() / s.view(1, -1, 1, 1)).clamp(-448, 448).to(FP8)


def _fp8_scales(hkv):
    """Per-head, distinct, no powers of two; k's are wide enough for `rising`
    (|k| up to 40 + noise must stay below 448 scale, where e4m3 saturates)."""
    steps = torch.arange(hkv, dtype=torch.float32)
    return 0.1171 + 0.0123 * steps, 0.0130 + 0.0041 * steps


@functools.lru_cache(maxsize=None)
def _kv_inputs(regime, d, h, hkv, nq, fp8=False):
    """q [B, H, Nq, d] bf16; k, v [B, Hkv, CAP, d], bf16 or e4m3 with their
    scales; the values the kernel multiplies (k, v dequantised) for the oracle."""
    seed = _seed(lib.REGIME_NAMES.index(regime), d, h, hkv, nq)
    q, k, v, _ = lib.make_inputs(regime, B, h, hkv, nq, CAP, d, seed)
    if not fp8:
        return q, k, v, None, None, k, v
    ks, vs = _fp8_scales(hkv)
    k8, v8 = _quant(k, ks), _quant(v, vs)
    assert k8.float().abs().max() < 448, 'k saturates: widen its scale'
    return q, k8, v8, ks, vs, k8.float() * ks.view(1, -1, 1, 1), v8.float() * vs.view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def _kv_oracle(regime, d, h, hkv, nq, lens, fp8=False):
    q, _, _, _, _, k, v = _kv_inputs(regime, d, h, hkv, nq, fp8)
    return lib.oracle(q, k, v, None, lib.kvcache_live(lens, nq, CAP))


def _paged(dense, lens, page, fill):
    """dense [B, Hkv, CAP, d] (device) -> (pool of B * pages + 3 pages filled
    with `fill` outside the live rows, int32 table); pages scattered by a
    fixed permutation, dead entries name a page of `fill`."""
    mp = CAP // page
    perm = torch.randperm(B * mp + 3, generator=torch.Generator().manual_seed(mp))
    table = perm[: B * mp].view(mp, B).t().contiguous()
    pool = torch.full((B * mp + 3, dense.shape[1], page, dense.shape[3]), fill, dtype=dense.dtype, device=DEV)
    for b, n in enumerate(lens):
        for p in range(mp):
            rows = min(page, n - p * page)
            if rows <= 0:
                table[b, p] = perm[-1]
            else:
                pool[table[b, p], :, :rows] = dense[b, :, p * page : p * page + rows]
    return pool, table.to(DEV, torch.int32)


def _run_kvcache(regime, d, h, hkv, nq, lens, splits, page=0, fp8=False):
    """The binding `sdpa_kvcache` would pick, called directly into canary
    buffers; NaN in every cache row at or past kv_len. (o, lse) on the CPU."""
    from dmlcloud_amd import _C

    q, k, v, ks, vs, _, _ = _kv_inputs(regime, d, h, hkv, nq, fp8)
    q = q.to(DEV)
    k, v = (t.view(torch.uint8).to(DEV).clone() if fp8 else t.to(DEV).clone() for t in (k, v))
    nan = NAN8 if fp8 else float('nan')
    for b, n in enumerate(lens):
        k[b, :, n:] = nan
        v[b, :, n:] = nan
    table = None
    if page:
        (k, table), (v, _) = _paged(k, lens, page, nan), _paged(v, lens, page, nan)
    if fp8:
        k, v, ks, vs = k.view(FP8), v.view(FP8), ks.to(DEV), vs.to(DEV)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    r, scale = h // hkv * nq, 1.0 / math.sqrt(d)
    tiled = fp8 or page or r > 16 or d == 128
    if tiled:
        assert _C.attn_decode_tiled_splits(B, hkv, r, CAP, splits, 0) == splits
        floats = _C.attn_decode_tiled_workspace_floats(B, hkv, r, splits, d)
    else:
        assert _C.attn_decode_splits(B, hkv, CAP, splits, 0) == splits
        floats = _C.attn_decode_workspace_floats(B, hkv, splits)
    bufs = {
        'o': carve(B * h * nq * d, 128 * d, torch.bfloat16, -7.5, DEV),
        'lse': carve(B * h * nq, 128, torch.float32, -12345.0, DEV),
        'ws': carve(floats, 128, torch.float32, -12345.0, DEV),
    }
    before = {name: bits(flat).clone() for name, (flat, _) in bufs.items()}
    o, lse, ws = bufs['o'][1].view(B, h, nq, d), bufs['lse'][1].view(B, h, nq), bufs['ws'][1]
    if fp8:
        _C.attn_decode_fp8(q, k, v, kv_len, o, lse, ws, scale, True, splits, ks, vs, table)
    elif tiled:
        _C.attn_decode_tiled(q, k, v, kv_len, o, lse, ws, scale, True, splits, table)
    else:
        _C.attn_decode(q, k, v, kv_len, o, lse, ws, scale, True, splits)
    torch.cuda.synchronize()
    for name, (flat, front) in bufs.items():
        assert torch.equal(bits(flat)[front.numel() :], before[name][front.numel() :]), f'{name}: sentinel overwritten'
    assert not torch.isnan(o).any() and not torch.isnan(lse).any(), 'rows left unwritten, or a dead cache row was read'
    return dict(o=o.cpu(), lse=lse.cpu())


@pytest.mark.parametrize('splits', [1, 3])
@pytest.mark.parametrize('h,hkv,nq', KV_CONFIGS)
@pytest.mark.parametrize('d', [64, 128])
@pytest.mark.parametrize('regime', lib.REGIME_NAMES)
def test_kvcache_within_per_element_bounds(regime, d, h, hkv, nq, splits):
    """Capacity 320 in three splits is keys 0..127 | 128..255 | 256..319:
    `rising` puts all the weight in the last split, `sink` in the first, and
    under `offset` every partial's maximum is ~ -128."""
    for lens in KV_LENS(nq):
        got = _run_kvcache(regime, d, h, hkv, nq, lens, splits)
        tag = f'VALUES kvcache D={d} regime={regime} H{h}/{hkv} Nq={nq} {lens} S={splits}'
        lib.assert_within_bounds(tag, got, _kv_oracle(regime, d, h, hkv, nq, lens), d)


@pytest.mark.parametrize('d', [64, 128])
def test_kvcache_paged_under_rising_is_bit_identical_to_dense(d):
    h, hkv, nq, lens = 4, 1, 20, (129, 320)
    dense = _run_kvcache('rising', d, h, hkv, nq, lens, 3)
    tiled = _run_kvcache('rising', d, h, hkv, nq, lens, 3, page=64)
    lib.assert_within_bounds(f'VALUES paged D={d} regime=rising', tiled, _kv_oracle('rising', d, h, hkv, nq, lens), d)
    assert torch.equal(bits(dense['o']), bits(tiled['o'])) and torch.equal(bits(dense['lse']), bits(tiled['lse']))


@pytest.mark.parametrize('d', [64, 128])
def test_kvcache_fp8_under_rising(d):
    """The oracle runs over the dequantised cache, which is exactly what the
    kernel multiplies (e4m3 -> bf16 is exact): the bf16 bounds, no margin."""
    h, hkv, nq, lens = 4, 2, 5, (129, 320)
    got = _run_kvcache('rising', d, h, hkv, nq, lens, 3, fp8=True)
    lib.assert_within_bounds(f'VALUES fp8 D={d} regime=rising', got, _kv_oracle('rising', d, h, hkv, nq, lens, True), d)


# ------------------------------------------------------ an identity with no tolerance
@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('d', [64, 128])
def test_sink_rows_return_v0_bit_for_bit(d, causal):
    """attn_values_lib.sink_identity_case: where the fp64 weight on key 0 is
    above 1 - 2^-10, o must be v[0] exactly."""
    h, hkv = 4, 1
    inputs, sure, _ = lib.sink_identity_case(B, N, d, h, hkv, causal, _seed(4, d, h, hkv))
    assert sure.float().mean() >= 0.5, 'the condition must cover at least half the rows'
    got = run_with_canaries(inputs, causal)
    want = inputs[2][:, :, :1].repeat_interleave(h // hkv, 1).expand(B, h, N, d)
    wrong = (bits(got['o']) != bits(want)).any(-1) & sure
    print(f'VALUES identity D={d} causal={causal}: {int(sure.sum())} of {sure.numel()} rows must equal v[0]')
    assert not wrong.any(), f'{int(wrong.sum())} rows differ from v[0], first at {wrong.nonzero()[0].tolist()}'
