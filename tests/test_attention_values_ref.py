"""The checker of test_gpu_attention_values.py, tested on the CPU
(attn_values_lib.py: regimes, fp64 oracle, derived per-element bounds and the
f32 emulation of the kernels' roundings). N = 200, D = 64 and 128, causal and
full, H = 2 query heads on one K/V head.

1. The emulation is inside every derived bound at every regime, so the bounds
   hold for a correct kernel. Worst ratios err / bound over these cases (also
   in docs/KERNELS.md): o 0.71, lse 0.16, delta 0.02, dq 0.13, dk 0.18,
   dv 0.81; the largest lse error is 4.8e-5. On the GPU tests' own cases
   (B = 2, more heads, the document and KV-cache cases) it reaches o 0.82 and
   dv 0.90.
2. The bounds have teeth: the emulation with one seeded defect must leave them
   in `peaked`, `rising` and `offset` alike, and two of the defects pass the
   absolute 3e-2 / 5e-2 gates of attn_testlib.assert_fwd_bwd_close on `flat`,
   the only data the suite had.
3. The regimes are where they are meant to be, and far from f32's limits.
"""

import functools

import pytest
import torch

import attn_values_lib as lib

N, H, HKV = 200, 2, 1
SPLITS = [(0, 128), (128, N)]  # for the merge defect: both partials live in every row (non-causal)


@functools.lru_cache(maxsize=None)
def _case(regime, d, causal):
    inputs = lib.make_inputs(regime, 1, H, HKV, N, N, d, seed=7)
    live = lib.causal_live(1, N, causal)
    return inputs, live, lib.oracle(*inputs, live)


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('d', [64, 128])
@pytest.mark.parametrize('regime', lib.REGIME_NAMES)
def test_emulation_is_within_every_bound(regime, d, causal):
    inputs, live, ref = _case(regime, d, causal)
    lib.assert_within_bounds(f'{regime} D={d} causal={causal}', lib.emulate(inputs, live), ref, d)
    if not causal:  # the merge of two partials is as accurate as one walk
        lib.assert_within_bounds(f'{regime} D={d} two splits', lib.emulate(inputs, live, SPLITS), ref, d)


def _caught(defect, regime, d, causal):
    """(tensors outside their bound, passes the old absolute gates)."""
    inputs, live, ref = _case(regime, d, causal)
    got = lib.emulate(inputs, live, SPLITS if defect == 'merge_wrong_max' else None, defect)
    ratios = lib.worst_ratios(got, ref, d)
    print(f'{defect} {regime} D={d} causal={causal}: ' + ', '.join(f'{n} {r:.3g}' for n, (r, _) in ratios.items()))
    return {n for n, (r, _) in ratios.items() if not r <= 1.0}, lib.passes_old_gates(got, ref)


# defect -> the tensors that must leave their bound in each of peaked, rising, offset
MUST_FAIL = {
    'alpha_next_row': {'o', 'dq'},  # o, and delta's share of dq; lse and dv never see the O accumulator
    'rowsum_drops_last_key': {'o', 'lse'},
    'delta_ulp': {'delta'},  # and nothing else: 1 / D of what dq and dk must grant
    'merge_wrong_max': {'o', 'lse'},
}


@pytest.mark.parametrize('d', [64, 128])
@pytest.mark.parametrize('defect', lib.DEFECTS)
def test_seeded_defects_fail_the_bounds(defect, d):
    for causal in [False] if defect == 'merge_wrong_max' else [True, False]:
        for regime in ('peaked', 'rising', 'offset'):
            failed, _ = _caught(defect, regime, d, causal)
            assert MUST_FAIL[defect] <= failed, f'{defect} in {regime}: only {sorted(failed)} left their bounds'
        _caught(defect, 'sink', d, causal)  # printed only: its later tiles carry no weight
        failed, old_gates_pass = _caught(defect, 'flat', d, causal)
        assert failed, f'{defect}: the per-element bounds miss it on flat data'
        if defect in ('rowsum_drops_last_key', 'delta_ulp'):
            assert old_gates_pass, f'{defect}: the absolute gates were expected to let it through on flat data'
    if defect == 'delta_ulp':
        assert failed == {'delta'}  # dq and dk stay inside: why delta has a bound of its own


@pytest.mark.parametrize('d', [64, 128])
def test_old_gates_do_not_fit_the_new_regimes(d):
    """The defect-free emulation leaves the absolute 5e-2 gradient gate under
    `rising` and `offset` (dq cancels against K's common component; G_dq
    measures that), so test_gpu_attention_values.py keeps that gate for the
    gradients on `flat` only. For o the 3e-2 gate holds everywhere."""
    for regime in lib.REGIME_NAMES:
        inputs, live, ref = _case(regime, d, True)
        got = lib.emulate(inputs, live)
        assert lib.passes_old_gates(dict(o=got['o']), ref), regime
        if regime == 'flat':
            assert lib.passes_old_gates(got, ref)
        if regime in ('rising', 'offset'):
            assert not lib.passes_old_gates(dict(dq=got['dq']), ref), regime


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('d', [64, 128])
def test_regimes_are_where_they_are_meant_to_be(d, causal):
    f32_max = torch.finfo(torch.float32).max
    stats = {}
    for regime in lib.REGIME_NAMES:
        inputs, live, ref = _case(regime, d, causal)
        for name in ('o', 'lse', 'dq', 'dk', 'dv', 'A_o', 'S', 'G_dq', 'G_dk', 'G_dv'):
            assert torch.isfinite(ref[name]).all(), f'{regime}: {name} is not finite'
        # log2-domain scores against f32 and against the kernels' -1e30
        big = max(ref['lse'].abs().max().item(), ref['S'].max().item()) * lib.LOG2E
        assert big * 2.0**20 < min(f32_max, -lib.NEG), regime
        stats[regime] = ref['lse'], ref['P']
    rows = torch.arange(N)
    lse, p = stats['flat']
    n_keys = (rows + 1.0) if causal else torch.full((N,), float(N))
    assert (lse - n_keys.log()).abs().max() < 1.0  # lse ~ log(n)
    assert stats['peaked'][1].amax(-1).median() > 0.3  # one key holds a third of the typical row
    lse, p = stats['rising']
    assert 80 < lse.max() < 130  # ~117 at D = 64, ~86 at D = 128
    last = rows if causal else torch.full((N,), N - 1)
    recent = torch.arange(N)[None, :] > last[:, None] - 32
    assert ((p * recent).sum(-1)[..., 64:] > 0.8).all()  # the weight sits in the row's last 32 keys
    lse, p = stats['sink']
    assert (p[..., 0] > 1 - 2.0**-10).float().mean() >= 0.5  # key 0 carries the row, in half the rows or more
    lse, p = stats['offset']
    assert lse.max() < -70 and lse.min() > -140  # ~ -128 + log(n) at D = 64, ~ -90 at D = 128


@pytest.mark.parametrize('causal', [True, False])
@pytest.mark.parametrize('d', [64, 128])
def test_sink_identity_holds_for_the_oracle_and_the_emulation(d, causal):
    """The tolerance-free check of test_gpu_attention_values.py, on its shapes:
    SINK_STRENGTH puts at least half the rows under eps < 2^-10, and there the
    fp64 o, rounded to bf16, and the emulation's o are v[0] bit for bit."""
    b, h, hkv = 2, 4, 1
    inputs, sure, ref = lib.sink_identity_case(b, N, d, h, hkv, causal, seed=11)
    assert sure.float().mean() >= 0.5
    want = inputs[2][:, :, :1].expand(b, h, N, d)
    for o in (ref['o'].to(torch.bfloat16), lib.emulate_forward(*inputs[:3], lib.causal_live(b, N, causal))[0]):
        assert torch.equal(o[sure], want[sure])


def test_bf16_next_up_is_one_ulp():
    x = torch.tensor([1.0, 1.9921875, -0.75, 3.0], dtype=torch.bfloat16)
    assert lib.bf16_next_up(x).tolist() == [1.0078125, 2.0, -0.75390625, 3.015625]
