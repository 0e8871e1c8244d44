"""Value regimes, an fp64 oracle with per-element error scales, and a CPU
emulation of the attention kernels' roundings. CPU only; shared by
test_attention_values_ref.py (which tests this checker) and
test_gpu_attention_values.py (which points it at the HIP kernels).
docs/KERNELS.md, "Value regimes", has the table and the derivations.

Regimes. Each is a function (n_q, n_k, D, generator, lead_q, lead_k) ->
bf16 (q [*lead_q, n_q, D], k and v [*lead_k, n_k, D], dO like q), drawn in
that order. u = e_0, i = the query row (within its chunk), j = the absolute
key index, g_i = 1 + (i % 16) / 4 (one gain per row of a 16-row fragment):

    flat    q = k = v = randn * .5: near-uniform softmax, the control
    peaked  q = randn * 4, k = randn, v = 1 + randn * .5: a few keys per row
    rising  q = randn * .5 + 8 g_i u, k = randn * .5 + (j / 8) u, v as peaked:
            the maximum moves in every tile, alpha << 1
    sink    q as rising, k = randn * .5, + 16 u for key 0 only, v as peaked:
            key 0 dominates, the maximum never moves again
    offset  q = randn * .5 + 16 u, k = randn * .5 - 64 u, v as peaked: every
            score is ~ -128 at D = 64, only the max subtraction keeps p alive

dO = randn * .5 throughout.

Bounds. bf16 keeps 8 significant bits, so one round-to-nearest is off by at
most u = 2^-8 of the value (half the 2^-7 spacing at 1.0; the 2^-9 sometimes
quoted is the average case). Every conversion of P, dS and the outputs in
attention.hip and the attention_*.h headers is a round-to-nearest-even cast,
none truncates, so no kernel needs a 2 u unit. Each bound is TWO such
roundings, u + u = 2^-7:

    |o - ref|   <= 2^-7 A_o,  A_o = P |V|. P is rounded to bf16 before P V (u
                   of every key's own share of A_o; the normaliser l is the sum
                   of the UNROUNDED p and takes no part in it), and o is
                   rounded on store (u |o| <= u A_o).
    |lse - ref| <= 1e-5 + D 2^-24 S_i, S_i = scale max_j |q_i| . |k_j|: an
                   f32 dot product of D exact bf16 products, then one log.
    |dX - ref|  <= 2^-7 G_dX. G_dq = scale (|dS| |K|) + scale E_i (P |K|)
                   with dS = P (dP - delta) and E_i = |dO_i| . A_o,i: dS is
                   rounded to bf16 (u) and dq on store (u), both within the
                   first term; delta = rowsum(dO O) is built from the kernel's
                   bf16 O, which the forward bound allows to be 2^-7 A_o off,
                   so delta may be 2^-7 E_i off, and that error reaches dq
                   through scale P K: the second term. G_dk is the transpose
                   with |Q|, G_dv = P^T |dO| (P rounded, dv rounded: 2 u),
                   both summed over the query heads of a K/V group.
                   What the 2^-7 does NOT grant: the second-order u^2 = 2^-16
                   and the f32 terms (the 1-ulp hardware exp2, the f32
                   rounding of a log2-domain exponent of size ~200, the
                   accumulation order), together under 1 % of the bound. An
                   element reaches them only when both of its roundings fall
                   on their worst case at once; the emulation's worst element
                   is at 0.90 of its bound (dv of a key that one row attends).
    |delta - rowsum(dO o_got)| <= D 2^-24 |dO_i| . |o_got,i|: the backward's
                   delta against the fp64 row sum over the bf16 o it was
                   GIVEN (the kernel's own), an f32 sum of D products. The
                   bounds on dq and dk cannot see a delta that is one bf16
                   ulp of one o column off: that is at most 1 / D of the
                   2^-7 E_i they must grant. This one does.

The emulation below meets all of them at every regime
(test_attention_values_ref.py prints and docs/KERNELS.md records its ratios);
no constant here is taken from a kernel's output.
"""

import math

import torch

REGIME_NAMES = ('flat', 'peaked', 'rising', 'sink', 'offset')
TENSORS = ('o', 'lse', 'delta', 'dq', 'dk', 'dv')
UNIT = 2.0**-7  # see the docstring: two bf16 roundings of 2^-8 each
LSE_ABS, LSE_DOT = 1e-5, 2.0**-24
NEG = -1e30  # the kernels' finite "minus infinity"
LOG2E, LN2 = 1.44269504, 0.69314718  # the kernels' f32 constants


# --------------------------------------------------------------- the regimes
def _randn(g, lead, n, d, std):
    return torch.randn(*lead, n, d, generator=g) * std


def _along_u(x, amount):
    """x + amount * u, `amount` one value per row (or a scalar)."""
    x[..., 0] += amount
    return x


def _gain(n_q):
    return 1 + (torch.arange(n_q) % 16) / 4


def _finish(q, k, v, g):
    do = torch.randn(q.shape, generator=g) * 0.5
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, do))


def flat(n_q, n_k, d, g, lead_q=(), lead_k=()):
    q, k, v = _randn(g, lead_q, n_q, d, 0.5), _randn(g, lead_k, n_k, d, 0.5), _randn(g, lead_k, n_k, d, 0.5)
    return _finish(q, k, v, g)


def peaked(n_q, n_k, d, g, lead_q=(), lead_k=()):
    q, k, v = _randn(g, lead_q, n_q, d, 4.0), _randn(g, lead_k, n_k, d, 1.0), 1 + _randn(g, lead_k, n_k, d, 0.5)
    return _finish(q, k, v, g)


def rising(n_q, n_k, d, g, lead_q=(), lead_k=()):
    q = _along_u(_randn(g, lead_q, n_q, d, 0.5), 8 * _gain(n_q))
    k = _along_u(_randn(g, lead_k, n_k, d, 0.5), torch.arange(n_k) / 8)
    return _finish(q, k, 1 + _randn(g, lead_k, n_k, d, 0.5), g)


SINK_STRENGTH = 16.0


def sink(n_q, n_k, d, g, lead_q=(), lead_k=()):
    q = _along_u(_randn(g, lead_q, n_q, d, 0.5), 8 * _gain(n_q))
    k = _randn(g, lead_k, n_k, d, 0.5)
    k[..., 0, 0] += SINK_STRENGTH
    return _finish(q, k, 1 + _randn(g, lead_k, n_k, d, 0.5), g)


def offset(n_q, n_k, d, g, lead_q=(), lead_k=()):
    q = _along_u(_randn(g, lead_q, n_q, d, 0.5), 16.0)
    k = _along_u(_randn(g, lead_k, n_k, d, 0.5), -64.0)
    return _finish(q, k, 1 + _randn(g, lead_k, n_k, d, 0.5), g)


REGIMES = dict(flat=flat, peaked=peaked, rising=rising, sink=sink, offset=offset)


def make_inputs(regime, b, h, hkv, n_q, n_k, d, seed):
    """bf16 q, dO [b, h, n_q, d] and k, v [b, hkv, n_k, d] of `regime`."""
    return REGIMES[regime](n_q, n_k, d, torch.Generator().manual_seed(seed), (b, h), (b, hkv))


V0 = (1.25, 1.5, 1.75, 1.5)  # bf16-exact, inside a binade: both neighbours are 2^-7 away


def sink_identity_case(b, n, d, h, hkv, causal, seed):
    """`sink` inputs with v[key 0] = V0 repeated, and the rows [b, h, n] of
    the fp64 oracle whose weight on key 0 is 1 - eps with eps < 2^-10. There
    o - v[0] = sum_j p_j (v_j - v[0]) is at most eps max|v_j - v[0]| <=
    2^-10 * 3.5, under the 2^-8 half ulp of V0's binade with an eighth of it
    to spare for a kernel's own roundings of that sum: o must be v[0] bit for
    bit, with no tolerance. Returns ((q, k, v, dO), rows, the oracle)."""
    q, k, v, do = make_inputs('sink', b, h, hkv, n, n, d, seed)
    v[:, :, 0] = torch.tensor(V0).repeat(d // 4).to(torch.bfloat16)
    assert (v.float() - v[:, :, :1].float()).abs().max() <= 3.5
    ref = oracle(q, k, v, None, causal_live(b, n, causal))
    return (q, k, v, do), (ref['P'][..., 0] > 1 - 2.0**-10).reshape(b, h, n), ref


# ----------------------------------------------------------------- the masks
def causal_live(b, n, causal=True, doc_start=None):
    """live [b, n, n] for `sdpa`: key j <= row i (causal), j >= doc_start[b, i]."""
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    live = (j <= i) if causal else torch.ones(n, n, dtype=torch.bool)
    live = live.expand(b, n, n)
    if doc_start is not None:
        live = live & (j[None] >= doc_start.long()[:, :, None])
    return live


def kvcache_live(lens, n_q, n_k, causal=True):
    """live [B, n_q, n_k] for `sdpa_kvcache`: row i sits at kv_len - n_q + i."""
    ln = torch.tensor(lens)
    last = ln[:, None] - n_q + torch.arange(n_q) if causal else (ln[:, None] - 1).expand(len(lens), n_q)
    return torch.arange(n_k)[None, None, :] <= last[:, :, None]


# ---------------------------------------------------------------- the oracle
def _grouped(t, hkv):
    b, h = t.shape[:2]
    return t.reshape(b, hkv, h // hkv, *t.shape[2:])


def oracle(q, k, v, do, live):
    """fp64 masked softmax attention of the given values, GQA by group sum;
    `live` is bool [B, n_q, n_k]. Returns a dict: o, lse, the error scales A_o
    and S, and with `do` also dq, dk, dv and G_dq, G_dk, G_dv."""
    (b, h, n_q, d), hkv = q.shape, k.shape[1]
    scale = 1.0 / math.sqrt(d)
    grad = do is not None
    qd, kd, vd = (t.double().requires_grad_(grad) for t in (q, k, v))
    qg = _grouped(qd, hkv)
    lv = live[:, None, None]
    s = (torch.einsum('bkgqd,bknd->bkgqn', qg, kd) * scale).masked_fill(~lv, -float('inf'))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum('bkgqn,bknd->bkgqd', p, vd)
    out = {}
    if grad:
        o.backward(_grouped(do.double(), hkv))
        out.update(dq=qd.grad, dk=kd.grad, dv=vd.grad)
    with torch.no_grad():
        qa, ka, va = _grouped(q.double().abs(), hkv), k.double().abs(), v.double().abs()
        a_o = torch.einsum('bkgqn,bknd->bkgqd', p, va)
        sabs = torch.einsum('bkgqd,bknd->bkgqn', qa, ka).masked_fill(~lv, 0.0).amax(-1) * scale
        out.update(o=o.detach().reshape(b, h, n_q, d), lse=lse.detach().reshape(b, h, n_q))
        out.update(A_o=a_o.reshape(b, h, n_q, d), S=sabs.reshape(b, h, n_q), P=p.detach())
        if grad:
            out['dO'] = do.double()
        if grad:
            dog = _grouped(do.double(), hkv)
            dp = torch.einsum('bkgqd,bknd->bkgqn', dog, vd.detach())
            delta = (dog * o.detach()).sum(-1, keepdim=True)
            ds = (p * (dp - delta)).abs()
            e = (dog.abs() * a_o).sum(-1, keepdim=True)  # E_i
            w = ds + e * p  # [b, hkv, g, q, n]
            out['G_dq'] = (scale * torch.einsum('bkgqn,bknd->bkgqd', w, ka)).reshape(b, h, n_q, d)
            out['G_dk'] = scale * torch.einsum('bkgqn,bkgqd->bknd', w, qa)
            out['G_dv'] = torch.einsum('bkgqn,bkgqd->bknd', p, dog.abs())
    return out


def bounds(ref, d, unit=UNIT):
    """The per-element bounds of the tensors `ref` holds."""
    out = dict(o=unit * ref['A_o'], lse=LSE_ABS + d * LSE_DOT * ref['S'])
    for name in ('dq', 'dk', 'dv'):
        if 'G_' + name in ref:
            out[name] = unit * ref['G_' + name]
    return out


def worst_ratios(got, ref, d, unit=UNIT):
    """{tensor: (max |got - ref| / bound, index of that element)} for the
    tensors of `got`. A NaN or an error where the bound is 0 counts as inf."""
    bnd, out = bounds(ref, d, unit), {}
    if 'delta' in got:  # against the o it was built from, see the docstring
        o_got = got['o'].double().cpu()
        ref = dict(ref, delta=(ref['dO'] * o_got).sum(-1))
        bnd['delta'] = d * LSE_DOT * (ref['dO'].abs() * o_got.abs()).sum(-1)
    for name, g in got.items():
        err = (g.double().cpu() - ref[name]).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd[name])
        ratio = torch.nan_to_num(ratio, nan=float('inf'))
        worst = torch.unravel_index(ratio.argmax(), ratio.shape)
        out[name] = (float(ratio[worst]), tuple(int(x) for x in worst))
    return out


def assert_within_bounds(tag, got, ref, d, unit=UNIT):
    """Prints the worst ratio per tensor; fails naming every tensor outside
    its bound with the worst element and its ratio. Returns the ratios."""
    ratios = worst_ratios(got, ref, d, unit)
    print(f'{tag}: ' + ', '.join(f'{n} {r:.3f}' for n, (r, _) in ratios.items()) + '  (max err / bound)')
    bad = [
        f'{n}: worst element {idx} is {r:.3f} x its bound (got {float(got[n][idx]):.6g}, ref {float(ref[n][idx]):.6g})'
        for n, (r, idx) in ratios.items()
        if not r <= 1.0
    ]
    assert not bad, f'{tag}: ' + '; '.join(bad)
    return ratios


def passes_old_gates(got, ref):
    """The absolute gates of attn_testlib.assert_fwd_bwd_close (3e-2 for o,
    5e-2 for the gradients, rtol = atol) on the tensors of `got`; lse is not
    gated there."""
    for name, g in got.items():
        if name in ('lse', 'delta'):
            continue
        tol = 3e-2 if name == 'o' else 5e-2
        w = ref[name]
        if not bool(((g.double() - w).abs() <= tol + tol * w.abs()).all()):
            return False
    return True


# ------------------------------------------------------------- the emulation
def _bf16(x):
    return x.to(torch.bfloat16).float()


def bf16_next_up(x):
    """The bf16 neighbour of larger magnitude, elementwise."""
    return (x.view(torch.int16) + 1).view(torch.bfloat16)


DEFECTS = ('alpha_next_row', 'rowsum_drops_last_key', 'delta_ulp', 'merge_wrong_max')


def emulate_forward(q, k, v, live, splits=None, tile=64, defect=None):
    """The kernels' forward in f32 with their roundings: 64-key tiles, log2
    domain online softmax, -1e30 for masked scores (a row whose 16-row
    fragment walks a tile that is fully masked for the row itself collects
    garbage that the first live tile wipes with alpha = 0), l from the
    unrounded p, P rounded to bf16 before P V, one partial (m, l, acc) per key
    range of `splits` merged with weights exp2(m_split - m), o rounded to
    bf16. Returns (o bf16, lse f32). `defect` seeds one of DEFECTS."""
    (b, h, n_q, d), hkv, n_k = q.shape, k.shape[1], k.shape[2]
    scale2 = (1.0 / math.sqrt(d)) * LOG2E
    qg, kf, vf = _grouped(q.float(), hkv), k.float(), v.float()
    shape = qg.shape[:-1]
    frag = torch.arange(n_q) // 16
    parts = []
    for lo, hi in splits or [(0, n_k)]:
        m, l, acc = torch.full(shape, NEG), torch.zeros(shape), torch.zeros(*shape, d)
        for j0 in range(lo, hi, tile):
            j1 = min(j0 + tile, hi)
            lv = live[:, :, j0:j1]
            rows_live = lv.any(-1)  # [b, n_q]
            # the fragment walks the tile when any of its rows has a live key in it
            padded = torch.nn.functional.pad(rows_live, (0, -n_q % 16))
            walked = padded.view(b, -1, 16).any(-1)[:, frag][:, None, None]
            if not bool(walked.any()):
                continue
            s = torch.einsum('bkgqd,bknd->bkgqn', qg, kf[:, :, j0:j1]) * scale2
            s = torch.where(lv[:, None, None], s, torch.tensor(NEG))
            m_new = torch.maximum(m, s.amax(-1))
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(s - m_new[..., None])
            ps = p[..., :-1].sum(-1) if defect == 'rowsum_drops_last_key' else p.sum(-1)
            a_o = alpha.roll(-1, -1) if defect == 'alpha_next_row' else alpha
            acc_new = acc * a_o[..., None] + torch.einsum('bkgqn,bknd->bkgqd', _bf16(p), vf[:, :, j0:j1])
            m = torch.where(walked, m_new, m)
            l = torch.where(walked, l * alpha + ps, l)
            acc = torch.where(walked[..., None], acc_new, acc)
        parts.append((m, l, acc))
    big = torch.stack([p[0] for p in parts]).amax(0)
    l, acc = torch.zeros(shape), torch.zeros(*shape, d)
    for s_idx, (pm, pl, pacc) in enumerate(parts):
        if defect == 'merge_wrong_max':
            pm = parts[(s_idx + 1) % len(parts)][0]
        w = torch.exp2(pm - big)
        l, acc = l + w * pl, acc + w[..., None] * pacc
    o = (acc / l[..., None]).to(torch.bfloat16).reshape(b, h, n_q, d)
    lse = (torch.tensor(LN2) * big + torch.log(l)).reshape(b, h, n_q)
    return o, lse


def emulate_backward(q, k, v, do, o, lse, live, defect=None):
    """The kernels' backward in f32 with their roundings: delta from the bf16
    `o`, p = exp2(s scale2 - lse2) recomputed from the f32 `lse`, P and dS
    rounded to bf16 before their matmuls (dS from the unrounded p), outputs
    rounded to bf16. The order of the f32 sums over the tiles is torch's.
    Returns (dq, dk, dv) in bf16 and delta [b, h, n_q] in f32."""
    (b, h, n_q, d), hkv = q.shape, k.shape[1]
    scale = 1.0 / math.sqrt(d)
    if defect == 'delta_ulp':  # one bf16 ulp, in one column
        o = o.clone()
        o[..., 1] = bf16_next_up(o[..., 1].contiguous())
    qg, dog, og = (_grouped(t.float(), hkv) for t in (q, do, o))
    kf, vf = k.float(), v.float()
    lse2 = _grouped(lse.float(), hkv) * LOG2E
    s2 = torch.einsum('bkgqd,bknd->bkgqn', qg, kf) * (scale * LOG2E)
    p = torch.where(live[:, None, None], torch.exp2(s2 - lse2[..., None]), torch.zeros(()))
    dp = torch.einsum('bkgqd,bknd->bkgqn', dog, vf)
    delta = (dog * og).sum(-1, keepdim=True)
    ds = _bf16(p * (dp - delta) * scale)
    dv = torch.einsum('bkgqn,bkgqd->bknd', _bf16(p), dog)
    dq = torch.einsum('bkgqn,bknd->bkgqd', ds, kf).reshape(b, h, n_q, d)
    dk = torch.einsum('bkgqn,bkgqd->bknd', ds, qg)
    return tuple(t.to(torch.bfloat16) for t in (dq, dk, dv)) + (delta.reshape(b, h, n_q),)


def emulate(inputs, live, splits=None, defect=None):
    """Forward and backward emulation of (q, k, v, dO) as a dict of TENSORS."""
    q, k, v, do = inputs
    o, lse = emulate_forward(q, k, v, live, splits, defect=defect)
    dq, dk, dv, delta = emulate_backward(q, k, v, do, o, lse, live, defect=defect)
    return dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)
