"""The temporal encoder stage by stage (plain torch on the CPU): an fp64 restatement of every stage tepose_encoder_tap can copy out of a finished forward,
the componentwise bound of each, and the checker tests/test_gpu_encoder_stages.py runs over the taps.  tests/test_encoder_stages_helper.py checks this
file on its own (no GPU).  Modelled on tests/_hmr_layers.py: every stage is judged IN ISOLATION -- its fp64 reference is computed from the taps of the
stages before it, not from the oracle's own chain -- so a stage's error is the error of the one kernel that made it, no bound is propagated through
time, and the report names stage, layer, direction, step, row and unit.

Stages (include/tepose_amd.h; directions 0 gru_fwd, 1 gru_rec reverse, 2 gru_rec forward; Hp = H rounded up to 64, gate g of unit u at column g Hp + u):
    gi(0, d)[t]        = x[:, t] W_ih^T + b_ih                                   from the caller's windows, frame order
    gi(l >= 1, d)[s]   = a_s W_ih^T + b_ih,  a_s = h(l-1, 0, s)  (d = 0)  |  [h(l-1, 2, s) | h(l-1, 1, T-1-s)]  (d = 1, 2)        from the tapped states
    h(l, d, st)        = oracle.tepose_ref.gru_cell(gi(l, d)[slab(st)], h(l, d, st-1)) in fp64, from the tapped gi and the tapped previous state (zero at st = 0);
                         slab(st) = st, T-1-st, st for d = 0, 1, 2 on layers >= 1 and frame st, st, T-1-st on layer 0 (the top layer's d = 2: its one slab)
    tail               = relu[h(top, 0, T-1) | h(top, 2, 0) | h(top, 1, T-1)]
    feature            = (tail [W_lf | W_lr]^T + b_lf + b_lr) / 2                from the tapped tail
Only what survives a forward can be tapped (csrc/tap.h).  Where a layer's gi did not survive (the middle layer of a 3-layer model) its cell steps are checked
against gi computed in fp64 from the tapped states below, and the product bound of that gi enters the step's bound as e_gi next to e_g.  A top-layer step
whose previous state did not survive (every step but T-1, and T-2 = 0) is only checked for finiteness and its pad columns.

Bounds (u = 2^-24; none is tuned on a kernel).
  Products  |y - y64| <= c A,  A = |a| |W|^T + |b|  (as tests/test_gpu_range.py asserts it for the product kernels alone):
        exact fp32 kernels   c = K u                                  K = the padded K the kernel runs (2144, Hp, 2 Hp, 3 Hp): one rounding per fmaf
        split kernels        c = 3 * 2^-22 + n_acc u                  operand halves (2 x 2^-22) and the dropped lo x lo term; n_acc = 3 K / 16 + 16 fp32
                             roundings per accumulator of the tiled kernels, + 8 where 8 (or 4) waves' K-partial sums are added: gru_seq_kernel (gru_seq.hip
                             NW = 8) and the width-first kernels (skinny_h3.hip)
        scale-1 input planes (gemm_h3s_kernel, gemm_h3s_persist16c_kernel<0> on layer 0; forward.hip "elements below 2^-3 keep an absolute error <= 2^-25"):
                             the row is scaled to [2^13, 2^14) first (gemm_h3.hip split_rows_kernel), so in the caller's units the absolute term is
                             <= 2^-38 max|x_row| per element: + 2^-38 max|x_row| sum_k |W_jk|
        the feature          as a product of K = 3 Hp (+ 4 in exact mode: two chains, their sum, two bias adds); the halving is exact
  Cell step, from e_g = c A on gh = h_prev W_hh^T + b_hh (0 at a first step: gh = b_hh), e_gi (0 where gi was tapped), eps = 3e-7 the absolute accuracy
  csrc/device.h:18-20 states for a gate on the exp2 / rcp forms, pre_x = gi_x + gh_x:
        sigma' <= 1/4:   dr, dz <= (e_g + e_gi + u |pre|) / 4 + eps                      (u |pre|: the rounding of the sum gi + gh)
        tanh' <= 1:      dn <= |gh_n| dr + e_g + e_gi + 2 u (|gi_n| + |r gh_n|) + eps    (the product r gh_n and the sum, one rounding each on either term)
        h = n + z (h_prev - n):   dh <= |n - h_prev| dz + (1 - z) dn + 3 u (|n| + |h_prev|)   (three roundings of (1 - z) n + z h_prev, each on a value <= |n| + |h_prev|)
        + 2^-22 |h| where the value is read from hi + lo planes (22 significant bits: gru_step16_kernel<true> writes no fp32 state)
  Exact facts: columns H .. Hp of every state and of every gate of every gi are 0 (pad weights and biases are zero, so h = 0 / 2 + h_prev / 2 = 0);
  tail == relu(final states) in fp32, or to 2^-22 |h| + 2^-36 where it lives in planes (the low half's fp16 subnormal step 2^-24, halved, / 2048).
  Everything finite: the GPU test poisons its workspace with 0xFF bytes, a place no kernel wrote reads as NaN and scores infinity.
"""
import collections

import torch

from oracle import tepose_ref as O

U = 2.0 ** -24
EPS_GATE = 3e-7
DIRS = ('gru_fwd', 'gru_rec reverse', 'gru_rec forward')
_KEYS = ('gru_fwd.%s_l%d', 'gru_rec.%s_l%d_reverse', 'gru_rec.%s_l%d')
FORMS = ('rows', 'state blocks', 'gi blocks', 'planes32', 'planes16')
PLANES = (3, 4)
EXACT_KERNELS = {'gemm_f32_kernel', 'skinny_gemm_kernel', 'gru_step_kernel', 'skinny_gru_kernel'}
SCALE1_KERNELS = {'gemm_h3s_kernel<1, 3, 4, 3, 4>', 'gemm_h3s_persist16c_kernel<0>'}
KIN = 2133
KIN_P = 2144

Taps = collections.namedtuple('Taps', 'gi h tail feat')     # gi[(l, d)] = ([S, B, 3Hp], form); h[(l, d, st)] = ([B, Hp], form); tail = ([B, 3Hp], form); feat [B, 2048]


def hp_of(H):
    return (H + 63) // 64 * 64


def n_dirs(L, l):
    return 2 if l == L - 1 else 3


def gi_slab(L, T, l, d, st):
    if d == 2 and l == L - 1:
        return 0
    return ((st, st, T - 1 - st) if l == 0 else (st, T - 1 - st, st))[d]


def gi_slabs(L, T, l, d):
    return 1 if d == 2 and l == L - 1 else T


def surviving(L, T):
    """What tepose_encoder_tap can return after a forward, in execution order: ('gi', l, d, None) | ('h', l, d, st) | ('tail', ...)."""
    out = []
    for l in range(L):
        top = l == L - 1
        if l == 0 or top:
            out += [('gi', l, d, None) for d in range(3)]
        for st in range(T):
            for d in range(n_dirs(L, l)):
                if (top and st >= T - 2) or (not top and not l + 2 < L - 1):
                    out.append(('h', l, d, st))
        if top:
            out.append(('h', l, 2, 0))
    return out + [('tail', L - 1, None, None)]


def coef(K, kernel):
    """c of |y - y64| <= c A for a product of (padded) depth K on `kernel` (a name of csrc/plan.hip)."""
    if kernel in EXACT_KERNELS:
        return K * U
    return 3 * 2.0 ** -22 + (3 * K / 16 + 16 + (8 if 'skinny' in kernel or 'gru_seq' in kernel else 0)) * U


def _w(enc, what, l, d):
    return enc[_KEYS[d] % (what, l)]


def _gates(t, H, Hp):
    """[..., 3 Hp] -> the real units [..., 3, H] and the pad columns [..., 3, Hp - H]"""
    g = t.reshape(*t.shape[:-1], 3, Hp)
    return g[..., :H], g[..., H:]


class StageMismatch(AssertionError):
    def __init__(self, failures):
        self.failures = failures
        more = '' if len(failures) <= 8 else '\n... and %d more' % (len(failures) - 8)
        super().__init__('%d stage(s) failed, first: %s\n%s%s' % (len(failures), failures[0]['name'], '\n'.join(format_record(f) for f in failures[:8]), more))


def _name(stage, l, d, st):
    if stage in ('tail', 'feature'):
        return stage
    return '%s(layer %d, %s%s)' % (stage, l, DIRS[d], '' if st is None else ', step %d' % st)


def _record(stage, l, d, st, kernel, form, ratio, shape_names, note=''):
    """ratio: error / bound per element (NaN = not finite = infinite); the record holds its maximum and where it is."""
    r = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)
    at = int(torch.argmax(r))
    loc = []
    for n in reversed(r.shape):
        loc.append(at % n)
        at //= n
    loc = dict(zip(shape_names, reversed(loc)))
    return {'stage': stage, 'layer': l, 'dir': d, 'step': st, 'name': _name(stage, l, d, st), 'kernel': kernel, 'form': form, 'ratio': float(r.max()),
            'loc': loc, 'n_bad': int((~(r <= 1.0)).sum()), 'n': r.numel(), 'note': note}


def format_record(r):
    loc = ', '.join('%s %d' % kv for kv in r['loc'].items())
    return '%-46s %-34s %-12s worst error / bound %9.4f at (%s)%s%s' % (r['name'], r['kernel'], r['form'], r['ratio'], loc,
                                                                      '; %d of %d over' % (r['n_bad'], r['n']) if r['n_bad'] else '', r['note'])


def format_records(records, tag=''):
    lines = ['%s%s' % (tag, format_record(r)) for r in records]
    worst = max(records, key=lambda r: r['ratio'])
    lines.append('%sworst: %s %.4f' % (tag, worst['name'], worst['ratio']))
    return lines


def _pad_inf(ratio, pad):
    """pad columns must be exactly 0: a row with a non-zero (or non-finite) pad column scores infinity.  pad [..., P] with ratio's leading dimensions"""
    if pad.shape[-1] == 0:
        return ratio
    bad = (~(pad == 0)).any(-1)
    while bad.dim() < ratio.dim():
        bad = bad.unsqueeze(-1)
    return torch.where(bad, torch.full_like(ratio, float('inf')), ratio)


def check_stages(taps, state, x, L, H, plan, raise_on_fail=True):
    """Every tapped stage against its fp64 restatement (module docstring).  state: the reference-keyed numpy state dict; x [B, T, 2133]; plan: the
    dict of tepose_select_kernels for this shape (which kernel made a stage decides c).  Returns the records in execution order; raises StageMismatch
    (its failures in the same order) unless raise_on_fail is False, in which case (records, failures) is returned."""
    enc = O.split_state_dict(state, torch.float64)[0]
    x = torch.as_tensor(x).double()
    B, T = int(x.shape[0]), int(x.shape[1])
    Hp = hp_of(H)
    records = []
    h64 = lambda l, d, st: taps.h[(l, d, st)][0][:, :H].double()

    def gi_ref(l, d, s):
        """fp64 gi(l, d)[s] as [B, 3, H], its magnitude A, the kernel that makes it, its K and the absolute term of the scale-1 input planes"""
        top = l == L - 1
        W, b = _w(enc, 'weight_ih', l, d), _w(enc, 'bias_ih', l, d)
        extra = 0.0
        if l == 0:
            a = x[:, T - 1 if (top and d == 2) else s]
            kernel, K = (plan['projection_one_step'] if top and d == 2 else plan['projection']), KIN_P
            if kernel in SCALE1_KERNELS:
                extra = 2.0 ** -38 * a.abs().max(dim=1, keepdim=True).values * W.abs().sum(dim=1)[None]
        else:
            a = h64(l - 1, 0, s) if d == 0 else torch.cat([h64(l - 1, 2, s), h64(l - 1, 1, T - 1 - s)], dim=1)
            kernel, K = (plan['projection_one_step'] if top and d == 2 else plan['projection_l1']), (Hp if d == 0 else 2 * Hp)
        y = a @ W.t() + b
        bound = coef(K, kernel) * (a.abs() @ W.abs().t() + b.abs()) + extra
        return y.reshape(B, 3, H), bound.reshape(B, 3, H), kernel

    for stage, l, d, st in surviving(L, T):
        if stage == 'gi':
            g, gform = taps.gi[(l, d)]
            S = gi_slabs(L, T, l, d)
            assert tuple(g.shape) == (S, B, 3 * Hp), (l, d, tuple(g.shape))
            real, pad = _gates(g, H, Hp)
            ref = [gi_ref(l, d, s) for s in range(S)]
            ratio = (real.double() - torch.stack([r[0] for r in ref])).abs() / torch.stack([r[1] for r in ref]).clamp_min(1e-300)
            ratio = _pad_inf(ratio, pad.reshape(S, B, -1))
            records.append(_record('gi', l, d, None, ref[0][2], FORMS[gform], ratio, ('slab', 'row', 'gate', 'unit')))
        elif stage == 'h':
            hv, form = taps.h[(l, d, st)]
            assert tuple(hv.shape) == (B, Hp), (l, d, st, tuple(hv.shape))
            first = st == 0
            kernel = plan['gru_first'] if first else plan['gru_step' if l == 0 else 'gru_step_l1']
            got, pad = hv[:, :H].double(), hv[:, H:]
            no_prev = not first and (l, d, st - 1) not in taps.h
            if no_prev or ((l, d) not in taps.gi and (l - 1, 0, 0) not in taps.h):           # (the latter: a layer two below the top of a 4-layer model)
                ratio = torch.where(torch.isfinite(got), torch.zeros_like(got), torch.full_like(got, float('inf')))
                records.append(_record('h', l, d, st, kernel, FORMS[form], _pad_inf(ratio, pad), ('row', 'unit'),
                                       '  [%s not kept: finite and pads only]' % ('previous state' if no_prev else 'inputs')))
                continue
            s = gi_slab(L, T, l, d, st)
            if (l, d) in taps.gi:
                gi, e_gi = _gates(taps.gi[(l, d)][0][s], H, Hp)[0].double(), torch.zeros(B, 3, H, dtype=torch.float64)
            else:
                gi, e_gi, _ = gi_ref(l, d, s)
            Whh, bhh = _w(enc, 'weight_hh', l, d), _w(enc, 'bias_hh', l, d)
            hprev = torch.zeros(B, H, dtype=torch.float64) if first else h64(l, d, st - 1)
            gh = (hprev @ Whh.t() + bhh).reshape(B, 3, H)
            e_g = torch.zeros_like(gh) if first else (coef(Hp, kernel) * (hprev.abs() @ Whh.abs().t() + bhh.abs())).reshape(B, 3, H)
            want = O.gru_cell(gi.reshape(B, 3 * H), hprev, Whh, bhh)
            pre = gi + gh
            r, z = torch.sigmoid(pre[:, 0]), torch.sigmoid(pre[:, 1])
            n = torch.tanh(gi[:, 2] + r * gh[:, 2])
            e = e_g + e_gi
            dr = (e[:, 0] + U * pre[:, 0].abs()) / 4 + EPS_GATE
            dz = (e[:, 1] + U * pre[:, 1].abs()) / 4 + EPS_GATE
            dn = gh[:, 2].abs() * dr + e[:, 2] + 2 * U * (gi[:, 2].abs() + (r * gh[:, 2]).abs()) + EPS_GATE
            bound = (n - hprev).abs() * dz + (1 - z) * dn + 3 * U * (n.abs() + hprev.abs())
            if form in PLANES:
                bound = bound + 2.0 ** -22 * want.abs()
            ratio = _pad_inf((got - want).abs() / bound, pad)
            records.append(_record('h', l, d, st, kernel, FORMS[form], ratio, ('row', 'unit')))
        else:
            tv, form = taps.tail
            assert tuple(tv.shape) == (B, 3 * Hp), tuple(tv.shape)
            fin = torch.cat([taps.h[(L - 1, 0, T - 1)][0], taps.h[(L - 1, 2, 0)][0], taps.h[(L - 1, 1, T - 1)][0]], dim=1).clamp_min(0)
            if form in PLANES:
                ratio = (tv.double() - fin.double()).abs() / (2.0 ** -22 * fin.double().abs() + 2.0 ** -36)
            else:
                ratio = torch.where(tv == fin, torch.zeros(B, 3 * Hp, dtype=torch.float64), torch.full((B, 3 * Hp), float('inf'), dtype=torch.float64))
            records.append(_record('tail', L - 1, None, None, 'relu of the final states', FORMS[form], ratio, ('row', 'column')))
            # ---- the feature from the tapped tail
            a = _gates(tv, H, Hp)[0].double()                                  # [B, 3, H]: relu[fwd | rec forward | rec reverse]
            Wf, Wr = enc['linear_fwd.weight'], enc['linear_rec.weight']         # [2048, H], [2048, 2H]
            bf, br = enc['linear_fwd.bias'], enc['linear_rec.bias']
            ar = a[:, 1:].reshape(B, 2 * H)
            want = (a[:, 0] @ Wf.t() + bf + ar @ Wr.t() + br) / 2
            A = (a[:, 0].abs() @ Wf.abs().t() + bf.abs() + ar.abs() @ Wr.abs().t() + br.abs()) / 2
            exact = plan['projection'] in EXACT_KERNELS
            c = (3 * Hp + 4) * U if exact else coef(3 * Hp, 'skinny_gemm_h3_kernel')
            ratio = (taps.feat.double() - want).abs() / (c * A)
            records.append(_record('feature', L - 1, None, None, 'tail product', 'rows', ratio, ('row', 'column')))
    failures = [r for r in records if not r['ratio'] <= 1.0]
    if not raise_on_fail:
        return records, failures
    if failures:
        raise StageMismatch(failures)
    return records


# ---- the stand-in for a device: what the taps would hold, had torch computed the forward in fp32 on the CPU ------------------------------------------
def split22(t):
    """an fp32 tensor rounded to its hi + lo fp16 halves as the split kernels' operands are (csrc/common.h split_hi_lo)"""
    hi = t.half().float()
    return hi + ((t - hi) * 2048.0).half().float() / 2048.0


def standin_taps(state, x, L, H, split):
    """Taps of an fp32 emulation: torch fp32 products and cells; split: every product's operands rounded to 22 bits first.  Pad columns are zero, every
    form is 'rows' (the tail: planes in split mode), and only what survives a forward is kept."""
    enc = O.split_state_dict(state, torch.float32)[0]
    x = torch.as_tensor(x).float()
    B, T = int(x.shape[0]), int(x.shape[1])
    Hp = hp_of(H)
    q = split22 if split else (lambda t: t)
    padg = lambda g: torch.nn.functional.pad(g.reshape(*g.shape[:-1], 3, H), (0, Hp - H)).reshape(*g.shape[:-1], 3 * Hp)
    padh = lambda h: torch.nn.functional.pad(h, (0, Hp - H))
    keep = set(surviving(L, T))
    gi_t, h_t = {}, {}
    below = None
    for l in range(L):
        top = l == L - 1
        gis = {}
        for d in range(3):
            W, b = q(_w(enc, 'weight_ih', l, d)), _w(enc, 'bias_ih', l, d)
            S = gi_slabs(L, T, l, d)
            if l == 0:
                a = [x[:, T - 1 if (top and d == 2) else s] for s in range(S)]
            else:
                a = [below[(0, s)] if d == 0 else torch.cat([below[(2, s)], below[(1, T - 1 - s)]], dim=1) for s in range(S)]
            gis[d] = torch.stack([q(v) @ W.t() + b for v in a])
            if ('gi', l, d, None) in keep:
                gi_t[(l, d)] = (padg(gis[d]), 0)
        cur = {}
        for d in range(3):
            Whh, bhh = _w(enc, 'weight_hh', l, d), _w(enc, 'bias_hh', l, d)
            h = torch.zeros(B, H)
            for st in range(1 if (top and d == 2) else T):
                g = gis[d][gi_slab(L, T, l, d, st)]
                gh = q(h) @ q(Whh).t() + bhh if st else bhh.expand(B, 3 * H)       # the product takes the rounded operands, the blend the fp32 state
                r, z = torch.sigmoid(g[:, :H] + gh[:, :H]), torch.sigmoid(g[:, H:2 * H] + gh[:, H:2 * H])
                h = (1 - z) * torch.tanh(g[:, 2 * H:] + r * gh[:, 2 * H:]) + z * h
                cur[(d, st)] = h
                if ('h', l, d, st) in keep:
                    h_t[(l, d, st)] = (padh(h), 0)
        below = cur
    tail = torch.cat([h_t[(L - 1, 0, T - 1)][0], h_t[(L - 1, 2, 0)][0], h_t[(L - 1, 1, T - 1)][0]], dim=1).clamp_min(0)
    tail = q(tail)
    a = _gates(tail, H, Hp)[0]
    feat = (q(a[:, 0]) @ q(enc['linear_fwd.weight']).t() + enc['linear_fwd.bias'] + q(a[:, 1:].reshape(B, 2 * H)) @ q(enc['linear_rec.weight']).t()
            + enc['linear_rec.bias']) / 2
    return Taps(gi_t, h_t, (tail, 3 if split else 0), feat)


def standin_plan(L, split):
    """a plan as tepose_select_kernels words it, for the emulation: the tiled split kernels, or the exact ones"""
    p = {'projection': 'gemm_h3_kernel', 'projection_one_step': 'gemm_h3_kernel', 'gru_step': 'gemm_h3_kernel<GRU>', 'gru_first': 'gru_first_kernel'} if split else \
        {'projection': 'gemm_f32_kernel', 'projection_one_step': 'gemm_f32_kernel', 'gru_step': 'gru_step_kernel', 'gru_first': 'gru_step_kernel'}
    if L >= 2:
        p.update(projection_l1=p['projection'], gru_step_l1=p['gru_step'])
    return p
