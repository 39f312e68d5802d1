"""The HMR backbone layer by layer (plain torch on the CPU): an independent restatement of the network, its fp64 walk, and the checker that
tests/test_gpu_hmr_layers.py runs over the tensors tepose_hmr_features_upto copies out -- every element of every one of the 53 convolution
outputs against an fp64 restatement of THAT layer, whose input is built from the device's own earlier tensors.  An error therefore stays where it
was made: it is not divided by the widths, map areas and the 49-pixel average of everything that follows, and the report names the layer.
tests/test_hmr_layers_helper.py checks this file on its own (no GPU).

What the device keeps (csrc/hmr.h): every convolution output BEFORE its ReLU in T_A / T_B / T_C / T_D (conv1 / conv2 / conv3 / downsample of a
block; the stem writes T_C), and the block input T_J = the max-pooled stem, then relu(conv3 + identity) as conv1 of the next block writes it back.

Per convolution i, with `x` its input promoted to fp64 (the image; relu(T_A) or relu(T_B); the tapped T_J), wf / bf the folded weights and shift,
K = C_in R^2:
    y64 = conv64(x, wf) + bf          A = conv64(|x|, |wf|) + |bf|
    |y - y64| <= ((K + 3) 2^-24 + (0 if exact else 2^-21)) A          for EVERY element
the bound of tests/test_gpu_conv.py (derived there; bound_c / conv_ref are that file's) plus one 2^-24: the library folds the batch norm on the
device, this file on the host, both in fp64 rounded once to fp32, and the two may differ by that one rounding (sqrt, or a fused multiply).

Without tolerance (one fp32 add and a select, or a maximum: nothing to round differently, nothing to contract):
    T_J tapped at convolution 0             == max_pool2d(relu(T_C), 3, 2, 1)
    T_J tapped at conv1 of a later block    == relu(T_C + identity) in fp32, identity = the T_J before (J_IDENT) or T_D (J_DOWN)
    T_J tapped anywhere else                == the T_J tapped one convolution earlier (no launch writes it)
and the features:  |feat - mean64(relu(T_C + T_J))| <= 50 * 2^-24 * max|.|  (test_avgpool7's bound; the fp32 add is one more of its 50 roundings).
"""
import collections

import torch
import torch.nn.functional as F

from test_gpu_conv import bound_c, conv_ref

STAGES = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))          # planes, blocks, stride of the first block's 3 x 3
IMAGE = 224
Layer = collections.namedtuple('Layer', 'idx name cin cout R stride pad src out join hin hout jshape')


def _out_size(h, R, stride, pad):
    return (h + 2 * pad - R) // stride + 1


def network():
    """The 53 convolutions in state-dict order.  src: 'img' | 'J' | 'A' | 'B' (A / B are read through a ReLU); out: 'A' .. 'D';
    join: None | 'ident' | 'down' -- what conv1 of a block adds to T_C to make its input; jshape: (h, c) of T_J once this convolution has run."""
    net, hw = [], {'img': IMAGE}
    state = {'join': None, 'j': None}

    def add(name, cin, cout, R, stride, src, out, join=None):
        if join:
            hw['J'] = hw['C']
            state['j'] = (hw['C'], cin)
        hin = hw[src]
        hw[out] = _out_size(hin, R, stride, R // 2)
        if not net:                                                  # the max pool belongs to the stem
            hw['J'] = _out_size(hw[out], 3, 2, 1)
            state['j'] = (hw['J'], cout)
        net.append(Layer(len(net), name, cin, cout, R, stride, R // 2, src, out, join, hin, hw[out], state['j']))

    add('conv1', 3, 64, 7, 2, 'img', 'C')
    inplanes = 64
    for s, (planes, blocks, stride) in enumerate(STAGES):
        for b in range(blocks):
            p = 'layer%d.%d.' % (s + 1, b)
            add(p + 'conv1', inplanes, planes, 1, 1, 'J', 'A', state['join'])
            add(p + 'conv2', planes, planes, 3, stride if b == 0 else 1, 'A', 'B')
            add(p + 'conv3', planes, 4 * planes, 1, 1, 'B', 'C')
            state['join'] = 'ident'
            if b == 0:
                add(p + 'downsample.0', inplanes, 4 * planes, 1, stride, 'J', 'D')
                state['join'] = 'down'
            inplanes = 4 * planes
    return net, state['join']


NET, FINAL_JOIN = network()


def out_count(i, N):
    return N * NET[i].hout ** 2 * NET[i].cout


def joined_count(i, N):
    h, c = NET[i].jshape
    return N * h * h * c


def kp(layer):
    return -(-layer.cin * layer.R ** 2 // 32) * 32


def fold(pairs, round32=True):
    """[(wf, bf)] of model.conv_bn_pairs(): w gamma / sqrt(var + 1e-5), beta - mean gamma / sqrt(var + 1e-5) in fp64, rounded once to fp32 as the
    library does (round32=False keeps fp64: what the reference's own fp64 run computes with)."""
    out = []
    for conv, bn in pairs:
        sc = bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.detach().cpu().double() + 1e-5)
        w = conv.weight.detach().cpu().double() * sc[:, None, None, None]
        b = bn.bias.detach().cpu().double() - bn.running_mean.detach().cpu().double() * sc
        out.append((w.float(), b.float()) if round32 else (w, b))
    return out


Taps = collections.namedtuple('Taps', 'out joined feat')              # out[i], joined[i]: NHWC fp32 as tapped after convolution i; feat [N, 2048]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _walk(weights, images, dtype, keep):
    t, outs, joins, jn = {}, [], [], None
    x = images.to(dtype)
    for L in NET:
        w, b = (v.to(dtype) for v in weights[L.idx])
        assert tuple(w.shape) == (L.cout, L.cin, L.R, L.R), (L.name, tuple(w.shape))
        if L.join:
            t['J'] = (t['C'] + (t['J'] if L.join == 'ident' else t['D'])).clamp_min(0)
            jn = None
        a = x if L.src == 'img' else (t['J'] if L.src == 'J' else t[L.src].clamp_min(0))
        t[L.out] = F.conv2d(a, w, b, stride=L.stride, padding=L.pad)
        if L.idx == 0:
            t['J'] = F.max_pool2d(t['C'].clamp_min(0), 3, 2, 1)
        if keep:
            jn = _nhwc(t['J']) if jn is None else jn
            outs.append(_nhwc(t[L.out]))
            joins.append(jn)
    feat = (t['C'] + (t['J'] if FINAL_JOIN == 'ident' else t['D'])).clamp_min(0).mean(dim=(2, 3))
    return Taps(outs, joins, feat)


def walk64(weights, images):
    """The whole network in fp64: images [N, 3, 224, 224] -> features [N, 2048]."""
    return _walk(weights, images, torch.float64, False).feat


def standin_taps(weights, images):
    """What a device would hand over, had it computed in fp32 torch on the CPU: every convolution output, join and pool kept."""
    return _walk(weights, images, torch.float32, True)


class LayerMismatch(AssertionError):
    def __init__(self, failures):
        self.failures = failures
        more = '' if len(failures) <= 6 else '\n... and %d more' % (len(failures) - 6)
        super().__init__('%d check(s) failed, first at convolution %d (%s):\n%s%s' % (len(failures), failures[0]['conv'], failures[0]['name'],
                                                                                        '\n'.join(f['msg'] for f in failures[:6]), more))


def _worst(L, kind, score, bad, got, want, what):
    """The failure record of one check: `score` (error / bound, or |difference| for the exact checks; NaN counts as infinite) at its worst element."""
    score = torch.where(torch.isnan(score), torch.full_like(score, float('inf')), score)
    at = int(torch.argmax(score))
    n, oh, ow, c = (int(v) for v in (at // (score.shape[1] * score.shape[2] * score.shape[3]), at // (score.shape[2] * score.shape[3]) % score.shape[1],
                                     at // score.shape[3] % score.shape[2], at % score.shape[3]))
    border = oh in (0, score.shape[1] - 1) or ow in (0, score.shape[2] - 1)
    f = {'kind': kind, 'conv': L.idx, 'name': L.name, 'loc': (n, oh, ow, c), 'ratio': float(score.flatten()[at]), 'border': border, 'n_bad': int(bad.sum())}
    f['msg'] = ('  convolution %d (%s) %s: worst at (n=%d, oh=%d, ow=%d, c=%d), %s the border of the %d x %d map: %s = %.4g (got %r, want %r); %d of %d elements fail'
                % (L.idx, L.name, kind, n, oh, ow, c, 'on' if border else 'off', score.shape[1], score.shape[2], what, f['ratio'],
                   float(got.flatten()[at]), float(want.flatten()[at]), f['n_bad'], score.numel()))
    return f


def _exact(L, kind, got, want, failures):
    if tuple(got.shape) != tuple(want.shape):
        failures.append({'kind': kind, 'conv': L.idx, 'name': L.name, 'loc': None, 'ratio': float('inf'), 'border': False, 'n_bad': got.numel(),
                         'msg': '  convolution %d (%s) %s: shape %s, want %s' % (L.idx, L.name, kind, tuple(got.shape), tuple(want.shape))})
        return
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    failures.append(_worst(L, kind, (got.double() - want.double()).abs().masked_fill(~bad, 0.0), bad, got, want, '|difference|'))


def check_layers(taps, weights, images, exact, raise_on_fail=True):
    """Every element of everything in `taps` (see the module docstring).  Returns one record per convolution (idx, name, rows, Kp, cout, ratio =
    its worst error / bound) plus the feature record; raises LayerMismatch (failures in network order) unless raise_on_fail is False, in which
    case (records, failures) is returned."""
    N = int(images.shape[0])
    failures, records, last = [], [], {}
    for L in NET:
        i = L.idx
        y, tj = taps.out[i], taps.joined[i]
        # ---- the block input as it stands after this convolution
        if i == 0:
            _exact(L, 'max pool', tj, F.max_pool2d(y.permute(0, 3, 1, 2).clamp_min(0), 3, 2, 1).permute(0, 2, 3, 1), failures)
        elif L.join:
            ident = taps.joined[i - 1] if L.join == 'ident' else taps.out[last['D']]
            _exact(L, 'join', tj, (taps.out[last['C']] + ident).clamp_min(0), failures)
        else:
            _exact(L, 'T_J kept', tj, taps.joined[i - 1], failures)
        # ---- the convolution
        if L.src == 'img':
            x, relu_in = images.permute(0, 2, 3, 1), False
        elif L.src == 'J':
            x, relu_in = (tj if L.join else taps.joined[i - 1]), False
        else:
            x, relu_in = taps.out[last[L.src]], True
        wf, bf = weights[i]
        K = L.cin * L.R * L.R
        want_shape = (N, L.hout, L.hout, L.cout)
        if tuple(y.shape) != want_shape or tuple(x.shape) != (N, L.hin, L.hin, L.cin):
            failures.append({'kind': 'conv', 'conv': i, 'name': L.name, 'loc': None, 'ratio': float('inf'), 'border': False, 'n_bad': y.numel(),
                             'msg': '  convolution %d (%s): output %s, want %s; input %s' % (i, L.name, tuple(y.shape), want_shape, tuple(x.shape))})
            records.append({'idx': i, 'name': L.name, 'rows': N * L.hout ** 2, 'Kp': kp(L), 'cout': L.cout, 'ratio': float('inf')})
            last[L.out] = i
            continue
        y64, A = conv_ref(x, wf, bf, L.stride, L.pad, relu_in, None)
        bound = (bound_c(K, exact) + 2.0 ** -24) * (A + bf.double().abs())
        ratio = (y.double() - y64).abs() / bound.clamp_min(1e-300)
        bad = ~(ratio <= 1.0)                                          # NaN (an element never written) fails
        rmax = float('inf') if bool(torch.isnan(ratio).any()) else float(ratio.max())
        records.append({'idx': i, 'name': L.name, 'rows': N * L.hout ** 2, 'Kp': kp(L), 'cout': L.cout, 'ratio': rmax})
        if bool(bad.any()):
            failures.append(_worst(L, 'conv', ratio, bad, y, y64, 'error / bound'))
        last[L.out] = i
    # ---- the features: the last join and the average pool
    L = NET[-1]
    v = (taps.out[last['C']].double() + (taps.joined[-1] if FINAL_JOIN == 'ident' else taps.out[last['D']]).double()).clamp_min(0)
    want = v.mean(dim=(1, 2))
    tol = 50 * 2.0 ** -24 * float(v.max())
    err = (taps.feat.double() - want).abs() if tuple(taps.feat.shape) == tuple(want.shape) else torch.full_like(want, float('inf'))
    emax = float('inf') if bool(torch.isnan(err).any()) else float(err.max())
    records.append({'idx': len(NET), 'name': 'avgpool', 'rows': N, 'Kp': 49, 'cout': L.cout, 'ratio': emax / tol})
    if not emax <= tol:
        s = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
        at = int(torch.argmax(s))
        failures.append({'kind': 'features', 'conv': len(NET), 'name': 'avgpool', 'loc': (at // L.cout, 0, 0, at % L.cout), 'ratio': emax / tol, 'border': False,
                         'n_bad': int((~(err <= tol)).sum()),
                         'msg': '  features: worst at (n=%d, c=%d): error / bound = %.4g' % (at // L.cout, at % L.cout, emax / tol)})
    if not raise_on_fail:
        return records, failures
    if failures:
        raise LayerMismatch(failures)
    return records


def format_records(records, mode):
    lines = ['%-5s %2d %-24s %6d x %4d x %4d   worst error / bound %.3f' % (mode, r['idx'], r['name'], r['rows'], r['Kp'], r['cout'], r['ratio']) for r in records]
    worst = max(records[:-1], key=lambda r: r['ratio'])
    lines.append('%-5s worst convolution: %d (%s) %.3f; features %.3f' % (mode, worst['idx'], worst['name'], worst['ratio'], records[-1]['ratio']))
    return lines
