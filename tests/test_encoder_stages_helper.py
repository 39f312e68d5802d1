"""CPU: the stage-by-stage encoder check of tests/test_gpu_encoder_stages.py checked on its own -- the tap's index arithmetic (csrc/tap.h) against offsets
written out longhand, with the host compiler; the bounds of tests/_encoder_stages.py hold for an fp32 emulation of the forward; a 1e-5 fault planted in one
element of any stage kind is reported at exactly that stage, step, row and unit, where the feature comparison of the other tests sees nothing; and the GPU
test's case table reaches every kernel family select_kernels can name for the encoder."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import _encoder_stages as ES
from oracle import tepose_ref as O
from tepose_amd import synth
from test_gpu_encoder_stages import CASES, KNOBS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = 792                      # L x Hp x B x T x plan flags of tests/c_client/tap_index_check.cpp (frame-major layer 0 only where B % 16 == 0)


# ---- the index header ---------------------------------------------------------------------------------------------------------------------------------
def _cxx():
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail('no host C++ compiler (c++ / g++ / clang++) on PATH')
    return cxx


def _build(exe, extra=()):
    cmd = [_cxx(), '-std=c++17', '-O1', '-Wall', '-Werror', *extra, '-I', os.path.join(ROOT, 'tepose_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'c_client', 'tap_index_check.cpp'), '-o', exe]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'ok %d' % COMBOS


def test_tap_index_on_the_host(tmp_path):
    """every form (rows, state blocks, gi blocks, blocked and scaled planes), ragged B, Hp = 64 / 192 / 320 (no multiple of 128), L = 1 .. 4"""
    exe = str(tmp_path / 'tap_index_check')
    p = _build(exe)
    assert p.returncode == 0, p.stdout[-3000:]
    _run(exe)


def test_tap_index_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'tap_index_check_san')
    p = _build(exe, ('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'))
    if p.returncode != 0:
        print(p.stdout[-2000:])        # a host compiler without the sanitizer runtimes: the plain build above is the check
        return
    _run(exe)


def test_the_entry_answers_arg_then_state_without_a_device():
    """TEPOSE_E_ARG for null pointers, empty shapes and a stage outside 0 .. 2, then TEPOSE_E_STATE for a handle that holds no encoder -- before shapes are
    looked at, so before any device call.  (SHAPE and WORKSPACE need a packed handle: tests/test_gpu_encoder_stages.py.)"""
    import ctypes
    from tepose_amd import _lib
    lib = _lib.load()
    h, v = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.tepose_create(2, 64, ctypes.byref(h)) == 0 and lib.tepose_create_vibe(1, 64, ctypes.byref(v)) == 0
    try:
        p = 4096                                  # a non-null "device pointer" that must never be touched
        tap = lambda m=h, B=3, T=4, stage=1, out=p, ws=p, layer=0, n=3 * 64: lib.tepose_encoder_tap(m, B, T, stage, layer, 0, 0, out, n, None, ws, 1 << 40, None)
        assert tap(m=None) == -1 and tap(out=None) == -1 and tap(ws=None) == -1 and tap(B=0) == -1 and tap(T=0) == -1 and tap(stage=-1) == -1 and tap(stage=3) == -1
        assert tap(m=v) == -1                                                             # a VIBE handle has no such encoder
        assert tap() == -4 and tap(layer=7) == -4 and tap(n=1) == -4                      # not packed: answered before layer and count are looked at
    finally:
        lib.tepose_destroy(h)
        lib.tepose_destroy(v)


# ---- the bounds hold for the reference alone ------------------------------------------------------------------------------------------------------------
EMULATED = [(2, 256, 3, 5), (3, 128, 5, 3), (1, 128, 7, 3), (2, 100, 9, 1), (2, 64, 20, 2), (2, 1024, 4, 6), (4, 64, 3, 4)]


def _inputs(L, H, B, T):
    return synth.synthetic_state_dict(L, H, 11), synth.synthetic_windows(B, T, 42)


@pytest.mark.parametrize('split', [True, False], ids=['split', 'exact'])
@pytest.mark.parametrize('L,H,B,T', EMULATED)
def test_the_fp32_emulation_stays_within_every_bound(L, H, B, T, split):
    """torch fp32 products and cells (split: operands rounded to their hi + lo fp16 halves) are the stand-in for the taps: ragged Hp (H = 100), T = 1, one
    to four layers (the middle layers of 3 and 4: gi not kept; layer 0 of 4: overwritten).  Asserts only <= 1; the worst ratio is printed."""
    state, x = _inputs(L, H, B, T)
    taps = ES.standin_taps(state, x, L, H, split)
    records = ES.check_stages(taps, state, x, L, H, ES.standin_plan(L, split))
    worst = max(records, key=lambda r: r['ratio'])
    print('\n'.join(ES.format_records(records)))
    print('L %d H %d B %d T %d %s: worst error / bound %.4f at %s' % (L, H, B, T, 'split' if split else 'exact', worst['ratio'], worst['name']))
    assert len(records) == len(ES.surviving(L, T)) + 1 and all(r['ratio'] <= 1.0 for r in records)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------------------------
# The model is small on purpose.  A componentwise a-priori bound grows with K and with A = |a| |W|^T, so what 1e-5 means depends on the stage: for a cell
# step the bound is ~1e-6 at any size; for gi of layer 1 it is c A = 3.5e-6 .. 6.1e-6 at H = 64 (gru_fwd, K = 64), 1.1e-5 .. 4.5e-5 at H = 256 and
# 4.6e-5 .. 1.7e-4 at H = 1024; for gi of layer 0 (K = 2133, A ~ 27) ~7e-4 at any H.  A 1e-5 fault can only be told from rounding where it exceeds that:
# H = 64 here, and test_a_1e5_fault_in_a_layer0_gate_preactivation for layer 0.
SL, SH, SB, ST = 2, 64, 3, 6


@pytest.fixture(scope='module')
def clean():
    state, x = _inputs(SL, SH, SB, ST)
    return state, x, ES.standin_taps(state, x, SL, SH, True)


def _planted(taps, kind, key, at, delta=1e-5):
    gi = {k: (v[0].clone(), v[1]) for k, v in taps.gi.items()}
    h = {k: (v[0].clone(), v[1]) for k, v in taps.h.items()}
    tail = (taps.tail[0].clone(), taps.tail[1])
    (gi[key][0] if kind == 'gi' else h[key][0] if kind == 'h' else tail[0])[at] += delta
    return ES.Taps(gi, h, tail, taps.feat)


FAULTS = [            # kind, key, element; what the first failing record must say
    ('gi', (1, 0), (2, 1, 2 * 64 + 37), dict(stage='gi', layer=1, dir=0, step=None, loc={'slab': 2, 'row': 1, 'gate': 2, 'unit': 37})),
    ('h', (0, 0, 0), (1, 20), dict(stage='h', layer=0, dir=0, step=0, loc={'row': 1, 'unit': 20})),                         # a first step
    ('h', (0, 1, 3), (2, 31), dict(stage='h', layer=0, dir=1, step=3, loc={'row': 2, 'unit': 31})),                         # a middle step
    ('h', (0, 2, ST - 1), (0, 63), dict(stage='h', layer=0, dir=2, step=ST - 1, loc={'row': 0, 'unit': 63})),
    ('h', (1, 0, ST - 1), (0, 3), dict(stage='h', layer=1, dir=0, step=ST - 1, loc={'row': 0, 'unit': 3})),                 # the last top-layer step
    ('h', (1, 2, 0), (2, 48), dict(stage='h', layer=1, dir=2, step=0, loc={'row': 2, 'unit': 48})),
    ('tail', None, (1, 64 + 9), dict(stage='tail', layer=1, dir=None, step=None, loc={'row': 1, 'column': 64 + 9})),
]


@pytest.mark.parametrize('kind,key,at,want', FAULTS, ids=['%s%s' % (f[0], '' if f[1] is None else f[1]) for f in FAULTS])
def test_a_1e5_fault_in_one_element_is_reported_where_it_is(clean, kind, key, at, want):
    state, x, taps = clean
    ES.check_stages(taps, state, x, SL, SH, ES.standin_plan(SL, True))                     # clean: passes
    with pytest.raises(ES.StageMismatch) as e:
        ES.check_stages(_planted(taps, kind, key, at), state, x, SL, SH, ES.standin_plan(SL, True))
    first = e.value.failures[0]
    assert {k: first[k] for k in want} == want, first
    assert first['n_bad'] == 1 and first['name'] in str(e.value).splitlines()[0]
    # today's feature check would have passed: the planted tap changes nothing in the feature the device handed over, and a real fault of this size
    # reaches it attenuated (test_the_feature_forgets_a_first_step_fault)


def test_a_1e5_fault_in_a_layer0_gate_preactivation(clean):
    """The layer-0 projection sums 2133 products of magnitude ~27 in all: its derived bound is c A ~ 7e-4 at the synthetic windows' scale (printed), so a
    1e-5 fault there is inside what rounding may do and NO componentwise a-priori bound can tell it from rounding -- the cell steps that consume it are
    judged against the tapped value.  It is reported where A is small: on windows scaled by 2^-10 (the bound scales with them), and in a pad column
    anywhere."""
    state, x, taps = clean
    Hp = ES.hp_of(SH)
    rec = ES.check_stages(taps, state, x, SL, SH, ES.standin_plan(SL, True))[0]
    g64 = torch.from_numpy(x[:, 0]).double() @ torch.from_numpy(state['encoder.gru_fwd.weight_ih_l0']).double().t()
    A = torch.from_numpy(x[:, 0]).double().abs() @ torch.from_numpy(state['encoder.gru_fwd.weight_ih_l0']).double().abs().t()
    print('layer-0 gi: |gi| <= %.2f, A = %.1f .. %.1f, bound %.2e .. %.2e; clean worst ratio %.4f' % (float(g64.abs().max()), float(A.min()), float(A.max()),
          ES.coef(ES.KIN_P, 'gemm_h3_kernel') * float(A.min()), ES.coef(ES.KIN_P, 'gemm_h3_kernel') * float(A.max()), rec['ratio']))
    xs = x.copy()
    xs[:, :, :2048] *= np.float32(2.0 ** -10)
    xs[:, :, 2048:] = 0
    small = ES.standin_taps(state, xs, SL, SH, True)
    ES.check_stages(small, state, xs, SL, SH, ES.standin_plan(SL, True))
    with pytest.raises(ES.StageMismatch) as e:
        ES.check_stages(_planted(small, 'gi', (0, 1), (4, 2, Hp + 40)), state, xs, SL, SH, ES.standin_plan(SL, True))
    first = e.value.failures[0]
    assert (first['stage'], first['layer'], first['dir'], first['loc']) == ('gi', 0, 1, {'slab': 4, 'row': 2, 'gate': 1, 'unit': 40}) and first['n_bad'] == 1


def test_a_nonzero_pad_column_and_a_nan_are_reported():
    L, H, B, T = 2, 100, 4, 3                                                              # Hp = 128
    state, x = _inputs(L, H, B, T)
    taps = ES.standin_taps(state, x, L, H, True)
    plan = ES.standin_plan(L, True)
    for kind, key, at, name in [('h', (0, 1, 1), (3, 100), 'h(layer 0, gru_rec reverse, step 1)'), ('gi', (0, 0), (1, 2, 128 + 127), 'gi(layer 0, gru_fwd)'),
                                ('h', (1, 1, T - 2), (0, 127), 'h(layer 1, gru_rec reverse, step 1)')]:
        _, failures = ES.check_stages(_planted(taps, kind, key, at, 1e-30), state, x, L, H, plan, raise_on_fail=False)
        assert failures[0]['name'] == name and failures[0]['ratio'] == float('inf') and failures[0]['loc']['row'] == at[-2], failures[0]
    _, failures = ES.check_stages(_planted(taps, 'h', (1, 0, T - 2), (2, 17), float('nan')), state, x, L, H, plan, raise_on_fail=False)
    assert failures[0]['name'] == 'h(layer 1, gru_fwd, step 1)' and failures[0]['loc'] == {'row': 2, 'unit': 17}      # (its previous state is not kept: finite and pads only)


def _feature64(enc, x, L, fault=None):
    """oracle.tepose_ref.encoder_fwd restated with one hook: fault = (layer, direction, step, units, delta) is added to that state as the step leaves it"""
    def scan(seq, l, d, steps, tag):
        w_ih, w_hh = ES._w(enc, 'weight_ih', l, d), ES._w(enc, 'weight_hh', l, d)
        b_ih, b_hh = ES._w(enc, 'bias_ih', l, d), ES._w(enc, 'bias_hh', l, d)
        h, out = seq.new_zeros(seq.shape[1], w_hh.shape[1]), []
        for t in range(steps):
            h = O.gru_cell(seq[t] @ w_ih.t() + b_ih, h, w_hh, b_hh)
            if fault and fault[:3] == (l, d, t):
                h = h.clone()
                h[:, fault[3]] += fault[4]
            out.append(h)
        return torch.stack(out)
    xs = x.transpose(0, 1)
    T = xs.shape[0]
    seq = xs
    for l in range(L):
        seq = scan(seq, l, 0, T, 'f')
    y_last = seq[-1]
    seq = xs.flip(0)
    for l in range(L):
        top = l == L - 1
        f = scan(seq, l, 2, 1 if top else T, 'r')
        b = scan(seq.flip(0), l, 1, T, 'b').flip(0)
        if top:
            y_rec0 = torch.cat([f[0], b[0]], dim=1)
        else:
            seq = torch.cat([f, b], dim=2)
    y_fwd = torch.relu(y_last) @ enc['linear_fwd.weight'].t() + enc['linear_fwd.bias']
    y_rec = torch.relu(y_rec0) @ enc['linear_rec.weight'].t() + enc['linear_rec.bias']
    return (y_fwd + y_rec) / 2


def test_the_feature_forgets_a_first_step_fault():
    """The oracle alone: 1e-3 -- a hundred times the faults above -- on a whole 16-unit tile of the first gru_fwd state of layer 0 of an (L 2, H 256, T 16)
    model moves the fp64 feature by less than the 2e-5 the feature tests allow."""
    L, H, B, T = 2, 256, 2, 16
    state, x = _inputs(L, H, B, T)
    enc = O.split_state_dict(state, torch.float64)[0]
    x64 = torch.from_numpy(x).double()
    with torch.no_grad():
        clean_feat = _feature64(enc, x64, L)
        assert torch.equal(clean_feat, O.encoder_fwd(enc, x64, L))                        # the restatement IS the oracle
        moved = float((_feature64(enc, x64, L, (0, 0, 0, slice(32, 48), 1e-3)) - clean_feat).abs().max())
    print('1e-3 on units 32 .. 47 of h(layer 0, gru_fwd, step 0): the feature moves by %.2e' % moved)
    assert 0 < moved < 2e-5


# ---- plan coverage ----------------------------------------------------------------------------------------------------------------------------------------
# Every symbol csrc/plan.hip's name() tables hold for a product and for a cell step, written out.  A kernel family added to the plan later fails
# test_case_table_covers_the_plan until CASES has a stage-by-stage case for it.
_MM = {'gemm_f32_kernel', 'skinny_gemm_kernel', 'gemm_h3_kernel', 'skinny_gemm_h3_kernel', 'gemm_h3s_kernel<1, 3, 4, 3, 4>',
       'gemm_h3s_persist16c_kernel<0>', 'gemm_h3s_persist16c_kernel<1>'}
_STEP = {'gru_step_kernel', 'skinny_gru_kernel', 'gemm_h3_kernel<GRU>', 'skinny_gru_h3_kernel', 'gru_seq_kernel', 'gru_seq_kernel(granules)',
         'gru_step16_kernel<false>', 'gru_step16_kernel<true>'}
_FIRST = {'gru_step_kernel', 'skinny_gru_kernel', 'gru_first_kernel', 'gru_first16_kernel', '(in gru_seq_kernel)'}


def _select(shapes, env):
    """select_kernels of every (L, H, B, T) of `shapes` from ONE fresh process with the knobs `env` (read when a handle is created)."""
    code = ("import json, sys\nsys.path.insert(0, %r)\nfrom tepose_amd.engine import Engine\n"
            "print(json.dumps([Engine(L, H).select_kernels(B, T) for L, H, B, T in %r]))" % (ROOT, [tuple(s) for s in shapes]))
    e = dict(os.environ, TEPOSE_ASSUME_CUS='256')
    for k in KNOBS:
        e.pop(k, None)
    e.update(env)
    out = subprocess.run([sys.executable, '-c', code], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope='module')
def plans():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    out = [None] * len(CASES)
    for env in {tuple(sorted(c[4].items())) for c in CASES}:            # a subprocess per environment
        idx = [i for i, c in enumerate(CASES) if tuple(sorted(c[4].items())) == env]
        for i, sel in zip(idx, _select([CASES[i][:4] for i in idx], dict(env))):
            out[i] = sel
    return out


def test_case_table_covers_the_plan(plans):
    src = open(os.path.join(ROOT, 'tepose_amd', 'csrc', 'plan.hip')).read()
    mm = src[src.index('const char* name(Mm v)'):src.index('const char* name(Step v)')]
    step = src[src.index('const char* name(Step v)'):src.index('const char* name(First v)')]
    first = src[src.index('const char* name(First v)'):src.index('const char* name(Smpl v)')]
    assert set(re.findall(r'"([^"]+)"', mm)) == _MM and set(re.findall(r'"([^"]+)"', step)) == _STEP and set(re.findall(r'"([^"]+)"', first)) == _FIRST
    seen = {k: set() for k in ('projection', 'projection_l1', 'projection_one_step', 'gru_step', 'gru_step_l1', 'gru_first', 'gi0_layout', 'gi1_layout')}
    for sel in plans:
        for k in seen:
            if k in sel:
                seen[k].add(sel[k])
    # what select_kernels can put where (csrc/plan.hip): layer 0 never runs on the scaled-state kernel <1>, layers >= 1 and the one-step product never on
    # the two layer-0 kernels of large and mid-size batches
    assert seen['projection'] == _MM - {'gemm_h3s_persist16c_kernel<1>'}, seen['projection'] ^ (_MM - {'gemm_h3s_persist16c_kernel<1>'})
    for k in ('projection_l1', 'projection_one_step'):
        assert seen[k] == _MM - ES.SCALE1_KERNELS, (k, seen[k] ^ (_MM - ES.SCALE1_KERNELS))
    assert seen['gru_step'] == _STEP and seen['gru_step_l1'] == _STEP, (_STEP ^ seen['gru_step'], _STEP ^ seen['gru_step_l1'])
    assert seen['gru_first'] == _FIRST, _FIRST ^ seen['gru_first']
    assert seen['gi0_layout'] == {'row_major', 'frame_major_blocked'} and seen['gi1_layout'] == {'row_major', 'blocked'}
    assert {c[0] for c in CASES} == {1, 2, 3} and any(ES.hp_of(c[1]) != c[1] for c in CASES) and any(c[3] == 1 for c in CASES)
