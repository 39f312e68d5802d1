"""CPU: the stage-by-stage decoder check of tests/test_gpu_decoder_stages.py checked on its own -- the tap's views (csrc/tap.h tap_decoder) against offsets
written out longhand, with the host compiler, plain and under the sanitizers; the entry's ARG / STATE answers without a device; the bounds of
tests/_decoder_stages.py hold for an fp32 emulation of every stage; a fault far below the 1e-4 of the output tests, planted in one element of any stage
kind, is reported at exactly that stage, person and element; a reference that took the rest joints from J0 + JS beta would hide a wrong JS, this one does
not; and the GPU test's case table reaches every Smpl, Reg and tail family select_kernels can name."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import _decoder_stages as DS
import _encoder_stages as ES
from tepose_amd import synth
from test_gpu_decoder_stages import CASES, KNOBS, T_FWD, smpl_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = 49                       # N x what the plan keeps of tests/c_client/tap_decoder_check.cpp
L, H = 1, 64


# ---- the views ------------------------------------------------------------------------------------------------------------------------------------------
def _cxx():
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail('no host C++ compiler (c++ / g++ / clang++) on PATH')
    return cxx


def _build(exe, extra=()):
    cmd = [_cxx(), '-std=c++17', '-O1', '-Wall', '-Werror', *extra, '-I', os.path.join(ROOT, 'tepose_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'c_client', 'tap_decoder_check.cpp'), '-o', exe]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'ok %d' % COMBOS


def test_tap_decoder_views_on_the_host(tmp_path):
    """every form (rows with the stage's leading dimension, blocked planes, scaled planes with row scales), N = 1 .. 130, what each plan refuses"""
    exe = str(tmp_path / 'tap_decoder_check')
    p = _build(exe)
    assert p.returncode == 0, p.stdout[-3000:]
    _run(exe)


def test_tap_decoder_views_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'tap_decoder_check_san')
    p = _build(exe, ('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'))
    if p.returncode != 0:
        print(p.stdout[-2000:])        # a host compiler without the sanitizer runtimes: the plain build above is the check
        return
    _run(exe)


def test_the_entry_answers_arg_then_state_without_a_device():
    """TEPOSE_E_ARG for null pointers, N < 1, a stage outside 0 .. 8 and an unknown entry kind, then TEPOSE_E_STATE for a handle without SMPL tables -- before
    count and workspace are looked at, so before any device call.  (SHAPE and WORKSPACE need a packed handle: tests/test_gpu_decoder_stages.py.)"""
    from tepose_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.tepose_create(1, 64, ctypes.byref(h)) == 0
    try:
        p = 4096                                  # a non-null "device pointer" that must never be touched
        tap = lambda m=h, N=3, stage=0, out=p, n=3 * 160, entry=0, T=1, ws=p: lib.tepose_decoder_tap(m, N, stage, out, n, None, entry, T, ws, 1 << 40, None)
        assert tap(m=None) == -1 and tap(out=None) == -1 and tap(ws=None) == -1 and tap(N=0) == -1 and tap(stage=-1) == -1 and tap(stage=9) == -1
        assert tap(entry=2) == -1 and tap(entry=-1) == -1 and tap(entry=1, T=0) == -1
        assert tap() == -4 and tap(n=1) == -4 and tap(stage=8, entry=1, T=4) == -4
    finally:
        lib.tepose_destroy(h)


# ---- the bounds hold for the reference alone ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def state():
    return synth.synthetic_state_dict(L, H, 11)


def _feat(N):
    return torch.from_numpy(synth.normal('dec/feat%d' % N, (N, 2048), std=0.5))


def _pose(N, mode):
    aa = synth.normal('dec/aa', (N, 24, 3), std=0.4)
    aa[0, 5] = 0
    aa[N - 1, 7] = np.array([np.pi, 0, 0], dtype=np.float32)
    pose = torch.from_numpy(aa.reshape(N, 72))
    if mode == 2:
        pose = DS.rodrigues64(pose.double().reshape(-1, 3)).float().reshape(N, 24, 3, 3)
    return pose, torch.from_numpy(synth.normal('dec/betas', (N, 10), std=0.5))


def _tail(N):
    """a relu-tail as the encoder tap hands it over: [N, 3 Hp], pad columns 0 (Hp = H = 64 here)"""
    return torch.from_numpy(np.abs(synth.normal('dec/tail%d' % N, (N, 3 * ES.hp_of(H)), std=0.3))), 3


def _src(way, N, state):
    if way == 'collapsed':
        return DS.Src('collapsed', feat=_feat(N)), 'collapsed', True
    if way == 'tail_collapsed':
        return DS.Src('tail_collapsed', tail=_tail(N), H=H), 'collapsed', True
    if way in ('seq1', 'seq3', 'loop1', 'tiled1', 'exact1', 'exact3'):
        return DS.Src('loop', feat=_feat(N), n_iter=int(way[-1]), init=DS.init_rows(state, N)), way[:-1], not way.startswith('exact')
    if way == 'init':
        g = np.load(os.path.join(ROOT, 'tests', 'golden', 'geometry.npz'))
        rows = torch.from_numpy(g['x6'][np.arange(N) % 64].copy())
        shape = torch.from_numpy(np.where(np.arange(N * 10).reshape(N, 10) % 2 == 0, 5.0, -5.0).astype(np.float32))
        cam = torch.from_numpy(synth.normal('dec/cam', (N, 3), std=0.05))
        cam[:, 0] = torch.tensor([0.9, 1e-3, 0.0, -0.5] * ((N + 3) // 4))[:N]
        return DS.Src('init', init=DS.init_rows(state, N, rows, shape, cam)), 'collapsed', True
    mode = int(way[-1])
    pose, betas = _pose(N, mode)
    return DS.Src('pose', mode=mode, pose=pose, betas=betas), 'collapsed', True


WAYS = ('collapsed', 'tail_collapsed', 'seq1', 'seq3', 'loop1', 'tiled1', 'exact1', 'exact3', 'init', 'pose1', 'pose2')
# every pose mode (0: one way of making xs per N, rotating through all of them; 1; 2) at N = 1, 5, 130 with sparse and dense skin tables
EMULATED = [(N, tables, way) for N in (1, 5, 130) for tables in ('synth', 'dense') for way in
            ((WAYS[:4] if N == 1 else WAYS[:9] if N == 5 else ('collapsed', 'tiled1', 'exact3')) + ('pose1', 'pose2'))]


@pytest.mark.parametrize('N,tables,way', EMULATED, ids=['N%d-%s-%s' % e for e in EMULATED])
def test_the_fp32_emulation_stays_within_every_bound(N, tables, way, state):
    """torch fp32 products (split families: operands rounded to their hi + lo fp16 halves), the op sequences of smpl.hip in fp32 and the pack-time
    constants in fp32 are the stand-in for taps and outputs; with and without the 17-row regressor.  Asserts only <= 1; the worst ratio is printed."""
    smpl_np = smpl_tables(tables)
    src, reg, split = _src(way, N, state)
    plan = DS.standin_plan(N, split, tables == 'dense', reg, blend16=N == 130 and way == 'collapsed')
    for J in (None,) if src.how == 'pose' else (None, smpl_np['J_regressor_h36m']):
        run = DS.standin_run(state, smpl_np, src, plan, J)
        records = DS.check_stages(run, state, smpl_np, plan)
        worst = max(records, key=lambda r: r['ratio'])
        print('\n'.join(DS.format_records(records, 'J17  ' if J is not None else '')))
        print('N %d %s %s: worst error / bound %.4f at %s' % (N, tables, way, worst['ratio'], worst['stage']))
        names = [r['stage'] for r in records]
        assert all(r['ratio'] <= 1.0 for r in records) and {'posed', 'amat', 'verts', 'kp_3d'} <= set(names)
        if src.how != 'pose':
            assert {'xs', 'rotmat', 'theta', 'kp_2d'} <= set(names)
        if plan['smpl'] != 'smpl_small_kernel':
            assert {'pf', 'vposed'} <= set(names) and ('pf_planes' in names) == split and ('pf16' in names) == ('h3s' in plan['smpl'])


def test_the_edge_tables_stay_within_every_bound(state):
    """the skin table with single-weight and -0.0 vertices, regressors with an empty row, a row at column 6889, a 65-entry row and a dense negative row"""
    for tables, N in (('edges', 5), ('edges5', 3)):
        smpl_np = smpl_tables(tables)
        plan = DS.standin_plan(N, True, tables == 'edges5')
        assert DS.tables(smpl_np)['dense'] == (tables == 'edges5')
        for J in (None, smpl_np['J_regressor_h36m']):
            run = DS.standin_run(state, smpl_np, DS.Src('collapsed', feat=_feat(N)), plan, J)
            records = DS.check_stages(run, state, smpl_np, plan)
            assert all(r['ratio'] <= 1.0 for r in records)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------------------------
SN = 5


@pytest.fixture(scope='module')
def clean(state):
    """one clean emulation per way the faults need, with every stage's bound tensor: (run, plan, bounds)"""
    out = {}
    for key, way in (('collapsed', 'collapsed'), ('init', 'init'), ('exact', 'exact1')):
        src, reg, split = _src(way, SN, state)
        plan = DS.standin_plan(SN, split, False, reg)
        run = DS.standin_run(state, smpl_tables('synth'), src, plan)
        bounds = {}
        DS.check_stages(run, state, smpl_tables('synth'), plan, bounds=bounds)                # clean: passes
        out[key] = (run, plan, bounds)
    return out


def _planted(run, where, name, at, delta):
    taps = {k: (v[0].clone(), v[1]) for k, v in run.taps.items()}
    out = {k: v.clone() for k, v in run.out.items()}
    t = (taps[name][0] if where == 'tap' else out[name]).reshape(run.N, -1)
    t[at] += delta
    return DS.Run(run.N, taps, out, run.src, run.J)


def _copied_and_regressed():
    from oracle import tepose_ref as O
    copied = next(k for k, s in enumerate(O.JOINT_MAP_49) if 24 <= s < 45)
    regressed = next(k for k, s in enumerate(O.JOINT_MAP_49) if s >= 45)
    return copied, regressed


# stage, where it lives, the clean run it is planted in, (person, element); element None: where the stage's bound is smallest for that person
FAULTS = [
    ('xs', 'tap', 'init', (2, 150)),              # (the collapsed product's bound is ~1e-4: test_where_the_derived_bound_is_wide; here xs is the init rows)
    ('pf_planes', 'tap', 'collapsed', (3, 11 + 9 * 4 + 5)),
    ('amat', 'tap', 'collapsed', (1, 12 * 7 + 6)),
    ('posed', 'tap', 'collapsed', (4, 3 * 15 + 1)),
    ('vposed', 'tap', 'collapsed', (2, 3 * 1234 + 2)),
    ('vposed', 'tap', 'exact', (0, None)),
    ('verts', 'out', 'collapsed', (3, 3 * 6889 + 0)),
    ('kp_3d', 'out', 'collapsed', (1, 'copied')),
    ('kp_3d', 'out', 'collapsed', (2, 'regressed')),
    ('kp_2d', 'out', 'collapsed', (0, 2 * 30 + 1)),
]


@pytest.mark.parametrize('stage,where,key,at', FAULTS, ids=['%s-%s-%s' % (f[0], f[2], f[3][1]) for f in FAULTS])
def test_a_small_fault_in_one_element_is_reported_where_it_is(clean, state, stage, where, key, at):
    """max(1e-5, 4 x the clean bound at that element), below the 1e-4 the output tests allow: the first failing stage is the planted one, with one
    element over, at that person and element -- and the output comparison at 1e-4 sees nothing."""
    run, plan, bounds = clean[key]
    person, el = at
    if el in ('copied', 'regressed'):
        el = 3 * _copied_and_regressed()[el == 'regressed'] + 1
    b = bounds.get(stage)
    if el is None:
        el = int(torch.argmin(b[person]))
    bound_there = 0.0 if b is None else float(b[person, el])
    delta = max(1e-5, 4 * bound_there)
    print('%s (%s run): bound at (person %d, element %d) %.2e, fault %.2e' % (stage, key, person, el, bound_there, delta))
    assert delta < 1e-4 and bound_there <= 2.5e-5
    bad = _planted(run, where, stage, (person, el), delta)
    with pytest.raises(DS.StageMismatch) as e:
        DS.check_stages(bad, state, smpl_tables('synth'), plan)
    first = e.value.failures[0]
    assert (first['stage'], first['row'], first['col'], first['n_bad']) == (stage, person, el, 1), first
    assert first['stage'] in str(e.value).splitlines()[0]
    worst, seen = DS.output_tests_see(bad, run)
    assert not seen and worst <= delta + 2.0 ** -20        # (the fault as fp32 stores it)


def test_where_the_derived_bound_is_wide(clean):
    """Two stages whose a-priori bound is itself above 2.5e-5 at the synthetic scale, so that a 1e-5 fault there is inside what rounding may do: xs of
    the collapsed product (K = 2048, A ~ 40: c A ~ 1e-4) and, element by element, v_posed on the exact-fp32 family (224 u A ~ 1.5e-5 at A ~ 1).  The
    faults above are planted where the bound is small instead -- xs on the per-call init rows, v_posed where A is smallest -- as the encoder helper
    does for layer-0 gi; what consumes xs is judged from the tapped value either way."""
    _, _, b = clean['collapsed']
    _, _, bx = clean['exact']
    print('collapsed xs: bound %.2e .. %.2e;  exact-fp32 v_posed: bound %.2e .. %.2e;  split v_posed: %.2e .. %.2e' % (
        float(b['xs'][:, :157].min()), float(b['xs'].max()), float(bx['vposed'].min()), float(bx['vposed'].max()), float(b['vposed'].min()), float(b['vposed'].max())))
    assert float(b['xs'].max()) > 2.5e-5 and float(bx['vposed'].max()) > 1e-5 and float(bx['vposed'].min()) < 2.5e-6


def test_a_pad_column_and_a_nan_are_reported(clean, state):
    run, plan, _ = clean['collapsed']
    for where, name, at in (('tap', 'xs', (1, 158)), ('tap', 'pf', (2, 220)), ('tap', 'pf_planes', (0, 223))):
        _, failures = DS.check_stages(_planted(run, where, name, at, 1e-30), state, smpl_tables('synth'), plan, raise_on_fail=False)
        assert (failures[0]['stage'], failures[0]['row'], failures[0]['col'], failures[0]['ratio']) == (name, at[0], at[1], float('inf')), failures[0]
    _, failures = DS.check_stages(_planted(run, 'out', 'verts', (4, 77), float('nan')), state, smpl_tables('synth'), plan, raise_on_fail=False)
    assert (failures[0]['stage'], failures[0]['row'], failures[0]['col'], failures[0]['ratio']) == ('verts', 4, 77, float('inf'))


def test_a_wrong_js_is_not_hidden_by_the_reference(state):
    """The forbidden shortcut: rest joints as J0 + JS beta in the reference would follow a wrong pack-time JS.  One JS entry off by 1e-3 in the stand-in:
    the chain's first stage reports it, at the person with the largest beta there and at that joint or one below it in the tree (the parent's rotation
    spreads the offset over the three coordinates), because the reference regresses the joints from the shaped template."""
    smpl_np = smpl_tables('synth')
    src, reg, split = _src('collapsed', SN, state)
    plan = DS.standin_plan(SN, split, False, reg)
    j, c, l = 4, 1, 2
    bad = DS.standin_run(state, smpl_np, src, plan, JS_fault=(j, c, l, 1e-3))
    with pytest.raises(DS.StageMismatch) as e:
        DS.check_stages(bad, state, smpl_np, plan)
    first = e.value.failures[0]
    beta = bad.taps['xs'][0][:, 144 + l]
    person = int(torch.argmax(beta.abs()))
    assert first['stage'] == 'posed' and first['row'] == person and first['col'] // 3 in (4, 7, 10) and first['n_bad'] >= SN, first      # (4 -> 7 -> 10 in SMPL's tree)
    assert {f['stage'] for f in e.value.failures} >= {'posed', 'amat'}
    # the stages before the chain and the ones judged from the chain's own outputs are untouched
    assert not {f['stage'] for f in e.value.failures} & {'xs', 'rotmat', 'pf', 'pf_planes', 'theta', 'vposed', 'verts', 'kp_2d'}


# ---- plan coverage ----------------------------------------------------------------------------------------------------------------------------------------
_SMPL = {'smpl_small_kernel', 'smpl_prep_kernel+gemm_f32_kernel+smpl_skin4_kernel', 'smpl_prep_kernel+skinny_gemm_kernel+smpl_skin4_kernel',
         'smpl_prep_kernel+gemm_h3_kernel+smpl_skin4_kernel', 'smpl_prep_kernel+gemm_h3s_persist16c_kernel<1>+smpl_skin4_kernel'}
# tail_name() of csrc/plan.hip on a handle whose encoder and regressor are both packed: the collapsed tail, reg_seq_kernel, and the loop on each of the
# four families name(Mm) holds for plan.tail
_TAIL = {'collapsed: one product (skinny_gemm_h3_kernel)', 'reg_seq_kernel', 'skinny_gemm_h3_kernel loop', 'gemm_h3_kernel loop',
         'skinny_gemm_kernel x (2 + 1 + 9)', 'gemm_f32_kernel x (2 + 1 + 9)'}


def _select(shapes, env):
    """select_kernels of every (N, T) of `shapes` from ONE fresh process with the knobs `env` (read when a handle is created)"""
    code = ("import json, sys\nsys.path.insert(0, %r)\nfrom tepose_amd.engine import Engine\ne = Engine(%d, %d)\n"
            "print(json.dumps([e.select_kernels(N, T) for N, T in %r]))" % (ROOT, L, H, [tuple(s) for s in shapes]))
    e = dict(os.environ, TEPOSE_ASSUME_CUS='256')
    for k in KNOBS:
        e.pop(k, None)
    e.update(env)
    out = subprocess.run([sys.executable, '-c', code], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_case_table_covers_the_plan():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    src = open(os.path.join(ROOT, 'tepose_amd', 'csrc', 'plan.hip')).read()
    smpl = src[src.index('const char* name(Smpl v)'):src.index('std::string tail_name')]
    assert set(re.findall(r'"([^"]+)"', smpl)) == _SMPL
    assert re.search(r'enum class Reg : unsigned char \{ loop, seq \}', open(os.path.join(ROOT, 'tepose_amd', 'csrc', 'plan.h')).read())
    seen = {'smpl': set(), 'tail_regressor': set()}
    for env in {tuple(sorted(c[1].items())) for c in CASES}:            # a subprocess per environment
        cases = [c for c in CASES if tuple(sorted(c[1].items())) == env]
        for c, sel in zip(cases, _select([(c[3], T_FWD if c[0] == 'forward' else 1) for c in cases], dict(env))):
            seen['smpl'].add(sel['smpl'])
            if c[0] in ('regressor', 'forward'):
                seen['tail_regressor'].add(sel['tail_regressor'])
    assert seen['smpl'] == _SMPL, seen['smpl'] ^ _SMPL
    assert seen['tail_regressor'] == _TAIL, seen['tail_regressor'] ^ _TAIL
    # the entries, the iteration counts that isolate (1), only bound (3) and skip (0) the FC loop, both pose modes of tepose_smpl_fwd, every table set
    assert {c[0] for c in CASES} == {'regressor', 'forward', 'init', 'smpl'} and {c[4] for c in CASES if c[0] in ('regressor', 'init')} == {0, 1, 3}
    assert {c[4] for c in CASES if c[0] == 'smpl'} == {0, 1} and {c[2] for c in CASES} == {'synth', 'dense', 'edges', 'edges5'}
    assert any(c[3] <= 4 and c[2] in ('dense', 'edges5') for c in CASES)      # a dense table at an N the small kernel would take
