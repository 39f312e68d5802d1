"""GPU: every stage behind the feature -- the regressor's state row and FC activations, rot6d -> R -> axis-angle, the pose features in each form the plan
keeps, the 24-joint chain, the blend-shape product, skinning, the joint regression, the projection -- copied out of the call's own workspace by
tepose_decoder_tap (or taken from the outputs) and judged against the fp64 restatement of THAT stage from the device's own value of the stage before it
(tests/_decoder_stages.py: bounds, exact facts and report are described and derived there; tests/test_decoder_stages_helper.py checks them, and that CASES
reaches every family of the plan, without a GPU).  The output comparisons of the other tests allow 1e-4; the stages here are held to what fp32 allows.

Workspace and outputs are the test's own, filled with 0xFF bytes / NaN before the call: a place no kernel wrote scores infinity.  One model (L 1, H 64) per
knob set and table set, shared by the cases.  CASES are the smallest N that reach each family and edge."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _decoder_stages as DS
import _encoder_stages as ES
from tepose_amd import _lib, synth
from tepose_amd.engine import out_shapes

pytestmark = pytest.mark.gpu
E_ARG, E_SHAPE, E_WORKSPACE, E_STATE = -1, -2, -3, -4
NAN = float('nan')
L, H, T_FWD = 1, 64, 3
KNOBS = ('TEPOSE_EXACT_FP32', 'TEPOSE_COLLAPSE_REGRESSOR', 'TEPOSE_LARGE_BATCH_KERNELS', 'TEPOSE_BLEND16_MIN_N', 'TEPOSE_PERSISTENT', 'TEPOSE_SMPL_SMALL_MAX_N',
         'TEPOSE_SPLIT_MIN_M')
LOOP, EXACT = {'TEPOSE_COLLAPSE_REGRESSOR': '0'}, {'TEPOSE_EXACT_FP32': '1'}

# (entry, knobs, tables, N, extra): entry 'regressor' (extra = n_iter) | 'forward' | 'init' | 'smpl' (extra = pose2rot); tables: a key of smpl_tables()
CASES = (
    # smpl_small_kernel, the collapsed product, joints<1024>
    [('regressor', {}, 'synth', n, 3) for n in (1, 3, 4)]
    # the general chain: gemm_h3_kernel with one and two ragged row tiles, a partial last prep block, joints<256>, skin_shape's person groups
    + [('regressor', {}, 'synth', n, 3) for n in (5, 17, 130)]
    # blend16: split_rows -> gemm_h3s_persist16c_kernel<1> with a full and a ragged last 16-row tile; the pf16 form
    + [('regressor', {}, 'synth', n, 3) for n in (512, 520)]
    # reg_seq_kernel up to its 64-row cap, then the loop
    + [('regressor', LOOP, 'synth', n, it) for n in (5, 64, 70) for it in (1, 3)]
    # ... and the loop on the tiled split kernel (more rows than the width-first one takes)
    + [('regressor', LOOP, 'synth', 770, 1)]
    # the exact kernels: width-first, and tiled above 768 rows
    + [('regressor', EXACT, 'synth', n, it) for n in (5, 770) for it in (1, 3)]
    # tail_collapsed: xs in the feature slot of tepose_forward's workspace
    + [('forward', {}, 'synth', 6, None)]
    # per-call init rows, n_iter = 0: degenerate 6D rows, cam scales 0.9 / 1e-3 / 0 / -0.5, shape +- 5
    + [('init', {}, 'synth', 8, 0)]
    # tepose_smpl_fwd: axis-angle (a zero joint, angles at pi) and given matrices
    + [('smpl', {}, 'synth', n, p2r) for n in (2, 9) for p2r in (1, 0)]
    # a dense skin table: smpl_skin_kernel; at N = 3 NOT the small kernel
    + [('regressor', {}, 'dense', n, 3) for n in (3, 40)]
    # skin table and regressor edges; the same table with a fifth weight on one vertex
    + [('regressor', {}, 'edges', 5, 3), ('regressor', {}, 'edges5', 3, 3)]
)


def _id(c):
    return '%s-%s-N%d%s%s' % (c[0], c[2], c[3], '' if c[4] is None else '-%s%d' % ('p2r' if c[0] == 'smpl' else 'it', c[4]),
                              ''.join('-%s=%s' % (k[7:].lower(), v) for k, v in sorted(c[1].items())))


_TABLES = {}


def smpl_tables(name):
    """'synth': the synthetic tables; 'dense': seven skin weights per vertex; 'edges': vertices with a single weight 1.0 on joint 23, vertices with a -0.0
    entry, at most 4 weights otherwise, and evaluation / extra regressors with an all-zero row, a row whose only entry is at column 6889, a row of 65
    entries and a fully dense row with negative weights; 'edges5': the same with a fifth weight on vertex 100"""
    if name in _TABLES:
        return _TABLES[name]
    if name == 'synth':
        t = synth.synthetic_smpl(0)
    elif name == 'dense':
        t = synth.synthetic_smpl(0, skin_nnz=7)
    else:
        t = synth.synthetic_smpl(0)
        w = t['lbs_weights'].copy()
        w[0:700:7] = 0
        w[0:700:7, 23] = 1.0
        for v in range(3, 700, 7):
            z = np.nonzero(w[v] == 0)[0][0]
            w[v, z] = -0.0
        if name == 'edges5':
            v = 100
            free = np.nonzero(w[v] == 0)[0]
            need = 5 - int((w[v] != 0).sum())
            w[v, free[:need]] = 0.0625
            w[v] /= w[v].sum()
        assert int((w != 0).sum(axis=1).max()) == (5 if name == 'edges5' else 4)
        t['lbs_weights'] = w
        for key, rows in (('J_regressor_extra', (1, 3, 5, 7)), ('J_regressor_h36m', (2, 8, 11, 16))):       # (the h36m rows are among the 14 that are kept)
            J = t[key].copy()
            J[rows[0]] = 0
            J[rows[1]] = 0
            J[rows[1], 6889] = 1.0
            J[rows[2]] = 0
            J[rows[2], 13:13 + 65 * 101:101] = synth.uniform('edge/%s/65' % key, (65,), 0.0, 1.0 / 32)
            J[rows[3]] = synth.uniform('edge/%s/dense' % key, (6890,), -2.0 / 6890, 3.0 / 6890)
            assert int((J[rows[2]] != 0).sum()) == 65 and int((J[rows[3]] != 0).sum()) > 6800
            t[key] = J
    _TABLES[name] = t
    return t


_MODELS = {}


def _model(knobs, tables):
    """one model per (knob set, table set): the knobs are read when the handle is created"""
    key = (tuple(sorted(knobs.items())), tables)
    if key not in _MODELS:
        from tepose_amd.testing import build_model
        saved = {k: os.environ.pop(k, None) for k in KNOBS}
        os.environ.update(knobs)
        try:
            model, state, _ = build_model(L, H, seed=11, device='cuda', smpl_np=smpl_tables(tables))
            model._engine.pack_model(model, torch.device('cuda', torch.cuda.current_device()))
        finally:
            for k in KNOBS:
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]
        _MODELS[key] = (model, state)
    return _MODELS[key]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _poisoned(eng, B, T):
    return torch.full((int(eng.lib.tepose_workspace_bytes(eng.handle, B, T)),), 0xFF, dtype=torch.uint8, device='cuda')


def _nan_outputs(N, nj):
    return {k: torch.full((N,) + tail, NAN, dtype=torch.float32, device='cuda') for k, tail in out_shapes(nj).items()}


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(eng, case, inp, ws, J):
    """the case's entry point once, into NaN-filled outputs; then the status word"""
    entry, _, _, N, extra = case
    jp = eng.jreg(torch.from_numpy(J), torch.device('cuda', torch.cuda.current_device()))[1] if J is not None else None
    out = _nan_outputs(N, 14 if J is not None else 49)
    o = [out[k].data_ptr() for k in ('theta', 'verts', 'kp_3d', 'kp_2d', 'rotmat')]
    if entry == 'forward':
        _lib.check(eng.lib.tepose_forward(eng.handle, inp['x'].data_ptr(), N, T_FWD, jp, *o, ws.data_ptr(), ws.numel(), _stream()), 'tepose_forward')
    elif entry == 'smpl':
        out = {'verts': out['verts'], 'kp_3d': out['kp_3d']}
        _lib.check(eng.lib.tepose_smpl_fwd(eng.handle, extra, inp['pose'].data_ptr(), inp['betas'].data_ptr(), N, out['verts'].data_ptr(), out['kp_3d'].data_ptr(),
                                           ws.data_ptr(), ws.numel(), _stream()), 'tepose_smpl_fwd')
        return out
    else:
        init = inp.get('init', (None, None, None))
        _lib.check(eng.lib.tepose_regressor_fwd_init(eng.handle, inp['feat'].data_ptr(), N, extra, *[_ptr(t) for t in init], jp, *o, ws.data_ptr(), ws.numel(), _stream()),
                   'tepose_regressor_fwd_init')
    _lib.check(eng.lib.tepose_forward_status(eng.handle, ws.data_ptr(), _stream()), 'tepose_forward_status')
    return out


def _tap(eng, N, stage, entry, ws, out=None, n=None, ws_bytes=None):
    out = torch.full((N, DS.WIDTH[stage]), NAN, dtype=torch.float32, device='cuda') if out is None else out
    form = ctypes.c_int(-1)
    rc = eng.lib.tepose_decoder_tap(eng.handle, N, DS.STAGE_ID[stage], out.data_ptr(), N * DS.WIDTH[stage] if n is None else n, ctypes.byref(form),
                                    1 if entry == 'forward' else 0, T_FWD, ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, _stream())
    return rc, form.value, out


def written(case, plan):
    """the stages this call writes under this plan"""
    entry, _, _, _, extra = case
    small, sm = plan['smpl'] == 'smpl_small_kernel', plan['smpl']
    names = [] if entry == 'smpl' else ['xs']
    if entry == 'regressor' and 'collapsed' not in plan['tail_regressor']:
        names += ['h1', 'h2']
    if not small:
        names += ['pf'] + (['pf_planes'] if 'h3' in sm else []) + (['pf16'] if 'h3s' in sm else []) + ['vposed']
    return names + ['amat', 'posed']


def _inputs(case, state):
    entry, _, _, N, extra = case
    if entry == 'forward':
        return {'x': torch.from_numpy(synth.synthetic_windows(N, T_FWD, 42)).cuda()}
    if entry == 'smpl':
        aa = synth.normal('dec/aa', (N, 24, 3), std=0.4)
        aa[0, 5] = 0                                                            # a zero axis-angle joint
        aa[N - 1, 7] = np.array([np.pi, 0, 0], dtype=np.float32)                # angles at pi
        aa[N - 1, 9] = (np.array([1, 2, -2], dtype=np.float64) / 3 * np.pi).astype(np.float32)
        betas = torch.from_numpy(synth.normal('dec/betas', (N, 10), std=0.5))
        pose = torch.from_numpy(aa.reshape(N, 72))
        if extra == 0:
            pose = DS.rodrigues64(pose.double().reshape(-1, 3)).float().reshape(N, 24, 3, 3).contiguous()
        return {'pose': pose.cuda(), 'betas': betas.cuda()}
    inp = {'feat': torch.from_numpy(synth.normal('dec/feat%d' % N, (N, 2048), std=0.5)).cuda()}
    if entry == 'init':
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'geometry.npz'))
        pose = torch.from_numpy(g['x6'][:N].copy())
        shape = torch.from_numpy(np.where(np.arange(N * 10).reshape(N, 10) % 2 == 0, 5.0, -5.0).astype(np.float32))
        cam = torch.from_numpy(synth.normal('dec/cam', (N, 3), std=0.05))
        cam[:, 0] = torch.tensor([0.9, 1e-3, 0.0, -0.5] * ((N + 3) // 4))[:N]
        inp['init'] = (pose.cuda(), shape.cuda(), cam.cuda())
    return inp


def run_case(case, J):
    """steps 1 .. 4 of the module docstring's procedure; returns the Run, the plan and the model's state"""
    entry, knobs, tables, N, extra = case
    model, state = _model(knobs, tables)
    eng = model._engine
    T = T_FWD if entry == 'forward' else 1
    plan = eng.select_kernels(N, T)
    inp = _inputs(case, state)
    ws = _poisoned(eng, N, T)
    out = _call(eng, case, inp, ws, J)
    taps = {}
    for name in written(case, plan):
        rc, form, t = _tap(eng, N, name, entry, ws)
        _lib.check(rc, 'tepose_decoder_tap(%s)' % name)
        taps[name] = (t, form)
    tail = None
    if entry == 'forward':                                                  # the product's operand: the encoder's tail of the same windows in the same workspace
        feat = torch.full((N, 2048), NAN, dtype=torch.float32, device='cuda')
        _lib.check(eng.lib.tepose_encoder_fwd(eng.handle, inp['x'].data_ptr(), N, T, 0, feat.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'tepose_encoder_fwd')
        tl = torch.full((N, 3 * ES.hp_of(H)), NAN, dtype=torch.float32, device='cuda')
        form = ctypes.c_int(-1)
        _lib.check(eng.lib.tepose_encoder_tap(eng.handle, N, T, 2, 0, 0, 0, tl.data_ptr(), tl.numel(), ctypes.byref(form), ws.data_ptr(), ws.numel(), _stream()),
                   'tepose_encoder_tap(tail)')
        tail = (tl.cpu(), form.value)
    again = _call(eng, case, inp, ws, J)                                    # the taps left nothing behind that the next call would see
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(again[k], out[k]), k
    cpu = lambda t: None if t is None else t.cpu()
    if entry == 'forward':
        src = DS.Src('tail_collapsed' if plan['tail_regressor'].startswith('collapsed') else 'collapsed', tail=tail, H=H)
    elif entry == 'smpl':
        src = DS.Src('pose', mode=1 if extra else 2, pose=inp['pose'].cpu(), betas=inp['betas'].cpu())
    elif entry == 'init':
        src = DS.Src('init', init=DS.init_rows(state, N, *[cpu(t) for t in inp['init']]))
    elif 'collapsed' in plan['tail_regressor'] and extra == 3:
        src = DS.Src('collapsed', feat=inp['feat'].cpu())
    else:
        src = DS.Src('loop', feat=inp['feat'].cpu(), n_iter=extra, init=DS.init_rows(state, N))
    run = DS.Run(N, {k: (v[0].cpu(), v[1]) for k, v in taps.items()}, {k: v.cpu() for k, v in out.items()}, src, J)
    return run, plan, state


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_every_stage_against_fp64(case):
    entry, knobs, tables, N, extra = case
    smpl_np = smpl_tables(tables)
    errs0 = int(_lib.load().tepose_debug_kernel_errors())
    run, plan, state = run_case(case, None)
    if tables in ('dense', 'edges5'):
        assert plan['smpl'] != 'smpl_small_kernel'                          # more than four weights on a vertex: not the compact tables' kernel
    if entry == 'forward':
        assert plan['tail_regressor'].startswith('collapsed')
    records, failures = DS.check_stages(run, state, smpl_np, plan, raise_on_fail=False)
    print('\n' + '\n'.join(DS.format_records(records, _id(case) + '  ')))
    if entry != 'smpl':                                                     # the same call with the 17-row evaluation regressor: only the joints change
        runJ, _, _ = run_case(case, smpl_np['J_regressor_h36m'])
        for k in run.taps:
            assert torch.equal(run.taps[k][0], runJ.taps[k][0]), k
        for k in ('theta', 'verts', 'rotmat'):
            assert torch.equal(run.out[k], runJ.out[k]), k
        recJ, failJ = DS.check_stages(runJ, state, smpl_np, plan, raise_on_fail=False, stages=('kp_3d', 'kp_2d'))
        print('\n'.join(DS.format_records(recJ, _id(case) + '  J17  ')))
        records, failures = records + recJ, failures + failJ
    if failures:
        raise DS.StageMismatch(failures)
    assert all(r['ratio'] <= 1.0 for r in records)
    assert int(_lib.load().tepose_debug_kernel_errors()) == errs0           # no wave of the barrier-free kernels gave up a poll


def test_refusals_come_before_any_launch():
    """ARG, SHAPE (a wrong count; a stage the plan never writes: pf, the plane forms and vposed under the small kernel, pf_planes on an exact handle, pf16
    below the blend16 threshold), WORKSPACE (shorter than the carve): nothing is written into the NaN-filled buffer, and a refused stage stays NaN."""
    model, state = _model({}, 'synth')
    exact, _ = _model(EXACT, 'synth')
    eng, N = model._engine, 3
    case = ('regressor', {}, 'synth', N, 3)
    ws = _poisoned(eng, N, 1)
    _call(eng, case, _inputs(case, state), ws, None)
    assert eng.select_kernels(N, 1)['smpl'] == 'smpl_small_kernel'
    big = torch.full((N * 20670 + 1,), NAN, dtype=torch.float32, device='cuda')
    for stage in ('pf', 'pf_planes', 'pf16', 'vposed'):
        assert _tap(eng, N, stage, 'regressor', ws, out=big)[0] == E_SHAPE, stage
    for stage in ('xs', 'amat', 'posed'):
        w = N * DS.WIDTH[stage]
        assert _tap(eng, N, stage, 'regressor', ws, out=big, n=w + 1)[0] == E_SHAPE and _tap(eng, N, stage, 'regressor', ws, out=big, n=w - 1)[0] == E_SHAPE, stage
        assert _tap(eng, N, stage, 'regressor', ws, out=big, ws_bytes=1024)[0] == E_WORKSPACE and _tap(eng, N, stage, 'forward', ws, out=big, ws_bytes=65536)[0] == E_WORKSPACE
    form = ctypes.c_int(-1)
    tap = lambda n=N, stage=0, out=big.data_ptr(), w=ws.data_ptr(), entry=0, T=1: eng.lib.tepose_decoder_tap(eng.handle, n, stage, out, n * 160, ctypes.byref(form), entry, T,
                                                                                                              w, ws.numel(), _stream())
    assert tap(n=0) == E_ARG and tap(stage=-1) == E_ARG and tap(stage=9) == E_ARG and tap(out=None) == E_ARG and tap(w=None) == E_ARG
    assert tap(entry=2) == E_ARG and tap(entry=1, T=0) == E_ARG
    # the general chain on a split handle keeps pf_planes but no pf16 below the threshold; an exact handle keeps neither
    N5 = 5
    for m, ok, no in ((model, ('pf', 'pf_planes', 'vposed'), ('pf16',)), (exact, ('pf', 'vposed'), ('pf_planes', 'pf16'))):
        e = m._engine
        c5 = ('regressor', {}, 'synth', N5, 3)
        w5 = _poisoned(e, N5, 1)
        _call(e, c5, _inputs(c5, state), w5, None)
        for stage in no:
            assert _tap(e, N5, stage, 'regressor', w5, out=big)[0] == E_SHAPE, stage
        torch.cuda.synchronize()
        assert bool(torch.isnan(big).all())
        for stage in ok:
            rc, f, t = _tap(e, N5, stage, 'regressor', w5)
            torch.cuda.synchronize()
            assert rc == 0 and f == (3 if stage == 'pf_planes' else 0) and bool(torch.isfinite(t).all()), stage
    torch.cuda.synchronize()
    assert bool(torch.isnan(big).all())
    rc, f, t = _tap(eng, N, 'xs', 'regressor', ws)
    torch.cuda.synchronize()
    assert rc == 0 and f == 0 and bool(torch.isfinite(t).all())
