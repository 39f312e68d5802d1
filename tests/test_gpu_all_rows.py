"""GPU: EVERY row of large batches against the fp64 oracle (tests/_replicated.py: batches of B rows that are copies of D distinct windows, laid out as
independent permutations per D-block, so one oracle run on D windows answers all B rows).

The large-batch kernels' likely faults are local -- one row tile, one unit tile, the second tile a workgroup takes, the ragged tile, a stale ring slot --
and the rest of the suite compares a few dozen rows of such batches.  Here no row is left out: encoder features in both modes and every output of the
full forward, for each kernel family the plan can select above 64 windows (CASES; tests/test_all_rows_helper.py checks that the table covers the plan),
and the clip driver in lock-step over hundreds of clips.

Tolerances are the suite's: 2e-5 on encoder features, 1e-4 on verts / kp_3d / kp_2d / rotmat / theta.  The axis-angle part of theta is compared on every
row too: each case first asserts that every oracle angle of its windows is below 3.0 rad (away from the pi singularity), so nothing is masked out.

Copies of one window must agree to 2e-5 (tile / split-K order only), and bit for bit where every 128-row tile is full and one kernel instantiation
serves all rows (B % 128 == 0 in the scaled class): the same operands through the same instruction sequence."""
import numpy as np
import pytest
import torch

import _replicated as R
from tepose_amd import synth

pytestmark = pytest.mark.gpu
TOL, TOL_FEAT, TOL_COPIES = 1e-4, 2e-5, 2e-5

# (L, H, B, T, knobs, D): D distinct windows (>= 128 from 640 rows on: no 16-, 64- or 128-row tile holds a window twice)
CASES = [
    (2, 1024, 8192, 16, {}, 128),     # the benchmark shape: barrier-free projections, frame-major blocked gi, plane-fed steps on both layers
    (2, 1024, 8192, 6, {}, 128),      # the same kernels at the published window length
    (2, 1024, 2305, 3, {}, 128),      # 128 x 288 tiles over 55 row tiles feeding the scaled class; ragged last tile of one row at the published width
    (2, 1024, 129, 6, {}, 64),        # mid class on 128 x 288 tiles, ragged last row tile (one row)
    (3, 256, 2064, 4, {}, 128),       # ragged last tile of 16 rows, B % 16 == 0: fp32-state steps on blocked operands, three layers
    (2, 64, 2050, 5, {}, 128),        # B % 16 != 0: row-major layer 0 under blocked layers >= 1
    (2, 192, 700, 3, {}, 128),        # just above the scaled threshold, B * T < 8192, Hp % 128 != 0
    (1, 320, 1000, 2, {}, 128),       # one layer
    (2, 256, 1024, 6, {}, 128),       # full tiles, B * T < 8192: fp32-state steps on row-major layer 0, plane-fed steps on blocked layer 1
    (2, 128, 300, 32, {}, 64),        # 65 <= B < 640, B * T >= 8192: barrier-free projection feeding two-accumulator steps
    (2, 128, 100, 1, {}, 64),         # width-first everything (T = 1: first steps only)
    (2, 128, 96, 2, {}, 64),          # width-first steps and layer-1 projection (192 real rows), tiled layer-0 projection
    (4, 64, 640, 3, {}, 128),         # four layers at the scaled threshold: one unit tile, three plane-fed layers over a row-major layer 0
    (2, 256, 2048, 4, {'TEPOSE_GRU_STATE': 'fp32'}, 128),
    (2, 192, 2100, 3, {'TEPOSE_LARGE_BATCH_KERNELS': 'twoacc'}, 128),
    (2, 256, 2100, 4, {'TEPOSE_EXACT_FP32': '1'}, 128),
    (2, 128, 200, 3, {'TEPOSE_EXACT_FP32': '1'}, 64),
]

_H3S0, _H3S1 = 'gemm_h3s_persist16c_kernel<0>', 'gemm_h3s_persist16c_kernel<1>'
_S16, _S16P = 'gru_step16_kernel<false>', 'gru_step16_kernel<true>'
_SMPL = 'smpl_prep_kernel+%s+smpl_skin4_kernel'
_COLLAPSED = 'collapsed: one product (skinny_gemm_h3_kernel)'
# what the plan (csrc/plan.hip select_kernels) must name for each case, index for index
PLANS = [
    dict(projection=_H3S0, gi0_layout='frame_major_blocked', gru_step=_S16P, gru_first='gru_first16_kernel', projection_l1=_H3S1, gi1_layout='blocked',
         gru_step_l1=_S16P, tail_regressor=_COLLAPSED, smpl=_SMPL % _H3S1),
    dict(projection=_H3S0, gi0_layout='frame_major_blocked', gru_step=_S16P, gru_first='gru_first16_kernel', projection_l1=_H3S1, gru_step_l1=_S16P),
    dict(projection='gemm_h3s_kernel<1, 3, 4, 3, 4>', gi0_layout='row_major', gru_step=_S16, gru_first='gru_first16_kernel', projection_l1=_H3S1,
         gi1_layout='blocked', gru_step_l1=_S16),
    dict(projection='gemm_h3s_kernel<1, 3, 4, 3, 4>', gru_step='gemm_h3_kernel<GRU>', projection_l1='gemm_h3_kernel', gi1_layout='row_major',
         gru_first='gru_first_kernel', smpl=_SMPL % 'gemm_h3_kernel'),
    dict(projection=_H3S0, gi0_layout='frame_major_blocked', gru_step=_S16, gru_first='gru_first16_kernel', projection_l1=_H3S1, gi1_layout='blocked',
         gru_step_l1=_S16, smpl=_SMPL % _H3S1),
    dict(projection=_H3S0, gi0_layout='row_major', gru_step=_S16, gru_first='gru_first_kernel', projection_l1=_H3S1, gi1_layout='blocked', gru_step_l1=_S16),
    dict(projection='gemm_h3_kernel', gi0_layout='row_major', gru_step=_S16, gru_first='gru_first_kernel', projection_l1=_H3S1, gru_step_l1=_S16),
    dict(projection='gemm_h3_kernel', gi0_layout='row_major', gru_step=_S16, gru_first='gru_first_kernel', smpl=_SMPL % _H3S1),
    dict(projection='gemm_h3_kernel', gi0_layout='row_major', gru_step=_S16, gru_first='gru_first16_kernel', gi1_layout='blocked', gru_step_l1=_S16P),
    dict(projection=_H3S0, gi0_layout='row_major', gru_step='gemm_h3_kernel<GRU>', projection_l1='gemm_h3_kernel', gru_step_l1='gemm_h3_kernel<GRU>'),
    dict(projection='skinny_gemm_h3_kernel', gru_step='skinny_gru_h3_kernel', projection_l1='skinny_gemm_h3_kernel', gru_first='gru_first_kernel'),
    dict(projection='gemm_h3_kernel', gru_step='skinny_gru_h3_kernel', projection_l1='skinny_gemm_h3_kernel', gru_step_l1='skinny_gru_h3_kernel'),
    dict(projection='gemm_h3_kernel', gi0_layout='row_major', gru_step=_S16, gru_first='gru_first_kernel', projection_l1=_H3S1, gru_step_l1=_S16P),
    dict(projection=_H3S0, gi0_layout='frame_major_blocked', gru_step=_S16, gi1_layout='blocked', gru_step_l1=_S16),
    dict(projection='gemm_h3_kernel', gi0_layout='row_major', gru_step='gemm_h3_kernel<GRU>', gi1_layout='row_major', gru_step_l1='gemm_h3_kernel<GRU>',
         smpl=_SMPL % 'gemm_h3_kernel'),
    dict(projection='gemm_f32_kernel', gru_step='gru_step_kernel', gru_first='gru_step_kernel', projection_l1='gemm_f32_kernel', smpl=_SMPL % 'gemm_f32_kernel'),
    dict(projection='skinny_gemm_kernel', gru_step='skinny_gru_kernel', gru_first='skinny_gru_kernel', projection_l1='skinny_gemm_kernel',
         smpl=_SMPL % 'skinny_gemm_kernel'),
]
assert len(PLANS) == len(CASES)

# lock-step driver: clips, distinct clips, window, model (the window plan of 704 ... 768 concurrent clips: fp32-state steps, the pair product split in two)
LOCKSTEP = dict(C=768, D=32, T=4, L=2, H=64)


@pytest.fixture(scope='module')
def smpl_np():
    return synth.synthetic_smpl(0)


def _model(L, H, knobs, smpl_np, monkeypatch, seed=11):
    from tepose_amd.testing import build_model
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)             # read when the handle is created
    model, state, _ = build_model(L, H, seed=seed, device='cuda', smpl_np=smpl_np)
    for k in knobs:
        monkeypatch.delenv(k)
    return model, state


def window_seed(L, H, B, T):
    """The synthetic windows' seed of a case: a function of its shape, so that adding a case leaves the others' inputs alone."""
    return 4200 + (31 * L + 7 * H + 3 * B + T) % 997


def _max_angle(theta):
    return float(theta[:, 3:75].reshape(-1, 3).double().norm(dim=1).max())


@pytest.mark.parametrize('case', range(len(CASES)), ids=['L%dH%dB%dT%d%s' % (c[0], c[1], c[2], c[3], ''.join('-' + v for v in c[4].values())) for c in CASES])
def test_every_row_against_the_fp64_oracle(case, smpl_np, monkeypatch):
    """Features (both modes) and all outputs of the full forward on all B rows; copies of one window within 2e-5 of each other, and bit-identical where
    all row tiles are full in the scaled class."""
    from oracle import tepose_ref as O
    from tepose_amd import _lib
    L, H, B, T, knobs, D = CASES[case]
    errs0 = int(_lib.load().tepose_debug_kernel_errors())
    model, state = _model(L, H, knobs, smpl_np, monkeypatch)
    sel = model._engine.select_kernels(B, T)
    for k, v in PLANS[case].items():
        assert sel.get(k) == v, (k, sel.get(k), v)
    x, xw, src = R.replicated_windows(B, T, D, window_seed(L, H, B, T), 'cuda')
    Jn = smpl_np['J_regressor_h36m']
    with torch.no_grad():
        got = dict(model(x, J_regressor=torch.from_numpy(Jn))[0])
        got['feature'] = model.encoder(x)
        got['feature_train'] = model.encoder(x, is_train=True)
    torch.cuda.synchronize()
    del x
    # the fp64 oracle on the D distinct windows only
    ref = O.tepose_fwd(state, smpl_np, xw, L, J_regressor=Jn, dtype=torch.float64)
    enc, _ = O.split_state_dict(state, torch.float64)
    with torch.no_grad():
        ref['feature_train'] = O.encoder_fwd(enc, torch.from_numpy(xw).double(), L, is_train=True)
    assert got['feature'].shape == (B, 2048) and got['feature_train'].shape == (B, 2, 2048) and got['verts'].shape == (B, 6890, 3)
    names = ('feature', 'feature_train', 'verts', 'kp_3d', 'kp_2d', 'rotmat', 'theta')
    tols = {k: TOL_FEAT if k.startswith('feature') else TOL for k in names}
    assert _max_angle(ref['theta']) < 3.0            # no axis-angle near the pi singularity: all of theta[:, 3:75] is compared below
    sep = R.assert_separated({k: ref[k] for k in names}, tols)
    reps = [R.compare_all_rows(got[k], ref[k], src, tols[k], name=k, raise_on_fail=False) for k in names]
    spread = {k: R.copies_spread(got[k], src) for k in names}
    ident = {k: R.copies_bit_identical(got[k], src) for k in names}
    print('\n  all rows L=%d H=%d B=%d T=%d %s D=%d: worst features %.2e, outputs %.2e; copies spread %.2e, bit-identical %s; min separation %.0f x tol' % (
        L, H, B, T, knobs or '', D, max(r.worst for r in reps[:2]), max(r.worst for r in reps[2:]), max(spread.values()), all(ident.values()), min(sep.values())))
    for r in reps:
        print('    ' + R.describe(r))
    for r in reps:
        assert r.rows == B                           # B of B rows compared
        assert r.n_over == 0, R.describe(r)
    for k in names:
        assert spread[k] <= TOL_COPIES, (k, spread[k])
    if B % 128 == 0 and sel['gru_step'].startswith('gru_step16'):
        assert all(ident.values()), ident
    assert int(_lib.load().tepose_debug_kernel_errors()) == errs0      # no wave of the barrier-free kernels gave up a poll


def test_lockstep_clips_every_clip_against_the_fp64_oracle(smpl_np, monkeypatch):
    """run_clips with the projection cache on over 768 clips that are copies of 32 distinct clips (features + initial thetas; copies share a length,
    lengths differ across distinct clips, one is shorter than the window): every clip, every window, theta / kp_3d / verts / rotmat against O.run_clip
    in float64 once per distinct clip."""
    from oracle import tepose_ref as O
    from tepose_amd.driver import run_clips
    C, D, T, L, H = (LOCKSTEP[k] for k in 'CDTLH')
    model, state = _model(L, H, {}, smpl_np, monkeypatch, seed=21)
    src = R.assignment(C, D, 77)
    w = synth.synthetic_windows(D, T + 6, 78)
    lens = [T + 5 + d % 2 - 3 * (d % 16 == 5) - (d % 16 == 11) for d in range(D)]      # 6 or 7 windows per clip; two clips 4
    lens[16] = T - 1                                                                       # shorter than the window: skipped, copies too
    active = sum(1 for s in src if lens[s] >= T)
    sel = model._engine.select_kernels(active, T)
    assert 704 <= active <= 768 and sel['projection_window'] == 'skinny_gemm_h3_kernel x 2' and sel['gru_step_window'] == 'gru_step16_kernel<false>'
    feats_d = [torch.from_numpy(w[d, :lens[d], :2048].copy()) for d in range(D)]
    inits_d = [torch.from_numpy(w[d, :T - 1, 2048:].copy()) for d in range(D)]
    res = run_clips(model, [feats_d[s] for s in src], [inits_d[s] for s in src], T, cache_projections=True)
    refs = [O.run_clip(state, smpl_np, feats_d[d].numpy(), inits_d[d].numpy(), T, L, dtype=torch.float64) if lens[d] >= T else None for d in range(D)]
    assert max(_max_angle(r['theta']) for r in refs if r is not None) < 3.0
    for j in (0, 3):        # the distinct clips' answers are far apart (first window; the last one all running clips have), as for the window batches
        R.assert_separated({k: torch.stack([r[k][j] for r in refs if r is not None]) for k in ('theta', 'kp_3d', 'verts', 'rotmat')},
                           dict(theta=TOL, kp_3d=TOL, verts=TOL, rotmat=TOL))
    compared, worst = 0, 0.0
    for i in range(C):
        assert (res[i] is None) == (refs[src[i]] is None), i
    for j in range(max(lens) - T + 1):                   # window j of every clip that has one: rows = clips, in input order
        clips = [i for i in range(C) if lens[src[i]] - T + 1 > j]
        for k in ('theta', 'kp_3d', 'verts', 'rotmat'):
            got = torch.stack([res[i][k][j] for i in clips])
            ref = torch.stack([refs[d][k][j] if lens[d] - T + 1 > j else torch.zeros_like(refs[0][k][0]) for d in range(D)])
            rep = R.compare_all_rows(got, ref, src[clips], TOL, name='window %d %s' % (j, k), raise_on_fail=False)
            assert rep.n_over == 0, R.describe(rep) + ' (rows are the clips with such a window; the worst row is clip %d)' % clips[rep.row]
            worst = max(worst, rep.worst)
        compared += len(clips)
    assert compared == sum(lens[s] - T + 1 for s in src if lens[s] >= T)      # every window of every clip
    print('\n  lock-step %d clips (%d active, %d distinct): %d clip-windows, worst %.2e' % (C, active, D, compared, worst))
