"""CPU: the whole-batch comparison of tests/test_gpu_all_rows.py checked on its own -- the row assignment has the properties the argument needs, the
comparison reports planted faults at the right row and tile, and the case table covers every kernel family the plan can select above 64 windows."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _replicated as R
from test_gpu_all_rows import CASES, LOCKSTEP, PLANS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('B,D', sorted({(c[2], c[5]) for c in CASES} | {(LOCKSTEP['C'], LOCKSTEP['D'])}))
def test_assignment_properties(B, D):
    src = R.assignment(B, D, 3)
    assert src.dtype == np.int64 and src.shape == (B,)
    assert np.array_equal(src, R.assignment(B, D, 3)) and not np.array_equal(src, R.assignment(B, D, 4))      # a pure function of its arguments
    assert np.array_equal(np.unique(src), np.arange(D))                                                       # every window occurs
    blocks = [src[a:a + D] for a in range(0, B, D)]
    for blk in blocks:
        assert len(np.unique(blk)) == len(blk)                   # D consecutive rows from a multiple of D on: all different
    full = [tuple(b) for b in blocks if len(b) == D]
    assert len(set(full)) == len(full)                           # different aligned blocks are different permutations
    if D >= 128 and B >= 640:
        for rows in (16, 64, 128):                               # no row tile of the large-batch kernels holds a window twice
            assert all(len(np.unique(src[a:a + rows])) == len(src[a:a + rows]) for a in range(0, B, rows))


def _planted(B=1100, D=128, W=37, seed=5):
    src = R.assignment(B, D, seed)
    ref = np.random.RandomState(seed).standard_normal((D, W, 3))            # rows far apart compared with the tolerance
    got = torch.from_numpy(ref[src]).float()
    return src, ref, got


def test_comparison_passes_a_clean_batch_and_counts_every_row():
    src, ref, got = _planted()
    rep = R.compare_all_rows(got, ref, src, 1e-4, name='clean')
    assert rep.rows == 1100 and rep.n_over == 0 and rep.bad_tiles == [] and rep.worst < 1e-6       # float32 rounding of the reference
    assert R.copies_spread(got, src) == 0.0 and R.copies_bit_identical(got, src)


def test_one_element_over_tolerance_is_reported_with_its_row_and_tile():
    src, ref, got = _planted()
    got[701, 11, 2] += 2e-4                                       # (a) 2 x tol on one element of one row
    rep = R.compare_all_rows(got, ref, src, 1e-4, name='a', raise_on_fail=False)
    assert (rep.row, rep.tile, rep.window, rep.n_over, rep.bad_tiles) == (701, 701 // 128, int(src[701]), 1, [5])
    assert 1.9e-4 < rep.worst < 2.1e-4
    with pytest.raises(AssertionError) as e:
        R.compare_all_rows(got, ref, src, 1e-4, name='a')
    msg = str(e.value)
    assert 'row 701 ' in msg and 'tile 5,' in msg and 'window %d)' % src[701] in msg and '1 of 1100 rows' in msg
    assert R.copies_spread(got, src) > 1.9e-4 and not R.copies_bit_identical(got, src)


def test_a_block_that_received_its_neighbours_rows_is_reported():
    src, ref, got = _planted()
    got[272:288] = got[288:304].clone()                           # (b) one 16-row block overwritten with the neighbouring block's rows
    assert not set(src[272:288]) & set(src[288:304])              # (same aligned D-block: no window twice)
    rep = R.compare_all_rows(got, ref, src, 1e-4, name='b', raise_on_fail=False)
    assert rep.n_over == 16 and rep.bad_tiles == [2] and 272 <= rep.row < 288 and rep.tile == 2 and rep.window == src[rep.row]
    with pytest.raises(AssertionError, match='16 of 1100 rows'):
        R.compare_all_rows(got, ref, src, 1e-4, name='b')


def test_a_nan_row_counts_as_over_tolerance():
    src, ref, got = _planted()
    got[1099, 0, 0] = float('nan')
    rep = R.compare_all_rows(got, ref, src, 1e-4, raise_on_fail=False)
    assert rep.n_over == 1 and rep.row == 1099 and rep.tile == 8
    assert not R.copies_spread(got, src) <= 2e-5


def test_a_row_overwritten_by_another_copy_of_its_own_window_is_invisible():
    """(c) The one thing replication cannot see: a row that received the data of a row holding the SAME window.  For a row that received some other
    row's data that is a 1-in-D event (no other row of its aligned D-block holds its window at all), independent in every D-block since the blocks are
    different permutations: a fault that repeats per tile or per workgroup passes with probability D ** -n over n affected rows."""
    src, ref, got = _planted()
    a, b = np.nonzero(src == src[300])[0][:2]
    got[a] = got[b].clone()
    assert R.compare_all_rows(got, ref, src, 1e-4).n_over == 0
    assert R.copies_bit_identical(got, src)


def test_separation_guard():
    ref = np.zeros((4, 5))
    ref[:, 0] = [0.0, 1.0, 2.0, 2.0 + 1.5e-4]
    assert abs(R.separation(ref) - 1.5e-4) < 1e-12
    with pytest.raises(AssertionError, match='too close'):
        R.assert_separated({'kp_3d': ref}, {'kp_3d': 1e-4})            # 1.5 x: not > 2 x
    assert R.assert_separated({'kp_3d': ref}, {'kp_3d': 5e-5})['kp_3d'] == pytest.approx(3.0)
    with pytest.raises(AssertionError, match='too close'):
        R.assert_separated({'verts': ref}, {'verts': 5e-5})            # verts need 50 x


# ---- plan coverage ----------------------------------------------------------------------------------------------------------------------------------
# Every symbol csrc/plan.hip's name() tables can return for more than 64 windows, written out: all of Mm; Step without the two gru_seq_kernel entries
# (B <= 64); First without "(in gru_seq_kernel)"; Smpl without smpl_small_kernel (<= 4 persons); both values of both layouts.  A kernel family added to
# the plan later fails test_case_table_covers_the_plan until CASES has a whole-batch case for it.
_MM = {'gemm_f32_kernel', 'skinny_gemm_kernel', 'gemm_h3_kernel', 'skinny_gemm_h3_kernel', 'gemm_h3s_kernel<1, 3, 4, 3, 4>',
       'gemm_h3s_persist16c_kernel<0>', 'gemm_h3s_persist16c_kernel<1>'}
_STEP = {'gru_step_kernel', 'skinny_gru_kernel', 'gemm_h3_kernel<GRU>', 'skinny_gru_h3_kernel', 'gru_step16_kernel<false>', 'gru_step16_kernel<true>'}
_FIRST = {'gru_step_kernel', 'skinny_gru_kernel', 'gru_first_kernel', 'gru_first16_kernel'}
_SMPL = {'smpl_prep_kernel+gemm_f32_kernel+smpl_skin4_kernel', 'smpl_prep_kernel+skinny_gemm_kernel+smpl_skin4_kernel',
         'smpl_prep_kernel+gemm_h3_kernel+smpl_skin4_kernel', 'smpl_prep_kernel+gemm_h3s_persist16c_kernel<1>+smpl_skin4_kernel'}
_NOT_ABOVE_64 = {'gru_seq_kernel', 'gru_seq_kernel(granules)', '(in gru_seq_kernel)', 'smpl_small_kernel'}


def _select(shapes, env):
    """select_kernels of every (L, H, B, T) of `shapes` from ONE fresh process with the knobs `env` (read when a handle is created)."""
    code = ("import json, sys\nsys.path.insert(0, %r)\nfrom tepose_amd.engine import Engine\n"
            "print(json.dumps([Engine(L, H).select_kernels(B, T) for L, H, B, T in %r]))" % (ROOT, [tuple(s) for s in shapes]))
    e = dict(os.environ, TEPOSE_ASSUME_CUS='256')
    for k in ('TEPOSE_EXACT_FP32', 'TEPOSE_LARGE_BATCH_KERNELS', 'TEPOSE_GRU_STATE', 'TEPOSE_S_MIN_B', 'TEPOSE_GI_BLK', 'TEPOSE_PERSISTENT'):
        e.pop(k, None)
    e.update(env)
    out = subprocess.run([sys.executable, '-c', code], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope='module')
def _built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope='module')
def plans(_built):
    out = [None] * len(CASES)
    for env in {tuple(sorted(c[4].items())) for c in CASES}:            # a subprocess per environment
        idx = [i for i, c in enumerate(CASES) if tuple(sorted(c[4].items())) == env]
        for i, sel in zip(idx, _select([CASES[i][:4] for i in idx], dict(env))):
            out[i] = sel
    return out


def test_every_case_selects_what_the_gpu_test_expects(plans):
    for case, sel, want in zip(CASES, plans, PLANS):
        for k, v in want.items():
            assert sel.get(k) == v, (case, k, sel.get(k), v)


def test_case_table_covers_the_plan(plans):
    src = open(os.path.join(ROOT, 'tepose_amd', 'csrc', 'plan.hip')).read()
    for sym in _MM | _STEP | _FIRST | _SMPL | _NOT_ABOVE_64:            # the literal sets are the name() tables of today's plan.hip, no more, no less
        assert '"%s"' % sym in src, sym
    tables = src[src.index('const char* name(Mm v)'):src.index('std::string tail_name')]
    assert set(re.findall(r'"([^"]+)"', tables)) == _MM | _STEP | _FIRST | _SMPL | _NOT_ABOVE_64
    seen = {k: set() for k in ('mm', 'step', 'first', 'smpl', 'gi0_layout', 'gi1_layout')}
    for sel in plans:
        seen['mm'] |= {sel[k] for k in ('projection', 'projection_l1') if k in sel}
        seen['step'] |= {sel[k] for k in ('gru_step', 'gru_step_l1') if k in sel}
        seen['first'].add(sel['gru_first'])
        seen['smpl'].add(sel['smpl'])
        for k in ('gi0_layout', 'gi1_layout'):
            if k in sel:
                seen[k].add(sel[k])
    assert seen['mm'] == _MM, _MM ^ seen['mm']
    assert seen['step'] == _STEP, _STEP ^ seen['step']
    assert seen['first'] == _FIRST, _FIRST ^ seen['first']
    assert seen['smpl'] == _SMPL, _SMPL ^ seen['smpl']
    assert seen['gi0_layout'] == {'row_major', 'frame_major_blocked'} and seen['gi1_layout'] == {'row_major', 'blocked'}


def test_lockstep_shape_plans_the_split_pair_product(_built):
    C, T = LOCKSTEP['C'] - LOCKSTEP['C'] // LOCKSTEP['D'], LOCKSTEP['T']          # one distinct clip is shorter than the window
    for B, sel in zip((704, C, 768), _select([(LOCKSTEP['L'], LOCKSTEP['H'], B, T) for B in (704, C, 768)], {})):
        assert sel['projection_window'] == 'skinny_gemm_h3_kernel x 2' and sel['gru_step_window'] == 'gru_step16_kernel<false>', (B, sel)
