"""CPU: the poisoned / guarded buffers of tests/_buffers.py checked on their own -- a planted write outside an owned region is reported with its
offset, one inside is not, the patterns read as the contract's tests need them to -- and the case table of tests/test_gpu_buffers.py reaches every
kernel family the plan (csrc/plan.hip) can select, the small-batch ones included."""
import os
import re

import pytest
import torch

import _buffers as BF
from test_all_rows_helper import _built, _select  # noqa: F401  (the fixture that builds the library; plans from a subprocess with TEPOSE_ASSUME_CUS=256)
from test_gpu_buffers import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the helper -------------------------------------------------------------------------------------------------------------------------------------
def test_guard_sizes_are_one_row_tile_of_the_widest_buffer():
    assert BF.GUARD_ROWS == 128
    assert BF.workspace_guard_bytes(1024) == 128 * 9 * 1024 * 4 and BF.workspace_guard_bytes(64) % 256 == 0
    t = BF.guarded_like((5, 6890, 3), 5, 'cpu')
    assert t.guard.lo == 128 * 6890 * 3 * 4 and t.guard.base.numel() - t.guard.hi == t.guard.lo


@pytest.mark.parametrize('pattern', sorted(BF.PATTERNS))
def test_poisoned_workspace_layout(pattern):
    ws = BF.poisoned(1000, pattern, 'cpu', guard_bytes=300)
    g = ws.guard
    assert ws.numel() == 1000 and ws.dtype == torch.uint8 and ws.is_contiguous()
    assert ws.data_ptr() % 256 == 0 and ws.data_ptr() == g.base.data_ptr() + g.lo and g.hi - g.lo == 1000
    assert g.lo >= 512 and g.base.numel() - g.hi >= 512         # 300 bytes of guard, rounded up to 256, on either side
    assert (g.lo - (-g.base.data_ptr()) % 256) % 256 == 0       # a multiple of 256 from a 256-byte-aligned allocation (every device allocation is one)
    assert bool((g.base[:g.lo] == BF.GUARD_BYTE).all()) and bool((g.base[g.hi:] == BF.GUARD_BYTE).all())
    assert not bool((ws == BF.GUARD_BYTE).any())                 # the guards hold a fourth pattern
    BF.assert_guards_intact(ws)
    assert ws[:8].tolist() == list(BF.PATTERNS[pattern]) * 4


def test_patterns_read_as_the_tests_need_them():
    ones = BF.poisoned(4096, 'ones', 'cpu', guard_bytes=256)
    assert bool(torch.isnan(ones.view(torch.float32)).all()) and bool(torch.isnan(ones.view(torch.float16)).all())
    assert bool((ones.view(torch.int32) == -1).all())            # 0xFFFFFFFF: as a counter, a tag or an index
    fin = BF.poisoned(4096, 'finite', 'cpu', guard_bytes=256)
    f32, f16 = fin.view(torch.float32), fin.view(torch.float16)
    assert bool(torch.isfinite(f32).all()) and bool((f32 != 0).all()) and bool((f16 == 1.0).all())
    assert bool((fin.view(torch.int16) == 0x3C00).all()) and 0 < float(f32[0]) < 0.01
    zeros = BF.poisoned(4096, 'zeros', 'cpu', guard_bytes=256)
    assert not bool(zeros.any())
    assert bool((BF.refill(zeros, 'ones') == 0xFF).all()) and zeros.guard.name.endswith('(ones)')
    BF.assert_guards_intact(zeros, ones, fin)
    assert BF.untouched(zeros) and BF.untouched(fin) and BF.untouched(ones)
    fin[1001] = 0x3D
    assert not BF.untouched(fin)                                 # a workspace the call under test never used would make every poison test vacuous


@pytest.mark.parametrize('side', ['front', 'behind'])
def test_a_one_byte_write_outside_a_workspace_is_reported_with_its_offset(side):
    ws = BF.poisoned(1000, 'finite', 'cpu', guard_bytes=256)
    g = ws.guard
    off = -1 if side == 'front' else 1000
    g.base[g.lo + off] = 0
    assert g.changed() == (off, off, 1)
    with pytest.raises(AssertionError, match=r'case 7: workspace \(finite\) written outside its owned 1000 bytes: 1 guard bytes changed, first at offset %d, last at offset %d' % (off, off)):
        BF.assert_guards_intact(ws, what='case 7')


def test_first_and_last_changed_offsets_span_both_guards():
    ws = BF.poisoned(512, 'zeros', 'cpu', guard_bytes=256)
    g = ws.guard
    g.base[g.lo - 246] = 1
    g.base[g.hi + 200] = 1
    assert g.changed() == (-246, 512 + 200, 2)


def test_a_write_inside_is_not_reported():
    ws = BF.poisoned(1000, 'ones', 'cpu', guard_bytes=256)
    ws[0] = 1
    ws[999] = 2
    ws[500:600] = BF.GUARD_BYTE
    BF.assert_guards_intact(ws)
    out = BF.guarded_like((7, 49, 3), 7, 'cpu')
    out.own.fill_(3.0)
    BF.assert_guards_intact(out, {'a': out, 'b': None}, None, [out, ws])


@pytest.mark.parametrize('row,word', [(-1, 146), (7, 0), (7 + 127, 146)])
def test_a_row_written_next_to_the_owned_rows_of_an_output_is_reported(row, word):
    out = BF.guarded_like((7, 49, 3), 7, 'cpu', name='kp_3d')
    assert tuple(out.shape) == (7 + 128, 49, 3) and tuple(out.own.shape) == (7, 49, 3) and out.is_contiguous() and out.own.data_ptr() == out.data_ptr()
    assert bool(torch.isnan(out.own).all())                      # owned rows start as NaN
    whole = out.guard.base.view(torch.float32).view(128 + 7 + 128, 147)
    whole[128 + row, word] = 0.0
    first, last, n = out.guard.changed()
    assert first == (row * 147 + word) * 4 and last - first == 3 and n == 4       # 0xA5A5A5A5 -> 0.0 changes four bytes
    with pytest.raises(AssertionError, match='kp_3d written outside'):
        BF.assert_guards_intact({'kp_3d': out})


def test_frozen_inputs_compare_bitwise():
    x, y = torch.tensor([0.0, float('nan'), 1.0]), torch.tensor([1, 2, 3])
    fr = BF.Frozen(x=x, y=y, absent=None)
    fr.assert_unchanged()
    x[0] = -0.0                                                  # equal as a number, another bit pattern
    with pytest.raises(AssertionError, match="input 'x' was written"):
        fr.assert_unchanged('case')
    assert BF.same_bits(torch.tensor([float('nan')]), torch.tensor([float('nan')])) and not BF.same_bits(torch.zeros(2), torch.zeros(3))


# ---- plan coverage ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def plans(_built):  # noqa: F811
    out = [None] * len(CASES)
    for env in {tuple(sorted(c[4].items())) for c in CASES}:            # a subprocess per environment
        idx = [i for i, c in enumerate(CASES) if tuple(sorted(c[4].items())) == env]
        for i, sel in zip(idx, _select([CASES[i][:4] for i in idx], dict(env))):
            out[i] = sel
    return out


def test_case_table_covers_the_plan(plans):
    """EVERY entry of the name(Mm), name(Step), name(First), name(Smpl) and name(Rows) tables of today's plan.hip, both values of both layouts, the three
    tail_regressor variants and both forms of the window projection: a kernel family added to the plan later fails here until CASES has a case for it."""
    src = open(os.path.join(ROOT, 'tepose_amd', 'csrc', 'plan.hip')).read()

    def table(sig):
        i = src.index('const char* name(%s v)' % sig)
        j = min(k for k in (src.find('const char* name(', i + 1), src.find('std::string tail_name', i)) if k > 0)       # up to the next table
        return set(re.findall(r'"([^"]+)"', src[i:j]))
    want = {k: table(k) for k in ('Rows', 'Mm', 'Step', 'First', 'Smpl')}
    assert all(want.values()), want
    seen = {k: set() for k in ('Rows', 'Mm', 'Step', 'First', 'Smpl', 'gi0_layout', 'gi1_layout', 'tail', 'window')}
    for sel in plans:
        seen['Rows'].add(sel['input'])
        seen['Mm'] |= {sel[k] for k in ('projection', 'projection_l1', 'projection_one_step') if k in sel}
        seen['Step'] |= {sel[k] for k in ('gru_step', 'gru_step_l1') if k in sel}
        seen['First'].add(sel['gru_first'])
        seen['Smpl'].add(sel['smpl'])
        for k in ('gi0_layout', 'gi1_layout'):
            if k in sel:
                seen[k].add(sel[k])
        t = sel['tail_regressor']
        seen['tail'].add('collapsed' if t.startswith('collapsed') else 'reg_seq_kernel' if t == 'reg_seq_kernel' else 'loop' if t.endswith(' loop') else t)
        seen['window'].add('pair' if sel['projection_window'].endswith('(pair)') else 'x 2' if sel['projection_window'].endswith(' x 2') else '?')
    for k in ('Rows', 'Mm', 'Step', 'First', 'Smpl'):
        assert seen[k] == want[k], (k, want[k] ^ seen[k])
    assert seen['gi0_layout'] == {'row_major', 'frame_major_blocked'} and seen['gi1_layout'] == {'row_major', 'blocked'}
    assert {'collapsed', 'reg_seq_kernel', 'loop'} <= seen['tail'], seen['tail']
    assert seen['window'] == {'pair', 'x 2'}, seen['window']


def test_the_table_keeps_the_edges_it_was_chosen_for(plans):
    """Ragged row tiles (B % 128 == 1, B % 16 != 0, a ragged 16-row tile), Hp > H, T = 1, one and three layers, granule and counter mode."""
    shapes = [c[:4] for c in CASES]
    assert any(B % 128 == 1 and B > 128 for _, _, B, _ in shapes) and any(B % 16 and B > 2048 for _, _, B, _ in shapes)
    assert any(B % 128 == 16 for _, _, B, _ in shapes) and any(H % 64 for _, H, _, _ in shapes) and any(T == 1 for _, _, _, T in shapes)
    assert {1, 2, 3} <= {L for L, _, _, _ in shapes}
    steps = {sel['gru_step'] for sel in plans}
    assert {'gru_seq_kernel', 'gru_seq_kernel(granules)'} <= steps
