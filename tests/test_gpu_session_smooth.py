"""GPU: tepose_session_smooth alone (csrc/filters.hip session_smooth_kernel) -- the one-euro step of a live session's slots,
handle-less and without a model.  Every slot runs its own schedule of joins, advances, holds and clears; per slot and life (join .. clear) the
history pose rows and the advanced theta rows are stacked and tepose_filter_one_euro runs over the stack: every tick's pose_hat is the matching row
in every bit, and so is the state.  cam and betas are copies; a slot that neither advances nor joins gives zero rows and reads nothing (its theta
and hist rows hold NaN); saved_state is the state before the call, and putting it back repeats the call bit for bit.  No tolerance appears here."""
import numpy as np
import pytest
import torch

import _buffers as BUF

pytestmark = pytest.mark.gpu
BASE = [2, 1, 0, 1, 3, 2, 1]                  # join, advance, hold, advance, clear, join again, advance
IDLE = [0, 9, -1]                             # what a slot shows before its schedule starts: 0 and two values outside 0 .. 3 (they act as 0)
TICKS = len(BASE) + 2


def _schedule(s):
    """Slot s: s % 3 idle ticks, then BASE (every third slot joins again WITHOUT a clear in between), then holds or advances; all live at the end."""
    base = list(BASE)
    if s % 3 == 2:
        base[4] = 1
    ops = IDLE[:s % 3] + base
    return ops + [1 if s % 2 else 0] * (TICKS - len(ops))


def _call(lib, theta, hist, S, T, ops, state, saved, mc, beta, outs):
    for o in outs:
        o.own.view(torch.int32).fill_(-1)                                     # NaN: a row the kernel leaves out shows
    rc = lib.tepose_session_smooth(theta.data_ptr(), None if hist is None else hist.data_ptr(), S, T, ops.data_ptr(), state.data_ptr(),
                                   None if saved is None else saved.data_ptr(), mc, beta, 1.0, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return [o.own.clone() for o in outs]


@pytest.mark.parametrize('mc,beta', [(0.004, 0.7), (0.35, 0.05)], ids=['demo', 'stiff'])
@pytest.mark.parametrize('T', [2, 4])
@pytest.mark.parametrize('S', [1, 3, 64])
def test_every_tick_equals_the_whole_sequence_filter_bit_for_bit(S, T, mc, beta):
    from tepose_amd import _lib, filters
    lib = _lib.load()
    dev = 'cuda'
    rng = np.random.default_rng(100 * S + T)
    sched = np.array([_schedule(s) for s in range(S)], dtype=np.int32)        # [S, TICKS]
    assert sched.shape == (S, TICKS) and {0, 1, 2, 3} <= set(sched[0].tolist())
    # a block serves 128 / 85 slots' columns: an index off by one slot stays within two slots of guard on each side
    state = BUF.guarded_like((S, 2, 72), S, dev, name='state', guard_rows=2)
    saved = BUF.guarded_like((S, 2, 72), S, dev, name='saved_state', guard_rows=2)
    outs = [BUF.guarded_like((S, w), S, dev, name=n, guard_rows=2) for n, w in (('theta_hat', 85), ('pose_hat', 72), ('betas_hat', 10))]
    state.own.zero_()
    seq = [None] * S                               # per slot: the rows of its current life (history pose rows, then advanced theta rows)
    got = [None] * S                               # ... and what the kernel gave for the advanced rows
    lives = []                                     # finished (rows, outputs) pairs

    def tick(ops_np, what):
        live = np.isin(ops_np, (1, 2))
        theta_np = rng.uniform(-np.pi, np.pi, (S, 85)).astype(np.float32)
        hist_np = rng.uniform(-np.pi, np.pi, (S, T - 1, 2133)).astype(np.float32)
        theta_np[~live] = np.nan                                              # not read: a NaN would reach the zero rows or the state
        hist_np[ops_np != 2] = np.nan
        theta, hist, ops = (torch.from_numpy(a).to(dev) for a in (theta_np, hist_np, ops_np))
        frozen = BUF.Frozen(theta=theta, hist=hist, ops=ops)
        before = state.own.clone()
        saved.own.view(torch.int32).fill_(-1)
        th, ph, bh = _call(lib, theta, hist, S, T, ops, state, saved, mc, beta, outs)
        after = state.own.clone()
        assert BUF.same_bits(saved.own, before), what                         # every slot, whatever its op
        # restore: the saved state put back, the same call again (no saved_state this time) -> every output bit and the state again
        state.own.copy_(saved.own)
        again = _call(lib, theta, hist, S, T, ops, state, None, mc, beta, outs)
        assert all(BUF.same_bits(a, b) for a, b in zip(again, (th, ph, bh))) and BUF.same_bits(state.own, after), what
        BUF.assert_guards_intact(state, saved, *outs, what=what)
        frozen.assert_unchanged(what)
        for t in (th, ph, bh, after):
            assert bool(torch.isfinite(t).all()), what                        # no NaN anywhere
        th_np, ph_np = th.cpu().numpy(), ph.cpu().numpy()
        for s in range(S):
            op = int(ops_np[s])
            if op in (1, 2):
                assert np.array_equal(th_np[s, :3].view(np.uint32), theta_np[s, :3].view(np.uint32)), (what, s)       # cam, betas: copies
                assert np.array_equal(th_np[s, 75:].view(np.uint32), theta_np[s, 75:].view(np.uint32)), (what, s)
                assert BUF.same_bits(bh[s], th[s, 75:]) and BUF.same_bits(ph[s], th[s, 3:75]), (what, s)
                if op == 2:
                    if seq[s] is not None:
                        lives.append((seq[s], got[s]))                        # a join over a live slot: the old life ends here
                    seq[s], got[s] = [hist_np[s, r, 2048 + 3:2048 + 75] for r in range(T - 1)], []
                seq[s].append(theta_np[s, 3:75])
                got[s].append((ph_np[s].copy(), after[s].cpu().numpy()))
            else:
                assert not th[s].any() and not ph[s].any() and not bh[s].any(), (what, s)                             # zero rows
                if op == 3:
                    assert not after[s].any(), (what, s)
                    lives.append((seq[s], got[s]))
                    seq[s], got[s] = None, None
                else:
                    assert BUF.same_bits(after[s], before[s]), (what, s)      # held: not one bit of the state moved

    for j in range(TICKS):
        tick(sched[:, j].copy(), 'S=%d T=%d tick %d ops=%s' % (S, T, j, sched[:, j].tolist()[:8]))
    assert all(q is not None for q in seq)
    tick(np.ones(S, dtype=np.int32), 'S=%d T=%d the common step' % (S, T))      # dx^ of the last scheduled tick shows in this step's rows
    lives += [(seq[s], got[s]) for s in range(S)]
    assert len(lives) >= 2 * S
    for rows, outs_ in lives:
        n = len(outs_)
        assert len(rows) == T - 1 + n and n >= 2
        want = filters.one_euro(np.stack(rows), min_cutoff=mc, beta=beta).cpu().numpy()         # tepose_filter_one_euro over the stack
        assert np.array_equal(want[0].view(np.uint32), rows[0].view(np.uint32))                  # the first history row passes through
        for i, (ph, st) in enumerate(outs_):
            assert np.array_equal(ph.view(np.uint32), want[T - 1 + i].view(np.uint32)), (S, T, n, i)
            assert np.array_equal(st[0].view(np.uint32), want[T - 1 + i].view(np.uint32)), (S, T, n, i)      # x^ of the state; dx^: the next row


def test_a_join_without_history_holds():
    from tepose_amd import _lib
    lib = _lib.load()
    S, T = 3, 4
    state = torch.randn(S, 2, 72, device='cuda')
    before = state.clone()
    theta = torch.full((S, 85), float('nan'), device='cuda')
    ops = torch.full((S,), 2, dtype=torch.int32, device='cuda')
    outs = [torch.full((S, w), float('nan'), device='cuda') for w in (85, 72, 10)]
    rc = lib.tepose_session_smooth(theta.data_ptr(), None, S, T, ops.data_ptr(), state.data_ptr(), None, 0.004, 0.7, 1.0, outs[0].data_ptr(),
                                   outs[1].data_ptr(), outs[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert BUF.same_bits(state, before) and not any(bool(o.any()) for o in outs)      # nothing is read through the null pointer
