"""CPU: the argument checks of tepose_session_advance / tepose_session_commit, which return before any device call, the numpy restatement of
the window ops (tests/_session_ref.py) against the shift StreamSession._tick defines, the slot bookkeeping errors that need no device, and
that the live sessions share one base (tepose_amd/stream.py)."""
import numpy as np
import pytest

import _session_ref as R

E_ARG, E_SHAPE = -1, -2


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from tepose_amd import _lib
    return _lib.load()


def test_every_argument_error_of_the_two_entry_points_without_a_device(lib):
    P = 4096                                                       # a non-null pointer value: never dereferenced, every call returns before a device call
    ok = dict(win=P, saved=P, S=4, T=6, ops=P, feat=P, hist=P, theta=P)

    def adv(**kw):
        a = dict(ok, **kw)
        return lib.tepose_session_advance(a['win'], a['saved'], a['S'], a['T'], a['ops'], a['feat'], a['hist'], None)

    def com(**kw):
        a = dict(ok, **kw)
        return lib.tepose_session_commit(a['win'], a['S'], a['T'], a['ops'], a['theta'], None)
    assert adv(win=None) == E_ARG and adv(ops=None) == E_ARG and adv(feat=None) == E_ARG
    assert com(win=None) == E_ARG and com(ops=None) == E_ARG and com(theta=None) == E_ARG
    for f in (adv, com):
        assert f(S=0) == E_SHAPE and f(S=-3) == E_SHAPE and f(S=4097) == E_SHAPE
        assert f(T=1) == E_SHAPE and f(T=0) == E_SHAPE and f(T=-6) == E_SHAPE
        assert f(win=None, S=0) == E_ARG                           # a null pointer is reported first
    # saved and hist may be NULL: with them, a bad shape is still what comes back (nothing was launched)
    assert adv(saved=None, hist=None, S=0) == E_SHAPE and adv(saved=None, hist=None, T=1) == E_SHAPE


@pytest.mark.parametrize('T', [2, 3, 6, 32])
def test_op_1_is_the_shift_stream_session_defines(T):
    """StreamSession._tick: tmp[:T-1] = win[1:]; tmp[T-1, :2048] = feature; tmp[T-1, 2048:] = 0; win = tmp -- then theta into win[T-1, 2048:]."""
    win, _, feat, hist, theta = R.random_case(3, T, 100 + T)
    ops = np.array([1, 1, 1], dtype=np.int32)
    tmp = np.empty_like(win)
    for s in range(3):
        tmp[s, :T - 1] = win[s, 1:]
        tmp[s, T - 1, :2048] = feat[s]
        tmp[s, T - 1, 2048:] = 0
    new, saved = R.advance(win, ops, feat, hist)
    assert R.same_bits(new, tmp) and R.same_bits(saved, win)
    tmp[:, T - 1, 2048:] = theta
    assert R.same_bits(R.commit(new, ops, theta), tmp)


def test_the_other_ops_of_the_restatement():
    T = 4
    win, _, feat, hist, theta = R.random_case(6, T, 7)
    ops = np.array([0, 2, 3, 4, -1, 1], dtype=np.int32)
    new, saved = R.advance(win, ops, feat, hist)
    assert R.same_bits(saved, win)
    for s in (0, 3, 4):
        assert R.same_bits(new[s], win[s])                         # hold, and every unknown code
    assert R.same_bits(new[1, :T - 1], hist[1]) and R.same_bits(new[1, T - 1, :2048], feat[1]) and not new[1, T - 1, 2048:].any()
    assert not new[2].any() and not np.signbit(new[2]).any()      # +0 everywhere
    assert R.same_bits(R.advance(win, ops, feat, None)[0][1], win[1])      # a join without history holds
    done = R.commit(new, ops, theta)
    for s in range(6):
        if s in (1, 5):
            assert R.same_bits(done[s, T - 1, 2048:], theta[s]) and R.same_bits(done[s, :, :2048], new[s, :, :2048]) and R.same_bits(done[s, :T - 1], new[s, :T - 1])
        else:
            assert R.same_bits(done[s], new[s])
    for shift in range(8):                                         # one slot walks through every code
        assert R.random_case(1, 2, 0, shift)[1].tolist() == [[0, 1, 2, 3, 4, -1, 7, 1 << 20][shift]]
    assert sorted(set(R.random_case(64, 2, 0)[1].tolist())) == [-1, 0, 1, 2, 3, 4, 7, 1 << 20]


def test_the_session_machinery_exists_once():
    """The weight watch, the capture, the warm-up and the run-and-recover loop are the base class's alone; PixelSession writes a feed, not a tick;
    one table of output row shapes serves engine.py, stream.py and live.py."""
    import inspect
    import re
    from tepose_amd import engine, live, stream
    base = stream.StreamSession.__mro__[1]
    assert base is stream.MultiStreamSession.__mro__[1] and live.PixelSession.__mro__[1:3] == (stream.MultiStreamSession, base)
    for name in ('_refresh', '_capture', '_warm_up', '_run'):
        assert name in base.__dict__, name
        for cls in (stream.StreamSession, stream.MultiStreamSession, live.PixelSession):
            assert name not in cls.__dict__, (cls.__name__, name)
    assert '_tick' not in live.PixelSession.__dict__ and '_feed' in live.PixelSession.__dict__
    src = inspect.getsource(live.PixelSession)
    assert 'tepose_session_advance' not in src and 'tepose_session_commit' not in src
    # a mapping of row shapes names every output with a shape: count the dict entries that open with a key and a tuple
    tables = [m for mod in (engine, stream, live) for m in re.findall(r"'(theta|verts|kp_2d|kp_3d|rotmat)'\s*:\s*\(", inspect.getsource(mod))]
    assert sorted(tables) == ['kp_2d', 'kp_3d', 'rotmat', 'theta', 'verts'], tables
    assert set(engine.OUT_TAILS) == set(tables) and stream.OUT_TAILS is engine.OUT_TAILS and live.OUT_TAILS is engine.OUT_TAILS


def test_the_capacity_limits_need_no_device():
    from tepose_amd.stream import MultiStreamSession
    for slots in (0, 65, -1):
        with pytest.raises(ValueError, match='slots'):
            MultiStreamSession(None, 6, slots)
