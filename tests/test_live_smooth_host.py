"""CPU: what of one-euro smoothing inside a live session's tick (DESIGN.md sections 17 and 18) needs no device -- every argument error of
tepose_session_smooth, which returns before any device call; the symbol in the header and the loader; the launch shape of its kernel
(tests/c_client/session_smooth_shape_check.cpp on the host compiler); the `smooth=` errors of MultiStreamSession and PixelSession, which are
raised before anything touches a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE = -1, -2


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from tepose_amd import _lib
    return _lib.load()


def test_every_argument_error_of_session_smooth_without_a_device(lib):
    P = 4096                                                       # a non-null pointer value: never dereferenced, every call returns before a device call
    ok = dict(theta=P, hist=P, S=3, T=4, ops=P, state=P, saved=P, mc=0.004, beta=0.7, dc=1.0, theta_hat=P, pose_hat=P, betas_hat=P)

    def smooth(**kw):
        a = dict(ok, **kw)
        return lib.tepose_session_smooth(a['theta'], a['hist'], a['S'], a['T'], a['ops'], a['state'], a['saved'], a['mc'], a['beta'], a['dc'],
                                         a['theta_hat'], a['pose_hat'], a['betas_hat'], None)
    for k in ('theta', 'ops', 'state', 'theta_hat', 'pose_hat', 'betas_hat'):
        assert smooth(**{k: None}) == E_ARG, k
    for k in ('mc', 'beta', 'dc'):
        for v in (-1e-3, -1.0, float('nan'), float('inf'), -float('inf')):
            assert smooth(**{k: v}) == E_ARG, (k, v)
    # the shape limits come second, whatever else is wrong
    for kw in (dict(S=0), dict(S=-1), dict(S=4097), dict(T=1), dict(T=0)):
        assert smooth(**kw) == E_SHAPE, kw
        assert smooth(theta=None, **kw) == E_ARG and smooth(beta=float('nan'), **kw) == E_ARG and smooth(pose_hat=None, **kw) == E_ARG, kw
    # hist and saved_state may be NULL, and a zero cutoff or beta is a value: with them a bad shape is still what comes back (nothing was launched)
    assert smooth(hist=None, saved=None, mc=0.0, beta=0.0, dc=0.0, S=4097) == E_SHAPE
    assert smooth(hist=None, saved=None, T=1) == E_SHAPE


def test_the_symbol_is_in_the_header_and_the_loader(lib):
    from tepose_amd import _lib
    assert 'tepose_session_smooth' in _lib.SYMBOLS
    header = open(os.path.join(ROOT, 'include', 'tepose_amd.h')).read()
    m = re.search(r'int tepose_session_smooth\(([^;]*)\);', header)
    assert m, 'tepose_session_smooth is not declared in include/tepose_amd.h'
    args = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['theta', 'hist', 'S', 'T', 'ops', 'state', 'saved_state', 'min_cutoff', 'beta', 'd_cutoff',
                                                         'theta_hat', 'pose_hat', 'betas_hat', 'stream']
    assert len(lib.tepose_session_smooth.argtypes) == len(args)
    assert lib.tepose_session_smooth.argtypes[7:10] == [ctypes.c_float] * 3          # the filter's constants travel as floats, not as integers


def test_the_smooth_launch_shape_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail('no host C++ compiler (c++ / g++ / clang++) on PATH')
    exe = str(tmp_path / 'session_smooth_shape_check')
    p = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'tepose_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'c_client', 'session_smooth_shape_check.cpp'), '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'ok 12'


BAD_SMOOTH = [(0.004,), (0.004, 0.7, 1.0), 0.004, 'ab', (0.004, None), (-0.004, 0.7), (0.004, -0.7), (float('nan'), 0.7), (0.004, float('inf')),
              (-float('inf'), 0.7)]


def test_the_smooth_errors_of_the_feature_session_need_no_device():
    from tepose_amd.stream import MultiStreamSession
    for bad in BAD_SMOOTH:
        with pytest.raises(ValueError, match='smooth'):
            MultiStreamSession(None, 6, 4, smooth=bad)
    with pytest.raises(ValueError, match='J_regressor'):
        MultiStreamSession(None, 6, 4, J_regressor=object(), smooth=(0.004, 0.7))
    # the older errors still come first
    with pytest.raises(ValueError, match='slots'):
        MultiStreamSession(None, 6, 65, smooth=(0.004,))
    with pytest.raises(ValueError, match='seqlen'):
        MultiStreamSession(None, 1, 4, smooth=(0.004,))


def test_the_smooth_errors_of_the_pixel_session_need_no_device():
    from tepose_amd.live import PixelSession
    for bad in BAD_SMOOTH:
        with pytest.raises(ValueError, match='smooth'):
            PixelSession(None, None, None, 6, 4, frame_size=(96, 128), smooth=bad)
    with pytest.raises(ValueError, match='J_regressor'):
        PixelSession(None, None, None, 6, 4, frame_size=(96, 128), J_regressor=object(), smooth=(0.004, 0.7))
    with pytest.raises(ValueError, match='frame_size'):
        PixelSession(None, None, None, 6, 4, frame_size=(96,), smooth=(0.004,))
