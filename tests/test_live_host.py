"""CPU: what of the live session from pixels needs no device -- every argument error of tepose_crop_boxes_u8, which returns
before any device call; the symbol in the header and the loader; the launch shape the two crop kernels share (tests/c_client/crop_shape_check.cpp on
the host compiler); the constructor and push errors of tepose_amd.live.PixelSession that precede device work."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE = -1, -2


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from tepose_amd import _lib
    return _lib.load()


def test_every_argument_error_of_crop_boxes_without_a_device(lib):
    P = 4096                                                       # a non-null pointer value: never dereferenced, every call returns before a device call
    ok = dict(frames=P, F=2, H=37, W=53, idx=P, boxes=P, scale=1.2, ops=P, n=6, S=224, out=P, raw=P, minv=P)

    def crop(**kw):
        a = dict(ok, **kw)
        return lib.tepose_crop_boxes_u8(a['frames'], a['F'], a['H'], a['W'], a['idx'], a['boxes'], a['scale'], a['ops'], a['n'], a['S'], a['out'], a['raw'],
                                        a['minv'], None)
    # the conditions of tepose_crop_frames_u8 ...
    assert crop(n=-1) == E_ARG
    for k in ('S', 'H', 'W', 'F'):
        assert crop(**{k: 0}) == E_ARG and crop(**{k: -5}) == E_ARG, k
    assert crop(out=None, raw=None) == E_ARG
    assert crop(frames=None) == E_ARG and crop(idx=None) == E_ARG
    # ... with boxes in place of minv, and the scale
    assert crop(boxes=None) == E_ARG
    for s in (0.0, -1.2, float('nan'), float('inf'), -float('inf')):
        assert crop(scale=s) == E_ARG, s
    # shape limits come second
    assert crop(S=32769) == E_SHAPE and crop(n=4097) == E_SHAPE
    assert crop(S=32769, boxes=None) == E_ARG and crop(n=4097, scale=0.0) == E_ARG and crop(S=32769, out=None, raw=None) == E_ARG
    assert crop(n=4097, frames=None) == E_ARG and crop(S=40000, n=-1) == E_ARG
    # n == 0 needs no pointer but an output, and launches nothing; the limits themselves pass the checks with n == 0
    assert crop(n=0, frames=None, idx=None, boxes=None, ops=None, minv=None) == 0
    assert crop(n=0, S=32768) == 0 and crop(n=0, S=32769) == E_SHAPE
    assert crop(n=0, scale=float('nan')) == E_ARG and crop(n=0, out=None, raw=None) == E_ARG
    # one output, no ops and no minv_out are all fine: with them a bad shape is still what comes back (nothing was launched)
    assert crop(out=None, ops=None, minv=None, n=4097) == E_SHAPE and crop(raw=None, ops=None, minv=None, S=32769) == E_SHAPE


def test_the_symbol_is_in_the_header_and_the_loader(lib):
    from tepose_amd import _lib
    assert 'tepose_crop_boxes_u8' in _lib.SYMBOLS
    header = open(os.path.join(ROOT, 'include', 'tepose_amd.h')).read()
    m = re.search(r'int tepose_crop_boxes_u8\(([^;]*)\);', header)
    assert m, 'tepose_crop_boxes_u8 is not declared in include/tepose_amd.h'
    args = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['frames', 'F', 'H', 'W', 'frame_index', 'boxes', 'scale', 'ops', 'n', 'S', 'out_nchw', 'raw_nhwc',
                                                         'minv_out', 'stream']
    assert len(lib.tepose_crop_boxes_u8.argtypes) == len(args)
    assert lib.tepose_crop_boxes_u8.argtypes[6] is __import__('ctypes').c_double          # the scale travels as a double, not as an integer


def test_the_crop_launch_shape_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail('no host C++ compiler (c++ / g++ / clang++) on PATH')
    exe = str(tmp_path / 'crop_shape_check')
    p = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'tepose_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'c_client', 'crop_shape_check.cpp'), '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'ok %d' % (13 * 11)


def test_the_constructor_errors_need_no_device():
    from tepose_amd.live import PixelSession
    for slots in (0, 65, -1):
        with pytest.raises(ValueError, match='slots'):
            PixelSession(None, None, None, 6, slots, frame_size=(96, 128))
    for size in ((0, 128), (96, -1), (96,), None, (96, 128, 3), 'ab'):
        with pytest.raises(ValueError, match='frame_size'):
            PixelSession(None, None, None, 6, 4, frame_size=size)
    for scale in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='bbox_scale'):
            PixelSession(None, None, None, 6, 4, frame_size=(96, 128), bbox_scale=scale)
    with pytest.raises(ValueError, match='theta'):
        PixelSession(None, None, None, 6, 4, frame_size=(96, 128), keep=('verts',))
    with pytest.raises(ValueError, match='seqlen'):
        PixelSession(None, None, None, 1, 4, frame_size=(96, 128))


def _bare(S=3, T=4, H=96, W=128):
    """A session with the host-side state only: the checks under test run before anything touches a device, so nothing else is needed."""
    from tepose_amd.live import PixelSession
    ses = PixelSession.__new__(PixelSession)
    ses.S, ses.T, ses.H, ses.W = S, T, H, W
    ses.occupied = [False] * S
    ses.occupied[1] = True
    return ses


def test_the_push_errors_precede_device_work():
    ses = _bare()
    frame = np.zeros((96, 128, 3), dtype=np.uint8)
    for bad in (np.zeros((96, 127, 3), dtype=np.uint8), np.zeros((128, 96, 3), dtype=np.uint8), np.zeros((1, 96, 128, 3), dtype=np.uint8),
                torch.zeros(96, 128, 4, dtype=torch.uint8), np.zeros((96, 128, 3), dtype=np.float32), torch.zeros(96, 128, 3), None):
        with pytest.raises(ValueError, match='96 x 128'):
            ses.push(bad, {1: (50., 50., 40., 60.)})
    with pytest.raises(ValueError, match='dict'):
        ses.push(frame, [(50., 50., 40., 60.)])
    with pytest.raises(ValueError, match='out of range'):
        ses.push(frame, {3: (50., 50., 40., 60.)})
    with pytest.raises(ValueError, match='out of range'):
        ses.push(frame, {-1: (50., 50., 40., 60.)})
    with pytest.raises(ValueError, match=r'c_x, c_y, w, h'):
        ses.push(frame, {1: (50., 50., 40.)})
    with pytest.raises(ValueError, match=r'c_x, c_y, w, h'):
        ses.push(frame, {1: np.zeros((1, 4))})
    with pytest.raises(ValueError, match='idle slot 0'):
        ses.push(frame, {1: (50., 50., 40., 60.), 0: (50., 50., 40., 60.)})


def test_the_join_from_frames_errors_precede_device_work():
    ses = _bare()
    frames, boxes = np.zeros((3, 96, 128, 3), dtype=np.uint8), np.tile([50., 50., 40., 60.], (3, 1))
    with pytest.raises(ValueError, match='occupied'):
        ses.join_from_frames(1, frames, boxes)
    with pytest.raises(ValueError, match='out of range'):
        ses.join_from_frames(3, frames, boxes)
    for bad in (frames[:2], np.zeros((3, 96, 127, 3), dtype=np.uint8), frames[0], frames.astype(np.int32)):
        with pytest.raises(ValueError, match='96 x 128'):
            ses.join_from_frames(0, bad, boxes)
    for bad in (boxes[:2], boxes[:, :3], boxes.reshape(-1)):
        with pytest.raises(ValueError, match='boxes'):
            ses.join_from_frames(0, frames, bad)
