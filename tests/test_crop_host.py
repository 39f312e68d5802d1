"""CPU: the host side of the pixels-to-mesh path -- the box -> affine rule (tepose_amd.crop.crop_transform), trans_point2d and the two
crop -> image conversions (tepose_amd.demo) against what the reference's own functions returned (tests/golden/crop_transform.npz, written by
tests/golden/make_golden_crop.py from AST slices of lib/data_utils/_img_utils.py and lib/utils/demo_utils.py); the argument checks of
tepose_crop_frames_u8 and crop_frames, which need no device; and the pixel oracle of the GPU test against its second formulation."""
import os

import numpy as np
import pytest
import torch

import _crop_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'crop_transform.npz'))
E_ARG = -1


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from tepose_amd import _lib
    return _lib.load()


def test_crop_transform_reproduces_the_reference_including_its_float32_roundings():
    from tepose_amd.crop import crop_transform
    W, H, crop, _ = (int(v) for v in G['meta'])
    bb, scale = G['bboxes'], float(G['scale'])
    M, Minv = crop_transform(bb, scale, crop)
    assert M.dtype == np.float64 and M.shape == G['M'].shape == (bb.shape[0], 2, 3) and Minv.shape == M.shape
    err = np.abs(M - G['M']).max()
    # the un-rounded rule crop / (w scale), centre unrounded: what the fixture is there to tell apart
    a, d = crop / (bb[:, 2] * scale), crop / (bb[:, 3] * scale)
    plain = np.zeros_like(M)
    plain[:, 0, 0], plain[:, 0, 2], plain[:, 1, 1], plain[:, 1, 2] = a, crop / 2 - a * bb[:, 0], d, crop / 2 - d * bb[:, 1]
    miss = np.abs(plain - G['M']).max()
    print('max |M - reference| = %.3g; the un-rounded formula misses by %.3g' % (err, miss))
    assert miss > 1e-3                                             # the fixture's boxes see the roundings
    assert err <= 1e-8, err
    eye = np.broadcast_to(np.eye(3), (bb.shape[0], 3, 3))
    full = lambda A: np.concatenate([A, np.broadcast_to(np.array([[[0., 0., 1.]]]), (A.shape[0], 1, 3))], axis=1)
    assert np.abs(full(Minv) @ full(M) - eye).max() <= 1e-9


def _rel(a, b):
    return float((np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny)).max())


def test_transform_keypoints_is_trans_point2d():
    from tepose_amd.crop import transform_keypoints
    got = transform_keypoints(G['kp'], G['M'])
    assert got.dtype == np.float64 and got.shape == G['kp_t'].shape
    assert _rel(got, G['kp_t']) <= 1e-12
    one = transform_keypoints(G['kp'][3], G['M'][3])               # one map for an array of points
    assert _rel(one, G['kp_t'][3]) <= 1e-12
    with_conf = np.concatenate([G['kp'], np.ones(G['kp'].shape[:2] + (1,))], axis=-1)      # [n,21,3]: the confidence column is not read
    assert np.array_equal(transform_keypoints(with_conf, G['M']), got)


def test_crop_to_image_conversions_match_the_reference():
    from tepose_amd.demo import convert_crop_cam_to_orig_img, convert_crop_coords_to_orig_img
    W, H, crop, _ = (int(v) for v in G['meta'])
    cam, j2d, box = G['cam'], G['j2d'], G['bboxes_scaled']
    assert cam.dtype == np.float32 and j2d.dtype == np.float32 and box.dtype == np.float64
    oc = convert_crop_cam_to_orig_img(cam, box, W, H)
    assert oc.dtype == G['orig_cam'].dtype == np.float64 and oc.shape == G['orig_cam'].shape == (box.shape[0], 4)
    assert _rel(oc, G['orig_cam']) <= 1e-12
    j2d_in = j2d.copy()
    ji = convert_crop_coords_to_orig_img(box, j2d_in, crop)
    assert np.array_equal(j2d_in, j2d)                             # the input is left alone
    assert ji.dtype == G['joints2d_img_coord'].dtype == np.float32
    assert np.array_equal(ji, G['joints2d_img_coord'])             # float32: bit for bit
    # float32 boxes: both results float32, bit for bit
    oc32 = convert_crop_cam_to_orig_img(cam, box.astype(np.float32), W, H)
    assert oc32.dtype == G['orig_cam_box32'].dtype == np.float32 and np.array_equal(oc32, G['orig_cam_box32'])
    ji32 = convert_crop_coords_to_orig_img(box.astype(np.float32), j2d, crop)
    assert ji32.dtype == np.float32 and np.array_equal(ji32, G['joints2d_img_coord_box32'])


def test_bbox_scaling_starts_at_row_seqlen_minus_1():
    """demo.py:315 scales width and height from row seq_len - 1 on only; the rows of the VIBE bootstrap keep the tracker's size."""
    from tepose_amd.demo import scale_bboxes
    b = np.arange(36, dtype=np.float64).reshape(9, 4) + 1
    keep = b.copy()
    out = scale_bboxes(b, 6, 1.2)
    assert np.array_equal(b, keep) and out is not b               # a copy
    assert np.array_equal(out[:5], keep[:5])
    assert np.array_equal(out[5:, :2], keep[5:, :2]) and np.array_equal(out[5:, 2:], keep[5:, 2:] * 1.2)
    assert scale_bboxes(b.astype(np.float32), 6, 1.2).dtype == np.float32 and scale_bboxes(b.astype(np.int64), 6, 1.2).dtype == np.float64


def test_every_argument_error_of_the_entry_point_without_a_device(lib):
    P = 4096                                                       # a non-null pointer value: never dereferenced, every call returns before a device call
    f = lib.tepose_crop_frames_u8
    ok = dict(frames=P, F=2, H=8, W=8, idx=P, minv=P, n=3, S=224, out=P, raw=P)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['frames'], a['F'], a['H'], a['W'], a['idx'], a['minv'], a['n'], a['S'], a['out'], a['raw'], None)
    assert call(n=-1) == E_ARG
    assert call(S=0) == E_ARG and call(S=-224) == E_ARG
    assert call(H=0) == E_ARG and call(W=0) == E_ARG and call(F=0) == E_ARG
    assert call(frames=None) == E_ARG and call(idx=None) == E_ARG and call(minv=None) == E_ARG
    assert call(out=None, raw=None) == E_ARG
    assert call(n=0, out=None, raw=None) == E_ARG                  # also for an empty call
    # the empty call: 0, nothing launched (there is no device here to launch on), null inputs allowed
    assert call(n=0) == 0 and call(n=0, frames=None, idx=None, minv=None, raw=None) == 0


def test_crop_frames_argument_errors():
    from tepose_amd.crop import crop_frames
    box = np.array([[4., 4., 6., 6.]])
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='MI355X only'):
        crop_frames(frames, [0], box)
    with pytest.raises(ValueError):
        crop_frames(frames.float(), [0], box)
    with pytest.raises(ValueError):
        crop_frames(frames[0], [0], box)
    with pytest.raises(IndexError):
        crop_frames(frames, [2], box)
    with pytest.raises(IndexError):
        crop_frames(frames, np.array([0, -1]), np.repeat(box, 2, axis=0))
    with pytest.raises(ValueError):
        crop_frames(frames, [0, 1], box)                           # one box per index
    with pytest.raises(ValueError):
        crop_frames(frames, [0], box, crop_size=0)


def test_run_tracklets_rejects_a_tracklet_shorter_than_the_window():
    from tepose_amd.demo import run_tracklets
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    tracks = {7: {'frames': np.arange(5) % 2, 'bbox': np.tile([4., 4., 6., 6.], (5, 1))}}
    with pytest.raises(ValueError, match='fewer than seqlen'):
        run_tracklets(frames, tracks, None, None, None, seqlen=6, bbox_scale=1.2)


def test_the_pixel_oracle_agrees_with_its_second_formulation():
    """Nested lerps over masked gathers against a weighted sum over a zero-padded frame, before rounding: boxes inside, over every edge and corner,
    outside, minifying and magnifying."""
    from tepose_amd.crop import crop_transform
    g = np.random.default_rng(5)
    frames = g.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    bb = np.array([[26.3, 18.2, 20.1, 14.7], [1.5, 18.0, 16.0, 16.0], [51.2, 20.0, 18.0, 22.0], [25.0, 0.7, 14.0, 14.0], [25.0, 36.1, 12.0, 17.0],
                   [-2.0, -3.0, 15.0, 15.0], [200.0, 100.0, 10.0, 10.0], [26.0, 18.0, 90.0, 70.0], [30.3, 20.6, 3.0, 3.0]])
    idx = np.arange(bb.shape[0]) % 2
    _, minv = crop_transform(bb, 1.2, 24)
    a, b = R.bilinear(frames, idx, minv, 24), R.bilinear_weights(frames, idx, minv, 24)
    assert a.shape == b.shape == (bb.shape[0], 24, 24, 3)
    assert np.abs(a - b).max() <= 1e-9
    assert a.min() >= 0 and a.max() <= 255  and not a[6].any() and a[0].max() > 0      # outside: all zero; inside: noise
    assert R.quantise(np.array([0.49999, 0.5, 1.5, 254.5])).tolist() == [0, 1, 2, 255]
    n = R.normalise(np.zeros((1, 2, 2, 3), dtype=np.uint8))
    assert n.shape == (1, 3, 2, 2) and np.allclose(n[0, :, 0, 0], -R.MEAN / R.STD)


REF = '/root/reference'
GEN = os.path.join(ROOT, 'tests', 'golden', 'make_golden_crop.py')
needs_reference = pytest.mark.skipif(not (os.path.isfile(os.path.join(REF, 'lib', 'data_utils', '_img_utils.py')) and os.path.isfile(GEN)),
                                     reason='reference checkout or generator absent')


@needs_reference
def test_fixture_regenerates_bit_identically_and_the_generator_holds_no_reference_text(tmp_path):
    """As tests/test_golden_generator.py does for make_golden.py: the generator executes the reference's functions, it does not retype them,
    and running it again gives the committed arrays."""
    import re
    import subprocess
    import sys

    def code_lines(path):
        return [l for l in (re.sub(r'\s+', '', l.split('#')[0]) for l in open(path)) if l]
    g = code_lines(GEN)
    for ref in ('lib/data_utils/_img_utils.py', 'lib/utils/demo_utils.py'):
        r = code_lines(os.path.join(REF, ref))
        runs = {tuple(r[i:i + 3]) for i in range(len(r) - 2)}
        assert not [g[i] for i in range(len(g) - 2) if tuple(g[i:i + 3]) in runs], ref
    p = subprocess.run([sys.executable, GEN, '--out', str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    a = np.load(os.path.join(str(tmp_path), 'crop_transform.npz'))
    assert sorted(a.files) == sorted(G.files)
    for k in a.files:
        assert a[k].dtype == G[k].dtype and np.array_equal(a[k], G[k]), k
