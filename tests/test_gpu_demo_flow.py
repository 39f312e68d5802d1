"""GPU: tepose_amd.demo.run_tracklets -- uint8 frames and tracker boxes in, the reference's per-person `output_dict` (demo.py:333-344) out --
against the same flow composed here from the separately pinned public pieces: crop_frames (tests/test_gpu_crop.py) -> HMR.feature_extractor
(tests/test_gpu_hmr.py) -> VIBE (tests/test_gpu_vibe.py) -> run_clips (tests/test_gpu_driver.py, tests/test_gpu_stream.py: demo.py:209-262 executed)
-> the two conversions (tests/test_crop_host.py).  Bit for bit: the driver adds plumbing, no arithmetic.

Two persons, ragged tracklets of 11 and 8 frames over eight 97 x 131 frames (the longer one revisits frames), seqlen 6; small models: VIBE L1 H64,
TePose L1 H64, synthetic HMR weights and SMPL tables."""
import numpy as np
import pytest
import torch

from tepose_amd import synth

pytestmark = pytest.mark.gpu
T, BBOX_SCALE = 6, 1.2
KEYS = ['pred_cam', 'orig_cam', 'verts', 'pose', 'betas', 'joints3d', 'joints2d', 'joints2d_img_coord', 'bboxes', 'frame_ids']


@pytest.fixture(scope='module')
def world():
    from test_gpu_hmr import build as build_hmr
    from test_gpu_vibe import _build as build_vibe
    from tepose_amd.testing import build_model
    smpl_np = synth.synthetic_smpl(0)
    hmr, _, _ = build_hmr('split')
    vibe, _ = build_vibe(1, 64, 32, smpl_np)
    model, _, _ = build_model(1, 64, seed=31, device='cuda', smpl_np=smpl_np, seqlen=T)
    g = np.random.default_rng(8)
    frames = torch.from_numpy(g.integers(0, 256, (8, 97, 131, 3), dtype=np.uint8)).cuda()

    def boxes(n, cx, cy, w, h):                          # a box drifting through the frame, over its right edge at the end
        t = np.arange(n, dtype=np.float64)
        return np.stack([cx + 4.3 * t, cy + 1.7 * t, w + 0.9 * t, h + 0.6 * t], axis=1)
    tracks = {3: {'frames': np.array([0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4]), 'bbox': boxes(11, 70.2, 40.4, 44.0, 61.0)},
              'b': {'frames': np.arange(8), 'bbox': boxes(8, 30.6, 52.1, 38.5, 38.5)}}
    return hmr, vibe, model, frames, tracks


def _composed(world):
    """demo.py:171-331 for every person, from the public pieces.  The window loops run as ONE run_clips call over both persons, as run_tracklets runs them:
    a call with two clips takes the cached-projection kernels, a call with one does not, and those agree to rounding only (tests/test_gpu_driver.py)."""
    from tepose_amd.crop import crop_frames
    from tepose_amd.demo import convert_crop_cam_to_orig_img, convert_crop_coords_to_orig_img
    from tepose_amd.driver import run_clips
    hmr, vibe, model, frames, tracks = world
    feats, boots = [], []
    with torch.no_grad():
        for t in tracks.values():
            f = hmr.feature_extractor(crop_frames(frames, t['frames'], t['bbox'], scale=BBOX_SCALE))          # per person: 11 and 8 images
            n = f.shape[0]
            b = vibe(f[None])[-1]
            feats.append(f)
            boots.append({'theta': b['theta'].reshape(n, 85)[:T - 1], 'verts': b['verts'].reshape(n, 6890, 3)[:T - 1],
                          'kp_3d': b['kp_3d'].reshape(n, 49, 3)[:T - 1], 'kp_2d': b['kp_2d'].reshape(n, 49, 2)[:T - 1]})
        wins = run_clips(model, feats, [b['theta'] for b in boots], T, keep=('theta', 'verts', 'kp_3d', 'kp_2d'))
    out = {}
    for (p, t), b, w in zip(tracks.items(), boots, wins):
        o = {k: torch.cat([b[k], w[k]]).cpu().numpy() for k in b}
        bb = np.array(t['bbox'], copy=True)
        bb[T - 1:, 2:] = bb[T - 1:, 2:] * BBOX_SCALE                                                          # demo.py:315
        out[p] = {'pred_cam': o['theta'][:, :3], 'pose': o['theta'][:, 3:75], 'betas': o['theta'][:, 75:], 'verts': o['verts'], 'joints3d': o['kp_3d'],
                  'orig_cam': convert_crop_cam_to_orig_img(o['theta'][:, :3], bb, 131, 97),
                  'joints2d_img_coord': convert_crop_coords_to_orig_img(bb, o['kp_2d'], 224), 'bboxes': bb}
    return out


def test_run_tracklets_equals_the_flow_composed_from_its_pieces(world):
    from tepose_amd.demo import run_tracklets
    hmr, vibe, model, frames, tracks = world
    keep = {p: (t['frames'].copy(), t['bbox'].copy()) for p, t in tracks.items()}
    res = run_tracklets(frames, tracks, hmr, vibe, model, seqlen=T, bbox_scale=BBOX_SCALE)
    want = _composed(world)
    assert list(res) == list(tracks)
    for p, t in tracks.items():
        r, n = res[p], t['frames'].shape[0]
        assert list(r) == KEYS                                                                                # demo.py:333-344, in its order
        shapes = {'pred_cam': (n, 3), 'orig_cam': (n, 4), 'verts': (n, 6890, 3), 'pose': (n, 72), 'betas': (n, 10), 'joints3d': (n, 49, 3),
                  'joints2d_img_coord': (n, 49, 2), 'bboxes': (n, 4)}
        for k, shp in shapes.items():
            assert isinstance(r[k], np.ndarray) and r[k].shape == shp, (p, k, r[k].shape)
            assert r[k].dtype == (np.float64 if k in ('orig_cam', 'bboxes') else np.float32), (p, k, r[k].dtype)
            assert np.array_equal(r[k], want[p][k]), (p, k, float(np.abs(r[k] - want[p][k]).max()))
            assert np.isfinite(r[k]).all()
        assert r['joints2d'] is None
        assert r['frame_ids'] is t['frames'] and np.array_equal(t['frames'], keep[p][0])
        # bboxes as demo.py:315 leaves them: rows from seqlen - 1 scaled, the bootstrap's rows not; the caller's array untouched
        assert np.array_equal(t['bbox'], keep[p][1])
        assert np.array_equal(r['bboxes'][:T - 1], keep[p][1][:T - 1]) and np.array_equal(r['bboxes'][T - 1:, 2:], keep[p][1][T - 1:, 2:] * BBOX_SCALE)
        assert np.array_equal(r['bboxes'][:, :2], keep[p][1][:, :2])
    assert not np.array_equal(res[3]['pred_cam'][:8], res['b']['pred_cam'])                                  # two persons, two results
    # another original-image size only moves the camera
    other = run_tracklets(frames, tracks, hmr, vibe, model, seqlen=T, bbox_scale=BBOX_SCALE, img_size=(262, 194))
    assert np.array_equal(other[3]['verts'], res[3]['verts']) and not np.array_equal(other[3]['orig_cam'], res[3]['orig_cam'])


def test_smoothing_is_the_existing_filter_path(world):
    from tepose_amd.demo import run_tracklets
    from tepose_amd.filters import smooth_pose
    hmr, vibe, model, frames, tracks = world
    plain = run_tracklets(frames, tracks, hmr, vibe, model, seqlen=T, bbox_scale=BBOX_SCALE)
    res = run_tracklets(frames, tracks, hmr, vibe, model, seqlen=T, bbox_scale=BBOX_SCALE, smooth=(0.004, 1.5))
    for p in tracks:
        n = tracks[p]['frames'].shape[0]
        verts, pose, joints3d = smooth_pose(plain[p]['pose'], plain[p]['betas'], model.regressor.smpl, min_cutoff=0.004, beta=1.5)
        assert res[p]['pose'].shape == (n, 24, 3) and res[p]['verts'].shape == (n, 6890, 3) and res[p]['joints3d'].shape == (n, 49, 3)
        assert np.array_equal(res[p]['verts'], verts) and np.array_equal(res[p]['pose'], pose) and np.array_equal(res[p]['joints3d'], joints3d)
        assert not np.array_equal(res[p]['verts'], plain[p]['verts'])
        for k in ('pred_cam', 'orig_cam', 'betas', 'joints2d_img_coord', 'bboxes'):                           # smoothing touches three outputs only
            assert np.array_equal(res[p][k], plain[p][k]), k


def test_short_tracklet_is_refused(world):
    from tepose_amd.demo import run_tracklets
    hmr, vibe, model, frames, tracks = world
    short = dict(tracks, c={'frames': np.arange(5), 'bbox': tracks['b']['bbox'][:5]})
    with pytest.raises(ValueError, match='fewer than seqlen'):
        run_tracklets(frames, short, hmr, vibe, model, seqlen=T, bbox_scale=BBOX_SCALE)
    assert run_tracklets(frames, {}, hmr, vibe, model, seqlen=T, bbox_scale=BBOX_SCALE) == {}
