"""GPU: one-euro smoothing inside the tick of the live sessions (MultiStreamSession / PixelSession with smooth=...; DESIGN.md sections 17, 18).
The feed is tests/_live_smooth_cases.py: S = 3, seqlen 4, 6 ticks with a held tick, a leave and a third person joining the freed slot.  A twin
session without `smooth` runs the same feed: what is not filtered (kp_2d, cam, betas) equals the twin's in every bit; the pose equals
tepose_amd.filters.one_euro over each person's (history + twin theta) rows in every bit; vertices and joints are within the fp32 budget of
filters.smooth_pose on that sequence; graph equals eager; from pixels, every key against run_tracklets(smooth=...) per person; the overlay draws
the smoothed vertices; and a session without `smooth` still gives the bits the parent commit gave (digests in profiles/live_smoothing.txt).

Measured on an MI355X, max over persons: against smooth_pose verts 1.55e-06, kp_3d 2.98e-07 at L1 H64 and 9.54e-07, 2.38e-07 at L2 H128; from pixels
against run_tracklets(smooth=...) verts 9.54e-07, joints3d 2.38e-07, pose 5.96e-08 at L1 H64 and verts 1.07e-06, joints3d 2.98e-07, pose 0 at L2 H128
(there the unsmoothed theta are bit-equal to run_tracklets', and so is the smoothed pose)."""
import numpy as np
import pytest
import torch

import _live_smooth_cases as C
from tepose_amd import synth

pytestmark = pytest.mark.gpu
SMOOTH = (0.004, 0.7)                              # demo.py's --smooth defaults
ARCH = [(1, 64), (2, 128)]
# sha256 of the unsmoothed sessions' rows (C.digest), made once with the parent commit's library and package on the same feeds
PARENT_DIGESTS = {
    ('feature', 1, 64): 'd2082ee22d94587e25f8543be0e97b5df8cef039d7b74fade5482650600b5312',
    ('feature', 2, 128): 'fc80877b6a94c2422975ec179d4189501afccd3c8d9ce927c1925d3f2dd3c2be',
    ('pixel', 1, 64): '710338715fcaa6328cb48bae852b53c09ebe6369d12696a03ae1bf248f417ee1',
    ('pixel', 2, 128): '0ab0fcbe62adf257273ac8747f691cb3d8bd1e555f90529947a6b9f610a5459e',
}


@pytest.fixture(scope='module')
def parts():
    from test_gpu_hmr import build as build_hmr
    from test_gpu_vibe import _build as build_vibe
    smpl_np = synth.synthetic_smpl(0)
    hmr, _, _ = build_hmr('split')
    vibe, _ = build_vibe(1, 64, 32, smpl_np)
    return smpl_np, hmr, vibe, C.frames()


@pytest.fixture(scope='module', params=ARCH, ids=lambda a: 'L%dH%d' % a)
def world(request, parts):
    from tepose_amd.testing import build_model
    smpl_np, hmr, vibe, frames = parts
    L, Hd = request.param
    model, _, _ = build_model(L, Hd, seed=71, device='cuda', smpl_np=smpl_np, seqlen=C.T)
    return model, hmr, vibe, frames, (L, Hd)


@pytest.fixture(scope='module')
def runs(world):
    """The smoothed session and its twin on the feature feed, once per model."""
    got, ses = C.feature_run(world[0], smooth=SMOOTH)
    twin, tses = C.feature_run(world[0])
    assert sorted(ses.graphs) == ['host'] and ses.ticks == C.TICKS and not hasattr(tses, 'fstate')
    return got, twin


def _sequence(person, twin):
    """The person's rows as the offline filter sees them: the theta history, then the twin's (unsmoothed) theta per tick."""
    return torch.cat([C.clip(person)[1][1], twin[person]['theta']])


def test_what_is_not_filtered_equals_the_twin_bit_for_bit(runs):
    got, twin = runs
    for p in C.SLOT:
        assert got[p]['theta'].shape == (len(C.PRESENT[p]), 85)
        assert torch.equal(got[p]['kp_2d'], twin[p]['kp_2d']), p
        assert torch.equal(got[p]['theta'][:, :3], twin[p]['theta'][:, :3]) and torch.equal(got[p]['theta'][:, 75:], twin[p]['theta'][:, 75:]), p
        assert not torch.equal(got[p]['theta'][:, 3:75], twin[p]['theta'][:, 3:75]) and not torch.equal(got[p]['verts'], twin[p]['verts']), p


def test_the_pose_is_the_offline_filter_bit_for_bit(runs):
    from tepose_amd import filters
    got, twin = runs
    for p in C.SLOT:
        seq = _sequence(p, twin)
        want = filters.one_euro(seq[:, 3:75], min_cutoff=SMOOTH[0], beta=SMOOTH[1]).cpu()
        assert torch.equal(got[p]['theta'][:, 3:75], want[C.T - 1:]), p        # B was held at tick 1: the held tick is no row of its sequence


def test_vertices_and_joints_are_smooth_pose_within_the_fp32_budget(world, runs):
    from tepose_amd import filters
    got, twin = runs
    worst = {}
    for p in C.SLOT:
        seq = _sequence(p, twin).cuda()
        verts, pose_hat, joints = filters.smooth_pose(seq[:, 3:75].contiguous(), seq[:, 75:].contiguous(), world[0].regressor.smpl, min_cutoff=SMOOTH[0],
                                                      beta=SMOOTH[1])
        for k, ref in (('verts', verts), ('kp_3d', joints)):
            assert torch.isfinite(got[p][k]).all()
            d = float((got[p][k] - ref[C.T - 1:].cpu()).abs().max())
            worst[k] = max(worst.get(k, 0.0), d)
            print('person %s %-6s max|session - smooth_pose| = %.3e' % (p, k, d))
            assert d < 1e-4, (p, k, d)                                         # the project's fp32 budget: another row count, maybe another SMPL kernel
    print('max over persons: %s' % worst)


def test_graph_equals_eager_bit_for_bit(world, runs):
    eager, ses = C.feature_run(world[0], graph=False, smooth=SMOOTH)
    assert not ses.graphs
    for p in C.SLOT:
        for k in C.KEYS:
            assert torch.equal(eager[p][k], runs[0][p][k]), (p, k)


def test_without_smooth_the_feature_session_gives_the_parents_bits(world, runs):
    assert C.digest(runs[1]) == PARENT_DIGESTS[('feature',) + world[4]]


# ------------------------------------------------------------------ from pixels
@pytest.fixture(scope='module')
def pixel(world):
    model, hmr, vibe, frames, _ = world
    return C.pixel_run(model, hmr, vibe, frames, smooth=SMOOTH), C.pixel_run(model, hmr, vibe, frames)


def test_from_pixels_every_key_against_the_offline_driver(world, pixel):
    from tepose_amd.demo import convert_crop_cam_to_orig_img, run_tracklets
    model, hmr, vibe, frames, _ = world
    got, raw = pixel
    ref = run_tracklets(frames.cuda(), C.tracks(), hmr, vibe, model, C.T, C.SCALE, smooth=SMOOTH)
    ref_raw = run_tracklets(frames.cuda(), C.tracks(), hmr, vibe, model, C.T, C.SCALE)
    worst = 0.0
    for p, t in C.tracks().items():
        th = got[p]['theta'].numpy()
        mine = {'pred_cam': th[:, :3], 'pose': th[:, 3:75], 'betas': th[:, 75:], 'verts': got[p]['verts'].numpy(), 'joints3d': got[p]['kp_3d'].numpy(),
                'orig_cam': got[p]['orig_cam'].numpy()}
        for k, v in mine.items():
            want = ref[p][k].reshape(v.shape)
            assert np.isfinite(v).all(), (p, k)
            d = float(np.abs(v - want).max())
            worst = max(worst, d)
            print('person %s %-8s max|session - run_tracklets(smooth)| = %.3e' % (p, k, d))
            assert d < 1e-4, (p, k, d)
        assert np.array_equal(got[p]['bbox'].numpy(), ref[p]['bboxes']), p
        assert np.array_equal(mine['orig_cam'], convert_crop_cam_to_orig_img(mine['pred_cam'], got[p]['bbox'].numpy(), C.W, C.H)), p
        assert np.array_equal(mine['orig_cam'], raw[p]['orig_cam'].numpy()), p            # the camera is not filtered
        rth = raw[p]['theta'].numpy()
        if np.array_equal(rth[:, 3:75], ref_raw[p]['pose'].reshape(-1, 72)):             # the same unsmoothed rows in: the same filtered bits out
            assert np.array_equal(mine['pose'], ref[p]['pose'].reshape(-1, 72)), p
            print('person %s: unsmoothed theta bit-equal to run_tracklets, and so is the smoothed pose' % p)
        # bootstrap rows and tick rows are one filtered sequence over the unsmoothed rows of the twin session
        from tepose_amd import filters
        one = filters.one_euro(torch.from_numpy(rth[:, 3:75].copy()), min_cutoff=SMOOTH[0], beta=SMOOTH[1]).cpu().numpy()
        assert np.array_equal(mine['pose'], one), p
    print('max over all = %.3e' % worst)


def test_without_smooth_the_pixel_session_gives_the_parents_bits(world, pixel):
    assert C.digest(pixel[1]) == PARENT_DIGESTS[('pixel',) + world[4]]


def test_the_overlay_draws_the_smoothed_vertices(world):
    from tepose_amd.demo import default_mesh_colors
    from tepose_amd.live import PixelSession
    from tepose_amd.render import Renderer
    model, hmr, vibe, frames, _ = world
    faces = np.stack([np.arange(0, 6888), np.arange(1, 6889), np.arange(2, 6890)], axis=1)
    ses = PixelSession(model, hmr, vibe, C.T, 2, frame_size=(C.H, C.W), bbox_scale=C.SCALE, keep=C.PIXEL_KEYS, overlay=Renderer(faces), smooth=SMOOTH)
    twin = PixelSession(model, hmr, vibe, C.T, 2, frame_size=(C.H, C.W), bbox_scale=C.SCALE, keep=C.PIXEL_KEYS, overlay=Renderer(faces))
    by_hand, cols = Renderer(faces), default_mesh_colors(range(2))
    for s in range(2):
        for one in (ses, twin):
            one.join(s, *C.clip('AB'[s])[1])
    differs = 0
    for j in (1, 2, 3):
        boxes = {s: C.box(s, j) for s in range(2)}
        out, ref = ses.push(frames[j], boxes), twin.push(frames[j], boxes)
        got = out.pop('frame')
        oc = np.stack([out[s]['orig_cam'] for s in range(2)])
        order = np.argsort(oc[:, 1])
        assert not torch.equal(out[0]['verts'], ref[0]['verts'])
        want = by_hand.render_frames(frames[j][None].cuda(), np.zeros(2, dtype=np.int64), np.stack([out[i]['verts'].numpy() for i in order]), oc[order],
                                     np.array([cols[i] for i in order], dtype=np.float32))[0]
        assert torch.equal(got, want), j
        differs += int(not torch.equal(got, ref['frame']))
    assert differs                                 # and that is not the picture of the unsmoothed meshes
