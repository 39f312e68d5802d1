"""GPU: the live session from pixels (tepose_amd.live.PixelSession) -- a uint8 frame and one box per person per tick.
Against the composition a caller writes without it (HMR.features_from_frames, then MultiStreamSession.push), bit for bit; graph against eager, a frame
on the host against one on the device, a second run; people who join from frames, miss a frame and leave against the offline driver
(tepose_amd.demo.run_tracklets) within the fp32 budget; the overlay against Renderer.render_frames called by hand; idle slots; a backbone weight
change followed by refresh().

Synthetic HMR backbone (tests/_hmr_synth.py through tests/test_gpu_hmr.py's builder), VIBE L1 H64, TePose L1 H64 and L2 H128, seqlen 4, frames of
96 x 128 seeded noise, boxes 40 - 70 px."""
import numpy as np
import pytest
import torch

from tepose_amd import synth

pytestmark = pytest.mark.gpu
T, SCALE, H, W, NF = 4, 1.2, 96, 128, 12
KEEP = ('theta', 'kp_3d', 'verts')
ARCH = [(1, 64), (2, 128)]


@pytest.fixture(scope='module')
def parts():
    from test_gpu_hmr import build as build_hmr
    from test_gpu_vibe import _build as build_vibe
    smpl_np = synth.synthetic_smpl(0)
    hmr, _, _ = build_hmr('split')
    vibe, _ = build_vibe(1, 64, 32, smpl_np)
    frames = torch.from_numpy(np.random.default_rng(18).integers(0, 256, (NF, H, W, 3), dtype=np.uint8))
    return smpl_np, hmr, vibe, frames


@pytest.fixture(scope='module', params=ARCH, ids=lambda a: 'L%dH%d' % a)
def world(request, parts):
    from tepose_amd.testing import build_model
    smpl_np, hmr, vibe, frames = parts
    L, Hd = request.param
    model, _, _ = build_model(L, Hd, seed=71, device='cuda', smpl_np=smpl_np, seqlen=T)
    return model, hmr, vibe, frames


def _box(person, f):
    """Person `person`'s box in frame f: 40 - 70 px, w != h, drifting; person 1 hangs over the right edge at the end."""
    cx, cy, w, h = [(38.3, 44.6, 41.0, 62.5), (96.7, 51.2, 55.4, 47.9), (64.1, 40.8, 48.6, 69.3), (70.9, 57.4, 66.2, 43.7)][person]
    return np.array([cx + 1.9 * f, cy + 0.8 * f, w + 0.7 * f, h + 0.4 * f])


def _history(seed):
    w = synth.synthetic_windows(1, T, seed)[0]
    return torch.from_numpy(w[:T - 1, :2048].copy()), torch.from_numpy(w[:T - 1, 2048:].copy())


def _session(world, S, **kw):
    from tepose_amd.live import PixelSession
    model, hmr, vibe, _ = world
    return PixelSession(model, hmr, vibe, T, S, frame_size=(H, W), bbox_scale=SCALE, keep=KEEP, **kw)


def _run_present(world, S, slots, ticks, graph=True, device_frame=False):
    """`slots` joined with seeded histories, every one given a box in each of `ticks` ticks.  -> {slot: {key: [ticks, ...]}}, the session."""
    frames = world[3]
    ses = _session(world, S, graph=graph)
    for s in slots:
        ses.join(s, *_history(300 + s))
    got = {s: {k: [] for k in KEEP + ('orig_cam', 'bbox')} for s in slots}
    for j in range(ticks):
        frame = frames[j].cuda() if device_frame else (frames[j] if j % 2 else frames[j].numpy())      # host frames as tensor and as numpy
        out = ses.push(frame, {s: _box(s, j) for s in slots})
        assert sorted(out) == sorted(slots)
        for s in slots:
            for k in got[s]:
                got[s][k].append(torch.as_tensor(out[s][k]).clone())
    return {s: {k: torch.stack(v) for k, v in d.items()} for s, d in got.items()}, ses


def _run_composed(world, S, slots, ticks):
    """What a caller writes today: the features of the tick's crops from HMR.features_from_frames, then MultiStreamSession.push."""
    from tepose_amd.stream import MultiStreamSession
    model, hmr, _, frames = world
    twin = MultiStreamSession(model, T, S, keep=KEEP)
    for s in slots:
        twin.join(s, *_history(300 + s))
    got = {s: {k: [] for k in KEEP} for s in slots}
    for j in range(ticks):
        with torch.no_grad():
            f = hmr.features_from_frames(frames[j][None].cuda(), np.zeros(len(slots), dtype=np.int64), np.stack([_box(s, j) for s in slots]), scale=SCALE)
        feats = torch.zeros(S, 2048, device='cuda')
        feats[list(slots)] = f
        out = twin.push(feats, slots=list(slots))
        for s in slots:
            for k in KEEP:
                got[s][k].append(out[s][k].clone())
    return {s: {k: torch.stack(v) for k, v in d.items()} for s, d in got.items()}


@pytest.fixture(scope='module')
def three(world):
    """S = 3, all present, 6 ticks: the pixel session's rows, shared by the tests below."""
    got, ses = _run_present(world, 3, (0, 1, 2), 6)
    assert sorted(ses.graphs) == ['host'] and ses.ticks == 6
    return got


# ------------------------------------------------------------------ 1. today's composition
def test_a_tick_equals_features_from_frames_then_the_feature_session(world, three):
    want = _run_composed(world, 3, (0, 1, 2), 6)
    for s in range(3):
        for k in KEEP:
            assert torch.isfinite(three[s][k]).all()
            assert torch.equal(three[s][k], want[s][k]), (s, k)
        assert not torch.equal(three[s]['theta'][0], three[s]['theta'][5])          # the ticks differ: the frame and the boxes are read


# ------------------------------------------------------------------ 2. variants
@pytest.mark.parametrize('variant', ['eager', 'device_frame', 'again', 'eager_device_frame'])
def test_the_variants_give_the_same_bits(variant, world, three):
    got, ses = _run_present(world, 3, (0, 1, 2), 6, graph='eager' not in variant, device_frame='device' in variant)
    # the constructor captures the host-frame tick, as the base class does; the device-frame tick is captured on first use
    assert sorted(ses.graphs) == ([] if 'eager' in variant else ['device', 'host'] if 'device' in variant else ['host'])
    for s in range(3):
        for k in three[s]:
            assert torch.equal(got[s][k], three[s][k]), (variant, s, k)


# ------------------------------------------------------------------ 3. the offline driver
def _tracks():
    """A: frames 0 .. 11 in slot 0.  B: frames 3 .. 10 in slot 1, no box in frame 8 (held), leaves after frame 10.  C: frames 8 .. 11, takes slot 1."""
    fa, fb, fc = np.arange(0, 12), np.array([3, 4, 5, 6, 7, 9, 10]), np.arange(8, 12)
    return {'A': {'frames': fa, 'bbox': np.stack([_box(0, f) for f in fa])}, 'B': {'frames': fb, 'bbox': np.stack([_box(1, f) for f in fb])},
            'C': {'frames': fc, 'bbox': np.stack([_box(2, f) for f in fc])}}


def test_joins_holds_and_leaves_against_the_offline_driver(world):
    from tepose_amd.demo import convert_crop_cam_to_orig_img, run_tracklets
    model, hmr, vibe, frames = world
    tracks = _tracks()
    ref = run_tracklets(frames.cuda(), tracks, hmr, vibe, model, T, SCALE)
    ses = _session(world, 2)
    slot = {'A': 0, 'B': 1, 'C': 1}
    rows = {p: [] for p in tracks}                                      # per person: (theta, verts, kp_3d, orig_cam, bbox) per frame of its tracklet

    def take(p, o):
        rows[p].append({k: np.array(torch.as_tensor(o[k]).numpy(), copy=True) for k in KEEP + ('orig_cam', 'bbox')})

    for f in range(NF):
        if f == 11:
            ses.leave(slot['B'])
        for p, t in tracks.items():
            if f == t['frames'][T - 1]:                                 # the person's first T - 1 frames are in (and B has left the slot C takes)
                first = t['frames'][:T - 1]
                boot = ses.join_from_frames(slot[p], frames[first] if p != 'B' else frames[first].cuda(), t['bbox'][:T - 1])
                assert sorted(boot) == sorted(KEEP + ('orig_cam', 'bbox')) and boot['verts'].shape == (T - 1, 6890, 3)
                for j in range(T - 1):
                    take(p, {k: boot[k][j] for k in boot})
        fed = {p: t['bbox'][list(t['frames']).index(f)] for p, t in tracks.items() if f in t['frames'][T - 1:]}
        if f < T - 1:
            assert not fed
            continue
        out = ses.push(frames[f], {slot[p]: b for p, b in fed.items()})
        assert sorted(out) == sorted(slot[p] for p in fed), f
        assert (f == 8) == (ses.occupied[1] and 1 not in out and f >= 6)                 # B is held in frame 8, and only there
        for p in fed:
            take(p, out[slot[p]])
    worst = 0.0
    for p, t in tracks.items():
        n = len(t['frames'])
        assert len(rows[p]) == n, p
        got = {k: np.stack([r[k] for r in rows[p]]) for k in rows[p][0]}
        mine = {'pred_cam': got['theta'][:, :3], 'pose': got['theta'][:, 3:75], 'betas': got['theta'][:, 75:], 'verts': got['verts'], 'joints3d': got['kp_3d']}
        for k, v in mine.items():
            assert v.shape == ref[p][k].shape and np.isfinite(v).all(), (p, k)
            d = float(np.abs(v - ref[p][k]).max())
            worst = max(worst, d)
            print('person %s %-8s max|session - run_tracklets| = %.3e' % (p, k, d))
            assert d < 1e-4, (p, k, d)                                   # the project's fp32 budget: other batch classes
        assert got['bbox'].dtype == np.float64 and np.array_equal(got['bbox'], ref[p]['bboxes']), p      # scale_bboxes: rows T - 1 .. scaled
        assert not np.array_equal(got['bbox'][T - 1], t['bbox'][T - 1]) and np.array_equal(got['bbox'][:T - 1], t['bbox'][:T - 1])
        want = convert_crop_cam_to_orig_img(mine['pred_cam'], got['bbox'], W, H)
        assert got['orig_cam'].dtype == want.dtype and np.array_equal(got['orig_cam'], want), p
    print('max over all = %.3e' % worst)


# ------------------------------------------------------------------ 4. the overlay
def test_the_overlay_is_render_frames_on_the_ticks_rows(world):
    from tepose_amd.demo import default_mesh_colors
    from tepose_amd.render import Renderer
    frames = world[3]
    faces = np.stack([np.arange(0, 6888), np.arange(1, 6889), np.arange(2, 6890)], axis=1)
    S = 4
    ses = _session(world, S, overlay=Renderer(faces))
    by_hand = Renderer(faces)
    cols = default_mesh_colors(range(S))
    for s in range(S):
        ses.join(s, *_history(300 + (s if s < 3 else 2)))               # slots 2 and 3: the same history ...
    person = (0, 1, 2, 2)                                               # ... and the same boxes: a tie in sy
    empty = ses.push(frames[0], {})
    assert list(empty) == ['frame'] and empty['frame'].is_cuda and torch.equal(empty['frame'].cpu(), frames[0])         # nobody present: the frame
    drawn = 0
    for j, present in enumerate([(0, 1, 2, 3), (1, 3, 2), (0, 1)], start=1):
        out = ses.push(frames[j], {s: _box(person[s], j) for s in present})
        got = out.pop('frame')
        assert sorted(out) == sorted(present) and tuple(got.shape) == (H, W, 3) and got.dtype == torch.uint8 and got.is_cuda
        act = sorted(present)
        oc = np.stack([out[s]['orig_cam'] for s in act])
        if 2 in present and 3 in present:
            assert np.array_equal(out[2]['orig_cam'], out[3]['orig_cam'])                 # the tie
        assert len(set(oc[:, 1].tolist())) >= 2
        order = np.argsort(oc[:, 1])
        want = by_hand.render_frames(frames[j][None].cuda(), np.zeros(len(act), dtype=np.int64), np.stack([out[act[i]]['verts'].numpy() for i in order]),
                                     oc[order], np.array([cols[act[i]] for i in order], dtype=np.float32))[0]
        assert torch.equal(got, want), j
        drawn += int((got.cpu() != frames[j]).any())
    assert drawn                                                         # a mesh covers pixels in at least one of the ticks
    assert torch.equal(ses.push(frames[5].cuda(), {})['frame'].cpu(), frames[5])


# ------------------------------------------------------------------ 5. idle slots
def test_idle_slots_change_no_row_and_stay_zero(world):
    got, ses = _run_present(world, 4, (2,), 5)
    want = _run_composed(world, 4, (2,), 5)
    for k in KEEP:
        assert torch.equal(got[2][k], want[2][k]), k
    for s in (0, 1, 3):
        assert not ses.win[s].any(), s
    assert ses.win[2].any()


# ------------------------------------------------------------------ staleness of the backbone
def test_a_backbone_weight_change_is_seen_after_refresh(world):
    """Backbone tensors changed in place: the push after refresh() re-packs (outside any capture) and re-captures; its rows are those of the composition
    with the new weights.  (The per-push cheap check does not watch the backbone: documented.)  The shared backbone is put back afterwards."""
    from tepose_amd.stream import MultiStreamSession
    model, hmr, _, frames = world
    ses = _session(world, 2)
    twin = MultiStreamSession(model, T, 2, keep=KEEP)
    for s in range(2):
        ses.join(s, *_history(300 + s))
        twin.join(s, *_history(300 + s))

    def both(j):
        boxes = np.stack([_box(s, j) for s in range(2)])
        out = ses.push(frames[j], {s: boxes[s] for s in range(2)})
        got = {s: {k: out[s][k].clone() for k in KEEP} for s in range(2)}
        with torch.no_grad():
            f = hmr.features_from_frames(frames[j][None].cuda(), np.zeros(2, dtype=np.int64), boxes, scale=SCALE)
        ref = twin.push(f, slots=[0, 1])
        return got, {s: {k: ref[s][k].clone() for k in KEEP} for s in range(2)}

    kept = (hmr.bn1.bias.detach().clone(), hmr.layer3[2].conv2.weight.detach().clone())
    try:
        both(0)
        gen = hmr._engine.packed_generation
        with torch.no_grad():
            hmr.bn1.bias.add_(0.05)
            hmr.layer3[2].conv2.weight.mul_(0.9)
        ses.refresh()
        got, ref = both(1)
        assert hmr._engine.packed_generation > gen and sorted(ses.graphs) == ['host']
        for s in range(2):
            for k in KEEP:
                assert torch.isfinite(got[s][k]).all() and torch.equal(got[s][k], ref[s][k]), (s, k)
        got, ref = both(2)                                               # and the tick after it, on the re-captured graph
        for s in range(2):
            assert torch.equal(got[s]['theta'], ref[s]['theta']), s
    finally:
        with torch.no_grad():
            hmr.bn1.bias.copy_(kept[0])
            hmr.layer3[2].conv2.weight.copy_(kept[1])
