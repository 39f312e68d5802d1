"""The reference's demo.py:161-346 between the tracker and the renderer: tracklets of boxes over decoded frames -> the per-person
result dict, on this stack alone.  `run_tracklets` crops on the device (tepose_amd.crop), extracts HMR features, bootstraps the theta
history with VIBE, runs the sliding window with theta feedback for all persons in lock-step (tepose_amd.driver.run_clips), optionally
smooths (tepose_amd.filters.smooth_pose), and maps camera and 2-D joints back into the frame with the two functions of
lib/utils/demo_utils.py:241-274 below.  `render_tracklets` is demo.py:361-420 after it: the meshes of every frame's persons drawn over the
frames on the device (tepose_amd.render).  Decoding, tracking, Temporal SMPLify, `.obj` export, wireframe, image and
video encoding and `--display` are not here."""
import colorsys
from collections import OrderedDict

import numpy as np
import torch

from .crop import CROP_SIZE, check_frames, on_gpu
from .driver import run_clips
from .filters import smooth_pose
from .render import Renderer


def convert_crop_cam_to_orig_img(cam, bbox, img_width, img_height):
    """lib/utils/demo_utils.py:241-258: weak-perspective cameras [n,3] (s, tx, ty) of the crops -> [n,4] (sx, sy, tx, ty) in the
    original image; bbox [n,>=3] (c_x, c_y, h, ...).  numpy; float64 out for float64 boxes, float32 for float32 boxes and cameras."""
    cam, bbox = np.asarray(cam), np.asarray(bbox)
    cx, cy, h = bbox[:, 0], bbox[:, 1], bbox[:, 2]
    half_w, half_h = img_width / 2., img_height / 2.
    s = cam[:, 0]
    sx = s * (1. / (img_width / h))                 # the operations in the reference's order: the float32 form is compared bit for bit
    sy = s * (1. / (img_height / h))
    tx = (cx - half_w) / half_w / sx + cam[:, 1]
    ty = (cy - half_h) / half_h / sy + cam[:, 2]
    return np.stack([sx, sy, tx, ty]).T


def convert_crop_coords_to_orig_img(bbox, keypoints, crop_size):
    """lib/utils/demo_utils.py:261-274: keypoints [n,J,2] in the crop's normalised [-1, 1] coordinates -> pixels of the original image.
    The result has the keypoints' dtype (float32 predictions stay float32: the box terms are fp64 and each step rounds into it, as the
    reference's in-place statements do); the input is not modified."""
    bbox = np.asarray(bbox)
    cx, cy, h = bbox[:, 0], bbox[:, 1], bbox[:, 2]
    kp = 0.5 * crop_size * (np.asarray(keypoints) + 1.0)      # crop pixels; a new array
    kp *= h[:, None, None] / crop_size                         # box pixels
    kp[:, :, 0] = (cx - h / 2)[:, None] + kp[:, :, 0]
    kp[:, :, 1] = (cy - h / 2)[:, None] + kp[:, :, 1]
    return kp


def scale_bboxes(bboxes, seqlen, bbox_scale):
    """demo.py:315, kept as it stands: width and height are scaled from row seqlen - 1 on ONLY -- the rows of the VIBE bootstrap keep the
    tracker's size -- and `orig_cam` / `joints2d_img_coord` / the returned `bboxes` are computed from that array.  Returns a copy."""
    b = np.array(bboxes, copy=True)
    if b.dtype.kind != 'f':
        b = b.astype(np.float64)
    b[seqlen - 1:, 2:] = b[seqlen - 1:, 2:] * bbox_scale
    return b


@torch.no_grad()
def run_tracklets(frames_u8, tracks, hmr, vibe, model, seqlen, bbox_scale, img_size=None, smooth=None):
    """frames_u8 [F,H,W,3] torch.uint8 cuda (RGB); tracks {person_id: {'frames': int[n], 'bbox': float[n,4] (c_x, c_y, w, h)}} -- the
    tracker's output as demo.py:95-100,167-168 holds it; hmr / vibe / model: tepose_amd HMR, VIBE and TePose(seqlen) on that device.
    img_size (width, height) of the original video, default the frames' own; smooth (min_cutoff, beta) or None (demo.py:308-313).
    -> {person_id: output_dict} with the keys of demo.py:333-344, numpy.

    Per person this is demo.py:171-331: crops at `bbox_scale` -> features; VIBE over the whole tracklet, whose first seqlen - 1 predictions
    are the outputs of those frames and the theta history; one window per further frame with theta feedback; optional one-euro smoothing;
    `scale_bboxes`; the two conversions.  Two things run differently with the same results: every person's crops go through
    `HMR.features_from_frames` as one stream of 64-crop passes, and all persons' window loops advance in lock-step."""
    T = int(seqlen)
    ids = list(tracks.keys())
    frames = {p: np.asarray(tracks[p]['frames']) for p in ids}
    for p in ids:
        if frames[p].shape[0] < T:
            raise ValueError('tracklet %r has %d frames, fewer than seqlen = %d (the reference drops short tracklets before this point, demo.py:97-100)'
                             % (p, frames[p].shape[0], T))
        if np.asarray(tracks[p]['bbox']).shape != (frames[p].shape[0], 4):
            raise ValueError('tracklet %r: bbox must be [%d, 4], got %s' % (p, frames[p].shape[0], np.asarray(tracks[p]['bbox']).shape))
    if not ids:
        return {}
    width, height = img_size if img_size is not None else (int(frames_u8.shape[2]), int(frames_u8.shape[1]))
    feats = hmr.features_from_frames(frames_u8, np.concatenate([frames[p] for p in ids]),
                                     np.concatenate([np.asarray(tracks[p]['bbox'], dtype=np.float64) for p in ids]), scale=bbox_scale)
    feats = list(torch.split(feats, [frames[p].shape[0] for p in ids]))
    boots = []
    for f in feats:
        boot = vibe(f[None])[-1]                                                       # demo.py:229, no J_regressor: 49 joints
        n = f.shape[0]
        boots.append({'theta': boot['theta'].reshape(n, 85)[:T - 1], 'verts': boot['verts'].reshape(n, -1, 3)[:T - 1],
                      'kp_3d': boot['kp_3d'].reshape(n, -1, 3)[:T - 1], 'kp_2d': boot['kp_2d'].reshape(n, -1, 2)[:T - 1]})
    wins = run_clips(model, feats, [b['theta'] for b in boots], T, keep=('theta', 'verts', 'kp_3d', 'kp_2d'))
    results = {}
    for p, boot, win in zip(ids, boots, wins):
        o = {k: torch.cat([boot[k], win[k]]).cpu().numpy() for k in boot}
        pred_cam, pred_pose, pred_betas = (np.ascontiguousarray(o['theta'][:, a:b]) for a, b in ((0, 3), (3, 75), (75, 85)))
        pred_verts, pred_joints3d = o['verts'], o['kp_3d']
        if smooth is not None:
            pred_verts, pred_pose, pred_joints3d = smooth_pose(pred_pose, pred_betas, model.regressor.smpl, min_cutoff=smooth[0], beta=smooth[1])
        bboxes = scale_bboxes(tracks[p]['bbox'], T, bbox_scale)
        results[p] = {
            'pred_cam': pred_cam,
            'orig_cam': convert_crop_cam_to_orig_img(pred_cam, bboxes, width, height),
            'verts': pred_verts,
            'pose': pred_pose,
            'betas': pred_betas,
            'joints3d': pred_joints3d,
            'joints2d': None,
            'joints2d_img_coord': convert_crop_coords_to_orig_img(bboxes, o['kp_2d'], CROP_SIZE),
            'bboxes': bboxes,
            'frame_ids': tracks[p]['frames'],
        }
    return results


def prepare_rendering_results(results, nframes):
    """lib/utils/demo_utils.py:277-295: {person_id: output_dict} -> one OrderedDict per frame, person_id -> {'verts', 'cam', 'bbox'} of that frame,
    ordered by ascending `orig_cam[:, 1]` (np.argsort as the reference calls it): the person with the largest camera scale is drawn last."""
    frames = [{} for _ in range(nframes)]
    for pid, data in results.items():
        for k, f in enumerate(data['frame_ids']):
            frames[f][pid] = {'verts': data['verts'][k], 'cam': data['orig_cam'][k], 'bbox': data['bboxes'][k]}
    for f, persons in enumerate(frames):
        ids = list(persons.keys())
        frames[f] = OrderedDict((ids[i], persons[ids[i]]) for i in np.argsort([persons[p]['cam'][1] for p in ids]))
    return frames


def default_mesh_colors(person_ids):
    """One hue per person at saturation 0.5, value 1 (demo.py:372 draws the hue at random; here it is the golden-ratio sequence over the persons'
    position in `results`, so a run repeats)."""
    return {p: colorsys.hsv_to_rgb((k * 0.6180339887498949) % 1.0, 0.5, 1.0) for k, p in enumerate(person_ids)}


RENDER_CHUNK_INSTANCES = 256      # instances whose vertices are stacked for one render_frames call (21 MB of fp32 SMPL vertices)


@torch.no_grad()
def render_tracklets(frames_u8, results, faces, colors=None, sideview=False, plain=False):
    """frames_u8 [F,H,W,3] torch.uint8 cuda; results: what `run_tracklets` returned (the keys 'verts', 'orig_cam', 'bboxes', 'frame_ids' are read);
    faces [Fc,3]: the SMPL topology, or a `tepose_amd.render.Renderer`.  -> [F,H,W,3] uint8 cuda, a new tensor: demo.py:371-420 without the files --
    per frame, every person's mesh over the frame in the order of `prepare_rendering_results`.  A frame without a person is returned unchanged.
    plain: the frames are zeroed first (demo.py:384-385; the camera override of :316-317 stays the caller's).  sideview: a second render of the
    same persons on zeros with angle = 270 about (0, 1, 0), concatenated on the right: [F,H,2W,3].  colors {person_id: (r, g, b)}, default
    `default_mesh_colors`."""
    renderer = faces if isinstance(faces, Renderer) else Renderer(faces)
    check_frames(frames_u8)
    frames_u8 = on_gpu(frames_u8)
    F = int(frames_u8.shape[0])
    per_frame = prepare_rendering_results(results, F)
    if colors is None:
        colors = default_mesh_colors(results.keys())
    img = torch.zeros_like(frames_u8) if plain else frames_u8.clone()
    side = torch.zeros_like(frames_u8) if sideview else None
    side_rot = None
    batch = []                                                                   # (frame, verts, cam, colour) in draw order

    def flush():
        if not batch:
            return
        idx = np.array([b[0] for b in batch])
        verts = [b[1] for b in batch]
        verts = torch.stack([v.to(img.device) for v in verts]) if torch.is_tensor(verts[0]) else np.stack([np.asarray(v, dtype=np.float32) for v in verts])
        cams = np.stack([np.asarray(b[2], dtype=np.float64) for b in batch])
        cols = np.stack([np.asarray(b[3], dtype=np.float32) for b in batch])
        f0, f1 = int(idx.min()), int(idx.max()) + 1
        renderer.render_frames(img[f0:f1], idx - f0, verts, cams, cols, out=img[f0:f1])
        if sideview:
            renderer.render_frames(side[f0:f1], idx - f0, verts, cams, cols, rot=np.broadcast_to(side_rot, (len(batch), 3, 3)), out=side[f0:f1])
        del batch[:]

    if sideview:
        from .render import rotation_matrix
        side_rot = rotation_matrix(270, [0, 1, 0])
    for f, persons in enumerate(per_frame):
        if len(batch) + len(persons) > RENDER_CHUNK_INSTANCES:
            flush()
        for pid, data in persons.items():
            batch.append((f, data['verts'], data['cam'], colors[pid]))
    flush()
    return torch.cat([img, side], dim=2) if sideview else img
