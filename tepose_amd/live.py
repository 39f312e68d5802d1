"""Live session from pixels: a decoded uint8 frame and one box per person in, meshes out, one graph replay per tick.

`tepose_amd.stream.MultiStreamSession` takes a 2048-float HMR feature per person and tick.  `PixelSession` is that session with the two steps in
front of it inside the tick: the person crops (csrc/crop.hip, `tepose_crop_boxes_u8`: the box -> affine rule of `tepose_amd.crop.crop_transform`
runs on the device, bit-equal to the host's) and the HMR backbone (`tepose_hmr_features`).  A tick is one chain on the session's stream --

    H2D copy of one pinned block (S boxes in fp64, S op codes) [and of the frame, when it arrives on the host]
    -> crops of the slots whose op is 1 or 2 into a fixed [S,3,224,224] buffer -> backbone at N = S into `feat`
    -> the rest of the base class's tick, from tepose_session_advance on

-- and with graph=True one captured graph per variant (frame on the host / on the device) that never changes.  The first three steps are this
class's FEED (`_alloc_feed`, `_feed`), which replaces the base class's upload of op codes and features; `push` stages the frame and the boxes and
runs the staged tick.  Nothing else of the tick is written here.

COST: a tick runs the backbone at N = S and the forward at B = S, however many people are present (an idle or held slot's crop is all zero, its
feature is computed and not used): the caller picks the capacity.

Slots, joins, holds, leaves and the op codes are `MultiStreamSession`'s; the warm-up, the graphs and the recovery from a give-up of a persistent
kernel are `stream._Session`'s; after a give-up the tick is run again from the frame and boxes still staged in pinned memory.

Backbone weights: a change in place is noticed at the full check (`_pack`, extended here) -- every 32nd push -- or at the push after `refresh()`;
the per-push cheap check covers the temporal model only (265 more tensors per push would be latency on every frame).  The re-pack runs outside any
capture; the signature carries the backbone's blob and workspace, so graphs captured against one that moved are dropped and captured again.
"""
import numpy as np
import torch

from . import _lib
from .crop import CROP_SIZE
from .demo import convert_crop_cam_to_orig_img, default_mesh_colors
from .engine import OUT_TAILS, on_device
from .filters import smooth_pose
from .stream import MultiStreamSession


def _frame_size(frame_size):
    try:
        H, W = (int(v) for v in frame_size)
    except (TypeError, ValueError):
        raise ValueError('frame_size must be (height, width), got %r' % (frame_size,))
    if H < 1 or W < 1:
        raise ValueError('frame_size must be (height, width) with both >= 1, got %r' % (frame_size,))
    return H, W


class PixelSession(MultiStreamSession):
    """
        ses = PixelSession(model, hmr, vibe, seqlen, slots, frame_size=(H, W))
        boot = ses.join_from_frames(slot, frames_u8[T-1,H,W,3], boxes[T-1,4])     # eager, once per person: HMR + VIBE over the first T - 1 frames
        out = ses.push(frame_u8[H,W,3], {slot: (c_x, c_y, w, h), ...})            # one tick
        out[slot]['verts'], out[slot]['orig_cam'], out[slot]['bbox']
        ses.leave(slot)

    model / hmr / vibe: tepose_amd TePose(seqlen), HMR and VIBE on one device.  `push` returns, per slot that got a box, the base class's pinned rows
    (`keep`, which must hold 'theta') and two host values: `bbox`, the box with width and height times `bbox_scale`, and `orig_cam`,
    `convert_crop_cam_to_orig_img` of theta[:3] and that box (demo.py:315-321).  A joined slot without a box is held.  With overlay=Renderer,
    out['frame'] is the frame with this tick's meshes drawn over it ([H,W,3] uint8 on the device, a new tensor), in ascending `orig_cam[:, 1]` order,
    coloured by `default_mesh_colors` over the slots: an eager step after the tick (draw order is data).

    smooth=(min_cutoff, beta): the base class's one-euro smoothing inside the tick.  `theta`, `verts` and `kp_3d` are the smoothed rows, the overlay draws
    the smoothed vertices, `orig_cam` is what it was (the camera is not filtered), and `join_from_frames` returns its bootstrap rows smoothed too: together
    with the tick rows they are ONE filtered sequence per person, `run_tracklets(smooth=...)`'s."""

    def __init__(self, model, hmr, vibe, seqlen, slots, frame_size, bbox_scale=1.2, J_regressor=None, keep=('theta', 'kp_3d', 'verts'), graph=True,
                 overlay=None, smooth=None):
        self.H, self.W = _frame_size(frame_size)
        self.bbox_scale = float(bbox_scale)
        if not (self.bbox_scale > 0.0 and np.isfinite(self.bbox_scale)):
            raise ValueError('bbox_scale must be finite and > 0, got %r' % (bbox_scale,))
        if 'theta' not in tuple(keep):
            raise ValueError("keep must hold 'theta' (orig_cam is computed from it), got %r" % (tuple(keep),))
        self.hmr, self.vibe, self.overlay = hmr, vibe, overlay
        self.hws = None                      # the backbone's workspace, the session's own (a graph bakes its address in): made by `_pack`
        # packs both models, makes the windows and this class's feed, warms the pixel tick up (every op 0: all-zero crops through the backbone)
        super().__init__(model, seqlen, slots, J_regressor=J_regressor, keep=keep, graph=graph, smooth=smooth)
        self._theta_np = self.out_host['theta'].numpy()
        cols = default_mesh_colors(range(self.S))
        self._colors = np.array([cols[s] for s in range(self.S)], dtype=np.float32)
        self._drawn = None                   # recorded after an overlay: the next tick overwrites frame_dev and the vertices it read

    def _alloc_feed(self):
        """What `_feed` uploads, as ONE pinned block and one device block: S boxes (fp64, first: 8-byte aligned), then S op codes (int32); the frame
        and its pinned staging; the crops; `feat`, which the backbone writes."""
        S, H, W, dev = self.S, self.H, self.W, self.dev
        self.pstage = torch.zeros(S * 36, dtype=torch.uint8, device=dev)
        self.pstage_host = torch.zeros(S * 36, dtype=torch.uint8).pin_memory()
        self.boxes, self.ops = self.pstage[:S * 32].view(torch.float64).view(S, 4), self.pstage[S * 32:].view(torch.int32)
        self.boxes_host, self.ops_host = self.pstage_host[:S * 32].view(torch.float64).view(S, 4), self.pstage_host[S * 32:].view(torch.int32)
        self._boxes_np, self._ops_np = self.boxes_host.numpy(), self.ops_host.numpy()        # the same memory
        self.feat = torch.zeros(S, 2048, device=dev)
        self.frame_host = torch.zeros(H, W, 3, dtype=torch.uint8).pin_memory()
        self.frame_dev = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=dev)
        self.fidx = torch.zeros(S, dtype=torch.int32, device=dev)       # every crop is cut from the one frame
        self.crops = torch.zeros(S, 3, CROP_SIZE, CROP_SIZE, device=dev)

    def _feed(self, variant):
        eng, heng, S = self.eng, self.hmr._engine, self.S
        st = torch.cuda.current_stream(self.dev).cuda_stream
        self.pstage.copy_(self.pstage_host, non_blocking=True)           # boxes and op codes
        if variant == 'host':
            self.frame_dev[0].copy_(self.frame_host, non_blocking=True)  # a frame on the device was copied in front of the tick
        _lib.check(eng.lib.tepose_crop_boxes_u8(self.frame_dev.data_ptr(), 1, self.H, self.W, self.fidx.data_ptr(), self.boxes.data_ptr(), self.bbox_scale,
                                                self.ops.data_ptr(), S, CROP_SIZE, self.crops.data_ptr(), None, None, st), 'tepose_crop_boxes_u8')
        _lib.check(heng.lib.tepose_hmr_features(heng.handle, self.crops.data_ptr(), S, self.feat.data_ptr(), self.hws.data_ptr(), self.hws.numel(), st),
                   'tepose_hmr_features')

    def _signature(self):
        heng = self.hmr._engine
        return super()._signature() + (heng.packed_generation, heng.blob.data_ptr() if heng.blob is not None else 0, self.hws.data_ptr())

    def _pack(self):
        """The full check takes in the backbone (outside any capture): re-packed if its tensors changed, its workspace grown if the packed backbone
        needs more; either moves the signature, and the graphs are dropped."""
        super()._pack()
        heng = self.hmr._engine
        with on_device(self.dev):
            heng.pack_backbone(self.hmr, self.dev)                         # no-op while the tensors' signatures stand
        need = int(heng.lib.tepose_hmr_workspace_bytes(heng.handle, self.S))
        if self.hws is None or self.hws.numel() < need:
            self.stream.synchronize()
            self.hws = torch.empty(need, dtype=torch.uint8, device=self.dev)

    def refresh(self):
        """The next push runs the full weight check (temporal model and backbone) whatever the count since the last one."""
        self._pushes_since_full = 32

    def _check_frames(self, frames, lead):
        shape = lead + (self.H, self.W, 3)
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or tuple(frames.shape) != shape:
            raise ValueError('expected a uint8 array or tensor of shape %s (the session was built for frames of %d x %d), got %s'
                             % (shape, self.H, self.W, (tuple(frames.shape), frames.dtype) if torch.is_tensor(frames) else type(frames)))
        return frames

    def _orig_cam(self, cam, bbox):
        return convert_crop_cam_to_orig_img(cam, bbox, self.W, self.H)

    @torch.no_grad()
    def join_from_frames(self, slot, frames_u8, boxes):
        """The bootstrap of demo.py:171-236 for one person, eager: frames_u8 [seqlen-1,H,W,3] uint8 (host or device) and boxes [seqlen-1,4] (c_x, c_y, w, h)
        -> HMR features of the crops at `bbox_scale`, VIBE over them, `join(slot, features, theta)`.  Returns those frames' outputs: the keys of `keep`
        as [seqlen-1, ...] host tensors (VIBE's: 49 joints), `bbox` (the boxes as given: demo.py:315 scales from row seqlen - 1 on only) and `orig_cam`."""
        s, n = self._slot(slot), self.T - 1
        if self.occupied[s]:
            raise ValueError('slot %d is occupied' % s)
        frames_u8 = self._check_frames(frames_u8, (n,))
        b = np.asarray(boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else boxes, dtype=np.float64)
        if b.shape != (n, 4):
            raise ValueError('boxes must be [seqlen-1, 4] = [%d, 4] (c_x, c_y, w, h), got %s' % (n, b.shape))
        f = self.hmr.features_from_frames(frames_u8.to(self.dev), np.arange(n), b, scale=self.bbox_scale)
        boot = self.vibe(f[None])[-1]
        theta = boot['theta'].reshape(n, 85)
        self.join(s, f, theta)                 # the history, of the windows and of the filter, is the unsmoothed theta
        if self.smooth is not None:
            # these rows eagerly, as run_tracklets does; the slot's first tick recomputes the same filter state from `hist` (op 2)
            verts, pose_hat, joints = smooth_pose(theta[:, 3:75].contiguous(), theta[:, 75:].contiguous(), self.model.regressor.smpl,
                                                  min_cutoff=self.smooth[0], beta=self.smooth[1])
            boot = dict(boot, theta=torch.cat([theta[:, :3], pose_hat.reshape(n, 72), theta[:, 75:]], dim=1), verts=verts, kp_3d=joints)
        out = {k: boot[k].reshape((n,) + tuple(boot[k].shape[-len(OUT_TAILS[k]):])).cpu() for k in self.keep}
        out['bbox'] = b.copy()
        out['orig_cam'] = self._orig_cam(out['theta'][:, :3].numpy(), out['bbox'])
        return out

    @torch.no_grad()
    def push(self, frame_u8, boxes):
        """frame_u8 [H,W,3] uint8: numpy or a host tensor (staged through one pinned buffer; its upload is a node of the graph) or a device tensor (copied
        device to device after the caller's current stream, in front of the replay).  boxes {slot: (c_x, c_y, w, h)} in frame pixels: the occupied slots
        that advance in this tick.  Blocks until the tick's outputs are in pinned memory; returns {slot: rows}, and 'frame' with an overlay."""
        frame_u8 = self._check_frames(frame_u8, ())
        if not isinstance(boxes, dict):
            raise ValueError('boxes must be a dict {slot: (c_x, c_y, w, h)}, got %s' % type(boxes))
        rows = {}
        for slot, box in boxes.items():
            s = self._slot(slot)
            b = np.asarray(box.detach().cpu().numpy() if torch.is_tensor(box) else box, dtype=np.float64)
            if b.shape != (4,):
                raise ValueError('the box of slot %d must be (c_x, c_y, w, h), got shape %s' % (s, b.shape))
            if not self.occupied[s]:
                raise ValueError('a box for idle slot %d' % s)
            rows[s] = b
        active = sorted(rows)
        for s in active:
            self._boxes_np[s] = rows[s]                                    # the other rows are not read: their op is neither 1 nor 2
        if self._drawn is not None:
            self.stream.wait_event(self._drawn)
            self._drawn = None
        if frame_u8.is_cuda:
            # the caller's stream, taken BEFORE the session's becomes current: whatever is still writing the frame there finishes first
            self.stream.wait_stream(torch.cuda.current_stream(frame_u8.device))
            with torch.cuda.stream(self.stream):
                self.frame_dev[0].copy_(frame_u8, non_blocking=True)
        else:
            self.frame_host.copy_(frame_u8)
        self._run_staged('device' if frame_u8.is_cuda else 'host', active, self._stage_ops(active))
        out = {}
        bb = np.stack([rows[s] for s in active]) if active else np.zeros((0, 4))
        bb[:, 2:] = bb[:, 2:] * self.bbox_scale                             # demo.py:315
        oc = self._orig_cam(self._theta_np[active, :3], bb) if active else np.zeros((0, 4))
        for j, s in enumerate(active):
            out[s] = dict(self._rows[s], orig_cam=oc[j], bbox=bb[j])
        if self.overlay is not None:
            if active:
                order = np.argsort(oc[:, 1])                              # as prepare_rendering_results sorts a frame's persons
                pick = np.asarray(active)[order]
                verts = self.rows_dev['verts'][torch.from_numpy(pick).to(self.dev)]
                out['frame'] = self.overlay.render_frames(self.frame_dev, np.zeros(len(active), dtype=np.int64), verts, oc[order], self._colors[pick])[0]
            else:
                out['frame'] = self.frame_dev[0].clone()
            self._drawn = torch.cuda.Event()
            self._drawn.record(torch.cuda.current_stream(self.dev))
        return out
