"""The SMPL overlay on video frames, on the device: the reference's `Renderer` (lib/utils/renderer.py:36-121) without pyrender, trimesh,
an OpenGL context or a host image.

`Renderer.render` has the reference's call shape -- one mesh onto one image; `Renderer.render_frames` draws all instances of a stack of
frames through csrc/render.hip in as few calls as the workspace cap allows.  The pixels are pinned to the definition in DESIGN.md section 15
(front faces, top-left fill rule on coordinates snapped to 1/256 px, nearest fragment per instance, later instances over earlier ones, Lambert
shading along the view axis), not to pyrender's fragment shader: that distance is not measured.  Wireframe, `.obj` export and image or video
encoding are not here."""
import numpy as np
import torch

from . import _lib
from .crop import check_frames, check_index, on_gpu

MAX_INSTANCES = 4096        # per call of the library: the pixel key's 12 bits of draw order
MAX_FACES = 1 << 20
MAX_SIDE = 16384
DEFAULT_COLOR = (1.0, 1.0, 0.9)


def rotation_matrix(angle_deg, axis):
    """The 3 x 3 rotation by `angle_deg` degrees about `axis` (Rodrigues, fp64): `angle` / `axis` of renderer.py:79-81."""
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    norm = np.sqrt((a * a).sum())
    if not norm > 0:
        raise ValueError('axis must not be zero, got %r' % (axis,))
    a = a / norm
    t = np.radians(float(angle_deg))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.cos(t) * np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * np.outer(a, a)


def vertex_face_adjacency(faces, V):
    """CSR vertex -> faces for faces [Fc,3] with indices in [0, V): (offsets int32 [V+1], list int32 [3 Fc]), ascending face index per vertex --
    the order in which the kernel sums a vertex' face normals."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vert, face = f.reshape(-1), np.repeat(np.arange(f.shape[0], dtype=np.int64), 3)
    order = np.lexsort((face, vert))
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(vert, minlength=V), out=off[1:])
    return off.astype(np.int32), face[order].astype(np.int32)


def _host(a, dtype, shape, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.dtype.kind not in 'fiu':
        raise ValueError('%s must be numeric, got dtype %s' % (what, a.dtype))
    if a.shape != shape:
        raise ValueError('%s must be %s, got %s' % (what, list(shape), a.shape))
    return np.ascontiguousarray(a, dtype=dtype)


class Renderer:
    """faces [Fc,3] integer (the SMPL topology, `get_smpl_faces()` in the reference); resolution (width, height) or None: with a resolution,
    images of another size are refused, as a pyrender viewport of that size would not fit them."""

    workspace_cap_bytes = 256 << 20      # key planes of one library call (8 bytes per pixel: 16.6 MB for a 1080p frame) plus vertex records

    def __init__(self, faces, resolution=None, orig_img=True, wireframe=False):
        if wireframe:
            raise NotImplementedError('wireframe rendering is not implemented (the filled, shaded mesh only)')
        f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in 'iu':
            raise ValueError('faces must be an integer [Fc, 3] array, got shape %s dtype %s' % (f.shape, f.dtype))
        if f.shape[0] > MAX_FACES:
            raise ValueError('at most %d faces, got %d' % (MAX_FACES, f.shape[0]))
        if f.size and int(f.min()) < 0:
            raise ValueError('faces holds a negative vertex index (%d)' % int(f.min()))
        self.faces = np.ascontiguousarray(f, dtype=np.int32)
        self.min_verts = int(f.max()) + 1 if f.size else 1
        if resolution is not None:
            resolution = (int(resolution[0]), int(resolution[1]))
        self.resolution = resolution
        self.orig_img = orig_img
        self._dev = {}          # (device, V) -> (faces, offsets, list) on that device
        self._ws = {}           # device -> workspace tensor, grown on demand

    # ---- device-side constants -----------------------------------------------------------------------------------------------------------
    def _tables(self, dev, V):
        key = (str(dev), V)
        if key not in self._dev:
            off, lst = vertex_face_adjacency(self.faces, V)
            self._dev[key] = tuple(torch.from_numpy(a).to(dev) for a in (self.faces, off, lst))
        return self._dev[key]

    def _workspace(self, dev, nbytes):
        ws = self._ws.get(str(dev))
        if ws is None or ws.numel() < nbytes:
            ws = self._ws[str(dev)] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return ws

    def _check_size(self, H, W):
        if self.resolution is not None and (W, H) != self.resolution:
            raise ValueError('image is %d x %d (width x height), the renderer was made for %d x %d' % ((W, H) + self.resolution))
        if H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError('images of at most %d x %d, got %d x %d' % (MAX_SIDE, MAX_SIDE, W, H))

    # ---- the reference's call ---------------------------------------------------------------------------------------------------------------
    def render(self, img, verts, cam, angle=None, axis=None, color=DEFAULT_COLOR):
        """img [H,W,3] torch.uint8 cuda; verts [V,3] numpy or cuda; cam (sx, sy, tx, ty) -> a new [H,W,3] cuda tensor: the mesh over the image."""
        if not torch.is_tensor(img) or img.dim() != 3:
            raise ValueError('img must be a [H, W, 3] torch.uint8 tensor, got %s' % ((tuple(img.shape), img.dtype) if torch.is_tensor(img) else type(img),))
        if torch.is_tensor(verts):
            if verts.dim() != 2:
                raise ValueError('verts must be [V, 3], got %s' % (tuple(verts.shape),))
            verts = verts[None]
        else:
            verts = np.asarray(verts)
            if verts.ndim != 2:
                raise ValueError('verts must be [V, 3], got %s' % (verts.shape,))
            verts = verts[None]
        rot = rotation_matrix(angle, axis)[None] if (angle and axis is not None and len(axis)) else None      # renderer.py:79: `if angle and axis`
        return self.render_frames(img[None], [0], verts, np.asarray(cam, dtype=np.float64).reshape(1, -1), np.asarray(color).reshape(1, -1), rot=rot)[0]

    # ---- the batched form -------------------------------------------------------------------------------------------------------------------
    def render_frames(self, frames_u8, frame_index, verts, cams, colors, rot=None, out=None, return_winner=False):
        """frames_u8 [F,H,W,3] torch.uint8 cuda; n instances in draw order (those of one frame contiguous; a later one overwrites an earlier one):
        frame_index int[n], verts [n,V,3] (numpy or cuda, float32), cams [n,4] (sx, sy, tx, ty), colors [n,3] in [0, 1], rot [n,3,3] or None.
        -> [F,H,W,3] uint8 (cuda): `out` if given (it may be `frames_u8` itself), else a new tensor.  Frames are processed in chunks whose
        workspace stays under `workspace_cap_bytes` (one frame at least); the result does not depend on the chunking.
        return_winner (tests): also winner [F,H,W,2] int32 (instance, face; -1 uncovered) and depth [F,H,W] float32 (+inf uncovered)."""
        check_frames(frames_u8)                        # shapes, dtypes and indices first, the device last: every argument error shows without a GPU
        F, H, W = (int(v) for v in frames_u8.shape[:3])
        self._check_size(H, W)
        idx = check_index(frame_index, F)
        n = int(idx.shape[0])
        if torch.is_tensor(verts):
            if verts.dim() != 3 or verts.shape[0] != n or verts.shape[2] != 3 or not verts.dtype.is_floating_point:
                raise ValueError('verts must be a floating [%d, V, 3] tensor, got %s %s' % (n, tuple(verts.shape), verts.dtype))
        else:
            verts = np.asarray(verts)
            if verts.ndim != 3 or verts.shape[0] != n or verts.shape[2] != 3 or verts.dtype.kind != 'f':
                raise ValueError('verts must be a floating [%d, V, 3] array, got %s %s' % (n, verts.shape, verts.dtype))
            verts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
        V = int(verts.shape[1])
        if V < self.min_verts:
            raise ValueError('the faces index %d vertices, verts has %d' % (self.min_verts, V))
        cams = _host(cams, np.float64, (n, 4), 'cams')
        colors = _host(colors, np.float32, (n, 3), 'colors')
        if rot is not None:
            rot = _host(rot, np.float64, (n, 3, 3), 'rot').reshape(n, 9)
        per_frame = np.bincount(idx, minlength=F)
        if n and int(per_frame.max()) > MAX_INSTANCES:
            raise ValueError('at most %d instances per frame, got %d' % (MAX_INSTANCES, int(per_frame.max())))
        if out is not None:
            if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (F, H, W, 3) or not out.is_contiguous():
                raise ValueError('out must be a contiguous [%d, %d, %d, 3] torch.uint8 tensor' % (F, H, W))
        frames_u8 = on_gpu(frames_u8)
        dev = frames_u8.device
        if out is None:
            out = torch.empty_like(frames_u8)
        elif out.device != dev:
            raise RuntimeError('out must be on the frames\' device')
        lib = _lib.load()
        with torch.cuda.device(dev):
            d_verts = verts.to(device=dev, dtype=torch.float32).contiguous()
            d_faces, d_off, d_list = self._tables(dev, V)
            winner = torch.empty((F, H, W, 2), dtype=torch.int32, device=dev) if return_winner else None
            depth = torch.empty((F, H, W), dtype=torch.float32, device=dev) if return_winner else None
            Fc = int(self.faces.shape[0])
            need = lambda nf, ni: int(lib.tepose_render_workspace_bytes(H, W, nf, ni, V, Fc))
            stream = torch.cuda.current_stream().cuda_stream
            f0 = 0
            while f0 < F:
                f1, count = f0 + 1, int(per_frame[f0])
                while f1 < F and count + int(per_frame[f1]) <= MAX_INSTANCES and need(f1 + 1 - f0, count + int(per_frame[f1])) <= self.workspace_cap_bytes:
                    count += int(per_frame[f1])
                    f1 += 1
                sel = np.nonzero((idx >= f0) & (idx < f1))[0]               # in draw order
                m = int(sel.shape[0])
                whole = m == n
                pick = (lambda t: t) if whole else (lambda t: t[torch.from_numpy(sel).to(dev)])
                c_verts = pick(d_verts) if m else d_verts
                c_idx = torch.from_numpy(np.ascontiguousarray(idx[sel] - f0, dtype=np.int32)).to(dev)
                c_cams = torch.from_numpy(np.ascontiguousarray(cams[sel])).to(dev)
                c_cols = torch.from_numpy(np.ascontiguousarray(colors[sel])).to(dev)
                c_rot = None if rot is None else torch.from_numpy(np.ascontiguousarray(rot[sel])).to(dev)
                nbytes = need(f1 - f0, m)
                ws = self._workspace(dev, max(nbytes, 8))
                _lib.check(lib.tepose_render_meshes_u8(
                    frames_u8[f0:f1].data_ptr(), f1 - f0, H, W, c_idx.data_ptr(), c_verts.data_ptr(), m, V, d_faces.data_ptr(), Fc,
                    d_off.data_ptr(), d_list.data_ptr(), int(d_list.shape[0]), c_cams.data_ptr(), None if c_rot is None else c_rot.data_ptr(),
                    c_cols.data_ptr(), out[f0:f1].data_ptr(), None if winner is None else winner[f0:f1].data_ptr(),
                    None if depth is None else depth[f0:f1].data_ptr(), ws.data_ptr(), int(ws.numel()), stream), 'tepose_render_meshes_u8')
                if winner is not None and m and not whole:
                    w = winner[f0:f1, :, :, 0]                              # the call's instance numbers -> the caller's
                    w[w >= 0] = torch.from_numpy(sel).to(dev)[w[w >= 0].long()].to(torch.int32)
                f0 = f1
        return (out, winner, depth) if return_winner else out
