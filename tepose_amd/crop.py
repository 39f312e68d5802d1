"""Person crops of video frames on the device: the reference's `CropDataset` (lib/dataset/inference.py:58-74 over
`get_single_image_crop_demo`, lib/data_utils/_img_utils.py:53-101,219-252) without OpenCV, torchvision or a host image.

`crop_transform` is the box -> affine rule of `gen_trans_from_patch_cv` for rot = 0, no flip (numpy, fp64, with the float32 roundings
of the reference's three source points); `crop_frames` cuts and normalises all crops of a call in one launch of csrc/crop.hip;
`transform_keypoints` is `trans_point2d`.  DESIGN.md section 14."""
import numpy as np
import torch

from . import _lib

CROP_SIZE = 224


def _f32(a):
    """The float32 rounding of an fp64 array, back in fp64."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def crop_transform(bboxes, scale, crop_size=CROP_SIZE):
    """bboxes [n,4] (c_x, c_y, w, h) -> (M [n,2,3], Minv [n,2,3]), fp64: M maps frame coordinates to crop pixels, Minv back.

    `gen_trans_from_patch_cv` (_img_utils.py:53-86) stores its three source points -- centre, centre + (0, h scale / 2), centre +
    (w scale / 2, 0) -- and the three destination points in float32 arrays before `cv2.getAffineTransform` solves for M in fp64.  With
    rot = 0 two points share each coordinate, so the solution is the diagonal map below; the roundings stay: the half extents are rounded
    on their own (`rotate_2d` returns float32), the outer points are rounded after the fp64 sum with the UNROUNDED centre, the centre is
    rounded.  The plain formula crop / (w scale) misses the reference's translation term by up to 0.035 px in a 1920-wide frame.
    Minv is formed from M as `cv2.warpAffine` does (determinant, adjugate, translation), all in fp64."""
    b = np.asarray(bboxes, dtype=np.float64).reshape(-1, 4)
    cx, cy, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    sx, sy = _f32(cx), _f32(cy)
    dx = _f32(cx + _f32(w * scale * 0.5)) - sx
    dy = _f32(cy + _f32(h * scale * 0.5)) - sy
    dc = float(_f32(crop_size * 0.5))
    dd = float(_f32(dc + dc)) - dc
    a, d = dd / dx, dd / dy
    M = np.zeros((b.shape[0], 2, 3), dtype=np.float64)
    M[:, 0, 0], M[:, 0, 2] = a, dc - a * sx
    M[:, 1, 1], M[:, 1, 2] = d, dc - d * sy
    return M, invert_affine(M)


def invert_affine(M):
    """[n,2,3] -> the inverse maps, in the arithmetic of cv2.warpAffine's own inversion (a singular map gives zeros, as there)."""
    M = np.asarray(M, dtype=np.float64)
    det = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
    with np.errstate(divide='ignore', invalid='ignore'):
        D = np.where(det != 0, 1.0 / det, 0.0)
    inv = np.empty_like(M)
    inv[:, 0, 0], inv[:, 1, 1] = M[:, 1, 1] * D, M[:, 0, 0] * D
    inv[:, 0, 1], inv[:, 1, 0] = M[:, 0, 1] * -D, M[:, 1, 0] * -D
    inv[:, 0, 2] = -inv[:, 0, 0] * M[:, 0, 2] - inv[:, 0, 1] * M[:, 1, 2]
    inv[:, 1, 2] = -inv[:, 1, 0] * M[:, 0, 2] - inv[:, 1, 1] * M[:, 1, 2]
    return inv


def transform_keypoints(kp, M):
    """`trans_point2d` (_img_utils.py:40-43) over arrays: kp [..., 2] (further columns, e.g. a confidence, are not read) through M [2,3],
    or through M [n,2,3] for kp [n, ..., 2] (one map per leading index).  fp64 out."""
    kp = np.asarray(kp, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 3:
        M = M.reshape((M.shape[0],) + (1,) * (kp.ndim - 2) + (2, 3))
    x, y = kp[..., 0], kp[..., 1]
    return np.stack([M[..., 0, 0] * x + M[..., 0, 1] * y + M[..., 0, 2], M[..., 1, 0] * x + M[..., 1, 1] * y + M[..., 1, 2]], axis=-1)


def check_frames(frames_u8):
    if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError('frames must be a [F, H, W, 3] torch.uint8 tensor (RGB), got %s'
                         % ((tuple(frames_u8.shape), frames_u8.dtype) if torch.is_tensor(frames_u8) else type(frames_u8),))
    if min(frames_u8.shape[:3]) < 1:
        raise ValueError('frames must not be empty, got %s' % (tuple(frames_u8.shape),))


def on_gpu(frames_u8):
    if not frames_u8.is_cuda:
        raise RuntimeError('tepose_amd runs on MI355X only: pass a cuda tensor (there is no CPU path)')
    return frames_u8.contiguous()


def check_index(frame_index, F):
    """Host copy of the frame indices as int32, every one checked against [0, F): the kernel answers a bad index with a black crop."""
    idx = frame_index.detach().cpu().numpy() if torch.is_tensor(frame_index) else np.asarray(frame_index)
    if idx.ndim != 1 or (idx.size and idx.dtype.kind not in 'iu'):
        raise ValueError('frame_index must be a 1-D integer array, got shape %s dtype %s' % (idx.shape, idx.dtype))
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= F):
        raise IndexError('frame_index must lie in [0, %d), got [%d, %d]' % (F, int(idx.min()), int(idx.max())))
    return idx.astype(np.int32)


def crop_into(frames_u8, idx_i32, minv, crop_size, out, raw):
    """One launch: idx_i32 [n] / minv [n,2,3] (host, checked) -> out [n,3,S,S] fp32 and / or raw [n,S,S,3] uint8 (device, contiguous, or None)."""
    n, dev = int(idx_i32.shape[0]), frames_u8.device
    if n == 0:
        return
    F, H, W = (int(v) for v in frames_u8.shape[:3])
    with torch.cuda.device(dev):
        d_idx = torch.from_numpy(np.ascontiguousarray(idx_i32)).to(dev)
        d_minv = torch.from_numpy(np.ascontiguousarray(minv, dtype=np.float64).reshape(n, 6)).to(dev)
        _lib.check(_lib.load().tepose_crop_frames_u8(frames_u8.data_ptr(), F, H, W, d_idx.data_ptr(), d_minv.data_ptr(), n, int(crop_size),
                                                     None if out is None else out.data_ptr(), None if raw is None else raw.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), 'tepose_crop_frames_u8')


def check_boxes(bboxes, n):
    b = np.asarray(bboxes.detach().cpu().numpy() if torch.is_tensor(bboxes) else bboxes, dtype=np.float64)
    if b.shape != (n, 4):
        raise ValueError('bboxes must be [%d, 4] (c_x, c_y, w, h), one row per frame index; got %s' % (n, b.shape))
    return b


def crop_frames(frames_u8, frame_index, bboxes, scale=1.2, crop_size=CROP_SIZE, return_raw=False):
    """frames_u8 [F,H,W,3] torch.uint8 cuda (RGB); frame_index int[n]; bboxes [n,4] (c_x, c_y, w, h) in frame pixels.
    -> [n,3,S,S] float32 ImageNet-normalised crops (cuda), and with return_raw also the 8-bit crops [n,S,S,3] they were computed from:
    `norm_img` and `raw_img` of `get_single_image_crop_demo` for every row, in one launch."""
    check_frames(frames_u8)                       # shapes, dtypes and indices first, the device last: every argument error shows without a GPU
    idx = check_index(frame_index, int(frames_u8.shape[0]))
    S = int(crop_size)
    if S < 1:
        raise ValueError('crop_size must be >= 1, got %r' % (crop_size,))
    _, minv = crop_transform(check_boxes(bboxes, idx.shape[0]), scale, S)
    frames_u8 = on_gpu(frames_u8)
    n, dev = idx.shape[0], frames_u8.device
    out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
    raw = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) if return_raw else None
    crop_into(frames_u8, idx, minv, S, out, raw)
    return (out, raw) if return_raw else out
