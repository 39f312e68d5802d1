"""Writers for the two files the evaluation reads (tepose_amd.data.load_eval_db): `*_db.pt` and `*_pseudotheta.pt`.

The reference makes them offline, per dataset: boxes from the annotated 2-D keypoints (lib/utils/smooth_bbox.py:9-121, then
`w = h = 150 / scale * 1.1`, lib/data_utils/threedpw_utils.py:117-133), HMR features of the crops at those boxes
(lib/data_utils/_feature_extractor.py:77-114) and VIBE's thetas over chunks of 450 frames (lib/data_utils/pseudo_theta.py:73-105).
Here the boxes and the schedule are numpy (no scipy: the two filters are restated below), the crops and features are
`HMR.features_from_frames`, the thetas are `VIBE` forwards; nothing is computed by another path.  DESIGN.md section 16."""
from collections import OrderedDict

import numpy as np

PERSON_PX = 150.0          # smooth_bbox.py:58: the box parameter `scale` is 150 / (diagonal of the visible keypoints' extent)


# ---- boxes from keypoints ---------------------------------------------------------------------------------------------------------------------
def _box_param(kp, vis_thresh):
    """`kp_to_bbox_param` (smooth_bbox.py:36-59): [K,3] -> (c_x, c_y, 150 / person height), or None."""
    if kp is None:
        return None
    kp = np.asarray(kp, dtype=np.float64)
    if kp.ndim != 2 or kp.shape[1] < 3:
        raise ValueError('a frame\'s keypoints must be [K, 3] (x, y, confidence) or None, got %s' % (kp.shape,))
    vis = kp[:, 2] > vis_thresh
    if not np.any(vis):
        return None
    lo, hi = kp[vis, :2].min(axis=0), kp[vis, :2].max(axis=0)
    height = np.linalg.norm(hi - lo)
    if height < 0.5:
        return None
    return np.append((lo + hi) / 2.0, PERSON_PX / height)


def _all_box_params(kps, vis_thresh):
    """`get_all_bbox_params` (smooth_bbox.py:62-103): params [end - start, 3] with interior gaps filled as np.linspace fills them, start, end."""
    rows, start, gap, last = [], -1, 0, -1
    for i, kp in enumerate(kps):
        last = i
        p = _box_param(kp, vis_thresh)
        if p is None:
            gap += 1
            continue
        if start == -1:
            start, gap = i, 0
        if gap > 0:
            rows.extend(np.linspace(rows[-1], p, gap + 2)[1:-1])
            gap = 0
        rows.append(p)
    if start == -1:
        raise ValueError('no frame of %d has a keypoint with confidence above vis_thresh = %r and a person of at least 0.5 px: there is no box to return'
                         % (last + 1, vis_thresh))
    return np.stack(rows), start, last - gap + 1


def median_filter_zero_padded(x, kernel_size):
    """`scipy.signal.medfilt(x, kernel_size)` for 1-D x: the median of a centred window, ZEROS beyond both ends (visible in the first and last
    kernel_size // 2 samples, kept because the reference's boxes carry it).  The kernel size must be odd, as scipy demands."""
    k = int(kernel_size)
    if k < 1 or k % 2 == 0:
        raise ValueError('kernel_size must be odd and positive, got %r' % (kernel_size,))
    x = np.asarray(x, dtype=np.float64)
    win = np.lib.stride_tricks.sliding_window_view(np.pad(x, k // 2), k)
    return np.sort(win, axis=1)[:, k // 2]


def gaussian_filter_reflect(x, sigma, truncate=4.0):
    """`scipy.ndimage.gaussian_filter1d(x, sigma)` at its defaults for 1-D x: radius int(truncate sigma + 0.5), weights exp(-t^2 / 2 sigma^2) normalised
    to sum 1, boundary mode 'reflect' (d c b a | a b c d | d c b a -- numpy calls it 'symmetric'), repeated when the signal is shorter than the radius."""
    x = np.asarray(x, dtype=np.float64)
    r = int(truncate * float(sigma) + 0.5)
    t = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * t * t)
    w /= w.sum()
    return np.lib.stride_tricks.sliding_window_view(np.pad(x, r, mode='symmetric'), 2 * r + 1) @ w


def boxes_from_keypoints(kps, vis_thresh, kernel_size=11, sigma=8, smooth=True, enlarge=1.1):
    """kps [N,K,3] (x, y, confidence), or a list of [K,3] arrays / None -> (bbox [n,4] float64 (c_x, c_y, w, h) with w = h, start, end): the boxes of
    frames start .. end - 1 as the reference's dataset builders compute them (`get_smooth_bbox_params` at the builder's `sigma=8`, then
    `w = h = 150 / scale * 1.1`), n = end - start.

    A frame has no box when no keypoint's confidence exceeds `vis_thresh` or the visible keypoints span less than 0.5 px.  Such frames inside the
    track get the linear interpolation of their neighbours' parameters, those before the first / after the last box are cut off: `start` is the first
    frame with a box, `end` one past the last (the reference's `i - num_to_interpolate + 1`).  With `smooth`, each parameter is median-filtered
    (zero padding) and then Gaussian-filtered (reflecting boundary), in this order.  Everything is float64, whatever the keypoints' type.
    The reference prepends `start` rows of zeros to the smoothed parameters; its builders would turn them into infinite boxes that no other column
    has rows for, so they are not reproduced.  No box at all is a ValueError (the reference fails on an empty array)."""
    p, start, end = _all_box_params(kps, vis_thresh)
    if smooth:
        p = np.stack([gaussian_filter_reflect(median_filter_zero_padded(c, kernel_size), sigma) for c in p.T], axis=1)
    side = PERSON_PX / p[:, 2] * float(enlarge)
    return np.stack([p[:, 0], p[:, 1], side, side], axis=1), start, end


# ---- features -------------------------------------------------------------------------------------------------------------------------------
def _passes(frames, n, pass_frames):
    """The caller's frames as a stream of [<= pass_frames, H, W, 3] pieces, each checked when its turn comes; the total is compared with n as early
    as it is known: at once for a tensor or a list, else before the piece that would exceed n, and before the last piece when the stream ends short."""
    import torch
    from . import crop as C
    chunks = [frames] if torch.is_tensor(frames) else frames
    if isinstance(chunks, (list, tuple)):
        for c in chunks:
            C.check_frames(c)
        total = sum(int(c.shape[0]) for c in chunks)
        if total != n:
            raise ValueError('frames hold %d frames, bbox has %d rows' % (total, n))
    seen, held = 0, None
    for c in chunks:
        C.check_frames(c)
        for i in range(0, int(c.shape[0]), pass_frames):
            piece = c[i:i + pass_frames]
            if seen + int(piece.shape[0]) > n:
                raise ValueError('frames hold more than the %d frames bbox has rows for' % n)
            if held is not None:
                yield held
            held, seen = piece, seen + int(piece.shape[0])
    if seen != n:
        raise ValueError('frames hold %d frames, bbox has %d rows' % (seen, n))
    if held is not None:
        yield held


def extract_features(hmr, frames, bbox, scale=1.3, pass_frames=256):
    """`extract_features` of the reference's builders (_feature_extractor.py:77-114; no occluders, no debug, not the `insta` branch): frame i cropped
    at bbox[i] (c_x, c_y, w, h) x `scale`, through the HMR backbone -> [n,2048] float32 numpy.

    `frames` is one [n,H,W,3] torch.uint8 tensor (RGB) or an iterable of such chunks, n = len(bbox) frames in all; anything else is a ValueError
    before the last pass runs.  A chunk on the cpu is uploaded `pass_frames` frames at a time, when their turn comes, and released after their
    pass, so a clip never has to be resident whole; a cuda chunk is sliced in place.  Every pass is `hmr.features_from_frames`; in split mode a row
    is bit-equal to the row a one-tensor call gives (a row does not depend on the pass it rides in)."""
    import torch
    b = np.asarray(bbox.detach().cpu().numpy() if torch.is_tensor(bbox) else bbox, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError('bbox must be [n, 4] (c_x, c_y, w, h), got %s' % (b.shape,))
    if int(pass_frames) < 1:
        raise ValueError('pass_frames must be >= 1, got %r' % (pass_frames,))
    n = b.shape[0]
    out = np.empty((n, 2048), dtype=np.float32)
    dev, at = None, 0
    with torch.no_grad():
        for piece in _passes(frames, n, int(pass_frames)):
            k = int(piece.shape[0])
            if not piece.is_cuda:
                if dev is None:
                    dev = next(hmr.parameters()).device
                piece = piece.to(dev)
            out[at:at + k] = hmr.features_from_frames(piece, np.arange(k), b[at:at + k], scale).cpu().numpy()
            del piece
            at += k
    return out


# ---- pseudo-theta ---------------------------------------------------------------------------------------------------------------------------
def _chunks(vid_name, chunk):
    """The forwards of pseudo_theta.py:73-100 as (first input row, length, first output row, offset of the first row used), in its order."""
    names = np.asarray(vid_name)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError('chunk must be >= 1, got %r' % (chunk,))
    if names.ndim != 1 or names.shape[0] == 0:
        raise ValueError('vid_name must be a non-empty 1-D array, got shape %s' % (names.shape,))
    cuts = np.flatnonzero(names[1:] != names[:-1]) + 1
    starts = np.concatenate([[0], cuts]).astype(np.int64)
    ends = np.concatenate([cuts, [names.shape[0]]]).astype(np.int64)
    runs, count = np.unique(names[starts], return_counts=True)
    if count.max() > 1:
        raise ValueError('the rows of a video must be one contiguous run (the reference slices indexes[0]:indexes[-1]+1); %r comes back after '
                         'another video' % str(runs[count > 1][0]))
    out = []
    for s, e in zip(starts, ends):
        n = int(e - s)
        full = n // chunk
        out += [(int(s) + k * chunk, chunk, int(s) + k * chunk, 0) for k in range(full)]
        if n % chunk:
            length = min(n, chunk)
            out.append((int(e) - length, length, int(s) + full * chunk, length - (n - full * chunk)))
    return out


def _calls(chunks, max_rows):
    """The chunks grouped into forwards: [(T, [chunk, ...]), ...], equal lengths together in order of first appearance, at most max_rows // T (>= 1) per call."""
    by_len = OrderedDict()
    for c in chunks:
        by_len.setdefault(c[1], []).append(c)
    calls = []
    for T, group in by_len.items():
        per_call = max(1, int(max_rows) // T)
        calls += [(T, group[g:g + per_call]) for g in range(0, len(group), per_call)]
    return calls


def pseudo_theta_schedule(vid_name, chunk=450):
    """[N,3] int64, per output row (first row of the chunk it is computed in, that chunk's length, its offset in the chunk): the loop of
    pseudo_theta.py:73-100.  Videos in order of first appearance; n // chunk full chunks from a video's start; when n % chunk != 0 one more chunk over the
    video's LAST min(n, chunk) rows, of which only the trailing n - (n // chunk) chunk rows are used (for n < chunk: the whole video, all used).  Row i
    of the output always describes row i of the input: first + offset == i.  A video whose rows are not one contiguous run is a ValueError."""
    chunks = _chunks(vid_name, chunk)
    sched = np.empty((len(vid_name), 3), dtype=np.int64)
    for first, length, row0, off in chunks:
        k = length - off
        sched[row0:row0 + k] = np.stack([np.full(k, first), np.full(k, length), np.arange(off, length)], axis=1)
    return sched


def pseudo_theta(vibe, features, vid_name, chunk=450, max_rows=16384):
    """The reference's pseudo-theta file for a database (pseudo_theta.py:73-105): features [N,2048] (numpy, or a torch tensor on either side) and
    vid_name [N] -> [N,85] float32 numpy.  Every chunk of `pseudo_theta_schedule` is its own sequence through `vibe(x)[-1]['theta']` (the GRU starts
    from zero in each, as in the reference's `model(batch)` with B = 1); chunks of equal length ride together as one [B,T,2048] forward of at most
    `max_rows` rows (B >= 1 always), and only the rows of a call are uploaded for it.  The camera columns are VIBE's (the readers overwrite them,
    evaluate.py:177-178)."""
    import torch
    chunks = _chunks(vid_name, chunk)
    N = int(np.asarray(vid_name).shape[0])
    is_t = torch.is_tensor(features)
    if tuple(features.shape) != (N, 2048):
        raise ValueError('features must be [%d, 2048] (one row per vid_name entry), got %s' % (N, tuple(features.shape)))
    dev = next(vibe.parameters()).device if isinstance(vibe, torch.nn.Module) else (features.device if is_t else torch.device('cpu'))
    out = np.empty((N, 85), dtype=np.float32)
    with torch.no_grad():
        for T, part in _calls(chunks, max_rows):
            if is_t:
                x = torch.stack([features[f:f + T] for f, _, _, _ in part]).float().to(dev)
            else:
                x = torch.from_numpy(np.stack([np.asarray(features[f:f + T], dtype=np.float32) for f, _, _, _ in part])).to(dev)
            theta = vibe(x)[-1]['theta'].reshape(len(part), T, 85).cpu().numpy()
            for b, (_, _, row0, off) in enumerate(part):
                out[row0:row0 + T - off] = theta[b, off:]
    return out


def forwards_of(vid_name, chunk=450, max_rows=16384):
    """[(T, B), ...]: the forwards `pseudo_theta` issues for this database, in its order."""
    return [(T, len(part)) for T, part in _calls(_chunks(vid_name, chunk), max_rows)]


# ---- the two files --------------------------------------------------------------------------------------------------------------------------
def write_eval_inputs(db_path, db, pseudotheta_path, thetas):
    """joblib.dump of the column dict and of the bare [N,85] array (pseudo_theta.py:104-105), after checking that every column has N =
    len(db['vid_name']) rows, `features` is [N,2048] float32 and `thetas` is [N,85]: the pair `tepose_amd.data.load_eval_db` reads."""
    import joblib
    if not isinstance(db, dict) or 'vid_name' not in db or 'features' not in db:
        raise ValueError('db must be a dict of per-frame columns with at least vid_name and features')
    N = len(db['vid_name'])
    for k, v in db.items():
        if not isinstance(v, np.ndarray) or v.ndim < 1 or v.shape[0] != N:
            raise ValueError('column %r must be a numpy array with %d rows (one per vid_name entry), got %s'
                             % (k, N, v.shape if isinstance(v, np.ndarray) else type(v)))
    f = db['features']
    if f.shape != (N, 2048) or f.dtype != np.float32:
        raise ValueError('features must be [%d, 2048] float32, got %s %s' % (N, f.shape, f.dtype))
    if not isinstance(thetas, np.ndarray) or thetas.shape != (N, 85) or thetas.dtype.kind != 'f':
        raise ValueError('thetas must be a float [%d, 85] numpy array, got %s'
                         % (N, (thetas.shape, thetas.dtype) if isinstance(thetas, np.ndarray) else type(thetas)))
    joblib.dump(db, str(db_path))
    joblib.dump(thetas, str(pseudotheta_path))
