"""The pixel oracle of the crop kernel (csrc/crop.hip): the mathematical definition, in numpy fp64.

  crop pixel (u, v), integer coordinates at pixel centres, samples the frame at x = m0 u + m1 v + m2, y = m3 u + m4 v + m5;
  exact bilinear interpolation of the four taps around (x, y), a tap outside [0, W) x [0, H) contributing 0 on its own;
  raw = floor(value + 0.5) as uint8; out = (raw / 255 - mean) / std per channel.

It is a restatement, not the reference: OpenCV is absent here, so no `cv2.warpAffine` vector exists (OpenCV's fixed-point path quantises
coordinates to 1 / 32 px and weights to 2^-15; that distance is not measured).  Two structurally different formulations are kept so that
the oracle is checked against itself (tests/test_crop_host.py): nested lerps over masked gathers, and a weighted sum over a zero-padded
frame."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])


def coordinates(minv, S):
    """minv [n,2,3] -> x, y [n,S,S] (fp64), indexed [crop, v, u]."""
    m = np.asarray(minv, dtype=np.float64).reshape(-1, 6)[:, :, None, None]
    v, u = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing='ij')
    return m[:, 0] * u + m[:, 1] * v + m[:, 2], m[:, 3] * u + m[:, 4] * v + m[:, 5]


def bilinear(frames, frame_index, minv, S):
    """frames [F,H,W,3] uint8, frame_index [n], minv [n,2,3] -> the interpolated values before rounding, [n,S,S,3] fp64.  Nested lerps; every tap is
    gathered at clipped indices and multiplied by its own inside mask."""
    frames = np.asarray(frames)
    H, W = frames.shape[1:3]
    x, y = coordinates(minv, S)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    f = np.asarray(frame_index, dtype=np.int64)[:, None, None]

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return frames[f, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.float64) * inside[..., None]

    top = tap(y0, x0) + fx * (tap(y0, x0 + 1) - tap(y0, x0))
    bot = tap(y0 + 1, x0) + fx * (tap(y0 + 1, x0 + 1) - tap(y0 + 1, x0))
    return top + fy * (bot - top)


def bilinear_weights(frames, frame_index, minv, S):
    """The same values as a weighted sum of the four taps, w = (1 - fx | fx) (1 - fy | fy), read from a copy of the frames with a one-pixel zero border
    (tap indices clipped onto that border: a tap further out reads a zero as well)."""
    frames = np.asarray(frames)
    H, W = frames.shape[1:3]
    padded = np.zeros((frames.shape[0], H + 2, W + 2, 3), dtype=np.float64)
    padded[:, 1:-1, 1:-1] = frames
    x, y = coordinates(minv, S)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    f = np.asarray(frame_index, dtype=np.int64)[:, None, None]
    out = np.zeros(x.shape + (3,), dtype=np.float64)
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            xi = np.clip(x0 + dx, -1, W).astype(np.int64) + 1
            yi = np.clip(y0 + dy, -1, H).astype(np.int64) + 1
            out += (wx * wy)[..., None] * padded[f, yi, xi]
    return out


def quantise(values):
    """Round half up to the 8-bit crop [n,S,S,3]."""
    return np.floor(values + 0.5).astype(np.uint8)


def near_half(values, window=1e-3):
    """Where the pre-rounding value lies within `window` of a half-integer: an fp32 interpolation may round the other way there."""
    return np.abs(values - np.floor(values) - 0.5) < window


def normalise(raw):
    """[n,S,S,3] uint8 -> [n,3,S,S] fp64, ToTensor + ImageNet Normalize."""
    return ((np.asarray(raw, dtype=np.float64) / 255.0 - MEAN) / STD).transpose(0, 3, 1, 2)
