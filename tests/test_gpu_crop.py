"""GPU: the crop kernel (csrc/crop.hip through tepose_amd.crop.crop_frames) against the fp64 pixel oracle tests/_crop_ref.py, and
HMR.features_from_frames against feature_extractor(crop_frames(...)).

Frames are seeded uint8 noise: the steepest gradients there are, so a sampling coordinate that is off by 1e-4 px (an fp32 coordinate near
x = 1900) moves a value by up to 0.03 grey levels and shows as rounding disagreements outside the window below.

The 8-bit crop must EQUAL the oracle's except where the oracle's pre-rounding value lies within 1e-3 of a half-integer; there +-1 is allowed.
The window is derived, not tuned: with fp64 coordinates and fractions, an fp32 interpolation of 8-bit taps (three lerps and the + 0.5) stays
within ~3.4e-5 grey levels of the exact value (emulated on the CPU), so it can round the other way only that close to a half.  Such pixels
must be rare for the comparison to mean anything: each case asserts, from the oracle alone and before it looks at the kernel, that they are
at most 0.5 % of the case (uniformly distributed fractions give 0.2 %).
"""
import numpy as np
import pytest
import torch

import _crop_ref as R

pytestmark = pytest.mark.gpu
SCALE = 1.2


def _noise(seed, F, H, W):
    return np.random.default_rng(seed).integers(0, 256, (F, H, W, 3), dtype=np.uint8)


def _kinds(W, H, S):
    """Boxes (c_x, c_y, w, h) of every kind for a W x H frame: inside (w != h), over the left / right / top / bottom edge, over a corner (negative
    coordinates), entirely outside, larger than the frame (minification), 12 px wide (magnification), and w * scale = S exactly on an integer corner
    (fx = fy = 0 everywhere: the crop is a copy)."""
    m = min(W, H)
    return np.array([[0.52 * W + 0.3, 0.47 * H + 0.6, 0.41 * m, 0.33 * m],
                     [0.04 * W + 0.2, 0.5 * H + 0.1, 0.37 * m, 0.37 * m],
                     [0.97 * W + 0.7, 0.5 * H + 0.4, 0.43 * m, 0.31 * m],
                     [0.5 * W + 0.9, 0.03 * H + 0.3, 0.29 * m, 0.45 * m],
                     [0.45 * W + 0.1, 0.98 * H + 0.8, 0.39 * m, 0.39 * m],
                     [-0.03 * W - 0.6, -0.02 * H - 0.3, 0.47 * m, 0.36 * m],
                     [-3.0 * W, 2.5 * H, 0.3 * m, 0.3 * m],
                     [0.5 * W + 0.37, 0.5 * H + 0.21, 1.37 * max(W, H), 1.21 * max(W, H)],
                     [0.4 * W + 0.77, 0.6 * H + 0.13, 12.0, 12.0],
                     [3.0 + S / 2.0, 2.0 + S / 2.0, S / SCALE, S / SCALE]])


COPY_ROW, OUTSIDE_ROW = 9, 6


def _case(name):
    """-> frames [F,H,W,3] uint8, frame_index [n], bboxes [n,4], S"""
    g = np.random.default_rng(sum(map(ord, name)))
    if name == 'two_97x131_n70_S56':                       # odd sizes, rows not dword-aligned; repeated, non-monotonic frame indices; more crops than kinds
        frames, S = _noise(1, 2, 97, 131), 56
        bb = np.concatenate([_kinds(131, 97, S)] * 7)
        bb[10:, :2] += g.uniform(-3, 3, (60, 2))
        bb[10:, 2:] *= g.uniform(0.8, 1.25, (60, 2))
        idx = g.integers(0, 2, 70)
        idx[:4] = [1, 0, 1, 1]
    elif name == 'two_97x131_n1_S224':
        frames, S = _noise(1, 2, 97, 131), 224
        bb, idx = _kinds(131, 97, S)[:1], np.array([1])
    elif name == 'one_480x640_S224':
        frames, S = _noise(2, 1, 480, 640), 224
        bb = _kinds(640, 480, S)
        idx = np.zeros(bb.shape[0], dtype=np.int64)
    elif name == 'one_1080x1920_S224':                     # where an fp32 sampling coordinate fails: x = 1700 ... 1900
        frames, S = _noise(3, 1, 1080, 1920), 224
        bb = np.array([[1790.3, 540.7, 170.2, 190.4], [1850.6, 300.2, 110.9, 110.9], [1905.4, 1000.3, 180.0, 240.6], [1765.15, 620.45, 95.3, 140.8]])
        idx = np.zeros(4, dtype=np.int64)
    elif name == 'two_97x131_n65600_S2':                   # more crops than the grid's second dimension holds: the kernel's loop over crops
        frames, S = _noise(1, 2, 97, 131), 2
        n = 65600
        bb = np.stack([g.uniform(-10, 141, n), g.uniform(-10, 107, n), g.uniform(4, 60, n), g.uniform(4, 60, n)], axis=1)
        idx = g.integers(0, 2, n)
    else:
        raise KeyError(name)
    return frames, idx, bb, S


CASES = ['two_97x131_n70_S56', 'two_97x131_n1_S224', 'one_480x640_S224', 'one_1080x1920_S224', 'two_97x131_n65600_S2']


def _oracle(name):
    from tepose_amd.crop import crop_transform
    frames, idx, bb, S = _case(name)
    _, minv = crop_transform(bb, SCALE, S)
    values = R.bilinear(frames, idx, minv, S)
    return frames, idx, bb, S, values


@pytest.mark.parametrize('name', CASES)
def test_crops_against_the_fp64_oracle(name):
    from tepose_amd.crop import crop_frames
    frames, idx, bb, S, values = _oracle(name)
    n = idx.shape[0]
    want, near = R.quantise(values), R.near_half(values, 1e-3)
    share = float(near.mean())
    print('%s: oracle values within 1e-3 of a half-integer: %.4f %%' % (name, 100 * share))
    assert share <= 0.005, share                           # from the oracle alone, before the kernel is looked at
    if name in ('two_97x131_n70_S56', 'one_480x640_S224'):  # the fixture's own sanity: the copy box samples on the pixel grid, the outside box nothing
        assert not want[OUTSIDE_ROW].any()
        assert np.array_equal(want[COPY_ROW], frames[idx[COPY_ROW], 2:2 + S, 3:3 + S])

    d_frames = torch.from_numpy(frames).cuda()
    out, raw = crop_frames(d_frames, idx, bb, scale=SCALE, crop_size=S, return_raw=True)
    assert tuple(out.shape) == (n, 3, S, S) and out.dtype == torch.float32 and tuple(raw.shape) == (n, S, S, 3) and raw.dtype == torch.uint8
    only_out = crop_frames(d_frames, torch.from_numpy(idx), bb, scale=SCALE, crop_size=S)                     # raw_nhwc NULL
    torch.cuda.synchronize()
    raw_np, out_np = raw.cpu().numpy(), out.cpu().numpy()

    diff = raw_np.astype(np.int16) - want.astype(np.int16)
    bad = (diff != 0) & ~(near & (np.abs(diff) <= 1))
    print('%s: %d of %d values differ from the oracle, all inside the window: %s' % (name, int((diff != 0).sum()), diff.size, not bad.any()))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), values[bad][:5].tolist(), raw_np[bad][:5].tolist())

    # the normalised output is the fp32 normalisation of the 8-bit crop the same call returned: two fp32 roundings, one amplified by 1 / std <= 4.5, at |out| <= 2.64
    err = float(np.abs(out_np.astype(np.float64) - R.normalise(raw_np)).max())
    print('%s: max |out - N(raw)| = %.3g' % (name, err))
    assert err <= 2e-6, err
    assert torch.equal(only_out, out)                      # either output alone reproduces the joint call bit for bit


@pytest.mark.parametrize('name', ['two_97x131_n70_S56', 'one_1080x1920_S224'])
def test_raw_output_alone_is_the_joint_call(name):
    """out_nchw NULL: through the C entry point (crop_frames always asks for the normalised output)."""
    from tepose_amd import _lib
    from tepose_amd.crop import crop_frames, crop_transform
    frames, idx, bb, S = _case(name)
    n = idx.shape[0]
    d_frames = torch.from_numpy(frames).cuda()
    _, raw = crop_frames(d_frames, idx, bb, scale=SCALE, crop_size=S, return_raw=True)
    _, minv = crop_transform(bb, SCALE, S)
    d_idx, d_minv = torch.from_numpy(idx.astype(np.int32)).cuda(), torch.from_numpy(minv.reshape(n, 6)).cuda()
    alone = torch.full((n, S, S, 3), 7, dtype=torch.uint8, device='cuda')
    F, H, W = frames.shape[:3]
    _lib.check(_lib.load().tepose_crop_frames_u8(d_frames.data_ptr(), F, H, W, d_idx.data_ptr(), d_minv.data_ptr(), n, S, None, alone.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), 'tepose_crop_frames_u8')
    torch.cuda.synchronize()
    assert torch.equal(alone, raw)


def test_empty_call_and_device_side_argument_checks():
    from tepose_amd.crop import crop_frames
    d_frames = torch.from_numpy(_noise(1, 2, 97, 131)).cuda()
    out, raw = crop_frames(d_frames, np.zeros(0, dtype=np.int64), np.zeros((0, 4)), return_raw=True)
    assert tuple(out.shape) == (0, 3, 224, 224) and tuple(raw.shape) == (0, 224, 224, 3)
    with pytest.raises(IndexError):
        crop_frames(d_frames, [0, 2], np.tile([50., 50., 20., 20.], (2, 1)))
    with pytest.raises(ValueError):
        crop_frames(d_frames.float(), [0], np.array([[50., 50., 20., 20.]]))
    strided = torch.from_numpy(_noise(1, 2, 97, 140)).cuda()[:, :, :131]           # a non-contiguous view is copied, not misread
    assert torch.equal(crop_frames(strided, [1], np.array([[60., 50., 40., 30.]]), crop_size=56),
                       crop_frames(strided.contiguous(), [1], np.array([[60., 50., 40., 30.]]), crop_size=56))


def test_features_from_frames_is_feature_extractor_of_crop_frames():
    """67 crops: a pass of 64 and a tail of 3 through the reused buffer; synthetic HMR weights, split mode: bit-identical (a row
    does not depend on the pass it rides in)."""
    from test_gpu_hmr import build
    from tepose_amd.crop import crop_frames
    model, _, _ = build('split')
    g = np.random.default_rng(67)
    frames = torch.from_numpy(_noise(1, 2, 97, 131)).cuda()
    n = 67
    idx = g.integers(0, 2, n)
    bb = np.stack([g.uniform(10, 120, n), g.uniform(10, 90, n), g.uniform(20, 90, n), g.uniform(20, 90, n)], axis=1)
    with torch.no_grad():
        want = model.feature_extractor(crop_frames(frames, idx, bb, scale=SCALE))
        got = model.features_from_frames(frames, idx, bb, scale=SCALE)
        few = model.features_from_frames(frames, idx[:5], bb[:5], scale=SCALE)
        none = model.features_from_frames(frames, idx[:0], bb[:0])
    assert tuple(got.shape) == (n, 2048) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert len({tuple(r) for r in got[:8].cpu().numpy().round(3).tolist()}) == 8           # different crops, different features
    assert torch.equal(got, want)
    assert torch.equal(few, want[:5])
    assert tuple(none.shape) == (0, 2048)
    with torch.no_grad():
        with pytest.raises(IndexError):
            model.features_from_frames(frames, [0, 5], bb[:2])
        with pytest.raises(RuntimeError, match='MI355X only'):
            model.features_from_frames(frames.cpu(), idx[:2], bb[:2])
