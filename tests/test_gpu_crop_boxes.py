"""GPU: tepose_crop_boxes_u8 (csrc/crop.hip) -- crops cut from BOXES, the box -> map rule run on the device -- handle-less
and without a model.  The map against tepose_amd.crop.crop_transform's, in every bit; the crops against tepose_crop_frames_u8 fed the host's maps,
in every bit, between guard rows; the op gate.  The existing entry is itself pinned to the fp64 pixel oracle by tests/test_gpu_crop.py, so no
tolerance appears here."""
import os

import numpy as np
import pytest
import torch

import _buffers as BUF

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
SCALE = 1.2
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _lib():
    from tepose_amd import _lib
    return _lib.load()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _outputs(n, S, want_out=True, want_raw=True, want_minv=True):
    """Guarded outputs: a block serves one crop, so an index off by one reaches at most the neighbouring crop -- two crops of guard on each side."""
    out = BUF.guarded_like((n, 3, S, S), n, 'cuda', name='out', guard_rows=2) if want_out else None
    raw = BUF.guarded_like((n, S, S, 3), n, 'cuda', name='raw', guard_rows=2, dtype=torch.uint8) if want_raw else None
    minv = BUF.guarded_like((n, 6), n, 'cuda', name='minv_out', guard_rows=2, dtype=torch.float64) if want_minv else None
    return out, raw, minv


def _from_boxes(frames, idx, boxes, S, ops=None, scale=SCALE, **want):
    n = boxes.shape[0]
    out, raw, minv = _outputs(n, S, **want)
    F, H, W = frames.shape[:3]
    d_idx, d_box, d_ops = _dev(idx, np.int32), _dev(boxes, np.float64), None if ops is None else _dev(ops, np.int32)
    frozen = BUF.Frozen(frames=frames, idx=d_idx, boxes=d_box, ops=d_ops)
    rc = _lib().tepose_crop_boxes_u8(frames.data_ptr(), F, H, W, d_idx.data_ptr(), d_box.data_ptr(), scale, _ptr(d_ops), n, S, _ptr(out), _ptr(raw),
                                     _ptr(minv), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    BUF.assert_guards_intact(out, raw, minv, what='tepose_crop_boxes_u8 n=%d S=%d' % (n, S))
    frozen.assert_unchanged('tepose_crop_boxes_u8')
    return tuple(None if t is None else t.own.clone() for t in (out, raw, minv))


def _from_maps(frames, idx, minv, S, want_out=True, want_raw=True):
    n = minv.shape[0]
    out, raw, _ = _outputs(n, S, want_out, want_raw, False)
    F, H, W = frames.shape[:3]
    d_idx, d_minv = _dev(idx, np.int32), _dev(minv.reshape(n, 6), np.float64)
    rc = _lib().tepose_crop_frames_u8(frames.data_ptr(), F, H, W, d_idx.data_ptr(), d_minv.data_ptr(), n, S, _ptr(out), _ptr(raw),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    BUF.assert_guards_intact(out, raw, what='tepose_crop_frames_u8 n=%d S=%d' % (n, S))
    return tuple(None if t is None else t.own.clone() for t in (out, raw))


def _zero_crop(S):
    """What a crop that reads nothing holds: raw 0, and the normalised constant (0 / 255 - mean) / std per channel in fp32 -- checked against what the
    existing entry stores for a map that lies outside the frame everywhere."""
    norm = torch.tensor([(np.float32(0) - np.float32(m)) / np.float32(s) for m, s in zip(MEAN, STD)], dtype=torch.float32)
    norm = norm.view(3, 1, 1).expand(3, S, S).contiguous().cuda()
    frames = torch.full((1, 5, 7, 3), 200, dtype=torch.uint8, device='cuda')
    out, raw = _from_maps(frames, np.zeros(1, dtype=np.int32), np.array([[[1.0, 0.0, -1e6], [0.0, 1.0, -1e6]]]), S)
    assert not bool(raw.any()) and BUF.same_bits(out[0], norm)
    return norm, torch.zeros(S, S, 3, dtype=torch.uint8, device='cuda')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------ the map
def test_the_device_map_equals_the_host_map_in_every_bit():
    from tepose_amd.crop import crop_transform
    g = np.load(os.path.join(GOLDEN, 'crop_transform.npz'))
    scale, S = float(g['scale']), int(g['meta'][2])
    corner = np.array([[1900.3, 1060.7, 83.4, 121.9], [1899.75, 1061.2, 140.6, 90.3], [1901.05, 1059.45, 61.7, 63.1], [1898.6, 1062.85, 200.2, 310.5]])
    boxes = np.concatenate([g['bboxes'], corner])
    assert boxes.shape == (53, 4) and (corner[:, 2] != corner[:, 3]).all()
    _, want = crop_transform(boxes, scale, S)
    assert np.isfinite(want).all()
    frames = torch.zeros(1, 1080, 1920, 3, dtype=torch.uint8, device='cuda')
    for crop_side in (S, 8):                                              # the map depends on the crop side through dc
        _, want = crop_transform(boxes, scale, crop_side)
        _, _, minv = _from_boxes(frames, np.zeros(53, dtype=np.int32), boxes, crop_side, want_out=False)
        got = minv.cpu().numpy().reshape(53, 2, 3)
        bad = np.nonzero((_bits(got) != _bits(want)).reshape(53, -1).any(axis=1))[0]
        assert bad.size == 0, ('S=%d rows %s: device %r host %r' % (crop_side, bad.tolist(), got[bad[0]].tolist(), want[bad[0]].tolist()))
    # another scale: the rule, not the fixture's constant
    _, want = crop_transform(boxes, 1.0, S)
    _, _, minv = _from_boxes(frames, np.zeros(53, dtype=np.int32), boxes, S, scale=1.0, want_out=False)
    assert (_bits(minv.cpu().numpy().reshape(53, 2, 3)) == _bits(want)).all()


def test_degenerate_boxes_give_the_all_zero_crop():
    frames = torch.from_numpy(np.random.default_rng(4).integers(1, 256, (1, 37, 53, 3), dtype=np.uint8)).cuda()       # no zero byte in the frame
    nan = float('nan')
    boxes = np.array([[26.0, 18.0, 0.0, 20.0], [26.0, 18.0, 20.0, 0.0], [26.0, 18.0, 0.0, 0.0], [nan, 18.0, 20.0, 20.0], [26.0, nan, 20.0, 20.0],
                      [26.0, 18.0, nan, 20.0], [26.0, 18.0, 20.0, nan], [nan, nan, nan, nan], [26.0, 18.0, 20.0, 20.0]])
    out, raw, minv = _from_boxes(frames, np.zeros(9, dtype=np.int32), boxes, 8)
    norm0, raw0 = _zero_crop(8)
    for i in range(8):
        assert not np.isfinite(minv[i].cpu().numpy()).all(), i             # no special case: the map itself is not finite
        assert torch.equal(raw[i], raw0) and BUF.same_bits(out[i], norm0), i
    assert bool((raw[8] != 0).any())                                         # the sound box next to them is cropped


# ------------------------------------------------------------------ the crops
def _six(W, H):
    """inside; over the left / top; over the right / bottom; fully outside; wider than the frame; inside, cut from frame 1"""
    return (np.array([[0.52 * W + 0.3, 0.47 * H + 0.6, 0.41 * H, 0.33 * H], [0.04 * W + 0.2, 0.03 * H + 0.1, 0.37 * H, 0.45 * H],
                      [0.97 * W + 0.7, 0.98 * H + 0.4, 0.43 * H, 0.31 * H], [-3.0 * W, 2.5 * H, 0.3 * H, 0.3 * H],
                      [0.5 * W + 0.37, 0.5 * H + 0.21, 1.37 * W, 1.21 * W], [0.4 * W + 0.77, 0.6 * H + 0.13, 0.5 * H, 0.6 * H]]),
            np.array([0, 0, 0, 0, 0, 1], dtype=np.int32))


@pytest.fixture(scope='module')
def small():
    frames = torch.from_numpy(np.random.default_rng(21).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)).cuda()     # W * 3 = 159: rows not dword-aligned
    boxes, idx = _six(53, 37)
    return frames, boxes, idx


@pytest.mark.parametrize('S', [8, 224])
def test_crops_equal_the_existing_entry_fed_the_host_maps(S, small):
    from tepose_amd.crop import crop_transform
    frames, boxes, idx = small
    _, minv = crop_transform(boxes, SCALE, S)
    want_out, want_raw = _from_maps(frames, idx, minv, S)
    assert bool((want_raw[0] != 0).any()) and not bool(want_raw[3].any()) and bool((want_raw[5] != want_raw[0]).any())
    out, raw, got_minv = _from_boxes(frames, idx, boxes, S)
    assert (_bits(got_minv.cpu().numpy().reshape(6, 2, 3)) == _bits(minv)).all()
    assert torch.equal(raw, want_raw) and BUF.same_bits(out, want_out)
    # each output with the other NULL, against the existing entry called the same way
    only_out, none, _ = _from_boxes(frames, idx, boxes, S, want_raw=False, want_minv=False)
    assert none is None and BUF.same_bits(only_out, _from_maps(frames, idx, minv, S, want_raw=False)[0]) and BUF.same_bits(only_out, want_out)
    none, only_raw, _ = _from_boxes(frames, idx, boxes, S, want_out=False, want_minv=False)
    assert none is None and torch.equal(only_raw, _from_maps(frames, idx, minv, S, want_out=False)[1]) and torch.equal(only_raw, want_raw)


def test_the_op_codes_gate_the_rows(small):
    frames, boxes6, _ = small
    S, ops = 8, np.array([0, 1, 2, 3, 4, -1, 7, 1 << 20], dtype=np.int32)
    boxes = np.concatenate([boxes6, boxes6[:2] + 0.25])
    idx = np.array([0, 1, 0, 1, 0, 1, 0, 1], dtype=np.int32)
    free_out, free_raw, free_minv = _from_boxes(frames, idx, boxes, S)                         # ops == NULL: every row is cropped
    assert all(bool(free_raw[i].any()) for i in (0, 1, 2, 4, 5, 6, 7))
    out, raw, minv = _from_boxes(frames, idx, boxes, S, ops=ops)
    norm0, raw0 = _zero_crop(S)
    for i in range(8):
        if i in (1, 2):
            assert torch.equal(raw[i], free_raw[i]) and BUF.same_bits(out[i], free_out[i]) and BUF.same_bits(minv[i], free_minv[i]), i
        else:
            assert torch.equal(raw[i], raw0) and BUF.same_bits(out[i], norm0) and not bool(minv[i].any()), i
    # the gated-off rows read nothing: NaN boxes and frame indices outside [0, F) in them change no bit
    wild_boxes, wild_idx = boxes.copy(), idx.copy()
    for i in (0, 3, 4, 5, 6, 7):
        wild_boxes[i], wild_idx[i] = float('nan'), (-7, 2, 1 << 30)[i % 3]
    out2, raw2, minv2 = _from_boxes(frames, wild_idx, wild_boxes, S, ops=ops)
    assert torch.equal(raw2, raw) and BUF.same_bits(out2, out) and BUF.same_bits(minv2, minv)
    # ... while an ungated row with a frame index out of range is the all-zero crop, as on the existing entry
    _, raw3, _ = _from_boxes(frames, np.array([2, -1], dtype=np.int32), boxes[:2], S)
    assert not bool(raw3.any())


def test_a_1080p_corner_box_equals_the_existing_entry():
    from tepose_amd.crop import crop_transform
    frames = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (1, 1080, 1920, 3), dtype=np.uint8)).cuda()
    boxes = np.array([[1900.3, 1000.3, 180.0, 240.6]])                     # where an fp32 sampling coordinate fails (tests/test_gpu_crop.py)
    idx = np.zeros(1, dtype=np.int32)
    _, minv = crop_transform(boxes, SCALE, 224)
    want_out, want_raw = _from_maps(frames, idx, minv, 224)
    out, raw, got = _from_boxes(frames, idx, boxes, 224)
    assert bool((raw != 0).any())
    assert (_bits(got.cpu().numpy().reshape(1, 2, 3)) == _bits(minv)).all()
    assert torch.equal(raw, want_raw) and BUF.same_bits(out, want_out)
