"""GPU: the convolution building blocks of the HMR backbone (csrc/conv.hip + the existing product kernels) against torch in fp64 on the CPU.

Shapes are the smallest at which the gather and the tile edge can go wrong: the network's five geometries on 7 x 7 and 8 x 8 maps (odd / even: every
border case), 1 and 3 images, 64 / 128 output channels -- 16 .. 192 product rows, no multiple of any tile; then the network's widths on the same maps
(WIDE: 256 .. 2048 input channels, K up to 4608, up to 2048 outputs).  The composed network, layer by layer: tests/test_gpu_hmr_layers.py.

Tolerance (derived, not tuned), componentwise against the absolute-value convolution A = |x| (*) |w| in fp64, K = C_in R^2 products per output:
  exact mode   |y - y64| <= (K + 2) 2^-24 A            fp32 products and sums, any summation order
  split mode   |y - y64| <= (2^-21 + (K + 2) 2^-24) A   both operands carried to 22 bits (2 x 2^-23, rounded up to 2^-21 with the dropped lo x lo term)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tepose_amd import _lib

pytestmark = pytest.mark.gpu

GEOMS = {'7x7s2p3': (3, 7, 2, 3), '3x3s1p1': (64, 3, 1, 1), '3x3s2p1': (64, 3, 2, 1), '1x1s1': (64, 1, 1, 0), '1x1s2': (64, 1, 2, 0)}   # C_in, R, stride, pad


def _rng(*key):
    return np.random.default_rng([17] + [int(k) for k in key])


def conv_gpu(x, w, b, stride, pad, relu_in, res, exact):
    lib = _lib.load()
    N, H, W, C = x.shape
    Cout, _, R, _ = w.shape
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    need = int(lib.tepose_conv2d_nhwc_workspace_bytes(N, H, W, C, Cout, R))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    xd, wd = x.cuda().contiguous(), w.cuda().contiguous()
    bd = None if b is None else b.cuda()
    rd = None if res is None else res.cuda().contiguous()
    y = torch.full((N, Ho, Wo, Cout), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(lib.tepose_conv2d_nhwc_f32(xd.data_ptr(), N, H, W, C, wd.data_ptr(), None if bd is None else bd.data_ptr(), Cout, R, stride, pad,
                                          1 if relu_in else 0, None if rd is None else rd.data_ptr(), y.data_ptr(), 1 if exact else 0,
                                          ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), 'tepose_conv2d_nhwc_f32')
    return y.cpu()


def conv_ref(x, w, b, stride, pad, relu_in, res):
    """(y64, A) in NHWC: the fp64 convolution and the absolute-value convolution the bound scales with."""
    a = x.double() + (0 if res is None else res.double())
    if relu_in:
        a = a.clamp_min(0)
    a = a.permute(0, 3, 1, 2)
    y = F.conv2d(a, w.double(), None if b is None else b.double(), stride=stride, padding=pad)
    A = F.conv2d(a.abs(), w.double().abs(), None, stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1), A.permute(0, 2, 3, 1)


def bound_c(K, exact):
    return (K + 2) * 2.0 ** -24 + (0.0 if exact else 2.0 ** -21)


def check_case(x, w, b, stride, pad, relu_in, res, exact, what):
    y = conv_gpu(x, w, b, stride, pad, relu_in, res, exact)
    y64, A = conv_ref(x, w, b, stride, pad, relu_in, res)
    assert tuple(y.shape) == tuple(y64.shape), what
    assert torch.isfinite(y).all(), what
    K = w.shape[1] * w.shape[2] * w.shape[3]
    ratio = float(((y.double() - y64).abs() / (bound_c(K, exact) * A).clamp_min(1e-300)).max())
    print('%s: max error / bound = %.3f' % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize('exact', [False, True], ids=['split', 'exact'])
@pytest.mark.parametrize('geom', sorted(GEOMS))
def test_conv2d_against_fp64(geom, exact):
    cin, R, stride, pad = GEOMS[geom]
    for hw in (7, 8):
        for N in (1, 3):
            for cout in (64, 128):
                g = _rng(hw, N, cout, R, stride)
                x = torch.from_numpy(g.standard_normal((N, hw, hw, cin)).astype(np.float32) * 2)             # negative inputs included
                res = torch.from_numpy(g.standard_normal((N, hw, hw, cin)).astype(np.float32))
                w = torch.from_numpy((g.standard_normal((cout, cin, R, R)) * np.sqrt(2.0 / (cin * R * R))).astype(np.float32))
                b = torch.from_numpy(g.standard_normal(cout).astype(np.float32) * 0.3)
                for relu_in in (False, True):
                    for r in (None, res):
                        check_case(x, w, b, stride, pad, relu_in, r, exact, '%s hw=%d N=%d cout=%d relu=%d res=%d' % (geom, hw, N, cout, relu_in, r is not None))


# The network's widths that the five geometries above never reach (C_in, C_out, R, stride, pad), on the same maps: 256 channels put the gather on
# 32 lanes per row (Kp 256 .. 511; 64 / 3 x 3 x 64 / 3 above take 8, 64 and 16), K = 4608 is the widest product, 2048 the most outputs.
WIDE = {'1x1s1 256-64': (256, 64, 1, 1, 0), '3x3s2p1 512-512': (512, 512, 3, 2, 1), '1x1s1 2048-512': (2048, 512, 1, 1, 0), '1x1s2 1024-2048': (1024, 2048, 1, 2, 0)}


@pytest.mark.parametrize('exact', [False, True], ids=['split', 'exact'])
@pytest.mark.parametrize('geom', sorted(WIDE))
def test_conv2d_network_widths_against_fp64(geom, exact):
    cin, cout, R, stride, pad = WIDE[geom]
    g = _rng(31, cin, cout, R, stride)
    w = torch.from_numpy((g.standard_normal((cout, cin, R, R)) * np.sqrt(2.0 / (cin * R * R))).astype(np.float32))
    b = torch.from_numpy(g.standard_normal(cout).astype(np.float32) * 0.3)
    for hw in (7, 8):
        for N in (1, 3):
            x = torch.from_numpy(g.standard_normal((N, hw, hw, cin)).astype(np.float32) * 2)
            res = torch.from_numpy(g.standard_normal((N, hw, hw, cin)).astype(np.float32))
            for relu_in in (False, True):
                for r in (None, res):
                    check_case(x, w, b, stride, pad, relu_in, r, exact, '%s hw=%d N=%d relu=%d res=%d' % (geom, hw, N, relu_in, r is not None))


@pytest.mark.parametrize('exact', [False, True], ids=['split', 'exact'])
@pytest.mark.parametrize('geom', ['1x1s1', '3x3s1p1'])
def test_rows_of_very_different_magnitude(geom, exact):
    """A pixel of magnitude 1e-3 next to one of 1e4: the split form scales every gathered row by its own power of two, so neither overflows fp16
    nor loses its low bits."""
    cin, R, stride, pad = GEOMS[geom]
    g = _rng(99, R)
    x = g.standard_normal((1, 7, 7, cin)).astype(np.float32)
    x[0, 3, 2] *= 1e-3
    x[0, 3, 3] *= 1e4
    x[0, 0, 0] *= 3e5                                                                 # beyond the fp16 range without the row scale
    w = torch.from_numpy((g.standard_normal((64, cin, R, R)) * np.sqrt(2.0 / (cin * R * R))).astype(np.float32))
    check_case(torch.from_numpy(x), w, None, stride, pad, False, None, exact, geom + ' magnitudes')


@pytest.mark.parametrize('hw', [7, 8, 112])
def test_maxpool_equals_torch(hw):
    """Padding contributes -inf, not 0: the borders (and one whole case) are negative."""
    lib = _lib.load()
    for all_negative in (False, True):
        g = _rng(5, hw, all_negative)
        x = g.standard_normal((2, hw, hw, 64)).astype(np.float32)
        neg = -np.abs(x) - 0.5
        if all_negative:
            x = neg
        else:
            x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1] = neg[:, 0], neg[:, -1], neg[:, :, 0], neg[:, :, -1]
        x = torch.from_numpy(x)
        ho = (hw - 1) // 2 + 1
        y = torch.full((2, ho, ho, 64), float('nan'), dtype=torch.float32, device='cuda')
        xd = x.cuda()
        _lib.check(lib.tepose_maxpool3x3s2_nhwc(xd.data_ptr(), 2, hw, hw, 64, y.data_ptr(), torch.cuda.current_stream().cuda_stream), 'maxpool')
        ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        assert torch.equal(y.cpu(), ref), (hw, all_negative)


def test_avgpool7():
    lib = _lib.load()
    x = torch.from_numpy(_rng(6).standard_normal((3, 7, 7, 2048)).astype(np.float32) * 5)
    y = torch.full((3, 2048), float('nan'), dtype=torch.float32, device='cuda')
    xd = x.cuda()
    _lib.check(lib.tepose_avgpool7_nhwc(xd.data_ptr(), 3, 2048, y.data_ptr(), torch.cuda.current_stream().cuda_stream), 'avgpool')
    ref = x.double().mean(dim=(1, 2))
    err = float((y.cpu().double() - ref).abs().max())
    print('avgpool7: max error %.3g, bound %.3g' % (err, 50 * 2.0 ** -24 * float(x.abs().max())))
    assert err <= 50 * 2.0 ** -24 * float(x.abs().max())


@pytest.mark.parametrize('exact', [False, True], ids=['split', 'exact'])
def test_batch_norm_fold(exact):
    """tepose_pack_hmr_backbone's fold kernel on one convolution with random statistics: the folded weights / shift are the fp64 formula rounded
    once, and the convolution with them equals batch_norm(conv(.)) in fp64 under the bound of this file."""
    lib = _lib.load()
    cout, cin, R = 64, 64, 3
    g = _rng(7)
    w = torch.from_numpy((g.standard_normal((cout, cin, R, R)) * np.sqrt(2.0 / (cin * R * R))).astype(np.float32))
    gamma = torch.from_numpy((g.uniform(0.5, 1.5, cout) * np.where(g.uniform(size=cout) < 0.2, -1, 1)).astype(np.float32))
    beta, mean = (torch.from_numpy(g.standard_normal(cout).astype(np.float32) * 0.3) for _ in range(2))
    var = torch.from_numpy(g.uniform(0.0, 2.0, cout).astype(np.float32))
    var[0] = 0.0                                                                       # eps alone keeps the root positive
    Kp = cin * R * R
    wf = torch.full((cout, Kp), float('nan'), dtype=torch.float32, device='cuda')
    bf = torch.full((cout,), float('nan'), dtype=torch.float32, device='cuda')
    dev = [t.cuda() for t in (w, gamma, beta, mean, var)]
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.tepose_hmr_fold_pack(*[t.data_ptr() for t in dev], cout, cin, R, wf.data_ptr(), bf.data_ptr(), stream), 'tepose_hmr_fold_pack')
    sc = gamma.double() / torch.sqrt(var.double() + 1e-5)
    w64 = w.double() * sc[:, None, None, None]
    b64 = beta.double() - mean.double() * sc
    w_f = wf.cpu().view(cout, R, R, cin).permute(0, 3, 1, 2).contiguous()             # (r, s, c) order back to OIHW
    assert ((w_f.double() - w64).abs() <= 2.0 ** -24 * w64.abs()).all()
    assert ((bf.cpu().double() - b64).abs() <= 2.0 ** -24 * b64.abs()).all()
    x = torch.from_numpy(g.standard_normal((3, 7, 7, cin)).astype(np.float32))
    y = conv_gpu(x, w_f, bf.cpu(), 1, 1, False, None, exact)
    ref = F.batch_norm(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1), mean.double(), var.double(), gamma.double(), beta.double(),
                       training=False, eps=1e-5).permute(0, 2, 3, 1)
    A = F.conv2d(x.double().abs().permute(0, 3, 1, 2), w64.abs(), padding=1).permute(0, 2, 3, 1)
    ratio = float(((y.double() - ref).abs() / (bound_c(Kp, exact) * A)).max())
    print('fold: max error / bound = %.3f' % ratio)
    assert ratio <= 1.0
    bad = var.clone()
    bad[5] = -1.0
    dev[4] = bad.cuda()
    assert lib.tepose_hmr_fold_pack(*[t.data_ptr() for t in dev], cout, cin, R, wf.data_ptr(), bf.data_ptr(), stream) == -1      # TEPOSE_E_ARG
