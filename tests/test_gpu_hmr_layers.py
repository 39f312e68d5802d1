"""GPU: every element of every one of the HMR backbone's 53 convolution outputs, and every join, of the production pass itself
(tepose_hmr_features_upto: the launches of tepose_hmr_features, ended after a given convolution) against the layer-by-layer fp64 reference of
tests/_hmr_layers.py -- bound, exact checks and failure report are described and derived there; tests/test_hmr_layers_helper.py checks them
without a GPU.  The feature comparison of tests/test_gpu_hmr.py sees the same pass only through 3 x 2048 numbers behind a 49-pixel average.

The 3 fixture images and synthetic weights of test_gpu_hmr.build(mode).  3 images are the smallest batch with the shapes that matter: 147-row
products in layer4 (no multiple of the 8, 4, 2 or 1 rows a gather wave takes, a ragged product tile), 9 408- and 37 632-row products in front,
more than one image per gather.  (A gather's second grid-stride trip needs more than 20 images: test_67_images_cross_the_64_image_pass.)

Cost per mode: 53 truncated passes (about 27 whole 3-image passes) and about 1.5 s of fp64 convolutions on 16 host threads.
"""
import pytest
import torch

import _hmr_layers as HL
from test_gpu_hmr import MODES, build
from tepose_amd import _lib

pytestmark = pytest.mark.gpu
E_SHAPE = -2
NAN = float('nan')


def _upto(model, x, i, out, out_n, joined, joined_n, ws):
    eng = model._engine
    return eng.lib.tepose_hmr_features_upto(eng.handle, x.data_ptr(), int(x.shape[0]), i, out.data_ptr(), out_n, None if joined is None else joined.data_ptr(),
                                            joined_n, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)


def _workspace(model, x):
    eng = model._engine
    return torch.empty(int(eng.lib.tepose_hmr_workspace_bytes(eng.handle, int(x.shape[0]))), dtype=torch.uint8, device=x.device)


def tap(model, x, feat):
    """One call per convolution, each into NaN-filled tensors of the size the RESTATEMENT gives them (the entry refuses any other)."""
    N, ws = int(x.shape[0]), _workspace(model, x)
    outs, joins = [], []
    for L in HL.NET:
        out = torch.full((N, L.hout, L.hout, L.cout), NAN, dtype=torch.float32, device=x.device)
        joined = torch.full((N, L.jshape[0], L.jshape[0], L.jshape[1]), NAN, dtype=torch.float32, device=x.device)
        assert out.numel() == HL.out_count(L.idx, N) and joined.numel() == HL.joined_count(L.idx, N)
        _lib.check(_upto(model, x, L.idx, out, out.numel(), joined, joined.numel(), ws), 'tepose_hmr_features_upto(%d)' % L.idx)
        outs.append(out.cpu())
        joins.append(joined.cpu())
    return HL.Taps(outs, joins, feat.cpu())


@pytest.mark.parametrize('mode', MODES)
def test_every_layer_against_fp64(mode):
    model, x, feat = build(mode)
    with torch.no_grad():
        now = model.feature_extractor(x)
    assert torch.equal(now, feat)                                     # the entry under test shares its launch sequence with this one
    taps = tap(model, x, now)
    with torch.no_grad():
        assert torch.equal(model.feature_extractor(x), feat)          # and leaves nothing behind that the next whole pass would see
    records, failures = HL.check_layers(taps, HL.fold(model.conv_bn_pairs()), x.cpu(), mode == 'exact', raise_on_fail=False)
    print('\n'.join(HL.format_records(records, mode)))
    if failures:
        raise HL.LayerMismatch(failures)
    assert len(records) == 54 and all(r['ratio'] <= 1.0 for r in records)


def test_counts_other_than_the_tables_are_refused_before_any_launch():
    """Right counts for all 53 convolutions are accepted above; here one float more or less, and the counts of the neighbouring convolution where
    they differ: TEPOSE_E_SHAPE, nothing written.  (This pins csrc/hmr.h to the restatement; it sits here because the entry checks the handle's
    state before the shapes, and only a packed handle passes that.)"""
    model, x, feat = build('split')
    N, ws = 3, _workspace(model, x)
    big = max(max(HL.out_count(i, N), HL.joined_count(i, N)) for i in range(53)) + 1
    out = torch.full((big,), NAN, dtype=torch.float32, device=x.device)
    joined = torch.full((big,), NAN, dtype=torch.float32, device=x.device)
    for i in range(53):
        o, j = HL.out_count(i, N), HL.joined_count(i, N)
        wrong = [(o + 1, j), (o - 1, j), (o, j + 1), (o, j - 1)]
        k = i + 1 if i < 52 else i - 1
        wrong += [(HL.out_count(k, N), j)] if HL.out_count(k, N) != o else []
        wrong += [(o, HL.joined_count(k, N))] if HL.joined_count(k, N) != j else []
        for on, jn in wrong:
            assert _upto(model, x, i, out, on, joined, jn, ws) == E_SHAPE, (i, on, jn)
        assert _upto(model, x, i, out, o + 1, None, 0, ws) == E_SHAPE and _upto(model, x, i, out, o, joined, j, ws[:1024]) == -3      # TEPOSE_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(joined).all())
    assert _upto(model, x, 52, out, HL.out_count(52, N), None, 12345, ws) == 0          # without `joined` its count is not looked at
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:HL.out_count(52, N)]).all()) and bool(torch.isnan(out[HL.out_count(52, N):]).all()) and bool(torch.isnan(joined).all())
