"""GPU: the HMR feature extractor and model (tepose_amd.spin.HMR: 53 convolutions as gather + product, folded batch norm, the pooling kernels,
then the regressor entry) against vectors the REFERENCE's own HMR class produced in fp64 on the weights / images of tests/_hmr_synth.py
(tests/golden/make_golden_hmr.py), in both numerics modes.

Feature margin, from the fixture's own e32 = max|feat32 - feat64| / max|feat64| of the reference (2.4e-7): split mode 4 e32 (operands carry 22
bits against the reference's 24), exact mode 2 e32 (the same arithmetic in another summation order).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _hmr_synth as HS
from tepose_amd import _lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'hmr_features_N3.npz'))
MODES = ['split', 'exact']
_cache = {}


def build(mode):
    """(model, features of the 3 fixture images), built once per numerics mode; TEPOSE_EXACT_FP32 is read when the handle is created."""
    if mode not in _cache:
        from tepose_amd.smpl import SMPL
        from tepose_amd.spin import hmr
        old = os.environ.get('TEPOSE_EXACT_FP32')
        os.environ['TEPOSE_EXACT_FP32'] = '1' if mode == 'exact' else '0'
        try:
            model = hmr(smpl_mean_params=synth.synthetic_mean_params(0), pretrained=False, smpl=SMPL.from_tables(synth.synthetic_smpl(0)))
        finally:
            if old is None:
                del os.environ['TEPOSE_EXACT_FP32']
            else:
                os.environ['TEPOSE_EXACT_FP32'] = old
        sd = model.state_dict()
        for k, v in HS.state_dict_np({k: tuple(v.shape) for k, v in sd.items() if not k.startswith('smpl.')}).items():
            sd[k] = torch.from_numpy(v)
        model.load_state_dict(sd, strict=True)
        model = model.cuda().eval()
        x = torch.from_numpy(HS.images(3)).cuda()
        with torch.no_grad():
            feat = model.feature_extractor(x)
        _cache[mode] = (model, x, feat)
    return _cache[mode]


def rel(feat, ref):
    return float(np.abs(feat.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize('mode', MODES)
def test_features_against_reference_fp64(mode):
    model, x, feat = build(mode)
    assert tuple(feat.shape) == (3, 2048) and feat.device == x.device
    e32, margin = float(G['e32']), (4 if mode == 'split' else 2) * float(G['e32'])
    r3 = rel(feat.cpu().numpy(), G['feat64'])
    with torch.no_grad():
        one = torch.cat([model.feature_extractor(x[i:i + 1]) for i in range(3)])
    r1 = rel(one.cpu().numpy(), G['feat64'])
    print('%s: max|feat - feat64| / max|feat64| = %.3g (N = 3), %.3g (N = 1 each); reference fp32 e32 = %.3g, margin %.3g' % (mode, r3, r1, e32, margin))
    assert r3 <= margin and r1 <= margin, (r3, r1, margin)


@pytest.mark.parametrize('mode', MODES)
def test_67_images_cross_the_64_image_pass(mode):
    model, x, feat = build(mode)
    idx = torch.arange(67, device=x.device) % 3
    with torch.no_grad():
        big = model.feature_extractor(x[idx])
    want = feat[idx]
    err = ((big - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max().item()
    print('%s: N = 67 rows against their N = 3 rows: %.3g relative' % (mode, err))
    assert err <= 1e-6, err


def _check_output(out, tag):
    o = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
    assert sorted(o) == ['kp_2d', 'kp_3d', 'theta', 'verts']
    assert o['kp_3d'].shape == (3, 49, 3) and o['kp_2d'].shape == (3, 49, 2) and o['verts'].shape == (3, 6890, 3)
    errs = {'theta': np.abs(o['theta'] - G[tag + '_theta']).max(), 'kp_3d': np.abs(o['kp_3d'] - G[tag + '_kp_3d']).max(),
            'kp_2d': np.abs(o['kp_2d'] - G[tag + '_kp_2d']).max(), 'verts': np.abs(o['verts'][:, ::108][:, :64] - G[tag + '_verts_sub']).max(),
            'verts_sum': np.abs(o['verts'].sum(axis=1) - G[tag + '_verts_sum']).max() / 6890}
    print(tag, {k: '%.3g' % v for k, v in errs.items()})
    for k, v in errs.items():
        assert v < 1e-4, (tag, k, v)


@pytest.mark.parametrize('mode', MODES)
def test_forward_against_reference_fp64(mode):
    model, x, feat = build(mode)
    ip, ish, ic = (torch.from_numpy(a).cuda() for a in HS.init_state(3))
    with torch.no_grad():
        _check_output(model(x)[0], 'default')
        _check_output(model(x, init_pose=ip, init_shape=ish, init_cam=ic)[0], 'init')
        _check_output(model(x, init_pose=ip, init_shape=ish, init_cam=ic, n_iter=0)[0], 'it0')
        xf, out = model(x, return_features=True)
    assert torch.equal(xf, feat)
    _check_output(out[0], 'default')


@pytest.mark.parametrize('mode', MODES)
def test_graph_replay_is_bit_identical(mode):
    model, x, feat = build(mode)
    eng = model._engine
    ws = torch.empty(int(eng.lib.tepose_hmr_workspace_bytes(eng.handle, 3)), dtype=torch.uint8, device=x.device)
    xs = x.clone()
    s = torch.cuda.Stream()
    with torch.no_grad(), eng.use_workspace(ws):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model.feature_extractor(xs)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = model.feature_extractor(xs)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, feat)
    xs.copy_(x.flip(0))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, feat.flip(0))


@pytest.mark.parametrize('mode', MODES)
def test_in_place_change_of_a_running_var_is_seen(mode):
    model, x, feat = build(mode)
    rv = model.layer4[2].bn3.running_var
    keep = rv.clone()
    try:
        with torch.no_grad():
            rv.mul_(4.0)
            changed = model.feature_extractor(x)
            assert not torch.equal(changed, feat)
            rv.copy_(keep)
            assert torch.equal(model.feature_extractor(x), feat)
    finally:
        with torch.no_grad():
            rv.copy_(keep)


@pytest.mark.parametrize('mode', MODES)
def test_blob_rebuilt_from_its_fp32_ranges_gives_identical_features(mode):
    """A second handle that received only tepose_fp32_ranges of the blob and derived the planes itself (the backbone's 53 matrices are entries
    of the handle's plane table like every other weight)."""
    model, x, feat = build(mode)
    src = model._engine
    from tepose_amd.engine import Engine
    old = os.environ.get('TEPOSE_EXACT_FP32')
    os.environ['TEPOSE_EXACT_FP32'] = '1' if mode == 'exact' else '0'
    try:
        dst = Engine(1, 64, kind='hmr')
    finally:
        if old is None:
            del os.environ['TEPOSE_EXACT_FP32']
        else:
            os.environ['TEPOSE_EXACT_FP32'] = old
    assert dst.packed_bytes == src.packed_bytes
    blob = torch.zeros(dst.packed_bytes, dtype=torch.uint8, device=x.device)
    ranges = src.fp32_ranges()
    assert sum(n for _, n in ranges) < 0.6 * src.packed_bytes
    for off, n in ranges:
        blob[off:off + n] = src.blob[off:off + n]
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(dst.lib.tepose_set_blob(dst.handle, blob.data_ptr(), blob.numel()), 'tepose_set_blob')
    _lib.check(dst.lib.tepose_derive_planes(dst.handle, stream), 'tepose_derive_planes')
    if mode == 'split':
        assert torch.equal(blob, src.blob)
    ws = torch.empty(int(dst.lib.tepose_hmr_workspace_bytes(dst.handle, 3)), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(feat)
    _lib.check(dst.lib.tepose_hmr_features(dst.handle, x.data_ptr(), 3, out.data_ptr(), ws.data_ptr(), ws.numel(), stream), 'tepose_hmr_features')
    assert torch.equal(out, feat)


def test_input_checks():
    model, x, feat = build('split')
    with torch.no_grad():
        with pytest.raises(ValueError):
            model.feature_extractor(x[:, :, :223])
        with pytest.raises(RuntimeError):
            model.feature_extractor(x.cpu())
    lib, h = model._engine.lib, model._engine.handle
    assert lib.tepose_hmr_features(h, x.data_ptr(), 3, feat.data_ptr(), x.data_ptr(), 1024, None) == -3     # TEPOSE_E_WORKSPACE before any launch


def test_dropin_import_builds_and_extracts():
    """`from lib.models.spin import hmr` with dropin/ ahead of a checkout: builds (no ImageNet file here: warns, downloads nothing) and extracts."""
    code = ("import warnings, torch\n"
            "from tepose_amd import synth\n"
            "from tepose_amd.smpl import SMPL\n"
            "from lib.models.spin import hmr\n"
            "with warnings.catch_warnings():\n"
            "    warnings.simplefilter('ignore')\n"
            "    m = hmr(smpl_mean_params=synth.synthetic_mean_params(0), smpl=SMPL.from_tables(synth.synthetic_smpl(0))).cuda().eval()\n"
            "with torch.no_grad():\n"
            "    f = m.feature_extractor(torch.randn(2, 3, 224, 224, device='cuda'))\n"
            "assert tuple(f.shape) == (2, 2048) and bool(torch.isfinite(f).all()) and float(f.abs().max()) > 0\n"
            "print('dropin hmr ok')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'dropin'), ROOT]))
    p = subprocess.run([sys.executable, '-c', code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and 'dropin hmr ok' in p.stdout, p.stdout
