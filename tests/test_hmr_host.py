"""CPU: the host side of the HMR feature extractor -- the module's state-dict layout against the reference class's (tests/golden/hmr_state_keys.npz),
the handle's sizes, and every argument-error path of the new C entries, all of which answer before any device access."""
import ctypes
import os
import socket
import warnings

import numpy as np
import pytest
import torch

from tepose_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = np.load(os.path.join(ROOT, 'tests', 'golden', 'hmr_state_keys.npz'))
E_ARG, E_WORKSPACE, E_STATE = -1, -3, -4


def _model(**kw):
    from tepose_amd.smpl import SMPL
    from tepose_amd.spin import hmr
    return hmr(smpl_mean_params=synth.synthetic_mean_params(0), smpl=SMPL.from_tables(synth.synthetic_smpl(0)), **kw)


def _ref_shapes():
    return {str(n): tuple(int(v) for v in s[:d]) for n, s, d in zip(KEYS['names'], KEYS['shapes'], KEYS['ndim'])}


def test_state_dict_matches_the_reference_class():
    """(The reference's `smpl.*` entries belong to smplx and differ by version; tepose_amd.smpl.SMPL accepts and ignores what it does not know.)"""
    model = _model(pretrained=False)
    own = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.startswith('smpl.')}
    ref = _ref_shapes()
    assert own == ref
    assert len(model.conv_bn_pairs()) == 53 and sum(1 for k in ref if k.endswith('num_batches_tracked')) == 53
    sd = {k: torch.full(s, 0.5) if 'num_batches' not in k else torch.tensor(3) for k, s in ref.items()}
    model.load_state_dict(sd, strict=True)
    assert float(model.layer3[5].bn3.running_var[7]) == 0.5
    # a torchvision ResNet-50 state dict: the same backbone keys plus fc.*, loaded non-strictly as the reference's hmr() does
    tv = {k: v for k, v in sd.items() if k.startswith(('conv1.', 'bn1.', 'layer'))}
    tv['fc.weight'], tv['fc.bias'] = torch.zeros(1000, 2048), torch.zeros(1000)
    res = model.load_state_dict(tv, strict=False)
    assert res.unexpected_keys == ['fc.weight', 'fc.bias'] and not any(k.startswith(('conv1.', 'bn1.', 'layer')) for k in res.missing_keys)


def test_layers_other_than_resnet50_are_refused():
    from tepose_amd.spin import HMR
    with pytest.raises(ValueError):
        HMR(None, [2, 2, 2, 2], synth.synthetic_mean_params(0))


def test_handle_sizes_and_error_paths():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.tepose_create_hmr(None) == E_ARG
    assert lib.tepose_create_hmr(ctypes.byref(h)) == 0
    try:
        # the folded backbone (the module's 23.5 M convolution weights, K padded to 32 and C_out to 128, + 53 shifts) + as many bytes of planes
        # + the regressor / SMPL sections of a VIBE handle (whose own encoder is 0.4 M floats at this size)
        v = ctypes.c_void_p()
        assert lib.tepose_create_vibe(1, 64, ctypes.byref(v)) == 0
        tail = lib.tepose_packed_bytes(v)
        lib.tepose_destroy(v)
        bb = lib.tepose_packed_bytes(h) - tail
        n_conv = sum(c.weight.numel() for c, _ in _model(pretrained=False).conv_bn_pairs())
        assert 23.4e6 < n_conv < 23.6e6
        assert 8 * n_conv - 4e6 < bb < 8 * 1.02 * n_conv, (bb, n_conv)
        sizes = [lib.tepose_hmr_workspace_bytes(h, n) for n in (1, 2, 3, 32, 63, 64, 65, 1000)]
        assert all(a < b for a, b in zip(sizes[:6], sizes[1:6])) and sizes[5] == sizes[6] == sizes[7]
        assert lib.tepose_hmr_workspace_bytes(h, 0) == 0 and lib.tepose_hmr_workspace_bytes(None, 1) == 0
        p = 4096                                  # a non-null "device pointer" that must never be touched
        assert lib.tepose_hmr_features(None, p, 1, p, p, 1 << 40, None) == E_ARG
        assert lib.tepose_hmr_features(h, None, 1, p, p, 1 << 40, None) == E_ARG
        assert lib.tepose_hmr_features(h, p, 1, None, p, 1 << 40, None) == E_ARG
        assert lib.tepose_hmr_features(h, p, 1, p, None, 1 << 40, None) == E_ARG
        assert lib.tepose_hmr_features(h, p, 0, p, p, 1 << 40, None) == E_ARG
        assert lib.tepose_hmr_features(h, p, 1, p, p, 1 << 40, None) == E_STATE          # not packed
        n0 = 3 * 112 * 112 * 64                   # what convolution 0 writes for 3 images
        upto = lambda m=h, x=p, N=3, last=0, out=p, ws=p: lib.tepose_hmr_features_upto(m, x, N, last, out, n0, None, 0, ws, 1 << 40, None)
        assert upto(m=None) == E_ARG and upto(x=None) == E_ARG and upto(out=None) == E_ARG and upto(ws=None) == E_ARG
        assert upto(last=-1) == E_ARG and upto(last=53) == E_ARG and upto(N=0) == E_ARG and upto(N=65) == E_ARG
        assert upto() == E_STATE and upto(last=52, N=64) == E_STATE                      # not packed: answered before the counts are looked at
        arr = _lib.ptr_array([p] * 265)
        assert lib.tepose_pack_hmr_backbone(h, arr, 264, None) == E_ARG
        assert lib.tepose_pack_hmr_backbone(None, arr, 265, None) == E_ARG
        assert lib.tepose_pack_hmr_backbone(h, arr, 265, None) == E_STATE                # no blob yet
        t = ctypes.c_void_p()
        assert lib.tepose_create(1, 64, ctypes.byref(t)) == 0
        assert lib.tepose_hmr_features(t, p, 1, p, p, 1 << 40, None) == E_STATE          # a TePose handle
        assert upto(m=t) == E_STATE
        assert lib.tepose_hmr_workspace_bytes(t, 1) == 0
        assert lib.tepose_pack_hmr_backbone(t, arr, 265, None) == E_ARG
        lib.tepose_destroy(t)
        assert b'input=' in lib.tepose_select_kernels(h, 4, 1)                           # the regressor entries plan on it like on a VIBE handle
    finally:
        lib.tepose_destroy(h)


def test_building_block_error_paths():
    lib = _lib.load()
    p = 4096
    need = lib.tepose_conv2d_nhwc_workspace_bytes(1, 7, 7, 64, 64, 3)
    assert need > 0 and lib.tepose_conv2d_nhwc_workspace_bytes(0, 7, 7, 64, 64, 3) == 0
    conv = lambda x=p, w=p, y=p, ws=p, n=need, R=3, stride=1, pad=1: lib.tepose_conv2d_nhwc_f32(x, 1, 7, 7, 64, w, None, 64, R, stride, pad, 0, None, y, 0, ws, n, None)
    assert conv(x=None) == E_ARG and conv(w=None) == E_ARG and conv(y=None) == E_ARG and conv(ws=None) == E_ARG
    assert conv(n=need - 1) == E_WORKSPACE
    assert conv(stride=3) == -2 and conv(pad=2) == -2 and conv(R=9) == -2               # TEPOSE_E_SHAPE
    assert lib.tepose_maxpool3x3s2_nhwc(None, 1, 7, 7, 64, p, None) == E_ARG and lib.tepose_maxpool3x3s2_nhwc(p, 1, 7, 7, 6, p, None) == -2
    assert lib.tepose_avgpool7_nhwc(p, 0, 64, p, None) == E_ARG and lib.tepose_avgpool7_nhwc(p, 1, 64, None, None) == E_ARG
    assert lib.tepose_hmr_fold_pack(p, None, p, p, p, 64, 64, 3, p, p, None) == E_ARG


def test_pretrained_without_a_local_file_warns_and_opens_no_socket(tmp_path, monkeypatch):
    import tepose_amd.spin as S

    def no_network(*a, **k):
        raise AssertionError('hmr() must not touch the network')
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    monkeypatch.setattr(socket, 'socket', no_network)
    monkeypatch.setattr(S, '_warned_imagenet', [False])
    with pytest.warns(RuntimeWarning, match='ImageNet initialisation is skipped'):
        _model(pretrained=True)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        _model(pretrained=True)                   # once
