"""CPU: the layer-by-layer reference of tests/test_gpu_hmr_layers.py checked on its own (tests/_hmr_layers.py) -- the restatement of the network
is the reference's (its fp64 walk reproduces the fixture the reference's own HMR class wrote), the reference arithmetic alone stays inside the
bound at this network's real widths (a stand-in device: the same walk in fp32 torch), and planted faults are reported at the right convolution
and location.

A fault is planted in the kept tensors only, so the convolution that READS a tampered tensor may fail as well (its kept output was computed from
the untampered one; on a device the error would have travelled on).  The tests therefore pin the FIRST failure, in network order, and the set of
convolutions that may follow it.

(The element counts of the restatement are checked against the library's table in tests/test_gpu_hmr_layers.py: tepose_hmr_features_upto answers
TEPOSE_E_STATE before TEPOSE_E_SHAPE, so a handle that was never packed -- all there is without a GPU -- cannot tell right counts from wrong ones.)
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _hmr_layers as HL
import _hmr_synth as HS
from tepose_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'hmr_features_N3.npz'))


@pytest.fixture(scope='module')
def model():
    from tepose_amd.smpl import SMPL
    from tepose_amd.spin import hmr
    m = hmr(smpl_mean_params=synth.synthetic_mean_params(0), pretrained=False, smpl=SMPL.from_tables(synth.synthetic_smpl(0)))
    sd = m.state_dict()
    for k, v in HS.state_dict_np({k: tuple(v.shape) for k, v in sd.items() if not k.startswith('smpl.')}).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.eval()


@pytest.fixture(scope='module')
def world(model):
    """(folded fp32 weights, the 3 fixture images, the stand-in device's tensors): computed once, never modified (the tests copy what they change)."""
    weights = HL.fold(model.conv_bn_pairs())
    x = torch.from_numpy(HS.images(3))
    return weights, x, HL.standin_taps(weights, x)


def test_restatement_names_the_modules_own_convolutions(model):
    sd = model.state_dict()
    assert len(HL.NET) == 53 and sum(1 for L in HL.NET if L.join) == 15 and HL.FINAL_JOIN == 'ident'        # 16 blocks: 15 joins by a conv1, the last by the pool
    assert [L.name + '.weight' for L in HL.NET] == [k for k in sd if k.endswith('.weight') and sd[k].dim() == 4]
    for L, (conv, _) in zip(HL.NET, model.conv_bn_pairs()):
        assert tuple(conv.weight.shape) == (L.cout, L.cin, L.R, L.R) and conv.stride == (L.stride, L.stride) and conv.padding == (L.pad, L.pad), L
    assert HL.out_count(0, 3) == 3 * 112 * 112 * 64 and HL.joined_count(0, 3) == HL.joined_count(4, 3) == 3 * 56 * 56 * 64
    assert HL.joined_count(5, 3) == 3 * 56 * 56 * 256 and HL.out_count(44, 3) == 147 * 512 and HL.joined_count(52, 3) == HL.out_count(52, 3) == 147 * 2048
    assert max(HL.kp(L) for L in HL.NET) == 4608 and HL.kp(HL.NET[0]) == 160


def test_walk64_reproduces_the_reference_classes_fp64_features(model):
    """The reference ran batch norm unfolded in fp64; the fold kept in fp64 is the same function.  Measured gap: 4.6e-16 of max|feat64|.
    (With the fold rounded to fp32, as the library packs it, the gap is 4.6e-8: that rounding is the device's, not the restatement's.)"""
    x = torch.from_numpy(HS.images(3))
    feat = HL.walk64(HL.fold(model.conv_bn_pairs(), round32=False), x).numpy()
    gap = float(np.abs(feat - G['feat64']).max() / np.abs(G['feat64']).max())
    print('walk64 against the fixture: %.3g of max|feat64|' % gap)
    assert gap <= 1e-12, gap


def test_standin_device_passes_every_layer(world):
    weights, x, taps = world
    records = HL.check_layers(taps, weights, x, True)
    print('\n'.join(HL.format_records(records, 'cpu32')))
    assert len(records) == 54 and [r['idx'] for r in records] == list(range(54))
    assert all(r['ratio'] <= 1.0 for r in records), [r for r in records if not r['ratio'] <= 1.0]
    assert [(r['rows'], r['Kp'], r['cout']) for r in records if r['idx'] in (0, 1, 44, 47)] == [(37632, 160, 64), (9408, 64, 64), (147, 4608, 512), (147, 2048, 512)]


def _copy(taps):
    return HL.Taps(list(taps.out), list(taps.joined), taps.feat)


def _failures(taps, weights, x, raises=False):
    """(failures, the message check_layers raises with); raises=True: through the raising path itself (one test does: a check costs a second)."""
    if raises:
        with pytest.raises(HL.LayerMismatch) as e:
            HL.check_layers(taps, weights, x, True)
        failures = e.value.failures
    else:
        records, failures = HL.check_layers(taps, weights, x, True, raise_on_fail=False)
        assert len(records) == 54 and failures
    msg = str(HL.LayerMismatch(failures))
    print(msg)
    return failures, msg


def _input_nchw(taps, src_idx):
    return taps.out[src_idx].permute(0, 3, 1, 2)


def test_one_element_four_bounds_off_in_a_middle_layer(world):
    weights, x, clean = world
    i, at = 25, (1, 5, 7, 100)                                       # layer3.0.conv2, an interior pixel of its 14 x 14 map
    L = HL.NET[i]
    y64, A = HL.conv_ref(clean.out[i - 1], *weights[i], L.stride, L.pad, True, None)
    bound = (HL.bound_c(L.cin * 9, True) + 2.0 ** -24) * (A + weights[i][1].double().abs())
    taps = _copy(clean)
    taps.out[i] = clean.out[i].clone()
    taps.out[i][at] = float(y64[at] + 4 * bound[at])
    failures, msg = _failures(taps, weights, x, raises=True)
    f = failures[0]
    assert (f['kind'], f['conv'], f['name'], f['loc'], f['border'], f['n_bad']) == ('conv', 25, 'layer3.0.conv2', at, False, 1)
    assert 3.9 < f['ratio'] < 4.1
    assert 'convolution 25 (layer3.0.conv2)' in msg and '(n=1, oh=5, ow=7, c=100), off the border of the 14 x 14 map' in msg
    assert {g['conv'] for g in failures} <= {25, 26} and all(g['loc'][:3] == at[:3] for g in failures)      # its reader, at the same pixel


def test_border_octet_zeroed_in_the_input_of_a_stride_2_layer(world):
    weights, x, clean = world
    i = 12                                                           # layer2.0.conv2: 3 x 3 stride 2 over the 56 x 56 x 128 T_A
    L = HL.NET[i]
    assert (L.R, L.stride, L.src, L.hin, L.cin) == (3, 2, 'A', 56, 128)
    a = _input_nchw(clean, i - 1).clamp_min(0).clone()
    o = int(a[1, :, 0, 0].view(16, 8).sum(dim=1).argmax())           # the corner pixel's heaviest octet: only output pixel (0, 0) reads it
    assert float(a[1, 8 * o:8 * o + 8, 0, 0].sum()) > 0
    a[1, 8 * o:8 * o + 8, 0, 0] = 0
    y = F.conv2d(a, *weights[i], stride=2, padding=1).permute(0, 2, 3, 1)
    taps = _copy(clean)
    taps.out[i] = clean.out[i].clone()
    taps.out[i][1, 0, 0] = y[1, 0, 0]
    failures, msg = _failures(taps, weights, x)
    f = failures[0]
    assert (f['kind'], f['conv'], f['name'], f['loc'][:3], f['border']) == ('conv', 12, 'layer2.0.conv2', (1, 0, 0), True) and f['ratio'] > 1
    assert 1 <= f['n_bad'] <= 128 and 'on the border of the 28 x 28 map' in msg
    assert {g['conv'] for g in failures} <= {12, 13} and all(g['loc'][:3] == (1, 0, 0) for g in failures)


def test_join_that_took_the_previous_blocks_input_as_identity(world):
    weights, x, clean = world
    i = 21                                                           # layer2.3.conv1: identity = the T_J of conv 18; conv 15's has the same shape
    assert HL.NET[i].join == 'ident' and HL.NET[15].join and HL.NET[18].join and clean.joined[15].shape == clean.joined[18].shape
    wrong = (clean.out[20] + clean.joined[15]).clamp_min(0)
    taps = _copy(clean)
    taps.joined[21] = taps.joined[22] = taps.joined[23] = wrong
    failures, msg = _failures(taps, weights, x)
    f = failures[0]
    diff = (wrong.double() - clean.joined[21].double()).abs()
    at = np.unravel_index(int(diff.argmax()), tuple(diff.shape))
    assert (f['kind'], f['conv'], f['name'], f['loc']) == ('join', 21, 'layer2.3.conv1', tuple(int(v) for v in at))
    assert f['n_bad'] == int((wrong != clean.joined[21]).sum()) > 1000
    assert {g['conv'] for g in failures} <= {21, 24}                 # conv 21 read the true join; conv 24 joins with the tampered identity


def test_reader_that_forgot_the_relu(world):
    weights, x, clean = world
    i = 29                                                           # layer3.1.conv2 reads T_A of conv 28 through a ReLU
    assert HL.NET[i].src == 'A'
    taps = _copy(clean)
    taps.out[i] = F.conv2d(_input_nchw(clean, 28), *weights[i], stride=1, padding=1).permute(0, 2, 3, 1).contiguous()
    failures, msg = _failures(taps, weights, x)
    f = failures[0]
    assert (f['kind'], f['conv'], f['name']) == ('conv', 29, 'layer3.1.conv2') and f['ratio'] > 100 and f['n_bad'] > taps.out[i].numel() // 2
    assert {g['conv'] for g in failures} <= {29, 30}


def test_last_three_rows_of_a_147_row_tensor_left_stale(world):
    weights, x, clean = world
    i = 50                                                           # layer4.2.conv1 writes the T_A that layer4.1.conv1 (47) wrote before it
    assert HL.out_count(i, 3) == HL.out_count(47, 3) == 147 * 512
    taps = _copy(clean)
    taps.out[i] = clean.out[i].clone()
    taps.out[i].view(147, 512)[144:] = clean.out[47].view(147, 512)[144:]
    failures, msg = _failures(taps, weights, x)
    f = failures[0]
    assert (f['kind'], f['conv'], f['name'], f['border']) == ('conv', 50, 'layer4.2.conv1', True)
    assert f['loc'][:2] == (2, 6) and f['loc'][2] in (4, 5, 6) and 3 <= f['n_bad'] <= 3 * 512
    assert {g['conv'] for g in failures} <= {50, 51} and all(g['loc'][0] == 2 and g['loc'][1] >= 5 and g['loc'][2] >= 3 for g in failures)


def test_join_one_ulp_off_at_one_element(world):
    weights, x, clean = world
    i, at = 31, (2, 13, 0, 1000)                                     # layer3.2.conv1, on the left border of its 14 x 14 x 1024 input
    assert HL.NET[i].join == 'ident' and tuple(clean.joined[i].shape) == (3, 14, 14, 1024)
    wrong = clean.joined[i].clone()
    wrong[at] = torch.nextafter(wrong[at], torch.tensor(float('inf')))
    assert int((wrong != clean.joined[i]).sum()) == 1
    taps = _copy(clean)
    taps.joined[31] = taps.joined[32] = taps.joined[33] = wrong
    failures, msg = _failures(taps, weights, x)
    f = failures[0]
    assert (f['kind'], f['conv'], f['name'], f['loc'], f['border'], f['n_bad']) == ('join', 31, 'layer3.2.conv1', at, True, 1)
    assert {g['conv'] for g in failures} <= {31, 34} and all(g['kind'] == 'join' for g in failures)


def test_other_things_that_must_not_pass(world):
    """One stale pixel of T_J between two joins, an element never written (still NaN), a wrong max pool border, features off by two bounds."""
    weights, x, clean = world
    taps = _copy(clean)
    taps.joined[13] = clean.joined[13].clone()                       # T_J while layer2.0 runs: written by conv 11, read again by the down-sample (14)
    taps.joined[13][0, 55, 55, 7] += 1.0
    taps.out[40] = clean.out[40].clone()
    taps.out[40][2, 13, 13, 255] = float('nan')
    taps.joined[0] = clean.joined[0].clone()
    taps.joined[0][1, 0, 3, 5] = 0.0
    assert float(clean.joined[0][1, 0, 3, 5]) > 0
    feat = taps.feat.clone()
    k = int(feat[1].argmax())
    feat[1, k] += 2 * 50 * 2.0 ** -24 * float((clean.out[52] + clean.joined[52]).max())
    failures, msg = _failures(HL.Taps(taps.out, taps.joined, feat), weights, x)
    got = [(f['kind'], f['conv'], f['loc']) for f in failures]
    assert got[0] == ('max pool', 0, (1, 0, 3, 5)) and ('T_J kept', 13, (0, 55, 55, 7)) in got and ('T_J kept', 14, (0, 55, 55, 7)) in got
    assert ('conv', 40, (2, 13, 13, 255)) in got and got[-1] == ('features', 53, (1, 0, 0, k))
    assert {c for _, c, _ in got} <= {0, 1, 4, 13, 14, 40, 41, 53}
