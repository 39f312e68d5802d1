"""CPU: tepose_amd.prepare -- the boxes, the pseudo-theta schedule and its scatter, the two files -- against what the reference's own statements produced
(tests/golden/prepare.npz, written by tests/golden/make_golden_prepare.py from lib/utils/smooth_bbox.py and lib/data_utils/pseudo_theta.py:73-102), and
tools/make_pseudotheta.py --check.

Box tolerance: 1e-8 px on the centre and 1e-8 relative on the scale parameter, the bound tepose_amd.crop.crop_transform is held to: the numpy filters
sum their windows in another order than scipy's C loops, nothing else differs."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tepose_amd import prepare as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'prepare.npz'))
SEED, K, KERNEL, SIGMA, CHUNK = [int(v) for v in G['meta']]
BOX_CASES = [str(c) for c in G['box_cases']]
THRESHOLDS = {'t03': 0.3, 't01': 0.1}


def _kps(name):
    kp, none = G['box_%s_kps' % name], G['box_%s_none' % name]
    return [None if none[i] else kp[i] for i in range(len(kp))]


def _params(bbox, enlarge=1.1):
    """(c_x, c_y, w, h) back to the reference's (c_x, c_y, scale): w = h = 150 / scale * enlarge."""
    assert np.array_equal(bbox[:, 2], bbox[:, 3])
    return np.stack([bbox[:, 0], bbox[:, 1], 150.0 * enlarge / bbox[:, 2]], axis=1)


def _assert_params(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.abs(got[:, :2] - want[:, :2]).max() <= 1e-8
    assert (np.abs(got[:, 2] - want[:, 2]) / np.abs(want[:, 2])).max() <= 1e-8


def test_the_fixture_holds_the_cases_it_should():
    assert BOX_CASES == ['all_visible_40', 'gaps_45', 'tiny_person_30', 'none_entries_36', 'short_7', 'exactly_33']
    assert (KERNEL, SIGMA, CHUNK) == (11, 8, 7)
    assert [tuple(G['box_gaps_45_%s_span' % t]) for t in THRESHOLDS] == [(2, 42)] * 2            # leading 2 and trailing 3 cut off
    assert tuple(G['box_none_entries_36_t03_span']) == (1, 35)
    assert len(G['box_short_7_kps']) < KERNEL and len(G['box_exactly_33_kps']) == int(4 * SIGMA + 0.5) + 1


@pytest.mark.parametrize('tag', sorted(THRESHOLDS))
@pytest.mark.parametrize('name', BOX_CASES)
def test_boxes_equal_the_reference(name, tag):
    thr = THRESHOLDS[tag]
    start, end = (int(v) for v in G['box_%s_%s_span' % (name, tag)])
    raw, s0, e0 = P.boxes_from_keypoints(_kps(name), thr, smooth=False)
    assert (s0, e0) == (start, end) and raw.shape == (end - start, 4)
    _assert_params(_params(raw), G['box_%s_%s_raw' % (name, tag)])
    smoothed, s1, e1 = P.boxes_from_keypoints(_kps(name), thr, kernel_size=KERNEL, sigma=SIGMA)
    assert (s1, e1) == (start, end)
    want = G['box_%s_%s_smoothed' % (name, tag)]
    assert not want[:start].any()                                  # the reference's zero rows in front: not reproduced
    _assert_params(_params(smoothed), want[start:])
    if not G['box_%s_none' % name].any():                          # the same track as one array
        again, s2, e2 = P.boxes_from_keypoints(G['box_%s_kps' % name], thr, kernel_size=KERNEL, sigma=SIGMA)
        assert (s2, e2) == (start, end) and np.array_equal(again, smoothed)
    other = P.boxes_from_keypoints(_kps(name), thr, smooth=False, enlarge=1.0)[0]
    assert np.allclose(other[:, 2] * 1.1, raw[:, 2], rtol=1e-15) and np.array_equal(other[:, :2], raw[:, :2])


def test_median_filter_pads_with_zeros():
    """A constant track of n samples under `scipy.signal.medfilt`'s zero padding: the window at the first frame holds min(n, k // 2 + 1) samples of the
    track and zeros otherwise, so the output there is the constant while those are the majority and 0 once the kernel is wider than twice the support
    left to it (k > 2 n)."""
    x = np.full(9, 5.0)
    assert np.array_equal(P.median_filter_zero_padded(x, 1), x) and np.array_equal(P.median_filter_zero_padded(x, 11), x)
    assert np.array_equal(P.median_filter_zero_padded(x, 17), x)                                       # 9 inside, 8 zeros at the ends
    y = P.median_filter_zero_padded(x, 19)                                                             # 19 > 2 * 9: zeros are the majority everywhere
    assert y[0] == 0.0 and not y.any()
    y = P.median_filter_zero_padded(np.full(5, 5.0), 7)                                                # window of 7 at frame 0: 4 inside; at frame 2: 5 inside
    assert np.array_equal(y, np.full(5, 5.0))
    y = P.median_filter_zero_padded(np.full(5, 5.0), 9)                                                # frame 0: 5 inside of 9 -> 5; all frames see all 5
    assert np.array_equal(y, np.full(5, 5.0))
    y = P.median_filter_zero_padded(np.full(5, 5.0), 11)                                               # 5 inside of 11 -> 0
    assert not y.any()
    ramp = np.arange(1.0, 8.0)                                                                          # 1 .. 7, kernel 5: [0 0 1 2 3] -> 1, [0 1 2 3 4] -> 2
    assert np.array_equal(P.median_filter_zero_padded(ramp, 5), [1, 2, 3, 4, 5, 5, 5])
    for bad in (0, 4, -3):
        with pytest.raises(ValueError):
            P.median_filter_zero_padded(x, bad)


def test_gaussian_filter_reflects():
    """The Gaussian of a constant is that constant only under a boundary mode that repeats the signal's own values with the weights summing to one:
    `reflect` here.  Zero padding would pull the ends towards 0; 7 and 33 samples are shorter than / exactly one more than the radius of 32."""
    for n in (1, 7, 33, 100):
        y = P.gaussian_filter_reflect(np.full(n, 3.25), 8)
        assert y.shape == (n,) and np.abs(y - 3.25).max() <= 1e-14
    x = np.array([1.0, 2.0, 4.0])                                   # radius 2 at sigma 0.5: d c b a | a b c d: [2 1 | 1 2 4 | 4 2]
    w = np.exp(-0.5 / 0.25 * np.arange(-2, 3) ** 2.0)
    w /= w.sum()
    want = [np.dot(w, [2, 1, 1, 2, 4]), np.dot(w, [1, 1, 2, 4, 4]), np.dot(w, [1, 2, 4, 4, 2])]
    assert np.abs(P.gaussian_filter_reflect(x, 0.5) - want).max() <= 1e-15


def test_no_box_at_all_names_the_threshold():
    kp = G['box_short_7_kps'].copy()
    with pytest.raises(ValueError, match='vis_thresh = 2'):
        P.boxes_from_keypoints(kp, 2)
    with pytest.raises(ValueError, match='vis_thresh = 0.3'):
        P.boxes_from_keypoints([None, None], 0.3)
    with pytest.raises(ValueError, match='vis_thresh'):
        P.boxes_from_keypoints([], 0.3)
    with pytest.raises(ValueError, match=r'\[K, 3\]'):
        P.boxes_from_keypoints([kp[0][:, :2]], 0.3)


# ---- schedule -------------------------------------------------------------------------------------------------------------------------------
def test_schedule_equals_the_reference_loop():
    names, coded = G['sched_vid_name'], G['sched_coded']                 # per output row: the row it came from, its chunk's first row, the chunk length
    assert [int((names == v).sum()) for v in dict.fromkeys(names.tolist())] == [5, 7, 14, 16, 3, 1]
    assert list(dict.fromkeys(names.tolist())) != sorted(set(names.tolist()))
    s = P.pseudo_theta_schedule(names, CHUNK)
    assert s.dtype == np.int64 and s.shape == (len(names), 3)
    assert np.array_equal(s[:, 0], coded[:, 1]) and np.array_equal(s[:, 1], coded[:, 2])
    assert np.array_equal(s[:, 0] + s[:, 2], coded[:, 0]) and np.array_equal(coded[:, 0], np.arange(len(names)))
    # the 16-frame video: two full chunks, then its last 7 rows of which the trailing 2 are used
    v = np.flatnonzero(names == 'a_jump')
    assert s[v[-2:], 0].tolist() == [v[-1] - 6] * 2 and s[v[-2:], 2].tolist() == [5, 6] and s[v[13], 0] == v[7]
    assert P.forwards_of(names, CHUNK, 16384) == [(5, 1), (7, 6), (3, 1), (1, 1)]
    assert P.forwards_of(names, CHUNK, 20) == [(5, 1), (7, 2), (7, 2), (7, 2), (3, 1), (1, 1)]
    assert P.forwards_of(names, CHUNK, 3) == [(5, 1)] + [(7, 1)] * 6 + [(3, 1), (1, 1)]


def test_schedule_refusals():
    with pytest.raises(ValueError, match='contiguous'):
        P.pseudo_theta_schedule(np.array(['a', 'a', 'b', 'a']), 7)
    for bad in (0, -1):
        with pytest.raises(ValueError, match='chunk'):
            P.pseudo_theta_schedule(np.array(['a', 'a']), bad)
    with pytest.raises(ValueError, match='non-empty'):
        P.pseudo_theta_schedule(np.array([], dtype='<U3'), 7)


@pytest.mark.parametrize('max_rows', [16384, 20, 14, 7, 3, 1])
@pytest.mark.parametrize('as_tensor', [False, True])
def test_pseudo_theta_scatters_by_the_schedule(max_rows, as_tensor):
    """The stand-in of the fixture generator: theta[..., :3] = (feature column 0 of the row, of the chunk's first row, the chunk length)."""
    names, coded = G['sched_vid_name'], G['sched_coded']
    N = len(names)
    feats = np.zeros((N, 2048), dtype=np.float32)
    feats[:, 0] = np.arange(N)
    calls = []

    def vibe(x):
        assert torch.is_tensor(x) and x.dtype == torch.float32 and x.shape[2] == 2048 and not x.is_cuda
        B, T = x.shape[:2]
        calls.append((T, B))
        theta = torch.zeros(B, T, 85)
        theta[:, :, 0], theta[:, :, 1], theta[:, :, 2] = x[:, :, 0], x[:, :1, 0], float(T)
        return [{'theta': theta}]

    got = P.pseudo_theta(vibe, torch.from_numpy(feats) if as_tensor else feats, names, CHUNK, max_rows)
    assert got.shape == (N, 85) and got.dtype == np.float32
    assert np.array_equal(got[:, :3].astype(np.int64), coded) and not got[:, 3:].any()
    assert calls == P.forwards_of(names, CHUNK, max_rows)
    assert all(B >= 1 and (B == 1 or B * T <= max_rows) for T, B in calls)
    with pytest.raises(ValueError, match='2048'):
        P.pseudo_theta(vibe, feats[:, :100], names, CHUNK)


# ---- the two files --------------------------------------------------------------------------------------------------------------------------
def test_write_eval_inputs_round_trip(tmp_path):
    import joblib
    from tepose_amd.data import load_eval_db, split_db_into_clips, synthetic_eval_db
    db, pse = synthetic_eval_db([7, 9, 4], seed=5)
    db['valid'][3] = 0
    a, b = str(tmp_path / 'x_db.pt'), str(tmp_path / 'x_pseudotheta.pt')
    P.write_eval_inputs(a, db, b, pse)
    back_db, back_pse = joblib.load(a), joblib.load(b)
    assert isinstance(back_pse, np.ndarray) and back_pse.dtype == pse.dtype and np.array_equal(back_pse, pse)
    assert sorted(back_db) == sorted(db) and all(back_db[k].dtype == db[k].dtype and np.array_equal(back_db[k], db[k]) for k in db)
    got, want = load_eval_db(a, b), split_db_into_clips(db, pse)
    assert list(got) == list(want) == ['clip_00', 'clip_01', 'clip_02'] and len(got['clip_00']['features']) == 6
    for c in want:
        assert sorted(got[c]) == sorted(want[c]) and all(np.array_equal(got[c][k], want[c][k]) for k in want[c])
    for bad_db, bad_pse in ((dict(db, features=db['features'].astype(np.float64)), pse), (dict(db, features=db['features'][:, :100]), pse),
                            (dict(db, pose=db['pose'][:-1]), pse), (dict(db, shape=list(db['shape'])), pse), (db, pse[:-1]), (db, pse[:, :84]),
                            ({k: v for k, v in db.items() if k != 'features'}, pse)):
        with pytest.raises(ValueError):
            P.write_eval_inputs(str(tmp_path / 'y_db.pt'), bad_db, str(tmp_path / 'y_pseudotheta.pt'), bad_pse)
    assert not os.path.exists(str(tmp_path / 'y_db.pt')) and not os.path.exists(str(tmp_path / 'y_pseudotheta.pt'))


# ---- extract_features: argument errors before any device --------------------------------------------------------------------------------------
class _NoDevice:
    def features_from_frames(self, *a, **k):
        raise AssertionError('reached the device')

    def parameters(self):
        raise AssertionError('asked for the device')


def test_extract_features_argument_errors_need_no_device():
    frames = torch.zeros((11, 8, 9, 3), dtype=torch.uint8)
    bb = np.tile([4.0, 4.0, 6.0, 6.0], (11, 1))
    hmr = _NoDevice()
    with pytest.raises(ValueError, match='10 frames'):
        P.extract_features(hmr, frames[:10], bb)                                   # one tensor, one frame short
    with pytest.raises(ValueError, match='12 frames'):
        P.extract_features(hmr, [frames[:4], frames[:4], frames[:4]], bb)          # a list: the total is known at once
    with pytest.raises(ValueError, match='more than the 11'):
        P.extract_features(hmr, (f for f in [frames[:7], frames[:5]]), bb, pass_frames=16)   # a stream: refused at the piece that exceeds, here the last
    with pytest.raises(ValueError, match='uint8'):
        P.extract_features(hmr, [frames[:4], frames[4:].float()], bb)
    with pytest.raises(ValueError, match='uint8'):
        P.extract_features(hmr, frames.numpy(), bb)
    for bad in (bb[:, :3], bb.reshape(-1), bb[None]):
        with pytest.raises(ValueError, match=r'\[n, 4\]'):
            P.extract_features(hmr, frames, bad)
    with pytest.raises(ValueError, match='pass_frames'):
        P.extract_features(hmr, frames, bb, pass_frames=0)


# ---- the tool -------------------------------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location('make_pseudotheta_tool', os.path.join(ROOT, 'tools', 'make_pseudotheta.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_check_mode(tmp_path, capsys):
    from _eval_fixture import write_checkpoint
    from tepose_amd import synth
    from tepose_amd.data import synthetic_eval_db
    T = _tool()
    db, pse = synthetic_eval_db([460, 450, 30, 900], seed=4)
    P.write_eval_inputs(str(tmp_path / 'x_db.pt'), db, str(tmp_path / 'unused.pt'), pse)
    write_checkpoint(tmp_path / 'vibe.pth.tar', synth.synthetic_vibe_state_dict(1, 64, 3))
    argv = ['--check', '--db', str(tmp_path / 'x_db.pt'), '--vibe-ckpt', str(tmp_path / 'vibe.pth.tar'), '--base-data', str(tmp_path / 'base')]
    with pytest.raises(SystemExit) as e:
        T.main(argv)
    assert e.value.code == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep['found'] == [str(tmp_path / 'x_db.pt'), str(tmp_path / 'vibe.pth.tar')] and not rep['ready']
    assert rep['missing'] == [str(tmp_path / 'base' / f) for f in T.BASE_FILES]
    assert rep['columns']['features'] == [1840, 2048] and rep['columns']['vid_name'] == [1840]
    assert (rep['frames'], rep['videos'], rep['chunks']) == (1840, 4, 6)
    assert rep['chunks_by_length'] == {'450': 5, '30': 1}                        # 460 -> 1 + the overlapping tail, 450 -> 1, 30 -> itself, 900 -> 2
    assert rep['forwards'] == 2 and rep['rows_per_forward'] == [2250, 30]
    assert rep['out'] == str(tmp_path / 'x_pseudotheta.pt') and abs(rep['performance'] - 51.2) < 1e-9
    rep = T.check_report(T.parse_args(argv + ['--chunk', '100', '--max-rows', '250']))
    assert rep['chunks_by_length'] == {'100': 19, '30': 1} and rep['rows_per_forward'] == [200] * 9 + [100, 30]
    rep = T.check_report(T.parse_args(['--check', '--db', str(tmp_path / 'nowhere_db.pt'), '--vibe-ckpt', str(tmp_path / 'no.pth.tar')]))
    assert len(rep['missing']) == 6 and 'columns' not in rep and not rep['ready']
    capsys.readouterr()
    with pytest.raises(SystemExit):
        T.parse_args(['--help'])
    assert 'insta_train' in capsys.readouterr().out                               # the h5 branch is out of scope, and --help says so


# ---- the fixture generator ------------------------------------------------------------------------------------------------------------------
GEN = os.path.join(ROOT, 'tests', 'golden', 'make_golden_prepare.py')
from test_golden_generator import REF  # noqa: E402 -- where the sibling generators' tests look for the reference checkout


@pytest.mark.skipif(not (os.path.isfile(os.path.join(REF, 'lib', 'utils', 'smooth_bbox.py')) and os.path.isfile(GEN)), reason='reference checkout or generator absent')
def test_fixture_regenerates_bit_identically(tmp_path):
    import subprocess
    import sys
    p = subprocess.run([sys.executable, GEN, '--ref', REF, '--out', str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    a = np.load(os.path.join(str(tmp_path), 'prepare.npz'))
    assert sorted(a.files) == sorted(G.files)
    for k in a.files:
        assert a[k].dtype == G[k].dtype and np.array_equal(a[k], G[k]), k
