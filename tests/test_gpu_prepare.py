"""GPU: tepose_amd.prepare on the device -- features of a clip in passes, pseudo-theta along the reference's chunk schedule against the fp64 oracle (at the
fixture's chunk of 7, and at the reference's own chunk of 450: sequences 14 times longer than any other test runs), and the whole way from frames and
keypoints to `run_clips` through the two files.

Long chunks: the bound comes from the oracle alone.  e32 = max|theta of the oracle in float32 - in float64| over the same chunks; the bound is the
project's parity budget of 1e-4 if 4 e32 <= 1e-4, else 4 e32 -- the margin section 13 gives split mode over the reference's own
fp32 distance.  Theta does not depend on the mesh, so the T = 450 oracle runs the functions `oracle.tepose_ref.vibe_fwd` runs up to theta and skips
its LBS (1 350 fp64 meshes would take longer than everything else here together)."""
import os

import numpy as np
import pytest
import torch

from tepose_amd import prepare as P
from tepose_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'prepare.npz'))
CHUNK = int(G['meta'][4])
BUDGET = 1e-4
_cache = {}


@pytest.fixture(scope='module')
def smpl_np():
    return synth.synthetic_smpl(0)


def _vibe(L, H, seed, smpl_np):
    if ('vibe', L, H, seed) not in _cache:
        from test_gpu_vibe import _build
        _cache['vibe', L, H, seed] = _build(L, H, seed, smpl_np)
    return _cache['vibe', L, H, seed]


def _chunks_of(sched):
    return sorted({(int(a), int(b)) for a, b, _ in sched})


def _scatter(sched, per_chunk):
    """per_chunk {(first, length): [length, 85]} -> [N, 85] by the schedule."""
    return np.stack([per_chunk[int(a), int(b)][int(o)] for a, b, o in sched])


def _oracle_theta(state, x, L, dtype):
    """theta [B*T, 85] of oracle.tepose_ref.vibe_fwd(state, ., x, L, dtype=dtype) without its mesh: the same functions in the same order up to theta."""
    from oracle import tepose_ref as O
    enc, reg = O.split_state_dict(state, dtype)
    with torch.no_grad():
        feat = O.vibe_encoder_fwd(enc, torch.as_tensor(x, dtype=dtype), L, True).reshape(-1, 2048)
        pose6d, shape, cam = O.regressor_iterations(reg, feat)
        aa = O.rotmat_to_angle_axis(O.rot6d_to_rotmat(pose6d)).reshape(-1, 72)
    return torch.cat([cam, aa, shape], dim=1).double().numpy()


# ---- 1. features ----------------------------------------------------------------------------------------------------------------------------
def test_extract_features_in_passes_equals_the_whole():
    """11 noise frames of 96 x 128, boxes partly outside: one cuda tensor, cpu chunks of 4 + 4 + 3 (from a generator), passes of 5 -- bit-equal (split mode)
    to each other and to HMR.features_from_frames on the whole."""
    from test_gpu_hmr import build
    model = build('split')[0]
    g = np.random.default_rng(1113)
    frames = torch.from_numpy(g.integers(0, 256, (11, 96, 128, 3), dtype=np.uint8))
    bb = np.stack([g.uniform(-10, 138, 11), g.uniform(-10, 106, 11), g.uniform(30, 120, 11), g.uniform(30, 120, 11)], axis=1)
    bb[0], bb[10] = [3.0, 50.0, 60.0, 60.0], [125.5, 93.25, 80.0, 80.0]                    # over the left edge; over the bottom right corner
    d_frames = frames.cuda()
    with torch.no_grad():
        want = model.features_from_frames(d_frames, np.arange(11), bb, 1.3).cpu().numpy()
    a = P.extract_features(model, d_frames, bb)
    b = P.extract_features(model, (c for c in (frames[:4], frames[4:8], frames[8:])), bb)
    c = P.extract_features(model, frames, bb, pass_frames=5)
    d = P.extract_features(model, [d_frames[:4], frames[4:]], torch.from_numpy(bb), pass_frames=3)
    for got in (a, b, c, d):
        assert isinstance(got, np.ndarray) and got.shape == (11, 2048) and got.dtype == np.float32 and np.isfinite(got).all()
        assert np.array_equal(got, want)
    assert len({tuple(r) for r in want.round(3).tolist()}) == 11                             # different crops, different features
    assert not np.array_equal(P.extract_features(model, d_frames, bb, scale=1.2), want)      # the scale reaches the crop
    with pytest.raises(ValueError, match='8 frames'):                                        # a stream that ends short: refused before its last pass
        P.extract_features(model, (c for c in (frames[:4], frames[4:8])), bb)


# ---- 2. / 4. the fixture's schedule -----------------------------------------------------------------------------------------------------------
def _case2(smpl_np):
    """(model, vid_name, features [46,2048], oracle theta [46,85] in fp64 along the fixture's schedule), computed once."""
    if 'case2' not in _cache:
        from oracle import tepose_ref as O
        model, state = _vibe(2, 64, 31, smpl_np)
        names = G['sched_vid_name']
        x = synth.synthetic_windows(1, len(names), 311)[0, :, :2048].copy()
        sched = P.pseudo_theta_schedule(names, CHUNK)
        assert np.array_equal(sched[:, 0], G['sched_coded'][:, 1]) and np.array_equal(sched[:, 1], G['sched_coded'][:, 2])
        ref = _scatter(sched, {(a, n): O.vibe_fwd(state, smpl_np, x[None, a:a + n], 2, dtype=torch.float64)['theta'].numpy() for a, n in _chunks_of(sched)})
        _cache['case2'] = (model, names, x, ref)
    return _cache['case2']


def test_pseudo_theta_along_the_fixture_schedule_vs_fp64_oracle(smpl_np):
    model, names, x, ref = _case2(smpl_np)
    got = P.pseudo_theta(model, x, names, CHUNK)
    assert got.shape == (len(names), 85) and got.dtype == np.float32
    err = np.abs(got - ref).max()
    print('chunk %d, %d videos, %d rows: max|theta - fp64 oracle| = %.3g' % (CHUNK, len(set(names.tolist())), len(names), err))
    assert err <= BUDGET
    again = P.pseudo_theta(model, torch.from_numpy(x).cuda(), names, CHUNK)                  # features already on the device: the same forwards
    assert np.array_equal(again, got)


def test_batched_and_unbatched_are_both_within_budget(smpl_np):
    """Stacked chunks (one [6,7,2048] forward for the six 7-chunks) and one chunk per call take different kernel families by design: each is held to the
    oracle, their mutual distance is printed."""
    model, names, x, ref = _case2(smpl_np)
    assert P.forwards_of(names, CHUNK, 16384) == [(5, 1), (7, 6), (3, 1), (1, 1)] and P.forwards_of(names, CHUNK, CHUNK) == [(5, 1)] + [(7, 1)] * 6 + [(3, 1), (1, 1)]
    stacked = P.pseudo_theta(model, x, names, CHUNK, max_rows=16384)
    single = P.pseudo_theta(model, x, names, CHUNK, max_rows=CHUNK)
    e1, e2 = np.abs(stacked - ref).max(), np.abs(single - ref).max()
    print('stacked %.3g, one chunk per call %.3g from the oracle; %.3g from each other' % (e1, e2, np.abs(stacked - single).max()))
    assert e1 <= BUDGET and e2 <= BUDGET


# ---- 3. chunks of 450 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lengths,max_rows', [((460,), 450), ((450, 450, 450), 16384)], ids=['one_video_460', 'three_videos_450'])
def test_long_chunks_vs_fp64_oracle(lengths, max_rows, smpl_np):
    """The published bootstrap model (L = 2, H = 1024, add_linear, residual) at the reference's chunk of 450: 460 frames = two B = 1 forwards (`max_rows` = 450
    keeps them apart), the second over the video's last 450 rows; three videos of 450 = one B = 3 forward.

    Measured on one MI355X (this test's printout, kept in profiles/pseudo_theta_long.txt): e32 = 2.65e-7 / 2.60e-7, so the bound is 1e-4 in both cases;
    the device is 2.33e-7 (step 67) / 2.57e-7 (step 445) from the fp64 oracle, and the per-step maxima are flat over the chunk: no growth with T."""
    model, state = _vibe(2, 1024, 3, smpl_np)
    names = np.concatenate([np.array(['v%d' % i] * n) for i, n in enumerate(lengths)])
    x = synth.synthetic_windows(1, len(names), 77)[0, :, :2048].copy()
    sched = P.pseudo_theta_schedule(names, 450)
    chunks = _chunks_of(sched)
    assert all(n == 450 for _, n in chunks) and len(chunks) == (2 if lengths == (460,) else 3)
    xs = np.stack([x[a:a + 450] for a, _ in chunks])
    t64 = _oracle_theta(state, xs, 2, torch.float64).reshape(len(chunks), 450, 85)
    t32 = _oracle_theta(state, xs, 2, torch.float32).reshape(len(chunks), 450, 85)
    e32 = float(np.abs(t32 - t64).max())
    bound = BUDGET if 4 * e32 <= BUDGET else 4 * e32
    calls = P.forwards_of(names, 450, max_rows)
    assert calls == ([(450, 1)] * 2 if lengths == (460,) else [(450, 3)])
    print('forwards (T, B) %s: oracle fp32 vs fp64 e32 = %.3g -> bound %.3g' % (calls, e32, bound))
    assert 0 < e32 and bound == BUDGET                         # which branch applies, from the oracle alone: before the device is looked at
    ref = _scatter(sched, {c: t64[i] for i, c in enumerate(chunks)})
    got = P.pseudo_theta(model, x, names, 450, max_rows)
    assert got.shape == (len(names), 85) and np.isfinite(got).all()
    err = np.abs(got - ref)
    by_step = np.zeros(450)
    np.maximum.at(by_step, sched[:, 2], err.max(axis=1))
    print('device: max|theta - fp64 oracle| = %.3g at step %d of its chunk (row %d, column %d)'
          % (err.max(), int(sched[err.max(axis=1).argmax(), 2]), int(err.max(axis=1).argmax()), int(err.max(axis=0).argmax())))
    print('error by step, maxima over 50-step spans from step 0: ' + ' '.join('%.2g' % by_step[i:i + 50].max() for i in range(0, 450, 50)))
    assert err.max() <= bound


# ---- 5. frames and keypoints -> files -> run_clips ------------------------------------------------------------------------------------------------
def _clip(g, n, H=96, W=128, K=12):
    """A bright blob drifting over noise, and keypoints scattered around it: frames [n,H,W,3] uint8, kps [n,K,3]."""
    t = np.arange(n)
    cx, cy = 40 + 4.0 * t + g.uniform(-1, 1, n), 45 + 1.5 * t + g.uniform(-1, 1, n)
    yy, xx = np.mgrid[0:H, 0:W]
    blob = np.exp(-(((xx[None] - cx[:, None, None]) / 14.0) ** 2 + ((yy[None] - cy[:, None, None]) / 22.0) ** 2))
    frames = np.clip(g.integers(0, 90, (n, H, W, 3)) + 160 * blob[..., None] * g.uniform(0.6, 1.0, 3), 0, 255).astype(np.uint8)
    body = g.uniform(-1, 1, (1, K, 2)) * np.array([14.0, 22.0])
    kps = np.concatenate([np.stack([cx, cy], axis=1)[:, None] + body + g.normal(0, 0.5, (n, K, 2)), g.uniform(0.4, 1.0, (n, K, 1))], axis=2)
    return torch.from_numpy(frames), kps


def test_from_frames_and_keypoints_to_run_clips(tmp_path, smpl_np):
    import joblib
    from test_gpu_hmr import build
    from tepose_amd.data import load_eval_db, split_db_into_clips
    from tepose_amd.driver import run_clips
    from tepose_amd.testing import build_model
    hmr = build('split')[0]
    vibe, _ = _vibe(2, 64, 31, smpl_np)
    model = build_model(1, 64, seed=2, smpl_np=smpl_np, seqlen=4)[0]
    g = np.random.default_rng(912)
    cols = {k: [] for k in ('vid_name', 'frame_id', 'bbox', 'features')}
    for name, n in (('walk_b', 9), ('run_a', 12)):                          # appearance order is not sorted order
        frames, kps = _clip(g, n)
        kps[0, :, 2] = 0.1                                                  # no box for the first frame: the track starts at frame 1
        bbox, start, end = P.boxes_from_keypoints(kps, 0.3)
        assert (start, end) == (1, n) and bbox.shape == (n - 1, 4)
        cols['vid_name'].append(np.array([name] * (end - start)))
        cols['frame_id'].append(np.arange(start, end))
        cols['bbox'].append(bbox)
        cols['features'].append(P.extract_features(hmr, frames[start:end], bbox, pass_frames=4))
    db = {k: np.concatenate(v) for k, v in cols.items()}
    N = len(db['vid_name'])
    assert N == 19 and db['features'].dtype == np.float32
    db.update(joints3D=synth.normal('prep/j3d', (N, 14, 3), std=0.3), pose=synth.normal('prep/pose', (N, 72), std=0.2),
              shape=synth.normal('prep/shape', (N, 10), std=0.5), valid=np.ones(N, dtype=np.float32))
    thetas = P.pseudo_theta(vibe, db['features'], db['vid_name'], chunk=5)
    assert P.forwards_of(db['vid_name'], 5) == [(5, 5)] and thetas.shape == (N, 85)      # 8 = 5 + tail, 11 = 5 + 5 + tail: five chunks of 5, stacked
    a, b = str(tmp_path / 'own_db.pt'), str(tmp_path / 'own_pseudotheta.pt')
    P.write_eval_inputs(a, db, b, thetas)
    back = joblib.load(a)
    assert sorted(back) == sorted(db) and all(back[k].dtype == db[k].dtype and np.array_equal(back[k], db[k]) for k in db)
    assert np.array_equal(joblib.load(b), thetas)
    J = torch.from_numpy(smpl_np['J_regressor_h36m'])

    def run(clips):
        assert list(clips) == ['run_a', 'walk_b'] and [len(c['features']) for c in clips.values()] == [11, 8]
        feats = [torch.from_numpy(np.ascontiguousarray(c['features'])).cuda() for c in clips.values()]
        inits = [torch.from_numpy(np.ascontiguousarray(c['theta_pseu'][:3])).cuda() for c in clips.values()]
        assert all(np.array_equal(c['theta_pseu'][:, :3], np.tile([1., 0., 0.], (len(c['theta_pseu']), 1))) for c in clips.values())
        return run_clips(model, feats, inits, 4, J_regressor=J)
    from_files, in_memory = run(load_eval_db(a, b)), run(split_db_into_clips(db, thetas))
    for f, m, n in zip(from_files, in_memory, (11, 8)):
        assert sorted(f) == sorted(m) == ['kp_3d', 'rotmat', 'theta', 'verts'] and tuple(f['theta'].shape) == (n - 3, 85)
        assert all(torch.equal(f[k], m[k]) and bool(torch.isfinite(f[k]).all()) for k in f)


# ---- 6. the tool ------------------------------------------------------------------------------------------------------------------------------
def test_the_tool_writes_what_pseudo_theta_computes(tmp_path, capsys, smpl_np):
    """tools/make_pseudotheta.py from files alone (fabricated base data, a checkpoint of the published size with a `performance`, a 23-frame database): the file it
    writes holds, bit for bit, `prepare.pseudo_theta` of the same model built in memory."""
    import importlib.util
    import joblib
    import json
    from _eval_fixture import write_base_data, write_checkpoint
    from tepose_amd.data import synthetic_eval_db
    spec = importlib.util.spec_from_file_location('make_pseudotheta_tool', os.path.join(ROOT, 'tools', 'make_pseudotheta.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    model, state = _vibe(2, 1024, 3, smpl_np)
    db, pse = synthetic_eval_db([9, 14], seed=8)
    P.write_eval_inputs(str(tmp_path / 'x_db.pt'), db, str(tmp_path / 'unused.pt'), pse)
    write_base_data(tmp_path / 'base', smpl_np, synth.synthetic_mean_params(0))
    write_checkpoint(tmp_path / 'vibe.pth.tar', state, prefix='module.')
    T.main(['--db', str(tmp_path / 'x_db.pt'), '--vibe-ckpt', str(tmp_path / 'vibe.pth.tar'), '--base-data', str(tmp_path / 'base'), '--chunk', '6'])
    out = capsys.readouterr().out
    assert 'Performance of pretrained model on 3DPW: 51.2' in out
    rec = json.loads(out.strip().splitlines()[-1])
    assert rec['out'] == str(tmp_path / 'x_pseudotheta.pt') and rec['frames'] == 23 and rec['rows_per_forward'] == [30]    # 9 = 6 + tail, 14 = 6 + 6 + tail
    got = joblib.load(rec['out'])
    assert isinstance(got, np.ndarray) and got.shape == (23, 85) and got.dtype == np.float32
    assert np.array_equal(got, P.pseudo_theta(model, db['features'], db['vid_name'], 6))
