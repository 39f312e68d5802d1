"""Generate tests/golden/prepare.npz by executing the REFERENCE's own statements.

Run only in the build container (needs the reference checkout and scipy; never on the GPU box -- the file is kept out of the GPU payload like the other
generators):

    python tests/golden/make_golden_prepare.py --ref <reference checkout> [--out DIR]

Boxes: `lib/utils/smooth_bbox.py` is parsed with `ast`, its four FunctionDef nodes are compiled into a namespace that holds numpy, `scipy.signal` and
`scipy.ndimage.gaussian_filter1d` (the module's own import line names a scipy path that newer releases dropped), and run on fabricated keypoint
tracks.  Schedule: the statements of `lib/data_utils/pseudo_theta.py` lines 73-102 (the per-video chunk loop inside `main`) are compiled as they
stand and run with a stand-in `model` whose "theta" says where each row came from.  Nothing of either file is written out here, and the fixture
holds arrays only.
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = [os.environ.get('TEPOSE_REFERENCE', '')]          # the reference checkout: --ref DIR, or this variable
SEED, K = 20261, 14
THRESHOLDS = {'t03': 0.3, 't01': 0.1}
KERNEL, SIGMA = 11, 8                       # the builders' call: get_smooth_bbox_params(j2d, vis_thresh=VIS_THRESH, sigma=8)
CHUNK = 7
VIDEOS = [('b_walk', 5), ('a_run', 7), ('c_sit', 14), ('a_jump', 16), ('c_bend', 3), ('b_wave', 1)]


def reference_functions(relpath, names, extra):
    tree = ast.parse(open(os.path.join(REF[0], relpath)).read(), relpath)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in nodes) == sorted(names), [n.name for n in nodes]
    ns = dict(extra, np=np)
    exec(compile(ast.Module(nodes, []), relpath, 'exec'), ns)
    return ns


def reference_statements(relpath, function, lo, hi):
    """The statements of `function` that lie within lines lo .. hi, compiled as one module."""
    tree = ast.parse(open(os.path.join(REF[0], relpath)).read(), relpath)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == function][0].body
    nodes = [s for s in body if s.lineno >= lo and s.end_lineno <= hi]
    assert nodes and nodes[0].lineno == lo and nodes[-1].end_lineno == hi, [(s.lineno, s.end_lineno) for s in nodes]
    return compile(ast.Module(nodes, []), relpath, 'exec')


def track(g, n):
    """A person drifting and breathing through n frames: [n,K,3]; every frame has keypoints above 0.3, and a few between 0.1 and 0.3 that lie OUTSIDE the
    others' extent, so that the two thresholds give different boxes."""
    t = np.arange(n)[:, None]
    body = g.uniform(-1, 1, (1, K, 2)) * np.array([40.0, 90.0])
    centre = np.stack([300 + 3.1 * t + 25 * np.sin(t / 5.0), 200 + 1.3 * t + 10 * np.cos(t / 3.0)], axis=-1)
    size = 1.0 + 0.3 * np.sin(t / 7.0)[..., None]
    xy = centre + body * size + g.normal(0, 1.5, (n, K, 2))
    conf = g.uniform(0.35, 1.0, (n, K))
    conf[:, :2] = g.uniform(0.12, 0.28, (n, 2))
    xy[:, :2] += np.array([70.0, -120.0])
    return np.concatenate([xy, conf[..., None]], axis=-1)


def box_cases(g):
    """name -> (kps [n,K,3], none [n] bool: the frames handed over as None)."""
    cases = {}
    cases['all_visible_40'] = (track(g, 40), np.zeros(40, bool))
    kp = track(g, 45)
    for f in (0, 1, 9, 20, 21, 22, 23, 24, 42, 43, 44):           # leading 2, interior 1 and 5, trailing 3
        kp[f, :, 2] = 0.05
    cases['gaps_45'] = (kp, np.zeros(45, bool))
    kp = track(g, 30)
    kp[12, :, 2] = 0.05                                             # two visible keypoints 0.2 px apart: a person below 0.5 px
    kp[12, 4] = [310.0, 220.0, 0.9]
    kp[12, 5] = [310.1, 220.17, 0.9]
    cases['tiny_person_30'] = (kp, np.zeros(30, bool))
    none = np.zeros(36, bool)
    none[[0, 7, 8, 15, 35]] = True
    cases['none_entries_36'] = (track(g, 36), none)
    cases['short_7'] = (track(g, 7), np.zeros(7, bool))
    cases['exactly_33'] = (track(g, 33), np.zeros(33, bool))
    return cases


def stand_in_model(torch):
    def model(batch):
        assert batch.dim() == 3 and batch.shape[0] == 1
        T = batch.shape[1]
        theta = torch.stack([batch[0, :, 0], batch[0, 0, 0].expand(T), torch.full((T,), float(T))], dim=1)
        return [{'theta': theta[None]}]
    return model


def main():
    import scipy.ndimage
    import scipy.signal
    import torch
    out = HERE
    if '--ref' in sys.argv:
        REF[0] = sys.argv[sys.argv.index('--ref') + 1]
    if not os.path.isdir(os.path.join(REF[0], 'lib')):
        raise SystemExit('give the reference checkout with --ref DIR (or TEPOSE_REFERENCE)')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    SB = reference_functions('lib/utils/smooth_bbox.py', ['get_smooth_bbox_params', 'kp_to_bbox_param', 'get_all_bbox_params', 'smooth_bbox_params'],
                             {'signal': scipy.signal, 'gaussian_filter1d': scipy.ndimage.gaussian_filter1d})
    g = np.random.default_rng(SEED)
    rec = {'meta': np.array([SEED, K, KERNEL, SIGMA, CHUNK], dtype=np.int64)}
    names = []
    for name, (kp, none) in box_cases(g).items():
        names.append(name)
        rec['box_%s_kps' % name], rec['box_%s_none' % name] = kp, none
        as_list = [None if none[i] else kp[i] for i in range(len(kp))]
        for tag, thr in THRESHOLDS.items():
            raw, start, end = SB['get_all_bbox_params'](as_list, thr)
            smoothed, s2, e2 = SB['get_smooth_bbox_params'](as_list, vis_thresh=thr, kernel_size=KERNEL, sigma=SIGMA)
            assert (s2, e2) == (start, end) and raw.dtype == smoothed.dtype == np.float64 and raw.shape == (end - start, 3)
            assert smoothed.shape == (end, 3) and not smoothed[:start].any()
            rec['box_%s_%s_raw' % (name, tag)], rec['box_%s_%s_smoothed' % (name, tag)] = raw, smoothed
            rec['box_%s_%s_span' % (name, tag)] = np.array([start, end], dtype=np.int64)
            print(name, tag, 'frames', len(kp), 'start', start, 'end', end)
        assert not np.array_equal(rec['box_%s_t03_raw' % name], rec['box_%s_t01_raw' % name])      # the threshold matters in every case
    rec['box_cases'] = np.array(names)
    # the chunk loop, with feature column 0 = the row number
    vid_name = np.concatenate([np.array([v] * n) for v, n in VIDEOS])
    N = vid_name.shape[0]
    feats = np.zeros((N, 4), dtype=np.float32)
    feats[:, 0] = np.arange(N)
    ns = {'np': np, 'torch': torch, 'db': {'vid_name': vid_name, 'features': feats}, 'tqdm': lambda it: it, 'device': torch.device('cpu'),
          'args': types.SimpleNamespace(vibe_batch_size=CHUNK), 'model': stand_in_model(torch)}
    exec(reference_statements('lib/data_utils/pseudo_theta.py', 'main', 73, 102), ns)
    coded = ns['thetas']
    assert coded.shape == (N, 3), coded.shape
    rec['sched_vid_name'], rec['sched_coded'] = vid_name, coded.astype(np.int64)
    assert np.array_equal(rec['sched_coded'], coded)
    print('schedule: rows', N, 'chunks', len({(int(a), int(b)) for _, a, b in rec['sched_coded']}))
    np.savez_compressed(os.path.join(out, 'prepare.npz'), **rec)


if __name__ == '__main__':
    main()
