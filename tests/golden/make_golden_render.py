"""Generate tests/golden/render_order.npz by executing the REFERENCE's own `prepare_rendering_results`.

Run only in the build container (needs the reference checkout; never on the GPU box -- the file is kept out of the GPU payload like the other generators):

    python tests/golden/make_golden_render.py [--out DIR]

`lib/utils/demo_utils.py` imports cv2 (and more) at the top and cannot be imported here.  As make_golden_crop.py does, this generator parses it
with `ast`, takes the one FunctionDef node it needs and compiles exactly that into a namespace that holds numpy and OrderedDict.  Nothing of the
function is written out here, and the fixture holds arrays only: fabricated tracklets (ragged frame lists, cameras with ties in the y scale, which
decides the draw order) and, per frame, the person ids in the order the reference returned them with the rows it attached.

There is no rendered image in the fixture and there cannot be one: pyrender and OpenGL are absent.  The pixels are pinned to the definition instead
(tests/_render_ref.py).
"""
import os
import sys
from collections import OrderedDict

import numpy as np

from make_golden_crop import reference_functions      # the AST slicer, and where the reference checkout lies

HERE = os.path.dirname(os.path.abspath(__file__))
NFRAMES, SEED, NV = 9, 20261, 5


def tracklets(g):
    """Six persons over NFRAMES frames: ragged, overlapping frame lists (one not sorted by id, one frame without anybody), y scales from a
    set of four values so that most frames hold ties, float32 cameras for one person."""
    frames = {3: np.arange(0, 7), 11: np.arange(2, 9), 5: np.array([1, 2, 3, 6]), 8: np.arange(0, 9)[::2], 2: np.array([5, 6, 8]), 20: np.arange(1, 4)}
    frames = {p: f[f != 7] for p, f in frames.items()}                            # nobody in frame 7
    out = OrderedDict()
    for p, f in frames.items():
        n = f.shape[0]
        cam = np.stack([g.uniform(0.3, 1.2, n), g.choice([0.5, 0.75, 0.75000001, 1.25], n), g.uniform(-1, 1, n), g.uniform(-1, 1, n)], axis=1)
        out[p] = {'frame_ids': f, 'orig_cam': cam.astype(np.float32) if p == 8 else cam, 'verts': g.normal(size=(n, NV, 3)).astype(np.float32),
                  'bboxes': g.uniform(10, 300, (n, 4))}
    return out


def main():
    out = HERE
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    DU = reference_functions('lib/utils/demo_utils.py', ['prepare_rendering_results'], {'OrderedDict': OrderedDict})
    tr = tracklets(np.random.default_rng(SEED))
    res = DU['prepare_rendering_results'](tr, NFRAMES)
    assert len(res) == NFRAMES
    arrays = {'meta': np.array([NFRAMES, SEED, NV], dtype=np.int64), 'person_ids': np.array(list(tr.keys()), dtype=np.int64)}
    for p, d in tr.items():
        for k in ('frame_ids', 'orig_cam', 'verts', 'bboxes'):
            arrays['p%d_%s' % (p, k)] = np.asarray(d[k])
    counts = [len(fr) for fr in res]
    arrays['frame_offsets'] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    arrays['order'] = np.array([p for fr in res for p in fr.keys()], dtype=np.int64)
    arrays['order_cam'] = np.array([np.asarray(v['cam'], dtype=np.float64) for fr in res for v in fr.values()])
    arrays['order_verts'] = np.array([v['verts'] for fr in res for v in fr.values()])
    arrays['order_bbox'] = np.array([v['bbox'] for fr in res for v in fr.values()])
    ties = sum(len(set(float(v['cam'][1]) for v in fr.values())) < len(fr) for fr in res)
    print('frames', NFRAMES, 'persons per frame', counts, 'frames with a tie in sy:', ties)
    assert ties >= 2 and min(counts) == 0
    np.savez_compressed(os.path.join(out, 'render_order.npz'), **arrays)


if __name__ == '__main__':
    main()
