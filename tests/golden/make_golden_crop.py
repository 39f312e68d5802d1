"""Generate tests/golden/crop_transform.npz by executing the REFERENCE's own functions.

Run only in the build container (needs the reference checkout; never on the GPU box -- the file is kept out of the GPU payload like the other two generators):

    python tests/golden/make_golden_crop.py [--out DIR]

`lib/data_utils/_img_utils.py` and `lib/utils/demo_utils.py` import cv2 (and more) at the top and cannot be imported here.  As
make_golden.py does for the scripts, this generator parses them with `ast`, takes the FunctionDef nodes it needs -- `rotate_2d`,
`gen_trans_from_patch_cv`, `trans_point2d`; `convert_crop_cam_to_orig_img`, `convert_crop_coords_to_orig_img` -- and compiles exactly those
into a namespace that holds numpy and a stand-in `cv2` whose only member is a float64 3-point affine solver (what `cv2.getAffineTransform`
computes).  Nothing of those functions is written out here, and the fixture holds arrays only.

There is no `warpAffine` vector and there cannot be one: OpenCV is absent.  The pixels are pinned to the mathematical definition instead
(tests/_crop_ref.py).
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
W, H, CROP, SCALE, SEED = 1920, 1080, 224, 1.2, 20260


def three_point_affine(src, dst):
    """The 2 x 3 map taking three points onto three points, solved in float64."""
    A = np.hstack([np.asarray(src, dtype=np.float64), np.ones((3, 1))])
    return np.linalg.solve(A, np.asarray(dst, dtype=np.float64)).T.copy()


def reference_functions(relpath, names, extra):
    tree = ast.parse(open(os.path.join(REF, relpath)).read(), relpath)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in nodes) == sorted(names), [n.name for n in nodes]
    ns = dict(extra, np=np)
    exec(compile(ast.Module(nodes, []), relpath, 'exec'), ns)
    return ns


def boxes(g):
    """Seeded (c_x, c_y, w, h) in a W x H frame: 40 anywhere with w != h, then boxes over each edge, a corner, outside, larger than the frame, 12 px wide,
    and w * scale = CROP exactly on an integer corner."""
    b = np.stack([g.uniform(100, W - 100, 40), g.uniform(100, H - 100, 40), g.uniform(40, 700, 40), g.uniform(40, 700, 40)], axis=1)
    b[:8, 3] = b[:8, 2]                                            # the tracker's square boxes
    b[8:14, 0] = g.uniform(1700, 1900, 6)                          # where an fp32 coordinate is coarse
    special = np.array([[30.25, 540.5, 300.0, 300.0], [1900.75, 500.1, 280.0, 350.0], [960.3, 12.7, 260.0, 260.0], [900.9, 1070.2, 310.0, 240.0],
                        [-20.5, -15.25, 200.0, 200.0], [2400.0, 1500.0, 150.0, 150.0], [960.0, 540.0, 2600.0, 2600.0], [1000.3, 400.6, 12.0, 12.0],
                        [512.0 + CROP / 2.0, 300.0 + CROP / 2.0, CROP / SCALE, CROP / SCALE]])
    return np.concatenate([b, special])


def main():
    out = HERE
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    cv2 = types.SimpleNamespace(getAffineTransform=three_point_affine)
    IU = reference_functions('lib/data_utils/_img_utils.py', ['rotate_2d', 'gen_trans_from_patch_cv', 'trans_point2d'], {'cv2': cv2})
    DU = reference_functions('lib/utils/demo_utils.py', ['convert_crop_cam_to_orig_img', 'convert_crop_coords_to_orig_img'], {})
    g = np.random.default_rng(SEED)
    bb = boxes(g)
    n = bb.shape[0]
    # the call of generate_patch_image_cv (_img_utils.py:96) with the arguments get_single_image_crop_demo passes (:231-242)
    M = np.stack([IU['gen_trans_from_patch_cv'](b[0], b[1], b[2], b[3], CROP, CROP, SCALE, 0, inv=False) for b in bb])
    assert M.shape == (n, 2, 3) and M.dtype == np.float64
    kp = np.stack([bb[:, :1] + g.uniform(-0.6, 0.6, (n, 21)) * bb[:, 2:3], bb[:, 1:2] + g.uniform(-0.6, 0.6, (n, 21)) * bb[:, 3:4]], axis=-1)
    kp_t = np.stack([[IU['trans_point2d'](kp[i, j], M[i]) for j in range(21)] for i in range(n)])
    assert kp_t.shape == (n, 21, 2) and kp_t.dtype == np.float64
    # predictions as the model emits them (float32), boxes as demo.py holds them at :320-331 (float64, columns 2.. already scaled)
    cam = np.stack([g.uniform(0.5, 1.4, n), g.uniform(-0.3, 0.3, n), g.uniform(-0.3, 0.3, n)], axis=1).astype(np.float32)
    j2d = g.uniform(-1.2, 1.2, (n, 49, 2)).astype(np.float32)
    box_s = bb.copy()
    box_s[:, 2:] *= SCALE
    orig_cam = DU['convert_crop_cam_to_orig_img'](cam=cam.copy(), bbox=box_s.copy(), img_width=W, img_height=H)
    j2d_img = DU['convert_crop_coords_to_orig_img'](bbox=box_s.copy(), keypoints=j2d.copy(), crop_size=CROP)
    # the same two calls on float32 boxes (a tracker may hand those over)
    orig_cam32 = DU['convert_crop_cam_to_orig_img'](cam=cam.copy(), bbox=box_s.astype(np.float32), img_width=W, img_height=H)
    j2d_img32 = DU['convert_crop_coords_to_orig_img'](bbox=box_s.astype(np.float32), keypoints=j2d.copy(), crop_size=CROP)
    print('M', M.shape, 'orig_cam', orig_cam.dtype, orig_cam.shape, 'joints2d_img_coord', j2d_img.dtype, j2d_img.shape, '| float32 boxes:', orig_cam32.dtype, j2d_img32.dtype)
    np.savez_compressed(os.path.join(out, 'crop_transform.npz'), meta=np.array([W, H, CROP, SEED], dtype=np.int64), scale=np.array(SCALE), bboxes=bb, M=M,
                        kp=kp, kp_t=kp_t, cam=cam, j2d=j2d, bboxes_scaled=box_s, orig_cam=orig_cam, joints2d_img_coord=j2d_img,
                        orig_cam_box32=orig_cam32, joints2d_img_coord_box32=j2d_img32)


if __name__ == '__main__':
    main()
