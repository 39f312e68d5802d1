"""CPU: the host side of the overlay renderer -- the oracle of the GPU test (tests/_render_ref.py) against its second formulation and on the fill
rule's own ground; `prepare_rendering_results` against what the reference's function returned (tests/golden/render_order.npz, written by
tests/golden/make_golden_render.py from an AST slice of lib/utils/demo_utils.py); the argument checks of the two C entries and the exceptions of
tepose_amd.render / tepose_amd.demo.render_tracklets, which need no device."""
import os

import numpy as np
import pytest
import torch

import _render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'render_order.npz'))
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
H, W = 37, 53
CAM = (0.6, 0.6 * W / H, 0.07, -0.04)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from tepose_amd import _lib
    return _lib.load()


def _pairs(frag):
    pix, face, depth, b = frag
    order = np.lexsort((face, pix))
    return pix[order], face[order], depth[order], b[order]


def _two_spheres():
    """Interpenetrating: the intersection curve runs through faces of both."""
    (a, f), (b, _) = R.uv_sphere(10, 7, 0.6, (-0.25, 0, 0)), R.uv_sphere(10, 7, 0.6, (0.25, 0.1, 0.2))
    return np.concatenate([a, b]), np.concatenate([f, f + a.shape[0]])


MESHES = {
    'sphere': lambda: R.uv_sphere(12, 8, 0.9) + (CAM,),
    'torus': lambda: R.torus(14, 8) + (CAM,),
    'two_spheres': lambda: _two_spheres() + (CAM,),
    'overflow': lambda: R.uv_sphere(12, 8, 0.9) + ((2.2, 2.2 * W / H, 0.1, 0.05),),
    'clipped': lambda: R.uv_sphere(12, 8, 1.3, (0, 0, -0.4)) + (CAM,),     # d = -zr: the near cap lies before d = -1
}


@pytest.mark.parametrize('name', sorted(MESHES))
def test_the_oracle_agrees_with_its_second_formulation(name):
    """Bounding boxes and three edge functions against exact rational barycentrics over all pixels: the same (pixel, face) pairs, the same
    barycentrics and depths to fp64 rounding."""
    verts, faces, cam = MESHES[name]()
    ix, iy, d, valid, _ = R.vertex_stage(verts, cam, None, H, W)
    a = _pairs(R.fragments(ix, iy, d, valid, faces, H, W))
    b = _pairs(R.fragments_rational(ix, iy, d, valid, faces, H, W))
    assert a[0].size > 150, a[0].size
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.abs(a[2] - b[2]).max() <= 1e-12 and np.abs(a[3] - b[3]).max() <= 1e-12
    assert (a[2] >= -1).all() and (a[2] < 1).all()
    one = R.render_instance(verts, faces, cam, None, (1.0, 1.0, 0.9), H, W)
    two = R.render_instance(verts, faces, cam, None, (1.0, 1.0, 0.9), H, W, formulation=R.fragments_rational)
    assert np.array_equal(one['face'], two['face']) and np.array_equal(one['count'], two['count'])
    assert np.abs(one['value'] - two['value']).max() <= 1e-9
    covered = one['face'] >= 0
    if name in ('sphere', 'torus'):                       # closed, convex silhouette per scanline or not: a front fragment and nothing else in front of it
        assert one['count'].max() <= 2 and covered.sum() > 300
    if name == 'clipped':                                 # the near cap is cut away: the pixels there show the inside of nothing (back faces are culled)
        assert not covered[H // 2, W // 2] and covered.sum() > 100
    assert one['value'][covered].min() >= 255 * 0.1 and one['value'][covered].max() <= 255.0


def _grid(nx, ny, x0, y0, step_px, H, W, flip=False):
    """A flat grid of nx x ny cells whose vertex (i, j) lands exactly at pixel coordinate (x0 + i step, y0 + j step) of an H x W image under the
    identity camera: two triangles per cell, front-facing (or all back-facing with flip)."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing='ij')
    px, py = x0 + step_px * i, y0 + step_px * j
    v = np.stack([px * 2.0 / W - 1.0, -(1.0 - py * 2.0 / H), np.zeros_like(px, dtype=np.float64)], axis=-1).reshape(-1, 3)      # y is flipped by the vertex stage
    idx = lambda a, b: a * (ny + 1) + b
    faces = []
    for a in range(nx):
        for b in range(ny):
            faces += [[idx(a, b), idx(a, b + 1), idx(a + 1, b)], [idx(a + 1, b), idx(a, b + 1), idx(a + 1, b + 1)]]
    faces = np.asarray(faces, dtype=np.int32)
    return v.astype(np.float32), faces[:, ::-1].copy() if flip else faces


@pytest.mark.parametrize('x0,y0,step', [(4.5, 3.5, 4.0), (4.0, 3.0, 4.0), (4.5, 3.0, 2.5), (2.5, 1.5, 1.0), (3.0, 2.0, 0.5)])
def test_fill_rule_every_centre_inside_the_outline_is_owned_exactly_once(x0, y0, step):
    """Vertices exactly on pixel centres (x.5) and on pixel corners (x.0), H = W = 32 so that the coordinates are exact in fp32: shared edges and
    shared vertices run through centres.  Each centre inside the outline -- left and top border included, right and bottom excluded -- belongs to
    exactly one triangle, in both formulations; the mirrored (back-facing) grid draws nothing."""
    H = W = 32
    nx, ny = 5, 4
    verts, faces = _grid(nx, ny, x0, y0, step, H, W)
    ix, iy, d, valid, _ = R.vertex_stage(verts, (1.0, 1.0, 0.0, 0.0), None, H, W)
    want_x = ((x0 + step * np.arange(nx + 1)) * 256).astype(np.int64)
    assert np.array_equal(ix.reshape(nx + 1, ny + 1)[:, 0], want_x)                    # the snap reproduces the construction exactly
    cx, cy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    inside = (cx >= x0) & (cx < x0 + nx * step) & (cy >= y0) & (cy < y0 + ny * step)
    for form in (R.fragments, R.fragments_rational):
        pix, face, depth, b = form(ix, iy, d, valid, faces, H, W)
        count = np.bincount(pix, minlength=H * W).reshape(H, W)
        assert np.array_equal(count, inside.astype(np.int64)), (form.__name__, np.argwhere(count != inside)[:5].tolist())
    back = _grid(nx, ny, x0, y0, step, H, W, flip=True)[1]
    assert R.fragments(ix, iy, d, valid, back, H, W)[0].size == 0


def test_vertex_stage_limits_and_bad_faces():
    verts, faces = R.uv_sphere(8, 6, 0.5)
    v = verts.copy()
    v[3] = [np.nan, 0, 0]
    v[5] = [np.inf, 0, 0]
    v[7] = [3e6, 0, 0]                                                              # 3e6 * W / 2 px: beyond 2^20
    ix, iy, d, valid, _ = R.vertex_stage(v, CAM, None, H, W)
    assert not valid[[3, 5, 7]].any() and valid.sum() == v.shape[0] - 3
    f = faces.copy()
    f[0, 1], f[1, 0] = v.shape[0], -1
    pix, face, _, _ = R.fragments(ix, iy, d, valid, f, H, W)
    assert 0 not in face and 1 not in face
    touched = np.unique(f[np.isin(f, [3, 5, 7]).any(axis=1)].reshape(-1))
    assert not np.isin(face, np.nonzero(np.isin(f, [3, 5, 7]).any(axis=1))[0]).any() and touched.size
    off, lst = R.adjacency(f, v.shape[0])
    assert off[-1] == lst.size == 3 * (f.shape[0] - 2) and 0 not in lst and 1 not in lst
    for k in (0, 9, v.shape[0] - 1):
        mine = lst[off[k]:off[k + 1]]
        assert np.array_equal(mine, np.sort(mine)) and all(k in f[j] for j in mine)
    from tepose_amd.render import vertex_face_adjacency, rotation_matrix
    o2, l2 = vertex_face_adjacency(faces, v.shape[0] + 4)                            # more vertices than the faces use: empty tails
    o1, l1 = R.adjacency(faces, v.shape[0] + 4)
    assert np.array_equal(o1, o2) and np.array_equal(l1, l2) and o2.shape[0] == v.shape[0] + 5
    assert np.abs(rotation_matrix(270, [0, 1, 0]) - np.array([[0, 0, -1.0], [0, 1, 0], [1, 0, 0]])).max() < 1e-15
    assert np.abs(rotation_matrix(33.0, [1, 2, 3]) - R.rotation(33.0, [1, 2, 3])).max() < 1e-15


def _fixture_results():
    return {int(p): {k: G['p%d_%s' % (p, k)] for k in ('frame_ids', 'orig_cam', 'verts', 'bboxes')} for p in G['person_ids']}


def test_prepare_rendering_results_reproduces_the_reference_order():
    from tepose_amd.demo import prepare_rendering_results
    nframes = int(G['meta'][0])
    res = _fixture_results()
    keep = {p: {k: v.copy() for k, v in d.items()} for p, d in res.items()}
    got = prepare_rendering_results(res, nframes)
    assert len(got) == nframes
    off = G['frame_offsets']
    ties = 0
    for f in range(nframes):
        want = G['order'][off[f]:off[f + 1]].tolist()
        assert list(got[f].keys()) == want, (f, list(got[f].keys()), want)
        for k, (p, row) in enumerate(got[f].items()):
            assert sorted(row.keys()) == ['bbox', 'cam', 'verts']
            assert np.array_equal(np.asarray(row['cam'], dtype=np.float64), G['order_cam'][off[f] + k])
            assert np.array_equal(row['verts'], G['order_verts'][off[f] + k]) and np.array_equal(row['bbox'], G['order_bbox'][off[f] + k])
        sy = [float(r['cam'][1]) for r in got[f].values()]
        assert sy == sorted(sy)                                                     # the largest camera scale is drawn last
        ties += len(set(sy)) < len(sy)
    assert ties >= 2 and any(len(fr) == 0 for fr in got)                            # the fixture sees ties and an empty frame
    for p in res:
        for k in res[p]:
            assert np.array_equal(res[p][k], keep[p][k])                            # the input is left alone


def test_every_argument_error_of_the_entry_points_without_a_device(lib):
    P = 4096                                                       # a non-null, 8-byte aligned pointer value: never dereferenced, every call returns before a device call
    f = lib.tepose_render_meshes_u8
    ok = dict(frames=P, F=2, H=8, W=8, idx=P, verts=P, n=3, V=10, faces=P, Fc=12, off=P, lst=P, n_adj=36, cams=P, rot=P, colors=P, out=P, winner=None,
              depth=None, ws=P, ws_bytes=1 << 30)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['frames'], a['F'], a['H'], a['W'], a['idx'], a['verts'], a['n'], a['V'], a['faces'], a['Fc'], a['off'], a['lst'], a['n_adj'], a['cams'],
                 a['rot'], a['colors'], a['out'], a['winner'], a['depth'], a['ws'], a['ws_bytes'], None)
    assert call(F=0) == E_ARG and call(H=0) == E_ARG and call(W=-1) == E_ARG and call(V=0) == E_ARG
    assert call(n=-1) == E_ARG and call(Fc=-1) == E_ARG and call(n_adj=-1) == E_ARG
    for k in ('frames', 'out', 'idx', 'verts', 'faces', 'off', 'lst', 'cams', 'colors', 'ws'):
        assert call(**{k: None}) == E_ARG, k
    assert call(ws=P + 4) == E_ARG                                 # misaligned workspace
    assert call(n=0, ws=None, winner=P) == E_ARG and call(n=0, ws=None, depth=P) == E_ARG
    assert call(H=16385) == E_SHAPE and call(W=16385) == E_SHAPE and call(n=4097) == E_SHAPE and call(Fc=(1 << 20) + 1) == E_SHAPE and call(V=(1 << 20) + 1) == E_SHAPE
    need = lib.tepose_render_workspace_bytes(8, 8, 2, 3, 10, 12)
    assert need >= 2 * 8 * 8 * 8 + 3 * 10 * 24 and need % 256 == 0
    assert call(ws_bytes=need - 1) == E_WORKSPACE
    assert call(H=0, ws_bytes=0) == E_ARG and call(n=4097, ws_bytes=0) == E_SHAPE            # the order: ARG, SHAPE, WORKSPACE
    w = lib.tepose_render_workspace_bytes
    assert w(0, 8, 1, 1, 10, 12) == 0 and w(8, 8, 0, 1, 10, 12) == 0 and w(8, 8, 1, -1, 10, 12) == 0 and w(8, 8, 1, 4097, 10, 12) == 0
    assert w(16384, 16384, 1, 0, 1, 0) == 8 * 16384 * 16384        # the limits themselves fit; no 32-bit overflow in the size
    assert w(1080, 1920, 1, 0, 6890, 13776) == 1080 * 1920 * 8     # "a 1080p key plane is 16.6 MB per frame"
    assert w(1080, 1920, 4, 64, 6890, 16384) > 0                   # 64 instances, 16 384 faces fit the key


def test_renderer_argument_errors():
    from tepose_amd.render import Renderer
    verts, faces = R.uv_sphere(8, 6)
    with pytest.raises(NotImplementedError):
        Renderer(faces, wireframe=True)
    with pytest.raises(ValueError, match='negative'):
        Renderer(np.array([[0, 1, -2]]))
    with pytest.raises(ValueError):
        Renderer(faces.astype(np.float32))
    with pytest.raises(ValueError):
        Renderer(faces.reshape(-1))
    r = Renderer(faces)
    n = 2
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    vv, cams, cols = np.stack([verts, verts]), np.tile([1.0, 1.0, 0.0, 0.0], (n, 1)), np.ones((n, 3), dtype=np.float32)
    with pytest.raises(RuntimeError, match='MI355X only'):
        r.render_frames(frames, [0, 1], vv, cams, cols)
    with pytest.raises(RuntimeError, match='MI355X only'):
        r.render(frames[0], verts, cams[0])
    with pytest.raises(ValueError):
        r.render_frames(frames.float(), [0, 1], vv, cams, cols)
    with pytest.raises(ValueError):
        r.render_frames(frames[0], [0, 1], vv, cams, cols)
    with pytest.raises(ValueError):
        r.render(frames, verts, cams[0])                           # render takes one image
    with pytest.raises(IndexError):
        r.render_frames(frames, [0, 2], vv, cams, cols)
    with pytest.raises(IndexError):
        r.render_frames(frames, [-1, 0], vv, cams, cols)
    with pytest.raises(ValueError):
        r.render_frames(frames, [0, 1], vv[:1], cams, cols)        # one mesh per index
    with pytest.raises(ValueError):
        r.render_frames(frames, [0, 1], vv, cams[:, :3], cols)
    with pytest.raises(ValueError):
        r.render_frames(frames, [0, 1], vv, cams, cols[:1])
    with pytest.raises(ValueError):
        r.render_frames(frames, [0, 1], vv, cams, cols, rot=np.zeros((n, 9)))
    with pytest.raises(ValueError, match='index'):
        r.render_frames(frames, [0, 1], vv[:, :-1], cams, cols)    # the faces index a vertex the meshes do not have: the bad index of a face
    with pytest.raises(ValueError):
        r.render_frames(frames, [0, 1], vv.astype(np.int64), cams, cols)
    with pytest.raises(ValueError):
        r.render_frames(frames, [0, 1], vv, cams, cols, out=torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError, match='made for'):
        Renderer(faces, resolution=(16, 8)).render_frames(frames, [0, 1], vv, cams, cols)


def test_render_tracklets_rejects_a_cpu_tensor_and_colours_repeat():
    from tepose_amd.demo import default_mesh_colors, render_tracklets
    _, faces = R.uv_sphere(8, 6)
    with pytest.raises(RuntimeError, match='MI355X only'):
        render_tracklets(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), {}, faces)
    with pytest.raises(ValueError):
        render_tracklets(torch.zeros(2, 8, 8, 3), {}, faces)
    a, b = default_mesh_colors([4, 9, 1]), default_mesh_colors([4, 9, 1])
    assert a == b and list(a) == [4, 9, 1] and len({a[4], a[9], a[1]}) == 3
    assert all(max(c) == 1.0 and abs(min(c) - 0.5) < 1e-12 for c in a.values())     # saturation 0.5, value 1


from test_crop_host import REF      # where the reference checkout lies on the build box
GEN = os.path.join(ROOT, 'tests', 'golden', 'make_golden_render.py')
needs_reference = pytest.mark.skipif(not (os.path.isfile(os.path.join(REF, 'lib', 'utils', 'demo_utils.py')) and os.path.isfile(GEN)),
                                     reason='reference checkout or generator absent')


@needs_reference
def test_fixture_regenerates_bit_identically_and_the_generator_holds_no_reference_text(tmp_path):
    """As tests/test_crop_host.py does for make_golden_crop.py: the generator executes the reference's function, it does not retype it, and running it
    again gives the committed arrays."""
    import re
    import subprocess
    import sys

    def code_lines(path):
        return [l for l in (re.sub(r'\s+', '', l.split('#')[0]) for l in open(path)) if l]
    g = code_lines(GEN)
    r = code_lines(os.path.join(REF, 'lib/utils/demo_utils.py'))
    runs = {tuple(r[i:i + 3]) for i in range(len(r) - 2)}
    assert not [g[i] for i in range(len(g) - 2) if tuple(g[i:i + 3]) in runs]
    p = subprocess.run([sys.executable, GEN, '--out', str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    a = np.load(os.path.join(str(tmp_path), 'render_order.npz'))
    assert sorted(a.files) == sorted(G.files)
    for k in a.files:
        assert a[k].dtype == G[k].dtype and np.array_equal(a[k], G[k]), k


def test_fp32_emulation_of_the_fragment_stage_stays_inside_the_windows_of_the_gpu_test():
    """The windows of tests/test_gpu_render.py -- 1e-3 grey levels around a half-integer, 1e-5 in depth -- must hold an fp32 fragment stage: barycentrics from the exact
    integer edge values rounded to fp32, the kernel's order of sums, fp32 normals.  Emulated on the GPU test's own cases; measured: 4.7e-5 grey levels, 1.6e-7 in depth."""
    import _render_cases as C
    worst_value = worst_depth = 0.0
    for name, make in C.CASES.items():
        c = make()
        F, H, W = c['frames'].shape[:3]
        for i in range(c['idx'].shape[0]):
            rot = None if c['rot'] is None else c['rot'][i]
            one = R.render_instance(c['verts'][i], c['faces'], c['cams'][i], rot, c['colors'][i], H, W)
            depth, value = R.fragment_stage_fp32(c['verts'][i], c['faces'], c['cams'][i], rot, c['colors'][i], H, W)
            m = one['face'] >= 0
            if m.any():
                worst_value = max(worst_value, float(np.abs(value[m] - one['value'][m]).max()))
                worst_depth = max(worst_depth, float(np.abs(depth[m] - one['depth'][m]).max()))
    print('fp32 fragment stage against fp64 over %d cases: colour within %.3g grey levels, depth within %.3g' % (len(C.CASES), worst_value, worst_depth))
    assert 0 < worst_value <= 1e-3 / 4 and 0 < worst_depth <= 1e-5 / 4                 # a quarter of each window: room for the device's own operation order
