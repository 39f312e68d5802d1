"""The cases of the overlay renderer's GPU test (tests/test_gpu_render.py), shared with the CPU test that emulates the kernel's fp32 fragment stage on
them (tests/test_render_host.py): small odd images, 97 x 131, so that a row's W * 3 bytes are not dword-aligned.  Depth is d = z of the input mesh
(the flip and the camera's -1 cancel), so every mesh that is to be seen keeps |z| < 1.  Each case is a dict of the arguments of
`Renderer.render_frames` / `_render_ref.render`: frames, idx, verts [n,V,3], faces, cams [n,4], colors [n,3], rot [n,3,3] or None."""
import numpy as np

import _render_ref as R

H, W = 97, 131
ASPECT = W / H


def noise(seed, F, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, (F, h, w, 3), dtype=np.uint8)


def cam(s, tx=0.0, ty=0.0, h=H, w=W):
    """Isotropic in pixels: s NDC units per mesh unit across the width."""
    return [s, s * w / h, tx, ty]


def _one(verts, faces, c, color=(1.0, 1.0, 0.9), rot=None, frames=None):
    return {'frames': noise(7, 1) if frames is None else frames, 'idx': np.array([0]), 'verts': verts[None], 'faces': faces, 'cams': np.array([c], dtype=np.float64),
            'colors': np.array([color], dtype=np.float32), 'rot': None if rot is None else np.asarray(rot)[None]}


def two_spheres():
    (a, f), (b, _) = R.uv_sphere(20, 14, 0.6, (-0.25, 0, 0)), R.uv_sphere(20, 14, 0.6, (0.25, 0.1, 0.2))
    return np.concatenate([a, b]), np.concatenate([f, f + a.shape[0]])


def front_half_reversed():
    """The camera's half of a sphere with every face turned over: back faces only."""
    v, f = R.uv_sphere(24, 16, 0.9)
    near = (v[f][:, :, 2] < -0.05).all(axis=1)                 # d = z: the near half
    return v, f[near][:, ::-1].copy()


def degenerate():
    """A sphere plus faces of zero area in front of it: two with a repeated vertex, one with three different vertices on one pixel column."""
    v, f = R.uv_sphere(24, 16, 0.8)
    extra = np.array([[0.125, 0.0, -0.95], [0.125, 0.25, -0.95], [0.125, 0.5, -0.95]], dtype=np.float32)
    n = v.shape[0]
    return np.concatenate([v, extra]), np.concatenate([f, np.array([[5, 5, 9], [3, 7, 3], [n, n + 1, n + 2], [n + 2, n + 1, n]], dtype=np.int32)])


def clip_mesh():
    """One sphere whose near cap lies before d = -1, one whose far side lies behind d = 1 with its front cap still inside."""
    (a, f), (b, _) = R.uv_sphere(24, 16, 1.3, (-0.5, 0, -0.4)), R.uv_sphere(24, 16, 0.5, (1.1, 0.2, 1.2))
    return np.concatenate([a, b]), np.concatenate([f, f + a.shape[0]])


def three_instances():
    """Three spheres on one frame, overlapping, drawn from the nearest to the farthest: the farthest is drawn last and must hide the others."""
    v, f = R.uv_sphere(24, 16, 0.5)
    verts = np.stack([v + np.array(o, dtype=np.float32) for o in ([-0.3, 0.0, -0.4], [0.0, 0.1, 0.0], [0.3, -0.1, 0.4])])
    return {'frames': noise(8, 1), 'idx': np.array([0, 0, 0]), 'verts': verts, 'faces': f, 'cams': np.array([cam(0.6)] * 3), 'rot': None,
            'colors': np.array([[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 1.0]], dtype=np.float32)}


def two_frames():
    """Frame indices repeated and not monotonic: 1, 0, 1, 1."""
    v, f = R.torus(40, 20)
    verts = np.stack([v * np.float32(s) for s in (1.0, 0.8, 0.6, 0.4)])
    cams = np.array([cam(0.6, 0.2, 0.1), cam(0.7, -0.3, 0.0), cam(0.9, 0.5, -0.3), cam(0.8, -0.6, 0.4)])
    cols = np.array([[1.0, 1.0, 0.9], [0.9, 0.6, 0.5], [0.5, 0.7, 1.0], [0.2, 0.3, 0.1]], dtype=np.float32)
    return {'frames': noise(9, 2), 'idx': np.array([1, 0, 1, 1]), 'verts': verts, 'faces': f, 'cams': cams, 'colors': cols, 'rot': None}


def full_hd():
    """One 1080p frame, one blob about 500 px tall hanging over the right edge: snapped coordinates near x = 1900, where fp32 pixel coordinates are coarse."""
    v, f = R.blob(3)
    s = 500.0 / (1.9 * 1920 / 2)
    return _one(v, f, cam(s, 0.975 / s, 0.3, 1080, 1920), frames=noise(10, 1, 1080, 1920))


CASES = {
    'sphere_24x16': lambda: _one(*R.uv_sphere(24, 16, 0.9), cam(0.6, 0.1, -0.05)),
    'torus_40x20': lambda: _one(*R.torus(40, 20), cam(0.8, -0.1, 0.1), color=(0.6, 0.9, 1.0)),
    'two_spheres': lambda: _one(*two_spheres(), cam(0.7)),
    'blob_6890': lambda: _one(*R.blob(1), cam(0.75, 0.05, 0.02)),
    'overflow': lambda: _one(*R.uv_sphere(24, 16, 0.9), cam(2.2, 0.1, 0.05)),
    'edge_left': lambda: _one(*R.uv_sphere(24, 16, 0.9), cam(0.6, -1.6, 0.0)),
    'edge_right': lambda: _one(*R.uv_sphere(24, 16, 0.9), cam(0.6, 1.7, 0.1)),
    'edge_top': lambda: _one(*R.torus(40, 20), cam(0.6, 0.1, -1.1)),
    'edge_bottom': lambda: _one(*R.torus(40, 20), cam(0.6, -0.2, 1.2)),
    'corner': lambda: _one(*R.blob(2), cam(0.9, -1.05, -0.85)),
    'outside': lambda: _one(*R.uv_sphere(24, 16, 0.9), cam(0.6, 5.0, -4.0)),
    'back_facing': lambda: _one(*front_half_reversed(), cam(0.6)),
    'degenerate': lambda: _one(*degenerate(), cam(0.6)),
    'clip': lambda: _one(*clip_mesh(), cam(0.45)),
    'three_instances': three_instances,
    'side_view': lambda: _one(*R.blob(1), cam(0.75, 0.05, 0.02), rot=R.rotation(270, [0, 1, 0])),
    'two_frames': two_frames,
    'full_hd': full_hd,
}
