"""The oracle of the overlay rasteriser (csrc/render.hip): the definition, in numpy.

  vertex stage, fp64, every product and sum rounded on its own: flip (x, -y, -z); rotate, xr = (R0 x + R1 y') + R2 z'; X = sx (xr + tx),
  Y = sy (yr - ty), d = -zr; px = (X + 1) (W / 2), py = (1 - Y) (H / 2); snap ix = floor(256 px + 1/2), iy alike; d is rounded to fp32 once
  (the kernel stores it so); a vertex that is not finite or beyond +-2^20 px is invalid.
  triangle stage, exact integers: A = (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0) < 0 is kept; three valid vertices, three indices in [0, V).
  coverage: the three edge functions at the pixel centre (256 c + 128, 256 r + 128) have the inside sign, a zero counting on an edge with
  dy > 0, or dy == 0 and dx < 0, walking v0 -> v1 -> v2.
  depth: b_i = -E_i / -A, d = sum b_i d_i, kept for -1 <= d < 1; smallest d, then smallest face index; instances composite in the order given.
  shading: vertex normals = normalised sum of the un-normalised face cross products after flip and R; n = sum b_i n_i normalised;
  lambda = max(0, n_z); colour = clamp(base (0.3 + (2.4 / pi) lambda) + 0.1, 0, 1); out = floor(255 colour + 1/2).

It is a restatement of what lib/utils/renderer.py sets up, not pyrender: no OpenGL output exists here.  Everything after the snap is integer
arithmetic (exact) or fp64.  Two structurally different formulations of coverage are kept so that the oracle is checked against itself
(tests/test_render_host.py): `fragments` walks clamped bounding boxes with three edge functions; `fragments_rational` solves every pixel
centre against every triangle for exact rational barycentrics in the (v1 - v0, v2 - v0) basis and classifies the edge on a zero."""
import numpy as np

LIMIT_PX = float(1 << 20)
LIGHT = 2.4 / np.pi


def rotation(angle_deg, axis):
    """Rodrigues' matrix in fp64: what trimesh.transformations.rotation_matrix(radians(angle), axis)[:3, :3] is."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.sqrt((a * a).sum())
    t = np.radians(float(angle_deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.cos(t) * np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * np.outer(a, a)


def place(verts, R=None):
    """[V,3] fp32 -> flipped and rotated positions [V,3] fp64."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    a, b, c = v[:, 0], -v[:, 1], -v[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([(R[k, 0] * a + R[k, 1] * b) + R[k, 2] * c for k in range(3)], axis=1)


def vertex_stage(verts, cam, R, H, W):
    """-> ix, iy int64 [V], d fp64 [V] (fp32 values), valid bool [V], P [V,3] fp64."""
    P = place(verts, R)
    sx, sy, tx, ty = (float(c) for c in cam)
    with np.errstate(invalid='ignore', over='ignore'):
        X, Y, d = sx * (P[:, 0] + tx), sy * (P[:, 1] - ty), -P[:, 2]
        px, py = (X + 1.0) * (0.5 * W), (1.0 - Y) * (0.5 * H)
        valid = (px >= -LIMIT_PX) & (px <= LIMIT_PX) & (py >= -LIMIT_PX) & (py <= LIMIT_PX) & (d >= -3.0e38) & (d <= 3.0e38)
        ix = np.where(valid, np.floor(256.0 * np.where(valid, px, 0.0) + 0.5), 0).astype(np.int64)
        iy = np.where(valid, np.floor(256.0 * np.where(valid, py, 0.0) + 0.5), 0).astype(np.int64)
        d = np.where(valid, d, 0.0).astype(np.float32).astype(np.float64)
    return ix, iy, d, valid, P


def usable_faces(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def vertex_normals(P, faces):
    """Normalised sum of the un-normalised cross products of the incident faces; a zero sum stays zero.  Faces with an index outside [0, V) do not count."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[usable_faces(f, P.shape[0])]
    with np.errstate(invalid='ignore', over='ignore'):
        c = np.cross(P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]])
        n = np.zeros_like(P)
        for k in range(3):
            np.add.at(n, f[:, k], c)
        length = np.sqrt((n * n).sum(axis=1, keepdims=True))
        return np.where(length > 0, n / np.where(length > 0, length, 1.0), n)


def owns(dx, dy):
    return (dy > 0) | ((dy == 0) & (dx < 0))


def front_faces(ix, iy, valid, faces):
    """-> indices of the faces that draw, and their signed doubled areas A < 0."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = usable_faces(f, ix.shape[0])
    g = np.where(ok[:, None], f, 0)
    ok &= valid[g].all(axis=1)
    x, y = ix[g], iy[g]
    A = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    keep = np.nonzero(ok & (A < 0))[0]
    return keep, A[keep]


def fragments(ix, iy, d, valid, faces, H, W, clip=True):
    """Every (pixel, face) pair that passes coverage and (with `clip`) the depth clip: -> pixel [m] (r W + c), face [m], depth [m], b [m,3], in no order."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keep, A = front_faces(ix, iy, valid, f)
    x, y, dv = ix[f[keep]], iy[f[keep]], d[f[keep]]
    c0 = np.maximum((x.min(axis=1) + 127) >> 8, 0)
    c1 = np.minimum((x.max(axis=1) - 128) >> 8, W - 1)
    r0 = np.maximum((y.min(axis=1) + 127) >> 8, 0)
    r1 = np.minimum((y.max(axis=1) - 128) >> 8, H - 1)
    some = (c0 <= c1) & (r0 <= r1)
    side = np.where(some, np.maximum(c1 - c0, r1 - r0) + 1, 0)
    out = []
    k = 1
    while True:
        sel_all = np.nonzero((side > k // 2 if k > 1 else side > 0) & (side <= k))[0]
        step = max(1, (1 << 21) // (k * k))
        for s in range(0, sel_all.size, step):
            sel = sel_all[s:s + step]
            rr = r0[sel][:, None, None] + np.arange(k)[None, :, None]
            cc = c0[sel][:, None, None] + np.arange(k)[None, None, :]
            inbox = (rr <= r1[sel][:, None, None]) & (cc <= c1[sel][:, None, None])
            px, py = cc * 256 + 128, rr * 256 + 128
            X, Y = x[sel][:, :, None, None], y[sel][:, :, None, None]
            inside, w = inbox, []
            for a, b in ((1, 2), (2, 0), (0, 1)):                                   # the edge opposite vertex 0, 1, 2
                dx, dy = X[:, b] - X[:, a], Y[:, b] - Y[:, a]
                e = dx * (py - Y[:, a]) - dy * (px - X[:, a])
                inside = inside & ((e < 0) | ((e == 0) & owns(dx, dy)))
                w.append(-e)
            t, ri, ci = np.nonzero(inside)
            if t.size == 0:
                continue
            area = (-A[sel][t]).astype(np.float64)
            b = np.stack([w[j][t, ri, ci].astype(np.float64) / area for j in range(3)], axis=1)
            depth = (b * dv[sel][t]).sum(axis=1)
            ok = ((depth >= -1.0) & (depth < 1.0)) | (not clip)
            out.append(((rr[t, ri, 0] * W + cc[t, 0, ci])[ok], keep[sel][t][ok], depth[ok], b[ok]))
        if k >= max(H, W):
            break
        k *= 2
    if not out:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 3))
    return tuple(np.concatenate([o[j] for o in out]) for j in range(4))


def fragments_rational(ix, iy, d, valid, faces, H, W, clip=True):
    """The second formulation: every pixel centre p against every front face, no bounding box.  p - v0 = u e1 + v e2 with e1 = v1 - v0,
    e2 = v2 - v0 has the exact rational solution u = ((p - v0) x e2) / A, v = (e1 x (p - v0)) / A, w = 1 - u - v.  p is inside when all three
    are positive; a zero puts p on an edge -- u: v2 -> v0, v: v0 -> v1, w: v1 -> v2 -- and then that edge's class decides.  Same return as `fragments`."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keep, A = front_faces(ix, iy, valid, f)
    r, c = np.divmod(np.arange(H * W, dtype=np.int64), W)
    px, py = c * 256 + 128, r * 256 + 128
    out = []
    for j, a in zip(keep, A):
        (x0, x1, x2), (y0, y1, y2) = ix[f[j]], iy[f[j]]
        qx, qy = px - x0, py - y0
        nu = qx * (y2 - y0) - (x2 - x0) * qy                  # u A
        nv = (x1 - x0) * qy - qx * (y1 - y0)                  # v A
        nw = a - nu - nv                                       # w A;  A < 0: a positive coordinate has a negative numerator
        inside = ((nu < 0) | ((nu == 0) & owns(x0 - x2, y0 - y2))) & ((nv < 0) | ((nv == 0) & owns(x1 - x0, y1 - y0))) \
            & ((nw < 0) | ((nw == 0) & owns(x2 - x1, y2 - y1)))
        p = np.nonzero(inside)[0]
        if p.size == 0:
            continue
        u, v = nu[p].astype(np.float64) / float(a), nv[p].astype(np.float64) / float(a)
        b = np.stack([1.0 - u - v, u, v], axis=1)
        depth = (b * d[f[j]]).sum(axis=1)
        ok = ((depth >= -1.0) & (depth < 1.0)) | (not clip)
        out.append((p[ok], np.full(int(ok.sum()), j, dtype=np.int64), depth[ok], b[ok]))
    if not out:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 3))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(4))


def render_instance(verts, faces, cam, R, color, H, W, formulation=fragments):
    """One mesh -> dict of [H,W] planes: face (-1 uncovered), depth, second (the next depth at that pixel, +inf if none), value [H,W,3]
    (255 colour before rounding; meaningless where uncovered), count (fragments per pixel) and, a scalar, clip_margin: how close any covered
    fragment's depth comes to a clip plane (an fp32 depth may fall on the other side only that close)."""
    ix, iy, d, valid, P = vertex_stage(verts, cam, R, H, W)
    pix, face, depth, b = formulation(ix, iy, d, valid, faces, H, W, clip=False)
    margin = float(np.minimum(np.abs(depth + 1.0), np.abs(depth - 1.0)).min()) if depth.size else np.inf
    ok = (depth >= -1.0) & (depth < 1.0)
    pix, face, depth, b = pix[ok], face[ok], depth[ok], b[ok]
    order = np.lexsort((face, depth, pix))
    pix, face, depth, b = pix[order], face[order], depth[order], b[order]
    first = np.ones(pix.size, dtype=bool)
    first[1:] = pix[1:] != pix[:-1]
    second = np.zeros(pix.size, dtype=bool)
    second[1:] = first[:-1] & ~first[1:]
    out = {'face': np.full(H * W, -1, dtype=np.int64), 'depth': np.full(H * W, np.inf), 'second': np.full(H * W, np.inf),
           'value': np.zeros((H * W, 3)), 'count': np.bincount(pix, minlength=H * W)}
    out['face'][pix[first]] = face[first]
    out['depth'][pix[first]] = depth[first]
    out['second'][pix[second]] = depth[second]
    n = vertex_normals(P, faces)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[face[first]]
    with np.errstate(invalid='ignore'):
        nn = (b[first][:, :, None] * n[f]).sum(axis=1)
        length = np.sqrt((nn * nn).sum(axis=1))
        lam = np.where(length > 0, np.maximum(0.0, nn[:, 2] / np.where(length > 0, length, 1.0)), 0.0)
    col = np.asarray(color, dtype=np.float32).astype(np.float64)
    out['value'][pix[first]] = 255.0 * np.clip(col[None, :] * (0.3 + LIGHT * lam)[:, None] + 0.1, 0.0, 1.0)
    out = {k: v.reshape((H, W) + v.shape[1:]) for k, v in out.items()}
    out['clip_margin'] = margin
    return out


def render(frames, frame_index, verts, faces, cams, colors, rot=None):
    """The call of tepose_render_meshes_u8: frames [F,H,W,3] uint8 and n instances in draw order -> dict of [F,H,W] planes: image [F,H,W,3] uint8,
    instance / face (-1 uncovered), depth, second (of the winning instance), value [F,H,W,3]; clip_margin: the smallest over the instances."""
    frames = np.asarray(frames)
    F, H, W = frames.shape[:3]
    out = {'image': frames.copy(), 'instance': np.full((F, H, W), -1, dtype=np.int64), 'face': np.full((F, H, W), -1, dtype=np.int64),
           'depth': np.full((F, H, W), np.inf), 'second': np.full((F, H, W), np.inf), 'value': np.zeros((F, H, W, 3)), 'clip_margin': np.inf}
    for i, fi in enumerate(np.asarray(frame_index)):
        one = render_instance(verts[i], faces, cams[i], None if rot is None else rot[i], colors[i], H, W)
        m = one['face'] >= 0
        out['clip_margin'] = min(out['clip_margin'], one['clip_margin'])
        out['instance'][fi][m] = i
        for k in ('face', 'depth', 'second', 'value'):
            out[k][fi][m] = one[k][m]
        out['image'][fi][m] = quantise(one['value'][m])
    return out


def quantise(values):
    return np.floor(values + 0.5).astype(np.uint8)


def near_half(values, window=1e-3):
    return np.abs(values - np.floor(values) - 0.5) < window


def fragment_stage_fp32(verts, faces, cam, R, color, H, W):
    """An fp32 emulation of the kernel's fragment stage on the oracle's own winners: barycentrics from the integer edge values rounded to fp32 and
    divided in fp32, depth and normal sums in the kernel's order, fp32 normals -> (depth [H,W], value [H,W,3]) as fp64 arrays of fp32 numbers.
    For the bound the GPU test records: how far fp32 shading may land from the fp64 value."""
    f32 = np.float32
    ix, iy, d, valid, P = vertex_stage(verts, cam, R, H, W)
    one = render_instance(verts, faces, cam, R, color, H, W)
    r, c = np.nonzero(one['face'] >= 0)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[one['face'][r, c]]
    px, py = c * 256 + 128, r * 256 + 128
    w = []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        w.append(-((ix[f[:, b]] - ix[f[:, a]]) * (py - iy[f[:, a]]) - (iy[f[:, b]] - iy[f[:, a]]) * (px - ix[f[:, a]])))
    area = (w[0] + w[1] + w[2]).astype(f32)
    b = [wi.astype(f32) / area for wi in w]
    dv = d[f].astype(f32)
    depth = (b[0] * dv[:, 0] + b[1] * dv[:, 1]) + b[2] * dv[:, 2]
    n = vertex_normals(P, faces).astype(f32)[f]
    nn = [(b[0] * n[:, 0, k] + b[1] * n[:, 1, k]) + b[2] * n[:, 2, k] for k in range(3)]
    length = np.sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2])
    lam = np.where(length > 0, np.maximum(f32(0), nn[2] / np.where(length > 0, length, f32(1))), f32(0)).astype(f32)
    light = f32(0.3) + f32(LIGHT) * lam
    col = np.asarray(color, dtype=f32)
    value = f32(255) * np.clip(col[None, :] * light[:, None] + f32(0.1), f32(0), f32(1))
    assert value.dtype == f32 and depth.dtype == f32
    D, Vv = np.full((H, W), np.inf), np.zeros((H, W, 3))
    D[r, c], Vv[r, c] = depth, value
    return D, Vv


def adjacency(faces, V):
    """CSR vertex -> faces, ascending face index per vertex, over the faces whose three indices lie in [0, V): offsets [V+1], list, int32."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = np.nonzero(usable_faces(f, V))[0]
    vert, face = f[ok].reshape(-1), np.repeat(ok, 3)
    order = np.lexsort((face, vert))
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(vert, minlength=V), out=off[1:])
    return off.astype(np.int32), face[order].astype(np.int32)


# ---- meshes of the tests ---------------------------------------------------------------------------------------------------------------------
def uv_sphere(segments, rings, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """A closed UV sphere: 2 + segments (rings - 1) vertices, 2 segments (rings - 1) faces, outward counter-clockwise.  84 x 83 has SMPL's counts:
    6 890 vertices, 13 776 faces."""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones(segments)[None], np.sin(th)[:, None] * np.sin(ph)[None]], axis=-1)
    v = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]]) * radius + np.asarray(centre)
    idx = lambda i, j: 1 + i * segments + (j % segments)
    faces = []
    for j in range(segments):
        faces.append([0, idx(0, j + 1), idx(0, j)])
        for i in range(rings - 2):
            faces.append([idx(i, j), idx(i, j + 1), idx(i + 1, j)])
            faces.append([idx(i, j + 1), idx(i + 1, j + 1), idx(i + 1, j)])
        faces.append([len(v) - 1, idx(rings - 2, j), idx(rings - 2, j + 1)])
    return v.astype(np.float32), np.asarray(faces, dtype=np.int32)


def torus(nu, nv, R=0.7, r=0.28, tilt=(0.5, 0.3, 0.2)):
    u, v = np.meshgrid(2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv, indexing='ij')
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), r * np.sin(v), (R + r * np.cos(v)) * np.sin(u)], axis=-1).reshape(-1, 3)
    p = p @ rotation(57.0, tilt).T
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    faces = []
    for i in range(nu):
        for j in range(nv):
            faces.append([idx(i, j), idx(i, j + 1), idx(i + 1, j)])
            faces.append([idx(i, j + 1), idx(i + 1, j + 1), idx(i + 1, j)])
    return p.astype(np.float32), np.asarray(faces, dtype=np.int32)


def blob(seed=0, scale=(0.35, 0.9, 0.3)):
    """6 890 vertices / 13 776 faces, closed: the 84 x 83 sphere, stretched to a person's proportions and dented smoothly."""
    v, f = uv_sphere(84, 83)
    g = np.random.default_rng(seed)
    k = g.uniform(1.0, 3.0, (4, 3))
    bump = 1.0 + 0.08 * sum(np.sin(v.astype(np.float64) @ k[i] * 2.0 + i) for i in range(4))
    return (v * bump[:, None] * np.asarray(scale)).astype(np.float32), f
