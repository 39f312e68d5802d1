"""GPU: the overlay rasteriser (csrc/render.hip through tepose_amd.render.Renderer) against the fp64 oracle tests/_render_ref.py on the cases of
tests/_render_cases.py: 97 x 131 images (rows of W * 3 bytes are not dword-aligned) and one 1080p frame.

What is pinned is the definition, not pyrender: no OpenGL output exists to compare with.

  coverage  the set of pixels with a winner equals the oracle's, exactly: coverage is integer arithmetic on coordinates snapped in fp64.  The depth clip
            is fp32 on the device, so each case first asserts, from the oracle alone, that no fragment lies within 1e-5 of a clip plane.
  winner    the winning instance equals the oracle's everywhere; the winning face equals it except where the oracle's two nearest fragments of that
            instance lie within 1e-5 in d -- and such pixels are at most 0.5 % of the covered ones, asserted from the oracle first (the cases have none).
  colour    equals the oracle's uint8, except where a pre-rounding value is within 1e-3 grey levels of a half-integer: there +-1 is allowed, and such
            values are at most 0.5 % of the covered ones, asserted from the oracle first (0.04 - 0.29 % here).  The window is derived, not tuned: an fp32
            emulation of the fragment stage on these very cases (tests/test_render_host.py) lands within 4.7e-5 grey levels of the fp64 colour and
            within 1.6e-7 of the fp64 depth, so it can round the other way only that close to a half; 1e-3 is about 20 times that.
  elsewhere an uncovered pixel is bit-equal to the input frame.
"""
import numpy as np
import pytest
import torch

import _render_cases as C
import _render_ref as R

pytestmark = pytest.mark.gpu
_ORACLE = {}


def _case(name):
    """The case and its oracle, computed once and shared."""
    if name not in _ORACLE:
        c = C.CASES[name]()
        _ORACLE[name] = (c, R.render(c['frames'], c['idx'], c['verts'], c['faces'], c['cams'], c['colors'], c['rot']))
    return _ORACLE[name]


def _renderer(c):
    from tepose_amd.render import Renderer
    return Renderer(c['faces'])


def _run(r, c, frames=None, out=None):
    d_frames = torch.from_numpy(c['frames']).cuda() if frames is None else frames
    got = r.render_frames(d_frames, c['idx'], c['verts'], c['cams'], c['colors'], rot=c['rot'], out=out, return_winner=True)
    torch.cuda.synchronize()
    return got


def _compare(name, c, want, img, winner, depth):
    covered = want['face'] >= 0
    n_cov = int(covered.sum())
    with np.errstate(invalid='ignore'):
        tie = covered & ((want['second'] - want['depth']) < 1e-5)
    near = R.near_half(want['value'], 1e-3) & covered[..., None]
    print('%s: covered %d px; near depth ties %d; values within 1e-3 of a half-integer %.3f %%; nearest fragment to a clip plane %.2e'
          % (name, n_cov, int(tie.sum()), 100.0 * near.sum() / max(1, 3 * n_cov), want['clip_margin']))
    assert tie.sum() <= 0.005 * n_cov and near.sum() <= 0.005 * 3 * n_cov and want['clip_margin'] >= 1e-5      # from the oracle alone

    assert np.array_equal(winner[..., 0] >= 0, covered), (int((winner[..., 0] >= 0).sum()), n_cov, np.argwhere((winner[..., 0] >= 0) != covered)[:5].tolist())
    assert np.array_equal(winner[..., 0], want['instance'])
    wrong = (winner[..., 1] != want['face']) & ~tie
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
    assert np.array_equal(np.isinf(depth), ~covered)
    derr = float(np.abs(depth[covered] - want['depth'][covered]).max()) if n_cov else 0.0
    diff = img.astype(np.int16) - want['image'].astype(np.int16)
    bad = (diff != 0) & ~(near & (np.abs(diff) <= 1))
    print('%s: max |depth - oracle| = %.3g; %d of %d values differ from the oracle, all inside the window: %s' % (name, derr, int((diff != 0).sum()), diff.size, not bad.any()))
    assert derr <= 1e-5, derr
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), want['value'][bad[..., 0] | bad[..., 1] | bad[..., 2]][:5].tolist())
    assert np.array_equal(img[~covered], c['frames'][~covered])                          # bit-equal to the input where nothing was drawn


@pytest.mark.parametrize('name', list(C.CASES))
def test_render_against_the_fp64_oracle(name):
    c, want = _case(name)
    covered = want['face'] >= 0
    # the fixture's own sanity, from the oracle
    if name in ('outside', 'back_facing'):
        assert not covered.any()
    elif name == 'clip':
        assert covered.sum() > 500 and not covered[0, C.H // 2, 51] and want['depth'][covered].min() < -0.99 and want['depth'][covered].max() > 0.99
    elif name == 'three_instances':                        # the farthest sphere is drawn last and hides nearer ones: draw order beats depth
        hides = want['instance'][0] == 2
        first = R.render(c['frames'], c['idx'][:2], c['verts'][:2], c['faces'], c['cams'][:2], c['colors'][:2])
        assert (hides & (first['face'][0] >= 0) & (first['depth'][0] < want['depth'][0])).sum() > 100
    elif name == 'degenerate':
        assert not np.isin(want['face'], np.arange(c['faces'].shape[0] - 4, c['faces'].shape[0])).any()
    elif name == 'two_frames':
        assert sorted(np.unique(want['instance'][1]).tolist()) == [-1, 0, 2, 3] and sorted(np.unique(want['instance'][0]).tolist()) == [-1, 1]
    elif name == 'full_hd':
        assert covered[0, :, 1900:].sum() > 3000
    elif name == 'side_view':
        assert not np.array_equal(covered, _case('blob_6890')[1]['face'] >= 0)
    else:
        border = {'edge_left': covered[0, :, 0], 'edge_right': covered[0, :, -1], 'edge_top': covered[0, 0], 'edge_bottom': covered[0, -1]}
        if name in border:
            assert border[name].sum() > 20
        if name == 'corner':
            assert covered[0, 0, 0] and covered[0, :, 0].sum() > 20 and covered[0, 0].sum() > 20
        if name == 'overflow':
            assert covered.all()
        assert covered.sum() > 1000
    img, winner, depth = _run(_renderer(c), c)
    assert img.dtype == torch.uint8 and tuple(img.shape) == c['frames'].shape and tuple(winner.shape) == c['frames'].shape[:3] + (2,)
    _compare(name, c, want, img.cpu().numpy(), winner.cpu().numpy(), depth.cpu().numpy())


def test_a_face_with_an_index_outside_the_mesh_draws_nothing():
    """Through the C entry (Renderer refuses such faces): two faces of the sphere point at vertex V and at -1.  The kernel skips a face whose index
    is outside [0, V) by definition -- it reads nothing for it -- and the picture is the oracle's, which leaves the two faces out."""
    from tepose_amd import _lib
    c, _ = _case('sphere_24x16')
    faces = c['faces'].copy()
    V = c['verts'].shape[1]
    front = np.unique(_case('sphere_24x16')[1]['face'])
    faces[front[5], 1], faces[front[9], 0] = V, -1
    c = dict(c, faces=faces)
    want = R.render(c['frames'], c['idx'], c['verts'], faces, c['cams'], c['colors'])
    assert (want['face'] >= 0).sum() < (_case('sphere_24x16')[1]['face'] >= 0).sum()       # the two faces leave a hole
    off, lst = R.adjacency(faces, V)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(v) for k, v in dict(frames=c['frames'], idx=c['idx'].astype(np.int32), verts=c['verts'], faces=faces, off=off, lst=lst, cams=c['cams'],
                                    colors=c['colors']).items()}
    F, H, W = c['frames'].shape[:3]
    lib = _lib.load()
    ws = torch.empty(int(lib.tepose_render_workspace_bytes(H, W, F, 1, V, faces.shape[0])), dtype=torch.uint8, device='cuda')
    img, winner, depth = torch.empty_like(d['frames']), torch.empty((F, H, W, 2), dtype=torch.int32, device='cuda'), torch.empty((F, H, W), device='cuda')
    _lib.check(lib.tepose_render_meshes_u8(d['frames'].data_ptr(), F, H, W, d['idx'].data_ptr(), d['verts'].data_ptr(), 1, V, d['faces'].data_ptr(), faces.shape[0],
                                           d['off'].data_ptr(), d['lst'].data_ptr(), lst.shape[0], d['cams'].data_ptr(), None, d['colors'].data_ptr(), img.data_ptr(),
                                           winner.data_ptr(), depth.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), 'tepose_render_meshes_u8')
    torch.cuda.synchronize()
    _compare('bad_face_index', c, want, img.cpu().numpy(), winner.cpu().numpy(), depth.cpu().numpy())


def test_repeated_calls_split_calls_and_chunked_calls_are_bit_equal(monkeypatch):
    c, _ = _case('two_frames')
    r = _renderer(c)
    a, b = _run(r, c), _run(r, c)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                                  # two calls
    d_frames = torch.from_numpy(c['frames']).cuda()
    for f in (0, 1):                                                                      # one call over two frames = two one-frame calls
        sel = np.nonzero(c['idx'] == f)[0]
        img, winner, depth = r.render_frames(d_frames[f:f + 1], np.zeros(sel.size, dtype=np.int64), c['verts'][sel], c['cams'][sel], c['colors'][sel], return_winner=True)
        assert torch.equal(img[0], a[0][f]) and torch.equal(depth[0], a[2][f]) and torch.equal(winner[0, :, :, 1], a[1][f, :, :, 1])
        inst = winner[0, :, :, 0]
        assert torch.equal(torch.where(inst >= 0, torch.from_numpy(sel).cuda()[inst.clamp(min=0).long()].to(torch.int32), inst), a[1][f, :, :, 0])
    small = _renderer(c)
    small.workspace_cap_bytes = 1                                                         # one frame per library call
    calls = []
    from tepose_amd import _lib
    lib = _lib.load()
    real = lib.tepose_render_meshes_u8

    class Counting:
        def __getattr__(self, k):
            return getattr(lib, k)

        def tepose_render_meshes_u8(self, *args):
            calls.append(args[1])
            return real(*args)
    monkeypatch.setattr(_lib, 'load', lambda: Counting())
    chunked = _run(small, c)
    assert calls == [1, 1]                                                                # the cap did split the call
    assert all(torch.equal(x, y) for x, y in zip(a, chunked))


def test_out_may_be_the_frames_and_an_empty_call_copies():
    c, want = _case('three_instances')
    r = _renderer(c)
    fresh = _run(r, c)[0]
    d_frames = torch.from_numpy(c['frames']).cuda()
    ret = r.render_frames(d_frames, c['idx'], c['verts'], c['cams'], c['colors'], out=d_frames)
    assert ret is d_frames and torch.equal(d_frames, fresh)
    d_frames = torch.from_numpy(c['frames']).cuda()
    none = r.render_frames(d_frames, np.zeros(0, dtype=np.int64), c['verts'][:0], c['cams'][:0], c['colors'][:0])
    assert none is not d_frames and torch.equal(none, d_frames)
    img, winner, depth = r.render_frames(d_frames, np.zeros(0, dtype=np.int64), c['verts'][:0], c['cams'][:0], c['colors'][:0], return_winner=True)
    assert torch.equal(img, d_frames) and bool((winner == -1).all()) and bool(torch.isinf(depth).all())
    # the reference's call shape: one image, one mesh, numpy or device vertices, angle / axis
    one = r.render(d_frames[0], c['verts'][0], c['cams'][0], color=c['colors'][0])
    again = r.render(d_frames[0], torch.from_numpy(c['verts'][0]).cuda(), tuple(c['cams'][0]), color=tuple(c['colors'][0]))
    assert tuple(one.shape) == (C.H, C.W, 3) and torch.equal(one, again) and not torch.equal(one, d_frames[0])
    first = R.render(c['frames'], c['idx'][:1], c['verts'][:1], c['faces'], c['cams'][:1], c['colors'][:1])
    assert (one.cpu().numpy() != first['image'][0]).sum() <= 0.005 * first['image'][0].size
    side = r.render(d_frames[0], c['verts'][0], c['cams'][0], angle=270, axis=[0, 1, 0], color=c['colors'][0])
    want_side = r.render_frames(d_frames, [0], c['verts'][:1], c['cams'][:1], c['colors'][:1], rot=R.rotation(270, [0, 1, 0])[None])[0]
    assert torch.equal(side, want_side) and not torch.equal(side, one)
