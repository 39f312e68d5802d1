"""GPU: tepose_amd.demo.render_tracklets -- demo.py:371-420 on the device -- on two ragged tracklets over 3 frames of 97 x 131.  Blob meshes stand in
for the SMPL vertices and the `results` dicts are fabricated: what is checked is the composition, bit for bit, of pieces that are pinned on their
own -- the draw order of `prepare_rendering_results` (tests/test_render_host.py, against the reference's function) and `Renderer.render` per person
(tests/test_gpu_render.py, against the fp64 oracle)."""
import numpy as np
import pytest
import torch

import _render_cases as C
import _render_ref as R

pytestmark = pytest.mark.gpu
F = 3


@pytest.fixture(scope='module')
def scene():
    """Person 4 in frames 0 and 1, person 9 in frame 1 only, nobody in frame 2; in frame 1 person 9 has the smaller y scale and is drawn first."""
    verts, faces = R.blob(5)
    g = np.random.default_rng(11)
    results = {
        4: {'frame_ids': np.array([0, 1]), 'verts': np.stack([verts, verts * np.float32(0.9)]), 'orig_cam': np.array([C.cam(0.7, 0.1, 0.0), C.cam(0.8, 0.2, 0.05)]),
            'bboxes': g.uniform(10, 90, (2, 4))},
        9: {'frame_ids': np.array([1]), 'verts': (verts * np.float32(1.1))[None], 'orig_cam': np.array([C.cam(0.6, -0.1, 0.1)]), 'bboxes': g.uniform(10, 90, (1, 4))},
    }
    return torch.from_numpy(C.noise(12, F)).cuda(), results, faces


def _compose(frames, results, faces, colors, start=None, **kw):
    """demo.py:380-420 with the pinned pieces: per frame, Renderer.render once per person in the order of prepare_rendering_results."""
    from tepose_amd.demo import prepare_rendering_results
    from tepose_amd.render import Renderer
    r = Renderer(faces)
    out = []
    for f, persons in enumerate(prepare_rendering_results(results, frames.shape[0])):
        img = frames[f] if start is None else start[f]
        for pid, data in persons.items():
            img = r.render(img, data['verts'], data['cam'], color=colors[pid], **kw)
        out.append(img)
    return torch.stack(out)


def test_render_tracklets_is_the_composition_of_its_pinned_pieces(scene):
    from tepose_amd.demo import default_mesh_colors, prepare_rendering_results, render_tracklets
    frames, results, faces = scene
    keep = frames.clone()
    order = [list(p.keys()) for p in prepare_rendering_results(results, F)]
    assert order == [[4], [9, 4], []]
    got = render_tracklets(frames, results, faces)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (F, C.H, C.W, 3) and torch.equal(frames, keep)      # a new tensor; the input is left alone
    want = _compose(frames, results, faces, default_mesh_colors(results.keys()))
    assert torch.equal(got, want)
    assert torch.equal(got[2], frames[2])                                          # nobody there: unchanged
    assert int((got[0] != frames[0]).any(dim=-1).sum()) > 1000 and int((got[1] != got[0]).any(dim=-1).sum()) > 1000
    # both persons show in frame 1, and the one drawn last is on top where they overlap
    colors = {4: (1.0, 0.0, 0.0), 9: (0.0, 0.0, 1.0)}
    two = render_tracklets(torch.zeros_like(frames), results, faces, colors=colors)
    red, blue = (two[1, :, :, 0] > 100) & (two[1, :, :, 2] < 50), (two[1, :, :, 2] > 100) & (two[1, :, :, 0] < 50)
    only4 = render_tracklets(torch.zeros_like(frames), {4: results[4]}, faces, colors=colors)
    assert int(red.sum()) > 1000 and int(blue.sum()) > 100
    assert torch.equal(red, (only4[1, :, :, 0] > 100))                             # person 4, drawn last, is complete
    assert torch.equal(render_tracklets(frames, results, faces, colors=colors), _compose(frames, results, faces, colors))


def test_plain_and_sideview(scene):
    from tepose_amd.demo import default_mesh_colors, render_tracklets
    frames, results, faces = scene
    colors = default_mesh_colors(results.keys())
    zeros = torch.zeros_like(frames)
    plain = render_tracklets(frames, results, faces, plain=True)
    assert torch.equal(plain, _compose(frames, results, faces, colors, start=zeros))
    assert not bool(plain[2].any()) and bool(plain[0].any())
    wide = render_tracklets(frames, results, faces, sideview=True)
    assert tuple(wide.shape) == (F, C.H, 2 * C.W, 3)
    assert torch.equal(wide[:, :, :C.W], render_tracklets(frames, results, faces))
    side = _compose(frames, results, faces, colors, start=zeros, angle=270, axis=[0, 1, 0])
    assert torch.equal(wide[:, :, C.W:], side)
    assert not bool(wide[2, :, C.W:].any()) and bool(wide[1, :, C.W:].any()) and not torch.equal(side, plain)
    both = render_tracklets(frames, results, faces, sideview=True, plain=True)
    assert torch.equal(both[:, :, :C.W], plain) and torch.equal(both[:, :, C.W:], side)
    assert tuple(render_tracklets(frames, {}, faces, sideview=True).shape) == (F, C.H, 2 * C.W, 3)
