"""GPU: the two tile walks of the persistent scaled-plane product (csrc/walk.h; option S16_WALK) compute the same bits.  The walk only permutes which
workgroup computes which 256 x 256 tile -- fragments, K order and epilogue of a tile do not change -- so handles of the published architecture built from
ONE state, one on walk 0 and the others on walk 1 (S16_GM 8, 4, 16), must return torch.equal outputs.  Shapes: the smallest at which the persistent kernel
runs and the map can go wrong (640 x 16: 40 row tiles, 1440 tiles = 5.6 rounds of 256 workgroups for the layer-0 projection, 480 tiles = less than two
rounds for the layer-1 projections; 650 x 16: a ragged last row tile; 1400 x 6: the published window length, ragged rows)."""
import pytest
import torch

from tepose_amd import synth

pytestmark = pytest.mark.gpu

KEYS = ('theta', 'verts', 'kp_3d', 'kp_2d', 'rotmat')
L, H = 2, 1024


@pytest.fixture(scope='module')
def handles():
    """{(walk, gm): model} from one synthetic state; options set before anything is packed."""
    from tepose_amd.testing import build_model
    smpl_np = synth.synthetic_smpl(0)
    state = synth.synthetic_state_dict(L, H, 7)
    out = {}
    for walk, gm in ((0, 8), (1, 8), (1, 4), (1, 16)):
        m, _, _ = build_model(L, H, seed=7, device='cuda', smpl_np=smpl_np, state=state)
        m._engine.set_option('S16_WALK', walk)
        m._engine.set_option('S16_GM', gm)
        assert m._engine.get_option('S16_WALK') == walk and m._engine.get_option('TEPOSE_S16_GM') == gm
        out[(walk, gm)] = m
    return out, torch.from_numpy(smpl_np['J_regressor_h36m'])


_REF = {}


def _run(model, J, B, T):
    x = torch.from_numpy(synth.synthetic_windows(B, T, 11)).cuda()
    with torch.no_grad():
        o = model(x, J_regressor=J)[0]
    torch.cuda.synchronize()
    return {k: o[k].clone() for k in KEYS}


def _reference(handles, B, T):
    """Walk 0's outputs of a shape: computed once, shared by the cases, never written."""
    if (B, T) not in _REF:
        hs, J = handles
        s = hs[(0, 8)]._engine.select_kernels(B, T)
        assert s['projection'] == 'gemm_h3s_persist16c_kernel<0>' and s['projection_l1'] == 'gemm_h3s_persist16c_kernel<1>', s
        _REF[(B, T)] = _run(hs[(0, 8)], J, B, T)
        assert all(torch.isfinite(v).all() for v in _REF[(B, T)].values())
    return _REF[(B, T)]


@pytest.mark.parametrize('B,T,gm', [(640, 16, 8), (650, 16, 8), (1400, 6, 8), (640, 16, 4), (640, 16, 16)])
def test_walk1_is_bit_identical_to_walk0(handles, B, T, gm):
    hs, J = handles
    ref = _reference(handles, B, T)
    assert hs[(1, gm)]._engine.select_kernels(B, T) == hs[(0, 8)]._engine.select_kernels(B, T)        # the plan does not move with the walk
    from tepose_amd import _lib
    gave_up = _lib.load().tepose_debug_kernel_errors()            # process-wide: other tests of the suite raise it on purpose
    got = _run(hs[(1, gm)], J, B, T)
    for k in KEYS:
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), (B, T, gm, k, float((got[k] - ref[k]).abs().max()))
    assert _lib.load().tepose_debug_kernel_errors() == gave_up
