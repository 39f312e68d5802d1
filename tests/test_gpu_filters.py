"""GPU: post-filter kernels against vectors from the reference's OneEuroFilter / quaternion utilities."""
import os

import numpy as np
import pytest
import torch

from tepose_amd import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def test_one_euro_and_slerp_match_reference():
    from tepose_amd.filters import one_euro, smooth_pose_mat
    g = np.load(os.path.join(GOLDEN, 'filters.npz'))
    hat = one_euro(g['pose']).cpu().numpy()
    assert hat.shape == g['pose_hat'].shape
    assert np.abs(hat - g['pose_hat']).max() < 1e-5
    Rs = smooth_pose_mat(g['R'], ratio=0.3)
    assert isinstance(Rs, np.ndarray) and np.abs(Rs - g['R_smooth']).max() < 1e-5
    one = smooth_pose_mat(torch.from_numpy(g['R'][:1]).cuda())
    assert (one.cpu() - torch.from_numpy(g['R'][:1])).abs().max() < 1e-6     # single frame: identity filter


@pytest.fixture(scope='module')
def edges():
    """tests/golden/filters_edges.npz (make_golden.py `edges`): the reference's two filters on rotations near pi about changing axes, angles
    over the whole circle, sweeps through pi about x / y / z, static joints, non-orthonormal frames; on axis-angle wraps and frozen frames."""
    return dict(np.load(os.path.join(GOLDEN, 'filters_edges.npz')))


def _wrapped_signal(tag, n, d):
    """[n, d] float32: smooth motion plus noise, +-2 pi jumps between consecutive frames in some columns (an axis-angle wrap) and, where
    the clip is long enough, frames that do not change."""
    x = (synth.normal(tag, (n, d), std=0.4) + 0.3 * np.sin(np.arange(n, dtype=np.float32) / 5.0)[:, None]).astype(np.float32)
    x[1:, ::7] += np.float32(2 * np.pi)                     # up at frame 1 and stays
    x[1:max(2, n // 2), 3::11] -= np.float32(2 * np.pi)     # down at frame 1, back up half way
    if n > 12:
        x[8:12] = x[7]
    return x


def test_slerp_edge_golden_every_branch_both_flips_all_ratios(edges):
    """smooth_pose_mat against the reference's on filters_edges.npz (16 frames x 72 joints: two blocks of slerp_smooth_kernel, the second
    partly filled; all four matrix -> quaternion branches at least 260 times each, 467 sign flips, 378 negative slerp dots at ratio 0.3 --
    tests/test_oracle.py counts them) at ratio 0.3, 0.85, 0 and 1 and for one and two frames, at 1e-5.  The error is reported per group
    of joints, so a failure names the branch family that went wrong: `sweep_x` / `pi_x_jitter` is the m00 branch, `sweep_y` m11,
    `sweep_z` m22, `near_pi` all three with both flips, `any_angle` adds trace > 0, the static groups are the slerp's early return.
    Expected: the fp32 rounding of the output.  Measured on an MI355X: worst 2.98e-8 = 2^-25, half the fp32 spacing below 1, in every case
    and in every group but `identity` (1.0e-8); a later drift from that is a finding even while it stays under the bound.
    What this test can and cannot see (tried with deliberately wrong builds): `d < 0` left unhandled fails it (0.89 in `near_pi` and
    `any_angle`), a wrong sign under the square root of the m11 branch fails it (NaN).  A wrong sign in one off-diagonal term of a branch
    does NOT change the output (3.1e-8): the branch only seeds two power steps that project onto the best-fit quaternion, so it must
    merely not be orthogonal to it.  Dropping the `dm > dp` flip alone does not change the output either: the slerp's shortest-path flip
    makes its result independent of the sign of q_t."""
    from tepose_amd.filters import smooth_pose_mat
    names = [str(n) for n in edges['group_names']]
    cases = [('ratio %.2f' % r, edges['R'], float(r), edges['R_smooth%d' % i]) for i, r in enumerate(edges['ratios'])]
    cases += [('N = %d' % n, edges['R'][:n], 0.3, edges['R_smooth_n%d' % n]) for n in (1, 2)]
    worst, bad = 0.0, []
    for label, R, ratio, ref in cases:
        out = smooth_pose_mat(R, ratio=ratio)
        assert isinstance(out, np.ndarray) and out.shape == ref.shape and np.isfinite(out).all(), label
        err = np.abs(out.astype(np.float64) - ref).max(axis=(0, 2, 3))                      # per joint
        per_group = {n: float(err[edges['group'] == k].max()) for k, n in enumerate(names)}
        print('slerp %-10s worst %.2e  %s' % (label, err.max(), '  '.join('%s %.1e' % kv for kv in per_group.items())))
        worst = max(worst, float(err.max()))
        bad += ['%s: %s %.2e' % (label, n, e) for n, e in per_group.items() if not e < 1e-5]
    print('slerp worst over all cases %.3e' % worst)
    assert not bad, bad


def test_slerp_in_place_equals_two_buffers_bitwise(edges):
    """tepose_filter_slerp allows rotmat_out == rotmat_in (include/tepose_amd.h): every thread reads a frame's matrix before it writes that
    frame's result.  The aliased call through the library itself, and the wrapper on a tensor that already lives on the device (which must
    not be written to), against the two-buffer call: bit for bit, at a ratio that slerps and at the two that return early."""
    from tepose_amd import _lib
    from tepose_amd.filters import smooth_pose_mat
    lib = _lib.load()
    src = torch.from_numpy(edges['R']).cuda()
    n, j = src.shape[:2]
    for ratio in (0.3, 0.0, 1.0):
        two = torch.full_like(src, float('nan'))
        _lib.check(lib.tepose_filter_slerp(src.data_ptr(), two.data_ptr(), n, j, ratio, torch.cuda.current_stream().cuda_stream), 'tepose_filter_slerp')
        one = src.clone()
        _lib.check(lib.tepose_filter_slerp(one.data_ptr(), one.data_ptr(), n, j, ratio, torch.cuda.current_stream().cuda_stream), 'tepose_filter_slerp')
        torch.cuda.synchronize()
        assert torch.isfinite(two).all() and not torch.equal(two, src)
        assert torch.equal(one, two), ratio
        dev = src.clone()
        out = smooth_pose_mat(dev, ratio=ratio)
        assert torch.is_tensor(out) and out.is_cuda and out.data_ptr() != dev.data_ptr()
        assert torch.equal(out, two) and torch.equal(dev, src), ratio
        assert np.array_equal(smooth_pose_mat(edges['R'], ratio=ratio), two.cpu().numpy()), ratio


def test_one_euro_edge_golden_wraps_static_frames_and_cutoffs(edges):
    """one_euro against the reference's smooth_pose on the [40, 24, 3] pose of filters_edges.npz (2 pi wraps between consecutive frames,
    eight frozen frames) at (min_cutoff, beta) = (0.004, 0.7), (0.004, 1.5), (1, 0), (1e-4, 5), at 1e-5.
    Measured on an MI355X: worst 4.8e-7 for the first three pairs and 9.5e-7 for (1e-4, 5) -- one and two fp32 spacings of the wrapped
    values (4 <= |x| < 8: 4.8e-7)."""
    from tepose_amd.filters import one_euro
    worst = 0.0
    for i, (mc, b) in enumerate(edges['euro']):
        hat = one_euro(edges['pose'], min_cutoff=float(mc), beta=float(b)).cpu().numpy()
        ref = edges['pose_hat%d' % i]
        assert hat.shape == ref.shape and np.array_equal(hat[0], edges['pose'][0])
        err = float(np.abs(hat - ref).max())
        print('one euro (%g, %g): worst %.2e' % (mc, b, err))
        worst = max(worst, err)
        assert err < 1e-5, (mc, b, err)
    print('one euro worst over the reference cases %.3e' % worst)


@pytest.mark.parametrize('n', [2, 33])
def test_one_euro_two_blocks_short_clips_and_d_cutoff_vs_oracle(n):
    """What the reference's wrapper fixes (72 components, d_cutoff = 1) against the oracle: D = 200 is two blocks of one_euro_kernel's 128
    threads with 72 threads of the second active; N = 2 is the shortest clip that filters at all; d_cutoff 0.5, 1 and 3; an input with
    2 pi wraps.  1e-5.  Measured on an MI355X: worst 4.8e-7 at N = 2; at N = 33 1.4e-6 (d_cutoff 0.5) and 9.5e-7 (1 and 3), the same in
    both blocks up to one fp32 spacing."""
    from oracle import tepose_ref as O
    from tepose_amd.filters import one_euro
    x = _wrapped_signal('flt/edge%d' % n, n, 200)
    assert np.abs(np.diff(x, axis=0)).max() > 5.0
    for d_cutoff in (0.5, 1.0, 3.0):
        hat = one_euro(x, min_cutoff=0.004, beta=0.7, d_cutoff=d_cutoff).cpu().numpy()
        ref = O.one_euro_filter(x, min_cutoff=0.004, beta=0.7, d_cutoff=d_cutoff)
        err = np.abs(hat - ref).max(axis=0)
        print('one euro N %d d_cutoff %g: worst %.2e (first block %.2e, second %.2e)' % (n, d_cutoff, err.max(), err[:128].max(), err[128:].max()))
        assert hat.shape == (n, 200) and err.max() < 1e-5, (n, d_cutoff, float(err.max()))
    if n > 2:                                                # d_cutoff is not a no-op on this input
        assert np.abs(O.one_euro_filter(x, d_cutoff=0.5) - O.one_euro_filter(x, d_cutoff=3.0)).max() > 1e-3


def test_one_euro_single_frame_is_returned_unchanged():
    from tepose_amd.filters import one_euro
    x = _wrapped_signal('flt/edge1', 1, 200)
    hat = one_euro(x, beta=1.5, d_cutoff=3.0)
    assert hat.shape == (1, 200) and np.array_equal(hat.cpu().numpy(), x)
    dev = torch.from_numpy(x).cuda()
    assert torch.equal(one_euro(dev), dev)


def test_smooth_pose_pipeline_vs_oracle():
    from oracle import tepose_ref as O
    from tepose_amd.filters import smooth_pose
    from tepose_amd.smpl import SMPL
    smpl_np = synth.synthetic_smpl(0)
    g = np.load(os.path.join(GOLDEN, 'filters.npz'))
    betas = synth.normal('flt/betas', (50, 10), std=0.5)
    verts, pose_hat, joints = smooth_pose(g['pose'], betas, SMPL.from_tables(smpl_np))
    assert verts.shape == (50, 6890, 3) and joints.shape == (50, 49, 3)
    ph = O.one_euro_filter(g['pose'])
    s = O.smpl_tensors(smpl_np)
    R = O.batch_rodrigues(torch.from_numpy(ph.reshape(-1, 3))).view(50, 24, 3, 3)
    v_ref, posed = O.lbs(s, torch.from_numpy(betas), R)
    assert np.abs(verts - v_ref.numpy()).max() < 1e-4
    assert np.abs(joints - O.smpl_joints49(s, v_ref, posed).numpy()).max() < 1e-4
    # ... and against what the reference's own smooth_pose returned for this very input (lib/utils/smooth_pose.py:24-68, called by the fixture generator)
    assert np.abs(pose_hat.reshape(50, 24, 3) - g['pose_hat']).max() < 1e-5
    assert np.abs(verts[:, ::53] - g['smooth_verts_sub']).max() < 1e-4
    assert np.abs(joints - g['smooth_joints']).max() < 1e-4
