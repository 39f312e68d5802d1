"""GPU: the SMPL backward (tepose_smpl_bwd, csrc/smpl_bwd.hip) against the fp64 gradient oracle (tests/_smpl_grad_ref.py: autograd
through oracle.tepose_ref on the CPU), and everything above it -- autograd through SMPL.forward, a captured graph of forward plus backward, fit_keypoints.

Bound, per output tensor: max|g - g64| / max|g64| <= 1e-4, the project's standing fp32 budget.  Every case prints that ratio next
to the fp32 oracle's on the same inputs, so what the kernels add to plain fp32 arithmetic is visible (the figures: profiles/smpl_backward.txt).

Shapes: N = 1 (the forward's one-launch family; 8-person tiles of the blend product's backward), N = 5 (just past SMPL_SMALL_MAX_N), N = 130 (crosses the
128-person tile of the forward's blend product; 32-person tiles with a tail of 2 in the backward's; 5 skinning block rows)."""
import functools

import pytest
import torch

import _buffers as BF
import _smpl_grad_ref as GR

pytestmark = pytest.mark.gpu
BOUND = 1e-4
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
REPEATED_K = (11, 25)        # 'OP RAnkle' and 'Right Ankle': both are posed joint 8 of the joint map


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _module(skin_nnz=4, exact=False):
    """A standalone SMPL layer on synthetic tables with its own engine (handle), packed.  exact: the handle is created under TEPOSE_EXACT_FP32=1."""
    from tepose_amd.engine import Engine
    from tepose_amd.smpl import SMPL
    smpl = SMPL.from_tables(GR.tables(skin_nnz), batch_size=1).cuda()
    mp = pytest.MonkeyPatch()
    try:
        if exact:
            mp.setenv('TEPOSE_EXACT_FP32', '1')
        else:
            mp.delenv('TEPOSE_EXACT_FP32', raising=False)
        eng = Engine(1, 64)
    finally:
        mp.undo()
    object.__setattr__(smpl, '_engine', eng)
    eng.pack_smpl(smpl, torch.device('cuda', torch.cuda.current_device()))
    return smpl, eng


@functools.lru_cache(maxsize=None)
def _inputs(N, pose_kind, pose2rot, grad_kind):
    """Seeded CPU fp32 inputs of a case: (pose, betas, g_verts | None, g_joints | None)."""
    g = torch.Generator().manual_seed(1000 * N + 7 * len(pose_kind) + len(grad_kind))
    aa = 0.4 * torch.randn(N, 24, 3, generator=g)
    aa = aa * torch.clamp(1.0 / aa.norm(dim=2, keepdim=True), max=1.0)              # generic: |aa| <= 1 per joint
    if pose_kind == 'zero':
        aa = torch.zeros(N, 24, 3)
    elif pose_kind == 'tiny':                                                       # one joint at 1e-4 rad, the rest at rest
        aa = torch.zeros(N, 24, 3)
        aa[:, 5] = torch.tensor([6e-5, -8e-5, 0.0])
    elif pose_kind == 'big':                                                        # one joint near 3.0 rad
        aa[:, 7] = 3.0 * torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=1)
    else:
        assert pose_kind == 'generic'
    pose = aa.reshape(N, 72) if pose2rot else GR.O.batch_rodrigues(aa.reshape(-1, 3)).view(N, 24, 3, 3).contiguous()
    betas = torch.randn(N, 10, generator=g)
    g_verts = torch.randn(N, 6890, 3, generator=g)
    g_joints = torch.randn(N, 49, 3, generator=g)
    if grad_kind == 'verts':
        g_joints = None
    elif grad_kind == 'joints':
        g_verts = None
    elif grad_kind == 'repeated':             # non-zero only on the two joints that are the same posed joint: a lost accumulation halves the result
        g_verts, keep = None, g_joints[:, REPEATED_K, :].clone()
        g_joints = torch.zeros(N, 49, 3)
        g_joints[:, REPEATED_K, :] = keep
    elif grad_kind == 'vertex':               # one vertex of the 10th skinning workgroup: every other partial of the transform gradient is zero
        g_joints, keep = None, g_verts[:, 5000].clone()
        g_verts = torch.zeros(N, 6890, 3)
        g_verts[:, 5000] = keep
    else:
        assert grad_kind == 'both'
    return pose, betas, g_verts, g_joints


@functools.lru_cache(maxsize=None)
def _oracle(N, pose_kind, pose2rot, grad_kind, skin_nnz):
    """(g_pose, g_betas) in fp64, and the fp32 oracle's ratios to it: computed once per input set, shared by every case on it, never written."""
    pose, betas, g_verts, g_joints = _inputs(N, pose_kind, pose2rot, grad_kind)
    smpl_np = GR.tables(skin_nnz)
    gp64, gb64 = GR.grads(smpl_np, pose, betas, pose2rot, g_verts, g_joints)
    gp32, gb32 = GR.grads(smpl_np, pose, betas, pose2rot, g_verts, g_joints, dtype=torch.float32)
    return gp64, gb64, GR.rel_err(gp32, gp64), GR.rel_err(gb32, gb64)


def _bwd(eng, pose2rot, pose, betas, g_verts, g_joints, want_pose=True, want_betas=True, ws=None, guarded=False):
    """tepose_smpl_bwd through the C entry on device tensors -> (g_pose | None, g_betas | None[, the guarded buffers])."""
    N = pose.shape[0]
    if ws is None:
        ws = torch.empty(int(eng.lib.tepose_smpl_bwd_workspace_bytes(eng.handle, N)), dtype=torch.uint8, device='cuda')
    if guarded:
        gp = BF.guarded_like(tuple(pose.shape), N, 'cuda', name='g_pose') if want_pose else None
        gb = BF.guarded_like((N, 10), N, 'cuda', name='g_betas') if want_betas else None
    else:
        gp = torch.full_like(pose, float('nan')) if want_pose else None
        gb = torch.full((N, 10), float('nan'), device='cuda') if want_betas else None
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = eng.lib.tepose_smpl_bwd(eng.handle, int(pose2rot), pose.data_ptr(), betas.data_ptr(), N, ptr(g_verts), ptr(g_joints), ptr(gp), ptr(gb),
                                 ws.data_ptr(), ws.numel(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    if guarded:
        return (None if gp is None else gp.own), (None if gb is None else gb.own), [t for t in (gp, gb) if t is not None]
    return gp, gb


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _check(what, got_pose, got_betas, N, pose_kind, pose2rot, grad_kind, skin_nnz):
    gp64, gb64, r32p, r32b = _oracle(N, pose_kind, pose2rot, grad_kind, skin_nnz)
    bad = []
    for name, got, ref, r32 in (('g_pose', got_pose, gp64, r32p), ('g_betas', got_betas, gb64, r32b)):
        if got is None:
            continue
        assert torch.isfinite(got).all(), (what, name)
        r = GR.rel_err(got.cpu(), ref)
        print('%s %-7s max|g - g64| / max|g64| = %.3e   (fp32 oracle: %.3e)' % (what, name, r, r32))
        if not r <= BOUND:
            bad.append((name, r))
    assert not bad, (what, bad)


# (N, pose2rot, gradients in, gradients out, skin_nnz, pose, exact fp32)
CASES = [
    # every N, both pose forms, both precision modes
    (1, True, 'both', 'both', 4, 'generic', False), (5, True, 'both', 'both', 4, 'generic', False), (130, True, 'both', 'both', 4, 'generic', False),
    (1, False, 'both', 'both', 4, 'generic', False), (5, False, 'both', 'both', 4, 'generic', False), (130, False, 'both', 'both', 4, 'generic', False),
    (1, True, 'both', 'both', 4, 'generic', True), (5, True, 'both', 'both', 4, 'generic', True), (130, True, 'both', 'both', 4, 'generic', True),
    # one gradient in; one gradient out
    (5, True, 'verts', 'both', 4, 'generic', False), (5, True, 'joints', 'both', 4, 'generic', False), (130, False, 'joints', 'both', 4, 'generic', False),
    (5, True, 'both', 'pose', 4, 'generic', False), (5, True, 'both', 'betas', 4, 'generic', False), (1, False, 'verts', 'pose', 4, 'generic', False),
    # the dense skin table (more than 4 non-zeros per vertex)
    (1, True, 'both', 'both', 6, 'generic', False), (5, False, 'both', 'both', 6, 'generic', False), (130, True, 'both', 'both', 6, 'generic', False),
    (5, True, 'both', 'both', 6, 'generic', True),
    # the poses a fit starts from and passes through
    (5, True, 'both', 'both', 4, 'zero', False), (1, True, 'both', 'both', 4, 'zero', True), (5, True, 'both', 'both', 4, 'tiny', False),
    (5, True, 'both', 'both', 4, 'big', False), (130, True, 'both', 'both', 4, 'big', True),
    # gradients that single out one accumulation
    (5, True, 'repeated', 'both', 4, 'generic', False), (5, False, 'repeated', 'both', 6, 'generic', False),
    (5, True, 'vertex', 'both', 4, 'generic', False), (130, True, 'vertex', 'both', 6, 'generic', False),
]
IDS = ['N%d-%s-g%s-out%s-nnz%d-%s%s' % (c[0], 'aa' if c[1] else 'rotmat', c[2], c[3], c[4], c[5], '-exact' if c[6] else '') for c in CASES]


@pytest.mark.parametrize('N,pose2rot,grad_kind,out_kind,skin_nnz,pose_kind,exact', CASES, ids=IDS)
def test_gradients_against_the_fp64_oracle(N, pose2rot, grad_kind, out_kind, skin_nnz, pose_kind, exact):
    _, eng = _module(skin_nnz, exact)
    pose, betas, g_verts, g_joints = _cuda(*_inputs(N, pose_kind, pose2rot, grad_kind))
    gp, gb = _bwd(eng, pose2rot, pose, betas, g_verts, g_joints, out_kind in ('both', 'pose'), out_kind in ('both', 'betas'))
    assert (gp is None) == (out_kind == 'betas') and (gb is None) == (out_kind == 'pose')
    _check(IDS[CASES.index((N, pose2rot, grad_kind, out_kind, skin_nnz, pose_kind, exact))], gp, gb, N, pose_kind, pose2rot, grad_kind, skin_nnz)


@pytest.mark.parametrize('N,skin_nnz', [(1, 4), (5, 6), (130, 4)])
def test_poison_guards_and_repeatability(N, skin_nnz):
    """Two calls on the same inputs are bit-equal; the results do not depend on what the workspace held (zeros, all-ones = NaN, 0x3C00); nothing is
    written outside the workspace and the first N rows of the outputs; the inputs are not written."""
    _, eng = _module(skin_nnz, False)
    pose, betas, g_verts, g_joints = _cuda(*_inputs(N, 'generic', True, 'both'))
    need = int(eng.lib.tepose_smpl_bwd_workspace_bytes(eng.handle, N))
    frozen = BF.Frozen(pose=pose, betas=betas, g_verts=g_verts, g_joints=g_joints)
    base = None
    for pattern in ('zeros', 'zeros', 'ones', 'finite'):
        ws = BF.poisoned(need, pattern, 'cuda', guard_bytes=BF.workspace_guard_bytes(64), name='smpl_bwd workspace')
        gp, gb, guards = _bwd(eng, True, pose, betas, g_verts, g_joints, ws=ws, guarded=True)
        BF.assert_guards_intact(ws, guards, what='smpl_bwd N = %d (%s)' % (N, pattern))
        frozen.assert_unchanged('smpl_bwd N = %d (%s)' % (N, pattern))
        got = (gp.clone(), gb.clone())
        if base is None:
            base = got
        assert BF.same_bits(got[0], base[0]) and BF.same_bits(got[1], base[1]), 'smpl_bwd N = %d: the result depends on the workspace (%s) or the run' % (N, pattern)
    assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all()


def test_a_person_does_not_depend_on_the_batch():
    """Rows 0..4 of an N = 130 call against the N = 5 call on the same five persons: bit for bit.  One kernel family serves both -- the same forward
    product recomputes v_posed row by row, the skinning partials are per person, and the blend product's backward cuts K into the same 323 chunks
    (every N <= 192) and adds a person's rows in the same order whatever the tile it sits in.  Row 0 of the N = 5 call against an N = 1 call is NOT
    the same family (N <= 4 recomputes v_posed on the exact-fp32 product, as the forward's one-launch kernel computes it; above, on the split
    product): there the difference stays within the bound, relative to the fp64 gradient of that row."""
    _, eng = _module(4, False)
    pose, betas, g_verts, g_joints = _inputs(130, 'generic', True, 'both')
    first = lambda n: _cuda(*[t[:n].contiguous() for t in (pose, betas, g_verts, g_joints)])
    big, few, one = _bwd(eng, True, *first(130)), _bwd(eng, True, *first(5)), _bwd(eng, True, *first(1))
    gp64, gb64, _, _ = _oracle(130, 'generic', True, 'both', 4)
    for name, a, b in (('g_pose', big[0][:5], few[0]), ('g_betas', big[1][:5], few[1])):
        assert BF.same_bits(a, b), 'N = 130 rows 0..4 differ from the N = 5 call: %s, max|difference| %.3e' % (name, float((a - b).abs().max()))
    for name, a, b, ref in (('g_pose', few[0][:1], one[0], gp64[:1]), ('g_betas', few[1][:1], one[1], gb64[:1])):
        r = float((a - b).abs().max().cpu() / ref.abs().max())
        print('N = 5 row 0 against N = 1: %s max|difference| / max|g64| = %.3e (bit-equal: %s)' % (name, r, BF.same_bits(a, b)))
        assert r <= BOUND, (name, r)


def test_error_returns_come_before_any_device_work():
    _, eng = _module(4, False)
    N = 5
    pose, betas, g_verts, g_joints = _cuda(*_inputs(N, 'generic', True, 'both'))
    need = int(eng.lib.tepose_smpl_bwd_workspace_bytes(eng.handle, N))
    ws = BF.poisoned(need, 'finite', 'cuda', guard_bytes=BF.workspace_guard_bytes(64))
    gp, gb = BF.guarded_like((N, 72), N, 'cuda', name='g_pose'), BF.guarded_like((N, 10), N, 'cuda', name='g_betas')

    def call(pose_=pose, betas_=betas, n=N, gv=g_verts, gj=g_joints, ws_ptr=ws.data_ptr(), ws_bytes=need):
        ptr = lambda t: None if t is None else t.data_ptr()
        return eng.lib.tepose_smpl_bwd(eng.handle, 1, ptr(pose_), ptr(betas_), n, ptr(gv), ptr(gj), gp.data_ptr(), gb.data_ptr(), ws_ptr, ws_bytes, _stream())
    assert call(pose_=None) == E_ARG and call(betas_=None) == E_ARG and call(ws_ptr=None) == E_ARG
    assert call(gv=None, gj=None) == E_ARG
    assert call(n=0) == E_SHAPE and call(n=-3) == E_SHAPE
    assert call(ws_bytes=need - 512) == E_WORKSPACE and call(ws_bytes=0) == E_WORKSPACE
    torch.cuda.synchronize()
    assert BF.untouched(ws), 'a refused call wrote into the workspace'
    assert bool(torch.isnan(gp.own).all()) and bool(torch.isnan(gb.own).all()), 'a refused call wrote an output'
    BF.assert_guards_intact(ws, gp, gb, what='refused smpl_bwd calls')
    assert call() == 0                                                              # and the same arguments, complete, run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gp.own).all()) and bool(torch.isfinite(gb.own).all())


# ---------------------------------------------------------------------------------------------- autograd through SMPL.forward
def _leaves(N, pose_kind='generic', dtype=torch.float32, device='cuda'):
    pose, betas, _, _ = _inputs(N, pose_kind, True, 'both')
    mk = lambda t: t.to(device=device, dtype=dtype).clone().requires_grad_(True)
    return mk(betas), mk(pose[:, 3:]), mk(pose[:, :3])


@pytest.mark.parametrize('N', [1, 5])
def test_autograd_through_the_module(N):
    smpl, _ = _module(4, False)
    pose, betas_np, _, _ = _inputs(N, 'generic', True, 'both')
    ones_v, w_j = torch.ones(N, 6890, 3), _inputs(N, 'generic', True, 'both')[3]
    # .vertices.sum().backward()
    betas, body, orient = _leaves(N)
    out = smpl(betas=betas, body_pose=body, global_orient=orient)
    assert out.vertices.grad_fn is not None and out.joints.grad_fn is not None
    out.vertices.sum().backward()
    gp64, gb64 = GR.grads(GR.tables(4), pose, betas_np, True, ones_v, None)
    got_pose = torch.cat([orient.grad, body.grad], dim=1)
    for name, got, ref in (('g_pose', got_pose, gp64), ('g_betas', betas.grad, gb64)):
        r = GR.rel_err(got.cpu(), ref)
        print('N = %d vertices.sum(): %s ratio %.3e' % (N, name, r))
        assert r <= BOUND, (name, r)
        assert got.device == betas.device and got.dtype == torch.float32
    # a joints-only loss
    betas2, body2, orient2 = _leaves(N)
    out2 = smpl(betas=betas2, body_pose=body2, global_orient=orient2)
    (out2.joints * w_j.cuda()).sum().backward()
    gp64, gb64 = GR.grads(GR.tables(4), pose, betas_np, True, None, w_j)
    for name, got, ref in (('g_pose', torch.cat([orient2.grad, body2.grad], dim=1), gp64), ('g_betas', betas2.grad, gb64)):
        r = GR.rel_err(got.cpu(), ref)
        print('N = %d joints loss: %s ratio %.3e' % (N, name, r))
        assert r <= BOUND, (name, r)
    # a call that asks for no gradient: no graph, the same bits
    plain = smpl(betas=betas.detach(), body_pose=body.detach(), global_orient=orient.detach())
    assert plain.vertices.grad_fn is None and plain.joints.grad_fn is None and not plain.vertices.requires_grad
    assert BF.same_bits(plain.vertices, out.vertices.detach()) and BF.same_bits(plain.joints, out.joints.detach())
    # the module's own default parameters never start a graph
    only_betas = smpl(betas=betas.detach())
    assert only_betas.vertices.grad_fn is None
    with torch.no_grad():
        quiet = smpl(betas=betas, body_pose=body, global_orient=orient)
    assert quiet.vertices.grad_fn is None and quiet.joints.grad_fn is None and BF.same_bits(quiet.vertices, plain.vertices)


def test_rotation_matrix_inputs_cpu_inputs_and_double_backward():
    smpl, _ = _module(4, False)
    N = 2
    pose, betas_np, g_verts, g_joints = _inputs(N, 'generic', False, 'both')
    # pose2rot=False: gradients for the rotation matrices; inputs on the CPU in fp64: gradients come back there, in that dtype
    betas = betas_np.double().clone().requires_grad_(True)
    R = pose.double().clone().requires_grad_(True)
    out = smpl(betas=betas, body_pose=R[:, 1:], global_orient=R[:, :1], pose2rot=False)
    assert out.vertices.device.type == 'cpu' and out.vertices.grad_fn is not None
    ((out.vertices * g_verts.double()).sum() + (out.joints * g_joints.double()).sum()).backward()
    assert R.grad.dtype == torch.float64 and R.grad.device.type == 'cpu' and betas.grad.dtype == torch.float64
    gp64, gb64 = GR.grads(GR.tables(4), pose, betas_np, False, g_verts, g_joints)
    for name, got, ref in (('g_rotmat', R.grad, gp64), ('g_betas', betas.grad, gb64)):
        r = GR.rel_err(got, ref)
        print('rotation matrices, CPU fp64 inputs: %s ratio %.3e' % (name, r))
        assert r <= BOUND, (name, r)
    # second order is not supported: it raises instead of returning something wrong
    b2, body2, orient2 = _leaves(N)
    v = smpl(betas=b2, body_pose=body2, global_orient=orient2).vertices
    (g1,) = torch.autograd.grad(v.sum(), b2, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


def test_forward_and_backward_in_one_captured_graph():
    """Forward plus backward captured on one stream (no side branches) inside Engine.use_workspace, replayed twice: bit-equal to the eager result.  A
    captured graph keeps the workspace address, so both calls run in the caller's tensor: a later, larger call on the same module -- which frees and
    re-allocates the engine's own workspaces -- leaves the replay right, and the engine's own backward workspace is never touched by the capture."""
    smpl, eng = _module(4, False)
    N = 5
    pose, betas_np, _, g_joints = _inputs(N, 'generic', True, 'both')
    w_j = g_joints.cuda()
    betas, body, orient = (t.detach().requires_grad_(True) for t in _leaves(N))

    def step():
        out = smpl(betas=betas, body_pose=body, global_orient=orient)
        loss = out.vertices.sum() + (out.joints * w_j).sum()
        return torch.autograd.grad(loss, [betas, body, orient])
    eager = [g.clone() for g in step()]
    torch.cuda.synchronize()
    need = max(eng.workspace_bytes(max(1, (N + 1) // 2), 1), eng.smpl_bwd_workspace_bytes(N))       # one tensor serves the forward and the backward
    ws = BF.poisoned(need, 'ones', 'cuda', guard_bytes=BF.workspace_guard_bytes(64), name='graph workspace')
    eng._ws_bwd = None                                                               # the capture must not fall back on the engine's own
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), eng.use_workspace(ws):
        step()                                                                       # warm-up on a side stream: the allocator's pools
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with eng.use_workspace(ws), torch.cuda.graph(graph):
        captured = step()
    assert eng._ws_bwd is None, 'the backward inside use_workspace allocated the engine-owned workspace'

    def replays(what):
        for i in range(2):
            for g in captured:
                g.fill_(float('nan'))
            graph.replay()
            torch.cuda.synchronize()
            for name, a, b in zip(('g_betas', 'g_body_pose', 'g_global_orient'), captured, eager):
                assert BF.same_bits(a, b), '%s, replay %d: %s differs from the eager result' % (what, i, name)
        BF.assert_guards_intact(ws, what=what)
    replays('after the capture')
    # a larger call outside the block grows (re-allocates) the engine's own workspaces; the graph does not depend on them
    b2, body2, orient2 = _leaves(130)
    smpl(betas=b2, body_pose=body2, global_orient=orient2).joints.sum().backward()
    torch.cuda.synchronize()
    assert eng._ws_bwd is not None and eng._ws_bwd.numel() >= eng.smpl_bwd_workspace_bytes(130)
    replays('after a larger backward on the same module')


def test_a_caller_owned_workspace_is_never_outgrown_silently():
    smpl, eng = _module(4, False)
    N = 5
    betas, body, orient = _leaves(N)
    small = torch.empty(eng.workspace_bytes(max(1, (N + 1) // 2), 1), dtype=torch.uint8, device='cuda')       # holds the forward, not the backward
    assert small.numel() < eng.smpl_bwd_workspace_bytes(N)
    with eng.use_workspace(small):
        with pytest.raises(RuntimeError, match='too small for the SMPL backward'):
            smpl(betas=betas, body_pose=body, global_orient=orient)                  # refused at the forward, before anything is recorded
        plain = smpl(betas=betas.detach(), body_pose=body.detach(), global_orient=orient.detach())        # no graph asked for: the forward alone fits
    assert plain.vertices.grad_fn is None
    pose, b, g_verts, _ = _cuda(*_inputs(N, 'generic', True, 'both'))
    with pytest.raises(RuntimeError, match='too small for the SMPL backward'):
        eng.smpl_bwd(pose, b, True, g_verts, None, ws=small)
    # pinned at the forward: backward() outside the block still runs in the caller's tensor
    big = torch.empty(eng.smpl_bwd_workspace_bytes(N), dtype=torch.uint8, device='cuda')
    eng._ws_bwd = None
    with eng.use_workspace(big):
        out = smpl(betas=betas, body_pose=body, global_orient=orient)
    out.vertices.sum().backward()
    assert eng._ws_bwd is None and bool(torch.isfinite(betas.grad).all())


# ---------------------------------------------------------------------------------------------- fit_keypoints
def test_fit_keypoints_follows_the_fp64_oracle():
    """Targets: the projected joints of a known (pose, betas, cam) at N = 3; start: the pose perturbed by 0.15 rad noise.  The same loop (fit.fit_loop)
    first runs on the fp64 oracle on the CPU and must at least halve the loss in 20 steps (lr = 0.005 and the perturbation were chosen there: it
    reaches 0.12 of the initial loss, decreasing at every step); the GPU run's history then stays within 1 % of the oracle's at every step and decreases."""
    from tepose_amd import fit
    smpl, _ = _module(4, False)
    g = torch.Generator().manual_seed(5)
    N, steps, lr = 3, 20, 0.005
    pose = 0.3 * torch.randn(N, 72, generator=g)
    betas = 0.5 * torch.randn(N, 10, generator=g)
    cam = torch.tensor([[0.9, 0.05, -0.03]]).repeat(N, 1)
    start = pose + 0.15 * torch.randn(N, 72, generator=g)
    conf = 0.5 + 0.5 * torch.rand(N, 49, generator=g)
    smpl_t = GR.O.smpl_tensors(GR.tables(4), torch.float64)
    oracle_joints = lambda p, b: GR.forward(smpl_t, p, b, True)[1]
    kp_2d = fit.projection(oracle_joints(pose.double(), betas.double()), cam.double())
    start_betas = betas
    ref = fit.fit_loop(oracle_joints, start.double(), start_betas.double(), cam.double(), kp_2d, conf.double(), steps, lr)[3]
    assert ref[-1] <= 0.5 * ref[0] and all(b < a for a, b in zip(ref, ref[1:])), ref
    p1, b1, c1, hist = fit.fit_keypoints(smpl, start.cuda(), start_betas.cuda(), cam.cuda(), kp_2d.float().cuda(), conf.cuda(), steps, lr)
    assert p1.shape == (N, 72) and b1.shape == (N, 10) and c1.shape == (N, 3) and p1.is_cuda and len(hist) == steps
    worst = max(abs(a - b) / b for a, b in zip(hist, ref))
    print('fit_keypoints: loss %.4g -> %.4g (oracle %.4g -> %.4g), worst relative deviation %.2e' % (hist[0], hist[-1], ref[0], ref[-1], worst))
    assert worst <= 0.01, (hist, ref)
    assert all(b < a for a, b in zip(hist, hist[1:])), hist
    # the inputs are not written, and a subset of the parameters can be held
    p2, b2, c2, _ = fit.fit_keypoints(smpl, start.cuda(), start_betas.cuda(), cam.cuda(), kp_2d.float().cuda(), conf.cuda(), 2, lr, optimise=('pose',))
    assert torch.equal(b2.cpu(), start_betas) and torch.equal(c2.cpu(), cam) and not torch.equal(p2.cpu(), start)
