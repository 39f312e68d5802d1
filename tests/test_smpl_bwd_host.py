"""CPU: what of the SMPL backward needs no device -- the two symbols in the header, the loader and the built library; the
argument errors of tepose_smpl_bwd, which all return before any device call; the workspace size (monotone in N, covering the partials of the chosen
launch shapes: tests/c_client/smpl_bwd_shape_check.cpp on the host compiler); the leaf-to-root order of the chain kernel; and the gradient oracle
itself (tests/_smpl_grad_ref.py) against central finite differences of the fp64 forward."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import _smpl_grad_ref as GR
from tepose_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE, E_WORKSPACE, E_STATE = -1, -2, -3, -4


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from tepose_amd import _lib
    return _lib.load()


def test_the_symbols_are_in_the_header_the_loader_and_the_library(lib):
    from tepose_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tepose_amd.h')).read()
    for name in ('tepose_smpl_bwd', 'tepose_smpl_bwd_workspace_bytes'):
        assert name in _lib.SYMBOLS, name
        assert re.search(r'\b%s\s*\(' % name, header), '%s is not declared in include/tepose_amd.h' % name
        assert hasattr(lib, name), name
    m = re.search(r'int tepose_smpl_bwd\(([^;]*)\);', header)
    args = [a.strip().split()[-1].lstrip('*') for a in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]
    assert args == ['m', 'pose2rot', 'pose', 'betas', 'N', 'g_verts', 'g_joints49', 'g_pose', 'g_betas', 'workspace', 'ws_bytes', 'stream']
    assert len(lib.tepose_smpl_bwd.argtypes) == len(args)
    assert lib.tepose_smpl_bwd_workspace_bytes.restype is ctypes.c_size_t


def test_every_argument_error_comes_before_any_device_call(lib):
    h = ctypes.c_void_p()
    assert lib.tepose_create(1, 64, ctypes.byref(h)) == 0
    try:
        P = 4096                  # a non-null pointer value: never dereferenced, every call below returns before a device call
        ok = dict(pose=P, betas=P, N=3, g_verts=P, g_joints=P, g_pose=P, g_betas=P, ws=P, ws_bytes=1 << 40)

        def bwd(pose2rot=1, **kw):
            a = dict(ok, **kw)
            return lib.tepose_smpl_bwd(h, pose2rot, a['pose'], a['betas'], a['N'], a['g_verts'], a['g_joints'], a['g_pose'], a['g_betas'], a['ws'],
                                       a['ws_bytes'], None)
        for k in ('pose', 'betas', 'ws'):
            assert bwd(**{k: None}) == E_ARG, k
        assert lib.tepose_smpl_bwd(None, 1, P, P, 3, P, P, P, P, P, 1 << 40, None) == E_ARG
        # no gradient-in while a gradient-out is asked for
        assert bwd(g_verts=None, g_joints=None) == E_ARG
        assert bwd(g_verts=None, g_joints=None, g_pose=None) == E_ARG and bwd(g_verts=None, g_joints=None, g_betas=None) == E_ARG
        # the shape comes after the pointers, whatever else is wrong
        for n in (0, -1, 65537):
            assert bwd(N=n) == E_SHAPE, n
            assert bwd(N=n, pose=None) == E_ARG and bwd(N=n, g_verts=None, g_joints=None) == E_ARG, n
            assert lib.tepose_smpl_bwd_workspace_bytes(h, n) == 0
        # nothing packed yet: a state error, before the workspace is looked at and before any device access
        assert bwd() == E_STATE and bwd(pose2rot=0, ws_bytes=0) == E_STATE
        assert lib.tepose_smpl_bwd_workspace_bytes(None, 3) == 0
    finally:
        lib.tepose_destroy(h)


def test_the_workspace_size_is_monotone_and_holds_the_backward_buffers(lib):
    for env in ({}, {'TEPOSE_EXACT_FP32': '1'}):
        mp = pytest.MonkeyPatch()
        try:
            for k, v in env.items():
                mp.setenv(k, v)
            h = ctypes.c_void_p()
            assert lib.tepose_create(1, 64, ctypes.byref(h)) == 0
        finally:
            mp.undo()
        try:
            prev = 0
            for n in (1, 2, 4, 5, 8, 9, 31, 32, 33, 64, 65, 130, 450, 511, 512, 513, 768, 769, 8192):
                need = lib.tepose_smpl_bwd_workspace_bytes(h, n)
                assert need > prev, (env, n, need, prev)
                # at least the backward's own buffers: joint sources, g_vposed, the skinning partials (14 workgroups x 24 x 12) and the summed blend product
                assert need >= 4 * n * (54 * 3 + 20672 + 14 * 288 + 224), (env, n)
                prev = need
        finally:
            lib.tepose_destroy(h)


def _run_shape_check(tmp_path, *args):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail('no host C++ compiler (c++ / g++ / clang++) on PATH')
    exe = str(tmp_path / 'smpl_bwd_shape_check')
    if not os.path.isfile(exe):
        p = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'tepose_amd', 'csrc'),
                            os.path.join(ROOT, 'tests', 'c_client', 'smpl_bwd_shape_check.cpp'), '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout.strip().splitlines()[-1]


def test_launch_shapes_and_buffer_sizes_on_the_host(tmp_path):
    assert _run_shape_check(tmp_path) == 'ok 21'


def test_the_bench_tool_restates_the_launch_shape_of_the_header(tmp_path):
    """tools/smpl_backward_bench.py computes its byte floors from the blend backward's split count: its Python restatement against csrc/shapes.h."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('smpl_backward_bench', os.path.join(ROOT, 'tools', 'smpl_backward_bench.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for n in (1, 8, 9, 16, 32, 33, 192, 193, 224, 225, 450, 1000, 8192, 8193, 65536):
        word, pt, splits, skin_blocks, chunks = _run_shape_check(tmp_path, n).split()
        assert word == 'blend' and tool.blend_splits(n) == (int(pt), int(splits)), (n, tool.blend_splits(n), pt, splits)
        assert (tool.SKIN_BLOCKS, tool.CHUNKS) == (int(skin_blocks), int(chunks))


def test_the_chain_order_visits_every_child_before_its_parent(tmp_path):
    trees = {'synthetic': [int(p) for p in synth.SMPL_PARENTS], 'chain': [-1] + list(range(23)), 'star': [-1] + [0] * 23}
    for name, parents in trees.items():
        last = _run_shape_check(tmp_path, *parents)
        assert last.startswith('ok order'), (name, last)
        order = [int(t) for t in last.split()[2:]]
        pos = {j: i for i, j in enumerate(order)}
        assert sorted(order) == list(range(24)) and all(pos[j] < pos[parents[j]] for j in range(1, 24)), name
    assert order[-1] == 0
    chain = [int(t) for t in _run_shape_check(tmp_path, *trees['chain']).split()[2:]]
    assert chain == list(range(23, -1, -1))                                   # the degenerate chain: 23 levels, one joint each


def test_the_gradient_oracle_agrees_with_central_differences():
    """20 random directions at N = 2, relative 1e-6: L = <g_verts, verts> + <g_joints, joints> of the fp64 forward, (L(x + h d) - L(x - h d)) / 2h against
    <grad, d>.  h = 1e-5: truncation ~h^2 |L'''| and rounding ~1e-16 |L| / h are both far below 1e-6 of the derivative."""
    smpl_np = GR.tables(4)
    smpl_t = GR.O.smpl_tensors(smpl_np, torch.float64)
    g = torch.Generator().manual_seed(11)
    N, h = 2, 1e-5
    for pose2rot in (True, False):
        aa = 0.5 * torch.randn(N, 72, generator=g, dtype=torch.float64)
        aa[0, 3:6] = 0.0                                                       # the oracle's own aa = 0 branch: angle = |1e-8|
        pose = aa if pose2rot else GR.O.batch_rodrigues(aa.reshape(-1, 3)).view(N, 24, 3, 3)
        betas = torch.randn(N, 10, generator=g, dtype=torch.float64)
        g_verts = torch.randn(N, 6890, 3, generator=g, dtype=torch.float64)
        g_joints = torch.randn(N, 49, 3, generator=g, dtype=torch.float64)
        g_pose, g_betas = GR.grads(smpl_np, pose, betas, pose2rot, g_verts, g_joints)

        def L(p, b):
            verts, joints = GR.forward(smpl_t, p, b, pose2rot)
            return float((g_verts * verts).sum() + (g_joints * joints).sum())
        worst = 0.0
        for _ in range(20):
            dp = torch.randn(pose.shape, generator=g, dtype=torch.float64)
            db = torch.randn(betas.shape, generator=g, dtype=torch.float64)
            fd = (L(pose + h * dp, betas + h * db) - L(pose - h * dp, betas - h * db)) / (2 * h)
            an = float((g_pose * dp).sum() + (g_betas * db).sum())
            worst = max(worst, abs(fd - an) / abs(an))
        print('pose2rot = %s: worst relative difference to central differences %.2e' % (pose2rot, worst))
        assert worst <= 1e-6, (pose2rot, worst)
        # a gradient-in left out is a zero gradient-in
        gp_v, gb_v = GR.grads(smpl_np, pose, betas, pose2rot, g_verts, None)
        gp_j, gb_j = GR.grads(smpl_np, pose, betas, pose2rot, None, g_joints)
        assert GR.rel_err(gp_v + gp_j, g_pose) < 1e-12 and GR.rel_err(gb_v + gb_j, g_betas) < 1e-12
