"""GPU: what a forward may read and write in the buffers it is given (include/tepose_amd.h, conventions):

  * its results depend only on its inputs and the packed weights, not on what the workspace held before;
  * it writes only inside [workspace, workspace + bytes) and inside the first B rows of each output, and never its inputs.

Per case one model, built once, run through Engine.use_workspace(...) with the caller's `out=` tensors (tests/_buffers.py: poisoned workspaces and
guarded outputs, views into the middle of larger allocations):

  a. baseline  two runs on a zero-filled workspace are bit-identical (else the family is not REPEATABLE: reported as that), and the second one is
               within the suite's tolerances of the fp64 oracle (2e-5 features, 1e-4 verts / kp_3d / kp_2d / rotmat) -- on every row where
               B * H <= 150000, else on the fuzz test's edge and sample rows;
  b. poison    the same forward on an all-0xFF workspace (NaN as fp32 and fp16, all-ones as a counter / tag / index) and on a 0x3C00 one (1.0 as
               fp16, small finite fp32): torch.equal to (a), for every output and the encoder features of both modes;
  c. residue   in ONE workspace sized for the larger of two shapes: (c1) the forward, and the encoder in each mode, each DIRECTLY after a forward of
               other windows at the same shape (another seed, features x 1e4) -- the granules and counters that forward left carry the very tags and
               counts this one waits for; (c2) a forward at a shape of another batch class (compared with its own zeros-workspace run), then the case's
               forward and encoder: torch.equal to (a);
  d. confinement  after every run all guards (workspace, five outputs, feature) are intact and the inputs bitwise unchanged;
  e. no accidental pass  warnings are errors; after each run tepose_forward_status == 0, tepose_status_peek == 0, uses_persistent(B) unchanged, the
               handle not degraded (a persistent launch that gave up and was re-run on the step kernels would otherwise pass (b) for the wrong reason).

CASES are the smallest shapes that reach each kernel family of csrc/plan.hip; tests/test_buffers_helper.py checks that they reach all of them.  The
other entry points that take a workspace follow below, at one or two small shapes each."""
import os
import warnings

import numpy as np
import pytest
import torch

import _buffers as BF
from tepose_amd import synth

pytestmark = pytest.mark.gpu
TOL, TOL_FEAT = 1e-4, 2e-5
_NC = {'TEPOSE_COLLAPSE_REGRESSOR': '0'}

# (L, H, B, T, knobs)
CASES = [
    (2, 256, 4, 6, {}),          # granule-mode persistent kernel, in-kernel first step, one-launch SMPL
    (1, 256, 3, 5, {}),          # the same on one layer
    (2, 256, 5, 6, {}),          # counter-mode persistent kernel, one row tile
    (2, 256, 64, 3, {}),         # ... four row tiles, tiled layer-0 projection
    (2, 100, 9, 4, {}),          # Hp > H padding, step-per-launch width-first kernels (H = 100 cannot run persistent)
    (2, 128, 100, 1, {}),        # T = 1, first steps only
    (2, 128, 129, 6, {}),        # gemm_h3_kernel<GRU>, ragged tile of one row
    (2, 1024, 129, 4, {}),       # 128 x 288 mid tiles (no smaller width selects them), 90 MiB
    (2, 64, 300, 32, {}),        # barrier-free layer-0 projection feeding two-accumulator steps
    (2, 192, 700, 3, {}),        # scaled class just above its threshold, Hp % 128 != 0
    (1, 64, 1000, 2, {}),        # scaled, one layer
    (2, 64, 1024, 6, {}),        # fp32-state layer 0, plane-fed layer 1
    (2, 64, 2048, 4, {}),        # frame-major blocked, plane-fed steps on both layers
    (3, 64, 2064, 4, {}),        # frame-major blocked, fp32-state steps, ragged 16-row tile
    (2, 64, 2050, 5, {}),        # B % 16 != 0, row-major layer 0 under blocked layer 1
    (2, 128, 2305, 3, {}),       # gru_first16_kernel, ragged tile of one row in the scaled class
    (2, 128, 200, 3, {'TEPOSE_EXACT_FP32': '1'}),      # exact fp32, width-first kernels
    (2, 64, 800, 2, {'TEPOSE_EXACT_FP32': '1'}),       # exact fp32, tiled kernels (B > 768)
    (2, 64, 1024, 3, {'TEPOSE_GRU_STATE': 'fp32'}),    # fp32-state steps where the default plan feeds planes
    (2, 64, 700, 3, {'TEPOSE_LARGE_BATCH_KERNELS': 'twoacc'}),
    (2, 256, 4, 6, _NC),         # reg_seq_kernel behind the granule-mode recurrence
    (2, 64, 70, 2, _NC),         # the regressor as a loop of products
]
IDS = ['L%dH%dB%dT%d%s' % (c[0], c[1], c[2], c[3], ''.join('-' + k.replace('TEPOSE_', '').lower() + v for k, v in c[4].items())) for c in CASES]
OUT_KEYS = ('theta', 'verts', 'kp_3d', 'kp_2d', 'rotmat')
NAMES = OUT_KEYS + ('feature', 'feature_train')


@pytest.fixture(scope='module')
def smpl_np():
    return synth.synthetic_smpl(0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _model(L, H, knobs, smpl_np, monkeypatch, seed=17):
    from tepose_amd.testing import build_model
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)             # read when the handle is created
    model, state, _ = build_model(L, H, seed=seed, device='cuda', smpl_np=smpl_np)
    for k in knobs:
        monkeypatch.delenv(k)
    eng = model._engine
    eng.pack_encoder(model.encoder, torch.device('cuda', torch.cuda.current_device()))
    eng.pack_regressor(model.regressor, torch.device('cuda', torch.cuda.current_device()))
    return model, state, eng


def _Hp(H):
    return (H + 63) // 64 * 64


def _windows(B, T, seed, scale=1.0):
    x = synth.synthetic_windows(B, T, seed)
    if scale != 1.0:
        x[:, :, :2048] *= scale
    return torch.from_numpy(x).cuda()


def _outs(B, nj=14):
    tails = {'theta': (85,), 'verts': (6890, 3), 'kp_3d': (nj, 3), 'kp_2d': (nj, 2), 'rotmat': (24, 3, 3)}
    return {k: BF.guarded_like((B,) + t, B, 'cuda', name=k) for k, t in tails.items()}


def _nan_rows(outs):
    for t in outs.values():
        t.own.view(torch.int32).fill_(-1)             # a row the forward leaves out shows as NaN, not as the previous run's answer


class Runner:
    """One model's entry points on caller-owned buffers, with checks (d) and (e) after every run."""

    def __init__(self, eng, J):
        self.eng, self.lib, self.J = eng, eng.lib, J

    def settled(self, ws, B, persistent, frozen, guarded, what, status=True):
        torch.cuda.synchronize()
        if status:
            assert self.lib.tepose_forward_status(self.eng.handle, ws.data_ptr(), _stream()) == 0, what + ': the forward gave up (TEPOSE_E_TIMEOUT)'
        assert self.lib.tepose_status_peek(self.eng.handle) == 0, what + ': the handle carries a fault'
        assert self.eng.uses_persistent(B) == persistent and not self.eng.degraded, what + ': the handle was switched to the step-per-launch kernels'
        BF.assert_guards_intact(ws, guarded, what=what)
        frozen.assert_unchanged(what)
        assert not BF.untouched(ws), what + ': the workspace was not used at all (the poison would prove nothing)'

    def forward(self, x, ws, outs, what):
        B = x.shape[0]
        frozen, persistent = BF.Frozen(x=x), self.eng.uses_persistent(B)
        _nan_rows(outs)
        with self.eng.use_workspace(ws):
            res = self.eng.forward(x, self.J, out=outs)
        self.settled(ws, B, persistent, frozen, outs, what)
        for k in OUT_KEYS:
            assert res[k].data_ptr() == outs[k].data_ptr() and res[k].shape[0] == B
        return {k: res[k].clone() for k in OUT_KEYS}

    def encoder(self, x, is_train, ws, what):
        B, T = x.shape[:2]
        frozen, persistent = BF.Frozen(x=x), self.eng.uses_persistent(B)
        feat = BF.guarded_like((B, 2, 2048) if is_train else (B, 2048), B, 'cuda', name='feature')
        rc = self.lib.tepose_encoder_fwd(self.eng.handle, x.data_ptr(), B, T, int(is_train), feat.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, (what, rc)
        self.settled(ws, B, persistent, frozen, feat, what)
        return feat.own.clone()

    def all(self, x, ws, outs, pattern, what):
        """The full forward and the encoder in both modes, each on the workspace freshly filled with `pattern`."""
        got = self.forward(x, BF.refill(ws, pattern), outs, '%s, forward, %s workspace' % (what, pattern))
        got['feature'] = self.encoder(x, False, BF.refill(ws, pattern), '%s, encoder, %s workspace' % (what, pattern))
        got['feature_train'] = self.encoder(x, True, BF.refill(ws, pattern), '%s, encoder (is_train), %s workspace' % (what, pattern))
        return got


def _assert_same(got, base, what):
    for k, v in base.items():
        assert BF.same_bits(got[k], v), '%s: %s differs from the baseline on a zero-filled workspace (max |diff| %.3e, %d of %d elements)' % (
            what, k, float((got[k].double() - v.double()).abs().nan_to_num(nan=float('inf')).max()), int((got[k] != v).sum()), v.numel())


def oracle_rows(B, H):
    """Every row where B * H <= 150000; else the fuzz test's rows: both ends of the batch (the first and the last row tile's edges) and a sample."""
    return np.arange(B) if B * H <= 150000 else np.unique(np.r_[0:24, B - 24:B, np.random.RandomState(B).randint(0, B, 48)])


@pytest.mark.parametrize('case', range(len(CASES)), ids=IDS)
def test_forward_ignores_the_workspace_contents_and_stays_in_its_buffers(case, smpl_np, monkeypatch):
    from oracle import tepose_ref as O
    L, H, B, T, knobs = CASES[case]
    what = IDS[case]
    model, state, eng = _model(L, H, knobs, smpl_np, monkeypatch)
    Jn = smpl_np['J_regressor_h36m']
    run = Runner(eng, torch.from_numpy(Jn))
    x = _windows(B, T, 900 + case)
    gb = BF.workspace_guard_bytes(_Hp(H))
    need = eng.workspace_bytes(B, T)
    outs = _outs(B)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ws = BF.poisoned(need, 'zeros', 'cuda', gb)
        # ---- a. baseline: repeatable, and right
        first = run.all(x, ws, outs, 'zeros', what)
        base = run.all(x, ws, outs, 'zeros', what)
        for k in NAMES:
            assert BF.same_bits(first[k], base[k]), '%s: NOT REPEATABLE -- two runs on a zero-filled workspace differ in %s' % (what, k)
        rows = oracle_rows(B, H)
        xr = x[torch.from_numpy(rows).cuda()].cpu().numpy()
        ref = O.tepose_fwd(state, smpl_np, xr, L, J_regressor=Jn, dtype=torch.float64)
        enc, _ = O.split_state_dict(state, torch.float64)
        with torch.no_grad():
            ref['feature'] = O.encoder_fwd(enc, torch.from_numpy(xr).double(), L)
            ref['feature_train'] = O.encoder_fwd(enc, torch.from_numpy(xr).double(), L, is_train=True)
        errs = {}
        for k in ('feature', 'feature_train', 'verts', 'kp_3d', 'kp_2d', 'rotmat'):
            assert torch.isfinite(base[k]).all(), (what, k)
            errs[k] = float((base[k][torch.from_numpy(rows).cuda()].cpu().double() - ref[k].reshape(base[k][:len(rows)].shape)).abs().max())
        print('\n  %s: %d of %d rows against fp64: %s' % (what, len(rows), B, ', '.join('%s %.2e' % kv for kv in errs.items())))
        for k, e in errs.items():
            assert e < (TOL_FEAT if k.startswith('feature') else TOL), (what, k, e)
        # ---- b. poison
        for pattern in ('ones', 'finite'):
            _assert_same(run.all(x, ws, outs, pattern, what), base, '%s, %s workspace' % (what, pattern))
        del ws
        # ---- c. residue of other forwards in one workspace sized for the larger of two shapes
        B2, T2 = (200, 3) if B <= 64 else (3, 4)              # another batch class: big then small, small then big
        other, x2, outs2 = _windows(B, T, 1900 + case, 1e4), _windows(B2, T2, 2900 + case, 1e4), _outs(B2)
        ws = BF.poisoned(max(need, eng.workspace_bytes(B2, T2)), 'zeros', 'cuda', gb)
        base2 = run.forward(x2, ws, outs2, what + ', the other shape (%d x %d), zeros workspace' % (B2, T2))
        # c1. DIRECTLY after a forward of other windows at the same shape, nothing in between: every counter, status word and granule that forward left
        #     (granules carry exactly the tags this one waits for: layer * 64 + step + 1) lies where this one looks -- once per entry point
        got = {}
        for name, entry in (('forward', lambda: run.forward(x, ws, outs, what + ', forward right after other windows at the same shape')),
                            ('feature', lambda: run.encoder(x, False, ws, what + ', encoder right after other windows at the same shape')),
                            ('feature_train', lambda: run.encoder(x, True, ws, what + ', encoder (is_train) right after other windows at the same shape'))):
            run.forward(other, ws, outs, what + ', other windows at the same shape')
            r = entry()
            got.update(r if name == 'forward' else {name: r})
        _assert_same(got, base, what + ', residue of other windows at the same shape')
        # c2. a forward at the other shape on that residue (against its own zeros-workspace run), then the case's forward on the other shape's
        _assert_same(run.forward(x2, ws, outs2, what + ', the other shape (%d x %d) after the case\'s' % (B2, T2)), base2, what + ', the other shape on residue')
        got = run.forward(x, ws, outs, what + ', after a forward at the other shape')
        got['feature'] = run.encoder(x, False, ws, what + ', encoder after the forwards')
        got['feature_train'] = run.encoder(x, True, ws, what + ', encoder (is_train) after the forwards')
        _assert_same(got, base, what + ', residue of a forward at the other shape')
    print('  %s: outputs and features bit-identical on zeros / ones / finite / residue workspaces (%d bytes); guards intact, no give-up' % (what, need))


# ---- the other entry points that take a workspace ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def small(smpl_np):
    """L = 1, H = 64: regressor and SMPL entry points."""
    mp = pytest.MonkeyPatch()
    try:
        return _model(1, 64, {}, smpl_np, mp, seed=23)
    finally:
        mp.undo()


def _patterns_agree(call, sizes, gb, what, residue=None):
    """call(ws, what) -> dict of tensors, on zeros twice (repeatable), ones, finite, and -- residue: one callable(ws) or a list of them -- directly
    after each of those other calls in ONE workspace sized for all of them."""
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ws = BF.poisoned(sizes[0], 'zeros', 'cuda', gb)
        first = call(ws, what + ', zeros workspace')
        base = call(BF.refill(ws, 'zeros'), what + ', zeros workspace')
        for k in base:
            assert BF.same_bits(first[k], base[k]), '%s: NOT REPEATABLE -- two runs on a zero-filled workspace differ in %s' % (what, k)
        for pattern in ('ones', 'finite'):
            _assert_same(call(BF.refill(ws, pattern), '%s, %s workspace' % (what, pattern)), base, '%s, %s workspace' % (what, pattern))
        if residue is not None:
            ws = BF.poisoned(max(sizes), 'zeros', 'cuda', gb)
            for i, r in enumerate(residue if isinstance(residue, (list, tuple)) else [residue]):
                r(ws)
                _assert_same(call(ws, '%s, after another call (%d) in the same workspace' % (what, i)), base, '%s, residue %d' % (what, i))
    return base


@pytest.mark.parametrize('N', [1, 17, 200])
def test_regressor_with_per_call_initial_state(N, small, smpl_np):
    model, state, eng = small
    run = Runner(eng, None)
    _, jp = eng.jreg(torch.from_numpy(smpl_np['J_regressor_h36m']), torch.device('cuda', torch.cuda.current_device()))

    def inputs(n, seed):
        g = torch.Generator().manual_seed(seed)
        return [t.cuda() for t in (torch.randn(n, 2048, generator=g), 0.3 * torch.randn(n, 144, generator=g), 0.5 * torch.randn(n, 10, generator=g),
                                   torch.tensor([0.9, 0.0, 0.0]) + 0.1 * torch.randn(n, 3, generator=g))]

    def call_n(n, ins, outs):
        def call(ws, what):
            feat, ip, ish, ic = ins
            frozen, persistent = BF.Frozen(feat=feat, init_pose=ip, init_shape=ish, init_cam=ic), eng.uses_persistent(n)
            _nan_rows(outs)
            rc = eng.lib.tepose_regressor_fwd_init(eng.handle, feat.data_ptr(), n, 3, ip.data_ptr(), ish.data_ptr(), ic.data_ptr(), jp, outs['theta'].data_ptr(),
                                                   outs['verts'].data_ptr(), outs['kp_3d'].data_ptr(), outs['kp_2d'].data_ptr(), outs['rotmat'].data_ptr(),
                                                   ws.data_ptr(), ws.numel(), _stream())
            assert rc == 0, (what, rc)
            run.settled(ws, n, persistent, frozen, outs, what)
            return {k: outs[k].own.clone() for k in OUT_KEYS}
        return call

    N2 = 3 if N == 200 else 200
    size = lambda n: eng.workspace_bytes(max(1, (n + 1) // 2), 1)        # what Engine.regressor_fwd asks for
    same, other = call_n(N, inputs(N, 99), _outs(N)), call_n(N2, inputs(N2, 77), _outs(N2))     # other inputs at the same N (reg_seq_kernel's counters), another N
    base = _patterns_agree(call_n(N, inputs(N, 70 + N), _outs(N)), (size(N), size(N2)), BF.workspace_guard_bytes(64), 'regressor_fwd N = %d' % N,
                           residue=[lambda ws: same(ws, 'regressor_fwd N = %d, other inputs' % N), lambda ws: other(ws, 'regressor_fwd N = %d' % N2)])
    assert all(torch.isfinite(v).all() for v in base.values())


@pytest.mark.parametrize('N', [3, 70])
@pytest.mark.parametrize('pose2rot', [True, False])
def test_smpl_fwd(pose2rot, N, small):
    model, state, eng = small
    run = Runner(eng, None)

    def make(n, seed):
        g = torch.Generator().manual_seed(seed)
        aa = 0.4 * torch.randn(n, 72, generator=g)
        pose = aa if pose2rot else torch.linalg.qr(torch.randn(n, 24, 3, 3, generator=g)).Q.contiguous()
        verts, joints = BF.guarded_like((n, 6890, 3), n, 'cuda', name='verts'), BF.guarded_like((n, 49, 3), n, 'cuda', name='joints')
        pose, betas = pose.cuda(), torch.randn(n, 10, generator=g).cuda()

        def call(ws, what):
            frozen = BF.Frozen(pose=pose, betas=betas)
            _nan_rows({'verts': verts, 'joints': joints})
            rc = eng.lib.tepose_smpl_fwd(eng.handle, int(pose2rot), pose.data_ptr(), betas.data_ptr(), n, verts.data_ptr(), joints.data_ptr(), ws.data_ptr(),
                                         ws.numel(), _stream())
            assert rc == 0, (what, rc)
            # (no status words of its own: this entry point launches no persistent kernel)
            run.settled(ws, n, eng.uses_persistent(n), frozen, [verts, joints], what, status=False)
            return {'verts': verts.own.clone(), 'joints': joints.own.clone()}
        return call

    N2 = 3 if N == 70 else 70
    size = lambda n: eng.workspace_bytes(max(1, (n + 1) // 2), 1)        # what Engine.smpl_fwd asks for
    same, other = make(N, 6), make(N2, 5)
    base = _patterns_agree(make(N, 40 + N), (size(N), size(N2)), BF.workspace_guard_bytes(64), 'smpl_fwd pose2rot = %s N = %d' % (pose2rot, N),
                           residue=[lambda ws: same(ws, 'smpl_fwd N = %d, other poses' % N), lambda ws: other(ws, 'smpl_fwd N = %d' % N2)])
    assert all(torch.isfinite(v).all() for v in base.values())


@pytest.fixture(scope='module')
def clip_model(smpl_np):
    """L = 2, H = 256: the cached window path and the frame projections."""
    mp = pytest.MonkeyPatch()
    try:
        return _model(2, 256, {}, smpl_np, mp, seed=29)
    finally:
        mp.undo()


def test_cached_window_path_through_run_clips(clip_model, smpl_np):
    """Five ragged clips at T = 6 with the projection cache: tepose_project_frames, tepose_window_step and tepose_forward_cached under use_workspace.
    The residue run is the same driver on other clips (features x 1e4) of other lengths in the same workspace.  run_clips allocates its result
    buffers, ring and pair workspace itself: those are neither poisoned nor guarded here (tests/test_gpu_buffers.py::test_frame_projections does that
    for the projections); the forward's workspace is."""
    from tepose_amd.driver import run_clips
    model, state, eng = clip_model
    T, lens = 6, [11, 9, 9, 7, 6]
    w = synth.synthetic_windows(5, max(lens), 61)
    feats = [torch.from_numpy(w[c, :lens[c], :2048].copy()) for c in range(5)]
    inits = [torch.from_numpy(w[c, :T - 1, 2048:].copy()) for c in range(5)]
    J = torch.from_numpy(smpl_np['J_regressor_h36m'])
    need = max(eng.workspace_bytes(b, T) for b in range(1, 6))

    def call(ws, what):
        persistent = [eng.uses_persistent(b) for b in range(1, 6)]
        with eng.use_workspace(ws):
            res = run_clips(model, feats, inits, T, J_regressor=J, cache_projections=True)
        torch.cuda.synchronize()
        assert eng.lib.tepose_status_peek(eng.handle) == 0 and not eng.degraded and persistent == [eng.uses_persistent(b) for b in range(1, 6)], what
        BF.assert_guards_intact(ws, what=what)
        assert not BF.untouched(ws), what + ': use_workspace did not reach the driver\'s forwards'
        return {'%s[%d]' % (k, c): res[c][k] for c in range(5) for k in res[c]}

    def residue(ws):
        other = synth.synthetic_windows(5, 8, 62)
        other[:, :, :2048] *= 1e4
        with eng.use_workspace(ws):
            run_clips(model, [torch.from_numpy(other[c, :, :2048].copy()) for c in range(5)], [torch.from_numpy(other[c, :T - 1, 2048:].copy()) for c in range(5)],
                      T, J_regressor=J, cache_projections=True)

    base = _patterns_agree(call, (need,), BF.workspace_guard_bytes(256), 'run_clips, 5 ragged clips', residue=residue)
    assert all(torch.isfinite(v).all() for v in base.values())


@pytest.mark.parametrize('B', [3, 37, 500])
def test_frame_projections(B, clip_model):
    """eng.project_frames and eng.project_frame_pair with a poisoned, guarded pair workspace; the rows next to the written ring / newest rows are guards.
    Residue: the same projection of other frames (x 1e4) at the same B, and one at another B (500 then 3, 3 then 500), in one shared workspace."""
    model, state, eng = clip_model
    W = eng.gate_width
    run = Runner(eng, None)

    def make(b, seed, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        fp, fn = (scale * torch.randn(b, 2048, generator=g)).cuda(), (scale * torch.randn(b, 2048, generator=g)).cuda()
        th = torch.randn(b, 85, generator=g).cuda()
        o1, o2, o3 = (BF.guarded_like((b, W), b, 'cuda', name=n) for n in ('ring slot', 'newest', 'ring slot (one product)'))

        def pair(ws, what):
            frozen = BF.Frozen(feat_prev=fp, feat_new=fn, theta=th)
            _nan_rows({'a': o1, 'b': o2})
            eng.project_frame_pair(fp.data_ptr(), fn.data_ptr(), 2048, th.data_ptr(), 85, b, o1.data_ptr(), W, o2.data_ptr(), W, ws)
            run.settled(ws, b, eng.uses_persistent(b), frozen, [o1, o2], what, status=False)     # (no status words: no persistent kernel here)
            return {'prev': o1.own.clone(), 'new': o2.own.clone()}

        def single(ws, what):
            frozen = BF.Frozen(feat_prev=fp, theta=th)
            _nan_rows({'c': o3})
            eng.project_frames(fp.data_ptr(), 2048, th.data_ptr(), 85, b, o3.data_ptr(), W, ws)
            run.settled(ws, b, eng.uses_persistent(b), frozen, [o3], what, status=False)
            return {'prev': o3.own.clone()}
        return pair, single

    B2 = 3 if B == 500 else 500
    size = lambda b: int(eng.lib.tepose_project_frames_workspace_bytes(eng.handle, b))
    (pair, single), (pair_s, single_s), (pair_o, single_o) = make(B, B), make(B, B + 1000, 1e4), make(B2, B + 2000, 1e4)
    gb = BF.workspace_guard_bytes(256)
    both = _patterns_agree(pair, (size(2 * B), size(2 * B2)), gb, 'project_frame_pair B = %d' % B,
                           residue=[lambda ws: pair_s(ws, 'project_frame_pair B = %d, other frames' % B), lambda ws: pair_o(ws, 'project_frame_pair B = %d' % B2)])
    one = _patterns_agree(single, (size(B), size(B2)), gb, 'project_frames B = %d' % B,
                          residue=[lambda ws: single_s(ws, 'project_frames B = %d, other frames' % B), lambda ws: single_o(ws, 'project_frames B = %d' % B2)])
    assert all(torch.isfinite(v).all() for v in list(both.values()) + list(one.values()))


@pytest.mark.parametrize('L,H,B,N,bidir', [(2, 128, 2, 20, False), (2, 64, 2, 7, True)])
def test_vibe_encoder(L, H, B, N, bidir, smpl_np):
    """tepose_vibe_encoder_fwd called directly as Engine.vibe_encoder_fwd does (that method allocates its own workspace).  Residue: other frames
    (x 1e4) at the same (B, N), and another (B, N) = (3, 5), in one shared workspace."""
    from test_gpu_vibe import _build
    model, _ = _build(L, H, 31, smpl_np, bidirectional=bidir)
    eng = model._engine
    x = torch.from_numpy(synth.synthetic_windows(B, N, 32)[:, :, :2048].copy()).cuda()
    eng.pack_vibe_encoder(model.encoder, x.device)
    D = int(eng.lib.tepose_vibe_feature_dim(eng.handle))
    run = Runner(eng, None)

    def make(x):
        b, n = x.shape[:2]
        feat = BF.guarded_like((b * n, D), b * n, 'cuda', name='feature')

        def call(ws, what):
            frozen = BF.Frozen(x=x)
            _nan_rows({'f': feat})
            rc = eng.lib.tepose_vibe_encoder_fwd(eng.handle, x.data_ptr(), b, n, 1, feat.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
            assert rc == 0, (what, rc)
            run.settled(ws, b, eng.uses_persistent(b), frozen, feat, what, status=False)
            return {'feature': feat.own.clone()}
        return call

    same = make(torch.from_numpy(1e4 * synth.synthetic_windows(B, N, 33)[:, :, :2048]).contiguous().cuda())
    other = make(torch.from_numpy(1e4 * synth.synthetic_windows(3, 5, 34)[:, :, :2048]).contiguous().cuda())
    size = lambda b, n: int(eng.lib.tepose_vibe_workspace_bytes(eng.handle, b, n))
    base = _patterns_agree(make(x), (size(B, N), size(3, 5)), BF.workspace_guard_bytes(_Hp(H)), 'vibe encoder L = %d H = %d bidirectional = %s' % (L, H, bidir),
                           residue=[lambda ws: same(ws, 'vibe encoder, other frames'), lambda ws: other(ws, 'vibe encoder B = 3 N = 5')])
    with torch.no_grad():
        assert torch.equal(base['feature'].view(B, N, D), model.encoder(x))


@pytest.mark.parametrize('mode', ['split', 'exact'])
def test_hmr_features(mode):
    """hmr_features honours use_workspace: N = 3 in both numerics modes of tests/test_gpu_hmr.py (the model and its features are that module's).
    Residue: other images (the fixture's, reversed and x 50) at N = 3, and N = 5 of them, in one shared workspace.  The feature tensor is allocated
    by Engine.hmr_features itself: it is not guarded here; the workspace is poisoned and guarded."""
    import test_gpu_hmr as TH
    model, x, feat = TH.build(mode)
    eng = model._engine

    def make(x):
        def call(ws, what):
            frozen = BF.Frozen(x=x)
            with eng.use_workspace(ws), torch.no_grad():
                got = model.feature_extractor(x)
            torch.cuda.synchronize()
            assert eng.lib.tepose_status_peek(eng.handle) == 0, what
            BF.assert_guards_intact(ws, what=what)
            frozen.assert_unchanged(what)
            assert not BF.untouched(ws), what + ': use_workspace did not reach hmr_features'
            return {'feature': got}
        return call

    xo = (50.0 * x.flip(0)).contiguous()
    same, other = make(xo), make(xo[torch.arange(5, device=x.device) % 3].contiguous())
    size = lambda n: int(eng.lib.tepose_hmr_workspace_bytes(eng.handle, n))
    # the widest rows of the backbone's workspace: 2048 channels
    base = _patterns_agree(make(x), (size(3), size(5)), BF.GUARD_ROWS * 2048 * 4, 'hmr_features (%s)' % mode,
                           residue=[lambda ws: same(ws, 'hmr_features, other images'), lambda ws: other(ws, 'hmr_features N = 5')])
    assert torch.equal(base['feature'], feat)


_GEMM_SHAPES = [(129, 96, 64), (2305, 864, 2144)]


@pytest.mark.parametrize('M,N,K', _GEMM_SHAPES)
@pytest.mark.parametrize('kernel', ['f32', 'h3s=0', 'h3s=1', 'h3s=mid'])
def test_gemm_entry_points(kernel, M, N, K, monkeypatch):
    """tepose_gemm_f32 and tepose_gemm_h3_f32 (TEPOSE_H3S = 0, 1, mid) at ragged M: C's rows are guarded, ldc > N, and the gap columns are guards too.
    Residue: the same product on other operands, and the product of the other shape of the table, in one shared workspace."""
    from tepose_amd import _lib
    lib = _lib.load()
    if kernel != 'f32':
        monkeypatch.setenv('TEPOSE_H3S', kernel.split('=')[1])

    def make(M, N, K, seed):
        if kernel == 'h3s=mid' and N % 288:
            N = 288                                           # the 128 x 288-tile kernel takes whole column tiles only
        g = torch.Generator().manual_seed(seed)
        # (operand ranges of tests/test_gpu_stress.py: |a| * 256 and |w| * 16384 stay below 65504, the scaled kernels' fp16 range)
        A, W, b = (3.0 * torch.randn(M, K, generator=g)).cuda(), (0.05 * torch.randn(N, K, generator=g)).cuda(), torch.randn(N, generator=g).cuda()
        ldc = N + 32
        C = BF.guarded_like((M, ldc), M, 'cuda', name='C')

        def call(ws, what):
            frozen = BF.Frozen(A=A, W=W, bias=b)
            _nan_rows({'C': C})
            if kernel == 'f32':
                rc = lib.tepose_gemm_f32(A.data_ptr(), K, W.data_ptr(), K, b.data_ptr(), C.data_ptr(), ldc, M, N, K, 0, ws.data_ptr(), ws.numel(), _stream())
            else:
                rc = lib.tepose_gemm_h3_f32(A.data_ptr(), K, W.data_ptr(), K, b.data_ptr(), C.data_ptr(), ldc, M, N, K, ws.data_ptr(), ws.numel(), _stream())
            assert rc == 0, (what, rc)
            torch.cuda.synchronize()
            BF.assert_guards_intact(ws, C, what=what)
            frozen.assert_unchanged(what)
            assert not BF.untouched(ws), what + ': the workspace was not used at all'
            assert bool((C.own[:, N:].contiguous().view(torch.int32) == -1).all()), what + ': the gap columns [N, ldc) of C were written'
            return {'C': C.own[:, :N].clone()}
        need = int(lib.tepose_gemm_workspace_bytes(N, K) if kernel == 'f32' else lib.tepose_gemm_h3_workspace_bytes(M, N, K))
        return call, need, (A, W, b), (M, N, K)

    M2, N2, K2 = [sh for sh in _GEMM_SHAPES if sh != (M, N, K)][0]
    (call, need, (A, W, b), (M, N, K)), (same, _, _, _), (other, need2, _, _) = make(M, N, K, M + N), make(M, N, K, M + N + 1), make(M2, N2, K2, M2 + N2 + 2)
    base = _patterns_agree(call, (need, need2), BF.GUARD_ROWS * max(N, K, N2, K2) * 4, 'gemm %s M = %d N = %d K = %d' % (kernel, M, N, K),
                           residue=[lambda ws: same(ws, 'gemm %s, other operands' % kernel), lambda ws: other(ws, 'gemm %s M = %d' % (kernel, M2))])
    ref = A.double() @ W.double().t() + b.double()
    mag = float((A.double().abs() @ W.double().abs().t()).max()) + 1.0
    assert float((base['C'].double() - ref).abs().max()) < 3e-6 * mag          # the bound tests/test_gpu_stress.py holds these entry points to
