#!/usr/bin/env python3
"""Bit-level A/B of two builds of the library: per case the kernel plan (tepose_select_kernels) and a SHA-256 of every output tensor's bytes.

  TEPOSE_AMD_LIB=<parent.so> python tools/output_digest.py > parent.txt
  python tools/output_digest.py > new.txt && diff parent.txt new.txt

The cases are the smallest shapes at which each kernel family is selected at the default knobs (csrc/plan.hip), and the stand-alone regressor / SMPL
entries (forward, backward, per person, from theta, per-call init rows) that a forward does not reach; `--plan` prints the plan
strings only and needs no GPU (TEPOSE_ASSUME_CUS=256, as tests/test_dispatch.py).  Synthetic weights and seeded inputs: two runs of one
library must print the same text (atomics only hand data over, they never reduce)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ('theta', 'verts', 'kp_3d', 'kp_2d', 'rotmat')

# (name, L, H, B, T, exact fp32, persistent kernels on): what each case is there to reach
CASES = [
    ('small_granules', 2, 256, 3, 6, False, True),          # persistent recurrence with granules, reg_seq_kernel, one-launch SMPL
    ('small_counters', 2, 256, 24, 6, False, True),         # persistent recurrence on counters
    ('small_no_persistent', 2, 256, 24, 6, False, False),   # gru_seq_kernel off: skinny_gru_h3_kernel, gru_first_kernel, tail loop
    ('mid_tiles', 2, 256, 160, 4, False, True),             # gemm_h3_kernel<GRU> and gemm_h3_kernel products
    ('mid_288', 2, 256, 256, 16, False, True),              # 128 x 288 mid tile projection (gemm_h3s_kernel)
    ('large_640', 2, 256, 640, 2, False, True),             # gru_step16_kernel<true> layer 1 / <false> layer 0, gru_first16_kernel, barrier-free <1>
    ('large_ragged', 2, 256, 650, 2, False, True),          # ragged tiles, general step everywhere
    ('large_blocked', 2, 256, 1024, 8, False, True),        # barrier-free <0> layer-0 projection, blocked gate pre-activations from layer 0
    ('one_layer', 1, 256, 3, 5, False, True),
    ('three_layers', 3, 256, 3, 4, False, True),
    ('exact_small', 2, 256, 3, 6, True, True),              # skinny_* fp32
    ('exact_large', 2, 256, 800, 2, True, True),            # gemm_f32_kernel / gru_step_kernel
    ('one_layer_large', 1, 256, 640, 2, False, True),       # scaled step on a one-layer model, x0 planes
    ('three_layers_large', 3, 256, 640, 2, False, True),    # second ping-pong pair of state buffers, blocked
    ('single_frame', 2, 256, 3, 1, False, True),            # the first step is the last step
    # TEPOSE_COLLAPSE_REGRESSOR=0 handles: feature-plane hand-over from the tail product, reg_seq_kernel / the FC loop on the activation records
    ('loop_small', 2, 256, 3, 6, False, True, {'TEPOSE_COLLAPSE_REGRESSOR': '0'}),
    ('loop_mid', 2, 256, 160, 4, False, True, {'TEPOSE_COLLAPSE_REGRESSOR': '0'}),
]
# the encoder alone with is_train = 1 (both tail linears side by side: the K ranges of the tail operand, launch_split_planes' tail, the persistent
# kernel's relu planes): (name, L, H, B, T)
ENCODER_TRAIN = [('encoder_train_small', 2, 256, 3, 6), ('encoder_train_large', 2, 256, 640, 2)]
# the stand-alone entries on the regressor's carve (L = 1, H = 64 handles): (name, entry, N, knobs).  N = 3: the one-launch SMPL kernel; 5 / 40 / 160: the
# general chain; EXACT: no operand planes are carved; BLEND16_MIN_N lowered: the scaled pose-feature planes and their row scales
STANDALONE = (
    [('smpl_p2r%d_N%d' % (p, n), 'smpl%d' % p, n, {}) for n in (3, 40) for p in (0, 1)]
    + [('smpl_bwd_p2r%d_N%d' % (p, n), 'bwd%d' % p, n, {}) for n in (3, 40) for p in (0, 1)]
    + [('verts_from_theta_N5', 'theta', 5, {}), ('per_person_N5', 'person', 5, {})]
    + [('regressor_init_N%d' % n, 'init', n, {}) for n in (3, 160)]
    + [('smpl_exact_N40', 'smpl1', 40, {'TEPOSE_EXACT_FP32': '1'}), ('smpl_blend16_N520', 'smpl1', 520, {'TEPOSE_BLEND16_MIN_N': '300'})]      # (520: a batch the suite runs on that kernel, ragged last tile)
)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def make(L, H, exact, device, env=None):
    from tepose_amd.testing import build_model
    env = dict(env or {}, **({'TEPOSE_EXACT_FP32': '1'} if exact else {}))      # read when the handle is created
    os.environ.update(env)
    try:
        return build_model(L, H, seed=0, device=device)
    finally:
        for k in env:
            os.environ.pop(k, None)


def standalone(name, entry, N, knobs, plan_only, device):
    """one stand-alone regressor / SMPL entry on its own handle: the plan of (N, 1) and the digest of everything it returns"""
    import torch
    from tepose_amd import _lib, synth
    model, _, smpl_np = make(1, 64, False, device, knobs)
    eng = model._engine
    plan = eng.select_kernels(N, 1)
    print('%s N%d plan %s' % (name, N, ';'.join('%s=%s' % kv for kv in sorted(plan.items()))))
    if plan_only:
        return
    dev = torch.device('cuda', torch.cuda.current_device())
    eng.pack_model(model, dev)
    aa = torch.from_numpy(synth.normal('digest/aa', (N, 24, 3), std=0.4))
    betas = torch.from_numpy(synth.normal('digest/betas', (N, 10), std=0.5)).cuda()
    if entry[:-1] in ('smpl', 'bwd') and entry[-1] == '0':            # given rotation matrices: exp of the axis-angle's skew matrix
        k = torch.zeros(N, 24, 3, 3, dtype=torch.float64)
        k[..., 0, 1], k[..., 0, 2], k[..., 1, 2] = -aa[..., 2].double(), aa[..., 1].double(), -aa[..., 0].double()
        pose = torch.linalg.matrix_exp(k - k.transpose(-1, -2)).float().contiguous().cuda()
    else:
        pose = aa.reshape(N, 72).contiguous().cuda()
    out = {}
    if entry.startswith('smpl'):
        out['verts'], out['joints'] = eng.smpl_fwd(pose, betas, entry[-1] == '1')
    elif entry.startswith('bwd'):
        gv = torch.from_numpy(synth.normal('digest/gv', (N, 6890, 3), std=1.0)).cuda()
        gj = torch.from_numpy(synth.normal('digest/gj', (N, 49, 3), std=1.0)).cuda()
        out['g_pose'], out['g_betas'] = eng.smpl_bwd(pose, betas, entry[-1] == '1', gv, gj)
    elif entry in ('theta', 'person'):
        ws = eng.workspace(max(1, (N + 1) // 2), 1, dev)
        out['verts'] = torch.empty((N, 6890, 3), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        if entry == 'theta':
            theta = torch.cat([torch.ones(N, 3, device=dev), pose, betas], 1).contiguous()
            _lib.check(eng.lib.tepose_smpl_verts_from_theta(eng.handle, theta.data_ptr(), N, out['verts'].data_ptr(), ws.data_ptr(), ws.numel(), st), name)
        else:
            _lib.check(eng.lib.tepose_smpl_fwd_per_person(eng.handle, pose.data_ptr(), betas.data_ptr(), N, out['verts'].data_ptr(), ws.data_ptr(), ws.numel(), st), name)
    else:                                                              # tepose_regressor_fwd_init with a given pose, shape and cam
        feat = torch.from_numpy(synth.normal('digest/feat', (N, 2048), std=0.5)).cuda()
        init = (torch.from_numpy(synth.normal('digest/p6', (N, 144), std=0.5)), betas, torch.from_numpy(synth.normal('digest/cam', (N, 3), std=0.3)))
        out = eng.regressor_fwd(feat, 3, torch.from_numpy(smpl_np['J_regressor_h36m']), init=init)
    torch.cuda.synchronize()
    for k in sorted(out):
        print('%s %s %s' % (name, k, sha(out[k])))


def main():
    plan_only = '--plan' in sys.argv
    if plan_only:
        os.environ.setdefault('TEPOSE_ASSUME_CUS', '256')
    import torch
    from tepose_amd import synth
    device = 'cpu' if plan_only else 'cuda'
    for name, L, H, B, T, exact, persistent, *env in CASES:
        model, _, smpl_np = make(L, H, exact, device, *env)
        if not persistent:
            model._engine.set_persistent(False)
        plan = model._engine.select_kernels(B, T)
        print('%s L%d H%d B%d T%d plan %s' % (name, L, H, B, T, ';'.join('%s=%s' % kv for kv in sorted(plan.items()))))
        if plan_only:
            continue
        x = torch.from_numpy(synth.synthetic_windows(B, T, 5)).cuda()
        J = torch.from_numpy(smpl_np['J_regressor_h36m'])
        with torch.no_grad():
            out = model(x, J_regressor=J)[0]
        torch.cuda.synchronize()
        for k in KEYS:
            print('%s %s %s' % (name, k, sha(out[k])))
        del model, out, x
    for name, L, H, B, T in ENCODER_TRAIN:
        model, _, _ = make(L, H, False, device)
        plan = model._engine.select_kernels(B, T)
        print('%s L%d H%d B%d T%d plan %s' % (name, L, H, B, T, ';'.join('%s=%s' % kv for kv in sorted(plan.items()))))
        if plan_only:
            continue
        x = torch.from_numpy(synth.synthetic_windows(B, T, 5)).cuda()
        with torch.no_grad():
            feat = model.encoder(x, is_train=True)
        torch.cuda.synchronize()
        print('%s feature %s' % (name, sha(feat)))
        del model, feat, x
    for case in STANDALONE:
        standalone(*case, plan_only, device)
    if plan_only:
        return
    # the VIBE encoder (tests/test_gpu_vibe.py: bidirectional, two layers, hidden 200, linear + residual)
    from tepose_amd.smpl import SMPL
    from tepose_amd.vibe import VIBE
    smpl_np = synth.synthetic_smpl(0)
    state = synth.synthetic_vibe_state_dict(2, 200, 21, bidirectional=True, add_linear=True)
    mean = {'pose': state['regressor.init_pose'][0], 'shape': state['regressor.init_shape'][0], 'cam': state['regressor.init_cam'][0]}
    vibe = VIBE(seqlen=16, n_layers=2, hidden_size=200, add_linear=True, bidirectional=True, use_residual=True, pretrained='',
                smpl=SMPL.from_tables(smpl_np), smpl_mean_params=mean)
    sd = vibe.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in state.items()})
    vibe.load_state_dict(sd, strict=True)
    vibe = vibe.cuda().eval()
    xv = torch.from_numpy(synth.synthetic_windows(5, 9, 79)[:, :, :2048].copy()).cuda()
    with torch.no_grad():
        print('vibe_encoder feature %s' % sha(vibe.encoder(xv)))
    # the window path: two clips in lock-step through run_clips (cached projections), 4 and 3 windows of 6 frames
    from tepose_amd.driver import run_clips
    model, _, smpl_np = make(2, 256, False, 'cuda')
    feats = [torch.from_numpy(synth.synthetic_windows(1, n, 31 + n)[0, :, :2048].copy()).cuda() for n in (9, 8)]
    th0 = torch.zeros(5, 85)
    th0[:, 0] = 1.                                            # pseudo-theta: cam = [1, 0, 0]
    res = run_clips(model, feats, [th0, th0], 6, J_regressor=torch.from_numpy(smpl_np['J_regressor_h36m']))
    torch.cuda.synchronize()
    for i, r in enumerate(res):
        for k in sorted(r):
            print('run_clips clip%d %s %s' % (i, k, sha(r[k])))


if __name__ == '__main__':
    main()
