"""Randomised parity sweep (manual, GPU): random (L, H, B, T) models and windows, HIP path vs the fp64 oracle --
encoder features in both modes for every configuration, the full forward for B <= 300.

    python tests/_fuzz_parity.py <seed> <seconds> [--replicated]

--replicated: batches of 640 windows and more are drawn as copies of 128 distinct windows (tests/_replicated.py), at every hidden size, and
features (both modes) and the full forward are compared on EVERY row against the oracle's 128 answers; a failure names row, tile and window.

Not collected by pytest (it runs for as long as it is told to); round 1: about 1 900 configurations in four runs (498 in
15 min on the final binary), worst absolute error 2.0e-6, none over the test tolerances (2e-5 features, 1e-4 outputs); round 3's
final binary: 322 configurations in 15 min, worst 1.9e-6; round 4 (16x16x32 kernels, barrier-free projection): 260 configurations in 15 min, worst 1.9e-6; round 4's final binary (blocked layouts, scaled-format path from
B = 640, full forwards up to B = 1300 against a random subset of the oracle's windows): 298 configurations in 14 min, 262 of them with the full forward, worst 2.4e-6;
round 5 (plane-fed step kernel, pruned dispatch, exact-tile small-batch kernels): 686 configurations in three runs, worst 2.3e-6 (profiles/r05_fuzz_soak.txt)."""
import sys, os, time
import numpy as np, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
REPLICATED = '--replicated' in sys.argv
sys.argv = [a for a in sys.argv if a != '--replicated']
import _replicated as R
from tepose_amd import synth
from tepose_amd.testing import build_model
from oracle import tepose_ref as O
rng = np.random.RandomState(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
smpl_np = synth.synthetic_smpl(0)
J = torch.from_numpy(smpl_np['J_regressor_h36m'])
worst = 0.0
t_end = time.time() + float(sys.argv[2]) if len(sys.argv) > 2 else time.time() + 300
n = 0
while time.time() < t_end:
    L = int(rng.choice([1, 2, 2, 3])); H = int(rng.choice([64, 100, 128, 192, 256, 320, 256, 512, 768, 1024]))   # % 256 == 0: persistent kernels
    B = int(rng.choice([1, 2, 3, 4, 5, 7, 16, 17, 31, 33, 48, 64, 65, 100, 128, 129, 200, 257, 400, 640, 768, 769, 1000, 1024, 1280, 1300, 2048, 2100, 4096, 4200]))   # % 128 == 0 from 640: the plane-fed step kernel
    T = int(rng.choice([1, 2, 3, 5, 6, 8, 16, 33]))
    if REPLICATED and B >= 640:
        seed = int(rng.randint(1 << 20))
        model, state, _ = build_model(L, H, seed=seed, device='cuda', smpl_np=smpl_np)
        xd, xw, src = R.replicated_windows(B, T, 128, seed + 1, 'cuda')
        with torch.no_grad():
            got = dict(model(xd, J_regressor=J)[0]); got['feature'] = model.encoder(xd); got['feature_train'] = model.encoder(xd, is_train=True)
        ref = O.tepose_fwd(state, smpl_np, xw, L, J_regressor=smpl_np['J_regressor_h36m'], dtype=torch.float64)
        with torch.no_grad():
            ref['feature_train'] = O.encoder_fwd(O.split_state_dict(state, torch.float64)[0], torch.from_numpy(xw).double(), L, is_train=True)
        names = ('feature', 'feature_train', 'verts', 'kp_3d', 'kp_2d', 'rotmat')
        tols = {k: 2e-5 if k.startswith('feature') else 1e-4 for k in names}
        try:
            R.assert_separated({k: ref[k] for k in names}, tols)
        except AssertionError as e:          # the guard stays as it is: a draw whose windows are too close is not compared at all
            print('L=%d H=%4d B=%4d T=%d  skipped: %s' % (L, H, B, T, e), flush=True)
            del model
            continue
        reps = [R.compare_all_rows(got[k], ref[k], src, tols[k], name=k, raise_on_fail=False) for k in names]
        spread = max(R.copies_spread(got[k], src) for k in names)
        worst = max([worst] + [r.worst for r in reps]); n += 1
        bad = [r for r in reps if r.n_over] if spread <= 2e-5 else reps
        print('L=%d H=%4d B=%4d T=%d  all rows: enc %.1e / %.1e  full %.1e  copies %.1e%s' % (
            L, H, B, T, reps[0].worst, reps[1].worst, max(r.worst for r in reps[2:]), spread, '   <<<<<< FAIL' if bad else ''), flush=True)
        for r in bad:
            print('    ' + R.describe(r), flush=True)
        del model
        continue
    if H >= 512 and B > 300:
        B = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 48, 64, 65]))      # keep the fp64 oracle of big models affordable
    seed = int(rng.randint(1 << 20))
    model, state, _ = build_model(L, H, seed=seed, device='cuda', smpl_np=smpl_np)
    x = synth.synthetic_windows(B, T, seed + 1)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        f = model.encoder(xd); ft = model.encoder(xd, is_train=True)
        out = model(xd, J_regressor=J)[0] if (B <= 300 or (H <= 256 and B <= 1300)) else None      # B >= 512: the blend-shape product on the persistent kernel
    enc, _ = O.split_state_dict(state, torch.float64)
    with torch.no_grad():
        rf = O.encoder_fwd(enc, torch.from_numpy(x).double(), L)
        rft = O.encoder_fwd(enc, torch.from_numpy(x).double(), L, is_train=True)
    e1 = (f.cpu().double() - rf).abs().max().item(); e2 = (ft.cpu().double() - rft).abs().max().item()
    e3 = 0.0
    if out is not None:
        sel = np.arange(B) if B <= 300 else np.sort(rng.choice(B, 96, replace=False))       # windows are independent: a random subset of a big batch
        ref = O.tepose_fwd(state, smpl_np, x[sel], L, J_regressor=smpl_np['J_regressor_h36m'], dtype=torch.float64)
        e3 = max((out[k][torch.from_numpy(sel).cuda()].cpu().double() - ref[k]).abs().max().item() for k in ('verts', 'kp_3d', 'rotmat', 'kp_2d'))
    worst = max(worst, e1, e2, e3); n += 1
    flag = '' if max(e1, e2) < 2e-5 and e3 < 1e-4 else '   <<<<<< FAIL'
    print('L=%d H=%3d B=%4d T=%d  enc %.1e / %.1e  full %.1e%s' % (L, H, B, T, e1, e2, e3, flag), flush=True)
    del model
print('configs', n, 'worst', worst)
