"""Arrival-to-result time of one tick of a multi-person live session (tepose_amd.stream.MultiStreamSession) with and without
one-euro smoothing inside the tick, on the published architecture (n_layers 2, hidden 1024), seqlen 6 and 32, S = 1 and 8 slots, all advancing,
keep = theta, kp_3d, verts.  Three arms:

    plain    MultiStreamSession(...)                         raw rows
    smooth   MultiStreamSession(..., smooth=(0.004, 0.7))    the filter step and SMPL on the filtered pose inside the one graph replay
    caller   the plain session, and after each push what a caller had to write before `smooth=` existed: the filter state of every person on the
             host, the step in numpy on the returned theta rows, the filtered pose uploaded, `SMPL` called eagerly, vertices and joints copied back

A sample is a host clock around one tick, ending when the (smoothed) rows are readable on the host.  Per configuration the arms alternate in
blocks, so all see the same state of the box; p50 / p95 are over all samples, the range is that of the per-block medians (run to run).  Not a test;
no threshold.  `--arms plain` runs on a tree that does not know `smooth=` (the parent commit, measured in the same sitting for the comparison).

    python tools/live_smoothing_latency.py [--out profiles/live_smoothing_latency.txt] [--blocks 4] [--ticks 60] [--arms plain smooth caller]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tepose_amd import synth  # noqa: E402
from tepose_amd.stream import MultiStreamSession  # noqa: E402
from tepose_amd.testing import build_model  # noqa: E402

SMOOTH = (0.004, 0.7)
KEEP = ('theta', 'kp_3d', 'verts')


def pct(a, q):
    return float(np.percentile(np.asarray(a), q)) * 1e3


def host_step(x, x_prev, dx_prev, min_cutoff, beta, d_cutoff=1.0):
    """lib/utils/one_euro_filter.py at t_e = 1, fp32 numpy over [S, 72]."""
    two_pi = np.float32(2.0 * np.pi)
    rd = two_pi * np.float32(d_cutoff)
    a_d = rd / (rd + np.float32(1))
    dx_hat = a_d * (x - x_prev) + (np.float32(1) - a_d) * dx_prev
    r = two_pi * (np.float32(min_cutoff) + np.float32(beta) * np.abs(dx_hat))
    a = r / (r + np.float32(1))
    return a * x + (np.float32(1) - a) * x_prev, dx_hat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'live_smoothing_latency.txt'))
    ap.add_argument('--blocks', type=int, default=4)
    ap.add_argument('--ticks', type=int, default=60, help='samples per block, for every arm')
    ap.add_argument('--slots', type=int, nargs='*', default=[1, 8])
    ap.add_argument('--seqlens', type=int, nargs='*', default=[6, 32])
    ap.add_argument('--arms', nargs='*', default=['plain', 'smooth', 'caller'], choices=['plain', 'smooth', 'caller'])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('live_smoothing_latency: needs the GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    prop = torch.cuda.get_device_properties(0)
    lines = ['one tick of MultiStreamSession, arms %s: host time from push() until the rows are readable on the host, ms' % ', '.join(a.arms),
             'box: %s, %d CUs; torch %s; model n_layers 2, hidden 1024, 49 joints, keep = %s; %d blocks of %d samples per arm, alternating in the order given'
             % (prop.name, prop.multi_processor_count, torch.__version__, ','.join(KEEP), a.blocks, a.ticks),
             'range = lowest .. highest per-block median', '']
    model, _, _ = build_model(2, 1024, seed=0, device=dev, smpl_np=synth.synthetic_smpl(0), seqlen=32)
    smpl = model.regressor.smpl
    for T in a.seqlens:
        for S in a.slots:
            w = synth.synthetic_windows(S, T + 7, 11)
            feats = torch.from_numpy(w[:, :, :2048].copy())
            th0 = torch.from_numpy(w[:, :T - 1, 2048:].copy())
            ses = {}
            if 'plain' in a.arms or 'caller' in a.arms:
                ses['plain'] = MultiStreamSession(model, T, S, keep=KEEP)
            if 'smooth' in a.arms:
                ses['smooth'] = MultiStreamSession(model, T, S, keep=KEEP, smooth=SMOOTH)
            for one in ses.values():
                for s in range(S):
                    one.join(s, feats[s, :T - 1], th0[s])
            # the caller's host state: started from the history as smooth_pose starts a tracklet
            state = [th0[:, 0, 3:75].numpy().copy(), np.zeros((S, 72), dtype=np.float32)]
            for t in range(1, T - 1):
                state = list(host_step(th0[:, t, 3:75].numpy(), state[0], state[1], *SMOOTH))
            pose_host = torch.zeros(S, 72).pin_memory()
            frame = [0]

            def tick(arm):
                f = feats[:, T - 1 + frame[0] % 8].contiguous()          # the frame's features as they arrive: one [S,2048] host tensor
                frame[0] += 1
                t0 = time.perf_counter()
                if arm != 'caller':
                    ses[arm].push(f)
                else:
                    out = ses['plain'].push(f)
                    theta = np.stack([out[s]['theta'].numpy() for s in range(S)])
                    state[0], state[1] = host_step(theta[:, 3:75], state[0], state[1], *SMOOTH)
                    pose_host.copy_(torch.from_numpy(state[0]))
                    pose = pose_host.to(dev, non_blocking=True).view(S, 24, 3)
                    res = smpl(betas=torch.from_numpy(theta[:, 75:]).to(dev), body_pose=pose[:, 1:], global_orient=pose[:, 0:1])
                    res.vertices.cpu(), res.joints.cpu()
                return time.perf_counter() - t0
            for _ in range(10):                                       # warm-up of every arm
                for arm in a.arms:
                    tick(arm)
            samples, meds = {arm: [] for arm in a.arms}, {arm: [] for arm in a.arms}
            for _ in range(a.blocks):
                for arm in a.arms:
                    b = [tick(arm) for _ in range(a.ticks)]
                    samples[arm] += b
                    meds[arm].append(pct(b, 50))
            for arm in a.arms:
                line = 'seqlen %2d S %2d %-6s | p50 %7.3f  p95 %7.3f  range %6.3f .. %6.3f' % (T, S, arm, pct(samples[arm], 50), pct(samples[arm], 95),
                                                                                             min(meds[arm]), max(meds[arm]))
                print(line, flush=True)
                lines.append(line)
            lines.append('')
            del ses
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
