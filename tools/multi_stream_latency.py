"""Arrival-to-result time of one tick of a multi-person live session (tepose_amd.stream.MultiStreamSession) next to the
same people served by one StreamSession each, pushed in turn, on the same model: the published architecture (n_layers 2, hidden 1024), seqlen
6 and 32, with and without the vertices among the kept outputs, S = 1, 2, 4, 8, 16, 64 slots, all advancing.

A sample is a host clock around one `push` (it ends in the event wait: the results are in pinned host memory) -- for the single sessions, around
the S pushes of one frame.  Per configuration the two ways alternate in blocks, so both see the same state of the box; p50 / p95 are over all
samples, the range is that of the per-block medians (run to run).  Not a test; no threshold.

    python tools/multi_stream_latency.py [--out profiles/multi_stream_latency.txt] [--blocks 4] [--ticks 60]
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
from tepose_amd.stream import MultiStreamSession, StreamSession  # noqa: E402
from tepose_amd.testing import build_model  # noqa: E402


def pct(a, q):
    return float(np.percentile(np.asarray(a), q)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_stream_latency.txt'))
    ap.add_argument('--blocks', type=int, default=4)
    ap.add_argument('--ticks', type=int, default=60, help='samples per block, for either way at every S')
    ap.add_argument('--slots', type=int, nargs='*', default=[1, 2, 4, 8, 16, 64])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('multi_stream_latency: needs the GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    prop = torch.cuda.get_device_properties(0)
    lines = ['one tick of MultiStreamSession against S StreamSession.push calls in turn: host time from push() to its return, ms',
             'box: %s, %d CUs; torch %s; model n_layers 2, hidden 1024, 49 joints; %d blocks of %d samples per way at every S, alternating, multi first'
             % (prop.name, prop.multi_processor_count, torch.__version__, a.blocks, a.ticks),
             'range = lowest .. highest per-block median; ratio = p50 of S single pushes / p50 of one tick', '']
    model, _, _ = build_model(2, 1024, seed=0, device=dev, smpl_np=synth.synthetic_smpl(0), seqlen=32)
    for T in (6, 32):
        for keep in (('theta', 'kp_3d', 'verts'), ('theta', 'kp_3d')):
            lines.append('seqlen %d, keep = %s' % (T, ','.join(keep)))
            lines.append('   S |  tick p50    p95   range            | S pushes p50    p95   range            | ratio')
            for S in a.slots:
                w = synth.synthetic_windows(S, T + 7, 11)
                feats = torch.from_numpy(w[:, :, :2048].copy())
                th0 = torch.from_numpy(w[:, :T - 1, 2048:].copy())
                multi = MultiStreamSession(model, T, S, keep=keep)
                singles = [StreamSession(model, T, feats[s, :T - 1], th0[s], keep=keep) for s in range(S)]
                for s in range(S):
                    multi.join(s, feats[s, :T - 1], th0[s])
                frame = [0]

                def tick_multi():
                    f = feats[:, T - 1 + frame[0] % 8].contiguous()      # the frame's features as they arrive: one [S,2048] host tensor
                    t0 = time.perf_counter()
                    multi.push(f)
                    return time.perf_counter() - t0

                def tick_singles():
                    f = feats[:, T - 1 + frame[0] % 8].contiguous()
                    t0 = time.perf_counter()
                    for s in range(S):
                        singles[s].push(f[s])
                    return time.perf_counter() - t0
                for _ in range(10):                                 # warm-up of both ways
                    tick_multi(), tick_singles()
                    frame[0] += 1
                tm, ts, med_m, med_s = [], [], [], []
                for _ in range(a.blocks):
                    bm = []
                    for _ in range(a.ticks):
                        bm.append(tick_multi())
                        frame[0] += 1
                    bs = []
                    for _ in range(a.ticks):
                        bs.append(tick_singles())
                        frame[0] += 1
                    tm += bm
                    ts += bs
                    med_m.append(pct(bm, 50))
                    med_s.append(pct(bs, 50))
                line = '%4d | %8.3f %7.3f  %6.3f .. %6.3f | %12.3f %7.3f  %6.3f .. %6.3f | %5.2f' % (
                    S, pct(tm, 50), pct(tm, 95), min(med_m), max(med_m), pct(ts, 50), pct(ts, 95), min(med_s), max(med_s), pct(ts, 50) / pct(tm, 50))
                print(line, flush=True)
                lines.append(line)
                del multi, singles
            lines.append('')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
