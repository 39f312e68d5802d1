"""Frame-to-result time of one tick of the live session from pixels (tepose_amd.live.PixelSession) next to the composition a
caller writes without it, on the same models: the published architecture (ResNet-50 backbone; n_layers 2, hidden 1024), a 1080p frame on the HOST,
seqlen 6 and 32, S = 1, 2, 4, 8 slots, every slot advancing.

    pixel      ses.push(frame, {slot: box})                                   one graph replay: boxes + ops + frame up, crops, backbone, tick
    composed   feats = hmr.features_from_frames(frame[None].cuda(), zeros(S), boxes, scale)      the frame uploaded, maps on the host (numpy), crop launch,
               multi.push(feats, slots=range(S))                              backbone launched eagerly; then the feature session's tick

A sample is a host clock around those lines: both start from the same uint8 host tensor and end with the results in pinned host memory.  Per
configuration the two ways alternate in blocks, so both see the same state of the box; p50 is over all samples, the range is that of the per-block
medians (run to run).  A third block per round pushes the same frame as a DEVICE tensor (a decoder that writes to the device): what staging and
uploading 6.2 MB costs shows as the difference.  Not a test; no threshold.

    python tools/pixel_session_latency.py [--out profiles/pixel_session_latency.txt] [--blocks 4] [--ticks 40]
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
from tepose_amd.live import PixelSession  # noqa: E402
from tepose_amd.smpl import SMPL  # noqa: E402
from tepose_amd.spin import hmr as make_hmr  # noqa: E402
from tepose_amd.stream import MultiStreamSession  # noqa: E402
from tepose_amd.testing import build_model  # noqa: E402

H, W, SCALE = 1080, 1920, 1.2


def pct(a, q):
    return float(np.percentile(np.asarray(a), q)) * 1e3


def boxes_of(S, tick):
    """S boxes of 120 - 330 px spread over the frame, the last one near the right edge, drifting with the tick."""
    s = np.arange(S, dtype=np.float64)
    return np.stack([180.0 + (1700.0 / max(S - 1, 1)) * s + 1.3 * (tick % 8), 300.0 + 55.0 * s + 0.7 * (tick % 8), 120.0 + 30.0 * s, 200.0 + 18.0 * s], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pixel_session_latency.txt'))
    ap.add_argument('--blocks', type=int, default=4)
    ap.add_argument('--ticks', type=int, default=40, help='samples per block, for either way at every S')
    ap.add_argument('--slots', type=int, nargs='*', default=[1, 2, 4, 8])
    ap.add_argument('--seqlen', type=int, nargs='*', default=[6, 32])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('pixel_session_latency: needs the GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    prop = torch.cuda.get_device_properties(0)
    lines = ['one tick from a 1080p uint8 frame on the host: PixelSession.push against features_from_frames + MultiStreamSession.push; host time, ms',
             'box: %s, %d CUs; torch %s; ResNet-50 backbone (split-precision products), model n_layers 2, hidden 1024, 49 joints, keep = theta,kp_3d,verts'
             % (prop.name, prop.multi_processor_count, torch.__version__),
             '%d blocks of %d samples per way at every S, alternating, pixel first; every slot advancing' % (a.blocks, a.ticks),
             'range = lowest .. highest per-block median; ratio = p50 composed / p50 pixel; last column: pixel with the frame already on the device, p50', '']
    smpl_np = synth.synthetic_smpl(0)
    model, _, _ = build_model(2, 1024, seed=0, device=dev, smpl_np=smpl_np, seqlen=32)
    backbone = make_hmr(smpl_mean_params=synth.synthetic_mean_params(0), pretrained=False, smpl=SMPL.from_tables(smpl_np)).to(dev).eval()
    frames = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (8, H, W, 3), dtype=np.uint8))
    frames_dev = frames.to(dev)
    for T in a.seqlen:
        lines.append('seqlen %d' % T)
        lines.append('   S | pixel p50    p95   range            | composed p50    p95   range            | ratio | device frame')
        for S in a.slots:
            w = synth.synthetic_windows(S, T, 11)
            pixel = PixelSession(model, backbone, None, T, S, frame_size=(H, W), bbox_scale=SCALE)
            multi = MultiStreamSession(model, T, S)
            for s in range(S):
                for ses in (pixel, multi):
                    ses.join(s, torch.from_numpy(w[s, :T - 1, :2048].copy()), torch.from_numpy(w[s, :T - 1, 2048:].copy()))
            tick, slots, zeros = [0], list(range(S)), np.zeros(S, dtype=np.int64)

            def tick_pixel():
                frame, b = frames[tick[0] % 8], boxes_of(S, tick[0])
                feed = {s: b[s] for s in slots}
                t0 = time.perf_counter()
                pixel.push(frame, feed)
                return time.perf_counter() - t0

            def tick_pixel_dev():
                frame, b = frames_dev[tick[0] % 8], boxes_of(S, tick[0])
                feed = {s: b[s] for s in slots}
                t0 = time.perf_counter()
                pixel.push(frame, feed)
                return time.perf_counter() - t0

            def tick_composed():
                frame, b = frames[tick[0] % 8], boxes_of(S, tick[0])
                t0 = time.perf_counter()
                feats = backbone.features_from_frames(frame[None].cuda(), zeros, b, scale=SCALE)
                multi.push(feats, slots=slots)
                return time.perf_counter() - t0
            with torch.no_grad():
                for _ in range(8):                                  # warm-up of both ways
                    tick_pixel(), tick_composed(), tick_pixel_dev()
                    tick[0] += 1
                tp, tc, td, med_p, med_c = [], [], [], [], []
                for _ in range(a.blocks):
                    bp = []
                    for _ in range(a.ticks):
                        bp.append(tick_pixel())
                        tick[0] += 1
                    bc = []
                    for _ in range(a.ticks):
                        bc.append(tick_composed())
                        tick[0] += 1
                    for _ in range(a.ticks):
                        td.append(tick_pixel_dev())
                        tick[0] += 1
                    tp += bp
                    tc += bc
                    med_p.append(pct(bp, 50))
                    med_c.append(pct(bc, 50))
            line = '%4d | %8.3f %7.3f  %6.3f .. %6.3f | %12.3f %7.3f  %6.3f .. %6.3f | %5.2f | %8.3f' % (
                S, pct(tp, 50), pct(tp, 95), min(med_p), max(med_p), pct(tc, 50), pct(tc, 95), min(med_c), max(med_c), pct(tc, 50) / pct(tp, 50), pct(td, 50))
            print(line, flush=True)
            lines.append(line)
            del pixel, multi
        lines.append('')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
