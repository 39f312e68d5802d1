"""Time the crop kernel (csrc/crop.hip) on the work of one HMR pass: 64 crops of 224 x 224 from 1080p frames.

    python tools/crop_bench.py [--out profiles/crop_frames.txt]

Three timings, each with device events around >= 0.5 s of warmed-up calls:
  * the kernel alone (tepose_crop_frames_u8 with index and maps resident on the device), normalised output only, as HMR.features_from_frames calls it;
  * tepose_amd.crop.crop_frames end to end (the affine maps on the host, two small uploads, the output allocation, the launch);
  * HMR.features_from_frames (crop + the 64-image feature pass, split mode) next to HMR.feature_extractor on ready crops.
Bytes come from shapes: the fp32 planes written, plus the scaled box area x 3 read (uint8; each source pixel counted once per crop).  Achieved
bytes / s = those bytes over the kernel-alone time, next to the 8.0 TB/s HBM peak.  Nothing here is a gate.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, S, SCALE = 64, 224, 1.2
HBM_PEAK_TBS = 8.0


def timed(fn, min_s=0.5, reps=16):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = 0
    e0.record()
    while True:
        for _ in range(reps):
            fn()
        calls += reps
        e1.record()
        e1.synchronize()
        if e0.elapsed_time(e1) >= min_s * 1e3:
            return e0.elapsed_time(e1) / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from tepose_amd import _lib
    from tepose_amd.crop import crop_frames, crop_transform
    from tools.hmr_bench import build
    g = np.random.default_rng(0)
    frames = torch.from_numpy(g.integers(0, 256, (16, 1080, 1920, 3), dtype=np.uint8)).cuda()
    idx = np.arange(N) % 16
    side = g.uniform(250, 520, N)                                     # a person in a 1080p frame; the tracker's square boxes
    bb = np.stack([g.uniform(300, 1620, N), g.uniform(300, 780, N), side, side], axis=1)
    written = N * 3 * S * S * 4
    read = float(((bb[:, 2] * SCALE) * (bb[:, 3] * SCALE)).sum() * 3)
    _, minv = crop_transform(bb, SCALE, S)
    d_idx, d_minv = torch.from_numpy(idx.astype(np.int32)).cuda(), torch.from_numpy(minv.reshape(N, 6)).cuda()
    out = torch.empty((N, 3, S, S), dtype=torch.float32, device='cuda')
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream

    def kernel():
        _lib.check(lib.tepose_crop_frames_u8(frames.data_ptr(), 16, 1080, 1920, d_idx.data_ptr(), d_minv.data_ptr(), N, S, out.data_ptr(), None, stream),
                   'tepose_crop_frames_u8')
    k_ms, k_calls = timed(kernel, reps=64)
    w_ms, w_calls = timed(lambda: crop_frames(frames, idx, bb, scale=SCALE))
    model = build(False)
    with torch.no_grad():
        crops = crop_frames(frames, idx, bb, scale=SCALE)
        f_ms, f_calls = timed(lambda: model.feature_extractor(crops), reps=4)
        c_ms, c_calls = timed(lambda: model.features_from_frames(frames, idx, bb, scale=SCALE), reps=4)
    tbs = (written + read) / (k_ms * 1e-3) / 1e12
    lines = ['crop kernel, %s: %d crops of %d x %d from 1080p uint8 frames, boxes %.0f - %.0f px at scale %.1f' % (torch.cuda.get_device_name(0), N, S, S, side.min(), side.max(), SCALE),
             'bytes from shapes: %.1f MB written (fp32 planes) + %.1f MB read (scaled box area x 3) = %.1f MB' % (written / 1e6, read / 1e6, (written + read) / 1e6),
             'kernel alone (normalised output only)      %8.4f ms / call over %d calls   %.2f TB/s achieved = %.0f %% of the %.1f TB/s HBM peak'
             % (k_ms, k_calls, tbs, 100 * tbs / HBM_PEAK_TBS, HBM_PEAK_TBS),
             'crop_frames end to end (maps, uploads)     %8.4f ms / call over %d calls' % (w_ms, w_calls),
             'feature_extractor on 64 ready crops        %8.3f ms / call over %d calls (split mode)' % (f_ms, f_calls),
             'features_from_frames (crop + features)     %8.3f ms / call over %d calls' % (c_ms, c_calls),
             "crop's share of crop + features: %.2f %% by the kernel alone, %.2f %% by the difference of the two lines above"
             % (100 * k_ms / (k_ms + f_ms), 100 * (c_ms - f_ms) / c_ms)]
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
