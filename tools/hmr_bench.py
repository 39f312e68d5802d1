"""Time the HMR feature extractor (tepose_amd.spin.HMR.feature_extractor): N in {1, 32, 64} images, both numerics modes.

    python tools/hmr_bench.py [--out profiles/hmr_features.txt] [--no-trace]

Per case: device events around >= 0.5 s of warmed-up calls; algorithmic FLOPs (2 x the multiply-adds of the 53 convolutions, counted from the
module's own layers) over that time, and its share of the peak of the MFMA the mode runs on (split: dense fp16 MFMA / 3 products; exact: the
fp32-input MFMA).  Then one kernel-trace run of its own (rocprofv3 --kernel-trace on a child process that runs N = 32 in split mode) and
the ten kernels with the largest share.  Nothing here is a gate: this path's speed is recorded, not asserted.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3          # fp32-input MFMA
PEAK_F16_MFMA_TFLOPS = 2516.6         # dense fp16 MFMA; a split-precision product is three of them


def build(exact):
    from tepose_amd import synth
    from tepose_amd.smpl import SMPL
    from tepose_amd.spin import hmr
    os.environ['TEPOSE_EXACT_FP32'] = '1' if exact else '0'
    model = hmr(smpl_mean_params=synth.synthetic_mean_params(0), pretrained=False, smpl=SMPL.from_tables(synth.synthetic_smpl(0)))
    return model.cuda().eval()


def macs_per_image(model):
    """Multiply-adds of the convolutions of one 224 x 224 image, from the module's layers (a block's map size changes at its strided convolution)."""
    total, size = 0, 224
    c = model.conv1
    size = (size + 2 * c.padding[0] - c.kernel_size[0]) // c.stride[0] + 1
    total += c.weight.numel() * size * size
    size = (size + 2 - 3) // 2 + 1                                  # the max pool
    for i in range(4):
        for blk in getattr(model, 'layer%d' % (i + 1)):
            total += blk.conv1.weight.numel() * size * size
            out = (size + 2 - 3) // blk.conv2.stride[0] + 1
            total += blk.conv2.weight.numel() * out * out + blk.conv3.weight.numel() * out * out
            if hasattr(blk, 'downsample'):
                total += blk.downsample[0].weight.numel() * out * out
            size = out
    return total


def time_case(model, n, min_s=0.5):
    import torch
    x = torch.randn(n, 3, 224, 224, device='cuda')
    with torch.no_grad():
        for _ in range(3):
            model.feature_extractor(x)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        calls, reps = 0, 4
        e0.record()
        while True:
            for _ in range(reps):
                model.feature_extractor(x)
            calls += reps
            e1.record()
            e1.synchronize()
            if e0.elapsed_time(e1) >= min_s * 1e3:
                break
    return e0.elapsed_time(e1) / calls


def trace(lines):
    tmp = tempfile.mkdtemp(prefix='hmr_trace_')
    cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', tmp, '--', sys.executable, os.path.abspath(__file__), '--child']
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    files = sorted(glob.glob(os.path.join(tmp, '**', '*kernel_trace.csv'), recursive=True))
    if p.returncode != 0 or not files:
        lines.append('kernel trace: not measured (rocprofv3 rc %d, %d trace files)' % (p.returncode, len(files)))
        return
    per = {}
    for r in csv.DictReader(open(files[0])):
        d = per.setdefault(r['Kernel_Name'], [0, 0.0])
        d[0] += 1
        d[1] += float(r['End_Timestamp']) - float(r['Start_Timestamp'])
    tot = sum(v[1] for v in per.values()) or 1.0
    lines.append('kernel trace (N = 32, split mode, 8 calls after packing; share of the summed kernel time of the process):')
    for name, (calls, ns) in sorted(per.items(), key=lambda kv: -kv[1][1])[:10]:
        lines.append('  %5.1f %%  %6d calls  %9.1f us mean  %s' % (100 * ns / tot, calls, ns / calls / 1e3, name[:110]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    import torch
    if a.child:
        model = build(False)
        x = torch.randn(32, 3, 224, 224, device='cuda')
        with torch.no_grad():
            for _ in range(8):
                model.feature_extractor(x)
        torch.cuda.synchronize()
        return
    lines = ['HMR feature extractor, %s' % torch.cuda.get_device_name(0)]
    for exact in (False, True):
        model = build(exact)
        gmac = macs_per_image(model) / 1e9
        peak = PEAK_F32_MFMA_TFLOPS if exact else PEAK_F16_MFMA_TFLOPS / 3
        for n in (1, 32, 64):
            ms = time_case(model, n)
            tf = 2 * gmac * n / ms                                   # GFLOP per ms = TFLOP/s
            lines.append('%-5s N = %2d  %8.3f ms / call  %7.1f images / s  %6.1f TFLOP/s algorithmic (%.2f GMAC / image)  %5.1f %% of the %s MFMA peak'
                         % ('exact' if exact else 'split', n, ms, n / ms * 1e3, tf, gmac, 100 * tf / peak, 'fp32' if exact else 'split fp16x3'))
        del model
    if a.no_trace:
        lines.append('kernel trace: not measured')
    else:
        trace(lines)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
