"""Time the overlay rasteriser (csrc/render.hip) on a clip's worth of work: 64 frames of 1080p, 1 and 4 persons per frame, each about 500 px tall.

    python tools/render_bench.py [--out profiles/render_frames.txt]

The synthetic SMPL tables are random vertices without a topology, so the meshes are the tests' closed blob with SMPL's counts (6 890 vertices, 13 776
faces: tests/_render_ref.py), one differently dented blob per person, spread across the frame.

Two kinds of numbers, nothing gated on either:
  * per pass (clear, vertex, triangle, resolve): kernel times from `rocprofv3 --kernel-trace --stats` around a child process that makes a few calls of
    tepose_render_meshes_u8 with every input resident -- a run of its own, started before this process touches the GPU;
  * whole calls, with device events around >= 0.5 s of warmed-up calls: the entry point alone, and Renderer.render_frames end to end (uploads, chunking).
The byte floor is computed from shapes: per frame the clear writes the key plane (8 B per pixel), the resolve reads it and reads and writes the frame
(3 B per pixel each); the vertex pass moves 36 B per vertex and instance; the triangle pass has no floor from shapes (its traffic is the atomics on
covered fragments).  Floor time = floor bytes over the 8.0 TB/s HBM peak.  64 frames move 2.9 GB per call, far beyond the 256 MB Infinity Cache:
these are not warm-cache figures.  There is no parent-commit number (the feature is new) and no pyrender number (it cannot run here) to compare with.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

F, H, W = 64, 1080, 1920
HBM_PEAK_TBS = 8.0
TALL_PX = 500.0
PASSES = (('clear', 'fillBuffer'), ('vertex', 'render_vertex_kernel'), ('triangle', 'render_triangle_kernel'), ('resolve', 'render_resolve_kernel'))


def scene(persons):
    """-> faces, idx [n], verts [n,V,3], cams [n,4], colors [n,3]: `persons` blobs per frame, side by side, swaying from frame to frame."""
    import _render_ref as R
    blobs = [R.blob(p) for p in range(persons)]
    faces = blobs[0][1]
    height = float(blobs[0][0][:, 1].max() - blobs[0][0][:, 1].min())
    sy = TALL_PX / (height * H / 2)
    sx = sy * H / W
    idx, verts, cams = [], [], []
    for f in range(F):
        for p in range(persons):
            idx.append(f)
            verts.append(blobs[p][0])
            x_ndc = (p + 0.5) / persons * 1.6 - 0.8 + 0.05 * np.sin(0.3 * f + p)
            cams.append([sx * (1 + 0.1 * p), sy * (1 + 0.1 * p), x_ndc / (sx * (1 + 0.1 * p)), 0.05 * np.cos(0.2 * f)])
    colors = np.tile(np.array([[1.0, 1.0, 0.9], [0.9, 0.6, 0.6], [0.6, 0.9, 0.6], [0.6, 0.6, 0.9]], dtype=np.float32)[:persons], (F, 1))
    return faces, np.array(idx), np.stack(verts), np.array(cams), colors


def resident(persons):
    """Everything tepose_render_meshes_u8 takes, on the device -> (call, frames, out)."""
    import torch
    import _render_ref as R
    from tepose_amd import _lib
    faces, idx, verts, cams, colors = scene(persons)
    n, V, Fc = idx.shape[0], verts.shape[1], faces.shape[0]
    off, lst = R.adjacency(faces, V)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (F, H, W, 3), dtype=np.uint8)).cuda()
    out = torch.empty_like(frames)
    d = [dev(a) for a in (idx.astype(np.int32), verts, faces, off, lst, cams, colors)]
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    ws = torch.empty(int(lib.tepose_render_workspace_bytes(H, W, F, n, V, Fc)), dtype=torch.uint8, device='cuda')

    def call():
        _lib.check(lib.tepose_render_meshes_u8(frames.data_ptr(), F, H, W, d[0].data_ptr(), d[1].data_ptr(), n, V, d[2].data_ptr(), Fc, d[3].data_ptr(),
                                               d[4].data_ptr(), int(lst.shape[0]), d[5].data_ptr(), None, d[6].data_ptr(), out.data_ptr(), None, None,
                                               ws.data_ptr(), ws.numel(), stream), 'tepose_render_meshes_u8')
    call.keep = (d, ws)
    return call, frames, out


def timed(fn, min_s=0.5, reps=2):
    import torch
    for _ in range(2):
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


def traced(persons, calls, workdir):
    """Kernel times of `calls` calls (after none: the first call's code-object load is in the host's time, not the kernels'), ms per call per pass, or None."""
    d = os.path.join(workdir, 'render_trace_p%d' % persons)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__), '--child', str(persons), '--calls', str(calls)]
    try:
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
    except (OSError, subprocess.TimeoutExpired) as e:
        return None, 'rocprofv3 did not run (%s)' % (e,)
    found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if p.returncode != 0 or not found:
        return None, 'rocprofv3 exit %d, %d stats files; %s' % (p.returncode, len(found), (p.stderr or '')[-300:].replace('\n', ' | '))
    ms = {}
    for row in csv.DictReader(open(found[0])):
        for name, needle in PASSES:
            if needle in row['Name']:
                ms[name] = ms.get(name, 0.0) + float(row['TotalDurationNs']) / 1e6 / calls
    return ms, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', type=int, default=0)
    ap.add_argument('--calls', type=int, default=6)
    ap.add_argument('--workdir', default=None, help='where the kernel traces are kept (default: a temporary directory)')
    a = ap.parse_args()
    if a.child:
        import torch
        call = resident(a.child)[0]
        for _ in range(a.calls):
            call()
        torch.cuda.synchronize()
        return
    if a.workdir is None:
        import tempfile
        a.workdir = tempfile.mkdtemp(prefix='render_trace_')
    os.makedirs(a.workdir, exist_ok=True)
    traces = {p: traced(p, a.calls, a.workdir) for p in (1, 4)}          # before this process opens the GPU
    import torch
    from tepose_amd.render import Renderer
    px = H * W
    floors = {'clear': 8 * px, 'vertex': None, 'triangle': None, 'resolve': (8 + 3 + 3) * px}
    lines = ['overlay rasteriser, %s: %d frames of %d x %d uint8, blobs of 6890 vertices / 13776 faces about %.0f px tall' % (torch.cuda.get_device_name(0), F, W, H, TALL_PX),
             'byte floor per frame from shapes: key plane write %.1f MB (clear) + key plane read %.1f MB + frame read %.1f MB + frame write %.1f MB (resolve) = %.1f MB'
             ' = %.4f ms at the %.1f TB/s HBM peak' % (8 * px / 1e6, 8 * px / 1e6, 3 * px / 1e6, 3 * px / 1e6, 22 * px / 1e6, 22 * px / (HBM_PEAK_TBS * 1e12) * 1e3, HBM_PEAK_TBS),
             'one call moves %.1f GB, far beyond the 256 MB Infinity Cache: not warm-cache figures.  No parent-commit and no pyrender number exists to compare with.'
             % (22 * px * F / 1e9)]
    for persons in (1, 4):
        faces, idx, verts, cams, colors = scene(persons)
        floors['vertex'] = 36 * persons * verts.shape[1]
        lines.append('--- %d person%s per frame (%d instances, %d triangles per call) ---' % (persons, '' if persons == 1 else 's', idx.shape[0], idx.shape[0] * faces.shape[0]))
        ms, why = traces[persons]
        if ms is None:
            lines.append('per pass: not measured (%s)' % why)
        else:
            for name, _ in PASSES:
                fl = floors[name]
                t = ms.get(name)
                if t is None:
                    lines.append('%-9s not found in the kernel trace' % name)
                elif fl is None:
                    lines.append('%-9s %8.4f ms / frame   (no floor from shapes: atomics on covered fragments)' % (name, t / F))
                else:
                    floor_ms = fl / (HBM_PEAK_TBS * 1e12) * 1e3
                    lines.append('%-9s %8.4f ms / frame   floor %.5f ms (%.2f MB)   %.0f %% of the floor rate' % (name, t / F, floor_ms, fl / 1e6, 100 * floor_ms / (t / F)))
            lines.append('%-9s %8.4f ms / frame   (sum of the passes, kernel time under rocprofv3, %d calls)' % ('kernels', sum(ms.values()) / F, a.calls))
        call, frames, out = resident(persons)
        k_ms, k_calls = timed(call)
        lines.append('entry point, inputs resident      %8.4f ms / frame (%.2f ms / call over %d calls, device events)' % (k_ms / F, k_ms, k_calls))
        r = Renderer(faces)
        r.workspace_cap_bytes = 2 << 30                                    # one library call for the 64 frames
        d_verts = torch.from_numpy(verts).cuda()
        w_ms, w_calls = timed(lambda: r.render_frames(frames, idx, d_verts, cams, colors, out=out))
        lines.append('render_frames, one chunk          %8.4f ms / frame (%.2f ms / call over %d calls; device vertices, host cameras)' % (w_ms / F, w_ms, w_calls))
        r.workspace_cap_bytes = Renderer.workspace_cap_bytes
        c_ms, c_calls = timed(lambda: r.render_frames(frames, idx, d_verts, cams, colors, out=out))
        lines.append('render_frames, default 256 MB cap %8.4f ms / frame (%.2f ms / call over %d calls; %d frames per chunk)'
                     % (c_ms / F, c_ms, c_calls, Renderer.workspace_cap_bytes // (8 * px)))
        drawn = int((out != frames).any(dim=-1).sum())
        lines.append('pixels drawn: %.2f %% of the %d frames' % (100.0 * drawn / (F * px), F))
        del call, frames, out, r, d_verts
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
