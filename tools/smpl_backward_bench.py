#!/usr/bin/env python3
"""Timing of the SMPL backward (tepose_smpl_bwd) next to the forward (tepose_smpl_fwd) -> profiles/smpl_backward.txt.

  python tools/smpl_backward_bench.py                      device-event time per call at N = 1, 16, 450, 8192, with the byte floors from shapes
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/smpl_backward_bench.py --loop 8192 20
                                                           a plain loop of backward calls for a kernel trace of its own (the per-kernel split)

Nothing is gated: a new feature has no parent number.  A figure that was not measured is not printed."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tepose_amd import _lib, synth  # noqa: E402
from tepose_amd.engine import Engine  # noqa: E402
from tepose_amd.smpl import SMPL  # noqa: E402

NV, VERT_LD, BLEND_K, SKIN_BLOCKS, CHUNKS = 6890, 20672, 224, 14, 323
HBM_BYTES_PER_S, CACHE_BYTES = 8e12, 256 * 2 ** 20
TABLE_BYTES = 3 * NV * BLEND_K * 4                       # the exact fp32 blend table: 18.5 MB


def blend_splits(N):
    """csrc/shapes.h blend_bwd_shape restated for the byte floors: (persons per workgroup, splits of K); 2048 = 8 workgroups x 256 CUs.  Held to the
    header, with SKIN_BLOCKS and CHUNKS, by tests/test_smpl_bwd_host.py (the host shape check prints the header's answer)."""
    pt = 8 if N <= 8 else 32
    tiles = (N + pt - 1) // pt
    splits = min(CHUNKS, max(1, (2048 + tiles - 1) // tiles))
    per = (CHUNKS + splits - 1) // splits
    return pt, (CHUNKS + per - 1) // per


def floors(N):
    """Bytes each stage has to move at least, from shapes: name -> bytes."""
    _, splits = blend_splits(N)
    pv = N * NV
    return {
        'recompute (prep + blend product: table once, v_posed out)': TABLE_BYTES + 12 * pv,
        'skinning backward (v_posed, g_verts in; g_vposed out; partials out)': 36 * pv + N * SKIN_BLOCKS * 288 * 4,
        'blend backward (table once, g_vposed in, partials out and in)': TABLE_BYTES + 12 * pv + 2 * splits * N * BLEND_K * 4,
        'chain backward (partials in)': N * SKIN_BLOCKS * 288 * 4,
    }


def setup():
    dev = torch.device('cuda', 0)
    smpl = SMPL.from_tables(synth.synthetic_smpl(0), batch_size=1).to(dev)
    eng = Engine(1, 64)
    eng.pack_smpl(smpl, dev)
    return dev, eng


def calls(dev, eng, N):
    g = torch.Generator().manual_seed(N)
    pose = (0.3 * torch.randn(N, 72, generator=g)).to(dev)
    betas = (0.5 * torch.randn(N, 10, generator=g)).to(dev)
    g_verts = torch.randn(N, NV, 3, generator=g).to(dev)
    g_joints = torch.randn(N, 49, 3, generator=g).to(dev)
    verts, joints = torch.empty(N, NV, 3, device=dev), torch.empty(N, 49, 3, device=dev)
    g_pose, g_betas = torch.empty(N, 72, device=dev), torch.empty(N, 10, device=dev)
    ws_f = torch.empty(eng.workspace_bytes(max(1, (N + 1) // 2), 1), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(int(eng.lib.tepose_smpl_bwd_workspace_bytes(eng.handle, N)), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def fwd():
        _lib.check(eng.lib.tepose_smpl_fwd(eng.handle, 1, pose.data_ptr(), betas.data_ptr(), N, verts.data_ptr(), joints.data_ptr(), ws_f.data_ptr(),
                                           ws_f.numel(), st), 'tepose_smpl_fwd')

    def bwd():
        _lib.check(eng.lib.tepose_smpl_bwd(eng.handle, 1, pose.data_ptr(), betas.data_ptr(), N, g_verts.data_ptr(), g_joints.data_ptr(), g_pose.data_ptr(),
                                           g_betas.data_ptr(), ws_b.data_ptr(), ws_b.numel(), st), 'tepose_smpl_bwd')
    return fwd, bwd, ws_b.numel()


def event_ms(f, reps):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        f()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    if not torch.cuda.is_available():
        sys.exit('smpl_backward_bench: no GPU (nothing is measured without one)')
    dev, eng = setup()
    if '--loop' in sys.argv:
        i = sys.argv.index('--loop')
        N, reps = int(sys.argv[i + 1]), int(sys.argv[i + 2])
        _, bwd, _ = calls(dev, eng, N)
        for _ in range(reps):
            bwd()
        torch.cuda.synchronize()
        print('looped tepose_smpl_bwd N = %d x %d' % (N, reps))
        return
    print('device-event time per call (ms), %s' % torch.cuda.get_device_name(0))
    print('%6s %12s %12s %8s %14s' % ('N', 'smpl_fwd', 'smpl_bwd', 'bwd/fwd', 'bwd workspace'))
    rows, ws_bytes = [], {}
    for N in (1, 16, 450, 8192):
        fwd, bwd, ws = calls(dev, eng, N)
        reps = 200 if N <= 450 else 20
        tf, tb = event_ms(fwd, reps), event_ms(bwd, reps)
        rows.append((N, tb))
        ws_bytes[N] = ws
        print('%6d %12.4f %12.4f %8.2f %11.1f MB' % (N, tf, tb, tb / tf, ws / 1e6), flush=True)
    print()
    print('byte floors from shapes (8 TB/s HBM peak; Infinity Cache 256 MB):')
    for N, tb in rows:
        fl = floors(N)
        total = sum(fl.values())
        # which side of the Infinity Cache: the call's whole footprint -- its workspace (every buffer of the recompute and of the backward), the
        # caller's g_verts and the fp32 table and its planes in the blob -- against 256 MiB; above 3/4 of it "borderline" (other traffic shares the cache)
        foot = ws_bytes[N] + 12 * N * NV + 3 * TABLE_BYTES
        side = 'inside' if foot < 0.75 * CACHE_BYTES else 'borderline: inside, above 3/4 of' if foot < CACHE_BYTES else 'beyond'
        print('N = %d: %.1f MB moved at least = %.4f ms at peak; measured %.4f ms = %.1f x the floor; footprint (workspace + g_verts + tables) %.1f MB: %s the Infinity Cache'
              % (N, total / 1e6, total / HBM_BYTES_PER_S * 1e3, tb, tb / (total / HBM_BYTES_PER_S * 1e3), foot / 1e6, side))
        for k, v in fl.items():
            print('    %-72s %10.2f MB  %8.4f ms' % (k, v / 1e6, v / HBM_BYTES_PER_S * 1e3))


if __name__ == '__main__':
    main()
