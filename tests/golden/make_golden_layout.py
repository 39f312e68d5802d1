"""Record tests/golden/blob_layout.json: the packed-blob layout and the workspace sizes of a set of handles, as the built library answers them.

    python tests/golden/make_golden_layout.py

Needs no GPU and no reference checkout: every entry point called here answers before any device access.  The fixture was recorded from the build
of the commit before the weight-record refactor; tests/test_blob_layout.py (which imports measure() from here) holds every later build to it.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'blob_layout.json')
SHAPES = [(1, 16), (64, 16), (700, 3), (8192, 16)]          # (B, T)
TEPOSE = [(1, 64), (2, 100), (2, 1024), (3, 320)]            # (L, H)
# (L, H, bidirectional, add_linear): every constructor-flag combination at the C exerciser's size, and the sizes of the VIBE fixtures
VIBE = [(2, 100, b, l) for b in (0, 1) for l in (0, 1)] + [(2, 128, 0, 1), (1, 64, 0, 1), (2, 64, 1, 0), (1, 100, 1, 1), (1, 2048, 0, 0), (2, 96, 0, 0)]


def _handle(lib, h):
    off, size = (ctypes.c_size_t * 64)(), (ctypes.c_size_t * 64)()
    n = lib.tepose_fp32_ranges(h, off, size, 64)
    assert n > 0, n
    return {
        'packed_bytes': lib.tepose_packed_bytes(h),
        'fp32_ranges': [[off[i], size[i]] for i in range(n)],
        'workspace_bytes': [lib.tepose_workspace_bytes(h, B, T) for B, T in SHAPES],
        'project_frames_workspace_bytes': [lib.tepose_project_frames_workspace_bytes(h, B) for B, _ in SHAPES],
        'vibe_workspace_bytes': [lib.tepose_vibe_workspace_bytes(h, B, T) for B, T in SHAPES],
    }


def measure(lib):
    """{handle name: sizes}; handles are created with TEPOSE_ASSUME_CUS=256, so the plans (and with them the carving) do not depend on the machine."""
    old = os.environ.get('TEPOSE_ASSUME_CUS')
    os.environ['TEPOSE_ASSUME_CUS'] = '256'
    out = {}
    try:
        def add(name, rc, h):
            assert rc == 0 and h.value, (name, rc)
            try:
                out[name] = _handle(lib, h)
            finally:
                lib.tepose_destroy(h)
        for L, H in TEPOSE:
            h = ctypes.c_void_p()
            add('tepose_L%dH%d' % (L, H), lib.tepose_create(L, H, ctypes.byref(h)), h)
        for L, H, bidir, lin in VIBE:
            h = ctypes.c_void_p()
            add('vibe_L%dH%d_bi%d_lin%d' % (L, H, bidir, lin), lib.tepose_create_vibe_ex(L, H, bidir, lin, ctypes.byref(h)), h)
        h = ctypes.c_void_p()
        add('hmr', lib.tepose_create_hmr(ctypes.byref(h)), h)
    finally:
        if old is None:
            del os.environ['TEPOSE_ASSUME_CUS']
        else:
            os.environ['TEPOSE_ASSUME_CUS'] = old
    return out


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tepose_amd import _lib
    with open(OUT, 'w') as f:
        json.dump(measure(_lib.load()), f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', OUT)
