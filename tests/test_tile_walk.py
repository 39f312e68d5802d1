"""CPU: the tile walk of the persistent scaled-plane product (tepose_amd/csrc/walk.h) as plain C++ -- tests/c_client/tile_walk_check.cpp, compiled with the
host compiler and run: both walks are permutations of the tiles for every group size / grid / tile count (partial last rounds included), walk 0 is the map the
kernel had before, walk 1 keeps a round of the chip inside two row groups and an XCD's patch what it was, and the fallback cases are walk 0."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_walk_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail('no host C++ compiler (c++ / g++ / clang++) on PATH')
    exe = str(tmp_path / 'tile_walk_check')
    cmd = [cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'tepose_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'c_client', 'tile_walk_check.cpp'), '-o', exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'ok %d' % (2 * 5 * 6 * 8 * 5)
