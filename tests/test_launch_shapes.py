"""CPU: the launch-shape rules (tepose_amd/csrc/shapes.h on options.h and formats.h) as plain C++ -- tests/c_client/launch_shapes_check.cpp, compiled with
the host compiler and run: which kernel instantiation, grid, block and tile-count arguments a shape gets at every option value equals the expressions the
launchers carried before the header existed (kept in the program as ref_* functions), and the outcomes DESIGN.md states -- 64-row tiles for 444 x 9216,
one round of 128 x 192 tiles for two products of 1024 x 3072, ... -- hold as literals.  Where the compiler has them, the same program once more under
the address and undefined-behaviour sanitizers, as a stand-alone executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = 43                               # default, each A/B switch alone, each forced tile, each threshold moved to either side
PRODUCTS = 27 * 10 * 3 + 55                 # M x N x products, and the shapes on each side of the thresholds that cross product does not straddle
STEPS = 27 * 5 * 3 + 22                     # M x Hp x directions, likewise
LITERALS = 8 + 2 + 8 + 2 + 7                # blocked-plane product, two-accumulator step, width-first product, exact-fp32 tiles, gru_seq row tiles
COMBOS = VARIANTS * (PRODUCTS + STEPS) + LITERALS


def _cxx():
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail('no host C++ compiler (c++ / g++ / clang++) on PATH')
    return cxx


def _build(cxx, exe, extra=()):
    cmd = [cxx, '-std=c++17', '-O1', '-Wall', '-Werror', *extra, '-I', os.path.join(ROOT, 'tepose_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'c_client', 'launch_shapes_check.cpp'), '-o', exe]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'ok %d' % COMBOS


def test_launch_shapes_on_the_host(tmp_path):
    exe = str(tmp_path / 'launch_shapes_check')
    p = _build(_cxx(), exe)
    assert p.returncode == 0, p.stdout[-3000:]
    _run(exe)


def test_launch_shapes_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'launch_shapes_check_san')
    p = _build(_cxx(), exe, ('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'))
    if p.returncode != 0:
        # a host compiler without the sanitizer runtimes: the plain build above is the check
        print(p.stdout[-2000:])
        return
    _run(exe)
