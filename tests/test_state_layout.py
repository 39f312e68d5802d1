"""CPU: the workspaces as numbers.  The encoder's workspace addressing (tepose_amd/csrc/state.h on formats.h) as plain C++ -- tests/c_client/state_layout_check.cpp, compiled with the
host compiler and run: every carved offset, and the fp32 / plane / blocked reference of every (layer, step, direction), equals the written-out expressions the
header replaced (kept in the program as ref_* functions); the recurrence's chain invariants hold; no reference leaves its buffer.  Where the compiler has
them, the same program once more under the address and undefined-behaviour sanitizers, as a stand-alone executable.  Every other layout of forward.hip
-- regressor and SMPL backward, frame projection, VIBE, and how a whole forward's workspace holds encoder, regressor and feature slot -- the same way:
tests/c_client/workspace_layout_check.cpp, plain and under the sanitizers in one test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = 3 * 2 * 5 * 5 * 4 * 2      # L x Hp x B x T x plan flags x granules
# regressor N x plan flags x L; projection M x h3; VIBE B N x directions x Hp; whole forward: the encoder shapes x regressor flags at B x at 2 B
WS_COMBOS = 9 * 3 * 3 + 8 * 2 + 4 * 2 * 3 + COMBOS * 3 * 3


def _cxx():
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail('no host C++ compiler (c++ / g++ / clang++) on PATH')
    return cxx


def _build(cxx, exe, extra=(), src='state_layout_check.cpp'):
    cmd = [cxx, '-std=c++17', '-O1', '-Wall', '-Werror', *extra, '-I', os.path.join(ROOT, 'tepose_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'c_client', src), '-o', exe]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe, combos=COMBOS):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'ok %d' % combos


def test_state_layout_on_the_host(tmp_path):
    exe = str(tmp_path / 'state_layout_check')
    p = _build(_cxx(), exe)
    assert p.returncode == 0, p.stdout[-3000:]
    _run(exe)


def test_state_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'state_layout_check_san')
    p = _build(_cxx(), exe, ('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'))
    if p.returncode != 0:
        # a host compiler without the sanitizer runtimes: the plain build above is the check
        print(p.stdout[-2000:])
        return
    _run(exe)


def test_workspace_layouts_on_the_host_and_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'workspace_layout_check')
    p = _build(_cxx(), exe, src='workspace_layout_check.cpp')
    assert p.returncode == 0, p.stdout[-3000:]
    _run(exe, WS_COMBOS)
    p = _build(_cxx(), exe + '_san', ('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'), src='workspace_layout_check.cpp')
    if p.returncode != 0:
        print(p.stdout[-2000:])        # a host compiler without the sanitizer runtimes: the plain build above is the check
        return
    _run(exe + '_san', WS_COMBOS)
