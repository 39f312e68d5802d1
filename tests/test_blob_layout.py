"""CPU: the packed blob's layout and every workspace size are what they were before the weight records (csrc/model.h Weight) replaced the loose offset
fields.  Blobs travel between ranks and are adopted by their float count, and a rank that receives only the fp32 sections rebuilds the planes between
them -- so the packed size, every (offset, size) of tepose_fp32_ranges and the workspace sizes of TePose, VIBE and HMR handles are held to the values
recorded from the build of the commit before that change (tests/golden/blob_layout.json, written by tests/golden/make_golden_layout.py)."""
import importlib.util
import json
import os

import pytest

from tepose_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_golden_layout', os.path.join(GOLDEN, 'make_golden_layout.py'))
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)

with open(os.path.join(GOLDEN, 'blob_layout.json')) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope='module')
def measured():
    return _gen.measure(_lib.load())


def test_the_fixture_covers_every_kind_of_handle(measured):
    assert sorted(measured) == sorted(RECORDED)
    assert {'tepose_L1H64', 'tepose_L2H100', 'tepose_L2H1024', 'tepose_L3H320', 'hmr'} <= set(RECORDED)
    assert sum(k.startswith('vibe_') for k in RECORDED) == len(_gen.VIBE)
    # the figures the change was specified with
    assert RECORDED['tepose_L2H1024']['packed_bytes'] == 824200960 and RECORDED['hmr']['packed_bytes'] == 278914048
    assert len(RECORDED['tepose_L2H1024']['fp32_ranges']) == 5 and len(RECORDED['hmr']['fp32_ranges']) == 4
    assert RECORDED['tepose_L2H1024']['workspace_bytes'][0] == 14581760 and RECORDED['tepose_L2H1024']['workspace_bytes'][3] == 15117392640
    pf = RECORDED['tepose_L2H1024']['project_frames_workspace_bytes']
    assert pf[0] == 18176 and pf[3] == 140542464


@pytest.mark.parametrize('name', sorted(RECORDED))
def test_layout_and_sizes_are_the_recorded_ones(measured, name):
    got, want = measured[name], RECORDED[name]
    assert got['packed_bytes'] == want['packed_bytes']
    assert got['fp32_ranges'] == want['fp32_ranges']
    for key in ('workspace_bytes', 'project_frames_workspace_bytes', 'vibe_workspace_bytes'):
        assert got[key] == want[key], key
