"""The XCD-team protocol has one home: csrc/team_common.h.  Reads the sources under csrc/ (compiles nothing, needs no GPU) and asserts that
the pieces a copy would have to carry -- the XCC-id read, the granule store, the arrival bound -- appear in that header only."""
from __future__ import annotations

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tacotronv2_wavernn_chinese_amd', 'csrc')
HOME = 'team_common.h'


def _files_with(needle: str) -> list[str]:
    out = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h')) and needle in open(os.path.join(CSRC, name), encoding='utf-8').read():
            out.append(name)
    return out


def test_xcc_id_is_read_in_the_header_only():
    assert _files_with('hwreg(HW_REG_XCC_ID)') == [HOME]


def test_granule_store_is_in_the_header_only():
    assert _files_with('global_store_dwordx2') == [HOME]


def test_arrival_bound_is_used_in_the_header_only():
    assert _files_with('WRNN_ARRIVE_POLLS') == [HOME]
