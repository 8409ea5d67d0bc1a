"""Host side of WRNN_KERNEL_TEAMG_BATCH (several rows per XCD team in lock-step, any model dims): the id, the three new exports, the plan
with a rows-per-team argument (`wrnn_teamg_batch_plan`, pure host code) on the dim sets of tests/teamg_cases.py, and the CLI flag.  No GPU."""
import os
import re

import pytest

from tests.teamg_cases import DIM_SETS, LDS_BYTES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, 'RAW') for s in 'ABCD'] + [('A', 'MOL'), ('B', 'MOL')]
ROWS = (1, 2, 4, 8)
# what must be accepted; everything else of ROWS may be either
MUST = {'A': (1, 2, 4, 8), 'B': (1, 2, 4, 8), 'C': (1, 2), 'D': (1, 2, 4)}


def _plan(name, mode, rows, budget=-1):
    from tacotronv2_wavernn_chinese_amd import _cabi
    return _cabi.teamg_batch_plan(rows, budget, mode=mode, **DIM_SETS[name])


def _accepted(name, mode):
    """rows per team -> plan, for every R of ROWS the plan accepts; the ones it must accept are asserted."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    out = {}
    for R in ROWS:
        try:
            out[R] = _plan(name, mode, R)
        except _cabi.WrnnError as e:
            assert e.code == _cabi.ERR_UNSUPPORTED and R not in MUST[name], (name, mode, R, e)
    return out


def test_kernel_id_matches_the_header_and_the_abi_stays_9():
    from tacotronv2_wavernn_chinese_amd import _cabi
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    assert int(re.search(r'#define WRNN_KERNEL_TEAMG_BATCH (\d+)', hdr).group(1)) == 7
    assert _cabi.KERNEL_TEAMG_BATCH == 7 and _cabi.KERNEL_IDS['teamg_batch'] == 7 and _cabi.KERNEL_NAMES[7] == 'teamg_batch'
    assert _cabi.ABI_VERSION == 9 and int(re.search(r'#define WRNN_ABI_VERSION (\d+)', hdr).group(1)) == 9
    assert _cabi.load_library().wrnn_abi_version() == 9


def test_the_three_new_symbols_are_exported():
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    for s in ('wrnn_teamg_batch_plan', 'wrnn_last_batch_rows', 'wrnn_debug_teamg_lds_budget'):
        assert s in _cabi.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(rf'\b{s}\s*\(', hdr)


@pytest.mark.parametrize('name,mode', CASES)
def test_one_row_is_the_one_row_plan_field_for_field(name, mode):
    from tacotronv2_wavernn_chinese_amd import _cabi
    for budget in (-1, 0, 40000):
        assert _plan(name, mode, 1, budget) == _cabi.teamg_plan(budget, mode=mode, **DIM_SETS[name])


@pytest.mark.parametrize('name,mode', CASES)
def test_plan_at_every_accepted_row_count(name, mode):
    from tacotronv2_wavernn_chinese_amd import _cabi
    one = _cabi.teamg_plan(-1, mode=mode, **DIM_SETS[name])
    plans = _accepted(name, mode)
    assert set(MUST[name]) <= set(plans)
    prev = None
    for R in sorted(plans):
        p = plans[R]
        assert p['lds_bytes'] <= LDS_BYTES
        assert p['lds_bytes'] == p['activation_bytes'] + sum(L['lds_bytes'] for L in p['layers'].values())
        assert p['mail_granules'] == R * one['mail_granules']
        for lname, L in p['layers'].items():
            assert L['resident_bytes_team'] + L['streamed_bytes_step'] == L['weight_bytes'], (R, lname)
            for f in ('units', 'rows_per_unit', 'k', 'k_padded', 'own_first', 'own_count', 'rows_min', 'rows_max', 'weight_bytes'):
                assert L[f] == one['layers'][lname][f], (R, lname, f)          # ownership and the image do not depend on R
        assert p['streamed_bytes_step'] == sum(L['streamed_bytes_step'] for L in p['layers'].values())
        if prev is not None:
            assert p['activation_bytes'] >= prev['activation_bytes']
            for lname, L in p['layers'].items():
                assert L['resident_bytes_team'] <= prev['layers'][lname]['resident_bytes_team'], (R, lname)
        prev = p


@pytest.mark.parametrize('name,mode', CASES)
def test_resident_bytes_are_monotone_in_the_budget_at_every_row_count(name, mode):
    for R, dflt in _accepted(name, mode).items():
        default = dflt['lds_budget_bytes']
        assert default == LDS_BYTES - dflt['activation_bytes']
        prev = None
        for b in sorted({0, 1000, 5000, 20000, 50000, 90000, 120000, default, default + 1}):
            p = _plan(name, mode, R, b)
            assert p['lds_bytes'] <= LDS_BYTES and p['activation_bytes'] == dflt['activation_bytes']
            res = {n: L['resident_bytes_team'] for n, L in p['layers'].items()}
            if prev is not None:
                assert all(res[n] >= prev[n] for n in res), (R, b, res, prev)
            prev = res
        assert res == {n: L['resident_bytes_team'] for n, L in dflt['layers'].items()}    # above the default = the default


def test_refusals():
    from tacotronv2_wavernn_chinese_amd import _cabi
    with pytest.raises(_cabi.WrnnError) as e:       # eight rows' input vectors of 1024 / 1024 alone exceed 160 KiB, and so does their mailbox
        _plan('C', 'RAW', 8)
    assert e.value.code == _cabi.ERR_UNSUPPORTED
    for R in (0, 9, -1):
        with pytest.raises(_cabi.WrnnError) as e:
            _plan('A', 'RAW', R)
        assert e.value.code == _cabi.ERR_INVALID, R
    with pytest.raises(_cabi.WrnnError) as e:
        _cabi.teamg_batch_plan(2, mode='RAW', **dict(DIM_SETS['A'], rnn_dims=2048))
    assert e.value.code == _cabi.ERR_INVALID


def test_cli_accepts_kernel_teamg_batch():
    from tacotronv2_wavernn_chinese_amd import gen
    assert gen.build_parser().parse_args(['--kernel', 'teamg_batch']).kernel == 'teamg_batch'
    assert gen.build_parser().parse_args([]).kernel == 'auto'
