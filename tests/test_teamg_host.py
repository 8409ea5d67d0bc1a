"""Host side of WRNN_KERNEL_TEAMG (the XCD-team kernel for any model dims): the ids, the two new exports, the ownership / placement plan
(`wrnn_teamg_plan`, pure host code) on the four dim sets of tests/teamg_cases.py, and the CLI flag.  No GPU."""
import os
import re

import pytest

from tests.teamg_cases import DIM_SETS, LDS_BYTES, layer_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, 'RAW') for s in 'ABCD'] + [('A', 'MOL'), ('B', 'MOL')]


def _plan(name, mode, budget=-1):
    from tacotronv2_wavernn_chinese_amd import _cabi
    return _cabi.teamg_plan(budget, mode=mode, **DIM_SETS[name])


def test_kernel_id_matches_the_header_and_the_abi_stays_9():
    from tacotronv2_wavernn_chinese_amd import _cabi
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    assert int(re.search(r'#define WRNN_KERNEL_TEAMG (\d+)', hdr).group(1)) == 6
    assert _cabi.KERNEL_TEAMG == 6 and _cabi.KERNEL_IDS['teamg'] == 6 and _cabi.KERNEL_NAMES[6] == 'teamg'
    assert _cabi.ABI_VERSION == 9 and int(re.search(r'#define WRNN_ABI_VERSION (\d+)', hdr).group(1)) == 9
    assert _cabi.load_library().wrnn_abi_version() == 9


def test_the_two_new_symbols_are_exported():
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    for s in ('wrnn_teamg_plan', 'wrnn_debug_teamg_lds_budget'):
        assert s in _cabi.EXPORTED_SYMBOLS and hasattr(lib, s)


def test_plan_struct_mirrors_the_header(tmp_path):
    """sizeof / offsetof of the two new structs, printed by a C program that includes the header."""
    import ctypes as C
    import subprocess
    from tacotronv2_wavernn_chinese_amd import _cabi
    structs = {'wrnn_teamg_layer_info': _cabi.TeamgLayerInfo, 'wrnn_teamg_plan_info': _cabi.TeamgPlanInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/wavernn_amd.h"', 'int main(void) {']
    for cname, st in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines + ['  return 0;', '}']))
    subprocess.check_call(['gcc', '-std=c11', '-o', str(tmp_path / 'layout'), str(src)])
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in subprocess.check_output([str(tmp_path / 'layout')], text=True).split('\n') if l.strip()}
    for cname, st in structs.items():
        assert got[(cname, 'size')] == C.sizeof(st)
        for f, _ in st._fields_:
            assert got[(cname, f)] == getattr(st, f).offset, (cname, f)


@pytest.mark.parametrize('name,mode', CASES)
def test_every_row_is_owned_exactly_once(name, mode):
    p = _plan(name, mode)
    for lname, (units, rpu, k) in layer_shapes(DIM_SETS[name], mode).items():
        L = p['layers'][lname]
        assert (L['units'], L['rows_per_unit'], L['k']) == (units, rpu, k)
        assert L['k_padded'] % 64 == 0 and k <= L['k_padded'] < k + 128
        owners = [0] * units
        for g in range(32):
            for u in range(L['own_first'][g], L['own_first'][g] + L['own_count'][g]):
                owners[u] += 1
        assert owners == [1] * units, lname
        rows = [c * rpu for c in L['own_count']]
        assert (min(rows), max(rows)) == (L['rows_min'], L['rows_max'])
        assert L['weight_bytes'] == 4 * units * rpu * k


def test_set_b_has_workgroups_without_hidden_units():
    p = _plan('B', 'RAW')
    assert p['layers']['rnn1']['own_count'].count(0) >= 2 and p['layers']['rnn1']['rows_min'] == 0
    assert p['layers']['fc1']['own_count'].count(0) >= 2


@pytest.mark.parametrize('name,mode', CASES)
def test_resident_plus_streamed_is_the_layer_and_lds_fits(name, mode):
    for budget in (-1, 0, 4096, 40000, 100000, 10 ** 9):
        p = _plan(name, mode, budget)
        assert p['lds_bytes'] <= LDS_BYTES
        assert p['lds_bytes'] == p['activation_bytes'] + sum(L['lds_bytes'] for L in p['layers'].values())
        assert sum(L['lds_bytes'] for L in p['layers'].values()) <= p['lds_budget_bytes'] <= LDS_BYTES - p['activation_bytes']
        for lname, L in p['layers'].items():
            assert L['resident_bytes_team'] + L['streamed_bytes_step'] == L['weight_bytes'], (budget, lname)
            assert 0 <= L['resident_bytes_wg'] <= L['lds_bytes']
            assert L['resident_bytes_wg'] == 4 * min(L['resident_units'], max(L['own_count'])) * L['rows_per_unit'] * L['k']
        assert p['streamed_bytes_step'] == sum(L['streamed_bytes_step'] for L in p['layers'].values())
        if budget == 0:
            assert all(L['resident_bytes_team'] == 0 and L['lds_bytes'] == 0 for L in p['layers'].values())
            assert p['lds_bytes'] == p['activation_bytes']


@pytest.mark.parametrize('name,mode', CASES)
def test_resident_bytes_are_monotone_in_the_budget(name, mode):
    default = _plan(name, mode)['lds_budget_bytes']
    budgets = sorted({0, 1000, 5000, 20000, 50000, 90000, 120000, default, default + 1})
    prev = None
    for b in budgets:
        p = _plan(name, mode, b)
        res = {n: L['resident_bytes_team'] for n, L in p['layers'].items()}
        if prev is not None:
            assert all(res[n] >= prev[n] for n in res), (b, res, prev)
        prev = res
    assert res == {n: L['resident_bytes_team'] for n, L in _plan(name, mode)['layers'].items()}    # above the default = the default


def test_small_model_is_almost_resident_and_the_large_one_streams():
    a, c = _plan('A', 'RAW'), _plan('C', 'RAW')
    tot = lambda p: sum(L['weight_bytes'] for L in p['layers'].values())
    assert a['streamed_bytes_step'] <= 0.15 * tot(a)
    assert c['streamed_bytes_step'] >= 0.9 * tot(c)


def test_plan_refuses_bad_dims():
    from tacotronv2_wavernn_chinese_amd import _cabi
    with pytest.raises(_cabi.WrnnError):
        _cabi.teamg_plan(-1, mode='RAW', **dict(DIM_SETS['A'], rnn_dims=2048))
    with pytest.raises(_cabi.WrnnError):
        _cabi.teamg_plan(-1, mode='RAW', **dict(DIM_SETS['A'], res_out_dims=98))


def test_cli_accepts_kernel_teamg():
    from tacotronv2_wavernn_chinese_amd import gen
    assert gen.build_parser().parse_args(['--kernel', 'teamg']).kernel == 'teamg'
    assert gen.build_parser().parse_args([]).kernel == 'auto'
    with pytest.raises(SystemExit):
        gen.build_parser().parse_args(['--kernel', 'nope'])
