"""Host side of the half-precision weight image of WRNN_KERNEL_TEAMG / WRNN_KERNEL_TEAMG_BATCH: the three new exports, the plan for a weight
format (`wrnn_teamg_plan_fmt`, pure host code) on the dim sets of tests/teamg_cases.py, and the CLI flag.  No GPU."""
import ctypes as C
import os
import re

import pytest

from tests.teamg_cases import DIM_SETS, LDS_BYTES, layer_shapes
from tests.test_teamg_host import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS = (-1, 0, 4096, 40000, 10 ** 9)


def _fmt(name, mode, rows, weights, budget=-1):
    from tacotronv2_wavernn_chinese_amd import _cabi
    return _cabi.teamg_plan_fmt(rows, weights, budget, mode=mode, **DIM_SETS[name])


def test_the_three_new_symbols_are_exported_and_the_abi_stays_9():
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    for s in ('wrnn_teamg_set_weight_format', 'wrnn_teamg_weight_format', 'wrnn_teamg_plan_fmt'):
        assert s in _cabi.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(rf'\b{s}\(', hdr), s
    assert int(re.search(r'#define WRNN_WEIGHTS_F32 (\d+)', hdr).group(1)) == 0 == _cabi.WEIGHT_FORMATS['f32']
    assert int(re.search(r'#define WRNN_WEIGHTS_F16 (\d+)', hdr).group(1)) == 1 == _cabi.WEIGHT_FORMATS['f16']
    assert _cabi.WEIGHT_FORMATS == {'f32': 0, 'f16': 1}
    assert _cabi.ABI_VERSION == 9 and int(re.search(r'#define WRNN_ABI_VERSION (\d+)', hdr).group(1)) == 9
    assert lib.wrnn_abi_version() == 9
    assert C.sizeof(_cabi.SampleOpts) == 88


@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D'])
def test_f32_is_the_existing_plan_field_for_field(name):
    """rows_per_team 1: wrnn_teamg_plan; 2, 4, 8: wrnn_teamg_batch_plan -- the refusals included."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    for budget in BUDGETS:
        assert _fmt(name, 'RAW', 1, 'f32', budget) == _cabi.teamg_plan(budget, mode='RAW', **DIM_SETS[name])
        for R in (2, 4, 8):
            try:
                want = _cabi.teamg_batch_plan(R, budget, mode='RAW', **DIM_SETS[name])
            except _cabi.WrnnError as e:
                with pytest.raises(_cabi.WrnnError) as got:
                    _fmt(name, 'RAW', R, 'f32', budget)
                assert got.value.code == e.code == _cabi.ERR_UNSUPPORTED
                continue
            assert _fmt(name, 'RAW', R, 'f32', budget) == want


@pytest.mark.parametrize('name,mode', CASES)
def test_f16_plan_counts_two_byte_weights(name, mode):
    shapes = layer_shapes(DIM_SETS[name], mode)
    for budget in BUDGETS:
        p16, p32 = _fmt(name, mode, 1, 'f16', budget), _fmt(name, mode, 1, 'f32', budget)
        assert p16['lds_bytes'] <= LDS_BYTES
        assert p16['activation_bytes'] == p32['activation_bytes'] and p16['mail_granules'] == p32['mail_granules']
        assert p16['lds_budget_bytes'] == p32['lds_budget_bytes']
        assert p16['lds_bytes'] == p16['activation_bytes'] + sum(L['lds_bytes'] for L in p16['layers'].values())
        assert p16['streamed_bytes_step'] == sum(L['streamed_bytes_step'] for L in p16['layers'].values())
        for lname, (units, rpu, k) in shapes.items():
            a, b = p16['layers'][lname], p32['layers'][lname]
            assert (a['units'], a['rows_per_unit'], a['k']) == (units, rpu, k)
            assert a['weight_bytes'] == 2 * units * rpu * k and b['weight_bytes'] == 2 * a['weight_bytes']
            assert a['resident_bytes_team'] + a['streamed_bytes_step'] == a['weight_bytes']
            assert a['k_padded'] == b['k_padded'] and a['k_padded'] % 64 == 0
            assert a['lds_bytes'] == 2 * a['resident_units'] * rpu * a['k_padded']
            assert a['resident_units'] >= b['resident_units'], (lname, budget)
            assert a['own_first'] == b['own_first'] and a['own_count'] == b['own_count']
            assert (a['rows_min'], a['rows_max']) == (b['rows_min'], b['rows_max'])


@pytest.mark.parametrize('name', ['C', 'D'])
def test_f16_streams_half_the_bytes_up_to_one_unit_per_workgroup(name):
    """Every dim divides by 32, so the 32 workgroups own the same units.  Half the bytes in total, an equal byte budget and whole-unit
    granularity: what f16 streams is at most half of what f32 streams plus, in each workgroup, the one unit of the partly resident layer
    that no longer fits."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    for R in (1, 2, 4):
        for budget in BUDGETS:
            try:
                p32 = _fmt(name, 'RAW', R, 'f32', budget)
            except _cabi.WrnnError:                                            # 1024 / 1024 at four rows: refused in either format
                continue
            p16 = _fmt(name, 'RAW', R, 'f16', budget)
            partial = [L for L in p16['layers'].values() if 0 < L['resident_units'] < max(L['own_count'])]
            assert len(partial) <= 1
            u = 2 * partial[0]['rows_per_unit'] * partial[0]['k'] if partial else 0
            assert p16['streamed_bytes_step'] <= p32['streamed_bytes_step'] / 2 + 32 * u, (R, budget)


def test_refusals_do_not_depend_on_the_format():
    """The activation vectors stay fp32: what f32 refuses for them, f16 refuses too."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    for name, mode, R in (('D', 'RAW', 8), ('C', 'RAW', 8), ('C', 'RAW', 4)):
        codes = []
        for w in ('f32', 'f16'):
            try:
                _fmt(name, mode, R, w)
                codes.append(0)
            except _cabi.WrnnError as e:
                codes.append(e.code)
        assert codes[0] == codes[1], (name, R, codes)
    for name, R in (('D', 8), ('C', 8)):
        with pytest.raises(_cabi.WrnnError) as e32:
            _cabi.teamg_batch_plan(R, mode='RAW', **DIM_SETS[name])
        with pytest.raises(_cabi.WrnnError) as e16:
            _fmt(name, 'RAW', R, 'f16')
        assert e16.value.code == e32.value.code == _cabi.ERR_UNSUPPORTED
    for R in (0, 9):
        with pytest.raises(_cabi.WrnnError) as e:
            _fmt('A', 'RAW', R, 'f16')
        assert e.value.code == _cabi.ERR_INVALID
    with pytest.raises(ValueError):
        _fmt('A', 'RAW', 1, 'bf16')
    # a format the C entry point does not know
    lib = _cabi.load_library()
    info, cfg = _cabi.TeamgPlanInfo(), _cabi.Config()
    d = DIM_SETS['A']
    cfg.rnn_dims, cfg.fc_dims, cfg.bits, cfg.pad, cfg.n_upsample = d['rnn_dims'], d['fc_dims'], d['bits'], d['pad'], len(d['upsample_factors'])
    for i, s in enumerate(d['upsample_factors']):
        cfg.upsample_factors[i] = s
    cfg.feat_dims, cfg.compute_dims, cfg.res_out_dims, cfg.res_blocks = d['feat_dims'], d['compute_dims'], d['res_out_dims'], d['res_blocks']
    cfg.hop_length, cfg.sample_rate = d['hop_length'], d['sample_rate']
    assert lib.wrnn_teamg_plan_fmt(C.byref(cfg), 1, 1, -1, C.byref(info)) == 0
    assert lib.wrnn_teamg_plan_fmt(C.byref(cfg), 1, 2, -1, C.byref(info)) == _cabi.ERR_INVALID


def test_model_property_validates_without_a_device():
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**DIM_SETS['B'], mode='RAW')
    assert m.teamg_weights == 'f32'
    m.teamg_weights = 'f16'
    assert m.teamg_weights == 'f16'
    for bad in ('bf16', 'F16', 1, None):
        with pytest.raises(ValueError):
            m.teamg_weights = bad
    assert m.teamg_weights == 'f16'


def test_cli_flag():
    from tacotronv2_wavernn_chinese_amd import gen
    p = gen.build_parser()
    assert p.parse_args([]).teamg_weights == 'f32'
    assert p.parse_args(['--kernel', 'teamg', '--teamg-weights', 'f16']).teamg_weights == 'f16'
    assert p.parse_args(['--teamg-weights', 'f16']).kernel == 'auto'          # accepted with any kernel
    with pytest.raises(SystemExit):
        p.parse_args(['--teamg-weights', 'bf16'])
