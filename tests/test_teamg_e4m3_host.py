"""Host side of the e4m3 weight image of WRNN_KERNEL_TEAMG / WRNN_KERNEL_TEAMG_BATCH: the new export and constant, the plan for 1-byte
weights (`wrnn_teamg_plan_fmt`, pure host code) on the dim sets of tests/teamg_cases.py, the row layout, the properties of the restatement
tests/teamg_e4m3_ref.py that the GPU tests lean on, the CLI flag and the validation of the property.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import teamg_e4m3_ref as ref
from tests.teamg_cases import DIM_SETS, LDS_BYTES, layer_shapes
from tests.test_gpu_teamg_e4m3 import DIM_SET_E
from tests.test_teamg_host import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS = (-1, 0, 4096, 40000, 10 ** 9)                                        # those of tests/test_teamg_f16_host.py
ALL_SETS = dict(DIM_SETS, E=DIM_SET_E)


def _fmt(name, mode, rows, weights, budget=-1):
    from tacotronv2_wavernn_chinese_amd import _cabi
    return _cabi.teamg_plan_fmt(rows, weights, budget, mode=mode, **ALL_SETS[name])


def test_the_new_symbol_and_constant_and_the_abi_stays_9():
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    s = 'wrnn_teamg_weight_scales'
    assert s in _cabi.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(rf'\b{s}\(', hdr)
    assert int(re.search(r'#define WRNN_WEIGHTS_E4M3 (\d+)', hdr).group(1)) == 3 == _cabi.TEAMG_WEIGHT_FORMATS['e4m3']
    assert 'reserved' in hdr
    assert _cabi.WEIGHT_FORMATS == {'f32': 0, 'f16': 1}
    assert _cabi.TEAMG_WEIGHT_FORMATS == {'f32': 0, 'f16': 1, 'e4m3': 3}
    assert _cabi.TEAMG_WEIGHT_FORMAT_NAMES == {0: 'f32', 1: 'f16', 3: 'e4m3'}
    assert _cabi.ABI_VERSION == 9 and int(re.search(r'#define WRNN_ABI_VERSION (\d+)', hdr).group(1)) == 9
    assert lib.wrnn_abi_version() == 9
    assert C.sizeof(_cabi.SampleOpts) == 88
    assert tuple(ref.LAYERS[:5]) == tuple(_cabi.TEAMG_LAYER_NAMES[:5])
    out = (C.c_float * 6)()
    assert lib.wrnn_teamg_weight_scales(None, out) == _cabi.ERR_INVALID


@pytest.mark.parametrize('name,mode', CASES)
def test_e4m3_plan_counts_one_byte_weights(name, mode):
    shapes = layer_shapes(DIM_SETS[name], mode)
    for budget in BUDGETS:
        p8, p16, p32 = (_fmt(name, mode, 1, w, budget) for w in ('e4m3', 'f16', 'f32'))
        assert p8['lds_bytes'] <= LDS_BYTES
        assert p8['activation_bytes'] == p32['activation_bytes'] and p8['mail_granules'] == p32['mail_granules']
        assert p8['lds_budget_bytes'] == p32['lds_budget_bytes']
        assert p8['lds_bytes'] == p8['activation_bytes'] + sum(L['lds_bytes'] for L in p8['layers'].values())
        assert p8['streamed_bytes_step'] == sum(L['streamed_bytes_step'] for L in p8['layers'].values())
        for lname, (units, rpu, k) in shapes.items():
            a, h, b = p8['layers'][lname], p16['layers'][lname], p32['layers'][lname]
            assert (a['units'], a['rows_per_unit'], a['k']) == (units, rpu, k)
            assert a['weight_bytes'] == units * rpu * k and b['weight_bytes'] == 4 * a['weight_bytes']
            assert a['resident_bytes_team'] + a['streamed_bytes_step'] == a['weight_bytes']
            assert a['k_padded'] == b['k_padded'] and a['k_padded'] % 64 == 0
            assert a['lds_bytes'] == a['resident_units'] * rpu * a['k_padded']
            assert a['resident_units'] >= h['resident_units'] >= b['resident_units'], (lname, budget)
            assert a['own_first'] == b['own_first'] and a['own_count'] == b['own_count']
            assert (a['rows_min'], a['rows_max']) == (b['rows_min'], b['rows_max'])


def test_refusals_are_those_of_fp32_and_code_2_stays_invalid():
    from tacotronv2_wavernn_chinese_amd import _cabi
    for name in 'ABCD':
        for R in (1, 2, 4, 8):
            codes = []
            for w in ('f32', 'e4m3'):
                try:
                    _fmt(name, 'RAW', R, w)
                    codes.append(0)
                except _cabi.WrnnError as e:
                    codes.append(e.code)
            assert codes[0] == codes[1], (name, R, codes)
    for R in (0, 9):
        with pytest.raises(_cabi.WrnnError) as e:
            _fmt('A', 'RAW', R, 'e4m3')
        assert e.value.code == _cabi.ERR_INVALID
    for bad in ('bf16', 'int8', 'F16', 'E4M3', 'fp8', 1, 3):               # (None means "no format given" to teamg_plan)
        with pytest.raises(ValueError):
            _fmt('A', 'RAW', 1, bad)
    lib = _cabi.load_library()
    info, cfg = _cabi.TeamgPlanInfo(), _cabi.Config()
    d = DIM_SETS['A']
    cfg.rnn_dims, cfg.fc_dims, cfg.bits, cfg.pad, cfg.n_upsample = d['rnn_dims'], d['fc_dims'], d['bits'], d['pad'], len(d['upsample_factors'])
    for i, s in enumerate(d['upsample_factors']):
        cfg.upsample_factors[i] = s
    cfg.feat_dims, cfg.compute_dims, cfg.res_out_dims, cfg.res_blocks = d['feat_dims'], d['compute_dims'], d['res_out_dims'], d['res_blocks']
    cfg.hop_length, cfg.sample_rate = d['hop_length'], d['sample_rate']
    assert lib.wrnn_teamg_plan_fmt(C.byref(cfg), 1, 3, -1, C.byref(info)) == 0
    for code in (2, 4, -1):
        assert lib.wrnn_teamg_plan_fmt(C.byref(cfg), 1, code, -1, C.byref(info)) == _cabi.ERR_INVALID


@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D', 'E'])
def test_the_row_layout_is_a_bijection_with_16_byte_quads(name):
    """Every row of every layer: the positions of its KP elements are a permutation of the row's KP bytes; lane q's 16 bytes of the four
    steps of a quad are contiguous and 16-byte aligned (rows are KP bytes apart, a multiple of 64); a pair's 8 bytes likewise, 8-byte
    aligned; k ascends inside every piece.  The segment lengths that occur are recorded, so that set E's quad-less 3 is known to be run."""
    p = _fmt(name, 'RAW', 1, 'e4m3')
    A = ALL_SETS[name]['res_out_dims'] // 4
    H = ALL_SETS[name]['rnn_dims']
    seen = set()
    for lname, L in p['layers'].items():
        KP = L['k_padded']
        KAP = {'rnn2': (H + A + 63) // 64 * 64, 'rnn1': (H + 63) // 64 * 64}.get(lname, KP)
        nA, nK = KAP // 64, KP // 64
        seen |= {nA, nK - nA} - {0}
        for row in sorted({0, 1, 2, 3, 5, L['rows_per_unit'] * max(L['own_count']) - 1}):
            at = np.array([ref.pos(e, row, KAP, KP) for e in range(KP)])
            assert sorted(at) == list(range(KP)), (lname, row)
            for k0, k1 in ((0, nA), (nA, nK)):
                n = k1 - k0
                for q in range(16):
                    for j in range(n // 4):
                        b = [at[64 * (k0 + 4 * j + u) + 4 * q + c] for u in range(4) for c in range(4)]
                        assert b[0] % 16 == 0 and b == list(range(b[0], b[0] + 16)), (lname, row, q, j)
                        assert 64 * (k0 + 4 * j) <= b[0] < 64 * (k0 + 4 * j + 4)
                    if n & 2:
                        kp = k0 + (n & ~3)
                        b = [at[64 * (kp + u) + 4 * q + c] for u in range(2) for c in range(4)]
                        assert b[0] % 8 == 0 and b == list(range(b[0], b[0] + 8))
            # two rows that one 16-byte LDS read serves together never meet on a bank: lanes {0-3, 12-15} of one, {4-11} of the other
            for other in (row + 1, row + 3):
                for k in range(0, (nA // 4) * 4, 4):
                    s0 = {((row * KP + ref.pos(64 * k + 4 * q, row, KAP, KP)) // 16) % 16 for q in (0, 1, 2, 3, 12, 13, 14, 15)}
                    s1 = {((other * KP + ref.pos(64 * k + 4 * q, other, KAP, KP)) // 16) % 16 for q in range(4, 12)}
                    assert len(s0) == len(s1) == 8 and not (s0 & s1), (lname, row, other)
    if name == 'E':
        assert seen == {1, 3}, seen                                            # pair then single, no quad
    if name == 'D':
        assert {8, 9} <= seen


def _sd(name, mode='RAW', seed=7):
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    return {k: np.array(v) for k, v in make_state_dict(seed, mode, 'peaky' if mode == 'RAW' else 'default', **ALL_SETS[name]).items()}


@pytest.mark.parametrize('name', ['B', 'E', 'D'])
def test_restatement_properties(name):
    """Derived, not measured.  A weight whose |w / s| is in e4m3's normal range [2^-6, 448] keeps half an ulp of 4 significand bits:
    |dw| <= 2^-4 |w|.  Below it the spacing is the smallest subnormal 2^-9, so |dw| <= s 2^-10.  s is the smallest power of two that
    brings the layer's maximum to 448 or below, so the maximum lands in (224, 448], and 448 is a value of the format, so it stays
    there.  Values that are already e4m3 multiples of s with the same maximum are a fixed point."""
    sd = _sd(name)
    sd8, scales = ref.quantise(sd)
    assert scales.dtype == np.float32 and scales.shape == (6,)
    for layer, s in zip(ref.LAYERS, scales):
        m, e = np.frexp(np.float64(s))
        assert m == 0.5 and s >= 2.0 ** -126                                   # a power of two, a normal float
        x, x8, s2 = ref.stored(sd, layer)
        assert s2 == s
        normal = np.abs(x) >= ref.E4M3_MIN_NORMAL
        assert (np.abs(x8[normal] - x[normal]) <= 2.0 ** -4 * np.abs(x[normal])).all(), layer
        assert (np.abs(x8[~normal] - x[~normal]) <= 2.0 ** -10).all(), layer
        assert 224.0 < np.abs(x8).max() <= 448.0, (layer, np.abs(x8).max())
        assert np.isfinite(x8).all()
        for k in ref.LAYER_KEYS[layer]:
            w, w8 = ref._part(k, sd[k]), ref._part(k, sd8[k])
            big = np.abs(w) >= s * np.float32(ref.E4M3_MIN_NORMAL)
            assert (np.abs(w8[big] - w[big]) <= 2.0 ** -4 * np.abs(w[big])).all()
            assert (np.abs(w8[~big] - w[~big]) <= s * 2.0 ** -10).all()
    np.testing.assert_array_equal(sd8['I.weight'][:, 0], sd['I.weight'][:, 0])
    for k in sd:
        if not any(k in keys for keys in ref.LAYER_KEYS.values()):
            np.testing.assert_array_equal(sd8[k], sd[k])
    again, scales2 = ref.quantise(sd8)
    np.testing.assert_array_equal(scales2, scales)
    for k in sd8:
        np.testing.assert_array_equal(again[k], sd8[k], err_msg=k)


def test_scale_of_edges():
    assert ref.scale_of(0.0) == 1.0
    assert ref.scale_of(448.0) == 1.0 and ref.scale_of(float(np.nextafter(np.float32(448), np.float32(1e9)))) == 2.0
    assert ref.scale_of(224.0) == 0.5 and ref.scale_of(float(np.nextafter(np.float32(224), np.float32(1e9)))) == 1.0
    assert ref.scale_of(1e5) == 256.0 and 1e5 / 256.0 <= 448 < 1e5 / 128.0
    assert ref.scale_of(1e-45) == 2.0 ** -126                                  # the clamp: the scale stays a normal float
    assert ref.scale_of(3.4e38) == 2.0 ** 120
    # torch's cast is what the restatement says it is
    x = np.array([2.0 ** -10, 3 * 2.0 ** -10, -2.0 ** -10, 2.0 ** -9, 0.0, -0.0, 17.0, 19.0, 448.0], np.float32)
    r = ref.e4m3_round(x)
    np.testing.assert_array_equal(r, np.array([0.0, 2.0 ** -8, -0.0, 2.0 ** -9, 0.0, -0.0, 16.0, 20.0, 448.0], np.float32))
    assert np.signbit(r[2]) and np.signbit(r[5]) and not np.signbit(r[4])


def test_model_property_validates_without_a_device():
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**DIM_SETS['B'], mode='RAW')
    assert m.teamg_weights == 'f32'
    m.teamg_weights = 'e4m3'
    assert m.teamg_weights == 'e4m3'
    for bad in ('bf16', 'int8', 'F16', 'E4M3', 1, 3, None):
        with pytest.raises(ValueError):
            m.teamg_weights = bad
    assert m.teamg_weights == 'e4m3'
    m.teamg_weights = 'f16'
    assert m.teamg_weights == 'f16'


def test_cli_flag():
    from tacotronv2_wavernn_chinese_amd import gen
    p = gen.build_parser()
    assert p.parse_args([]).teamg_weights == 'f32'
    assert p.parse_args(['--kernel', 'teamg', '--teamg-weights', 'e4m3']).teamg_weights == 'e4m3'
    assert p.parse_args(['--teamg-weights', 'e4m3']).kernel == 'auto'          # accepted with any kernel
    with pytest.raises(SystemExit):
        p.parse_args(['--teamg-weights', 'bf16'])
    for tool in ('any_dims_latency.py', 'any_dims_batch_latency.py'):
        assert "'e4m3'" in open(os.path.join(ROOT, 'tools', tool)).read(), tool


def test_quality_figures_on_set_d_are_recorded_not_asserted(capsys):
    """The only quality evidence there is without a trained checkpoint (DESIGN.md 3.5d records the figures): on set D, peaky RAW and
    default MOL, how far the oracle's teacher-forced logits on the e4m3-dequantised model are from those on the original, and the share
    of free-run labels that agree -- with the same two figures for the fp16-rounded model.  Printed; nothing depends on their size."""
    from oracle import oracle as orc
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    lines = []
    for mode, bits in (('RAW', DIM_SETS['D']['bits']), ('MOL', 9)):
        dims = dict(DIM_SETS['D'], bits=bits)
        from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
        sd = {k: np.array(v) for k, v in make_state_dict(7, mode, 'peaky' if mode == 'RAW' else 'default', **dims).items()}
        sd8, _ = ref.quantise(sd)
        sd16 = dict(sd)
        for keys in ref.LAYER_KEYS.values():
            for k in keys:
                r = sd[k].astype(np.float16).astype(np.float32)
                if k == 'I.weight':
                    r[:, 0] = sd[k][:, 0]
                sd16[k] = r
        B, L = 2, 64
        mels = make_mels(3, B, 1, feat_dims=dims['feat_dims'])
        rng = np.random.Generator(np.random.PCG64(8))
        if mode == 'RAW':
            noise = (orc.NOISE_EXPO, rng.standard_exponential((L, B, 2 ** bits)).astype(np.float32))
        else:
            noise = (0, rng.uniform(1e-5, 1 - 1e-5, size=(L, B, 10)).astype(np.float32), rng.uniform(1e-5, 1 - 1e-5, size=(L, B)).astype(np.float32))
        runs = {}
        for tag, s in (('f32', sd), ('e4m3', sd8), ('f16', sd16)):
            om = orc.OracleModel(s, mode=mode, bits=bits, upsample_factors=dims['upsample_factors'], pad=dims['pad'], fast=True)
            cm, ca = om.conditioning(mels)
            cm, ca = cm[:, :L], ca[:, :L]
            if tag == 'f32':
                base_free = om.loop(cm, ca, *noise)
            free = om.loop(cm, ca, *noise)
            forced = om.loop(cm, ca, *noise, x_forced=base_free['samples'], want_logits=True)
            runs[tag] = (free, forced)
        top = float(np.abs(runs['f32'][1]['logits']).max())
        for tag in ('e4m3', 'f16'):
            dl = float(np.abs(runs[tag][1]['logits'] - runs['f32'][1]['logits']).max())
            agree = float((runs[tag][0]['labels'] == runs['f32'][0]['labels']).mean())
            lines.append(f'set D {mode} {tag}: max |dlogit| teacher-forced {dl:.3e} (largest logit {top:.2f}), free-run labels equal {100 * agree:.1f} % of {B * L}')
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
