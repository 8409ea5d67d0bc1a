"""The 8-bit weight image of WRNN_KERNEL_TEAMG / WRNN_KERNEL_TEAMG_BATCH (`teamg_weights='e4m3'`), section by section as
tests/test_gpu_teamg_f16.py.

An e4m3 byte widens to fp32 exactly, the e4m3 kernels multiply and add in the fp32 kernels' order and multiply a row's sums by the
layer's power-of-two scale, which commutes with every rounding as long as nothing is subnormal.  So a model `sd` run with the e4m3 image
(`m8`) must be BIT-equal -- labels, samples, logits -- to the model `sd8` run with the fp32 image (`m32`), where `sd8` is the restatement's
dequantised model (tests/teamg_e4m3_ref.py: per-layer scale from the layer's maximum, torch's float8_e4m3fn cast, times the scale).
Section 6 compares with the oracle on `sd8` directly under the rules of tests/parity_util.py, nothing loosened.

Before quantising, a handful of entries of every matrix are overwritten with values that land in e4m3's subnormals after scaling, in
both signs, with one tie to even and one tie to zero: a conversion that flushed or mis-rounded them, in the pack or in the kernel, would
show.  Every layer's maximum is inside [2^-20, 2^20] (asserted), so no product of the fp32 kernel on `sd8` is subnormal.

Dim sets A to D of tests/teamg_cases.py with the calls of the f16 file (B, C: hop 6 x 20 frames; A one frame of 128 steps; D one frame of
275), and set E below, whose segments have 3 steps: a pair and a single step with no quad, which no other set runs.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import teamg_e4m3_ref as ref
from tests.parity_util import NEAR_TIE, check_free_run_raw, check_mol, check_teacher_forced_raw, parity_report
from tests.teamg_cases import DIM_SETS

pytestmark = pytest.mark.gpu

# rnn 160: rows of 192 + 192 elements, segments of 3 + 3 steps (rnn1, rnn2); fc 136: 192 elements, 3 steps (fc1, fc2, fc3); the rest is set B's
DIM_SET_E = dict(DIM_SETS['B'], rnn_dims=160, fc_dims=136)
SETS = dict(DIM_SETS, E=DIM_SET_E)

TEAMG, TEAMG_BATCH = 6, 7
FRAMES = {'A': 1, 'B': 20, 'C': 20, 'D': 1, 'E': 20}
MATRICES = ('I.weight', 'rnn1.weight_ih_l0', 'rnn1.weight_hh_l0', 'rnn2.weight_ih_l0', 'rnn2.weight_hh_l0', 'fc1.weight', 'fc2.weight', 'fc3.weight')
# in units of the layer's smallest e4m3 subnormal s 2^-9, and what round-to-nearest-even must store for them: exact subnormals of both
# signs, two that round, the tie 2.5 -> 2 (even), the tie 0.5 -> 0 (even)
PLANTED = (3.0, -5.0, 1.0, -1.0, 1.3, 2.5, -0.6, 0.5)
PLANTED_STORED = (3.0, -5.0, 1.0, -1.0, 1.0, 2.0, -1.0, 0.0)
ROWS = 5
STATE_SEED = {'E': 11}                                                        # synth seed 7 elsewhere; at set E's dims it gives a model that sits on one class
SEED = 0x5EED5

_STATE, _MODELS, _REF = {}, {}, {}


def _dims(name, mode):
    d = dict(SETS[name])
    if mode == 'MOL' and name == 'D':
        d['bits'] = 9
    return d


def _where(w, c0, i):
    return (7 * i + 3) % w.shape[0], c0 + (11 * i + 2) % (w.shape[1] - c0)


def _plant_and_quantise(sd):
    """(sd with the planted entries, sd8, scales); asserts what the restatement stores for the planted entries and the range of the maxima."""
    sd = {k: np.array(v) for k, v in sd.items()}
    for layer in ref.LAYERS:
        amax = max(float(np.abs(ref._part(k, sd[k])).max()) for k in ref.LAYER_KEYS[layer])
        assert 2.0 ** -20 <= amax <= 2.0 ** 20, (layer, amax)
        s = np.float32(ref.scale_of(amax))
        for k in ref.LAYER_KEYS[layer]:
            c0 = 1 if k == 'I.weight' else 0
            for i, v in enumerate(PLANTED):
                sd[k][_where(sd[k], c0, i)] = np.float32(v) * np.float32(2.0 ** -9) * s
    sd8, scales = ref.quantise(sd)
    for layer, s in zip(ref.LAYERS, scales):
        for k in ref.LAYER_KEYS[layer]:
            c0 = 1 if k == 'I.weight' else 0
            got = np.array([sd8[k][_where(sd8[k], c0, i)] for i in range(len(PLANTED))], np.float32)
            want = np.array(PLANTED_STORED, np.float32) * np.float32(2.0 ** -9) * s
            np.testing.assert_array_equal(got, want, err_msg=f'{k}: planted subnormals')
            assert (np.signbit(got) == np.signbit(np.array(PLANTED, np.float32)))[np.array(PLANTED_STORED) != 0].all()
            assert (got != 0).sum() == len(PLANTED) - 1 and (np.abs(got) < s * np.float32(2.0 ** -6)).all()
    return sd, sd8, scales


def _state(name, mode='RAW'):
    key = (name, mode)
    if key not in _STATE:
        from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
        _STATE[key] = _plant_and_quantise(make_state_dict(STATE_SEED.get(name, 7), mode, 'peaky' if mode == 'RAW' else 'default', **_dims(name, mode)))
    return _STATE[key]


def _new_model(name, mode, sd, weights):
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**_dims(name, mode), mode=mode)
    m.verbose = False
    m.teamg_weights = weights
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    return m


def _models(name, mode='RAW'):
    """(m8 = model of sd with the e4m3 image, m32 = model of sd8 with the fp32 image), once per module."""
    key = (name, mode)
    if key not in _MODELS:
        sd, sd8, _ = _state(name, mode)
        _MODELS[key] = (_new_model(name, mode, sd, 'e4m3'), _new_model(name, mode, sd8, 'f32'))
    return _MODELS[key]


def _mels(name, seed=3, B=ROWS, T=None):
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    return make_mels(seed, B, FRAMES[name] if T is None else T, feat_dims=SETS[name]['feat_dims'])


def _call(m, weights, mels, kernel='teamg', batched=False, target=11000, overlap=550, **kw):
    from tacotronv2_wavernn_chinese_amd import _cabi
    kw.setdefault('noise_mode', 'philox')
    if kw['noise_mode'] == 'philox' and 'seeds' not in kw:
        kw.setdefault('seed', SEED)
    res = m.generate_raw(mels, batched, target, overlap, kernel=kernel, **kw)
    assert m.last_timing['kernel'] == _cabi.KERNEL_IDS[kernel]                 # no silent fallback
    assert m.last_timing['teamg_weights'] == weights == m.native().teamg_weights
    assert m.native().lib.wrnn_teamg_weight_format(m.native()._h) == _cabi.TEAMG_WEIGHT_FORMATS[weights]
    return {k: res[k].cpu().numpy() for k in ('labels', 'samples') + (('logits',) if res['logits'] is not None else ())}


def _same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f'{what}: {k}')


def _ref_f32(name, mode):
    """The fp32 kernel on sd8: the free run with its logits, once per module."""
    key = (name, mode)
    if key not in _REF:
        _REF[key] = _call(_models(name, mode)[1], 'f32', _mels(name), want_logits=True)
    return _REF[key]


def _budgets(name, mode):
    """The default, all streamed, and rnn2 half resident in the e4m3 plan.  Where fc3, fc2 and fc1 alone exceed the LDS no budget reaches
    rnn2: there the third budget is half the default, which leaves one of those three partly resident."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    dims = dict(mode=mode, **_dims(name, mode))
    full = _cabi.teamg_plan_fmt(1, 'e4m3', -1, **dims)
    unit = lambda L: L['rows_per_unit'] * L['k_padded']
    need = sum(max(full['layers'][n]['own_count']) * unit(full['layers'][n]) for n in ('fc3', 'fc2', 'fc1'))
    r2 = full['layers']['rnn2']
    half = need + max(r2['own_count']) // 2 * unit(r2)
    if half <= full['lds_budget_bytes']:
        p = _cabi.teamg_plan_fmt(1, 'e4m3', half, **dims)
        assert 0 < p['layers']['rnn2']['resident_units'] < max(r2['own_count']) and p['layers']['rnn1']['resident_units'] == 0
    else:
        half = full['lds_budget_bytes'] // 2
        p = _cabi.teamg_plan_fmt(1, 'e4m3', half, **dims)
        assert sum(0 < L['resident_units'] < max(L['own_count']) for L in p['layers'].values()) == 1
    return (-1, 0, half)


# ---- 1. the one-row kernel: bit-equal to the fp32 kernel on the dequantised model, under three placements -------------------------

@pytest.mark.parametrize('name,mode', [(n, 'RAW') for n in 'ABCD'] + [('A', 'MOL'), ('B', 'MOL')])
def test_teamg_e4m3_is_bit_equal_to_f32_on_the_dequantised_model(name, mode):
    m8, _ = _models(name, mode)
    want = _ref_f32(name, mode)
    assert want['labels'].shape == (ROWS, FRAMES[name] * SETS[name]['hop_length'])
    nat = m8.native()
    try:
        for budget in _budgets(name, mode):
            nat.debug_teamg_lds_budget(budget)
            _same(_call(m8, 'e4m3', _mels(name), want_logits=True), want, f'set {name} {mode}, e4m3 image, LDS budget {budget}')
    finally:
        nat.debug_teamg_lds_budget(-1)
    assert len({want['labels'][r].tobytes() for r in range(ROWS)}) == ROWS    # the rows are different signals: equality is not vacuous


# ---- 2. several rows per team -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,batch_rows', [(n, r) for n in 'AB' for r in (2, 4, 8)] + [('D', 2), ('D', 4), ('C', 2)])
def test_teamg_batch_e4m3_is_bit_equal_to_f32_and_to_teamg_e4m3(name, batch_rows):
    m8, m32 = _models(name)
    mels = _mels(name)
    got = _call(m8, 'e4m3', mels, 'teamg_batch', batch_rows=batch_rows, want_logits=True)
    assert m8.last_timing['batch_rows'] == batch_rows and m8.last_timing['rows'] == ROWS
    _same(got, _call(m32, 'f32', mels, 'teamg_batch', batch_rows=batch_rows, want_logits=True), f'set {name}, batch_rows {batch_rows}: e4m3 image against fp32 on the dequantised model')
    _same(got, _ref_f32(name, 'RAW'), f'set {name}, batch_rows {batch_rows}: against the one-row kernel')
    _same(got, _call(m8, 'e4m3', mels, want_logits=True), f'set {name}, batch_rows {batch_rows}: every row against e4m3 teamg')


@pytest.mark.parametrize('batch_rows', [2, 4])
def test_teamg_batch_e4m3_mol(batch_rows):
    m8, _ = _models('B', 'MOL')
    got = _call(m8, 'e4m3', _mels('B'), 'teamg_batch', batch_rows=batch_rows, want_logits=True)
    _same(got, _ref_f32('B', 'MOL'), f'set B MOL, batch_rows {batch_rows}')


def test_teamg_batch_e4m3_ragged_and_folded_on_set_a():
    m8, m32 = _models('A')
    lens = [2, 1, 3, 1, 2, 3, 1, 2, 1, 3, 2]                                   # 11 rows of 128 .. 384 steps: more rows than teams
    mels = np.zeros((len(lens), 40, 3), np.float32)
    for i, t in enumerate(lens):
        mels[i, :, :t] = _mels('A', 500 + i, 1, t)[0]
    kw = dict(frames=np.asarray(lens, np.int32))
    want = _call(m32, 'f32', mels, **kw)
    for br in (2, 4):
        got = _call(m8, 'e4m3', mels, 'teamg_batch', batch_rows=br, **kw)
        _same(got, want, f'ragged, batch_rows {br}')
        for i, t in enumerate(lens):
            assert not got['labels'][i, t * 128:].any() and not got['samples'][i, t * 128:].any(), f'row {i}: written past its own length'
    _same(_call(m8, 'e4m3', mels, **kw), want, 'ragged, one row per team')
    # folds of one clip: 4 frames = 512 steps in folds of 100 + 2 * 20
    clip = _mels('A', 13, 1, 4)
    want = _call(m32, 'f32', clip, batched=True, target=100, overlap=20)
    assert want['labels'].shape[0] >= 4
    _same(_call(m8, 'e4m3', clip, 'teamg_batch', batched=True, target=100, overlap=20, batch_rows=2), want, 'folded, batch_rows 2')
    _same(_call(m8, 'e4m3', clip, batched=True, target=100, overlap=20), want, 'folded, one row per team')


# ---- 3. set E: segments of 3 steps, a pair and a single step with no quad -----------------------------------------------------------

def test_set_e_segments_of_three_steps():
    from tacotronv2_wavernn_chinese_amd import _cabi
    p = _cabi.teamg_plan_fmt(1, 'e4m3', -1, mode='RAW', **DIM_SET_E)
    assert {n: L['k_padded'] for n, L in p['layers'].items()} == dict(fc3=192, fc2=192, fc1=192, rnn2=384, rnn1=384, cond=64)
    m8, m32 = _models('E')
    want = _ref_f32('E', 'RAW')
    assert want['labels'].shape == (ROWS, 120) and len({want['labels'][r].tobytes() for r in range(ROWS)}) == ROWS
    nat = m8.native()
    try:
        nat.debug_teamg_lds_budget(_budgets('E', 'RAW')[2])                     # rnn2 half resident: LDS and streamed rows in one call
        _same(_call(m8, 'e4m3', _mels('E'), want_logits=True), want, 'set E, one row per team')
        got = _call(m8, 'e4m3', _mels('E'), 'teamg_batch', batch_rows=2, want_logits=True)
    finally:
        nat.debug_teamg_lds_budget(-1)
    _same(got, want, 'set E, batch_rows 2, against the one-row fp32 kernel')
    _same(got, _call(m32, 'f32', _mels('E'), 'teamg_batch', batch_rows=2, want_logits=True), 'set E, batch_rows 2, against fp32 on the dequantised model')


# ---- 4. / 5. planted values and the scales ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['A', 'B', 'D', 'E'])
def test_weight_scales_equal_the_restatement(name):
    """_state asserts what the restatement stores for the planted subnormals and ties; the bit-equality tests then hold the pack and the
    kernels to it.  Here: the six scales the pack found are the restatement's, exactly; an fp32 image reports ones."""
    m8, m32 = _models(name)
    _, _, scales = _state(name)
    _call(m8, 'e4m3', _mels(name, 3, 1))
    got = m8.native().teamg_weight_scales()
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, scales)
    assert len(set(scales.tolist())) > 1                                        # the layers do have different scales
    _call(m32, 'f32', _mels(name, 3, 1))
    np.testing.assert_array_equal(m32.native().teamg_weight_scales(), np.ones(6, np.float32))


# ---- 6. the oracle on the dequantised model, directly -------------------------------------------------------------------------------

ORACLE_NOISE_SEED = {'A': 8, 'B': 8, 'D': 8}                                   # chosen on the CPU: the oracle's run on sd8 has no margin below NEAR_TIE


@pytest.mark.parametrize('name', ['A', 'B', 'D'])
def test_raw_e4m3_every_step_against_the_oracle_on_the_dequantised_model(name):
    """tests/test_gpu_teamg.py's rule: injected noise, the oracle's own run has no race margin below NEAR_TIE (asserted), so no step is
    excused and label equality is exact, free and teacher-forced; logits within 2e-5 of the largest logit.  Nothing is wider for e4m3."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m8, _ = _models(name)
    _, sd8, _ = _state(name)
    dims = _dims(name, 'RAW')
    om = orc.OracleModel(sd8, mode='RAW', bits=dims['bits'], upsample_factors=dims['upsample_factors'], pad=dims['pad'], fast=True)
    B, L = 3, FRAMES[name] * dims['hop_length']
    mels = _mels(name, 3, B)
    q = np.random.Generator(np.random.PCG64(ORACLE_NOISE_SEED[name])).standard_exponential((L, B, m8.n_classes)).astype(np.float32)
    cm, ca = om.conditioning(mels)
    free = om.loop(cm, ca, orc.NOISE_EXPO, q)
    forced = om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=free['samples'], want_logits=True)
    assert float(free['margin'].min()) >= NEAR_TIE, f'set {name}: the oracle has a near-tie (margin {float(free["margin"].min()):.3e}): pick another seed'
    bound = 2e-5 * max(1.0, float(np.abs(forced['logits']).max()))
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    got = _call(m8, 'e4m3', mels, **kw)['labels'].T
    assert got.shape == (L, B)
    assert all(f is None for f in check_free_run_raw(got, free))
    res = _call(m8, 'e4m3', mels, x_forced=free['samples'], want_logits=True, **kw)
    assert check_teacher_forced_raw(res['labels'].T, forced) == 0
    err = float(np.abs(res['logits'] - forced['logits']).max())
    parity_report(f'teamg e4m3: set {name} RAW B={B}: steps compared {2 * got.size} (free + forced), near-tie divergences 0 (oracle min margin '
                  f'{float(free["margin"].min()):.2e}), max |dlogit| {err:.3e} (bound {bound:.3e})')
    assert err <= bound


@pytest.mark.parametrize('name', ['A', 'B'])
def test_mol_e4m3_against_the_oracle_on_the_dequantised_model(name):
    from tacotronv2_wavernn_chinese_amd import _cabi
    m8, _ = _models(name, 'MOL')
    _, sd8, _ = _state(name, 'MOL')
    dims = _dims(name, 'MOL')
    om = orc.OracleModel(sd8, mode='MOL', bits=dims['bits'], upsample_factors=dims['upsample_factors'], pad=dims['pad'], fast=True)
    B, L = 3, FRAMES[name] * dims['hop_length']
    mels = _mels(name, 3, B)
    rng = np.random.Generator(np.random.PCG64(8))
    n1, n2 = rng.uniform(1e-5, 1 - 1e-5, size=(L, B, 10)).astype(np.float32), rng.uniform(1e-5, 1 - 1e-5, size=(L, B)).astype(np.float32)
    cm, ca = om.conditioning(mels)
    free = om.loop(cm, ca, 0, n1, n2)
    forced = om.loop(cm, ca, 0, n1, n2, x_forced=free['samples'], want_logits=True)
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=n1, noise2=n2)
    res = _call(m8, 'e4m3', mels, **kw)
    check_mol(res['samples'].T, res['labels'].T, free, teacher_forced=False)
    res = _call(m8, 'e4m3', mels, x_forced=free['samples'], **kw)
    check_mol(res['samples'].T, res['labels'].T, forced, teacher_forced=True)


# ---- 7. the switch ------------------------------------------------------------------------------------------------------------------

def test_switching_formats_and_loading_weights_repack_the_image():
    from tacotronv2_wavernn_chinese_amd import _cabi
    sd, sd8, scales = _state('B')
    mels = _mels('B')
    ref8 = _ref_f32('B', 'RAW')                                                # what the e4m3 image of sd must give
    sd16 = dict(sd)
    for k in MATRICES:
        sd16[k] = sd[k].astype(np.float16).astype(np.float32)
    sd16['I.weight'][:, 0] = sd['I.weight'][:, 0]
    ref16 = _call(_new_model('B', 'RAW', sd16, 'f32'), 'f32', mels, want_logits=True)
    m = _new_model('B', 'RAW', sd, 'f32')
    full = _call(m, 'f32', mels, want_logits=True)                             # the unrounded model on the fp32 image
    np.testing.assert_array_equal(m.native().teamg_weight_scales(), np.ones(6, np.float32))
    assert not np.array_equal(full['logits'], ref8['logits']) and not np.array_equal(ref16['logits'], ref8['logits'])
    simple = m.generate_raw(mels, False, 11000, 550, kernel='simple', seed=SEED, want_logits=True)
    m.teamg_weights = 'e4m3'
    assert m.native().lib.wrnn_teamg_weight_format(m.native()._h) == 3
    _same(_call(m, 'e4m3', mels, want_logits=True), ref8, 'f32 -> e4m3')
    np.testing.assert_array_equal(m.native().teamg_weight_scales(), scales)
    m.teamg_weights = 'f16'
    _same(_call(m, 'f16', mels, 'teamg_batch', batch_rows=2, want_logits=True), ref16, 'e4m3 -> f16, batch')
    np.testing.assert_array_equal(m.native().teamg_weight_scales(), np.ones(6, np.float32))
    m.teamg_weights = 'e4m3'
    _same(_call(m, 'e4m3', mels, 'teamg_batch', batch_rows=2, want_logits=True), ref8, 'f16 -> e4m3, batch')
    _same(_call(m, 'e4m3', mels, want_logits=True), ref8, 'e4m3 again')
    again = m.generate_raw(mels, False, 11000, 550, kernel='simple', seed=SEED, want_logits=True)
    assert m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE and m.last_timing['teamg_weights'] == 'e4m3'
    for k in ('labels', 'samples', 'logits'):                                  # no other kernel reads the setting
        np.testing.assert_array_equal(again[k].cpu().numpy(), simple[k].cpu().numpy(), err_msg=f'simple: {k}')
    # load_state_dict under e4m3: the setting stays, the image and the scales follow the new weights
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    other = {k: np.array(v) for k, v in make_state_dict(11, 'RAW', 'peaky', **_dims('B', 'RAW')).items()}
    other['fc2.weight'] *= np.float32(4.0)
    other8, other_scales = ref.quantise(other)
    assert not np.array_equal(other_scales, scales)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in other.items()})
    assert m.teamg_weights == 'e4m3'
    got = _call(m, 'e4m3', mels, want_logits=True)
    assert not np.array_equal(got['logits'], ref8['logits'])
    _same(got, _call(_new_model('B', 'RAW', other8, 'f32'), 'f32', mels, want_logits=True), 'after load_state_dict')
    np.testing.assert_array_equal(m.native().teamg_weight_scales(), other_scales)
    with pytest.raises(ValueError):
        m.teamg_weights = 'bf16'
    with pytest.raises(ValueError):
        m.native().set_teamg_weights('int8')
    assert m.native().lib.wrnn_teamg_set_weight_format(m.native()._h, 2) == _cabi.ERR_INVALID
    assert m.native().teamg_weights == 'e4m3'


# ---- 8. a weight that is not finite; a large one --------------------------------------------------------------------------------------

def test_a_nan_weight_is_refused_by_name_f32_still_runs_and_a_large_weight_is_accepted():
    from tacotronv2_wavernn_chinese_amd import _cabi
    sd, _, _ = _state('B')
    bad = {k: np.array(v) for k, v in sd.items()}
    bad['fc1.weight'][5, 7] = np.nan
    m = _new_model('B', 'RAW', bad, 'e4m3')
    mels = _mels('B', 3, 2)
    for kernel, kw in (('teamg', {}), ('teamg_batch', dict(batch_rows=2))):
        with pytest.raises(_cabi.WrnnError, match='fc1') as e:
            m.generate_raw(mels, False, 11000, 550, kernel=kernel, seed=SEED, **kw)
        assert e.value.code == _cabi.ERR_UNSUPPORTED
        np.testing.assert_array_equal(m.native().teamg_weight_scales(), np.ones(6, np.float32))
    m.teamg_weights = 'f32'
    assert _call(m, 'f32', mels)['labels'].shape == (2, 120)                   # the fp32 image runs whatever the weights hold
    # 1e5 has no fp16; here the layer's scale absorbs it: 1e5 / 256 = 390.6 <= 448
    big = {k: np.array(v) for k, v in sd.items()}
    big['fc1.weight'][5, 7] = 1e5
    big8, big_scales = ref.quantise(big)
    assert big_scales[ref.LAYERS.index('fc1')] == 256.0
    m = _new_model('B', 'RAW', big, 'e4m3')
    got = _call(m, 'e4m3', mels, want_logits=True)
    assert np.isfinite(got['samples']).all()
    np.testing.assert_array_equal(m.native().teamg_weight_scales(), big_scales)
    _same(got, _call(_new_model('B', 'RAW', big8, 'f32'), 'f32', mels, want_logits=True), 'a weight of 1e5')
