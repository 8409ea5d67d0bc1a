"""The half-precision weight image of WRNN_KERNEL_TEAMG / WRNN_KERNEL_TEAMG_BATCH (`teamg_weights='f16'`).

An fp16 weight converts to fp32 exactly and the f16 kernels multiply and add in the fp32 kernels' order, so a model `sd` run with the f16
image must be BIT-equal -- labels, samples, logits -- to the model `sd16` run with the fp32 image, where `sd16` is `sd` with the matrices of
the image rounded to fp16 beforehand (`w.half().float()`).  That is most of this file; section 3 compares with the oracle on `sd16` directly
under the rules of tests/parity_util.py, with nothing loosened.

The matrices of the image are the four GRU matrices, fc1, fc2, fc3 and W_I[:, 1:]: column 0 of `I.weight` (the fed-back sample's) is a vector
the kernels keep in fp32, so `sd16` leaves that column as it is.  Before rounding, a handful of entries of every matrix are overwritten with
values that are subnormal in fp16, both signs: a conversion that flushed them, in the pack or in the kernel, would show.

Dim sets A to D of tests/teamg_cases.py; B and C keep hop 6 (120 steps), A runs one frame of 128 steps, D one frame of its hop 275 -- the
shortest call its dims allow.  Philox noise unless said otherwise.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.parity_util import NEAR_TIE, check_free_run_raw, check_mol, check_teacher_forced_raw, parity_report
from tests.teamg_cases import DIM_SETS

pytestmark = pytest.mark.gpu

TEAMG, TEAMG_BATCH = 6, 7
FRAMES = {'A': 1, 'B': 20, 'C': 20, 'D': 1}
MATRICES = ('I.weight', 'rnn1.weight_ih_l0', 'rnn1.weight_hh_l0', 'rnn2.weight_ih_l0', 'rnn2.weight_hh_l0', 'fc1.weight', 'fc2.weight', 'fc3.weight')
SUBNORMALS = (3e-6, -3e-6, 6e-8, -6e-8, 2.5e-5, -4e-7)       # all below fp16's smallest normal 6.1e-5, all at or above half its smallest subnormal
ROWS = 5
SEED = 0x5EED5

_STATE, _MODELS, _REF = {}, {}, {}


def _dims(name, mode):
    d = dict(DIM_SETS[name])
    if mode == 'MOL' and name == 'D':
        d['bits'] = 9
    return d


def _round_f16(w):
    return torch.from_numpy(np.ascontiguousarray(w)).half().float().numpy()


def _state(name, mode='RAW'):
    """(sd with fp16-subnormal entries planted in every matrix of the image, sd16 = sd with exactly those matrices rounded to fp16)."""
    key = (name, mode)
    if key not in _STATE:
        from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
        sd = {k: np.array(v) for k, v in make_state_dict(7, mode, 'peaky' if mode == 'RAW' else 'default', **_dims(name, mode)).items()}
        sd16 = dict(sd)
        for k in MATRICES:
            w = sd[k]
            c0 = 1 if k == 'I.weight' else 0
            for i, v in enumerate(SUBNORMALS):
                w[(7 * i + 3) % w.shape[0], c0 + (11 * i + 2) % (w.shape[1] - c0)] = v
            r = _round_f16(w)
            if c0:
                r[:, 0] = w[:, 0]
            planted = np.array([r[(7 * i + 3) % w.shape[0], c0 + (11 * i + 2) % (w.shape[1] - c0)] for i in range(len(SUBNORMALS))])
            assert (planted != 0).all() and (np.abs(planted) < 6.1e-5).all() and (np.sign(planted) == np.sign(SUBNORMALS)).all()
            sd16[k] = r
        _STATE[key] = (sd, sd16)
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
    """(model of sd with the f16 image, model of sd16 with the fp32 image), once per module."""
    key = (name, mode)
    if key not in _MODELS:
        sd, sd16 = _state(name, mode)
        _MODELS[key] = (_new_model(name, mode, sd, 'f16'), _new_model(name, mode, sd16, 'f32'))
    return _MODELS[key]


def _mels(name, seed=3, B=ROWS, T=None):
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    return make_mels(seed, B, FRAMES[name] if T is None else T, feat_dims=DIM_SETS[name]['feat_dims'])


def _call(m, weights, mels, kernel='teamg', batched=False, target=11000, overlap=550, **kw):
    from tacotronv2_wavernn_chinese_amd import _cabi
    kw.setdefault('noise_mode', 'philox')
    if kw['noise_mode'] == 'philox' and 'seeds' not in kw:
        kw.setdefault('seed', SEED)
    res = m.generate_raw(mels, batched, target, overlap, kernel=kernel, **kw)
    assert m.last_timing['kernel'] == _cabi.KERNEL_IDS[kernel]                 # no silent fallback
    assert m.last_timing['teamg_weights'] == weights == m.native().teamg_weights
    assert m.native().lib.wrnn_teamg_weight_format(m.native()._h) == _cabi.WEIGHT_FORMATS[weights]
    return {k: res[k].cpu().numpy() for k in ('labels', 'samples') + (('logits',) if res['logits'] is not None else ())}


def _same(got, ref, what):
    assert set(got) == set(ref)
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f'{what}: {k}')


def _ref_f32(name, mode):
    """The fp32 kernel on sd16: the free run with its logits, once per module."""
    key = (name, mode)
    if key not in _REF:
        _REF[key] = _call(_models(name, mode)[1], 'f32', _mels(name), want_logits=True)
    return _REF[key]


def _budgets(name, mode):
    """The default, all streamed, and rnn2 half resident in the F16 plan.  Where fc3, fc2 and fc1 alone exceed the LDS (set C) no budget
    reaches rnn2: there the third budget is half the default, which leaves one of those three partly resident."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    dims = dict(mode=mode, **_dims(name, mode))
    full = _cabi.teamg_plan_fmt(1, 'f16', -1, **dims)
    unit = lambda L: 2 * L['rows_per_unit'] * L['k_padded']
    need = sum(max(full['layers'][n]['own_count']) * unit(full['layers'][n]) for n in ('fc3', 'fc2', 'fc1'))
    r2 = full['layers']['rnn2']
    half = need + max(r2['own_count']) // 2 * unit(r2)
    if half <= full['lds_budget_bytes']:
        p = _cabi.teamg_plan_fmt(1, 'f16', half, **dims)
        assert 0 < p['layers']['rnn2']['resident_units'] < max(r2['own_count']) and p['layers']['rnn1']['resident_units'] == 0
    else:
        half = full['lds_budget_bytes'] // 2
        p = _cabi.teamg_plan_fmt(1, 'f16', half, **dims)
        assert sum(0 < L['resident_units'] < max(L['own_count']) for L in p['layers'].values()) == 1
    return (-1, 0, half)


# ---- 1. the one-row kernel: bit-equal to the fp32 kernel on the rounded model, under three placements --------------------------------

@pytest.mark.parametrize('name,mode', [(n, 'RAW') for n in 'ABCD'] + [('A', 'MOL'), ('B', 'MOL')])
def test_teamg_f16_is_bit_equal_to_f32_on_the_rounded_model(name, mode):
    m16, _ = _models(name, mode)
    ref = _ref_f32(name, mode)
    assert ref['labels'].shape == (ROWS, FRAMES[name] * DIM_SETS[name]['hop_length'])
    nat = m16.native()
    try:
        for budget in _budgets(name, mode):
            nat.debug_teamg_lds_budget(budget)
            _same(_call(m16, 'f16', _mels(name), want_logits=True), ref, f'set {name} {mode}, f16 image, LDS budget {budget}')
    finally:
        nat.debug_teamg_lds_budget(-1)
    assert len({ref['labels'][r].tobytes() for r in range(ROWS)}) == ROWS     # the rows are different signals: equality is not vacuous


# ---- 2. several rows per team ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,batch_rows', [(n, r) for n in 'AB' for r in (2, 4, 8)] + [('D', 2), ('D', 4), ('C', 2)])
def test_teamg_batch_f16_is_bit_equal_to_f32_and_to_teamg_f16(name, batch_rows):
    m16, m32 = _models(name)
    mels = _mels(name)
    got = _call(m16, 'f16', mels, 'teamg_batch', batch_rows=batch_rows, want_logits=True)
    assert m16.last_timing['batch_rows'] == batch_rows and m16.last_timing['rows'] == ROWS
    _same(got, _call(m32, 'f32', mels, 'teamg_batch', batch_rows=batch_rows, want_logits=True), f'set {name}, batch_rows {batch_rows}: f16 image against fp32 on the rounded model')
    _same(got, _ref_f32(name, 'RAW'), f'set {name}, batch_rows {batch_rows}: against the one-row kernel')
    _same(got, _call(m16, 'f16', mels, want_logits=True), f'set {name}, batch_rows {batch_rows}: every row against f16 teamg')


@pytest.mark.parametrize('batch_rows', [2, 4])
def test_teamg_batch_f16_mol(batch_rows):
    m16, m32 = _models('B', 'MOL')
    got = _call(m16, 'f16', _mels('B'), 'teamg_batch', batch_rows=batch_rows, want_logits=True)
    _same(got, _ref_f32('B', 'MOL'), f'set B MOL, batch_rows {batch_rows}')


def test_teamg_batch_f16_ragged_and_folded_on_set_a():
    m16, m32 = _models('A')
    lens = [2, 1, 3, 1, 2, 3, 1, 2, 1, 3, 2]                                   # 11 rows of 128 .. 384 steps: more rows than teams
    mels = np.zeros((len(lens), 40, 3), np.float32)
    for i, t in enumerate(lens):
        mels[i, :, :t] = _mels('A', 500 + i, 1, t)[0]
    kw = dict(frames=np.asarray(lens, np.int32))
    ref = _call(m32, 'f32', mels, **kw)
    for br in (2, 4):
        got = _call(m16, 'f16', mels, 'teamg_batch', batch_rows=br, **kw)
        _same(got, ref, f'ragged, batch_rows {br}')
        for i, t in enumerate(lens):
            assert not got['labels'][i, t * 128:].any() and not got['samples'][i, t * 128:].any(), f'row {i}: written past its own length'
    _same(_call(m16, 'f16', mels, **kw), ref, 'ragged, one row per team')
    # folds of one clip: 4 frames = 512 steps in folds of 100 + 2 * 20
    clip = _mels('A', 13, 1, 4)
    ref = _call(m32, 'f32', clip, batched=True, target=100, overlap=20)
    assert ref['labels'].shape[0] >= 4
    _same(_call(m16, 'f16', clip, 'teamg_batch', batched=True, target=100, overlap=20, batch_rows=2), ref, 'folded, batch_rows 2')
    _same(_call(m16, 'f16', clip, batched=True, target=100, overlap=20), ref, 'folded, one row per team')


# ---- 3. the oracle on the rounded model, directly ----------------------------------------------------------------------------------------

ORACLE_NOISE_SEED = {'A': 8, 'B': 8, 'D': 8}


@pytest.mark.parametrize('name', ['A', 'B', 'D'])
def test_raw_f16_every_step_against_the_oracle_on_the_rounded_model(name):
    """tests/test_gpu_teamg.py's rule: injected noise, the oracle's own run has no race margin below NEAR_TIE (asserted), so no step is
    excused and label equality is exact, free and teacher-forced; logits within 2e-5 of the largest logit.  Nothing is wider for f16."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m16, _ = _models(name)
    _, sd16 = _state(name)
    dims = _dims(name, 'RAW')
    om = orc.OracleModel(sd16, mode='RAW', bits=dims['bits'], upsample_factors=dims['upsample_factors'], pad=dims['pad'], fast=True)
    B, L = 3, FRAMES[name] * dims['hop_length']
    mels = _mels(name, 3, B)
    q = np.random.Generator(np.random.PCG64(ORACLE_NOISE_SEED[name])).standard_exponential((L, B, m16.n_classes)).astype(np.float32)
    cm, ca = om.conditioning(mels)
    free = om.loop(cm, ca, orc.NOISE_EXPO, q)
    forced = om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=free['samples'], want_logits=True)
    assert float(free['margin'].min()) >= NEAR_TIE, f'set {name}: the oracle has a near-tie (margin {float(free["margin"].min()):.3e}): pick another seed'
    bound = 2e-5 * max(1.0, float(np.abs(forced['logits']).max()))
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    got = _call(m16, 'f16', mels, **kw)['labels'].T
    assert got.shape == (L, B)
    assert all(f is None for f in check_free_run_raw(got, free))
    res = _call(m16, 'f16', mels, x_forced=free['samples'], want_logits=True, **kw)
    assert check_teacher_forced_raw(res['labels'].T, forced) == 0
    err = float(np.abs(res['logits'] - forced['logits']).max())
    parity_report(f'teamg f16: set {name} RAW B={B}: steps compared {2 * got.size} (free + forced), near-tie divergences 0 (oracle min margin '
                  f'{float(free["margin"].min()):.2e}), max |dlogit| {err:.3e} (bound {bound:.3e})')
    assert err <= bound


@pytest.mark.parametrize('name', ['A', 'B'])
def test_mol_f16_against_the_oracle_on_the_rounded_model(name):
    from tacotronv2_wavernn_chinese_amd import _cabi
    m16, _ = _models(name, 'MOL')
    _, sd16 = _state(name, 'MOL')
    dims = _dims(name, 'MOL')
    om = orc.OracleModel(sd16, mode='MOL', bits=dims['bits'], upsample_factors=dims['upsample_factors'], pad=dims['pad'], fast=True)
    B, L = 3, FRAMES[name] * dims['hop_length']
    mels = _mels(name, 3, B)
    rng = np.random.Generator(np.random.PCG64(8))
    n1, n2 = rng.uniform(1e-5, 1 - 1e-5, size=(L, B, 10)).astype(np.float32), rng.uniform(1e-5, 1 - 1e-5, size=(L, B)).astype(np.float32)
    cm, ca = om.conditioning(mels)
    free = om.loop(cm, ca, 0, n1, n2)
    forced = om.loop(cm, ca, 0, n1, n2, x_forced=free['samples'], want_logits=True)
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=n1, noise2=n2)
    res = _call(m16, 'f16', mels, **kw)
    check_mol(res['samples'].T, res['labels'].T, free, teacher_forced=False)
    res = _call(m16, 'f16', mels, x_forced=free['samples'], **kw)
    check_mol(res['samples'].T, res['labels'].T, forced, teacher_forced=True)


# ---- 4. the switch ---------------------------------------------------------------------------------------------------------------------------

def test_switching_formats_and_loading_weights_repack_the_image():
    from tacotronv2_wavernn_chinese_amd import _cabi
    sd, sd16 = _state('B')
    mels = _mels('B')
    ref16 = _ref_f32('B', 'RAW')                                              # what the f16 image of sd must give
    m = _new_model('B', 'RAW', sd, 'f16')
    _same(_call(m, 'f16', mels, want_logits=True), ref16, 'f16')
    simple = m.generate_raw(mels, False, 11000, 550, kernel='simple', seed=SEED, want_logits=True)
    assert m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE and m.last_timing['teamg_weights'] == 'f16'
    m.teamg_weights = 'f32'
    assert m.native().lib.wrnn_teamg_weight_format(m.native()._h) == 0
    full = _call(m, 'f32', mels, want_logits=True)                             # the unrounded model on the fp32 image
    assert not np.array_equal(full['logits'], ref16['logits'])                 # rounding the weights does change the logits
    _same(_call(m, 'f32', mels, 'teamg_batch', batch_rows=2, want_logits=True), full, 'f32, batch')
    again = m.generate_raw(mels, False, 11000, 550, kernel='simple', seed=SEED, want_logits=True)
    for k in ('labels', 'samples', 'logits'):                                  # no other kernel reads the setting
        np.testing.assert_array_equal(again[k].cpu().numpy(), simple[k].cpu().numpy(), err_msg=f'simple: {k}')
    m.teamg_weights = 'f16'
    _same(_call(m, 'f16', mels, 'teamg_batch', batch_rows=2, want_logits=True), ref16, 'f16 again, batch')
    _same(_call(m, 'f16', mels, want_logits=True), ref16, 'f16 again')
    # load_state_dict under f16: the setting stays, the image follows the new weights
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    other = {k: np.array(v) for k, v in make_state_dict(11, 'RAW', 'peaky', **_dims('B', 'RAW')).items()}
    other16 = dict(other)
    for k in MATRICES:
        other16[k] = _round_f16(other[k])
    other16['I.weight'][:, 0] = other['I.weight'][:, 0]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in other.items()})
    assert m.teamg_weights == 'f16'
    got = _call(m, 'f16', mels, want_logits=True)
    assert not np.array_equal(got['logits'], ref16['logits'])
    _same(got, _call(_new_model('B', 'RAW', other16, 'f32'), 'f32', mels, want_logits=True), 'after load_state_dict')
    with pytest.raises(ValueError):
        m.teamg_weights = 'bf16'
    with pytest.raises(ValueError):
        m.native().set_teamg_weights('int8')
    assert m.native().lib.wrnn_teamg_set_weight_format(m.native()._h, 2) == _cabi.ERR_INVALID
    assert m.native().teamg_weights == 'f16'


# ---- 5. a weight fp16 cannot hold ----------------------------------------------------------------------------------------------------------

def test_a_weight_out_of_fp16_range_is_refused_by_name_and_f32_still_runs():
    from tacotronv2_wavernn_chinese_amd import _cabi
    sd, _ = _state('B')
    big = {k: np.array(v) for k, v in sd.items()}
    big['fc1.weight'][5, 7] = 1e5
    m = _new_model('B', 'RAW', big, 'f16')
    mels = _mels('B', 3, 2)
    for kernel, kw in (('teamg', {}), ('teamg_batch', dict(batch_rows=2))):
        with pytest.raises(_cabi.WrnnError, match='fc1') as e:
            m.generate_raw(mels, False, 11000, 550, kernel=kernel, seed=SEED, **kw)
        assert e.value.code == _cabi.ERR_UNSUPPORTED
    m.teamg_weights = 'f32'
    res = _call(m, 'f32', mels)
    assert res['labels'].shape == (2, 120) and np.isfinite(res['samples']).all()
    # 65519 still rounds to the largest finite fp16
    big['fc1.weight'][5, 7] = 65519.0
    m = _new_model('B', 'RAW', big, 'f16')
    assert np.isfinite(_call(m, 'f16', mels)['samples']).all()
