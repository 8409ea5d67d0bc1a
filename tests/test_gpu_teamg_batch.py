"""WRNN_KERNEL_TEAMG_BATCH: several rows per XCD team in lock-step on the kernel for any model dims.

Per (row, output) its arithmetic is WRNN_KERNEL_TEAMG's operand for operand, so every row's labels, samples and logits must be BIT-equal
to `kernel='teamg'` on the same inputs, whatever batch the row lands in -- that is most of this file.  So that it does not lean on the
other kernel alone, section 2 compares with the oracle directly, under the rules and with the models, mels, noise seeds and frame counts
of tests/test_gpu_teamg.py (its caches are shared: the oracle runs once per dim set for both files).  `last_timing['kernel'] == 7` and
`last_timing['batch_rows']` are asserted after every call of the new kernel.
"""
import numpy as np
import pytest

from tests.parity_util import check_free_run_raw, check_mol, check_teacher_forced_raw, parity_report
from tests.test_gpu_teamg import _case, _mels, _model, _no_near_tie, _noise_kw

pytestmark = pytest.mark.gpu

TEAMG, TEAMG_BATCH = 6, 7
_REF = {}


def _gen(m, *args, batch_rows, expect=None, **kw):
    """A call on the new kernel; `expect`: the rows per team batch it must report (default: the batch_rows asked for)."""
    res = m.generate_raw(*args, kernel='teamg_batch', batch_rows=batch_rows, **kw)
    assert m.last_timing['kernel'] == TEAMG_BATCH                               # no silent fallback, no other kernel
    assert m.last_timing['batch_rows'] == (batch_rows if expect is None else expect)
    return res


def _ref(m, *args, **kw):
    res = m.generate_raw(*args, kernel='teamg', **kw)
    assert m.last_timing['kernel'] == TEAMG and m.last_timing['batch_rows'] == 1
    return res


def _same(got, ref, what, logits=False):
    for k in ('labels', 'samples') + (('logits',) if logits else ()):
        np.testing.assert_array_equal(got[k].cpu().numpy(), ref[k].cpu().numpy(), err_msg=f'{what}: {k}')


def _x0(rows):
    return np.asarray([0.5, -0.25, 1.0, -1.0][:rows], np.float32)


def _teamg_runs(name, mode, B=3):
    """TEAMG's free run and teacher-forced run (x_init, logits) of one case, once per module."""
    key = (name, mode, B)
    if key not in _REF:
        m, _, _ = _model(name, mode)
        c = _case(name, mode, B)
        free = _ref(m, c['mels'], False, 11000, 550, **_noise_kw(c))
        forced = _ref(m, c['mels'], False, 11000, 550, x_forced=c['free']['samples'], x_init=_x0(B), want_logits=True, **_noise_kw(c))
        _REF[key] = (free, forced)
    return _REF[key]


def _both_runs(name, mode, batch_rows, B=3, expect=None):
    m, _, _ = _model(name, mode)
    c = _case(name, mode, B)
    free = _gen(m, c['mels'], False, 11000, 550, batch_rows=batch_rows, expect=expect, **_noise_kw(c))
    forced = _gen(m, c['mels'], False, 11000, 550, batch_rows=batch_rows, expect=expect, x_forced=c['free']['samples'], x_init=_x0(B), want_logits=True,
                  **_noise_kw(c))
    assert m.last_timing['rows'] == B and m.last_timing['steps'] == c['L']
    return free, forced


# ---- 1. bit-equality with TEAMG --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,batch_rows', [(n, r) for n in 'ABD' for r in (2, 3, 4)] + [('C', 2)])
def test_raw_is_bit_equal_to_teamg(name, batch_rows):
    rfree, rforced = _teamg_runs(name, 'RAW')
    free, forced = _both_runs(name, 'RAW', batch_rows)
    _same(free, rfree, f'set {name} RAW free, batch_rows {batch_rows}')
    _same(forced, rforced, f'set {name} RAW teacher-forced with x_init, batch_rows {batch_rows}', logits=True)


@pytest.mark.parametrize('name,batch_rows', [(n, r) for n in 'AB' for r in (2, 4)])
def test_mol_is_bit_equal_to_teamg(name, batch_rows):
    rfree, rforced = _teamg_runs(name, 'MOL')
    free, forced = _both_runs(name, 'MOL', batch_rows)
    _same(free, rfree, f'set {name} MOL free, batch_rows {batch_rows}')
    _same(forced, rforced, f'set {name} MOL teacher-forced with x_init, batch_rows {batch_rows}', logits=True)


def test_one_row_with_three_idle_slots_and_eight_rows_per_team():
    rfree, rforced = _teamg_runs('B', 'RAW', 1)
    free, forced = _both_runs('B', 'RAW', 4, B=1)
    _same(free, rfree, 'set B, one row in a batch of 4')
    _same(forced, rforced, 'set B, one row in a batch of 4, teacher-forced', logits=True)
    rfree, rforced = _teamg_runs('B', 'RAW')
    free, forced = _both_runs('B', 'RAW', 8)
    _same(free, rfree, 'set B, batch_rows 8')
    _same(forced, rforced, 'set B, batch_rows 8, teacher-forced', logits=True)


# ---- 2. the oracle, directly ----------------------------------------------------------------------------------------------------------------

ORACLE_ROWS = {'A': 4, 'B': 2, 'C': 2, 'D': 4}


@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D'])
def test_raw_every_step_against_the_oracle(name):
    m, _, _ = _model(name)
    c = _case(name, 'RAW')
    free, forced = c['free'], c['forced']
    _no_near_tie(free, f'set {name}')                                           # asserted on the oracle's output: nothing is excused
    np.testing.assert_array_equal(forced['labels'], free['labels'])
    bound = 2e-5 * max(1.0, float(np.abs(forced['logits']).max()))
    br = ORACLE_ROWS[name]
    res = _gen(m, c['mels'], False, 11000, 550, batch_rows=br, **_noise_kw(c))
    got = res['labels'].cpu().numpy().T
    assert got.shape == (c['L'], 3)
    assert all(f is None for f in check_free_run_raw(got, free))
    smp = res['samples'].cpu().numpy().T
    np.testing.assert_array_equal(smp, 2.0 * got.astype(np.float32) / np.float32(m.n_classes - 1.0) - np.float32(1.0))
    res = _gen(m, c['mels'], False, 11000, 550, batch_rows=br, x_forced=free['samples'], want_logits=True, **_noise_kw(c))
    gotf = res['labels'].cpu().numpy().T
    assert check_teacher_forced_raw(gotf, forced) == 0
    err = float(np.abs(res['logits'].cpu().numpy() - forced['logits']).max())
    parity_report(f'teamg_batch: set {name} RAW B=3 batch_rows={br}: steps compared {got.size + gotf.size} (free + forced), near-tie divergences 0 '
                  f'(oracle min margin {float(free["margin"].min()):.2e}), max |dlogit| {err:.3e} (bound {bound:.3e})')
    assert err <= bound


@pytest.mark.parametrize('name', ['A', 'B'])
def test_mol_against_the_oracle(name):
    m, _, _ = _model(name, 'MOL')
    c = _case(name, 'MOL')
    res = _gen(m, c['mels'], False, 11000, 550, batch_rows=4, **_noise_kw(c))
    check_mol(res['samples'].cpu().numpy().T, res['labels'].cpu().numpy().T, c['free'], teacher_forced=False)
    res = _gen(m, c['mels'], False, 11000, 550, batch_rows=4, x_forced=c['free']['samples'], **_noise_kw(c))
    check_mol(res['samples'].cpu().numpy().T, res['labels'].cpu().numpy().T, c['forced'], teacher_forced=True)


# ---- 3. ragged: a 6-step row shares a batch with a 240-step row -------------------------------------------------------------------------------

def test_eleven_ragged_rows_are_bit_equal_and_zero_past_their_length():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _model('B')
    hop, F = 6, 13
    lens = [40, 1, 33, 2, 38, 22, 31, 40, 25, 36, 29]
    B, Tm = len(lens), max(lens)
    teams = m.native().team_info()[1]
    mels = np.zeros((B, F, Tm), np.float32)
    for i, t in enumerate(lens):
        mels[i, :, :t] = _mels('B', 500 + i, 1, t)[0]
    q = np.random.Generator(np.random.PCG64(15)).standard_exponential((Tm * hop, B, m.n_classes), dtype=np.float32)
    kw = dict(frames=np.asarray(lens, np.int32), noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    ref = _ref(m, mels, False, 11000, 550, **kw)
    rl, rs = ref['labels'].cpu().numpy(), ref['samples'].cpu().numpy()
    for br in (0, 3, 8):
        res = _gen(m, mels, False, 11000, 550, batch_rows=br, expect=-(-B // teams) if br == 0 else br, **kw)
        assert m.last_timing['rows'] == B
        lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
        np.testing.assert_array_equal(lab, rl, err_msg=f'batch_rows {br}')
        np.testing.assert_array_equal(smp, rs, err_msg=f'batch_rows {br}')
        for i, t in enumerate(lens):
            assert not lab[i, t * hop:].any() and not smp[i, t * hop:].any(), f'batch_rows {br}, row {i}: written past its own length'
            assert smp[i, :t * hop].any()


# ---- 4. folds ----------------------------------------------------------------------------------------------------------------------------------

def test_folds_of_one_utterance_and_of_three():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _model('B')
    teams = m.native().team_info()[1]
    T, target, overlap = 60, 47, 9
    mels = _mels('B', 13, 1, T)
    rows, steps = m.native().plan(1, T, True, target, overlap)
    q = np.random.Generator(np.random.PCG64(14)).standard_exponential((steps, rows, m.n_classes), dtype=np.float32)
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    ref = _ref(m, mels, True, target, overlap, **kw)
    for br in (2, 4):
        res = _gen(m, mels, True, target, overlap, batch_rows=br, **kw)
        assert m.last_timing['rows'] == rows and m.last_timing['steps'] == steps
        _same(res, ref, f'folds {target}/{overlap} of one clip, batch_rows {br}')
    if rows <= teams:                                                           # left to the library, one row per team is TEAMG itself
        res = m.generate_raw(mels, True, target, overlap, kernel='teamg_batch', **kw)
        assert m.last_timing['kernel'] == TEAMG and m.last_timing['batch_rows'] == 1
        _same(res, ref, 'folds of one clip, one per team')

    lens, seeds = [60, 31, 44], [0xA1, 0xB2B2B2B2B2, 0xC3]
    batch = np.zeros((3, 13, 60), np.float32)
    for i, t in enumerate(lens):
        batch[i, :, :t] = _mels('B', 700 + i, 1, t)[0]
    want = m.generate_raw_folded(batch, lens, target, overlap, seeds=seeds, kernel='teamg')
    assert m.last_timing['kernel'] == TEAMG
    many = m.generate_raw_folded(batch, lens, target, overlap, seeds=seeds, kernel='teamg_batch', batch_rows=3)
    assert m.last_timing['kernel'] == TEAMG_BATCH and m.last_timing['batch_rows'] == 3 and m.last_timing['rows'] == many['fold0'][-1]
    _same(many, want, 'three clips folded in one call')
    lm, sm, fold0 = many['labels'].cpu().numpy(), many['samples'].cpu().numpy(), many['fold0']
    for i, t in enumerate(lens):
        solo = _gen(m, batch[i:i + 1, :, :t], True, target, overlap, batch_rows=2, seed=seeds[i])
        np.testing.assert_array_equal(lm[fold0[i]:fold0[i + 1]], solo['labels'].cpu().numpy(), err_msg=f'clip {i}')
        np.testing.assert_array_equal(sm[fold0[i]:fold0[i + 1]], solo['samples'].cpu().numpy(), err_msg=f'clip {i}')


# ---- 5. device Philox noise and ARGMAX ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['A', 'B'])
def test_philox_and_argmax_are_bit_equal_to_teamg(name):
    from tacotronv2_wavernn_chinese_amd import _cabi
    T = {'A': 5, 'B': 50}[name]
    seeds = [0x1234567, 0xFEDCBA9800000000 + 0x1234567, 0x77]
    for mode in ('RAW', 'MOL'):
        m, _, _ = _model(name, mode)
        mels = _mels(name, 41, 3, T)
        for kw in (dict(noise_mode='philox', seed=0x5EED), dict(noise_mode='philox', seeds=seeds)):
            ref = _ref(m, mels, False, 11000, 550, **kw)
            for br in (2, 4):
                _same(_gen(m, mels, False, 11000, 550, batch_rows=br, **kw), ref, f'set {name} {mode} {sorted(kw)} batch_rows {br}')
            lab = ref['labels' if mode == 'RAW' else 'samples'].cpu().numpy()
            assert len({lab[b].tobytes() for b in range(3)}) == 3              # the rows drew different noise
    m, _, _ = _model(name)
    ref = _ref(m, mels, False, 11000, 550, noise_mode=_cabi.NOISE_ARGMAX)
    _same(_gen(m, mels, False, 11000, 550, batch_rows=2, noise_mode=_cabi.NOISE_ARGMAX), ref, f'set {name} ARGMAX')


# ---- 6. placements: all streamed, rnn2 half resident, the default ------------------------------------------------------------------------------

def test_set_b_is_bit_equal_under_every_weight_placement():
    m, _, _ = _model('B')
    c = _case('B', 'RAW')
    nat = m.native()
    full = nat.teamg_batch_plan(4)
    assert all(L['resident_units'] == max(L['own_count']) for L in full['layers'].values())      # set B at 4 rows: everything fits
    r2 = full['layers']['rnn2']
    half = sum(full['layers'][n]['lds_bytes'] for n in ('fc3', 'fc2', 'fc1')) + r2['lds_bytes'] // 2
    p = nat.teamg_batch_plan(4, half)
    assert 0 < p['layers']['rnn2']['resident_units'] < max(r2['own_count']) and p['layers']['rnn1']['resident_units'] == 0
    rfree, _ = _teamg_runs('B', 'RAW')
    try:
        for budget in (0, half, -1):
            nat.debug_teamg_lds_budget(budget)
            _same(_gen(m, c['mels'], False, 11000, 550, batch_rows=4, **_noise_kw(c)), rfree, f'set B, LDS budget {budget}')
    finally:
        nat.debug_teamg_lds_budget(-1)


# ---- 7. what stays refused ---------------------------------------------------------------------------------------------------------------------

def test_refusals():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _model('C')
    mels = _mels('C', 21, 1, 2)
    with pytest.raises(_cabi.WrnnError, match='exceed') as e:                    # the plan's reason
        m.generate_raw(mels, False, 11000, 550, kernel='teamg_batch', batch_rows=8, noise_mode=_cabi.NOISE_ARGMAX)
    assert e.value.code == _cabi.ERR_UNSUPPORTED
    m, _, _ = _model('A')
    mels = _mels('A', 21, 1, 2)
    m.native().debug_force_no_teams(True)
    try:
        with pytest.raises(_cabi.WrnnError, match='force_no_teams'):
            m.generate_raw(mels, False, 11000, 550, kernel='teamg_batch', batch_rows=2, noise_mode=_cabi.NOISE_ARGMAX)
    finally:
        m.native().debug_force_no_teams(False)
    with pytest.raises(ValueError, match='stream'):
        m.stream(kernel='teamg_batch')
    with pytest.raises(_cabi.WrnnError, match='stream'):
        m.stream(kernel=_cabi.KERNEL_TEAMG_BATCH)
    with pytest.warns(RuntimeWarning, match="kernel='teamg_batch'"):
        m._slow_warned = False
        m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_ARGMAX)
    assert m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE and m.last_timing['batch_rows'] == 1   # AUTO is untouched: both kernels are opt-in
