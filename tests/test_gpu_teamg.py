"""WRNN_KERNEL_TEAMG, the XCD-team kernel for any model dims, against the oracle under the rules of tests/parity_util.py.

The four dim sets of tests/teamg_cases.py (A small and mostly LDS resident, B where nothing divides and workgroups own nothing, C 1024 / 1024
almost fully streamed, D the reference hparams on the generic kernel); models from synth.make_state_dict, oracle OracleModel(fast=True),
injected noise, every step compared, `last_timing['kernel'] == 6` after every call.  The RAW seeds are chosen so that the oracle's own run has
no race margin below NEAR_TIE (asserted on its output, as tests/test_gpu_team_hops.py does): no step is excused, label equality is exact.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import philox_ref
from tests.parity_util import (NEAR_TIE, bound_near_ties, check_free_run_raw, check_mol, check_on_gpu_trajectory_mol,
                               check_on_gpu_trajectory_raw, check_teacher_forced_raw, parity_report)
from tests.teamg_cases import DIM_SETS

pytestmark = pytest.mark.gpu

TEAMG = 6
FRAMES = {'A': 9, 'B': 100, 'C': 20, 'D': 4}            # 1 152, 600, 120 and 1 100 steps
NOISE_SEED = {('A', 'RAW'): 8, ('B', 'RAW'): 8, ('C', 'RAW'): 8, ('D', 'RAW'): 8}

_MODELS, _CASES = {}, {}


def _dims(name, mode):
    d = dict(DIM_SETS[name])
    if mode == 'MOL' and name == 'D':
        d['bits'] = 9
    return d


def _model(name, mode='RAW'):
    """One (WaveRNN on the GPU, state_dict, oracle) per (dim set, mode) for the whole module: the weights are packed once."""
    key = (name, mode)
    if key not in _MODELS:
        from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
        from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
        dims = _dims(name, mode)
        sd = make_state_dict(7, mode, 'peaky' if mode == 'RAW' else 'default', **dims)
        m = WaveRNN(**dims, mode=mode)
        m.verbose = False
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        m.to('cuda:0')
        om = orc.OracleModel(sd, mode=mode, bits=dims['bits'], upsample_factors=dims['upsample_factors'], pad=dims['pad'], fast=True)
        _MODELS[key] = (m, sd, om)
    return _MODELS[key]


def _mels(name, seed, B, T):
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    return make_mels(seed, B, T, feat_dims=DIM_SETS[name]['feat_dims'])


def _case(name, mode, B=3):
    """Mels, injected noise and the oracle's free + teacher-forced runs of one (dim set, mode), computed once."""
    key = (name, mode, B)
    if key in _CASES:
        return _CASES[key]
    m, _, om = _model(name, mode)
    T, hop = FRAMES[name], DIM_SETS[name]['hop_length']
    L = T * hop
    mels = _mels(name, 3, B, T)
    rng = np.random.Generator(np.random.PCG64(NOISE_SEED.get((name, mode), 8)))
    cm, ca = om.conditioning(mels)
    if mode == 'RAW':
        noise = (rng.standard_exponential((L, B, m.n_classes)).astype(np.float32),)
        run = lambda **kw: om.loop(cm, ca, orc.NOISE_EXPO, noise[0], **kw)
    else:
        noise = (rng.uniform(1e-5, 1 - 1e-5, size=(L, B, 10)).astype(np.float32), rng.uniform(1e-5, 1 - 1e-5, size=(L, B)).astype(np.float32))
        run = lambda **kw: om.loop(cm, ca, 0, noise[0], noise[1], **kw)
    free = run()
    forced = run(x_forced=free['samples'], want_logits=True)
    _CASES[key] = dict(mels=mels, noise=noise, free=free, forced=forced, L=L, T=T, hop=hop)
    return _CASES[key]


def _noise_kw(c):
    from tacotronv2_wavernn_chinese_amd import _cabi
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=c['noise'][0])
    if len(c['noise']) > 1:
        kw['noise2'] = c['noise'][1]
    return kw


def _no_near_tie(ref, what):
    """The condition the seeds were picked for: the oracle's own run has no near-tie, so nothing is excused."""
    assert float(ref['margin'].min()) >= NEAR_TIE, f'{what}: the oracle has a near-tie (margin {float(ref["margin"].min()):.3e}): pick other seeds'


def _gen(m, *args, **kw):
    res = m.generate_raw(*args, kernel='teamg', **kw)
    assert m.last_timing['kernel'] == TEAMG                                   # no silent fallback
    return res


# ---- 1. every step of every row, free and teacher-forced -------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D'])
def test_raw_every_step_free_and_teacher_forced(name):
    m, _, _ = _model(name)
    c = _case(name, 'RAW')
    B, L = 3, c['L']
    free, forced = c['free'], c['forced']
    _no_near_tie(free, f'set {name}')
    np.testing.assert_array_equal(forced['labels'], free['labels'])
    bound = 2e-5 * max(1.0, float(np.abs(forced['logits']).max()))
    res = _gen(m, c['mels'], False, 11000, 550, **_noise_kw(c))
    assert m.last_timing['rows'] == B and m.last_timing['steps'] == L
    got = res['labels'].cpu().numpy().T
    assert got.shape == (L, B)
    assert all(f is None for f in check_free_run_raw(got, free))             # no near-tie in the oracle: the rule excuses nothing
    smp = res['samples'].cpu().numpy().T
    np.testing.assert_array_equal(smp, 2.0 * got.astype(np.float32) / np.float32(m.n_classes - 1.0) - np.float32(1.0))
    res = _gen(m, c['mels'], False, 11000, 550, x_forced=free['samples'], want_logits=True, **_noise_kw(c))
    gotf = res['labels'].cpu().numpy().T
    assert check_teacher_forced_raw(gotf, forced) == 0
    err = float(np.abs(res['logits'].cpu().numpy() - forced['logits']).max())
    parity_report(f'teamg: set {name} RAW B={B} T={c["T"]}: steps compared {got.size + gotf.size} (free + forced), near-tie divergences 0 '
                  f'(oracle min margin {float(free["margin"].min()):.2e}), max |dlogit| {err:.3e} (bound {bound:.3e})')
    assert err <= bound


@pytest.mark.parametrize('name', ['A', 'B'])
def test_mol_free_and_teacher_forced(name):
    m, _, _ = _model(name, 'MOL')
    c = _case(name, 'MOL')
    res = _gen(m, c['mels'], False, 11000, 550, **_noise_kw(c))
    assert m.last_timing['rows'] == 3
    smp, mix = res['samples'].cpu().numpy().T, res['labels'].cpu().numpy().T
    check_mol(smp, mix, c['free'], teacher_forced=False)
    res = _gen(m, c['mels'], False, 11000, 550, x_forced=c['free']['samples'], **_noise_kw(c))
    smpf, mixf = res['samples'].cpu().numpy().T, res['labels'].cpu().numpy().T
    check_mol(smpf, mixf, c['forced'], teacher_forced=True)
    samef = mixf == c['forced']['labels']
    parity_report(f'teamg: set {name} MOL B=3 T={c["T"]}: steps compared {mix.size} free + {mixf.size} forced, mixture-index mismatches '
                  f'{int((mix != c["free"]["labels"]).sum())} / {int((~samef).sum())}, max |dsample| forced '
                  f'{float(np.abs(smpf - c["forced"]["samples"])[samef].max()):.3e} (tol 2.0e-05)')


def test_x_init_feeds_step_zero():
    """x_init with teacher forcing = the pass WaveRNN.forward makes: the logits of step 0 depend on x_init, and equal the SIMPLE kernel's
    within the logit bound at every step."""
    m, _, _ = _model('B')
    c = _case('B', 'RAW')
    x0 = np.asarray([0.5, -0.25, 1.0], np.float32)
    kw = dict(x_forced=c['free']['samples'], want_logits=True, x_init=x0, **_noise_kw(c))
    a = _gen(m, c['mels'], False, 11000, 550, **kw)['logits'].cpu().numpy()
    b = m.generate_raw(c['mels'], False, 11000, 550, kernel='simple', **kw)['logits'].cpu().numpy()
    assert np.abs(a - b).max() <= 2e-5 * max(1.0, float(np.abs(b).max()))
    assert np.abs(a[0] - c['forced']['logits'][0]).max() > 1e-3               # step 0 saw x_init, not 0


# ---- 2. placements: all streamed, one layer half resident, the default ------------------------------------------------------------------

def test_set_b_is_bit_equal_under_every_weight_placement():
    m, _, _ = _model('B')
    c = _case('B', 'RAW')
    nat = m.native()
    full = nat.teamg_plan()
    assert all(L['resident_units'] == max(L['own_count']) for L in full['layers'].values())      # set B: everything fits
    order = ['fc3', 'fc2', 'fc1', 'rnn2']
    r2 = full['layers']['rnn2']
    half = sum(full['layers'][n]['lds_bytes'] for n in order[:3]) + r2['lds_bytes'] // 2
    p = nat.teamg_plan(half)
    assert 0 < p['layers']['rnn2']['resident_units'] < max(r2['own_count']) and p['layers']['rnn1']['resident_units'] == 0
    _no_near_tie(c['free'], 'set B')
    outs = []
    try:
        for budget in (0, half, -1):
            nat.debug_teamg_lds_budget(budget)
            res = _gen(m, c['mels'], False, 11000, 550, **_noise_kw(c))
            outs.append((res['labels'].cpu().numpy(), res['samples'].cpu().numpy()))
    finally:
        nat.debug_teamg_lds_budget(-1)
    for lab, smp in outs[1:]:
        np.testing.assert_array_equal(lab, outs[0][0])
        np.testing.assert_array_equal(smp, outs[0][1])
    assert all(f is None for f in check_free_run_raw(outs[0][0].T, c['free']))


# ---- 3. more rows than teams, ragged -----------------------------------------------------------------------------------------------------

def test_eleven_ragged_rows_make_a_second_pass():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, om = _model('B')
    hop, F = 6, 13
    lens = [33, 21, 40, 27, 38, 22, 31, 40, 25, 36, 29]
    B, Tm = len(lens), max(lens)
    assert B > m.native().team_info()[1]                                      # some team runs two rows one after the other
    mels = np.zeros((B, F, Tm), np.float32)
    for i, t in enumerate(lens):
        mels[i, :, :t] = _mels('B', 500 + i, 1, t)[0]
    q = np.random.Generator(np.random.PCG64(15)).standard_exponential((Tm * hop, B, m.n_classes), dtype=np.float32)
    res = _gen(m, mels, False, 11000, 550, frames=np.asarray(lens, np.int32), noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    assert m.last_timing['rows'] == B
    lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
    compared, near = 0, []
    for i, t in enumerate(lens):
        L = t * hop
        cm, ca = om.conditioning(mels[i:i + 1, :, :t])
        qi = np.ascontiguousarray(q[:L, i:i + 1])
        st = check_on_gpu_trajectory_raw(lab[i:i + 1, :L].T, smp[i:i + 1, :L].T, lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, qi, x_forced=xf))
        compared += st['compared']
        near += [(t_, i, d) for t_, _, d in st['near_ties']]
        assert not lab[i, L:].any() and not smp[i, L:].any(), f'row {i}: written past its own length'
    assert compared == hop * sum(lens)
    bound_near_ties('teamg: set B RAW, 11 ragged rows of 21 .. 40 frames', compared, near)


# ---- 4. folds ----------------------------------------------------------------------------------------------------------------------------

def test_folds_of_one_utterance_and_of_three():
    """generate_raw(batched=True): the folds start every 56 positions, inside a frame of hop 6, and the last one runs past the clip's end
    (zero conditioning from there on).  Then three clips folded in one call with per-utterance seeds: every clip's rows are bit-equal to
    the call on that clip alone."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, om = _model('B')
    hop, T, target, overlap = 6, 60, 47, 9
    mels = _mels('B', 13, 1, T)
    cm, ca = om.conditioning(mels)
    fm, fa = om.fold(cm, target, overlap), om.fold(ca, target, overlap)
    rows, steps = fm.shape[0], target + 2 * overlap
    assert rows >= 6 and (rows - 1) * (target + overlap) + steps > T * hop    # the last fold is padded 'after'
    q = np.random.Generator(np.random.PCG64(14)).standard_exponential((steps, rows, m.n_classes), dtype=np.float32)
    res = _gen(m, mels, True, target, overlap, noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    assert m.last_timing['rows'] == rows and m.last_timing['steps'] == steps
    lab, smp = res['labels'].cpu().numpy().T, res['samples'].cpu().numpy().T
    st = check_on_gpu_trajectory_raw(lab, smp, lambda xf: om.loop(fm, fa, orc.NOISE_EXPO, q, x_forced=xf))
    assert st['compared'] == rows * steps
    bound_near_ties(f'teamg: set B RAW folds {target}/{overlap} ({rows} rows x {steps})', st['compared'], st['near_ties'])

    lens, seeds = [60, 31, 44], [0xA1, 0xB2B2B2B2B2, 0xC3]
    batch = np.zeros((3, 13, 60), np.float32)
    for i, t in enumerate(lens):
        batch[i, :, :t] = _mels('B', 700 + i, 1, t)[0]
    many = m.generate_raw_folded(batch, lens, target, overlap, seeds=seeds, kernel='teamg')
    assert m.last_timing['kernel'] == TEAMG and m.last_timing['rows'] == many['fold0'][-1] > m.native().team_info()[1]
    lm, sm, fold0 = many['labels'].cpu().numpy(), many['samples'].cpu().numpy(), many['fold0']
    for i, t in enumerate(lens):
        solo = _gen(m, batch[i:i + 1, :, :t], True, target, overlap, seed=seeds[i])
        np.testing.assert_array_equal(lm[fold0[i]:fold0[i + 1]], solo['labels'].cpu().numpy(), err_msg=f'clip {i}')
        np.testing.assert_array_equal(sm[fold0[i]:fold0[i + 1]], solo['samples'].cpu().numpy(), err_msg=f'clip {i}')


# ---- 5. device Philox noise, per-utterance seeds -------------------------------------------------------------------------------------------

def test_philox_raw_with_per_utterance_seeds_is_the_replayed_stream():
    m, _, om = _model('A')
    B, T, hop = 3, 5, 128
    L = T * hop
    mels = _mels('A', 41, B, T)
    seeds = [0x1234567, 0xFEDCBA9800000000 + 0x1234567, 0x77]
    res = _gen(m, mels, False, 11000, 550, noise_mode='philox', seeds=seeds)
    lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
    compared, near = 0, []
    for b in range(B):                                                        # row key of an utterance with its own seed: (seed, step, 0)
        u = philox_ref.philox_uniform_raw(seeds[b], L, 1, m.n_classes)
        q = (-np.log(u.astype(np.float64))).astype(np.float32)
        cm, ca = om.conditioning(mels[b:b + 1])
        st = check_on_gpu_trajectory_raw(lab[b:b + 1].T, smp[b:b + 1].T, lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=xf))
        compared += st['compared']
        near += [(t, b, d) for t, _, d in st['near_ties']]
    assert compared == L * B
    bound_near_ties('teamg: set A RAW Philox, per-utterance seeds', compared, near)
    assert len({lab[b].tobytes() for b in range(B)}) == B
    # the call-wide seed keys row b by (seed, step, b)
    res = _gen(m, mels, False, 11000, 550, noise_mode='philox', seed=0x5EED)
    lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
    q = (-np.log(philox_ref.philox_uniform_raw(0x5EED, L, B, m.n_classes).astype(np.float64))).astype(np.float32)
    cm, ca = om.conditioning(mels)
    st = check_on_gpu_trajectory_raw(lab.T, smp.T, lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=xf))
    bound_near_ties('teamg: set A RAW Philox, call-wide seed', st['compared'], st['near_ties'])


def test_philox_mol_with_per_utterance_seeds_is_the_replayed_stream():
    m, _, om = _model('A', 'MOL')
    B, T, hop = 3, 5, 128
    L = T * hop
    mels = _mels('A', 42, B, T)
    seeds = [0x1234568, 0x1234567 + 2 ** 32, 0x99]
    res = _gen(m, mels, False, 11000, 550, noise_mode='philox', seeds=seeds)
    smp, mix = res['samples'].cpu().numpy(), res['labels'].cpu().numpy()
    compared = mism = 0
    for b in range(B):
        u_mix, u_log = philox_ref.philox_mol_uniforms(seeds[b], 0, L, [0])
        cm, ca = om.conditioning(mels[b:b + 1])
        st = check_on_gpu_trajectory_mol(np.ascontiguousarray(smp[b:b + 1].T), np.ascontiguousarray(mix[b:b + 1].T),
                                         lambda xf: om.loop(cm, ca, 0, u_mix, u_log, x_forced=xf))
        compared, mism = compared + st['compared'], mism + st['index_mismatches']
    parity_report(f'teamg: set A MOL Philox, per-utterance seeds: steps compared {compared}, mixture-index near-ties {mism}')
    assert compared == L * B and mism <= 1 + int(1e-5 * compared)
    assert np.abs(smp).max() <= 1.0 and len({smp[b].tobytes() for b in range(B)}) == B


def test_argmax_noise_mode():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, om = _model('B')
    mels = _mels('B', 9, 2, 30)
    res = _gen(m, mels, False, 11000, 550, noise_mode=_cabi.NOISE_ARGMAX)
    cm, ca = om.conditioning(mels)
    check_free_run_raw(res['labels'].cpu().numpy().T, om.loop(cm, ca, orc.NOISE_ARGMAX))


# ---- 6. / 7. what stays refused --------------------------------------------------------------------------------------------------------------

def test_a_stream_refuses_teamg():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _model('A')
    with pytest.raises(ValueError, match='stream'):
        m.stream(kernel='teamg')
    with pytest.raises(_cabi.WrnnError, match='stream'):
        m.stream(kernel=_cabi.KERNEL_TEAMG)


def test_explicit_team2_on_other_dims_still_raises_and_auto_is_unchanged():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _model('A')
    mels = _mels('A', 21, 1, 2)
    with pytest.raises(_cabi.WrnnError):
        m.generate_raw(mels, False, 11000, 550, kernel=_cabi.KERNEL_TEAM2, noise_mode=_cabi.NOISE_ARGMAX)
    with pytest.warns(RuntimeWarning, match="kernel='teamg'"):
        m._slow_warned = False
        m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_ARGMAX)
    assert m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE                     # TEAMG is opt-in
    m.native().debug_force_no_teams(True)
    try:
        with pytest.raises(_cabi.WrnnError, match='force_no_teams'):
            m.generate_raw(mels, False, 11000, 550, kernel='teamg', noise_mode=_cabi.NOISE_ARGMAX)
    finally:
        m.native().debug_force_no_teams(False)
