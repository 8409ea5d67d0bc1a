"""WRNN_KERNEL_SIMPLE, the any-shape loop kernel AUTO runs for every model that is not the reference hparams, at the dim sets of
tests/simple_cases.py: more than 512 hidden units (a thread owns two), more than 512 fc rows, more classes than threads (up to 32 768 and 133 KB
of dynamic LDS), the smallest dims the library admits, pad 1 and pad 3 -- and, at such dims, the call forms that were only tested at the reference
hparams: Philox noise, per-utterance seeds, ragged rows, folds of one and of two utterances, streams, the greedy race on exact ties.

Models from synth.make_state_dict, oracle OracleModel(fast=True), one of each per (set, mode) for the whole module; `last_timing['kernel'] ==
KERNEL_SIMPLE` after every call.  tests/test_simple_cases_host.py asserts on the CPU that the oracle's own runs on these inputs have no race margin
below NEAR_TIE / NEAR_TIE_MOL: the parity rules excuse nothing here, labels are equal at every step or the test fails.  Logits are held to
simple_cases.logit_bound, the conditioning to simple_cases.conditioning_bounds (both from the reference side alone: the fp32 oracle against
float64); everything else is exact equality.
"""
import time

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import simple_cases as sc
from tests.parity_util import (NEAR_TIE, NEAR_TIE_MOL, check_free_run_raw, check_mol, check_on_gpu_trajectory_mol, check_on_gpu_trajectory_raw,
                               check_teacher_forced_raw, parity_report, stream_raw)

pytestmark = pytest.mark.gpu

_MODELS = {}
AUTO_CASE = ('S1', 'RAW')            # the one case that passes kernel=None: AUTO -> SIMPLE on foreign dims, with its warning


def _build(name, mode, sd, **over):
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**dict(sc.DIM_SETS[name], **over), mode=mode)
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    return m


def _model(name, mode='RAW'):
    """One WaveRNN on the GPU per (dim set, mode) for the whole module: the weights are packed once."""
    if (name, mode) not in _MODELS:
        _MODELS[name, mode] = _build(name, mode, sc.state_dict(name, mode))
    return _MODELS[name, mode]


def _gen(m, *args, kernel='simple', **kw):
    from tacotronv2_wavernn_chinese_amd import _cabi
    res = m.generate_raw(*args, kernel=kernel, **kw)
    assert m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE
    return res


def _noise_kw(noise):
    from tacotronv2_wavernn_chinese_amd import _cabi
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=noise[0])
    if len(noise) > 1:
        kw['noise2'] = noise[1]
    return kw


def _no_near_tie(ref, mode, what):
    floor = NEAR_TIE if mode == 'RAW' else NEAR_TIE_MOL
    assert float(ref['margin'].min()) >= floor, f'{what}: the oracle has a near-tie (margin {float(ref["margin"].min()):.3e})'


def _t(res):
    return res['labels'].cpu().numpy().T, res['samples'].cpu().numpy().T


def _raw_samples(labels, nc):
    """sample = 2 k / (n_classes - 1) - 1 evaluated in fp32, as the kernel and the oracle do."""
    return 2.0 * labels.astype(np.float32) / np.float32(nc - 1.0) - np.float32(1.0)


# ---- 1. every step of every row, free and teacher-forced -------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode', sc.CASES)
def test_every_step_free_and_teacher_forced(name, mode):
    t0 = time.time()
    m, c = _model(name, mode), sc.case(name, mode)
    L, nc = c['L'], sc.n_classes(name, mode)
    free, forced = c['free'], c['forced']
    _no_near_tie(free, mode, f'{name} {mode}')
    np.testing.assert_array_equal(forced['labels'], free['labels'])
    bound, g = sc.logit_bound(name, mode)
    lg_range = float(forced['logits'].max() - forced['logits'].min())
    assert bound < 1e-3 * lg_range
    if (name, mode) == AUTO_CASE:
        m._slow_warned = False
        with pytest.warns(RuntimeWarning, match='WRNN_KERNEL_SIMPLE'):
            res = _gen(m, c['mels'], False, 11000, 550, kernel=None, **_noise_kw(c['noise']))
    else:
        res = _gen(m, c['mels'], False, 11000, 550, **_noise_kw(c['noise']))
    assert m.last_timing['rows'] == sc.B and m.last_timing['steps'] == L
    us_step = 1e3 * m.last_timing['loop_ms'] / L
    lab, smp = _t(res)
    assert lab.shape == (L, sc.B)
    if mode == 'RAW':
        assert all(f is None for f in check_free_run_raw(lab, free))          # no near-tie in the oracle: the rule excuses nothing
        np.testing.assert_array_equal(lab, free['labels'])
        np.testing.assert_array_equal(smp, _raw_samples(lab, nc))
    else:
        check_mol(smp, lab, free, teacher_forced=False)
        assert int((lab != free['labels']).sum()) == 0
    res = _gen(m, c['mels'], False, 11000, 550, x_forced=free['samples'], want_logits=True, **_noise_kw(c['noise']))
    labf, smpf = _t(res)
    if mode == 'RAW':
        assert check_teacher_forced_raw(labf, forced) == 0
        np.testing.assert_array_equal(smpf, _raw_samples(labf, nc))
    else:
        check_mol(smpf, labf, forced, teacher_forced=True)
        assert int((labf != forced['labels']).sum()) == 0
    lg = res['logits'].cpu().numpy()
    assert lg.shape == (L, sc.B, nc)
    err = float(np.abs(lg - forced['logits']).max())
    parity_report(f'simple dims: {name} {mode} B={sc.B} T={c["T"]}: steps compared {lab.size + labf.size} (free + forced), label mismatches 0 '
                  f'(oracle min margin {float(free["margin"].min()):.2e}), g = max |oracle fp32 - float64| {g:.3e}, kernel max |dlogit| {err:.3e} '
                  f'= {err / g if g else float("nan"):.2f} g (bound {bound:.3e}, logit range {lg_range:.3e}), loop {us_step:.0f} us/step, '
                  f'wall {time.time() - t0:.2f} s')
    assert err <= bound


# ---- 2. the prologue ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['S3', 'S5'])
def test_prologue_against_the_oracle(name):
    """S3: one channel, three taps, res_out 4 above compute 1 (the MelResNet kernel's thread count is max(C, R)); S5: seven taps over three
    upsample layers, 72 aux channels in four slices of 18."""
    m, c, d = _model(name), sc.case(name, 'RAW'), sc.DIM_SETS[name]
    (b_up, g_up), (b_aux, g_aux) = sc.conditioning_bounds(name, 'RAW')
    nat = m.native()
    up = torch.full((sc.B, c['L'], d['feat_dims']), float('nan'), device='cuda')
    aux = torch.full((sc.B, c['L'], d['res_out_dims']), float('nan'), device='cuda')
    nat.conditioning(torch.from_numpy(c['mels']).cuda().data_ptr(), sc.B, c['T'], up.data_ptr(), aux.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    e_up, e_aux = float(np.abs(up.cpu().numpy() - c['cm']).max()), float(np.abs(aux.cpu().numpy() - c['ca']).max())
    parity_report(f'simple dims: {name} prologue: up g {g_up:.3e}, kernel error {e_up:.3e} = {e_up / g_up:.2f} g (bound {b_up:.3e}); '
                  f'aux g {g_aux:.3e}, kernel error {e_aux:.3e} = {e_aux / g_aux:.2f} g (bound {b_aux:.3e})')
    np.testing.assert_allclose(up.cpu().numpy(), c['cm'], rtol=0, atol=b_up)
    np.testing.assert_allclose(aux.cpu().numpy(), c['ca'], rtol=0, atol=b_aux)


# ---- 3. device Philox noise, per-utterance seeds -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode', sc.PHILOX_CASES)
def test_philox_is_the_replayed_stream(name, mode):
    """The draws of (seed, step, row, class) replayed by tests/philox_ref.py and handed to the oracle, which is driven along the GPU's own
    samples: every step.  S4: class indices up to 32 767, 64 draws per thread and step."""
    m, c, om = _model(name, mode), sc.philox_case(name, mode), sc.oracle_model(name, mode)
    _no_near_tie(c['free'], mode, f'{name} {mode} Philox')
    res = _gen(m, c['mels'], False, 11000, 550, noise_mode='philox', seed=sc.PHILOX_SEED)
    lab, smp = _t(res)
    loop = lambda xf: sc.oracle_loop(om, mode, c['cm'], c['ca'], c['noise'], x_forced=xf)
    if mode == 'RAW':
        st = check_on_gpu_trajectory_raw(lab, smp, loop)
        assert st['compared'] == c['L'] * sc.B and st['near_ties'] == []
    else:
        st = check_on_gpu_trajectory_mol(np.ascontiguousarray(smp), np.ascontiguousarray(lab), loop)
        assert st['compared'] == c['L'] * sc.B and st['index_mismatches'] == 0 and np.abs(smp).max() <= 1.0
    np.testing.assert_array_equal(lab, c['free']['labels'])                   # so the run IS the oracle's free run on these draws
    assert len({lab[:, b].tobytes() for b in range(sc.B)}) == sc.B
    other = _t(_gen(m, c['mels'], False, 11000, 550, noise_mode='philox', seed=sc.PHILOX_SEED ^ (1 << 40)))[0]
    assert not np.array_equal(other, lab)                                     # the high word of the seed is in the key


def test_per_utterance_seeds_in_two_batch_orders():
    m, c = _model('S1'), sc.case('S1', 'RAW')
    solo = [_gen(m, c['mels'][b:b + 1], False, 11000, 550, noise_mode='philox', seed=sc.UTT_SEEDS[b]) for b in range(sc.B)]
    solo = [(r['labels'].cpu().numpy()[0], r['samples'].cpu().numpy()[0]) for r in solo]
    assert len({s[0].tobytes() for s in solo}) == sc.B
    for order in ([0, 1, 2], [2, 0, 1]):
        res = _gen(m, c['mels'][order], False, 11000, 550, noise_mode='philox', seeds=[sc.UTT_SEEDS[b] for b in order])
        lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
        for i, b in enumerate(order):
            np.testing.assert_array_equal(lab[i], solo[b][0], err_msg=f'order {order}: row {i} (utterance {b})')
            np.testing.assert_array_equal(smp[i], solo[b][1], err_msg=f'order {order}: row {i} (utterance {b})')


# ---- 4. ragged rows and folds, S5 --------------------------------------------------------------------------------------------------------

def test_ragged_rows_on_s5():
    """frames (20, 1, 7) at pad 3: each row equals the oracle on its clip alone and its solo call, and is zero past its own length."""
    m, r = _model('S5'), sc.ragged_case()
    hop = r['hop']
    res = _gen(m, r['mels'], False, 11000, 550, frames=np.asarray(sc.RAGGED_FRAMES, np.int32), **_noise_kw(r['noise']))
    assert m.last_timing['rows'] == sc.B
    lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
    for b, t in enumerate(sc.RAGGED_FRAMES):
        L, ref = t * hop, r['refs'][b]
        _no_near_tie(ref['free'], 'RAW', f'ragged row {b}')
        np.testing.assert_array_equal(lab[b, :L], ref['free']['labels'][:, 0], err_msg=f'row {b} against the oracle')
        solo = _gen(m, r['mels'][b:b + 1, :, :t], False, 11000, 550, **_noise_kw((ref['q'],)))
        np.testing.assert_array_equal(lab[b, :L], solo['labels'].cpu().numpy()[0], err_msg=f'row {b} against its solo call')
        np.testing.assert_array_equal(smp[b, :L], solo['samples'].cpu().numpy()[0], err_msg=f'row {b} against its solo call')
        assert not lab[b, L:].any() and not smp[b, L:].any(), f'row {b}: written past its own length'


def test_folds_of_one_utterance_and_of_two_on_s5():
    """target 50 / overlap 7: the folds start every 57 positions, inside a frame of hop 12, and the last one runs into the zero padding.
    Every step of every fold against the oracle's fold on the replayed Philox draws of its global row; then two clips in one call, whose rows
    of clip 0 are the single call's."""
    m, f, om = _model('S5'), sc.fold_case(), sc.oracle_model('S5', 'RAW')
    fold0, steps = f['fold0'], f['steps']

    def check(lab, smp, b):
        ref = f['refs'][b]
        _no_near_tie(ref['free'], 'RAW', f'folds of clip {b}')
        st = check_on_gpu_trajectory_raw(lab.T, smp.T, lambda xf: om.loop(ref['fm'], ref['fa'], orc.NOISE_EXPO, ref['q'], x_forced=xf))
        assert st['compared'] == lab.size and st['near_ties'] == []
        np.testing.assert_array_equal(lab.T, ref['free']['labels'])

    one = _gen(m, f['clips'][0][None], True, sc.FOLD_TARGET, sc.FOLD_OVERLAP, noise_mode='philox', seed=sc.FOLD_SEED)
    assert m.last_timing['rows'] == fold0[1] and m.last_timing['steps'] == steps
    lab1, smp1 = one['labels'].cpu().numpy(), one['samples'].cpu().numpy()
    assert lab1.shape == (fold0[1], steps)
    check(lab1, smp1, 0)

    from tacotronv2_wavernn_chinese_amd import _cabi
    many = m.generate_raw_folded(f['batch'], list(sc.FOLD_FRAMES), sc.FOLD_TARGET, sc.FOLD_OVERLAP, seed=sc.FOLD_SEED, kernel='simple')
    assert m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE and m.last_timing['rows'] == fold0[-1]
    assert many['fold0'].tolist() == fold0 and many['steps'] == steps
    lab, smp = many['labels'].cpu().numpy(), many['samples'].cpu().numpy()
    for b in range(2):
        check(lab[fold0[b]:fold0[b + 1]], smp[fold0[b]:fold0[b + 1]], b)
    np.testing.assert_array_equal(lab[:fold0[1]], lab1)
    np.testing.assert_array_equal(smp[:fold0[1]], smp1)


# ---- 5. streams --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode,rows', [('S1', 'RAW', 1), ('S1', 'RAW', 3), ('S5', 'RAW', 1), ('S5', 'RAW', 3), ('S1', 'MOL', 1), ('S1', 'MOL', 3)])
def test_a_stream_equals_the_offline_call(name, mode, rows):
    """Pushes of (1, 7, 3, 9) frames: the later ones resume from the saved state [h1 | h2 | x] -- at S1 with the second units of threads 0..7,
    at S5 with a 3-frame look-ahead and pushes that begin inside a frame.  A scratch build whose kernel saved only h1[0..511] failed every S5
    case and both S1 MOL cases; the S1 RAW cases passed it (eight stale units of 520 did not move a 128-class label in 120 steps): at S1 it is
    the continuous MOL sample that pins the second units' state.
    Workspace: csrc/stream.hip sizes each buffer to the largest push so far ("bounded by the largest push"), and the largest
    push here, 9 frames, comes last -- so `workspace_bytes` does grow after the second push, by design.  What is asserted instead is stronger
    than "does not grow": the value after EVERY push equals the one predicted from the pushes alone (simple_cases.stream_buffer_bytes), and
    the last, empty push adds nothing."""
    m, c, d = _model(name, mode), sc.case(name, mode), sc.DIM_SETS[name]
    mels = c['mels'][:rows]
    off = _gen(m, mels, False, 11000, 550, noise_mode='philox', seed=sc.PHILOX_SEED)
    infos = []
    lab, smp = stream_raw(m, mels, sc.STREAM_CHUNKS, infos=infos, seed=sc.PHILOX_SEED, kernel='simple', tail='none')
    np.testing.assert_array_equal(lab, off['labels'].cpu().numpy())
    np.testing.assert_array_equal(smp, off['samples'].cpu().numpy())
    assert infos[-1]['frames_in'] == c['T'] and infos[-1]['steps_done'] == c['L']
    pushes_that_ran = sum(1 for a, b in zip(infos, infos[1:]) if b['steps_done'] > a['steps_done'])
    assert pushes_that_ran >= 3                                               # at least two resumes from the saved state
    ws = [i['workspace_bytes'] for i in infos]
    want = [ws[0] + b for b in sc.stream_buffer_bytes(d, rows, sc.STREAM_CHUNKS)]
    assert ws[1:] == want, f'workspace after each push {ws[1:]}, predicted {want}'
    assert ws[-1] == ws[-2]                                                   # the last, empty push grows nothing
    if rows == 1:
        assert len(set(lab[0].tolist())) >= 2


# ---- 6. exact ties in the greedy race ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c1,c2', sc.TIE_PAIRS)
def test_an_exact_tie_goes_to_the_first_index(c1, c2):
    """S2, fc3 row and bias of class c1 copied onto c2, +50 on both biases: the pair ties exactly and wins every step.  The oracle's rule is a
    strict `>`, so c1: inside one thread (5, 517), across waves (70, 200), and with the higher index in a lower wave and lane (100, 522)."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    sd = sc.tie_state_dict(c1, c2)
    m = _build('S2', 'RAW', sd)
    mels = sc.mels_of('S2', T=sc.TIE_FRAMES)
    om = sc.oracle_of(sd, 'S2', 'RAW')
    cm, ca = om.conditioning(mels)
    ref = om.loop(cm, ca, orc.NOISE_ARGMAX, want_logits=True)
    np.testing.assert_array_equal(ref['logits'][:, :, c1], ref['logits'][:, :, c2])
    assert (ref['labels'] == c1).all()
    res = _gen(m, mels, False, 11000, 550, noise_mode=_cabi.NOISE_ARGMAX, want_logits=True)
    lab, smp = _t(res)
    lg = res['logits'].cpu().numpy()
    np.testing.assert_array_equal(lg[:, :, c1], lg[:, :, c2])                 # the kernel's two sums tie exactly too
    assert (lg[:, :, c1] > np.delete(lg, [c1, c2], axis=2).max(axis=2) + 1.0).all()
    assert (lab == c1).all(), f'labels {sorted(set(lab.reshape(-1).tolist()))}, want {c1} everywhere'
    np.testing.assert_array_equal(lab, ref['labels'])
    np.testing.assert_array_equal(smp, _raw_samples(lab, 1024))


# ---- 7. what is refused ------------------------------------------------------------------------------------------------------------------

def test_sixteen_bits_at_s4_is_refused_by_the_lds_limit():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    dims = dict(sc.DIM_SETS['S4'], bits=16)
    assert sc.simple_lay_bytes(dims) > sc.LDS_LIMIT
    m = _build('S4', 'RAW', make_state_dict(sc.WEIGHT_SEED, 'RAW', 'peaky', **dims), bits=16)
    with pytest.raises(_cabi.WrnnError, match='160 KB of LDS') as ei:
        m.generate_raw(sc.mels_of('S4'), False, 11000, 550, kernel='simple', noise_mode=_cabi.NOISE_ARGMAX)
    assert ei.value.code == _cabi.ERR_INVALID and str(sc.simple_lay_bytes(dims)) in str(ei.value)
    # nothing was launched: the next valid call of the process, at 15 bits, is the oracle's run
    c = sc.case('S4', 'RAW')
    lab, _ = _t(_gen(_model('S4'), c['mels'], False, 11000, 550, **_noise_kw(c['noise'])))
    np.testing.assert_array_equal(lab, c['free']['labels'])


def test_an_explicit_reference_dims_kernel_on_s1_is_refused():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, c = _model('S1'), sc.case('S1', 'RAW')
    for kernel in ('team2', 'batch', 'batch_cs'):
        with pytest.raises(_cabi.WrnnError) as ei:
            m.generate_raw(c['mels'], False, 11000, 550, kernel=kernel, **_noise_kw(c['noise']))
        assert ei.value.code == _cabi.ERR_INVALID, kernel
    lab, _ = _t(_gen(m, c['mels'], False, 11000, 550, **_noise_kw(c['noise'])))
    np.testing.assert_array_equal(lab, c['free']['labels'])
