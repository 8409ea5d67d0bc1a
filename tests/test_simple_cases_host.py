"""What tests/test_gpu_simple_dims.py relies on, checked on the CPU: on the inputs of tests/simple_cases.py the C oracle's own runs have no race
margin below NEAR_TIE (RAW) / NEAR_TIE_MOL (MOL), so `check_free_run_raw`, `check_teacher_forced_raw` and `check_mol` excuse no step there and a
green GPU run means equal labels at every step; the runs are not degenerate (several labels win, at S4 one past class 1024); the kernel's LDS
need, restated, is where the GPU file says it is; the logit and conditioning bounds come out of the reference side alone.
"""
import numpy as np
import pytest

from tests import simple_cases as sc
from tests.parity_util import NEAR_TIE, NEAR_TIE_MOL


def _no_near_tie(ref, mode, what):
    floor = NEAR_TIE if mode == 'RAW' else NEAR_TIE_MOL
    worst = float(ref['margin'].min())
    assert worst >= floor, f'{what}: the oracle has a near-tie (margin {worst:.3e} < {floor:.0e}): pick other seeds'


@pytest.mark.parametrize('name,mode', sc.CASES)
def test_the_oracle_run_excuses_nothing(name, mode):
    c = sc.case(name, mode)
    free, forced = c['free'], c['forced']
    assert free['labels'].shape == (c['L'], sc.B) and c['L'] == sc.FRAMES[name] * sc.DIM_SETS[name]['hop_length']
    _no_near_tie(free, mode, f'{name} {mode} free')
    _no_near_tie(forced, mode, f'{name} {mode} teacher-forced')
    np.testing.assert_array_equal(forced['labels'], free['labels'])
    assert np.unique(free['labels']).size >= 2
    if mode == 'RAW':
        assert free['labels'].max() < sc.n_classes(name, mode)
        np.testing.assert_array_equal(free['samples'], 2.0 * free['labels'].astype(np.float32) / np.float32(sc.n_classes(name, mode) - 1.0) - np.float32(1.0))
    if name == 'S4':
        assert free['labels'].max() >= 1024, 'S4: no winning class past 1024: change the noise seed'


@pytest.mark.parametrize('name,mode', sc.CASES)
def test_the_logit_bound_comes_from_the_reference_side(name, mode):
    """2e-5 * max(1, max |logit|) unless the fp32 oracle is itself more than an eighth of that from float64; below 1e-3 of the logit range."""
    bound, g = sc.logit_bound(name, mode)
    lg = sc.case(name, mode)['forced']['logits']
    print(f'\n[simple dims] {name} {mode}: g = max |oracle fp32 - float64| = {g:.3e}, bound {bound:.3e}, logit range {float(lg.max() - lg.min()):.3e}')
    assert np.isfinite(sc.float64_logits(name, mode)).all()
    moves = float(np.ptp(lg, axis=0).max()) > 0.0                                # the logits depend on the step: the loop's layers reach them
    assert moves == (name != 'S3'), 'S3 under weight seed 7 has both ReLUs dead (logits = fc3 bias); S3b is the same dims with live ones'
    assert bound < 1e-3 * float(lg.max() - lg.min())


@pytest.mark.parametrize('name', ['S3', 'S5'])
def test_the_conditioning_bounds_come_from_the_reference_side(name):
    (b_up, g_up), (b_aux, g_aux) = sc.conditioning_bounds(name, 'RAW')
    c = sc.case(name, 'RAW')
    d = sc.DIM_SETS[name]
    assert c['cm'].shape == (sc.B, c['L'], d['feat_dims']) and c['ca'].shape == (sc.B, c['L'], d['res_out_dims'])
    print(f'\n[simple dims] {name} conditioning: g_up {g_up:.3e} (bound {b_up:.3e}), g_aux {g_aux:.3e} (bound {b_aux:.3e}), '
          f'max |up| {float(np.abs(c["cm"]).max()):.3e}, max |aux| {float(np.abs(c["ca"]).max()):.3e}')
    assert b_up < 1e-3 * float(np.abs(c['cm']).max()) and b_aux < 1e-3 * float(np.abs(c['ca']).max())


def test_the_lds_need_of_every_set():
    need = {n: sc.simple_lay_bytes(d) for n, d in sc.DIM_SETS.items()}
    assert need['S4'] == 132992 and 65536 < need['S4'] <= sc.LDS_LIMIT
    assert sc.simple_lay_bytes(dict(sc.DIM_SETS['S4'], bits=16)) > sc.LDS_LIMIT
    assert all(b <= sc.LDS_LIMIT for b in need.values())
    assert all(need[n] <= 65536 for n in ('S1', 'S2', 'S3', 'S5'))            # S4 alone launches above 64 KB
    assert all(sc.simple_lay_bytes(d, 'MOL') <= 65536 for d in sc.DIM_SETS.values())


def test_the_sets_reach_what_they_are_for():
    threads = 512
    two = lambda n: max(n - threads, 0)                                      # threads that own a second unit / row / class
    d = sc.DIM_SETS
    assert (two(d['S1']['rnn_dims']), two(d['S1']['fc_dims'])) == (8, 8) and d['S1']['res_out_dims'] // 4 == 5 and sc.n_classes('S1', 'RAW') < threads
    assert (two(d['S2']['rnn_dims']), two(d['S2']['fc_dims']), two(sc.n_classes('S2', 'RAW'))) == (512, 512, 512)
    assert d['S3']['res_out_dims'] > d['S3']['compute_dims'] and 2 * d['S3']['pad'] + 1 == 3 and sc.n_classes('S3', 'RAW') == 2
    assert sc.n_classes('S4', 'RAW') == 32768
    assert two(d['S5']['rnn_dims']) == 488 and two(d['S5']['fc_dims']) == 88 and 2 * d['S5']['pad'] + 1 == 7 and d['S5']['res_out_dims'] // 4 == 18
    for n, s in d.items():
        assert int(np.prod(s['upsample_factors'])) == s['hop_length'], n
    for c1, c2 in sc.TIE_PAIRS:
        assert c1 < c2 < sc.n_classes('S2', 'RAW')
    (a1, a2), (b1, b2), (c1, c2) = sc.TIE_PAIRS
    assert a1 % threads == a2 % threads                                       # one thread meets both
    assert b1 % threads // 64 != b2 % threads // 64 and b1 < threads and b2 < threads
    assert c2 % threads // 64 < c1 % threads // 64 and c2 % threads % 64 < c1 % threads % 64


@pytest.mark.parametrize('name,mode', sc.PHILOX_CASES)
def test_the_replayed_philox_runs_excuse_nothing(name, mode):
    c = sc.philox_case(name, mode)
    assert sc.PHILOX_SEED & 0xFFFFFFFF and sc.PHILOX_SEED >> 32
    _no_near_tie(c['free'], mode, f'{name} {mode} Philox')
    assert np.unique(c['free']['labels']).size >= 2
    if name == 'S4':
        assert c['free']['labels'].max() >= 1024


def test_the_ragged_rows_excuse_nothing():
    r = sc.ragged_case()
    for b, (t, ref) in enumerate(zip(sc.RAGGED_FRAMES, r['refs'])):
        assert ref['free']['labels'].shape == (t * r['hop'], 1)
        _no_near_tie(ref['free'], 'RAW', f'ragged row {b}')
        assert not r['mels'][b, :, t:].any()


def test_the_folds_excuse_nothing():
    f = sc.fold_case()
    stride, total = sc.FOLD_TARGET + sc.FOLD_OVERLAP, sc.FOLD_FRAMES[0] * f['hop']
    assert stride % f['hop'] != 0
    assert f['fold0'] == [0, 5, 7] and f['steps'] == 64
    assert (f['fold0'][1] - 1) * stride + f['steps'] > total                   # the last fold of clip 0 runs into the zero padding
    for b, ref in enumerate(f['refs']):
        assert ref['free']['labels'].shape == (64, f['fold0'][b + 1] - f['fold0'][b])
        _no_near_tie(ref['free'], 'RAW', f'folds of clip {b}')


@pytest.mark.parametrize('c1,c2', sc.TIE_PAIRS)
def test_the_oracle_breaks_an_exact_tie_towards_the_first_index(c1, c2):
    from oracle import oracle as orc
    om = sc.oracle_of(sc.tie_state_dict(c1, c2), 'S2', 'RAW')
    cm, ca = om.conditioning(sc.mels_of('S2', T=sc.TIE_FRAMES))
    ref = om.loop(cm, ca, orc.NOISE_ARGMAX, want_logits=True)
    lg = ref['logits']
    np.testing.assert_array_equal(lg[:, :, c1], lg[:, :, c2])                 # an exact tie, at every step
    rest = np.delete(lg, [c1, c2], axis=2).max(axis=2)
    assert (lg[:, :, c1] > rest + 1.0).all()                                  # and the pair is far ahead of every other class
    assert (ref['labels'] == c1).all()                                        # strict `>`: the first index wins


def test_the_stream_buffers_follow_the_largest_push():
    for name, rows in (('S1', 1), ('S1', 3), ('S5', 1), ('S5', 3)):
        ws = sc.stream_buffer_bytes(sc.DIM_SETS[name], rows, sc.STREAM_CHUNKS)
        assert len(ws) == len(sc.STREAM_CHUNKS) + 1 and ws == sorted(ws) and ws[-1] == ws[-2] and ws[0] > 0
        d = sc.DIM_SETS[name]
        big = max(sc.STREAM_CHUNKS) + 2 * d['pad'] + 2                         # frames the largest push can span, with its context
        assert ws[-1] <= 4 * rows * big * (3 * d['feat_dims'] + d['res_out_dims'])
