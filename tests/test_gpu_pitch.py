"""The YIN track and the pair scores on the GPU (``csrc/pitch.hip``) against the float64 restatement ``tests/pitch_ref.py``.

What is compared, on every frame of every fixture (``tests/test_pitch_host.py`` asserts the margins that make equal decisions a fair
demand, so no frame is excused):
  * voiced flags, and the integer lag recovered as ``round(sr / f0)`` where the restatement's ``|off| < 0.49``: equal;
  * ``f0``: within one float32 spacing of the restatement's float64 value (the one spacing is for double rounding);
  * aperiodicity: within ``2^-23 max(1, ref)``.
Both value bounds are the float32 output format's; the float64 disagreement (another summation order) is orders of magnitude below.
The summaries are recomputed in float64 from the kernel's own float32 tracks and agree within 1e-12 relative; counts, and the first
four fields of identical pairs, exactly.  Every parity test prints its figures before it asserts (``pytest -s``).  Measured on an
MI355X over the eight configurations: ``f0`` 0.35 - 0.50 spacings (correctly rounded), aperiodicity 0.23 - 0.43 of its bound."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pitch_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = pr.N


def _settings(config):
    return dict(pr.DEFAULTS, **pr.CONFIGS[config])


def _native(config):
    from tacotronv2_wavernn_chinese_amd import _cabi
    return _cabi.NativePitch(_cabi.PitchConfig(**_settings(config)))


def _rows(clips, n_max):
    host = np.zeros((len(clips), n_max), np.float32)
    for i, c in enumerate(clips):
        host[i, :min(len(c), n_max)] = c[:n_max]
    return torch.from_numpy(host).cuda()


def device_track(nat, clips, n_max=None, n_dev=None, with_ap=True):
    """One ``wrnn_pitch_track`` call on a ragged batch -> the raw (B, F) rows of f0 and aperiodicity."""
    n_max = n_max or max(max(len(c) for c in clips), 1)
    wav = _rows(clips, n_max)
    lens = torch.tensor(n_dev if n_dev is not None else [len(c) for c in clips], dtype=torch.int32).cuda()
    F = nat.frames(n_max)
    out = torch.full((2, len(clips), F), -7.0, dtype=torch.float32, device='cuda')
    nat.track(wav.data_ptr(), n_max, lens.data_ptr(), len(clips), out[0].data_ptr(), out[1].data_ptr() if with_ap else 0, F,
              torch.cuda.current_stream().cuda_stream)
    out = out.cpu().numpy()
    return out[0], out[1]


def device_score(nat, targets, tests, n_max=None, n_dev=None, per_frame=True):
    n_max = n_max or max(max(len(c) for c in targets), 1)
    wa, wb = _rows(targets, n_max), _rows(tests, n_max)
    lens = torch.tensor(n_dev if n_dev is not None else [len(c) for c in targets], dtype=torch.int32).cuda()
    B, F = len(targets), nat.frames(n_max)
    summary = torch.full((B, 8), -7.0, dtype=torch.float64, device='cuda')
    frames = torch.full((B, 5 * F), -7.0, dtype=torch.float32, device='cuda') if per_frame else None
    nat.score(wa.data_ptr(), wb.data_ptr(), n_max, lens.data_ptr(), B, summary.data_ptr(), frames.data_ptr() if per_frame else 0, 5 * F,
              torch.cuda.current_stream().cuda_stream)
    return summary.cpu().numpy(), (frames.cpu().numpy().reshape(B, 5, F) if per_frame else None)


def check_track(tag, ref, f0, ap):
    """One clip's device rows (F entries, zeros past the clip's own frames) against the restatement's track."""
    s = ref['settings']
    T = len(ref['f0'])
    assert not f0[T:].any() and not ap[T:].any(), f'{tag}: entries past the clip\'s own {T} frames are not 0'
    f0, ap = f0[:T], ap[:T]
    if T == 0:
        return 0.0, 0.0
    voiced = f0 > 0
    assert np.array_equal(voiced, ref['voiced']), f'{tag}: voiced flags differ at frames {np.flatnonzero(voiced != ref["voiced"])}'
    lag = voiced & (np.abs(ref['off']) < 0.49)
    got_tau = np.round(s['sample_rate'] / f0[lag].astype(np.float64)).astype(int)
    assert np.array_equal(got_tau, ref['tau'][lag]), f'{tag}: integer lags differ'
    spacing = np.spacing(np.abs(ref['f0_64']).astype(np.float32)).astype(np.float64)
    e_f0 = np.abs(f0.astype(np.float64) - ref['f0_64']) / spacing
    e_ap = np.abs(ap.astype(np.float64) - ref['aperiodicity_64']) / (2.0 ** -23 * np.maximum(1.0, ref['aperiodicity_64']))
    return float(e_f0.max()), float(e_ap.max())


@pytest.mark.parametrize('config', list(pr.CONFIGS))
def test_tracks_equal_the_restatement_on_every_frame(config):
    """All the fixtures of one configuration as one ragged batch."""
    cases = [c for c in pr.CASES if c[0] == config]
    s = _settings(config)
    clips = [pr.signal(name, n, s['sample_rate']) for _, name, n in cases]
    nat = _native(config)
    assert (nat.tau_min, nat.tau_max) == pr.lags(s['sample_rate'], s['fmin'], s['fmax'])
    f0, ap = device_track(nat, clips)
    worst = [0.0, 0.0]
    for i, (_, name, n) in enumerate(cases):
        e = check_track(f'{config}/{name}/{n}', pr.case_track(config, name, n), f0[i], ap[i])
        worst = [max(a, b) for a, b in zip(worst, e)]
    print(f'{config}: lags {nat.tau_min} .. {nat.tau_max}, {len(cases)} clips, f0 error {worst[0]:.3f} float32 spacings, '
          f'aperiodicity error {worst[1]:.3f} x 2^-23 max(1, ref)')
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_batch_equals_each_clip_alone_and_a_second_call_bit_for_bit():
    names = [('sine_233.3', N), ('chirp', 2049), ('noise', N), ('chirp', 1), ('stop_3100', N), ('chirp', 276)]
    clips = [pr.signal(name, n) for name, n in names]
    nat = _native('default')
    f0, ap = device_track(nat, clips)
    f0_2, ap_2 = device_track(nat, clips)
    assert f0.tobytes() == f0_2.tobytes() and ap.tobytes() == ap_2.tobytes()
    for i, c in enumerate(clips):
        a_f0, a_ap = device_track(nat, [c])          # B = 1, n_max the clip's own length
        T = nat.frames(len(c))
        assert a_f0.shape == (1, T)
        assert a_f0[0].tobytes() == f0[i, :T].tobytes() and a_ap[0].tobytes() == ap[i, :T].tobytes(), names[i]
    # the same clips in another order and another grid: a clip's place in the batch changes nothing
    r_f0, r_ap = device_track(nat, clips[::-1] + clips[:2])
    assert r_f0[:6][::-1].tobytes() == f0.tobytes() and r_ap[:6][::-1].tobytes() == ap.tobytes()
    # aperiodicity_dev is optional
    o_f0, o_ap = device_track(nat, clips, with_ap=False)
    assert o_f0.tobytes() == f0.tobytes() and (o_ap == -7.0).all()


def test_ragged_batch_with_a_length_at_above_and_of_zero():
    """B = 5: one length equal to n_max, one above it (read as n_max), one empty clip, one sample, and one in between."""
    nat = _native('default')
    chirp, sine = pr.signal('chirp', N), pr.signal('sine_220.5', N)
    clips = [chirp, sine, chirp, chirp[:1], sine[:2049]]
    f0, ap = device_track(nat, clips, n_max=N, n_dev=[N, N + 500, 0, 1, 2049])
    for i, case in enumerate([('chirp', N), ('sine_220.5', N), None, ('chirp', 1), ('sine_220.5', 2049)]):
        if case is None:
            assert not f0[i].any() and not ap[i].any()
        else:
            assert max(check_track(f'row {i}', pr.case_track('default', *case), f0[i], ap[i])) <= 1.0
    # an empty clip alone, and a negative length, have no frames either
    z_f0, z_ap = device_track(nat, [chirp[:5]], n_max=5, n_dev=[0])
    assert z_f0.shape == (1, 1) and not z_f0.any() and not z_ap.any()
    z_f0, _ = device_track(nat, [chirp[:5]], n_max=5, n_dev=[-3])
    assert not z_f0.any()


def _check_summary(tag, got, ft, fs, gpe_ratio=0.2):
    """A summary row against the float64 formulas on the kernel's own float32 tracks."""
    want = pr.pair_scores(ft, fs, gpe_ratio)
    assert want['m_gpe'] >= 1e-6, f'{tag}: a frame sits on the gross-error bound'
    for i, k in enumerate(pr.FIELDS):
        if i >= 5:
            assert got[i] == want[k], (tag, k, got[i], want[k])
        else:
            assert abs(got[i] - want[k]) <= 1e-12 * abs(want[k]), (tag, k, got[i], want[k])
    return want


def test_pair_scores():
    nat = _native('default')
    targets = [pr.signal(a, N) for a, _ in pr.PAIRS]
    tests = [pr.signal(b, N) for _, b in pr.PAIRS]
    summary, frames = device_score(nat, targets, tests)
    F = nat.frames(N)
    worst = [0.0, 0.0]
    by_name = {}
    for i, (a, b) in enumerate(pr.PAIRS):
        ra, rb = pr.case_track('default', a, N), pr.case_track('default', b, N)
        e = check_track(f'{a} (target)', ra, frames[i, 0], frames[i, 1]) + check_track(f'{b} (test)', rb, frames[i, 2], frames[i, 3])
        worst = [max(worst[0], e[0], e[2]), max(worst[1], e[1], e[3])]
        want = _check_summary(f'{a} / {b}', summary[i], frames[i, 0], frames[i, 2])
        cents64 = want['cents']     # the per-frame cents: float32 of the same float64 expression, one spacing for double rounding
        assert (np.abs(frames[i, 4].astype(np.float64) - cents64) <= np.spacing(np.abs(cents64).astype(np.float32)).astype(np.float64)).all()
        # the restatement's own tracks give the same counts (equal decisions) and nearly the same values
        ref = pr.pair_scores(ra['f0'], rb['f0'])
        assert [summary[i, j] for j in (5, 6, 7)] == [ref[k] for k in pr.FIELDS[5:]]
        assert summary[i, 2] == ref['vde'] and summary[i, 3] == ref['ffe'] and summary[i, 1] == ref['gpe']
        by_name[a, b] = dict(zip(pr.FIELDS, summary[i]))
        print(f'{a} / {b}: ' + ', '.join(f'{k} {v:.6g}' for k, v in by_name[a, b].items()))
    print(f'tracks of the pairs: f0 error {worst[0]:.3f} spacings, aperiodicity error {worst[1]:.3f} x 2^-23 max(1, ref)')
    assert max(worst) <= 1.0
    # identical clips and two silences: exactly 0 on the first four fields; the correlation as the restatement gives it
    for pair, corr in ((('chirp', 'chirp'), 1.0), (('sine_220.5', 'sine_220.5'), None), (('zeros', 'zeros'), 0.0), (('noise', 'noise'), 0.0)):
        s = by_name[pair]
        assert s['f0_rmse_cents'] == s['gpe'] == s['vde'] == s['ffe'] == 0.0, pair
        ref = pr.pair_scores(pr.case_track('default', pair[0], N)['f0'], pr.case_track('default', pair[1], N)['f0'])
        assert abs(s['f0_corr'] - ref['f0_corr']) <= 1e-12 and (corr is None or ref['f0_corr'] == pytest.approx(corr, abs=1e-12)), pair
    detuned = by_name['chirp', 'chirp_x%r' % (2 ** (10 / 1200))]
    assert abs(detuned['f0_rmse_cents'] - 10.0) < 0.5 and detuned['gpe'] == 0.0 and detuned['voiced_both'] >= 2
    gross = by_name['chirp', 'chirp_x1.3']
    assert gross['gpe'] == 1.0 and gross['vde'] == 0.0 and gross['ffe'] == gross['voiced_both'] / F      # all gross errors
    vs_noise = by_name['chirp', 'noise']
    assert vs_noise['voiced_test'] == 0 and vs_noise['vde'] == vs_noise['voiced_target'] / F > 0.5      # the target's voiced share
    assert vs_noise['f0_rmse_cents'] == vs_noise['gpe'] == vs_noise['f0_corr'] == 0.0                  # V is empty
    switch = by_name['chirpstop_3100', 'chirpstop_4200']
    assert switch['vde'] == (switch['voiced_test'] - switch['voiced_target']) / F > 0 and switch['voiced_both'] == switch['voiced_target'] >= 2
    assert by_name['noise', 'zeros']['voiced_both'] == 0 and not any(by_name['noise', 'zeros'].values())
    # without frames_dev the per-frame values go to the handle's scratch: the same summaries, bit for bit, and again on a second call
    for _ in range(2):
        s2, none = device_score(nat, targets, tests, per_frame=False)
        assert none is None and s2.tobytes() == summary.tobytes()
    # a pair of the batch alone (B = 1, the scratch already large enough), and a ragged batch with an empty pair and a clamped length
    s1, f1 = device_score(nat, targets[4:5], tests[4:5])
    assert s1[0].tobytes() == summary[4].tobytes() and f1[0].tobytes() == frames[4].tobytes()
    pick = [0, 1, 4]
    sr_, fr_ = device_score(nat, [targets[i] for i in pick], [tests[i] for i in pick], n_max=N, n_dev=[N + 1, 0, 2049])
    assert sr_[0].tobytes() == summary[0].tobytes() and not sr_[1].any() and not fr_[1].any()
    short, fs_ = device_score(nat, [targets[4][:2049]], [tests[4][:2049]])
    T = fs_.shape[2]
    assert short[0, 7] >= 2 and sr_[2].tobytes() == short[0].tobytes()
    assert fr_[2][:, :T].tobytes() == fs_[0].tobytes() and not fr_[2][:, T:].any()


def test_pair_scores_at_another_gross_error_bound_and_rate():
    from tacotronv2_wavernn_chinese_amd import _cabi
    s = dict(_settings('sr16k'), gpe_ratio=0.004)       # 10 cents are 0.58 %: every frame of V is a gross error at this bound
    nat = _cabi.NativePitch(_cabi.PitchConfig(**s))
    a, b = pr.signal('chirp', N, 16000), pr.signal('chirp_x%r' % (2 ** (10 / 1200)), N, 16000)
    summary, frames = device_score(nat, [a], [b])
    want = _check_summary('sr16k detuned', summary[0], frames[0, 0], frames[0, 2], 0.004)
    assert want['gpe'] == 1.0 and summary[0, 7] >= 2


def test_python_wrappers():
    from tacotronv2_wavernn_chinese_amd.frontend import PitchScore, PitchTracker
    names = [('chirp', N), ('sine_233.3', N), ('zeros', N), ('chirp', 276), ('chirp', 1)]
    clips = [pr.signal(name, n) for name, n in names]
    tracker = PitchTracker()
    assert (tracker.tau_min, tracker.tau_max, tracker.hop, tracker.sample_rate) == (37, 367, 275, 22050)
    got = tracker.track(clips)
    assert len(got) == len(clips)
    for (name, n), (f0, ap) in zip(names, got):
        ref = pr.case_track('default', name, n)
        assert f0.dtype == ap.dtype == np.float32 and f0.shape == ap.shape == (tracker.frames(n),)
        assert max(check_track(name, ref, f0, ap)) <= 1.0
    # one clip as an array, a device tensor, a 2-D batch, an empty clip
    one = tracker.track(clips[0])
    assert len(one) == 1 and one[0][0].tobytes() == got[0][0].tobytes()
    dev = tracker.track(torch.from_numpy(np.stack(clips[:2])).cuda())
    assert dev[1][0].tobytes() == got[1][0].tobytes() and dev[0][1].tobytes() == got[0][1].tobytes()
    empty = tracker.track([clips[0][:0], clips[1]])
    assert empty[0][0].shape == (0,) and empty[1][0].tobytes() == got[1][0].tobytes()
    assert tracker.track(clips[0][:0])[0][0].shape == (0,)
    scorer = PitchScore()
    detune = pr.signal('chirp_x1.3', N)
    res = scorer.score([clips[0], clips[0], clips[1]], [clips[0], detune, clips[2][:3000]], per_frame=True)
    assert res[0]['f0_rmse_cents'] == res[0]['gpe'] == res[0]['vde'] == res[0]['ffe'] == 0.0 and res[0]['f0_corr'] == pytest.approx(1.0, abs=1e-12)
    assert res[1]['gpe'] == 1.0 and isinstance(res[1]['voiced_both'], int) and res[1]['voiced_both'] >= 2 and res[1]['n'] == N
    assert res[2]['n'] == 3000 and res[2]['frames'] == 11 == len(res[2]['cents']) and res[2]['voiced_test'] == 0 and res[2]['vde'] > 0.5
    for r in res:
        want = pr.pair_scores(r['f0_target'], r['f0_test'])
        for k in pr.FIELDS:
            assert abs(r[k] - want[k]) <= 1e-12 * abs(want[k]), k
    plain = scorer.score(clips[0], detune)
    assert set(plain[0]) == set(pr.FIELDS) | {'n', 'frames'} and plain[0]['f0_rmse_cents'] == res[1]['f0_rmse_cents']
    hp = type('hp', (), dict(sample_rate=16000, hop_length=256))
    t16 = PitchTracker(hp, frame_length=1024, window=512, fmin=80)
    assert (t16.sample_rate, t16.hop, t16.tau_max) == (16000, 256, 200)
    f0, ap = t16.track(pr.signal('chirp', N, 16000))[0]
    assert max(check_track('sr16k chirp', pr.case_track('sr16k', 'chirp', N), f0, ap)) <= 1.0


def test_cli_pitch_flag_adds_the_eight_keys_and_changes_nothing_without_it(tmp_path):
    from tacotronv2_wavernn_chinese_amd.dsp import save_wav
    from tacotronv2_wavernn_chinese_amd.frontend import PitchScore, SpectralScore, read_wav
    from tacotronv2_wavernn_chinese_amd import score as cli
    save_wav(pr.signal('chirp', N), tmp_path / 'a.wav', 22050)
    save_wav(pr.signal('chirp_x1.3', N), tmp_path / 'b.wav', 22050)
    base = [sys.executable, os.path.join(ROOT, 'wavernn_score.py'), '--target', str(tmp_path / 'a.wav'), '--test', str(tmp_path / 'b.wav')]
    runs = {}
    for tag, extra in (('json', ['--json']), ('json_pitch', ['--json', '--pitch', '--fmax', '500', '--per_frame', str(tmp_path / 'f.npz')])):
        r = subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[tag] = r.stdout
    plain, with_pitch = json.loads(runs['json'].strip().splitlines()[-1]), json.loads(runs['json_pitch'].strip().splitlines()[-1])
    a, b = read_wav(tmp_path / 'a.wav')[0], read_wav(tmp_path / 'b.wav')[0]
    # without the flag: the one line of before, byte for byte
    spectral = SpectralScore().score(a, b)[0]
    mean = {k: float(np.mean([spectral[k]])) for k in cli.SUMMARY_KEYS}
    assert runs['json'].strip().splitlines()[-1] == json.dumps(dict(pairs=[dict(spectral, name='b')], mean=mean))
    assert set(plain['mean']) == set(cli.SUMMARY_KEYS) and set(plain['pairs'][0]) == set(cli.SUMMARY_KEYS) | {'n', 'stft', 'name'}
    want = PitchScore(fmax=500.0).score(a, b, per_frame=True)[0]
    # the table: the lines of before, then (under --pitch alone) an empty line and the pitch table
    before = cli.table(['b'], [spectral], mean)
    assert before.count('\n') == 2 and 'f0_rmse_cents' not in before
    after = cli.table(['b'], [dict(spectral, **want)], dict(mean, **{k: want[k] for k in cli.PITCH_KEYS}), 275)
    assert after.startswith(before + '\n\n') and after.count('\n') == 6 and 'f0_rmse_cents' in after
    for k in cli.PITCH_KEYS:
        assert with_pitch['pairs'][0][k] == want[k] == with_pitch['mean'][k], k
    assert {k: v for k, v in with_pitch['pairs'][0].items() if k not in cli.PITCH_KEYS} == plain['pairs'][0]
    assert {k: with_pitch['mean'][k] for k in cli.SUMMARY_KEYS} == plain['mean']
    assert want['gpe'] == 1.0
    with np.load(tmp_path / 'f.npz') as z:
        np.testing.assert_array_equal(z['b/f0_test'], want['f0_test'])
        np.testing.assert_array_equal(z['b/cents'], want['cents'])
        assert 'b/lsd' in z


def test_training_checkpoint_appends_the_pitch_columns_only_when_asked(tmp_path):
    """``wavernn_train.py --score_at_checkpoint --score_pitch``: the hook is called directly, as the loop calls it at a checkpoint."""
    from types import SimpleNamespace
    from tacotronv2_wavernn_chinese_amd import train as T
    from tacotronv2_wavernn_chinese_amd.frontend import PitchScore, SpectralScore
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    model = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    model.verbose = False
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(0, variant='peaky').items()})
    model = model.to('cuda:0')
    hp = SimpleNamespace(voc_target=11000, voc_overlap=550, voc_gen_batched=False, voc_gen_at_checkpoint=1, voc_mode='RAW', bits=10, mu_law=True,
                         sample_rate=22050)
    paths = T.VocPaths(tmp_path)
    test_set = T.synthetic_pairs(2, 21, bits=10, n_mels=80, hop_length=275, seed=1)
    T.checkpoint_generator(hp, paths, SpectralScore())(model, test_set, 1000)             # without the flag: the six columns of before
    T.checkpoint_generator(hp, paths, SpectralScore(), PitchScore())(model, test_set, 2000)
    rows = [l.split() for l in (paths.voc_checkpoints / 'scores.txt').read_text().splitlines()]
    assert [(r[0], r[1], len(r)) for r in rows] == [('1000', '1', 6), ('2000', '1', 9)]
    f0_rmse, gpe, vde = (float(v) for v in rows[1][6:])
    assert np.isfinite([f0_rmse, gpe, vde]).all() and f0_rmse >= 0 and 0 <= gpe <= 1 and 0 <= vde <= 1
