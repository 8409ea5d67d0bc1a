"""The spectral scores on the GPU (``csrc/score.hip``) against the float64 restatement ``tests/score_ref.py``.

Tolerance, the rule of ``tests/test_gpu_mel.py``: for every input and every per-frame quantity q the test evaluates the restatement in
float32 as well and takes g = max_t |q32 - q64|; the kernel passes with max_t |kernel - q64| <= 8 g, and 8 g <= 1e-3 max_t |q64| is
asserted so that an ill-conditioned input cannot hide a failure.  Every parity test prints g, the kernel's error and their ratio before
it asserts (``pytest -s``).  Measured on an MI355X: 0.01 - 0.95 g on the STFT quantities (the kernel transforms in float64 and rounds
re^2 + im^2 once; a float32 transform reached 13.2 g on ``lm`` at n_fft 2048 for the white-noise pair, where ``ln`` of a bin a thousand
times under the frame's RMS amplifies the transform's error), 0.25 - 1.43 g on the mel distances (the float32 mel of ``melspec.hip``).

The summaries are checked against the float64 formulas applied to the kernel's own per-frame float32 values, within 1e-12 relative:
only the order of a float64 sum differs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mel_ref as mr
from tests import score_ref as sr
from tests import taco_mel_ref as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the smallest and the largest n_fft, and a window with an odd remainder
RES = ((256, 64, 256), (1024, 100, 601), (2048, 240, 1200))
LENGTHS = (1025, 6000, 22050)   # the shortest legal clip; no multiple of any hop; 345 frames at hop 64, several reduction chunks
HOP = 275


def _scorer(**kw):
    from tacotronv2_wavernn_chinese_amd.frontend import SpectralScore
    return SpectralScore(**dict(dict(resolutions=RES), **kw))


@pytest.fixture(scope='module')
def scorer():
    return _scorer()


@pytest.fixture(scope='module')
def refs():
    """(pair name, n) -> (a, b, score64, score32), computed once."""
    out = {}
    for name in sr.PAIR_NAMES:
        for n in LENGTHS:
            a, b = sr.parity_pair(name, n)
            out[name, n] = (a, b, sr.score(a, b, RES), sr.score(a, b, RES, dtype=np.float32))
    return out


def _check_quantities(tag, got, s64, s32, names=None):
    q64, q32, qk = sr.per_frame_quantities(s64), sr.per_frame_quantities(s32), sr.per_frame_quantities(got)
    bad = []
    for name in names or q64:
        r64 = np.asarray(q64[name], np.float64)
        g = float(np.abs(np.asarray(q32[name], np.float64) - r64).max())
        peak = float(np.abs(r64).max())
        assert qk[name].dtype == np.float32 and qk[name].shape == r64.shape, (tag, name)
        err = float(np.abs(qk[name].astype(np.float64) - r64).max())
        print(f'score parity {tag} {name}: frames {r64.size}, g = {g:.3e} = {g / peak:.2e} of max |q|, kernel error = {err:.3e} = '
              f'{err / g:.2f} g, bound 8 g = {8 * g:.3e}')
        assert 0 < 8 * g <= 1e-3 * peak, (tag, name, g, peak)
        if not err <= 8 * g:
            bad.append((name, err, g))
    assert not bad, (tag, bad)


def _check_summaries(got, resolutions=RES):
    """Every summary against the float64 formula on the kernel's own per-frame values."""
    want = sr.summarise(got['lsd'], got['mcd'], got['stft'], resolutions)
    for k in ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag'):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    for g, w in zip(got['stft'], want['stft']):
        assert (g['n_fft'], g['hop'], g['win'], g['frames']) == (w['n_fft'], w['hop'], w['win'], w['frames'])
        for k in ('sc', 'logmag'):
            assert abs(g[k] - w[k]) <= 1e-12 * abs(w[k]), (k, g[k], w[k])


@pytest.mark.parametrize('n', LENGTHS)
@pytest.mark.parametrize('name', sr.PAIR_NAMES)
def test_parity_of_every_per_frame_quantity(scorer, refs, name, n):
    a, b, s64, s32 = refs[name, n]
    got = scorer.score(a, b, per_frame=True)[0]
    assert got['n'] == n and [r['frames'] for r in got['stft']] == [1 + n // h for _, h, _ in RES] and got['lsd'].shape == (1 + n // HOP,)
    _check_quantities(f'{name}/{n}', got, s64, s32)
    _check_summaries(got)
    assert all(np.isfinite(got[k]) and got[k] > 0 for k in ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag'))


@pytest.mark.parametrize('features', ['vocoder', 'tacotron'])
@pytest.mark.parametrize('order', [13, 39])
def test_parity_of_the_mel_scores_at_40_mels(features, order):
    a, b = sr.parity_pair('scaled', 6000)
    cfg, f = dict(n_mels=40), (None if features == 'vocoder' else tm.TACOTRON)
    s64 = sr.score(a, b, RES[:1], cfg=cfg, features=f, mcd_order=order)
    s32 = sr.score(a, b, RES[:1], cfg=cfg, features=f, mcd_order=order, dtype=np.float32)
    got = _scorer(resolutions=RES[:1], features=features, n_mels=40, mcd_order=order).score(a, b, per_frame=True)[0]
    _check_quantities(f'{features}/K={order}', got, s64, s32, names=('lsd', 'mcd'))
    _check_summaries(got, RES[:1])


def _assert_all_zero(s, floor_den=None):
    for k in ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag'):
        assert s[k] == 0.0, (k, s[k])
    assert not s['lsd'].any() and not s['mcd'].any()
    for r in s['stft']:
        assert r['sc'] == 0.0 and r['logmag'] == 0.0
        assert not r['num'].any() and not r['lm'].any()
        assert (r['den'] > 0).all()
        if floor_den is not None:   # both sides sit at the floor: den_t = bins * floor up to the rounding of the sum
            np.testing.assert_allclose(r['den'], (r['n_fft'] // 2 + 1) * floor_den, rtol=1e-5)


def test_identical_clips_and_two_silences_score_exactly_zero(scorer):
    a = sr.parity_pair('scaled', 6000)[0]
    _assert_all_zero(scorer.score(a, a.copy(), per_frame=True)[0])
    z = np.zeros(4321, np.float32)
    _assert_all_zero(scorer.score(z, z.copy(), per_frame=True)[0], floor_den=1e-7)


def _bits(s):
    out = [np.asarray([s[k] for k in ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag')] + [r[k] for r in s['stft'] for k in ('sc', 'logmag')]).view(np.uint64)]
    out += [v.view(np.uint32) for v in sr.per_frame_quantities(s).values()]
    return out


def _assert_bit_equal(x, y):
    assert x['n'] == y['n']
    for u, v in zip(_bits(x), _bits(y)):
        np.testing.assert_array_equal(u, v)


def test_a_second_call_and_device_tensors_give_the_same_bits(scorer):
    a, b = sr.parity_pair('noise', 6000)
    first = scorer.score(a, b, per_frame=True)[0]
    _assert_bit_equal(first, scorer.score(a, b, per_frame=True)[0])
    _assert_bit_equal(first, scorer.score(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), per_frame=True)[0])
    # without the caller's per-frame buffer the values go through the handle's scratch: the summaries are the same bits
    plain = scorer.score(a, b)[0]
    assert 'lsd' not in plain and all(plain[k] == first[k] for k in ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag'))
    # the test clip is cut to the target's length
    assert scorer.score(a, np.concatenate([b, b[:100]]))[0] == plain


def test_ragged_batch_is_bit_equal_to_the_solo_calls(scorer):
    lens = (1025, 6000, 4321)
    pairs = [sr.parity_pair(name, n) for name, n in zip(sr.PAIR_NAMES, lens)]
    batch = scorer.score([p[0] for p in pairs], [p[1] for p in pairs], per_frame=True)
    raw, layout = scorer.last_frames_buffer, scorer.last_layout
    assert raw.shape[0] == 3 and [s['n'] for s in batch] == list(lens)
    for i, (a, b) in enumerate(pairs):
        _assert_bit_equal(batch[i], scorer.score(a, b, per_frame=True)[0])
        for name, r, off, t_max in layout:                      # exactly 0 past the clip's own frames, in every segment of the row
            t = scorer.frames(r, lens[i])
            assert t_max == scorer.frames(r, max(lens)) and not raw[i, off + t:off + t_max].any()
            assert raw[i, off:off + t].any()


def test_error_paths_start_no_launch(monkeypatch):
    from tacotronv2_wavernn_chinese_amd import _cabi
    launches = []
    real = _cabi.NativeScore.score
    monkeypatch.setattr(_cabi.NativeScore, 'score', lambda self, *a: (launches.append(a), real(self, *a))[1])
    sc = _scorer()
    ok = mr.white(3000, 0.1)
    with pytest.raises(ValueError):
        sc.score(ok, np.zeros(1024, np.float32))                  # the pair is cut to 1024 samples: too short to pad
    with pytest.raises(ValueError):
        sc.score([ok, ok], [ok])
    with pytest.raises(ValueError):
        sc.score(ok, ok, device='cpu')
    assert not launches
    sc.score(ok, ok)
    assert len(launches) == 1


@pytest.fixture(scope='module')
def model():
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    sd = make_state_dict(0, variant='peaky')
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to('cuda:0')


def test_two_vocodings_of_one_mel_score_like_the_restatement(model, scorer):
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    mels = make_mels(7, 1, 20)
    x, y = (model.generate_raw(mels, False, 11000, 550, seed=s, kernel='team2')['samples'][0] for s in (1, 2))
    assert x.is_cuda and x.shape == (20 * HOP,) and not torch.equal(x, y)
    got = scorer.score(x, y, per_frame=True)[0]
    assert all(np.isfinite(got[k]) and got[k] > 0 for k in ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag'))
    a, b = x.cpu().numpy(), y.cpu().numpy()
    _check_quantities('vocoded', got, sr.score(a, b, RES), sr.score(a, b, RES, dtype=np.float32))
    _check_summaries(got)


def test_cli_prints_the_numbers_of_the_class(tmp_path):
    from tacotronv2_wavernn_chinese_amd.dsp import save_wav
    from tacotronv2_wavernn_chinese_amd.frontend import SpectralScore
    a, b = sr.parity_pair('scaled', 6000)
    save_wav(a, tmp_path / 'a.wav', 22050)
    save_wav(b, tmp_path / 'b.wav', 22050)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_score.py'), '--target', str(tmp_path / 'a.wav'), '--test', str(tmp_path / 'b.wav'),
                        '--json', '--per_frame', str(tmp_path / 'f.npz')], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    from tacotronv2_wavernn_chinese_amd.frontend import read_wav
    want = SpectralScore().score(read_wav(tmp_path / 'a.wav')[0], read_wav(tmp_path / 'b.wav')[0], per_frame=True)[0]
    assert len(out['pairs']) == 1 and out['pairs'][0]['name'] == 'b' and out['pairs'][0]['n'] == 6000
    for k in ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag'):
        assert out['pairs'][0][k] == want[k] == out['mean'][k]
    assert [(s['n_fft'], s['sc'], s['logmag']) for s in out['pairs'][0]['stft']] == [(s['n_fft'], s['sc'], s['logmag']) for s in want['stft']]
    with np.load(tmp_path / 'f.npz') as z:
        np.testing.assert_array_equal(z['b/lsd'], want['lsd'])
        np.testing.assert_array_equal(z['b/lm_2048_240_1200'], want['stft'][2]['lm'])


def test_training_checkpoint_writes_one_finite_score_row_per_generated_clip(model, tmp_path):
    """``wavernn_train.py --score_at_checkpoint`` hands ``train.checkpoint_generator`` a scorer; the hook is called directly here, as the
    loop calls it at a checkpoint (a run of the command line costs a process start and a thousand steps)."""
    from types import SimpleNamespace
    from tacotronv2_wavernn_chinese_amd import train as T
    from tacotronv2_wavernn_chinese_amd.frontend import SpectralScore
    hp = SimpleNamespace(voc_target=11000, voc_overlap=550, voc_gen_batched=False, voc_gen_at_checkpoint=2, voc_mode='RAW', bits=10, mu_law=True,
                         sample_rate=22050)
    paths = T.VocPaths(tmp_path)
    test_set = T.synthetic_pairs(3, 21, bits=10, n_mels=80, hop_length=HOP, seed=1)
    T.checkpoint_generator(hp, paths, None)(model, test_set, 1000)
    assert not (paths.voc_checkpoints / 'scores.txt').exists()               # off by default: the files of before and nothing else
    assert len(list(paths.voc_output.glob('1k_steps_*_target.wav'))) == 2
    hook = T.checkpoint_generator(hp, paths, SpectralScore())
    hook(model, test_set, 1000)
    hook(model, test_set, 2000)
    rows = [l.split() for l in (paths.voc_checkpoints / 'scores.txt').read_text().splitlines()]
    assert [(r[0], r[1]) for r in rows] == [('1000', '1'), ('1000', '2'), ('2000', '1'), ('2000', '2')]
    vals = np.array([[float(v) for v in r[2:]] for r in rows])
    assert vals.shape == (4, 4) and np.isfinite(vals).all() and (vals > 0).all()
    assert T.build_parser().parse_args(['--synthetic', '4', '--score_at_checkpoint']).score_at_checkpoint
    assert not T.build_parser().parse_args(['--synthetic', '4']).score_at_checkpoint
