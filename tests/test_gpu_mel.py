"""The mel front end on the GPU (``csrc/melspec.hip``) against the float64 restatement ``tests/mel_ref.py``.

Tolerance: the reference's own arithmetic is float32 (``librosa.stft`` returns complex64), so for every input the test evaluates the
restatement in float32 as well and takes g = max |mel_ref32 - mel_ref64|; the kernel passes with max |kernel - mel_ref64| <= 8 g (another,
equally float32, FFT factorisation and summation order), and 8 g <= 1e-5 (0.001 dB) is asserted so that an ill-conditioned input cannot
loosen the bound.  Every parity test prints g, the kernel's error and their ratio before it asserts (``pytest -s``).

Composition runs at 21 frames, the shortest clip ``generate`` accepts (the reference's fade-out raises ``ValueError`` below that, which the
10-frame clip is used to show)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mel_ref as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONDEFAULT = dict(mr.DEFAULT, win_length=800, hop_length=200, n_mels=40, fmin=0.0)
HOP = 275


def _inputs():
    gap = mr.speech_like(3000, 2)
    gap[1200:2600] = 0.0
    return {'speech_1025': mr.speech_like(1025, 0), 'speech_tail': mr.speech_like(HOP * 9 + 17, 1), 'speech_gap': gap,
            'noise_0.3': mr.white(3000, 0.3, 3), 'noise_1e-4': mr.white(2200, 1e-4, 4)}


@pytest.fixture(scope='module')
def cases():
    """name -> (clip, mel_ref64, g) at the default configuration, computed once."""
    out = {}
    for name, y in _inputs().items():
        r64 = mr.melspectrogram(y, **mr.DEFAULT)
        g = float(np.abs(mr.melspectrogram(y, **mr.DEFAULT, dtype=np.float32).astype(np.float64) - r64).max())
        out[name] = (y, r64, g)
    return out


def _fe(**cfg):
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    return MelFrontEnd(**cfg)


def _check(name, got, r64, g):
    err = float(np.abs(got.astype(np.float64) - r64).max())
    print(f'mel parity {name}: frames {r64.shape[1]}, g = {g:.3e}, kernel error = {err:.3e} = {err / g:.2f} g, bound 8 g = {8 * g:.3e}')
    assert 0 < 8 * g <= 1e-5, (name, g)
    assert got.shape == r64.shape and got.dtype == np.float32
    assert err <= 8 * g, (name, err, g)


@pytest.mark.parametrize('name', ['speech_1025', 'speech_tail', 'speech_gap', 'noise_0.3', 'noise_1e-4'])
def test_parity_each_clip_alone(cases, name):
    y, r64, g = cases[name]
    got = _fe().melspectrogram(y).cpu().numpy()
    assert got.shape[0] == 1
    _check(name, got[0], r64, g)
    assert (r64 > 0).mean() > 0.8 and (r64 < 1).mean() > 0.5      # the input exercises the open range, not the clip at 0 or 1
    if name == 'speech_gap':
        floor = np.flatnonzero((r64 == 0).all(axis=0))
        assert floor.size >= 1                                    # frames whose taps are all zero sit on the 1e-5 floor ...
        assert not got[0][:, floor].any()                         # ... and come out as exact zeros
    if name == 'speech_1025':
        assert r64.shape[1] == 4                                  # shortest legal clip: both reflect edges in every frame


def test_ragged_batch_rows_are_bit_equal_to_the_solo_calls(cases):
    fe = _fe()
    names = list(cases)
    clips = [cases[n][0] for n in names]
    batch = fe.melspectrogram(clips).cpu().numpy()
    frames = [cases[n][1].shape[1] for n in names]
    assert batch.shape == (5, 80, max(frames)) and fe.last_frames == frames and len(set(frames)) > 2
    for i, n in enumerate(names):
        solo = fe.melspectrogram(clips[i]).cpu().numpy()[0]
        np.testing.assert_array_equal(batch[i, :, :frames[i]].view(np.uint32), solo.view(np.uint32))
        assert not batch[i, :, frames[i]:].any()                  # exactly 0 past the clip's own end
        _check('ragged/' + n, batch[i, :, :frames[i]], cases[n][1], cases[n][2])


def test_device_clips_stay_on_the_device(cases):
    fe = _fe()
    y = cases['speech_tail'][0]
    a = fe.melspectrogram(torch.from_numpy(y).cuda())
    assert a.is_cuda and torch.equal(a, fe.melspectrogram(y))


def test_parity_nondefault_configuration():
    y = mr.speech_like(2 * 1025 + 77, 5)
    r64 = mr.melspectrogram(y, **NONDEFAULT)
    g = float(np.abs(mr.melspectrogram(y, **NONDEFAULT, dtype=np.float32).astype(np.float64) - r64).max())
    got = _fe(**NONDEFAULT).melspectrogram(y).cpu().numpy()[0]
    assert r64.shape == (40, 1 + y.size // 200)
    _check('nondefault', got, r64, g)
    lo = _fe(**dict(mr.DEFAULT, min_level_db=-80.0)).melspectrogram(y).cpu().numpy()[0]
    r = mr.melspectrogram(y, **dict(mr.DEFAULT, min_level_db=-80.0))
    _check('min_level_db=-80', lo, r, float(np.abs(mr.melspectrogram(y, **dict(mr.DEFAULT, min_level_db=-80.0), dtype=np.float32) - r).max()))


def test_error_paths_start_no_launch(monkeypatch):
    from tacotronv2_wavernn_chinese_amd import _cabi
    launches = []
    real = _cabi.NativeMel.melspectrogram
    monkeypatch.setattr(_cabi.NativeMel, 'melspectrogram', lambda self, *a: (launches.append(a), real(self, *a))[1])
    fe = _fe()
    with pytest.raises(ValueError):
        fe.melspectrogram(np.zeros(1024, np.float32))
    with pytest.raises(ValueError):
        fe.melspectrogram([mr.white(3000, 0.1), np.zeros(1024, np.float32)])
    with pytest.raises(ValueError):
        _fe(n_fft=1024)
    assert not launches
    fe.melspectrogram(mr.white(1025, 0.1))
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


def test_generate_from_wav_is_generate_on_the_device_mel(model, tmp_path):
    x = mr.speech_like(HOP * 20 + 17, 6)                                   # 21 frames
    torch.manual_seed(3)
    a = model.generate_from_wav(x, tmp_path / 'a.wav', False, 11000, 550, True)
    mel = model.mel_front_end().melspectrogram(x)
    assert mel.is_cuda and tuple(mel.shape) == (1, 80, 21)
    torch.manual_seed(3)
    b = model.generate(mel, tmp_path / 'b.wav', False, 11000, 550, True)
    assert a.shape == (20 * HOP,) and a.dtype == np.float64
    np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match='broadcast'):                     # a 10-frame clip: generate()'s own refusal (T < 21), unchanged
        model.generate_from_wav(mr.speech_like(HOP * 9 + 17, 1), tmp_path / 'c.wav', False, 11000, 550, True)


def test_generate_many_from_wavs_is_generate_many_on_their_mels(model):
    a, b = mr.speech_like(HOP * 20 + 17, 6), mr.white(HOP * 22 + 100, 0.05, 7)
    fe = model.mel_front_end()
    mel_a, mel_b = fe.melspectrogram(a)[0].cpu().numpy(), fe.melspectrogram(b)[0].cpu().numpy()
    got = model.generate_many(wavs=[a, b], seeds=[11, 12])
    ref = model.generate_many([mel_a, mel_b], seeds=[11, 12])
    assert [g.shape for g in got] == [(20 * HOP,), (22 * HOP,)]
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g, r)
    with pytest.raises(ValueError):
        model.generate_many([mel_a], wavs=[a])


def test_cli_vocodes_a_wav_file(tmp_path):
    """``wavernn_gen.py --file x.wav``: the input saved as the reference's target file, the vocoded file next to it, (T - 1) hop samples."""
    from scipy.io import wavfile
    from tacotronv2_wavernn_chinese_amd.dsp import save_wav
    x = mr.speech_like(HOP * 20 + 17, 6)
    save_wav(x, tmp_path / 'x.wav', 22050)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_gen.py'), '--file', str(tmp_path / 'x.wav'), '-u', '--seed', '5'],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path / 'wavernn_inference_output'
    sr, tgt = wavfile.read(out / '__x__0k_steps_target.wav')
    assert sr == 22050
    np.testing.assert_array_equal(tgt, x)
    sr, voc = wavfile.read(out / 'x_gen_NOT_BATCHED_step=0k.wav')
    assert sr == 22050 and voc.dtype == np.float32 and voc.shape == (20 * HOP,) and np.isfinite(voc).all()
