"""The mel front end, host side (no GPU): the float64 yardstick ``tests/mel_ref.py`` pinned by analytic checks, the library's host-built
tables against it, frame counts, ``load_wav`` and the ``.wav`` branch of ``gen_from_file`` up to the device call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mel_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONDEFAULT = dict(mr.DEFAULT, win_length=800, hop_length=200, n_mels=40, fmin=0.0)


# ---- the yardstick itself -------------------------------------------------------------------------------------------------------
def test_slaney_scale_and_its_inverse():
    # 15 up to the one rounding of 1000 / (200 / 3), which librosa's own expression makes too
    assert abs(float(mr.hz_to_mel(1000.0)) - 15.0) <= np.spacing(15.0)
    assert abs(float(mr.mel_to_hz(15.0)) - 1000.0) <= 2 * np.spacing(1000.0)   # exp of a 2e-15 argument: one more rounding
    assert float(mr.hz_to_mel(500.0)) == pytest.approx(7.5, rel=1e-15)
    assert float(mr.hz_to_mel(6400.0)) == pytest.approx(15.0 + 27.0, rel=1e-14)   # 27 mels per factor 6.4 above 1 kHz
    f = np.array([0.0, 95.0, 999.0, 1000.0, 1001.0, 4000.0, 11025.0])
    np.testing.assert_allclose(mr.mel_to_hz(mr.hz_to_mel(f)), f, rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize('cfg', [mr.DEFAULT, NONDEFAULT], ids=['default', 'nondefault'])
def test_filterbank_rows(cfg):
    sr, n_fft, n_mels, fmin = cfg['sample_rate'], cfg['n_fft'], cfg['n_mels'], cfg['fmin']
    w = mr.mel_basis(sr, n_fft, n_mels, fmin)
    assert w.shape == (n_mels, n_fft // 2 + 1) and (w >= 0).all()
    freqs = np.arange(n_fft // 2 + 1) * sr / n_fft
    for r in w:
        nz = np.flatnonzero(r)
        assert nz.size and freqs[nz[0]] > fmin and freqs[nz[-1]] < sr / 2          # support strictly inside (fmin, sr / 2)
        assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))                     # one contiguous triangle
        assert np.all(np.diff(r[nz[0]:np.argmax(r) + 1]) > 0) and np.all(np.diff(r[np.argmax(r):nz[-1] + 1]) < 0)
    if cfg is mr.DEFAULT:
        counts = (w != 0).sum(axis=1)
        assert counts.min() == 7 and counts.max() == 80
        assert w[0].sum() == pytest.approx(0.0923, abs=5e-5)


def test_full_scale_sinusoid_on_a_bin_centre():
    c = mr.DEFAULT
    k = 200
    n = 6000
    y = np.cos(2 * np.pi * k * np.arange(n) / c['n_fft'])
    D = np.abs(mr.stft(y, c['n_fft'], c['hop_length'], c['win_length']))
    t = 10                                            # interior: no reflected sample under the window
    assert t * c['hop_length'] - c['win_length'] // 2 > 0 and t * c['hop_length'] + c['win_length'] // 2 < n
    # the image at -k adds the window's transform 2 k = 400 bins away: Hann sidelobes there are below 1e-7 of the main lobe
    assert D[k, t] == pytest.approx(mr.window(c['win_length']).sum() / 2, rel=1e-7)
    assert D.shape == (c['n_fft'] // 2 + 1, 1 + n // c['hop_length'])


def test_digital_silence_is_exactly_zero():
    for dt in (np.float64, np.float32):
        m = mr.melspectrogram(np.zeros(3000, np.float32), **mr.DEFAULT, dtype=dt)
        assert m.shape == (80, 11) and m.dtype == dt and not m.any()


def test_reflect_padding_and_window_placement():
    c = mr.DEFAULT
    y = np.arange(1, 3001, dtype=np.float64)
    yp = np.pad(y, 1024, mode='reflect')
    assert yp[1024] == 1 and yp[1023] == 2 and yp[0] == 1025 and yp[-1] == 3000 - 1024
    w = mr.padded_window(c['n_fft'], c['win_length'])
    assert w[:474].sum() == 0 and w[474] == 0 and w[475] > 0 and w[474 + 1100:].sum() == 0 and w[474 + 550] == 1.0


# ---- the library's tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', [mr.DEFAULT, NONDEFAULT], ids=['default', 'nondefault'])
def test_library_tables_are_the_float64_tables_rounded_once(cfg):
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    fe = MelFrontEnd(**{k: v for k, v in cfg.items()})
    tb = fe.tables()
    np.testing.assert_array_equal(tb['window'], mr.window(cfg['win_length']).astype(np.float32))
    np.testing.assert_array_equal(tb['twiddle'], mr.twiddles(cfg['n_fft']).astype(np.float32))
    rows, packed = mr.sparse_rows(mr.mel_basis(cfg['sample_rate'], cfg['n_fft'], cfg['n_mels'], cfg['fmin']).astype(np.float32))
    np.testing.assert_array_equal(tb['rows'], rows)
    np.testing.assert_array_equal(tb['weights'], packed)
    if cfg is mr.DEFAULT:
        assert rows[:, 1].min() == 7 and rows[:, 1].max() == 80


def test_mel_config_matches_the_header_layout(tmp_path):
    from tacotronv2_wavernn_chinese_amd import _cabi
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/wavernn_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(wrnn_mel_config));']
    lines += [f'  printf("{f} %zu\\n", offsetof(wrnn_mel_config, {f}));' for f, _ in _cabi.MelConfig._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / 'l.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c11', '-o', str(tmp_path / 'l'), str(tmp_path / 'l.c')])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / 'l')], text=True).splitlines())
    assert int(got['size']) == C.sizeof(_cabi.MelConfig)
    for f, _ in _cabi.MelConfig._fields_:
        assert int(got[f]) == getattr(_cabi.MelConfig, f).offset, f


# ---- frame counts and refusals --------------------------------------------------------------------------------------------------
def test_frames_and_refusals():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    fe = MelFrontEnd()
    nat = fe._native(0)
    assert nat.lib.wrnn_mel_frames(nat._h, 1024) == _cabi.ERR_INVALID
    with pytest.raises(ValueError, match='1025'):
        fe.frames(1024)
    for n, t in ((1025, 4), (2492, 10), (3000, 11)):
        assert nat.lib.wrnn_mel_frames(nat._h, n) == t == fe.frames(n) == mr.frames(n, 2048, 275)
    with pytest.raises(ValueError, match='UNSUPPORTED'):
        MelFrontEnd(n_fft=1024)
    h = C.c_void_p()
    cfg = _cabi.MelConfig(22050, 1024, 275, 1100, 80, 95.0, -100.0, 0)
    assert nat.lib.wrnn_mel_create(C.byref(cfg), C.byref(h)) == _cabi.ERR_UNSUPPORTED
    assert nat.lib.wrnn_mel_frames(h, 3000) < 0       # a refused handle computes nothing
    nat.lib.wrnn_mel_destroy(h)
    for bad in (dict(win_length=2049), dict(hop_length=0), dict(n_mels=129), dict(fmin=11025), dict(fmin=-1), dict(min_level_db=0)):
        with pytest.raises(ValueError, match='INVALID'):
            MelFrontEnd(**bad)
    with pytest.raises(ValueError):                    # refused on the host, before any device is touched
        fe.melspectrogram(np.zeros(1024, np.float32))
    with pytest.raises(ValueError):
        fe.melspectrogram([np.zeros(3000, np.float32), np.zeros(100, np.float32)])


# ---- load_wav -------------------------------------------------------------------------------------------------------------------
def test_load_wav(tmp_path):
    from scipy.io import wavfile
    from tacotronv2_wavernn_chinese_amd.frontend import load_wav
    rng = np.random.Generator(np.random.PCG64(1))
    pcm = rng.integers(-32768, 32768, size=500).astype(np.int16)
    pcm[:2] = (-32768, 32767)
    wavfile.write(tmp_path / 'i16.wav', 22050, pcm)
    y = load_wav(tmp_path / 'i16.wav', 22050)
    assert y.dtype == np.float32 and y.shape == (500,) and y[0] == -1.0 and y[1] == np.float32(32767 / 32768)
    np.testing.assert_array_equal(y, pcm.astype(np.float32) / 32768)
    st = rng.uniform(-1, 1, size=(400, 2)).astype(np.float32)
    wavfile.write(tmp_path / 'f32.wav', 22050, st)
    y = load_wav(tmp_path / 'f32.wav', 22050)
    assert y.dtype == np.float32 and y.shape == (400,)
    np.testing.assert_allclose(y, st.mean(axis=1), rtol=0, atol=1e-7)
    wavfile.write(tmp_path / 'u8.wav', 22050, np.array([0, 128, 255], np.uint8))
    np.testing.assert_array_equal(load_wav(tmp_path / 'u8.wav', 22050), np.array([-1.0, 0.0, 127 / 128], np.float32))
    wavfile.write(tmp_path / 'r16k.wav', 16000, pcm)
    with pytest.raises(ValueError, match=r'16000.*22050'):
        load_wav(tmp_path / 'r16k.wav', 22050)


# ---- gen_from_file, .wav branch ---------------------------------------------------------------------------------------------------
def test_gen_from_file_wav_branch_up_to_the_device_call(tmp_path):
    """In a child process (``hp.configure`` is once per process): the clip is loaded, saved as the reference's ``__{idx}__{k}k_steps_target.wav``,
    its samples go to the model's front end and the mel that comes back goes to ``generate`` under the ``.npy`` branch's file name."""
    code = (
        "import numpy as np, sys, torch\n"
        "from scipy.io import wavfile\n"
        "from tacotronv2_wavernn_chinese_amd.hparams import hparams as hp\n"
        "hp.configure()\n"
        "from tacotronv2_wavernn_chinese_amd.gen import gen_from_file\n"
        "class FE:\n"
        "    def melspectrogram(self, wav, device=None):\n"
        "        print('MEL', wav.dtype, wav.shape, float(np.abs(wav).max()), device)\n"
        "        return torch.full((1, 80, 1 + wav.shape[0] // 275), 0.5)\n"
        "class M:\n"
        "    def get_step(self): return 123456\n"
        "    def _device_index(self): return 0\n"
        "    def mel_front_end(self): return FE()\n"
        "    def generate(self, mel, path, batched, target, overlap, mu_law):\n"
        "        print('CALL', tuple(mel.shape), float(mel.min()), path, batched, target, overlap, mu_law)\n"
        f"d = r'{tmp_path}'\n"
        "wavfile.write(d + '/clip-7.wav', 22050, (np.arange(6000) % 100 * 300 - 15000).astype(np.int16))\n"
        "wavfile.write(d + '/slow.wav', 16000, np.zeros(6000, np.int16))\n"
        "gen_from_file(M(), d + '/clip-7.wav', d, False, 11000, 550)\n"
        "for bad in ('slow.wav', 'missing.wav'):\n"
        "    try:\n        gen_from_file(M(), d + '/' + bad, d, False, 11000, 550)\n        sys.exit(5)\n"
        "    except ValueError:\n        pass\n")
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    mel = [l for l in r.stdout.splitlines() if l.startswith('MEL')]
    call = [l for l in r.stdout.splitlines() if l.startswith('CALL')]
    assert len(mel) == 1 and 'float32 (6000,)' in mel[0] and 'cuda:0' in mel[0]
    assert len(call) == 1 and '(1, 80, 22) 0.5' in call[0] and 'clip-7_gen_NOT_BATCHED_step=123k.wav' in call[0] and call[0].endswith('True')
    from scipy.io import wavfile
    sr, tgt = wavfile.read(tmp_path / '__clip-7__123k_steps_target.wav')
    assert sr == 22050 and tgt.dtype == np.float32 and tgt.shape == (6000,)
    np.testing.assert_array_equal(tgt, ((np.arange(6000) % 100 * 300 - 15000) / 32768).astype(np.float32))
