"""The resampler without a GPU: properties of the float64 restatement ``tests/resample_ref.py``, the library's host-only entries
(``wrnn_resample_create / _out_len / _bank``) against it, and the Python surface up to the device call.

Bounds of the property tests: the values a float64 prototype of the closed form gives (every phase's taps sum to 1 within 3e-8, a
passband sine comes out as the ideal sine within 4e-8, a tone above the transition band comes out below -153 dB), each with a factor 4 of
slack; they are properties of the filter, not of an implementation.

The bank sizes: 22050 -> 16000 reduces to p / q = 320 / 441 (gcd 50), hence 320 phases of 2 ceil(64 * 441 / 320) = 178 taps."""
import math
import subprocess
import sys

import numpy as np
import pytest

from tests import resample_ref as rr

RATES = [(48000, 22050), (44100, 22050), (16000, 22050), (96000, 22050), (22050, 16000)]
TABLE = {(48000, 22050): (147, 320, 280), (44100, 22050): (1, 2, 256), (16000, 22050): (441, 320, 128), (96000, 22050): (147, 640, 558),
         (22050, 16000): (320, 441, 178)}


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('src,dst', RATES)
def test_ref_plan_and_dc_gain(src, dst):
    p, q, scale, half = rr.plan(src, dst)
    assert (p, q, 2 * half) == TABLE[(src, dst)]
    assert p * src == q * dst and math.gcd(p, q) == 1
    assert scale == min(1.0, dst / src) and half == math.ceil(64 / scale)
    b = rr.bank(src, dst)
    assert b.shape == (p, 2 * half)
    dc = float(np.abs(b.sum(axis=1) - 1.0).max())
    print(f'{src} -> {dst}: max |phase sum - 1| = {dc:.3e}')
    assert dc <= 4 * 3e-8


def _inner(n_in, src, dst):
    """Outputs whose whole filter support lies inside a clip of n_in samples."""
    p, q, _, half = rr.plan(src, dst)
    t = np.arange(rr.out_len(n_in, src, dst))
    n = (t * q) // p
    return t[(n - half + 1 >= 0) & (n + half < n_in)]


@pytest.mark.parametrize('src,dst', [(48000, 22050), (44100, 22050), (16000, 22050), (22050, 16000)])
def test_ref_passband_sines_and_stopband_tones(src, dst):
    n_in = 4 * rr.plan(src, dst)[3] + 1500
    t_in = np.arange(n_in) / src
    keep = _inner(n_in, src, dst)
    assert keep.size > 300
    lo_nyq = min(src, dst) / 2.0
    for f in (440.0, 0.8 * lo_nyq):
        y = rr.resample(np.sin(2 * np.pi * f * t_in + 0.3), src, dst)
        err = float(np.abs(y[keep] - np.sin(2 * np.pi * f * keep / dst + 0.3)).max())
        print(f'{src} -> {dst}: sine at {f:.0f} Hz, max error {err:.3e}')
        assert err <= 4 * 4e-8
    if dst < src:          # tones between the target Nyquist and the source's must vanish
        for k in (1.06, 1.2, 1.5):
            f = k * dst / 2.0
            if f >= src / 2.0:
                continue
            y = rr.resample(np.sin(2 * np.pi * f * t_in + 0.3), src, dst)
            amp = float(np.abs(y[keep]).max())
            print(f'{src} -> {dst}: tone at {k} x Nyquist, {20 * np.log10(max(amp, 1e-300)):.1f} dB')
            assert amp <= 4 * 10 ** (-153 / 20)


def test_ref_ranges_and_dtype():
    x = np.random.Generator(np.random.PCG64(0)).standard_normal(900).astype(np.float32)
    full = rr.resample(x, 48000, 22050)
    assert full.shape == (rr.out_len(900, 48000, 22050),) == (414,) and full.dtype == np.float64
    np.testing.assert_array_equal(rr.resample(x, 48000, 22050, start=100, stop=160), full[100:160])
    np.testing.assert_array_equal(rr.resample(x, 48000, 22050, start=400, stop=10 ** 6), full[400:])
    f32 = rr.resample(x, 48000, 22050, dtype=np.float32)
    assert f32.dtype == np.float32 and 0 < np.abs(f32 - full).max() < 1e-5


# ---- the library's host-only entries -----------------------------------------------------------------------------------------------
def _nat(src, dst):
    from tacotronv2_wavernn_chinese_amd import _cabi
    return _cabi.NativeResampler(src, dst)


@pytest.mark.parametrize('src,dst', RATES)
def test_bank_is_the_restatement_rounded_once(src, dst):
    nat = _nat(src, dst)
    assert (nat.p, nat.q, nat.taps) == TABLE[(src, dst)]
    got = nat.bank()
    want = rr.bank(src, dst).astype(np.float32)
    assert got.shape == want.shape and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f'{src} -> {dst}: max |bank - float32(ref64)| = {err:.3e}, bound {2.0 ** -24 * float(np.abs(got).max()):.3e}')
    assert err <= 2.0 ** -24 * float(np.abs(got).max())


@pytest.mark.parametrize('src,dst', RATES + [(22050, 22050)])
def test_out_len_is_the_integer_ceiling(src, dst):
    nat = _nat(src, dst)
    p, q = nat.p, nat.q
    for n in (0, 1, 2, q - 1, q, q + 1, 7 * q, 7 * q + 1, 110250, 15_000_000, 2 ** 31 - 1):
        assert nat.out_len(n) == -((-n * p) // q) == rr.out_len(n, src, dst)
    assert nat.out_len(q) == p and nat.out_len(1) == -(-p // q)
    with pytest.raises(ValueError):
        nat.out_len(-1)
    with pytest.raises(ValueError):
        nat.out_len(2 ** 31)


def test_refusals_name_the_rates_and_touch_no_device():
    import ctypes as C
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.frontend import Resampler
    lib = _cabi.load_library()
    for src, dst, code in [(0, 22050, _cabi.ERR_INVALID), (22050, 0, _cabi.ERR_INVALID), (-48000, 22050, _cabi.ERR_INVALID),
                           (22050 * 33, 22050, _cabi.ERR_UNSUPPORTED),        # scale < 1 / 32
                           (192000, 191999, _cabi.ERR_UNSUPPORTED)]:          # 191999 phases x 130 taps > 2**24
        h = C.c_void_p()
        assert lib.wrnn_resample_create(src, dst, 0, C.byref(h)) == code
        msg = lib.wrnn_resample_last_error(h).decode()
        assert str(src) in msg and str(dst) in msg
        assert lib.wrnn_resample_out_len(h, 100) < 0                          # a refused handle computes nothing
        assert lib.wrnn_resample_bank(h, None, None, None, None) == _cabi.ERR_INVALID
        assert lib.wrnn_resample(h, None, 1, None, 1, 1, None, None) == _cabi.ERR_STATE
        lib.wrnn_resample_destroy(h)
        with pytest.raises(ValueError, match=_cabi.ERR_NAMES[code]):
            Resampler(src, dst)
    assert 22050 * 130 <= 2 ** 24
    assert Resampler(22051, 22050).taps == 130                                 # 22050 phases: large, inside the limit
    assert Resampler(22050 * 32, 22050).taps == 2 * 64 * 32                    # scale = 1 / 32 exactly is accepted
    # bad launch arguments come back before any device call (this machine may have no GPU at all)
    nat = _nat(48000, 22050)
    for args in [(None, 10, 1, 1, 5, 1), (1, 10, None, 1, 5, 1), (1, 10, 1, 1, 5, None), (1, 0, 1, 1, 5, 1), (1, 10, 1, 0, 5, 1),
                 (1, 10, 1, 65536, 5, 1), (1, 10, 1, 1, 0, 1)]:
        assert lib.wrnn_resample(nat._h, *args, None) == _cabi.ERR_INVALID
    eq = _nat(22050, 22050)
    assert lib.wrnn_resample(eq._h, 1, 10, 1, 1, 10, 1, None) == _cabi.ERR_INVALID   # the low-pass never runs at ratio 1


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
def _write(path, rate, n=600, seed=1):
    from scipy.io import wavfile
    pcm = np.random.Generator(np.random.PCG64(seed)).integers(-20000, 20000, size=n).astype(np.int16)
    wavfile.write(path, rate, pcm)
    return pcm


def test_read_wav_returns_the_rate_and_load_wav_still_refuses(tmp_path):
    from tacotronv2_wavernn_chinese_amd.frontend import load_wav, read_wav
    pcm = _write(tmp_path / 'a.wav', 16000)
    y, sr = read_wav(tmp_path / 'a.wav')
    assert sr == 16000 and isinstance(sr, int) and y.dtype == np.float32
    np.testing.assert_array_equal(y, pcm.astype(np.float32) / 32768)
    _write(tmp_path / 'b.wav', 22050)
    np.testing.assert_array_equal(load_wav(tmp_path / 'b.wav', 22050), read_wav(tmp_path / 'b.wav')[0])
    np.testing.assert_array_equal(load_wav(tmp_path / 'b.wav', 22050, resample=True), read_wav(tmp_path / 'b.wav')[0])   # no device needed
    with pytest.raises(ValueError, match=r'16000.*22050.*resample=True'):
        load_wav(tmp_path / 'a.wav', 22050)


def test_equal_rates_return_the_input_object():
    import torch
    from tacotronv2_wavernn_chinese_amd.frontend import Resampler
    rs = Resampler(22050, 22050)
    for x in (np.zeros(10, np.float32), [np.zeros(3), np.zeros(4)], torch.zeros(7)):
        assert rs.resample(x) is x and rs(x) is x
    assert rs.out_len(12345) == 12345 and (rs.p, rs.q) == (1, 1)


def test_resampler_refuses_before_the_device():
    import torch
    from tacotronv2_wavernn_chinese_amd.frontend import Resampler
    rs = Resampler(48000, 22050)
    assert (rs.p, rs.q, rs.taps) == (147, 320, 280) and rs.bank().shape == (147, 280) and rs.out_len(320) == 147
    with pytest.raises(ValueError):
        rs.resample([])
    with pytest.raises(ValueError):
        rs.resample(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        rs.resample([np.zeros(5, np.float32), np.zeros(0, np.float32)])
    with pytest.raises(ValueError):
        rs.resample(np.zeros(5, np.float32), device='cpu')
    with pytest.raises(ValueError):
        rs.resample_padded(torch.zeros((2, 8)), [8, 4])                        # a host buffer


def test_from_wavs_default_still_refuses_another_rate(tmp_path):
    """Up to the first file: in a child process that hides the GPU, so that the refusal is shown to come before any device work."""
    _write(tmp_path / 'slow.wav', 16000, n=30000)
    code = ("import sys\n"
            "from tacotronv2_wavernn_chinese_amd import dataset\n"
            "from tacotronv2_wavernn_chinese_amd.hparams import hparams as hp\n"
            "hp.configure()\n"
            "dataset._device = lambda d: None\n"
            "class FE:\n"
            "    hop_length, n_mels, sample_rate = 275, 80, 22050\n"
            "    def __init__(self, *a, **k): pass\n"
            "import tacotronv2_wavernn_chinese_amd.frontend as fe\n"
            "fe.MelFrontEnd = FE\n"
            "try:\n"
            f"    dataset.DeviceCorpus.from_wavs([r'{tmp_path}/slow.wav'], hp)\n"
            "    sys.exit(5)\n"
            "except ValueError as e:\n"
            "    assert '16000' in str(e) and '22050' in str(e), e\n"
            "try:\n"
            "    import numpy as np\n"
            "    dataset.DeviceCorpus.from_wavs([(np.zeros(30000, np.float32), 16000)], hp)\n"
            "    sys.exit(6)\n"
            "except ValueError as e:\n"
            "    assert '16000' in str(e) and 'resample=True' in str(e), e\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout


def test_clis_know_the_flag():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for script in ('wavernn_gen.py', 'wavernn_preprocess.py', 'wavernn_train.py'):
        r = subprocess.run([sys.executable, os.path.join(root, script), '--help'], cwd=root, capture_output=True, text=True)
        assert r.returncode == 0 and '--resample' in r.stdout, (script, r.stderr[-500:])
