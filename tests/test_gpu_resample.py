"""The resampler on the GPU (``csrc/resample.hip``) against the float64 restatement ``tests/resample_ref.py``.

Tolerance, the mel test's rule for the same situation (another, equally float32, summation order): for every input the restatement is
evaluated in float32 as well, g = max |ref32 - ref64|; the kernel passes with max |kernel - ref64| <= 8 g, and 8 g <= 2**-17 (half a
16-bit step) is asserted so that no input can loosen the bound.  Every parity test prints g, the kernel's error and their ratio before it
asserts (``pytest -s``).  The tone tests do not use the restatement's output as the target: the kernel's output is compared with the
ideal sine at the new rate (8 g + 2e-7) and, above the target Nyquist, with silence (8 g + 1e-7).

Measured on an MI355X: the kernel's error is 0.97 to 2.56 g over all the cases below (``profiles/resample.txt``)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import mel_ref as mr
from tests import resample_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 275
TILE = 256        # outputs per workgroup of the kernel
RATIOS = [(48000, 22050), (44100, 22050), (16000, 22050), (22050, 16000)]
INPUTS = ['speech_3000', 'noise_0.3', 'noise_1e-4', 'speech_5', 'one_sample']


def _input(name):
    return {'speech_3000': lambda: mr.speech_like(3000, 0), 'noise_0.3': lambda: mr.white(3000, 0.3, 3), 'noise_1e-4': lambda: mr.white(2200, 1e-4, 4),
            'speech_5': lambda: mr.speech_like(5, 5), 'one_sample': lambda: np.array([0.5], np.float32)}[name]()


def _ref(x, src, dst, **kw):
    """(ref64, g) of a clip (or of a range of its outputs)."""
    b = rr.bank(src, dst)
    r64 = rr.resample(x, src, dst, _bank=b, **kw)
    g = float(np.abs(rr.resample(x, src, dst, dtype=np.float32, _bank=b, **kw).astype(np.float64) - r64).max())
    return r64, g


_cache = {}


def case(name, src, dst):
    """(clip, ref64, g), computed once and shared."""
    key = (name, src, dst)
    if key not in _cache:
        x = _input(name)
        _cache[key] = (x,) + _ref(x, src, dst)
    return _cache[key]


def _rs(src, dst):
    from tacotronv2_wavernn_chinese_amd.frontend import Resampler
    return Resampler(src, dst)


def _check(name, got, r64, g, extra=0.0):
    err = float(np.abs(got.astype(np.float64) - r64).max())
    print(f'resample parity {name}: {r64.shape[0]} outputs, g = {g:.3e}, kernel error = {err:.3e} = {err / g:.2f} g, bound 8 g = {8 * g:.3e}')
    assert 0 < 8 * g <= 2.0 ** -17, (name, g)
    assert got.shape == r64.shape and got.dtype == np.float32
    assert err <= 8 * g + extra, (name, err, g)


@pytest.mark.parametrize('src,dst', RATIOS)
@pytest.mark.parametrize('name', INPUTS)
def test_parity_each_clip_alone(name, src, dst):
    x, r64, g = case(name, src, dst)
    rs = _rs(src, dst)
    out = rs.resample(x)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (1, rr.out_len(x.size, src, dst)) and rs.last_lens == [out.shape[1]]
    _check(f'{name} {src}->{dst}', out[0].cpu().numpy(), r64, g)


@pytest.mark.parametrize('n_out', [TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1])
def test_parity_at_the_tile_edges(n_out):
    src, dst = 48000, 22050
    n_in = next(n for n in range(1, 4000) if rr.out_len(n, src, dst) == n_out)
    x = mr.white(n_in, 0.3, 10 + n_out)
    r64, g = _ref(x, src, dst)
    got = _rs(src, dst).resample(x)[0].cpu().numpy()
    assert got.shape == (n_out,)
    _check(f'n_out = {n_out}', got, r64, g)


def test_ragged_batch_rows_are_bit_equal_to_the_solo_calls_and_padding_is_never_read():
    src, dst = 48000, 22050
    rs = _rs(src, dst)
    names = ['speech_3000', 'speech_5', 'noise_1e-4']
    clips = [case(n, src, dst)[0] for n in names]
    lens = [c.size for c in clips]
    buf = torch.full((3, max(lens) + 7), float('nan'), dtype=torch.float32, device='cuda')
    for i, c in enumerate(clips):
        buf[i, :lens[i]] = torch.from_numpy(c).cuda()
    out = rs.resample_padded(buf, lens)
    out_lens = [rr.out_len(n, src, dst) for n in lens]
    assert tuple(out.shape) == (3, max(out_lens)) and rs.last_lens == out_lens and len(set(out_lens)) == 3
    host = out.cpu().numpy()
    listed = rs.resample(clips).cpu().numpy()                       # the same batch from host clips, zero padding
    np.testing.assert_array_equal(host.view(np.uint32), listed.view(np.uint32))
    for i, n in enumerate(names):
        solo = rs.resample(clips[i]).cpu().numpy()[0]
        np.testing.assert_array_equal(host[i, :out_lens[i]].view(np.uint32), solo.view(np.uint32))
        assert not host[i, out_lens[i]:].view(np.uint32).any()     # exactly +0 past the clip's own end
        _check('ragged/' + n, host[i, :out_lens[i]], case(n, src, dst)[1], case(n, src, dst)[2])


def test_device_clips_stay_on_the_device():
    rs = _rs(16000, 22050)
    x = case('speech_3000', 16000, 22050)[0]
    a = rs.resample(torch.from_numpy(x).cuda())
    assert a.is_cuda and torch.equal(a, rs.resample(x))
    b = rs.resample([torch.from_numpy(x).cuda(), torch.from_numpy(x[:100]).cuda()])
    assert b.is_cuda and torch.equal(b[0], a[0]) and rs.last_lens == [a.shape[1], rr.out_len(100, 16000, 22050)]


def test_positions_are_64_bit():
    """96000 -> 22050 over 15 000 000 samples: t q passes 2**31 at t = 2**31 / 640, inside the clip."""
    src, dst = 96000, 22050
    x = mr.white(15_000_000, 0.3, 9)
    n_out = rr.out_len(x.size, src, dst)
    edge = 2 ** 31 // 640
    assert n_out == 3_445_313 and edge + 2048 < n_out - 4096
    rs = _rs(src, dst)
    out = rs.resample(x)
    assert tuple(out.shape) == (1, n_out)
    for label, (a, b) in {'around t q = 2**31': (edge - 2048, edge + 2048), 'last 4096': (n_out - 4096, n_out)}.items():
        r64, g = _ref(x, src, dst, start=a, stop=b)
        _check(f'96000->22050 {label}', out[0, a:b].cpu().numpy(), r64, g)


def test_tones_through_the_kernel():
    src, dst = 48000, 22050
    n_in = 6000
    t_in = np.arange(n_in) / src
    rs = _rs(src, dst)
    n_out = rr.out_len(n_in, src, dst)
    mid = slice(int(0.15 * n_out), int(0.85 * n_out))
    t_out = np.arange(n_out) / dst
    for f in (440.0, 0.8 * dst / 2):
        x = (0.5 * np.sin(2 * np.pi * f * t_in + 0.3)).astype(np.float32)
        _, g = _ref(x, src, dst)
        got = rs.resample(x)[0].cpu().numpy().astype(np.float64)
        err = float(np.abs(got - 0.5 * np.sin(2 * np.pi * f * t_out + 0.3))[mid].max())
        print(f'tone {f:.0f} Hz: g = {g:.3e}, distance to the ideal sine {err:.3e}, bound {8 * g + 2e-7:.3e}')
        assert 0 < 8 * g <= 2.0 ** -17 and err <= 8 * g + 2e-7
    x = (0.5 * np.sin(2 * np.pi * 1.2 * dst / 2 * t_in + 0.3)).astype(np.float32)
    _, g = _ref(x, src, dst)
    amp = float(np.abs(rs.resample(x)[0].cpu().numpy())[mid].max())
    print(f'tone at 1.2 x Nyquist: g = {g:.3e}, amplitude {amp:.3e}, bound {8 * g + 1e-7:.3e}')
    assert 8 * g <= 2.0 ** -17 and amp <= 8 * g + 1e-7


def test_error_paths_start_no_launch(monkeypatch):
    from tacotronv2_wavernn_chinese_amd import _cabi
    launches = []
    real = _cabi.NativeResampler.resample
    monkeypatch.setattr(_cabi.NativeResampler, 'resample', lambda self, *a: (launches.append(a), real(self, *a))[1])
    rs = _rs(48000, 22050)
    good = torch.zeros((2, 500), dtype=torch.float32, device='cuda')
    for wav, lens in [(good.cpu(), [500, 400]),                    # a host buffer
                      (good[:0], []),                              # B = 0
                      (good, [500, 501]),                          # a length longer than the buffer
                      (good, [500]), (good, [500, 0]), (good.double(), [500, 400]), (good[:, ::2], [250, 250])]:
        with pytest.raises(ValueError):
            rs.resample_padded(wav, lens)
    with pytest.raises(ValueError):
        rs.resample([])
    assert not launches
    nat = rs._native(0)
    for args in [(0, 500, 1, 2, 230, good.data_ptr()), (good.data_ptr(), 500, good.data_ptr(), 0, 230, good.data_ptr())]:
        with pytest.raises(_cabi.WrnnError):
            real(nat, *args, 0)
    same = _rs(22050, 22050)
    assert same.resample_padded(good, [500, 400]) is good and not launches
    rs.resample_padded(good, [500, 400])
    assert len(launches) == 1


# ---- composition ------------------------------------------------------------------------------------------------------------------
def _hp():
    return types.SimpleNamespace(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100, bits=10,
                                 mu_law=True, voc_mode='RAW', voc_pad=2, voc_seq_len=550)


def test_from_wavs_resamples_48k_files_into_the_same_corpus(tmp_path):
    from scipy.io import wavfile
    from tacotronv2_wavernn_chinese_amd import dataset as D
    from tacotronv2_wavernn_chinese_amd.frontend import read_wav
    rs = _rs(48000, 22050)
    paths, arrays = [], []
    for i, n in enumerate((9000, 16001, 12345, 5000)):             # the last one is too short after resampling: 2297 samples, 9 frames < 12
        pcm = np.round(mr.speech_like(n, 20 + i, 48000) * 5 * 32767).astype(np.int16)
        wavfile.write(tmp_path / f'c{i}.wav', 48000, pcm)
        paths.append(tmp_path / f'c{i}.wav')
        y, sr = read_wav(paths[-1])
        assert sr == 48000
        arrays.append(rs.resample(y)[0].cpu().numpy())
    native = mr.speech_like(4000, 30)                               # a clip at the model's own rate rides along
    with pytest.raises(ValueError, match='48000'):
        D.DeviceCorpus.from_wavs(paths, _hp(), 'cuda:0')
    a = D.DeviceCorpus.from_wavs(paths[:2] + [native] + paths[2:], _hp(), 'cuda:0', batch_clips=2, resample=True)
    b = D.DeviceCorpus.from_wavs(arrays[:2] + [native] + arrays[2:], _hp(), 'cuda:0', batch_clips=2)
    assert len(a) == len(b) == 4 and a.stems == ['c0', 'c1', 'utt00002', 'c2']
    assert a.label_len.tolist() == b.label_len.tolist() == [rr.out_len(9000, 48000, 22050), rr.out_len(16001, 48000, 22050), 4000, rr.out_len(12345, 48000, 22050)]
    assert a.frames.tolist() == b.frames.tolist() and a.n_clipped == b.n_clipped
    assert torch.equal(a.labels, b.labels) and torch.equal(a.mels, b.mels)
    c = D.DeviceCorpus.from_wavs([(read_wav(p)[0], 48000) for p in paths], _hp(), 'cuda:0', resample=True)     # (array, rate) pairs
    d = D.DeviceCorpus.from_wavs(paths, _hp(), 'cuda:0', resample=True)
    assert len(c) == len(d) == 3 and torch.equal(c.labels, d.labels) and torch.equal(c.mels, d.mels)
    with pytest.raises(ValueError, match='resample=True'):
        D.DeviceCorpus.from_wavs([(read_wav(paths[0])[0], 48000)], _hp(), 'cuda:0')


@pytest.fixture(scope='module')
def model():
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    sd = make_state_dict(0, variant='peaky')
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to('cuda:0')


def _clip48(seed=6):
    n = next(n for n in range(12000, 14000) if rr.out_len(n, 48000, 22050) == HOP * 20 + 17)     # 21 frames at 22.05 kHz
    return mr.speech_like(n, seed, 48000)


def test_generate_from_wav_at_another_rate_is_generate_from_the_resampled_wav(model, tmp_path):
    x48 = _clip48()
    torch.manual_seed(3)
    a = model.generate_from_wav(x48, tmp_path / 'a.wav', False, 11000, 550, True, wav_rate=48000)
    y = _rs(48000, 22050)(x48)
    assert y.is_cuda and tuple(y.shape) == (1, HOP * 20 + 17)
    torch.manual_seed(3)
    b = model.generate_from_wav(y, tmp_path / 'b.wav', False, 11000, 550, True)
    assert a.shape == (20 * HOP,) and a.dtype == np.float64
    np.testing.assert_array_equal(a, b)
    torch.manual_seed(3)
    np.testing.assert_array_equal(model.generate_from_wav(y[0].cpu().numpy(), tmp_path / 'c.wav', False, 11000, 550, True, wav_rate=22050), b)


def test_generate_many_takes_the_clips_rates(model):
    x48, x22 = _clip48(7), mr.speech_like(HOP * 22 + 100, 8)
    y = _rs(48000, 22050)(x48)[0].cpu().numpy()
    got = model.generate_many(wavs=[x48, x22], wav_rates=[48000, 22050], seeds=[11, 12])
    ref = model.generate_many(wavs=[y, x22], seeds=[11, 12])
    assert [g.shape for g in got] == [(20 * HOP,), (22 * HOP,)]
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g, r)
    both = model.generate_many(wavs=[x48, x48], wav_rates=48000, seeds=[11, 11])
    np.testing.assert_array_equal(both[0], got[0])
    np.testing.assert_array_equal(both[1], got[0])
    with pytest.raises(ValueError):
        model.generate_many(wavs=[x48, x22], wav_rates=[48000])


def test_cli_vocodes_a_48k_wav_file(tmp_path):
    """``wavernn_gen.py --file clip48k.wav --resample``: the target file is the resampled clip at 22 050 Hz, ceil(n 147 / 320) samples."""
    from scipy.io import wavfile
    from tacotronv2_wavernn_chinese_amd.dsp import save_wav
    x48 = _clip48()
    save_wav(x48, tmp_path / 'clip48k.wav', 48000)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_gen.py'), '--file', str(tmp_path / 'clip48k.wav'), '-u', '--seed', '5', '--resample'],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path / 'wavernn_inference_output'
    sr, tgt = wavfile.read(out / '__clip48k__0k_steps_target.wav')
    assert sr == 22050 and tgt.shape == (-(-x48.size * 147 // 320),) == (HOP * 20 + 17,)
    np.testing.assert_array_equal(tgt, _rs(48000, 22050)(x48)[0].cpu().numpy())
    sr, voc = wavfile.read(out / 'clip48k_gen_NOT_BATCHED_step=0k.wav')
    assert sr == 22050 and voc.dtype == np.float32 and voc.shape == (20 * HOP,) and np.isfinite(voc).all()
