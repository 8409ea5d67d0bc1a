"""Griffin-Lim on the GPU (``csrc/griffin_lim.hip``, ``frontend.GriffinLim``, ``wavernn_gen.py --griffin_lim``) against the restatement
``tests/griffin_lim_ref.py``.

Tolerance, the rule of the mel tests: for every input g = max |ref32 - ref64| of the restatement evaluated in float32 and in float64, the
kernel passes with max |kernel - ref64| <= K g, K = 8.  An absolute ceiling on K g keeps a degenerate g from hiding a failure: 1e-3 of
the reference's peak for the waves and the magnitudes (an error 60 dB under the signal; the chain is a few hundred float32 operations
deep per sample and round, each good to 6e-8), 1e-4 of the peak for the de-emphasis alone (its float32 recurrence settles at about
eps / (1 - k) = 2e-6 of the signal).  Every parity check prints g, the kernel's error and their ratio before it asserts (``pytest -s``);
``profiles/griffin_lim.txt`` records them: 0.00 - 0.18 g for the magnitudes and the waves (the kernels compute in float64, so what is
left is the float32 rounding of the output) and up to 1.00 g for the de-emphasis alone (at n = 2, where g itself is one rounding).  K
stays at the mel tests' 8: the de-emphasis cases leave no room under 1, and a factor between 1 and 8 would be fitted to this table.
The inputs are seeded harmonic chirps run through the restated forward chain."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal
import torch

from tests import griffin_lim_ref as gr
from tests import taco_mel_ref as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, NFFT, WIN, NB = 275, 2048, 1100, 1025
K = 8
PROFILES = {'tacotron': tm.TACOTRON, 'vocoder': tm.VOCODER}
ROUNDS = (0, 1, 2, 60)

_GL, _MELS, _REFS = {}, {}, {}


def _gl(name, **kw):
    """One ``GriffinLim`` per configuration (the handle owns device tables and workspaces)."""
    from tacotronv2_wavernn_chinese_amd.frontend import GriffinLim
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _GL:
        _GL[key] = GriffinLim(features=name, **kw)
    return _GL[key]


def _mel(name, T, **framing):
    """The first T frames of the restated mel of a seeded chirp, float32 (n_mels, T)."""
    key = (name,) + tuple(sorted(framing.items()))
    if key not in _MELS:
        hop = framing.get('hop_length', HOP)
        _MELS[key] = tm.melspectrogram(gr.harmonic_chirp(max(hop * 60, 1500), 4), **dict(PROFILES[name], **framing)).astype(np.float32)
    assert _MELS[key].shape[1] >= T
    return np.ascontiguousarray(_MELS[key][:, :T])


def _phases(T, seed=9):
    return np.random.Generator(np.random.PCG64(seed)).random((T, NB), dtype=np.float32)


def _ref(name, T, n_iter, **framing):
    """(ref64, g) per round of ``ROUNDS`` up to n_iter, computed once per (profile, T, framing)."""
    key = (name, T, n_iter) + tuple(sorted(framing.items()))
    if key not in _REFS:
        keep = tuple(i for i in ROUNDS if i <= n_iter)
        _REFS[key] = gr.error_scale(_mel(name, T, **framing), _phases(T), n_iter, keep=keep, **dict(PROFILES[name], **framing))
    return _REFS[key]


def _check(label, got, r64, g, ceiling):
    err = float(np.abs(got.astype(np.float64) - r64).max()) if r64.size else 0.0
    peak = float(np.abs(r64).max()) if r64.size else 0.0
    print(f'griffin-lim parity {label}: peak {peak:.3e}, g = {g:.3e}, kernel error = {err:.3e} = {err / g if g else float("nan"):.2f} g, '
          f'bound {K} g = {K * g:.3e}')
    assert got.shape == r64.shape and got.dtype == np.float32, label
    assert K * g <= ceiling * peak, (label, g, peak)
    assert err <= K * g, (label, err, g)


@pytest.mark.parametrize('T', [1, 2, 9])
@pytest.mark.parametrize('name', ['tacotron', 'vocoder'])
def test_stage_a_magnitudes(name, T):
    mel = _mel(name, T).copy()
    mel[3, :] = 0.0                # both clips of the [0, 1] range, reached and passed
    mel[7, :] = 1.0
    mel[11, :] = -0.2
    mel[13, :] = 1.3
    f = PROFILES[name]
    s64 = gr.mel_to_magnitude(mel, **f)
    s32 = gr.mel_to_magnitude(mel, dtype=np.float32, **f).astype(np.float64)
    assert (s64 <= 1.0001e-15).any() and (s64 > 1.0).any()               # the 1e-10 floor (** 1.5) and the open range
    _, S = _gl(name).reconstruct(mel, n_iter=0, phases='zero', magnitude=True)
    got = S.cpu().numpy()
    assert got.shape == (1, T, NB)
    _check(f'stage a {name} T={T}', got[0].T, s64, float(np.abs(s32 - s64).max()), 1e-3)
    assert (got[0].T[s64 <= 1.0001e-15] <= np.float32(1.0001e-15)).all()   # floored bins stay on the floor


@pytest.mark.parametrize('n_iter', ROUNDS)
@pytest.mark.parametrize('T', [2, 5, 9, 41])
@pytest.mark.parametrize('name', ['tacotron', 'vocoder'])
def test_injected_phases_whole_wave(name, T, n_iter):
    """Measured on an MI355X: 0.00 - 0.18 g on the 32 cases, the float32 rounding of the output.  The rounds run in float64 for this
    test's sake: a float32 version of the kernels gave 0.23 - 3.79 g on 31 cases and 9.19 g on vocoder, T = 41, n_iter = 60, because
    X / |X| turns rounding into a phase error where a bin passes near zero (``DESIGN.md`` 3.16)."""
    r64, g = _ref(name, T, 60)
    gl = _gl(name)
    args = dict(n_iter=n_iter, phases=_phases(T)[None])
    got = gl.reconstruct(_mel(name, T), **args).cpu().numpy()
    assert got.shape == (1, HOP * (T - 1)) and gl.last_samples == [HOP * (T - 1)]
    _check(f'wave {name} T={T} n_iter={n_iter}', got[0], r64[n_iter], g[n_iter], 1e-3)
    again = gl.reconstruct(_mel(name, T), **args).cpu().numpy()
    np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize('name', ['tacotron', 'vocoder'])
def test_ragged_batch_rows_are_bit_equal_to_the_solo_calls(name):
    gl = _gl(name)
    frames, T_max = (9, 1, 5), 11
    mels = np.zeros((3, 80, T_max), np.float32)
    ph = np.stack([_phases(T_max, 20 + b) for b in range(3)])
    for b, T in enumerate(frames):
        mels[b, :, :T] = _mel(name, T)
    mels[:, :, 9:] = 0.5                                                  # what lies past a clip's own frames is never read
    out = gl.reconstruct(torch.from_numpy(mels), frames, n_iter=2, phases=ph).cpu().numpy()
    assert out.shape == (3, HOP * (T_max - 1)) and gl.last_samples == [HOP * 8, 0, HOP * 4]
    for b, T in enumerate(frames):
        solo = gl.reconstruct(mels[b, :, :T], n_iter=2, phases=ph[b:b + 1, :T]).cpu().numpy()
        n = HOP * (T - 1)
        assert solo.shape == (1, max(1, n))
        np.testing.assert_array_equal(out[b, :n].view(np.uint32), solo[0, :n].view(np.uint32))
        assert not out[b, n:].any() and not solo[0, n:].any()             # exact zeros past the clip, the whole T = 1 clip included
        assert n == 0 or np.abs(out[b, :n]).max() > 1e-3


@pytest.mark.parametrize('framing', [dict(hop_length=256), dict(hop_length=200), dict(hop_length=1100), dict(hop_length=6),
                                     dict(win_length=2048)], ids=lambda d: '-'.join(f'{k}={v}' for k, v in d.items()))
@pytest.mark.parametrize('name', ['tacotron', 'vocoder'])
def test_other_framings(name, framing):
    """hop = win_length: no overlap at all; hop = 6: 184 frames cover every sample; win_length = n_fft: no zero margin in the frame.

    Measured on an MI355X: 0.01 - 0.12 g on the 10 cases."""
    hop = framing.get('hop_length', HOP)
    T = {256: 3, 200: 3, 1100: 2, 6: 51, 275: 3}[hop]
    r64, g = _ref(name, T, 2, **framing)
    got = _gl(name, **framing).reconstruct(_mel(name, T, **framing), n_iter=2, phases=_phases(T)[None]).cpu().numpy()
    assert got.shape == (1, hop * (T - 1)) and 300 <= got.shape[1] <= 1100
    _check(f'framing {name} {framing}', got[0], r64[2], g[2], 1e-3)


def test_philox_phases_equal_the_replayed_injected_ones():
    gl = _gl('tacotron')
    T = 5
    mels = [_mel('tacotron', T), _mel('vocoder', T)]                      # two different clips; any [0, 1] mel is an input
    out = gl.reconstruct(mels, n_iter=2, seed=1234567890123).cpu().numpy()
    ph = np.stack([gr.philox_phases(1234567890123, b, T) for b in range(2)])
    assert ph.shape == (2, T, NB) and 0 < ph.min() and ph.max() < 1
    inj = gl.reconstruct(mels, n_iter=2, phases=ph).cpu().numpy()
    np.testing.assert_array_equal(out.view(np.uint32), inj.view(np.uint32))
    other = gl.reconstruct(mels, n_iter=2, seed=1234567890124).cpu().numpy()
    assert np.abs(other - out).max() > 1e-3 * np.abs(out).max()
    assert np.abs(out[0] - out[1]).max() > 1e-3 * np.abs(out).max()       # the clip index is part of the key (and the mels differ)
    zero = gl.reconstruct(mels, n_iter=2, phases='zero').cpu().numpy()
    inj0 = gl.reconstruct(mels, n_iter=2, phases=np.zeros((2, T, NB), np.float32)).cpu().numpy()
    np.testing.assert_array_equal(zero.view(np.uint32), inj0.view(np.uint32))
    gl.reconstruct(mels, n_iter=1)                                        # neither: a fresh seed, kept
    assert isinstance(gl.last_seed, int)


@pytest.mark.parametrize('lens', [(1, 255, 11000), (2, 256, 257), (2047, 2048, 2049)], ids=lambda l: '-'.join(map(str, l)))
@pytest.mark.parametrize('k', [0.97, 0.5])
def test_deemphasis_alone(k, lens):
    """(2047, 2048, 2049) are the kernel's own edge: its scan walks tiles of 2048 samples."""
    from tacotronv2_wavernn_chinese_amd.frontend import deemphasis
    rng = np.random.Generator(np.random.PCG64(sum(lens)))
    n_max = max(lens) + 5
    x = (0.3 * rng.standard_normal((3, n_max))).astype(np.float32)
    x[:, :] += 0.1                                                        # a DC part: the filter's gain is 1 / (1 - k) there
    out = deemphasis(torch.from_numpy(x).cuda(), lens, k).cpu().numpy()
    assert out.shape == x.shape and out.dtype == np.float32
    for b, n in enumerate(lens):
        r64 = scipy.signal.lfilter([1.0], [1.0, -k], x[b, :n].astype(np.float64))
        g = float(np.abs(gr.deemphasis(x[b, :n], k, np.float32).astype(np.float64) - r64).max())
        if n == 1:
            assert g == 0.0 and out[b, 0] == x[b, 0]                      # y[0] = x[0] exactly, in both
        _check(f'de-emphasis k={k} n={n}', out[b, :n], r64, g, 1e-4)
        assert not out[b, n:].any()


@pytest.mark.parametrize('name', ['tacotron', 'vocoder'])
def test_round_trip_on_the_device_only(name):
    """wav -> mel -> wav -> mel on this repository's kernels alone: the mel of the reconstruction is as close to the input mel as the
    float64 restatement's own round trip says Griffin-Lim gets after 60 rounds, times 1.05 (the two differ by rounding only).  Measured
    on an MI355X: 0.06132 against 0.06132 (tacotron), 0.05607 against 0.05607 (vocoder), ratio 1.0000 both: the margin stays 1.05."""
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    f, seed = PROFILES[name], 77
    y = gr.harmonic_chirp(HOP * 40, 6)
    fe, gl = MelFrontEnd(features=name), _gl(name)
    mel = fe.melspectrogram(y)
    T = mel.shape[2]
    assert T == 41
    wav = gl.reconstruct(mel[0], n_iter=60, seed=seed)
    assert wav.is_cuda and wav.shape == (1, HOP * (T - 1))
    mel2 = fe.melspectrogram(wav[0])
    dev = float((mel2 - mel)[0, :, 2:T - 2].abs().mean())
    m64 = tm.melspectrogram(y, **f).astype(np.float64)
    w64 = gr.reconstruct(m64, gr.philox_phases(seed, 0, T), 60, **f)
    ref = float(np.abs(tm.melspectrogram(w64, **f).astype(np.float64) - m64)[:, 2:T - 2].mean())
    print(f'round trip {name}: device {dev:.5f}, float64 restatement {ref:.5f}, ratio {dev / ref:.4f}')
    assert 0 < ref < 0.1                                                  # Griffin-Lim does get close: a [0, 1] mel, 1 = 100 dB
    assert dev <= 1.05 * ref


def test_class_on_a_list_equals_the_c_entry():
    from tacotronv2_wavernn_chinese_amd import _cabi
    gl = _gl('tacotron')
    mels = [_mel('tacotron', 9), _mel('tacotron', 5)]
    out = gl.reconstruct(mels, n_iter=3, seed=5).cpu().numpy()
    assert gl.last_samples == [HOP * 8, HOP * 4]
    nat = _cabi.NativeGriffinLim(sample_rate=22050, n_fft=NFFT, hop_length=HOP, win_length=WIN, n_mels=80, fmin=95, min_level_db=-100, device=0,
                                 features=_cabi.MelFeatures(1, 2, 7600.0, 20.0, 0.97, 0.999, 4.0), griffin=_cabi.GriffinConfig(1.5, 3))
    batch = np.zeros((2, 80, 9), np.float32)
    batch[0], batch[1, :, :5] = mels[0], mels[1]
    b = torch.from_numpy(batch).cuda()
    fr = torch.tensor([9, 5], dtype=torch.int32).cuda()
    raw = torch.full((2, HOP * 8 + 3), 7.0, device='cuda')
    nat.griffin_lim(b.data_ptr(), fr.data_ptr(), 2, 9, -1, _cabi.GRIFFIN_PHASE_PHILOX, 5, 0, raw.data_ptr(), raw.shape[1], 0, 0)   # n_iter < 0: the default, 3
    torch.cuda.synchronize()
    raw = raw.cpu().numpy()
    np.testing.assert_array_equal(raw[:, :HOP * 8].view(np.uint32), out.view(np.uint32))
    assert not raw[:, HOP * 8:].any() and not raw[1, HOP * 4:].any()
    with pytest.raises(_cabi.WrnnError, match='INVALID'):                 # a buffer shorter than the longest clip
        nat.griffin_lim(b.data_ptr(), fr.data_ptr(), 2, 9, 1, _cabi.GRIFFIN_PHASE_ZERO, 0, 0, raw.ctypes.data, HOP * 8 - 1, 0, 0)
    with pytest.raises(_cabi.WrnnError, match='INVALID'):                 # injected mode without phases
        nat.griffin_lim(b.data_ptr(), fr.data_ptr(), 2, 9, 1, _cabi.GRIFFIN_PHASE_INJECTED, 0, 0, raw.ctypes.data, HOP * 8, 0, 0)


def test_command_line_writes_the_wav_of_the_class_and_loads_no_weights(tmp_path):
    from scipy.io import wavfile
    mel = _mel('vocoder', 9)
    np.save(tmp_path / 'mel.npy', mel.T)                                  # (T, n_mels), the reference's file layout
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_gen.py'), '--file', str(tmp_path / 'mel.npy'), '--griffin_lim', '3', '--seed', '1'],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'Initialising Model' not in r.stdout and 'latest_weights' not in r.stdout
    sr, got = wavfile.read(tmp_path / 'wavernn_inference_output' / 'mel_griffin_lim.wav')
    assert sr == 22050 and got.dtype == np.float32 and got.shape == (HOP * 8,)
    want = _gl('vocoder').reconstruct(mel, n_iter=3, seed=1).cpu().numpy()[0]
    peak = float(np.abs(want).max())
    if peak > 1.0:
        assert 'rescaled to 0.999' in r.stderr
        want = want * np.float32(0.999 / peak)
    else:
        assert 'rescaled' not in r.stderr
    np.testing.assert_array_equal(got, want)
