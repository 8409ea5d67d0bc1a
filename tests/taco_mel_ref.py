"""NumPy restatement of the feature profiles of the mel front end (``wrnn_mel_features``), the yardstick of the profile tests.

Written from the formulas of ``include/wavernn_amd.h`` (which follow ``tacotron/datasets/audio.py:95-102, 203-207, 250-295``,
``tacotron/datasets/preprocessor.py:52-121`` and ``wavernn_preprocess.py:149-159``), in the style of ``tests/mel_ref.py``, whose window,
Slaney scale and input generators it imports.  It is a restatement and not the reference's output: librosa and TensorFlow are not
dependencies of this repository, and nothing here has been compared with them.

For one clip x of n >= 1 samples, every step a switch of its own (``TACOTRON`` holds the reference's values, ``VOCODER`` today's):

1. ``preemphasis`` k:       p[0] = x[0], p[i] = x[i] - k x[i-1] (``lfilter([1, -k], [1], x)``); 0: p = x.
2. ``preemph_rescale`` r:   p <- p / max|p| * r; 0, or max|p| == 0: unchanged.
3. ``pad_mode``:            frame t = p[t hop - n_fft/2 + i], 0 <= i < n_fft, T = 1 + n // hop frames; outside [0, n) the reflection
                            ('reflect', n >= n_fft/2 + 1 needed) or 0 ('zero', any n >= 1); times the centred periodic Hann window.
4. ``magnitude_power``:     |X| (1) or re^2 + im^2 (2).
5. ``fmax``:                the Slaney filterbank from fmin to fmax (0: sample_rate / 2); the bin frequencies run to sample_rate / 2.
6. ``ref_level_db``:        S = 20 log10(max(10^(min_level_db / 20), mel)) - ref_level_db.
7. ``max_abs_value`` A:     sym = clip(2 A ((S - min_level_db) / -min_level_db) - A, -A, A), ROUNDED TO float32 (the file Tacotron's
                            preprocessing writes);
8.                          out = clip((sym + A) / (2 A), 0, 1) in float32 (``wavernn_preprocess.py``).
                            A == 0: out = clip((S - min_level_db) / -min_level_db, 0, 1) in ``dtype``, as ``mel_ref``.

``dtype=np.float32`` evaluates steps 1 to 7 in float32 throughout (float32 frames through ``scipy.fft.rfft``); the distance between
the two evaluations is the rounding error of the chain on an input, which the GPU tests scale their tolerance from.
"""
from __future__ import annotations

import numpy as np
import scipy.fft

from tests import condition_ref as cr
from tests import mel_ref as mr

VOCODER = dict(pad_mode='reflect', magnitude_power=1, fmax=0.0, ref_level_db=0.0, preemphasis=0.0, preemph_rescale=0.0, max_abs_value=0.0)
TACOTRON = dict(pad_mode='zero', magnitude_power=2, fmax=7600.0, ref_level_db=20.0, preemphasis=0.97, preemph_rescale=0.999, max_abs_value=4.0)


def mel_basis(sample_rate, n_fft, n_mels, fmin, fmax=0.0):
    """(n_mels, n_fft // 2 + 1) float64; ``fmax == 0`` is ``sample_rate / 2`` and then equals ``mel_ref.mel_basis``."""
    fmax = sample_rate / 2.0 if not fmax else float(fmax)
    fftfreqs = np.linspace(0.0, sample_rate / 2.0, 1 + n_fft // 2)
    mel_f = mr.mel_frequencies(n_mels + 2, fmin, fmax)
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        w[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def frames(n, n_fft, hop_length, pad_mode='zero'):
    least = 1 if pad_mode == 'zero' else n_fft // 2 + 1
    if n < least:
        raise ValueError(f'{n} samples: {pad_mode} padding needs {least}')
    return 1 + n // hop_length


def preemphasised(x, k, r, dtype=np.float64):
    """Steps 1 and 2."""
    x = np.asarray(x, dtype=dtype)
    p = x.copy()
    if k:
        p[1:] = x[1:] - dtype(k) * x[:-1]
    peak = np.max(np.abs(p))
    if r and peak > 0:
        p = p / peak * dtype(r)
    assert p.dtype == dtype
    return p


def stft(p, n_fft, hop_length, win_length, pad_mode, dtype=np.float64):
    """Step 3 and the transform: (n_fft // 2 + 1, T) complex."""
    T = frames(p.size, n_fft, hop_length, pad_mode)
    pp = np.pad(p, n_fft // 2, mode='reflect') if pad_mode == 'reflect' else np.pad(p, n_fft // 2)
    w = mr.padded_window(n_fft, win_length).astype(dtype)
    idx = np.arange(T)[:, None] * hop_length + np.arange(n_fft)[None, :]
    fr = pp[idx] * w[None, :]
    assert fr.dtype == dtype
    return scipy.fft.rfft(fr, axis=1).T


def db_mel(y, sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, n_mels=80, fmin=95.0, min_level_db=-100.0, dtype=np.float64,
           **features):
    """Steps 1 to 6: S (n_mels, T) in ``dtype``; ``features`` are the switches, those left out take today's (``VOCODER``) value."""
    f = dict(VOCODER, **features)
    p = preemphasised(y, f['preemphasis'], f['preemph_rescale'], dtype)
    D = stft(p, n_fft, hop_length, win_length, f['pad_mode'], dtype)
    mag = np.abs(D) if f['magnitude_power'] == 1 else D.real * D.real + D.imag * D.imag
    mel = mel_basis(sample_rate, n_fft, n_mels, fmin, f['fmax']).astype(dtype) @ mag
    floor = dtype(10.0 ** (min_level_db / 20.0))
    S = dtype(20.0) * np.log10(np.maximum(floor, mel)) - dtype(f['ref_level_db'])
    assert S.dtype == dtype
    return S


def symmetric(S, min_level_db, A, dtype=np.float64):
    """Step 7: the [-A, A] values, float32."""
    v = (S - dtype(min_level_db)) / dtype(-min_level_db)
    return np.clip(dtype(2.0 * A) * v - dtype(A), -A, A).astype(np.float32)


def melspectrogram(y, min_level_db=-100.0, dtype=np.float64, **kw):
    """(n_mels, T): float32 where ``max_abs_value`` is on (steps 7 and 8 go through the float32 intermediate), else ``dtype``."""
    S = db_mel(y, min_level_db=min_level_db, dtype=dtype, **kw)
    A = dict(VOCODER, **kw)['max_abs_value']
    if not A:
        out = np.clip((S - dtype(min_level_db)) / dtype(-min_level_db), 0, 1)
        assert out.dtype == dtype
        return out
    sym = symmetric(S, min_level_db, A, dtype)
    out = np.clip((sym + np.float32(A)) / np.float32(2.0 * A), 0, 1)
    assert out.dtype == np.float32
    return out


def error_scale(y, **kw):
    """(ref64 as float64, g): g = max |ref32 - ref64|, the chain's own rounding error on this input."""
    r64 = melspectrogram(y, dtype=np.float64, **kw).astype(np.float64)
    r32 = melspectrogram(y, dtype=np.float32, **kw).astype(np.float64)
    return r64, float(np.abs(r32 - r64).max())


def quantise(x, bits, mu_law):
    """Labels of float samples: ``encode_mu_law`` / ``float_2_label`` (``wavernn/utils/dsp.py:12-15, 92-95``) in float64."""
    mu = 2 ** bits - 1
    xd = np.asarray(x, np.float64)
    if mu_law:
        lab = np.floor((np.sign(xd) * np.log(1 + mu * np.abs(xd)) / np.log(1 + mu) + 1) / 2 * mu + 0.5)
    else:
        lab = (xd + 1.) * mu / 2
    return lab.clip(0, mu).astype(np.int64)


def process_utterance(x, trim_top_db=25.0, peak_target=0.999, bits=10, mu_law=True, dtype=np.float64, **mel_kw):
    """``_process_utterance_v1`` + ``wavernn_preprocess.py:149-159`` for one clip, on ``condition_ref``: trim, rescale, the mel of the
    pre-emphasised clip, the NOT pre-emphasised clip zero-padded on the right to T hop samples and quantised.  The reference
    pre-emphasises the unscaled clip and this chain the scaled one; the two commute up to rounding.
    -> (labels (T hop,) int64, mel (n_mels, T) float32, the conditioned clip float32)."""
    wav = cr.condition(x, trim_top_db, peak_target)[0]
    kw = dict(TACOTRON, **mel_kw)
    mel = melspectrogram(wav, dtype=dtype, **kw)
    hop = kw.get('hop_length', 275)
    out = np.zeros(mel.shape[1] * hop, np.float32)
    out[:wav.shape[0]] = wav
    return quantise(out, bits, mu_law), mel, wav
