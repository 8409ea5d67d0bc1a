"""Float64 NumPy restatement of the reference's mel front end, the yardstick of the mel tests (as ``philox_ref`` is for the noise).

``melspectrogram(y) = normalize(amp_to_db(mel_basis @ |stft(y)|))`` of ``wavernn/utils/dsp.py:41-43, 50-51, 58-59, 72-81`` with the
librosa semantics of the reference's era, written out from their definitions (librosa itself is not a dependency of this
repository, and this restatement has not been compared with it; ``tests/test_mel_host.py`` pins it with analytic checks instead):

* ``stft``: ``center=True`` reflect padding of ``n_fft // 2``, the periodic Hann window of ``win_length``
  (``scipy.signal.get_window('hann', win_length, fftbins=True)``) zero-padded to ``n_fft`` with ``(n_fft - win_length) // 2`` on the
  left, ``1 + n // hop`` frames, ``n_fft // 2 + 1`` bins;
* ``mel_basis``: Slaney scale (``htk=False``), ``fmax = sr / 2``, triangles between ``n_mels + 2`` mel-spaced edges, every row scaled by
  ``2 / (f[i + 2] - f[i])``;
* ``amp_to_db``: ``20 log10(max(1e-5, .))``; ``normalize``: ``clip((S - min_level_db) / -min_level_db, 0, 1)``.  ``ref_level_db`` is
  not subtracted (only ``spectrogram`` does that).

``dtype=np.float32`` evaluates the same chain in the arithmetic the reference itself runs (``librosa.stft`` returns complex64):
float32 frames through ``scipy.fft.rfft``, float32 filterbank product, float32 logarithm.  The distance between the two is the
reference's own rounding error on an input, which the GPU parity test scales its tolerance from.
"""
from __future__ import annotations

import numpy as np
import scipy.fft
import scipy.signal

DEFAULT = dict(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, n_mels=80, fmin=95.0, min_level_db=-100.0)

F_SP = 200.0 / 3.0
MIN_LOG_HZ = 1000.0
MIN_LOG_MEL = MIN_LOG_HZ / F_SP          # 15
LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= MIN_LOG_HZ, MIN_LOG_MEL + np.log(np.maximum(f, 1e-300) / MIN_LOG_HZ) / LOGSTEP, f / F_SP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= MIN_LOG_MEL, MIN_LOG_HZ * np.exp(LOGSTEP * (m - MIN_LOG_MEL)), F_SP * m)


def mel_frequencies(n, fmin, fmax):
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n))


def mel_basis(sample_rate, n_fft, n_mels, fmin):
    """(n_mels, n_fft // 2 + 1) float64."""
    fmax = sample_rate / 2.0
    fftfreqs = np.linspace(0.0, fmax, 1 + n_fft // 2)
    mel_f = mel_frequencies(n_mels + 2, fmin, fmax)
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def window(win_length):
    return scipy.signal.get_window('hann', win_length, fftbins=True).astype(np.float64)


def padded_window(n_fft, win_length):
    w = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = window(win_length)
    return w


def twiddles(n_fft):
    """(n_fft, 2) float64: cos and -sin of 2 pi k / n_fft."""
    ang = 2.0 * np.pi * np.arange(n_fft) / n_fft
    return np.stack([np.cos(ang), -np.sin(ang)], axis=1)


def frames(n, n_fft, hop_length):
    if n < n_fft // 2 + 1:
        raise ValueError(f'{n} samples cannot be reflect-padded by {n_fft // 2}')
    return 1 + n // hop_length


def stft(y, n_fft, hop_length, win_length, dtype=np.float64):
    """(n_fft // 2 + 1, T) complex; every step in ``dtype``."""
    y = np.asarray(y, dtype=dtype)
    T = frames(y.size, n_fft, hop_length)
    yp = np.pad(y, n_fft // 2, mode='reflect')
    w = padded_window(n_fft, win_length).astype(dtype)
    idx = np.arange(T)[:, None] * hop_length + np.arange(n_fft)[None, :]
    fr = yp[idx] * w[None, :]
    assert fr.dtype == dtype
    return scipy.fft.rfft(fr, axis=1).T


def melspectrogram(y, sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, n_mels=80, fmin=95.0, min_level_db=-100.0,
                   dtype=np.float64):
    """(n_mels, T) in ``dtype``."""
    D = stft(y, n_fft, hop_length, win_length, dtype)
    basis = mel_basis(sample_rate, n_fft, n_mels, fmin).astype(dtype)
    S = basis @ np.abs(D)
    S = dtype(20.0) * np.log10(np.maximum(dtype(1e-5), S))
    out = np.clip((S - dtype(min_level_db)) / dtype(-min_level_db), 0, 1)
    assert out.dtype == dtype
    return out


def sparse_rows(basis32):
    """(rows (n_mels, 3) int32 = first_bin, n_bins, offset; packed weights) of a float32 filterbank, the device layout."""
    rows, packed = [], []
    off = 0
    for r in basis32:
        nz = np.flatnonzero(r)
        first, nb = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        rows.append((first, nb, off))
        packed.append(r[first:first + nb])
        off += nb
    return np.asarray(rows, np.int32), np.concatenate(packed).astype(np.float32)


def speech_like(n, seed=0, sample_rate=22050):
    """Harmonics of a gliding pitch under a slow envelope plus 1 % white noise: every bin of every frame carries energy well inside
    float32's dynamic range of the frame's peak (a pure tone does not: its far bins sit below it)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / sample_rate
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 1.5 * t)
    ph = 2 * np.pi * np.cumsum(f0) / sample_rate
    y = sum(np.sin(h * ph + 0.7 * h) / h for h in range(1, 30))
    y *= 0.02 * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t + 0.3))
    y += 0.01 * 0.02 * rng.standard_normal(n)
    return y.astype(np.float32)


def white(n, rms, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rms * rng.standard_normal(n)).astype(np.float32)
