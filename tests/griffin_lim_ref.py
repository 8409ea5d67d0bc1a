"""NumPy restatement of Griffin-Lim as ``wrnn_griffin_lim`` defines it (``include/wavernn_amd.h``), the yardstick of the Griffin-Lim tests.

Written from the header's formulas, which follow ``inv_mel_spectrogram`` of ``tacotron/datasets/audio.py`` with librosa's ``stft`` /
``istft`` semantics; librosa is not a dependency of this repository and nothing here has been compared with it
(``tests/test_griffin_lim_host.py`` pins the restatement with analytic checks instead).  The basis, the window and the framing are those
of ``tests/mel_ref.py`` / ``tests/taco_mel_ref.py``, the device-drawn phases those of ``tests/philox_ref.py``.

For one [0, 1] mel ``(n_mels, T)`` under a feature profile (``taco_mel_ref.TACOTRON`` / ``VOCODER``):

a. ``mel_to_magnitude``: A = max_abs_value > 0: sym = clip(2 A m - A, -A, A), S_db = (sym + A) (-min_level_db) / (2 A) + min_level_db;
   A == 0: S_db = clip(m, 0, 1) (-min_level_db) + min_level_db; a = 10^((S_db + ref_level_db) / 20); a^(1 / magnitude_power);
   lin = max(1e-10, pinv(basis) a); S = lin^power.
b. first round: y = istft(S exp(2 pi i r)).
c. every further round: X = stft(y); u = X / |X|, 1 where |X| == 0; y = istft(S u).
d. ``deemphasis``: out[i] = y[i] + k out[i-1].

``stft``: frame t reads y at t hop - n_fft/2 + i under the centred periodic Hann window, zeros or numpy's reflection outside the clip.
``istft``: irfft of every frame times the window, overlap-added in ascending frame order, divided by the window-sum-square where that
exceeds float32's ``tiny``, cut to the ``hop (T - 1)`` samples behind the first ``n_fft / 2``; one frame gives an empty clip.

Every stage takes a ``dtype``.  ``np.float32`` evaluates it in single precision throughout -- the transforms included (``scipy.fft`` on
float32 / complex64 input stays in single precision), as librosa returns complex64 / float32 -- and the distance between the two
evaluations is the chain's own rounding error on an input, which the GPU tests scale their tolerance from.
"""
from __future__ import annotations

import numpy as np
import scipy.fft
import scipy.signal

from tests import mel_ref as mr
from tests import philox_ref
from tests import taco_mel_ref as tm

N_FFT = 2048
CFG = dict(sample_rate=22050, n_fft=N_FFT, hop_length=275, win_length=1100, n_mels=80, fmin=95.0, min_level_db=-100.0)
TINY = float(np.finfo(np.float32).tiny)


def pinv_basis(sample_rate=22050, n_fft=N_FFT, n_mels=80, fmin=95.0, fmax=0.0):
    """(n_fft // 2 + 1, n_mels) float64: ``numpy.linalg.pinv`` of the restated filterbank."""
    return np.linalg.pinv(tm.mel_basis(sample_rate, n_fft, n_mels, fmin, fmax))


def mel_to_magnitude(mel, power=1.5, sample_rate=22050, n_fft=N_FFT, n_mels=80, fmin=95.0, min_level_db=-100.0, dtype=np.float64, **features):
    """Step a: (n_mels, T) in [0, 1] -> S (n_fft // 2 + 1, T) in ``dtype``."""
    f = dict(tm.VOCODER, **features)
    m = np.asarray(mel, dtype=dtype)
    A, lo = f['max_abs_value'], dtype(min_level_db)
    if A:
        sym = np.clip(dtype(2.0 * A) * m - dtype(A), dtype(-A), dtype(A))
        S_db = (sym + dtype(A)) * -lo / dtype(2.0 * A) + lo
    else:
        S_db = np.clip(m, dtype(0), dtype(1)) * -lo + lo
    a = np.power(dtype(10.0), (S_db + dtype(f['ref_level_db'])) / dtype(20.0))
    if f['magnitude_power'] == 2:
        a = np.sqrt(a)
    lin = np.maximum(dtype(1e-10), pinv_basis(sample_rate, n_fft, n_mels, fmin, f['fmax']).astype(dtype) @ a)
    S = np.power(lin, dtype(power))
    assert S.dtype == dtype
    return S


def stft(y, hop_length=275, win_length=1100, pad_mode='zero', n_fft=N_FFT, dtype=np.float64):
    """(n_fft // 2 + 1, T) complex, T = 1 + n // hop; an empty clip has its one frame of zeros."""
    y = np.asarray(y, dtype=dtype)
    T = 1 + y.size // hop_length
    if y.size == 0:
        return np.zeros((n_fft // 2 + 1, 1), np.complex64 if dtype == np.float32 else np.complex128)
    yp = np.pad(y, n_fft // 2, mode='reflect') if pad_mode == 'reflect' else np.pad(y, n_fft // 2)
    w = mr.padded_window(n_fft, win_length).astype(dtype)
    idx = np.arange(T)[:, None] * hop_length + np.arange(n_fft)[None, :]
    fr = yp[idx] * w[None, :]
    assert fr.dtype == dtype
    return scipy.fft.rfft(fr, axis=1).T


def window_sumsquare(T, hop_length=275, win_length=1100, n_fft=N_FFT, dtype=np.float64):
    """(n_fft + hop (T - 1),): the squared window summed over the frames that cover each position of the padded signal."""
    w2 = mr.padded_window(n_fft, win_length).astype(dtype) ** 2
    out = np.zeros(n_fft + hop_length * (T - 1), dtype)
    for t in range(T):
        out[t * hop_length:t * hop_length + n_fft] += w2
    return out


def istft(D, hop_length=275, win_length=1100, n_fft=N_FFT, dtype=np.float64):
    """(n_fft // 2 + 1, T) complex -> (hop (T - 1),) in ``dtype``."""
    D = np.asarray(D, dtype=np.complex64 if dtype == np.float32 else np.complex128)
    T = D.shape[1]
    w = mr.padded_window(n_fft, win_length).astype(dtype)
    fr = scipy.fft.irfft(D.T, n=n_fft, axis=1) * w[None, :]
    assert fr.dtype == dtype
    y = np.zeros(n_fft + hop_length * (T - 1), dtype)
    for t in range(T):
        y[t * hop_length:t * hop_length + n_fft] += fr[t]
    wss = window_sumsquare(T, hop_length, win_length, n_fft, dtype)
    nz = wss > TINY
    y[nz] /= wss[nz]
    return y[n_fft // 2:n_fft // 2 + hop_length * (T - 1)]


def unit_phase(X):
    """X / |X|, 1 where |X| == 0 (``np.exp(1j * np.angle(0))``)."""
    mag = np.abs(X)
    safe = np.where(mag > 0, mag, 1).astype(mag.dtype)
    return np.where(mag > 0, X / safe, 1).astype(X.dtype)


def first_phase(r, dtype=np.float64):
    """exp(2 pi i r) for r (T, bins) -> (bins, T) complex in ``dtype``'s precision."""
    ang = dtype(2.0 * np.pi) * np.asarray(r, dtype=dtype).T
    return (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64 if dtype == np.float32 else np.complex128)


def griffin_lim(S, r, n_iter, hop_length=275, win_length=1100, pad_mode='zero', n_fft=N_FFT, dtype=np.float64, keep=()):
    """Steps b and c: S (bins, T), r (T, bins) in [0, 1) -> the wave after ``n_iter`` rounds, not de-emphasised; with ``keep`` (round
    numbers, 0 = the first istft) a dict round -> wave instead."""
    S = np.asarray(S, dtype=dtype)
    kw = dict(hop_length=hop_length, win_length=win_length, n_fft=n_fft, dtype=dtype)
    y = istft(S * first_phase(r, dtype), **kw)
    kept = {0: y} if 0 in keep else {}
    for i in range(1, n_iter + 1):
        y = istft(S * unit_phase(stft(y, pad_mode=pad_mode, **kw)), **kw)
        if i in keep:
            kept[i] = y
    assert y.dtype == dtype
    return kept if keep else y


def deemphasis(x, k, dtype=np.float64):
    """Step d.  float64: ``scipy.signal.lfilter([1], [1, -k], x)``.  float32: the sequential recurrence, every product and sum rounded."""
    if not k or len(x) == 0:
        return np.asarray(x, dtype=dtype).copy()
    if dtype == np.float64:
        return scipy.signal.lfilter([1.0], [1.0, -float(k)], np.asarray(x, np.float64))
    x = np.asarray(x, np.float32)
    out = np.empty_like(x)
    prev, k32 = np.float32(0), np.float32(k)
    for i in range(x.size):
        prev = out[i] = x[i] + k32 * prev
    return out


def library_k(features):
    """The de-emphasis coefficient the library uses: the float32 field of ``wrnn_mel_features``, the k the mel kernel pre-emphasised with."""
    return float(np.float32(dict(tm.VOCODER, **features)['preemphasis']))


def reconstruct(mel, r, n_iter, power=1.5, dtype=np.float64, keep=(), deemph=True, **cfg):
    """The whole chain for one mel; ``cfg``: the ``CFG`` names and the profile's fields.  ``keep``: as ``griffin_lim``."""
    c = dict(CFG, **{k: v for k, v in cfg.items() if k in CFG})
    features = {k: v for k, v in cfg.items() if k not in CFG}
    f = dict(tm.VOCODER, **features)
    S = mel_to_magnitude(mel, power, c['sample_rate'], c['n_fft'], c['n_mels'], c['fmin'], c['min_level_db'], dtype, **features)
    out = griffin_lim(S, r, n_iter, c['hop_length'], c['win_length'], f['pad_mode'], c['n_fft'], dtype, keep)
    k = library_k(features) if deemph else 0.0
    return {i: deemphasis(y, k, dtype) for i, y in out.items()} if keep else deemphasis(out, k, dtype)


def error_scale(mel, r, n_iter, keep=(), **kw):
    """(ref64, g) -- or dicts round -> those with ``keep`` --: g = max |ref32 - ref64|, the chain's own rounding error on this input."""
    r64 = reconstruct(mel, r, n_iter, dtype=np.float64, keep=keep, **kw)
    r32 = reconstruct(mel, r, n_iter, dtype=np.float32, keep=keep, **kw)
    if keep:
        return r64, {i: float(np.abs(r32[i].astype(np.float64) - r64[i]).max()) if r64[i].size else 0.0 for i in r64}
    return r64, float(np.abs(r32.astype(np.float64) - r64).max()) if r64.size else 0.0


def philox_phases(seed, clip, T, n_bins=N_FFT // 2 + 1):
    """(T, n_bins) float32: the r of WRNN_GRIFFIN_PHASE_PHILOX for clip ``clip`` of a call: step = frame, row = clip, element = bin."""
    return philox_ref.philox_uniform_at(int(seed), np.arange(T, dtype=np.uint64), [clip], n_bins)[:, 0, :]


def harmonic_chirp(n, seed=0, sample_rate=22050):
    """Seeded harmonics of a rising pitch with decaying amplitudes plus 0.5 % white noise, peak about 0.5: energy in every mel band."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / sample_rate
    f0 = rng.uniform(90.0, 140.0) * (1.0 + rng.uniform(0.5, 1.5) * t)
    ph = 2 * np.pi * np.cumsum(f0) / sample_rate
    y = sum(np.sin(h * ph + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 40))
    y = 0.5 * y / np.abs(y).max() + 0.005 * rng.standard_normal(n)
    return y.astype(np.float32)


def spectral_convergence(y, S, hop_length=275, win_length=1100, pad_mode='zero'):
    """|| |stft(y)| - S || / || S ||."""
    return float(np.linalg.norm(np.abs(stft(y, hop_length, win_length, pad_mode)) - S) / np.linalg.norm(S))
