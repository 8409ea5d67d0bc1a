"""Float64 NumPy / SciPy restatement of the spectral scores (``csrc/score.hip``), the yardstick of the score tests.

Written out from the definitions in ``include/wavernn_amd.h``; the mel is ``tests/mel_ref.py``'s (``tests/taco_mel_ref.py`` for a
feature profile, which builds on it), the framing of the STFT scores is ``mel_ref.stft``'s.  For a target clip ``a`` and a test clip
``b`` over their first ``n = min(len a, len b)`` samples:

* ``D = (Ma - Mb) (-min_level_db)``; ``lsd_t = sqrt(mean_m D^2)``; ``mcd_t = (10 / ln 10) sqrt(2 sum_{k=1..K} c[k, t]^2)`` with
  ``c = C (D ln 10 / 20)`` and ``C`` the orthonormal DCT-II without its row 0;
* per resolution ``(n_fft, hop, win)``: ``A = sqrt(max(re^2 + im^2, floor))`` of the target, ``B`` of the test, ``num_t = sum_k (B - A)^2``,
  ``den_t = sum_k A^2``, ``lm_t = sum_k |ln A - ln B|``;
* ``mel_lsd_db``, ``mcd_db`` = the means over the frames; ``sc = sqrt(sum num) / sqrt(sum den)``; ``logmag = sum lm / (frames bins)``;
  ``mr_sc``, ``mr_logmag`` = the means over the resolutions.

``dtype=np.float32`` evaluates the same per-frame chain in float32 (float32 frames through ``scipy.fft.rfft``, float32 sums and
logarithms); the distance between the two is the chain's own rounding error on an input, which the GPU parity test scales its tolerance
from.  The summaries are always float64 sums of the per-frame values.
"""
from __future__ import annotations

import numpy as np

from tests import mel_ref as mr
from tests import taco_mel_ref as tm

DEFAULT_RESOLUTIONS = ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200))
MAG_FLOOR = 1e-7
MCD_ORDER = 13
N_FFTS = (256, 512, 1024, 2048)


def dct_matrix(n_mels, K):
    """(K, n_mels) float64: rows 1 .. K of the orthonormal DCT-II."""
    k = np.arange(1, K + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (m + 0.5) / n_mels)


def min_samples(resolutions, mel_n_fft=2048, pad_mode='reflect'):
    return max([r[0] // 2 + 1 for r in resolutions] + [mel_n_fft // 2 + 1 if pad_mode == 'reflect' else 1])


def pair(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n = min(a.size, b.size)
    return a[:n], b[:n], n


def magnitudes(y, n_fft, hop, win, floor=MAG_FLOOR, dtype=np.float64):
    """(bins, T) in ``dtype``: ``sqrt(max(re^2 + im^2, floor))``."""
    D = mr.stft(y, n_fft, hop, win, dtype)
    p = D.real * D.real + D.imag * D.imag
    out = np.sqrt(np.maximum(p, dtype(floor)))
    assert out.dtype == dtype
    return out


def stft_frames(a, b, n_fft, hop, win, floor=MAG_FLOOR, dtype=np.float64):
    """dict of ``num``, ``den``, ``lm``: (T,) arrays in ``dtype``."""
    a, b, _ = pair(a, b)
    A, B = magnitudes(a, n_fft, hop, win, floor, dtype), magnitudes(b, n_fft, hop, win, floor, dtype)
    d = B - A
    out = dict(num=(d * d).sum(axis=0), den=(A * A).sum(axis=0), lm=np.abs(np.log(A) - np.log(B)).sum(axis=0))
    assert all(v.dtype == dtype for v in out.values())
    return out


def mel(y, cfg=None, features=None, dtype=np.float64):
    cfg = dict(mr.DEFAULT, **(cfg or {}))
    if not features or features == tm.VOCODER:
        return mr.melspectrogram(y, **cfg, dtype=dtype)
    return tm.melspectrogram(y, dtype=dtype, **cfg, **features)


def mel_frames(a, b, cfg=None, features=None, mcd_order=MCD_ORDER, dtype=np.float64):
    """dict of ``lsd``, ``mcd``: (T,) arrays in ``dtype``."""
    a, b, _ = pair(a, b)
    c = dict(mr.DEFAULT, **(cfg or {}))
    Ma, Mb = mel(a, cfg, features, dtype).astype(dtype), mel(b, cfg, features, dtype).astype(dtype)
    D = (Ma - Mb) * dtype(-c['min_level_db'])
    lsd = np.sqrt((D * D).mean(axis=0))
    C = dct_matrix(c['n_mels'], mcd_order).astype(dtype)
    cep = C @ (D * dtype(np.log(10.0) / 20.0))
    mcd = dtype(10.0 / np.log(10.0)) * np.sqrt(dtype(2.0) * (cep * cep).sum(axis=0))
    assert lsd.dtype == dtype and mcd.dtype == dtype
    return dict(lsd=lsd, mcd=mcd)


def summarise(lsd, mcd, stft, resolutions):
    """The float64 summaries of given per-frame values: ``stft`` a list of dicts with ``num``, ``den``, ``lm``."""
    f64 = lambda v: np.asarray(v, np.float64)
    out = dict(mel_lsd_db=float(f64(lsd).mean()), mcd_db=float(f64(mcd).mean()), stft=[])
    for (n_fft, hop, win), q in zip(resolutions, stft):
        T = len(q['num'])
        out['stft'].append(dict(n_fft=n_fft, hop=hop, win=win, frames=T, sc=float(np.sqrt(f64(q['num']).sum()) / np.sqrt(f64(q['den']).sum())),
                                logmag=float(f64(q['lm']).sum() / (T * (n_fft // 2 + 1)))))
    out['mr_sc'] = float(np.mean([s['sc'] for s in out['stft']]))
    out['mr_logmag'] = float(np.mean([s['logmag'] for s in out['stft']]))
    return out


def score(a, b, resolutions=DEFAULT_RESOLUTIONS, cfg=None, features=None, mcd_order=MCD_ORDER, mag_floor=MAG_FLOOR, dtype=np.float64):
    """The dict ``SpectralScore.score(..., per_frame=True)`` returns for one pair, every per-frame value in ``dtype``."""
    a, b, n = pair(a, b)
    c = dict(mr.DEFAULT, **(cfg or {}))
    pad_mode = (features or tm.VOCODER).get('pad_mode', 'reflect')
    least = min_samples(resolutions, c['n_fft'], pad_mode)
    if n < least:
        raise ValueError(f'{n} samples: at least {least} are needed')
    m = mel_frames(a, b, cfg, features, mcd_order, dtype)
    st = [stft_frames(a, b, *r, floor=mag_floor, dtype=dtype) for r in resolutions]
    out = summarise(m['lsd'], m['mcd'], st, resolutions)
    out.update(n=n, lsd=m['lsd'], mcd=m['mcd'])
    for s, q in zip(out['stft'], st):
        s.update(q)
    return out


def per_frame_quantities(s):
    """name -> array for every per-frame quantity of a score dict: ``lsd``, ``mcd``, ``num/<n_fft>`` ..."""
    out = dict(lsd=s['lsd'], mcd=s['mcd'])
    for r in s['stft']:
        for q in ('num', 'den', 'lm'):
            out[f"{q}/{r['n_fft']}"] = r[q]
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

def mu_law_round_trip(y, bits=10):
    """Encode to ``2**bits`` mu-law classes and decode again, in float64."""
    mu = 2 ** bits - 1
    y = np.clip(np.asarray(y, np.float64), -1.0, 1.0)
    lab = np.floor((np.sign(y) * np.log1p(mu * np.abs(y)) / np.log1p(mu) + 1.0) / 2.0 * mu + 0.5)
    x = 2.0 * lab / mu - 1.0
    return (np.sign(x) / mu * ((1.0 + mu) ** np.abs(x) - 1.0)).astype(np.float32)


PAIR_NAMES = ('noise', 'mulaw', 'scaled')


def parity_pair(name, n):
    """The parity inputs: white noise against itself plus 30 % noise; a harmonic speech-like clip against its 10-bit mu-law round trip;
    the same clip against 0.7 clip + noise.  The speech-like clip is scaled up so that mu-law resolves it."""
    if name == 'noise':
        a = mr.white(n, 0.1, 11)
        return a, (a + 0.3 * mr.white(n, 0.1, 12)).astype(np.float32)
    a = (20.0 * mr.speech_like(n, 13)).astype(np.float32)
    if name == 'mulaw':
        return a, mu_law_round_trip(a)
    if name == 'scaled':
        return a, (0.7 * a + mr.white(n, 0.01, 14)).astype(np.float32)
    raise KeyError(name)
