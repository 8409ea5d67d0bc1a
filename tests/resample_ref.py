"""Float64 NumPy restatement of the resampler, the yardstick of the resampler tests (as ``mel_ref`` is for the mel front end).

For integer rates ``src -> dst``: ``g = gcd(src, dst)``, ``p = dst / g``, ``q = src / g``, ``scale = min(1, p / q)``,
``half = ceil(64 / scale)``.  Output ``t`` sits at input time ``t q / p``: ``n = (t q) // p``, ``r = (t q) % p`` in integers, and

    y[t] = sum_{j = -half + 1 .. half} h(j - r / p) x[n + j],      x = 0 outside [0, n_in),   n_out = ceil(n_in p / q)

    h(u) = scale * rolloff * sinc(rolloff v) * I0(beta sqrt(1 - (v / 64)^2)) / I0(beta)   for v = scale |u| < 64, else 0

with ``rolloff = 0.9475937167399596`` and ``beta = 14.769656459379492``, the ``kaiser_best`` parameters (64 zero crossings).  The filter
is evaluated at every tap position (no table, no interpolation); neither librosa nor resampy is a dependency of this repository and this
restatement has not been compared with them: ``tests/test_resample_host.py`` pins it with analytic checks (DC gain, passband sines,
stopband tones) instead.

``dtype=np.float32`` rounds the bank and the clip to float32 and accumulates every output in float32 (``np.dot`` of float32 vectors): the
distance to the float64 evaluation is the rounding error of a float32 resampler on that input, which the GPU test scales its tolerance
from.  ``start`` / ``stop`` evaluate a range of outputs only.
"""
from __future__ import annotations

import math

import numpy as np

ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492


def plan(src, dst):
    """(p, q, scale, half) with Python integers."""
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1:
        raise ValueError('rates must be positive')
    g = math.gcd(src, dst)
    p, q = dst // g, src // g
    half = ZEROS if p >= q else -((-ZEROS * q) // p)     # ceil(64 / scale) in integers
    return p, q, min(1.0, p / q), half


def out_len(n_in, src, dst):
    p, q, _, _ = plan(src, dst)
    return -((-int(n_in) * p) // q)


def h(u, scale):
    """The filter at real offsets ``u`` (float64 array)."""
    v = scale * np.abs(np.asarray(u, np.float64))
    inside = v < ZEROS
    w = np.where(inside, v / ZEROS, 0.0)
    out = scale * ROLLOFF * np.sinc(ROLLOFF * v) * np.i0(BETA * np.sqrt(1.0 - w * w)) / np.i0(BETA)
    return np.where(inside, out, 0.0)


def bank(src, dst):
    """(p, 2 half) float64: row r holds h(j - r / p) for j = -half + 1 .. half."""
    p, q, scale, half = plan(src, dst)
    j = np.arange(-half + 1, half + 1, dtype=np.float64)[None, :]
    r = np.arange(p, dtype=np.float64)[:, None]
    return h(j - r / p, scale)


def resample(x, src, dst, dtype=np.float64, start=0, stop=None, _bank=None):
    """Outputs ``start .. stop`` (default: all ``n_out``) of the clip ``x`` in ``dtype``."""
    p, q, scale, half = plan(src, dst)
    x = np.asarray(x)
    n_in = x.shape[0]
    n_out = out_len(n_in, src, dst)
    stop = n_out if stop is None else min(int(stop), n_out)
    start = max(int(start), 0)
    B = (bank(src, dst) if _bank is None else _bank).astype(dtype)
    out = np.zeros(max(stop - start, 0), dtype)
    if not out.size:
        return out
    # the part of the clip these outputs can touch, zero-padded on both sides
    lo = (start * q) // p - half + 1
    hi = ((stop - 1) * q) // p + half
    seg = np.zeros(hi - lo + 1, dtype)
    a, b = max(lo, 0), min(hi + 1, n_in)
    if b > a:
        seg[a - lo:b - lo] = x[a:b].astype(dtype)
    for i, t in enumerate(range(start, stop)):
        n, r = divmod(t * q, p)                            # Python integers: no overflow
        k0 = n - half + 1 - lo
        out[i] = np.dot(B[r], seg[k0:k0 + 2 * half])
    assert out.dtype == dtype
    return out
