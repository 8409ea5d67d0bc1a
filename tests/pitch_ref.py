"""The pitch definitions of ``include/wavernn_amd.h`` in NumPy float64, written from the definitions and not from ``csrc/pitch.hip``: the
YIN track of one clip with, for every frame, the margins of each decision it took, the pair scores from two float32 tracks, and the
seeded fixtures the host and the device tests share.

The device tests demand EQUAL decisions (voicing, the integer lag), which float64 summation-order noise (about 1e-13) cannot flip as
long as every comparison a frame makes is decided by more than that.  ``check_margins`` states the conditions; the host test asserts
them for every frame of every fixture, so no frame is ever excused."""
import math

import numpy as np

DEFAULTS = dict(sample_rate=22050, hop=275, frame_length=2048, window=1024, fmin=60.0, fmax=600.0, threshold=0.15, silence_rms=1e-4,
                gpe_ratio=0.2)
FIELDS = ('f0_rmse_cents', 'gpe', 'vde', 'ffe', 'f0_corr', 'voiced_target', 'voiced_test', 'voiced_both')


def lags(sample_rate, fmin, fmax):
    return math.ceil(sample_rate / fmax), math.floor(sample_rate / fmin)


def frames_of(n, hop):
    return 1 + n // hop if n > 0 else 0


def difference(x, W, tau_hi):
    """d(tau) = sum_{j < W} (x[j] - x[j + tau])^2 for tau = 0 .. tau_hi, the direct form."""
    shifted = np.lib.stride_tricks.sliding_window_view(x, W)[:tau_hi + 1]
    return ((x[:W][None, :] - shifted) ** 2).sum(axis=1)


def cmnd(d):
    """d'(0) = 1, d'(tau) = d(tau) tau / sum_{k <= tau} d(k), 1 wherever that sum is exactly 0."""
    cs = np.cumsum(d[1:])
    tau = np.arange(1, len(d), dtype=np.float64)
    out = np.ones(len(d))
    nz = cs > 0
    out[1:][nz] = d[1:][nz] * tau[nz] / cs[nz]
    return out


def track(wav, **settings):
    """The track of one float32 clip.  Per frame: ``f0``, ``aperiodicity`` (float32, rounded once) and their float64 values ``f0_64``,
    ``aperiodicity_64``; ``voiced``; ``tau`` (the integer lag, -1 without a candidate) and ``off``; and the margins: ``m_threshold`` (the
    least |d'(tau) - threshold| over the lags examined up to the candidate, or over the whole range without one), ``m_descent`` (the
    least |d'(tau + 1) - d'(tau)| over the comparisons of the descent, the stopping one included; inf without one), ``rms`` and ``den``."""
    s = dict(DEFAULTS, **settings)
    sr, hop, FL, W, thr = s['sample_rate'], s['hop'], s['frame_length'], s['window'], s['threshold']
    tau_min, tau_max = lags(sr, s['fmin'], s['fmax'])
    assert 1 <= tau_min <= tau_max and W + tau_max + 1 <= FL
    wav = np.asarray(wav, np.float32)
    n = len(wav)
    T = frames_of(n, hop)
    out = {k: np.zeros(T) for k in ('f0_64', 'aperiodicity_64', 'off', 'm_threshold', 'm_descent', 'rms', 'den')}
    out['tau'] = np.full(T, -1)
    out['voiced'] = np.zeros(T, bool)
    padded = np.zeros(n + 2 * FL + T * hop, np.float64)
    padded[FL:FL + n] = wav
    for t in range(T):
        start = t * hop - FL // 2 + FL
        x = padded[start:start + FL]
        dp = cmnd(difference(x, W, tau_max + 1))
        rng = dp[tau_min:tau_max + 1]
        out['aperiodicity_64'][t] = rng.min()
        rms = math.sqrt((x[:W] ** 2).sum() / W)
        out['rms'][t] = rms
        below = np.flatnonzero(rng < thr)
        out['m_descent'][t] = np.inf
        if below.size == 0:
            out['m_threshold'][t] = np.abs(rng - thr).min()
            continue
        tau = tau_min + int(below[0])
        out['m_threshold'][t] = np.abs(dp[tau_min:tau + 1] - thr).min()
        while tau + 1 <= tau_max:
            out['m_descent'][t] = min(out['m_descent'][t], abs(dp[tau + 1] - dp[tau]))
            if not dp[tau + 1] < dp[tau]:
                break
            tau += 1
        out['tau'][t] = tau
        if not rms >= s['silence_rms']:
            continue
        a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
        den = a - 2 * b + c
        off = 0.5 * (a - c) / den if den > 0 else 0.0
        off = min(max(off, -0.5), 0.5)
        out['voiced'][t], out['den'][t], out['off'][t] = True, den, off
        out['f0_64'][t] = sr / (tau + off)
    out['f0'] = out['f0_64'].astype(np.float32)
    out['aperiodicity'] = out['aperiodicity_64'].astype(np.float32)
    out['settings'] = s
    return out


def check_margins(tr):
    """The conditions under which another float64 summation order takes the same decisions on every frame of a track."""
    s = tr['settings']
    assert (tr['m_threshold'] >= 1e-6).all(), ('threshold', tr['m_threshold'].min())
    assert (tr['m_descent'] >= 1e-9).all(), ('descent', tr['m_descent'].min())
    rms = tr['rms'][tr['rms'] != 0]
    assert s['silence_rms'] == 0 or (np.abs(rms - s['silence_rms']) >= 1e-6 * s['silence_rms']).all(), 'rms'
    assert (tr['den'][tr['voiced']] >= 1e-6).all(), ('den', tr['den'][tr['voiced']].min())


def pair_scores(ft, fs, gpe_ratio=0.2):
    """The summary fields from two float32 tracks of equal length, in float64; ``cents`` per frame (0 outside V) and ``m_gpe``, the
    least | |fs / ft - 1| - gpe_ratio | over V (inf when V is empty)."""
    assert ft.dtype == fs.dtype == np.float32 and ft.shape == fs.shape
    ft, fs = ft.astype(np.float64), fs.astype(np.float64)
    T = len(ft)
    out = dict.fromkeys(FIELDS, 0.0)
    out.update(cents=np.zeros(T), m_gpe=np.inf)
    if T == 0:
        return out
    vt, vs = ft > 0, fs > 0
    V = vt & vs
    nV, n_vde, n_gpe = int(V.sum()), int((vt != vs).sum()), 0
    if nV:
        ratio = fs[V] / ft[V]
        cents = 1200.0 * np.log2(ratio)
        out['cents'][V] = cents
        dev = np.abs(ratio - 1.0)
        n_gpe = int((dev > gpe_ratio).sum())
        out['m_gpe'] = float(np.abs(dev - gpe_ratio).min())
        out['f0_rmse_cents'] = math.sqrt((cents ** 2).sum() / nV)
        out['gpe'] = n_gpe / nV
        if nV >= 2:
            lt, ls = np.log2(ft[V]), np.log2(fs[V])
            a, c = lt - lt.sum() / nV, ls - ls.sum() / nV
            var_t, var_s = (a * a).sum(), (c * c).sum()
            if var_t > 0 and var_s > 0:
                out['f0_corr'] = (a * c).sum() / math.sqrt(var_t * var_s)
    out['vde'] = n_vde / T
    out['ffe'] = (n_gpe + n_vde) / T
    out['voiced_target'], out['voiced_test'], out['voiced_both'] = float(vt.sum()), float(vs.sum()), float(nV)
    return out


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------

def sine(f, n, sr=22050, amp=0.5, phase=0.3):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / sr + phase)).astype(np.float32)


def chirp(f_a, f_b, n, sr=22050, amp=0.5, n_total=None):
    """A linear sweep from ``f_a`` at sample 0 to ``f_b`` at sample ``n_total`` (default ``n``)."""
    t = np.arange(n) / sr
    k = (f_b - f_a) / ((n_total or n) / sr)
    return (amp * np.sin(2 * np.pi * (f_a * t + 0.5 * k * t * t))).astype(np.float32)


def noise(n, amp=0.1, seed=0):
    return (amp * np.random.Generator(np.random.PCG64(seed)).standard_normal(n)).astype(np.float32)


def signal(name, n, sr=22050):
    """A fixture by name; ``sine_<Hz>``, ``detune_<cents>`` and ``chirp_x<factor>`` take their number from the name."""
    t = np.arange(n) / sr
    if name.startswith('sine_') and name != 'sine_noise':
        return sine(float(name[5:]), n, sr)
    if name == 'complex_110':                 # a second harmonic of 5 x the fundamental's power
        return (0.2 * np.sin(2 * np.pi * 110 * t) + 0.2 * math.sqrt(5.0) * np.sin(2 * np.pi * 220 * t + 0.7)).astype(np.float32)
    if name == 'missing_150':                 # 300 / 450 / 600 Hz, no fundamental
        return (0.2 * (np.sin(2 * np.pi * 300 * t) + np.sin(2 * np.pi * 450 * t + 1.0) + np.sin(2 * np.pi * 600 * t + 2.0))).astype(np.float32)
    if name == 'chirp':
        return chirp(100.0, 300.0, n, sr, n_total=6000)
    if name.startswith('chirp_x'):            # the same sweep, every frequency times the factor
        g = float(name[7:])
        return chirp(100.0 * g, 300.0 * g, n, sr, n_total=6000)
    if name == 'am':
        return ((0.3 * (1.0 + 0.5 * np.sin(2 * np.pi * 5 * t))) * np.sin(2 * np.pi * 200 * t)).astype(np.float32)
    if name.startswith('stop_'):              # a 200 Hz sine up to the given sample, silence after it
        x = sine(200.0, n, sr)
        x[int(name[5:]):] = 0
        return x
    if name.startswith('chirpstop_'):
        x = chirp(100.0, 300.0, n, sr, n_total=6000)
        x[int(name[10:]):] = 0
        return x
    if name == 'noise':
        return noise(n, 0.1, 1)
    if name == 'zeros':
        return np.zeros(n, np.float32)
    if name == 'dc':
        return np.full(n, 0.3, np.float32)
    if name == 'sine_noise':                  # 200 Hz with noise 20 dB under it
        return (sine(200.0, n, sr).astype(np.float64) + noise(n, 0.5 / math.sqrt(2) / 10.0, 2)).astype(np.float32)
    raise KeyError(name)


N = 6000
CONFIGS = {
    # lags 37 .. 367: more than one pass of a 256-thread workgroup
    'default': dict(),
    'sr16k': dict(sample_rate=16000, hop=256, frame_length=1024, window=512, fmin=80.0),
    'small': dict(hop=64, frame_length=512, window=256, fmin=200.0),                 # lags 37 .. 110
    'one_block': dict(hop=64, frame_length=512, window=255, fmin=350.0),             # lags 37 .. 63: one block of the running sum
    'long': dict(frame_length=4096, window=1024, fmin=21.6),                         # tau_max 1020
    'edge': dict(frame_length=2048, window=1024, fmin=21.6),                         # window + tau_max + 1 three below frame_length
    'single_lag': dict(window=1022, fmin=220.0, fmax=220.5),                         # lags 100 .. 100
    'hop256': dict(hop=256, window=1021),
}
LENGTHS = (1, 274, 275, 276, 1023, 1025, 2047, 2049, N)     # hop -+ 1, frame_length / 2 -+ 1, frame_length -+ 1
TABLE_SINES = ('sine_60.5', 'sine_100', 'sine_220.5', 'sine_233.3', 'sine_441', 'sine_595')
# (config, signal, n): the clips of one config go to the device as one ragged batch
CASES = (
    [('default', s, N) for s in TABLE_SINES + ('sine_%r' % (22050 / 37), 'sine_%r' % (22050 / 367), 'complex_110', 'missing_150', 'chirp', 'am',
                                               'stop_3100', 'noise', 'zeros', 'dc', 'sine_noise')]
    + [('default', 'chirp', n) for n in LENGTHS[:-1]] + [('default', 'sine_220.5', n) for n in (1, 276, 2049)]
    + [('sr16k', s, N) for s in ('sine_100', 'sine_441', 'chirp', 'noise', 'zeros')] + [('sr16k', 'chirp', n) for n in (255, 256, 257, 511, 513, 1023, 1025)]
    + [('small', s, N) for s in ('sine_233.3', 'sine_441', 'chirp_x2', 'noise', 'dc')] + [('small', 'sine_441', n) for n in (63, 64, 65, 255, 257, 511, 513)]
    + [('one_block', s, N) for s in ('sine_441', 'sine_595', 'noise')]
    + [('long', s, N) for s in ('sine_60.5', 'sine_220.5', 'chirp', 'noise', 'zeros')] + [('long', 'chirp', n) for n in (2047, 2049, 4095, 4097)]
    + [('edge', s, N) for s in ('sine_60.5', 'chirp', 'noise')]
    + [('single_lag', s, N) for s in ('sine_220.5', 'sine_100', 'noise')]
    + [('hop256', s, N) for s in ('sine_233.3', 'chirp', 'am', 'sine_noise')]
)
# (target, test) at the default config and N samples.  The pairs whose correlation is compared are sweeps, or identical: log2 f0 of a
# steady tone varies in its last places only, and the correlation of two such tracks is all rounding.
PAIRS = (
    ('chirp', 'chirp'), ('sine_220.5', 'sine_220.5'), ('zeros', 'zeros'), ('noise', 'noise'),
    ('chirp', 'chirp_x%r' % (2 ** (10 / 1200))), ('chirp', 'chirp_x1.3'),
    ('chirp', 'noise'), ('chirpstop_3100', 'chirpstop_4200'), ('noise', 'zeros'),
)

_cache = {}


def case_track(config, name, n):
    """The restatement's track of a fixture, computed once and shared (never modified) by the tests that need it."""
    key = (config, name, n)
    if key not in _cache:
        s = dict(DEFAULTS, **CONFIGS[config])
        _cache[key] = track(signal(name, n, s['sample_rate']), **s)
    return _cache[key]
