"""The wav conditioning restated in NumPy float64, and the fixtures the tests of the device path share.

Definition (include/wavernn_amd.h).  For a clip x of n samples, frame_length L, hop h, top_db D:
p = x reflect-padded by L // 2 on both sides, F = 1 + n // h frames, e[f] = mean(p[f h : f h + L] ** 2); frame f is non-silent when
10 log10(max(1e-10, e[f])) - 10 log10(max(1e-10, max e)) > -D; start = first non-silent * h, end = min(n, (last non-silent + 1) * h).
Then peak = max |x[start:end]| and y = x[start:end] / peak * target in float32 (peak == 0: unscaled).
"""
import numpy as np

AMIN = 1e-10


def frame_energies(x, frame_length=2048, hop=512):
    x = np.asarray(x, np.float64)
    n, pad = x.shape[0], frame_length // 2
    if n < pad + 1:
        raise ValueError(f'a clip of {n} samples cannot be reflect-padded by {pad}')
    p = np.pad(x, pad, mode='reflect')
    return np.array([np.mean(p[f * hop:f * hop + frame_length] ** 2) for f in range(1 + n // hop)])


def frame_db(e):
    """Every frame's level relative to the loudest frame, in dB (<= 0)."""
    return 10.0 * np.log10(np.maximum(AMIN, e)) - 10.0 * np.log10(max(AMIN, float(np.max(e))))


def trim_bounds(x, top_db, frame_length=2048, hop=512):
    n = int(np.shape(x)[0])
    loud = np.flatnonzero(frame_db(frame_energies(x, frame_length, hop)) > -float(top_db))
    return int(loud[0]) * hop, min(n, (int(loud[-1]) + 1) * hop)


def margin_db(x, top_db, frame_length=2048, hop=512):
    """The distance of the closest frame from the threshold, in dB."""
    return float(np.min(np.abs(frame_db(frame_energies(x, frame_length, hop)) + float(top_db))))


def scale(x, peak, target):
    """float32: one divide, then one multiply, as NumPy evaluates ``x / peak * target`` on float32 operands."""
    x = np.asarray(x, np.float32)
    if not peak > 0:
        return x.copy()
    return x / np.float32(peak) * np.float32(target)


def condition(x, trim_top_db=None, peak_target=None, frame_length=2048, hop=512):
    """-> (y float32, (start, end), peak float32)."""
    x = np.asarray(x, np.float32)
    start, end = trim_bounds(x, trim_top_db, frame_length, hop) if trim_top_db is not None else (0, x.shape[0])
    cut = x[start:end]
    peak = np.float32(np.max(np.abs(cut))) if cut.size else np.float32(0)
    return (scale(cut, peak, peak_target) if peak_target else cut.copy()), (start, end), peak


# ---------------------------------------------------------------------------------------------------------------- fixtures
WINDOWS = ((2048, 512), (1024, 256), (1000, 300))
MIN_MARGIN_DB = 0.1


def burst_clip(n, lo, hi, floor, seed):
    """A uniform-noise floor of amplitude ``floor`` with one full-band burst (uniform noise of amplitude 0.5) over ``[lo, hi)``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-floor, floor, n)
    x[lo:hi] = rng.uniform(-0.5, 0.5, hi - lo)
    return x.astype(np.float32)


def clear_clip(n, lo, hi, floor, top_db, window=(2048, 512), seed0=0):
    """``burst_clip`` with the first of the 8 seeds from ``seed0`` that keeps every frame MIN_MARGIN_DB from the threshold in the float64
    restatement: what lets a test ask the device for exactly the restatement's bounds."""
    for seed in range(seed0, seed0 + 8):
        x = burst_clip(n, lo, hi, floor, seed)
        if margin_db(x, top_db, *window) >= MIN_MARGIN_DB:
            return x
    raise AssertionError(f'no seed keeps n={n} [{lo}, {hi}) top_db={top_db} window={window} {MIN_MARGIN_DB} dB from the threshold')


def _spans(n):
    """where -> (lo, hi) of the burst.  In a clip of 4096 samples or more (under the 2048 / 512 window) 'mid' is trimmed at both ends,
    'tail' (the burst touches sample n - 1, so the end is clamped to n) at the start only, 'head' (it touches sample 0, so frame 0's
    energy comes through the reflection) at the end only, 'full' not at all; a shorter clip has too few frames for all of that, and
    what is trimmed there is whatever the restatement says."""
    if n < 4096:
        return {'tail': (n - 300, n), 'head': (0, 300), 'full': (0, n)}
    return {'mid': (n // 2 - n // 8, n // 2 + n // 8), 'tail': (n - n // 4, n), 'head': (0, n // 4), 'full': (0, n)}


def trim_kind(x, top_db, frame_length=2048, hop=512):
    start, end = trim_bounds(x, top_db, frame_length, hop)
    return {(True, True): 'both', (True, False): 'start', (False, True): 'end', (False, False): 'none'}[(start > 0, end < np.shape(x)[0])]


LENGTHS = (1025, 2047, 2048, 2049, 5119, 5120, 5121, 6000, 12345)
TOP_DBS = (10.0, 25.0, 60.0)


def _make_cases():
    """(name, clip, top_db, frame_length, hop) for every GPU case, each a ``clear_clip``."""
    cases = []

    def add(n, where, span, top_db, window):
        floor = 1e-5 if top_db >= 60.0 and where != 'full' else 1e-3
        x = clear_clip(n, span[0], span[1], floor, top_db, window, 1000 * len(cases))
        cases.append((f'n{n}_{where}_db{int(top_db)}_w{window[0]}', x, top_db, window[0], window[1]))

    for n in LENGTHS:                                       # every length, every kind it has room for, the reference's window, 25 dB
        for kind, span in _spans(n).items():
            add(n, kind, span, 25.0, WINDOWS[0])
    for top_db in (10.0, 60.0):                             # the other thresholds: every kind, on one length either side of a hop multiple
        for n in (5119, 5121, 12345):
            for kind, span in _spans(n).items():
                add(n, kind, span, top_db, WINDOWS[0])
    for window in WINDOWS[1:]:                              # the other windows, frame_length % hop != 0 among them
        for n in (1025, 5120, 6000, 12345):
            for kind, span in _spans(n).items():
                add(n, kind, span, 25.0, window)
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _make_cases()
    return _CASES
