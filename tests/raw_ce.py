"""Chosen fc3 outputs for the RAW cross-entropy loss and its gradient: `ce_rows_kernel` (csrc/losses.hip) and `ce_grad_kernel`
(csrc/train.hip) shown the logits a trained model produces, and the ones that break a careless log-sum-exp, on purpose.

Plain numpy, no oracle, no reference.  The seeded synthetic weights of the rest of the suite give near-uniform logits of size ~0.1: the
maximum, the sum of exponentials and the target's logit are all of one size there, nothing underflows, and any way of writing
`logsumexp(row) - row[y]` is accurate.  Here the rows are written down for any class count NC = 2^bits (seeded noise + the chosen
structure), so the regime of every row is known beforehand (asserted by tests/test_raw_ce_host.py, not assumed):

    uniform      the control: all logits equal (0 and 3.75), and today's regime, N(0, 0.05)
    peaky_hit    one class at 25, the rest N(0, 2); target = that class.  s = sum exp(p - max) rounds to 1 in float32 up to 512
                 classes, the loss is near NC e^-25
    peaky_miss   the same rows; targets 25 to 40 below the maximum, the row's argmin among them: a loss of 25 to 40
    mixed        the same rows; hits and misses 3 to 1 in one call (the mix of the gradient tests), the cycle starting 3 i slots on in
                 row i of P, so that the first few rows of a call already hold a miss
    offset_32, offset_1k, offset_30k
                 the `mixed` and `peaky_miss` rows shifted so that the maximum is 32.3, 1024.3, 30000.3 (rounded to float32 AFTER the
                 shift: the rows are exact float32, a naive exp overflows at the last two); offset_30k also holds the mirror image,
                 maximum -30000.3.  In the peaky rows log s is ~1e-8, so `(m + log s) - p[t]` happens to be exact on them; between
                 them stand spread rows (`_spread_row`: no peak, log s above 0.02) chosen so that rounding m + log s at the spacing
                 of m loses 0.30 ... 0.45 of that spacing, always downwards.  P rows come in threes: mixed, spread, peaky_miss
    underflow    every class but two is 120 to 200 below the maximum (`expf` returns 0) or, in the later rows, 89 to 102 below (a
                 subnormal); targets on the two live classes and on dead ones
    masked       loss only: about a quarter of the logits are -inf, the targets are finite classes.  `masked_target` (not in
                 GROUP_NAMES: a call of its own) puts the targets ON masked classes: +inf, as torch returns
    ties         two classes equal at the maximum (ends of the row; 63 and 64), then all classes equal (7.25, -3.5)

N(0, v) has variance v.  A group is `P` (n_p, NC) float32 and `y` (n_p, K) int64: its rows are all pairs (P[i], y[i, j]).  `P[0]` with
`y[0]` is what the gradient test loads into fc3.bias (one P per call).  Over a group the targets cover class 0, class NC - 1, 63 and
64 where they exist, the argmax and the argmin.  Every value has `+ 0.0f` added: no -0.0 (fc3's `0 + bias` would return +0.0, other bits).

The derived row bound (`row_bound`): a float32 evaluation of `log(s) - (p[t] - m)` rounds p[t] - m once, log(s) to an ulp or two, the
difference once, and carries s's own error -- NC / 64 sequential float32 additions per lane and an `expf` of a few ulp per term -- into
log(s) at no more than its relative size, since s >= 1:

    2^-24 (|p[t] - m| + 2 |log s| + |nll| + NC / 64 + 10)

Nothing in it is measured on a kernel; torch's float32 F.cross_entropy meets it on every row here (the host test).  A mean of rows is
held to the mean of the row bounds plus 2^-24 |mean| for the final rounding (`mean_bound`).
"""
from __future__ import annotations

import functools

import numpy as np

GROUP_NAMES = ('uniform', 'peaky_hit', 'peaky_miss', 'mixed', 'offset_32', 'offset_1k', 'offset_30k', 'underflow', 'masked', 'ties')
OFFSETS = {'offset_32': 32.3, 'offset_1k': 1024.3, 'offset_30k': 30000.3}
K = 20                         # targets per P row
PEAK = 25.0
MISS_GAP = (25.0, 40.0)
DEAD_GAP = (120.0, 200.0)      # expf(-120) = 0 in float32 (the smallest subnormal is e^-103.28)
SUBNORMAL_GAP = (89.0, 102.0)  # e^-87.34 is the smallest normal float32
U24 = 2.0 ** -24


def _f32(rows):
    return np.ascontiguousarray(np.asarray(rows, np.float64).astype(np.float32) + np.float32(0.0))


def _rng(bits, name):
    return np.random.Generator(np.random.PCG64([bits, sum(name.encode()), len(name)]))


def _dedupe(seq, nc, drop=()):
    out = []
    for c in seq:
        c = int(c)
        if 0 <= c < nc and c not in out and c not in drop:
            out.append(c)
    return out


def _cycle(seq, n=K):
    return [seq[i % len(seq)] for i in range(n)]


def _cover(row, nc, extra=()):
    """class 0, NC - 1, 63, 64, the argmax and the argmin of a row (finite entries only), then `extra`."""
    fin = np.where(np.isfinite(row), row, np.nan)
    cand = [0, nc - 1, 63, 64, int(np.nanargmax(fin)), int(np.nanargmin(fin))] + list(extra)
    return _dedupe([c for c in cand if c < nc and np.isfinite(row[c])], nc)


def _peaky(bits):
    """(rows float64 (n_p, NC), peaks, misses): one class at PEAK over N(0, 2); the peak walks over an interior class, 0, NC - 1, 63, 64;
    classes 0, NC - 1, 63, 64 (but the peak) are lowered to 25 ... 40 below it and are, with the row's argmin, its miss targets."""
    nc = 1 << bits
    rng = _rng(bits, 'peaky')
    interior = int(rng.integers(65, nc - 1)) if nc >= 128 else int(rng.integers(0, nc))
    peaks = _dedupe([interior, 0, nc - 1, 63, 64], nc)
    rows, misses = [], []
    for pk in peaks:
        r = rng.normal(0.0, np.sqrt(2.0), size=nc)
        r[pk] = PEAK
        low = _dedupe([0, nc - 1, 63, 64], nc, drop=(pk,))
        for c in low:
            r[c] = PEAK - rng.uniform(*MISS_GAP)
        tmp = r.copy()
        tmp[[pk] + low] = np.inf
        nat = [int(np.argmin(tmp))] if np.isfinite(tmp).any() and tmp.min() <= 0.0 else []   # the lowest class the noise itself gave
        rows.append(r)
        tmp = r.copy()
        tmp[pk] = np.inf
        misses.append(_dedupe(low + nat + [int(np.argmin(tmp))], nc))
    return np.stack(rows), peaks, misses


def _y_hit(peaks):
    return np.array([[pk] * K for pk in peaks], np.int64)


def _y_miss(misses):
    return np.array([_cycle(ms) for ms in misses], np.int64)


def _y_mixed(peaks, misses):
    # row i of P starts its hit, hit, hit, miss cycle 3 i slots on: the first few pairs of a group (P[0], P[1], ...) already hold a miss
    return np.array([[pk if (j + 3 * i) % 4 != 3 else ms[(j // 4) % len(ms)] for j in range(K)]
                     for i, (pk, ms) in enumerate(zip(peaks, misses))], np.int64)


def _spread_row(rng, nc, top):
    """An N(0, 2) row with no peak, shifted so that its maximum is float32(top) and rounded to float32; then its runners-up are moved down
    float by float until the float64 log-sum-exp of the float32 row lies 0.30 ... 0.45 of the maximum's float32 spacing above a multiple
    of that spacing.  log s is above 0.02 here (asserted by the host test), so a float32 `m + log(s)` is rounded at the spacing of m and loses that much, always
    downwards; a form that never adds m to log(s) loses nothing."""
    r = rng.normal(0.0, np.sqrt(2.0), size=nc)
    row = (r - r.max() + top).astype(np.float32)
    m = float(row.max())
    u = float(np.spacing(np.float32(abs(m))))
    order = np.argsort(row)[::-1][1:]                                       # the runners-up that hold 8 % of the row's probability
    prob = np.exp(row[order].astype(np.float64) - m) / np.exp(row.astype(np.float64) - m).sum()
    c = order[:int(np.searchsorted(np.cumsum(prob), 0.08)) + 1]
    for _ in range(100000):
        frac = ((m + np.log(np.exp(row.astype(np.float64) - m).sum())) / u) % 1.0
        if 0.30 <= frac <= 0.45:
            return row.astype(np.float64)
        row[c] = np.nextafter(row[c], np.float32(-np.inf))
    raise AssertionError('no such row')


def _offset_group(name, bits, rows, peaks, misses):
    """P rows in threes -- a `mixed` row, a spread row, a `peaky_miss` row -- at maximum +OFFSETS[name]; offset_30k: then at -OFFSETS."""
    nc = 1 << bits
    rng = _rng(bits, name)
    y_mixed, y_miss = _y_mixed(peaks, misses), _y_miss(misses)
    out_rows, ys, kinds = [], [], []
    for sign in ((1.0, -1.0) if name == 'offset_30k' else (1.0,)):
        for i in range(len(peaks)):
            sp = _spread_row(rng, nc, sign * OFFSETS[name])
            for kind, r, yy in (('mixed', rows[i] + (sign * OFFSETS[name] - PEAK), y_mixed[i]), ('spread', sp, _cycle(_cover(sp, nc))),
                                ('miss', rows[i] + (sign * OFFSETS[name] - PEAK), y_miss[i])):
                out_rows.append(r)
                ys.append(yy)
                kinds.append((kind, sign))
    return _finish(out_rows, ys, nc, kinds)


def _finish(rows, ys, nc, kinds=None):
    P, y = _f32(rows), np.asarray(ys, np.int64)
    assert P.shape == (y.shape[0], nc) and y.shape[1] == K and y.min() >= 0 and y.max() < nc
    P.setflags(write=False)
    y.setflags(write=False)
    return dict(P=P, y=y, kinds=kinds)


@functools.lru_cache(maxsize=None)
def group(name, bits):
    """dict(P (n_p, NC) float32, y (n_p, K) int64) of one group at NC = 2^bits; read-only, shared by every caller."""
    nc = 1 << bits
    rng = _rng(bits, name)
    if name == 'uniform':
        rows = [np.zeros(nc), np.full(nc, 3.75)] + [rng.normal(0.0, np.sqrt(0.05), size=nc) for _ in range(3)]
        ys = [_cycle(_cover(r, nc, extra=rng.integers(0, nc, size=4))) for r in rows]
    elif name in ('peaky_hit', 'peaky_miss', 'mixed') or name in OFFSETS:
        rows, peaks, misses = _peaky(bits)
        if name == 'peaky_hit':
            ys = _y_hit(peaks)
        elif name == 'peaky_miss':
            ys = _y_miss(misses)
        elif name == 'mixed':
            ys = _y_mixed(peaks, misses)
        else:
            return _offset_group(name, bits, rows, peaks, misses)
    elif name == 'underflow':
        rows, ys = [], []
        for gap, (a, b) in ((DEAD_GAP, (0, nc - 1)), (DEAD_GAP, (63 % nc, 64 % nc)), (SUBNORMAL_GAP, (nc // 2, (nc // 2 + 1) % nc)),
                            (SUBNORMAL_GAP, (nc - 1, 0))):
            top = float(rng.uniform(-2.0, 6.0))
            r = top - rng.uniform(*gap, size=nc)
            r[a], r[b] = top, top - 0.7
            dead = _dedupe(_cover(r, nc) + list(rng.integers(0, nc, size=4)), nc, drop=(a, b))
            rows.append(r)
            ys.append(_cycle(_dedupe([a, b], nc) + dead))
    elif name in ('masked', 'masked_target'):
        base, peaks, _ = _peaky(bits)
        rng = _rng(bits, 'masked')                         # both groups: the same rows
        rows, ys = [], []
        for i in range(4):
            pk = peaks[i % len(base)]
            r = base[i % len(base)].copy() if i % 2 else rng.normal(0.0, np.sqrt(2.0), size=nc)
            mask = rng.random(nc) < 0.25
            if nc > 2:
                mask[(nc // 2 + i) % (nc - 2) + 1] = True
            if i % 2:
                mask[pk] = i == 3                          # row 1 keeps its peak, row 3 loses it
            mask[[0, nc - 1][i % 2]] = True                # one end of the row is masked, the other is not
            mask[[nc - 1, 0][i % 2]] = False
            r[mask] = -np.inf
            rows.append(r)
            extra = rng.integers(0, nc, size=6)
            ys.append(_cycle(_cover(r, nc, extra=extra) if name == 'masked' else [int(c) for c in np.flatnonzero(mask)]))
    elif name == 'ties':
        rows = []
        for a, b in ((0, nc - 1), (63 % nc, 64 % nc)):
            r = rng.normal(0.0, np.sqrt(2.0), size=nc)
            r[a] = r[b] = float(np.float32(r.max() + 1.5))
            rows.append(r)
        rows += [np.full(nc, 7.25), np.full(nc, -3.5)]
        ys = [_cycle(_cover(r, nc, extra=[nc - 1, 64 % nc, 1 % nc])) for r in rows]
    else:
        raise KeyError(name)
    return _finish(rows, ys, nc)


def pair_index(g, n_rows=None, first_only=False):
    """(i, j) of the pair (P[i], y[i, j]) each row of rows_of() is: P-row-major, so that a few rows already come from different P."""
    n_p = 1 if first_only else g['P'].shape[0]
    idx = np.arange(n_p * K if n_rows is None else n_rows)
    return idx % n_p, (idx // n_p) % K


def rows_of(g, n_rows=None, first_only=False):
    """(logits (n, NC) float32, y (n,) int64) of a group: the pairs (P[0], y[0, 0]), (P[1], y[1, 0]), ..., (P[0], y[0, 1]), ... repeated
    cyclically up to n_rows; first_only: the pairs of P[0] alone (what the gradient test loads)."""
    i, j = pair_index(g, n_rows, first_only)
    return np.ascontiguousarray(g['P'][i]), np.ascontiguousarray(g['y'][i, j])


def row_terms64(logits, y):
    """float64 m = max, s = sum exp(p - m), p[t], nll = log s - (p[t] - m) of every row, on the float32 inputs as they are."""
    p = np.asarray(logits, np.float64)
    m = p.max(axis=1)
    with np.errstate(under='ignore'):
        s = np.exp(p - m[:, None]).sum(axis=1)
    pt = p[np.arange(p.shape[0]), np.asarray(y)]
    return dict(m=m, s=s, pt=pt, nll=np.log(s) - (pt - m))


def row_bound(logits, y):
    """The derived bound on a float32 evaluation of each row's loss (module docstring), float64 (n,)."""
    t = row_terms64(logits, y)
    return U24 * (np.abs(t['pt'] - t['m']) + 2.0 * np.abs(np.log(t['s'])) + np.abs(t['nll']) + logits.shape[1] / 64.0 + 10.0)


def mean_bound(logits, y):
    """The bound on a float32 mean of the rows' losses: the mean of the row bounds + 2^-24 |mean| for the final rounding."""
    return float(row_bound(logits, y).mean() + U24 * abs(row_terms64(logits, y)['nll'].mean()))
