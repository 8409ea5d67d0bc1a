"""Float64 NumPy restatement of the time alignment (``csrc/align.hip``), the yardstick of the alignment tests.

Written out from the definitions in ``include/wavernn_amd.h``; the mel is ``tests/score_ref.mel`` (either feature profile), the DCT is
``tests/score_ref.dct_matrix``.  For a target clip ``a`` and a test clip ``b``, which need not be equally long:

* ``ca = (C Ma) (-min_level_db) ln 10 / 20`` with ``C`` rows 1 .. K of the orthonormal DCT-II, ``cb`` likewise;
* ``d(i, j) = (10 / ln 10) sqrt(2 sum_k (ca[k, i] - cb[k, j])^2)``;
* ``D(0, 0) = d(0, 0)``, ``D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1))`` over the predecessors inside the matrix, the
  predecessor picked in that order (a later one only if strictly smaller), one byte per cell recording the pick;
* the path: backtracked from ``(Ta-1, Tb-1)`` to ``(0, 0)``, returned ascending;
* the summaries of ``_cabi.ALIGN_FIELD_NAMES``.

``dtype=np.float32`` evaluates the chain up to the cost matrix in float32 (the float32 mel, a float32 DCT, float32 sums): the distance
between the two is the chain's own rounding error on an input, which the GPU cost test scales its tolerance from.  The DP, the path
and the summaries are always float64.  ``dp`` adds the same float64 numbers in the same order as the kernel (one addition per cell),
so on equal cost matrices the two agree bit for bit.
"""
from __future__ import annotations

import numpy as np

from tests import mel_ref as mr
from tests import score_ref as sr

MCD_ORDER = 13
GPE_RATIO = 0.2
FIELDS = ('total_cost', 'path_len', 'frames_target', 'frames_test', 'mcd_dtw_db', 'mel_lsd_dtw_db', 'f0_rmse_cents', 'gpe', 'vde', 'ffe',
          'f0_corr', 'voiced_both')
HOP = 275


def cepstra(M, min_level_db=-100.0, mcd_order=MCD_ORDER, dtype=np.float64):
    """(K, T) in ``dtype`` from a mel ``M`` (n_mels, T) in [0, 1]."""
    M = np.asarray(M).astype(dtype)
    C = sr.dct_matrix(M.shape[0], mcd_order).astype(dtype)
    out = (C @ M) * dtype(-min_level_db * np.log(10.0) / 20.0)
    assert out.dtype == dtype
    return out


def cost_from_cepstra(ca, cb):
    """(Ta, Tb) in the cepstra's dtype."""
    dtype = ca.dtype.type
    df = ca[:, :, None] - cb[:, None, :]
    out = dtype(10.0 / np.log(10.0)) * np.sqrt(dtype(2.0) * (df * df).sum(axis=0))
    assert out.dtype == ca.dtype
    return out


def mels(a, b, cfg=None, features=None, dtype=np.float64):
    return sr.mel(np.asarray(a, np.float32), cfg, features, dtype).astype(dtype), sr.mel(np.asarray(b, np.float32), cfg, features, dtype).astype(dtype)


def cost(a, b, cfg=None, features=None, mcd_order=MCD_ORDER, dtype=np.float64):
    """(Ta, Tb) cost matrix of two clips, every step in ``dtype``."""
    c = dict(mr.DEFAULT, **(cfg or {}))
    Ma, Mb = mels(a, b, cfg, features, dtype)
    return cost_from_cepstra(cepstra(Ma, c['min_level_db'], mcd_order, dtype), cepstra(Mb, c['min_level_db'], mcd_order, dtype))


def dp(cost):
    """(D float64 (Ta, Tb), choice uint8 (Ta, Tb)): 0 the diagonal, 1 (i-1, j), 2 (i, j-1), 3 the cell (0, 0).  Anti-diagonal by
    anti-diagonal; a comparison with a NaN is false, so a NaN never displaces the predecessor held."""
    c = np.asarray(cost).astype(np.float64)
    Ta, Tb = c.shape
    D, ch = np.empty((Ta, Tb)), np.empty((Ta, Tb), np.uint8)
    for s in range(Ta + Tb - 1):
        i = np.arange(max(0, s - Tb + 1), min(s, Ta - 1) + 1)
        j = s - i
        best, pick = np.zeros(i.size), np.full(i.size, 3, np.uint8)
        inner = (i > 0) & (j > 0)
        ii, jj = i[inner], j[inner]
        b, p = D[ii - 1, jj - 1].copy(), np.zeros(ii.size, np.uint8)
        with np.errstate(invalid='ignore'):
            for code, v in ((1, D[ii - 1, jj]), (2, D[ii, jj - 1])):
                m = v < b
                b[m] = v[m]
                p[m] = code
        best[inner], pick[inner] = b, p
        e = (i > 0) & (j == 0)
        best[e], pick[e] = D[i[e] - 1, 0], 1
        e = (i == 0) & (j > 0)
        best[e], pick[e] = D[0, j[e] - 1], 2
        with np.errstate(invalid='ignore'):
            D[i, j] = np.where(pick == 3, c[i, j], c[i, j] + best)
        ch[i, j] = pick
    return D, ch


def backtrack(ch):
    """(P, 2) int32, ascending.  At most Ta + Tb - 1 steps whatever ``ch`` holds: every step lowers i + j and stays inside."""
    Ta, Tb = ch.shape
    i, j, rev = Ta - 1, Tb - 1, []
    while len(rev) < Ta + Tb - 1:
        rev.append((i, j))
        if i == 0 and j == 0:
            break
        c = ch[i, j]
        if c == 0 and i > 0 and j > 0:
            i, j = i - 1, j - 1
        elif c == 2 and j > 0:
            j -= 1
        elif i > 0:
            i -= 1
        else:
            j -= 1
    return np.array(rev[::-1], np.int32).reshape(-1, 2)


def path_of(cost):
    """(path, total, D) of one cost matrix; an empty matrix has an empty path and total 0."""
    cost = np.asarray(cost)
    if 0 in cost.shape:
        return np.zeros((0, 2), np.int32), 0.0, np.zeros(cost.shape)
    D, ch = dp(cost)
    return backtrack(ch), float(D[-1, -1]), D


def decision_gaps(D, path):
    """The gap between the best and the second-best predecessor at every path cell that has more than one (inf where it has one)."""
    out = []
    for i, j in path:
        if i > 0 and j > 0:
            v = sorted((D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]))
            out.append(v[1] - v[0])
        else:
            out.append(np.inf)
    return np.array(out)


def lsd_along(Ma, Mb, path, min_level_db=-100.0):
    """(P,) float64: sqrt(mean_m ((Ma[m, i_p] - Mb[m, j_p]) (-min_level_db))^2) from mels of any float dtype."""
    Ma, Mb = np.asarray(Ma).astype(np.float64), np.asarray(Mb).astype(np.float64)
    d = (Ma[:, path[:, 0]] - Mb[:, path[:, 1]]) * (-min_level_db)
    return np.sqrt((d * d).mean(axis=0))


def pitch_along(ft, fs, path, gpe_ratio=GPE_RATIO):
    """The six pitch fields over a path from float32 tracks, in float64, and ``cents`` per path pair (0 outside V)."""
    ft, fs = np.asarray(ft), np.asarray(fs)
    assert ft.dtype == fs.dtype == np.float32
    P = len(path)
    a, b = ft[path[:, 0]].astype(np.float64), fs[path[:, 1]].astype(np.float64)
    va, vb = a > 0, b > 0
    V = va & vb
    nV = int(V.sum())
    out = dict(f0_rmse_cents=0.0, gpe=0.0, vde=0.0, ffe=0.0, f0_corr=0.0, voiced_both=float(nV), cents=np.zeros(P))
    if P == 0:
        return out
    ratio = b[V] / a[V]
    cents = 1200.0 * np.log2(ratio)
    out['cents'][V] = cents
    n_gpe, n_vde = int((np.abs(ratio - 1.0) > gpe_ratio).sum()), int((va != vb).sum())
    if nV:
        out['f0_rmse_cents'] = float(np.sqrt((cents * cents).sum() / nV))
        out['gpe'] = n_gpe / nV
    out['vde'], out['ffe'] = n_vde / P, (n_gpe + n_vde) / P
    if nV >= 2:
        la, lb = np.log2(a[V]), np.log2(b[V])
        da, db = la - la.sum() / nV, lb - lb.sum() / nV
        va2, vb2 = (da * da).sum(), (db * db).sum()
        if va2 > 0 and vb2 > 0:
            out['f0_corr'] = float((da * db).sum() / np.sqrt(va2 * vb2))
    return out


def summaries(path, total, Ma, Mb, min_level_db=-100.0, f0_target=None, f0_test=None, gpe_ratio=GPE_RATIO):
    """The dict of ``FIELDS`` for one pair from a path, its total, the two mels (n_mels, T) and, optionally, the two tracks."""
    P, Ta, Tb = len(path), Ma.shape[1], Mb.shape[1]
    out = dict.fromkeys(FIELDS, 0.0)
    if P == 0:
        return out
    out.update(total_cost=float(total), path_len=float(P), frames_target=float(Ta), frames_test=float(Tb), mcd_dtw_db=float(total) / P,
               mel_lsd_dtw_db=float(lsd_along(Ma, Mb, path, min_level_db).sum() / P))
    if f0_target is not None:
        p = pitch_along(f0_target, f0_test, path, gpe_ratio)
        out.update({k: p[k] for k in ('f0_rmse_cents', 'gpe', 'vde', 'ffe', 'f0_corr', 'voiced_both')})
    return out


def score(a, b, cfg=None, features=None, mcd_order=MCD_ORDER, f0_target=None, f0_test=None, gpe_ratio=GPE_RATIO):
    """The whole chain in float64 for one pair: the ``FIELDS`` plus ``cost``, ``D``, ``path`` and the two mels."""
    c = dict(mr.DEFAULT, **(cfg or {}))
    Ma, Mb = mels(a, b, cfg, features)
    d = cost_from_cepstra(cepstra(Ma, c['min_level_db'], mcd_order), cepstra(Mb, c['min_level_db'], mcd_order))
    path, total, D = path_of(d)
    out = summaries(path, total, Ma, Mb, c['min_level_db'], f0_target, f0_test, gpe_ratio)
    out.update(cost=d, D=D, path=path, mel_target=Ma, mel_test=Mb)
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

def delayed_pair(T, m, hop=HOP):
    """The delayed fixture: a speech-like clip of ``hop T`` samples over a little noise, and the same clip after ``m hop`` zeros."""
    n = hop * T
    a = (20.0 * mr.speech_like(n, 13) + mr.white(n, 0.02, 5)).astype(np.float32)
    return a, np.concatenate([np.zeros(m * hop, np.float32), a])


DELAYED = ((40, 3), (40, 7), (70, 3), (70, 7))     # (T, m)
# what the float64 restatement gives on them (tests/test_align_host.py asserts it): the share of the path on j - i = m.  Every frame of
# the target sits on that diagonal, the m other pairs lead up to it: 0.93, 0.85, 0.96, 0.91 to two places.
DELAYED_SHARE = {(T, m): (T + 1) / (T + 1 + m) for T, m in DELAYED}


def on_offset(path, m):
    """The share of the path's pairs with j - i = m."""
    return float((path[:, 1] - path[:, 0] == m).mean())


def speech_clip(T, seed, hop=HOP):
    return (20.0 * mr.speech_like(hop * T, seed) + mr.white(hop * T, 0.02, 5)).astype(np.float32)


def sweep_clip(T, hop=HOP):
    """A tone gliding from 150 Hz to 7 kHz over the clip, over a little noise: every frame is far from its neighbours."""
    n = hop * T
    phase = 2.0 * np.pi * np.cumsum(150.0 * (7000.0 / 150.0) ** (np.arange(n) / n)) / 22050.0
    return (0.5 * np.sin(phase) + mr.white(n, 0.02, 5)).astype(np.float32)


# The fixtures on which the GPU tests demand the float64 path: on every decision along it the best predecessor leads the second best
# by at least 1000 (Ta + Tb) g, g the float32 chain's worst cost error on the fixture (tests/test_align_host.py asserts it).  The delayed
# fixtures above do NOT meet that (their paths absorb the delay in a corner where the predecessors lie within 0.8 .. 2.4 dB, against
# 11 .. 21 dB asked), so on them the GPU tests assert the scores and the share of the path on the delay's diagonal, not the path.
QUALIFIED = ('delay_s13_T8_m2', 'delay_s14_T12_m3', 'delay_s14_T14_m1', 'cut_s14_T7_m2', 'noisy_sweep_T20', 'noisy_sweep_T40')


def qualified_pair(name):
    kind, *rest = name.split('_')
    if kind == 'noisy':
        a = sweep_clip(int(rest[1][1:]))
        return a, (a + mr.white(a.size, 0.02, 9)).astype(np.float32)
    seed, T, m = int(rest[0][1:]), int(rest[1][1:]), int(rest[2][1:])
    a = speech_clip(T, seed)
    if kind == 'delay':
        return a, np.concatenate([np.zeros(m * HOP, np.float32), a])
    if kind == 'cut':
        return a, a[m * HOP:].copy()
    raise KeyError(name)


def case_of(a, b, cfg=None, features=None, mcd_order=MCD_ORDER):
    """``score`` plus the clips and ``g``, the float32 chain's worst cost error against the float64 one."""
    s = score(a, b, cfg, features, mcd_order)
    s['a'], s['b'] = a, b
    s['g'] = float(np.abs(cost(a, b, cfg, features, mcd_order, dtype=np.float32).astype(np.float64) - s['cost']).max())
    return s


_cache = {}


def qualified_case(name):
    """The float64 restatement of a qualified fixture, computed once and shared (never modified) by the tests that need it."""
    if name not in _cache:
        _cache[name] = case_of(*qualified_pair(name))
    return _cache[name]


def delayed_case(T, m):
    """The same for a delayed fixture."""
    if (T, m) not in _cache:
        _cache[T, m] = case_of(*delayed_pair(T, m))
    return _cache[T, m]
