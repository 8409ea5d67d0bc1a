"""Chosen fc3 outputs for the MOL loss, its gradient and the MOL sampler: every arm of `mol_rows_kernel` / `mol_grad_kernel`
(csrc/losses.hip, csrc/train.hip) and the floor / clamps of the sampler in the loop kernels, reached on purpose.

Plain numpy, no oracle, no reference.  The seeded synthetic weights of the rest of the suite put every log-scale near 0: there the
discretised likelihood always takes one arm (cdf_delta ~ 7.6e-6 < 1e-5: the pdf-mid fallback), the floor `log(1e-14)` and the clamp
of the sample to [-1, 1] are never reached.  Here the 30 numbers of a row are written down, so the arm of every (row, component) is
known beforehand and sits away from every threshold:

    arm 0  y < -0.999                log sigmoid(plus_in)
    arm 1  y >  0.999                -softplus(min_in)
    arm 2  cdf_delta > 1e-5          log(cdf_delta)
    arm 3  otherwise                 log_pdf_mid - log((nc - 1) / 2)

A group is `P` (n_p, 30) float32 -- [10 logit_probs | 10 means | 10 raw log-scales] -- and `y` (n_p, n_y) float32: its rows are all
pairs (P[i], y[i, j]).  `P[0]` with `y[0]` is what the gradient test loads into fc3.bias (one P per call).  Margins (asserted by
tests/test_mol_arms_host.py, not assumed): in every group but the two edge groups the float64 cdf_delta of every (row, component) lies
outside CDF_BAND, and |y| of every row lies outside Y_BAND.  THRESHOLD is the one place that sits ON a threshold: y = float32(0.999)
and its float32 successor, and the same pair mirrored; which side the reference's float32 comparison puts them on is recorded in
tests/golden/mol_arms_threshold.json.
"""
from __future__ import annotations

import numpy as np

NR = 10
NUM_CLASSES = 65536
HALF_BIN = 1.0 / (NUM_CLASSES - 1)
LOG_SCALE_MIN = float(np.log(1e-14))
ARM_EDGE_LO, ARM_EDGE_HI, ARM_LOG, ARM_MID = 0, 1, 2, 3
CDF_BAND = (2.5e-6, 4e-5)       # no non-edge (row, component) has its float64 cdf_delta in here (the arm threshold is 1e-5)
Y_BAND = (0.998, 0.9995)        # no row has |y| in this open interval (the edge threshold is 0.999)
EDGE_GROUPS = ('edge_lo', 'edge_hi')


def _pack(lp, mean, ls):
    lp, mean, ls = (np.asarray(v, np.float64) for v in (lp, mean, ls))
    assert lp.shape == mean.shape == ls.shape == (NR,)
    return np.concatenate([lp, mean, ls]).astype(np.float32) + np.float32(0.0)     # no -0.0: fc3's `0 + bias` would return +0.0, not the same bits


def _sig(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def cdf_delta64(logits, y):
    """float64 cdf_plus - cdf_min of every (row, component): logits (n, 30), y (n,) -> (n, 10)."""
    lg = np.asarray(logits, np.float64)
    cy = np.asarray(y, np.float64)[:, None] - lg[:, NR:2 * NR]
    inv = np.exp(-np.maximum(lg[:, 2 * NR:], LOG_SCALE_MIN))
    return _sig(inv * (cy + HALF_BIN)) - _sig(inv * (cy - HALF_BIN))


def expected_arms(logits, y):
    """The arm of every (row, component) in exact arithmetic on the float32 inputs: (n, 10) ints."""
    yy = np.asarray(y, np.float64)[:, None]
    arm = np.where(cdf_delta64(logits, y) > 1e-5, ARM_LOG, ARM_MID)
    arm = np.where(yy > 0.999, ARM_EDGE_HI, arm)
    return np.where(yy < -0.999, ARM_EDGE_LO, arm)


def at_floor(logits):
    """(n, 10) bool: the raw log-scale is below log(1e-14)."""
    return np.asarray(logits, np.float64)[:, 2 * NR:] < LOG_SCALE_MIN


def rows_of(group, n_rows=None):
    """(logits (n, 30), y (n,)) of a group: every (P[i], y[i, j]) pair, repeated cyclically up to n_rows."""
    P, y = group['P'], group['y']
    logits = np.repeat(P, y.shape[1], axis=0)
    yy = y.reshape(-1)
    if n_rows is not None:
        idx = np.arange(n_rows) % yy.size
        logits, yy = logits[idx], yy[idx]
    return np.ascontiguousarray(logits, np.float32), np.ascontiguousarray(yy, np.float32)


_LP_A = [0.3, -0.2, 1.0, -1.5, 0.0, 0.5, -0.7, 0.2, -0.1, 0.4]
_LP_B = [-0.4, 0.6, 0.1, 0.0, -1.0, 0.8, 0.3, -0.3, 0.2, -0.6]
_GRID = [-0.9, -0.7, -0.5, -0.3, -0.1, 0.1, 0.3, 0.5, 0.7, 0.9]


def _group(Ps, ys):
    P = np.stack(Ps).astype(np.float32)
    y = np.asarray(ys, np.float32)
    assert y.shape[0] == P.shape[0]
    return dict(P=P, y=y)


def build_groups():
    g = {}
    # ---- the two edges: every component takes the edge arm, whatever its scale (sharp, wide, one at the floor)
    edge_means = [-0.95, -0.999, -1.0, -0.9, -0.5, 0.0, 0.5, 0.9, -0.97, -0.99]
    edge_ls_a = [-5.0, -6.0, -7.0, -8.0, -9.0, -3.0, -1.0, 0.0, -2.0, -4.0]
    edge_ls_b = [0.1, -0.1, 0.05, -35.0, 0.0, -0.05, 0.12, -0.02, 0.08, -0.08]
    one_m = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    ys = [1.0, one_m, 0.9999, 0.9996]
    g['edge_lo'] = _group([_pack(_LP_A, edge_means, edge_ls_a), _pack(_LP_B, [0.5 * m for m in edge_means], edge_ls_b)],
                          [[-v for v in ys]] * 2)
    g['edge_hi'] = _group([_pack(_LP_A, [-m for m in edge_means], edge_ls_a), _pack(_LP_B, [-0.5 * m for m in edge_means], edge_ls_b)],
                          [ys] * 2)
    # ---- sharp_near: log-scales -5 .. -9, every mean within two of ITS scales of a centre, y within a few scales of the centre:
    # the log arm everywhere, cdf_delta from 0.06 (on a mean) down to under 1e-4 (8 scales off the sharpest component)
    ls = np.linspace(-5.0, -9.0, NR)
    zk = np.array([-2.0, 1.5, -1.0, 0.5, 0.0, -0.5, 1.0, -1.5, 2.0, 0.3])
    offs = [0.0, 2e-4, -2e-4, 5e-4, 1e-3, -1e-3]
    Ps, ys = [], []
    for c, lp in ((0.25, _LP_A), (-0.6, _LP_B)):
        Ps.append(_pack(lp, c + zk * np.exp(ls), ls))
        ys.append([c + o for o in offs])
    g['sharp_near'] = _group(Ps, ys)
    # ---- sharp_far: the same scales, means on a 0.2 grid, y at least 0.07 (> 10 scales) from every mean: pdf-mid everywhere
    far_y = [-0.83, -0.42, 0.03, 0.37, 0.78, 0.0]
    g['sharp_far'] = _group([_pack(_LP_A, _GRID, ls), _pack(_LP_B, _GRID, ls[::-1])], [far_y] * 2)
    # ---- mixed: components 0-4 at scale e^-5 within 3 scales of y (log arm), 5-9 sharper and far away (pdf-mid); one logit_prob at
    # -30 on a near component; the dominant one (+4) on a near component in P[0], on a far one in P[1]
    s5 = float(np.exp(-5.0))
    y0 = 0.1
    near = [y0 + z * s5 for z in (0.0, 1.0, -2.0, 3.0, -1.0)]
    mix_mean = near + [-0.6, 0.5, -0.3, 0.8, -0.85]
    mix_ls = [-5.0] * 5 + [-6.0, -7.0, -8.0, -9.0, -6.5]
    mix_y = [y0, y0 + 0.5 * s5, y0 - 0.5 * s5, y0 + 0.25 * s5]
    g['mixed'] = _group([_pack([4.0, -30.0, 0.0, 0.5, -0.5, 0.2, -0.2, 0.1, 0.3, -0.1], mix_mean, mix_ls),
                         _pack([0.0, -30.0, 0.3, 0.5, -0.5, 4.0, -0.2, 0.1, 0.3, -0.1], mix_mean, mix_ls)], [mix_y] * 2)
    # ---- floor: raw log-scales -40, -33, -35 (below log(1e-14) = -32.24) among ordinary ones (-3.2 .. -3.6, the log arm).  A floored
    # component is 1e-14 wide: with y inside its bin cdf_delta is 1 (y on the mean, y 1e-5 next to it), anywhere else it is 0
    fl_ls = [-40.0, -33.0, -3.3, -3.2, -3.6, -35.0, -3.5, -3.4, -3.25, -3.45]
    fl_mean = [0.05, -0.04, 0.01, -0.02, 0.0, 0.5, 0.02, -0.01, 0.015, -0.015]
    fl_y = [0.05, -0.04, 0.01, -0.02, 0.05 + 1e-5]
    g['floor'] = _group([_pack(_LP_A, fl_mean, fl_ls), _pack(_LP_B, fl_mean, fl_ls)], [fl_y] * 2)
    # ---- floor_far: every component below the floor and at least 0.07 from y: a loss of 1e14 x 0.07.  P[1] lifts the component next
    # to y just above the floor (-32.0): it alone then has a log-scale gradient
    ff_ls = [-40.0, -33.0, -35.0, -50.0, -32.5, -38.0, -34.0, -45.0, -33.5, -36.0]
    ff_ls_b = [-32.0 if v in (-33.0, -32.5, -34.0) else v for v in ff_ls]
    g['floor_far'] = _group([_pack(_LP_A, _GRID, ff_ls), _pack(_LP_B, _GRID, ff_ls_b)], [far_y[:5]] * 2)
    # ---- wide, the control.  The suite's synthetic weights give log-scales within 0.15 of 0, where cdf_delta = 7.6e-6 at the mean: the
    # pdf-mid arm, but inside CDF_BAND.  P[0] is that regime moved to the nearest scales that keep the margin (1.3 .. 2.0: cdf_delta <=
    # 2.1e-6, still pdf-mid); P[1] the widest scales that take the log arm with margin (-3.2 .. -3.6)
    w_lp = [0.05, -0.03, 0.1, -0.11, 0.0, 0.13, -0.07, 0.02, -0.01, 0.04]
    w_mean = [0.02, -0.08, 0.15, 0.0, -0.03, 0.07, 0.11, -0.05, 0.01, 0.04]
    g['wide'] = _group([_pack(w_lp, w_mean, np.linspace(1.3, 2.0, NR)), _pack(w_lp, [0.2 * m for m in w_mean], np.linspace(-3.2, -3.6, NR))],
                       [[-0.99, -0.5, 0.0, 0.3, 0.99], [-0.04, -0.02, 0.0, 0.03, 0.04]])
    return g


GROUPS = build_groups()

# On the edge threshold itself: y = float32(0.999) -- which is ABOVE the real number 0.999 -- and its successor, and both mirrored.  A
# sharp component 0.099 from y makes the two arms differ by several nats, so the side a comparison takes shows in the loss.
_T = np.float32(0.999)
THRESHOLD_Y = np.array([_T, np.nextafter(_T, np.float32(2.0)), -_T, -np.nextafter(_T, np.float32(2.0))], np.float32)
THRESHOLD_P = _pack([2.0, 2.0, 0.0, 0.3, -0.3, 0.1, -0.1, 0.2, -0.2, 0.0], [0.9, -0.9, 0.0, 0.5, -0.5, 0.95, -0.95, 0.2, -0.2, 0.7],
                    [-5.0, -5.0, -1.0, -3.0, -3.0, -6.0, -6.0, -2.0, -2.0, -4.0])


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
# One P for every row (the rows of a call share fc3.bias); the noise differs per row.  Component 0 and 4 are below the floor (sample ==
# mean), 1 and 2 have mean +-0.99 at log-scale 0 (the clamp to exactly +-1 when u_log is at the matching extreme), 3 has log-scale -9.
SAMPLER_P = _pack([0.3, -0.2, 0.45, -0.5, 0.0, 0.5, -0.35, 0.2, -0.1, 0.4], [0.3, 0.99, -0.99, -0.5, -0.2, 0.1, 0.6, -0.7, 0.45, -0.35],
                  [-40.0, 0.0, 0.0, -9.0, -33.0, -5.0, -6.0, -7.0, -8.0, -2.0])
U_LOG_CYCLE = (1e-5, 1.0 - 1e-5, 0.5, None)     # None: an ordinary draw
GUMBEL_MARGIN = 1e-3


def gumbel_scores(P, u_mix):
    """float64 `logit_prob - log(-log(u))` (distribution.py:107) of float32 draws: (..., 10)."""
    return np.asarray(P, np.float64)[:NR] - np.log(-np.log(np.asarray(u_mix, np.float64)))


def sampler_noise(L, rows, seed=0, P=SAMPLER_P):
    """u_mix (L, rows, 10), u_log (L, rows) float32 and what they decide: `winner` (L, rows) = (t + row) % 10, beating the runner-up by a
    margin drawn log-uniformly from 5e-3 .. 1 (tight races, but none under GUMBEL_MARGIN); `phase` (L, rows) = (t // 10) % 4 indexes
    U_LOG_CYCLE, so every (winner, phase) pair comes round every 40 steps."""
    rng = np.random.Generator(np.random.PCG64(seed))
    u_mix = rng.uniform(0.02, 0.98, size=(L, rows, NR))
    t = np.arange(L)[:, None]
    winner = (t + np.arange(rows)[None, :]) % NR
    phase = np.broadcast_to((t // 10) % 4, (L, rows)).copy()
    sc = gumbel_scores(P, u_mix)
    np.put_along_axis(sc, winner[..., None], -np.inf, axis=2)
    target = sc.max(axis=2) + 10.0 ** rng.uniform(np.log10(5e-3), 0.0, size=(L, rows))
    lp_w = np.asarray(P, np.float64)[:NR][winner]
    np.put_along_axis(u_mix, winner[..., None], np.exp(-np.exp(-(target - lp_w)))[..., None], axis=2)
    u_log = rng.uniform(0.05, 0.95, size=(L, rows))
    for i, v in enumerate(U_LOG_CYCLE):
        if v is not None:
            u_log[phase == i] = v
    return dict(u_mix=u_mix.astype(np.float32), u_log=u_log.astype(np.float32), winner=winner.astype(np.int32), phase=phase)
