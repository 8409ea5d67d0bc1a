"""Restatement of the e4m3 weight image of WRNN_KERNEL_TEAMG / WRNN_KERNEL_TEAMG_BATCH (`teamg_weights='e4m3'`).

`quantise(sd, dims)` returns the dequantised model `sd8` and the six scales the pack must find.  A layer of the image -- fc3, fc2, fc1,
rnn2 (weight_ih and weight_hh together, all gates), rnn1 (likewise), `I.weight[:, 1:]` -- gets s = 2^e with e the smallest integer such
that max|w| / 2^e <= 448, clamped to e >= -126, s = 1 for an all-zero layer; a stored byte is RNE(w / s) in OCP e4m3fn (torch's
float8_e4m3fn cast: nearest even, subnormals kept, ties to even at half the smallest subnormal, the sign of zero kept).  `I.weight[:, 0]`
is left alone.  `pos` restates the row layout of csrc/teamg_layout.h (`tg8_pos`) for the host test of its properties; the function the
kernels and the pack share is exercised by the GPU tests, where any disagreement between the two breaks bit-equality.
"""
import math

import numpy as np
import torch

LAYERS = ('fc3', 'fc2', 'fc1', 'rnn2', 'rnn1', 'I')          # wrnn_teamg_layer_names
LAYER_KEYS = {'fc3': ('fc3.weight',), 'fc2': ('fc2.weight',), 'fc1': ('fc1.weight',),
              'rnn2': ('rnn2.weight_ih_l0', 'rnn2.weight_hh_l0'), 'rnn1': ('rnn1.weight_ih_l0', 'rnn1.weight_hh_l0'), 'I': ('I.weight',)}
E4M3_MAX = 448.0
E4M3_MIN_NORMAL = 2.0 ** -6
E4M3_MIN_SUBNORMAL = 2.0 ** -9


def scale_of(amax: float) -> float:
    """2^e, e the smallest integer with amax / 2^e <= 448 (frexp, no log2 rounding), e >= -126; 1 for amax == 0."""
    amax = float(amax)
    if not amax > 0.0:
        return 1.0
    f, e = math.frexp(amax)                                   # amax = f 2^e, 0.5 <= f < 1; 448 = 0.875 * 2^9
    e -= 9 if f <= 0.875 else 8
    return math.ldexp(1.0, max(e, -126))


def _part(key, w):
    """The part of tensor `key` that is in the image."""
    return w[:, 1:] if key == 'I.weight' else w


def e4m3_round(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).float().numpy()


def quantise(sd, dims=None):
    """(sd8, scales): sd with the matrices of the image replaced by e4m3(w / s) * s, and the six scales in LAYERS order (float32)."""
    sd8 = {k: np.array(v) for k, v in sd.items()}
    scales = []
    for layer in LAYERS:
        amax = max(float(np.abs(_part(k, np.asarray(sd[k], np.float32))).max()) for k in LAYER_KEYS[layer])
        assert np.isfinite(amax), layer
        s = np.float32(scale_of(amax))
        scales.append(s)
        for k in LAYER_KEYS[layer]:
            w = np.asarray(sd[k], np.float32)
            r = e4m3_round(w / s) * s
            if k == 'I.weight':
                r[:, 0] = w[:, 0]
            sd8[k] = r.astype(np.float32)
    return sd8, np.asarray(scales, np.float32)


def stored(sd, layer):
    """(w / s of every image element of the layer, flattened, the e4m3 values stored for them, s)."""
    s = np.float32(scale_of(max(float(np.abs(_part(k, np.asarray(sd[k], np.float32))).max()) for k in LAYER_KEYS[layer])))
    x = np.concatenate([(_part(k, np.asarray(sd[k], np.float32)) / s).ravel() for k in LAYER_KEYS[layer]])
    return x, e4m3_round(x), s


def rot(row: int, KP: int) -> int:
    return ((-(row * (KP >> 6))) & 3) << 2


def pos(p: int, row: int, KAP: int, KP: int) -> int:
    """Byte of element p inside row `row` of a layer whose rows are [segment A: KAP | segment B: KP - KAP] elements (tg8_pos)."""
    k, q, c = p >> 6, (p >> 2) & 15, p & 3
    k0, k1 = (0, KAP >> 6) if p < KAP else (KAP >> 6, KP >> 6)
    rel, n = k - k0, k1 - k0
    nq = n & ~3
    if rel < nq:
        return 64 * (k - (rel & 3)) + 16 * ((q + rot(row, KP)) & 15) + 4 * (rel & 3) + c
    if (n & 2) and rel - nq < 2:
        return 64 * (k - (rel - nq)) + 8 * q + 4 * (rel - nq) + c
    return p
