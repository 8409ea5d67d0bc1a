"""NumPy restatement of what ``wrnn_taco_gta_corpus`` does around the decoder, and the fixtures the GTA-corpus tests share.

The pack rule: the target of a [0, 1] mel ``m`` is ``clip(2A m - A, -A, A)`` in float32 (two roundings), rows from ``frames`` up to the
next multiple of r are ``-A``, rows past that (up to the group's longest) are 0.  The cut: the first ``frames`` rows of the call's mel.
Nothing here touches a GPU."""
import functools

import numpy as np

from tests import tacotron_fixtures as fx
from tacotronv2_wavernn_chinese_amd.synth import make_tacotron_state

UTTERANCES = ((7, 5), (12, 17), (13, 31), (24, 64), (1, 1))   # (frames, Tx) of u = 0 .. 4
DIMS = {'small': fx.SMALL, 'small2': fx.SMALL2}               # r = 1, r = 2
HOP = 4                                                        # the corpus's hop: 4 * frames dummy labels per utterance


def target(mel01, r, A=4.0):
    """(frames, M) float32 in [0, 1] -> (r ceil(frames / r), M) float32: the decoder's own range, then the -A padding rows."""
    m = np.asarray(mel01, dtype=np.float32)
    A32 = np.float32(A)
    t = np.clip(np.float32(2.0 * A) * m - A32, -A32, A32).astype(np.float32)
    pad = -m.shape[0] % r
    if pad:
        t = np.concatenate([t, np.full((pad, m.shape[1]), -A32, dtype=np.float32)])
    return t


def pack(mels01, r, A=4.0):
    """The (B, gta_max, M) array a group's decoder reads and the steps per utterance: zeros behind every utterance's padded rows."""
    ts = [target(m, r, A) for m in mels01]
    gta_max = max(t.shape[0] for t in ts)
    out = np.zeros((len(ts), gta_max, ts[0].shape[1]), dtype=np.float32)
    for b, t in enumerate(ts):
        out[b, :t.shape[0]] = t
    return out, [t.shape[0] // r for t in ts]


def cut(mel_pred, frames):
    """The reference's ``mel[:target_length]``."""
    return mel_pred[:frames]


@functools.lru_cache(maxsize=None)
def state(name):
    return dict(make_tacotron_state(21, 'peaked', **DIMS[name]))


@functools.lru_cache(maxsize=None)
def utterance(u):
    """seq, the ground-truth mel (frames, 20) in [0, 1], the dropout seed."""
    frames, tx = UTTERANCES[u]
    rng = np.random.Generator(np.random.PCG64(5000 + u))
    seq = rng.integers(0, fx.SMALL['n_symbols'], tx).tolist()
    mel = rng.random((frames, 20), dtype=np.float32)
    return seq, mel, 900 + u


@functools.lru_cache(maxsize=None)
def restated(name, u):
    """The float64 and float32 restatements of utterance u teacher-forced on its restated target: r64, r32, g (max |r32 - r64| of the
    kept mel rows and of the forward alignments), the leads of the attention argmaxes."""
    dims, d = DIMS[name], fx.full_dims(DIMS[name])
    seq, mel, seed = utterance(u)
    tg = target(mel, d['outputs_per_step'], d['max_abs_value'])
    kw = dict(gta_target=tg, seed=seed, prenet_dropout=True)
    r64, r32 = fx.run_ref(state(name), dims, seq, np.float64, **kw), fx.run_ref(state(name), dims, seq, np.float32, **kw)
    f = mel.shape[0]
    g = dict(mel=float(np.max(np.abs(r32['mel'][:f].astype(np.float64) - r64['mel'][:f]))),
             forward=float(np.max(np.abs(r32['forward'].astype(np.float64) - r64['forward']))))
    return dict(r64=r64, r32=r32, g=g, leads=fx.decision_leads(r64, False), target=tg)
