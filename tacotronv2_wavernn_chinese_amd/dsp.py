"""Host-side DSP helpers on the generate() path.

Mirror of the subset of ``wavernn/utils/dsp.py`` the mel->wav path touches:
``label_2_float`` (:8-9), ``save_wav`` (:22-23), ``decode_mu_law`` (:98-103), and of the two quantisers the training data is made
with, ``float_2_label`` (:12-15) and ``encode_mu_law`` (:92-95): float64 NumPy, for small inputs and the tests -- a corpus is quantised
on the device (``csrc/dataset.hip``, ``dataset.DeviceCorpus``).
``load_wav`` (:18-19) and ``melspectrogram`` (:72-81) live in ``frontend.py``: the mel is built on the device (``csrc/melspec.hip``).
Pre-emphasis is fused into the mel kernel, and Griffin-Lim with its de-emphasis is ``frontend.GriffinLim`` (``csrc/griffin_lim.hip``);
``spectrogram`` is not mirrored.
"""
from __future__ import annotations

import math

import numpy as np


def label_2_float(x, bits):
    return 2 * x / (2 ** bits - 1.) - 1.


def float_2_label(x, bits):
    """[-1, 1] -> the linear class scale [0, 2**bits - 1], not yet truncated (the collate's ``.astype(np.int64)`` does that)."""
    x = np.asarray(x, dtype=np.float64)
    assert abs(x).max() <= 1.0
    x = (x + 1.) * (2 ** bits - 1) / 2
    return x.clip(0, 2 ** bits - 1)


def encode_mu_law(x, mu):
    """[-1, 1] -> mu-law class indices 0 .. mu - 1 as float64 (``mu`` = the number of classes, 2**bits)."""
    x = np.asarray(x, dtype=np.float64)
    mu = mu - 1
    fx = np.sign(x) * np.log(1 + mu * np.abs(x)) / np.log(1 + mu)
    return np.floor((fx + 1) / 2 * mu + 0.5)


def decode_mu_law(y, mu, from_labels=True):
    if from_labels:
        y = label_2_float(y, math.log2(mu))
    mu = mu - 1
    return np.sign(y) / mu * ((1 + mu) ** np.abs(y) - 1)


def save_wav(x, path, sample_rate=None):
    """float32 WAV at hp.sample_rate, what ``librosa.output.write_wav`` (librosa <= 0.7) produced."""
    from scipy.io import wavfile
    if sample_rate is None:
        from .hparams import hparams as hp
        sample_rate = hp.sample_rate
    wavfile.write(str(path), int(sample_rate), np.asarray(x).astype(np.float32))
