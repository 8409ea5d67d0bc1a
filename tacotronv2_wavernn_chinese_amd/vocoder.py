"""Drop-in host side of the WaveRNN vocoder (mel -> wav) for MI355X.

Mirrors the call surface of ``wavernn/models/fatchord_version.py`` of the
reference: ``WaveRNN(rnn_dims, fc_dims, bits, pad, upsample_factors, feat_dims,
compute_dims, res_out_dims, res_blocks, hop_length, sample_rate, mode)``
(:93-95), ``generate(mels, save_path, batched, target, overlap, mu_law)``
(:169-264), ``load``/``save``/``get_step``/``num_params`` (:407-429), the flat
``state_dict`` key layout, and the reference's observable quirks (listed in
``generate``).  The arithmetic of the hot path runs in libwavernn_amd.so (HIP,
gfx950) through the C-ABI of ``include/wavernn_amd.h``; this module only holds
parameters, moves pointers, and performs the float64 epilogue (:243-260).

The class is an ``nn.Module`` purely as a parameter container: sub-module
names and construction order follow the reference so that ``state_dict()``
keys, ``load_state_dict`` and the default initialisation under a given
``torch.manual_seed`` are interchangeable with it.  ``forward`` (teacher-forced
pass, :131-167) runs the same loop kernels with the fed-back value forced;
the losses of the training script live in ``losses.py``.
"""
from __future__ import annotations

import math
import sys
import time
import warnings
from pathlib import Path
from typing import Optional, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _cabi
from .dsp import decode_mu_law, save_wav


def _bag(**mods) -> nn.Module:
    m = nn.Module()
    for k, v in mods.items():
        m.add_module(k, v)
    return m


def _make_upsample(feat_dims, upsample_scales, compute_dims, res_blocks, res_out_dims, pad) -> nn.Module:
    """Parameter containers with the key layout of UpsampleNetwork/MelResNet (:31-80)."""
    resnet = nn.Module()
    resnet.add_module('conv_in', nn.Conv1d(feat_dims, compute_dims, kernel_size=2 * pad + 1, bias=False))
    resnet.add_module('batch_norm', nn.BatchNorm1d(compute_dims))
    blocks = nn.ModuleList()
    for _ in range(res_blocks):
        blocks.append(_bag(conv1=nn.Conv1d(compute_dims, compute_dims, kernel_size=1, bias=False),
                           conv2=nn.Conv1d(compute_dims, compute_dims, kernel_size=1, bias=False),
                           batch_norm1=nn.BatchNorm1d(compute_dims),
                           batch_norm2=nn.BatchNorm1d(compute_dims)))
    resnet.add_module('layers', blocks)
    resnet.add_module('conv_out', nn.Conv1d(compute_dims, res_out_dims, kernel_size=1))
    up = nn.Module()
    up.add_module('resnet', resnet)
    layers = nn.ModuleList()
    for s in upsample_scales:
        layers.append(nn.Identity())  # slot of the parameter-free Stretch2d (:74)
        conv = nn.Conv2d(1, 1, kernel_size=(1, 2 * s + 1), padding=(0, s), bias=False)
        conv.weight.data.fill_(1. / (2 * s + 1))  # :78
        layers.append(conv)
    up.add_module('up_layers', layers)
    return up


def fold_target(total_len: int, overlap: int, n_folds: int) -> int:
    """Smallest ``target`` for which ``fold_with_overlap`` (:293-340) cuts ``total_len`` samples into at most
    ``n_folds`` folds: ceil((total_len - overlap) / n_folds) - overlap, never below ``overlap``."""
    return max(-(-(int(total_len) - int(overlap)) // int(n_folds)) - int(overlap), int(overlap), 1)


def fold_count(total_len: int, target: int, overlap: int) -> int:
    """Number of folds ``fold_with_overlap`` cuts ``total_len`` samples into (:319-325; = ``wrnn_plan``'s rows)."""
    num_folds, remaining = divmod(int(total_len) - int(overlap), int(target) + int(overlap))
    return num_folds + (1 if remaining != 0 else 0)


# Microseconds per lock-step loop step of ONE XCD team on an MI355X, by what the team runs (profiles/r06_fold_latency_{raw,mol}.txt):
# 'team2' the latency kernel (one row per team), 'cs4' / 'cs8' the batch kernel at <= 4 / <= 8 rows per team.  Only the RATIOS matter to
# ``fold_plan`` (it compares fold counts on one device); a device with another clock shifts all three alike.
STEP_US = {'RAW': {'team2': 3.30, 'cs4': 5.28, 'cs8': 7.52}, 'MOL': {'team2': 3.43, 'cs4': 4.85, 'cs8': 8.16}}
ROWS_PER_TEAM_MAX = 8   # WRNN_BATCH_MAX_ROWS


def predicted_loop_us(rows: int, steps: int, n_teams: int, mode: str = 'RAW') -> float:
    """Loop time ``WRNN_KERNEL_AUTO`` needs for ``rows`` rows of ``steps`` steps on ``n_teams`` XCD teams (api.hip: rows <= teams run one per
    team on the latency kernel; more rows are spread evenly, ceil(rows / teams) <= 8 per team batch in lock-step, a team runs its batches
    back to back)."""
    us = STEP_US[mode]
    if rows <= n_teams:
        return steps * us['team2']
    rpb = min(-(-rows // n_teams), ROWS_PER_TEAM_MAX)
    passes = -(-(-(-rows // rpb)) // n_teams)
    return steps * passes * (us['cs4'] if rpb <= 4 else us['cs8'])


def fold_plan(total_len: int, overlap: int, n_teams: int = 8, mode: str = 'RAW', min_target: int = 0):
    """The fold count that minimises the predicted loop time of ONE utterance in the reference's batched mode (``target='auto'``):
    every count from 1 to 2 x 8 x teams is priced as steps(target, overlap) x us/step(rows per team) x passes -- fewer, longer folds
    cost steps, more folds cost the 2 x overlap samples each one generates twice and, past 8 per team, a second pass.  On an MI355X
    a 5 s clip lands at 64 folds (8 per team, 2 265 steps, ~17 ms) against 47 ms for one fold per team.  Returns
    (target, folds, predicted_us); ties go to the smaller fold count (fewer crossfades).  ``min_target`` bounds the crossfade DENSITY
    from below (the latency optimum of a 5 s clip is a 550-sample crossfade every 1 715 samples: a third of the audio lies inside one;
    ``min_target=5500`` gives 18 folds / 35 ms instead of 64 / 17 ms); a one-fold plan is always admissible.
    The step times are those of the 512 / 512 kernels (``STEP_US``) whatever the model: ``target='auto'`` uses them for a model on
    ``kernel='teamg'`` / ``'teamg_batch'`` too -- a cost model for other dims is a follow-up."""
    best = None
    for n in range(1, 2 * ROWS_PER_TEAM_MAX * max(n_teams, 1) + 1):
        target = fold_target(total_len, overlap, n)
        rows = fold_count(total_len, target, overlap)
        if rows < 1 or (target < min_target and n > 1):
            continue
        cost = predicted_loop_us(rows, target + 2 * overlap, max(n_teams, 1), mode)
        if best is None or cost < best[2] * (1.0 - 1e-9):
            best = (target, rows, cost)
    if best is None:
        raise ValueError(f'no fold plan for {total_len} samples with overlap {overlap}')
    return best


def fold_plan_many(total_lens, overlap: int, n_teams: int = 8, mode: str = 'RAW', min_target: int = 0):
    """``fold_plan`` for a call that folds SEVERAL utterances with one common ``target`` (``generate_many(batched=True, target='auto')``):
    minimises ``predicted_loop_us(sum_b fold_count(len_b, target, overlap), target + 2 x overlap, ...)`` over the candidates
    ``fold_target(len_b, overlap, n)`` of every utterance b and every n <= 2 x 8 x teams -- the targets at which some utterance's fold count
    changes.  Ties go to the larger target (fewer crossfades).  ``min_target`` as in ``fold_plan``; the plan that leaves every utterance in
    one fold is always admissible.  Returns (target, rows, predicted_us); for one utterance this is ``fold_plan``'s result."""
    lens = [int(t) for t in total_lens]
    if not lens:
        raise ValueError('fold_plan_many needs at least one utterance')
    teams = max(int(n_teams), 1)
    one_fold = fold_target(max(lens), overlap, 1)
    cands = {fold_target(t, overlap, n) for t in lens for n in range(1, 2 * ROWS_PER_TEAM_MAX * teams + 1)}
    best = None
    for target in sorted(cands, reverse=True):
        counts = [fold_count(t, target, overlap) for t in lens]
        if min(counts) < 1 or (target < min_target and target != one_fold):
            continue
        cost = predicted_loop_us(sum(counts), target + 2 * overlap, teams, mode)
        if best is None or cost < best[2] * (1.0 - 1e-9):
            best = (target, sum(counts), cost)
    if best is None:
        raise ValueError(f'no fold plan for {lens} samples with overlap {overlap}')
    return best


_CU_COUNT = {}   # torch.cuda.get_device_properties costs ~0.1 s on its first call (amdsmi): asked once per device


def request_seeds(seeds, n_utterances, noise_mode=_cabi.NOISE_PHILOX, seed=None) -> np.ndarray:
    """Host check of ``seeds=`` (``wrnn_sample_opts.utt_seeds_dev``): a sequence of ``n_utterances`` Python ints, one Philox key per
    utterance, returned as uint64 (taken mod 2**64).  ``ValueError`` -- raised by the callers before any device work -- when a call-wide
    ``seed`` is given as well, when the length is wrong, or when the noise does not come from the device RNG (injected / argmax /
    reference)."""
    if seed is not None:
        raise ValueError('seeds (one per utterance) and seed (one for the call) are exclusive: give one of them')
    if noise_mode not in (_cabi.NOISE_PHILOX, 'philox'):
        raise ValueError(f"seeds key the device RNG: noise_mode must be 'philox', got {noise_mode!r}")
    vals = [int(s) for s in seeds]
    if len(vals) != int(n_utterances):
        raise ValueError(f'seeds must hold one seed per utterance: expected {int(n_utterances)}, got {len(vals)}')
    return np.array([v & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)


def _draw_call_seed(native_opts):
    """The Philox seed of a call that was given none: one draw from the global torch generator, so that ``torch.manual_seed`` makes the
    call reproducible like it does for the reference."""
    if 'seed' not in native_opts and native_opts.get('noise_mode', _cabi.NOISE_PHILOX) in (_cabi.NOISE_PHILOX, 'philox'):
        native_opts['seed'] = int(torch.randint(0, 2 ** 62, (1,)).item())


def _fade_broadcast_error(wave_len, hop):
    """The ``ValueError`` the reference's 20-hop fade-out raises for a clip of fewer than 21 frames (:256-258)."""
    return ValueError(f'operands could not be broadcast together with shapes ({max(wave_len, 0)},) ({20 * hop},) ({max(wave_len, 0)},)')


def _device_teams(dev) -> int:
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _CU_COUNT:
        _CU_COUNT[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return max(1, min(8, _CU_COUNT[idx] // 32))


def reference_noise(mode: str, rows: int, steps: int, n_classes: int, rnn_dims: int, aux_dims: int, device, chunk_bytes: int = 64 << 20):
    """The sampling noise of the reference's ``generate`` (:169-264) drawn from the GLOBAL torch CPU generator exactly as the reference
    consumes it, so that ``torch.manual_seed(s); model.generate(..., noise_mode='reference')`` is the reference's own output for seed s
    (model on the CPU there; a reference model on a CUDA device draws from that device's generator, which cannot be replayed):
      1. ``get_gru_cell`` builds two ``nn.GRUCell`` objects whose default initialisation draws from the generator (:178-179, :273-279);
      2. RAW: ``Categorical.sample()`` = ``torch.multinomial(p, 1, True)`` = argmax p / q with ``q = empty(rows, n_classes).exponential_(1)``,
         one call per step (:231-235);  MOL: ``uniform_(1e-5, 1 - 1e-5)`` on (1, rows, 10) and then on (1, rows), per step
         (``wavernn/utils/distribution.py:106,118``).
    One generator call per step like the reference (``exponential_`` seeds a per-call stream whose content depends on the call's size),
    written straight into a host chunk and uploaded.  Returns (noise1, noise2) device tensors laid out as ``wrnn_sample_opts`` wants them:
    RAW (steps, rows, n_classes), None;  MOL (steps, rows, 10), (steps, rows)."""
    device = torch.device(device)
    pin = device.type == 'cuda'
    nn.GRUCell(rnn_dims, rnn_dims)                 # get_gru_cell(self.rnn1): draws discarded, as in the reference
    nn.GRUCell(rnn_dims + aux_dims, rnn_dims)      # get_gru_cell(self.rnn2)
    width = n_classes if mode == 'RAW' else 11
    chunk = int(max(1, min(steps, chunk_bytes // (rows * width * 4))))
    if mode == 'RAW':
        out1, out2 = torch.empty((steps, rows, n_classes), dtype=torch.float32, device=device), None
        b1 = torch.empty((chunk, rows, n_classes), dtype=torch.float32, pin_memory=pin)
        for t0 in range(0, steps, chunk):
            n = min(chunk, steps - t0)
            for t in range(n):
                b1[t].exponential_(1)
            out1[t0:t0 + n].copy_(b1[:n])
        # exponential_ may return 0 (p / q = inf in the reference: that class wins); the log-domain race needs a finite -log q
        out1.clamp_(min=1.2e-38)
    else:
        out1 = torch.empty((steps, rows, 10), dtype=torch.float32, device=device)
        out2 = torch.empty((steps, rows), dtype=torch.float32, device=device)
        b1 = torch.empty((chunk, 1, rows, 10), dtype=torch.float32, pin_memory=pin)
        b2 = torch.empty((chunk, 1, rows), dtype=torch.float32, pin_memory=pin)
        for t0 in range(0, steps, chunk):
            n = min(chunk, steps - t0)
            for t in range(n):
                b1[t].uniform_(1e-5, 1.0 - 1e-5)
                b2[t].uniform_(1e-5, 1.0 - 1e-5)
            out1[t0:t0 + n].copy_(b1[:n, 0])
            out2[t0:t0 + n].copy_(b2[:n, 0])
    return out1, out2


_NOISE_REFERENCE = -1   # host-side mode: resolved to NOISE_INJECTED with the reference's own draws before the C-ABI call
_NOISE_MODES = {'philox': _cabi.NOISE_PHILOX, 'injected': _cabi.NOISE_INJECTED, 'argmax': _cabi.NOISE_ARGMAX, 'reference': _NOISE_REFERENCE}


def _noise_mode_id(noise_mode):
    """A ``noise_mode`` argument as its id: names are looked up (``ValueError`` for an unknown one), ids pass."""
    if not isinstance(noise_mode, str):
        return noise_mode
    if noise_mode not in _NOISE_MODES:
        raise ValueError(f'noise_mode must be one of {sorted(_NOISE_MODES)} or a WRNN_NOISE_* id, got {noise_mode!r}')
    return _NOISE_MODES[noise_mode]


class WaveRNN(nn.Module):
    def __init__(self, rnn_dims, fc_dims, bits, pad, upsample_factors,
                 feat_dims, compute_dims, res_out_dims, res_blocks,
                 hop_length, sample_rate, mode='RAW'):
        super().__init__()
        self.mode = mode
        self.pad = pad
        if self.mode == 'RAW':
            self.n_classes = 2 ** bits
        elif self.mode == 'MOL':
            self.n_classes = 30
        else:
            # the reference builds the exception without raising it (:102-103) and then
            # fails on the missing n_classes; raise the same type explicitly
            raise RuntimeError("Unknown model mode value - ", self.mode)
        self.bits = bits
        self.rnn_dims = rnn_dims
        self.fc_dims = fc_dims
        self.aux_dims = res_out_dims // 4
        self.hop_length = hop_length
        self.sample_rate = sample_rate
        self.feat_dims = feat_dims
        self._ctor = dict(rnn_dims=rnn_dims, fc_dims=fc_dims, bits=bits, pad=pad,
                          upsample_factors=tuple(int(s) for s in upsample_factors), feat_dims=feat_dims,
                          compute_dims=compute_dims, res_out_dims=res_out_dims, res_blocks=res_blocks,
                          hop_length=hop_length, sample_rate=sample_rate, mode=mode)

        self.upsample = _make_upsample(feat_dims, upsample_factors, compute_dims, res_blocks, res_out_dims, pad)
        self.I = nn.Linear(feat_dims + self.aux_dims + 1, rnn_dims)
        self.rnn1 = nn.GRU(rnn_dims, rnn_dims, batch_first=True)
        self.rnn2 = nn.GRU(rnn_dims + self.aux_dims, rnn_dims, batch_first=True)
        self.fc1 = nn.Linear(rnn_dims + self.aux_dims, fc_dims)
        self.fc2 = nn.Linear(fc_dims + self.aux_dims, fc_dims)
        self.fc3 = nn.Linear(fc_dims, self.n_classes)
        self.register_buffer('step', torch.zeros(1, dtype=torch.long))
        self.num_params()

        # native state (created lazily, per device)
        self._native: Optional[_cabi.NativeVocoder] = None
        self._native_key = None
        # knobs that are not part of the reference signature
        self.kernel = _cabi.KERNEL_AUTO
        self._teamg_weights = 'f32'       # see the property teamg_weights
        self._teamg_sparse = False        # see the property teamg_sparse
        self._train_precision = 'f32'     # see the property train_precision
        # True: every training call (training_loss, forward / backward in train() mode) waits for its kernels and raises on a device-side
        # error (a busy GPU, a timed-out team kernel) -- safe, but the host cannot queue the rest of the iteration (the upsample network's
        # backward, clipping, Adam: ~150 small launches) under the running step.  'deferred': no wait; the caller asks once per iteration
        # with ``training_status()`` (``train.voc_train_loop`` does, at its ``loss.item()``, and before it writes a checkpoint).
        self.check_device_errors = True
        self.fold_min_target = 0          # target='auto': never plan folds shorter than this many samples (0: latency optimum, see fold_plan)
        self.busy_retry_seconds = 0.05   # WRNN_ERR_BUSY under AUTO: wait this long, retry the team kernel once, then fall back (loudly)
        self.verbose = True
        self.last_timing: Optional[dict] = None

    # ------------------------------------------------------------------ native
    def _device_index(self) -> int:
        dev = next(self.parameters()).device
        if dev.type == 'cuda':
            return dev.index if dev.index is not None else torch.cuda.current_device()
        if not torch.cuda.is_available():
            raise RuntimeError('WaveRNN.generate needs an MI355X (HIP) device: no GPU is visible and there is '
                               'no CPU fallback in this package')
        return torch.cuda.current_device()

    def _weights_key(self, dev: int):
        """Cheap fingerprint of the parameters the native handle was packed from: identity, in-place version counter
        and storage address of every tensor.  Catches ``load_state_dict``, optimizer steps, ``p.data = t`` (the idiom of
        the reference's ``get_gru_cell``) and ``.to()``.  Writes through ``p.data`` that keep the storage
        (``p.data.copy_()``, ``p.data.fill_()``) bump neither: call :meth:`invalidate_native` after those."""
        # `step` and BatchNorm's `num_batches_tracked` are never read by wrnn_load_weights: leaving them out keeps forward()
        # (which bumps `step` in place, :139) from repacking and re-uploading every weight on every call
        # (read from the sub-modules' own `_parameters` / `_buffers` dicts: `parameters()` + `named_buffers()` with their de-duplication
        # sets cost 0.5 ms per call, 3 % of a 19 ms single-utterance generate)
        objs = []
        for m in self.modules():
            objs.extend(m._parameters.values())
            objs.extend(b for n, b in m._buffers.items() if n != 'step' and n != 'num_batches_tracked')
        return (dev,) + tuple((id(p), p._version, p.data_ptr()) for p in objs if p is not None)

    @property
    def teamg_weights(self) -> str:
        """Element type of the weight image of ``kernel='teamg'`` / ``'teamg_batch'``: ``'f32'`` (default) or ``'f16'``.  With ``'f16'`` the six
        loop matrices are stored as IEEE binary16 (rounded to nearest even; activations, accumulators, biases and samplers stay fp32), which
        halves the bytes a team streams per step and doubles what fits in LDS.  The outputs are bit-equal to the fp32 kernel's on a model
        whose matrices were rounded to fp16 beforehand.  The setting belongs to the model: it survives ``load_state_dict`` and ``.to()``,
        the image is packed again by the next call, and no other kernel reads it (``last_timing['teamg_weights']`` says what ran).  A
        weight that has no finite fp16 makes that call raise ``WrnnError`` (WRNN_ERR_UNSUPPORTED) naming the layer.

        ``'e4m3'``: the same matrices as OCP e4m3fn bytes with one power-of-two scale per image layer (a quarter of fp32's bytes; the
        scales are found at pack time, ``native().teamg_weight_scales()``).  Bit-equal to the fp32 kernel on the dequantised model; only a
        weight that is not finite is refused."""
        return self._teamg_weights

    @teamg_weights.setter
    def teamg_weights(self, fmt: str):
        if not isinstance(fmt, str) or fmt not in _cabi.TEAMG_WEIGHT_FORMATS:
            raise ValueError(f"teamg_weights must be 'f32', 'f16' or 'e4m3', not {fmt!r}")
        self._teamg_weights = fmt
        if self._native is not None:
            self._native.set_teamg_weights(fmt)

    @property
    def teamg_sparse(self) -> bool:
        """``True``: ``kernel='teamg'`` / ``'teamg_batch'`` run the block-sparse fp32 weight image.  A block is 64 consecutive elements of
        one padded image row (``sparsity.block_layout``); the pack reads the pattern off the weights and leaves out every block whose
        weights are all zero, so a model pruned in such blocks (``sparsity.block_masks``, ``voc_train_loop(sparsify=...)``) streams and
        multiplies only what it kept.  The outputs equal the dense fp32 kernel's on the same model number for number, for any model
        (``native().teamg_sparse_info()`` says what was kept).  Default ``False``; the setting belongs to the model like ``teamg_weights``
        and no other kernel reads it (``last_timing['teamg_sparse']``).  With ``teamg_weights`` other than ``'f32'`` the call that packs
        raises ``WrnnError`` (WRNN_ERR_UNSUPPORTED)."""
        return self._teamg_sparse

    @teamg_sparse.setter
    def teamg_sparse(self, on: bool):
        if not isinstance(on, bool):
            raise ValueError(f'teamg_sparse must be a bool, not {on!r}')
        self._teamg_sparse = on
        if self._native is not None:
            self._native.set_teamg_sparse(on)

    @property
    def train_precision(self) -> str:
        """Precision of the batched GEMMs of training (``forward`` in ``train()`` mode, ``training_loss``, both autograd functions):
        ``'f32'`` (default) or ``'bf16'``.  With ``'bf16'`` every operand of those GEMMs -- forward, input gradients, weight gradients --
        is rounded once to bfloat16 (nearest even) on its way to the matrix cores; accumulators, parameters, activations in memory,
        biases, losses, the sample input's column of ``I`` and both recurrences stay fp32, and bfloat16's fp32 exponent range needs no
        loss scaling.  The setting belongs to the model like ``teamg_weights``: it survives ``invalidate_native`` and ``.to()`` and is
        applied when the native handle is made.  ``training_status()`` reports it."""
        return self._train_precision

    @train_precision.setter
    def train_precision(self, precision: str):
        if precision not in _cabi.TRAIN_PRECISIONS:
            raise ValueError(f"train_precision must be 'f32' or 'bf16', not {precision!r}")
        self._train_precision = precision
        if self._native is not None:
            self._native.set_train_precision(precision)

    def invalidate_native(self):
        """Force the next ``generate`` to repack the weights into the native handle."""
        self._native_key = None

    def _native_handle(self) -> _cabi.NativeVocoder:
        """The wrnn_handle for the current device WITHOUT (re)packing the inference weights: what ``wrnn_train_step`` needs
        (dims, mode, workspace) -- the parameters change every optimizer step and are read where torch keeps them."""
        dev = self._device_index()
        if self._native is None or self._native.device != dev:
            if self._native is not None:
                self._native.close()
            self._native = _cabi.NativeVocoder(device=dev, **self._ctor)
            self._native.set_teamg_weights(self._teamg_weights)
            self._native.set_teamg_sparse(self._teamg_sparse)
            self._native.set_train_precision(self._train_precision)
            self._native_key = None
        return self._native

    def native(self) -> _cabi.NativeVocoder:
        """The wrnn_handle for the current device, repacked if parameters changed."""
        dev = self._device_index()
        key = self._weights_key(dev)
        if self._native is None or self._native.device != dev:
            if self._native is not None:
                self._native.close()
            self._native = _cabi.NativeVocoder(device=dev, **self._ctor)
            self._native.set_teamg_weights(self._teamg_weights)
            self._native.set_teamg_sparse(self._teamg_sparse)
            self._native.set_train_precision(self._train_precision)
            self._native_key = None
        if self._native_key != key:
            sd = {k: v.detach().cpu().numpy() for k, v in self.state_dict().items()}
            self._native.load_weights(sd)
            self._native_key = key
        return self._native

    def forward(self, x, mels):
        """``forward`` of the reference (:131-167).

        * ``self.training`` and gradients enabled (what ``y_hat = model(x, m)`` is in the reference's training loop,
          ``wavernn_train.py:103-110``): the DIFFERENTIABLE pass -- BatchNorm on batch statistics like the reference module in
          train() mode, loop layers in ``wrnn_train_forward``; the returned y_hat (B, L, n_classes) carries an autograd graph whose
          backward is ``wrnn_train_backward``, so ``loss_func(y_hat, y).backward()`` with ANY torch loss fills every ``.grad``: the
          reference's training script runs unchanged (``training_loss`` fuses the script's own loss and its gradient into one call).
        * otherwise (``eval()`` or ``torch.no_grad()``): the teacher-forced pass on the hot path's own loop kernels, see below.

        Teacher-forced pass on the loop kernels: ``x`` (B, L) is the
        input sample sequence, ``mels`` (B, n_mels, T + 2*pad) the mel window already padded with ``pad`` context frames on
        both sides (what the training collate hands over, :143), L = T * hop.  Returns the fc3 outputs (B, L, n_classes) --
        logits (RAW) / mixture parameters (MOL) -- as a float32 tensor on the model's device.  Inference only (no autograd
        graph): it is the loop of ``generate`` with the fed-back value forced to ``x`` and the sampler's result ignored.
        Increments ``step`` like the reference (:139).
        """
        x_t = torch.as_tensor(x, dtype=torch.float32)
        mels_t = torch.as_tensor(mels)
        if mels_t.dim() != 3 or x_t.dim() != 2:
            raise ValueError(f'expected x (B, L) and mels (B, n_mels, T + 2*pad), got {tuple(x_t.shape)}, {tuple(mels_t.shape)}')
        T = mels_t.size(-1) - 2 * self.pad
        if T < 1 or x_t.shape != (mels_t.size(0), T * self.hop_length):
            raise ValueError(f'x must be (B, {max(T, 0) * self.hop_length}) for mels {tuple(mels_t.shape)} (pad {self.pad}, hop {self.hop_length})')
        self.step += 1
        if self.training and torch.is_grad_enabled():
            dev = next(self.parameters()).device
            if dev.type != 'cuda':
                raise RuntimeError('forward() in training mode needs the model on the MI355X (no CPU path in this package)')
            mels_up, aux = self.upsample_torch(mels_t.to(device=dev, dtype=torch.float32))
            return _LoopForwardFn.apply(self, x_t.to(device=dev).contiguous(), mels_up.contiguous(), aux.contiguous(), *self._loop_params())
        xs = x_t.detach().cpu().numpy()
        x_forced = np.zeros((xs.shape[1], xs.shape[0]), np.float32)
        x_forced[:-1] = xs[:, 1:].T                      # the value fed to step t + 1 is x[:, t + 1]
        kw = dict(noise_mode=_cabi.NOISE_ARGMAX) if self.mode == 'RAW' else \
            dict(noise_mode=_cabi.NOISE_PHILOX, seed=0)  # the drawn samples are discarded
        res = self.generate_raw(mels_t, False, 11000, 550, x_forced=x_forced, x_init=xs[:, 0], want_logits=True,
                                mels_padded=True, **kw)
        return res['logits'].permute(1, 0, 2).contiguous()

    # ---------------------------------------------------------------- training
    def upsample_torch(self, mels):
        """``self.upsample(mels)`` of the reference (UpsampleNetwork.forward :82-89, MelResNet :42-48, ResBlock :21-28,
        Stretch2d :57-61) on the framework's own ops, for TRAINING: BatchNorm follows ``self.training`` (batch statistics +
        running-stat updates in train mode) and the result carries an autograd graph, so the upsample network's parameters
        train through ``loss.backward()``.  mels (B, n_mels, T + 2*pad) -> (mels_up (B, L, n_mels), aux (B, L, res_out))."""
        r = self.upsample.resnet
        x = F.relu(r.batch_norm(r.conv_in(mels)))
        for blk in r.layers:
            res = x
            x = F.relu(blk.batch_norm1(blk.conv1(x)))
            x = blk.batch_norm2(blk.conv2(x))
            x = x + res
        aux = r.conv_out(x)                                                   # (B, res_out, T)
        aux = aux.repeat_interleave(self.hop_length, dim=2)                   # Stretch2d(total_scale, 1) (:70,:84)
        m = mels.unsqueeze(1)
        for i, s in enumerate(self._ctor['upsample_factors']):
            m = m.repeat_interleave(s, dim=3)                                 # Stretch2d(s, 1)
            m = self.upsample.up_layers[2 * i + 1](m)
        indent = self.pad * self.hop_length
        m = m.squeeze(1)[:, :, indent:-indent]
        return m.transpose(1, 2), aux.transpose(1, 2)

    def _loop_params(self):
        sd = dict(self.named_parameters())
        return [sd[k] for k in _cabi.LOOP_PARAM_KEYS]

    def training_loss(self, x, mels, y, return_logits=False):
        """One training step's forward as the reference's loop body computes it (``wavernn_train.py:103-121``):
        ``y_hat = model(x, mels)`` + ``F.cross_entropy`` (RAW) / ``discretized_mix_logistic_loss`` (MOL), as a 0-dim tensor WITH
        an autograd graph: ``loss.backward()`` fills ``.grad`` of every parameter, after which ``clip_grad_norm_`` /
        ``optimizer.step()`` work as in the reference.  The loop layers (I, rnn1, rnn2, fc1-3: 97 % of the FLOPs) run
        forward AND backward in ``wrnn_train_step`` (csrc/train.hip: batched fp32 MFMA GEMMs over all (batch, step) pairs +
        BPTT step kernels replayed from hipGraphs); the upsample network runs on the framework's ops (``upsample_torch``).
        x (B, L) float inputs, mels (B, n_mels, T + 2*pad), y (B, L) int labels (RAW) / float targets (MOL), L = T * hop.
        Increments ``step`` like ``forward`` (:139)."""
        dev = next(self.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('training_loss needs the model on the MI355X (no CPU path in this package)')
        x = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()
        mels = torch.as_tensor(mels).to(device=dev, dtype=torch.float32)
        y = torch.as_tensor(y).to(device=dev)
        y = (y.to(torch.int32) if self.mode == 'RAW' else y.to(torch.float32)).contiguous()
        T = mels.size(-1) - 2 * self.pad
        if mels.dim() != 3 or T < 1 or tuple(x.shape) != (mels.size(0), T * self.hop_length) or tuple(y.shape) != tuple(x.shape):
            raise ValueError(f'expected x, y (B, {max(T, 0) * self.hop_length}) for mels {tuple(mels.shape)}')
        self.step += 1
        mels_up, aux = self.upsample_torch(mels)
        if not torch.is_grad_enabled():   # a validation pass: forward + loss only (wrnn_train_step without gradient outputs)
            mels_up, aux = mels_up.contiguous(), aux.contiguous()
            nat = self._native_handle()
            loss = torch.empty((), dtype=torch.float32, device=dev)
            logits = torch.empty((x.size(0), x.size(1), self.n_classes), dtype=torch.float32, device=dev) if return_logits else None
            ps = [p.detach().contiguous() for p in self._loop_params()]
            with torch.cuda.device(dev):
                st = torch.cuda.current_stream(dev).cuda_stream
                nat.train_step([p.data_ptr() for p in ps], None, x.data_ptr(), mels_up.data_ptr(), aux.data_ptr(), y.data_ptr(), x.size(0), x.size(1),
                               loss.data_ptr(), logits.data_ptr() if return_logits else 0, 0, 0, st)
                if self.check_device_errors is True:
                    nat.sync_status(st)
            return (loss, logits) if return_logits else loss
        out = _LoopTrainFn.apply(self, x, y, return_logits, mels_up.contiguous(), aux.contiguous(), *self._loop_params())
        return out if return_logits else out[0]

    def training_status(self):
        """Waits for the model's stream and raises ``WrnnError`` if a training kernel launched since the last forward pass reported a
        device-side error (``wrnn_sync_status``).  For ``check_device_errors = 'deferred'``: call it once per iteration, before the weights
        of that iteration are trusted (written to a checkpoint).  Returns ``dict(train_precision=..., gemms=...)``: the precision the
        training GEMMs run in (the handle's, where there is one) and ``(on the fp32 kernel, on the bf16 kernel)`` of the last training
        call, ``None`` before any."""
        dev = next(self.parameters()).device
        if dev.type != 'cuda' or self._native is None:
            return dict(train_precision=self._train_precision, gemms=None)
        with torch.cuda.device(dev):
            self._native.sync_status(torch.cuda.current_stream(dev).cuda_stream)
        try:
            gemms = self._native.train_last_gemms()
        except _cabi.WrnnError:
            gemms = None
        return dict(train_precision=self._native.train_precision, gemms=gemms)

    # ---------------------------------------------------------------- generate
    def generate_raw(self, mels, batched, target, overlap, *, noise_mode=_cabi.NOISE_PHILOX, seed=None,
                     noise1=None, noise2=None, x_forced=None, want_logits=False, kernel=None, x_init=None,
                     mels_padded=False, frames=None, batch_rows=0, team2_segment=0, seeds=None):
        """Device part of generate() (:183-241).  Returns dict(samples (rows, L) float32 cuda tensor,
        labels (rows, L) int32 cuda tensor, logits or None, rows, steps).

        noise_mode: ``_cabi.NOISE_PHILOX`` / ``'philox'`` (device counter RNG keyed by ``seed``), ``NOISE_INJECTED`` / ``'injected'``
        (noise1 / noise2 given), ``NOISE_ARGMAX`` / ``'argmax'`` (RAW, greedy), or ``'reference'``: the draws the reference's own
        ``generate`` makes from the global torch CPU generator in its own order (``reference_noise``), injected -- under
        ``torch.manual_seed(s)`` the call then reproduces the reference's output for that seed.
        noise1/noise2/x_forced: array-likes laid out like the reference consumes them (step-major):
        RAW noise1 (L, rows, n_classes) Exp(1) draws; MOL noise1 (L, rows, 10), noise2 (L, rows).
        frames: optional (B,) valid frames per utterance of a ragged, right-zero-padded batch (``wrnn_sample_opts.frames_dev``):
        row b runs frames[b] * hop steps, the rest of its output row is left unwritten (here: zero).
        batch_rows / team2_segment: tuning knobs of the BATCH, TEAMG_BATCH / TEAM2 kernels (0 = the library's choice).
        kernel: None (the model's ``kernel``), a name of ``_cabi.KERNEL_IDS`` or a WRNN_KERNEL_* id; ``'teamg'`` / ``'teamg_batch'`` are
        the XCD-team kernels for any model dims with one / several rows per team (``last_timing['batch_rows']`` says how many ran).
        seed (default 0) keys the Philox draws of the whole call by (seed, step, row): a row's draws depend on its place in the batch.
        seeds (unbatched calls only): B ints instead, one per utterance -- row b draws exactly what a call on utterance b alone with
        ``seed=seeds[b]`` draws (same kernel), whatever else is in the batch and wherever it stands (``request_seeds``).
        """
        noise_mode = _noise_mode_id(noise_mode)
        seeds_np = None
        if seeds is not None:
            if batched:
                raise ValueError('seeds is for unbatched calls (one seed per utterance); a batched call has one utterance: use seed')
            shape = mels.shape if hasattr(mels, 'shape') else np.shape(mels)
            seeds_np = request_seeds(seeds, shape[0] if len(shape) else 0, noise_mode, seed)
        seed = 0 if seed is None else seed
        nat = self.native()
        dev = torch.device('cuda', nat.device)
        with torch.cuda.device(dev):
            mels_t = torch.as_tensor(mels).to(device=dev, dtype=torch.float32).contiguous()
            if mels_t.dim() != 3:
                raise ValueError(f'expected mels shaped (B, n_mels, T), got {tuple(mels_t.shape)}')
            B, F, T = mels_t.shape
            if mels_padded:
                T -= 2 * self.pad                        # forward()'s layout: `pad` context frames on both sides
            if F != self.feat_dims:   # the reference dies in conv_in with a channel mismatch (:43); a (T, n_mels) array lands here too
                raise ValueError(f'expected mels shaped (B, {self.feat_dims}, T), got {tuple(mels_t.shape)}')
            rows, steps = nat.plan(B, T, batched, target, overlap)
            ragged = frames is not None
            samples = (torch.zeros if ragged else torch.empty)((rows, steps), dtype=torch.float32, device=dev)
            labels = (torch.zeros if ragged else torch.empty)((rows, steps), dtype=torch.int32, device=dev)
            fr_t = None
            if ragged:
                fr_t = torch.as_tensor(frames).to(device=dev, dtype=torch.int32).contiguous()
                if tuple(fr_t.shape) != (B,):
                    raise ValueError(f'frames must have shape ({B},), got {tuple(fr_t.shape)}')
            if noise_mode == _NOISE_REFERENCE:
                if noise1 is not None or noise2 is not None:
                    raise ValueError("noise_mode='reference' draws its own noise: noise1 / noise2 must be None")
                noise1, noise2 = reference_noise(self.mode, rows, steps, self.n_classes, self.rnn_dims, self.aux_dims, dev)
                noise_mode = _cabi.NOISE_INJECTED
            logits = torch.empty((steps, rows, self.n_classes), dtype=torch.float32, device=dev) if want_logits else None

            def call(**staged):
                nat.generate(mels_t.data_ptr(), B, T, batched, target, overlap, labels_ptr=labels.data_ptr(), samples_ptr=samples.data_ptr(),
                             logits_ptr=logits.data_ptr() if logits is not None else 0, mels_padded=mels_padded,
                             frames_ptr=fr_t.data_ptr() if ragged else 0, batch_rows=batch_rows, team2_segment=team2_segment, **staged)
            self._stage_and_launch(nat, dev, call, rows, steps, noise_mode, seed, seeds_np, noise1, noise2, kernel,
                                   x_forced_ptr=(x_forced, (steps, rows)), x_init_ptr=(x_init, (rows,)))
        return dict(samples=samples, labels=labels, logits=logits, rows=rows, steps=steps, frames=fr_t)

    def _stage_and_launch(self, nat, dev, call, rows, steps, noise_mode, seed, seeds_np, noise1, noise2, kernel, **extra):
        """What ``generate_raw`` and ``generate_raw_folded`` do alike once rows and steps are known: upload the per-utterance seeds, the
        injected noise and the ``extra`` float32 arrays (keyword of the native call = (array-like or None, required shape); None becomes
        a null pointer), resolve the kernel (None: the model's; a name or a WRNN_KERNEL_* id) and run ``call(kernel=, noise_mode=,
        seed=, utt_seeds_ptr=, stream=, noise1_ptr=, noise2_ptr=, **extra pointers)`` under the busy-GPU policy.  The uploads live
        until the call has synchronised (``last_timing``)."""
        keep = []
        us = 0
        if seeds_np is not None:
            keep.append(torch.from_numpy(seeds_np.view(np.int64)).to(dev))   # the bits of the uint64 keys
            us = keep[-1].data_ptr()

        def to_dev(a, shape):
            if a is None:
                return 0
            t = torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f'expected shape {shape}, got {tuple(t.shape)}')
            keep.append(t)
            return t.data_ptr()
        nmix = self.n_classes if self.mode == 'RAW' else self.n_classes // 3
        ptrs = dict(noise1_ptr=to_dev(noise1, (steps, rows, nmix)), noise2_ptr=to_dev(noise2, (steps, rows)))
        ptrs.update((name, to_dev(a, shape)) for name, (a, shape) in extra.items())
        stream = torch.cuda.current_stream(dev).cuda_stream
        want_kernel = self.kernel if kernel is None else kernel
        if isinstance(want_kernel, str):
            want_kernel = _cabi.KERNEL_IDS[want_kernel]

        def launch(k):
            call(kernel=k, noise_mode=noise_mode, seed=int(seed), utt_seeds_ptr=us, stream=stream, **ptrs)
            return nat.last_timing()  # synchronises; surfaces device-side errors
        self._launch_with_busy_retry(nat, launch, want_kernel, steps)

    def _launch_with_busy_retry(self, nat, launch, want_kernel, steps):
        """``self.last_timing = launch(kernel)`` with the policy for a busy GPU.  Called by ``_stage_and_launch``: the slow-path warning is
        attributed to ITS caller (``generate_raw`` / ``generate_raw_folded``), four frames up."""
        try:
            self.last_timing = launch(want_kernel)
        except _cabi.WrnnError as e:
            # WRNN_ERR_BUSY: a team kernel's 32 workgroups per XCD did not all become resident (another process holds CUs).  An explicit
            # kernel request fails as it is; AUTO retries once after a moment, then runs the any-shape kernel -- loudly.
            if e.code != _cabi.ERR_BUSY or want_kernel != _cabi.KERNEL_AUTO:
                raise
            time.sleep(self.busy_retry_seconds)
            try:
                self.last_timing = launch(_cabi.KERNEL_AUTO)
            except _cabi.WrnnError as e2:
                if e2.code != _cabi.ERR_BUSY:
                    raise
                self._warn_slow_path(f'the GPU is shared with another kernel ({e2})', steps, stacklevel=4)
                self.last_timing = launch(_cabi.KERNEL_SIMPLE)
        if want_kernel == _cabi.KERNEL_AUTO and self.last_timing['kernel'] == _cabi.KERNEL_SIMPLE and not getattr(self, '_slow_warned', False):
            self._warn_slow_path(nat.team_info()[2] or 'the team kernels cannot run on this device', steps, stacklevel=4)

    def generate_raw_folded(self, mels, frames, target, overlap, *, noise_mode=_cabi.NOISE_PHILOX, seed=None, noise1=None, noise2=None,
                            kernel=None, batch_rows=0, team2_segment=0, rows_total=None, seeds=None):
        """Device part of ``generate_many(batched=True)``: ONE ``wrnn_generate_folded`` call whose rows are the folds of ALL utterances.
        mels (B, n_mels, T), every clip right-zero-padded to T frames; frames (B,) the clips' own frame counts.  Utterance b is cut as
        ``generate_raw(mels[b:b+1, :, :frames[b]], True, target, overlap)`` cuts it and owns rows fold0[b] .. fold0[b + 1] - 1.  Returns
        dict(samples, labels (rows, steps) cuda tensors, fold0 (B + 1,) int32 numpy, rows, steps, frames (cuda int32), B, target, overlap).
        noise1 / noise2 (injected): (steps, rows, .) over ALL rows.  Philox: ``seeds`` (B ints, one per utterance) keys fold i of
        utterance b by (seeds[b], step, i) -- its rows are bit-equal to ``generate_raw(clip b, True, target, overlap, seed=seeds[b])`` on the
        same kernel and batch_rows, whatever else is in the call; with the call-wide ``seed`` (default 0) a row is keyed by its GLOBAL row
        index fold0[b] + i, so a clip's audio depends on its position in the call.  rows_total: test hook, overrides the planned row
        count."""
        noise_mode = _noise_mode_id(noise_mode)
        if noise_mode == _NOISE_REFERENCE:
            raise ValueError("noise_mode='reference' replays the reference's own generate(): it has no call that folds several utterances")
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        seeds_np = None if seeds is None else request_seeds(seeds, fr.size, noise_mode, seed)
        seed = 0 if seed is None else seed
        nat = self.native()
        dev = torch.device('cuda', nat.device)
        with torch.cuda.device(dev):
            mels_t = torch.as_tensor(mels).to(device=dev, dtype=torch.float32).contiguous()
            if mels_t.dim() != 3 or mels_t.size(1) != self.feat_dims:
                raise ValueError(f'expected mels shaped (B, {self.feat_dims}, T), got {tuple(mels_t.shape)}')
            B, _, T = mels_t.shape
            if fr.shape != (B,) or fr.min() < 1 or fr.max() > T:
                raise ValueError(f'frames must be ({B},) integers in [1, {T}], got {fr.tolist()}')
            fold0, steps = _cabi.plan_folded(fr, self.hop_length, target, overlap)
            rows = int(fold0[-1]) if rows_total is None else int(rows_total)
            samples = torch.empty((rows, steps), dtype=torch.float32, device=dev)
            labels = torch.empty((rows, steps), dtype=torch.int32, device=dev)
            fr_t = torch.from_numpy(fr).to(dev)

            def call(**staged):
                nat.generate_folded(mels_t.data_ptr(), B, T, fr_t.data_ptr(), rows, target, overlap, labels_ptr=labels.data_ptr(),
                                    samples_ptr=samples.data_ptr(), batch_rows=batch_rows, team2_segment=team2_segment, **staged)
            self._stage_and_launch(nat, dev, call, rows, steps, noise_mode, seed, seeds_np, noise1, noise2, kernel)
        return dict(samples=samples, labels=labels, fold0=fold0, rows=rows, steps=steps, frames=fr_t, B=B, target=int(target), overlap=int(overlap))

    def _warn_slow_path(self, why: str, steps: int, stacklevel: int = 3):
        """Once per model: AUTO is running ``WRNN_KERNEL_SIMPLE`` (one workgroup per row, weights streamed every step, ~1 ms per step:
        ~300x slower than the team kernels and slower than the reference on a few CPU cores)."""
        if getattr(self, '_slow_warned', False):
            return
        self._slow_warned = True
        warnings.warn(f'WaveRNN: generating on the any-shape fallback kernel (WRNN_KERNEL_SIMPLE), ~1 ms per sample step -- about 300x slower '
                      f'than the XCD-team kernels ({steps} steps: ~{steps * 1e-3:.0f} s per row).  Reason: {why}.  A model of other dims runs an '
                      f"XCD-team kernel with kernel='teamg' (generate_raw(..., kernel='teamg') or model.kernel = 'teamg'), many rows at once -- folds, "
                      f"generate_many -- with kernel='teamg_batch'.", RuntimeWarning, stacklevel=stacklevel)

    def epilogue_device(self, res, batched, target, overlap, mu_law, wave_len):
        """float64 tail of generate() (:243-258) on the GPU (``wrnn_epilogue``): (wave_len,) float64 cuda tensor."""
        nat = self._native if self._native is not None else self.native()   # the tail reads no weights: no repack check
        dev = res['samples'].device
        with torch.cuda.device(dev):
            out = torch.empty((int(wave_len),), dtype=torch.float64, device=dev)
            nat.epilogue(res['samples'].data_ptr(), res['labels'].data_ptr(), res['rows'], res['steps'], batched, target,
                         overlap, mu_law, wave_len, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return out

    def fold_target_for_device(self, n_frames, overlap, device=None, policy='per_xcd'):
        """``target`` for the extension values of ``generate``'s ``target`` argument (batched mode, one utterance):
        ``'per_xcd'``: as many folds (:293-340) as the device has 32-CU teams (8 on an MI355X), one per team on the latency kernel;
        ``'auto'``: the fold count with the lowest predicted loop time (``fold_plan``: 8 folds per team on the batch kernel for clips
        of a second or more -- 2.5-3x faster than ``'per_xcd'`` -- fewer for short clips, where 2 x overlap per fold dominates)."""
        dev = device if device is not None else next(self.parameters()).device
        n = _device_teams(dev)
        total = int(n_frames) * self.hop_length
        if policy == 'per_xcd':
            return fold_target(total, int(overlap), n)
        if policy != 'auto':
            raise ValueError(f"target must be an int, 'auto' or 'per_xcd', got {policy!r}")
        return fold_plan(total, int(overlap), n, self.mode, int(self.fold_min_target))[0]

    def generate(self, mels, save_path: Union[str, Path], batched, target, overlap, mu_law, epilogue='host',
                 **native_opts):
        """Same contract as the reference ``generate`` (:169-264), including its quirks:
        generates T*hop samples but returns (T-1)*hop (:184,:257); raises ``ValueError`` for T < 21
        (fade-out broadcast, :256-258); an unbatched call with B > 1 returns only utterance 0 (:253);
        batched mode needs B == 1 (:338); MOL forces ``mu_law=False`` (:174); the return value is float64
        (:245); the model is left in train mode (:262) and a wav is always written (:260).
        Sampling draws from a device counter RNG seeded from the global torch generator, so
        ``torch.manual_seed`` makes a call reproducible like it does for the reference; ``noise_mode='reference'`` instead replays
        the reference's OWN draws from that generator (``reference_noise``): ``torch.manual_seed(s)`` + this call returns what the
        reference's ``generate`` returns for seed s on a CPU model (labels bit-equal up to a near-tie of the sampler's race).
        ``target='auto'`` (extension, batched mode): the fold length with the lowest predicted latency for ONE utterance on this
        device (``fold_plan``; a 5 s clip: 64 folds of 2 265 steps on the batch kernel, ~18 ms); ``target='per_xcd'``: one fold per XCD
        team on the latency kernel (fewest crossfades that still use the whole chip, ~48 ms).  Crossfades as in the reference's batched mode.
        ``epilogue='device'`` runs decode / unfold / fade-out on the GPU (tables built like NumPy builds them;
        identical output up to the host libm's ``pow``) instead of the float64 NumPy pass on the host.
        """
        # (the reference calls self.eval() here, :170: BatchNorm on its running statistics.  The native prologue always folds the running
        # statistics, whatever the flag says, so the ~70-module walk is left out; the observable state -- train mode on return, :262 -- is kept)
        mu_law = mu_law if self.mode == 'RAW' else False
        start = time.time()
        mels_t = torch.as_tensor(mels)
        wave_len = (mels_t.size(-1) - 1) * self.hop_length
        if isinstance(target, str):
            target = self.fold_target_for_device(mels_t.size(-1), overlap, policy=target)
        _draw_call_seed(native_opts)
        res = self.generate_raw(mels_t, batched, target, overlap, **native_opts)
        if self.verbose:
            self.gen_display(res['steps'] - 1, res['steps'], res['rows'], start)
        if epilogue == 'device':
            if wave_len < 20 * self.hop_length:
                raise _fade_broadcast_error(wave_len, self.hop_length)
            output = self.epilogue_device(res, batched, target, overlap, mu_law, wave_len).cpu().numpy()
            save_wav(output, save_path, self.sample_rate)
            self.train()
            return output
        if epilogue != 'host':
            raise ValueError(f"epilogue must be 'host' or 'device', got {epilogue!r}")
        output = self._finish_host(res['samples'].cpu().numpy().astype(np.float64), mu_law, batched, target, overlap, wave_len)
        save_wav(output, save_path, self.sample_rate)
        self.train()
        return output

    def mel_front_end(self, front_end=None, features='vocoder'):
        """The wav -> mel front end of this model (``frontend.MelFrontEnd``): the model's own ``sample_rate``, ``hop_length`` and
        ``feat_dims``, the remaining parameters (``n_fft``, ``win_length``, ``fmin``, ``min_level_db``) from the configured hparams where they
        set them, else the reference's defaults.  ``features``: the feature profile (``frontend.FEATURE_PROFILES``; one front end per
        profile is kept).  ``front_end``: use this one instead (its mel must have ``feat_dims`` channels; the features are then its own)."""
        from .frontend import MelFrontEnd
        if front_end is None:
            cache = self.__dict__.setdefault('_mel_front_ends', {})
            if features not in cache:
                from .hparams import hparams as hp
                cache[features] = MelFrontEnd(hp, sample_rate=self.sample_rate, hop_length=self.hop_length, n_mels=self.feat_dims,
                                              features=features)
            front_end = cache[features]
        if front_end.n_mels != self.feat_dims or front_end.hop_length != self.hop_length:
            raise ValueError(f'the front end makes {front_end.n_mels} mel channels at hop {front_end.hop_length}, the model needs '
                             f'{self.feat_dims} at hop {self.hop_length}')
        return front_end

    def resampler(self, wav_rate):
        """The ``frontend.Resampler`` from ``wav_rate`` to this model's ``sample_rate`` (one per source rate, kept)."""
        from .frontend import Resampler
        cache = self.__dict__.setdefault('_resamplers', {})
        if int(wav_rate) not in cache:
            cache[int(wav_rate)] = Resampler(int(wav_rate), self.sample_rate)
        return cache[int(wav_rate)]

    def generate_from_wav(self, wav, save_path: Union[str, Path], batched, target, overlap, mu_law, front_end=None, wav_rate=None,
                          trim_top_db=None, peak_norm=None, features='vocoder', **generate_opts):
        """Copy-synthesis, the ``.wav`` branch of ``wavernn_gen.py:17-20``: the mel of ``wav`` (1-D samples in [-1, 1] at the model's sample
        rate) is built on the device (``mel_front_end``) and handed to ``generate`` as a device tensor, without a host round trip.  Returns
        what ``generate`` returns for that mel: ``(T - 1) * hop`` samples, ``T = 1 + len(wav) // hop``.  ``wav_rate``: the clip's own sample
        rate; one that differs from the model's is resampled on the device first (``frontend.Resampler``), and ``len(wav)`` above is then
        the resampled length ``ceil(len * sample_rate / wav_rate)``.  ``trim_top_db`` / ``peak_norm`` (off by default): the clip is
        conditioned on the device after the resampler, as ``DeviceCorpus.from_wavs`` conditions training wavs with the same settings
        (``frontend.WavConditioner``: silence trimmed, then rescaled to the peak), and ``len(wav)`` is the trimmed length.  ``features``:
        the feature profile of the mel (``mel_front_end``); ``'tacotron'`` for a model trained on Tacotron's mels."""
        from .frontend import condition_settings
        trim_top_db, peak_norm = condition_settings(trim_top_db, peak_norm)
        fe = self.mel_front_end(front_end, features)
        dev = torch.device('cuda', self._device_index())
        if wav_rate is not None and int(wav_rate) != self.sample_rate:
            wav = self.resampler(wav_rate).resample(wav, device=dev)   # (1, n) on the device
        if trim_top_db is not None or peak_norm is not None:
            wav = self._condition_clips(wav, trim_top_db, peak_norm, dev)[0]
        mel = fe.melspectrogram(wav, device=dev)
        return self.generate(mel, save_path, batched, target, overlap, mu_law, **generate_opts)

    def _resample_clips(self, wavs, wav_rates, dev):
        """``wavs`` with every clip at another rate than the model's replaced by its resampled version on the device: one launch per
        source rate.  When anything was resampled the remaining clips go to the device too, so that the front end's ragged launch reads
        device clips only."""
        rates = [int(wav_rates)] * len(wavs) if np.ndim(wav_rates) == 0 else [int(r) for r in wav_rates]
        if len(rates) != len(wavs):
            raise ValueError(f'{len(rates)} wav_rates for {len(wavs)} clips')
        if all(r == self.sample_rate for r in rates):
            return list(wavs)
        out = [w if r != self.sample_rate else torch.as_tensor(w).to(device=dev, dtype=torch.float32) for w, r in zip(wavs, rates)]
        for rate in sorted(set(rates) - {self.sample_rate}):
            ids = [i for i, r in enumerate(rates) if r == rate]
            rs = self.resampler(rate)
            rows = rs.resample([wavs[i] for i in ids], device=dev)
            for row, n, i in zip(rows, rs.last_lens, ids):
                out[i] = row[:n]
        return out

    def _condition_clips(self, wavs, trim_top_db, peak_norm, dev):
        """``wavs`` (a list of clips, or the ``(B, n)`` rows of the resampler) conditioned on the device by one ``frontend.WavConditioner``
        call: a list of 1-D device tensors, clip i cut to its trimmed length."""
        from .frontend import WavConditioner
        cond = WavConditioner(trim_top_db, peak_norm)
        rows = cond.condition(wavs, device=dev)
        return [row[:n] for row, n in zip(rows, cond.last_lens)]

    def generate_many(self, mels_list=None, save_paths=None, mu_law=True, epilogue='host', batched=False, target='auto', overlap=550, seeds=None,
                      wavs=None, front_end=None, wav_rates=None, trim_top_db=None, peak_norm=None, features='vocoder', **native_opts):
        """Extension for serving loops: several independent utterances of different lengths in ONE device call, so that all
        8 XCD teams of the GPU work (a single unbatched utterance keeps one team = 1/8 of the chip busy; up to 8 utterances
        run on the latency kernel one per team, more on the batch kernel).  ``mels_list``: sequence of (n_mels, T_i) arrays.
        The clips are zero-padded on the right to the longest one -- exactly the padding ``generate`` itself applies
        (``pad_tensor``, :183) -- and handed over as a RAGGED batch (``frames_dev``): row i runs T_i * hop steps, the library
        orders the rows by length on the device and balances them over the XCD teams, so a short clip costs its own length, not
        the longest one's.  The first T_i * hop samples of row i are what a single ``generate`` call on clip i computes for the
        same noise.  Returns a list of float64 arrays, each what ``generate(mels_i[None], path_i, False, ...)`` returns
        ((T_i - 1) * hop samples, mu-law decoded, 20-hop fade-out); writes the wavs when ``save_paths`` is given.
        ``epilogue='device'``: decode / trim / fade-out of all rows in one ``wrnn_epilogue_rows`` launch.

        ``batched=True``: the reference's fold mode (:293-405) for ALL clips in one ``wrnn_generate_folded`` call -- every clip is cut into
        folds of one common ``target`` (an int, or ``'auto'``: ``fold_plan_many``, the target with the lowest predicted loop time for the
        whole queue) and every fold of every clip is one row of the batch kernel, so that short clips fill the chip together.  Element i
        is what ``generate(mels_i[None], path_i, True, target, overlap, mu_law)`` returns in shape, dtype and length.
        ``epilogue='device'``: crossfade / unfold / trim / fade-out of all clips in one ``wrnn_epilogue_folded`` launch.
        ``noise_mode='reference'`` raises ``ValueError``: the reference has no such call.

        Noise.  ``seeds=None``: ONE call seed (``seed=``, or a draw from the global torch generator) and rows keyed by their index in the
        call -- the audio of a clip then depends on the other clips of the queue and on its position in ``mels_list``.  ``seeds``: one int
        per clip (mod 2**64) -- clip i draws what a call on clip i ALONE with ``seed=seeds[i]`` draws, in both modes: a request can be
        replayed, reordered, queued with others or dealt to another number of GPUs (``generate_sharded`` with
        ``lambda idx, ms: model.generate_many(ms, seeds=[S[i] for i in idx])``) and sounds the same.  Not covered: ``target='auto'``
        picks the common fold length from the WHOLE queue, so a folded clip's cut -- and with it its audio -- still depends on the queue
        unless ``target`` is fixed; and bit-equality to a solo call holds on the same kernel (eight or fewer rows run TEAM2, more run
        the batch kernel) -- across kernels it is the usual parity up to near-ties of the sampler.  ``ValueError`` before any device work:
        ``seeds`` with ``seed``, a wrong length, or a ``noise_mode`` other than ``'philox'``.

        ``wavs=`` in place of ``mels_list``: a list of 1-D sample arrays; their mels are built by ONE ragged launch of the device front end
        (``mel_front_end``; clip i has ``1 + len(wavs[i]) // hop`` frames) and stay on the device.  Everything else is as for the same
        mels given as ``mels_list``.  ``wav_rates``: the clips' own sample rates, one int for all or one per clip; clips at another rate
        than the model's are resampled on the device first (``frontend.Resampler``, one launch per source rate).  ``trim_top_db`` /
        ``peak_norm`` (with ``wavs=`` only; off by default): all clips are then conditioned by one ``frontend.WavConditioner`` call, and
        the frame counts follow the trimmed lengths.  ``features`` (with ``wavs=`` only): the feature profile of the mels."""
        from .frontend import condition_settings
        trim_top_db, peak_norm = condition_settings(trim_top_db, peak_norm)
        if (mels_list is None) == (wavs is None):
            raise ValueError('give either mels_list or wavs')
        if wavs is None and (trim_top_db is not None or peak_norm is not None):
            raise ValueError('trim_top_db and peak_norm condition wavs: give wavs=, not mels_list')
        if wavs is None and features != 'vocoder':
            raise ValueError('features names the mels made from wavs: give wavs=, not mels_list')
        n_req = len(mels_list) if wavs is None else len(wavs)
        if seeds is not None:
            native_opts['seeds'] = request_seeds(seeds, n_req, native_opts.get('noise_mode', _cabi.NOISE_PHILOX), native_opts.get('seed'))
        if batched and native_opts.get('noise_mode') in ('reference', _NOISE_REFERENCE):
            raise ValueError("noise_mode='reference' replays the reference's own generate(): it has no call that folds several utterances")
        if batched and epilogue not in ('host', 'device'):
            raise ValueError(f"epilogue must be 'host' or 'device', got {epilogue!r}")
        self.eval()
        mu_law = mu_law if self.mode == 'RAW' else False
        if wavs is not None:
            fe = self.mel_front_end(front_end, features)
            if not len(wavs):
                raise ValueError('expected a non-empty sequence of clips')
            if wav_rates is not None:
                wavs = self._resample_clips(wavs, wav_rates, torch.device('cuda', self._device_index()))
            if trim_top_db is not None or peak_norm is not None:
                wavs = self._condition_clips(list(wavs), trim_top_db, peak_norm, torch.device('cuda', self._device_index()))
            lens = [fe.frames(int(np.shape(w)[0])) for w in wavs]
            arrs = lens   # one entry per clip; the mels themselves are made on the device below
        else:
            arrs = [np.asarray(torch.as_tensor(m).detach().cpu().numpy(), dtype=np.float32) for m in mels_list]
            if not arrs or any(a.ndim != 2 or a.shape[0] != self.feat_dims for a in arrs):
                raise ValueError(f'expected a non-empty sequence of (n_mels={self.feat_dims}, T_i) arrays')
            lens = [a.shape[1] for a in arrs]
        if min(lens) < 21:   # raised before any device work
            raise _fade_broadcast_error((min(lens) - 1) * self.hop_length, self.hop_length)
        tmax = max(lens)
        if wavs is not None:
            batch = fe.melspectrogram(list(wavs), device=torch.device('cuda', self._device_index()))   # (B, n_mels, tmax) on the device, zero past each clip
        else:
            batch = np.zeros((len(arrs), self.feat_dims, tmax), np.float32)
            for i, a in enumerate(arrs):
                batch[i, :, :lens[i]] = a
        if seeds is None:
            _draw_call_seed(native_opts)
        ragged = len(set(lens)) > 1
        if batched:
            outs = self._generate_many_folded(batch, lens, mu_law, epilogue, target, overlap, native_opts)
            if save_paths is not None:
                for out, path in zip(outs, save_paths):
                    save_wav(out, path, self.sample_rate)
            self.train()
            return outs
        res = self.generate_raw(batch, False, 11000, 550, frames=np.asarray(lens, np.int32) if ragged else None, **native_opts)
        if epilogue == 'device':
            outs = self._finish_device(res, lens, lambda nat, waves, wl_max, st: nat.epilogue_rows(
                res['samples'].data_ptr(), res['labels'].data_ptr(), res['rows'], res['steps'], mu_law, wl_max,
                res['frames'].data_ptr() if ragged else 0, waves, wl_max, st))
        elif epilogue == 'host':
            samples = res['samples'].cpu().numpy().astype(np.float64)
            outs = [self._finish_host(samples[i:i + 1, :t_i * self.hop_length], mu_law, False, 0, 0, (t_i - 1) * self.hop_length)
                    for i, t_i in enumerate(lens)]
        else:
            raise ValueError(f"epilogue must be 'host' or 'device', got {epilogue!r}")
        if save_paths is not None:
            for out, path in zip(outs, save_paths):
                save_wav(out, path, self.sample_rate)
        self.train()
        return outs

    def _generate_many_folded(self, batch, lens, mu_law, epilogue, target, overlap, native_opts):
        """``generate_many(batched=True)`` behind the argument checks: batch (B, n_mels, max T) zero-padded, lens the clips' frames."""
        hop = self.hop_length
        if isinstance(target, str):
            if target != 'auto':
                raise ValueError(f"target must be an int or 'auto', got {target!r}")
            target = fold_plan_many([t * hop for t in lens], int(overlap), _device_teams(next(self.parameters()).device), self.mode,
                                    int(self.fold_min_target))[0]
        res = self.generate_raw_folded(batch, lens, int(target), int(overlap), **native_opts)
        fold0 = res['fold0']
        if epilogue == 'device':
            return self._finish_device(res, lens, lambda nat, waves, wl_max, st: nat.epilogue_folded(
                res['samples'].data_ptr(), res['labels'].data_ptr(), len(lens), res['rows'], res['steps'], res['target'], res['overlap'], mu_law,
                res['frames'].data_ptr(), waves, wl_max, st))
        samples = res['samples'].cpu().numpy().astype(np.float64)   # (rows, steps)   :243-245
        return [self._finish_host(samples[fold0[i]:fold0[i + 1]], mu_law, True, res['target'], res['overlap'], (t_i - 1) * hop)
                for i, t_i in enumerate(lens)]

    def _finish_host(self, rows_f64, mu_law, batched, target, overlap, wave_len):
        """float64 host tail of the reference's generate() (:243-258) for one clip: rows_f64 (rows, L) are its loop outputs -- its folds
        when batched, else row 0 is the clip.  Decode mu-law, crossfade and unfold, trim to wave_len = (T - 1) * hop, fade the last
        20 hops out (a shorter clip raises the reference's broadcast ``ValueError`` here).  May write into rows_f64."""
        out = decode_mu_law(rows_f64, self.n_classes, False) if mu_law else rows_f64
        out = self.xfade_and_unfold(out, target, overlap) if batched else out[0]
        out = out[:wave_len]
        out[-20 * self.hop_length:] *= np.linspace(1, 0, 20 * self.hop_length)
        return out

    def _finish_device(self, res, lens, epilogue):
        """Device tail of ``generate_many``: ``epilogue(nat, waves_ptr, wl_max, stream)`` -- one ``nat.epilogue_*`` launch -- fills a
        (clips, wl_max) float64 buffer, wl_max = the longest clip's (T - 1) * hop; returns clip i's first (T_i - 1) * hop samples."""
        nat = self.native()
        dev = res['samples'].device
        wl_max = (max(lens) - 1) * self.hop_length
        with torch.cuda.device(dev):
            waves = torch.empty((len(lens), wl_max), dtype=torch.float64, device=dev)
            epilogue(nat, waves.data_ptr(), wl_max, torch.cuda.current_stream(dev).cuda_stream)
        waves = waves.cpu().numpy()
        return [waves[i, :(t_i - 1) * self.hop_length].copy() for i, t_i in enumerate(lens)]

    def stream(self, batch=1, mu_law=True, seed=None, noise_mode='philox', kernel=None, tail='reference', raw=False,
               batched=False) -> 'VocoderStream':
        """Streaming generation (extension): a :class:`VocoderStream` that takes mel frames as they arrive (``push``) and returns
        the audio they make final.  Fed the frames of a mel (B, n_mels, T) in any partition into pushes and then ``finish()``-ed,
        its labels / samples are bit-identical to ``generate_raw(mels, False, ..., noise_mode, seed, kernel)`` and, with
        ``tail='reference'``, its float64 audio (concatenated) to what ``generate(mels[0:1], path, False, ..., mu_law)`` returns
        after the same ``torch.manual_seed``: ``seed=None`` draws the Philox seed from the global torch generator exactly as
        ``generate`` does.  ``tail='reference'`` holds the last 21 hops back until ``finish()`` (the trim to (T - 1) * hop and the
        20-hop fade-out need the end); ``tail='none'`` returns every decoded sample as soon as it exists, all T * hop of them,
        untrimmed and unfaded (lowest latency).  ``raw=True``: push / finish return dict(labels, samples) device tensors (B, n).
        noise_mode: 'philox' or 'argmax' (RAW).  The reference's own noise ('reference', 'injected') needs the whole clip's draws,
        and batched (fold) mode needs the whole clip to cut it into folds: both raise ``ValueError``.  kernel: None (the
        model's ``kernel``, AUTO: TEAM2 where the team kernels can run, else SIMPLE -- with a warning), 'team2' / 'simple' or a
        WRNN_KERNEL_* id.  A busy GPU (WRNN_ERR_BUSY) is raised, not retried on another kernel."""
        if batched:
            raise ValueError('batched (fold) generation needs the whole clip to cut it into folds: a stream is unbatched')
        return VocoderStream(self, batch=batch, mu_law=mu_law, seed=seed, noise_mode=noise_mode, kernel=kernel, tail=tail, raw=raw)

    def generate_stream(self, mel_chunks, **kw):
        """Generator over ``stream(**kw)``: yields ``push(chunk)`` for every chunk of ``mel_chunks`` ((n_mels, k) or
        (B, n_mels, k) each), then ``finish()``."""
        with self.stream(**kw) as st:
            for chunk in mel_chunks:
                yield st.push(chunk)
            yield st.finish()

    def gen_display(self, i, seq_len, b_size, start):
        """The reference's own ksamples/s meter (:267-271)."""
        gen_rate = (i + 1) / (time.time() - start) * b_size / 1000
        sys.stdout.write(f'\r| {(i + 1) * b_size}/{seq_len * b_size} | Batch Size: {b_size} | '
                         f'Gen Rate: {gen_rate:.1f}kHz | ')

    def xfade_and_unfold(self, y, target, overlap):
        """Equal-power crossfade + overlap-add of the folds (:342-405), float64 on the host."""
        num_folds, length = y.shape
        target = length - 2 * overlap
        total_len = num_folds * (target + overlap) + overlap
        silence_len = overlap // 2
        fade_len = overlap - silence_len
        ramp = np.linspace(-1, 1, fade_len, dtype=np.float64)
        fade_in = np.concatenate([np.zeros(silence_len, dtype=np.float64), np.sqrt(0.5 * (1 + ramp))])
        fade_out = np.concatenate([np.ones(silence_len, dtype=np.float64), np.sqrt(0.5 * (1 - ramp))])
        y[:, :overlap] *= fade_in
        y[:, -overlap:] *= fade_out
        unfolded = np.zeros(total_len, dtype=np.float64)
        for i in range(num_folds):
            lo = i * (target + overlap)
            unfolded[lo:lo + target + 2 * overlap] += y[i]
        return unfolded

    # ------------------------------------------------------------ bookkeeping
    def get_step(self):
        return self.step.data.item()

    def log(self, path, msg):
        with open(path, 'a') as f:
            print(msg, file=f)

    def load(self, path: Union[str, Path]):
        device = next(self.parameters()).device
        self.load_state_dict(torch.load(path, map_location=device), strict=False)

    def save(self, path: Union[str, Path]):
        torch.save(self.state_dict(), path)

    def num_params(self, print_out=True):
        n = sum(int(np.prod(p.size())) for p in self.parameters() if p.requires_grad) / 1_000_000
        if print_out:
            print('Trainable Parameters: %.3fM' % n)
        return n


class _LoopTrainFn(torch.autograd.Function):
    """loss = L(loop layers(x, mels_up, aux; params)) with forward and backward in ``wrnn_train_step``."""

    @staticmethod
    def forward(ctx, model, x, y, want_logits, mels_up, aux, *params):
        nat = model._native_handle()
        dev = x.device
        B, L = x.shape
        grads = [torch.empty_like(p) for p in params]
        d_m, d_a = torch.empty_like(mels_up), torch.empty_like(aux)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        logits = torch.empty((B, L, model.n_classes), dtype=torch.float32, device=dev) if want_logits else None
        ps = [p.detach().contiguous() for p in params]
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.train_step([p.data_ptr() for p in ps], [g.data_ptr() for g in grads], x.data_ptr(), mels_up.data_ptr(), aux.data_ptr(),
                           y.data_ptr(), B, L, loss.data_ptr(), logits.data_ptr() if want_logits else 0, d_m.data_ptr(), d_a.data_ptr(), st)
            model._train_generation = getattr(model, '_train_generation', 0) + 1   # the workspace now holds THIS pass (see _LoopForwardFn)
            if model.check_device_errors is True:
                nat.sync_status(st)   # waits for the stream: a busy GPU / a timed-out team kernel raises here, not as a silent NaN
        ctx.save_for_backward(d_m, d_a, *grads)
        if want_logits:
            ctx.mark_non_differentiable(logits)
            return loss, logits
        return (loss,)

    @staticmethod
    def backward(ctx, g_loss, *unused):
        d_m, d_a, *grads = ctx.saved_tensors
        return (None, None, None, None, d_m * g_loss, d_a * g_loss) + tuple(g * g_loss for g in grads)


class _LoopForwardFn(torch.autograd.Function):
    """y_hat = loop layers(x, mels_up, aux; params): ``wrnn_train_forward`` / ``wrnn_train_backward`` (activations stay in the handle's
    workspace between the two, so backward must be the next training call on the model -- what a training loop does)."""

    @staticmethod
    def forward(ctx, model, x, mels_up, aux, *params):
        nat = model._native_handle()
        dev = x.device
        B, L = x.shape
        logits = torch.empty((B, L, model.n_classes), dtype=torch.float32, device=dev)
        ps = [p.detach().contiguous() for p in params]
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.train_forward([p.data_ptr() for p in ps], x.data_ptr(), mels_up.data_ptr(), aux.data_ptr(), B, L, logits.data_ptr(), st)
            if model.check_device_errors is True:
                nat.sync_status(st)
        # the activations of this pass live in the handle's ONE workspace: stamp the pass, so that a backward that comes after another
        # training call on the model (a second forward, a validation batch through training_loss, gradient accumulation over two forwards)
        # fails loudly instead of differentiating the other pass (round-3 advisor finding)
        model._train_generation = getattr(model, '_train_generation', 0) + 1
        ctx.generation = model._train_generation
        ctx.model = model
        ctx.save_for_backward(x, mels_up, aux, *ps)
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        x, mels_up, aux, *ps = ctx.saved_tensors
        model = ctx.model
        if getattr(model, '_train_generation', 0) != ctx.generation:
            raise RuntimeError('WaveRNN: another training call on this model ran between this forward and its backward; the forward\'s '
                               'activations (kept in the native handle\'s single workspace) are gone.  Call backward() before the next '
                               'forward / training_loss, or use training_loss() (forward + backward in one native call).')
        nat = model._native_handle()
        dev = x.device
        B, L = x.shape
        grads = [torch.empty_like(p) for p in ps]
        d_m, d_a = torch.empty_like(mels_up), torch.empty_like(aux)
        dl = d_logits.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.train_backward([p.data_ptr() for p in ps], [g.data_ptr() for g in grads], dl.data_ptr(), x.data_ptr(), mels_up.data_ptr(),
                               aux.data_ptr(), B, L, d_m.data_ptr(), d_a.data_ptr(), st)
            if model.check_device_errors is True:
                nat.sync_status(st)
        return (None, None, d_m, d_a) + tuple(grads)


def stream_release(frames_in: int, steps_done: int, last: bool, hop: int, tail: str = 'reference') -> int:
    """Audio samples of a stream that are final after ``frames_in`` frames and ``steps_done`` generated steps.  tail='none': every
    generated sample.  tail='reference': sample m once it cannot lie in the last 21 hops -- the trim to (T - 1) * hop and the
    20-hop fade-out of generate() (:255-258) -- i.e. m < (frames_in - 21) * hop; at the end (``last``) all (T - 1) * hop."""
    if tail == 'none':
        return int(steps_done)
    if last:
        return (int(frames_in) - 1) * int(hop)
    return min(max((int(frames_in) - 21) * int(hop), 0), int(steps_done))


class VocoderStream:
    """One utterance (or B in lock-step) generated while its mel frames arrive: see :meth:`WaveRNN.stream`.

    ``push(mels)`` takes the next frames, (n_mels, k) or (B, n_mels, k) (numpy or torch, k >= 0), runs every loop step that has
    become ready (``wrnn_stream_ready_steps``: (frames_in - pad) * hop rounded down to 32 steps before the end), waits for them
    and returns the newly final float64 audio, (n,) for ``batch=1`` else (B, n); ``finish()`` ends the utterance and returns the
    rest.  A device-side error raises ``WrnnError`` and leaves the stream unusable; a push after ``finish()`` raises
    ``WrnnError`` (WRNN_ERR_STATE).  ``close()`` (or leaving the ``with`` block) frees the native stream."""

    def __init__(self, model: 'WaveRNN', *, batch, mu_law, seed, noise_mode, kernel, tail, raw):
        if tail not in ('reference', 'none'):
            raise ValueError(f"tail must be 'reference' or 'none', got {tail!r}")
        noise_mode = _noise_mode_id(noise_mode)
        if noise_mode not in (_cabi.NOISE_PHILOX, _cabi.NOISE_ARGMAX):
            raise ValueError("a stream draws its noise on the device (noise_mode 'philox' or 'argmax'): 'reference' / 'injected' "
                             "noise needs the draws of the whole clip up front")
        if noise_mode == _cabi.NOISE_ARGMAX and model.mode != 'RAW':
            raise ValueError("noise_mode='argmax' is RAW-only")
        if int(batch) < 1:
            raise ValueError(f'batch must be >= 1, got {batch}')
        if isinstance(kernel, str):
            if kernel not in ('auto', 'team2', 'simple'):
                raise ValueError(f"a stream runs kernel 'auto', 'team2' or 'simple', got {kernel!r}")
            kernel = _cabi.KERNEL_IDS[kernel]
        kernel = model.kernel if kernel is None else int(kernel)
        if seed is None:
            # what generate() does (its native_opts['seed']): one draw from the global torch generator, philox only
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise_mode == _cabi.NOISE_PHILOX else 0
        self.model, self.B, self.tail, self.raw = model, int(batch), tail, bool(raw)
        self.mu_law = bool(mu_law) if model.mode == 'RAW' else False   # MOL forces mu_law=False (:174)
        self.hop, self.pad, self.seed = model.hop_length, model.pad, int(seed)
        self._nat = model.native()
        self._dev = torch.device('cuda', self._nat.device)
        if kernel == _cabi.KERNEL_AUTO:
            ok, _, why = self._nat.team_info()
            if not ok:
                model._warn_slow_path(why or 'the team kernels cannot run on this device', 0)
        with torch.cuda.device(self._dev):
            self._ns = _cabi.NativeStream(self._nat, self.B, noise_mode=noise_mode, seed=self.seed, kernel=kernel)
        self.frames_in = 0        # mel frames pushed
        self.steps = 0            # loop steps generated (per row)
        self.released = 0         # audio samples returned (per row)
        self._pending = np.zeros((self.B, 0), np.float64)   # decoded samples [released, steps) held back (tail='reference')
        self._ended = False

    # ------------------------------------------------------------------ api
    def push(self, mels):
        return self._push(mels, last=False)

    def finish(self):
        return self._push(None, last=True)

    def info(self) -> dict:
        """frames_in, steps_done, workspace_bytes (device memory the native stream owns)."""
        return self._ns.info()

    def close(self):
        if self._ns is not None:
            self._ns.close()
            self._ns = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ internals
    def _mels(self, mels):
        t = torch.as_tensor(mels)
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or t.size(0) != self.B or t.size(1) != self.model.feat_dims:
            raise ValueError(f'expected mels shaped ({self.model.feat_dims}, k) or ({self.B}, {self.model.feat_dims}, k), got {tuple(torch.as_tensor(mels).shape)}')
        return t

    def _push(self, mels, last):
        if self._ns is None:
            raise _cabi.WrnnError(-3, 'the stream is closed')
        t = self._mels(mels) if mels is not None else None
        k = 0 if t is None else int(t.size(-1))
        hop = self.hop
        if last and self.tail == 'reference' and self.frames_in + k < 21 and not self._ended:
            wave_len = (self.frames_in + k - 1) * hop   # the fade-out broadcast error of generate() (:256-258)
            raise ValueError(f'operands could not be broadcast together with shapes ({max(wave_len, 0)},) '
                             f'({20 * hop},) ({max(wave_len, 0)},)')
        n = max(_cabi.stream_ready_steps(self.frames_in + k, hop, self.pad, last) - self.steps, 0)
        with torch.cuda.device(self._dev):
            mels_d = t.to(device=self._dev, dtype=torch.float32).contiguous() if k else None
            labels = torch.empty((self.B, max(n, 1)), dtype=torch.int32, device=self._dev)
            samples = torch.empty((self.B, max(n, 1)), dtype=torch.float32, device=self._dev)
            st = torch.cuda.current_stream(self._dev).cuda_stream
            got = self._ns.push(mels_d.data_ptr() if k else 0, k, last, labels.data_ptr(), samples.data_ptr(), labels.numel(), st)
            self._ns.sync(st)   # waits; raises WrnnError for a device-side error (busy GPU, timeout)
            del mels_d
        if got != n:
            raise RuntimeError(f'internal: the native stream ran {got} steps, the host planned {n}')
        self.frames_in += k
        self.steps += got
        self._ended = self._ended or last
        labels, samples = labels[:, :got], samples[:, :got]
        if self.raw:
            return dict(labels=labels, samples=samples)
        audio = samples.cpu().numpy().astype(np.float64)   # :243-245
        if self.mu_law:
            audio = decode_mu_law(audio, self.model.n_classes, False)
        if self.tail == 'none':
            return self._shape(audio)
        self._pending = np.concatenate([self._pending, audio], axis=1)
        upto = stream_release(self.frames_in, self.steps, last, hop, self.tail)
        out = self._pending[:, :upto - self.released]
        self._pending = self._pending[:, upto - self.released:]
        if last:
            fade_from = upto - 20 * hop - self.released   # >= 0: nothing past (T - 21) * hop was released before
            out[:, fade_from:] *= np.linspace(1, 0, 20 * hop)
            self._pending = np.zeros((self.B, 0), np.float64)
        self.released = upto
        return self._shape(out)

    def _shape(self, a):
        return a[0] if self.B == 1 else a
