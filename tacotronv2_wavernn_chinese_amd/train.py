"""The caller of the training step: the vocoder training loop and its checkpoint files.

What ``wavernn_train.py:88-151`` does with a ``WaveRNN`` and a loader of ``(x, y, mels)`` batches (``collate_vocoder``,
``wavernn/utils/dataset.py:107-133``), and what ``wavernn/utils/checkpoints.py:28-78,81-138`` write next to it -- the same two
files per checkpoint (``*_weights.pyt`` = ``model.state_dict()``, ``*_optim.pyt`` = ``optimizer.state_dict()``) at the same
places (``logs_wavernn/checkpoints/latest_*.pyt`` + ``wave_step{k}K_*.pyt``, ``wavernn/utils/paths.py:11-17``), so a run can be
resumed by either code base and ``wavernn_gen.py`` finds the weights where it looks for them.

``train_set`` is any sized iterable of ``(x, y, mels)``; ``collate_windows`` below builds such batches on the host from ``(mel,
quantised wav)`` pairs the way the reference's collate cuts its windows (``.npy`` files of a training list, or in-memory arrays as the
tests and ``--synthetic`` use them).  ``dataset.py`` makes the list from a folder of wavs and serves the same batches from a corpus
resident on the device (``--wav_dir``, ``--resident``).

The iteration itself is ``WaveRNN.training_loss`` (one ``wrnn_train_step``: forward, loss and backward of the loop layers on
the MI355X) unless a ``loss_func`` is given, in which case the loop body is the reference's own
``loss_func(model(x, m), y)`` through the differentiable ``forward()``.
"""
from __future__ import annotations

import time
from pathlib import Path
from typing import Callable, Iterable, Optional, Sequence, Tuple, Union

import numpy as np
import torch


class VocPaths:
    """The vocoder half of ``Paths`` (``wavernn/utils/paths.py:5-32``), rooted at ``base`` instead of the package's parent."""

    def __init__(self, base: Union[str, Path] = '.', create: bool = True):
        self.base = Path(base).expanduser().resolve()
        self.voc_checkpoints = self.base / 'logs_wavernn' / 'checkpoints'
        self.voc_latest_weights = self.voc_checkpoints / 'latest_weights.pyt'
        self.voc_latest_optim = self.voc_checkpoints / 'latest_optim.pyt'
        self.voc_output = self.base / 'logs_wavernn' / 'model_outputs'
        self.voc_log = self.voc_checkpoints / 'log.txt'
        if create:
            self.voc_checkpoints.mkdir(parents=True, exist_ok=True)
            self.voc_output.mkdir(parents=True, exist_ok=True)

    def named(self, name: Optional[str]) -> Tuple[Path, Path]:
        """(weights file, optimizer file) of the latest (``name=None``) or a named checkpoint."""
        if name is None:
            return self.voc_latest_weights, self.voc_latest_optim
        return self.voc_checkpoints / f'{name}_weights.pyt', self.voc_checkpoints / f'{name}_optim.pyt'


def _write_pair(files: Tuple[Path, Path], model, optimizer):
    have = [f.exists() for f in files]
    if have[0] != have[1]:          # checkpoints.py:45-49: a half-written checkpoint is an error, not something to overwrite
        raise FileNotFoundError(f'checkpoint {files[0].name} / {files[1].name}: exactly one of the two files exists')
    files[0].parent.mkdir(parents=True, exist_ok=True)
    model.save(files[0])
    torch.save(optimizer.state_dict(), files[1])


def save_checkpoint(paths: VocPaths, model, optimizer, *, name: Optional[str] = None):
    """``save_checkpoint('voc', ...)`` (checkpoints.py:28-78): always refresh ``latest_*``; with ``name`` also write the named pair."""
    _write_pair(paths.named(None), model, optimizer)
    if name:
        _write_pair(paths.named(name), model, optimizer)


def restore_checkpoint(paths: VocPaths, model, optimizer, *, name: Optional[str] = None, create_if_missing: bool = False):
    """``restore_checkpoint('voc', ...)`` (checkpoints.py:81-138).  Call after ``model.to(device)``: the optimizer state lands
    on the device of the parameters it belongs to."""
    w, o = paths.named(name)
    if w.exists() and o.exists():
        model.load(w)
        optimizer.load_state_dict(torch.load(o, map_location=next(model.parameters()).device))
    elif create_if_missing:
        save_checkpoint(paths, model, optimizer, name=name)
    else:
        raise FileNotFoundError(f'no {"named" if name else "latest"} checkpoint at {w}')


def label_2_float(x, bits: int):
    """dsp.py:36 of the reference: class index -> [-1, 1]."""
    return 2.0 * x / (2 ** bits - 1.0) - 1.0


def draw_window_offsets(frames: Sequence[int], *, hop_length: int, pad: int, seq_len: int, rng: np.random.Generator):
    """The random part of one batch (dataset.py:108-110): for utterances of ``frames`` mel frames, in order, the first mel frame of
    each one's window, one ``rng.integers(0, room)`` per utterance.  The one place the draws are made: ``collate_windows`` and
    ``dataset.DeviceWindowLoader`` both call it, so with the same generator they cut the same windows.  ``ValueError`` for a
    ``seq_len`` that is no multiple of the hop and for an utterance too short for a window."""
    if seq_len % hop_length:
        raise ValueError('seq_len must be a multiple of hop_length')
    win = seq_len // hop_length + 2 * pad
    offs = []
    for n in frames:
        room = int(n) - 2 - (win + 2 * pad)
        if room <= 0:
            raise ValueError(f'an utterance of {int(n)} frames is too short for a window of {win} (+{2 * pad + 2})')
        offs.append(int(rng.integers(0, room)))
    return offs


def collate_windows(batch: Sequence[Tuple[np.ndarray, np.ndarray]], *, mode: str, bits: int, hop_length: int, pad: int,
                    seq_len: int, rng: np.random.Generator):
    """One training batch from ``(mel (n_mels, frames), quantised wav (frames * hop,) of class indices)`` pairs: a random window of
    ``seq_len`` samples + the ``pad`` context frames either side per pair (dataset.py:107-133).  Returns (x, y, mels) as the loop
    wants them: x (B, seq_len) floats in [-1, 1], y (B, seq_len) the next-sample targets (int64 classes for RAW, floats of a
    16-bit signal for MOL), mels (B, n_mels, seq_len / hop + 2 * pad)."""
    offs = draw_window_offsets([mel.shape[-1] for mel, _ in batch], hop_length=hop_length, pad=pad, seq_len=seq_len, rng=rng)
    win = seq_len // hop_length + 2 * pad
    mels, labels = [], []
    for (mel, wav), off in zip(batch, offs):
        s0 = (off + pad) * hop_length
        mels.append(mel[:, off:off + win])
        labels.append(wav[s0:s0 + seq_len + 1])
    mels = torch.from_numpy(np.stack(mels).astype(np.float32))
    labels = torch.from_numpy(np.stack(labels).astype(np.int64))
    sig_bits = 16 if mode == 'MOL' else bits
    x = label_2_float(labels[:, :seq_len].float(), sig_bits)
    y = labels[:, 1:]
    if mode == 'MOL':
        y = label_2_float(y.float(), sig_bits)
    return x, y, mels


def voc_train_loop(paths: VocPaths, model, loss_func: Optional[Callable], optimizer, train_set: Iterable, test_set, lr: float,
                   total_steps: int, *, clip_grad_norm: Optional[float] = 4, checkpoint_every: int = 1000,
                   at_checkpoint: Optional[Callable] = None, report: Optional[Callable[[str], None]] = None, sparsify=None):
    """``voc_train_loop`` (wavernn_train.py:88-151) on the MI355X.

    ``loss_func=None``: each iteration is ``model.training_loss(x, m, y)`` (forward + loss + backward of the loop layers fused
    in ``wrnn_train_step``).  With a ``loss_func`` (``F.cross_entropy`` / a MOL loss on torch tensors) the body is the
    reference's (:103-121): ``y_hat = model(x, m)``, the transpose / unsqueeze that fit torch's loss signatures, ``loss_func``.
    ``clip_grad_norm`` / ``checkpoint_every`` are ``hp.voc_clip_grad_norm`` / ``hp.voc_checkpoint_every``; ``at_checkpoint(model,
    test_set, step)`` stands where the reference calls ``gen_testset`` (:137-138); ``report`` receives the progress line
    (``stream(msg)``, :145).  Returns the list of per-iteration losses of this call.
    Deferred device errors (``check_device_errors='deferred'``): ``training_status()`` raises AFTER ``optimizer.step()`` of the failing
    iteration has run on whatever the step produced -- nothing corrupt reaches disk (no checkpoint is written behind a raised error), but the
    in-memory parameters and Adam moments are then poisoned: restore the latest checkpoint (``restore_checkpoint``) before continuing, do
    not just retry the iteration.
    ``sparsify``: a ``sparsity.SparsitySchedule``.  After ``optimizer.step()`` of a step at which the schedule is due the block masks are
    recomputed (``sparsity.block_masks`` at the schedule's density, intersected with the masks so far: a pruned block stays pruned), and
    the masks are re-applied after every step, so the pruned blocks are exactly zero in every checkpoint.  Training itself stays dense.
    """
    device = next(model.parameters()).device
    for g in optimizer.param_groups:
        g['lr'] = lr
    per_epoch = len(train_set)
    if per_epoch < 1:
        raise ValueError('voc_train_loop: the training set is empty')
    epochs = (total_steps - model.get_step()) // per_epoch + 1
    params = [p for p in model.parameters() if p.requires_grad]
    losses = []
    masks = None
    if sparsify is not None:
        from .sparsity import apply_masks_, block_masks
    model.train()
    # Device-side errors of the training kernels are asked for once per iteration (at the loss.item() below, where the host waits anyway)
    # instead of inside every call, and the NaN message of the clipping waits for the same point: the host queues the upsample network's
    # backward, the clipping and Adam while the step is still running.  An error raises before the iteration's weights can reach a
    # checkpoint.
    check_mode, model.check_device_errors = getattr(model, 'check_device_errors', True), 'deferred'
    try:
        for epoch in range(1, epochs + 1):
            t0 = time.time()
            running = 0.0
            msg = ''
            for i, (x, y, m) in enumerate(train_set, 1):
                x, m, y = x.to(device), m.to(device), y.to(device)
                if loss_func is None:
                    loss = model.training_loss(x, m, y)
                else:
                    y_hat = model(x, m)
                    if model.mode == 'RAW':
                        y_hat = y_hat.transpose(1, 2).unsqueeze(-1)
                    else:
                        y = y.float()
                    loss = loss_func(y_hat, y.unsqueeze(-1))
                optimizer.zero_grad()
                loss.backward()
                norm = torch.nn.utils.clip_grad_norm_(params, clip_grad_norm) if clip_grad_norm is not None else None
                optimizer.step()
                if sparsify is not None:
                    if sparsify.due(model.get_step()):
                        masks = block_masks(model, sparsify.density(model.get_step()), sparsify.layers, keep=masks)
                    if masks is not None:
                        apply_masks_(model, masks)
                value = loss.item()                  # the one host sync of an iteration (the reference has it too, :129)
                if hasattr(model, 'training_status'):
                    model.training_status()
                if norm is not None and not bool(torch.isfinite(norm)):
                    print('grad_norm was NaN!')
                losses.append(value)
                running += value
                step = model.get_step()
                if step % checkpoint_every == 0:
                    if at_checkpoint is not None:
                        at_checkpoint(model, test_set, step)
                        model.train()
                    save_checkpoint(paths, model, optimizer, name=f'wave_step{step // 1000}K')
                msg = (f'| Epoch: {epoch}/{epochs} ({i}/{per_epoch}) | Loss: {running / i:.4f} | '
                       f'{i / (time.time() - t0):.1f} steps/s | Step: {step // 1000}k | ')
                if report is not None:
                    report(msg)
            save_checkpoint(paths, model, optimizer)     # the optimizer state of the epoch's end, so resuming does not jump (:147-149)
            model.log(paths.voc_log, msg)
    finally:
        model.check_device_errors = check_mode
    return losses


# --------------------------------------------------------------------------- the data side of the loop
def read_feature_list(feature_path: Union[str, Path], *, seq_len: int, hop_length: int, pad: int, test_samples: int):
    """The training list ``get_vocoder_datasets`` reads (dataset.py:62-88): one ``wav.npy|...|mel.npy`` line per utterance (field 0
    the quantised wav, field 2 the (frames, n_mels) mel), utterances too short for one window dropped, ids shuffled with seed
    1234 and the last ``test_samples`` set aside.  Returns (train pairs, test pairs) of (wav path, mel path)."""
    import random
    win = seq_len // hop_length + 2 * pad
    items = []
    with open(feature_path, 'r', encoding='utf-8') as f:
        for line in f:
            parts = line.strip().split('|')
            if len(parts) < 3:
                continue
            wav, mel = parts[0].strip(), parts[2].strip()
            if np.load(mel, mmap_mode='r').shape[0] - (win + 2 * pad + 2) < 0:
                continue
            items.append((wav, mel))
    ids = list(range(len(items)))
    random.Random(1234).shuffle(ids)
    if test_samples:
        return [items[i] for i in ids[:-test_samples]], [items[i] for i in ids[-test_samples:]]
    return [items[i] for i in ids], []


class WindowLoader:
    """The train ``DataLoader`` of dataset.py:90-95 as the loop sees it: a sized iterable, shuffled per epoch, each batch a fresh
    random window per utterance (``collate_windows``).  ``pairs`` are (wav path, mel path) of ``.npy`` files or in-memory
    (mel (n_mels, frames), wav) arrays; a last short batch is kept, like the reference's loader."""

    def __init__(self, pairs, batch_size: int, *, mode: str, bits: int, hop_length: int, pad: int, seq_len: int, seed: int = 0):
        self.pairs, self.batch_size = list(pairs), int(batch_size)
        self.kw = dict(mode=mode, bits=bits, hop_length=hop_length, pad=pad, seq_len=seq_len)
        self.rng = np.random.Generator(np.random.PCG64(seed))

    def __len__(self):
        return (len(self.pairs) + self.batch_size - 1) // self.batch_size

    @staticmethod
    def _arrays(pair):
        a, b = pair
        if isinstance(a, (str, Path)):
            return np.load(b).T, np.load(a)           # VocoderDataset.__getitem__ (dataset.py:52-57): files hold (frames, n_mels)
        return a, b

    def __iter__(self):
        order = self.rng.permutation(len(self.pairs))
        for i in range(0, len(order), self.batch_size):
            yield collate_windows([self._arrays(self.pairs[j]) for j in order[i:i + self.batch_size]], rng=self.rng, **self.kw)


def synthetic_pairs(n: int, frames: int, *, bits: int, n_mels: int, hop_length: int, seed: int = 0):
    """``n`` in-memory (mel, quantised wav) pairs of a slow random walk: stands in for a corpus (there is none in this repository)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(n):
        walk = np.cumsum(rng.integers(-3, 4, size=frames * hop_length)) + 2 ** (bits - 1)
        out.append((rng.random((n_mels, frames), dtype=np.float32), (walk % 2 ** bits).astype(np.int64)))
    return out


def checkpoint_generator(hp, paths: VocPaths, scorer=None, pitch=None):
    """The ``at_checkpoint`` of the command line: ``gen_testset`` (dataset.py:18-43), vocode a few held-out mels next to the checkpoint.
    ``scorer``: a ``frontend.SpectralScore``; every generated clip is then scored against its decoded target (both are in memory) and
    ``step, clip, mel_lsd_db, mcd_db, mr_sc, mr_logmag`` is appended to ``checkpoints/scores.txt``.  ``None``: nothing else is written.
    ``pitch``: a ``frontend.PitchScore`` (with a scorer only); ``f0_rmse_cents gpe vde`` of the pair then follow on the same line."""
    def at_checkpoint(mod, test_set, step):
        from .dsp import decode_mu_law, label_2_float, save_wav
        k = step // 1000
        batch_str = f'gen_batched_target{hp.voc_target}_overlap{hp.voc_overlap}' if hp.voc_gen_batched else 'gen_NOT_BATCHED'
        rows = []
        for i, pair in enumerate(test_set[:hp.voc_gen_at_checkpoint], 1):
            mel, x = WindowLoader._arrays(pair)       # (wav path, mel path) of .npy files, or in-memory (mel (n_mels, frames), labels)
            # the quantised target (:28-37): decoded and kept next to the generated file, as the reference does
            bits = 16 if hp.voc_mode == 'MOL' else hp.bits
            x = decode_mu_law(x, 2 ** bits, from_labels=True) if (hp.mu_law and hp.voc_mode != 'MOL') else label_2_float(x.astype(np.float64), bits)
            save_wav(x, paths.voc_output / f'{k}k_steps_{i}_target.wav', hp.sample_rate)
            m = torch.from_numpy(np.ascontiguousarray(mel, dtype=np.float32)).unsqueeze(0)
            wav = mod.generate(m, str(paths.voc_output / f'{k}k_steps_{i}_{batch_str}.wav'), hp.voc_gen_batched, hp.voc_target,
                               hp.voc_overlap, hp.mu_law)
            if scorer is not None:
                s = scorer.score(np.asarray(x, np.float32), np.asarray(wav, np.float32), device=next(mod.parameters()).device)[0]
                row = f"{step} {i} {s['mel_lsd_db']:.6f} {s['mcd_db']:.6f} {s['mr_sc']:.6f} {s['mr_logmag']:.6f}"
                if pitch is not None:
                    p = pitch.score(np.asarray(x, np.float32), np.asarray(wav, np.float32), device=next(mod.parameters()).device)[0]
                    row += f" {p['f0_rmse_cents']:.6f} {p['gpe']:.6f} {p['vde']:.6f}"
                rows.append(row + '\n')
        if rows:
            with open(paths.voc_checkpoints / 'scores.txt', 'a') as fh:
                fh.writelines(rows)
    return at_checkpoint


def build_parser():
    import argparse
    from .hparams import DEFAULT_HPARAMS
    parser = argparse.ArgumentParser(description='Train WaveRNN Vocoder')
    parser.add_argument('--gta', '-g', action='store_true', help='accepted for compatibility: the list file names the mels to train on')
    parser.add_argument('--hp_file', metavar='FILE', default=DEFAULT_HPARAMS, help='The file to use for the hyperparameters')
    parser.add_argument('--synthetic', type=int, metavar='N', default=0, help='train on N synthetic utterances instead of hp.feature_path')
    parser.add_argument('--wav_dir', metavar='DIR', help='train on the wav files of a folder: mels and labels are made on the device and stay '
                                                         'there (dataset.DeviceCorpus), every batch is cut by one kernel launch')
    parser.add_argument('--resample', action='store_true', help='with --wav_dir: resample files at another rate to hp.sample_rate on the '
                                                                'device (default: such a file is an error)')
    from .frontend import add_condition_arguments, add_features_argument
    add_condition_arguments(parser, 'the --wav_dir files')
    add_features_argument(parser, 'the --wav_dir files; a saved corpus (hp.feature_path) must hold the same ones')
    from .dataset import add_gta_arguments
    add_gta_arguments(parser)   # --gta_checkpoint ...: GTA mels for the --wav_dir corpus; --gta / -g above stays what it is
    parser.add_argument('--resident', action='store_true', help='load the corpus of hp.feature_path onto the device once instead of reading '
                                                                '.npy files every iteration')
    parser.add_argument('--train-precision', dest='train_precision', choices=('f32', 'bf16'), default='f32',
                        help="precision of the loop layers' batched GEMMs: f32 (default), or bf16 operands on the matrix cores with fp32 "
                             'accumulators (WaveRNN.train_precision; parameters, recurrences and losses stay fp32)')
    parser.add_argument('--sparse-density', dest='sparse_density', type=float, metavar='D', default=None,
                        help='extension: prune rnn1, rnn2, fc1 and fc2 while training, in blocks of 64 weights of a row, down to the share D '
                             'of blocks per row (sparsity.SparsitySchedule; needs --sparse-start and --sparse-end).  The checkpoints run on '
                             'wavernn_gen.py --kernel teamg --teamg-sparse')
    parser.add_argument('--sparse-start', dest='sparse_start', type=int, metavar='S', default=None, help='step at which pruning begins')
    parser.add_argument('--sparse-end', dest='sparse_end', type=int, metavar='E', default=None, help='step at which the density reaches D')
    parser.add_argument('--sparse-every', dest='sparse_every', type=int, metavar='N', default=100,
                        help='recompute the masks every N steps between S and E (default 100)')
    parser.add_argument('--total_steps', type=int, help='override hp.voc_total_steps')
    parser.add_argument('--score_at_checkpoint', action='store_true',
                        help='extension: at every checkpoint, score each generated held-out clip against its target on the device '
                             '(frontend.SpectralScore) and append "step clip mel_lsd_db mcd_db mr_sc mr_logmag" to '
                             'logs_wavernn/checkpoints/scores.txt (default: off; with --synthetic, hp.voc_gen_at_checkpoint more synthetic '
                             'utterances are held out for it)')
    parser.add_argument('--score_pitch', action='store_true',
                        help='extension, with --score_at_checkpoint: also append "f0_rmse_cents gpe vde" (frontend.PitchScore, a YIN track of '
                             'both clips on the device) to each line of scores.txt (default: off)')
    parser.add_argument('--reference_body', action='store_true',
                        help="run the reference's loop body (model(x, m) + torch loss) instead of the fused training_loss")
    return parser


def sparsity_schedule(args):
    """The ``sparsity.SparsitySchedule`` of the --sparse-* arguments, or ``None`` without --sparse-density (``ValueError`` for half a set)."""
    if args.sparse_density is None:
        if args.sparse_start is not None or args.sparse_end is not None:
            raise ValueError('--sparse-start / --sparse-end need --sparse-density')
        return None
    if args.sparse_start is None or args.sparse_end is None:
        raise ValueError('--sparse-density needs --sparse-start and --sparse-end')
    from .sparsity import SparsitySchedule
    return SparsitySchedule(args.sparse_density, args.sparse_start, args.sparse_end, args.sparse_every)


def main(argv=None):
    """``python wavernn_train.py`` (wavernn_train.py:20-86) on the MI355X."""
    import torch.nn.functional as F
    from .frontend import condition_arguments
    from .gen import build_model_from_hparams
    from .hparams import hparams as hp
    args = build_parser().parse_args(argv)
    if args.score_pitch and not args.score_at_checkpoint:
        raise ValueError('--score_pitch extends --score_at_checkpoint: give both')
    conditioning = condition_arguments(args)
    sparsify = sparsity_schedule(args)
    from .dataset import gta_arguments
    want_gta = gta_arguments(args)
    hp.configure(args.hp_file)
    if not args.synthetic and not args.wav_dir:
        from .dataset import check_saved_features
        check_saved_features(hp.feature_path, args.features)   # ValueError: the saved mels are of another kind than the ones asked for
    if not torch.cuda.is_available():
        raise RuntimeError('this vocoder trains on an MI355X only (no CPU path)')
    if int(np.prod(hp.voc_upsample_factors)) != hp.hop_length:
        raise ValueError('voc_upsample_factors must factorise hop_length')
    paths = VocPaths('.')
    model = build_model_from_hparams().to(torch.device('cuda'))
    model.train_precision = args.train_precision
    optimizer = torch.optim.Adam(model.parameters())
    restore_checkpoint(paths, model, optimizer, create_if_missing=True)
    kw = dict(mode=hp.voc_mode, bits=hp.bits, hop_length=hp.hop_length, pad=hp.voc_pad, seq_len=hp.voc_seq_len)
    if args.synthetic:
        sig_bits = 16 if hp.voc_mode == 'MOL' else hp.bits
        train, test = synthetic_pairs(args.synthetic, 40, bits=sig_bits, n_mels=hp.num_mels, hop_length=hp.hop_length), []
        if args.score_at_checkpoint:   # the synthetic run holds nothing out: utterances of another seed stand in, the training set stays
            test = synthetic_pairs(hp.voc_gen_at_checkpoint, 40, bits=sig_bits, n_mels=hp.num_mels, hop_length=hp.hop_length, seed=1)
    elif args.wav_dir:
        from .dataset import DeviceCorpus
        wavs = sorted(Path(args.wav_dir).expanduser().glob('*.wav'))
        if not wavs:
            raise FileNotFoundError(f'no *.wav files in {args.wav_dir}')
        corpus = DeviceCorpus.from_wavs(wavs, hp, 'cuda', resample=args.resample, features=args.features, **conditioning)
        print(f'{len(corpus)} utterances of {len(wavs)} files | {corpus.hours:.3f} hours | {corpus.n_clipped} clipped samples')
        if want_gta:   # train on the mels the Tacotron will hand the vocoder; nothing is written
            from .dataset import gta_from_arguments
            corpus = gta_from_arguments(corpus, args)
        train, held_out = corpus.split(hp.voc_test_samples)
        test = held_out.pairs()
    else:
        train, test = read_feature_list(hp.feature_path, seq_len=hp.voc_seq_len, hop_length=hp.hop_length, pad=hp.voc_pad,
                                        test_samples=hp.voc_test_samples)
        if args.resident:
            from .dataset import DeviceCorpus
            train = DeviceCorpus.load(train, 'cuda', hop_length=hp.hop_length, features=args.features)
    if isinstance(train, list):
        loader = WindowLoader(train, hp.voc_batch_size, **kw)
    else:
        from .dataset import DeviceWindowLoader
        loader = DeviceWindowLoader(train, hp.voc_batch_size, **kw)
    total = args.total_steps if args.total_steps is not None else hp.voc_total_steps
    print(f'Remaining {total - model.get_step()} steps | batch {hp.voc_batch_size} | lr {hp.voc_lr} | seq_len {hp.voc_seq_len} | '
          f'{len(train)} training utterances | GEMMs in {model.train_precision}')
    loss_func = None
    if args.reference_body:
        if hp.voc_mode != 'RAW':
            raise ValueError('--reference_body: pass your own MOL loss to voc_train_loop; the CLI only carries F.cross_entropy')
        loss_func = F.cross_entropy

    scorer = None
    if args.score_at_checkpoint:
        from .frontend import SpectralScore
        scorer = SpectralScore(hp, features=args.features)
    pitch = None
    if args.score_pitch:
        from .frontend import PitchScore
        pitch = PitchScore(hp)
    at_checkpoint = checkpoint_generator(hp, paths, scorer, pitch)

    voc_train_loop(paths, model, loss_func, optimizer, loader, test, hp.voc_lr, total,
                   clip_grad_norm=hp.voc_clip_grad_norm, checkpoint_every=hp.voc_checkpoint_every, at_checkpoint=at_checkpoint,
                   report=lambda s: print('\r' + s, end='', flush=True), sparsify=sparsify)
    print('\nTraining Complete.')


if __name__ == "__main__":
    main()
