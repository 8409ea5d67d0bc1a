#!/usr/bin/env python
"""Time the training-data side on the MI355X: preprocessing a corpus on the device, and what one batch costs next to the 22 ms step.

    python tools/loader_latency.py [--clips 200] [--epochs 30] [--out profiles/device_loader.txt]

1. Preprocessing: a synthetic corpus of `--clips` clips of 2 to 8 s (seeded sums of sinusoids plus noise) held in host memory ->
   `DeviceCorpus.from_wavs` (upload, mel front end, `wrnn_quantise`, packing), wall clock around a call that ends in a device
   synchronise, after one warm-up call on a few clips, median of 5 runs.  Reported as a multiple of real time.  Reading and decoding wav files is not in it.
2. Time per batch at the hp defaults (B = 32, seq_len 1 375, hop 275, pad 2, RAW 10 bits), one session, after a warm-up epoch, a device
   synchronise after every batch, alternating the two loaders epoch by epoch:
   (a) the path of the parent commit: `WindowLoader` over the `.npy` files `save` wrote (np.load of 2 B files, stack on the host) plus the
       three `.to(device)` copies `voc_train_loop` makes;
   (b) `DeviceWindowLoader` over the resident corpus: one small copy of (utterance, offset) and one `wrnn_collate_windows` launch.
   The batches of the two are checked to be bit-equal in the first epoch."""
import argparse
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tacotronv2_wavernn_chinese_amd import dataset as D, train as T  # noqa: E402

STEP_MS = 22.0   # wrnn_train_step at B = 32 x 1 375 (profiles/r03_train_step_kernel_stats.txt)


def clip(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / 22050.0
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.3, 0.2, 0.1), rng.uniform(100, 3000, 3), rng.uniform(0, 6.28, 3)))
    return np.clip(x + 0.02 * rng.standard_normal(n), -1, 1).astype(np.float32)


def per_batch(loader, to_device):
    """Milliseconds of every batch of one epoch, each ending in a device synchronise."""
    ms, it = [], iter(loader)
    while True:
        t0 = time.perf_counter()
        try:
            x, y, m = next(it)
        except StopIteration:
            return ms
        if to_device:
            x, m, y = x.to('cuda'), m.to('cuda'), y.to('cuda')   # what voc_train_loop does with a host batch
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=200)
    ap.add_argument('--epochs', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('loader_latency.py measures on an MI355X: no GPU, no figures')
    hp = types.SimpleNamespace(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100,
                               bits=10, mu_law=True, voc_mode='RAW', voc_pad=2, voc_seq_len=1375)
    kw = dict(mode='RAW', bits=10, hop_length=275, pad=2, seq_len=1375)
    rng = np.random.Generator(np.random.PCG64(0))
    clips = [clip(int(n), i) for i, n in enumerate(rng.integers(2 * 22050, 8 * 22050, size=args.clips))]
    seconds = sum(len(c) for c in clips) / 22050.0
    lines = [f'training data on the device, {torch.cuda.get_device_name(0)}, torch {torch.__version__}', '',
             f'1. preprocessing: {args.clips} synthetic clips of 2 to 8 s, {seconds:.0f} s of audio ({seconds / 3600:.3f} h), already decoded in host memory']
    D.DeviceCorpus.from_wavs(clips[:8], hp, 'cuda')   # warm-up: code objects, the front end's tables, the allocator
    torch.cuda.synchronize()
    for batch_clips in (16, 64):
        runs = []
        for _ in range(5):
            t0 = time.perf_counter()
            corpus = D.DeviceCorpus.from_wavs(clips, hp, 'cuda', batch_clips=batch_clips)
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        dt = float(np.median(runs))
        lines.append(f'   from_wavs(batch_clips={batch_clips:2d}): median of 5 runs {dt:6.3f} s wall (min {min(runs):.3f}, max {max(runs):.3f}) = {seconds / dt:7.0f} x real time; {len(corpus)} utterances, '
                     f'{(corpus.labels.numel() * 4 + corpus.mels.numel() * 4) / 2 ** 20:.0f} MiB resident '
                     f'({(corpus.labels.numel() * 4 + corpus.mels.numel() * 4) / 2 ** 20 / (seconds / 3600):.0f} MiB per hour)')
    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        listing = corpus.save(td)
        lines.append(f'   save (device -> {len(corpus)} x 2 .npy files + list): {time.perf_counter() - t0:.2f} s')
        files, _ = T.read_feature_list(listing, seq_len=1375, hop_length=275, pad=2, test_samples=0)
        t0 = time.perf_counter()
        resident = D.DeviceCorpus.load(files, 'cuda', hop_length=275)
        torch.cuda.synchronize()
        lines.append(f'   load (the list back onto the device): {time.perf_counter() - t0:.2f} s')
        host = T.WindowLoader(files, 32, seed=1, **kw)
        dev = D.DeviceWindowLoader(resident, 32, seed=1, **kw)
        same = all(torch.equal(a.cpu(), b) for da, ho in zip(dev, host) for a, b in zip(da, ho))   # also the warm-up epoch of both
        a_ms, b_ms = [], []
        for _ in range(args.epochs):
            a_ms += per_batch(host, True)
            b_ms += per_batch(dev, False)
    a_ms, b_ms = np.asarray(a_ms), np.asarray(b_ms)
    lines += ['', f'2. one batch, B = 32 x 1 375 (mels 32 x 80 x 9), wall clock to a device synchronise, {args.epochs} epochs of {len(host)} batches each '
                  f'after a warm-up epoch, loaders alternating; first-epoch batches bit-equal: {same}',
              f'   (a) WindowLoader over .npy files + 3 .to(device): median {np.median(a_ms):7.3f} ms  (min {a_ms.min():.3f}, p90 {np.percentile(a_ms, 90):.3f}, max {a_ms.max():.3f}; '
              f'the files are in the page cache)',
              f'   (b) DeviceWindowLoader:                           median {np.median(b_ms):7.3f} ms  (min {b_ms.min():.3f}, p90 {np.percentile(b_ms, 90):.3f}, max {b_ms.max():.3f})',
              f'   next to the {STEP_MS:.0f} ms training step: (a) {np.median(a_ms) / STEP_MS * 100:.1f} %, (b) {np.median(b_ms) / STEP_MS * 100:.2f} %; (a) / (b) = {np.median(a_ms) / np.median(b_ms):.1f}',
              f'   condition "(b) is not slower than (a)": {"met" if np.median(b_ms) <= np.median(a_ms) else "NOT met"}']
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
