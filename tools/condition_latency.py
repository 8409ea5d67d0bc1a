#!/usr/bin/env python
"""Time the wav conditioning on the device (csrc/condition.hip) and what it adds to preprocessing a corpus, in one session.

    python tools/condition_latency.py [--iters 200] [--warmup 20] [--clips 200] [--out profiles/condition.txt]

1. The launches: one 5 s clip, and a ragged queue of 8 clips, already on the device; HIP events around one `condition_padded` call at a
   time after a warm-up (the lengths' copy, the allocations, the three launches), median and min / max, for trimming + peak, trimming alone
   and peak alone.  Next to the queue: the NumPy restatement (tests/condition_ref.py) of the same 8 clips on at most 16 host threads.
2. Preprocessing: 200 synthetic clips of 2 to 8 s (the tones of tools/resample_latency.py between a leading and a trailing stretch of
   noise floor), `DeviceCorpus.from_wavs` with the conditioning off, with it on, and with it off on clips the NumPy restatement
   conditioned on the host first (its time included: the only other way to the same corpus); wall clock around a call that ends in a
   device synchronise, median of 5 runs each, alternating.  The two conditioned corpora are compared for equality."""
import argparse
import os
import sys
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.resample_latency import clip as tones, timed   # noqa: E402


def clip(n, seed, rate=22050):
    """Tones between 10 % to 25 % of noise floor (amplitude 1e-3) at either end."""
    rng = np.random.Generator(np.random.PCG64(seed + 5 * 10 ** 6))
    lead, tail = (int(f * n) for f in rng.uniform(0.10, 0.25, 2))
    x = rng.uniform(-1e-3, 1e-3, n).astype(np.float32)
    x[lead:n - tail] += 0.8 * tones(n - lead - tail, seed, rate)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--clips', type=int, default=200)
    ap.add_argument('--skip-corpus', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('condition_latency.py measures on an MI355X: no GPU, no figures')
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd import dataset as D
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd, WavConditioner
    from tests import condition_ref as cr
    dev = torch.device('cuda', 0)
    threads = min(16, os.cpu_count() or 1)
    settings = (('trim 25 dB + peak', 25.0, True), ('trim 25 dB alone', 25.0, None), ('peak alone', None, True))
    lines = [f'wav conditioning, {torch.cuda.get_device_name(0)}, torch {torch.__version__}, library {os.path.relpath(_cabi.LIB_PATH, ROOT)}', '',
             f'1. the launches alone: HIP events, {args.warmup} warm-up + {args.iters} timed calls, microseconds; clips already on the device',
             '   (condition_padded: the lengths\' copy, three allocations, energy + decision + gather launches)']
    one_host = clip(5 * 22050, 1)
    one = torch.from_numpy(one_host).to(dev).view(1, -1)
    fe = MelFrontEnd(device=dev)
    m = timed(lambda: fe.melspectrogram_padded(one, [one.shape[1]]), args.iters, args.warmup)
    for label, top_db, peak in settings:
        c = WavConditioner(top_db, peak, device=dev)
        o = timed(lambda: c.condition_padded(one, [one.shape[1]]), args.iters, args.warmup)
        c.condition(one)
        moved = 4.0 * ((4 * one.shape[1] if top_db else 0) + 2 * c.last_lens[0] + one.shape[1])   # every frame reads 2048 samples at hop 512; peak; gather in; out
        lines.append(f'   one 5 s clip ({one.shape[1]} samples -> {c.last_lens[0]}), {label:18s}: median {o[0]:7.1f} (min {o[1]:.1f}, max {o[2]:.1f})'
                     f'   = {moved / o[0] / 1e3:.1f} GB/s of the bytes the three launches ask for')
    lines.append(f'   for scale, the mel front end on the same clip: median {m[0]:.1f}')
    lens = [int(s * 22050) for s in (5.0, 1.5, 2.14, 4.08, 2.74, 3.4, 4.58, 2.36)]
    queue_host = [clip(n, 10 + i) for i, n in enumerate(lens)]
    queue = torch.zeros((8, max(lens)), dtype=torch.float32, device=dev)
    for i, n in enumerate(lens):
        queue[i, :n] = torch.from_numpy(queue_host[i]).to(dev)
    for label, top_db, peak in settings:
        c = WavConditioner(top_db, peak, device=dev)
        o = timed(lambda: c.condition_padded(queue, lens), args.iters, args.warmup)
        lines.append(f'   ragged queue of 8 clips (1.5 to 5 s), {label:18s}: median {o[0]:7.1f} (min {o[1]:.1f}, max {o[2]:.1f})')
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            host_out = list(ex.map(lambda x: cr.condition(x, 25.0, 0.999)[0], queue_host))
        runs.append(time.perf_counter() - t0)
    c = WavConditioner(25.0, True, device=dev)
    got = c.condition(queue_host).cpu().numpy()
    same = all(np.array_equal(got[i, :c.last_lens[i]].view(np.uint32), y.view(np.uint32)) for i, y in enumerate(host_out))
    lines.append(f'   the same queue through the NumPy restatement on {threads} host threads, trim 25 dB + peak: median of 5 runs {np.median(runs) * 1e6:9.1f} '
                 f'(min {min(runs) * 1e6:.1f}); device output bit-equal to it: {same}')
    if not args.skip_corpus:
        hp = types.SimpleNamespace(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100,
                                   bits=10, mu_law=True, voc_mode='RAW', voc_pad=2, voc_seq_len=1375)
        rng = np.random.Generator(np.random.PCG64(0))
        clips = [clip(int(n), i) for i, n in enumerate(rng.integers(2 * 22050, 8 * 22050, size=args.clips))]
        seconds = sum(x.shape[0] for x in clips) / 22050.0
        lines += ['', f'2. preprocessing: {args.clips} synthetic clips of 2 to 8 s, {seconds:.0f} s of audio, already decoded in host memory; DeviceCorpus.from_wavs,',
                  f'   wall clock to a device synchronise, median of 5 runs after a warm-up call, the three ways alternating; host = NumPy restatement on {threads} threads']

        def off():
            return D.DeviceCorpus.from_wavs(clips, hp, 'cuda', batch_clips=batch_clips)

        def on():
            return D.DeviceCorpus.from_wavs(clips, hp, 'cuda', batch_clips=batch_clips, trim_top_db=25, peak_norm=True)

        def host():
            with ThreadPoolExecutor(threads) as ex:
                done = list(ex.map(lambda x: cr.condition(x, 25.0, 0.999)[0], clips))
            return D.DeviceCorpus.from_wavs(done, hp, 'cuda', batch_clips=batch_clips)

        batch_clips = 16
        D.DeviceCorpus.from_wavs(clips[:8], hp, 'cuda')
        D.DeviceCorpus.from_wavs(clips[:8], hp, 'cuda', trim_top_db=25, peak_norm=True)
        torch.cuda.synchronize()
        for batch_clips in (16, 64):
            runs = {'off': [], 'device': [], 'host': []}
            kept = {}
            for _ in range(5):
                for name, fn in (('off', off), ('device', on), ('host', host)):
                    t0 = time.perf_counter()
                    kept[name] = fn()
                    torch.cuda.synchronize()
                    runs[name].append(time.perf_counter() - t0)
            med = {k: float(np.median(v)) for k, v in runs.items()}
            equal = torch.equal(kept['device'].labels, kept['host'].labels) and torch.equal(kept['device'].mels, kept['host'].mels)
            lines.append(f'   batch_clips={batch_clips:2d}: conditioning off {med["off"]:6.3f} s (min {min(runs["off"]):.3f}, max {max(runs["off"]):.3f});  '
                         f'on the device {med["device"]:6.3f} s (min {min(runs["device"]):.3f}, max {max(runs["device"]):.3f}) = {seconds / med["device"]:6.0f} x real time;  '
                         f'on the host first {med["host"]:6.3f} s (min {min(runs["host"]):.3f}, max {max(runs["host"]):.3f});  '
                         f'device / off {med["device"] / med["off"]:.2f}, host / device {med["host"] / med["device"]:.2f};  '
                         f'{len(kept["device"])} utterances, {kept["device"].hours * 3600:.0f} s kept of {kept["off"].hours * 3600:.0f} s, '
                         f'the two conditioned corpora equal: {equal}')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
