#!/usr/bin/env python
"""Time the device resampler (csrc/resample.hip) and what it adds to preprocessing a corpus, in one session.

    python tools/resample_latency.py [--iters 200] [--warmup 20] [--clips 200] [--lib build_variants/libX.so] [--out profiles/resample.txt]

1. The kernel: one 5 s clip at 48 kHz and at 44.1 kHz (and a ragged queue of 8 clips at 48 kHz) already on the device -> 22.05 kHz, HIP
   events around one call at a time after a warm-up, median and min / max; also the kernel's error against the float64 restatement
   (tests/resample_ref.py) on the parity inputs of tests/test_gpu_resample.py.
2. Preprocessing: the 200 synthetic clips of tools/loader_latency.py (2 to 8 s), supplied at 22.05 kHz (the path without the resampler)
   and the same signals sampled at 48 kHz with `from_wavs(resample=True)`, wall clock around a call that ends in a device synchronise,
   median of 5 runs each, alternating.
3. scipy.signal.resample_poly(x, 147, 320) on the host for the same 48 kHz clips, a pool of at most 16 threads: another filter (not an
   oracle), the only host resampler at hand."""
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


def clip(n, seed, rate):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / float(rate)
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.3, 0.2, 0.1), rng.uniform(100, 3000, 3), rng.uniform(0, 6.28, 3)))
    return np.clip(x + 0.02 * np.random.Generator(np.random.PCG64(seed + 10 ** 6)).standard_normal(n), -1, 1).astype(np.float32)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.asarray(ms) * 1e3
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--clips', type=int, default=200)
    ap.add_argument('--lib', default=None, help='a variant of the library (tools/build_variant.sh)')
    ap.add_argument('--skip-corpus', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('resample_latency.py measures on an MI355X: no GPU, no figures')
    from tacotronv2_wavernn_chinese_amd import _cabi
    if args.lib:
        _cabi.LIB_PATH = os.path.abspath(args.lib)
    from tacotronv2_wavernn_chinese_amd import dataset as D
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd, Resampler
    from tests import mel_ref as mr, resample_ref as rr
    dev = torch.device('cuda', 0)
    lines = [f'resampler, {torch.cuda.get_device_name(0)}, torch {torch.__version__}, library {os.path.relpath(_cabi.LIB_PATH, ROOT)}', '',
             'parity against tests/resample_ref.py in float64 (g = max |ref32 - ref64|, the bound of tests/test_gpu_resample.py is 8 g)']
    from tests.test_gpu_resample import INPUTS, RATIOS, _input, _ref
    for src, dst in RATIOS:
        rs = Resampler(src, dst, device=dev)
        for name in INPUTS:
            x = _input(name)
            r64, g = _ref(x, src, dst)
            err = np.abs(rs.resample(x)[0].cpu().numpy().astype(np.float64) - r64).max()
            lines.append(f'  {src:5d} -> {dst:5d}  {name:12s} outputs {r64.shape[0]:5d}  g {g:.3e}  kernel error {err:.3e} = {err / g:.2f} g')
    lines += ['', f'1. the kernel alone: HIP events, {args.warmup} warm-up + {args.iters} timed calls, microseconds; clips already on the device',
              '   (resample_padded: the lengths\' copy, the output\'s allocation, the launch and the kernel)']
    fe = MelFrontEnd(device=dev)
    for src in (48000, 44100, 16000):
        rs = Resampler(src, 22050, device=dev)
        one = torch.from_numpy(clip(5 * src, 1, src)).to(dev).view(1, -1)
        o = timed(lambda: rs.resample_padded(one, [one.shape[1]]), args.iters, args.warmup)
        out = rs.resample_padded(one, [one.shape[1]])
        m = timed(lambda: fe.melspectrogram_padded(out, [out.shape[1]]), args.iters, args.warmup)
        flop = 2.0 * out.shape[1] * rs.taps
        lines.append(f'   one 5 s clip {src:5d} -> 22050 ({rs.p} x {rs.taps} bank, {one.shape[1]} -> {out.shape[1]} samples): median {o[0]:7.1f} (min {o[1]:.1f}, max {o[2]:.1f})'
                     f'   = {flop / o[0] / 1e3:.1f} GFLOP/s; the mel front end on its output: median {m[0]:.1f}')
    rs = Resampler(48000, 22050, device=dev)
    lens = [int(s * 48000) for s in (5.0, 1.5, 2.14, 4.08, 2.74, 3.4, 4.58, 2.36)]
    queue = torch.zeros((8, max(lens)), dtype=torch.float32, device=dev)
    for i, n in enumerate(lens):
        queue[i, :n] = torch.from_numpy(clip(n, 10 + i, 48000)).to(dev)
    o = timed(lambda: rs.resample_padded(queue, lens), args.iters, args.warmup)
    lines.append(f'   ragged queue of 8 clips (1.5 to 5 s) 48000 -> 22050, one launch: median {o[0]:7.1f} (min {o[1]:.1f}, max {o[2]:.1f})')
    if not args.skip_corpus:
        hp = types.SimpleNamespace(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100,
                                   bits=10, mu_law=True, voc_mode='RAW', voc_pad=2, voc_seq_len=1375)
        rng = np.random.Generator(np.random.PCG64(0))
        n22 = [int(n) for n in rng.integers(2 * 22050, 8 * 22050, size=args.clips)]
        clips22 = [clip(n, i, 22050) for i, n in enumerate(n22)]
        clips48 = [(clip(n * 320 // 147, i, 48000), 48000) for i, n in enumerate(n22)]
        seconds = sum(n22) / 22050.0
        lines += ['', f'2. preprocessing: {args.clips} synthetic clips of 2 to 8 s, {seconds:.0f} s of audio, already decoded in host memory; DeviceCorpus.from_wavs,',
                  '   wall clock to a device synchronise, median of 5 runs after a warm-up call, the two inputs alternating']
        D.DeviceCorpus.from_wavs(clips22[:8], hp, 'cuda')
        D.DeviceCorpus.from_wavs(clips48[:8], hp, 'cuda', resample=True)
        torch.cuda.synchronize()
        for batch_clips in (16, 64):
            runs = {22050: [], 48000: []}
            for _ in range(5):
                for rate, items, kw in ((22050, clips22, {}), (48000, clips48, dict(resample=True))):
                    t0 = time.perf_counter()
                    corpus = D.DeviceCorpus.from_wavs(items, hp, 'cuda', batch_clips=batch_clips, **kw)
                    torch.cuda.synchronize()
                    runs[rate].append(time.perf_counter() - t0)
            a, b = float(np.median(runs[22050])), float(np.median(runs[48000]))
            lines.append(f'   batch_clips={batch_clips:2d}: clips at 22.05 kHz {a:6.3f} s (min {min(runs[22050]):.3f}, max {max(runs[22050]):.3f}) = {seconds / a:6.0f} x real time;  '
                         f'at 48 kHz with resample=True {b:6.3f} s (min {min(runs[48000]):.3f}, max {max(runs[48000]):.3f}) = {seconds / b:6.0f} x real time;  '
                         f'ratio {b / a:.2f}, {len(corpus)} utterances, {corpus.n_clipped} clipped samples')
        threads = min(16, os.cpu_count() or 1)
        from scipy.signal import resample_poly
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            with ThreadPoolExecutor(threads) as ex:
                outs = list(ex.map(lambda c: resample_poly(c[0], 147, 320).astype(np.float32), clips48))
            runs.append(time.perf_counter() - t0)
        ours = rs.resample(clips48[0][0])[0].cpu().numpy()
        lines += ['', f'3. scipy.signal.resample_poly(x, 147, 320) on the host for the same {args.clips} clips at 48 kHz, {threads} threads: median of 3 runs '
                      f'{float(np.median(runs)):.3f} s (min {min(runs):.3f}) = {seconds / float(np.median(runs)):.0f} x real time',
                  f'   (its default filter is another one: max |resample_poly - kernel| on the first clip {float(np.abs(outs[0][:ours.size] - ours[:outs[0].size]).max()):.2e})']
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
