#!/usr/bin/env python
"""Time the device mel front end (csrc/melspec.hip) and the same mel built from PyTorch-ROCm ops, in one session.

    python tools/mel_latency.py [--iters 200] [--warmup 20] [--out profiles/mel_frontend.txt]
    python tools/mel_latency.py --features tacotron [--out FILE]

Two workloads: the 401-frame clip of the benchmark's configs[1] (110 000 samples, 5 s) and a ragged queue of 8 clips (1.5 to 5 s).  Each
is timed with HIP events around one call at a time after a warm-up (clips already on the device: the launch and the kernel, not the
copy), median and min / max over the iterations.  The torch path is torch.stft (center, reflect, periodic Hann) + filterbank matmul +
log10 + clamp on the same tensors; for the ragged queue it runs clip by clip, as it has no ragged form.  Also prints the kernel's
error against the float64 restatement (tests/mel_ref.py) for the parity inputs of tests/test_gpu_mel.py, and the front end's share of a
folded 5 s generate call (~18 ms).

--features tacotron times the same two workloads under that feature profile (the peak launch in front of the mel launch is inside the
timed call; there is no torch path to compare with), prints the kernel's error against tests/taco_mel_ref.py for the inputs of
tests/test_gpu_taco_mel.py, and times DeviceCorpus.from_wavs over 200 synthetic clips with and without the profile."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd  # noqa: E402
from tests import mel_ref as mr  # noqa: E402


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


def torch_mel(y, window, basis, hop):
    D = torch.stft(y, 2048, hop_length=hop, win_length=window.numel(), window=window, center=True, pad_mode='reflect', return_complex=True)
    S = 20.0 * torch.log10(torch.clamp(basis @ D.abs(), min=1e-5))
    return torch.clamp((S + 100.0) / 100.0, 0.0, 1.0)


def tacotron(args, dev):
    import time
    import types
    from tacotronv2_wavernn_chinese_amd.dataset import DeviceCorpus
    from tests import taco_mel_ref as tm
    from tests.test_gpu_taco_mel import NO_RESCALE, _clips
    fe, plain = MelFrontEnd(device=dev, features='tacotron'), MelFrontEnd(device=dev)
    lines = [f"mel front end, features='tacotron', {torch.cuda.get_device_name(0)}, torch {torch.__version__}; HIP events, {args.warmup} warm-up + "
             f'{args.iters} timed calls, microseconds', '',
             'parity against tests/taco_mel_ref.py in float64 (g = max |ref32 - ref64|, the bound of tests/test_gpu_taco_mel.py is 8 g)']
    inputs = [(n, y, tm.TACOTRON, fe) for n, y in _clips().items()]
    inputs.append(('noise_0.3, no rescale', _clips()['noise_0.3'], NO_RESCALE, MelFrontEnd(device=dev, features='tacotron', preemph_rescale=0)))
    for name, y, f, front in inputs:
        r64, g = tm.error_scale(y, **f)
        err = np.abs(front.melspectrogram(y).cpu().numpy()[0].astype(np.float64) - r64).max()
        lines.append(f'  {name:22s} frames {r64.shape[1]:3d}  g {g:.3e}  kernel error {err:.3e} = {err / g:.2f} g')
    one = torch.from_numpy(mr.speech_like(400 * 275, 1)).to(dev)
    queue = [torch.from_numpy(mr.speech_like(n, i)).to(dev) for i, n in enumerate((110000, 33000, 47123, 90000, 60500, 75001, 101010, 52000))]
    lines += ['', 'one call = the lengths\' copy, one allocation, (tacotron: a memset and the peak launch,) the mel launch; clips already on the device']
    for name, clips in (('one clip, 401 frames', one), ('ragged queue of 8 clips', queue)):
        t, v = timed(lambda: fe.melspectrogram(clips), args.iters, args.warmup), timed(lambda: plain.melspectrogram(clips), args.iters, args.warmup)
        lines.append(f'  {name:24s} tacotron median {t[0]:8.1f} (min {t[1]:.1f}, max {t[2]:.1f})   vocoder median {v[0]:8.1f} (min {v[1]:.1f}, '
                     f'max {v[2]:.1f})   tacotron / vocoder {t[0] / v[0]:.2f}x')
    hp = types.SimpleNamespace(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100, bits=10,
                               mu_law=True, voc_mode='RAW', voc_pad=2, voc_seq_len=1375)
    rng = np.random.Generator(np.random.PCG64(7))
    corpus = [mr.speech_like(int(n), 100 + i) for i, n in enumerate(rng.integers(2 * 22050, 8 * 22050, size=200))]
    secs = sum(c.size for c in corpus) / 22050
    lines += ['', f'preprocessing: 200 synthetic clips of 2 to 8 s, {secs:.0f} s of audio, already decoded in host memory; DeviceCorpus.from_wavs, '
              'batch_clips=16,', 'wall clock to a device synchronise, median of 5 runs after a warm-up call, the ways alternating']
    ways = {'vocoder': dict(), 'tacotron': dict(features='tacotron'), 'vocoder, trim + peak': dict(trim_top_db=25, peak_norm=True),
            'tacotron, trim + peak': dict(features='tacotron', trim_top_db=25, peak_norm=True)}
    took = {k: [] for k in ways}
    for rep in range(6):
        for k, kw in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            DeviceCorpus.from_wavs(corpus, hp, dev, batch_clips=16, **kw)
            torch.cuda.synchronize()
            if rep:
                took[k].append(time.perf_counter() - t0)
    for k, v in took.items():
        lines.append(f'  {k:24s} {np.median(v):.3f} s (min {min(v):.3f}, max {max(v):.3f}) = {secs / np.median(v):7.0f} x real time')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--features', choices=('vocoder', 'tacotron'), default='vocoder', help="'tacotron': time that feature profile instead")
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    if args.features == 'tacotron':
        text = '\n'.join(tacotron(args, dev)) + '\n'
        print(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text)
        return
    fe = MelFrontEnd(device=dev)
    lines = [f'mel front end, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; HIP events, {args.warmup} warm-up + {args.iters} timed calls, microseconds',
             '', 'parity against tests/mel_ref.py in float64 (g = max |mel_ref32 - mel_ref64|, the bound of tests/test_gpu_mel.py is 8 g)']
    from tests.test_gpu_mel import _inputs
    for name, y in _inputs().items():
        r64 = mr.melspectrogram(y, **mr.DEFAULT)
        g = np.abs(mr.melspectrogram(y, **mr.DEFAULT, dtype=np.float32) - r64).max()
        err = np.abs(fe.melspectrogram(y).cpu().numpy()[0].astype(np.float64) - r64).max()
        lines.append(f'  {name:12s} frames {r64.shape[1]:3d}  g {g:.3e}  kernel error {err:.3e} = {err / g:.2f} g')
    window = torch.from_numpy(mr.window(1100).astype(np.float32)).to(dev)
    basis = torch.from_numpy(mr.mel_basis(22050, 2048, 80, 95.0).astype(np.float32)).to(dev)
    one = torch.from_numpy(mr.speech_like(400 * 275, 1)).to(dev)
    queue = [torch.from_numpy(mr.speech_like(n, i)).to(dev) for i, n in enumerate((110000, 33000, 47123, 90000, 60500, 75001, 101010, 52000))]
    agree = float((torch_mel(one, window, basis, 275) - fe.melspectrogram(one)[0]).abs().max())
    lines += ['', f'torch.stft path vs kernel on the 401-frame clip: max difference {agree:.3e}', '']
    rows = [('one clip, 401 frames', lambda: fe.melspectrogram(one), lambda: torch_mel(one, window, basis, 275)),
            ('ragged queue of 8 clips', lambda: fe.melspectrogram(queue), lambda: [torch_mel(q, window, basis, 275) for q in queue])]
    for name, ours, theirs in rows:
        o, t = timed(ours, args.iters, args.warmup), timed(theirs, args.iters, args.warmup)
        lines.append(f'  {name:24s} melspec.hip median {o[0]:8.1f} (min {o[1]:.1f}, max {o[2]:.1f})   torch ops median {t[0]:8.1f} (min {t[1]:.1f}, max {t[2]:.1f})   torch / ours {t[0] / o[0]:.2f}x')
        if name.startswith('one'):
            lines.append(f'  {"":24s} share of an 18 ms folded generate of the same 5 s clip: {o[0] / 18000 * 100:.2f} %')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
