"""Developer tool (GPU): Griffin-Lim by the library call against the same recipe from PyTorch-ROCm ops.

Two workloads under the 'tacotron' profile, mels already on the device: one 401-frame clip, and a ragged queue of 8 clips.  The library
side is ONE ``wrnn_griffin_lim`` call (``frontend.GriffinLim.reconstruct``) on the whole queue; the torch side restates steps a to c with
``torch.matmul`` / ``torch.stft`` / ``torch.istft`` (one clip at a time: under zero padding a clip's edge frames depend on its own
length, so a padded batch would compute something else).  Neither side de-emphasises -- torch has no recursive filter -- and the
library's de-emphasis launch is timed on its own below.  Both start from the same injected phases, already on the device, so the two
waves can be compared (zero phases would not do: that start is ill-conditioned, two float32 evaluations of it part by 0.3 %).

Timing: HIP events around the call on the current stream ("device"), and the host time until the call returns ("enqueue": the library
call never waits, so this is the cost of issuing its 2 + 2 (1 + n_iter) launches).  The two sides alternate in one session, ``--reps``
timed repetitions after one warm-up of each; median [min .. max].  Per iteration = (t(n_iter) - t(0)) / n_iter of the medians.

    python tools/griffin_lim_latency.py [--reps 8] [--n_iter 60] [--out FILE]      # the record: section 2 of profiles/griffin_lim.txt
    python tools/griffin_lim_latency.py --calls 3        # nothing but 3 library calls on the 401-frame clip, for a kernel trace
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUEUE = (401, 240, 160, 80, 120, 90, 300, 45)
N_FFT, HOP, WIN = 2048, 275, 1100


def torch_recipe(mel, r, pinv, window, n_iter, f, power=1.5, min_level_db=-100.0):
    """Steps a to c for one (n_mels, T) mel with torch ops, first phases exp(2 pi i r) with r (T, bins), no de-emphasis -> (hop (T - 1),)."""
    import torch
    A = f['max_abs_value']
    if A:
        S_db = (torch.clamp(2 * A * mel - A, -A, A) + A) * (-min_level_db / (2 * A)) + min_level_db
    else:
        S_db = torch.clamp(mel, 0, 1) * -min_level_db + min_level_db
    a = torch.pow(10.0, (S_db + f['ref_level_db']) * 0.05)
    if f['magnitude_power'] == 2:
        a = torch.sqrt(a)
    S = torch.clamp(pinv @ a, min=1e-10) ** power
    Z = torch.polar(S, (2 * np.pi) * r.T)
    mode = 'constant' if f['pad_mode'] == 'zero' else 'reflect'
    y = torch.istft(Z, N_FFT, HOP, WIN, window, center=True)
    for _ in range(n_iter):
        X = torch.stft(y, N_FFT, HOP, WIN, window, center=True, pad_mode=mode, return_complex=True)
        mag = X.abs()
        u = torch.where(mag > 0, X / torch.where(mag > 0, mag, torch.ones_like(mag)), torch.ones_like(X))
        y = torch.istft(S * u, N_FFT, HOP, WIN, window, center=True)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=8)
    ap.add_argument('--n_iter', type=int, default=60)
    ap.add_argument('--calls', type=int, default=0, help='only this many library calls on the 401-frame clip (for rocprofv3 --kernel-trace)')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    from tacotronv2_wavernn_chinese_amd.frontend import FEATURE_PROFILES, GriffinLim, MelFrontEnd, deemphasis
    from tests import griffin_lim_ref as gr
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    f = FEATURE_PROFILES['tacotron']
    gl = GriffinLim(features='tacotron', device=dev)
    fe = MelFrontEnd(features='tacotron', device=dev)
    wavs = [gr.harmonic_chirp(HOP * (t - 1) + 3, 10 + i) for i, t in enumerate(QUEUE)]
    mels = fe.melspectrogram(wavs)                                   # (8, 80, 401) on the device, zero past each clip
    assert fe.last_frames == list(QUEUE)
    one = mels[:1].contiguous()
    phases = torch.rand((len(QUEUE), max(QUEUE), N_FFT // 2 + 1), generator=torch.Generator().manual_seed(0)).to(dev)
    tab = gl.tables()
    pinv, window = torch.from_numpy(tab['pinv']).to(dev), torch.from_numpy(tab['window']).to(dev)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def lib(batch, frames, n_iter):
        return gl.reconstruct(batch, frames, n_iter=n_iter, phases=phases[:batch.shape[0]], deemphasis=False)

    def ref(batch, frames, n_iter):
        return [torch_recipe(batch[b, :, :t], phases[b, :t], pinv, window, n_iter, f) for b, t in enumerate(frames)]

    def timed(fn, *a):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn(*a)
        e1.record()
        host = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), host, out

    if args.calls:
        lib(one, [401], args.n_iter)
        torch.cuda.synchronize()
        for _ in range(args.calls):
            lib(one, [401], args.n_iter)
        torch.cuda.synchronize()
        return

    def fmt(v):
        return f'{np.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]'

    say(f'Griffin-Lim, tacotron profile, injected first phases, no de-emphasis: ONE library call against torch.stft / torch.istft / matmul, {torch.cuda.get_device_name(dev)}')
    say(f'device = HIP events around the call, enqueue = host time until the call returns; median [min .. max] of {args.reps} alternating repetitions after a warm-up, ms')
    say()
    verdict = []
    for name, batch, frames in (('1 x 401 frames', one, [401]), (f'ragged queue {QUEUE}', mels, list(QUEUE))):
        med = {}
        for n_iter in (0, args.n_iter):
            a, b = lib(batch, frames, n_iter), ref(batch, frames, n_iter)   # warm-up of both; also the parity of the two recipes
            torch.cuda.synchronize()
            diff = max(float((a[i, :HOP * (t - 1)] - b[i]).abs().max()) for i, t in enumerate(frames))
            peak = max(float(x.abs().max()) for x in b)
            t_lib, t_ref = [], []
            for _ in range(args.reps):
                t_lib.append(timed(lib, batch, frames, n_iter)[:2])
                t_ref.append(timed(ref, batch, frames, n_iter)[:2])
            ld, lh = [x[0] for x in t_lib], [x[1] for x in t_lib]
            rd, rh = [x[0] for x in t_ref], [x[1] for x in t_ref]
            med[n_iter] = (float(np.median(ld)), float(np.median(rd)))
            say(f'{name}, n_iter = {n_iter}: max |library - torch| = {diff:.3e} on a peak of {peak:.3e}')
            say(f'    library  device {fmt(ld)}   enqueue {fmt(lh)}')
            say(f'    torch    device {fmt(rd)}   enqueue {fmt(rh)}')
        n = args.n_iter
        per = [(med[n][i] - med[0][i]) / n for i in (0, 1)] if n else [float('nan')] * 2
        say(f'    per iteration: library {per[0] * 1e3:.1f} us, torch {per[1] * 1e3:.1f} us; per call: library / torch = {med[n][0] / med[n][1]:.3f}')
        verdict.append(med[n][0] <= med[n][1] and (not n or per[0] <= per[1]))
        say()
    # the de-emphasis launch alone, on the longest wave
    w = lib(one, [401], 0)
    t = [timed(deemphasis, w, [w.shape[1]], 0.97)[0] for _ in range(args.reps + 1)][1:]
    say(f'wrnn_deemphasis alone, {w.shape[1]} samples, k = 0.97: device {fmt(t)}')
    say()
    say('the library call is not slower than the torch path, per call and per iteration: ' + ('yes' if all(verdict) else 'NO'))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
