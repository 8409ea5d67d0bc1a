"""Developer tool (GPU): the pitch scores by the library call against the same recipe from PyTorch-ROCm ops.

Two workloads at the default configuration (frame 2048, window 1024, lags 37 .. 367 at 22050 Hz, hop 275), clips already on the device:
one 5 s pair, and a ragged queue of 8 pairs.  The library side is ONE ``wrnn_pitch_score`` call (``frontend.PitchScore.score``) on the
whole queue, summaries read back.  The torch side restates the definitions in float64 with ``unfold``, broadcast differences and
``cumsum`` (one clip at a time, 64 frames at a time: the (frames, lags, window) block of differences is 1.2 GB for a 5 s clip
otherwise) and reads its summaries back too.

Timing: wall clock around the call including the read-back of the summaries ("call"), and HIP events around the same span ("device").
The two sides alternate in one session, ``--reps`` timed repetitions after two warm-ups of each; median [min .. max].

    python tools/pitch_latency.py [--reps 20] [--out FILE]     # the record: profiles/pitch.txt
    python tools/pitch_latency.py --calls 5                    # nothing but 5 library calls on the 5 s pair, for a kernel trace
    python tools/pitch_latency.py --parity                     # the kernel's error on the fixtures of tests/test_gpu_pitch.py
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, HOP, FL, W = 22050, 275, 2048, 1024
QUEUE = (5.0, 3.1, 2.2, 1.3, 4.4, 0.9, 2.7, 3.8)     # seconds
THRESHOLD, SILENCE, GPE = 0.15, 1e-4, 0.2


def torch_track(y, tau_min, tau_max, chunk=64):
    """One clip (1-D float32 device tensor) -> its f0 track (float32), the definitions in float64 torch ops."""
    import torch
    n = y.numel()
    T = 1 + n // HOP
    x = torch.cat([torch.zeros(FL // 2, dtype=torch.float64, device=y.device), y.double(), torch.zeros(T * HOP + FL, dtype=torch.float64, device=y.device)])
    frames = x.unfold(0, FL, HOP)[:T]                                 # (T, FL)
    tau = torch.arange(1, tau_max + 2, dtype=torch.float64, device=y.device)
    out = []
    for f in frames.split(chunk):
        lagged = f.unfold(1, W, 1)[:, :tau_max + 2]                   # (t, tau_max + 2, W)
        d = ((f[:, None, :W] - lagged) ** 2).sum(dim=2)
        cs = torch.cumsum(d[:, 1:], dim=1)
        dp = torch.cat([torch.ones_like(d[:, :1]), torch.where(cs > 0, d[:, 1:] * tau / cs, torch.ones_like(cs))], dim=1)
        below = dp[:, tau_min:tau_max + 1] < THRESHOLD
        has = below.any(dim=1)
        first = tau_min + below.int().argmax(dim=1)
        idx = torch.arange(dp.shape[1] - 1, device=y.device)[None, :]
        stops = ((dp[:, 1:] >= dp[:, :-1]) | (idx >= tau_max)) & (idx >= first[:, None])     # tau stays where its successor is no smaller
        best = stops.int().argmax(dim=1)
        a, b, c = (dp.gather(1, (best + k)[:, None])[:, 0] for k in (-1, 0, 1))
        den = a - 2 * b + c
        off = torch.where(den > 0, 0.5 * (a - c) / den, torch.zeros_like(den)).clamp(-0.5, 0.5)
        rms = torch.sqrt((f[:, :W] ** 2).sum(dim=1) / W)
        f0 = torch.where(has & (rms >= SILENCE), SR / (best + off), torch.zeros_like(off))
        out.append(f0.float())
    return torch.cat(out)


def torch_recipe(a, b, tau_min, tau_max):
    """One pair -> the eight summaries as a float64 device tensor."""
    import torch
    ft, fs = torch_track(a, tau_min, tau_max).double(), torch_track(b, tau_min, tau_max).double()
    T = ft.numel()
    vt, vs = ft > 0, fs > 0
    V = vt & vs
    nV = V.sum()
    ratio = torch.where(V, fs / torch.where(V, ft, torch.ones_like(ft)), torch.ones_like(ft))
    cents = 1200.0 * torch.log2(ratio)
    n_gpe = (V & ((ratio - 1.0).abs() > GPE)).sum()
    n_vde = (vt != vs).sum()
    nz = nV.clamp(min=1)
    lt, ls = torch.log2(torch.where(V, ft, torch.ones_like(ft))), torch.log2(torch.where(V, fs, torch.ones_like(fs)))
    da, dc = torch.where(V, lt - lt.sum() / nz, torch.zeros_like(lt)), torch.where(V, ls - ls.sum() / nz, torch.zeros_like(ls))
    var = (da * da).sum() * (dc * dc).sum()
    corr = torch.where((nV >= 2) & (var > 0), (da * dc).sum() / torch.sqrt(var.clamp(min=1e-300)), torch.zeros_like(var))
    return torch.stack([torch.sqrt((cents ** 2).sum() / nz), n_gpe / nz, n_vde / T, (n_gpe + n_vde) / T, corr, vt.sum().double(), vs.sum().double(), nV.double()])


def parity(say):
    """The figures of tests/test_gpu_pitch.py: per configuration, the worst f0 and aperiodicity error over every frame of its fixtures."""
    from tests import pitch_ref as pr
    from tests.test_gpu_pitch import _native, _settings, check_track, device_track
    say('parity: every fixture of tests/pitch_ref.py as one ragged batch per configuration; voiced flags and integer lags equal on every frame; '
        'f0 error in float32 spacings of the float64 restatement (bound 1), aperiodicity error in 2^-23 max(1, ref) (bound 1)')
    for config in pr.CONFIGS:
        cases = [c for c in pr.CASES if c[0] == config]
        s = _settings(config)
        nat = _native(config)
        f0, ap = device_track(nat, [pr.signal(name, n, s['sample_rate']) for _, name, n in cases])
        errs = [check_track(f'{config}/{name}/{n}', pr.case_track(config, name, n), f0[i], ap[i]) for i, (_, name, n) in enumerate(cases)]
        frames = sum(len(pr.case_track(*c)['f0']) for c in cases)
        say(f'  {config:>10}: frame {s["frame_length"]}, window {s["window"]}, hop {s["hop"]}, lags {nat.tau_min} .. {nat.tau_max}, {len(cases)} clips, '
            f'{frames} frames: f0 {max(e[0] for e in errs):.3f}, aperiodicity {max(e[1] for e in errs):.3f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=0, help='only this many library calls on the 5 s pair (for rocprofv3 --kernel-trace)')
    ap.add_argument('--parity', action='store_true', help='only the parity figures')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    from tacotronv2_wavernn_chinese_amd.frontend import PitchScore
    from tests import mel_ref as mr
    from tests import score_ref as sr
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')

    if args.parity:
        parity(say)
        return finish()
    scorer = PitchScore(device=dev)
    lens = [int(s * SR) for s in QUEUE]
    targets = [torch.from_numpy((10.0 * mr.speech_like(n, 20 + i)).astype(np.float32)).to(dev) for i, n in enumerate(lens)]
    tests = [torch.from_numpy(sr.mu_law_round_trip(t.cpu().numpy())).to(dev) for t in targets]
    fields = ('f0_rmse_cents', 'gpe', 'vde', 'ffe', 'f0_corr', 'voiced_target', 'voiced_test', 'voiced_both')

    def lib(a, b):
        return np.array([[s[k] for k in fields] for s in scorer.score(a, b)])

    def ref(a, b):
        return torch.stack([torch_recipe(x, y, scorer.tau_min, scorer.tau_max) for x, y in zip(a, b)]).cpu().numpy()

    if args.calls:
        lib(targets[:1], tests[:1])
        for _ in range(args.calls):
            lib(targets[:1], tests[:1])
        torch.cuda.synchronize()
        return

    def timed(fn, *a):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn(*a)
        e1.record()
        wall = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), wall, out

    def fmt(v):
        return f'{np.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]'

    say(f'pitch scores, default configuration (frame {FL}, window {W}, hop {HOP}, lags {scorer.tau_min} .. {scorer.tau_max}): ONE library call against '
        f'unfold / broadcast differences / cumsum in float64, {torch.cuda.get_device_name(dev)}')
    say(f'call = wall clock including the read-back of the summaries, device = HIP events around the same span; median [min .. max] of {args.reps} '
        'alternating repetitions after two warm-ups, ms')
    say()
    for name, a, b in (('one 5 s pair', targets[:1], tests[:1]), (f'ragged queue of 8 ({", ".join(str(s) for s in QUEUE)} s)', targets, tests)):
        for _ in range(2):
            x, y = lib(a, b), ref(a, b)                  # warm-up of both; also the agreement of the two recipes
        diff = float(np.abs(x - y).max() / max(1.0, np.abs(y).max()))
        counts = bool((x[:, 5:] == y[:, 5:]).all())
        t_lib, t_ref = [], []
        for _ in range(args.reps):
            t_lib.append(timed(lib, a, b)[:2])
            t_ref.append(timed(ref, a, b)[:2])
        say(f'{name}: summaries of the first pair ({", ".join(fields)}) = {", ".join(f"{v:.6g}" for v in x[0])}; voiced counts library == torch: {counts}; '
            f'max difference library - torch over all pairs and fields, relative to the largest field = {diff:.2e}')
        say(f'    library  call {fmt([t[1] for t in t_lib])}   device {fmt([t[0] for t in t_lib])}')
        say(f'    torch    call {fmt([t[1] for t in t_ref])}   device {fmt([t[0] for t in t_ref])}')
        say(f'    library / torch per call (medians) = {np.median([t[1] for t in t_lib]) / np.median([t[1] for t in t_ref]):.4f}')
        say()
    parity(say)
    finish()


if __name__ == '__main__':
    main()
