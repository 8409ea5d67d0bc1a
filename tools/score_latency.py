"""Developer tool (GPU): the spectral scores by the library call against the same recipe from PyTorch-ROCm ops.

Two workloads at the default configuration (vocoder mel, resolutions (512, 50, 240), (1024, 120, 600), (2048, 240, 1200)), clips already
on the device: one 5 s pair, and a ragged queue of 8 pairs.  The library side is ONE ``wrnn_score`` call (``frontend.SpectralScore.score``)
on the whole queue, summaries read back.  The torch side restates the definitions with ``torch.stft`` / ``torch.matmul`` (one pair at a
time: a clip's edge frames reflect at its own end, so a padded batch would compute something else) and reads its summaries back too.

Timing: wall clock around the call including the read-back of the summaries, since a score is a number on the host ("call"), and HIP
events around the same span ("device").  The two sides alternate in one session, ``--reps`` timed repetitions after one warm-up of each;
median [min .. max].

    python tools/score_latency.py [--reps 20] [--out FILE]     # the record: profiles/spectral_score.txt
    python tools/score_latency.py --calls 5                    # nothing but 5 library calls on the 5 s pair, for a kernel trace
    python tools/score_latency.py --parity                     # the kernel's error as a multiple of g for every quantity (tests/test_gpu_score.py's inputs)
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 22050
QUEUE = (5.0, 3.1, 2.2, 1.3, 4.4, 0.9, 2.7, 3.8)     # seconds
MEL = dict(n_fft=2048, hop=275, win=1100, n_mels=80, fmin=95.0, min_level_db=-100.0)


def torch_recipe(a, b, resolutions, basis, dct, windows, mel_window, floor=1e-7):
    """One pair (1-D device tensors of equal length) -> the four summaries as a device tensor, float32 per frame, float64 sums."""
    import torch
    def mel(y):
        X = torch.stft(y, MEL['n_fft'], MEL['hop'], MEL['win'], mel_window, center=True, pad_mode='reflect', return_complex=True)
        S = 20.0 * torch.log10(torch.clamp(basis @ X.abs(), min=1e-5))
        return torch.clamp((S - MEL['min_level_db']) / -MEL['min_level_db'], 0, 1)
    D = (mel(a) - mel(b)) * -MEL['min_level_db']
    lsd = torch.sqrt((D * D).mean(dim=0))
    c = dct @ (D * (np.log(10.0) / 20.0))
    mcd = (10.0 / np.log(10.0)) * torch.sqrt(2.0 * (c * c).sum(dim=0))
    sc, lm = [], []
    for (n_fft, hop, win), w in zip(resolutions, windows):
        X = torch.stft(torch.stack([a, b]), n_fft, hop, win, w, center=True, pad_mode='reflect', return_complex=True)
        A = torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=floor))
        d = A[1] - A[0]
        sc.append(torch.sqrt((d * d).sum(dim=0).double().sum()) / torch.sqrt((A[0] * A[0]).sum(dim=0).double().sum()))
        lm.append((torch.log(A[0]) - torch.log(A[1])).abs().sum(dim=0).double().sum() / (A.shape[1] * A.shape[2]))
    return torch.stack([lsd.double().mean(), mcd.double().mean(), torch.stack(sc).mean(), torch.stack(lm).mean()])


def parity(say):
    """The figures of tests/test_gpu_score.py: for its nine inputs and every per-frame quantity, g and the kernel's error."""
    from tacotronv2_wavernn_chinese_amd.frontend import SpectralScore
    from tests import score_ref as sr
    from tests.test_gpu_score import LENGTHS, RES
    scorer = SpectralScore(resolutions=RES)
    say(f'parity: resolutions {RES}; g = max_t |restatement32 - restatement64|, err = max_t |kernel - restatement64|; the bound is err <= 8 g')
    worst = {}
    for name in sr.PAIR_NAMES:
        for n in LENGTHS:
            a, b = sr.parity_pair(name, n)
            s64, s32 = sr.score(a, b, RES), sr.score(a, b, RES, dtype=np.float32)
            got = scorer.score(a, b, per_frame=True)[0]
            q64, q32, qk = sr.per_frame_quantities(s64), sr.per_frame_quantities(s32), sr.per_frame_quantities(got)
            cells = []
            for q in q64:
                g = float(np.abs(q32[q].astype(np.float64) - q64[q]).max())
                err = float(np.abs(qk[q].astype(np.float64) - q64[q]).max())
                cells.append(f'{q} {err / g:.2f}')
                if err / g > worst.get(q, (0,))[0]:
                    worst[q] = (err / g, name, n, g / float(np.abs(q64[q]).max()))
            say(f'  {name:>6} n = {n:>5}: err / g: ' + ', '.join(cells))
    say('  worst per quantity (err / g, input, g / max |q|): ' + '; '.join(f'{q} {w[0]:.2f} ({w[1]}/{w[2]}, {w[3]:.1e})' for q, w in worst.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=0, help='only this many library calls on the 5 s pair (for rocprofv3 --kernel-trace)')
    ap.add_argument('--parity', action='store_true', help='only the parity figures')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    from tacotronv2_wavernn_chinese_amd.frontend import SpectralScore
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
    scorer = SpectralScore(device=dev)
    res = scorer.resolutions
    lens = [int(s * SR) for s in QUEUE]
    targets = [torch.from_numpy((10.0 * mr.speech_like(n, 20 + i)).astype(np.float32)).to(dev) for i, n in enumerate(lens)]
    tests = [torch.from_numpy(sr.mu_law_round_trip(t.cpu().numpy())).to(dev) for t in targets]
    basis = torch.from_numpy(mr.mel_basis(SR, MEL['n_fft'], MEL['n_mels'], MEL['fmin']).astype(np.float32)).to(dev)
    dct = torch.from_numpy(sr.dct_matrix(MEL['n_mels'], 13).astype(np.float32)).to(dev)
    windows = [torch.from_numpy(mr.window(w).astype(np.float32)).to(dev) for _, _, w in res]
    mel_window = torch.from_numpy(mr.window(MEL['win']).astype(np.float32)).to(dev)

    def lib(a, b):
        return np.array([[s[k] for k in ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag')] for s in scorer.score(a, b)])

    def ref(a, b):
        return torch.stack([torch_recipe(x, y, res, basis, dct, windows, mel_window) for x, y in zip(a, b)]).cpu().numpy()

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

    say(f'spectral scores, default configuration {res}: ONE library call against torch.stft / matmul, {torch.cuda.get_device_name(dev)}')
    say(f'call = wall clock including the read-back of the summaries, device = HIP events around the same span; median [min .. max] of {args.reps} '
        'alternating repetitions after a warm-up, ms')
    say()
    for name, a, b in (('one 5 s pair', targets[:1], tests[:1]), (f'ragged queue of 8 ({", ".join(str(s) for s in QUEUE)} s)', targets, tests)):
        x, y = lib(a, b), ref(a, b)                      # warm-up of both; also the agreement of the two recipes
        rel = float(np.abs(x / y - 1.0).max())
        t_lib, t_ref = [], []
        for _ in range(args.reps):
            t_lib.append(timed(lib, a, b)[:2])
            t_ref.append(timed(ref, a, b)[:2])
        say(f'{name}: summaries of the first pair (mel_lsd_db, mcd_db, mr_sc, mr_logmag) = {", ".join(f"{v:.5f}" for v in x[0])}; '
            f'max relative difference library / torch over all pairs = {rel:.2e}')
        say(f'    library  call {fmt([t[1] for t in t_lib])}   device {fmt([t[0] for t in t_lib])}')
        say(f'    torch    call {fmt([t[1] for t in t_ref])}   device {fmt([t[0] for t in t_ref])}')
        say(f'    library / torch per call (medians) = {np.median([t[1] for t in t_lib]) / np.median([t[1] for t in t_ref]):.3f}')
        say()
    parity(say)
    finish()


if __name__ == '__main__':
    main()
