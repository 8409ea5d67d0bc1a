"""Developer tool (GPU): the aligned scores by the library call against the same recipe from PyTorch-ROCm ops.

Two workloads at the default configuration (80 mels, hop 275, 13 cepstra), clips already on the device: one 5 s pair (401 x 401
frames, the test clip a mu-law round trip of the target delayed by 3 frames), and a ragged queue of 8 pairs.  The library side is ONE
``wrnn_align_score`` call (``frontend.AlignedScore.score``) on the whole queue, summaries read back; with ``pitch=True`` the two
``wrnn_pitch_track`` calls in front of it are inside the span.  The torch side takes the same mels (``MelFrontEnd``), makes the cepstra
and the cost matrix with ``matmul`` in float64, runs the DP as a loop over the anti-diagonals on the device and backtracks on the host.

Timing: wall clock around the call including the read-back ("call"), and HIP events around the same span ("device").  The two sides
alternate in one session, ``--reps`` timed repetitions after two warm-ups of each; median [min .. max].

The split of the library call, each part timed on its own with HIP events in the same session: the two mels (``MelFrontEnd``), mels +
cepstra + cost (``AlignedScore.cost``), DP + backtrack (``dtw_path`` on that cost matrix).  The backtrack runs inside the DP kernel; its
share is measured as a slope: the same 401 x 401 shape with a path of 401 pairs (zeros on the diagonal) and of 800 pairs (zeros along
the first row and the last column) differs by 399 backtrack steps and nothing else.

    python tools/align_latency.py [--reps 20] [--out FILE]     # the record: profiles/align.txt
    python tools/align_latency.py --calls 5                    # nothing but 5 library calls on the 5 s pair, for a kernel trace
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, HOP, K = 22050, 275, 13
QUEUE = (5.0, 3.1, 2.2, 1.3, 4.4, 0.9, 2.7, 3.8)     # seconds, the targets; every test clip is 3 frames longer


def torch_recipe(fe, dct, a, b):
    """One pair -> (total_cost, path_len, mcd_dtw_db, mel_lsd_dtw_db) as floats; float64 torch ops on the device, the backtrack on the host."""
    import torch
    Ma, Mb = fe.melspectrogram(a)[0].double(), fe.melspectrogram(b)[0].double()
    scale = 100.0 * np.log(10.0) / 20.0
    ca, cb = (dct @ Ma) * scale, (dct @ Mb) * scale                                     # (K, T)
    sq = (ca * ca).sum(0)[:, None] + (cb * cb).sum(0)[None, :] - 2.0 * (ca.T @ cb)
    d = (10.0 / np.log(10.0)) * torch.sqrt(2.0 * sq.clamp(min=0.0))
    Ta, Tb = d.shape
    D = torch.full((Ta + 1, Tb + 1), float('inf'), dtype=torch.float64, device=d.device)   # a border of inf stands for "outside"
    D[0, 0] = 0.0
    choice = torch.zeros((Ta, Tb), dtype=torch.uint8, device=d.device)
    for s in range(Ta + Tb - 1):
        i = torch.arange(max(0, s - Tb + 1), min(s, Ta - 1) + 1, device=d.device)
        j = s - i
        cand = torch.stack([D[i, j], D[i, j + 1], D[i + 1, j]])                         # diagonal, (i - 1, j), (i, j - 1) in the bordered matrix
        best, pick = cand.min(dim=0)                                                     # the first minimum: the tie order
        D[i + 1, j + 1] = d[i, j] + best
        choice[i, j] = pick.to(torch.uint8)
    ch = choice.cpu().numpy()
    i, j, path = Ta - 1, Tb - 1, []
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        c = ch[i, j]
        i, j = (i - 1, j - 1) if c == 0 else (i - 1, j) if c == 1 else (i, j - 1)
    p = torch.tensor(path[::-1], device=d.device)
    lsd = torch.sqrt((((Ma[:, p[:, 0]] - Mb[:, p[:, 1]]) * 100.0) ** 2).mean(dim=0)).mean()
    total = float(D[Ta, Tb])
    return total, len(path), total / len(path), float(lsd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=0, help='only this many library calls on the 5 s pair (for rocprofv3 --kernel-trace)')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    from tacotronv2_wavernn_chinese_amd.frontend import AlignedScore, MelFrontEnd, dtw_path
    from tests import mel_ref as mr
    from tests import score_ref as sr
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    plain, pitched, fe = AlignedScore(device=dev), AlignedScore(device=dev, pitch=True), MelFrontEnd(device=dev)
    dct = torch.from_numpy(sr.dct_matrix(80, K)).to(dev)
    lens = [HOP * (int(s * SR) // HOP) for s in QUEUE]                 # 5 s: 400 hops, 401 frames
    host_t = [(10.0 * mr.speech_like(n, 20 + i)).astype(np.float32) for i, n in enumerate(lens)]
    host_s = [np.concatenate([np.zeros(3 * HOP, np.float32), sr.mu_law_round_trip(t)])[:t.size if i == 0 else None] for i, t in enumerate(host_t)]
    targets, tests = [torch.from_numpy(t).to(dev) for t in host_t], [torch.from_numpy(t).to(dev) for t in host_s]
    fields = ('total_cost', 'path_len', 'mcd_dtw_db', 'mel_lsd_dtw_db')

    def lib(scorer, a, b):
        r = scorer.score(a, b)
        return np.stack([r[k].numpy() for k in fields], axis=1)

    def ref(a, b):
        return np.array([torch_recipe(fe, dct, x, y) for x, y in zip(a, b)])

    if args.calls:
        for _ in range(args.calls + 1):
            lib(plain, targets[:1], tests[:1])
        torch.cuda.synchronize()
        return

    def timed(fn, *a):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn(*a)
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return e0.elapsed_time(e1), wall, out

    def fmt(v):
        return f'{np.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]'

    def series(fn, *a):
        for _ in range(2):
            fn(*a)
        return [timed(fn, *a)[0] for _ in range(args.reps)]

    say(f'aligned scores, default configuration (80 mels, hop {HOP}, {K} cepstra): ONE wrnn_align_score call against matmul + an anti-diagonal loop in '
        f'float64 torch ops, {torch.cuda.get_device_name(dev)}')
    say(f'call = wall clock including the read-back of the summaries, device = HIP events around the same span; median [min .. max] of {args.reps} '
        'alternating repetitions after two warm-ups, ms')
    say()
    for name, a, b in (('one 5 s pair (401 x 401 frames)', targets[:1], tests[:1]),
                       (f'ragged queue of 8 (targets {", ".join(str(s) for s in QUEUE)} s, every test clip 3 frames longer)', targets, tests)):
        for _ in range(2):
            x, xp, y = lib(plain, a, b), lib(pitched, a, b), ref(a, b)       # warm-up of all three; also the agreement of the two recipes
        diff = float(np.abs(x / y - 1.0).max())
        t_lib, t_pitch, t_ref = [], [], []
        for _ in range(args.reps):
            t_lib.append(timed(lib, plain, a, b)[:2])
            t_pitch.append(timed(lib, pitched, a, b)[:2])
            t_ref.append(timed(ref, a, b)[:2])
        say(f'{name}: first pair ({", ".join(fields)}) = {", ".join(f"{v:.6g}" for v in x[0])}; path lengths library == torch: {bool((x[:, 1] == y[:, 1]).all())}; '
            f'largest relative difference library / torch over all pairs and fields = {diff:.2e}; with pitch the same four fields: {bool((x == xp).all())}')
        say(f'    library               call {fmt([t[1] for t in t_lib])}   device {fmt([t[0] for t in t_lib])}')
        say(f'    library, pitch=True   call {fmt([t[1] for t in t_pitch])}   device {fmt([t[0] for t in t_pitch])}')
        say(f'    torch                 call {fmt([t[1] for t in t_ref])}   device {fmt([t[0] for t in t_ref])}')
        say(f'    library / torch per call (medians) = {np.median([t[1] for t in t_lib]) / np.median([t[1] for t in t_ref]):.5f}')
        say()
    # the split on the 5 s pair: HIP events around each part alone (device tensors in, nothing read back inside the span)
    a, b = targets[:1], tests[:1]
    cost = plain.cost(a, b)[0].contiguous()
    Ta, Tb = cost.shape
    t_mel = series(lambda: (fe.melspectrogram(a), fe.melspectrogram(b)))
    t_cost = series(lambda: plain.cost(a, b))
    t_dp = series(lambda: dtw_path(cost))
    P = len(dtw_path(cost)[0][0])
    big = torch.full((Ta, Tb), 50.0, device=dev)
    diag_m, edge_m = big.clone(), big.clone()
    diag_m.fill_diagonal_(0.0)
    edge_m[0, :] = 0.0
    edge_m[:, -1] = 0.0
    P_short, P_long = len(dtw_path(diag_m)[0][0]), len(dtw_path(edge_m)[0][0])
    t_short, t_long = series(lambda: dtw_path(diag_m)), series(lambda: dtw_path(edge_m))
    step = (np.median(t_long) - np.median(t_short)) / (P_long - P_short)
    say(f'split of the 5 s pair ({Ta} x {Tb} frames, path of {P} pairs), each part alone, device ms (the spans include torch\'s own small launches: the '
        'length upload and the output allocation):')
    say(f'    the two mels (MelFrontEnd, 2 launches)                  {fmt(t_mel)}')
    say(f'    mels + cepstra + cost (AlignedScore.cost, 4 launches)   {fmt(t_cost)}     -> cepstra + cost = {np.median(t_cost) - np.median(t_mel):.3f} by difference')
    say(f'    DP + backtrack + path (dtw_path, 1 launch, 1 workgroup) {fmt(t_dp)}')
    say(f'    the same shape, path of {P_short} pairs (zero diagonal)                {fmt(t_short)}')
    say(f'    the same shape, path of {P_long} pairs (zero first row, last column)  {fmt(t_long)}')
    say(f'    -> one backtrack step = {1e3 * step:.3f} us (slope); the backtrack of the {P} pairs above = {step * P:.3f} ms of the {np.median(t_dp):.3f}, '
        f'the {Ta + Tb - 1} diagonals of the DP = {1e3 * (np.median(t_dp) - step * P) / (Ta + Tb - 1):.3f} us each')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
