"""Developer tool (GPU): latency of streaming generation (WaveRNN.stream) against the offline unbatched call.

A 5 s clip (401 frames, BASELINE configs[1]'s shape) held in memory is pushed in chunks of 1, 4, 8 and 32 frames, in both tail
modes.  Per run it reports the time from opening the stream to the first push that returns audio, the stream's total wall time
against one offline unbatched generate_raw + the same host epilogue, and the per-push host + launch overhead:
(stream wall - offline wall) / pushes; the last lines time single pushes that make no step and one frame of steps ready.

    python tools/stream_latency.py [--frames 401] [--chunks 1,4,8,32] [--reps 3]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=401)
    ap.add_argument('--chunks', default='1,4,8,32')
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    import torch
    from tacotronv2_wavernn_chinese_amd.dsp import decode_mu_law
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    sd = make_state_dict(0, variant='peaky')
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    T, hop = args.frames, m.hop_length
    mels = make_mels(1, 1, T)
    mel2 = mels[0]

    def offline():
        t0 = time.perf_counter()
        res = m.generate_raw(mels, False, 11000, 550, seed=7)   # waits (last_timing)
        out = decode_mu_law(res['samples'].cpu().numpy().astype(np.float64), m.n_classes, False)
        return time.perf_counter() - t0, out

    offline()   # warm-up: weights packed, kernels loaded
    off = sorted(offline()[0] for _ in range(args.reps))[args.reps // 2]
    print(f'clip: {T} frames = {T * hop} samples ({T * hop / m.sample_rate:.3f} s), RAW 10-bit, TEAM2, B=1')
    print(f'offline unbatched generate_raw + host decode: {off * 1e3:.2f} ms (median of {args.reps})')
    print()
    print(f'{"chunk":>5} {"tail":>9} {"pushes":>6} {"first audio ms":>14} {"frames in":>9} {"wall ms":>9} {"vs offline":>10} '
          f'{"overhead/push us":>16} {"workspace MB":>12}')
    for chunk in [int(c) for c in args.chunks.split(',')]:
        for tail in ('none', 'reference'):
            runs = []
            for rep in range(args.reps + 1):   # the first run warms the stream's workspace up
                first = None
                t0 = time.perf_counter()
                with m.stream(seed=7, tail=tail) as st:
                    pushes = 0
                    for f in range(0, T, chunk):
                        out = st.push(mel2[:, f:f + chunk])
                        pushes += 1
                        b = time.perf_counter()
                        if first is None and out.size:
                            first = (b - t0, f + min(chunk, T - f))
                    out = st.finish()
                    pushes += 1
                    if first is None:
                        first = (time.perf_counter() - t0, T)
                    wall = time.perf_counter() - t0
                    ws = st.info()['workspace_bytes']
                if rep:
                    runs.append((wall, first, pushes, ws))
            runs.sort(key=lambda r: r[0])
            wall, first, pushes, ws = runs[len(runs) // 2]
            print(f'{chunk:>5} {tail:>9} {pushes:>6} {first[0] * 1e3:>14.2f} {first[1]:>9} {wall * 1e3:>9.2f} {wall / off:>10.3f} '
                  f'{(wall - off) / pushes * 1e6:>16.1f} {ws / 2 ** 20:>12.1f}')
    print()
    # where a push's time goes: the host side of one push (planning, ctypes, allocations, ~12 launches, the wait) for a push that
    # makes no step ready (only the mel history is updated) and for a 1-frame push (275 steps of loop)
    with m.stream(seed=7, tail='none') as st:
        st.push(mel2[:, :40])
        idle = []
        for f in range(40, 80):
            a = time.perf_counter()
            st.push(mel2[:, f:f])
            idle.append(time.perf_counter() - a)
        one = []
        for f in range(40, 80):
            a = time.perf_counter()
            st.push(mel2[:, f:f + 1])
            one.append(time.perf_counter() - a)
    print(f'zero-frame push (no step ready: mel history only): median {np.median(idle) * 1e6:.1f} us')
    print(f'one-frame push (275 steps ready, ~{275 * 3.3:.0f} us of loop at 3.3 us/step): median {np.median(one) * 1e6:.1f} us')


if __name__ == '__main__':
    main()
