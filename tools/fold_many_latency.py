"""Developer tool (GPU): several queued clips in fold mode -- one `generate_many(batched=True)` call against one
`generate(batched=True)` call per clip.

Five queues of RAW 10-bit clips (mel frames): 4 x 401, (401, 240, 160, 80), 8 x 80, (120, 90, 60, 45, 30, 200, 150, 100), 2 x 401.
Both sides use target='auto', overlap 550 and the device epilogue, so both return the finished float64 audio on the host.  The two are
interleaved (sequential, joint, sequential, ...), `--reps` timed repetitions after one warm-up of each; per queue the tool prints the median
and the range of the wall time of both, the sum of the loop times the library measured (`last_timing`), and what the cost model
(`vocoder.predicted_loop_us` on `STEP_US`, fitted to single-utterance runs) predicted for the loops alone.

    python tools/fold_many_latency.py [--reps 7] [--out profiles/fold_many_latency.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [('4 x 401', [401] * 4), ('401, 240, 160, 80', [401, 240, 160, 80]), ('8 x 80', [80] * 8),
             ('120, 90, 60, 45, 30, 200, 150, 100', [120, 90, 60, 45, 30, 200, 150, 100]), ('2 x 401', [401] * 2)]
OVERLAP = 550


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps must be at least 5')
    import torch
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN, fold_plan, fold_plan_many
    sd = make_state_dict(0, variant='peaky')
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    hop = m.hop_length
    teams = m.native().team_info()[1]
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say(f'fold mode, several queued clips: sequential generate(batched=True) calls vs ONE generate_many(batched=True) call')
    say(f'RAW 10-bit, target=\'auto\', overlap {OVERLAP}, epilogue=\'device\', {teams} XCD teams; wall = host time until the float64 audio of every clip is on the host;')
    say(f'loop = sum of the loop times of the calls (HIP events); median [min .. max] of {args.reps} interleaved repetitions after one warm-up, ms')
    say()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, 'x.wav')
        for name, frames in WORKLOADS:
            clips = [make_mels(100 + i, 1, t) for i, t in enumerate(frames)]
            lens = [t * hop for t in frames]
            plans = [fold_plan(n, OVERLAP, teams, 'RAW') for n in lens]
            joint = fold_plan_many(lens, OVERLAP, teams, 'RAW')

            def sequential():
                loop = 0.0
                t0 = time.perf_counter()
                for c in clips:
                    m.generate(c, path, True, 'auto', OVERLAP, True, epilogue='device', seed=7)
                    loop += m.last_timing['loop_ms']
                return (time.perf_counter() - t0) * 1e3, loop

            def one_call():
                t0 = time.perf_counter()
                m.generate_many([c[0] for c in clips], None, True, 'device', batched=True, target='auto', overlap=OVERLAP, seed=7)
                return (time.perf_counter() - t0) * 1e3, m.last_timing['loop_ms']

            sequential(), one_call()   # warm-up: scratch grown, epilogue tables built
            seq, one = [], []
            for _ in range(args.reps):
                seq.append(sequential())
                one.append(one_call())
            rows, steps, kern = m.last_timing['rows'], m.last_timing['steps'], m.last_timing['kernel']

            def stat(v):
                return f'{np.median(v):7.2f} [{min(v):7.2f} .. {max(v):7.2f}]'
            say(f'queue {name} frames ({sum(lens) / m.sample_rate:.2f} s of audio)')
            say(f'  sequential: {len(frames)} calls, folds {[p[1] for p in plans]}')
            say(f'    wall {stat([s[0] for s in seq])}   loop {stat([s[1] for s in seq])}   model (loops) {sum(p[2] for p in plans) / 1e3:6.1f}')
            say(f'  one call:   {rows} rows x {steps} steps (target {joint[0]}), kernel id {kern}')
            say(f'    wall {stat([s[0] for s in one])}   loop {stat([s[1] for s in one])}   model (loop)  {joint[2] / 1e3:6.1f}')
            say(f'  one call / sequential: wall {np.median([s[0] for s in one]) / np.median([s[0] for s in seq]):.3f}, '
                f'loop {np.median([s[1] for s in one]) / np.median([s[1] for s in seq]):.3f}, model {joint[2] / sum(p[2] for p in plans):.3f}')
            say()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
